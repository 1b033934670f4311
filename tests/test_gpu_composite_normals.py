"""``lse_eval_composite_normals`` (csrc/volrend.hip) against the float64 twin of tests/normals_ref.py: ray lengths around the
64-sample walk in one packed batch with capacity-extent arrays, field and world space under both position maps, an offset output,
and the edge cases (zero gradients, zero weights, a NaN sigma).  Bar: 5 x TOL_FWD, that of the compositing tests."""
import functools

import numpy as np
import pytest
import torch

from tests import normals_ref as nr
from tests.util import TOL_FWD, nmax_err

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 130, 1024, 0, 7)      # the trailing (0, 7): a ray behind an empty one
PAD = 333                                          # capacity beyond the samples: packed_info is authoritative
AABB = [-1.0, -0.8, -1.2, 1.1, 0.9, 1.0]
SENTINEL = -7.5


@functools.lru_cache(maxsize=None)
def _batch():
    """Seeded rays (float32, CPU): step sizes and densities of a marched ray, gradients over six decades, origins and directions
    that put samples inside the unit ball, outside it (contraction) and outside the box (aabb)."""
    g = torch.Generator().manual_seed(77)
    R, n = len(LENGTHS), sum(LENGTHS)
    packed = torch.tensor([[sum(LENGTHS[:i]), c] for i, c in enumerate(LENGTHS)], dtype=torch.int64)
    ts = torch.cat([0.3 + torch.arange(c) * 0.004 for c in LENGTHS]).float()
    te = ts + 0.004
    sigma = torch.rand(n, generator=g) * 8.0
    d_x01 = torch.randn(n, 3, generator=g) * torch.pow(10.0, torch.rand(n, 1, generator=g) * 6 - 3)
    rays_o = (torch.rand(R, 3, generator=g) - 0.5) * 1.2
    rays_d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1)
    pad = lambda t, v: torch.cat([t, torch.full((PAD, *t.shape[1:]), v)])
    return dict(packed=packed, ts=pad(ts, 9.0), te=pad(te, 9.5), sigma=pad(sigma, 3.0), d_x01=pad(d_x01, 1.0), rays_o=rays_o,
                rays_d=rays_d, n=n, R=R)


def _run(b, world=False, contraction=True, renormalize=True, out=None, **replace):
    from lsenerf_amd import ops
    t = {k: (replace.get(k, v).cuda() if torch.is_tensor(v) else v) for k, v in b.items()}
    if out is None:
        out = torch.full((b["R"], 3), SENTINEL, device="cuda")
    ops.eval_composite_normals(t["ts"], t["te"], t["sigma"], t["d_x01"], t["packed"], out, world=world, renormalize=renormalize,
                               rays_o=t["rays_o"] if world else None, rays_d=t["rays_d"] if world else None, contraction=contraction,
                               aabb6=None if contraction else AABB)
    return out


def _twin(b, world=False, contraction=True, renormalize=True, **replace):
    t = {**b, **replace}
    return nr.composite_normals(t["ts"], t["te"], t["sigma"], t["d_x01"], t["packed"], world=world, rays_o=t["rays_o"],
                                rays_d=t["rays_d"], contraction=contraction, aabb6=None if contraction else AABB, renormalize=renormalize)


@pytest.mark.parametrize("space", ["field", "world_contraction", "world_aabb"])
@pytest.mark.parametrize("renormalize", [True, False])
def test_against_the_twin(space, renormalize):
    b = _batch()
    kw = dict(world=space != "field", contraction=space != "world_aabb", renormalize=renormalize)
    got = _run(b, **kw).cpu()
    ref = torch.from_numpy(_twin(b, **kw))
    err = nmax_err(got, ref)
    print("COMPOSITE_NORMALS", space, "renormalize" if renormalize else "raw", "error", err, "max |N|", float(ref.abs().max()))
    assert err < 5 * TOL_FWD, (space, renormalize, err)
    empty = [i for i, c in enumerate(LENGTHS) if c == 0]
    assert bool((got[empty] == 0.0).all())                               # a ray without samples: (0, 0, 0), written
    if renormalize:
        lens = got.norm(dim=-1)
        full = [i for i, c in enumerate(LENGTHS) if c > 0]
        assert float((lens[full] - 1.0).abs().max()) < 1e-5              # unit vectors
    if space == "world_aabb":                                            # the case is not vacuous: samples on both sides of the box
        s6 = int(b["packed"][6, 0])
        pos = b["rays_o"][6] + b["rays_d"][6] * ((b["ts"] + b["te"]) / 2)[s6:s6 + 1024, None]
        _, sel = nr.unit_cube64(pos.double(), False, AABB)
        assert 0 < int(sel.sum()) < sel.numel()


def test_offset_output_leaves_other_rows_alone():
    b = _batch()
    image = torch.full((b["R"] + 11, 3), SENTINEL, device="cuda")
    _run(b, out=image[4:4 + b["R"]])
    assert bool((image[:4] == SENTINEL).all()) and bool((image[4 + b["R"]:] == SENTINEL).all())
    assert torch.equal(image[4:4 + b["R"]], _run(b))


def test_zero_gradients_zero_weights_and_nan_sigma():
    b = _batch()
    s5, s3 = int(b["packed"][5, 0]), int(b["packed"][3, 0])
    g = b["d_x01"].clone()
    g[s5 + 10:s5 + 50] = 0.0                      # a run of zero gradients inside ray 5 (130 samples)
    g[s3:s3 + 64] = 0.0                           # ray 3: every gradient zero
    sigma = b["sigma"].clone()
    s4 = int(b["packed"][4, 0])
    sigma[s4:s4 + 65] = 0.0                       # ray 4: every weight zero
    got = _run(b, d_x01=g, sigma=sigma).cpu()
    ref = torch.from_numpy(_twin(b, d_x01=g, sigma=sigma))
    assert bool(torch.isfinite(got).all())
    assert bool((got[3] == 0.0).all()) and bool((got[4] == 0.0).all())
    assert nmax_err(got, ref) < 5 * TOL_FWD
    # a NaN sigma reaches every later sample of its ray through the transmittance, as in lse_eval_composite; other rays are untouched
    sigma = b["sigma"].clone()
    s6 = int(b["packed"][6, 0])
    sigma[s6 + 70] = float("nan")
    bad = _run(b, sigma=sigma).cpu()
    assert bool(torch.isnan(bad[6]).all())
    keep = [i for i in range(b["R"]) if i != 6]
    assert torch.equal(bad[keep], _run(b).cpu()[keep])


def test_weights_are_the_colour_kernels_bit_for_bit():
    """d_x01 = (-1, 0, 0) in field space without renormalisation makes every sample's normal (1, 0, 0) exactly, so the x sum is
    fmaf(w, 1, nx) = nx + w rounded once -- the accumulation of ``eval_composite`` over the same samples, reduced over the wave in
    the same order: equal bit patterns pin the weights of the two kernels (group_weights) to each other."""
    from lsenerf_amd import ops
    lengths = (0, 1, 63, 64, 65, 128, 129)
    g = torch.Generator().manual_seed(78)
    R, n = len(lengths), sum(lengths)
    packed = torch.tensor([[sum(lengths[:i]), c] for i, c in enumerate(lengths)], dtype=torch.int64).cuda()
    dt = 0.002 + torch.rand(n, generator=g) * 0.004
    ts = torch.cat([0.3 + torch.cumsum(dt[sum(lengths[:i]):sum(lengths[:i + 1])], 0) for i in range(R)]) - dt
    te = ts + dt
    sigma = torch.rand(n, generator=g) * 8.0
    surface = int(packed[6, 0]) + 100                    # a surface sample of a trained scene behind more than one group of ray 6
    sigma[surface] = 2500.0 / float(dt[surface])
    assert 1e3 < float(sigma[surface] * (te[surface] - ts[surface])) < 1e4
    ts, te, sigma = ts.cuda(), te.cuda(), sigma.cuda()
    d_x01 = torch.tensor([-1.0, 0.0, 0.0]).repeat(n, 1).cuda()
    normals = torch.full((R, 3), SENTINEL, device="cuda")
    ops.eval_composite_normals(ts, te, sigma, d_x01, packed, normals, world=False, renormalize=False)
    rgb = torch.rand(n, 3, generator=g).cuda()
    out_rgb, acc, depth = torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
    nsamples = torch.empty(R, dtype=torch.int64, device="cuda")
    ops.eval_composite(ts, te, sigma, rgb, packed, out_rgb, acc, depth, nsamples, nan_to_num=False, background=None, clamp=False)
    print("COMPOSITE_NORMALS weights: acc", acc.tolist(), "N_x", normals[:, 0].tolist())
    assert nsamples.tolist() == list(lengths)
    assert float(acc[1:].min()) > 0.0 and float(acc[6]) > 0.5          # not vacuous: every ray with samples has weight
    assert torch.equal(normals[:, 0].contiguous().view(torch.int32), acc.view(torch.int32))
    assert bool((normals[:, 1:] == 0.0).all())


def test_bad_arguments():
    from lsenerf_amd import ops
    b = _batch()
    t = {k: v.cuda() for k, v in b.items() if torch.is_tensor(v)}
    out = torch.empty(b["R"], 3, device="cuda")
    with pytest.raises(ValueError, match="out_normals"):
        ops.eval_composite_normals(t["ts"], t["te"], t["sigma"], t["d_x01"], t["packed"], out[:-1])
    with pytest.raises(ValueError, match="rays_o"):
        ops.eval_composite_normals(t["ts"], t["te"], t["sigma"], t["d_x01"], t["packed"], out, world=True)
    with pytest.raises(ValueError, match="aabb6"):
        ops.eval_composite_normals(t["ts"], t["te"], t["sigma"], t["d_x01"], t["packed"], out, world=True, rays_o=t["rays_o"],
                                   rays_d=t["rays_d"], contraction=False)
