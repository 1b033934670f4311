"""CPU tier of the compositing tests: the float64 per-ray reference (tests/util.composite_ref) against the oracle and against
nerfacc's semantics at sigma = inf, and the evidence that the tolerances tests/test_gpu_compositing.py asserts are attainable:
a float32 lane-exact emulation of the kernel's walk (exclusive prefix by lane shift) meets them with a factor 4 to spare on
every input the GPU tests use, and the float64 reference keeps the visibility exclusion band under its cap."""
import math

import pytest
import torch

from oracle import volrend as ovr
from tests.util import (AUTO_STEP, SURFACE_SIGMAS, TOL_FWD, TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, composite_ref,
                        emulate_composite_f32, emulate_render_grad_f32, emulated_per_ray_grad_error, nmax_err, ray_bounds, rel_l2, ray_exclusive_sum, select_rays, trained_scene_rays, visibility_ref)

STEPS = ("const", "cone")
ONSETS = ("abrupt", "ramp")
VIS_BAND_CAP = 0.002      # at most 0.2 % of a case's samples may sit within 1e-5 (relative) of a visibility threshold


def test_generator_shape():
    inp = trained_scene_rays(1e5, seed=3, step="cone", onset="ramp", rgb_stride=4)
    ts, te, sg, pk = inp["ts"], inp["te"], inp["sigma"], inp["packed_info"]
    cnt = pk[:, 1]
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 1024, 2000} <= set(cnt.tolist())
    assert torch.equal(pk[:, 0], torch.cumsum(cnt, 0) - cnt) and int(cnt.sum()) == ts.numel() == inp["rgb"].shape[0]
    dt = te - ts
    assert float(dt.min()) > 0.0029 and float(dt.max()) < 0.1001 and float(dt.max()) > 0.05
    same_ray = inp["ray_indices"][1:] == inp["ray_indices"][:-1]
    assert torch.equal(te[:-1][same_ray], ts[1:][same_ray]), "intervals must be contiguous inside a ray"
    assert float((sg == 0).float().mean()) > 0.1 and float(sg.max()) == 1e5
    assert bool(inp["has_surface"].any()) and not bool(inp["has_surface"].all())
    const = trained_scene_rays(30.0, seed=3)
    assert float((const["te"] - const["ts"] - AUTO_STEP).abs().max()) < 1e-6
    again = trained_scene_rays(1e5, seed=3, step="cone", onset="ramp", rgb_stride=4)
    assert all(torch.equal(inp[k], again[k]) for k in inp)


@pytest.mark.parametrize("onset", ONSETS)
@pytest.mark.parametrize("seed", range(1, 8))
def test_generator_places_the_surface_where_kernels_go_wrong(seed, onset):
    """The realised surface positions of every seed the GPU tests use: first in the ray, at offsets 62, 63, 64, 65 of rays that
    go on beyond the 64-lane chunk border, and ending with the last sample of a ray longer than one chunk."""
    sigma = 1e6
    inp = trained_scene_rays(sigma, seed=seed, onset=onset)
    start, cnt = inp["packed_info"][:, 0], inp["packed_info"][:, 1]
    at = inp["surface_at"]
    assert torch.equal(at >= 0, inp["has_surface"]) and bool((at[inp["has_surface"]] < cnt[inp["has_surface"]]).all())
    rays = torch.nonzero(at >= 0).flatten().tolist()
    for r in rays:      # the recorded offset is where the surface begins: the dense value there (ramp: its thousandth first)
        first = float(inp["sigma"][start[r] + at[r]])
        assert first == sigma or (onset == "ramp" and first == pytest.approx(sigma / 1000, rel=1e-6)), (r, first)
    assert {0, 1, 62, 63, 64, 65} <= {int(at[r]) for r in rays if cnt[r] > 66}
    ends = [r for r in rays if cnt[r] > 64 and float(inp["sigma"][start[r] + cnt[r] - 1]) == sigma
            and at[r] >= cnt[r] - 3 and float(inp["sigma"][start[r] + at[r] - 1]) < 0.5]
    assert len(ends) >= 2, "no ray longer than a chunk ends on its surface"
    assert any(cnt[r] % 64 not in (0, 1) for r in ends), "the last sample must also fall inside a partial chunk"


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", [s for s in SURFACE_SIGMAS if s <= 1e10])
def test_ref_equals_oracle_on_finite_input(sigma, step):
    """Same mathematics as oracle/volrend.py wherever that one is defined.  The oracle forms its exclusive sum as cumsum - x minus
    a per-ray offset; evaluated one ray at a time (no foreign offset) its only deviation from the shifted cumsum is the rounding of
    that subtraction, at most an ulp of the ray's inclusive optical depth D in the exponent: 1e-12 holds as it stands for D < 1e3
    (surface sigma <= 1e4) and the bound grows by 4 * 2^-52 * D beyond."""
    inp = trained_scene_rays(sigma, seed=5, step=step, onset="ramp", rgb_stride=3, n_random=20, max_random=100)
    ts, te, sg, pk, ri = (inp[k].double() if inp[k].is_floating_point() else inp[k] for k in ("ts", "te", "sigma", "packed_info", "ray_indices"))
    R = pk.shape[0]
    ref = composite_ref(ts, te, sg, pk, inp["rgb"])
    per_ray = [ovr.render_weight_from_density(ts[s:s + c], te[s:s + c], sg[s:s + c], torch.tensor([[0, c]])) for s, c in pk.tolist() if c]
    w, T, a = (torch.cat([p[i] for p in per_ray]) for i in range(3))
    depth_max = max(float((sg[s:s + c] * (te - ts)[s:s + c]).sum()) for s, c in pk.tolist() if c)
    tol = 1e-12 + 4 * 2.0 ** -52 * depth_max
    if sigma <= 1e4:      # the statement as the reference is specified: equal to the oracle to a flat 1e-12
        assert float((ref["weights"] - w).abs().max()) < 1e-12 and float((ref["trans"] - T).abs().max()) < 1e-12
    assert float((ref["weights"] - w).abs().max()) < tol and float((ref["trans"] - T).abs().max()) < tol
    assert float((ref["alphas"] - a).abs().max()) < 1e-12
    wr = ref["weights"]
    assert float((ref["rgb"] - ovr.accumulate_along_rays(wr, inp["rgb"].double(), ri, R)).abs().max()) < 1e-12
    assert float((ref["acc"] - ovr.render_accumulation(wr[:, None], ri, R)[:, 0]).abs().max()) < 1e-12
    assert float((ref["depth"] - ovr.render_depth_expected(wr[:, None], ts, te, ri, R)[:, 0]).abs().max()) < 1e-12
    for thre in (0.0, 0.01):
        vis, und = visibility_ref(ref, 1e-4, thre)
        ov = torch.cat([ovr.render_visibility_from_density(ts[s:s + c], te[s:s + c], sg[s:s + c], torch.tensor([[0, c]]), 1e-4, thre)
                        for s, c in pk.tolist() if c])
        assert torch.equal(vis[~und], ov[~und])


def test_exclusive_sum_is_per_ray():
    pk = torch.tensor([[0, 3], [3, 0], [3, 2], [5, 1]])
    x = torch.tensor([1.0, math.inf, 2.0, 4.0, 8.0, 16.0], dtype=torch.float64)
    assert ray_exclusive_sum(x, pk).tolist() == [0.0, 1.0, math.inf, 0.0, 4.0, 0.0]
    assert torch.isnan(ovr.exclusive_sum(x, pk)).any(), "the oracle's global cumsum is what this reference replaces"


@pytest.mark.parametrize("step", STEPS)
def test_ref_at_infinite_sigma(step):
    """nerfacc's exclusive-sum semantics: the infinite sample has w = T (alpha = 1), everything behind it 0, rays without one are
    what they are without the infinite rays; gradients stay finite."""
    inp = trained_scene_rays(math.inf, seed=9, step=step, onset="abrupt", n_random=20, max_random=100)
    sg = inp["sigma"].double().requires_grad_(True)
    c = inp["rgb"].double().requires_grad_(True)
    ref = composite_ref(inp["ts"], inp["te"], sg, inp["packed_info"], c)
    w, T = ref["weights"].detach(), ref["trans"].detach()
    assert all(bool(torch.isfinite(ref[k]).all()) for k in ("weights", "trans", "alphas", "rgb", "acc", "num", "depth"))
    isinf = torch.isinf(inp["sigma"])
    assert int(isinf.sum()) > 50
    for s0, cnt in inp["packed_info"].tolist():
        k = torch.nonzero(isinf[s0:s0 + cnt]).flatten()
        if k.numel():
            first = s0 + int(k[0])
            assert float(w[first]) == float(T[first])
            assert float(w[first + 1:s0 + cnt].abs().max() if first + 1 < s0 + cnt else 0.0) == 0.0
    (ref["rgb"].sum() + ref["acc"].sum() + ref["depth"].sum()).backward()
    assert bool(torch.isfinite(sg.grad).all()) and bool(torch.isfinite(c.grad).all())
    keep = ~inp["has_surface"]
    sub = select_rays(inp, keep)
    rs = composite_ref(sub["ts"], sub["te"], sub["sigma"], sub["packed_info"], sub["rgb"])
    assert torch.equal(rs["weights"], w[keep[inp["ray_indices"]]]) and torch.equal(rs["acc"], ref["acc"].detach()[keep])


@pytest.mark.parametrize("onset", ONSETS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", SURFACE_SIGMAS)
def test_f32_emulation_meets_the_tolerances(sigma, step, onset):
    """A correct float32 kernel (shifted scan) is within TOL_FWD / 4 over all samples and 5 TOL_FWD / 4 per ray of the float64
    reference on the inputs of the GPU tests: the bounds asserted there leave a factor 4 for the device's expf and its fused
    multiply-adds, neither of which this emulation models."""
    _assert_emulation_within_a_quarter(trained_scene_rays(sigma, seed=1, step=step, onset=onset), (sigma, step, onset))


def _assert_emulation_within_a_quarter(inp, tag):
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])
    bounds = ray_bounds(inp["packed_info"])
    for name, got in zip(("weights", "trans", "alphas"), emulate_composite_f32(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])):
        assert bool(torch.isfinite(got).all()), (tag, name)
        e, eb = nmax_err(got, ref[name]), blockwise_nmax_err(got, ref[name], bounds)
        assert e < TOL_FWD / 4 and eb < 5 * TOL_FWD / 4, (tag, name, e, eb)


@pytest.mark.parametrize("seed", range(2, 8))
def test_f32_emulation_meets_the_tolerances_on_the_other_seeds(seed):
    """Seeds 2 .. 7 of the GPU tests (backward, eval, special colours, capacity, clip and visibility cases), at a reduced number
    of random rays, over the sigmas, steps and onsets in turn."""
    for k, sigma in enumerate(SURFACE_SIGMAS):
        step, onset = STEPS[(k + seed) % 2], ONSETS[(k // 2 + seed) % 2]
        _assert_emulation_within_a_quarter(trained_scene_rays(sigma, seed=seed, step=step, onset=onset, n_random=12), (seed, sigma, step, onset))


def test_f32_emulation_meets_the_tolerances_on_the_hand_made_cases():
    """The two inputs the GPU tests build themselves: the clip case, and the ray-count cases up to 4097 rays."""
    from tests.test_gpu_compositing import _clip_case, _sized_case
    # clip case: its first ray is nearly transparent on purpose (w ~ 2.4e-7, four ulps of 1 - expf); the GPU test asserts the depth
    inp = _clip_case()
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])
    w = emulate_composite_f32(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])[0]
    mid = (inp["ts"] + inp["te"]) * 0.5
    R = inp["packed_info"].shape[0]
    acc, num = torch.zeros(R).index_add(0, inp["ray_indices"], w), torch.zeros(R).index_add(0, inp["ray_indices"], w * mid)
    depth = torch.clip(num / (acc + 1e-10), mid.min(), mid.max())
    e, eb = nmax_err(depth, ref["depth"]), blockwise_nmax_err(depth, ref["depth"], list(range(R + 1)))
    assert e < TOL_FWD / 4 and eb < 5 * TOL_FWD / 4, (e, eb)
    for n_rays in (1, 5, 1025, 4097):
        for owner in sorted({0, n_rays // 2, n_rays - 1}):
            _assert_emulation_within_a_quarter(_sized_case(n_rays, owner, seed=n_rays + owner)[0], (n_rays, owner))


def test_f32_emulation_of_the_subtracted_prefix_misses_them():
    """What the tests are for: `(incl - sd) + carry` loses the optical depth in front of a dense sample to the rounding of sd."""
    inp = trained_scene_rays(1e6, seed=1, step="cone")
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])
    w = emulate_composite_f32(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"], shifted=False)[0]
    assert nmax_err(w, ref["weights"]) > 10 * TOL_FWD
    inp = trained_scene_rays(math.inf, seed=1)
    w = emulate_composite_f32(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"], shifted=False)[0]
    assert bool(torch.isnan(w).any())


@pytest.mark.parametrize("onset", ONSETS)
@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", SURFACE_SIGMAS)
def test_visibility_band_stays_under_its_cap(sigma, step, onset):
    """The GPU visibility test leaves out samples within 1e-5 (relative) of a threshold; on these inputs that is under 0.2 %
    of the samples, and the float32 emulation decides every other sample as the reference does."""
    inp = trained_scene_rays(sigma, seed=1, step=step, onset=onset)
    ref = composite_ref(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])
    _, T, a = emulate_composite_f32(inp["ts"], inp["te"], inp["sigma"], inp["packed_info"])
    for thre in (0.0, 0.01):
        vis, und = visibility_ref(ref, 1e-4, thre)
        assert float(und.float().mean()) <= VIS_BAND_CAP, (sigma, step, onset, thre, float(und.float().mean()))
        emu = (T >= 1e-4) & ((a >= thre) if thre > 0 else torch.ones_like(vis))
        assert torch.equal(emu[~und], vis[~und])
        assert bool(vis.any()) and (sigma < 1e3 or not bool(vis.all()))


@pytest.mark.parametrize("step", STEPS)
@pytest.mark.parametrize("sigma", [s for s in SURFACE_SIGMAS if s <= 1e10])
def test_f32_emulation_of_the_backward(sigma, step):
    """The backward recurrence of volrend_bwd_kernel in float32 (T_{k+1} = (1 - sum w) + sum_{i>k} w_i, no stored transmittance)
    against float64 autograd, per upstream combination:
    * every combination: TOL_GRAD / 4 over all samples and in L2;
    * a gradient on the colour alone: TOL_GRAD_BLOCK / 4 per ray with the t_end this emulation happens to form;
    * per ray with t_end moved by +-2^-24 (one ulp of the float32 sum of an opaque ray's weights, which the last bits of expf
      decide) the strict bound is NOT attainable in general: dw_k 2^-24 dt stands against a per-ray scale of 1e-4 of the call's
      largest gradient.  The worst ray of each combination is printed; the GPU test bounds d_sigma per ray by 4 x that figure
      (tests/util.emulated_per_ray_grad_error), never by less than TOL_GRAD_BLOCK.  Recorded here: colour alone up to 8.6e-4,
      accumulation alone up to 2.1e-2, depth alone up to 8.3e-3 (far end of long cone-step rays), all three up to 5.8e-3."""
    onset = ONSETS[(SURFACE_SIGMAS.index(sigma) + STEPS.index(step)) % 2]
    inp = trained_scene_rays(sigma, seed=2, step=step, onset=onset)
    R = inp["packed_info"].shape[0]
    g = torch.Generator().manual_seed(4)
    up = (torch.randn(R, 3, generator=g), torch.randn(R, generator=g), torch.randn(R, generator=g))
    bounds = ray_bounds(inp["packed_info"])
    for epilogue in (False, True):
        for use in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
            sg = inp["sigma"].double().requires_grad_(True)
            ref = composite_ref(inp["ts"], inp["te"], sg, inp["packed_info"], inp["rgb"])
            outs = (ref["rgb"], ref["acc"], ref["depth"] if epilogue else ref["num"])
            sum((o * u.double()).sum() for o, u, on in zip(outs, up, use) if on).backward()
            emu = emulate_render_grad_f32(inp, epilogue, *(u if on else None for u, on in zip(up, use)))
            e, l2, eb = nmax_err(emu, sg.grad, 1e-12), rel_l2(emu, sg.grad), blockwise_nmax_err(emu, sg.grad, bounds)
            print(f"emulated backward sigma={sigma:.4g} step={step} epilogue={epilogue} use={use} nmax={e:.2e} l2={l2:.2e} per_ray={eb:.2e}")
            assert e < TOL_GRAD / 4 and l2 < TOL_GRAD / 4, (sigma, step, epilogue, use, e, l2)
            if use == (True, False, False):
                assert eb < TOL_GRAD_BLOCK / 4, (sigma, step, epilogue, use, eb)
            shifted = emulated_per_ray_grad_error(inp, epilogue, sg.grad, *(u if on else None for u, on in zip(up, use)))
            print(f"  with t_end +-2^-24: per_ray={shifted:.2e}")
            assert eb <= shifted < 0.25, (sigma, step, epilogue, use, shifted)
