"""lse_distortion_fwd / lse_distortion_bwd on the device against the float64 twin (tests/distortion_ref.py) at trained-scene
densities, at the bars tests/test_distortion_cpu.py holds the float32 emulation to with a factor 4 to spare; finiteness, ray
isolation, capacity-extent arrays, determinism, the fused d_sigma against lse_render_weight_bwd, and the nerfacc-style entry."""
import ctypes

import numpy as np
import pytest
import torch

from tests import distortion_ref as dr
from tests.util import TOL_FWD, TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, nmax_err, ray_bounds, rel_l2, select_rays, trained_scene_rays

pytestmark = pytest.mark.gpu

BARS = {"loss": TOL_FWD, "d_weights": TOL_GRAD, "d_weights_ray": TOL_GRAD_BLOCK, "d_sigma": TOL_GRAD, "d_sigma_l2": TOL_GRAD,
        "d_sigma_ray": TOL_GRAD_BLOCK}
CASES = [(sg, st) for sg in dr.SIGMAS for st in dr.STEPS]
NAN = float("nan")


def _ops():
    from lsenerf_amd import ops
    return ops


def _cuda(inp):
    return {k: v.cuda() for k, v in inp.items()}


@torch.no_grad()
def _weights(d):
    return _ops().render_weight_from_density(d["ts"], d["te"], d["sigma"], d["packed_info"])[0]


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _run(d, w, g, g_stride, t_scale, n=None, sigma=True, fill=NAN):
    """Both kernels through the C-ABI on device tensors: (loss [R], totals [R,2], d_weights, d_sigma), the per-sample outputs
    pre-filled with ``fill``.  ``n``: extent of the per-sample outputs (default: that of ``w``)."""
    from lsenerf_amd import _lib
    R = d["packed_info"].shape[0]
    n = w.shape[0] if n is None else n
    loss, totals = torch.full((R,), NAN, device="cuda"), torch.full((R, 2), NAN, device="cuda")
    dw, ds = torch.full((n,), fill, device="cuda"), torch.full((n,), fill, device="cuda")
    g = torch.as_tensor(g, dtype=torch.float32).reshape(-1).cuda()
    assert g.numel() == (R if g_stride else 1)
    _lib.call("lse_distortion_fwd", _p(d["ts"]), _p(d["te"]), _p(w), _p(d["packed_info"]), R, t_scale, _p(loss), _p(totals), None)
    _lib.call("lse_distortion_bwd", _p(d["ts"]), _p(d["te"]), _p(d["sigma"]) if sigma else None, _p(w), _p(d["packed_info"]), R, t_scale,
              _p(totals), _p(g), g_stride, _p(dw), _p(ds), None)
    torch.cuda.synchronize()
    return loss, totals, dw, ds


def _errors(loss, dw, ds, ref, bounds):
    return {"loss": nmax_err(loss, ref["loss"]),
            "d_weights": nmax_err(dw, ref["d_weights"], 1e-12), "d_weights_ray": blockwise_nmax_err(dw, ref["d_weights"], bounds),
            "d_sigma": nmax_err(ds, ref["d_sigma"], 1e-12), "d_sigma_l2": rel_l2(ds, ref["d_sigma"]),
            "d_sigma_ray": blockwise_nmax_err(ds, ref["d_sigma"], bounds)}


@pytest.mark.parametrize("sigma,step", CASES, ids=[f"{sg:g}-{st}" for sg, st in CASES])
def test_kernels_against_the_float64_twin(sigma, step):
    """Per-ray loss < TOL_FWD; d_weights and d_sigma < TOL_GRAD over all samples (d_sigma in l2 too) and < TOL_GRAD_BLOCK per ray,
    for per-ray and scalar upstream gradients and t_scale 1 and 0.25; the fused d_sigma agrees with lse_render_weight_bwd on the
    kernel's own d_weights at TOL_GRAD; the autograd op hands out the kernel's bits."""
    from lsenerf_amd import _lib
    ops = _ops()
    inp, ref1, g_ray = dr.case(sigma, step)
    bounds = ray_bounds(inp["packed_info"])
    d = _cuda(inp)
    w = _weights(d)
    for g_stride, t_scale in dr.COMBOS:
        g = g_ray if g_stride else dr.G_SCALAR
        loss, totals, dw, ds = _run(d, w, g, g_stride, t_scale)
        for name, t in (("loss", loss), ("totals", totals), ("d_weights", dw), ("d_sigma", ds)):
            assert bool(torch.isfinite(t).all()), f"{name}: {int((~torch.isfinite(t)).sum())} values not finite or not written"
        err = _errors(loss, dw, ds, dr.scaled(ref1, inp, g, t_scale), bounds)
        print(f"DISTORTION sigma {sigma:g} {step} g_stride {g_stride} t_scale {t_scale}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        for k, v in err.items():
            assert v < BARS[k], (k, v, BARS[k])
        # the existing route over the same numbers: render_weight_from_density's backward fed the kernel's d_weights
        via = torch.empty_like(ds)
        _lib.call("lse_render_weight_bwd", _p(d["ts"]), _p(d["te"]), _p(d["sigma"]), _p(d["packed_info"]), inp["packed_info"].shape[0],
                  _p(w), _p(dw), _p(via), None)
        e, l2 = nmax_err(ds, via, 1e-12), rel_l2(ds, via)
        print(f"DISTORTION   fused d_sigma against lse_render_weight_bwd: nmax {e:.2e} l2 {l2:.2e}")
        assert e < TOL_GRAD and l2 < TOL_GRAD
        assert nmax_err(totals[:, 0], torch.zeros(totals.shape[0], device="cuda").index_add(0, d["ray_indices"], w)) < TOL_FWD
    # the autograd ops: the same launches, so the same bits (weights of volume_render_depth: group_weights, as above)
    sg = d["sigma"].clone().requires_grad_(True)
    w_vr = ops.volume_render_depth(d["ts"], d["te"], sg, d["rgb"], d["packed_info"])[3]
    assert torch.equal(w_vr, w) and not w_vr.requires_grad
    out = ops.distortion_loss(d["ts"], d["te"], sg, w_vr, d["packed_info"], 0.25)
    (out * g_ray.cuda()).sum().backward(retain_graph=True)
    loss, _, dw, ds = _run(d, w, g_ray, 1, 0.25)
    assert torch.equal(out.detach(), loss) and torch.equal(sg.grad, ds)
    sg.grad = None
    out.sum().backward()                                    # a broadcast gradient goes in as one scalar (g_stride 0)
    assert torch.equal(sg.grad, _run(d, w, 1.0, 0, 0.25)[3])
    wl = w.clone().requires_grad_(True)
    (ops.distortion_from_weights(wl, d["ts"], d["te"], d["packed_info"], 0.25) * g_ray.cuda()).sum().backward()
    assert torch.equal(wl.grad, dw)


@pytest.mark.parametrize("step", dr.STEPS)
@pytest.mark.parametrize("sigma", (3e38, float("inf")))
def test_finite_at_densities_beyond_any_gradient(sigma, step):
    """sigma = 3e38 and +inf: the weights are in [0, 1] whatever the density, so the loss and d_weights are finite and right."""
    inp = trained_scene_rays(sigma, seed=0, step=step, onset="ramp")
    d = _cuda(inp)
    w = _weights(d)
    g = torch.from_numpy(np.random.default_rng(5).random(inp["packed_info"].shape[0]).astype(np.float32) + 0.5)
    loss, totals, dw, _ = _run(d, w, g, 1, 1.0, sigma=False)
    for name, t in (("loss", loss), ("totals", totals), ("d_weights", dw)):
        assert bool(torch.isfinite(t).all()), name
    ref = dr.reference(dict(inp, sigma=inp["sigma"].clamp_max(1e30)), 1.0, g)      # (the same weights in float64: exp(-3e27) = 0)
    e, ew, ewb = nmax_err(loss, ref["loss"]), nmax_err(dw, ref["d_weights"], 1e-12), \
        blockwise_nmax_err(dw, ref["d_weights"], ray_bounds(inp["packed_info"]))
    print(f"DISTORTION sigma {sigma:g} {step}: loss {e:.2e} d_weights {ew:.2e} per ray {ewb:.2e}")
    assert e < TOL_FWD and ew < TOL_GRAD and ewb < TOL_GRAD_BLOCK


def test_a_ray_does_not_depend_on_the_other_rays():
    inp, _, g = dr.case(1e5, "cone")
    keep = torch.arange(inp["packed_info"].shape[0]) % 3 != 1
    sub = select_rays(inp, keep)
    d, ds_ = _cuda(inp), _cuda(sub)
    full = _run(d, _weights(d), g, 1, 1.0)
    part = _run(ds_, _weights(ds_), g[keep], 1, 1.0)
    ks = keep[inp["ray_indices"]].cuda()
    for name, a, b in zip(("loss", "totals", "d_weights", "d_sigma"), full, part):
        sel = a[keep.cuda()] if name in ("loss", "totals") else a[ks]
        assert torch.equal(sel, b), name


def test_capacity_extent_arrays_and_determinism():
    """The count-free path hands over arrays of capacity extent: what lies behind the last ray is NaN here and must reach no
    result, and the per-sample outputs behind it keep their fill.  Two calls give the same bits."""
    inp, _, g = dr.case(1e3, "const")
    d = _cuda(inp)
    w = _weights(d)
    n, pad = w.shape[0], 777
    first = _run(d, w, g, 1, 1.0)
    again = _run(d, w, g, 1, 1.0)
    for name, a, b in zip(("loss", "totals", "d_weights", "d_sigma"), first, again):
        assert torch.equal(a, b), name
    tail = torch.full((pad,), NAN, device="cuda")
    big = dict(d, ts=torch.cat([d["ts"], tail]), te=torch.cat([d["te"], tail]), sigma=torch.cat([d["sigma"], tail]))
    padded = _run(big, torch.cat([w, tail]), g, 1, 1.0, n=n + pad, fill=-7.0)
    assert torch.equal(padded[0], first[0]) and torch.equal(padded[1], first[1])
    for a, b in zip(padded[2:], first[2:]):
        assert torch.equal(a[:n], b) and bool((a[n:] == -7.0).all())
    # and the autograd op on such arrays (what render_packed calls with n_dev)
    sg = big["sigma"].clone().requires_grad_(True)
    _ops().distortion_loss(big["ts"], big["te"], sg, torch.cat([w, tail]), d["packed_info"]).backward(g.cuda())
    assert torch.equal(sg.grad[:n], first[3])


def test_nerfacc_style_entry_against_torch_ops():
    """nerfacc_compat.distortion(weights, t_starts, t_ends, ray_indices, n_rays) on three rays (70, 1 and 5 samples, none for a
    fourth) against the double sum written with torch ops, value and gradient."""
    from lsenerf_amd import nerfacc_compat
    rng = np.random.default_rng(11)
    cnt = torch.tensor([70, 1, 0, 5])
    n = int(cnt.sum())
    edges = np.cumsum(0.01 + 0.05 * rng.random(n + 4)).astype(np.float32)
    ts = torch.from_numpy(np.concatenate([edges[0:70], edges[71:72], edges[73:78]]))
    te = torch.from_numpy(np.concatenate([edges[1:71], edges[72:73], edges[74:79]]))
    w = torch.from_numpy((0.1 * rng.random(n)).astype(np.float32))
    ri = torch.repeat_interleave(torch.arange(4), cnt)
    up = torch.tensor([1.5, -0.5, 3.0, 0.75])
    wg = w.cuda().requires_grad_(True)
    out = nerfacc_compat.distortion(wg, ts.cuda(), te.cuda(), ray_indices=ri.cuda(), n_rays=4)
    (out * up.cuda()).sum().backward()
    wr = w.double().requires_grad_(True)
    packed = torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], -1)
    ref = dr.loss64(wr, ts, te, packed)
    (ref * up.double()).sum().backward()
    assert out.shape == (4,) and float(out.detach()[2]) == 0.0
    assert nmax_err(out, ref) < TOL_FWD and nmax_err(wg.grad, wr.grad, 1e-12) < TOL_GRAD
    assert blockwise_nmax_err(wg.grad, wr.grad, ray_bounds(packed)) < TOL_GRAD_BLOCK
    # the packed_info form, and no samples at all: zeros without a launch
    assert torch.equal(nerfacc_compat.distortion(w.cuda(), ts.cuda(), te.cuda(), packed_info=packed.cuda()), out.detach())
    z = torch.zeros(0, device="cuda")
    assert nerfacc_compat.distortion(z, z, z, packed_info=torch.zeros(3, 2, dtype=torch.int64, device="cuda")).tolist() == [0.0] * 3
