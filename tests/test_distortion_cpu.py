"""Distortion loss without a device: the twins (tests/distortion_ref.py) on hand-made rays and against each other at trained-scene
densities -- every bar tests/test_gpu_distortion.py asserts, with a factor 4 to spare, on the same seeded inputs -- the two
formulations the kernels do not use and why, the config fields, and header / binding / library agreement."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import distortion_ref as dr
from tests.util import TOL_FWD, TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, nmax_err, ray_bounds, rel_l2, trained_scene_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _rays(weights, t0=1.0, dt=0.1):
    """Hand-made rays of contiguous samples of length dt with the given WEIGHTS (lists; several: packed in order)."""
    ts, te, w, cnt = [], [], [], []
    for ws in weights:
        e = (t0 + dt * np.arange(len(ws) + 1)).astype(F)
        ts.append(e[:-1]); te.append(e[1:]); w.append(np.asarray(ws, F)); cnt.append(len(ws))
    cnt = torch.tensor(cnt, dtype=torch.int64)
    cat = lambda parts: torch.from_numpy(np.concatenate(parts))       # noqa: E731
    return cat(ts), cat(te), cat(w), torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], -1)


def test_hand_made_rays():
    """No sample: 0.  One sample: the interval term alone.  Two samples: 2 w0 w1 (m1 - m0) + the interval terms.  A delta of weight
    has only its own width; the same weight split over two distant samples pays their distance."""
    ts, te, w, packed = _rays([[], [0.5], [0.25, 0.5], [0.0, 1.0, 0.0, 0.0], [0.5, 0.0, 0.0, 0.5]])
    d = (te - ts).double()
    ref = dr.loss64(w.double(), ts, te, packed)
    em, totals = dr.emulate_fwd_f32(ts, te, w, packed)
    mid = (ts.double() + te.double()) / 2
    want = [0.0, 0.25 * float(d[0]) / 3, 2 * 0.25 * 0.5 * float(mid[2] - mid[1]) + (0.0625 * float(d[1]) + 0.25 * float(d[2])) / 3,
            float(d[4]) / 3, 2 * 0.25 * float(mid[10] - mid[7]) + 0.25 * (float(d[7]) + float(d[10])) / 3]
    assert ref.tolist() == pytest.approx(want, rel=1e-12, abs=0)
    assert em.double().tolist() == pytest.approx(want, rel=1e-6, abs=0)
    assert totals[:, 0].tolist() == [0.0, 0.5, 0.75, 1.0, 1.0] and totals[0].tolist() == [0.0, 0.0]
    assert float(totals[1, 1]) == 0.0                      # M is taken relative to the ray's first mid-point
    # the gradient: dL/dw of the pair ray, by hand
    g = dr.emulate_dw_f32(ts, te, w, packed, totals, 1.0).double()
    m10 = float(mid[2] - mid[1])
    assert g[1:3].tolist() == pytest.approx([2 * 0.5 * m10 + 2 / 3 * 0.25 * float(d[1]), 2 * 0.25 * m10 + 2 / 3 * 0.5 * float(d[2])], rel=1e-6)
    # unsorted mid-points are the twin's business alone: |m_i - m_j| does not care about the order
    perm = torch.tensor([2, 1])
    assert float(dr.loss64(w[perm].double(), ts[perm], te[perm], torch.tensor([[0, 2]]))) == pytest.approx(want[2], rel=1e-12)


def _errors(em, ref, bounds):
    return {"loss": nmax_err(em["loss"], ref["loss"]),
            "d_weights": nmax_err(em["d_weights"], ref["d_weights"], 1e-12), "d_weights_ray": blockwise_nmax_err(em["d_weights"], ref["d_weights"], bounds),
            "d_sigma": nmax_err(em["d_sigma"], ref["d_sigma"], 1e-12), "d_sigma_l2": rel_l2(em["d_sigma"], ref["d_sigma"]),
            "d_sigma_ray": blockwise_nmax_err(em["d_sigma"], ref["d_sigma"], bounds)}


BARS = {"loss": TOL_FWD, "d_weights": TOL_GRAD, "d_weights_ray": TOL_GRAD_BLOCK, "d_sigma": TOL_GRAD, "d_sigma_l2": TOL_GRAD,
        "d_sigma_ray": TOL_GRAD_BLOCK}
CASES = [(sg, st) for sg in dr.SIGMAS for st in dr.STEPS]


@pytest.mark.parametrize("sigma,step", CASES, ids=[f"{sg:g}-{st}" for sg, st in CASES])
def test_emulation_meets_every_gpu_bar_with_a_factor_4_to_spare(sigma, step):
    """Worst figures of this emulation over all cases: per-ray loss 4.6e-6 of TOL_FWD = 2e-5 (the float32 WEIGHTS' own error, 4.4e-6,
    twice over: the loss is quadratic in them), d_weights 2.5e-6 / per ray 3.9e-6, d_sigma 2.6e-6 / l2 2.1e-6 / per ray 3.9e-6."""
    inp, ref1, g_ray = dr.case(sigma, step)
    bounds = ray_bounds(inp["packed_info"])
    for g_stride, t_scale in dr.COMBOS:
        g = g_ray if g_stride else dr.G_SCALAR
        em = dr.emulate_f32(inp, t_scale, g.numpy() if g_stride else g)
        err = _errors(em, dr.scaled(ref1, inp, g, t_scale), bounds)
        print(f"DISTORTION_EMU sigma {sigma:g} {step} g_stride {g_stride} t_scale {t_scale}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        for k, v in err.items():
            assert 4 * v < BARS[k], (k, v, BARS[k])
        assert all(bool(torch.isfinite(em[k]).all()) for k in ("loss", "d_weights", "d_sigma"))


def test_absolute_mid_points_miss_the_per_ray_bars_far_from_the_origin():
    """Why the shift is part of the contract: at t ~ 400 the products m W_< and the sums M_< are ~ 400 and their difference is a
    ray's extent -- an ulp of 400 is 3e-5.  The same rays, the same weights: relative to the ray's first mid-point every bar holds
    with its factor 4; with absolute mid-points the gradients are off by 9e-3 of the ray's own scale."""
    R = trained_scene_rays(30.0)["packed_info"].shape[0]
    inp = trained_scene_rays(30.0, t0=np.full(R, 400.0))
    ref = dr.reference(inp)
    bounds = ray_bounds(inp["packed_info"])
    good, bad = (_errors(dr.emulate_f32(inp, shifted=s), ref, bounds) for s in (True, False))
    print("DISTORTION_EMU t0 = 400 shifted", good, "absolute", bad)
    for k, v in good.items():
        assert 4 * v < BARS[k], (k, v)
    assert bad["d_weights_ray"] > TOL_GRAD_BLOCK and bad["d_sigma_ray"] > TOL_GRAD_BLOCK


def test_t_end_from_the_weights_misses_the_per_ray_bar_behind_a_surface():
    """Why lse_distortion_bwd reads the densities: the recurrence of volrend_bwd_kernel with T_end = 1 - sum w, fed the same
    d_weights, leaves dw_k 2^-24 dt_k behind an opaque surface, and this loss's dw grows with the distance from the ray's centre of
    mass -- 2.3e-2 of the per-ray scale on the cone-step rays, against 2.1e-6 with T_end = exp(-sum sigma dt).  Over all samples the
    two agree far inside TOL_GRAD (3.2e-5): lse_render_weight_bwd on the kernel's own d_weights is a valid cross-check there."""
    inp, ref1, g = dr.case(1e3, "cone")
    ref = dr.scaled(ref1, inp, g, 1.0)
    em = dr.emulate_f32(inp, 1.0, g.numpy())
    bounds = ray_bounds(inp["packed_info"])
    one_minus_w = blockwise_nmax_err(em["d_sigma_1mw"], ref["d_sigma"], bounds)
    from_sigma = blockwise_nmax_err(em["d_sigma"], ref["d_sigma"], bounds)
    same_arith = blockwise_nmax_err(dr.emulate_dsigma_f32(inp["ts"], inp["te"], None, em["weights"], inp["packed_info"], em["d_weights"]),
                                    ref["d_sigma"], bounds)
    print(f"DISTORTION_EMU per-ray d_sigma: T_end = 1 - sum w {one_minus_w:.2e} (this module's scans: {same_arith:.2e}), from sigma {from_sigma:.2e}")
    assert one_minus_w > TOL_GRAD_BLOCK and same_arith > TOL_GRAD_BLOCK and 4 * from_sigma < TOL_GRAD_BLOCK
    assert 4 * nmax_err(em["d_sigma"], em["d_sigma_1mw"], 1e-12) < TOL_GRAD


def test_config_fields_and_their_validation():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    cfg = LSENeRFModelConfig()
    assert cfg.distortion_loss_mult == 0.0 and cfg.distortion_t_scale == 1.0
    box = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    small = dict(grid_levels=1, grid_resolution=16, log2_hashmap_size=12)
    for name in ("distortion_loss_mult", "distortion_t_scale"):
        for bad in (-1e-3, float("nan"), float("inf"), -float("inf"), "0.01", None):
            with pytest.raises(ValueError, match=name):
                LSENeRFModel(LSENeRFModelConfig(**{name: bad}, **small), box, 4)
    m = LSENeRFModel(LSENeRFModelConfig(distortion_loss_mult=0.01, distortion_t_scale=0.25, **small), box, 4)
    assert m.training and m.distortion_on()
    m.eval()
    assert not m.distortion_on()                             # eval mode never computes it
    m.train()
    m.freeze_field()
    assert not m.distortion_on()                             # nor a frozen field
    m.unfreeze_field()
    assert m.distortion_on()
    off = LSENeRFModel(LSENeRFModelConfig(**small), box, 4)
    assert not off.distortion_on()


def _declared(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    m = re.search(r"\b%s\s*\((.*?)\)\s*;" % name, src, flags=re.S)
    assert m, f"include/lse_hip.h does not declare {name}"
    return [a.strip() for a in m.group(1).split(",")]


def test_header_binding_and_library_agree():
    from lsenerf_amd import _lib
    lib = _lib.load()
    assert lib.lse_abi_version() == 6 == _lib.LSE_ABI_VERSION                # additive: the ABI number stays
    fwd = _declared("lse_distortion_fwd")
    assert len(fwd) == 9 == len(_lib.SIGNATURES["lse_distortion_fwd"])
    assert fwd[:4] == ["const float *t_starts", "const float *t_ends", "const float *weights", "const int64_t *packed_info"]
    assert fwd[4:] == ["int32_t n_rays", "float t_scale", "float *out_loss", "float *out_totals", "lse_stream_t stream"]
    bwd = _declared("lse_distortion_bwd")
    assert len(bwd) == 13 == len(_lib.SIGNATURES["lse_distortion_bwd"])
    assert bwd[2:4] == ["const float *sigmas", "const float *weights"] and bwd[5:7] == ["int32_t n_rays", "float t_scale"]
    assert bwd[7:] == ["const float *totals", "const float *g_loss", "int32_t g_stride", "float *d_weights", "float *d_sigmas", "lse_stream_t stream"]
    assert _lib.SIGNATURES["lse_distortion_fwd"][5] is ctypes.c_float and _lib.SIGNATURES["lse_distortion_bwd"][6] is ctypes.c_float
    for name in ("lse_distortion_fwd", "lse_distortion_bwd"):
        assert hasattr(lib, name) and hasattr(ctypes.CDLL(_lib.DEV_LIB_PATH), name), name
    hdr = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    assert "mip-NeRF 360" in hdr and "RELATIVE TO THE RAY'S FIRST" in hdr


def test_argument_checks_need_no_device():
    from lsenerf_amd import _lib, nerfacc_compat, ops
    lib = _lib.load()
    one = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))

    def fwd(n=0, t_scale=1.0, w=one, loss=one):
        return lib.lse_distortion_fwd(one, one, w, one, n, t_scale, loss, None, None)

    def bwd(n=0, t_scale=1.0, stride=1, totals=one, g=one, dw=one, ds=None):
        return lib.lse_distortion_bwd(one, one, None, one, one, n, t_scale, totals, g, stride, dw, ds, None)

    assert fwd() == 0 and fwd(t_scale=0.0) == 0 and bwd() == 0 and bwd(stride=0, dw=None, ds=one) == 0
    for call, who, refused in ((fwd, b"lse_distortion_fwd", {"negative n": dict(n=-1), "negative scale": dict(t_scale=-0.5),
                                                           "nan scale": dict(t_scale=float("nan")), "inf scale": dict(t_scale=float("inf")),
                                                           "null weights": dict(n=4, w=None), "null loss": dict(n=4, loss=None)}),
                               (bwd, b"lse_distortion_bwd", {"negative n": dict(n=-1), "negative scale": dict(t_scale=-0.5),
                                                           "nan scale": dict(t_scale=float("nan")), "stride 2": dict(stride=2),
                                                           "stride -1": dict(stride=-1), "null totals": dict(n=4, totals=None),
                                                           "null g": dict(n=4, g=None), "no output": dict(n=4, dw=None, ds=None)})):
        for what, kw in refused.items():
            assert call(**kw) == -1, what
            assert who in lib.lse_last_error(), what
    # the wrappers: tensors that are not on the device, scale, and the no-sample case (zeros, no launch: nothing here has a GPU)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt)       # noqa: E731
    packed = torch.tensor([[0, 2], [2, 2]])
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        ops.distortion_loss(z(4), z(4), z(4), z(4), packed)
    with pytest.raises(_lib.LseHipError, match="must live on the GPU"):
        nerfacc_compat.distortion(z(4), z(4), z(4), packed_info=packed)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="t_scale"):
            ops.distortion_loss(z(4), z(4), z(4), z(4), packed, t_scale=bad)
    with pytest.raises(ValueError, match="shape"):
        ops.distortion_loss(z(4), z(4), z(3), z(4), packed)
    none = z(3, 2, dt=torch.int64)
    assert ops.distortion_loss(z(0), z(0), z(0), z(0), none).tolist() == [0.0] * 3
    assert nerfacc_compat.distortion(z(0), z(0), z(0), ray_indices=z(0, dt=torch.int64), n_rays=3).tolist() == [0.0] * 3
