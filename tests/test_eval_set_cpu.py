"""Whole-eval-set evaluation, the parts that need no GPU: the three C-ABI entry points and the workspace query (declared, bound,
exported, arguments refused before any launch), the float64 numpy restatement of the reference's event-only scale fit
(``to_gray`` / ``correct_img_scale`` / ``solve_normal_equations``, R:lse_nerf/utils.py:99-135) that tests/test_gpu_eval_set.py
imports, and the host logic of ``evaluate_set`` with the device calls replaced."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSE_E_INVALID = -1
ENTRY_POINTS = ("lse_camera_rays", "lse_eval_image_prep", "lse_log_scale_correct", "lse_log_scale_correct_workspace")
GRAY = (0.2989, 0.5870, 0.1140)
EPS = 1e-6


# ----------------------------------------------------------------------------------------------------
# float64 restatement (imported by the GPU tests)
# ----------------------------------------------------------------------------------------------------
def to_gray64(img) -> np.ndarray:
    """[..., 3] -> [...]: img @ (0.2989, 0.5870, 0.1140), in float64."""
    img = np.asarray(img, dtype=np.float64)
    return img[..., 0] * GRAY[0] + img[..., 1] * GRAY[1] + img[..., 2] * GRAY[2]


def scale_fit_f64(gt, pred):
    """``(a, b, corrected, gray)`` of the reference's event-only metric in float64: ``gt`` [H, W, 3] is the (masked) ground truth,
    ``pred`` [H, W, 3] the (unmasked) prediction whose blue channel is zeroed and whose channels are summed; y = log(gray + 1e-6),
    x = log(pred_r + pred_g + 1e-6); the normal equations of y ~ a x + b; a NaN coefficient becomes 5/255 (a singular system counts
    as NaN: the reference's ``inv`` raises there); corrected = exp(a x + b)."""
    gray = to_gray64(gt)
    pred = np.asarray(pred, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = np.log(gray + EPS).reshape(-1)
        x = np.log(pred[..., 0] + pred[..., 1] + EPS).reshape(-1)
        n = float(x.size)
        sx, sxx, sy, sxy = x.sum(), (x * x).sum(), y.sum(), (x * y).sum()
        det = n * sxx - sx * sx
        # "zero": within the rounding of the two terms (a constant x leaves rounding noise, not 0.0); the kernel's rule
        if not math.isfinite(det) or not abs(det) > 2.0 ** -40 * abs(n * sxx):
            a = b = math.nan
        else:
            a, b = (n * sxy - sx * sy) / det, (sxx * sy - sx * sxy) / det
        a = 5 / 255 if math.isnan(a) else float(a)
        b = 5 / 255 if math.isnan(b) else float(b)
        corrected = np.exp(a * x + b).reshape(gray.shape)
    return a, b, corrected, gray


def seeded_pair(h: int, w: int, seed: int, masked: bool):
    """The inputs of the scale-correction tests as float32 arrays: pred ~ U(0.02, 1) [h, w, 3], gt = clip(0.7 pred^1.3 * U(0.8,
    1.25), 0, 1), and a {0, 1} float32 mask [h, w] over ~70 % of the pixels (None when not ``masked``)."""
    rng = np.random.default_rng(seed)
    pred = rng.uniform(0.02, 1.0, (h, w, 3)).astype(np.float32)
    gt = np.clip(0.7 * pred.astype(np.float64) ** 1.3 * rng.uniform(0.8, 1.25, (h, w, 3)), 0.0, 1.0).astype(np.float32)
    msk = (rng.uniform(size=(h, w)) > 0.3).astype(np.float32) if masked else None
    return gt, pred, msk


def test_scale_fit_recovers_an_exact_power_law():
    rng = np.random.default_rng(3)
    a0, b0 = 1.3, -0.35
    pred = rng.uniform(0.05, 1.0, (19, 23, 3))
    s = pred[..., 0] + pred[..., 1] + EPS
    gray = math.exp(b0) * s ** a0 - EPS                       # gray + eps = exp(b0) (r + g + eps)^a0, exactly
    gt = np.repeat((gray / sum(GRAY))[..., None], 3, axis=-1)
    a, b, corrected, g = scale_fit_f64(gt, pred)
    assert abs(a - a0) <= 1e-9 and abs(b - b0) <= 1e-9, (a, b)
    assert np.allclose(g, gray, rtol=1e-12, atol=0) and np.allclose(corrected, gray + EPS, rtol=1e-8, atol=0)
    # the prediction's blue channel does not enter
    pred2 = pred.copy()
    pred2[..., 2] = 7.0
    assert scale_fit_f64(gt, pred2)[:2] == (a, b)


def test_scale_fit_nan_rule():
    rng = np.random.default_rng(4)
    pred = rng.uniform(0.05, 1.0, (12, 13, 3))
    gt = rng.uniform(0.05, 1.0, (12, 13, 3))
    gt[5, 6] = -0.5                                           # grey level below -1e-6: log of a negative number
    a, b, corrected, _ = scale_fit_f64(gt, pred)
    assert a == 5 / 255 and b == 5 / 255
    assert np.all(np.isfinite(corrected))
    # a constant prediction: singular normal equations count as NaN too
    a, b, corrected, _ = scale_fit_f64(rng.uniform(0.05, 1.0, (12, 13, 3)), np.full((12, 13, 3), 0.5))
    assert a == 5 / 255 and b == 5 / 255 and np.all(np.isfinite(corrected))


def test_seeded_pair_is_what_the_issue_states():
    gt, pred, msk = seeded_pair(37, 53, 1, True)
    assert gt.dtype == pred.dtype == msk.dtype == np.float32
    assert pred.min() >= 0.02 and pred.max() <= 1.0 and gt.min() >= 0.0 and gt.max() <= 1.0
    assert set(np.unique(msk)) == {0.0, 1.0} and 0.5 < msk.mean() < 0.9
    a, b, _, _ = scale_fit_f64(gt, pred)
    assert 0.3 < a < 1.5 and -1.5 < b < 0.5                  # a usable fit, far from the NaN rule's 5/255
    assert seeded_pair(37, 53, 1, False)[2] is None


# ----------------------------------------------------------------------------------------------------
# bindings and refusals
# ----------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    from lsenerf_amd import _lib, ops
    import lsenerf_amd as la
    hdr = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/lse_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib"
        assert hasattr(lib, name), f"liblse_hip.so does not export {name}"
    assert lib.lse_abi_version() == 6 and _lib.LSE_ABI_VERSION == 6
    assert "#define LSE_ABI_VERSION 6" in hdr
    for name in ("camera_rays", "eval_image_prep", "log_scale_correct"):
        assert callable(getattr(ops, name))
    assert la.EvalSet is not None and callable(la.evaluate_set) and callable(la.LSENeRFModel.evaluate_set)
    assert ctypes.sizeof(_lib.CameraDesc) == 13 * 4


def _ptr():
    """A host buffer's address, 16-byte aligned: validation never dereferences it and refuses the call before any launch."""
    buf = (ctypes.c_float * 16)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(addr)


def test_camera_rays_refuses_bad_arguments_without_gpu():
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    keep, p = _ptr()
    cam = ops.camera_desc(30.0, 30.0, 20.0, 12.0, 24, 40)
    assert cam.distort == 0 and ops.camera_desc(30.0, 30.0, 20.0, 12.0, 24, 40, (0.1, 0, 0, 0, 0, 0)).distort == 1

    def rays(first=0, n=4, pose=p, out=p, last=p, desc=cam):
        return lib.lse_camera_rays(ctypes.byref(desc) if desc is not None else None, pose, first, n, out, out, out, last, None)
    assert rays(desc=None) == LSE_E_INVALID and b"lse_camera_rays: null descriptor" in lib.lse_last_error()
    assert rays(first=-1) == LSE_E_INVALID and b"first < 0" in lib.lse_last_error()
    assert rays(n=-1) == LSE_E_INVALID and b"n < 0" in lib.lse_last_error()
    assert rays(first=957, n=4) == LSE_E_INVALID and b"leave the 24 x 40 image" in lib.lse_last_error()
    assert rays(first=961, n=0) == LSE_E_INVALID and rays(first=0, n=961) == LSE_E_INVALID
    assert rays(first=2 ** 62, n=2 ** 62) == LSE_E_INVALID                    # no overflow in first + n
    assert rays(out=None) == LSE_E_INVALID and b"null output" in lib.lse_last_error()
    assert rays(last=None) == LSE_E_INVALID and b"null output" in lib.lse_last_error()
    assert rays(pose=None) == LSE_E_INVALID and b"null pose" in lib.lse_last_error()
    assert rays(desc=ops.camera_desc(0.0, 30.0, 20.0, 12.0, 24, 40)) == LSE_E_INVALID and b"focal" in lib.lse_last_error()
    assert rays(desc=ops.camera_desc(30.0, 30.0, 20.0, 12.0, 0, 40)) == LSE_E_INVALID
    assert rays(first=0, n=0, pose=None, out=None, last=None) == 0            # zero-sized work is a no-op, not an error
    assert rays(first=960, n=0, pose=None, out=None, last=None) == 0
    with pytest.raises(_lib.LseHipError, match="first < 0"):
        _lib.call("lse_camera_rays", ctypes.byref(cam), p, -3, 4, p, p, p, p, None)
    # the wrapper: shapes on the host, then "no CPU fallback"
    with pytest.raises(ValueError, match="pose"):
        ops.camera_rays(cam, torch.zeros(4, 4), 0, 4)
    with pytest.raises(ValueError, match="at least 8 rows"):
        ops.camera_rays(cam, torch.zeros(3, 4), 0, 8, out=(torch.zeros(4, 3), torch.zeros(8, 3), torch.zeros(8, 1), torch.zeros(8, 1)))
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.camera_rays(cam, torch.zeros(3, 4), 0, 4)
    del keep


def test_prep_and_correct_refuse_bad_arguments_without_gpu():
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)
    U8, F32, NONE = _lib.LSE_PIX_U8, _lib.LSE_PIX_F32, _lib.LSE_PIX_NONE
    need = ops.log_scale_correct_workspace_bytes(24, 40)
    assert need == 4 * 8 and ops.log_scale_correct_workspace_bytes(480, 640) == 4 * 8 * 75
    v = ctypes.c_int64(0)
    assert lib.lse_log_scale_correct_workspace(24, 40, None) == LSE_E_INVALID
    assert lib.lse_log_scale_correct_workspace(0, 40, ctypes.byref(v)) == LSE_E_INVALID

    def prep(gt=p, gt_type=U8, msk=None, msk_type=NONE, rgb=p, H=24, W=40, flags=0, a=p, b=p, stats=None, nbytes=0):
        return lib.lse_eval_image_prep(gt, gt_type, msk, msk_type, rgb, H, W, flags, a, b, stats, nbytes, None)
    assert prep(gt=None) == LSE_E_INVALID and b"lse_eval_image_prep: null pointer" in lib.lse_last_error()
    assert prep(b=None) == LSE_E_INVALID and b"null pointer" in lib.lse_last_error()
    assert prep(H=0) == LSE_E_INVALID and b"H and W" in lib.lse_last_error()
    assert prep(gt_type=_lib.LSE_PIX_I16) == LSE_E_INVALID and b"gt_type" in lib.lse_last_error()
    assert prep(msk_type=_lib.LSE_PIX_I32, msk=p) == LSE_E_INVALID and b"msk_type" in lib.lse_last_error()
    assert prep(msk_type=F32, msk=None) == LSE_E_INVALID and b"null mask" in lib.lse_last_error()
    assert prep(flags=2) == LSE_E_INVALID and b"unknown flags" in lib.lse_last_error()
    assert prep(flags=1) == LSE_E_INVALID and b"null stats" in lib.lse_last_error()
    assert prep(flags=1, stats=p, nbytes=need - 8) == LSE_E_INVALID and b"stats workspace of" in lib.lse_last_error()
    assert prep(flags=1, stats=odd, nbytes=need) == LSE_E_INVALID and b"8-byte aligned" in lib.lse_last_error()

    def corr(gt=p, rgb=p, H=24, W=40, stats=p, nbytes=need, coef=p, c=p, g=p):
        return lib.lse_log_scale_correct(gt, rgb, H, W, stats, nbytes, coef, c, g, None)
    assert corr(gt=None) == LSE_E_INVALID and b"lse_log_scale_correct: null pointer" in lib.lse_last_error()
    assert corr(coef=None) == LSE_E_INVALID and corr(stats=None) == LSE_E_INVALID and corr(g=None) == LSE_E_INVALID
    assert corr(W=-1) == LSE_E_INVALID and b"H and W" in lib.lse_last_error()
    assert corr(nbytes=8) == LSE_E_INVALID and b"stats workspace of" in lib.lse_last_error()
    assert corr(stats=odd) == LSE_E_INVALID and b"8-byte aligned" in lib.lse_last_error()
    # the wrappers
    gt, rgb = torch.zeros(24, 40, 3, dtype=torch.uint8), torch.zeros(960, 3)
    with pytest.raises(ValueError, match="gt must be"):
        ops.eval_image_prep(gt.to(torch.int16), rgb)
    with pytest.raises(ValueError, match="rgb must be"):
        ops.eval_image_prep(gt, torch.zeros(959, 3))
    with pytest.raises(ValueError, match="msk must be"):
        ops.eval_image_prep(gt, rgb, msk=torch.zeros(24, 41))
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.eval_image_prep(gt, rgb)
    with pytest.raises(ValueError, match="stats of at least"):
        ops.log_scale_correct(torch.zeros(1, 3, 24, 40), rgb, torch.zeros(1, dtype=torch.float64))
    with pytest.raises(ValueError, match="gt_planes must be"):
        ops.log_scale_correct(torch.zeros(3, 24, 40), rgb, torch.zeros(4, dtype=torch.float64))
    del keep


# ----------------------------------------------------------------------------------------------------
# host logic of evaluate_set, the device calls replaced
# ----------------------------------------------------------------------------------------------------
H, W = 12, 14


class _Grid:
    def __init__(self):
        self.reads = 0

    def check_deferred_overflow(self):
        self.reads += 1


class _LPIPS:
    def __init__(self, available):
        self.available = available
        self.calls = []

    def __call__(self, a, b):
        assert self.available
        self.calls.append((tuple(a.shape), tuple(b.shape)))
        return torch.tensor(0.25 + 0.01 * len(self.calls))


class _Model:
    def __init__(self, lpips_available, training=False):
        self.training = training
        self.occupancy_grid = _Grid()
        self.lpips = _LPIPS(lpips_available)
        self.modes = []

    def eval(self):
        self.training = False
        self.modes.append("eval")

    def train(self):
        self.training = True
        self.modes.append("train")


def _eval_set(n=3):
    from lsenerf_amd import EvalSet
    from lsenerf_amd.cameras import EdCameras
    c2w = torch.eye(4)[:3][None].repeat(n, 1, 1)
    cams = EdCameras(c2w, fx=10.0, fy=10.0, cx=W / 2, cy=H / 2, width=W, height=H, times=torch.arange(n).float())
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (n, H, W, 3), generator=g, dtype=torch.uint8)
    return EvalSet("cpu", images, cams, msk=torch.ones(n, H, W, dtype=torch.bool))


def _patch_device_calls(monkeypatch, log):
    """camera_bundle / render_flat / the three ops as host stand-ins that record their calls; image i gets ssim 0.5 + 0.1 i and
    mse 10^-(i + 1) (colour) or ssim 0.9 - 0.1 i and mse 10^-(i + 2) (the C = 1 event-only planes)."""
    from lsenerf_amd import eval_set as es, evaluation, ops, RayBundle

    def camera_bundle(s, i):
        log.append(("bundle", i))
        rb = RayBundle(origins=torch.zeros(H, W, 3), directions=torch.zeros(H, W, 3),
                       camera_indices=torch.full((H, W, 1), i, dtype=torch.long))
        return rb

    def render_flat(model, rb, check_overflow=True):
        assert check_overflow is False and not model.training
        i = int(rb.camera_indices[0, 0])
        log.append(("render", i))
        return {"rgb": torch.full((H * W, 3), 0.1 * (i + 1)), "accumulation": torch.ones(H * W, 1), "depth": torch.ones(H * W, 1)}

    def eval_image_prep(gt, rgb, msk=None, event_stats=False, out=None, stats=None):
        i = int(round(float(rgb[0, 0]) * 10)) - 1
        log.append(("prep", i, event_stats, gt.dtype, None if msk is None else msk.dtype))
        out[0].fill_(float(i))
        out[1].copy_(rgb.reshape(H, W, 3).permute(2, 0, 1)[None])
        return out[0], out[1], stats

    def log_scale_correct(gt_planes, rgb, stats, out=None):
        log.append(("correct", int(gt_planes[0, 0, 0, 0])))
        out[1].fill_(float(gt_planes[0, 0, 0, 0]))
        out[2].fill_(float(gt_planes[0, 0, 0, 0]))
        return out

    def image_metrics(a, b, out=None, workspace=None):
        i = int(a.reshape(-1)[0])
        log.append(("metrics", i, a.shape[1]))
        out[0] = 0.5 + 0.1 * i if a.shape[1] == 3 else 0.9 - 0.1 * i
        out[1] = 10.0 ** -(i + 1) if a.shape[1] == 3 else 10.0 ** -(i + 2)
        return out[0], out[1]
    monkeypatch.setattr(es, "camera_bundle", camera_bundle)
    monkeypatch.setattr(evaluation, "render_flat", render_flat)
    monkeypatch.setattr(ops, "eval_image_prep", eval_image_prep)
    monkeypatch.setattr(ops, "log_scale_correct", log_scale_correct)
    monkeypatch.setattr(ops, "image_metrics", image_metrics)


@pytest.mark.parametrize("events_only", [False, True])
@pytest.mark.parametrize("lpips", [False, True])
def test_evaluate_set_host_logic(monkeypatch, events_only, lpips):
    from lsenerf_amd import evaluate_set
    log, seen = [], []
    _patch_device_calls(monkeypatch, log)
    model, s = _Model(lpips, training=True), _eval_set(3)

    def on_image(i, outputs, images):
        seen.append(i)
        assert tuple(outputs["rgb"].shape) == (H, W, 3)
        assert set(images) == {"img", "accumulation", "depth", "err_map"}
        assert tuple(images["img"].shape) == (H, 2 * W, 3) and tuple(images["err_map"].shape) == (H, W, 3)
    average, per_image = evaluate_set(model, s, events_only=events_only, on_image=on_image)
    assert seen == [0, 1, 2]                                                  # every index once, in order
    assert model.occupancy_grid.reads == 1 and model.modes == ["eval", "train"] and model.training
    keys = {"psnr", "ssim"} | ({"lpips"} if lpips else set())
    assert len(per_image) == 3 and all(set(r) == keys for r in per_image)
    assert set(average) == keys | {"num_rays_per_sec", "fps"}
    assert average["fps"] > 0 and average["num_rays_per_sec"] == pytest.approx(average["fps"] * H * W)
    for i, r in enumerate(per_image):
        ssim, mse = (0.9 - 0.1 * i, 10.0 ** -(i + 2)) if events_only else (0.5 + 0.1 * i, 10.0 ** -(i + 1))
        assert r["ssim"] == pytest.approx(ssim, rel=1e-6)
        assert r["psnr"] == pytest.approx(10 * math.log10(1 / mse), rel=1e-6)
    for k in keys:                                                            # the averages: float32 means of the rows
        assert average[k] == pytest.approx(float(np.mean(np.array([r[k] for r in per_image], dtype=np.float32))), rel=1e-6)
    # per image: rays, render, prep (+ correction), metrics on the right planes, in that order
    want = []
    for i in range(3):
        want += [("bundle", i), ("render", i), ("prep", i, events_only, torch.uint8, torch.uint8)]
        want += [("correct", i), ("metrics", i, 1)] if events_only else [("metrics", i, 3)]
    assert log == want
    if lpips:                                                                 # three channels either way
        assert model.lpips.calls == [((1, 3, H, W), (1, 3, H, W))] * 3
    else:
        assert model.lpips.calls == []


def test_evaluate_set_without_callback_and_eval_set_poses(monkeypatch):
    from lsenerf_amd import evaluate_set
    log = []
    _patch_device_calls(monkeypatch, log)
    model, s = _Model(False), _eval_set(2)
    average, per_image = evaluate_set(model, s)
    assert len(per_image) == 2 and model.modes == [] and not model.training   # an eval-mode model is left alone
    assert len(s) == 2 and tuple(s.poses.shape) == (2, 3, 4) and s.poses.data_ptr() != s.cameras.camera_to_worlds.data_ptr()
    ptr = s.poses.data_ptr()
    s.set_poses(s.poses + 1.0)
    assert s.poses.data_ptr() == ptr and float(s.poses[0, 0, 0]) == 2.0        # in place
    assert float(s.cameras.camera_to_worlds[0, 0, 0]) == 1.0                  # the cameras' own poses are not touched
    with pytest.raises(ValueError, match="pose table"):
        s.set_poses(torch.zeros(3, 3, 4))
    with pytest.raises(ValueError, match="eval images"):
        from lsenerf_amd import EvalSet
        EvalSet("cpu", torch.zeros(2, H, W, dtype=torch.uint8), s.cameras)
