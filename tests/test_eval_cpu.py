"""CPU tests of the whole-image evaluation surface: the model methods the reference's pipeline calls at eval time exist, the two new
entry points (lse_eval_composite, lse_image_metrics) are declared, bound and exported, LPIPS without torchmetrics fails by name
and drops out of the metrics, and the float64 numpy restatement of torchmetrics' SSIM that tests/test_gpu_eval.py holds the kernel
against behaves as the algorithm says."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("lse_eval_composite", "lse_image_metrics", "lse_image_metrics_workspace")


# ---- numpy restatement (float64) of torchmetrics structural_similarity_index_measure with its defaults -----------------------------
def _filter_valid(x: np.ndarray, g: np.ndarray) -> np.ndarray:
    """Correlation of the last two axes with outer(g, g), 'valid' windows only (separable: rows, then columns)."""
    k = g.shape[0]
    win = np.lib.stride_tricks.sliding_window_view(x, k, axis=-1)          # [..., H, W-k+1, k]
    x = win @ g
    win = np.lib.stride_tricks.sliding_window_view(x, k, axis=-2)          # [..., H-k+1, W-k+1, k]
    return win @ g


def ssim_numpy(preds: np.ndarray, target: np.ndarray, window: np.ndarray, pad_mode: str = "reflect") -> float:
    """SSIM of [B,C,H,W] images as torchmetrics computes it: pad by (k-1)/2 (``pad_mode``: torchmetrics reflects), filter the five
    moments with the Gaussian window, crop the pad again, mean.  The crop leaves exactly the windows that lie inside the image, so
    the padding mode cannot matter (test below)."""
    p = preds.astype(np.float64)
    t = target.astype(np.float64)
    g = window.astype(np.float64)
    k = g.shape[0]
    r = (k - 1) // 2
    data_range = max(float(p.max() - p.min()), float(t.max() - t.min()))
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    pad = [(0, 0), (0, 0), (r, r), (r, r)]
    pp, tp = np.pad(p, pad, mode=pad_mode), np.pad(t, pad, mode=pad_mode)
    mu_p, mu_t = _filter_valid(pp, g), _filter_valid(tp, g)
    e_pp, e_tt, e_pt = _filter_valid(pp * pp, g), _filter_valid(tp * tp, g), _filter_valid(pp * tp, g)
    s_pp, s_tt, s_pt = e_pp - mu_p ** 2, e_tt - mu_t ** 2, e_pt - mu_p * mu_t
    m = ((2 * mu_p * mu_t + c1) * (2 * s_pt + c2)) / ((mu_p ** 2 + mu_t ** 2 + c1) * (s_pp + s_tt + c2))
    return float(m[..., r:-r, r:-r].mean())


def _window():
    from lsenerf_amd import ops
    return ops.ssim_window().numpy()


# ---- the model surface ----------------------------------------------------------------------------------------------------------
def test_model_has_the_eval_surface():
    """R:lse_nerf/lse_pipeline.py:149-233 and nerfstudio's eval-image step call these on the model."""
    from lsenerf_amd import LSENeRFModel
    for name in ("get_outputs_for_camera_ray_bundle", "get_image_metrics_and_images", "ssim", "lpips", "render_camera", "psnr"):
        assert hasattr(LSENeRFModel, name), name


def test_new_entry_points_declared_bound_exported():
    from lsenerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    lib = _lib.load()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES, name
        assert name in exported and hasattr(lib, name), name
    assert lib.lse_abi_version() == 6
    for flag, v in (("LSE_EVAL_NAN_TO_NUM", 1), ("LSE_EVAL_BACKGROUND", 2), ("LSE_EVAL_CLAMP", 4)):
        assert re.search(r"#define\s+" + flag + r"\s+" + str(v) + r"\b", hdr) and getattr(_lib, flag) == v, flag


def test_image_metrics_workspace_and_refusals_host_side():
    """The workspace query is host-only: sizes follow the tile layout, and images smaller than the 11x11 window are refused with
    the library's message."""
    from lsenerf_amd import _lib, ops
    small = ops.image_metrics_workspace_bytes(1, 1, 11, 11)
    big = ops.image_metrics_workspace_bytes(2, 3, 480, 640)
    assert small == 8 * (5 * 1 + 1)
    assert big == 8 * (5 * 450 + 2 * 3 * 30 * 40)
    for shape in ((1, 1, 10, 11), (1, 1, 11, 10), (0, 1, 32, 32)):
        with pytest.raises(_lib.LseHipError, match="lse_image_metrics_workspace"):
            ops.image_metrics_workspace_bytes(*shape)
    with pytest.raises(ValueError, match=r"\[B,C,H,W\]"):
        ops.image_metrics(torch.zeros(3, 16, 16), torch.zeros(3, 16, 16))


def test_ssim_window_is_torchmetrics_gaussian():
    w = _window()
    assert w.dtype == np.float32 and w.shape == (11,)
    d = np.arange(-5, 6, dtype=np.float32)
    g = np.exp(-((d / np.float32(1.5)) ** 2) / 2).astype(np.float32)
    np.testing.assert_allclose(w, g / g.sum(), rtol=1e-6)
    assert np.array_equal(w, w[::-1]) and abs(float(w.sum()) - 1.0) < 1e-6


def _model_cpu():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(0)
    cfg = LSENeRFModelConfig(grid_levels=1, grid_resolution=16, num_levels=4, log2_hashmap_size=12)
    return LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4)


def test_lpips_without_torchmetrics_is_named_and_omitted(monkeypatch):
    """Where torchmetrics cannot be imported, ``model.lpips`` raises ModuleNotFoundError naming it, and the metrics dictionary of
    get_image_metrics_and_images has psnr / ssim only.  (The SSIM / MSE kernel is replaced by the numpy restatement here.)"""
    from lsenerf_amd import ops
    monkeypatch.setitem(sys.modules, "torchmetrics", None)
    m = _model_cpu()
    with pytest.raises(ModuleNotFoundError, match="torchmetrics") as ei:
        m.lpips(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    assert ei.value.name == "torchmetrics"
    assert m.lpips.available is False

    def image_metrics_numpy(p, t):
        s = ssim_numpy(p.numpy(), t.numpy(), _window())
        return torch.tensor(s, dtype=torch.float32), ((p.double() - t.double()) ** 2).mean().float()
    monkeypatch.setattr(ops, "image_metrics", image_metrics_numpy)
    g = torch.Generator().manual_seed(1)
    H, W = 16, 20
    outputs = {"rgb": torch.rand(H, W, 3, generator=g), "accumulation": torch.rand(H, W, 1, generator=g),
               "depth": torch.rand(H, W, 1, generator=g) * 3}
    batch = {"image": torch.rand(H, W, 3, generator=g), "msk": (torch.rand(H, W, generator=g) > 0.5).float()}
    metrics, images = m.get_image_metrics_and_images(outputs, batch)
    assert set(metrics) == {"psnr", "ssim"}
    msk = batch["msk"][..., None]
    mse = float(((batch["image"] * msk - outputs["rgb"] * msk) ** 2).mean())
    assert metrics["psnr"] == pytest.approx(10 * np.log10(1 / mse), rel=1e-5)
    assert set(images) == {"img", "accumulation", "depth", "err_map"}
    assert tuple(images["img"].shape) == (H, 2 * W, 3) and torch.equal(images["img"][:, W:], outputs["rgb"])
    assert all(tuple(images[k].shape) == (H, W, 3) for k in ("accumulation", "depth", "err_map"))
    # err_map: white where the masked images agree (masked-out pixels), red-ish where the ground truth is brighter
    off = batch["msk"] == 0
    assert torch.equal(images["err_map"][off], torch.ones_like(images["err_map"][off]))


# ---- the numpy SSIM restatement --------------------------------------------------------------------------------------------------
def test_ssim_numpy_identical_images_is_one():
    g = np.random.default_rng(0)
    x = g.random((2, 3, 23, 31), dtype=np.float64).astype(np.float32)
    assert ssim_numpy(x, x, _window()) == 1.0


def test_ssim_numpy_constant_offset_closed_form():
    """target = preds + c: the variances and the covariance are equal, so the structure term is exactly 1 and SSIM reduces to the
    luminance term (2 mu (mu + c) + C1) / (mu^2 + (mu + c)^2 + C1) -- mu from a direct 11x11 window sum here."""
    rng = np.random.default_rng(1)
    x = rng.random((1, 1, 17, 19)).astype(np.float64)
    c = 0.25
    w = _window().astype(np.float64)
    w = w / w.sum()           # taps that sum to 1 in float64: the float32 taps miss by ~1e-8, which leaks c into the variance
    k2 = np.outer(w, w)
    R = float(x.max() - x.min())
    c1 = (0.01 * R) ** 2
    vals = []
    for i in range(17 - 10):
        for j in range(19 - 10):
            mu = float((x[0, 0, i:i + 11, j:j + 11] * k2).sum())
            vals.append((2 * mu * (mu + c) + c1) / (mu ** 2 + (mu + c) ** 2 + c1))
    assert ssim_numpy(x, x + c, w) == pytest.approx(float(np.mean(vals)), rel=1e-12, abs=1e-12)


@pytest.mark.parametrize("mode", ["constant", "edge", "symmetric", "wrap"])
def test_ssim_numpy_independent_of_padding(mode):
    rng = np.random.default_rng(2)
    p = rng.random((2, 3, 20, 26)).astype(np.float32)
    t = np.clip(p + 0.1 * rng.standard_normal(p.shape), 0, 1).astype(np.float32)
    assert ssim_numpy(p, t, _window(), pad_mode=mode) == pytest.approx(ssim_numpy(p, t, _window(), "reflect"), rel=0, abs=1e-15)
