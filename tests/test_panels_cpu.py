"""CPU tests of the eval panels: the numpy twin (tests/panels_ref.py) against hand-checked facts about Canny's classification, its
two hysteresis formulations against each other, and the host side of the new entry points (header, binding, library, config
default, CPU tensors refused).  The kernels themselves are held against the twin in tests/test_gpu_panels.py."""
import os
import re

import numpy as np
import pytest
import torch

from tests import panels_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lse_gray8_planes", "lse_canny_workspace", "lse_canny_classify", "lse_canny_hysteresis", "lse_canny_u8",
               "lse_eval_panels_workspace", "lse_eval_panels")
SIZES = [(1, 1), (3, 3), (5, 7), (37, 53), (64, 96), (97, 130)]


def test_vertical_step_gives_one_edge_column_on_the_dark_side():
    img = ref.step_image(9, 12, vertical=True, at=6)               # columns 0..5 dark, 6..11 bright
    _, _, mag = ref.sobel_mag(img)
    assert (mag[:, 5] == 1020).all() and (mag[:, 6] == 1020).all() and (mag[:, :5] == 0).all() and (mag[:, 7:] == 0).all()
    cls = ref.canny_classify(img)
    want = np.zeros((9, 12), dtype=np.uint8)
    want[:, 5] = 2                                                 # m > mag[left] and m >= mag[right]: the left of the tie wins
    assert (cls == want).all()
    assert (ref.hysteresis_flood(cls) == want // 2 * 255).all()


def test_horizontal_step_gives_the_row_above():
    img = ref.step_image(9, 12, vertical=False, at=4)              # rows 0..3 dark
    cls = ref.canny_classify(img)
    want = np.zeros((9, 12), dtype=np.uint8)
    want[3, :] = 2
    assert (cls == want).all()


def test_constant_image_and_low_steps():
    assert not ref.canny_classify(np.full((9, 12), 200, dtype=np.uint8)).any()
    lo = ref.step_image(9, 12, height=12, at=6)
    assert ref.sobel_mag(lo)[2].max() == 48 and not ref.canny_classify(lo).any()          # 48 <= 50: no candidate
    weak = ref.step_image(9, 12, height=13, at=6)
    cls = ref.canny_classify(weak)
    assert ref.sobel_mag(weak)[2].max() == 52 and set(np.unique(cls)) == {0, 1} and (cls[:, 5] == 1).all()
    assert not ref.hysteresis_flood(cls).any() and not ref.hysteresis_label(cls).any()   # weak only: no edge


def test_border_magnitude_uses_the_replicated_border():
    # a step in the first column only: with a replicated border dx at column 0 sees (col 1 - col 0) * 4, with a zero border it
    # would see col 1 * 4; and the corner rows replicate too, so the whole column has one magnitude
    img = np.full((5, 7), 100, dtype=np.uint8)
    img[:, 0] = 40
    dx, dy, mag = ref.sobel_mag(img)
    assert (dx[:, 0] == 240).all() and (dx[:, 1] == 240).all() and (dy == 0).all() and (mag[:, 2:] == 0).all()
    cls = ref.canny_classify(img)
    assert (cls[:, 0] == 2).all() and not cls[:, 1:].any()         # mag[left of column 0] is 0 outside the image
    # a single bright pixel in a corner: replicated rows and columns weigh it 1 + 2 = 3 times
    img = np.zeros((5, 7), dtype=np.uint8)
    img[0, 0] = 90
    dx, dy, _ = ref.sobel_mag(img)
    assert dx[0, 0] == -270 and dy[0, 0] == -270 and dx[0, 1] == -270 and dx[1, 1] == -90


@pytest.mark.parametrize("hw", SIZES)
def test_the_two_hysteresis_formulations_agree(hw):
    H, W = hw
    maps = ref.hysteresis_fixtures(H, W) + [(n, ref.canny_classify(img)) for n, img in ref.classify_fixtures(H, W)]
    for name, cls in maps:
        assert (ref.hysteresis_flood(cls) == ref.hysteresis_label(cls)).all(), name


def test_hysteresis_fixtures_are_what_they_claim():
    H, W = 97, 130
    m, n = ref.spiral_map(H, W)
    assert n > 2000 and (m == 2).sum() == 1 and (m > 0).sum() == n
    ys, xs = np.nonzero(m)
    assert {(y // ref.TILE, x // ref.TILE) for y, x in zip(ys, xs)} == {(a, b) for a in range(4) for b in range(5)}      # every tile
    assert (ref.hysteresis_flood(m) == (m > 0) * 255).all()                        # all of it is an edge
    assert not ref.hysteresis_flood(ref.spiral_map(H, W, seeded=False)[0]).any()
    m, want = ref.corner_blobs_map(H, W)
    assert m[ref.TILE - 1, ref.TILE - 1] == 1 and m[ref.TILE, ref.TILE] == 1 and not m[ref.TILE - 1, ref.TILE] and not m[ref.TILE, ref.TILE - 1]
    e = ref.hysteresis_flood(m) > 0
    assert (e == want).all() and (m > 0).sum() > want.sum()                       # the seeded pair, not the unseeded one
    assert (ref.hysteresis_flood(ref.border_map(H, W)) == (ref.border_map(H, W) > 0) * 255).all()
    big = ref.hysteresis_label(ref.random_map(H, W, 0.4))
    assert 0 < (big > 0).mean() < 0.45


@pytest.mark.parametrize("hw", [s for s in SIZES if s[0] * s[1] >= 35])
def test_classify_fixtures_take_every_branch(hw):
    counts = {}
    for _, img in ref.classify_fixtures(*hw):
        ref.canny_classify(img, branches=counts)
    assert all(counts[k] > 0 for k in ("horizontal", "vertical", "diagonal_pos", "diagonal_neg")), counts


def test_new_symbols_are_declared_bound_and_exported():
    from lsenerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.lse_abi_version() == _lib.LSE_ABI_VERSION == 6
    assert (_lib.LSE_PANEL_IMG, _lib.LSE_PANEL_DEPTH, _lib.LSE_PANEL_ERR_MAP, _lib.LSE_PANEL_OVERLAY, _lib.LSE_PANEL_EV_OUT) == (1, 2, 4, 8, 16)
    for flag in ("IMG 1", "DEPTH 2", "ERR_MAP 4", "OVERLAY 8", "EV_OUT 16"):
        assert "#define LSE_PANEL_" + flag in hdr


def test_workspace_sizes_and_invalid_arguments_without_gpu():
    import ctypes
    from lsenerf_amd import _lib, ops
    assert ops.canny_workspace_bytes(97, 130) == (97 * 130 * 4 + 7) // 8 * 8
    assert ops.canny_workspace_bytes(3, 3, 2) == 2 * 40 and ops.eval_panels_workspace_bytes(24, 40) % 8 == 0
    lib = _lib.load()
    v = ctypes.c_int64(0)
    assert lib.lse_canny_workspace(0, 5, ctypes.byref(v)) == -1 and b"H and W" in lib.lse_last_error()
    assert lib.lse_canny_u8(None, 1, 4, 4, 50, 200, None, 0, None, None) == -1 and b"null" in lib.lse_last_error()
    assert lib.lse_eval_panels(None, None, None, None, None, None, None, None, None, 0, 4, 4, 0, None, 0, None, None) == -1
    assert lib.lse_eval_panels(None, None, None, None, None, None, None, None, None, 0, 4, 4, 64, None, 0, None, None) == -1
    assert ops.panel_columns(("overlay", "img")) == 3 and ops.panel_columns(ops.PANEL_KEYS) == 6 == ref.panel_columns(ref.PANEL_KEYS)


def test_cpu_tensors_are_refused():
    from lsenerf_amd import _lib, ops
    g = torch.zeros((5, 7), dtype=torch.uint8)
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.canny_edges(g)
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.canny_classify(g)
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.canny_hysteresis(g)
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.gray8_planes(torch.zeros((3, 5, 7)))
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.eval_panels(("overlay",), 5, 7, edges=torch.zeros((2, 5, 7), dtype=torch.uint8))


def test_overlay_is_opt_in_and_the_default_dictionary_is_unchanged():
    from lsenerf_amd import LSENeRFModelConfig
    from lsenerf_amd import eval_set as es
    assert LSENeRFModelConfig().eval_overlay is False
    H, W = 4, 6
    out = {"rgb": torch.rand(H, W, 3), "accumulation": torch.rand(H, W, 1), "depth": torch.rand(H, W, 1)}
    gt, pr = torch.rand(1, 3, H, W), torch.rand(1, 3, H, W)
    assert list(es._image_dict(out, gt, pr)) == ["img", "accumulation", "depth", "err_map"]
    out["ev_out"] = torch.rand(H, W, 1)
    assert list(es._image_dict(out, gt, pr)) == ["img", "accumulation", "depth", "err_map", "ev_out"]
    marker = torch.zeros(H, W, 3)
    assert list(es._image_dict(out, gt, pr, overlay=marker)) == ["img", "accumulation", "depth", "err_map", "overlay", "ev_out"]
    with pytest.raises(ValueError, match="subset"):
        es.PanelSet.__init__(es.PanelSet.__new__(es.PanelSet), None, keys=("accumulation",))


def test_twin_panels_layout_and_rounding():
    H, W = 3, 4
    rng = np.random.default_rng(3)
    gt, pr = rng.random((3, H, W), dtype=np.float32), rng.random((3, H, W), dtype=np.float32)
    rgb = rng.random((H * W, 3), dtype=np.float32)
    edges = np.zeros((2, H, W), dtype=np.uint8)
    edges[0, 0, 0] = edges[1, 0, 1] = edges[0, 1, 1] = edges[1, 1, 1] = 255
    depth = np.full((H, W, 1), 2.5, dtype=np.float32)                             # far == near: d = 0 everywhere, no NaN
    acc = np.full((H, W, 1), 0.25, dtype=np.float32)
    g = ref.panels(ref.PANEL_KEYS, gt_planes=gt, pred_planes=pr, rgb=rgb, depth=depth, acc=acc, edges=edges,
                   ev_out=np.full((H, W, 1), np.nan, dtype=np.float32))
    assert g.shape == (H, 6 * W, 3) and g.dtype == np.uint8
    assert (g[:, :W] == (np.moveaxis(gt, 0, -1) * np.float32(255)).astype(np.uint8)).all()
    assert (g[:, 2 * W:3 * W] == 255).all()                                       # (1 - 0) * acc + (1 - acc) = 1
    ov = g[:, 4 * W:5 * W]
    assert tuple(ov[0, 0]) == (255, 0, 0) and tuple(ov[0, 1]) == (0, 0, 255) and tuple(ov[1, 1]) == (255, 0, 255) and tuple(ov[2, 2]) == (255,) * 3
    assert (g[:, 5 * W:] == 0).all()                                              # a NaN gives 0
    assert ref.to_u8(np.float32([-1, 0.5, 1.0, 2.0, 254.999 / 255])).tolist() == [0, 127, 255, 255, 254]
