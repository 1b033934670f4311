"""The weighted pixel draw without a GPU: the numpy twin (tests/pixel_draw_ref.py) enumerated over every position of small tables,
``PixelSampling``'s validation, the composer's host side over an injected twin backend (zero totals, ``indices_host``, nothing new
with ``sampling=None``), the C-ABI surface and the library's argument checks, which precede any device work."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import pixel_draw_ref as pr
from tests.test_compose_cpu import _cams
from tests.test_host_cpu import _exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lse_pixel_rows_build", "lse_pixel_draw")


# ---------------------------------------------------------------------------------------------------- the twin, exhaustively
def _tables():
    rng = np.random.default_rng(5)
    out = {}
    out["one pixel"] = np.array([[[3]]])
    out["dense"] = rng.integers(1, 10, (2, 3, 7))
    w = rng.integers(0, 4, (3, 4, 9))
    w[0, :2] = 0                      # zero rows at the start ...
    w[1, 1:3] = 0                     # ... in the middle ...
    w[2, 2:] = 0                      # ... and at the end
    out["zero rows"] = w
    w = rng.integers(1, 6, (2, 5, 11))
    w[:, :, :3] = 0                   # zero pixels at both row ends
    w[:, :, -4:] = 0
    w[1, 2, 3:7] = 0                  # ... and a row whose one drawable pixel sits between two runs of zeros
    w[1, 2, 5] = 7
    out["zero row ends"] = w
    w = np.zeros((4, 3, 70), np.int64)
    w[3, 1, 69] = 1
    w[0, 2, 64] = 255
    w[2, 0, 63] = 2
    out["lonely pixels"] = w
    w = rng.integers(0, 2, (5, 13, 5)) * rng.integers(0, 16, (5, 13, 5))
    w[::2] = 0                        # whole images of zero weight
    out["zero images"] = w
    return {k: np.asarray(v, np.int64) for k, v in out.items()}


@pytest.mark.parametrize("name", sorted(_tables()))
def test_every_position_hits_each_pixel_exactly_its_weight(name):
    w = _tables()[name]
    row_off = pr.row_table(w)
    total = int(row_off[-1])
    assert 0 < total == int(w.sum()) <= 5000 and row_off.dtype == np.int64 and len(row_off) == w.shape[0] * w.shape[1] + 1
    hits = np.zeros_like(w).reshape(-1, w.shape[-1])
    last = (-1, -1)
    for t in range(total):
        r, x, wt = pr.pick(w, row_off, t)
        assert wt == w.reshape(-1, w.shape[-1])[r, x] > 0
        assert (r, x) >= last                                   # positions walk the pixels in row-major order
        last = (r, x)
        hits[r, x] += 1
    assert np.array_equal(hits.reshape(w.shape), w)             # each pixel w times, zero-weight pixels never


def test_mulhi64_and_the_positions_are_exact_and_in_range():
    assert pr.mulhi64(2 ** 64 - 1, 2 ** 62) == 2 ** 62 - 1 and pr.mulhi64(2 ** 63, 7) == 3 and pr.mulhi64(12345, 1) == 0
    big = 4112 * 4112 * 255
    assert big > 2 ** 32
    t = pr.positions(seed=2 ** 40 + 7, step=3, stream_id=1, n=500, total=big)
    assert all(0 <= v < big for v in t) and max(t) > 2 ** 32 and len(set(t)) == 500
    assert t == pr.positions(2 ** 40 + 7, 2 ** 32 + 3, 1, 500, big)                 # the low 32 bits of the step enter the counter
    assert t != pr.positions(2 ** 40 + 7, 3, 0, 500, big) and t != pr.positions(2 ** 40 + 8, 3, 1, 500, big)
    for total in range(2, 8):                                                        # both ends of a tiny total occur within a few steps
        seen = {v for s in range(8) for v in pr.positions(1, s, 1, 8, total)}
        assert seen == set(range(total)), (total, seen)


def test_weights_follow_the_float_comparison():
    img = np.array([[[0.0, -0.0, 1e-30, -3.0, np.nan]]], np.float32)
    msk = np.array([[[1.0, 1.0, -0.0, 0.5, 1.0]]], np.float32)
    assert pr.pixel_weights(img, None, 9, 2).tolist() == [[[2, 2, 9, 9, 9]]]       # -0.0 is idle, NaN is active
    assert pr.pixel_weights(img, msk, 9, 2).tolist() == [[[2, 2, 0, 9, 9]]]        # a mask of -0.0 masks
    assert pr.pixel_weights(np.array([[[0, -1, 127]]], np.int8), None, 5, 0).tolist() == [[[0, 5, 5]]]
    assert pr.pixel_weights((1, 1, 3), np.array([[[1, 0, 2]]], np.uint8), 1, 1).tolist() == [[[1, 0, 1]]]


# ---------------------------------------------------------------------------------------------------- PixelSampling
def test_pixel_sampling_validation():
    from lsenerf_amd.data import PixelSampling
    s = PixelSampling()
    assert (s.respect_mask, s.evs_active_weight, s.evs_idle_weight) == (True, 1, 1)
    s = PixelSampling(respect_mask=False, evs_active_weight=255, evs_idle_weight=0)
    assert (s.respect_mask, s.evs_active_weight, s.evs_idle_weight) == (False, 255, 0)
    assert PixelSampling(evs_active_weight=np.int64(9)).evs_active_weight == 9
    for kw in ({"evs_active_weight": -1}, {"evs_idle_weight": 256}, {"evs_active_weight": 1.5}, {"evs_idle_weight": "3"},
               {"evs_active_weight": True}, {"evs_active_weight": None}):
        with pytest.raises(ValueError, match=r"integer in \[0, 255\]"):
            PixelSampling(**kw)
    with pytest.raises(ValueError, match="both zero"):
        PixelSampling(evs_active_weight=0, evs_idle_weight=0)
    assert "-0.0" in PixelSampling.__doc__ and "net 0" in PixelSampling.__doc__ and "objective" in PixelSampling.__doc__.lower()


# ---------------------------------------------------------------------------------------------------- the composer's host side
COL_HW, EVS_HW, N_COL, N_FRAMES = (7, 9), (6, 11), 3, 4


def small_scene(device, seed=0, masks=True, frames_dtype=np.int8, active=0.3):
    """A two-stream scene with masks (colour: bool, events: float32) and sparse event frames; also the numpy arrays."""
    from lsenerf_amd.data import DeviceScene
    rng = np.random.default_rng(seed)
    col_img = rng.integers(0, 256, (N_COL,) + COL_HW + (3,), dtype=np.uint8)
    frames = (rng.integers(1, 6, (N_FRAMES,) + EVS_HW) * rng.choice([-1, 1], (N_FRAMES,) + EVS_HW)
              * (rng.random((N_FRAMES,) + EVS_HW) < active)).astype(frames_dtype)
    col_msk = rng.random((N_COL,) + COL_HW) < 0.6 if masks else None
    evs_msk = (rng.random((N_FRAMES,) + EVS_HW) < 0.6).astype(np.float32) if masks else None
    if masks:
        col_msk[:, 0], col_msk[1], evs_msk[:, :, -3:], evs_msk[0] = False, False, 0.0, 0.0     # a border, a whole image
    scene = DeviceScene.from_arrays(
        device, col_images=col_img, col_cameras=_cams(N_COL, COL_HW, 2, [0.0, 1.0, 2.0], 31.0), col_appearance_ids=[0, 1, 2],
        col_msk=col_msk, evs_frames=frames, evs_cameras=_cams(N_FRAMES + 1, EVS_HW, 5, [0.5, 1.5, 2.5, 3.5, 4.5], 27.0),
        evs_appearance_ids=[0, 1, 2, 0], evs_msk=evs_msk, e_thresh=0.25, rgb_times=torch.tensor([0.0, 1.0, 2.0]))
    return scene, dict(col_img=col_img, frames=frames, col_msk=col_msk, evs_msk=evs_msk)


def scene_weights(arrays, sampling):
    """The twin's weights of both streams of a ``small_scene`` under a ``PixelSampling``."""
    use = sampling.respect_mask
    col = pr.pixel_weights(arrays["col_img"].shape[:3], arrays["col_msk"] if use else None, 1, 1)
    evs = pr.pixel_weights(arrays["frames"], arrays["evs_msk"] if use else None, sampling.evs_active_weight, sampling.evs_idle_weight)
    return col, evs


@pytest.fixture
def twin_backend(monkeypatch):
    """``ops.pixel_rows_build`` on CPU tensors through the numpy twin: the composer's set-up without a device."""
    from lsenerf_amd import ops
    calls = []

    def rows_build(images, msk, shape, w_active, w_idle, row_off=None):
        img = tuple(shape) if images is None else images.numpy()
        w = pr.pixel_weights(img, None if msk is None else msk.numpy(), w_active, w_idle)
        row_off.copy_(torch.from_numpy(pr.row_table(w)))
        calls.append((images is not None, msk is not None, tuple(shape), w_active, w_idle))
        return row_off
    monkeypatch.setattr(ops, "pixel_rows_build", rows_build)
    return calls


def test_a_composer_without_sampling_has_nothing_new(twin_backend):
    from lsenerf_amd.data import BatchComposer, PixelSampling
    scene, _ = small_scene("cpu")
    plain = BatchComposer(scene, 5, 4, seed=3)
    assert plain.sampling is None and plain.draw_weights is None and plain.sampling_totals is None and plain._weighted == (None, None)
    assert not twin_backend                                                          # nothing was built
    with pytest.raises(ValueError, match="sampling=None"):
        plain.rebuild_sampling()
    with pytest.raises(ValueError, match="PixelSampling"):
        BatchComposer(scene, 5, 4, sampling={"evs_active_weight": 9})
    weighted = BatchComposer(scene, 5, 4, seed=3, sampling=PixelSampling())

    def tensors(c):
        found = {}
        for k, v in vars(c).items():
            for t in (v if isinstance(v, (tuple, list)) else v.values() if isinstance(v, dict) else [v]):
                if torch.is_tensor(t):
                    found.setdefault(k, []).append(tuple(t.shape))
        return found
    assert tensors(weighted).keys() - tensors(plain).keys() == {"draw_weights"}     # (the tables live inside _weighted)
    assert {k: v for k, v in tensors(weighted).items() if k != "draw_weights"} == tensors(plain)
    # the uniform convention is the one of tests/test_compose_cpu.py, for both
    from lsenerf_amd.data import draw_indices_host
    want = draw_indices_host(3, 7, 1, 4, N_FRAMES, *EVS_HW)
    assert np.array_equal(plain.indices_host(7)[1], want)


def test_draw_indices_host_is_untouched():
    """Values recorded from the uniform draw as it was before weighted sampling existed."""
    from lsenerf_amd.data import draw_indices_host
    got = draw_indices_host(2 ** 40 + 7, 11, 1, 4, 9, 18, 24)
    ctr = np.array([[11, i, 1, 0] for i in range(4)], np.uint32)
    from lsenerf_amd.data import philox4x32_10
    w = philox4x32_10(ctr, (7, 256)).astype(np.uint64)
    assert np.array_equal(got, np.stack([(w[:, 0] * 9) >> 32, (w[:, 1] * 18) >> 32, (w[:, 2] * 24) >> 32], 1).astype(np.int64))
    assert got.tolist() == [[5, 12, 15], [7, 1, 11], [6, 6, 9], [3, 5, 1]]


def test_totals_tables_and_the_zero_total_error(twin_backend):
    from lsenerf_amd.data import BatchComposer, PixelSampling
    scene, arrays = small_scene("cpu")
    s = PixelSampling(evs_active_weight=9, evs_idle_weight=1)
    comp = BatchComposer(scene, 5, 4, seed=3, sampling=s)
    w_col, w_evs = scene_weights(arrays, s)
    assert comp.sampling_totals == (int(w_col.sum()), int(w_evs.sum())) and all(isinstance(v, int) for v in comp.sampling_totals)
    assert twin_backend == [(False, True, (N_COL,) + COL_HW, 1, 1), (True, True, (N_FRAMES,) + EVS_HW, 9, 1)]
    assert [tuple(t.shape) for t in comp.draw_weights] == [(5,), (4,)] and all(t.dtype == torch.int32 for t in comp.draw_weights)
    assert "draw_weights" not in comp.batch["col_batch"] and "draw_weights" not in comp.batch["evs_batch"]
    # respect_mask=False: the masks do not reach the tables
    free = BatchComposer(scene, 5, 4, sampling=PixelSampling(respect_mask=False, evs_active_weight=0))
    assert twin_backend[-2:] == [(False, False, (N_COL,) + COL_HW, 1, 1), (True, False, (N_FRAMES,) + EVS_HW, 0, 1)]
    assert free.sampling_totals == (N_COL * COL_HW[0] * COL_HW[1], int((arrays["frames"] == 0).sum()))
    # a stream nothing can be drawn from is refused at construction, and again by rebuild_sampling
    scene.evs.msk.zero_()
    with pytest.raises(ValueError, match="event stream has a total weight of 0"):
        BatchComposer(scene, 5, 4, sampling=s)
    with pytest.raises(ValueError, match="event stream has a total weight of 0"):
        comp.rebuild_sampling()
    BatchComposer(scene, 5, 4, sampling=PixelSampling(respect_mask=False))           # ... unless the mask is not respected
    scene2, _ = small_scene("cpu", seed=1)
    scene2.col.msk.zero_()
    with pytest.raises(ValueError, match="colour stream has a total weight of 0"):
        BatchComposer(scene2, 5, 4, sampling=PixelSampling())
    scene3, _ = small_scene("cpu", seed=2, masks=False, active=0.0)                  # no event anywhere, and idle pixels weigh nothing
    with pytest.raises(ValueError, match="event stream has a total weight of 0"):
        BatchComposer(scene3, 5, 4, sampling=PixelSampling(evs_idle_weight=0))
    # after an edit in place, rebuild_sampling follows the data
    scene4, arrays4 = small_scene("cpu", seed=4)
    c4 = BatchComposer(scene4, 5, 4, sampling=s)
    scene4.evs.images[1] = 0
    arrays4["frames"][1] = 0
    assert c4.rebuild_sampling() == c4.sampling_totals == tuple(int(w.sum()) for w in scene_weights(arrays4, s))


@pytest.mark.parametrize("kw", [dict(evs_active_weight=9, evs_idle_weight=1), dict(evs_idle_weight=0), dict(respect_mask=False)])
def test_indices_host_is_the_twins_draw(twin_backend, kw):
    from lsenerf_amd.data import BatchComposer, PixelSampling
    scene, arrays = small_scene("cpu")
    s = PixelSampling(**kw)
    comp = BatchComposer(scene, 65, 63, seed=2 ** 40 + 7, sampling=s)
    w_col, w_evs = scene_weights(arrays, s)
    for step in (0, 5, 2 ** 32 + 5):
        col, evs = comp.indices_host(step)
        assert col.dtype == evs.dtype == np.int64
        assert np.array_equal(col, pr.draw(w_col, comp.seed, step, 0, 65)[0])
        assert np.array_equal(evs, pr.draw(w_evs, comp.seed, step, 1, 63)[0])
        assert (w_col[tuple(col.T)] > 0).all() and (w_evs[tuple(evs.T)] > 0).all()
    assert np.array_equal(comp.indices_host(5)[1], comp.indices_host(2 ** 32 + 5)[1])
    assert not np.array_equal(comp.indices_host(0)[1], comp.indices_host(5)[1])


def test_ops_refuse_bad_arguments_before_the_library(monkeypatch):
    from lsenerf_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", no_library)
    img, row_off = torch.zeros(2, 3, 4, dtype=torch.int8), torch.zeros(7, dtype=torch.int64)
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.pixel_rows_build(img, None, (2, 3, 4), 9, 1)
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.pixel_draw(None, None, (2, 3, 4), 1, 1, row_off, 0, 0, 5, step=0)
    for wa, wi in ((256, 1), (-1, 1), (0, 0), (1.0, 1), (True, 1)):
        with pytest.raises(ValueError, match="not both zero"):
            ops.pixel_rows_build(img, None, (2, 3, 4), wa, wi)
    with pytest.raises(ValueError, match="w_active must equal w_idle"):
        ops.pixel_rows_build(None, None, (2, 3, 4), 9, 1, row_off=row_off)
    with pytest.raises(ValueError, match="at least 1"):
        ops.pixel_rows_build(img, None, (2, 0, 4), 9, 1)
    with pytest.raises(ValueError, match="expected, got"):
        ops.pixel_rows_build(img.double(), None, (2, 3, 4), 9, 1)
    with pytest.raises(ValueError, match="give step or step_dev"):
        ops.pixel_draw(None, None, (2, 3, 4), 1, 1, row_off, 0, 0, 5)
    with pytest.raises(ValueError, match="step number"):
        ops.pixel_draw(None, None, (2, 3, 4), 1, 1, row_off, 0, 0, 5, step=-1)
    with pytest.raises(ValueError, match="n < 0"):
        ops.pixel_draw(None, None, (2, 3, 4), 1, 1, row_off, 0, 0, -5, step=0)
    with pytest.raises(ValueError, match="stream_id"):
        ops.pixel_draw(None, None, (2, 3, 4), 1, 1, row_off, 0, 2, 5, step=0)
    with pytest.raises(ValueError, match="seed"):
        ops.pixel_draw(None, None, (2, 3, 4), 1, 1, row_off, 2 ** 64, 0, 5, step=0)


# ---------------------------------------------------------------------------------------------------- the C-ABI
def test_header_libraries_and_binding_carry_the_entry_points():
    from lsenerf_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    shipped, dev = _exported(_lib.LIB_PATH), _exported(_lib.DEV_LIB_PATH)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        assert m, f"{name} is not declared"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name]) == len([a for a in m.group(1).split(",") if a.strip()]), name
        assert name in shipped and name in dev and hasattr(lib, name), name
    assert _lib.SIGNATURES["lse_pixel_draw"][10] is ctypes.c_uint64 and _lib.SIGNATURES["lse_pixel_draw"][13] is ctypes.c_int64
    assert lib.lse_abi_version() == _lib.LSE_ABI_VERSION == 6                         # additive: the number stays
    assert "#define LSE_ABI_VERSION 6" in open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    mk = open(os.path.join(ROOT, "lsenerf_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS = .*\bpixel_draw\b", mk, flags=re.M)


def test_the_library_refuses_bad_arguments_before_any_launch():
    """The host-side checks of csrc/pixel_draw.hip return LSE_E_INVALID without touching a device: callable without a GPU."""
    from lsenerf_amd import _lib
    fake, fake2, odd = ctypes.c_void_p(4096), ctypes.c_void_p(8192), ctypes.c_void_p(4100)     # never dereferenced
    U8, F32, I8, NONE = _lib.LSE_PIX_U8, _lib.LSE_PIX_F32, _lib.LSE_PIX_I8, _lib.LSE_PIX_NONE

    def build(images=fake, pix=I8, msk=fake2, mt=U8, n=2, H=3, W=70, wa=9, wi=1, row_off=fake):
        _lib.call("lse_pixel_rows_build", images, pix, msk, mt, n, H, W, wa, wi, row_off, None)

    def draw(images=fake, pix=I8, msk=fake2, mt=U8, n_img=2, H=3, W=70, wa=9, wi=1, row_off=fake, seed=0, sid=1, step_dev=None,
             step=0, n=5, idx=fake, wt=fake2):
        _lib.call("lse_pixel_draw", images, pix, msk, mt, n_img, H, W, wa, wi, row_off, seed, sid, step_dev, step, n, idx, wt, None)
    for fn, what in ((build, "lse_pixel_rows_build"), (draw, "lse_pixel_draw")):
        for pix in (-1, 5, 17):
            with pytest.raises(_lib.LseHipError, match=f"{what}: pix_type {pix}"):
                fn(pix=pix)
        for mt in (NONE, I8, 2, 3, 9):
            with pytest.raises(_lib.LseHipError, match=f"{what}: msk_type {mt}"):
                fn(mt=mt)
        with pytest.raises(_lib.LseHipError, match="without a mask"):
            fn(msk=None, mt=U8)
        for kw in ({"n": 0} if fn is build else {"n_img": 0}, {"H": 0}, {"W": -1}):
            with pytest.raises(_lib.LseHipError, match="must be >= 1"):
                fn(**kw)
        with pytest.raises(_lib.LseHipError, match=r"2147483648 image rows exceed the supported 2147483647"):
            fn(**({"n": 65536} if fn is build else {"n_img": 65536}), H=32768)
        with pytest.raises(_lib.LseHipError, match="a row sum must fit 32 bits"):
            fn(W=(2 ** 31 - 1) // 255 + 1)
        for wa, wi in ((256, 1), (1, 256), (-1, 1), (1, -1)):
            with pytest.raises(_lib.LseHipError, match=r"outside \[0, 255\]"):
                fn(wa=wa, wi=wi)
        with pytest.raises(_lib.LseHipError, match="both weights are zero"):
            fn(wa=0, wi=0)
        with pytest.raises(_lib.LseHipError, match="w_active must equal w_idle"):
            fn(images=None)
        for bad in (None, odd):
            with pytest.raises(_lib.LseHipError, match="row_off must be"):
                fn(row_off=bad)
    with pytest.raises(_lib.LseHipError, match="n < 0"):
        draw(n=-1)
    with pytest.raises(_lib.LseHipError, match="stream_id 2"):
        draw(sid=2)
    with pytest.raises(_lib.LseHipError, match="negative step without step_dev"):
        draw(step=-1)
    for kw in ({"idx": None}, {"wt": None}):
        with pytest.raises(_lib.LseHipError, match="null output"):
            draw(**kw)
    draw(n=0, row_off=None, idx=None, wt=None)           # nothing to draw: no launch, whatever the pointers
    with pytest.raises(_lib.LseHipError, match="n < 0"):
        draw(n=-1, step_dev=fake, step=-1)               # (a step_dev excuses the step, nothing else)
