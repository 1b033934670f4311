"""Early ray termination of the eval render, the parts that need no GPU: the segment schedule, the two config fields and their
validation, the four C-ABI entry points (declared, bound, exported, arguments refused before any launch), and the float64 numpy
restatement of "composite the first m samples" / of the termination rule that tests/test_gpu_eval_early_stop.py imports."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSE_E_INVALID = -1
ENTRY_POINTS = ("lse_eval_segment_state_bytes", "lse_eval_segment_begin", "lse_eval_composite_segment", "lse_eval_composite_finish")
STATE_BYTES_PER_RAY = (5 * 64 + 8) * 4


# ----------------------------------------------------------------------------------------------------
# float64 restatement (imported by the GPU tests)
# ----------------------------------------------------------------------------------------------------
def schedule_boundaries(cap: int, base: int):
    """Sample counts at which a segment of ``segment_schedule(cap, base)`` ends: the only places a ray may stop short."""
    from lsenerf_amd.evaluation import segment_schedule
    return [off + length for off, length in segment_schedule(cap, base)]


def tau_prefix64(ts, te, sigma) -> np.ndarray:
    """tau[m] = optical depth of the first m samples of one ray, in float64 (tau[0] = 0); a sample of infinite density gives inf."""
    sd = np.asarray(sigma, dtype=np.float64) * (np.asarray(te, dtype=np.float64) - np.asarray(ts, dtype=np.float64))
    return np.concatenate([[0.0], np.cumsum(sd)])


def stop_count_numpy(tau: np.ndarray, boundaries, tau_stop: float) -> int:
    """The termination rule: a ray of n = len(tau) - 1 samples is composited up to the first segment boundary b < n at which its
    optical depth tau[b] has reached ``tau_stop``, else in full."""
    n = len(tau) - 1
    for b in boundaries:
        if b >= n:
            break
        if tau[b] >= tau_stop:
            return b
    return n


def composite_first_m_numpy(ts, te, sigma, rgb, m: int, nan_to_num: bool = False):
    """(rgb[3], accumulation, depth numerator, smallest mid-point, largest mid-point) of the first ``m`` samples of one ray in
    float64: w_k = exp(-tau[k]) * (1 - exp(-sigma_k dt_k)), sums of w, w * colour, w * mid-point.  Before the renderer epilogue."""
    ts, te = np.asarray(ts, dtype=np.float64)[:m], np.asarray(te, dtype=np.float64)[:m]
    sg = np.asarray(sigma, dtype=np.float64)[:m]
    c = np.asarray(rgb, dtype=np.float64)[:m, :3]
    if nan_to_num:
        c = np.nan_to_num(c, nan=0.0, posinf=float(np.finfo(np.float32).max), neginf=-float(np.finfo(np.float32).max))
    if m == 0:
        return np.zeros(3), 0.0, 0.0, math.inf, -math.inf
    sd = sg * (te - ts)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.exp(-tau_prefix64(ts, te, sg)[:m]) * (1.0 - np.exp(-sd))
    mid = (ts + te) * 0.5
    return (w[:, None] * c).sum(0), float(w.sum()), float((w * mid).sum()), float(mid.min()), float(mid.max())


# ----------------------------------------------------------------------------------------------------
# the schedule
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [1, 63, 64, 65, 128, 129, 1136, 1568, 8040])
@pytest.mark.parametrize("base", [64, 128, 256])
def test_segment_schedule(cap, base):
    from lsenerf_amd.evaluation import segment_schedule
    sched = segment_schedule(cap, base)
    lengths = [length for _, length in sched]
    assert all(length > 0 for length in lengths) and sum(lengths) == cap
    off = 0
    for o, length in sched:                      # contiguous, every offset a multiple of 64
        assert o == off and o % 64 == 0
        off += length
    want = [base, base] + [base << k for k in range(1, 40)]           # S, S, 2S, 4S, ...
    assert lengths[:-1] == want[:len(lengths) - 1]                     # ... every segment but the last is a full one
    assert 0 < lengths[-1] <= want[len(lengths) - 1]                   # and the last is cut
    assert segment_schedule(cap, base) == sched                        # a pure function of (cap, S)


@pytest.mark.parametrize("cap,base", [(0, 64), (-3, 64), (100, 0), (100, -64), (100, 32), (100, 96), (100, 100)])
def test_segment_schedule_refuses_bad_arguments(cap, base):
    from lsenerf_amd.evaluation import segment_schedule
    with pytest.raises(ValueError):
        segment_schedule(cap, base)


# ----------------------------------------------------------------------------------------------------
# config and bindings
# ----------------------------------------------------------------------------------------------------
def test_config_has_the_two_fields_off_by_default():
    import lsenerf_amd as la
    cfg = la.LSENeRFModelConfig()
    assert cfg.eval_early_stop_eps == 0.0 and cfg.eval_segment_samples == 128
    cfg = la.LSENeRFModelConfig(eval_early_stop_eps=1e-4, eval_segment_samples=64)
    assert cfg.eval_early_stop_eps == 1e-4 and cfg.eval_segment_samples == 64


@pytest.mark.parametrize("kw", [dict(eval_early_stop_eps=-1e-3), dict(eval_early_stop_eps=1.0), dict(eval_early_stop_eps=2.0),
                                dict(eval_early_stop_eps=float("nan")), dict(eval_early_stop_eps=0.1, eval_segment_samples=0),
                                dict(eval_segment_samples=-64), dict(eval_early_stop_eps=0.1, eval_segment_samples=100),
                                dict(eval_segment_samples=96), dict(eval_early_stop_eps=0.1, eval_segment_samples=64.5)])
def test_bad_values_raise_before_anything_touches_a_device(kw):
    """Validated at render time, on the host: the model and the bundle live on the CPU here, where any launch would fail with the
    library's own error instead."""
    import lsenerf_amd as la
    from lsenerf_amd.evaluation import early_stop_settings
    cfg = la.LSENeRFModelConfig(grid_levels=1, grid_resolution=8, num_levels=2, log2_hashmap_size=4, **kw)
    with pytest.raises(ValueError, match="eval_early_stop_eps|eval_segment_samples"):
        early_stop_settings(cfg)
    m = la.LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 2).eval()
    rb = la.RayBundle(origins=torch.zeros(4, 3), directions=torch.tensor([[0.0, 0, 1]]).repeat(4, 1),
                      camera_indices=torch.zeros(4, 1, dtype=torch.long))
    with pytest.raises(ValueError, match="eval_early_stop_eps|eval_segment_samples"):
        m.get_outputs_for_camera_ray_bundle(rb)


def test_good_values_pass_validation():
    import lsenerf_amd as la
    from lsenerf_amd import ops
    from lsenerf_amd.evaluation import early_stop_settings
    assert early_stop_settings(la.LSENeRFModelConfig()) == (0.0, 128)
    assert early_stop_settings(la.LSENeRFModelConfig(eval_early_stop_eps=0.5, eval_segment_samples=192)) == (0.5, 192)
    # tau_stop = float32(-ln eps), the logarithm in double
    for eps in (1e-4, 1e-2, 0.5):
        assert ops.eval_tau_stop(eps) == float(np.float32(-math.log(eps)))
    for eps in (0.0, 1.0, -1.0):
        with pytest.raises(ValueError):
            ops.eval_tau_stop(eps)


def test_entry_points_are_declared_bound_and_exported():
    from lsenerf_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "lse_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in include/lse_hip.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib"
        assert hasattr(lib, name), f"liblse_hip.so does not export {name}"
    assert lib.lse_abi_version() == 6 and _lib.LSE_ABI_VERSION == 6
    assert "#define LSE_ABI_VERSION 6" in hdr


def test_state_bytes():
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    for n in (0, 1, 131, 3512, 32768):
        assert ops.eval_segment_state_bytes(n) == n * STATE_BYTES_PER_RAY
    assert lib.lse_eval_segment_state_bytes(4, None) == LSE_E_INVALID
    v = ctypes.c_int64(0)
    assert lib.lse_eval_segment_state_bytes(-1, ctypes.byref(v)) == LSE_E_INVALID


def _ptr():
    """A host buffer's address, 16-byte aligned: validation never dereferences it and refuses the call before any launch."""
    buf = (ctypes.c_float * 16)()
    addr = (ctypes.addressof(buf) + 15) & ~15
    return buf, ctypes.c_void_p(addr)


def test_entry_points_refuse_bad_arguments_without_gpu():
    from lsenerf_amd import _lib
    lib = _lib.load()
    keep, p = _ptr()
    odd = ctypes.c_void_p(p.value + 4)

    beg = lib.lse_eval_segment_begin
    assert beg(None, 4, 64, None, None, None) == LSE_E_INVALID and b"lse_eval_segment_begin: null pointer" in lib.lse_last_error()
    assert beg(p, 4, 64, p, None, None) == LSE_E_INVALID and b"null pointer" in lib.lse_last_error()
    assert beg(p, -1, 64, p, p, None) == LSE_E_INVALID and b"n_rays < 0" in lib.lse_last_error()
    assert beg(p, 4, 0, p, p, None) == LSE_E_INVALID and b"first_len" in lib.lse_last_error()
    assert beg(p, 4, 64, odd, p, None) == LSE_E_INVALID and b"16-byte aligned" in lib.lse_last_error()
    assert beg(None, 0, 64, None, None, None) == 0           # zero-sized work is a no-op, not an error

    def seg(ptr=p, n=4, stride=4, flags=0, seg_end=64, next_len=64, state=p, nxt=p):
        return lib.lse_eval_composite_segment(ptr, ptr, ptr, ptr, stride, ptr, ptr, n, flags, seg_end, next_len, 9.2, state, nxt, None)
    assert seg(ptr=None) == LSE_E_INVALID and b"lse_eval_composite_segment: null pointer" in lib.lse_last_error()
    assert seg(state=None) == LSE_E_INVALID and b"null pointer" in lib.lse_last_error()
    assert seg(nxt=None) == LSE_E_INVALID and b"next_seg_cnts" in lib.lse_last_error()
    assert seg(n=-1) == LSE_E_INVALID and b"n_rays < 0" in lib.lse_last_error()
    assert seg(stride=2) == LSE_E_INVALID and b"rgb_stride" in lib.lse_last_error()
    assert seg(flags=8) == LSE_E_INVALID and b"unknown flags" in lib.lse_last_error()
    assert seg(state=odd) == LSE_E_INVALID and b"16-byte aligned" in lib.lse_last_error()
    for bad_end in (1, 63, 65, 100, 320 + 32):               # a segment follows: its offset must be a multiple of 64
        assert seg(seg_end=bad_end) == LSE_E_INVALID and b"multiple of 64" in lib.lse_last_error(), bad_end
    assert seg(seg_end=0) == LSE_E_INVALID and seg(next_len=-1) == LSE_E_INVALID
    assert seg(ptr=None, n=0, state=None, nxt=None) == 0
    assert seg(ptr=None, n=0, state=None, nxt=None, seg_end=1136, next_len=0) == 0        # the last segment may end anywhere
    assert seg(ptr=None, n=0, state=None, nxt=None, seg_end=1136, next_len=64) == LSE_E_INVALID

    fin = lib.lse_eval_composite_finish
    assert fin(None, 4, 0, 0.0, None, None, None, None, None, None) == LSE_E_INVALID
    assert b"lse_eval_composite_finish: null pointer" in lib.lse_last_error()
    assert fin(p, 4, 0, 0.0, p, p, p, p, None, None) == LSE_E_INVALID and b"null pointer" in lib.lse_last_error()
    assert fin(p, -1, 0, 0.0, p, p, p, p, p, None) == LSE_E_INVALID and b"n_rays < 0" in lib.lse_last_error()
    assert fin(p, 4, 16, 0.0, p, p, p, p, p, None) == LSE_E_INVALID and b"unknown flags" in lib.lse_last_error()
    assert fin(odd, 4, 0, 0.0, p, p, p, p, p, None) == LSE_E_INVALID and b"16-byte aligned" in lib.lse_last_error()
    assert fin(None, 0, 0, 0.0, None, None, None, None, None, None) == 0
    # the binding raises with the same text
    with pytest.raises(_lib.LseHipError, match="multiple of 64"):
        _lib.call("lse_eval_composite_segment", p, p, p, p, 4, p, p, 4, 0, 100, 64, 9.2, p, p, None)
    del keep


def test_ops_wrappers_refuse_cpu_tensors_and_bad_slot_offsets():
    from lsenerf_amd import _lib, ops
    cnts = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="segment state"):
        ops.eval_segment_begin(cnts, 64, torch.zeros(8, dtype=torch.uint8), torch.zeros(4, dtype=torch.int64))
    slots = torch.zeros(4 * 10)
    packed = torch.zeros(4, 2, dtype=torch.int64)
    for bad in (-1, 10, 11):
        with pytest.raises(ValueError, match="slot_offset"):
            ops.compact_ray_slots(slots, slots, 10, packed, torch.zeros(4, dtype=torch.int32), slots, slots, slot_offset=bad)
    with pytest.raises(_lib.LseHipError, match="no CPU fallback"):
        ops.compact_ray_slots(slots, slots, 10, packed, torch.zeros(4, dtype=torch.int32), slots, slots, slot_offset=2)


# ----------------------------------------------------------------------------------------------------
# the restatement against closed forms
# ----------------------------------------------------------------------------------------------------
def test_numpy_restatement_against_closed_forms():
    n, dt, sg = 200, 1.0 / 256, 3.0
    ts = np.arange(n) * dt
    te = ts + dt
    sigma = np.full(n, sg)
    rgb = np.tile(np.array([0.25, 0.5, 1.0]), (n, 1))
    tau = tau_prefix64(ts, te, sigma)
    assert tau[0] == 0.0 and abs(tau[n] - n * dt * sg) < 1e-12
    for m in (0, 1, 64, 128, 200):
        c, acc, num, lo, hi = composite_first_m_numpy(ts, te, sigma, rgb, m)
        assert abs(acc - (1.0 - math.exp(-tau[m]))) < 1e-12           # the weights telescope: 1 - T(m)
        assert np.allclose(c, acc * np.array([0.25, 0.5, 1.0]), rtol=0, atol=1e-12)
        if m:
            assert lo == 0.5 * dt and hi == (m - 0.5) * dt and lo * acc <= num <= hi * acc
        else:
            assert num == 0.0 and lo == math.inf and hi == -math.inf
    # the rule: first boundary (before the end of the ray) at which tau has reached tau_stop
    bounds = schedule_boundaries(320, 64)                              # 64, 128, 256, 320
    assert bounds == [64, 128, 256, 320]
    assert stop_count_numpy(tau, bounds, tau[64]) == 64
    assert stop_count_numpy(tau, bounds, np.nextafter(tau[64], 1.0)) == 128
    assert stop_count_numpy(tau, bounds, tau[129]) == 200              # next boundary (256) lies beyond the ray: rendered in full
    assert stop_count_numpy(tau[:65], bounds, 0.0) == 64               # a ray that ends on a boundary is not "stopped"
    assert stop_count_numpy(tau[:1], bounds, 0.0) == 0
    # an opaque wall: inf optical depth behind it, finite in front, weights stay finite
    sigma[70] = np.inf
    tau = tau_prefix64(ts, te, sigma)
    assert np.isfinite(tau[70]) and tau[71] == np.inf
    assert stop_count_numpy(tau, bounds, 9.2) == 128
    c, acc, _, _, _ = composite_first_m_numpy(ts, te, sigma, rgb, 128)
    assert abs(acc - 1.0) < 1e-12 and np.all(np.isfinite(c))
    # nan_to_num of the colours
    rgb[3] = [np.nan, np.inf, -np.inf]
    c, _, _, _, _ = composite_first_m_numpy(ts, te, sigma, rgb, 64, nan_to_num=True)
    assert np.all(np.isfinite(c))
    c, _, _, _, _ = composite_first_m_numpy(ts, te, sigma, rgb, 64)
    assert not np.all(np.isfinite(c))
