"""Torch-facing custom ops over the C-ABI (include/lse_hip.h): tensor checks, workspace allocation, autograd.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); every op below launches the
hand-written gfx950 kernels on torch's current HIP stream.  No CPU implementation exists on this path.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import ctypes
import functools
import time

import torch

from . import _lib
from ._lib import GridDesc, MlpDesc


# ----------------------------------------------------------------------------------------------------
# helpers
# ----------------------------------------------------------------------------------------------------
def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk(t: Optional[torch.Tensor], dtype, name: str, allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError(f"{name} is None")
    if not t.is_cuda:
        raise _lib.LseHipError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _f32(t, name, allow_none=False):
    return _chk(t, torch.float32, name, allow_none)


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


_N_DEV_AT = {"lse_positions_fwd": 6, "lse_positions_bwd": 6, "lse_hash_bwd_ex": 10, "lse_point_normals_world": 5,
             "lse_tsdf_vertex_colors": 8}    # elsewhere: right before the stream


def _call_n(name: str, n_dev: Optional[torch.Tensor], *args):
    """``_lib.call`` of a per-sample entry point: inserts the ``n_dev`` argument (include/lse_hip.h: device-side sample count,
    right behind ``n``).  With a tensor (int64, on the device) the ``n`` among ``args`` is a CAPACITY and the kernels clamp it to
    ``n_dev[0]``; ``None``: plain call."""
    ptr = None
    if n_dev is not None:
        assert n_dev.dtype == torch.int64 and n_dev.is_cuda and n_dev.numel() >= 1
        ptr = ctypes.c_void_p(n_dev.data_ptr())
    at = _N_DEV_AT.get(name, len(args) - 1)
    return _lib.call(name, *args[:at], ptr, *args[at:])


# ----------------------------------------------------------------------------------------------------
# descriptors
# ----------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GridMeta:
    """tcnn HashGrid level table (host side).  Same arithmetic as tcnn's GridEncoding constructor; the oracle's
    ``tcnn_grid_meta`` is an independent restatement used by the tests to cross-check these numbers."""
    n_levels: int
    n_features: int
    log2_hashmap_size: int
    base_resolution: int
    per_level_scale: float
    scales: Tuple[float, ...]
    resolutions: Tuple[int, ...]
    offsets: Tuple[int, ...]
    # overrides of lse_hash_bwd_opts for this grid's backward, as ((field, value), ...): the caller's knowledge of the sample
    # regime (HASH_BWD_DENSE_STEPS / HASH_BWD_DEFAULT below); call arguments of lse_hash_bwd_ex, nothing the library remembers
    bwd_tuning: Tuple[Tuple[str, int], ...] = ()

    @property
    def n_entries(self):
        return self.offsets[-1]

    @property
    def n_params(self):
        return self.offsets[-1] * self.n_features

    def desc(self) -> GridDesc:
        d = GridDesc()
        d.n_levels, d.n_features = self.n_levels, self.n_features
        for i, o in enumerate(self.offsets):
            d.offsets[i] = o
        for i in range(self.n_levels):
            d.scales[i] = self.scales[i]
            d.resolutions[i] = self.resolutions[i]
        return d


def make_grid_meta(n_levels=16, n_features=2, log2_hashmap_size=19, base_resolution=16, per_level_scale=None,
                   max_res=2048) -> GridMeta:
    import numpy as np
    if per_level_scale is None:   # R:lse_nerf/lse_field.py:59
        per_level_scale = float(np.exp((np.log(max_res) - np.log(base_resolution)) / (n_levels - 1))) if n_levels > 1 else 1.0
    pls = np.float32(per_level_scale)
    l2 = np.log2(pls, dtype=np.float32)
    scales, ress, offs = [], [], [0]
    for l in range(n_levels):
        s = np.float32(np.exp2(np.float32(l) * l2, dtype=np.float32) * np.float32(base_resolution) - np.float32(1))
        r = int(np.ceil(s)) + 1
        n = min(r ** 3, (2 ** 32 - 1) // 2)
        n = (n + 7) // 8 * 8
        n = min(n, 1 << log2_hashmap_size)
        scales.append(float(s)); ress.append(r); offs.append(offs[-1] + n)
    return GridMeta(n_levels, n_features, log2_hashmap_size, base_resolution, float(pls), tuple(scales), tuple(ress),
                    tuple(offs))


@dataclass(frozen=True)
class MlpMeta:
    n_in: int                 # padded input width seen by the kernel (8/16/32/64)
    width: int
    n_hidden_layers: int
    out_activation: int = _lib.LSE_ACT_NONE
    in_layout: int = _lib.LSE_IN_ROWMAJOR
    w0_ld: int = 0            # first-layer view into params (include/lse_hip.h: lse_mlp_desc); 0 = plain layout
    w0_col: int = 0
    w0_mask_col0: int = 0
    arith: int = _lib.LSE_MLP_ARITH_AUTO      # forward arithmetic route where two are built (include/lse_hip.h: lse_mlp_desc.arith)

    @property
    def n_params(self):
        return self.width * (self.w0_ld or self.n_in) + (self.n_hidden_layers - 1) * self.width * self.width + 16 * self.width

    def desc(self) -> MlpDesc:
        return MlpDesc(self.n_in, self.width, self.n_hidden_layers, self.out_activation, self.in_layout, self.w0_ld,
                       self.w0_col, self.w0_mask_col0, self.arith)


# ----------------------------------------------------------------------------------------------------
# sampler
# ----------------------------------------------------------------------------------------------------
MAX_SLOT_ELEMS = 1 << 28   # single-pass marcher: upper limit for R * cap (2 x 1 GiB of scratch)
SYNC_STATS = {"seconds": 0.0, "count": 0}   # host time spent blocked in the sampler's count read-backs (bench.py reports it)


@torch.no_grad()
def traverse_grids(rays_o, rays_d, binaries, aabbs, near_planes, far_planes, step_size: float, cone_angle: float,
                   max_span: float = None, fma_setup: bool = False):
    """nerfacc.grid.traverse_grids as consumed at R:lse_nerf/lse_grid_estimator.py:93-106.
    Returns (ray_indices int32 [N], t_starts [N], t_ends [N], packed_info int64 [R,2]).  One host sync (N).

    max_span: host-known upper bound of (t_exit - t_enter) over all rays (clipped by the planes and the outermost aabb).
    With it the march runs ONCE into fixed-capacity per-ray slots (every sample interval is >= step_size long, so
    cap = max_span / step_size + slack bounds the count) and a copy kernel packs them; without it (or when the slots
    would be too large) the published count pass + write pass run.
    fma_setup: LSE_TRAVERSE_FMA_SETUP -- nvcc's default contraction at the four a*b+c sites of the traversal set-up."""
    flags = _lib.LSE_TRAVERSE_FMA_SETUP if fma_setup else 0
    R = rays_o.shape[0]
    L, rx, ry, rz = binaries.shape
    dev = rays_o.device
    cnts = torch.empty(R, dtype=torch.int64, device=dev)
    packed = torch.empty((R, 2), dtype=torch.int64, device=dev)
    total = torch.zeros(2, dtype=torch.int64, device=dev)   # [N, overflow flag of the single-pass marcher]
    args = (_f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), R, _chk(binaries, torch.uint8, "binaries"),
            _f32(aabbs, "aabbs"), L, rx, ry, rz, _f32(near_planes, "near_planes"), _f32(far_planes, "far_planes"),
            float(step_size), float(cone_angle))
    if SINGLE_PASS_MARCH and max_span is not None and step_size > 0 and R > 0:
        cap = int(max_span / step_size) + 8
        if 0 < cap and R * cap <= MAX_SLOT_ELEMS:
            ts_slots = torch.empty(R * cap, dtype=torch.float32, device=dev)
            te_slots = torch.empty(R * cap, dtype=torch.float32, device=dev)
            flag = total[1:].view(torch.int32)    # low word of total[1]
            _lib.call("lse_traverse_grids_slots", *args, cap, ctypes.c_void_p(cnts.data_ptr()),
                      ctypes.c_void_p(ts_slots.data_ptr()), ctypes.c_void_p(te_slots.data_ptr()),
                      ctypes.c_void_p(flag.data_ptr()), flags, _stream())
            _lib.call("lse_pack_info_from_counts", ctypes.c_void_p(cnts.data_ptr()), R, ctypes.c_void_p(packed.data_ptr()),
                      ctypes.c_void_p(total.data_ptr()), _stream())
            _t0 = time.perf_counter()
            n, overflow = (int(v) for v in total.tolist())        # <- host sync #1: the marcher's sample count
            SYNC_STATS["seconds"] += time.perf_counter() - _t0
            SYNC_STATS["count"] += 1
            if not overflow:
                ri = torch.empty(n, dtype=torch.int32, device=dev)
                ts = torch.empty(n, dtype=torch.float32, device=dev)
                te = torch.empty(n, dtype=torch.float32, device=dev)
                if n > 0:
                    _lib.call("lse_compact_ray_slots", ctypes.c_void_p(ts_slots.data_ptr()), ctypes.c_void_p(te_slots.data_ptr()),
                              cap, ctypes.c_void_p(packed.data_ptr()), R, ctypes.c_void_p(ri.data_ptr()),
                              ctypes.c_void_p(ts.data_ptr()), ctypes.c_void_p(te.data_ptr()), _stream())
                return ri, ts, te, packed
            total.zero_()   # bound violated (not expected): redo with the two-pass scheme
    _lib.call("lse_traverse_grids", *args, 0, ctypes.c_void_p(cnts.data_ptr()), None, None, None, None, flags, _stream())
    _lib.call("lse_pack_info_from_counts", ctypes.c_void_p(cnts.data_ptr()), R, ctypes.c_void_p(packed.data_ptr()),
              ctypes.c_void_p(total.data_ptr()), _stream())
    n = int(total[0].item())
    ri = torch.empty(n, dtype=torch.int32, device=dev)
    ts = torch.empty(n, dtype=torch.float32, device=dev)
    te = torch.empty(n, dtype=torch.float32, device=dev)
    if n > 0:
        starts = packed[:, 0].contiguous()
        _lib.call("lse_traverse_grids", *args, 1, None, ctypes.c_void_p(starts.data_ptr()),
                  ctypes.c_void_p(ri.data_ptr()), ctypes.c_void_p(ts.data_ptr()), ctypes.c_void_p(te.data_ptr()),
                  flags, _stream())
    return ri, ts, te, packed


@torch.no_grad()
def traverse_grids_deferred(rays_o, rays_d, binaries, aabbs, near_planes, far_planes, step_size: float, cone_angle: float,
                            cap: int, out=None, overflow=None, fma_setup: bool = False):
    """``traverse_grids`` without the host read-back of the sample count.  ``cap`` is a PROVEN upper bound of the samples of
    one ray (LSEOccGridEstimator._cap_per_ray); the packed outputs have room for ``R * cap`` samples and the actual count stays
    on the device.  Returns (ray_indices int32 [C], t_starts [C], t_ends [C], packed_info int64 [R,2], n_dev int64 [1],
    overflow int32 [1]) with C = R * cap; entries at and beyond n_dev[0] are never written nor read by the kernels that are
    handed ``n_dev``.
    ``overflow``: int32 [1] on the device that the marcher ORs into and NEVER clears -- a sticky accumulator the caller owns
    (LSEOccGridEstimator keeps one for all its calls, captured ones included, and reads it at the occupancy refresh); a fresh
    zero is allocated when absent.  Bit 0: a ray exceeded ``cap`` (its samples were truncated to ``cap``: nothing is read or
    written out of bounds); bit 1: such a ray's direction was shorter than 1.
    ``out``: a previous result of this function for the same R and cap, written into instead of allocating (a marcher that runs
    ahead of its step on a side stream fills buffers at addresses the consumer already knows: lsenerf_amd.graph)."""
    R = rays_o.shape[0]
    L, rx, ry, rz = binaries.shape
    dev = rays_o.device
    C = R * cap
    if not (0 < cap and C <= MAX_SLOT_ELEMS):
        raise _lib.LseHipError(f"deferred sampling: {R} rays x {cap} slots exceed the slot budget ({MAX_SLOT_ELEMS})")
    cnts = torch.empty(R, dtype=torch.int64, device=dev)
    if out is not None:
        ri, ts, te, packed, total, flag_o = out
        if not (ri.shape == ts.shape == te.shape == (C,) and packed.shape == (R, 2) and total.shape == (1,)):
            raise _lib.LseHipError("traverse_grids_deferred: `out` is not a result of this function for the same rays x capacity")
        if overflow is None:
            overflow = flag_o
    else:
        packed = torch.empty((R, 2), dtype=torch.int64, device=dev)
        total = torch.empty(1, dtype=torch.int64, device=dev)       # written (not accumulated) by lse_pack_info_from_counts
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    flag = _chk(overflow, torch.int32, "overflow")
    ts_slots = torch.empty(C, dtype=torch.float32, device=dev)
    te_slots = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.call("lse_traverse_grids_slots", _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), R, _chk(binaries, torch.uint8, "binaries"),
              _f32(aabbs, "aabbs"), L, rx, ry, rz, _f32(near_planes, "near_planes"), _f32(far_planes, "far_planes"),
              float(step_size), float(cone_angle), cap, ctypes.c_void_p(cnts.data_ptr()), ctypes.c_void_p(ts_slots.data_ptr()),
              ctypes.c_void_p(te_slots.data_ptr()), flag, _lib.LSE_TRAVERSE_FMA_SETUP if fma_setup else 0, _stream())
    _lib.call("lse_pack_info_from_counts", ctypes.c_void_p(cnts.data_ptr()), R, ctypes.c_void_p(packed.data_ptr()),
              ctypes.c_void_p(total.data_ptr()), _stream())
    if out is None:
        ri = torch.empty(C, dtype=torch.int32, device=dev)
        ts = torch.empty(C, dtype=torch.float32, device=dev)
        te = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.call("lse_compact_ray_slots", ctypes.c_void_p(ts_slots.data_ptr()), ctypes.c_void_p(te_slots.data_ptr()), cap,
              ctypes.c_void_p(packed.data_ptr()), R, ctypes.c_void_p(ri.data_ptr()), ctypes.c_void_p(ts.data_ptr()),
              ctypes.c_void_p(te.data_ptr()), _stream())
    return ri, ts, te, packed, total, overflow


@torch.no_grad()
def traverse_grids_slots_deferred(rays_o, rays_d, binaries, aabbs, near_planes, far_planes, step_size: float, cone_angle: float,
                                  cap: int, overflow=None, fma_setup: bool = False):
    """The marcher half of ``traverse_grids_deferred``: the same ``lse_traverse_grids_slots`` call, nothing packed.  Returns
    (cnts int64 [R], t_start_slots [R * cap], t_end_slots [R * cap], overflow int32 [1]): ray r's samples are the first cnts[r]
    entries of its slot row [r * cap, (r + 1) * cap); ``overflow`` is the sticky accumulator described there.
    ``compact_ray_slots`` packs any window of the rows."""
    R = rays_o.shape[0]
    L, rx, ry, rz = binaries.shape
    dev = rays_o.device
    C = R * cap
    if not (0 < cap and C <= MAX_SLOT_ELEMS):
        raise _lib.LseHipError(f"deferred sampling: {R} rays x {cap} slots exceed the slot budget ({MAX_SLOT_ELEMS})")
    if overflow is None:
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    flag = _chk(overflow, torch.int32, "overflow")
    cnts = torch.empty(R, dtype=torch.int64, device=dev)
    ts_slots = torch.empty(C, dtype=torch.float32, device=dev)
    te_slots = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.call("lse_traverse_grids_slots", _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), R, _chk(binaries, torch.uint8, "binaries"),
              _f32(aabbs, "aabbs"), L, rx, ry, rz, _f32(near_planes, "near_planes"), _f32(far_planes, "far_planes"),
              float(step_size), float(cone_angle), cap, ctypes.c_void_p(cnts.data_ptr()), ctypes.c_void_p(ts_slots.data_ptr()),
              ctypes.c_void_p(te_slots.data_ptr()), flag, _lib.LSE_TRAVERSE_FMA_SETUP if fma_setup else 0, _stream())
    return cnts, ts_slots, te_slots, overflow


@torch.no_grad()
def compact_ray_slots(t_start_slots, t_end_slots, cap: int, packed_info, ray_indices, t_starts, t_ends, slot_offset: int = 0):
    """``lse_compact_ray_slots``: ray r's ``packed_info[r, 1]`` samples, taken from its slot row starting at entry ``slot_offset``,
    go to ``packed_info[r, 0]`` of ``ray_indices`` / ``t_starts`` / ``t_ends`` (written in place; their extent must cover the
    packed total).  ``slot_offset + packed_info[r, 1] <= cap`` is the caller's to hold."""
    R = packed_info.shape[0]
    slot_offset = int(slot_offset)
    if not (0 <= slot_offset < cap) or t_start_slots.numel() < R * cap or t_end_slots.numel() < R * cap:
        raise ValueError(f"compact_ray_slots: slot_offset {slot_offset} outside [0, {cap}) or slot arrays shorter than {R} x {cap}")
    if R == 0:
        return
    src_s, src_e = _f32(t_start_slots, "t_start_slots"), _f32(t_end_slots, "t_end_slots")
    _lib.call("lse_compact_ray_slots", ctypes.c_void_p(src_s.value + 4 * slot_offset),
              ctypes.c_void_p(src_e.value + 4 * slot_offset), cap, _chk(packed_info, torch.int64, "packed_info"), R,
              _chk(ray_indices, torch.int32, "ray_indices"), _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _stream())


@torch.no_grad()
def fake_sample_if_empty(packed_info, n_dev, ray_indices, t_starts, t_ends, features=None):
    """nerfstudio's single fake sample (ray 0, t = 1) when the device-side count is 0 (lse_fake_sample_if_empty); in place.
    ``features = (x01 [C,3], selector [C], y [L,C,F])``: the parked pre-pass features of these very buffers -- slot 0 is zeroed
    together with the insertion (no survivor means nothing was compacted into it)."""
    fx = fs = fy = None
    stride, L, F = 0, 0, 0
    if features is not None:
        x01, sel, y = features
        fx, fs, fy = _f32(x01, "features.x01"), _chk(sel, torch.uint8, "features.selector"), _f32(y, "features.y")
        L, stride, F = y.shape[0], y.shape[1] * y.shape[2], y.shape[2]
    _lib.call("lse_fake_sample_if_empty", _chk(packed_info, torch.int64, "packed_info"), packed_info.shape[0],
              _chk(n_dev, torch.int64, "n_dev"), _chk(ray_indices, torch.int32, "ray_indices"), _f32(t_starts, "t_starts"),
              _f32(t_ends, "t_ends"), fx, fs, fy, stride, L, F, _stream())


@torch.no_grad()
def visibility_compact_deferred(ray_indices, t_starts, t_ends, sigmas, packed_info, early_stop_eps: float, alpha_thre: float,
                                from_alpha: bool = False, alpha_cap: Optional[torch.Tensor] = None):
    """``visibility_compact`` with the survivors' count left on the device: outputs keep the inputs' capacity.
    ``alpha_cap``: float32 [1] on the device; the threshold used is min(alpha_thre, alpha_cap[0]) (lse_visibility_mask_cap).
    Returns (ray_indices, t_starts, t_ends, packed_info, mask, n_dev)."""
    R = packed_info.shape[0]
    C = t_starts.shape[0]
    dev = t_starts.device
    mask = torch.empty(C, dtype=torch.uint8, device=dev)
    new_cnts = torch.empty(R, dtype=torch.int64, device=dev)
    if from_alpha:
        _lib.call("lse_visibility_mask_alpha", _f32(sigmas, "alphas"), _chk(packed_info, torch.int64, "packed_info"), R,
                  float(early_stop_eps), float(alpha_thre), ctypes.c_void_p(mask.data_ptr()),
                  ctypes.c_void_p(new_cnts.data_ptr()), _stream())
    elif alpha_cap is not None:
        _lib.call("lse_visibility_mask_cap", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
                  _chk(packed_info, torch.int64, "packed_info"), R, float(early_stop_eps), float(alpha_thre),
                  _f32(alpha_cap, "alpha_cap"), ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(new_cnts.data_ptr()), _stream())
    else:
        _lib.call("lse_visibility_mask", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
                  _chk(packed_info, torch.int64, "packed_info"), R, float(early_stop_eps), float(alpha_thre),
                  ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(new_cnts.data_ptr()), _stream())
    new_packed, total = pack_info_from_counts(new_cnts)
    o_ri = torch.empty(C, dtype=torch.int32, device=dev)
    o_ts = torch.empty(C, dtype=torch.float32, device=dev)
    o_te = torch.empty(C, dtype=torch.float32, device=dev)
    _lib.call("lse_compact_samples", ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(packed_info.data_ptr()),
              ctypes.c_void_p(new_packed.data_ptr()), R, _chk(ray_indices, torch.int32, "ray_indices"),
              _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), ctypes.c_void_p(o_ri.data_ptr()),
              ctypes.c_void_p(o_ts.data_ptr()), ctypes.c_void_p(o_te.data_ptr()), _stream())
    return o_ri, o_ts, o_te, new_packed, mask, total[0:1]


@torch.no_grad()
def ray_planes(n_rays: int, device, near_plane: float, far_plane: float, t_min=None, t_max=None, jitter=None,
               step_size: float = 0.0):
    """(near_planes[R], far_planes[R]) of R:lse_nerf/lse_grid_estimator.py:83-92 in one launch."""
    if torch.device(device).type != "cuda":      # the kernel writes both outputs: host memory would be written from the GPU
        raise _lib.LseHipError(f"ray_planes: rays must live on the GPU (got {device}); the HIP path has no CPU fallback")
    near = torch.empty(n_rays, dtype=torch.float32, device=device)
    far = torch.empty(n_rays, dtype=torch.float32, device=device)
    keep = [x for x in (t_min, t_max, jitter) if x is not None]      # (contiguous views stay alive through `keep`)
    keep = [_c(x.reshape(-1).float()) for x in keep]
    it = iter(keep)
    ptrs = [(_f32(next(it), n) if x is not None else None) for x, n in ((t_min, "t_min"), (t_max, "t_max"), (jitter, "jitter"))]
    _lib.call("lse_ray_planes", float(near_plane), float(far_plane), ptrs[0], ptrs[1], ptrs[2], float(step_size), n_rays,
              ctypes.c_void_p(near.data_ptr()), ctypes.c_void_p(far.data_ptr()), _stream())
    return near, far


@torch.no_grad()
def pack_info_from_counts(cnts: torch.Tensor, out=None):
    """``out``: (packed_info int64 [R, 2], total int64 [1]) to write into instead of allocating."""
    R = cnts.shape[0]
    if out is not None:
        packed, total = out
        if packed.shape != (R, 2) or total.shape != (1,):
            raise ValueError("pack_info_from_counts: out = (packed_info [R, 2], total [1]) expected")
        _chk(packed, torch.int64, "out.packed_info"), _chk(total, torch.int64, "out.total")
    else:
        packed = torch.empty((R, 2), dtype=torch.int64, device=cnts.device)
        total = torch.empty(1, dtype=torch.int64, device=cnts.device)   # written (not accumulated) by the kernel, also for R == 0
    _lib.call("lse_pack_info_from_counts", _chk(cnts, torch.int64, "cnts"), R, ctypes.c_void_p(packed.data_ptr()),
              ctypes.c_void_p(total.data_ptr()), _stream())
    return packed, total


@torch.no_grad()
def visibility_compact(ray_indices, t_starts, t_ends, sigmas, packed_info, early_stop_eps: float, alpha_thre: float,
                       from_alpha: bool = False):
    """render_visibility_from_density (or, ``from_alpha``, render_visibility_from_alpha with ``sigmas`` holding opacities)
    + mask compaction (R:lse_nerf/lse_grid_estimator.py:120-143)."""
    R = packed_info.shape[0]
    n = t_starts.shape[0]
    dev = t_starts.device
    if n == 0:   # nothing to cull (every ray missed every grid)
        return ray_indices, t_starts, t_ends, packed_info, torch.empty(0, dtype=torch.uint8, device=dev)
    mask = torch.empty(n, dtype=torch.uint8, device=dev)
    new_cnts = torch.empty(R, dtype=torch.int64, device=dev)
    if from_alpha:
        _lib.call("lse_visibility_mask_alpha", _f32(sigmas, "alphas"), _chk(packed_info, torch.int64, "packed_info"), R,
                  float(early_stop_eps), float(alpha_thre), ctypes.c_void_p(mask.data_ptr()),
                  ctypes.c_void_p(new_cnts.data_ptr()), _stream())
    else:
        _lib.call("lse_visibility_mask", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
                  _chk(packed_info, torch.int64, "packed_info"), R, float(early_stop_eps), float(alpha_thre),
                  ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(new_cnts.data_ptr()), _stream())
    new_packed, total = pack_info_from_counts(new_cnts)
    _t0 = time.perf_counter()
    m = int(total.item())                                         # <- host sync #2: the survivors of the visibility cull
    SYNC_STATS["seconds"] += time.perf_counter() - _t0
    SYNC_STATS["count"] += 1
    o_ri = torch.empty(m, dtype=torch.int32, device=dev)
    o_ts = torch.empty(m, dtype=torch.float32, device=dev)
    o_te = torch.empty(m, dtype=torch.float32, device=dev)
    if m > 0:
        _lib.call("lse_compact_samples", ctypes.c_void_p(mask.data_ptr()), ctypes.c_void_p(packed_info.data_ptr()),
                  ctypes.c_void_p(new_packed.data_ptr()), R, _chk(ray_indices, torch.int32, "ray_indices"),
                  _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), ctypes.c_void_p(o_ri.data_ptr()),
                  ctypes.c_void_p(o_ts.data_ptr()), ctypes.c_void_p(o_te.data_ptr()), _stream())
    return o_ri, o_ts, o_te, new_packed, mask


# ----------------------------------------------------------------------------------------------------
# positions (frustum mid-point -> contraction -> [0,1] -> selector)
# ----------------------------------------------------------------------------------------------------
class _PositionsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_o, rays_d, ray_idx, t_starts, t_ends, packed_info, contraction: bool, aabb6, pre=None, n_dev=None):
        direct = ray_idx is None
        n = rays_o.shape[0] if direct else ray_idx.shape[0]
        if pre is not None:     # (x01, selector) already computed for exactly these samples by the visibility pre-pass
            x01, sel = pre
            assert x01.shape == (n, 3) and sel.shape == (n,)
            x01 = x01.detach().view_as(x01)     # fresh tensor objects: outputs of this node
            sel = sel.view_as(sel)
        else:
            x01 = torch.empty((n, 3), dtype=torch.float32, device=rays_o.device)
            sel = torch.empty(n, dtype=torch.uint8, device=rays_o.device)
            aabb_arr = (ctypes.c_float * 6)(*aabb6) if aabb6 is not None else None
            _call_n("lse_positions_fwd", n_dev, _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d", True),
                      _chk(ray_idx, torch.int32, "ray_idx", True), _f32(t_starts, "t_starts", True),
                      _f32(t_ends, "t_ends", True), n, int(contraction), aabb_arr, ctypes.c_void_p(x01.data_ptr()),
                      ctypes.c_void_p(sel.data_ptr()), _stream())
        ctx.save_for_backward(rays_o, rays_d, ray_idx, t_starts, t_ends, packed_info)
        ctx.contraction, ctx.aabb6, ctx.n, ctx.n_dev = contraction, aabb6, n, n_dev
        ctx.mark_non_differentiable(sel)
        return x01, sel

    @staticmethod
    def backward(ctx, d_x01, _d_sel):
        rays_o, rays_d, ray_idx, t_starts, t_ends, packed_info = ctx.saved_tensors
        n = ctx.n
        d_x01 = _c(d_x01)
        aabb_arr = (ctypes.c_float * 6)(*ctx.aabb6) if ctx.aabb6 is not None else None
        if FUSED_RAY_GRAD and ray_idx is not None and packed_info is not None:
            # ray path: d(pos) is formed and summed per ray in one launch, it never exists in memory (same bits as the two launches)
            d_o = torch.empty_like(rays_o) if ctx.needs_input_grad[0] else None
            d_d = torch.empty_like(rays_d) if ctx.needs_input_grad[1] else None
            if d_o is not None or d_d is not None:
                _lib.call("lse_ray_grad_from_dx01", _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d"), _f32(t_starts, "t_starts"),
                          _f32(t_ends, "t_ends"), _chk(packed_info, torch.int64, "packed_info"), rays_o.shape[0],
                          int(ctx.contraction), aabb_arr, _f32(d_x01, "d_x01"), _f32(d_o, "d_o", True), _f32(d_d, "d_d", True),
                          _stream())
            return d_o, d_d, None, None, None, None, None, None, None, None
        d_pos = torch.empty((n, 3), dtype=torch.float32, device=d_x01.device)
        _call_n("lse_positions_bwd", ctx.n_dev, _f32(rays_o, "rays_o"), _f32(rays_d, "rays_d", True),
                  _chk(ray_idx, torch.int32, "ray_idx", True), _f32(t_starts, "t_starts", True),
                  _f32(t_ends, "t_ends", True), n, int(ctx.contraction), aabb_arr, _f32(d_x01, "d_x01"),
                  ctypes.c_void_p(d_pos.data_ptr()), _stream())
        if ray_idx is None:
            return d_pos, None, None, None, None, None, None, None, None, None
        if packed_info is None:
            raise _lib.LseHipError("positions backward w.r.t. rays needs packed_info")
        R = rays_o.shape[0]
        d_o = torch.empty_like(rays_o) if ctx.needs_input_grad[0] else None
        d_d = torch.empty_like(rays_d) if ctx.needs_input_grad[1] else None
        if d_o is not None or d_d is not None:
            _lib.call("lse_ray_grad_reduce", ctypes.c_void_p(d_pos.data_ptr()), _f32(t_starts, "t_starts"),
                      _f32(t_ends, "t_ends"), _chk(packed_info, torch.int64, "packed_info"), R,
                      _f32(d_o, "d_o", True), _f32(d_d, "d_d", True), _stream())
        return d_o, d_d, None, None, None, None, None, None, None, None


def positions(rays_o, rays_d, ray_idx, t_starts, t_ends, packed_info, contraction=True, aabb6=None, precomputed=None,
              n_dev=None):
    """Sample positions in the field's unit cube + in-bounds selector (R:lse_nerf/lse_field.py:266-274).
    ``ray_idx is None``: ``rays_o`` holds positions directly (Field.density_fn).  ``precomputed = (x01, selector)``: values
    the visibility pre-pass already produced for exactly these samples (only the autograd node is created)."""
    return _PositionsFn.apply(rays_o, rays_d, ray_idx, t_starts, t_ends, packed_info, contraction, aabb6, precomputed, n_dev)


# ----------------------------------------------------------------------------------------------------
# hash grid
# ----------------------------------------------------------------------------------------------------
def _direct_grad(p: torch.Tensor):
    """Leaf parameter whose .grad is already allocated (optim.FlatParams keeps every .grad as a view of one flat, zeroed
    buffer): the backward kernels accumulate straight into it -- the entry points accumulate anyway -- and the Function
    returns None for that input, which saves a zero-fill plus an accumulate pass per parameter and step."""
    if DIRECT_PARAM_GRADS and p.is_leaf and p.requires_grad and p.grad is not None and p.grad.dtype == torch.float32 \
            and p.grad.is_contiguous() and p.grad.shape == p.shape:
        return p.grad
    return None


class _DirectGradFn(torch.autograd.Function):
    """Identity on a leaf parameter whose gradient buffer exists (``_direct_grad``): the backward adds the incoming gradient into
    that buffer and hands NOTHING on, so the parameter's AccumulateGrad node never receives a gradient.  For parameters that plain
    torch ops consume (the torch route of the loss: MLP intensity mappers, ``ThreeToOne``, ``Powpow``) -- the kernels of the fast
    path write their parameter gradients in place already."""

    @staticmethod
    def forward(ctx, p):
        ctx.param = p
        return p.view_as(p)

    @staticmethod
    def backward(ctx, g):
        direct = _direct_grad(ctx.param)
        if direct is None:
            return g
        direct.add_(g)
        return None


def direct_grad_params(module: torch.nn.Module) -> Optional[dict]:
    """``{name: tensor}`` for ``torch.func.functional_call(module, ...)``: every parameter of ``module`` that has a preallocated
    gradient buffer behind ``_DirectGradFn``.  None when there is nothing to redirect (no such parameter, or no autograd)."""
    if not torch.is_grad_enabled():
        return None
    out = {n: _DirectGradFn.apply(p) for n, p in module.named_parameters() if _direct_grad(p) is not None}
    return out or None


# Path-selection thresholds of the hash backward by sample regime (profiles/r05_hash_bwd_thresholds.txt, MI355X): a wave that ends
# <= few_runs runs at a level adds them straight to memory; a level that ends > stage_max runs passes the sector cache unstaged.
#   constant step (cone_angle == 0: consecutive samples walk through cells at a fixed pace, the run-end count grows smoothly from
#   level to level and the queue fills well): (3, 56) -- re-tuned on the round-5 kernel (leaner cache pass, one wave per workgroup,
#   whole rays per XCD: a cache pass got cheaper than the direct adds it replaces), profiles/r05_hash_bwd_thresholds_final.txt:
#   against (6, 32) headline 2.53 -> 2.46 ms, inside-box 2.19 -> 2.14, M-packed 3.03 -> 2.96; (2, 64) is 0.6 % better at the
#   headline and 2 % worse on M-packed, and few_runs 1 falls off a cliff (2.69);
#   steps that grow with the distance (cone_angle > 0, the reference's default: sparser samples, more run ends per level):
#   (8, 48) = the library's defaults -- default configuration 1.51 -> 1.43 ms (still the best pair on the final kernel).
HASH_BWD_DENSE_STEPS = (("few_runs", 3), ("stage_max", 56))
HASH_BWD_DEFAULT = ()


_HASH_BWD_WS = {}      # (device index, stream) -> zeroed workspace of the hash backward's coarse-level replicas


def hash_bwd_opts_with_workspace(desc: GridDesc, device) -> "_lib.HashBwdOpts":
    """Default lse_hash_bwd_opts plus the zero-initialised replica workspace the call needs (lse_hash_bwd_workspace_bytes): one
    buffer per (device, stream), allocated once -- the call returns it zeroed, so it is never cleared from here."""
    o = _lib.hash_bwd_default_opts()
    nbytes = int(_lib.load().lse_hash_bwd_workspace_bytes(ctypes.byref(desc), ctypes.byref(o)))
    if nbytes > 0:
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        ws = _HASH_BWD_WS.get(key)
        if ws is None or ws.numel() * 4 < nbytes:
            ws = _HASH_BWD_WS[key] = torch.zeros((nbytes + 3) // 4, dtype=torch.float32, device=device)
        o.workspace, o.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    return o


class _HashFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x01, table, meta: GridMeta, pre_y=None, n_dev=None):
        n = x01.shape[0]
        if pre_y is not None:      # features of exactly these positions, encoded by the visibility pre-pass with this table
            assert pre_y.shape == (meta.n_levels, n, meta.n_features)
            y = pre_y.detach().view_as(pre_y)
        else:
            y = torch.empty((meta.n_levels, n, meta.n_features), dtype=torch.float32, device=x01.device)
            desc = meta.desc()
            _call_n("lse_hash_fwd", n_dev, ctypes.byref(desc), _f32(x01, "x01"), _f32(table, "table"),
                    ctypes.c_void_p(y.data_ptr()), n, _stream())
        ctx.save_for_backward(x01, table)
        ctx.meta, ctx.n_dev = meta, n_dev
        return y

    @staticmethod
    def backward(ctx, dy):
        x01, table = ctx.saved_tensors
        meta = ctx.meta
        n = x01.shape[0]
        dy = _c(dy)
        if not ctx.needs_input_grad[1]:
            # frozen table (test-time refinement): the input gradient alone -- a gather, no table-sized tensor, no scatter
            hooks = _hash_bwd_hooks_of(table)
            if hooks and hooks.get("before") is not None:
                hooks["before"]()
            dx = None
            if ctx.needs_input_grad[0]:
                dx = torch.empty_like(x01)
                desc = meta.desc()
                _call_n("lse_hash_bwd_input", ctx.n_dev, ctypes.byref(desc), _f32(x01, "x01"), _f32(dy, "dy"),
                        _f32(table, "table"), ctypes.c_void_p(dx.data_ptr()), n, _stream())
            return dx, None, None, None, None
        direct = _direct_grad(table)
        dtable = direct if direct is not None else torch.zeros_like(table)
        dx = torch.empty_like(x01) if ctx.needs_input_grad[0] else None
        desc = meta.desc()
        opts = hash_bwd_opts_with_workspace(desc, x01.device)     # defaults + the coarse-level replica workspace
        for k, v in meta.bwd_tuning:                              # the caller's regime hint (call arguments, not library state)
            setattr(opts, k, v)
        hooks = _hash_bwd_hooks_of(table)      # per TABLE, not per process: other models in the process are untouched
        split = hooks.get("split") if hooks else None
        if hooks and hooks.get("before") is not None:     # e.g. fork a side stream here: the scatter below is the last big kernel of the backward pass
            hooks["before"]()
        if split is not None and direct is not None and 0 < split[0] < meta.n_levels:
            # fine levels first (most of the table bytes); their gradients are final when the callback runs, so the caller
            # can start exchanging them while the coarse levels are still being computed (dist.OverlappedGradExchange)
            for lo, hi, acc in ((split[0], meta.n_levels, 0), (0, split[0], 1)):
                _call_n("lse_hash_bwd_ex", ctx.n_dev, ctypes.byref(desc), _f32(x01, "x01"), _f32(dy, "dy"), _f32(table, "table"),
                        ctypes.c_void_p(dtable.data_ptr()), _f32(dx, "dx", True), acc, lo, hi, n, ctypes.byref(opts), _stream())
                if acc == 0:
                    split[1]()
        else:
            _call_n("lse_hash_bwd_ex", ctx.n_dev, ctypes.byref(desc), _f32(x01, "x01"), _f32(dy, "dy"), _f32(table, "table"),
                    ctypes.c_void_p(dtable.data_ptr()), _f32(dx, "dx", True), 0, 0, meta.n_levels, n, ctypes.byref(opts),
                    _stream())
        return dx, (None if direct is not None else dtable), None, None, None


def hash_encode(x01: torch.Tensor, table: torch.Tensor, meta: GridMeta, precomputed: Optional[torch.Tensor] = None,
                n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tcnn HashGrid forward.  Returns level-major features y[L, N, F] (the fused MLP consumes this directly);
    ``y.permute(1, 0, 2).reshape(N, L*F)`` is the [N, L*F] tensor tcnn's torch binding returns.
    ``precomputed``: y already encoded for exactly these positions with this table (only the autograd node is created)."""
    return _HashFn.apply(x01, table, meta, precomputed, n_dev)


@torch.no_grad()
def compact_features(mask, packed_info, new_packed_info, n_new: int, x01, sel, y):
    """(x01, selector, y) of the ``n_new`` samples that survive ``mask`` (lse_compact_features); y is level-major [L, N, 2]."""
    R = packed_info.shape[0]
    n_old, L = x01.shape[0], y.shape[0]
    dev = x01.device
    o_x = torch.empty((n_new, 3), dtype=torch.float32, device=dev)
    o_s = torch.empty(n_new, dtype=torch.uint8, device=dev)
    o_y = torch.empty((L, n_new, 2), dtype=torch.float32, device=dev)
    _lib.call("lse_compact_features", _chk(mask, torch.uint8, "mask"), _chk(packed_info, torch.int64, "packed_info"),
              _chk(new_packed_info, torch.int64, "new_packed_info"), R, _f32(x01, "x01"), _chk(sel, torch.uint8, "selector"),
              _f32(y, "y"), L, n_old, n_new, ctypes.c_void_p(o_x.data_ptr()), ctypes.c_void_p(o_s.data_ptr()),
              ctypes.c_void_p(o_y.data_ptr()), _stream())
    return o_x, o_s, o_y


# ----------------------------------------------------------------------------------------------------
# fused MLP
# ----------------------------------------------------------------------------------------------------
def frozen_wgrad_scratch(params: torch.Tensor) -> torch.Tensor:
    """Where the recomputing MLP backward (act_tiled = 3) puts the weight-gradient products of a FROZEN parameter vector
    (``requires_grad == False``): the kernel forms them together with the data gradients, so they need an address, and nothing ever
    reads it.  One buffer of the parameter's size, kept on the parameter object for its whole life -- a captured graph bakes the
    address in (the reason ``GlobalEmbedding._zero_idx`` is a buffer) -- and therefore never allocated during a stream capture,
    whose allocations belong to that graph's pool: run one eager step first (``GraphedTrainStep`` warms up, ``freeze_field``
    allocates at once)."""
    s = getattr(params, "_lse_wgrad_scratch", None)
    if s is None or s.numel() != params.numel() or s.device != params.device:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.LseHipError("the weight-gradient scratch of a frozen MLP parameter cannot be allocated inside a stream "
                                   "capture: run one eager step (or ops.frozen_wgrad_scratch(param)) before capturing")
        s = params._lse_wgrad_scratch = torch.zeros(params.numel(), dtype=torch.float32, device=params.device)
    return s


def _x6_shape(meta: MlpMeta) -> bool:      # what mlp_x6.h recomputes: head 16 -> 64 -> 64 -> 16 row-major, base 32 -> 64 -> 16
    return meta.width == 64 and ((meta.n_in == 16 and meta.n_hidden_layers == 2 and meta.in_layout == _lib.LSE_IN_ROWMAJOR)
                                 or (meta.n_in == 32 and meta.n_hidden_layers == 1))


def mlp_input_only_shape(meta: MlpMeta) -> bool:
    """The calls ``lse_mlp_bwd_input`` and ``lse_mlp_fwd_pair`` serve: a recompute shape whose forward runs in bf16x6 arithmetic."""
    return _x6_shape(meta) and meta.arith == _lib.LSE_MLP_ARITH_AUTO


# The forward's arithmetic routes by name (include/lse_hip.h: lse_mlp_desc.arith).  "bf16x6" is what trains; the two reduced-piece
# routes are inference forwards of the head / base shapes (LSEField.inference_arith, LSENeRFModelConfig.eval_mlp_arith).
MLP_ARITH_ROUTES = {"bf16x6": _lib.LSE_MLP_ARITH_AUTO, "bf16x3": _lib.LSE_MLP_ARITH_BF16X3, "bf16x1": _lib.LSE_MLP_ARITH_BF16X1}


def mlp_reduced_arith(meta: MlpMeta) -> bool:
    return meta.arith in (_lib.LSE_MLP_ARITH_BF16X3, _lib.LSE_MLP_ARITH_BF16X1)


def mlp_reduced_shape(meta: MlpMeta) -> bool:
    """The shapes the reduced-piece forwards are built for: the head's and the base's (whatever ``meta.arith`` says)."""
    return _x6_shape(meta)


def _check_reduced_call(who: str, metas, tensors) -> None:
    """A reduced-piece route is a forward and nothing else: refuse, before any launch, a call that would need a backward or a shape
    the kernels do not serve."""
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise ValueError(f"{who}: the reduced-piece routes (bf16x3 / bf16x1) run the forward only -- call under torch.no_grad(), or "
                         "with tensors that need no gradient (a backward runs in bf16x6)")
    for meta in metas:
        if not mlp_reduced_shape(meta):
            raise ValueError(f"{who}: the reduced-piece routes serve the 16->64->64->16 row-major head and the 32->64->16 base only "
                             f"(got n_in={meta.n_in} width={meta.width} n_hidden_layers={meta.n_hidden_layers} "
                             f"in_layout={meta.in_layout})")


def _bias_grad_in_kernel(bias_grad: bool, bias_sorted: bool) -> bool:      # a needed row-bias gradient can be reduced in-kernel
    return not bias_grad or bool(FUSED_BIAS_GRAD and bias_sorted)


def mlp_bwd_route(meta: MlpMeta, *, params_grad: bool, need_grad: bool, bias_grad: bool, bias_sorted: bool, has_count: bool,
                  input_only: bool):
    """What ``fused_mlp`` saves and which backward runs, ``(act_tiled, input_only_kernel)``; touches no tensor.  0 / 1: row-major /
    tile-major saved activations.  2: the head-like case (two hidden layers, row-major input, trainable parameters), first hidden layer
    recomputed.  3: nothing saved, mlp_x6.h recomputes every hidden layer -- head / base shape with trainable parameters, or frozen
    ones under a device-side count (``has_count``: the saved-activation kernels have none; weight-gradient products go to
    ``frozen_wgrad_scratch``) or under the caller's ``input_only``, whose backward is ``lse_mlp_bwd_input``.  2 and 3 need the bias
    gradient, if any, reduced in-kernel."""
    if not (FUSED_WGRAD and ACT_TILED):
        return 0, False
    if not (need_grad and _bias_grad_in_kernel(bias_grad, bias_sorted)):
        return 1, False
    input_only = bool(input_only) and not params_grad and mlp_input_only_shape(meta)
    if RECOMPUTE_ALL and _x6_shape(meta) and (params_grad or has_count or input_only):
        return 3, input_only
    if RECOMPUTE_FIRST_LAYER and params_grad and meta.n_hidden_layers == 2 and meta.in_layout == _lib.LSE_IN_ROWMAJOR \
            and meta.n_in % 16 == 0:
        return 2, False
    return 1, False


@torch.no_grad()
def mlp_bwd_input(params, x, meta: MlpMeta, n: int, out, out_cols: int, d_out, d_sigma=None, selector=None,
                  density_scale: float = 0.0, d_in=None, row_bias=None, row_bias_idx=None, d_row_bias=None, n_dev=None) -> None:
    """``lse_mlp_bwd_input``: the data gradients of a fused MLP with FROZEN parameters -- ``d_in`` (like ``x``; overwritten) and / or
    ``d_row_bias`` (like ``row_bias``; accumulated) -- from the layer-0 input ``x``, the forward's ``out`` and ``d_out``.  No
    weight-gradient product is formed and nothing parameter-sized is written.  ``d_in`` is bit-equal to what ``lse_mlp_bwd``
    (act_tiled = 3) writes.  Head (16 -> 64 -> 64 -> 16, row-major) and base (32 -> 64 -> 16) shapes only: anything else raises."""
    desc = meta.desc()
    _call_n("lse_mlp_bwd_input", n_dev, ctypes.byref(desc), _f32(params, "params"), _f32(x, "mlp input"), _f32(out, "out", True),
            out_cols, _f32(d_out, "d_out"), _f32(d_sigma, "d_sigma", True), _chk(selector, torch.uint8, "selector", True),
            float(density_scale or 0.0), _f32(d_in, "d_in", True), _f32(row_bias, "row_bias", True),
            _chk(row_bias_idx, torch.int32, "row_bias_idx", True), _f32(d_row_bias, "d_row_bias", True), n, _stream())


def density_logit_shape(meta: MlpMeta) -> bool:
    """The call ``lse_density_logit_grad`` serves: the 32 -> 64 -> 16 base without an output activation, in bf16x6 arithmetic."""
    return meta.n_in == 32 and meta.width == 64 and meta.n_hidden_layers == 1 and meta.out_activation == _lib.LSE_ACT_NONE \
        and meta.arith == _lib.LSE_MLP_ARITH_AUTO


@torch.no_grad()
def density_logit_grad(params, x, meta: MlpMeta, n: int, d_in=None, n_dev=None) -> torch.Tensor:
    """``lse_density_logit_grad``: ``d_in = d(out[:, 0]) / d(x)`` of the base MLP (32 -> 64 -> 16, either input layout, bf16x6) --
    what ``mlp_bwd_input`` gives for a ``d_out`` of (1, 0, .., 0), without the seed and without the output layer's product.  ``d_in``
    (like ``x``; allocated when absent) is overwritten, rows at or beyond ``n_dev[0]`` are left alone; returned.  Any other shape or
    arithmetic route raises before a launch."""
    if d_in is None:
        d_in = torch.empty_like(x)
    elif d_in.shape != x.shape:
        raise ValueError(f"density_logit_grad: d_in {tuple(d_in.shape)} must have the shape of the input {tuple(x.shape)}")
    desc = meta.desc()
    _call_n("lse_density_logit_grad", n_dev, ctypes.byref(desc), _f32(params, "params"), _f32(x, "mlp input"), _f32(d_in, "d_in"),
            n, _stream())
    return d_in


@torch.no_grad()
def hash_bwd_input(x01, dy, table, meta: GridMeta, dx=None, n_dev=None) -> torch.Tensor:
    """``lse_hash_bwd_input``: ``dx[N,3]`` (allocated when absent; overwritten) from the level-major feature gradient ``dy`` -- a
    gather over the table, no atomics, nothing table-sized written."""
    if dx is None:
        dx = torch.empty_like(x01)
    desc = meta.desc()
    _call_n("lse_hash_bwd_input", n_dev, ctypes.byref(desc), _f32(x01, "x01"), _f32(dy, "dy"), _f32(table, "table"),
            _f32(dx, "dx"), x01.shape[0], _stream())
    return dx


def _mlp_bwd_recompute(params, x, meta: MlpMeta, n: int, out, out_cols: int, d_out, d_sigma, selector, density_scale, row_bias,
                       row_bias_idx, n_dev, *, input_only: bool, want_params: bool, want_in: bool, want_bias: bool, scratch=None):
    """The backward of one network on the route that saved nothing (act_tiled = 3): ``lse_mlp_bwd_input`` for frozen parameters
    under ``input_only`` -- no launch when neither gradient is wanted, no scratch -- else ``lse_mlp_bwd``, whose weight-gradient
    products go to the leaf's preallocated ``.grad`` (``_direct_grad``), to a fresh zeroed tensor, or, unwanted, to
    ``scratch`` (the forward's ``frozen_wgrad_scratch``).  Returns what autograd receives for ``(params, x, row_bias)``."""
    d_in = torch.empty_like(x) if want_in else None
    d_bias = torch.zeros_like(row_bias) if want_bias else None
    if input_only:
        if d_in is not None or d_bias is not None:
            mlp_bwd_input(params, x, meta, n, out, out_cols, d_out, d_sigma, selector, density_scale, d_in, row_bias, row_bias_idx,
                          d_bias, n_dev)
        return None, d_in, d_bias
    direct = _direct_grad(params) if want_params else None
    d_params = direct if direct is not None else (torch.zeros_like(params) if want_params else scratch)
    desc = meta.desc()
    _call_n("lse_mlp_bwd", n_dev, ctypes.byref(desc), _f32(params, "params"), _f32(x, "mlp input"), None, 3, _f32(out, "out"),
            out_cols, _f32(d_out, "d_out"), _f32(d_sigma, "d_sigma", True), _chk(selector, torch.uint8, "selector", True),
            float(density_scale or 0.0), None, None, None, _f32(d_in, "d_in", True), _f32(d_params, "d_params"),
            _f32(row_bias, "row_bias", True), _chk(row_bias_idx, torch.int32, "row_bias_idx", True), _f32(d_bias, "d_bias", True),
            n, _stream())
    return (d_params if (want_params and direct is None) else None), d_in, d_bias


class _MlpFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, params, x, row_bias, row_bias_idx, bias_packed_info, selector, meta: MlpMeta, n: int, out_cols: int,
                density_scale, n_dev=None, input_only: bool = False):
        dev = params.device
        out = torch.empty((n, out_cols), dtype=torch.float32, device=dev)
        sigma = torch.empty(n, dtype=torch.float32, device=dev) if density_scale is not None else None
        need_grad = any(t is not None and t.requires_grad for t in (params, x, row_bias))
        tiled, ctx.input_only = mlp_bwd_route(
            meta, params_grad=params.requires_grad, need_grad=need_grad, bias_grad=row_bias is not None and row_bias.requires_grad,
            bias_sorted=row_bias_idx is not None and bias_packed_info is not None, has_count=n_dev is not None, input_only=input_only)
        n_act = (n + 15) // 16 * 16 if tiled else n
        n_saved = meta.n_hidden_layers - (1 if tiled == 2 else 0)
        act = torch.empty((n_saved, n_act, meta.width), dtype=torch.float32, device=dev) if (need_grad and tiled != 3) else None
        ctx.act_tiled = tiled
        ctx.wscratch = frozen_wgrad_scratch(params) if (tiled == 3 and not params.requires_grad and not ctx.input_only) else None
        desc = meta.desc()
        if n_dev is not None and need_grad and tiled != 3:
            raise _lib.LseHipError("a device-side sample count needs the recomputing MLP kernels (width 64, head / base shape)")
        _call_n("lse_mlp_fwd", n_dev, ctypes.byref(desc), _f32(params, "params"), _f32(x, "mlp input"),
                  _f32(row_bias, "row_bias", True), _chk(row_bias_idx, torch.int32, "row_bias_idx", True),
                  ctypes.c_void_p(out.data_ptr()), out_cols, _f32(act, "act", True), tiled, _f32(sigma, "sigma", True),
                  _chk(selector, torch.uint8, "selector", True), float(density_scale or 0.0), n, _stream())
        ctx.save_for_backward(params, x, act, out, row_bias, row_bias_idx, bias_packed_info, selector)
        ctx.meta, ctx.n, ctx.out_cols, ctx.density_scale, ctx.n_dev = meta, n, out_cols, density_scale, n_dev
        ctx.set_materialize_grads(False)
        return out if sigma is None else (out, sigma)

    @staticmethod
    def backward(ctx, d_out, d_sigma=None):
        params, x, act, out, row_bias, row_bias_idx, bias_packed_info, selector = ctx.saved_tensors
        meta, n, out_cols = ctx.meta, ctx.n, ctx.out_cols
        dev = params.device
        d_out = _c(d_out) if d_out is not None else torch.zeros((n, out_cols), dtype=torch.float32, device=dev)
        d_sigma = _c(d_sigma) if d_sigma is not None else None
        need_bias = row_bias is not None and ctx.needs_input_grad[2]
        if ctx.act_tiled == 3:
            grads = _mlp_bwd_recompute(params, x, meta, n, out, out_cols, d_out, d_sigma, selector, ctx.density_scale, row_bias,
                                       row_bias_idx, ctx.n_dev, input_only=ctx.input_only, want_params=ctx.needs_input_grad[0],
                                       want_in=ctx.needs_input_grad[1], want_bias=need_bias, scratch=ctx.wscratch)
            return grads + (None,) * 9
        # sorted row indices (packed samples): the kernel reduces the bias gradient per row itself
        fused_bias = need_bias and _bias_grad_in_kernel(True, row_bias_idx is not None and bias_packed_info is not None)
        d_bias = torch.zeros_like(row_bias) if fused_bias else None
        d_act0 = torch.empty((n, meta.width), dtype=torch.float32, device=dev) if (need_bias and not fused_bias) else None
        d_in = torch.empty_like(x) if ctx.needs_input_grad[1] else None
        direct = _direct_grad(params) if (ctx.needs_input_grad[0] and (ctx.act_tiled or FUSED_WGRAD)) else None
        d_params = direct if direct is not None else (torch.zeros_like(params) if ctx.needs_input_grad[0] else None)
        desc = meta.desc()
        scale = float(ctx.density_scale or 0.0)
        sel = _chk(selector, torch.uint8, "selector", True)
        if ctx.act_tiled or FUSED_WGRAD or d_params is None:
            _call_n("lse_mlp_bwd", ctx.n_dev, ctypes.byref(desc), _f32(params, "params"), _f32(x, "mlp input"), _f32(act, "act"),
                      ctx.act_tiled, _f32(out, "out"), out_cols, _f32(d_out, "d_out"), _f32(d_sigma, "d_sigma", True), sel, scale,
                      None, None, _f32(d_act0, "d_act0", True), _f32(d_in, "d_in", True),
                      _f32(d_params, "d_params", True), _f32(row_bias, "row_bias", True),
                      _chk(row_bias_idx, torch.int32, "row_bias_idx", True) if (fused_bias or ctx.act_tiled >= 2) else None,
                      _f32(d_bias if fused_bias else None, "d_bias", True), n, _stream())
        else:   # reference structure: materialise d_act, then one G^T A reduction per layer (padded outputs only)
            assert out_cols == 16
            d_out_pre = torch.empty((n, 16), dtype=torch.float32, device=dev)
            d_act = torch.empty((meta.n_hidden_layers, n, meta.width), dtype=torch.float32, device=dev)
            _lib.call("lse_mlp_bwd", ctypes.byref(desc), _f32(params, "params"), _f32(x, "mlp input"), _f32(act, "act"),
                      0, _f32(out, "out"), out_cols, _f32(d_out, "d_out"), _f32(d_sigma, "d_sigma", True), sel, scale,
                      ctypes.c_void_p(d_out_pre.data_ptr()), ctypes.c_void_p(d_act.data_ptr()), None,
                      _f32(d_in, "d_in", True), None, None, None, None, n, None, _stream())
            _lib.call("lse_mlp_wgrad", ctypes.byref(desc), _f32(x, "mlp input"), _f32(act, "act"),
                      ctypes.c_void_p(d_act.data_ptr()), ctypes.c_void_p(d_out_pre.data_ptr()),
                      ctypes.c_void_p(d_params.data_ptr()), n, _stream())
            d_act0 = d_act[0] if need_bias else None
            fused_bias, d_bias = False, None
        if need_bias and not fused_bias:
            if row_bias_idx is None:
                d_bias = d_act0
            elif bias_packed_info is not None:
                d_bias = torch.zeros_like(row_bias)
                _lib.call("lse_segment_sum_rows", ctypes.c_void_p(d_act0.data_ptr()), meta.width,
                          _chk(bias_packed_info, torch.int64, "bias_packed_info"), row_bias.shape[0],
                          ctypes.c_void_p(d_bias.data_ptr()), _stream())
            else:   # unsorted row indices: generic scatter-add (not on the hot path)
                d_bias = torch.zeros_like(row_bias).index_add_(0, row_bias_idx.long(), d_act0)
        return (None if direct is not None else d_params), d_in, d_bias, None, None, None, None, None, None, None, None, None


def _mlp_fwd_reduced(params, x, row_bias, row_bias_idx, selector, meta: MlpMeta, n: int, out_cols: int, density_scale, n_dev):
    """``lse_mlp_fwd`` in a reduced-piece route: nothing saved, nothing recorded for autograd."""
    with torch.no_grad():
        dev = params.device
        out = torch.empty((n, out_cols), dtype=torch.float32, device=dev)
        sigma = torch.empty(n, dtype=torch.float32, device=dev) if density_scale is not None else None
        desc = meta.desc()
        _call_n("lse_mlp_fwd", n_dev, ctypes.byref(desc), _f32(params, "params"), _f32(x, "mlp input"),
                _f32(row_bias, "row_bias", True), _chk(row_bias_idx, torch.int32, "row_bias_idx", True),
                ctypes.c_void_p(out.data_ptr()), out_cols, None, 3, _f32(sigma, "sigma", True),
                _chk(selector, torch.uint8, "selector", True), float(density_scale or 0.0), n, _stream())
    return out if sigma is None else (out, sigma)


def _mlp_pair_shapes(base_meta: MlpMeta, head_meta: MlpMeta) -> bool:
    """The shapes lse_mlp_fwd_pair is built for: the recompute-all production pair (base 32 -> 64 -> 16, head 16 -> 64 -> 64 -> 16)."""
    return (mlp_input_only_shape(base_meta) and base_meta.n_in == 32 and base_meta.out_activation == _lib.LSE_ACT_NONE
            and mlp_input_only_shape(head_meta) and head_meta.n_in == 16)


class _MlpPairFn(torch.autograd.Function):
    """Base MLP (+ density head) and head MLP on the same samples: ONE forward launch (lse_mlp_fwd_pair), the two recomputing
    backward launches of ``_MlpFn`` (act_tiled = 3) with the same arguments -- head first, its d_in (plus any gradient that reaches
    ``h`` from elsewhere) is the base's d_out."""

    @staticmethod
    def forward(ctx, base_params, y, selector, head_params, row_bias, row_bias_idx, bias_packed_info, base_meta: MlpMeta,
                head_meta: MlpMeta, n: int, out_cols: int, density_scale, n_dev=None, input_only: bool = False):
        dev = base_params.device
        h = torch.empty((n, 16), dtype=torch.float32, device=dev)
        sigma = torch.empty(n, dtype=torch.float32, device=dev)
        out = torch.empty((n, out_cols), dtype=torch.float32, device=dev)
        bdesc, hdesc = base_meta.desc(), head_meta.desc()
        _call_n("lse_mlp_fwd_pair", n_dev, ctypes.byref(bdesc), _f32(base_params, "base params"), _f32(y, "mlp input"),
                _chk(selector, torch.uint8, "selector", True), float(density_scale), ctypes.byref(hdesc),
                _f32(head_params, "head params"), _f32(row_bias, "row_bias", True),
                _chk(row_bias_idx, torch.int32, "row_bias_idx", True), ctypes.c_void_p(h.data_ptr()),
                ctypes.c_void_p(sigma.data_ptr()), ctypes.c_void_p(out.data_ptr()), out_cols, n, _stream())
        ctx.save_for_backward(base_params, y, selector, head_params, row_bias, row_bias_idx, bias_packed_info, h, out)
        ctx.base_meta, ctx.head_meta, ctx.n, ctx.out_cols, ctx.density_scale, ctx.n_dev = \
            base_meta, head_meta, n, out_cols, density_scale, n_dev
        # frozen parameters: the recomputing backward still forms the weight-gradient products; they go where nothing reads them
        # (input_only: a frozen network's backward is lse_mlp_bwd_input, which forms none -- no scratch is created or touched)
        need_grad = any(t is not None and t.requires_grad for t in (base_params, y, head_params, row_bias))
        ctx.head_input_only = bool(input_only) and not head_params.requires_grad and mlp_input_only_shape(head_meta)
        ctx.base_input_only = bool(input_only) and not base_params.requires_grad and mlp_input_only_shape(base_meta)
        ctx.head_scratch = frozen_wgrad_scratch(head_params) if (need_grad and not head_params.requires_grad
                                                                 and not ctx.head_input_only) else None
        ctx.base_scratch = frozen_wgrad_scratch(base_params) if (need_grad and not base_params.requires_grad
                                                                 and y.requires_grad and not ctx.base_input_only) else None
        ctx.set_materialize_grads(False)
        return h, sigma, out

    @staticmethod
    def backward(ctx, d_h, d_sigma, d_out):
        base_params, y, selector, head_params, row_bias, row_bias_idx, bias_packed_info, h, out = ctx.saved_tensors
        n, out_cols, dev = ctx.n, ctx.out_cols, base_params.device
        wants_base = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        # ---- head (a frozen input-only head's d_in is wanted only where the base launch below will run)
        d_hp = d_in_head = d_bias = None
        if d_out is not None:
            d_hp, d_in_head, d_bias = _mlp_bwd_recompute(
                head_params, h, ctx.head_meta, n, out, out_cols, _c(d_out), None, None, 0.0, row_bias, row_bias_idx, ctx.n_dev,
                input_only=ctx.head_input_only, want_params=ctx.needs_input_grad[3], want_in=not ctx.head_input_only or wants_base,
                want_bias=row_bias is not None and ctx.needs_input_grad[4], scratch=ctx.head_scratch)
        # ---- base: d_out = the head's d_in + whatever else consumed h
        d_base = d_in_head + d_h if (d_h is not None and d_in_head is not None) else (d_in_head if d_in_head is not None else d_h)
        d_bp = d_y = None
        # (a frozen field refining its embedding needs neither d_y nor base gradients: no base launch at all)
        if (d_base is not None or d_sigma is not None) and wants_base:
            d_base = _c(d_base) if d_base is not None else torch.zeros((n, 16), dtype=torch.float32, device=dev)
            d_bp, d_y, _ = _mlp_bwd_recompute(
                base_params, y, ctx.base_meta, n, h, 16, d_base, _c(d_sigma) if d_sigma is not None else None, selector,
                ctx.density_scale, None, None, ctx.n_dev, input_only=ctx.base_input_only, want_params=ctx.needs_input_grad[0],
                want_in=ctx.needs_input_grad[1], want_bias=False, scratch=ctx.base_scratch)
        return d_bp, d_y, None, d_hp, d_bias, None, None, None, None, None, None, None, None, None


def _mlp_pair_reduced(base_meta: MlpMeta, head_meta: MlpMeta) -> bool:
    """The production pair with the same reduced-piece route in both networks."""
    return (mlp_reduced_arith(base_meta) and head_meta.arith == base_meta.arith and _x6_shape(base_meta) and base_meta.n_in == 32
            and base_meta.out_activation == _lib.LSE_ACT_NONE and _x6_shape(head_meta) and head_meta.n_in == 16)


def mlp_pair_usable(base_params, y, base_meta: MlpMeta, head_params, head_meta: MlpMeta, row_bias, row_bias_idx,
                    bias_packed_info) -> bool:
    """Whether ``fused_mlp_pair`` may replace ``fused_mlp`` (base, density head) followed by ``fused_mlp`` (head) on the same
    samples: the switch is on, the shapes are the pair's, and either nothing needs a gradient or both backward launches can take
    the recompute-all path (nothing saved, act_tiled = 3) -- with trainable parameters what ``_MlpFn.forward`` would choose, with
    frozen ones (``requires_grad == False``) the same kernels writing their weight-gradient products to ``frozen_wgrad_scratch``."""
    reduced = _mlp_pair_reduced(base_meta, head_meta)      # (a reduced-piece pair: forward only, the same route in both)
    if not (MLP_FWD_PAIR and (reduced or _mlp_pair_shapes(base_meta, head_meta))):
        return False
    need_grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (base_params, y, head_params, row_bias))
    if not need_grad:
        return True
    if reduced:
        return False
    # the pair saves nothing, so frozen parameters recompute too, as they do under a device-side count: has_count=True
    route = functools.partial(mlp_bwd_route, need_grad=True, has_count=True, input_only=False)
    base = route(base_meta, params_grad=base_params.requires_grad, bias_grad=False, bias_sorted=False)
    head = route(head_meta, params_grad=head_params.requires_grad, bias_grad=row_bias is not None and row_bias.requires_grad,
                 bias_sorted=row_bias_idx is not None and bias_packed_info is not None)
    return base[0] == 3 and head[0] == 3


def fused_mlp_pair(base_params, y, selector, density_scale, base_meta: MlpMeta, head_params, head_meta: MlpMeta, n: int,
                   row_bias=None, row_bias_idx=None, bias_packed_info=None, out_cols: int = 4, n_dev=None,
                   input_only: bool = False):
    """``fused_mlp(base_params, y, base_meta, n, density=(selector, density_scale))`` followed by ``fused_mlp(head_params, h,
    head_meta, n, row_bias, row_bias_idx, bias_packed_info, out_cols)`` with one forward launch; returns ``(h[n,16], sigma[n],
    out[n,out_cols])`` with the same bits.  Callers check ``mlp_pair_usable`` first.  ``input_only``: as in ``fused_mlp``.  Both metas
    in the same reduced route: the forward only, as in ``fused_mlp`` (same bits as its two calls in that route)."""
    if mlp_reduced_arith(base_meta) or mlp_reduced_arith(head_meta):
        _check_reduced_call("fused_mlp_pair", (base_meta, head_meta), (base_params, y, head_params, row_bias))
        if not _mlp_pair_reduced(base_meta, head_meta):
            raise ValueError("fused_mlp_pair: a reduced-piece pair needs the production shapes and the same route in both networks")
        with torch.no_grad():      # nothing saved, nothing recorded for autograd
            dev = base_params.device
            h = torch.empty((n, 16), dtype=torch.float32, device=dev)
            sigma = torch.empty(n, dtype=torch.float32, device=dev)
            out = torch.empty((n, out_cols), dtype=torch.float32, device=dev)
            bdesc, hdesc = base_meta.desc(), head_meta.desc()
            _call_n("lse_mlp_fwd_pair", n_dev, ctypes.byref(bdesc), _f32(base_params, "base params"), _f32(y, "mlp input"),
                    _chk(selector, torch.uint8, "selector", True), float(density_scale), ctypes.byref(hdesc),
                    _f32(head_params, "head params"), _f32(row_bias, "row_bias", True),
                    _chk(row_bias_idx, torch.int32, "row_bias_idx", True), ctypes.c_void_p(h.data_ptr()),
                    ctypes.c_void_p(sigma.data_ptr()), ctypes.c_void_p(out.data_ptr()), out_cols, n, _stream())
        return h, sigma, out
    return _MlpPairFn.apply(base_params, y, selector, head_params, row_bias, row_bias_idx, bias_packed_info, base_meta, head_meta,
                            n, out_cols, density_scale, n_dev, input_only)


# Hooks into the hash backward, keyed by the TABLE they belong to (its storage address): a second model in the same process -- an
# evaluation copy, the viewer thread nerfstudio runs beside training -- never sees the hooks of the model being trained.  (Until round
# 3 these were two process-global variables.)
#   "before": callable run (in the autograd thread, on the backward's stream) right before the hash backward is launched
#   "split":  (level, callback) of dist.OverlappedGradExchange: two launches, callback in between
_HASH_BWD_HOOKS: dict = {}


def _hash_bwd_hooks_of(table: torch.Tensor):
    """The hooks registered for the table stored at ``table``'s address, or None.  An entry whose owner (the tensor object the hooks
    were installed through) has been collected is dropped: its address may belong to somebody else's table by now."""
    h = _HASH_BWD_HOOKS.get(table.data_ptr())
    if h is not None and h["owner"]() is None:
        _HASH_BWD_HOOKS.pop(table.data_ptr(), None)
        return None
    return h


def set_hash_bwd_hook(table: torch.Tensor, kind: str, value) -> None:
    """Install (``value`` not None) or remove a hook of the hash backward of ``table`` (``kind``: "before" | "split").  Keyed by
    the table's storage address as it is NOW: install after optim.FlatParams has re-pointed the parameter into the flat buffer."""
    import weakref
    assert kind in ("before", "split")
    key = table.data_ptr()
    h = _hash_bwd_hooks_of(table)
    if value is None:
        if h is not None:
            h.pop(kind, None)
            if set(h) == {"owner"}:
                _HASH_BWD_HOOKS.pop(key, None)
        return
    if h is None:
        h = _HASH_BWD_HOOKS[key] = {"owner": weakref.ref(table)}
    h[kind] = value


def get_hash_bwd_hook(table: torch.Tensor, kind: str):
    h = _hash_bwd_hooks_of(table)
    return None if h is None else h.get(kind)


DIRECT_PARAM_GRADS = True   # backward kernels accumulate into a preallocated leaf .grad (see _direct_grad)
SINGLE_PASS_MARCH = True   # False: always the published count pass + write pass
FUSED_WGRAD = True    # False: materialised d_act + lse_mlp_wgrad (kept as an in-library cross-check)
FUSED_BIAS_GRAD = True   # per-row bias gradient reduced inside lse_mlp_bwd (False: d_act0 + lse_segment_sum_rows)
RECOMPUTE_ALL = True   # head + base MLPs: save no activations at all, third-generation backward (bf16 pieces) recomputes them
RECOMPUTE_FIRST_LAYER = True   # head MLP: the backward recomputes the first hidden layer instead of reading 1 KiB/sample back
ACT_TILED = True      # tile-major saved activations (1 KiB contiguous per store/load instruction); fused path only
MLP_FWD_PAIR = True   # base + head MLP forward on the same samples in one launch (lse_mlp_fwd_pair); False: two lse_mlp_fwd launches
FUSED_RAY_GRAD = True   # ray path of the positions backward: one launch (lse_ray_grad_from_dx01); False: lse_positions_bwd + lse_ray_grad_reduce


def fused_mlp(params, x, meta: MlpMeta, n: int, row_bias=None, row_bias_idx=None, bias_packed_info=None,
              out_cols: int = 16, density=None, n_dev=None, input_only: bool = False):
    """Bias-free fused MLP (tcnn layout).  Returns the padded output [n, 16] (or the compact [n, 4] = outputs 0..3).
    ``row_bias[rows, width]`` is added to the layer-0 pre-activation of sample i from row ``row_bias_idx[i]``;
    ``bias_packed_info[rows, 2]`` (start, count) must describe those rows' contiguous sample segments.
    ``density=(selector_or_None, scale)`` fuses the trunc_exp density head on output 0 and returns ``(out, sigma[n])``.
    ``input_only`` (this call's, not the process's): where ``params`` is frozen (``requires_grad == False``) and the shape is the
    head's or the base's, the backward is ``lse_mlp_bwd_input`` -- d(input) and d(row_bias) alone, no weight-gradient products and
    no ``frozen_wgrad_scratch``; everywhere else it changes nothing.
    A reduced ``meta.arith`` (``MLP_ARITH_ROUTES``: bf16x3 / bf16x1) runs the forward only, on the head / base shapes: ``ValueError``
    before any launch where gradients are enabled and params / input / row bias require one, or for another shape."""
    selector, scale = (None, None) if density is None else density
    if mlp_reduced_arith(meta):
        _check_reduced_call("fused_mlp", (meta,), (params, x, row_bias))
        return _mlp_fwd_reduced(params, x, row_bias, row_bias_idx, selector, meta, n, out_cols, scale, n_dev)
    return _MlpFn.apply(params, x, row_bias, row_bias_idx, bias_packed_info, selector, meta, n, out_cols, scale, n_dev, input_only)


# ----------------------------------------------------------------------------------------------------
# density activation
# ----------------------------------------------------------------------------------------------------
class _DensityFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, selector, scale: float):
        n = h.shape[0]
        sigma = torch.empty(n, dtype=torch.float32, device=h.device)
        _lib.call("lse_density_fwd", _f32(h, "h"), _chk(selector, torch.uint8, "selector", True), float(scale),
                  ctypes.c_void_p(sigma.data_ptr()), n, _stream())
        ctx.save_for_backward(h, selector)
        ctx.scale = scale
        return sigma

    @staticmethod
    def backward(ctx, d_sigma):
        h, selector = ctx.saved_tensors
        n = h.shape[0]
        d_h = torch.zeros_like(h)
        d_sigma = _c(d_sigma)     # bound to a name: stays alive until after the launch
        _lib.call("lse_density_bwd", _f32(h, "h"), _chk(selector, torch.uint8, "selector", True), float(ctx.scale),
                  _f32(d_sigma, "d_sigma"), ctypes.c_void_p(d_h.data_ptr()), n, _stream())
        return d_h, None, None


def density_from_mlp_out(h: torch.Tensor, selector: Optional[torch.Tensor], scale: float = 1.0) -> torch.Tensor:
    """sigma[N] = scale * trunc_exp(h[:,0]) * selector  (R:lse_nerf/lse_field.py:286-287); h is the [N,16] base output."""
    return _DensityFn.apply(h, selector, scale)


# ----------------------------------------------------------------------------------------------------
# per-ray head features and small dense layers
# ----------------------------------------------------------------------------------------------------
class _RayFeaturesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rays_d, emb_table, emb_idx):
        R = rays_d.shape[0]
        emb_dim = 0 if emb_table is None else emb_table.shape[1]
        feat = torch.empty((R, 64), dtype=torch.float32, device=rays_d.device)
        _lib.call("lse_ray_features_fwd", _f32(rays_d, "rays_d"), _f32(emb_table, "emb_table", True),
                  _chk(emb_idx, torch.int32, "emb_idx", True), R, emb_dim, ctypes.c_void_p(feat.data_ptr()), _stream())
        ctx.save_for_backward(rays_d, emb_table, emb_idx)
        return feat

    @staticmethod
    def backward(ctx, d_feat):
        rays_d, emb_table, emb_idx = ctx.saved_tensors
        R = rays_d.shape[0]
        emb_dim = 0 if emb_table is None else emb_table.shape[1]
        d_feat = _c(d_feat)
        d_dirs = torch.empty_like(rays_d) if ctx.needs_input_grad[0] else None
        d_emb = torch.zeros_like(emb_table) if (emb_table is not None and ctx.needs_input_grad[1]) else None
        _lib.call("lse_ray_features_bwd", _f32(rays_d, "rays_d"), _f32(d_feat, "d_feat"),
                  _chk(emb_idx, torch.int32, "emb_idx", True), R, emb_dim,
                  0 if emb_table is None else emb_table.shape[0], _f32(d_dirs, "d_dirs", True),
                  _f32(d_emb, "d_emb", True), _stream())
        return d_dirs, d_emb, None


def ray_features(rays_d, emb_table=None, emb_idx=None):
    """[R,64] = [SH16 | 15 zeros | emb32 | 1] per ray (tcnn SH-4 of the shifted direction)."""
    return _RayFeaturesFn.apply(rays_d, emb_table, emb_idx)


class _RayBiasFn(torch.autograd.Function):
    """Per-ray share of the head's first layer (lse_ray_bias_fwd / _bwd): directions + embedding rows -> row_bias[R, width].
    ``head_params`` is the head's tcnn parameter vector; its first width * in_pad floats are W_in[width][in_pad]."""

    @staticmethod
    def forward(ctx, rays_d, emb_table, emb_idx, head_params, width: int):
        R = rays_d.shape[0]
        emb_dim = 0 if emb_table is None else emb_table.shape[1]
        in_pad = (31 + emb_dim + 15) // 16 * 16
        dev = rays_d.device
        feat = torch.empty((R, in_pad), dtype=torch.float32, device=dev)
        row_bias = torch.empty((R, width), dtype=torch.float32, device=dev)
        _lib.call("lse_ray_bias_fwd", _f32(rays_d, "rays_d"), _f32(emb_table, "emb_table", True),
                  _chk(emb_idx, torch.int32, "emb_idx", True), R, emb_dim, _f32(head_params, "head params"), in_pad, width,
                  ctypes.c_void_p(feat.data_ptr()), ctypes.c_void_p(row_bias.data_ptr()), _stream())
        ctx.save_for_backward(rays_d, emb_table, emb_idx, head_params, feat)
        ctx.width, ctx.in_pad, ctx.emb_dim = width, in_pad, emb_dim
        return row_bias

    @staticmethod
    def backward(ctx, d_rb):
        rays_d, emb_table, emb_idx, head_params, feat = ctx.saved_tensors
        R, width, in_pad, emb_dim = rays_d.shape[0], ctx.width, ctx.in_pad, ctx.emb_dim
        d_rb = _c(d_rb)
        d_feat = torch.empty_like(feat)
        d_dirs = torch.empty_like(rays_d) if ctx.needs_input_grad[0] else None
        d_emb = direct_emb = None
        if emb_table is not None and ctx.needs_input_grad[1] and emb_idx is not None:
            direct_emb = _direct_grad(emb_table)
            d_emb = direct_emb if direct_emb is not None else torch.zeros_like(emb_table)
        _lib.call("lse_ray_bias_bwd", _f32(rays_d, "rays_d"), _chk(emb_idx, torch.int32, "emb_idx", True), R, emb_dim,
                  0 if emb_table is None else emb_table.shape[0], _f32(head_params, "head params"), in_pad, width,
                  _f32(d_rb, "d_row_bias"), ctypes.c_void_p(d_feat.data_ptr()), _f32(d_dirs, "d_dirs", True),
                  _f32(d_emb, "d_emb", True), _stream())
        d_params = None
        direct_w = None
        if ctx.needs_input_grad[3]:
            direct_w = _direct_grad(head_params)
            d_params = direct_w if direct_w is not None else torch.zeros_like(head_params)
            if in_pad in (16, 32, 64):
                _lib.call("lse_gemm_tn_acc", _f32(d_rb, "d_row_bias"), width, _f32(feat, "feat"), in_pad, _lib.LSE_IN_ROWMAJOR, R,
                          ctypes.c_void_p(d_params.data_ptr()), in_pad, _stream())
            else:       # other embedding widths (padded input 48, 80 .. 128): a plain [width x R] x [R x in_pad] library GEMM, per ray
                with torch.no_grad():
                    d_params[: width * in_pad].view(width, in_pad).addmm_(d_rb.t(), feat)
        return (d_dirs, None if direct_emb is not None else d_emb, None,
                None if direct_w is not None else d_params, None)


def ray_bias(rays_d, emb_table, emb_idx, head_params, width: int):
    """row_bias[R, width] = [SH16(dir) | 0 x 15 | emb[idx] | 1-padding] @ W_in^T, W_in = the head's tcnn input matrix."""
    return _RayBiasFn.apply(rays_d, emb_table, emb_idx, head_params, width)


class _LinearFn(torch.autograd.Function):
    """y[R,M] = x[R,K] @ w[M,K]^T on the HIP helpers (per-ray matrices only)."""

    @staticmethod
    def forward(ctx, x, w):
        R, K = x.shape
        M = w.shape[0]
        y = torch.empty((R, M), dtype=torch.float32, device=x.device)
        _lib.call("lse_linear_fwd", _f32(w, "w"), _f32(x, "x"), R, M, K, ctypes.c_void_p(y.data_ptr()), _stream())
        ctx.save_for_backward(x, w)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        R, K = x.shape
        M = w.shape[0]
        dy = _c(dy)
        dx = dw = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            _lib.call("lse_linear_bwd_input", _f32(w, "w"), _f32(dy, "dy"), R, M, K, ctypes.c_void_p(dx.data_ptr()),
                      _stream())
        if ctx.needs_input_grad[1]:
            dw = torch.zeros_like(w)
            _lib.call("lse_gemm_tn_acc", _f32(dy, "dy"), M, _f32(x, "x"), K, _lib.LSE_IN_ROWMAJOR, R,
                      ctypes.c_void_p(dw.data_ptr()), K, _stream())
        return dx, dw


def linear(x, w):
    return _LinearFn.apply(x, w)


# ----------------------------------------------------------------------------------------------------
# volume rendering
# ----------------------------------------------------------------------------------------------------
class _VolRendFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t_starts, t_ends, sigmas, rgb, packed_info, finish_depth: bool):
        R = packed_info.shape[0]
        n = t_starts.shape[0]
        dev = t_starts.device
        weights = torch.empty(n, dtype=torch.float32, device=dev)
        out_rgb = torch.empty((R, 3), dtype=torch.float32, device=dev) if rgb is not None else None
        out_acc = torch.empty(R, dtype=torch.float32, device=dev)
        out_dep = torch.empty(R, dtype=torch.float32, device=dev)      # depth numerator: sum w * (ts + te) / 2
        stride = rgb.stride(0) if rgb is not None else 0
        head = (_f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"), _rgb_ptr(rgb), stride,
                _chk(packed_info, torch.int64, "packed_info"), R, ctypes.c_void_p(weights.data_ptr()),
                _f32(out_rgb, "out_rgb", True), ctypes.c_void_p(out_acc.data_ptr()), ctypes.c_void_p(out_dep.data_ptr()))
        depth = rng = None
        if finish_depth:     # DepthRenderer("expected") epilogue in the same call: one [R,2] workspace, no pass over N
            ws = torch.empty((R, 2), dtype=torch.float32, device=dev)
            depth = torch.empty(R, dtype=torch.float32, device=dev)
            rng = torch.empty(2, dtype=torch.float32, device=dev)
            _lib.call("lse_volrend_depth_fwd", *head, ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(depth.data_ptr()),
                      ctypes.c_void_p(rng.data_ptr()), _stream())
        else:
            _lib.call("lse_volrend_fwd", *head, _stream())
        ctx.save_for_backward(t_starts, t_ends, sigmas, rgb, packed_info, weights, out_acc, out_dep, rng)
        ctx.finish_depth = finish_depth
        ctx.mark_non_differentiable(weights)
        ctx.set_materialize_grads(False)     # unused outputs (accumulation / depth) arrive as None, not as zero-filled tensors
        if out_rgb is None:
            out_rgb = torch.zeros((R, 3), dtype=torch.float32, device=dev)
        return out_rgb, out_acc, (depth if finish_depth else out_dep), weights

    @staticmethod
    def backward(ctx, g_rgb, g_acc, g_dep, _g_w):
        t_starts, t_ends, sigmas, rgb, packed_info, weights, out_acc, out_dep, rng = ctx.saved_tensors
        R = packed_info.shape[0]
        if ctx.finish_depth and g_dep is not None:
            # depth = clip(num / (acc + eps), lo, hi): O(R) chain rule back to (num, acc); zero where the clip is active
            den = out_acc + 1e-10
            raw = out_dep / den
            g = torch.where((raw >= rng[0]) & (raw <= rng[1]), g_dep.reshape(-1), torch.zeros_like(raw))
            extra_acc = -g * raw / den
            g_acc = extra_acc if g_acc is None else g_acc.reshape(-1) + extra_acc
            g_dep = g / den
        # every packed sample belongs to exactly one ray, so the kernel writes all of d_sigma; with the compact [N, 4] colour
        # layout it also writes the pad column (one 16-B store per sample), so neither buffer needs a zero-fill
        d_sigma = torch.empty_like(sigmas)
        stride = rgb.stride(0) if rgb is not None else 0
        d_rgb = None
        if rgb is not None and ctx.needs_input_grad[3]:
            d_rgb = torch.empty_like(rgb) if (stride == 4 and rgb.is_contiguous() and rgb.data_ptr() % 16 == 0) else torch.zeros_like(rgb)
        # contiguous copies are bound to names: a temporary freed before the launch could be re-used by the next allocation
        g_rgb = _c(g_rgb) if g_rgb is not None else None
        g_acc = _c(g_acc) if g_acc is not None else None
        g_dep = _c(g_dep) if g_dep is not None else None
        _lib.call("lse_volrend_bwd", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
                  _rgb_ptr(rgb), stride, _chk(packed_info, torch.int64, "packed_info"), R, _f32(weights, "weights"),
                  _f32(g_rgb, "g_rgb", True), _f32(g_acc, "g_acc", True), _f32(g_dep, "g_dep", True),
                  ctypes.c_void_p(d_sigma.data_ptr()), _rgb_ptr(d_rgb), _stream())
        return None, None, d_sigma, d_rgb, None, None


class _RenderWeightFn(torch.autograd.Function):
    """nerfacc.render_weight_from_density on packed samples (generic route: the caller composites with the weights)."""

    @staticmethod
    def forward(ctx, t_starts, t_ends, sigmas, packed_info):
        R = packed_info.shape[0]
        weights = torch.empty_like(sigmas)
        trans = torch.empty_like(sigmas)
        alphas = torch.empty_like(sigmas)
        _lib.call("lse_render_weight_fwd", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
                  _chk(packed_info, torch.int64, "packed_info"), R, ctypes.c_void_p(weights.data_ptr()),
                  ctypes.c_void_p(trans.data_ptr()), ctypes.c_void_p(alphas.data_ptr()), _stream())
        ctx.save_for_backward(t_starts, t_ends, sigmas, packed_info, weights)
        ctx.mark_non_differentiable(trans, alphas)
        return weights, trans, alphas

    @staticmethod
    def backward(ctx, g_w, _g_t, _g_a):
        t_starts, t_ends, sigmas, packed_info, weights = ctx.saved_tensors
        if g_w is None:
            return None, None, None, None
        g_w = _c(g_w)
        d_sigma = torch.empty_like(sigmas)
        _lib.call("lse_render_weight_bwd", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
                  _chk(packed_info, torch.int64, "packed_info"), packed_info.shape[0], _f32(weights, "weights"),
                  _f32(g_w, "d_weights"), ctypes.c_void_p(d_sigma.data_ptr()), _stream())
        return None, None, d_sigma, None


def render_weight_from_density(t_starts, t_ends, sigmas, packed_info):
    """(weights, transmittance, alphas), each [N]; differentiable w.r.t. sigmas through the weights."""
    if t_starts.shape[0] == 0:
        z = torch.zeros_like(sigmas)
        return z, z.clone(), z.clone()
    return _RenderWeightFn.apply(_c(t_starts), _c(t_ends), _c(sigmas), packed_info)


def _distortion_t_scale(t_scale) -> float:
    t_scale = float(t_scale)
    if not (0.0 <= t_scale < float("inf")):
        raise ValueError(f"distortion: t_scale {t_scale} is negative or not finite")
    return t_scale


def _distortion_fwd(t_starts, t_ends, weights, packed_info, t_scale: float):
    """(loss [R], totals [R,2]) of lse_distortion_fwd."""
    R = packed_info.shape[0]
    loss = torch.empty(R, dtype=torch.float32, device=weights.device)
    totals = torch.empty((R, 2), dtype=torch.float32, device=weights.device)
    _lib.call("lse_distortion_fwd", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(weights, "weights"),
              _chk(packed_info, torch.int64, "packed_info"), R, t_scale, ctypes.c_void_p(loss.data_ptr()),
              ctypes.c_void_p(totals.data_ptr()), _stream())
    return loss, totals


def _distortion_bwd(t_starts, t_ends, sigmas, weights, packed_info, t_scale: float, totals, g):
    """lse_distortion_bwd into a fresh d_sigmas buffer (``sigmas`` given: the densities the weights came from) or d_weights buffer
    (None).  ``g``: the upstream gradient [R]; a broadcast one (what the backward of a sum hands over) goes to the kernel as the
    single scalar it is."""
    to_sigma = sigmas is not None
    R = packed_info.shape[0]
    stride = 1
    if R > 0 and (g.numel() == 1 or g.stride(0) == 0):
        g, stride = g.as_strided((1,), (1,)), 0
    else:
        g = _c(g)
    out = torch.empty_like(weights)         # every sample a ray covers is written: no zero-fill (padding behind n_dev is never read)
    ptr = ctypes.c_void_p(out.data_ptr())
    _lib.call("lse_distortion_bwd", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas", True), _f32(weights, "weights"),
              _chk(packed_info, torch.int64, "packed_info"), R, t_scale, _f32(totals, "totals"), _f32(g, "g_loss"), stride,
              None if to_sigma else ptr, ptr if to_sigma else None, _stream())
    return out


class _DistortionFn(torch.autograd.Function):
    """Distortion loss per ray with its gradient sent to the densities (``to_sigma``: through render_weight_from_density inside
    the backward kernel) or to the weights themselves."""

    @staticmethod
    def forward(ctx, t_starts, t_ends, diff, weights, packed_info, t_scale: float, to_sigma: bool):
        loss, totals = _distortion_fwd(t_starts, t_ends, weights, packed_info, t_scale)
        ctx.save_for_backward(t_starts, t_ends, diff if to_sigma else None, weights, packed_info, totals)
        ctx.t_scale = t_scale
        return loss

    @staticmethod
    def backward(ctx, g):
        t_starts, t_ends, sigmas, weights, packed_info, totals = ctx.saved_tensors
        d = _distortion_bwd(t_starts, t_ends, sigmas, weights, packed_info, ctx.t_scale, totals, g)
        return None, None, d, None, None, None, None


def distortion_loss(t_starts, t_ends, sigmas, weights, packed_info, t_scale: float = 1.0):
    """Distortion loss of mip-NeRF 360 per ray, [R] (include/lse_hip.h: lse_distortion_fwd), differentiable with respect to
    ``sigmas`` only.  ``weights``: the non-differentiable fourth output of ``volume_render`` / ``volume_render_depth`` on the same
    samples; the backward is ONE launch that goes from the loss straight to d_sigma (lse_distortion_bwd), and autograd adds it
    to the d_sigma of the render (it reads ``sigmas`` for the transmittance behind the ray, exp(-sum sigma dt): 1 - sum w is
    0 or +-2^-24 on an opaque ray).  The interval ends are not differentiated.  Sample arrays may have capacity extent."""
    t_scale = _distortion_t_scale(t_scale)
    if t_starts.shape[0] == 0:
        return torch.zeros(packed_info.shape[0], dtype=torch.float32, device=sigmas.device)
    if sigmas.shape != weights.shape:
        raise ValueError(f"distortion_loss: sigmas {tuple(sigmas.shape)} and weights {tuple(weights.shape)} differ in shape")
    return _DistortionFn.apply(_c(t_starts), _c(t_ends), _c(sigmas), _c(weights.detach()), packed_info, t_scale, True)


def distortion_from_weights(weights, t_starts, t_ends, packed_info, t_scale: float = 1.0):
    """The same loss per ray, [R], differentiable with respect to ``weights`` (the generic route: the weights come from
    ``render_weight_from_density`` and the caller composites with them).  Zero samples: zeros, no launch."""
    t_scale = _distortion_t_scale(t_scale)
    if t_starts.shape[0] == 0:
        return torch.zeros(packed_info.shape[0], dtype=torch.float32, device=weights.device)
    w = _c(weights)
    return _DistortionFn.apply(_c(t_starts), _c(t_ends), w, w.detach(), packed_info, t_scale, False)


def _rgb_ptr(rgb):
    if rgb is None:
        return None
    if not rgb.is_cuda or rgb.dtype != torch.float32 or rgb.dim() != 2 or rgb.stride(1) != 1 or rgb.stride(0) < 3:
        raise ValueError("rgb must be a float32 GPU matrix [N, >=3] with unit column stride")
    return ctypes.c_void_p(rgb.data_ptr())


def volume_render(t_starts, t_ends, sigmas, rgb, packed_info):
    """render_weight_from_density + accumulate_along_rays (R:lse_nerf/lsenerf.py:301-318).
    ``rgb`` may be the padded [N,16] head output (only columns 0..2 are read).
    Returns (rgb[R,3], accumulation[R], depth_numerator[R] = sum w*(ts+te)/2, weights[N])."""
    return _VolRendFn.apply(t_starts, t_ends, sigmas, rgb, packed_info, False)


def volume_render_depth(t_starts, t_ends, sigmas, rgb, packed_info):
    """``volume_render`` + the DepthRenderer("expected") epilogue (R:lse_nerf/lsenerf.py:315-317) in one call:
    returns (rgb[R,3], accumulation[R], depth[R] = clip(num / (acc + 1e-10), min mid-point, max mid-point), weights[N])."""
    return _VolRendFn.apply(t_starts, t_ends, sigmas, rgb, packed_info, True)


@torch.no_grad()
def eval_composite(t_starts, t_ends, sigmas, rgb, packed_info, out_rgb, out_acc, out_depth, out_nsamples,
                   nan_to_num: bool, background: Optional[float], clamp: bool, workspace: Optional[torch.Tensor] = None):
    """Forward-only compositing of an evaluation render (lse_eval_composite): the values ``volume_render_depth`` and the renderer
    epilogue of ``LSENeRFModel.render_packed`` produce, bit for bit, written into ``out_rgb [n,3]``, ``out_acc [n]``, ``out_depth [n]``
    and ``out_nsamples [n]`` (int64) -- contiguous row blocks (views) of the caller's image buffers.  Sample arrays may have capacity
    extent (``packed_info`` rows are authoritative); ``rgb`` is the head output [N, >=3].  ``nan_to_num``: per-sample
    torch.nan_to_num of the colour; ``background``: blend ``rgb + background * (1 - acc)`` (None: no blend); ``clamp``:
    clamp(0, 1).  ``workspace``: float32, at least 3 n elements (allocated when absent)."""
    n = packed_info.shape[0]
    if n == 0:
        return
    if out_rgb.shape != (n, 3) or out_acc.shape != (n,) or out_depth.shape != (n,) or out_nsamples.shape != (n,):
        raise ValueError("eval_composite: out_rgb [n,3], out_acc / out_depth / out_nsamples [n] expected")
    if workspace is None:
        workspace = torch.empty(3 * n, dtype=torch.float32, device=packed_info.device)
    elif workspace.numel() < 3 * n:
        raise ValueError(f"eval_composite: workspace of {workspace.numel()} floats, {3 * n} needed")
    flags = (_lib.LSE_EVAL_NAN_TO_NUM if nan_to_num else 0) | (_lib.LSE_EVAL_BACKGROUND if background is not None else 0) \
        | (_lib.LSE_EVAL_CLAMP if clamp else 0)
    _lib.call("lse_eval_composite", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"), _rgb_ptr(rgb),
              rgb.stride(0), _chk(packed_info, torch.int64, "packed_info"), n, flags,
              float(background) if background is not None else 0.0, _f32(workspace, "workspace"), _f32(out_rgb, "out_rgb"),
              _f32(out_acc, "out_acc"), _f32(out_depth, "out_depth"), _chk(out_nsamples, torch.int64, "out_nsamples"), _stream())


@torch.no_grad()
def eval_composite_normals(t_starts, t_ends, sigmas, d_x01, packed_info, out_normals, world: bool = False, renormalize: bool = True,
                           rays_o=None, rays_d=None, contraction: bool = True, aabb6=None):
    """Rendered normals of an evaluation render (lse_eval_composite_normals) into ``out_normals [n,3]`` -- a contiguous row block
    (view) of the caller's image buffer: the render weights of ``eval_composite`` over the same samples applied to
    ``-d_x01 / max(|d_x01|, 1e-12)``, then ``N / (|N| + 1e-10)`` with ``renormalize``.  ``d_x01 [N,3]`` is the gradient of the
    density logit with respect to the unit-cube position (``LSEField.normals_packed``).  ``world``: the gradient goes through the
    transposed Jacobian of the position map first, which needs ``rays_o`` / ``rays_d [n,3]`` and ``contraction`` or ``aabb6`` as
    ``positions`` takes them.  Sample arrays may have capacity extent (``packed_info`` rows are authoritative)."""
    n = packed_info.shape[0]
    if n == 0:
        return
    if out_normals.shape != (n, 3):
        raise ValueError("eval_composite_normals: out_normals [n,3] expected")
    if d_x01.dim() != 2 or d_x01.shape[1] != 3:
        raise ValueError("eval_composite_normals: d_x01 [N,3] expected")
    flags = (_lib.LSE_NORMALS_WORLD if world else 0) | (_lib.LSE_NORMALS_RENORMALIZE if renormalize else 0)
    aabb_arr = None
    if world:
        if rays_o is None or rays_d is None or rays_o.shape != (n, 3) or rays_d.shape != (n, 3):
            raise ValueError("eval_composite_normals: world space needs rays_o and rays_d [n,3]")
        if not contraction:
            if aabb6 is None:
                raise ValueError("eval_composite_normals: world space without contraction needs aabb6")
            aabb_arr = (ctypes.c_float * 6)(*aabb6)
    _lib.call("lse_eval_composite_normals", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
              _f32(d_x01, "d_x01"), _chk(packed_info, torch.int64, "packed_info"), n, _f32(rays_o, "rays_o", not world),
              _f32(rays_d, "rays_d", not world), 1 if contraction else 0, aabb_arr, flags, _f32(out_normals, "out_normals"), _stream())


def _eval_flags(nan_to_num: bool, background: Optional[float], clamp: bool) -> int:
    return (_lib.LSE_EVAL_NAN_TO_NUM if nan_to_num else 0) | (_lib.LSE_EVAL_BACKGROUND if background is not None else 0) \
        | (_lib.LSE_EVAL_CLAMP if clamp else 0)


def eval_tau_stop(eps: float) -> float:
    """The optical depth at which the early-stop eval route finishes a ray: float32(-ln(eps)), the logarithm taken in double."""
    import math
    import numpy as np
    if not (0.0 < eps < 1.0):
        raise ValueError(f"eval_tau_stop: eps must lie in (0, 1), got {eps}")
    return float(np.float32(-math.log(float(eps))))


def eval_segment_state_bytes(n_rays: int) -> int:
    """Bytes of the per-ray compositing state the three calls below share (lse_eval_segment_state_bytes)."""
    v = ctypes.c_int64(0)
    _lib.call("lse_eval_segment_state_bytes", int(n_rays), ctypes.byref(v))
    return int(v.value)


def _segment_state_ptr(state: torch.Tensor, n_rays: int):
    if not state.is_cuda or not state.is_contiguous() or state.numel() * state.element_size() < eval_segment_state_bytes(n_rays):
        raise ValueError(f"segment state: a contiguous GPU buffer of at least {eval_segment_state_bytes(n_rays)} bytes expected")
    return ctypes.c_void_p(state.data_ptr())


@torch.no_grad()
def eval_segment_begin(ray_cnts, first_len: int, state, seg_cnts):
    """Start of a segmented eval compositing (lse_eval_segment_begin): resets ``state`` (a buffer of ``eval_segment_state_bytes``)
    for the ``ray_cnts.shape[0]`` rays and writes segment 0's counts ``seg_cnts[r] = min(ray_cnts[r], first_len)``."""
    n = ray_cnts.shape[0]
    if seg_cnts.shape != (n,):
        raise ValueError("eval_segment_begin: seg_cnts [n] expected")
    st = _segment_state_ptr(state, n)
    _lib.call("lse_eval_segment_begin", _chk(ray_cnts, torch.int64, "ray_cnts"), n, int(first_len), st,
              _chk(seg_cnts, torch.int64, "seg_cnts"), _stream())


@torch.no_grad()
def eval_composite_segment(t_starts, t_ends, sigmas, rgb, seg_packed, ray_cnts, seg_end: int, next_len: int, tau_stop: float, state,
                           next_seg_cnts, nan_to_num: bool):
    """One segment of the segmented eval compositing (lse_eval_composite_segment): every ray continues from ``state`` over the
    ``seg_packed`` samples of this segment's packed arrays; a ray with no sample beyond ``seg_end`` or a carried optical depth
    >= ``tau_stop`` is finished.  ``next_seg_cnts`` receives the next segment's counts (``next_len == 0``: last segment, may be
    None)."""
    n = seg_packed.shape[0]
    if ray_cnts.shape != (n,) or (next_seg_cnts is not None and next_seg_cnts.shape != (n,)):
        raise ValueError("eval_composite_segment: ray_cnts / next_seg_cnts [n] expected")
    _lib.call("lse_eval_composite_segment", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"), _rgb_ptr(rgb),
              rgb.stride(0), _chk(seg_packed, torch.int64, "seg_packed"), _chk(ray_cnts, torch.int64, "ray_cnts"), n,
              _eval_flags(nan_to_num, None, False), int(seg_end), int(next_len), float(tau_stop), _segment_state_ptr(state, n),
              _chk(next_seg_cnts, torch.int64, "next_seg_cnts", allow_none=True), _stream())


@torch.no_grad()
def eval_composite_finish(state, out_rgb, out_acc, out_depth, out_nsamples, background: Optional[float], clamp: bool,
                          workspace: Optional[torch.Tensor] = None):
    """End of the segmented eval compositing (lse_eval_composite_finish): ``eval_composite``'s reductions and epilogue over the state;
    ``out_nsamples`` = samples composited per ray.  Outputs and ``workspace`` as in ``eval_composite``."""
    n = out_acc.shape[0]
    if n == 0:
        return
    if out_rgb.shape != (n, 3) or out_depth.shape != (n,) or out_nsamples.shape != (n,):
        raise ValueError("eval_composite_finish: out_rgb [n,3], out_acc / out_depth / out_nsamples [n] expected")
    if workspace is None:
        workspace = torch.empty(3 * n, dtype=torch.float32, device=out_acc.device)
    elif workspace.numel() < 3 * n:
        raise ValueError(f"eval_composite_finish: workspace of {workspace.numel()} floats, {3 * n} needed")
    _lib.call("lse_eval_composite_finish", _segment_state_ptr(state, n), n, _eval_flags(False, background, clamp),
              float(background) if background is not None else 0.0, _f32(workspace, "workspace"), _f32(out_rgb, "out_rgb"),
              _f32(out_acc, "out_acc"), _f32(out_depth, "out_depth"), _chk(out_nsamples, torch.int64, "out_nsamples"), _stream())


def depth_tau(q: float) -> float:
    """The optical depth behind which a ray's accumulated weight has reached ``q``: float32(-ln(1 - q)), the logarithm taken in
    double (``1 - exp(-tau) >= q``); ``q = 0.5`` is the median depth's.  ValueError unless ``0 < q < 1``."""
    import math
    import numpy as np
    q = float(q)
    if not (0.0 < q < 1.0):
        raise ValueError(f"depth_tau: q must lie in (0, 1), got {q}")
    return float(np.float32(-math.log1p(-q)))


def _depth_quantile_args(who: str, n: int, tau_q, depth_q, reached, depth_sel, interpolate: bool, sel: int, max_spread):
    taus = [float(v) for v in tau_q]
    n_q = len(taus)
    if tuple(depth_q.shape) != (n, n_q) or tuple(reached.shape) != (n,) or (depth_sel is not None and tuple(depth_sel.shape) != (n,)):
        raise ValueError(f"{who}: depth_q [n, {n_q}], reached [n] and depth_sel [n] expected for n = {n} rays")
    if not 0 <= int(sel) <= 3:
        raise ValueError(f"{who}: sel {sel} outside 0..3")
    flags = (_lib.LSE_DEPTH_INTERPOLATE if interpolate else 0) | (int(sel) << 8)
    spread = float("inf") if max_spread is None else float(max_spread)
    return n_q, (ctypes.c_float * max(n_q, 1))(*taus), flags, spread


@torch.no_grad()
def eval_depth_quantiles(t_starts, t_ends, sigmas, packed_info, tau_q, depth_q, reached, depth_sel=None, interpolate: bool = False,
                         sel: int = 0, max_spread: Optional[float] = None):
    """Quantile depths of an evaluation render (lse_eval_depth_quantiles; the definition is in include/lse_hip.h): per ray and per
    ``tau_q[j]`` (``depth_tau(q_j)``, 1..4 strictly ascending values) the depth of the first sample behind which the optical depth
    has reached it -- its mid-point, or with ``interpolate`` the crossing inside it -- into ``depth_q [n, n_q]``; bit j of
    ``reached [n]`` (uint8) says whether it was reached (else the depth is the last sample's mid-point; a ray without samples gets
    0).  ``depth_sel [n]`` (optional): column ``sel`` where it was reached and, with ``max_spread``, the last column was reached too
    and lies at most ``max_spread`` behind the first; NaN elsewhere.  The outputs may be contiguous row blocks (views) of image
    buffers; sample arrays may have capacity extent (``packed_info`` rows are authoritative)."""
    n = packed_info.shape[0]
    n_q, taus, flags, spread = _depth_quantile_args("eval_depth_quantiles", n, tau_q, depth_q, reached, depth_sel, interpolate, sel,
                                                    max_spread)
    _lib.call("lse_eval_depth_quantiles", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
              _chk(packed_info, torch.int64, "packed_info"), n, n_q, taus, flags, spread, _f32(depth_q, "depth_q"),
              _chk(reached, torch.uint8, "reached"), _f32(depth_sel, "depth_sel", allow_none=True), _stream())


@torch.no_grad()
def eval_depth_quantiles_segment(t_starts, t_ends, sigmas, seg_packed, tau_q, state, depth_q, reached, depth_sel=None,
                                 interpolate: bool = False, sel: int = 0, max_spread: Optional[float] = None):
    """One segment of ``eval_depth_quantiles`` on the early-stop route (lse_eval_depth_quantiles_segment): every ray with a count in
    ``seg_packed`` continues from ``state [n, 2]`` (float32: the carry and the found mask; zeros are the start) over this segment's
    packed samples; other rays are left alone.  ``depth_q`` / ``reached`` / ``depth_sel`` persist between the segments and start as
    0 / 0 / NaN; after the last segment they hold what ``eval_depth_quantiles`` gives over the samples walked, bit for bit."""
    n = seg_packed.shape[0]
    n_q, taus, flags, spread = _depth_quantile_args("eval_depth_quantiles_segment", n, tau_q, depth_q, reached, depth_sel,
                                                    interpolate, sel, max_spread)
    if tuple(state.shape) != (n, 2):
        raise ValueError(f"eval_depth_quantiles_segment: state [n, 2] expected for n = {n} rays")
    _lib.call("lse_eval_depth_quantiles_segment", _f32(t_starts, "t_starts"), _f32(t_ends, "t_ends"), _f32(sigmas, "sigmas"),
              _chk(seg_packed, torch.int64, "seg_packed"), n, n_q, taus, flags, spread, _f32(state, "state"),
              _f32(depth_q, "depth_q"), _chk(reached, torch.uint8, "reached"), _f32(depth_sel, "depth_sel", allow_none=True),
              _stream())


def ssim_window(size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    """torchmetrics' 1-D Gaussian window in float32: exp(-(d / sigma)^2 / 2) for d = -(size-1)/2 .. (size-1)/2, normalised.  The
    image-metrics kernel takes these taps from the host (their outer product is the 2-D window), so kernel and test oracle share them."""
    d = torch.arange((1 - size) / 2, (1 + size) / 2, 1.0, dtype=torch.float32)
    g = torch.exp(-torch.pow(d / sigma, 2) / 2)
    return g / g.sum()


_SSIM_WINDOW = None


def image_metrics_workspace_bytes(B: int, C: int, H: int, W: int) -> int:
    v = ctypes.c_int64(0)
    _lib.call("lse_image_metrics_workspace", int(B), int(C), int(H), int(W), ctypes.byref(v))
    return int(v.value)


@torch.no_grad()
def image_metrics(preds: torch.Tensor, target: torch.Tensor, out: Optional[torch.Tensor] = None,
                  workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ssim, mse): two 0-dim float32 device tensors for ``preds`` / ``target`` [B,C,H,W] f32 (lse_image_metrics; H, W >= 11).
    SSIM is torchmetrics' ``structural_similarity_index_measure(preds, target)`` with its defaults (Gaussian 11-tap window, sigma 1.5,
    data range from the inputs, K = (0.01, 0.03), mean over the valid windows), restated from the published algorithm: torchmetrics
    is not a dependency, so that parity is UNPINNED -- the tests hold the kernel against a float64 numpy restatement.  MSE is the mean
    squared difference over every pixel.  Nothing is read back to the host.  ``out``: a contiguous float32 device tensor whose
    first two elements receive (ssim, mse) -- a row of a metrics table; ``workspace``: float64, at least
    ``image_metrics_workspace_bytes`` bytes (both allocated when absent)."""
    global _SSIM_WINDOW
    if preds.dim() != 4 or preds.shape != target.shape:
        raise ValueError(f"image_metrics: preds and target must both be [B,C,H,W] (got {tuple(preds.shape)} and {tuple(target.shape)})")
    B, C, H, W = preds.shape
    nbytes = image_metrics_workspace_bytes(B, C, H, W)       # refuses H or W < 11 with the library's message
    if _SSIM_WINDOW is None:
        _SSIM_WINDOW = (ctypes.c_float * 11)(*ssim_window().tolist())
    if workspace is None:
        workspace = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=preds.device)
    elif workspace.numel() * 8 < nbytes:
        raise ValueError(f"image_metrics: workspace of {workspace.numel() * 8} bytes, {nbytes} needed")
    if out is None:
        out = torch.empty(2, dtype=torch.float32, device=preds.device)
    elif out.dim() != 1 or out.numel() < 2:
        raise ValueError("image_metrics: out must be a 1-D tensor of at least two elements")
    _lib.call("lse_image_metrics", _f32(preds, "preds"), _f32(target, "target"), B, C, H, W, _SSIM_WINDOW,
              _chk(workspace, torch.float64, "workspace"), nbytes, _f32(out, "out"), ctypes.c_void_p(out.data_ptr() + 4), _stream())
    return out[0], out[1]


# ----------------------------------------------------------------------------------------------------
# whole eval sets: rays of one camera, metric planes, the event-only metric's scale correction
# ----------------------------------------------------------------------------------------------------
def camera_desc(fx: float, fy: float, cx: float, cy: float, H: int, W: int, dist=None) -> "_lib.CameraDesc":
    """``lse_camera_desc`` of one camera set; ``dist``: (k1, k2, k3, k4, p1, p2), None or all zero = pinhole."""
    d = [0.0] * 6 if dist is None else [float(v) for v in dist]
    if len(d) != 6:
        raise ValueError("camera_desc: six distortion parameters (k1, k2, k3, k4, p1, p2) expected")
    return _lib.CameraDesc(fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), dist=(ctypes.c_float * 6)(*d),
                           distort=int(any(v != 0.0 for v in d)), H=int(H), W=int(W))


@torch.no_grad()
def camera_rays(cam_desc, pose: torch.Tensor, first: int, n: int, out=None):
    """(origins [n, 3], directions [n, 3], pixel_area [n, 1], directions_norm [n, 1]) of the row-major pixels ``[first, first + n)``
    of the camera ``cam_desc`` (``camera_desc``) with the pose ``pose`` [3, 4] -- a float32 device tensor, usually a row of a pose
    table (lse_camera_rays: ``EdCameras.generate_rays`` with the composer's arithmetic, bit-equal to ``BatchComposer.compose`` on the
    same pixels).  ``out``: four contiguous float32 tensors of at least ``n`` rows to write rows ``[0, n)`` of (returned as given)."""
    first, n = int(first), int(n)
    if tuple(pose.shape) != (3, 4):
        raise ValueError(f"camera_rays: pose must be [3, 4], got {tuple(pose.shape)}")
    if out is None:
        dev = pose.device
        rows = max(n, 0)
        out = (torch.empty((rows, 3), dtype=torch.float32, device=dev), torch.empty((rows, 3), dtype=torch.float32, device=dev),
               torch.empty((rows, 1), dtype=torch.float32, device=dev), torch.empty((rows, 1), dtype=torch.float32, device=dev))
    o, d, area, norm = out
    for t, width, name in ((o, 3, "origins"), (d, 3, "directions"), (area, 1, "pixel_area"), (norm, 1, "directions_norm")):
        if t.numel() < max(n, 0) * width or (t.dim() > 1 and t.shape[-1] != width):
            raise ValueError(f"camera_rays: {name} must hold at least {n} rows of {width}")
    _lib.call("lse_camera_rays", ctypes.byref(cam_desc), _f32(pose, "pose"), first, n, _f32(o, "origins"), _f32(d, "directions"),
              _f32(area, "pixel_area"), _f32(norm, "directions_norm"), _stream())
    return out


def log_scale_correct_workspace_bytes(H: int, W: int) -> int:
    v = ctypes.c_int64(0)
    _lib.call("lse_log_scale_correct_workspace", int(H), int(W), ctypes.byref(v))
    return int(v.value)


_PIX_OF_DTYPE = {torch.uint8: _lib.LSE_PIX_U8, torch.float32: _lib.LSE_PIX_F32}


@torch.no_grad()
def eval_image_prep(gt: torch.Tensor, rgb: torch.Tensor, msk: Optional[torch.Tensor] = None, event_stats: bool = False, out=None,
                    stats: Optional[torch.Tensor] = None):
    """(gt_planes, pred_planes, stats): the two [1, 3, H, W] float32 images ``image_metrics`` takes, from the resident ground truth
    ``gt`` [H, W, 3] (uint8: ``float(u8) / 255``; or float32), the rendered ``rgb`` [H * W, 3] (or [H, W, 3]) and the optional mask
    ``msk`` [H, W] (uint8 or float32): ``moveaxis(image * msk)`` / ``moveaxis(rgb * msk)`` of ``image_metrics_and_images`` bit for
    bit, in one launch (lse_eval_image_prep).  ``event_stats``: also the per-workgroup moments of the event-only metric into
    ``stats`` (float64, ``log_scale_correct_workspace_bytes``; allocated when absent) for ``log_scale_correct``; else ``stats``
    is returned as None.  ``out``: (gt_planes, pred_planes) to write into."""
    if gt.dim() != 3 or gt.shape[-1] != 3 or gt.dtype not in _PIX_OF_DTYPE:
        raise ValueError(f"eval_image_prep: gt must be uint8 or float32 [H, W, 3], got {gt.dtype} {tuple(gt.shape)}")
    H, W = int(gt.shape[0]), int(gt.shape[1])
    if rgb.numel() != H * W * 3 or rgb.shape[-1] != 3:
        raise ValueError(f"eval_image_prep: rgb must be [{H * W}, 3], got {tuple(rgb.shape)}")
    msk_type = _lib.LSE_PIX_NONE
    if msk is not None:
        if tuple(msk.shape) != (H, W) or msk.dtype not in _PIX_OF_DTYPE:
            raise ValueError(f"eval_image_prep: msk must be uint8 or float32 [{H}, {W}], got {msk.dtype} {tuple(msk.shape)}")
        msk_type = _PIX_OF_DTYPE[msk.dtype]
    if out is None:
        out = (torch.empty((1, 3, H, W), dtype=torch.float32, device=rgb.device),
               torch.empty((1, 3, H, W), dtype=torch.float32, device=rgb.device))
    gt_pl, pr_pl = out
    if gt_pl.numel() != 3 * H * W or pr_pl.numel() != 3 * H * W:
        raise ValueError(f"eval_image_prep: the planes must be [1, 3, {H}, {W}]")
    nbytes = 0
    if event_stats:
        nbytes = log_scale_correct_workspace_bytes(H, W)
        if stats is None:
            stats = torch.empty(nbytes // 8, dtype=torch.float64, device=rgb.device)
        elif stats.numel() * 8 < nbytes:
            raise ValueError(f"eval_image_prep: stats of {stats.numel() * 8} bytes, {nbytes} needed")
    else:
        stats = None
    _lib.call("lse_eval_image_prep", _chk(gt, gt.dtype, "gt"), _PIX_OF_DTYPE[gt.dtype],
              _chk(msk, msk.dtype, "msk") if msk is not None else None, msk_type, _f32(rgb, "rgb"), H, W,
              _lib.LSE_PREP_EVENT_STATS if event_stats else 0, _f32(gt_pl, "gt_planes"), _f32(pr_pl, "pred_planes"),
              _chk(stats, torch.float64, "stats", allow_none=True), nbytes, _stream())
    return gt_pl, pr_pl, stats


@torch.no_grad()
def log_scale_correct(gt_planes: torch.Tensor, rgb: torch.Tensor, stats: torch.Tensor, out=None):
    """(coef [2], corrected [1, 1, H, W], gray [1, 1, H, W]) of the event-only metric (lse_log_scale_correct;
    R:lse_nerf/utils.py:99-135): the least-squares affine fit ``log(gray gt + 1e-6) ~ a log(pred_r + pred_g + 1e-6) + b`` from the
    moments ``eval_image_prep(..., event_stats=True)`` left in ``stats``, solved in double (``coef`` = (a, b) in float32; 5/255
    where the reference's NaN rule applies or the system is singular), the corrected prediction ``exp(a x + b)`` and the grey
    ground truth.  ``gt_planes`` [1, 3, H, W] and ``rgb`` are those of the prep call.  Deterministic; nothing is read back."""
    if gt_planes.dim() != 4 or gt_planes.shape[:2] != (1, 3):
        raise ValueError(f"log_scale_correct: gt_planes must be [1, 3, H, W], got {tuple(gt_planes.shape)}")
    H, W = int(gt_planes.shape[2]), int(gt_planes.shape[3])
    if rgb.numel() != H * W * 3 or rgb.shape[-1] != 3:
        raise ValueError(f"log_scale_correct: rgb must be [{H * W}, 3], got {tuple(rgb.shape)}")
    nbytes = log_scale_correct_workspace_bytes(H, W)
    if stats is None or stats.numel() * 8 < nbytes:
        raise ValueError(f"log_scale_correct: stats of at least {nbytes} bytes expected (eval_image_prep(..., event_stats=True))")
    if out is None:
        dev = rgb.device
        out = (torch.empty(2, dtype=torch.float32, device=dev), torch.empty((1, 1, H, W), dtype=torch.float32, device=dev),
               torch.empty((1, 1, H, W), dtype=torch.float32, device=dev))
    coef, corrected, gray = out
    if coef.numel() < 2 or corrected.numel() != H * W or gray.numel() != H * W:
        raise ValueError(f"log_scale_correct: coef [2] and two [1, 1, {H}, {W}] planes expected")
    _lib.call("lse_log_scale_correct", _f32(gt_planes, "gt_planes"), _f32(rgb, "rgb"), H, W, _chk(stats, torch.float64, "stats"),
              nbytes, _f32(coef, "coef"), _f32(corrected, "corrected"), _f32(gray, "gray"), _stream())
    return coef, corrected, gray


# ----------------------------------------------------------------------------------------------------
# eval panels: 8-bit grey, Canny edges, the writer's uint8 grid (csrc/panels.hip)
# ----------------------------------------------------------------------------------------------------
PANEL_KEYS = ("img", "depth", "err_map", "overlay", "ev_out")          # the grid's column order; "img" is two images wide
_PANEL_FLAG = {"img": _lib.LSE_PANEL_IMG, "depth": _lib.LSE_PANEL_DEPTH, "err_map": _lib.LSE_PANEL_ERR_MAP,
               "overlay": _lib.LSE_PANEL_OVERLAY, "ev_out": _lib.LSE_PANEL_EV_OUT}


def _u8(t, name, allow_none=False):
    return _chk(t, torch.uint8, name, allow_none)


def _planes_hw(t: torch.Tensor, name: str) -> Tuple[int, int]:
    if t.dim() < 3 or t.numel() != 3 * t.shape[-2] * t.shape[-1] or t.shape[-3] != 3:
        raise ValueError(f"{name} must be [3, H, W] or [1, 3, H, W], got {tuple(t.shape)}")
    return int(t.shape[-2]), int(t.shape[-1])


def _images_u8(t: torch.Tensor, name: str) -> Tuple[int, int, int]:
    if t.dim() not in (2, 3) or t.numel() == 0:
        raise ValueError(f"{name} must be a non-empty uint8 [H, W] or [n, H, W], got {tuple(t.shape)}")
    return (1 if t.dim() == 2 else int(t.shape[0])), int(t.shape[-2]), int(t.shape[-1])


def canny_workspace_bytes(H: int, W: int, n_images: int = 1) -> int:
    v = ctypes.c_int64(0)
    _lib.call("lse_canny_workspace", int(H), int(W), ctypes.byref(v))
    return int(v.value) * int(n_images)


def _canny_workspace(workspace, n, H, W, device, name):
    nbytes = canny_workspace_bytes(H, W, n)
    if workspace is None:
        workspace = torch.empty(nbytes // 8, dtype=torch.int64, device=device)
    elif workspace.numel() * workspace.element_size() < nbytes or workspace.element_size() != 8:
        raise ValueError(f"{name}: an 8-byte-typed workspace of at least {nbytes} bytes expected (canny_workspace_bytes)")
    if not workspace.is_cuda or not workspace.is_contiguous():
        raise _lib.LseHipError(f"{name}: the workspace must be a contiguous tensor on the GPU; the HIP path has no CPU fallback")
    return workspace, ctypes.c_void_p(workspace.data_ptr()), nbytes


@torch.no_grad()
def gray8_planes(planes_a: torch.Tensor, planes_b: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 [2, H, W] (or [1, H, W] without ``planes_b``): ``clip(grey * 255, 0, 255)`` truncated, of the float32 [3, H, W] planes
    ``eval_image_prep`` writes, grey = (0.2989 r + 0.5870 g) + 0.1140 b as that kernel takes it (lse_gray8_planes).  What the
    reference's ``_make_overlay`` feeds ``cv2.Canny``; a NaN gives 0 (numpy's cast of a NaN is undefined)."""
    H, W = _planes_hw(planes_a, "gray8_planes: planes_a")
    if planes_b is not None and _planes_hw(planes_b, "gray8_planes: planes_b") != (H, W):
        raise ValueError("gray8_planes: the two images differ in size")
    n = 1 if planes_b is None else 2
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.uint8, device=planes_a.device)
    elif out.numel() != n * H * W:
        raise ValueError(f"gray8_planes: out must be [{n}, {H}, {W}]")
    _lib.call("lse_gray8_planes", _f32(planes_a, "planes_a"), _f32(planes_b, "planes_b", allow_none=True), H, W, _u8(out, "out"),
              _stream())
    return out


@torch.no_grad()
def canny_classify(gray_u8: torch.Tensor, low: int = 50, high: int = 200, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The class map (0 none, 1 weak, 2 strong; uint8, shaped like the input) of ``gray_u8`` [H, W] or [n, H, W]: OpenCV's
    ``Canny(image, low, high)`` (aperture 3, L1 gradient) up to the hysteresis, restated from the published algorithm -- parity
    unpinned (lse_canny_classify).  ``low`` / ``high`` are floored to integers as OpenCV floors them."""
    n, H, W = _images_u8(gray_u8, "canny_classify: gray_u8")
    ptr = _u8(gray_u8, "gray_u8")
    if out is None:
        out = torch.empty_like(gray_u8)
    elif out.shape != gray_u8.shape:
        raise ValueError("canny_classify: out must have the input's shape")
    _lib.call("lse_canny_classify", ptr, n, H, W, int(low // 1), int(high // 1), _u8(out, "out"), _stream())
    return out


@torch.no_grad()
def canny_hysteresis(classes: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Edges (uint8 0 / 255, shaped like the input) of a class map: strong pixels, and weak ones 8-connected to a strong one through
    weak and strong pixels (lse_canny_hysteresis: union-find on the device, three bounded launches, no host loop; the result is a
    set, so two calls are bit-equal).  ``workspace``: an int64 / float64 device tensor of ``canny_workspace_bytes(H, W, n)`` bytes
    (allocated when absent; its content does not matter).  ``out`` may be ``classes``."""
    n, H, W = _images_u8(classes, "canny_hysteresis: classes")
    ptr = _u8(classes, "classes")
    if out is None:
        out = torch.empty_like(classes)
    elif out.shape != classes.shape:
        raise ValueError("canny_hysteresis: out must have the input's shape")
    workspace, ws_ptr, nbytes = _canny_workspace(workspace, n, H, W, classes.device, "canny_hysteresis")
    _lib.call("lse_canny_hysteresis", ptr, n, H, W, ws_ptr, nbytes, _u8(out, "out"), _stream())
    return out


@torch.no_grad()
def canny_edges(gray_u8: torch.Tensor, low: int = 50, high: int = 200, out: Optional[torch.Tensor] = None,
                workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``cv2.Canny(gray_u8, low, high)`` (uint8 0 / 255) of a uint8 [H, W] image or [n, H, W] stack on the device: ``canny_classify``
    then ``canny_hysteresis`` on one stream (lse_canny_u8).  Restated from OpenCV's published algorithm; OpenCV is no dependency, so
    that parity is UNPINNED -- the tests hold the kernels against a numpy twin.  The reference's ``detect_edges`` uses (50, 200)."""
    n, H, W = _images_u8(gray_u8, "canny_edges: gray_u8")
    ptr = _u8(gray_u8, "gray_u8")
    if out is None:
        out = torch.empty_like(gray_u8)
    elif out.shape != gray_u8.shape:
        raise ValueError("canny_edges: out must have the input's shape")
    workspace, ws_ptr, nbytes = _canny_workspace(workspace, n, H, W, gray_u8.device, "canny_edges")
    _lib.call("lse_canny_u8", ptr, n, H, W, int(low // 1), int(high // 1), ws_ptr, nbytes, _u8(out, "out"), _stream())
    return out


def eval_panels_workspace_bytes(H: int, W: int) -> int:
    v = ctypes.c_int64(0)
    _lib.call("lse_eval_panels_workspace", int(H), int(W), ctypes.byref(v))
    return int(v.value)


def panel_columns(keys) -> int:
    """Width of the grid of ``keys`` in images ("img" counts two)."""
    return sum(2 if k == "img" else 1 for k in PANEL_KEYS if k in keys)


@torch.no_grad()
def eval_panels(keys, H: int, W: int, gt_planes=None, pred_planes=None, rgb=None, pair=None, depth=None, accumulation=None,
                edges=None, ev_out=None, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The uint8 grid [H, columns * W, 3] the reference's ``LSEWriter`` saves as its combined image, in one launch behind a
    two-stage min / max of ``depth`` (lse_eval_panels).  ``keys`` selects among ``PANEL_KEYS``; the columns always come in that order:
    "img" (``gt_planes`` [3, H, W] masked beside ``rgb`` [H * W, 3] unmasked, or the grey ``pair`` = (ground truth, prediction) of
    the event-only metric), "depth" (``depth_gray_map(depth, accumulation)``), "err_map" (``make_error_map`` of ``gt_planes`` and
    ``pred_planes``), "overlay" (from ``edges`` uint8 [2, H, W] = ``canny_edges(gray8_planes(gt_planes, pred_planes))``) and
    "ev_out" ([H, W, 1 or 3]).  Every value is ``clamp(v * 255, 0, 255)`` truncated, v the float32 expression of ``evaluation.py``
    with each operation rounded once; a NaN gives 0.  ``workspace``: float32, ``eval_panels_workspace_bytes`` bytes; its first
    two elements hold the depth's (near, far) afterwards."""
    keys = tuple(keys)
    unknown = [k for k in keys if k not in _PANEL_FLAG]
    if unknown or not keys:
        raise ValueError(f"eval_panels: keys must be a non-empty subset of {PANEL_KEYS}, got {keys}")
    H, W = int(H), int(W)
    flags = 0
    for k in keys:
        flags |= _PANEL_FLAG[k]
    n = H * W

    def want(t, name, numel, dtype=torch.float32):
        if t is None:
            return None
        if t.numel() != numel:
            raise ValueError(f"eval_panels: {name} must hold {numel} elements for a {H} x {W} image, got {tuple(t.shape)}")
        return _chk(t, dtype, name)
    pair_gt, pair_pred = (None, None) if pair is None else pair
    ev_channels = 0
    if ev_out is not None:
        ev_channels = int(ev_out.shape[-1])
        if ev_channels not in (1, 3):
            raise ValueError(f"eval_panels: ev_out must be [H, W, 1] or [H, W, 3], got {tuple(ev_out.shape)}")
    given = [t for t in (gt_planes, pred_planes, rgb, pair_gt, depth, edges, ev_out) if t is not None]
    if not given:
        raise ValueError(f"eval_panels: no input for {keys}")
    device = given[0].device
    cols = panel_columns(keys)
    if out is None:
        out = torch.empty((H, cols * W, 3), dtype=torch.uint8, device=device)
    elif out.numel() != n * cols * 3:
        raise ValueError(f"eval_panels: out must be [{H}, {cols * W}, 3]")
    nbytes = eval_panels_workspace_bytes(H, W)
    if workspace is None:
        workspace = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    elif workspace.numel() * 4 < nbytes:
        raise ValueError(f"eval_panels: workspace of {workspace.numel() * 4} bytes, {nbytes} needed")
    _lib.call("lse_eval_panels", want(gt_planes, "gt_planes", 3 * n), want(pred_planes, "pred_planes", 3 * n), want(rgb, "rgb", 3 * n),
              want(pair_gt, "pair[0]", n), want(pair_pred, "pair[1]", n), want(depth, "depth", n),
              want(accumulation, "accumulation", n), want(edges, "edges", 2 * n, torch.uint8),
              want(ev_out, "ev_out", n * max(ev_channels, 1)), ev_channels, H, W, flags, _f32(workspace, "workspace"), nbytes,
              _u8(out, "out"), _stream())
    return out


# ----------------------------------------------------------------------------------------------------
# training epilogue: routing + mappers + losses
# ----------------------------------------------------------------------------------------------------
def _mapper_mlp_shapes(in_dim: int):
    return [(16, in_dim), (16,), (16, 16), (16,), (16, 16), (16,), (in_dim, 16), (in_dim,)]


def _mapper_mlp_struct(params, grads=None) -> Optional["_lib.MapperMlp"]:
    """lse_mapper_mlp of an MLP intensity mapper: ``params`` = its eight tensors in module order (layers.0.weight, layers.0.bias,
    ... layers.3.bias: nn.Linear layout), ``grads`` = the eight buffers the backward accumulates into."""
    if not params:
        return None
    in_dim = params[0].shape[1]
    if len(params) != 8 or in_dim not in (1, 3) or [tuple(p.shape) for p in params] != _mapper_mlp_shapes(in_dim):
        raise ValueError(f"MLP mapper parameters {[tuple(p.shape) for p in params]}: expected the four nn.Linear layers of "
                         f"MLP(in, num_layers=4, layer_width=16, out=in), in = 1 | 3")
    m = _lib.MapperMlp()
    for l in range(4):
        m.w[l] = _f32(params[2 * l], f"mlp.w[{l}]").value
        m.b[l] = _f32(params[2 * l + 1], f"mlp.b[{l}]").value
        if grads is not None:
            m.dw[l] = _f32(grads[2 * l], f"mlp.dw[{l}]").value
            m.db[l] = _f32(grads[2 * l + 1], f"mlp.db[{l}]").value
    return m


def _mapper_mlp_grads(params):
    """(buffers the kernel accumulates into, what the autograd Function returns for the eight inputs): a parameter whose .grad is
    preallocated (optim.FlatParams) takes its gradient there and the Function returns None for it (``_direct_grad``)."""
    bufs, rets = [], []
    for p in params:
        direct = _direct_grad(p)
        if direct is not None:
            bufs.append(direct)
            rets.append(None)
        else:
            g = torch.zeros_like(p, memory_format=torch.contiguous_format)
            bufs.append(g)
            rets.append(g)
    return bufs, tuple(rets)


def _byref(struct):
    return ctypes.byref(struct) if struct is not None else None


class _LossEpilogueFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, desc_fields, col_rgb, col_gt, prev_rgb, next_rgb, evs_gt, pow_rgb, pow_evs, w31, e_thresh=None, n_mlp_rgb=0,
                *mlp_params):
        dev = (col_rgb if col_rgb is not None else prev_rgb).device
        desc = _lib.EpilogueDesc(*desc_fields)
        group = desc.deblur_group
        n_col = col_rgb.shape[0] // group if col_rgb is not None else 0
        n_ev = prev_rgb.shape[0] if prev_rgb is not None else 0
        if col_rgb is not None and (col_rgb.shape[0] % group != 0 or col_gt.shape[0] != n_col):
            raise ValueError(f"colour bundle of {col_rgb.shape[0]} rays does not split into groups of {group} for {col_gt.shape[0]} targets")
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.call("lse_loss_epilogue_fwd", ctypes.byref(desc), _f32(col_rgb, "col_rgb", True), _f32(col_gt, "col_gt", True),
                  n_col, _f32(prev_rgb, "prev_rgb", True), _f32(next_rgb, "next_rgb", True), _f32(evs_gt, "evs_gt", True),
                  _f32(e_thresh, "e_thresh", True), n_ev, _f32(pow_rgb, "pow_rgb", True), _f32(pow_evs, "pow_evs", True),
                  _f32(w31, "w31", True),
                  _byref(_mapper_mlp_struct(mlp_params[:n_mlp_rgb])), _byref(_mapper_mlp_struct(mlp_params[n_mlp_rgb:])),
                  ctypes.c_void_p(losses.data_ptr()), _stream())
        ctx.save_for_backward(col_rgb, col_gt, prev_rgb, next_rgb, evs_gt, pow_rgb, pow_evs, w31, e_thresh, *mlp_params)
        ctx.desc_fields, ctx.n_col, ctx.n_ev, ctx.n_mlp_rgb = desc_fields, n_col, n_ev, n_mlp_rgb
        ctx.set_materialize_grads(False)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_rgb, g_evs):
        col_rgb, col_gt, prev_rgb, next_rgb, evs_gt, pow_rgb, pow_evs, w31, e_thresh, *mlp_params = ctx.saved_tensors
        dev = (col_rgb if col_rgb is not None else prev_rgb).device
        desc = _lib.EpilogueDesc(*ctx.desc_fields)
        mlp_bufs, mlp_rets = _mapper_mlp_grads(mlp_params)
        k = ctx.n_mlp_rgb
        g_rgb = g_rgb.reshape(1).contiguous().float() if g_rgb is not None else None
        g_evs = g_evs.reshape(1).contiguous().float() if g_evs is not None else None
        d_col = torch.empty_like(col_rgb) if col_rgb is not None else None
        d_prev = torch.empty_like(prev_rgb) if prev_rgb is not None else None
        d_next = torch.empty_like(next_rgb) if next_rgb is not None else None
        d_sc = torch.empty(5, dtype=torch.float32, device=dev)
        _lib.call("lse_loss_epilogue_bwd", ctypes.byref(desc), _f32(col_rgb, "col_rgb", True), _f32(col_gt, "col_gt", True),
                  ctx.n_col, _f32(prev_rgb, "prev_rgb", True), _f32(next_rgb, "next_rgb", True), _f32(evs_gt, "evs_gt", True),
                  _f32(e_thresh, "e_thresh", True), ctx.n_ev, _f32(pow_rgb, "pow_rgb", True), _f32(pow_evs, "pow_evs", True),
                  _f32(w31, "w31", True),
                  _byref(_mapper_mlp_struct(mlp_params[:k], mlp_bufs[:k])), _byref(_mapper_mlp_struct(mlp_params[k:], mlp_bufs[k:])),
                  _f32(g_rgb, "g_rgb_loss", True), _f32(g_evs, "g_event_loss", True), _f32(d_col, "d_col", True),
                  _f32(d_prev, "d_prev", True), _f32(d_next, "d_next", True), ctypes.c_void_p(d_sc.data_ptr()), _stream())
        return (None, d_col, None, d_prev, d_next, None) + _scalar_param_grads(d_sc, pow_rgb, pow_evs, w31) + (None, None) + mlp_rets


def _scalar_param_grads(d_sc, pow_rgb, pow_evs, w31):
    """Gradients of the epilogue's three scalar parameters (d_sc = [d pow_rgb, d pow_evs, d w31[3]]).  A parameter whose .grad is
    already allocated (optim.FlatParams: a view of the flat gradient buffer) is accumulated into HERE and the Function returns None
    for it, like the big parameters (_direct_grad): the step then runs no AccumulateGrad node of a model parameter at all.  That is
    what makes a captured step indifferent to EARLIER eager graphs of the same model that are still alive -- they keep the
    parameters' AccumulateGrad nodes alive, bound to the stream they were created on, and a capture whose backward executed such a
    node left the capturing stream (torch warns; the HIP runtime crashed in hipStreamEndCapture, round 4)."""
    out = []
    for p, lo, hi in ((pow_rgb, 0, 1), (pow_evs, 1, 2), (w31, 2, 5)):
        if p is None:
            out.append(None)
            continue
        g = d_sc[lo:hi].view_as(p)
        direct = _direct_grad(p)
        if direct is not None:
            direct.add_(g)
            out.append(None)
        else:
            out.append(g)
    return tuple(out)


class _LossEpiloguePackedFn(torch.autograd.Function):
    """``_LossEpilogueFn`` on the render of ONE packed pass: ``rgb_all`` [n_col_rays + 2 n_ev, 3] holds the colour, previous-event and
    next-event bundles' rows one after the other (LSENeRFModel.train_step_bundles).  The three parts are handed to the kernels as
    pointers into that one buffer, and the backward fills ONE gradient buffer -- the per-bundle slices of the generic route cost, in
    backward, a zero-fill + a copy per bundle and two adds (eight ~5 us launches per step in the rocprofv3 timeline of a replayed
    3-bundle step, tools/graph_timeline.py)."""

    @staticmethod
    def forward(ctx, desc_fields, rgb_all, n_col_rays, n_ev, col_gt, evs_gt, pow_rgb, pow_evs, w31, e_thresh=None, n_mlp_rgb=0,
                *mlp_params):
        dev = rgb_all.device
        desc = _lib.EpilogueDesc(*desc_fields)
        group = desc.deblur_group
        if n_col_rays % group != 0 or (n_col_rays and col_gt.shape[0] != n_col_rays // group):
            raise ValueError(f"colour bundle of {n_col_rays} rays does not split into groups of {group} for "
                             f"{0 if col_gt is None else col_gt.shape[0]} targets")
        if rgb_all.shape[0] != n_col_rays + 2 * n_ev:
            raise ValueError(f"packed render of {rgb_all.shape[0]} rays for {n_col_rays} colour + 2 x {n_ev} event rays")
        col = rgb_all[:n_col_rays] if n_col_rays else None
        prev = rgb_all[n_col_rays:n_col_rays + n_ev] if n_ev else None
        nxt = rgb_all[n_col_rays + n_ev:] if n_ev else None
        losses = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.call("lse_loss_epilogue_fwd", ctypes.byref(desc), _f32(col, "col_rgb", True), _f32(col_gt, "col_gt", True),
                  n_col_rays // group, _f32(prev, "prev_rgb", True), _f32(nxt, "next_rgb", True), _f32(evs_gt, "evs_gt", True),
                  _f32(e_thresh, "e_thresh", True), n_ev, _f32(pow_rgb, "pow_rgb", True), _f32(pow_evs, "pow_evs", True),
                  _f32(w31, "w31", True),
                  _byref(_mapper_mlp_struct(mlp_params[:n_mlp_rgb])), _byref(_mapper_mlp_struct(mlp_params[n_mlp_rgb:])),
                  ctypes.c_void_p(losses.data_ptr()), _stream())
        ctx.save_for_backward(rgb_all, col_gt, evs_gt, pow_rgb, pow_evs, w31, e_thresh, *mlp_params)
        ctx.desc_fields, ctx.n_col_rays, ctx.n_ev, ctx.n_mlp_rgb = desc_fields, n_col_rays, n_ev, n_mlp_rgb
        ctx.set_materialize_grads(False)
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_rgb, g_evs):
        rgb_all, col_gt, evs_gt, pow_rgb, pow_evs, w31, e_thresh, *mlp_params = ctx.saved_tensors
        dev = rgb_all.device
        desc = _lib.EpilogueDesc(*ctx.desc_fields)
        mlp_bufs, mlp_rets = _mapper_mlp_grads(mlp_params)
        k = ctx.n_mlp_rgb
        n0, ne = ctx.n_col_rays, ctx.n_ev
        g_rgb = g_rgb.reshape(1).contiguous().float() if g_rgb is not None else None
        g_evs = g_evs.reshape(1).contiguous().float() if g_evs is not None else None
        d_all = torch.empty_like(rgb_all)          # every row belongs to exactly one part, and the kernel overwrites its parts
        part = lambda t, a, b: (t[a:b] if b > a else None)
        _lib.call("lse_loss_epilogue_bwd", ctypes.byref(desc), _f32(part(rgb_all, 0, n0), "col_rgb", True), _f32(col_gt, "col_gt", True),
                  n0 // desc.deblur_group, _f32(part(rgb_all, n0, n0 + ne), "prev_rgb", True),
                  _f32(part(rgb_all, n0 + ne, n0 + 2 * ne), "next_rgb", True), _f32(evs_gt, "evs_gt", True),
                  _f32(e_thresh, "e_thresh", True), ne,
                  _f32(pow_rgb, "pow_rgb", True), _f32(pow_evs, "pow_evs", True), _f32(w31, "w31", True),
                  _byref(_mapper_mlp_struct(mlp_params[:k], mlp_bufs[:k])), _byref(_mapper_mlp_struct(mlp_params[k:], mlp_bufs[k:])),
                  _f32(g_rgb, "g_rgb_loss", True), _f32(g_evs, "g_event_loss", True), _f32(part(d_all, 0, n0), "d_col", True),
                  _f32(part(d_all, n0, n0 + ne), "d_prev", True), _f32(part(d_all, n0 + ne, n0 + 2 * ne), "d_next", True),
                  ctypes.c_void_p((d_sc := torch.empty(5, dtype=torch.float32, device=dev)).data_ptr()), _stream())
        return (None, d_all, None, None, None, None) + _scalar_param_grads(d_sc, pow_rgb, pow_evs, w31) + (None, None) + mlp_rets


def _event_thresholds(e_thresh, n_ev: int, like):
    """evs_batch["e_thresh"] (a number, a 1-element tensor or one value per event ray, R:lse_nerf/lse_pixel_sampler.py:36-37) as the
    [n_ev] float vector of lse_loss_epilogue_*; None stays None (= 1)."""
    if e_thresh is None or like is None:
        return None
    if not torch.is_tensor(e_thresh):      # a number: a fill kernel (capturable), not a host-to-device copy
        return torch.full((n_ev,), float(e_thresh), dtype=torch.float32, device=like.device)
    t = e_thresh.to(device=like.device, dtype=torch.float32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(n_ev)
    if t.numel() != n_ev:
        raise ValueError(f"e_thresh holds {t.numel()} values for {n_ev} event rays")
    return t.contiguous()


def loss_epilogue_packed(desc_fields: tuple, rgb_all, n_col_rays: int, n_ev: int, col_gt, evs_gt, pow_rgb=None, pow_evs=None, w31=None,
                         mlp_rgb=(), mlp_evs=(), e_thresh=None):
    """``loss_epilogue`` for the bundles of one packed pass, given as row blocks [colour | previous | next] of ONE render."""
    c = lambda t: _c(t.float()) if t is not None else None
    return _LossEpiloguePackedFn.apply(tuple(desc_fields), c(rgb_all), int(n_col_rays), int(n_ev), c(col_gt),
                                       c(evs_gt.reshape(-1)) if evs_gt is not None else None, pow_rgb, pow_evs, w31,
                                       _event_thresholds(e_thresh, int(n_ev), evs_gt), len(mlp_rgb), *mlp_rgb, *mlp_evs)


def loss_epilogue(desc_fields: tuple, col_rgb, col_gt, prev_rgb, next_rgb, evs_gt, pow_rgb=None, pow_evs=None, w31=None,
                  mlp_rgb=(), mlp_evs=(), e_thresh=None):
    """Routing + intensity mappers + rgb MSE + log-intensity event MSE in one launch (lse_loss_epilogue_fwd).
    ``desc_fields`` = (rgb_mapped, rgb_mapper, evs_mapper, ev_one_dim, deblur_group, evs_loss_weight[, event_loss_kind]).
    ``e_thresh``: evs_batch["e_thresh"] for event_loss_kind = LSE_EVLOSS_ENERF_NORM (R:lse_nerf/lsenerf.py:406-419).
    ``mlp_rgb`` / ``mlp_evs``: the eight parameters (module order) of an MLP mapper on the colour / event side (kinds LSE_MAP_MLP,
    LSE_MAP_RGB_MLP; R:lse_nerf/intensity_mappers.py:28-62).  Returns (rgb_loss, event_loss) as 0-dim tensors."""
    c = lambda t: _c(t.float()) if t is not None else None
    return _LossEpilogueFn.apply(tuple(desc_fields), c(col_rgb), c(col_gt), c(prev_rgb), c(next_rgb),
                                 c(evs_gt.reshape(-1)) if evs_gt is not None else None, pow_rgb, pow_evs, w31,
                                 _event_thresholds(e_thresh, prev_rgb.shape[0] if prev_rgb is not None else 0, evs_gt),
                                 len(mlp_rgb), *mlp_rgb, *mlp_evs)


# ----------------------------------------------------------------------------------------------------
# optimiser / occupancy grid
# ----------------------------------------------------------------------------------------------------
@torch.no_grad()
def adam_step(params, grads, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step: int, grad_scale: float = 1.0):
    # (the scalars go as doubles: 1 - beta2 taken from a float beta2 is 1.3e-5 off, and exp_avg_sq with it -- lse_hip.h)
    _lib.call("lse_adam_step_f64", _f32(params, "params"), _f32(grads, "grads"), _f32(exp_avg, "exp_avg"),
              _f32(exp_avg_sq, "exp_avg_sq"), params.numel(), float(lr), float(beta1), float(beta2), float(eps),
              int(step), float(grad_scale), _stream())


@torch.no_grad()
def adam_step_dev(params, grads, exp_avg, exp_avg_sq, hyper, grad_scale: float = 1.0, sched=None):
    """Adam with every scalar of the step -- lr, 1 - beta1^t, 1 / sqrt(1 - beta2^t), beta1, beta2, eps -- in ``hyper`` (float32 [6]
    on the device, written by ``adam_schedule_dev``).  ``sched``: the float64 [6] constants ``adam_schedule_dev`` read; 1 - beta
    is then taken from its double betas (lse_adam_step_dev_sched), as the bias corrections in ``hyper`` were."""
    if sched is None:
        _lib.call("lse_adam_step_dev", _f32(params, "params"), _f32(grads, "grads"), _f32(exp_avg, "exp_avg"),
                  _f32(exp_avg_sq, "exp_avg_sq"), params.numel(), _f32(hyper, "hyper"), float(grad_scale), _stream())
        return
    if sched.numel() < 6:
        raise ValueError("adam_step_dev: sched holds six doubles")
    _lib.call("lse_adam_step_dev_sched", _f32(params, "params"), _f32(grads, "grads"), _f32(exp_avg, "exp_avg"),
              _f32(exp_avg_sq, "exp_avg_sq"), params.numel(), _f32(hyper, "hyper"), _chk(sched, torch.float64, "sched"),
              float(grad_scale), _stream())


@torch.no_grad()
def adam_schedule_dev(step_dev, hyper, sched):
    """Advance the device-side optimizer step counter (int64 [1]) and write the six scalars of the new step into ``hyper``
    (float32 [6]) from the schedule constants ``sched`` (float64 [6] on the device: lr_init, lr_final, max_steps, beta1, beta2,
    eps) -- lse_adam_schedule_dev; capturable, reads nothing from the host."""
    _lib.call("lse_adam_schedule_dev", _chk(step_dev, torch.int64, "step_dev"), _f32(hyper, "hyper"),
              _chk(sched, torch.float64, "sched"), _stream())


@torch.no_grad()
def occ_update_cells(occs, cell_ids, occ_new, ema_decay: float):
    n = cell_ids.shape[0]
    ws = torch.empty(n, dtype=torch.float32, device=occs.device)
    _lib.call("lse_occ_update_cells", _f32(occs, "occs"), _chk(cell_ids, torch.int64, "cell_ids"),
              _f32(occ_new, "occ_new"), n, float(ema_decay), ctypes.c_void_p(ws.data_ptr()), _stream())


@torch.no_grad()
def occ_binarize(occs, threshold: torch.Tensor, binaries_u8):
    _lib.call("lse_occ_binarize", _f32(occs, "occs"), occs.numel(), _f32(threshold, "threshold"),
              _chk(binaries_u8, torch.uint8, "binaries"), _stream())


# ---- count-free occupancy refresh (csrc/occ_refresh.hip; driven by lsenerf_amd.occ_refresh.DeviceGridRefresher) ----
def occ_list_tiles(cells: int) -> int:
    return (int(cells) + _lib.LSE_OCC_LIST_TILE - 1) // _lib.LSE_OCC_LIST_TILE


@torch.no_grad()
def occ_list_occupied(binaries_u8, cell_list, counts, workspace):
    """Per level the ascending indices of the set cells of ``binaries_u8`` [L, C] into ``cell_list`` (int32 [L, C]) and their number
    into ``counts`` (int64 [L]): ``torch.nonzero(binaries[l])[:, 0]`` without a host-known size.  ``workspace``: int32
    [L * occ_list_tiles(C)]."""
    levels, cells = binaries_u8.shape
    if cell_list.shape != (levels, cells) or counts.numel() != levels or workspace.numel() < levels * occ_list_tiles(cells):
        raise ValueError("occ_list_occupied: list [L, C], counts [L] and workspace [L * tiles] do not fit binaries [L, C]")
    _lib.call("lse_occ_list_occupied", _chk(binaries_u8, torch.uint8, "binaries"), levels, cells,
              _chk(cell_list, torch.int32, "cell_list"), _chk(counts, torch.int64, "counts"),
              _chk(workspace, torch.int32, "workspace"), _stream())


@torch.no_grad()
def occ_draw_cells(occs, cell_list, counts, aabbs, level: int, cells: int, res, warmup: bool, step_dev, seed: int, cell_ids,
                   positions, n_dev):
    """Cells and jittered positions of one level's refresh (lse_occ_draw_cells; spec: occ_refresh.draw_cells_host).  ``cell_ids``
    int64 [cap], ``positions`` float32 [cap, 3], ``n_dev`` int64 [1] are written; ``step_dev`` int64 [1] is read on the device."""
    cap = cell_ids.shape[0]
    if positions.shape != (cap, 3) or occs.numel() < (level + 1) * cells or aabbs.shape[0] <= level:
        raise ValueError("occ_draw_cells: positions must be [cap, 3]; occs / aabbs must cover the level")
    _lib.call("lse_occ_draw_cells", _f32(occs, "occs"), _chk(cell_list, torch.int32, "cell_list", True),
              _chk(counts, torch.int64, "counts", True), _f32(aabbs, "aabbs"), int(level), int(cells), int(res[0]), int(res[1]),
              int(res[2]), int(bool(warmup)), _chk(step_dev, torch.int64, "step_dev"), int(seed) & 0xFFFFFFFFFFFFFFFF, cap,
              _chk(cell_ids, torch.int64, "cell_ids"), _f32(positions, "positions"), _chk(n_dev, torch.int64, "n_dev"), _stream())


@torch.no_grad()
def occ_update_cells_dev(occs, cell_ids, sigma, step_size: float, n_dev, ema_decay: float, workspace):
    """``occ_update_cells`` on the leading ``n_dev[0]`` entries with ``occ_new = sigma * step_size``; ids < 0 are skipped."""
    cap = cell_ids.shape[0]
    if sigma.numel() < cap or workspace.numel() < cap:
        raise ValueError("occ_update_cells_dev: sigma and workspace need one entry per slot")
    _lib.call("lse_occ_update_cells_dev", _f32(occs, "occs"), _chk(cell_ids, torch.int64, "cell_ids"), _f32(sigma, "sigma"),
              float(step_size), _chk(n_dev, torch.int64, "n_dev"), cap, float(ema_decay), _f32(workspace, "workspace"), _stream())


@torch.no_grad()
def occ_mean_threshold(occs, occ_thre: float, workspace, mean_all, threshold):
    """``mean_all[0] = occs.mean()`` and ``threshold[0] = min(occs[occs >= 0].mean(), occ_thre)``, both float32 on the device, from
    one deterministic double-precision reduction.  ``workspace``: float64 [3 * LSE_OCC_MEAN_BLOCKS]."""
    if workspace.numel() < 3 * _lib.LSE_OCC_MEAN_BLOCKS:
        raise ValueError("occ_mean_threshold: workspace needs 3 * LSE_OCC_MEAN_BLOCKS doubles")
    _lib.call("lse_occ_mean_threshold", _f32(occs, "occs"), occs.numel(), float(occ_thre), _chk(workspace, torch.float64, "workspace"),
              _f32(mean_all, "mean_all"), _f32(threshold, "threshold"), _stream())


# ---- mesh export (csrc/mesh.hip; driven by lsenerf_amd.mesh.extract_mesh) ----
def _res3(res) -> Tuple[int, int, int]:
    r = tuple(int(v) for v in res) if hasattr(res, "__len__") else (int(res),) * 3
    if len(r) != 3:
        raise ValueError(f"resolution {res!r}: an int or three ints expected")
    return r


def _box3(lo, hi):
    lo, hi = [float(v) for v in lo], [float(v) for v in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo and hi: three floats each expected")
    return (ctypes.c_float * 3)(*lo), (ctypes.c_float * 3)(*hi)


def lattice_points(res) -> int:
    nx, ny, nz = _res3(res)
    return (nx + 1) * (ny + 1) * (nz + 1)


@torch.no_grad()
def lattice_positions(res, lo, hi, first: int = 0, n: Optional[int] = None, out: Optional[torch.Tensor] = None,
                      device="cuda") -> torch.Tensor:
    """World positions [n, 3] of the lattice points ``first .. first + n`` of a ``res = (nx, ny, nz)``-cell lattice over the box
    ``lo .. hi`` (lse_lattice_positions; point order and arithmetic: include/lse_hip.h, "mesh export").  ``n`` defaults to the rest
    of the lattice; ``out``: a float32 [n, 3] buffer to write into."""
    nx, ny, nz = _res3(res)
    first = int(first)
    n = lattice_points(res) - first if n is None else int(n)
    if out is None:
        out = torch.empty((max(n, 0), 3), dtype=torch.float32, device=device)
    elif out.shape != (n, 3):
        raise ValueError("lattice_positions: out [n, 3] expected")
    c_lo, c_hi = _box3(lo, hi)
    _lib.call("lse_lattice_positions", c_lo, c_hi, nx, ny, nz, first, n, _f32(out, "out") if n > 0 else None, _stream())
    return out


def surface_nets_workspace_bytes(res) -> int:
    v = ctypes.c_int64(0)
    _lib.call("lse_surface_nets_workspace", *_res3(res), ctypes.byref(v))
    return int(v.value)


@torch.no_grad()
def surface_nets_count(sigma: torch.Tensor, res, level: float, workspace: torch.Tensor, totals: torch.Tensor,
                       skip_nan: bool = False) -> None:
    """First pass of ``surface_nets``: fills ``workspace`` (uint8, ``surface_nets_workspace_bytes(res)``) and ``totals`` (int64 [2] on
    the device: vertices, quads).  No host read.  ``skip_nan``: lse_surface_nets_count_ex with LSE_NETS_SKIP_NAN."""
    if sigma.numel() != lattice_points(res):
        raise ValueError(f"surface_nets: sigma has {sigma.numel()} values, the lattice {lattice_points(res)} points")
    name, flags = ("lse_surface_nets_count_ex", (_lib.LSE_NETS_SKIP_NAN,)) if skip_nan else ("lse_surface_nets_count", ())
    _lib.call(name, _f32(sigma, "sigma"), *_res3(res), float(level), *flags, _chk(workspace, torch.uint8, "workspace"),
              workspace.numel(), _chk(totals, torch.int64, "totals"), _stream())


@torch.no_grad()
def surface_nets_emit(sigma: torch.Tensor, res, lo, hi, level: float, workspace: torch.Tensor, vertices: torch.Tensor,
                      triangles: torch.Tensor, skip_nan: bool = False) -> None:
    """Second pass of ``surface_nets`` with the workspace ``surface_nets_count`` filled for the same ``sigma``, ``res``, ``level`` and
    ``skip_nan``: writes ``vertices`` (float32 [cap_vertices, 3]) and ``triangles`` (int32 [2 * cap_quads, 3]); rows beyond a buffer
    are dropped."""
    if sigma.numel() != lattice_points(res):
        raise ValueError(f"surface_nets: sigma has {sigma.numel()} values, the lattice {lattice_points(res)} points")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or triangles.dim() != 2 or triangles.shape[1] != 3 or triangles.shape[0] % 2:
        raise ValueError("surface_nets: vertices [cap_vertices, 3] and triangles [2 * cap_quads, 3] expected")
    c_lo, c_hi = _box3(lo, hi)
    cap_v, cap_q = vertices.shape[0], triangles.shape[0] // 2
    name, flags = ("lse_surface_nets_emit_ex", (_lib.LSE_NETS_SKIP_NAN,)) if skip_nan else ("lse_surface_nets_emit", ())
    _lib.call(name, _f32(sigma, "sigma"), *_res3(res), c_lo, c_hi, float(level), *flags,
              _chk(workspace, torch.uint8, "workspace"), workspace.numel(), cap_v, cap_q,
              _f32(vertices, "vertices") if cap_v else None, _chk(triangles, torch.int32, "triangles") if cap_q else None, _stream())


@torch.no_grad()
def surface_nets(sigma: torch.Tensor, res, lo, hi, level: float, caps: Optional[Tuple[int, int]] = None, skip_nan: bool = False):
    """Naive surface nets of the density lattice ``sigma`` (float32, one value per point of the ``res``-cell lattice over the box
    ``lo .. hi``, iz fastest) at the iso value ``level``: ``(vertices [V, 3] float32, triangles [2 Q, 3] int32, totals int64 [2])``.
    The definition -- one vertex per active cell, one quad per sign-changing interior lattice edge, ordered, deterministic -- is in
    include/lse_hip.h ("mesh export").  Without ``caps`` the buffers are sized from ONE host read of ``totals`` between the two
    passes; with ``caps = (cap_vertices, cap_quads)`` nothing is read, the buffers have the capacities' extent, rows beyond the true
    counts are left unwritten and ``totals`` (on the device) says how many there are.  ``skip_nan`` (LSE_NETS_SKIP_NAN; include/lse_hip.h,
    "TSDF fusion"): NaN marks unobserved points -- a cell with a NaN corner gives no vertex and a quad next to such a cell is
    dropped, so no surface is built against unobserved space."""
    sigma = _c(sigma.detach()).reshape(-1)
    dev = sigma.device
    ws = torch.empty(surface_nets_workspace_bytes(res), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    surface_nets_count(sigma, res, level, ws, totals, skip_nan)
    if caps is None:
        n_v, n_q = (int(v) for v in totals.tolist())
    else:
        n_v, n_q = int(caps[0]), int(caps[1])
    vertices = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
    triangles = torch.empty((2 * n_q, 3), dtype=torch.int32, device=dev)
    surface_nets_emit(sigma, res, lo, hi, level, ws, vertices, triangles, skip_nan)
    return vertices, triangles, totals


@torch.no_grad()
def point_normals_world(d_x01: torch.Tensor, positions: torch.Tensor, contraction: bool = True, aabb6=None,
                        out: Optional[torch.Tensor] = None, n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """World-space normals [n, 3] at ``positions`` from ``d_x01`` (``LSEField.normals_packed``): the gradient through the transposed
    Jacobian of the position map (``contraction`` or ``aabb6`` as ``positions`` takes them), then ``-g / max(|g|, 1e-12)`` -- unit
    vectors, zero where the gradient is or the point lies outside the field's domain (lse_point_normals_world)."""
    n = d_x01.shape[0]
    if d_x01.shape != (n, 3) or positions.shape != (n, 3):
        raise ValueError("point_normals_world: d_x01 and positions [n, 3] expected")
    if not contraction and aabb6 is None:
        raise ValueError("point_normals_world: aabb normalisation needs aabb6")
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=d_x01.device)
    elif out.shape != (n, 3):
        raise ValueError("point_normals_world: out [n, 3] expected")
    aabb_arr = None if aabb6 is None else (ctypes.c_float * 6)(*[float(v) for v in aabb6])
    if n > 0:
        _call_n("lse_point_normals_world", n_dev, _f32(d_x01, "d_x01"), _f32(positions, "positions"), 1 if contraction else 0, aabb_arr,
                n, _f32(out, "out"), _stream())
    return out


# ---- TSDF fusion (csrc/tsdf.hip; driven by lsenerf_amd.tsdf.export_tsdf_mesh) ----
def _tsdf_ptrs(*specs):
    """Pointers of contiguous float32 device tensors, one per spec ``(tensor, shape, name, allow_none)``.  Every violation is a
    ValueError; dtype, shape and contiguity of ALL tensors are checked before the device of any."""
    for t, shape, name, allow_none in specs:
        if t is None:
            if allow_none:
                continue
            raise ValueError(f"{name} is None")
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{name}: a float32 tensor expected, got {getattr(t, 'dtype', type(t))}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: {list(shape)} expected, got {list(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    for t, _, name, _ in specs:
        if t is not None and not t.is_cuda:
            raise ValueError(f"{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback")
    return [ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None for t, _, _, _ in specs]


@torch.no_grad()
def tsdf_integrate(tw: torch.Tensor, cw: Optional[torch.Tensor], res, lo, hi, cam_desc, poses: torch.Tensor, depth: torch.Tensor,
                   acc: torch.Tensor, rgb: Optional[torch.Tensor] = None, truncation: float = 0.0, min_acc: float = 0.5,
                   carve: bool = True, r2_max: float = float("inf")) -> None:
    """Folds the views ``poses`` [V, 3, 4] (rows of a device pose table) of the camera ``cam_desc`` (``camera_desc``) into the TSDF
    state ``tw`` [points, 2] = (tsdf, weight) and, with ``cw`` [points, 4] = (r, g, b, weight) and ``rgb`` [V, H * W, 3], the fused
    colours, in place and in view order (lse_tsdf_integrate; the update is in include/lse_hip.h, "TSDF fusion").  ``depth``, ``acc``:
    [V, H * W].  One launch for the batch: the state is read and written once however many views it holds.  No host read."""
    import math
    n = lattice_points(res)
    hw = int(cam_desc.H) * int(cam_desc.W)
    truncation = float(truncation)
    if not (truncation > 0.0 and math.isfinite(truncation)):
        raise ValueError(f"truncation must be positive and finite, got {truncation}")
    if not torch.is_tensor(poses) or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"poses: [V, 3, 4] expected, got {list(getattr(poses, 'shape', ()))}")
    V = poses.shape[0]
    p_tw, p_cw, p_poses, p_depth, p_acc, p_rgb = _tsdf_ptrs(
        (tw, (n, 2), "tw", False), (cw, (n, 4), "cw", True), (poses, (V, 3, 4), "poses", False), (depth, (V, hw), "depth", False),
        (acc, (V, hw), "acc", False), (rgb, (V, hw, 3), "rgb", True))
    c_lo, c_hi = _box3(lo, hi)
    _lib.call("lse_tsdf_integrate", p_tw, p_cw, *_res3(res), c_lo, c_hi, ctypes.byref(cam_desc), p_poses, V, p_depth, p_acc, p_rgb,
              truncation, float(min_acc), 1 if carve else 0, float(r2_max), _stream())


@torch.no_grad()
def tsdf_vertex_colors(cw: torch.Tensor, res, lo, hi, vertices: torch.Tensor, out: Optional[torch.Tensor] = None,
                       n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Fused colours [n, 3] at ``vertices`` [n, 3]: the trilinear blend of the colours ``cw`` [points, 4] holds at the 8 corners of
    each vertex's cell, over the corners with a colour weight > 0 (black where none has) -- lse_tsdf_vertex_colors.  ``n_dev``
    (int64 [1] on the device): only the first ``n_dev[0]`` rows are written."""
    if not torch.is_tensor(vertices) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"vertices: [n, 3] expected, got {list(getattr(vertices, 'shape', ()))}")
    n = vertices.shape[0]
    if out is None:
        out = torch.empty((n, 3), dtype=torch.float32, device=vertices.device)
    c_ptr, v_ptr, o_ptr = _tsdf_ptrs((cw, (lattice_points(res), 4), "cw", False), (vertices, (n, 3), "vertices", False),
                                     (out, (n, 3), "out", False))
    c_lo, c_hi = _box3(lo, hi)
    _call_n("lse_tsdf_vertex_colors", n_dev, c_ptr, *_res3(res), c_lo, c_hi, v_ptr, n, o_ptr, _stream())
    return out


# ---- point-cloud export (csrc/pointcloud.hip; driven by lsenerf_amd.pointcloud.export_point_cloud) ----
PC_MAX_AXIS = 1 << 20      # voxels per axis lse_voxel_keys accepts


def _rows3(t: Optional[torch.Tensor], n: int, name: str, allow_none: bool = False):
    """Pointer of a float32 ``[n, 3]`` tensor."""
    ptr = _f32(t, name, allow_none)
    if t is not None and tuple(t.shape) != (n, 3):
        raise ValueError(f"{name}: [{n}, 3] expected, got {tuple(t.shape)}")
    return ptr


def _vec(t: Optional[torch.Tensor], dtype, n: int, name: str, allow_none: bool = False):
    ptr = _chk(t, dtype, name, allow_none)
    if t is not None and tuple(t.shape) != (n,):
        raise ValueError(f"{name}: [{n}] expected, got {tuple(t.shape)}")
    return ptr


def _count1(t: Optional[torch.Tensor], name: str, allow_none: bool = False):
    ptr = _chk(t, torch.int64, name, allow_none)
    if t is not None and t.numel() != 1:
        raise ValueError(f"{name}: one int64 on the device expected")
    return ptr


def _pc_workspace_bytes(fn: str, n: int) -> int:
    v = ctypes.c_int64(0)
    _lib.call(fn, int(n), ctypes.byref(v))
    return int(v.value)


def unproject_workspace_bytes(n_rays: int) -> int:
    return _pc_workspace_bytes("lse_unproject_workspace", n_rays)


def voxel_merge_workspace_bytes(n: int) -> int:
    return _pc_workspace_bytes("lse_voxel_merge_workspace", n)


def voxel_support_workspace_bytes(m: int) -> int:
    return _pc_workspace_bytes("lse_voxel_support_workspace", m)


def _pc_workspace(fn: str, n: int, workspace: Optional[torch.Tensor], dev):
    """(tensor, pointer, bytes) of a compaction workspace for an extent of ``n``: the caller's (uint8) or a fresh one."""
    if workspace is None:
        workspace = torch.empty(_pc_workspace_bytes(fn, n), dtype=torch.uint8, device=dev)
    ptr = _chk(workspace, torch.uint8, "workspace")
    return workspace, (ptr if workspace.numel() else None), workspace.numel()


def voxel_lattice(lo, hi, voxel_size: float) -> Tuple[int, int, int]:
    """Voxels per axis of the box ``lo .. hi`` at ``voxel_size``: ``max(1, ceil((hi_k - lo_k) / voxel_size))`` in double.
    ValueError: a size that is not positive and finite, a count above 2^20 (lse_voxel_keys' limit).  Pure host code."""
    import math
    v = float(voxel_size)
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"voxel_size must be positive and finite, got {voxel_size}")
    res = tuple(max(1, int(math.ceil((float(h) - float(l)) / v))) for l, h in zip(lo, hi))
    if len(res) != 3:
        raise ValueError("lo and hi: three floats each expected")
    if max(res) > PC_MAX_AXIS:
        raise ValueError(f"voxel_size {v} over {list(lo)} .. {list(hi)} gives a lattice of {res}: more than 2^20 voxels on an axis")
    return res


@torch.no_grad()
def unproject_append(origins: torch.Tensor, directions: torch.Tensor, depth: torch.Tensor, acc: torch.Tensor, lo, hi,
                     min_acc: float, out_points: torch.Tensor, total: torch.Tensor, colors: Optional[torch.Tensor] = None,
                     normals: Optional[torch.Tensor] = None, out_colors: Optional[torch.Tensor] = None,
                     out_normals: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> None:
    """Appends the valid rays' points ``o + d * depth`` (and their ``colors`` / ``normals`` rows) to ``out_points`` (``out_colors``,
    ``out_normals``; float32 [cap, 3]) behind row ``total[0]`` in ray order and adds their number to ``total`` (int64 [1] on the
    device) -- lse_unproject_append; the validity rule is in include/lse_hip.h ("point-cloud export").  Rows beyond ``cap`` are
    dropped while ``total`` keeps counting.  No host read."""
    n = origins.shape[0]
    args = [_rows3(origins, n, "origins"), _rows3(directions, n, "directions"), _vec(depth, torch.float32, n, "depth"),
            _vec(acc, torch.float32, n, "acc"), _rows3(colors, n, "colors", True), _rows3(normals, n, "normals", True)]
    cap = out_points.shape[0]
    outs = [_rows3(out_points, cap, "out_points"), _rows3(out_colors, cap, "out_colors", True),
            _rows3(out_normals, cap, "out_normals", True), _count1(total, "total")]
    if (out_colors is not None and colors is None) or (out_normals is not None and normals is None):
        raise ValueError("unproject_append: an output without its input")
    c_lo, c_hi = _box3(lo, hi)
    _, ws, ws_bytes = _pc_workspace("lse_unproject_workspace", n, workspace, origins.device)
    _lib.call("lse_unproject_append", *args, n, c_lo, c_hi, float(min_acc), ws, ws_bytes, cap, *(o if cap else None for o in outs[:3]),
              outs[3], _stream())


@torch.no_grad()
def voxel_keys(points: torch.Tensor, lo, voxel_size: float, res, n_dev: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """int64 [n] voxel keys ``(vx * ny + vy) * nz + vz`` of ``points`` [n, 3] on the ``res = (nx, ny, nz)`` lattice of ``voxel_size``
    cells from ``lo`` (coordinates clamped into the lattice); rows at or beyond ``n_dev[0]`` get INT64_MAX, so a stable sort leaves
    them last (lse_voxel_keys)."""
    n = points.shape[0]
    p = _rows3(points, n, "points")
    nd = _count1(n_dev, "n_dev", True)
    if out is None:
        out = torch.empty(n, dtype=torch.int64, device=points.device)
    k = _vec(out, torch.int64, n, "out")
    nx, ny, nz = _res3(res)
    c_lo, _ = _box3(lo, lo)
    _lib.call("lse_voxel_keys", p if n else None, n, nd, c_lo, float(voxel_size), nx, ny, nz, k if n else None, _stream())
    return out


@torch.no_grad()
def voxel_merge(sorted_keys: torch.Tensor, order: torch.Tensor, points: torch.Tensor, colors: Optional[torch.Tensor] = None,
                normals: Optional[torch.Tensor] = None, cap: Optional[int] = None, workspace: Optional[torch.Tensor] = None):
    """One point per voxel from a cloud sorted by key (``sorted_keys, order = torch.sort(keys, stable=True)``): ``(keys int64 [cap],
    counts int32 [cap], points, colors | None, normals | None [cap, 3], total int64 [1])`` -- means in run order, normals
    renormalised, voxels in ascending key (lse_voxel_merge).  ``cap`` defaults to n; rows at or beyond ``total[0]`` are unwritten.
    No host read."""
    n = sorted_keys.shape[0]
    args = [_vec(sorted_keys, torch.int64, n, "sorted_keys"), _vec(order, torch.int64, n, "order"), _rows3(points, n, "points"),
            _rows3(colors, n, "colors", True), _rows3(normals, n, "normals", True)]
    cap = n if cap is None else int(cap)
    if cap < 0:
        raise ValueError("voxel_merge: negative capacity")
    dev = points.device
    new3 = lambda src: None if src is None else torch.empty((cap, 3), dtype=torch.float32, device=dev)
    out_keys = torch.empty(cap, dtype=torch.int64, device=dev)
    out_counts = torch.empty(cap, dtype=torch.int32, device=dev)
    out_p, out_c, out_n = new3(points), new3(colors), new3(normals)
    total = torch.empty(1, dtype=torch.int64, device=dev)
    _, ws, ws_bytes = _pc_workspace("lse_voxel_merge_workspace", n, workspace, dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if (t is not None and t.numel()) else None
    _lib.call("lse_voxel_merge", *(a if n else None for a in args), n, ws, ws_bytes, cap, ptr(out_keys), ptr(out_counts), ptr(out_p),
              ptr(out_c), ptr(out_n), ptr(total), _stream())
    return out_keys, out_counts, out_p, out_c, out_n, total


@torch.no_grad()
def voxel_support_filter(keys: torch.Tensor, counts: torch.Tensor, points: torch.Tensor, res, min_support: int,
                         colors: Optional[torch.Tensor] = None, normals: Optional[torch.Tensor] = None,
                         m_dev: Optional[torch.Tensor] = None, cap: Optional[int] = None, want_support: bool = False,
                         workspace: Optional[torch.Tensor] = None):
    """Keeps the voxels whose 3 x 3 x 3 neighbourhood on the ``res`` lattice holds at least ``min_support`` raw points (the sum of
    ``counts`` over the present neighbours, the voxel included): ``(keys, counts, points, colors | None, normals | None, total int64
    [1], support int32 [m] | None)``, compacted in order (lse_voxel_support_filter).  ``keys`` ascending and unique, as
    ``voxel_merge`` writes them; ``m_dev``: device count of the present voxels (``voxel_merge``'s total).  No host read."""
    m = keys.shape[0]
    args = [_vec(keys, torch.int64, m, "keys"), _vec(counts, torch.int32, m, "counts"), _rows3(points, m, "points"),
            _rows3(colors, m, "colors", True), _rows3(normals, m, "normals", True)]
    md = _count1(m_dev, "m_dev", True)
    cap = m if cap is None else int(cap)
    if cap < 0:
        raise ValueError("voxel_support_filter: negative capacity")
    min_support = int(min_support)
    if not -(1 << 31) <= min_support < (1 << 31):
        raise ValueError("voxel_support_filter: min_support must fit an int32")
    nx, ny, nz = _res3(res)
    dev = points.device
    new3 = lambda src: None if src is None else torch.empty((cap, 3), dtype=torch.float32, device=dev)
    out_keys = torch.empty(cap, dtype=torch.int64, device=dev)
    out_counts = torch.empty(cap, dtype=torch.int32, device=dev)
    out_p, out_c, out_n = new3(points), new3(colors), new3(normals)
    support = torch.empty(m, dtype=torch.int32, device=dev) if want_support else None
    total = torch.empty(1, dtype=torch.int64, device=dev)
    _, ws, ws_bytes = _pc_workspace("lse_voxel_support_workspace", m, workspace, dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if (t is not None and t.numel()) else None
    _lib.call("lse_voxel_support_filter", *(a if m else None for a in args), m, md, nx, ny, nz, min_support, ws, ws_bytes, cap,
              ptr(out_keys), ptr(out_counts), ptr(out_p), ptr(out_c), ptr(out_n), ptr(support), ptr(total), _stream())
    return out_keys, out_counts, out_p, out_c, out_n, total, support


# ---- event synthesis (csrc/events.hip; driven by lsenerf_amd.events) ----
EVENT_MAX_AXIS = 32767     # x and y of an event are int16
EVENT_MAX_CAP_STEP = 32767


def _ev(t: Optional[torch.Tensor], dtype, shape, name: str, allow_none: bool = False):
    """Pointer of a contiguous device tensor of ``dtype`` and ``shape``; every violation is a ValueError."""
    if t is None:
        if allow_none:
            return None
        raise ValueError(f"{name} is None")
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{name} must live on the GPU (got {getattr(t, 'device', type(t))}); the HIP path has no CPU fallback")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: {list(shape)} expected, got {list(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _ev_sensor(c_pos: float, c_neg: float, cap_step: int):
    import math
    c_pos, c_neg, cap_step = float(c_pos), float(c_neg), int(cap_step)
    if not (c_pos > 0.0 and math.isfinite(c_pos) and c_neg > 0.0 and math.isfinite(c_neg)):
        raise ValueError(f"the thresholds must be positive and finite, got {c_pos} and {c_neg}")
    if not 1 <= cap_step <= EVENT_MAX_CAP_STEP:
        raise ValueError(f"cap_step {cap_step} outside [1, {EVENT_MAX_CAP_STEP}]")
    return c_pos, c_neg, cap_step


def _ev_planes(planes: torch.Tensor):
    if not torch.is_tensor(planes) or planes.dim() != 2 or planes.shape[0] < 1:
        raise ValueError(f"planes: [K + 1, P] expected, got {list(getattr(planes, 'shape', ()))}")
    return planes.shape[0] - 1, planes.shape[1]


def event_workspace_bytes(K: int, P: int) -> int:
    """Bytes of the workspace ``event_append`` needs for ``K`` intervals of ``P`` pixels (lse_event_workspace)."""
    v = ctypes.c_int64(0)
    _lib.call("lse_event_workspace", int(K), int(P), ctypes.byref(v))
    return int(v.value)


@torch.no_grad()
def event_count(planes: torch.Tensor, ref_in: torch.Tensor, c_pos: float, c_neg: float, cap_step: int,
                counts: Optional[torch.Tensor] = None, ref_out: Optional[torch.Tensor] = None,
                window_total: Optional[torch.Tensor] = None):
    """The sensor walk of include/lse_hip.h ("event synthesis") over ``planes`` (float32 [K + 1, P], log intensity) from the levels
    ``ref_in`` (float32 [P]), without a stream: ``(counts int32 [K, P], ref_out float32 [P], window_total int64 [1])`` --
    lse_event_count.  ``window_total`` = the sum of ``|counts|``.  No host read."""
    K, P = _ev_planes(planes)
    c_pos, c_neg, cap_step = _ev_sensor(c_pos, c_neg, cap_step)
    lp = _ev(planes, torch.float32, (K + 1, P), "planes")
    ri = _ev(ref_in, torch.float32, (P,), "ref_in")
    dev = planes.device
    if counts is None:
        counts = torch.empty((K, P), dtype=torch.int32, device=dev)
    if ref_out is None:
        ref_out = torch.empty(P, dtype=torch.float32, device=dev)
    if window_total is None:
        window_total = torch.empty(1, dtype=torch.int64, device=dev)
    outs = (_ev(counts, torch.int32, (K, P), "counts"), _ev(ref_out, torch.float32, (P,), "ref_out"),
            _ev(window_total, torch.int64, (1,), "window_total"))
    if P and ref_out.data_ptr() == ref_in.data_ptr():
        raise ValueError("event_count: ref_out must not alias ref_in")
    _lib.call("lse_event_count", lp, K, P, ri, c_pos, c_neg, cap_step, *outs, _stream())
    return counts, ref_out, window_total


@torch.no_grad()
def event_append(planes: torch.Tensor, times: torch.Tensor, W: int, ref_in: torch.Tensor, c_pos: float, c_neg: float, cap_step: int,
                 out_x: torch.Tensor, out_y: torch.Tensor, out_t: torch.Tensor, out_p: torch.Tensor, total: torch.Tensor,
                 counts: Optional[torch.Tensor] = None, ref_out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Appends the events of the window ``planes`` (float32 [K + 1, P]) at ``times`` (float64 [K + 1], device, ascending) to ``out_x``,
    ``out_y`` (int16), ``out_t`` (float64), ``out_p`` (int8), all [cap], behind row ``total[0]`` in stream order (interval, pixel,
    emission) and adds their number to ``total`` (int64 [1] on the device) -- lse_event_append.  ``counts`` (int32 [K, P]) is
    optional; returns ``ref_out`` (float32 [P], not ``ref_in``).  Rows beyond ``cap`` are dropped while ``total`` keeps counting.
    No host read."""
    K, P = _ev_planes(planes)
    c_pos, c_neg, cap_step = _ev_sensor(c_pos, c_neg, cap_step)
    W = int(W)
    if not 1 <= W <= EVENT_MAX_AXIS or P % W != 0 or P // W > EVENT_MAX_AXIS:
        raise ValueError(f"event_append: {P} pixels in rows of {W}: the width and the height must divide the plane and lie in "
                         f"[1, {EVENT_MAX_AXIS}]")
    lp = _ev(planes, torch.float32, (K + 1, P), "planes")
    tp = _ev(times, torch.float64, (K + 1,), "times")
    ri = _ev(ref_in, torch.float32, (P,), "ref_in")
    cap = int(out_t.shape[0]) if torch.is_tensor(out_t) and out_t.dim() == 1 else -1
    if cap < 0:
        raise ValueError("out_t: [cap] expected")
    outs = (_ev(out_x, torch.int16, (cap,), "out_x"), _ev(out_y, torch.int16, (cap,), "out_y"),
            _ev(out_t, torch.float64, (cap,), "out_t"), _ev(out_p, torch.int8, (cap,), "out_p"))
    tot = _ev(total, torch.int64, (1,), "total")
    cn = _ev(counts, torch.int32, (K, P), "counts", True)
    dev = planes.device
    if ref_out is None:
        ref_out = torch.empty(P, dtype=torch.float32, device=dev)
    ro = _ev(ref_out, torch.float32, (P,), "ref_out")
    if P and ref_out.data_ptr() == ref_in.data_ptr():
        raise ValueError("event_append: ref_out must not alias ref_in")
    need = event_workspace_bytes(K, P)
    if workspace is None:
        workspace = torch.empty(need, dtype=torch.uint8, device=dev)
    if not torch.is_tensor(workspace) or workspace.dim() != 1:
        raise ValueError("workspace: a flat uint8 tensor expected")
    ws = _ev(workspace, torch.uint8, (workspace.numel(),), "workspace")
    if workspace.numel() < need:
        raise ValueError(f"event_append: workspace of {workspace.numel()} bytes < {need}")
    _lib.call("lse_event_append", lp, tp, K, P, W, ri, c_pos, c_neg, cap_step, ws, workspace.numel(), cap, *outs, cn, ro, tot, _stream())
    return ref_out


@torch.no_grad()
def event_accumulate(x: torch.Tensor, y: torch.Tensor, t: torch.Tensor, p: torch.Tensor, bounds: torch.Tensor, acc: torch.Tensor,
                     n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adds the events ``x, y`` (int16), ``t`` (float64), ``p`` (int8), all [n] -- the first ``n_dev[0]`` of them with ``n_dev`` --
    into the frames ``acc`` (int32 [F, H, W]): frame f holds ``bounds[f] <= t < bounds[f + 1]`` (``bounds`` float64 [F + 1], device,
    ascending) -- lse_event_accumulate.  Events outside the bounds or the image are skipped.  ``acc`` is not zeroed: a stream can
    arrive in pieces.  Integer atomics: bit-reproducible."""
    if not torch.is_tensor(acc) or acc.dim() != 3 or min(acc.shape) < 1:
        raise ValueError(f"acc: int32 [F, H, W] with every extent at least 1 expected, got {list(getattr(acc, 'shape', ()))}")
    F, H, W = (int(s) for s in acc.shape)
    n = int(t.shape[0]) if torch.is_tensor(t) and t.dim() == 1 else -1
    if n < 0:
        raise ValueError("t: [n] expected")
    args = (_ev(x, torch.int16, (n,), "x"), _ev(y, torch.int16, (n,), "y"), _ev(t, torch.float64, (n,), "t"),
            _ev(p, torch.int8, (n,), "p"))
    nd = _ev(n_dev, torch.int64, (1,), "n_dev", True)
    b = _ev(bounds, torch.float64, (F + 1,), "bounds")
    a = _ev(acc, torch.int32, (F, H, W), "acc")
    _lib.call("lse_event_accumulate", *args, n, nd, b, F, H, W, a, _stream())
    return acc


# ---- weighted pixel draw (csrc/pixel_draw.hip; driven by lsenerf_amd.data.BatchComposer) ----
PIXEL_MAX_WEIGHT = 255
_PIXEL_TYPE = {torch.int8: _lib.LSE_PIX_I8, torch.uint8: _lib.LSE_PIX_U8, torch.int16: _lib.LSE_PIX_I16, torch.int32: _lib.LSE_PIX_I32,
               torch.float32: _lib.LSE_PIX_F32}


def _px_weights(w_active: int, w_idle: int) -> Tuple[int, int]:
    ok = all(isinstance(w, int) and not isinstance(w, bool) and 0 <= w <= PIXEL_MAX_WEIGHT for w in (w_active, w_idle))
    if not ok or w_active + w_idle == 0:
        raise ValueError(f"pixel weights are integers in [0, {PIXEL_MAX_WEIGHT}], not both zero; got {w_active!r} and {w_idle!r}")
    return w_active, w_idle


def _px_planes(t: Optional[torch.Tensor], shape, name: str, dtypes):
    """(pointer, LSE_PIX_* code) of an optional resident [n_images, H, W] tensor."""
    if t is None:
        return None, _lib.LSE_PIX_NONE
    if not torch.is_tensor(t) or t.dtype not in dtypes:
        raise ValueError(f"{name}: a tensor of one of {[str(d) for d in dtypes]} expected, got {getattr(t, 'dtype', type(t))}")
    return _ev(t, t.dtype, shape, name), _PIXEL_TYPE[t.dtype]


def _px_set(images, msk, shape, w_active, w_idle):
    n_images, H, W = (int(s) for s in shape)
    if min(n_images, H, W) < 1:
        raise ValueError(f"a camera set of {n_images} images of {H} x {W}: every extent must be at least 1")
    w_active, w_idle = _px_weights(w_active, w_idle)
    im, pix_type = _px_planes(images, (n_images, H, W), "images", tuple(_PIXEL_TYPE))
    mk, msk_type = _px_planes(msk, (n_images, H, W), "msk", (torch.uint8, torch.float32))
    if images is None:
        if w_active != w_idle:
            raise ValueError("without images every pixel weighs the same: w_active must equal w_idle")
        pix_type = _lib.LSE_PIX_U8
    return (im, pix_type, mk, msk_type, n_images, H, W, w_active, w_idle), n_images * H


@torch.no_grad()
def pixel_rows_build(images: Optional[torch.Tensor], msk: Optional[torch.Tensor], shape, w_active: int, w_idle: int,
                     row_off: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``row_off`` int64 [n_images * H + 1] of a resident camera set of ``shape = (n_images, H, W)``: the exclusive prefix sums of the
    rows' summed pixel weights and, last, the total -- lse_pixel_rows_build (include/lse_hip.h, "weighted pixel draw": the weight of a
    pixel is 0 where ``msk`` is 0, else ``w_active`` / ``w_idle`` by ``images != 0``; ``images=None``: ``w_idle`` everywhere).
    No host read."""
    args, rows = _px_set(images, msk, shape, w_active, w_idle)
    if row_off is None:
        ref = images if images is not None else msk
        if ref is None:
            raise ValueError("pixel_rows_build: without images and a mask, pass row_off (it names the device)")
        row_off = torch.empty(rows + 1, dtype=torch.int64, device=ref.device)
    ro = _ev(row_off, torch.int64, (rows + 1,), "row_off")
    _lib.call("lse_pixel_rows_build", *args, ro, _stream())
    return row_off


@torch.no_grad()
def pixel_draw(images: Optional[torch.Tensor], msk: Optional[torch.Tensor], shape, w_active: int, w_idle: int, row_off: torch.Tensor,
               seed: int, stream_id: int, n: int, step: Optional[int] = None, step_dev: Optional[torch.Tensor] = None,
               indices: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None):
    """``n`` pixels of the set drawn by weight at ``step`` (an int) or at ``step_dev[0]`` (int64 [1] on the device; exactly one of the
    two): ``(indices int32 [n, 3] = (c, y, x), weights int32 [n])`` -- lse_pixel_draw over the ``row_off`` of ``pixel_rows_build`` with
    the same images, mask and weights.  One launch whose grid depends on ``n`` only; no host read."""
    args, rows = _px_set(images, msk, shape, w_active, w_idle)
    n, seed, stream_id = int(n), int(seed), int(stream_id)
    if n < 0:
        raise ValueError("pixel_draw: n < 0")
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must fit 64 unsigned bits")
    if stream_id not in (0, 1):
        raise ValueError("stream_id is 0 (colour) or 1 (events)")
    if (step is None) == (step_dev is None):
        raise ValueError("pixel_draw: give step or step_dev")
    if step is not None and not 0 <= int(step) < 2 ** 63:
        raise ValueError(f"the draw position is a step number, got {step}")
    ro = _ev(row_off, torch.int64, (rows + 1,), "row_off")
    sd = _ev(step_dev, torch.int64, (1,), "step_dev", True)
    dev = row_off.device
    if indices is None:
        indices = torch.empty((n, 3), dtype=torch.int32, device=dev)
    if weights is None:
        weights = torch.empty(n, dtype=torch.int32, device=dev)
    ix, wt = _ev(indices, torch.int32, (n, 3), "indices"), _ev(weights, torch.int32, (n,), "weights")
    _lib.call("lse_pixel_draw", *args, ro, seed, stream_id, sd, 0 if step is None else int(step), n, ix, wt, _stream())
    return indices, weights
