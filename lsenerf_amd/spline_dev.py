"""The spline pose path of ``cameras.py`` on the device: the pose tables of a ``BatchComposer`` from a ``SplineCameraOptimizer``'s
parameters by ONE launch (``lse_spline_poses``), and the gradient of the tables back to ``ctrl_tangents`` / ``scale`` by one more
(``lse_spline_poses_bwd``) -- csrc/spline.hip.  ``BatchComposer.attach_spline`` (lsenerf_amd.data) builds a ``SplinePoses``.

What depends only on buffers that never change during training is computed ONCE, on the host, with the very torch expressions of
``cameras.py`` (the functions of the first half of this module: they need no device):
  * the query times of every fed table ("rgb" / "evs": the cameras' times; "deblur": ``cam_t - exp_t / 2 + k * exp_t / 3``);
  * per query the bracketing control index and the fraction (``vectorized_generalized_interpolation`` after the clip of
    ``get_rgb_cameras``);
  * per control point the list of the queries it brackets (CSR over ``idx`` and ``idx + 1``, ascending query order): the order of the
    backward's fixed-order sums.
The kernels read ``ctrl_tangents`` and ``scale`` from the parameters' own storage, so an in-place optimiser update is seen by the next
launch -- or the next replay of a captured step -- without a copy.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib

KINDS = ("rgb", "evs", "deblur")
SEGMENTS = ("col", "prev", "nxt")


# ---------------------------------------------------------------------------------------------------- host precomputation
def deblur_times(cam_ts: Tensor, exp_t: float, n_deblur_rays: int = 4) -> Tensor:
    """``get_deblur_cameras``' query times: cam_ts [n, 1] exposure mid-times -> [n * n_deblur_rays] (the same expression, so the same
    bits)."""
    delta = exp_t / (n_deblur_rays - 1)
    steps = delta * torch.arange(n_deblur_rays, device=cam_ts.device)
    return (cam_ts - exp_t / 2 + steps[None]).reshape(-1)


def query_times(times: Tensor, kind: str, exp_t: float = 0.0, n_deblur_rays: int = 4) -> Tensor:
    """The times a table of ``kind`` is evaluated at, for cameras at ``times`` ([C] or [C, 1]): "rgb" / "evs" -> [C], "deblur" ->
    [C * n_deblur_rays] (slot k of camera c at c * n + k, the layout of the composer's colour table)."""
    assert kind in KINDS, kind
    times = times.detach().cpu().float()
    return deblur_times(times.reshape(-1, 1), exp_t, n_deblur_rays) if kind == "deblur" else times.reshape(-1)


def brackets(ctrl_ts: Tensor, times: Tensor) -> Tuple[Tensor, Tensor]:
    """``(idx int64 [N], frac float32 [N])``: the control interval ``[idx, idx + 1]`` of every time and the position inside it -- the
    clip of ``get_rgb_cameras`` followed by the index and fraction lines of ``vectorized_generalized_interpolation``."""
    ctrl_ts = ctrl_ts.detach().cpu()
    ts = torch.clip(times.detach().cpu(), ctrl_ts[0], ctrl_ts[-1]).reshape(-1)
    control_ts, interp_ts = ctrl_ts.float(), ts.float()
    idx = torch.searchsorted(control_ts, interp_ts, right=True)
    idx = torch.clamp(idx, 1, len(control_ts) - 1) - 1
    t0, t1 = control_ts[idx], control_ts[idx + 1]
    return idx, (interp_ts - t0) / (t1 - t0)


def control_point_lists(idx: Tensor, n_ctrl: int) -> Tuple[Tensor, Tensor]:
    """CSR ``(start int32 [n_ctrl + 1], query int32 [2 N])``: control point k owns ``query[start[k]:start[k + 1]]`` = the queries with
    ``idx == k`` or ``idx + 1 == k``, in ascending query order."""
    idx = idx.reshape(-1).long()
    n = idx.numel()
    q = torch.arange(n, dtype=torch.int64)
    owner, query = torch.cat([idx, idx + 1]), torch.cat([q, q])
    order = torch.argsort(owner * max(n, 1) + query)            # by control point, then by query (all keys distinct)
    start = torch.zeros(n_ctrl + 1, dtype=torch.int64)
    start[1:] = torch.cumsum(torch.bincount(owner, minlength=n_ctrl), 0)
    return start.to(torch.int32), query[order].to(torch.int32)


class SplinePlan:
    """Everything ``SplinePoses`` precomputes, on the host: per segment (col | prev | nxt) its kind and query times, and over all
    queries (segment after segment) ``idx``, ``frac`` and the control points' lists."""

    def __init__(self, ctrl_ts: Tensor, segments: Sequence[Optional[Tuple[str, Tensor]]], exp_t: float = 0.0, n_deblur_rays: int = 4):
        assert len(segments) == 3, "one entry per pose table: (col, prev, nxt), None where the spline feeds none"
        self.n_ctrl = int(ctrl_ts.numel())
        if self.n_ctrl < 2:
            raise ValueError("a pose spline needs at least two control points")
        self.kinds: List[Optional[str]] = [None if s is None else s[0] for s in segments]
        self.times: List[Optional[Tensor]] = [None if s is None else query_times(s[1], s[0], exp_t, n_deblur_rays) for s in segments]
        self.n_query = [0 if t is None else int(t.numel()) for t in self.times]
        if sum(self.n_query) == 0:
            raise ValueError("the spline feeds no pose table")
        self.idx, self.frac = brackets(ctrl_ts, torch.cat([t for t in self.times if t is not None]))
        self.csr_start, self.csr_query = control_point_lists(self.idx, self.n_ctrl)
        # the kernels clamp what they read for memory safety only: a plan that leaves its tables is refused here, once
        n = sum(self.n_query)
        assert self.idx.numel() == self.frac.numel() == n and int(self.idx.min()) >= 0 and int(self.idx.max()) <= self.n_ctrl - 2
        assert int(self.csr_start[0]) == 0 and int(self.csr_start[-1]) == self.csr_query.numel() == 2 * n
        assert bool((torch.diff(self.csr_start) >= 0).all()) and int(self.csr_query.min()) >= 0 and int(self.csr_query.max()) < n


# ---------------------------------------------------------------------------------------------------- the device side
def _ptr(t: Optional[Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _SplineTables(torch.autograd.Function):
    """(ctrl_tangents, scale) -> the fed pose tables (new tensors); backward = lse_spline_poses_bwd (new tensors)."""

    @staticmethod
    def forward(ctx, poses, ctrl_tangents, scale):
        out = tuple(torch.empty(shape, dtype=torch.float32, device=poses.device) for shape in poses.fed_shapes)
        poses.forward(poses._spread(out))
        ctx.poses = poses
        return out

    @staticmethod
    def backward(ctx, *grads):
        poses = ctx.poses
        grads = [torch.zeros(shape, dtype=torch.float32, device=poses.device) if g is None else g.contiguous().float()
                 for g, shape in zip(grads, poses.fed_shapes)]
        g = poses.backward(poses._spread(grads), static=False)
        return None, g["ctrl_tangents"], g["scale"]


class SplinePoses:
    """The device-side counterpart of ``spline_tables`` for up to three pose tables.  ``segments``: per table (col, prev, nxt)
    ``(kind, camera times)`` or None; ``shapes``: the tables' shapes (None where not fed)."""

    def __init__(self, spline, segments: Sequence[Optional[Tuple[str, Tensor]]], shapes: Sequence[Optional[Tuple[int, ...]]], device):
        if spline.config.mode == "off":
            raise ValueError("the spline's mode is 'off' (frozen, or a 'delayed' scheme before turn_on()): its tables are constant -- "
                             "set_poses(...) once is the right call; attach after turn_on() and rebuild the captured step")
        self.spline, self.device = spline, torch.device(device)
        self.plan = plan = SplinePlan(spline.ctrl_ts, segments, float(spline.exp_t), int(spline.n_deblur_rays))
        for name, n, shape in zip(SEGMENTS, plan.n_query, shapes):
            rows = 0 if shape is None else int(torch.Size(shape[:-2]).numel())
            if n and (shape is None or tuple(shape[-2:]) != (3, 4) or rows != n):
                raise ValueError(f"the '{name}' pose table is {shape}, the spline has {n} poses for it")
        self.shapes = [tuple(s) if n else None for s, n in zip(shapes, plan.n_query)]
        self.fed = [n > 0 for n in plan.n_query]
        self.fed_shapes = [s for s in self.shapes if s is not None]
        self.idx = plan.idx.to(torch.int32).to(self.device)
        dev = self.device = self.idx.device               # ("cuda" -> "cuda:0": what the parameters' .device says)
        self.frac = plan.frac.to(dev)
        self.csr_start, self.csr_query = plan.csr_start.to(dev), plan.csr_query.to(dev)
        self.grads: Dict[str, Tensor] = {"ctrl_tangents": torch.zeros(plan.n_ctrl, 6, dtype=torch.float32, device=dev),
                                         "scale": torch.zeros(1, dtype=torch.float32, device=dev)}
        dM = spline.dM if spline.dM is not None else torch.eye(4)
        if any(k == "evs" for k in plan.kinds) and spline.dM is None:
            raise ValueError("an 'evs' table needs the spline's dM")
        self._params = self._check_params()
        self._ptrs = tuple(p.data_ptr() for p in self._params)     # (the addresses themselves: re-pointing .data keeps the Parameter)
        self._desc = _lib.SplineDesc(
            n_ctrl=plan.n_ctrl, n_query=(ctypes.c_int32 * 3)(*plan.n_query), evs=(ctypes.c_int32 * 3)(*[int(k == "evs") for k in plan.kinds]),
            csr_len=int(plan.csr_query.numel()), dM=(ctypes.c_float * 16)(*[float(v) for v in dM.detach().cpu().float().reshape(-1)]),
            ctrl_tangents=_ptr(self._params[0]), scale=_ptr(self._params[1]), idx=_ptr(self.idx), frac=_ptr(self.frac),
            csr_start=_ptr(self.csr_start), csr_query=_ptr(self.csr_query))

    def _check_params(self) -> Tuple[Tensor, Tensor]:
        ct, sc = self.spline.ctrl_tangents, self.spline.scale
        for name, p, shape in (("ctrl_tangents", ct, (self.plan.n_ctrl, 6)), ("scale", sc, (1,))):
            if p.device != self.device or p.dtype != torch.float32 or not p.is_contiguous() or tuple(p.shape) != shape:
                raise ValueError(f"the spline's {name} must be a contiguous float32 {shape} tensor on {self.device} "
                                 f"(got {tuple(p.shape)} {p.dtype} on {p.device}): move the spline to the composer's device first")
        return ct, sc

    def _current_desc(self):
        """The kernels read the parameters where they were at attach time (a captured step keeps reading there): a spline whose
        parameters were moved or replaced since (``.to()``, a loaded checkpoint that swaps ``.data``) must be attached again."""
        ct, sc = self.spline.ctrl_tangents, self.spline.scale
        if (ct.data_ptr(), sc.data_ptr()) != self._ptrs:
            raise ValueError("the spline's parameters have moved since attach_spline(): attach again (and rebuild a captured step)")
        return self._desc

    def _spread(self, fed: Sequence[Tensor]) -> List[Optional[Tensor]]:
        """One tensor per FED table -> (col, prev, nxt) with None where the spline feeds none."""
        it = iter(fed)
        return [next(it) if f else None for f in self.fed]

    def _checked(self, tensors: Sequence[Optional[Tensor]], what: str) -> List[Optional[Tensor]]:
        out = []
        for name, t, shape in zip(SEGMENTS, tensors, self.shapes):
            if shape is None:
                out.append(None)
                continue
            if t is None or tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{what}: the '{name}' table must be a contiguous float32 {shape} tensor on {self.device}")
            out.append(t)
        return out

    def forward(self, tables: Sequence[Optional[Tensor]]) -> None:
        """Fill the fed tables (col, prev, nxt; entries of tables the spline does not feed are ignored) from the current parameters."""
        t = self._checked(tables, "lse_spline_poses")
        _lib.call("lse_spline_poses", ctypes.byref(self._current_desc()), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _stream())

    def backward(self, d_tables: Sequence[Optional[Tensor]], static: bool = True, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
        """``{"ctrl_tangents": [K, 6], "scale": [1]}`` from the gradients of the fed tables; ``static``: in the tensors of
        ``self.grads``, which the next call overwrites; ``out``: in the caller's tensors instead (the ``.grad`` views of a flat
        optimiser buffer: no copy)."""
        g = self._checked(d_tables, "lse_spline_poses_bwd")
        if out is not None:
            for k, v in self.grads.items():
                t = out.get(k)
                if t is None or tuple(t.shape) != tuple(v.shape) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                    raise ValueError(f"lse_spline_poses_bwd: out['{k}'] must be a contiguous float32 {tuple(v.shape)} tensor on {self.device}")
        else:
            out = self.grads if static else {k: torch.empty_like(v) for k, v in self.grads.items()}
        _lib.call("lse_spline_poses_bwd", ctypes.byref(self._current_desc()), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                  _ptr(out["ctrl_tangents"]), _ptr(out["scale"]), _stream())
        return out

    def tables(self) -> List[Optional[Tensor]]:
        """The fed tables as NEW tensors with autograd history back to the spline's parameters (None where not fed)."""
        return self._spread(_SplineTables.apply(self, self.spline.ctrl_tangents, self.spline.scale))
