"""The per-camera pose path of ``cameras.py`` on the device: the pose tables of a ``BatchComposer`` from the ``pose_adjustment`` of
``CameraOptimizer`` / ``PrevNextCamOptimizer`` by ONE launch (``lse_pose_delta_tables``), and the gradient of the tables back to the
parameters by one more (``lse_pose_delta_tables_bwd``) -- csrc/pose_delta.hip.  ``BatchComposer.attach_camera_optimizers``
(lsenerf_amd.data) builds a ``DeltaPoses``; ``spline_dev.SplinePoses`` is its counterpart for the spline.

What never changes during training is fixed ONCE, on the host: per fed table a static device copy of the scene's
``camera_to_worlds`` (the base poses), the exponential (SO3xR3 / SE3) and the mask of non-trainable cameras.  The kernels read
``pose_adjustment`` from the parameters' own storage, so an in-place optimiser update is seen by the next launch -- or the next
replay of a captured step -- without a copy.

A PARAMETER BLOCK is one ``pose_adjustment``; it carries the name of the first table it feeds ("col", "prev", "nxt").  One
``CameraOptimizer`` that feeds both "prev" and "nxt" is ONE block, "prev": its gradient is row(prev) + row(nxt).
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor

from . import _lib
from .spline_dev import SEGMENTS, _ptr, _stream

MODES = {"SO3xR3": _lib.LSE_POSE_SO3XR3, "SE3": _lib.LSE_POSE_SE3}


def check_trainable(optim, what: str) -> None:
    """The refusal ``attach_spline`` makes for a spline that is off, for a per-camera optimiser."""
    if optim.config.mode == "off":
        raise ValueError(f"the {what} optimiser's mode is 'off' (frozen, or a 'delayed' scheme before turn_on()): its tables are "
                         "constant -- set_poses(...) once is the right call; attach after turn_on() and rebuild the captured step")
    if optim.config.mode not in MODES:
        raise ValueError(f"the {what} optimiser's mode is {optim.config.mode!r}: one of {sorted(MODES)}")


class _DeltaTables(torch.autograd.Function):
    """(pose_adjustment per block) -> the fed pose tables (new tensors); backward = lse_pose_delta_tables_bwd (new tensors)."""

    @staticmethod
    def forward(ctx, poses, *params):
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
        return (None,) + tuple(g[name] for name in poses.blocks)


class DeltaPoses:
    """The device-side counterpart of ``data.camera_tables`` for up to three pose tables.  ``feeds``: per table (col, prev, nxt)
    ``(CameraOptimizer, base poses [C, 3, 4])`` or None; ``shapes``: the tables' shapes (None where not fed).  The same optimiser
    object under "prev" and "nxt" is one shared parameter block."""

    def __init__(self, feeds: Sequence[Optional[Tuple[object, Tensor]]], shapes: Sequence[Optional[Tuple[int, ...]]], device):
        assert len(feeds) == 3 and len(shapes) == 3, "one entry per pose table: (col, prev, nxt), None where no optimiser feeds it"
        self.fed = [f is not None for f in feeds]
        if not any(self.fed):
            raise ValueError("the camera optimisers feed no pose table")
        self.optims: List[Optional[object]] = [None if f is None else f[0] for f in feeds]
        for name, o in zip(SEGMENTS, self.optims):
            if o is not None:
                check_trainable(o, f"'{name}'")
        self.shared = self.fed[1] and self.fed[2] and self.optims[1] is self.optims[2]
        if self.fed[0] and any(self.optims[0] is o for o in self.optims[1:]):
            raise ValueError("one optimiser cannot feed the colour table and an event table: the camera sets differ")
        if self.fed[2] and not self.fed[1]:
            raise ValueError("the 'nxt' table is fed together with 'prev' only")
        dev = torch.zeros(0, device=device).device                      # ("cuda" -> "cuda:0": what the parameters' .device says)
        self.device = dev
        self.n_cam = [0 if o is None else int(o.num_cameras) for o in self.optims]
        self.shapes: List[Optional[Tuple[int, ...]]] = []
        self.base: List[Optional[Tensor]] = []
        self.frozen: List[Optional[Tensor]] = []
        for name, f, o, n, shape in zip(SEGMENTS, feeds, self.optims, self.n_cam, shapes):
            if f is None:
                self.shapes.append(None); self.base.append(None); self.frozen.append(None)
                continue
            rows = 0 if shape is None else int(torch.Size(shape[:-2]).numel())
            if shape is None or tuple(shape[-2:]) != (3, 4) or rows != n or n < 1:
                raise ValueError(f"the '{name}' pose table is {shape}, the optimiser has {n} cameras for it")
            base = f[1].detach()
            if tuple(base.shape) != (n, 3, 4):
                raise ValueError(f"the '{name}' base poses are {tuple(base.shape)}, the optimiser has {n} cameras")
            self.shapes.append(tuple(shape))
            self.base.append(base.to(dev, torch.float32).contiguous().clone())
            self.frozen.append(self._mask(o, n, dev))
        if self.shared:
            self.frozen[2] = self.frozen[1]
        self.fed_shapes = [s for s in self.shapes if s is not None]
        # the parameter blocks, by the name of the first table each feeds
        self.blocks: Dict[str, int] = {name: i for i, name in enumerate(SEGMENTS) if self.fed[i] and not (i == 2 and self.shared)}
        self._params = self._check_params()
        self._ptrs = [None if p is None else p.data_ptr() for p in self._params]
        self.grads: Dict[str, Tensor] = {name: torch.zeros(self.n_cam[i], 6, dtype=torch.float32, device=dev) for name, i in self.blocks.items()}
        arr3 = lambda ts: (ctypes.c_void_p * 3)(*[None if t is None else t.data_ptr() for t in ts])
        self._desc = _lib.PoseDeltaDesc(
            n_cam=(ctypes.c_int32 * 3)(*self.n_cam), mode=(ctypes.c_int32 * 3)(*[0 if o is None else MODES[o.config.mode] for o in self.optims]),
            shared_prev_next=int(self.shared), base=arr3(self.base), adj=arr3(self._params), frozen=arr3(self.frozen))

    @staticmethod
    def _mask(optim, n: int, dev) -> Optional[Tensor]:
        """``non_trainable_camera_indices`` as uint8 [n] (validated here, once: the kernels index it by camera)."""
        idx = optim.non_trainable_camera_indices
        if idx is None:
            return None
        idx = torch.as_tensor(idx).detach().cpu().reshape(-1).long()
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError(f"non_trainable_camera_indices must name cameras 0 .. {n - 1}")
        mask = torch.zeros(n, dtype=torch.uint8)
        mask[idx] = 1
        return mask.to(dev)

    def _check_params(self) -> List[Optional[Tensor]]:
        out = []
        for name, o, n in zip(SEGMENTS, self.optims, self.n_cam):
            if o is None:
                out.append(None)
                continue
            p = o.pose_adjustment
            if p.device != self.device or p.dtype != torch.float32 or not p.is_contiguous() or tuple(p.shape) != (n, 6):
                raise ValueError(f"the '{name}' optimiser's pose_adjustment must be a contiguous float32 {(n, 6)} tensor on {self.device} "
                                 f"(got {tuple(p.shape)} {p.dtype} on {p.device}): move the optimiser to the composer's device first")
            out.append(p)
        return out

    def parameters(self) -> List[Tensor]:
        """The attached ``pose_adjustment`` parameters, one per block, in block order."""
        return [self.optims[i].pose_adjustment for i in self.blocks.values()]

    def _current_desc(self):
        """The kernels read the parameters where they were at attach time (a captured step keeps reading there): an optimiser whose
        parameters were moved or replaced since (``.to()``, a ``FlatParams`` built afterwards, a loaded checkpoint that swaps
        ``.data``) must be attached again."""
        for o, ptr in zip(self.optims, self._ptrs):
            if o is not None and o.pose_adjustment.data_ptr() != ptr:
                raise ValueError("the camera optimisers' parameters have moved since attach_camera_optimizers(): attach again "
                                 "(and rebuild a captured step)")
        return self._desc

    def _spread(self, fed: Sequence[Tensor]) -> List[Optional[Tensor]]:
        """One tensor per FED table -> (col, prev, nxt) with None where no optimiser feeds it."""
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
        """Fill the fed tables (col, prev, nxt; entries of tables no optimiser feeds are ignored) from the current parameters."""
        t = self._checked(tables, "lse_pose_delta_tables")
        _lib.call("lse_pose_delta_tables", ctypes.byref(self._current_desc()), _ptr(t[0]), _ptr(t[1]), _ptr(t[2]), _stream())

    def backward(self, d_tables: Sequence[Optional[Tensor]], static: bool = True, out: Optional[Dict[str, Tensor]] = None) -> Dict[str, Tensor]:
        """``{block: [C, 6]}`` from the gradients of the fed tables; ``static``: in the tensors of ``self.grads``, which the next call
        overwrites; ``out``: in the caller's tensors instead (the ``.grad`` views of a flat optimiser buffer: no copy)."""
        g = self._checked(d_tables, "lse_pose_delta_tables_bwd")
        if out is not None:
            for k, v in self.grads.items():
                t = out.get(k)
                if t is None or tuple(t.shape) != tuple(v.shape) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                    raise ValueError(f"lse_pose_delta_tables_bwd: out['{k}'] must be a contiguous float32 {tuple(v.shape)} tensor on {self.device}")
        else:
            out = self.grads if static else {k: torch.empty_like(v) for k, v in self.grads.items()}
        o = [out.get(name) if name in self.blocks else None for name in SEGMENTS]
        _lib.call("lse_pose_delta_tables_bwd", ctypes.byref(self._current_desc()), _ptr(g[0]), _ptr(g[1]), _ptr(g[2]),
                  _ptr(o[0]), _ptr(o[1]), _ptr(o[2]), _stream())
        return {name: out[name] for name in self.blocks}

    def tables(self) -> List[Optional[Tensor]]:
        """The fed tables as NEW tensors with autograd history back to the parameters (None where not fed)."""
        return self._spread(_DeltaTables.apply(self, *self.parameters()))
