"""Event synthesis: a trained field back in the event domain.  ``log_intensity_planes`` renders the quantity the event loss compares
(``log(v + EPS)`` of the event-side output) along a trajectory with the count-free eval render; ``simulate_events`` walks the
sensor model of include/lse_hip.h ("event synthesis") over those planes in windows and returns an ordered stream ``(x, y, t, p)``;
``predict_event_frames`` gives the signed counts between the poses of each frame -- what ``eimgs_1x.npy`` records between
``prev_camera`` and ``next_camera``; ``accumulate_events`` is the inverse, a stream -> frames.  The planes, the walk, the ordered
append and the accumulation stay on the device; the host reads are the occupancy grid's overflow check behind the last pose and the
counts that size the stream."""
from __future__ import annotations

import os
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import numpy as np
import torch
from torch import Tensor

from . import evaluation, ops


@dataclass
class EventStream:
    x: Tensor          # [n] int16, column
    y: Tensor          # [n] int16, row
    t: Tensor          # [n] float64
    p: Tensor          # [n] int8, +1 or -1
    H: int
    W: int

    def __len__(self) -> int:
        return int(self.t.shape[0])

    def sorted_by_time(self) -> "EventStream":
        """The stream in non-decreasing ``t``: a stable sort, so events of equal time keep their stream order."""
        _, order = torch.sort(self.t, stable=True)
        return EventStream(self.x[order], self.y[order], self.t[order], self.p[order], self.H, self.W)

    def write_npz(self, path: str) -> None:
        host = lambda v: v.detach().cpu().numpy()
        np.savez(path, x=host(self.x), y=host(self.y), t=host(self.t), p=host(self.p), H=np.int64(self.H), W=np.int64(self.W))

    @staticmethod
    def read_npz(path: str, device=None) -> "EventStream":
        with np.load(path) as z:
            arr = {k: z[k] for k in ("x", "y", "t", "p", "H", "W")}
        put = lambda v, dt: torch.from_numpy(np.ascontiguousarray(v.astype(dt))).to(device or "cpu")
        return EventStream(put(arr["x"], np.int16), put(arr["y"], np.int16), put(arr["t"], np.float64), put(arr["p"], np.int8),
                           int(arr["H"]), int(arr["W"]))


# ---- the model's side -----------------------------------------------------------------------------------------------------------
@contextmanager
def _eval_no_grad(model):
    """Eval mode without gradients and without the normals pass for the duration; every module's mode and ``config.eval_normals``
    come back, also behind an exception.  The configuration is written only where it has to change."""
    cfg = model.config
    saved = cfg.eval_normals
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        if saved != "off":
            cfg.eval_normals = "off"
        with torch.no_grad():
            yield
    finally:
        if saved != "off":
            cfg.eval_normals = saved
        for m, was in modes:
            m.training = was


def _camera_desc(cameras):
    dist = cameras.distortion_params
    if dist is not None and dist.dim() != 1:
        raise ValueError("one set of distortion parameters per camera set expected")
    distort = bool(dist is not None and bool((dist != 0).any()))
    return ops.camera_desc(cameras.fx, cameras.fy, cameras.cx, cameras.cy, cameras.height, cameras.width,
                           [float(v) for v in dist] if distort else None)


def _check_poses(poses: Tensor, dev) -> Tensor:
    if not torch.is_tensor(poses) or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
        raise ValueError(f"poses: [n, 3, 4] expected, got {tuple(getattr(poses, 'shape', ()))}")
    return poses.detach().to(dev, torch.float32).contiguous()


def _plane_renderer(model, cameras, poses: Tensor, times: Optional[Tensor], appearance_id: int, camera_index: int) -> Callable:
    """``render(i0, i1, out)``: the log-intensity planes of poses ``i0 .. i1 - 1`` into the rows of ``out`` [i1 - i0, H * W].  The
    model must be in eval mode (``_eval_no_grad``)."""
    from .eval_set import pose_bundle
    from .model import EPS, to_gray
    dev = model.scene_aabb.device
    H, W = cameras.height, cameras.width
    desc = _camera_desc(cameras)
    app = torch.full((1,), int(appearance_id), dtype=torch.int32, device=dev)
    rows = {k: v[int(camera_index)].to(dev) for k, v in (cameras.metadata or {}).items() if torch.is_tensor(v)}
    if times is not None:
        times = times.detach().to(dev, torch.float32).reshape(-1)
        if times.numel() != poses.shape[0]:
            raise ValueError(f"{times.numel()} times for {poses.shape[0]} poses")
    key = model._plan()["ev_key"]

    def render(i0: int, i1: int, out: Tensor) -> None:
        for i in range(i0, i1):
            bundle = pose_bundle(desc, poses[i], H, W, camera_index, app, None if times is None else times[i], rows)
            res = evaluation.render_flat(model, evaluation._flatten_bundle(bundle, device=dev), check_overflow=False)
            v = res[key]
            if v.shape[-1] != 1:
                v = to_gray(v)
            out[i - i0].copy_(torch.log(v + EPS).reshape(-1))
    return render


def log_intensity_planes(model, cameras, poses: Tensor, times: Optional[Tensor] = None, appearance_id: int = 0,
                         camera_index: int = 0) -> Tensor:
    """float32 ``[n, H * W]``: per pose of ``poses`` ([n, 3, 4], camera to world) the operand of the event loss, ``log(v + EPS)``
    with ``v`` the eval render's event-side output ("ev_out", or "rgb" when no mapping routes events; grey when it has three
    channels) -- rendered like an eval image: ``ops.camera_rays`` over the pose, the bundle of ``eval_set.camera_bundle``
    (``directions_norm``, ``appearance_id``, ``times`` [n] when given, the per-camera metadata of camera ``camera_index``) and
    ``evaluation.render_flat``.  ``cameras`` (``EdCameras``) gives intrinsics, distortion and size.  One overflow read behind the
    last pose."""
    dev = model.scene_aabb.device
    poses = _check_poses(poses, dev)
    n, P = poses.shape[0], cameras.height * cameras.width
    with _eval_no_grad(model):
        planes = torch.empty((n, P), dtype=torch.float32, device=dev)
        _plane_renderer(model, cameras, poses, times, appearance_id, camera_index)(0, n, planes)
        if n:
            model.occupancy_grid.check_deferred_overflow()
    return planes


def _thresholds(threshold: float, threshold_neg: Optional[float], cap_step: int) -> Tuple[float, float, int]:
    return ops._ev_sensor(threshold, threshold if threshold_neg is None else threshold_neg, cap_step)


def _simulate_windows(render: Callable, times: Tensor, P: int, W: int, c_pos: float, c_neg: float, window: int, cap_step: int,
                      max_events: Optional[int], ref: Optional[Tensor], backend=ops):
    """The window loop of ``simulate_events`` over ``render(i0, i1, out)`` and a ``backend`` with ``event_count``, ``event_append`` and
    ``event_workspace_bytes`` (``ops``; the tests inject the numpy twin): ``(x, y, t, p, ref_out, total)`` with the arrays trimmed to
    ``min(total, capacity)`` and ``total`` the true count."""
    window = int(window)
    if window < 1:
        raise ValueError(f"window {window} < 1")
    if max_events is not None and int(max_events) < 0:
        raise ValueError(f"max_events {max_events} < 0")
    dev = times.device
    K = times.shape[0] - 1
    new = lambda n, dt: torch.empty(n, dtype=dt, device=dev)
    dtypes = (torch.int16, torch.int16, torch.float64, torch.int8)
    cap = 0 if max_events is None else int(max_events)
    arrays = [new(cap, dt) for dt in dtypes]
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    planes = new((min(window, max(K, 0)) + 1) * P, torch.float32).view(-1, P)
    render(0, 1, planes[:1])
    refs = [new(P, torch.float32), new(P, torch.float32)]
    refs[0].copy_(planes[0] if ref is None else ref.detach().to(dev, torch.float32).reshape(P))
    ws = new(backend.event_workspace_bytes(min(window, max(K, 0)), P), torch.uint8)
    have = 0
    for k0 in range(0, K, window):
        k1 = min(k0 + window, K)
        kw = k1 - k0
        if k0 > 0:
            planes[0].copy_(planes[window])                     # the last plane of a window is the first of the next: not rendered twice
        render(k0 + 1, k1 + 1, planes[1:kw + 1])
        win = planes[:kw + 1]
        if max_events is None:
            _, _, wt = backend.event_count(win, refs[0], c_pos, c_neg, cap_step, ref_out=refs[1])
            have += int(wt.item())                              # the one host read of the window
            if have > cap:                                      # grow exactly
                grown = [new(have, dt) for dt in dtypes]
                for g, a in zip(grown, arrays):
                    g[:cap].copy_(a)
                arrays, cap = grown, have
        backend.event_append(win, times[k0:k1 + 1], W, refs[0], c_pos, c_neg, cap_step, *arrays, total, ref_out=refs[1], workspace=ws)
        refs.reverse()
    return arrays, refs[0], total, have if max_events is None else None


def simulate_events(model, cameras, poses: Tensor, times, threshold: float, threshold_neg: Optional[float] = None, window: int = 16,
                    cap_step: int = 127, max_events: Optional[int] = None, ref: Optional[Tensor] = None, sort: bool = True,
                    **bundle_kwargs):
    """Events of an ideal sensor (include/lse_hip.h, "event synthesis") that sees ``model``'s field from ``poses`` ([n, 3, 4]) at
    ``times`` ([n], ascending; kept in float64): ``(EventStream, ref_out, counts_total)``.  ``threshold`` / ``threshold_neg``: the
    contrast thresholds of positive / negative events (one value for both by default); ``cap_step``: most events of a pixel in one
    interval.  Planes are rendered in windows of ``window`` intervals (memory: ``window + 1`` planes and a workspace); ``ref``
    (float32 [H * W]) is the sensor's level per pixel on entry (default: the first plane) and ``ref_out`` the level behind the last
    pose, so trajectories chain.  ``max_events=None``: per window one host read of its count, the arrays grow exactly, nothing is
    dropped.  ``max_events=int``: preallocated arrays, no read inside the loop, events beyond the capacity are dropped in stream
    order; ``counts_total`` is the true count either way.  ``sort``: return the stream in non-decreasing time (stable) instead of
    stream order (interval, pixel, emission).  ``bundle_kwargs``: ``appearance_id``, ``camera_index`` and ``bundle_times`` ([n], the
    bundles' ``times``) of ``log_intensity_planes``.  Runs without gradients in eval mode and restores modes and settings."""
    c_pos, c_neg, cap_step = _thresholds(threshold, threshold_neg, cap_step)
    dev = model.scene_aabb.device
    poses = _check_poses(poses, dev)
    times = torch.as_tensor(times, dtype=torch.float64).detach().reshape(-1).to(dev).contiguous()
    if times.shape[0] != poses.shape[0] or poses.shape[0] < 1:
        raise ValueError(f"{times.shape[0]} times for {poses.shape[0]} poses (at least one)")
    H, W = cameras.height, cameras.width
    kw = dict(bundle_kwargs)
    bundle_times = kw.pop("bundle_times", None)
    with _eval_no_grad(model):
        render = _plane_renderer(model, cameras, poses, bundle_times, kw.pop("appearance_id", 0), kw.pop("camera_index", 0))
        if kw:
            raise TypeError(f"unexpected arguments {sorted(kw)}")
        arrays, ref_out, total, known = _simulate_windows(render, times, H * W, W, c_pos, c_neg, window, cap_step, max_events, ref)
        model.occupancy_grid.check_deferred_overflow()          # the read render_flat left out: once, behind the last pose
        true_total = int(total.item()) if known is None else known
    n = min(true_total, arrays[0].shape[0])
    stream = EventStream(*(a[:n] for a in arrays), H, W)
    return (stream.sorted_by_time() if sort else stream), ref_out, true_total


def predict_event_frames(model, cameras, poses: Tensor, threshold: float, threshold_neg: Optional[float] = None, cap_step: int = 127,
                         times: Optional[Tensor] = None, appearance_id: int = 0, camera_index: int = 0) -> Tensor:
    """int32 ``[F, H, W]``: per frame of ``poses`` ([F, S + 1, 3, 4]) the signed event counts of the sensor model summed over the
    frame's ``S`` intervals, the level starting at the frame's first plane -- the quantity ``eimgs[i]`` records between
    ``prev_camera`` and ``next_camera`` (``S = 1``: exactly those two poses).  ``times`` ([F, S + 1]): the bundles' times."""
    c_pos, c_neg, cap_step = _thresholds(threshold, threshold_neg, cap_step)
    if not torch.is_tensor(poses) or poses.dim() != 4 or tuple(poses.shape[2:]) != (3, 4) or poses.shape[1] < 2:
        raise ValueError(f"poses: [F, S + 1, 3, 4] with S >= 1 expected, got {tuple(getattr(poses, 'shape', ()))}")
    dev = model.scene_aabb.device
    F, S1 = poses.shape[:2]
    H, W = cameras.height, cameras.width
    flat = _check_poses(poses.reshape(F * S1, 3, 4), dev)
    with _eval_no_grad(model):
        render = _plane_renderer(model, cameras, flat, None if times is None else times.reshape(-1), appearance_id, camera_index)
        frames = torch.empty((F, H * W), dtype=torch.int32, device=dev)
        planes = torch.empty((S1, H * W), dtype=torch.float32, device=dev)
        counts = torch.empty((S1 - 1, H * W), dtype=torch.int32, device=dev)
        ref_out = torch.empty(H * W, dtype=torch.float32, device=dev)
        wt = torch.empty(1, dtype=torch.int64, device=dev)
        for f in range(F):
            render(f * S1, (f + 1) * S1, planes)
            ops.event_count(planes, planes[0], c_pos, c_neg, cap_step, counts=counts, ref_out=ref_out, window_total=wt)
            torch.sum(counts, dim=0, dtype=torch.int32, out=frames[f])
        if F:
            model.occupancy_grid.check_deferred_overflow()
    return frames.view(F, H, W)


def event_frame_metrics(pred: Tensor, recorded: Tensor) -> dict:
    """``{"mean_abs_diff", "sign_agreement"}`` of predicted against recorded event frames (same shape, any integer or float type):
    the mean absolute count difference, and the share of the pixels with a non-zero recorded count whose predicted count has the
    same sign (NaN when no pixel recorded anything).  Torch ops on the tensors' device, one read-back."""
    if tuple(pred.shape) != tuple(recorded.shape):
        raise ValueError(f"predicted frames are {tuple(pred.shape)}, recorded ones {tuple(recorded.shape)}")
    a, b = pred.to(torch.float64), recorded.to(pred.device, torch.float64)
    fired = b != 0
    agree = (torch.sign(a) == torch.sign(b)) & fired
    mad, share = torch.stack([(a - b).abs().mean(), agree.sum().to(torch.float64) / fired.sum().to(torch.float64)]).tolist()
    return {"mean_abs_diff": mad, "sign_agreement": share}


def accumulate_events(stream: EventStream, bounds, dtype=torch.int8) -> Tensor:
    """``[F, H, W]`` frames of ``stream``: frame f sums the polarities of the events with ``bounds[f] <= t < bounds[f + 1]``
    (``bounds``: F + 1 ascending times), saturated to the range of ``dtype`` (int8: the format of ``eimgs_1x.npy``)."""
    dev = stream.t.device
    bounds = torch.as_tensor(bounds, dtype=torch.float64).detach().reshape(-1).to(dev).contiguous()
    if bounds.shape[0] < 2:
        raise ValueError("bounds: at least two times expected")
    acc = torch.zeros((bounds.shape[0] - 1, stream.H, stream.W), dtype=torch.int32, device=dev)
    ops.event_accumulate(stream.x.contiguous(), stream.y.contiguous(), stream.t.contiguous(), stream.p.contiguous(), bounds, acc)
    if dtype == torch.int32:
        return acc
    info = torch.iinfo(dtype)
    return acc.clamp(max(info.min, -2 ** 31), min(info.max, 2 ** 31 - 1)).to(dtype)


def write_event_frames(ecam_dir: str, frames) -> str:
    """Writes ``frames`` ([n, H, W], saturated to int8) as ``<ecam_dir>/eimgs/eimgs_1x.npy``, where
    ``scene_io.EventSceneReader.load_events`` reads them; returns the path."""
    arr = frames.detach().cpu().numpy() if torch.is_tensor(frames) else np.asarray(frames)
    if arr.ndim != 3:
        raise ValueError(f"event frames are [n, H, W], got {arr.shape}")
    if arr.dtype != np.int8:
        arr = np.clip(arr, -128, 127).astype(np.int8)
    os.makedirs(os.path.join(ecam_dir, "eimgs"), exist_ok=True)
    path = os.path.join(ecam_dir, "eimgs", "eimgs_1x.npy")
    np.save(path, np.ascontiguousarray(arr))
    return path


def spline_event_poses(spline, times) -> Tensor:
    """float32 ``[n, 3, 4]``: the event camera's poses of a ``SplineCameraOptimizer`` at ``times`` (``get_evs_cameras``), detached."""
    with torch.no_grad():
        poses = spline.get_evs_cameras(torch.as_tensor(times))
    return poses.detach()[..., :3, :4].to(torch.float32).contiguous()
