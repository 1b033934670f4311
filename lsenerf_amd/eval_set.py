"""A whole eval set on the device: the reference's ``LSENeRFPipeline.get_average_eval_image_metrics`` /
``get_eval_image_metrics_and_images`` (R:lse_nerf/lse_pipeline.py:149-233) without host work per image.

    eval_set = EvalSet("cuda", images_u8, cameras, msk=masks)            # uploaded once
    eval_set.set_poses(camera_tables(cameras, camera_optimizer))          # optional: an optimised rig
    average, per_image = model.evaluate_set(eval_set, events_only=(rgb_frac == 0))

``evaluation.py`` stays the per-image layer (``render_flat``, the image dictionary's helpers); this module is the loop over it.  Per
image: ``lse_camera_rays`` builds the rays from a device pose table, ``render_flat`` renders them without its overflow read,
``lse_eval_image_prep`` turns the resident ground truth and the render into the metric planes, ``lse_log_scale_correct`` (event-only
metric) fits the prediction to the ground truth in log space, and ``lse_image_metrics`` writes its two scalars into row ``i`` of a
device table.  Nothing waits for the device until the last image is enqueued: then one overflow read, the column means on the
device and ONE read-back of table plus means.

``PanelSet`` adds the images the reference's evaluation writes: per image the uint8 grid of its writer's combined picture (overlay
of Canny edges included) from ``lse_gray8_planes`` / ``lse_canny_u8`` / ``lse_eval_panels``, copied asynchronously into a row of
a pinned host buffer -- still without a wait inside the loop.
"""
from __future__ import annotations

import time
from typing import Callable, Dict, List, Optional, Tuple

import torch
from torch import Tensor

from . import evaluation, ops
from .cameras import EdCameras
from .data import CameraSetData, _as_tensor, camera_tables
from .rays import RayBundle

_SSIM, _MSE, _PSNR, _LPIPS = 0, 1, 2, 3          # columns of the metrics table


class EvalSet:
    """The eval images of one camera set in device memory -- a ``CameraSetData`` (``.data``: images uint8 or float32 [n, H, W, 3],
    optional masks, appearance ids, the camera of every image) plus a device pose table ``.poses`` [n_cameras, 3, 4] that starts
    as ``camera_tables(cameras)``."""

    def __init__(self, device, images, cameras: EdCameras, msk=None, appearance_ids=None, image_idx=None):
        images = _as_tensor(images)
        if images.dim() != 4 or images.shape[-1] < 3:
            raise ValueError(f"eval images are [n, H, W, 3], got {tuple(images.shape)}")
        images = images[..., :3]
        if images.dtype != torch.uint8:
            images = images.to(torch.float32)
        if appearance_ids is None:
            appearance_ids = torch.zeros(images.shape[0], dtype=torch.int64)
        self.device = torch.device(device)
        self.cameras = cameras
        self.data = d = CameraSetData(self.device, images, cameras, appearance_ids, msk, image_idx, channels=3)
        self.cam_desc = ops.camera_desc(cameras.fx, cameras.fy, cameras.cx, cameras.cy, d.H, d.W, d.dist if d.distort else None)
        self.poses = camera_tables(cameras).detach().to(self.device, torch.float32).clone().contiguous()
        self.camera_metadata = {k: v.to(self.device) for k, v in (cameras.metadata or {}).items() if torch.is_tensor(v)}

    def __len__(self) -> int:
        return self.data.n_images

    @torch.no_grad()
    def set_poses(self, table: Tensor) -> None:
        """Copy a pose table [n_cameras, 3, 4] -- ``camera_tables(cameras, optimizer)`` or ``spline_tables(spline, cameras)`` -- into
        the device table, in place and in stream order (no synchronisation for a table that is on the device already)."""
        if tuple(table.shape) != tuple(self.poses.shape):
            raise ValueError(f"the pose table is {tuple(self.poses.shape)}, got {tuple(table.shape)}")
        self.poses.copy_(table.detach(), non_blocking=True)


@torch.no_grad()
def pose_bundle(cam_desc, pose: Tensor, H: int, W: int, camera_index: int, appearance_id: Tensor, time: Optional[Tensor] = None,
                metadata_rows: Optional[Dict[str, Tensor]] = None) -> RayBundle:
    """The [H, W] bundle of one device pose ``pose`` [3, 4]: rays from ``ops.camera_rays``, ``camera_indices``, ``times`` when
    ``time`` (one element, on the device) is given, and the metadata ``generate_rays`` and the composer attach: ``directions_norm``,
    ``appearance_id`` (one element, on the device) and ``metadata_rows`` (the camera's row of every per-camera metadata tensor).
    What ``camera_bundle`` and ``events.log_intensity_planes`` share.  No host-to-device copy, no synchronisation."""
    o, dirs, area, norm = ops.camera_rays(cam_desc, pose, 0, H * W)
    dev = o.device
    meta = {"directions_norm": norm.reshape(H, W, 1), "appearance_id": appearance_id.reshape(1, 1, 1).expand(H, W, 1)}
    for k, row in (metadata_rows or {}).items():
        meta[k] = row.expand(H, W, *row.shape)
    times = time.reshape(1, 1, 1).expand(H, W, 1) if time is not None else None
    return RayBundle(origins=o.reshape(H, W, 3), directions=dirs.reshape(H, W, 3), pixel_area=area.reshape(H, W, 1),
                     camera_indices=torch.full((H, W, 1), int(camera_index), dtype=torch.long, device=dev), times=times,
                     metadata=meta)


@torch.no_grad()
def camera_bundle(eval_set: EvalSet, i: int) -> RayBundle:
    """The [H, W] bundle of eval image ``i``: rays from ``ops.camera_rays`` over the set's device pose table (the values of
    ``EdCameras.generate_rays`` over ``get_image_coords()``, bit-equal to the composer's), ``camera_indices``, ``times`` when the
    cameras have them, and the metadata ``generate_rays`` and the composer attach: ``directions_norm``, ``appearance_id`` and the
    cameras' own per-camera metadata.  No host-to-device copy, no synchronisation."""
    d = eval_set.data
    if not 0 <= int(i) < d.n_images:
        raise IndexError(f"eval image {i} of {d.n_images}")
    cam = int(d.image_idx_host[int(i)])
    return pose_bundle(eval_set.cam_desc, eval_set.poses[cam], d.H, d.W, cam, d.appearance_id[int(i)],
                       d.times[cam] if eval_set.cameras.times is not None else None,
                       {k: v[cam] for k, v in eval_set.camera_metadata.items()})


class PanelSet:
    """uint8 panels of a whole eval set, in the layout of the reference's writer (R:lse_nerf/lse_writer.py:32-64: every image of
    the dictionary but "accumulation" as ``clamp(v * 255, 0, 255)`` uint8, concatenated along the width).

        panel_set = PanelSet(eval_set)                                  # keys: a subset of ops.PANEL_KEYS, in that order
        model.evaluate_set(eval_set, panels=panel_set)
        panel_set.host[i]                                               # [H, Wtot, 3] uint8: comb_imgs/00i.png plus the overlay column

    Holds a device buffer for one image's grid and a pinned host buffer for the set.  ``evaluate_set`` launches the grey / Canny /
    panel kernels behind the metrics of image ``i`` and issues ONE asynchronous device-to-host copy of the grid into row ``i``; it
    adds no wait: the rows are valid after the wait ``evaluate_set`` ends with (copies and kernels share one stream).  "ev_out" is
    a column only when the model renders it (the writer walks the dictionary's keys); ``columns`` names what the last set produced
    and ``host`` is shaped to it.  "overlay" does not need ``config.eval_overlay``.  Writing files stays the caller's business."""

    def __init__(self, eval_set: EvalSet, keys=ops.PANEL_KEYS):
        keys = tuple(keys)
        if not keys or any(k not in ops.PANEL_KEYS for k in keys):
            raise ValueError(f"PanelSet: keys must be a non-empty subset of {ops.PANEL_KEYS}, got {keys}")
        d = eval_set.data
        self.keys = tuple(k for k in ops.PANEL_KEYS if k in keys)
        self.n, self.H, self.W = d.n_images, d.H, d.W
        dev = eval_set.device
        cells = self.H * ops.panel_columns(self.keys) * self.W * 3          # sized for every key; a set without "ev_out" uses less
        self._dev = torch.empty(cells, dtype=torch.uint8, device=dev)
        self._host = torch.empty(self.n * cells, dtype=torch.uint8, pin_memory=True)
        self._gray = torch.empty((2, self.H, self.W), dtype=torch.uint8, device=dev)
        self._edges = torch.empty((2, self.H, self.W), dtype=torch.uint8, device=dev)
        self._canny_ws = torch.empty(ops.canny_workspace_bytes(self.H, self.W, 2) // 8, dtype=torch.int64, device=dev)
        self._ws = torch.empty(ops.eval_panels_workspace_bytes(self.H, self.W) // 4, dtype=torch.float32, device=dev)
        self.columns: Tuple[str, ...] = ()
        self.host: Optional[Tensor] = None

    def _begin(self, outputs: Dict[str, Tensor]) -> None:
        """Fix the columns of this set from the first image's outputs and shape ``host`` to them (host work only)."""
        self.columns = tuple(k for k in self.keys if k != "ev_out" or outputs.get("ev_out") is not None)
        if not self.columns:
            raise ValueError("PanelSet: the only key is \"ev_out\" and the model renders none")
        self._cells = self.H * ops.panel_columns(self.columns) * self.W * 3
        self.host = self._host[:self.n * self._cells].view(self.n, self.H, -1, 3)

    def edges(self, gt_planes: Tensor, pred_planes: Tensor) -> Tensor:
        """uint8 [2, H, W]: the Canny edges (50, 200) of the 8-bit grey ground truth and prediction (buffers of this object)."""
        ops.gray8_planes(gt_planes, pred_planes, out=self._gray)
        return ops.canny_edges(self._gray, out=self._edges, workspace=self._canny_ws)

    def add(self, i: int, outputs: Dict[str, Tensor], gt_planes: Tensor, pred_planes: Tensor, pair=None) -> Tensor:
        """Enqueue the grid of image ``i`` and its copy into ``host[i]``; returns the device grid [H, Wtot, 3] (overwritten by the
        next image).  ``outputs``: the [H, W, C] outputs; ``pair``: the grey pair of the event-only metric as "img"."""
        if i == 0 or self.host is None:
            self._begin(outputs)
        edges = self.edges(gt_planes, pred_planes) if "overlay" in self.columns else None
        ev = outputs.get("ev_out") if "ev_out" in self.columns else None
        grid = self._dev[:self._cells].view(self.H, -1, 3)
        ops.eval_panels(self.columns, self.H, self.W, gt_planes=gt_planes, pred_planes=pred_planes,
                        rgb=outputs["rgb"].to(torch.float32).contiguous(), pair=pair,
                        depth=outputs["depth"].contiguous(), accumulation=outputs["accumulation"].contiguous(), edges=edges,
                        ev_out=None if ev is None else ev.to(torch.float32).contiguous(), out=grid, workspace=self._ws)
        self.host[i].copy_(grid, non_blocking=True)
        return grid


def _image_dict(outputs: Dict[str, Tensor], gt_planes: Tensor, pred_planes: Tensor, pair=None, overlay=None) -> Dict[str, Tensor]:
    """The reference's image dictionary (``evaluation.image_metrics_and_images``) from the metric planes; ``pair`` = (grey ground
    truth, corrected prediction) [1, 1, H, W]: the "img" of the event-only metric (R:lse_nerf/lse_pipeline.py:171-181)."""
    image, rgb = gt_planes[0].permute(1, 2, 0), pred_planes[0].permute(1, 2, 0)          # masked, [H, W, 3]
    if pair is None:
        img = torch.cat([image, outputs["rgb"]], dim=1)          # the unmasked prediction beside the (masked) ground truth
    else:
        img = torch.cat([p[0].permute(1, 2, 0).expand(-1, -1, 3) for p in pair], dim=1)
    images = {"img": img, "accumulation": evaluation.gray_colormap(outputs["accumulation"]),
              "depth": evaluation.depth_gray_map(outputs["depth"], outputs["accumulation"]),
              "err_map": evaluation.make_error_map(image, rgb)}
    if overlay is not None:
        images["overlay"] = overlay
    if outputs.get("ev_out") is not None:
        images["ev_out"] = outputs["ev_out"]
    if outputs.get("normals") is not None:
        images["normals"] = evaluation.normals_colormap(outputs["normals"], outputs["accumulation"])
    return images


@torch.no_grad()
def evaluate_set(model, eval_set: EvalSet, events_only: bool = False,
                 on_image: Optional[Callable[[int, Dict[str, Tensor], Dict[str, Tensor]], None]] = None,
                 panels: Optional[PanelSet] = None) -> Tuple[Dict[str, float], List[Dict[str, float]]]:
    """``(average, per_image)`` over every image of ``eval_set`` (R:lse_nerf/lse_pipeline.py:186-233): ``per_image[i]`` holds
    "psnr" (10 log10(1 / mse), float32 on the device), "ssim", and "lpips" only where ``model.lpips.available``; ``average`` their
    float32 column means (taken on the device) plus "num_rays_per_sec" and "fps".

    ``events_only=True`` (the reference's ``update_evs_only_metric``, chosen when ``rgb_frac == 0``) replaces those keys by the
    metrics of the grey ground truth against the prediction's R + G after a least-squares affine fit in log space
    (``ops.log_scale_correct``; the ground truth masked, the prediction not, as the reference passes them).

    The model renders in eval mode (its mode is restored) on whichever route ``evaluation.render_flat`` takes, the early-stop route
    included.  On the count-free routes nothing waits for the device inside the loop: the occupancy grid's sticky overflow
    accumulator is read once behind the last image (a truncated ray of ANY image raises there), then table and means come back in
    one copy.  Deviation from the reference: it times every image with ``time()`` around render and metrics, which would put a wait
    into the loop; here "num_rays_per_sec" and "fps" come from ONE wall-clock interval around the whole set (first launch to
    read-back) and appear in ``average`` only.

    ``on_image(i, outputs, images)``: called per image with the [H, W, C] outputs and the reference's image dictionary ("img",
    "accumulation", "depth", "err_map", "ev_out" when rendered; with ``events_only`` "img" is the grey pair).  The tensors are on
    the device, are not read back here, and those of the dictionary alias buffers the next image overwrites.  With
    ``config.eval_overlay`` the dictionary also holds "overlay" (``evaluation.make_overlay``), after "err_map".

    ``panels``: a ``PanelSet`` of this eval set.  Behind the metrics of image ``i`` its uint8 grid is computed on the device and
    copied asynchronously into ``panels.host[i]``; the metrics are untouched and no wait is added -- the rows are valid when this
    function returns."""
    d = eval_set.data
    n, H, W = d.n_images, d.H, d.W
    if n == 0:
        raise ValueError("empty eval set")
    if panels is not None and (panels.n, panels.H, panels.W) != (n, H, W):
        raise ValueError(f"the PanelSet holds {panels.n} images of {panels.H} x {panels.W}, the eval set {n} of {H} x {W}")
    want_overlay = on_image is not None and bool(getattr(getattr(model, "config", None), "eval_overlay", False))
    dev = eval_set.device
    lpips = model.lpips
    has_lpips = bool(getattr(lpips, "available", True))
    table = torch.zeros((n, 4 if has_lpips else 3), dtype=torch.float32, device=dev)
    planes = (torch.empty((1, 3, H, W), dtype=torch.float32, device=dev), torch.empty((1, 3, H, W), dtype=torch.float32, device=dev))
    stats = pair = None
    if events_only:
        stats = torch.empty(ops.log_scale_correct_workspace_bytes(H, W) // 8, dtype=torch.float64, device=dev)
        pair = (torch.empty(2, dtype=torch.float32, device=dev), torch.empty((1, 1, H, W), dtype=torch.float32, device=dev),
                torch.empty((1, 1, H, W), dtype=torch.float32, device=dev))
    C = 1 if events_only else 3
    ws = torch.empty((ops.image_metrics_workspace_bytes(1, C, H, W) + 7) // 8, dtype=torch.float64, device=dev)
    was_training = bool(model.training)
    if was_training:
        model.eval()
    try:
        t0 = time.perf_counter()
        for i in range(n):
            flat = evaluation._flatten_bundle(camera_bundle(eval_set, i))
            out = evaluation.render_flat(model, flat, check_overflow=False)
            rgb = out["rgb"].to(torch.float32).contiguous()
            gt_pl, pr_pl, _ = ops.eval_image_prep(d.images[i], rgb, None if d.msk is None else d.msk[i], event_stats=events_only,
                                                  out=planes, stats=stats)
            if events_only:
                _, corrected, gray = ops.log_scale_correct(gt_pl, rgb, stats, out=pair)
                a, b = gray, corrected
            else:
                a, b = gt_pl, pr_pl
            ops.image_metrics(a, b, out=table[i], workspace=ws)          # (ground truth, prediction): the reference's order
            if has_lpips:
                table[i, _LPIPS] = lpips(a.expand(-1, 3, -1, -1), b.expand(-1, 3, -1, -1)) if events_only else lpips(a, b)
            if on_image is not None or panels is not None:
                outputs = {k: v.reshape(H, W, -1) for k, v in out.items()}
                img_pair = (gray, corrected) if events_only else None
            if panels is not None:
                panels.add(i, outputs, gt_pl, pr_pl, img_pair)
            if on_image is not None:
                overlay = evaluation.make_overlay(gt_pl, pr_pl) if want_overlay else None
                on_image(i, outputs, _image_dict(outputs, gt_pl, pr_pl, img_pair, overlay))
        model.occupancy_grid.check_deferred_overflow()          # the one overflow read of the set
        table[:, _PSNR] = 10.0 * torch.log10(1.0 / table[:, _MSE])
        rows = torch.cat([table, table.mean(dim=0, keepdim=True)]).tolist()          # the one read-back
        seconds = time.perf_counter() - t0
    finally:
        if was_training:
            model.train()
    keys = [("psnr", _PSNR), ("ssim", _SSIM)] + ([("lpips", _LPIPS)] if has_lpips else [])
    per_image = [{k: float(r[c]) for k, c in keys} for r in rows[:n]]
    average = {k: float(rows[n][c]) for k, c in keys}
    average["num_rays_per_sec"] = n * H * W / seconds
    average["fps"] = n / seconds
    return average, per_image
