"""TSDF mesh export: a mesh of what the cameras see of a trained field.  Per view an eval render (``evaluation.render_flat``) whose
depth, accumulation and colour are staged; per batch of views one ``ops.tsdf_integrate`` folds them into a truncated signed distance
and a colour per lattice point; then surface nets that skip unobserved cells (``ops.surface_nets(..., skip_nan=True)``), fused or
field colours and analytic normals at the vertices.  The definitions are in include/lse_hip.h ("TSDF fusion").  Everything stays on
the device: the only host reads are the occupancy grid's overflow check behind the last view and the pair of surface-nets totals."""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch import Tensor

from . import evaluation, ops
from . import mesh as _mesh

COLOR_MODES = ("fused", "field", None)


def border_r2_max(cam_desc) -> float:
    """``r2_max`` of ``ops.tsdf_integrate`` for the camera ``cam_desc``: the largest ``X^2 + Y^2`` over the undistorted camera points
    (``cameras.radial_and_tangential_undistort``) of the image's border pixels -- the radius beyond which the distortion polynomial
    may fold far-off points back into the image; ``+inf`` for a pinhole camera.  Pure host code."""
    if not cam_desc.distort:
        return float("inf")
    from .cameras import radial_and_tangential_undistort
    H, W = int(cam_desc.H), int(cam_desc.W)
    xs, ys = torch.arange(W, dtype=torch.float32), torch.arange(H, dtype=torch.float32)
    x = torch.cat([xs, xs, torch.zeros(H), torch.full((H,), float(W - 1))])
    y = torch.cat([torch.zeros(W), torch.full((W,), float(H - 1)), ys, ys])
    xy = torch.stack([(x - cam_desc.cx) / cam_desc.fx, -(y - cam_desc.cy) / cam_desc.fy], -1)
    dist = torch.tensor([float(v) for v in cam_desc.dist], dtype=torch.float32)
    u = radial_and_tangential_undistort(xy, dist.expand(xy.shape[0], 6))
    return float((u * u).sum(-1).max())


class TSDFVolume:
    """The fusion state on the points of the ``resolution``-cell lattice over ``lo .. hi`` (point order: ``ops.lattice_positions``):
    ``tw`` [points, 2] = (tsdf, weight) and, with ``colors``, ``cw`` [points, 4] = (r, g, b, colour weight), zero at the start."""

    def __init__(self, resolution, lo, hi, truncation: float, device, colors: bool = True):
        self.res = ops._res3(resolution)
        self.lo, self.hi = [float(v) for v in lo], [float(v) for v in hi]
        self.truncation = float(truncation)
        if not self.truncation > 0.0:
            raise ValueError(f"truncation {truncation} <= 0")
        n = ops.lattice_points(self.res)
        self.tw = torch.zeros((n, 2), dtype=torch.float32, device=device)
        self.cw = torch.zeros((n, 4), dtype=torch.float32, device=device) if colors else None

    @torch.no_grad()
    def integrate(self, cam_desc, poses: Tensor, depth: Tensor, acc: Tensor, rgb: Optional[Tensor] = None,
                  min_accumulation: float = 0.5, carve: bool = True, r2_max: Optional[float] = None) -> None:
        """Folds the views ``poses`` [V, 3, 4] with ``depth``, ``acc`` [V, H * W] (and ``rgb`` [V, H * W, 3]) into the state, in
        order, with one launch.  A pixel below ``min_accumulation`` marks the points on its ray as observed empty when ``carve``, and
        is ignored otherwise.  ``r2_max``: ``border_r2_max(cam_desc)`` unless given."""
        if r2_max is None:
            r2_max = border_r2_max(cam_desc)
        ops.tsdf_integrate(self.tw, self.cw, self.res, self.lo, self.hi, cam_desc, poses, depth, acc,
                           rgb if self.cw is not None else None, self.truncation, min_accumulation, carve, r2_max)

    @torch.no_grad()
    def field(self, min_weight: float = 1) -> Tensor:
        """float32 [points]: ``-tsdf`` (positive behind the surface) where ``weight >= min_weight``, NaN -- unobserved -- elsewhere."""
        return torch.where(self.tw[:, 1] >= float(min_weight), -self.tw[:, 0], self.tw.new_tensor(float("nan")))

    @torch.no_grad()
    def extract(self, min_weight: float = 1) -> Tuple[Tensor, Tensor, Tensor]:
        """``(vertices, triangles, totals)`` of the zero crossing of ``field(min_weight)``, without a surface against unobserved space
        (one host read: the totals)."""
        return ops.surface_nets(self.field(min_weight), self.res, self.lo, self.hi, 0.0, skip_nan=True)

    @torch.no_grad()
    def vertex_colors(self, vertices: Tensor) -> Tensor:
        if self.cw is None:
            raise ValueError("this volume was built without colours")
        return ops.tsdf_vertex_colors(self.cw, self.res, self.lo, self.hi, vertices)


def _views(views, image_indices):
    """(EvalSet or None, cameras, poses, indices) of ``views`` after the range check of ``image_indices``; nothing is moved yet."""
    from .eval_set import EvalSet
    if isinstance(views, EvalSet):
        es, cameras, poses, n = views, views.cameras, views.poses, len(views)
    else:
        try:
            cameras, poses = views
        except (TypeError, ValueError):
            raise ValueError("views: an EvalSet or a pair (EdCameras, poses [n, 3, 4]) expected") from None
        if not torch.is_tensor(poses) or poses.dim() != 3 or tuple(poses.shape[1:]) != (3, 4):
            raise ValueError(f"poses: [n, 3, 4] expected, got {tuple(getattr(poses, 'shape', ()))}")
        es, n = None, poses.shape[0]
    idx = list(range(n)) if image_indices is None else [int(i) for i in image_indices]
    for i in idx:
        if not 0 <= i < n:
            raise ValueError(f"image index {i} of {n}")
    return es, cameras, poses, idx


def export_tsdf_mesh(model, views, image_indices=None, resolution=256, bounds=None, truncation: Optional[float] = None,
                     min_accumulation: float = 0.5, carve: bool = True, min_weight: float = 1, colors: Optional[str] = "fused",
                     normals: bool = True, views_per_launch: int = 8, depth: str = "expected",
                     max_depth_spread: Optional[float] = None) -> _mesh.Mesh:
    """Mesh of the surface ``views`` see of ``model``'s field, by TSDF fusion of eval depth renders.  ``views``: an
    ``eval_set.EvalSet`` (its camera, pose table and the camera of every image) or a pair ``(EdCameras, poses [n, 3, 4])``;
    ``image_indices`` selects and orders the images / poses (order is part of the definition: views are folded one after the other).
    The volume is a lattice of ``resolution`` cells (an int or three) over ``bounds`` ([2, 3]; default: the field's aabb) with the
    truncation distance ``truncation`` (default: 3 x the longest voxel edge).  A pixel whose accumulation is at least
    ``min_accumulation`` gives a surface at its depth; other pixels carve the points on their ray as observed empty (``carve``) or
    are ignored.  Points fewer than ``min_weight`` views updated are unobserved: no vertex in a cell with such a corner, no quad next
    to such a cell, so the mesh is open where observation ends.  ``colors``: ``"fused"`` -- the mean of the renders' rgb at every
    lattice point, blended at the vertices (``render_flat``'s rgb has passed the model's output mapping already, so
    ``mesh.eval_colour_mapping`` is not applied again); ``"field"`` -- ``mesh.vertex_colors``, the field's colour seen against the
    normal; ``None``.  ``normals``: ``mesh.vertex_normals``.  ``views_per_launch``: views per integration launch; it does not change
    a bit.  ``depth``: ``"expected"`` -- the render's "depth" -- or ``"median"`` -- the interpolated depth at which the accumulated
    weight crosses one half (``pointcloud.export_point_cloud`` has the definition; ``config.eval_depth_quantiles`` and
    ``eval_depth_interpolate`` are set for the duration): a pixel whose weights never reach one half, or -- with
    ``max_depth_spread`` -- whose quartile depths lie further apart, has no usable depth and is skipped without carving.  Runs
    without gradients in eval mode with ``config.eval_normals`` off, and puts the settings and every module's mode back; an
    early-stop eval render is used as it is."""
    from .events import _camera_desc, _check_poses, _eval_no_grad
    from .eval_set import camera_bundle, pose_bundle
    from .pointcloud import MEDIAN_COLUMN, depth_mode, median_settings
    median, spread = depth_mode(depth, max_depth_spread)
    if colors not in COLOR_MODES:
        raise ValueError(f"colors {colors!r}: one of {COLOR_MODES} expected")
    vpl = int(views_per_launch)
    if vpl < 1:
        raise ValueError(f"views_per_launch {views_per_launch} < 1")
    res = ops._res3(resolution)
    if min(res) < 1 or ops.lattice_points(res) >= 1 << 31:
        raise ValueError(f"resolution {res}: every count >= 1 and fewer than 2^31 points")
    lo, hi = _mesh._bounds(model.field, bounds)
    if truncation is None:
        truncation = 3.0 * max((h - l) / n for l, h, n in zip(lo, hi, res))
    truncation = float(truncation)
    if not truncation > 0.0:
        raise ValueError(f"truncation {truncation} <= 0")
    es, cameras, poses, idx = _views(views, image_indices)

    dev = model.scene_aabb.device
    if es is not None:
        desc, H, W = es.cam_desc, es.data.H, es.data.W
        table = es.poses
        cam_of = [int(es.data.image_idx_host[i]) for i in idx]
    else:
        desc, H, W = _camera_desc(cameras), cameras.height, cameras.width
        table = _check_poses(poses, dev)
        cam_of = idx
        app = torch.zeros(1, dtype=torch.int32, device=dev)
        rows = {k: v[0].to(dev) for k, v in (cameras.metadata or {}).items() if torch.is_tensor(v)}
    r2_max = border_r2_max(desc)
    with _eval_no_grad(model), median_settings(model.config, median):
        vol = TSDFVolume(res, lo, hi, truncation, dev, colors=colors == "fused")
        fuse = vol.cw is not None
        pose_b = torch.empty((vpl, 3, 4), dtype=torch.float32, device=dev)
        depth_b = torch.empty((vpl, H * W), dtype=torch.float32, device=dev)
        acc_b = torch.empty((vpl, H * W), dtype=torch.float32, device=dev)
        rgb_b = torch.empty((vpl, H * W, 3), dtype=torch.float32, device=dev) if fuse else None

        def flush(k: int) -> None:
            vol.integrate(desc, pose_b[:k], depth_b[:k], acc_b[:k], rgb_b[:k] if fuse else None, min_accumulation, carve, r2_max)

        k = 0
        for i, cam in zip(idx, cam_of):
            bundle = camera_bundle(es, i) if es is not None else pose_bundle(desc, table[cam], H, W, 0, app, None, rows)
            flat = evaluation._flatten_bundle(bundle, device=dev)
            if median:
                out = evaluation.render_flat(model, flat, check_overflow=False, depth_select=(MEDIAN_COLUMN, spread))
            else:
                out = evaluation.render_flat(model, flat, check_overflow=False)
            pose_b[k].copy_(table[cam])
            depth_b[k].copy_(out["depth_selected" if median else "depth"].reshape(-1))
            acc_b[k].copy_(out["accumulation"].reshape(-1))
            if fuse:
                rgb_b[k].copy_(out["rgb"].reshape(-1, 3))
            k += 1
            if k == vpl:
                flush(k)
                k = 0
        if k:
            flush(k)
        if idx:
            model.occupancy_grid.check_deferred_overflow()      # the read render_flat left out: once, behind the last view
        vertices, triangles, _ = vol.extract(min_weight)         # the one read of the surface-nets totals
        nrm = _mesh.vertex_normals(model.field, vertices) if (normals or colors == "field") else None
        if colors == "fused":
            col = vol.vertex_colors(vertices)
        elif colors == "field":
            col = _mesh.vertex_colors(model, vertices, nrm)
        else:
            col = None
    return _mesh.Mesh(vertices, triangles, nrm if normals else None, col)
