"""Point-cloud export: what the cameras see of a trained field, as one cloud.  Per view an eval render (``evaluation.render_flat``)
and ``ops.unproject_append`` (depth -> world point, validity filter, ordered append behind a device count); then, optionally, one
point per voxel (``ops.voxel_keys``, a stable sort, ``ops.voxel_merge``) and the removal of voxels without neighbours -- the
"floaters" semi-transparent rays leave in mid-air (``ops.voxel_support_filter``).  The definitions are in include/lse_hip.h
("point-cloud export").  Everything stays on the device and nothing waits for it until the last stage is enqueued: the only host
reads are the occupancy grid's overflow check behind the last view and the final count that trims the arrays."""
from __future__ import annotations

import contextlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
from torch import Tensor

from . import evaluation, ops
from .mesh import _bounds, _np


@dataclass
class PointCloud:
    points: Tensor                     # [n, 3] float32, world coordinates
    colors: Optional[Tensor] = None    # [n, 3] float32 in [0, 1]: the eval render's mapped rgb
    normals: Optional[Tensor] = None   # [n, 3] float32: unit vectors, zero where the density gradient is
    counts: Optional[Tensor] = None    # [n] int32: raw points merged into each point (with voxel_size only)


DEPTH_MODES = ("expected", "median")
MEDIAN_QUANTILES, MEDIAN_COLUMN = (0.25, 0.5, 0.75), 1      # what ``depth="median"`` renders, and the column it uses


def depth_mode(depth: str, max_depth_spread: Optional[float]):
    """(median?, max spread or None) of an exporter's ``depth`` / ``max_depth_spread`` arguments, validated."""
    if depth not in DEPTH_MODES:
        raise ValueError(f"depth {depth!r}: one of {DEPTH_MODES} expected")
    if max_depth_spread is None:
        return depth == "median", None
    if depth != "median":
        raise ValueError("max_depth_spread compares quantile depths: it needs depth='median'")
    spread = float(max_depth_spread)
    if not spread >= 0.0:
        raise ValueError(f"max_depth_spread {max_depth_spread} is negative or NaN")
    return True, spread


@contextlib.contextmanager
def median_settings(cfg, median: bool):
    """``cfg.eval_depth_quantiles`` / ``eval_depth_interpolate`` as ``depth="median"`` renders, for the duration; both come back, also
    behind an exception.  Without ``median`` the configuration is not written."""
    if not median:
        yield
        return
    saved = (cfg.eval_depth_quantiles, cfg.eval_depth_interpolate)
    try:
        cfg.eval_depth_quantiles, cfg.eval_depth_interpolate = MEDIAN_QUANTILES, True
        yield
    finally:
        cfg.eval_depth_quantiles, cfg.eval_depth_interpolate = saved


def _views(views, image_indices):
    """The bundles to render, lazily, and their total ray count."""
    from .eval_set import EvalSet, camera_bundle
    if isinstance(views, EvalSet):
        idx = list(range(len(views))) if image_indices is None else [int(i) for i in image_indices]
        for i in idx:
            if not 0 <= i < len(views):
                raise ValueError(f"image index {i} of {len(views)}")
        rays = len(idx) * views.data.H * views.data.W
        return (camera_bundle(views, i) for i in idx), rays
    if image_indices is not None:
        raise ValueError("image_indices selects images of an EvalSet")
    bundles = list(views)
    return iter(bundles), sum(int(b.origins.numel()) // 3 for b in bundles)


def export_point_cloud(model, views, image_indices=None, min_accumulation: float = 0.9, bounds=None,
                       voxel_size: Optional[float] = None, min_support: int = 0, normals: bool = True, colors: bool = True,
                       max_points: Optional[int] = None, depth: str = "expected",
                       max_depth_spread: Optional[float] = None) -> PointCloud:
    """Point cloud of ``model``'s field seen from ``views``: an ``eval_set.EvalSet`` (all images, or ``image_indices``) or an iterable
    of ray bundles of any leading shape.  A ray gives a point ``origin + direction * depth`` when its accumulation is at least
    ``min_accumulation``, its depth is positive and finite and the point lies inside ``bounds`` ([2, 3]; default: the field's aabb);
    points come in view order, rays in row-major order.  ``voxel_size``: merge the points of every voxel of that size into their
    mean (colours averaged, normals averaged and renormalised, ``counts`` = points merged; voxels in ascending key).  ``min_support``
    (needs ``voxel_size``): drop voxels whose 3 x 3 x 3 neighbourhood holds fewer raw points.  ``normals``: analytic world-space
    normals of the render -- ``config.eval_normals = "world"`` and ``config.eval_early_stop_eps = 0`` for the duration of the call
    (normals are not built for the segment route); ``colors``: the render's mapped rgb.  ``max_points``: capacity of the raw cloud
    (default: every ray, so nothing can be dropped; beyond it rays are dropped in order).  ``depth``: ``"expected"`` -- the render's
    "depth", the mean of the weights -- or ``"median"`` -- the depth at which the accumulated weight crosses one half, interpolated
    inside the sample (``config.eval_depth_quantiles = (0.25, 0.5, 0.75)`` and ``eval_depth_interpolate`` for the duration): on a
    silhouette or behind a half-transparent floater the mean lies between two surfaces, the median on one of them; a ray whose
    weights never reach one half gives no point.  ``max_depth_spread`` (median only): also drop rays whose quartile depths lie
    further apart -- smeared surfaces.  Runs without gradients in eval mode and puts the settings and every module's mode back."""
    median, spread = depth_mode(depth, max_depth_spread)
    lo, hi = _bounds(model.field, bounds)
    if voxel_size is not None:
        res = ops.voxel_lattice(lo, hi, voxel_size)
    min_support = int(min_support)
    if min_support > 0 and voxel_size is None:
        raise ValueError("min_support needs voxel_size: support is counted over the voxel lattice")
    bundles, n_rays = _views(views, image_indices)
    cap = n_rays if max_points is None else int(max_points)
    if cap < 0:
        raise ValueError(f"max_points {max_points} < 0")
    dev = model.scene_aabb.device
    cfg = model.config
    saved = (cfg.eval_normals, cfg.eval_early_stop_eps)
    modes = [(m, m.training) for m in model.modules()]
    model.eval()
    try:
        if normals:
            cfg.eval_normals, cfg.eval_early_stop_eps = "world", 0.0
        with torch.no_grad(), median_settings(cfg, median):
            new3 = lambda on: torch.empty((cap, 3), dtype=torch.float32, device=dev) if on else None
            pts, col, nrm = new3(True), new3(colors), new3(normals)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            ws = None
            for bundle in bundles:
                rb = evaluation._flatten_bundle(bundle, device=dev)
                if median:
                    out = evaluation.render_flat(model, rb, check_overflow=False, depth_select=(MEDIAN_COLUMN, spread))
                else:
                    out = evaluation.render_flat(model, rb, check_overflow=False)
                if normals and "normals" not in out:
                    raise ValueError("this model's eval render has no normals (they need the count-free route): pass normals=False")
                if ws is None or ws.numel() < ops.unproject_workspace_bytes(len(rb)):
                    ws = torch.empty(ops.unproject_workspace_bytes(len(rb)), dtype=torch.uint8, device=dev)
                ops.unproject_append(rb.origins.contiguous(), rb.directions.contiguous(),
                                     out["depth_selected" if median else "depth"].reshape(-1).contiguous(),
                                     out["accumulation"].reshape(-1).contiguous(), lo, hi, min_accumulation, pts, total,
                                     colors=out["rgb"].contiguous() if colors else None,
                                     normals=out["normals"].contiguous() if normals else None, out_colors=col, out_normals=nrm,
                                     workspace=ws)
            model.occupancy_grid.check_deferred_overflow()      # the read render_flat left out: once, behind the last view
            counts = None
            if voxel_size is not None:
                keys = ops.voxel_keys(pts, lo, voxel_size, res, n_dev=total)
                sorted_keys, order = torch.sort(keys, stable=True)
                keys, counts, pts, col, nrm, total = ops.voxel_merge(sorted_keys, order, pts, col, nrm)
                if min_support > 0:
                    keys, counts, pts, col, nrm, total, _ = ops.voxel_support_filter(keys, counts, pts, res, min_support, col, nrm,
                                                                                    m_dev=total)
            n = min(int(total.item()), cap)                     # the read that trims the arrays
    finally:
        if normals:
            cfg.eval_normals, cfg.eval_early_stop_eps = saved
        for m, was in modes:
            m.training = was
    cut = lambda t: None if t is None else t[:n]
    return PointCloud(pts[:n], cut(col), cut(nrm), cut(counts))


def write_ply_points(path: str, cloud: PointCloud) -> None:
    """Binary little-endian PLY of vertices only: ``x y z`` (float), ``nx ny nz`` (float) when the cloud has normals, ``red green
    blue`` (uchar, round(255 c)) when it has colours -- the property names and colour rounding of ``mesh.write_ply``; no face
    element."""
    v = _np(cloud.points, "<f4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    props = ["property float x", "property float y", "property float z"]
    if cloud.normals is not None:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        props += ["property float nx", "property float ny", "property float nz"]
    if cloud.colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        props += ["property uchar red", "property uchar green", "property uchar blue"]
    rec = np.zeros(v.shape[0], dtype=np.dtype(fields))
    for k, name in enumerate("xyz"):
        rec[name] = v[:, k]
    if cloud.normals is not None:
        n = _np(cloud.normals, "<f4").reshape(-1, 3)
        for k, name in enumerate(("nx", "ny", "nz")):
            rec[name] = n[:, k]
    if cloud.colors is not None:
        c = np.rint(np.clip(_np(cloud.colors, "<f4").reshape(-1, 3), 0.0, 1.0) * 255.0).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = c[:, k]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}", *props, "end_header"]
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(rec.tobytes())
