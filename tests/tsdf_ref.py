"""numpy twin of the TSDF-fusion definition in include/lse_hip.h ("TSDF fusion"): the integration of a batch of views, the field
handed to surface nets, surface nets that skip unobserved cells, and the fused vertex colours -- plus the analytic sphere scene of
tests/test_tsdf_cpu.py and the GPU tests of csrc/tsdf.hip.  Not a test file.

Every numpy operation on float32 arrays rounds once, as the kernels built without FMA contraction do; numpy's float32 division and
square root are correctly rounded, and ``np.rint`` rounds ties to even like ``rintf``."""
from __future__ import annotations

from dataclasses import dataclass, field as _dc_field
from typing import Optional, Tuple

import numpy as np

from tests import mesh_ref as mr

F = np.float32


@dataclass
class Camera:
    """What ``lse_camera_desc`` holds."""
    fx: float
    fy: float
    cx: float
    cy: float
    H: int
    W: int
    dist: Tuple[float, ...] = _dc_field(default_factory=lambda: (0.0,) * 6)      # (k1, k2, k3, k4, p1, p2)

    @property
    def distort(self) -> bool:
        return any(v != 0.0 for v in self.dist)


def new_state(res, colors: bool = True):
    n = int(np.prod([r + 1 for r in mr._res3(res)]))
    return np.zeros((n, 2), dtype=F), (np.zeros((n, 4), dtype=F) if colors else None)


# ---------------------------------------------------------------------------------------------------- integration
def integrate(tw, cw, res, lo, hi, cam: Camera, poses, depth, acc, rgb=None, truncation=0.25, min_acc=0.5, carve=True,
              r2_max=np.inf):
    """lse_tsdf_integrate: folds the views of ``poses`` [V, 3, 4] in ascending order into copies of ``tw`` [P, 2] and ``cw`` [P, 4]
    (or None); ``depth``, ``acc`` [V, H * W], ``rgb`` [V, H * W, 3] or None.  Returns the new (tw, cw)."""
    x = mr.lattice_positions(res, lo, hi)                                  # float32, the kernel's arithmetic
    tw = np.array(tw, dtype=F, copy=True)
    fuse = cw is not None and rgb is not None
    cw = None if cw is None else np.array(cw, dtype=F, copy=True)
    poses = np.asarray(poses, dtype=F).reshape(-1, 3, 4)
    depth = np.asarray(depth, dtype=F).reshape(poses.shape[0], -1)
    acc = np.asarray(acc, dtype=F).reshape(poses.shape[0], -1)
    if rgb is not None:
        rgb = np.asarray(rgb, dtype=F).reshape(poses.shape[0], -1, 3)
    trunc, min_acc, r2_max = F(truncation), F(min_acc), F(r2_max)
    fx, fy, cx, cy = F(cam.fx), F(cam.fy), F(cam.cx), F(cam.cy)
    k1, k2, k3, k4, p1, p2 = (F(v) for v in cam.dist)
    one, two, zero = F(1), F(2), F(0)
    with np.errstate(all="ignore"):
        for j in range(poses.shape[0]):
            M = poses[j]
            v0, v1, v2 = x[:, 0] - M[0, 3], x[:, 1] - M[1, 3], x[:, 2] - M[2, 3]
            xc = (v0 * M[0, 0] + v1 * M[1, 0]) + v2 * M[2, 0]
            yc = (v0 * M[0, 1] + v1 * M[1, 1]) + v2 * M[2, 1]
            zc = (v0 * M[0, 2] + v1 * M[1, 2]) + v2 * M[2, 2]
            z = -zc
            ok = z > zero
            X, Y = xc / z, yc / z
            if cam.distort:
                r = X * X + Y * Y
                ok &= r <= r2_max
                d = one + r * (k1 + r * (k2 + r * (k3 + r * k4)))
                xd = (d * X + ((two * p1) * X) * Y) + p2 * (r + (two * X) * X)
                yd = (d * Y + ((two * p2) * X) * Y) + p1 * (r + (two * Y) * Y)
                X, Y = xd, yd
            u, v = np.rint(X * fx + cx), np.rint(cy - Y * fy)
            ok &= (u >= zero) & (u < F(cam.W)) & (v >= zero) & (v < F(cam.H))
            pix = np.where(ok, v, zero).astype(np.int64) * cam.W + np.where(ok, u, zero).astype(np.int64)
            dp, a = depth[j][pix], acc[j][pix]
            dist = np.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
            surface = a >= min_acc
            sdf = np.where(surface, dp - dist, F(np.inf))
            ok &= np.where(surface, (dp > zero) & (dp < F(np.inf)), bool(carve))
            ok &= ~(sdf < -trunc)
            t = np.fmin(one, sdf / trunc)
            new_t = (tw[:, 0] * tw[:, 1] + t) / (tw[:, 1] + one)
            new_w = tw[:, 1] + one
            tw[:, 0], tw[:, 1] = np.where(ok, new_t, tw[:, 0]), np.where(ok, new_w, tw[:, 1])
            if fuse:
                okc = ok & surface & (sdf <= trunc)
                q = rgb[j][pix]
                for k in range(3):
                    cw[:, k] = np.where(okc, (cw[:, k] * cw[:, 3] + q[:, k]) / (cw[:, 3] + one), cw[:, k])
                cw[:, 3] = np.where(okc, cw[:, 3] + one, cw[:, 3])
    return tw, cw


def field(tw, min_weight=1) -> np.ndarray:
    """-tsdf where weight >= min_weight, NaN elsewhere."""
    tw = np.asarray(tw, dtype=F)
    return np.where(tw[:, 1] >= F(min_weight), -tw[:, 0], F(np.nan)).astype(F)


# ---------------------------------------------------------------------------------------------------- masked surface nets
def cell_masks(sigma, res, level=0.0):
    """(mixed, nan_corner): boolean [cells] in cell order -- the cell's corners are neither all inside nor all outside; one of its 8
    corners is NaN."""
    nx, ny, nz = mr._res3(res)
    S = np.asarray(sigma, dtype=F).reshape(nx + 1, ny + 1, nz + 1)
    with np.errstate(invalid="ignore"):
        inside = S > F(level)
    nan = np.isnan(S)
    cnt = np.zeros((nx, ny, nz), dtype=np.int32)
    bad = np.zeros((nx, ny, nz), dtype=bool)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cnt += inside[dx:dx + nx, dy:dy + ny, dz:dz + nz]
                bad |= nan[dx:dx + nx, dy:dy + ny, dz:dz + nz]
    return ((cnt != 0) & (cnt != 8)).ravel(), bad.ravel()


def surface_nets(sigma, res, lo, hi, level=0.0, skip_nan=True, with_cells=False):
    """(vertices, triangles) of LSE_NETS_SKIP_NAN: the unmasked mesh (``mesh_ref.surface_nets``: a vertex depends on its own cell's
    corners only, and vertices and quads are ordered) without the vertices of cells with a NaN corner and without the quads that
    touch a dropped cell, vertex ids renumbered in order.  ``with_cells``: also the cell index of every vertex."""
    v, t = mr.surface_nets(sigma, res, lo, hi, level)
    mixed, bad = cell_masks(sigma, res, level)
    cells = np.flatnonzero(mixed)
    assert cells.shape[0] == v.shape[0]
    if not skip_nan:
        return (v, t, cells) if with_cells else (v, t)
    keep_v = ~bad[cells]
    new_id = (np.cumsum(keep_v) - 1).astype(np.int32)
    quads = t.reshape(-1, 6)
    keep_q = keep_v[quads[:, [0, 1, 2, 5]]].all(axis=1) if quads.shape[0] else np.zeros(0, dtype=bool)
    t2 = new_id[quads[keep_q]].reshape(-1, 3).astype(np.int32)
    return (v[keep_v], t2, cells[keep_v]) if with_cells else (v[keep_v], t2)


# ---------------------------------------------------------------------------------------------------- vertex colours
def vertex_colors(cw, res, lo, hi, vertices) -> np.ndarray:
    """lse_tsdf_vertex_colors: [n, 3] float32."""
    n3 = mr._res3(res)
    cw = np.asarray(cw, dtype=F).reshape(n3[0] + 1, n3[1] + 1, n3[2] + 1, 4)
    vtx = np.asarray(vertices, dtype=F).reshape(-1, 3)
    lo, hi = np.asarray(lo, dtype=F), np.asarray(hi, dtype=F)
    one, zero = F(1), F(0)
    cc, f = [], []
    with np.errstate(all="ignore"):
        for k in range(3):
            u = ((vtx[:, k] - lo[k]) / (hi[k] - lo[k])) * F(n3[k])
            fl = np.floor(u)
            c = np.where(fl >= F(n3[k] - 1), n3[k] - 1, np.where(fl > zero, fl, zero).astype(np.int64)).astype(np.int64)
            cc.append(c)
            f.append(np.fmin(np.fmax(u - c.astype(F), zero), one))
        s = np.zeros((vtx.shape[0], 3), dtype=F)
        W = np.zeros(vtx.shape[0], dtype=F)
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    c = cw[cc[0] + dx, cc[1] + dy, cc[2] + dz]
                    wt = ((f[0] if dx else one - f[0]) * (f[1] if dy else one - f[1])) * (f[2] if dz else one - f[2])
                    has = c[:, 3] > zero
                    s = np.where(has[:, None], s + wt[:, None] * c[:, :3], s)
                    W = np.where(has, W + wt, W)
        return np.where((W > zero)[:, None], s / W[:, None], zero).astype(F)


# ---------------------------------------------------------------------------------------------------- the sphere scene
CENTRE, RADIUS = (0.07, -0.05, 0.11), 0.5


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)) -> np.ndarray:
    """Pose [3, 4] float32 (camera to world) of a camera at ``eye`` that looks along its -z at ``target``."""
    eye, target, up = (np.asarray(a, dtype=np.float64) for a in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    if abs(back @ up) > 0.999:
        up = np.array([0.0, 1.0, 0.0])
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    return np.concatenate([np.stack([right, np.cross(back, right), back], axis=1), eye[:, None]], axis=1).astype(F)


def undistort64(cam: Camera, xd, yd):
    """Newton inverse of the forward distortion model in float64 (what ``undistort()`` of csrc/compose.hip iterates)."""
    k1, k2, k3, k4, p1, p2 = cam.dist
    x, y = xd.copy(), yd.copy()
    for _ in range(20):
        r = x * x + y * y
        d = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
        gx = d * x + 2 * p1 * x * y + p2 * (r + 2 * x * x) - xd
        gy = d * y + 2 * p2 * x * y + p1 * (r + 2 * y * y) - yd
        d_r = k1 + r * (2 * k2 + r * (3 * k3 + r * 4 * k4))
        a, b = d + 2 * x * x * d_r + 2 * p1 * y + 6 * p2 * x, 2 * x * y * d_r + 2 * p1 * x + 2 * p2 * y
        c, e = 2 * x * y * d_r + 2 * p2 * y + 2 * p1 * x, d + 2 * y * y * d_r + 2 * p2 * x + 6 * p1 * y
        det = a * e - b * c
        x, y = x - (gx * e - gy * b) / det, y - (gy * a - gx * c) / det
    return x, y


def camera_points64(cam: Camera):
    """Undistorted camera-frame points (x, y) [H * W] of the integer pixel coordinates, row-major."""
    py, px = np.meshgrid(np.arange(cam.H, dtype=np.float64), np.arange(cam.W, dtype=np.float64), indexing="ij")
    x, y = ((px - cam.cx) / cam.fx).ravel(), (-(py - cam.cy) / cam.fy).ravel()
    return undistort64(cam, x, y) if cam.distort else (x, y)


def border_r2_max(cam: Camera) -> float:
    """r2_max of ``cam``: the largest X^2 + Y^2 over the undistorted camera points of the border pixels; +inf for a pinhole."""
    if not cam.distort:
        return float("inf")
    x, y = camera_points64(cam)
    r = (x * x + y * y).reshape(cam.H, cam.W)
    return float(max(r[0].max(), r[-1].max(), r[:, 0].max(), r[:, -1].max()))


def render_sphere(cam: Camera, pose, centre=CENTRE, radius=RADIUS):
    """(depth [H * W], acc [H * W], rgb [H * W, 3]) float32 of the sphere seen through ``pose``: the Euclidean distance to the first
    hit along the pixel's unit ray, accumulation 1 on a hit and 0 elsewhere (depth 0 there), colour 0.5 + 0.5 * outward normal."""
    x, y = camera_points64(cam)
    pose = np.asarray(pose, dtype=np.float64)
    d = np.stack([x, y, -np.ones_like(x)], axis=1) @ pose[:, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    oc = pose[:, 3] - np.asarray(centre, dtype=np.float64)
    b = d @ oc
    disc = b * b - (oc @ oc - radius * radius)
    hit = (disc > 0) & (-b - np.sqrt(np.maximum(disc, 0)) > 0)
    t = np.where(hit, -b - np.sqrt(np.maximum(disc, 0)), 0.0)
    nrm = (pose[:, 3] + t[:, None] * d - np.asarray(centre)) / radius
    rgb = np.where(hit[:, None], 0.5 + 0.5 * nrm, 0.0)
    return t.astype(F), hit.astype(F), rgb.astype(F)


def render_views(cam: Camera, poses, centre=CENTRE, radius=RADIUS):
    out = [render_sphere(cam, p, centre, radius) for p in poses]
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def sphere_distance(vertices, centre=CENTRE, radius=RADIUS) -> np.ndarray:
    """| |v - centre| - radius | per vertex, float64."""
    v = np.asarray(vertices, dtype=np.float64)
    return np.abs(np.linalg.norm(v - np.asarray(centre), axis=1) - radius)
