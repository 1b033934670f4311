"""An analytic scene with closed-form images, depths and normals: a sphere and an axis-aligned box inside [-1, 1]^3 on a white
background, float64 numpy throughout.  Imports nothing of the project and nothing of the oracle: the ground truth a trained field is
held to (tests/test_gpu_analytic_scene.py) must not come from a restatement of the code under test.  The helper itself is checked
against brute force in tests/test_analytic_scene_cpu.py.

Conventions, written out here independently of lsenerf_amd/cameras.py: a camera-to-world matrix [3, 4] holds the camera's x (right),
y (up) and z (backwards: the camera looks along -z) axes as columns and the eye as the fourth; pixel (y, x) has the camera-frame
direction ((x - cx) / fx, -(y - cy) / fy, -1), no half-pixel offset; world direction = R @ that, normalised.  ``t`` is the Euclidean
distance along the unit direction, never the z-depth.
"""
from __future__ import annotations

import numpy as np

# ---------------------------------------------------------------------------------------------------- geometry (asymmetric on purpose)
SPHERE_C = np.array([0.15, -0.10, 0.05])
SPHERE_R = 0.45
BOX_LO = np.array([-0.75, -0.70, -0.60])
BOX_HI = np.array([-0.35, -0.20, 0.30])
# face colours in the order (-x, +x, -y, +y, -z, +z)
BOX_COLOURS = np.array([[0.85, 0.20, 0.20], [0.20, 0.75, 0.25], [0.20, 0.30, 0.85],
                        [0.85, 0.80, 0.20], [0.75, 0.25, 0.80], [0.20, 0.75, 0.80]])
BACKGROUND = np.array([1.0, 1.0, 1.0])
BODY_NONE, BODY_SPHERE, BODY_BOX = 0, 1, 2

H, W = 48, 64
FX = FY = 70.0
CX, CY = W / 2, H / 2
GRAY = np.array([0.2989, 0.5870, 0.1140])          # the grey weights of csrc/metrics.hip and events.py

# the one training configuration the fixture generator (tests/golden/make_analytic_scene.py) and the GPU test share
CONFIG = dict(
    log2_hashmap_size=17, grid_resolution=64, grid_levels=1, render_step_size=None, cone_angle=0.004, alpha_thre=0.01,
    near_plane=0.05, background="white", num_embeddings=1, lr=1e-2, eps=1e-15, rays_per_step=1024, steps=400,
    occ_every=16, occ_warmup_steps=256, draw_seed=1234, init_seeds=(11, 12, 13), n_train=24, n_heldout=4, n_trajectory=8,
    height=H, width=W, fx=FX, fy=FY, lattice=48, event_threshold=0.1,
)


# ---------------------------------------------------------------------------------------------------- closed-form queries
def _sphere_hit(o, d):
    oc = o - SPHERE_C
    b = (oc * d).sum(-1)
    c = (oc * oc).sum(-1) - SPHERE_R ** 2
    disc = b * b - c
    ok = disc > 0
    root = np.sqrt(np.where(ok, disc, 0.0))
    t0, t1 = -b - root, -b + root
    t = np.where(t0 > 0, t0, t1)                 # an origin inside the sphere sees the far root
    return np.where(ok & (t > 0), t, np.inf)


def _box_hit(o, d):
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (BOX_LO - o) * inv, (BOX_HI - o) * inv
    par = d == 0                                  # parallel to a slab: inside it or never
    inside = (o >= BOX_LO) & (o <= BOX_HI)
    tmin = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(ta, tb))
    tmax = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(ta, tb))
    axis = tmin.argmax(-1)
    tn, tf = tmin.max(-1), tmax.min(-1)
    ok = (tn < tf) & (tn > 0)
    return np.where(ok, tn, np.inf), axis


def trace(origins, directions):
    """Nearest hit of rays (unit directions) -> t [N] (inf for a miss), colour [N, 3], outward normal [N, 3] (0 for a miss), body [N]."""
    o = np.asarray(origins, np.float64).reshape(-1, 3)
    d = np.asarray(directions, np.float64).reshape(-1, 3)
    ts = _sphere_hit(o, d)
    tb, axis = _box_hit(o, d)
    t = np.minimum(ts, tb)
    body = np.where(np.isfinite(t), np.where(ts <= tb, BODY_SPHERE, BODY_BOX), BODY_NONE)
    tt = np.where(np.isfinite(t), t, 0.0)
    p = o + tt[:, None] * d
    n_s = (p - SPHERE_C) / SPHERE_R
    sign = -np.sign(d[np.arange(len(d)), axis])   # the entry face looks against the ray
    n_b = np.zeros_like(p)
    n_b[np.arange(len(d)), axis] = sign
    face = 2 * axis + (sign > 0)
    normal = np.where((body == BODY_SPHERE)[:, None], n_s, np.where((body == BODY_BOX)[:, None], n_b, 0.0))
    colour = np.where((body == BODY_SPHERE)[:, None], 0.5 + 0.4 * n_s,
                      np.where((body == BODY_BOX)[:, None], BOX_COLOURS[face], BACKGROUND))
    return t, colour, normal, body


def _sdf_sphere(p):
    return np.linalg.norm(p - SPHERE_C, axis=-1) - SPHERE_R


def _sdf_box(p):
    q = np.abs(p - 0.5 * (BOX_LO + BOX_HI)) - 0.5 * (BOX_HI - BOX_LO)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)


def sdf(points):
    """Signed distance to the union of the two bodies, positive outside (exact: the bodies do not touch)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    return np.minimum(_sdf_sphere(p), _sdf_box(p))


def outward_normal(points):
    """Gradient of ``sdf``: unit vectors, away from the nearer body."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    v = p - SPHERE_C
    g_s = v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-300)
    c = p - 0.5 * (BOX_LO + BOX_HI)
    q = np.abs(c) - 0.5 * (BOX_HI - BOX_LO)
    out = np.maximum(q, 0.0)
    ln = np.linalg.norm(out, axis=-1, keepdims=True)
    g_out = np.sign(c) * out / np.maximum(ln, 1e-300)
    g_in = np.zeros_like(p)
    g_in[np.arange(len(p)), q.argmax(-1)] = 1.0
    g_b = np.where(ln > 0, g_out, np.sign(c) * g_in)
    return np.where((_sdf_sphere(p) <= _sdf_box(p))[:, None], g_s, g_b)


def surface_colour(points):
    """The analytic colour at the surface point nearest to each point."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = outward_normal(p)
    near_sphere = _sdf_sphere(p) <= _sdf_box(p)
    axis = np.abs(n).argmax(-1)
    face = 2 * axis + (n[np.arange(len(p)), axis] > 0)
    return np.where(near_sphere[:, None], 0.5 + 0.4 * n, BOX_COLOURS[face])


def surface_samples(n=2000):
    """Points on the two surfaces with their outward normals: ``n`` on the sphere (Fibonacci), a regular grid of about ``n`` on the
    box faces (cell centres, so no point lies on an edge).  -> points [M, 3], normals [M, 3], body [M]."""
    i = np.arange(n) + 0.5
    z = 1 - 2 * i / n
    phi = np.pi * (1 + 5 ** 0.5) * i
    r = np.sqrt(1 - z * z)
    ns = np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)
    pts, nrm, body = [SPHERE_C + SPHERE_R * ns], [ns], [np.full(n, BODY_SPHERE)]
    k = max(2, int(round((n / 6) ** 0.5)))
    u = (np.arange(k) + 0.5) / k
    uu, vv = np.meshgrid(u, u, indexing="ij")
    ext = BOX_HI - BOX_LO
    for axis in range(3):
        a, b = [x for x in range(3) if x != axis]
        for side in (0, 1):
            p = np.zeros((k * k, 3))
            p[:, axis] = BOX_HI[axis] if side else BOX_LO[axis]
            p[:, a] = BOX_LO[a] + uu.ravel() * ext[a]
            p[:, b] = BOX_LO[b] + vv.ravel() * ext[b]
            nn = np.zeros((k * k, 3))
            nn[:, axis] = 1.0 if side else -1.0
            pts.append(p), nrm.append(nn), body.append(np.full(k * k, BODY_BOX))
    return np.concatenate(pts), np.concatenate(nrm), np.concatenate(body)


# ---------------------------------------------------------------------------------------------------- cameras
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 0.0, 1.0)):
    """Camera-to-world [3, 4] float64: columns right, up, backwards, eye."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    return np.stack([right, np.cross(back, right), back, eye], 1)


def _fibonacci(n, radius, offset=0.5):
    i = np.arange(n) + offset
    z = 1 - 2 * i / n
    phi = np.pi * (1 + 5 ** 0.5) * i
    r = np.sqrt(1 - z * z)
    return radius * np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)


def train_cameras():
    """24 poses [24, 3, 4] on a Fibonacci sphere of radius 2.2, looking at the origin."""
    return np.stack([look_at(e) for e in _fibonacci(24, 2.2)])


def heldout_cameras():
    """4 poses at directions (12 - 21 degrees from the nearest training camera) and radii (2.0 - 2.4) no training camera has.
    They were picked among 33 candidates on a Fibonacci sphere with the trained ORACLE (tests/golden/make_analytic_scene.py), never
    with the code under test: the border of a held-out image looks through the periphery of the cube, which only the few training
    cameras nearly in line with it constrain, and a trained field may keep a floater there.  From these four every oracle seed
    separates hit from miss on every interior pixel (tests/test_analytic_scene_cpu.py holds the committed fixture to that)."""
    eyes = [(-0.685, 0.165, 0.709), (0.227, -0.920, 0.321), (0.262, 0.901, -0.346), (-0.829, 0.322, -0.457)]
    radii = [2.0, 2.2, 2.4, 2.1]
    return np.stack([look_at(np.asarray(e) / np.linalg.norm(e) * r) for e, r in zip(eyes, radii)])


def trajectory_cameras():
    """8 poses on a short arc at radius 2.2, consecutive ones 3 degrees apart, both bodies in view."""
    ang = np.deg2rad(-150.0 + 3.0 * np.arange(8))
    return np.stack([look_at((2.2 * np.cos(0.35) * np.cos(a), 2.2 * np.cos(0.35) * np.sin(a), 2.2 * np.sin(0.35))) for a in ang])


def pixel_rays(c2w, ys=None, xs=None):
    """Rays of one camera through pixels (ys, xs) (default: the whole image, row-major) -> origins [N, 3], unit directions [N, 3]."""
    if ys is None:
        ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ys, xs = np.asarray(ys, np.float64).ravel(), np.asarray(xs, np.float64).ravel()
    cam = np.stack([(xs - CX) / FX, -(ys - CY) / FY, -np.ones_like(xs)], -1)
    d = cam @ np.asarray(c2w, np.float64)[:, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(np.asarray(c2w, np.float64)[:, 3], d.shape).copy(), d


def optical_axis(c2w):
    return -np.asarray(c2w, np.float64)[:, 2]


# ---------------------------------------------------------------------------------------------------- images and event frames
def images(cameras):
    """-> dict: rgb8 uint8 [N, H, W, 3] = round(255 colour), rgb float64, t [N, H, W], normal [N, H, W, 3], hit bool, body int."""
    out = {k: [] for k in ("rgb", "t", "normal", "body")}
    for c2w in cameras:
        t, col, nrm, body = trace(*pixel_rays(c2w))
        out["rgb"].append(col.reshape(H, W, 3)), out["t"].append(t.reshape(H, W))
        out["normal"].append(nrm.reshape(H, W, 3)), out["body"].append(body.reshape(H, W))
    out = {k: np.stack(v) for k, v in out.items()}
    out["rgb8"] = np.rint(255.0 * out["rgb"]).astype(np.uint8)
    out["hit"] = out["body"] != BODY_NONE
    return out


def interior(id_map):
    """Pixels whose 3 x 3 neighbourhood (inside the image) has the same hit/miss state or body id.  [..., H, W] -> bool."""
    m = np.asarray(id_map)
    hh, ww = m.shape[-2:]
    pad = np.pad(m, [(0, 0)] * (m.ndim - 2) + [(1, 1), (1, 1)], mode="edge")     # neighbours outside the image do not count
    ok = np.ones(m.shape, bool)
    for dy in range(3):
        for dx in range(3):
            ok &= pad[..., dy:dy + hh, dx:dx + ww] == m
    return ok


def log_gray(rgb):
    return np.log((np.asarray(rgb, np.float64) * GRAY).sum(-1) + 1e-6)


def event_frames(rgb, threshold):
    """Analytic event frames between consecutive poses: (log(gray + 1e-6)_next - log(gray + 1e-6)_prev) / C.  [N, H, W, 3] -> [N-1, H, W]."""
    lg = log_gray(rgb)
    return (lg[1:] - lg[:-1]) / threshold


def psnr(a, b, mask=None):
    e = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    if mask is not None:
        e = e[mask]
    return float(-10.0 * np.log10(max(e.mean(), 1e-20)))


def err_stats(err):
    e = np.abs(np.asarray(err, np.float64).ravel())
    return dict(median=float(np.median(e)), p95=float(np.percentile(e, 95)), rmse=float(np.sqrt((e ** 2).mean())))


# ---------------------------------------------------------------------------------------------------- exported geometry against the scene
def mesh_stats(vertices, triangles, signed_volume, near=None):
    """|sdf| percentiles of a mesh's vertices, the share of its triangles whose geometric normal has a positive dot product with
    ``outward_normal`` at the centroid, and the sign of its ``signed_volume(vertices, triangles)``.  ``near``: also that share over
    the triangles whose centroid lies within ``near`` of the surface (a density field is unconstrained inside a body and where no
    camera looks, and its isosurface has sheets there that face anywhere)."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles).reshape(-1, 3)
    d = np.abs(sdf(v))
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    centroid = (a + b + c) / 3
    out = (np.cross(b - a, c - a) * outward_normal(centroid)).sum(-1)
    res = dict(sdf_p50=float(np.median(d)), sdf_p95=float(np.percentile(d, 95)), outward_share=float((out > 0).mean()),
               volume_sign=float(np.sign(signed_volume(v.astype(np.float32), t))), vertices=int(len(v)))
    if near is not None:
        close = np.abs(sdf(centroid)) < near
        res.update(outward_share_near=float((out[close] > 0).mean()), near_share=float(close.mean()))
    return res


def visible_surface_samples(cams, n=1500):
    """The ``surface_samples`` some camera of ``cams`` sees: the ray from its eye hits the sample first and the sample projects into
    the image."""
    pts, _, _ = surface_samples(n)
    seen = np.zeros(len(pts), bool)
    for c2w in cams:
        v = pts - c2w[:, 3]
        dist = np.linalg.norm(v, axis=-1)
        t = trace(np.broadcast_to(c2w[:, 3], pts.shape), v / dist[:, None])[0]
        pc = v @ c2w[:, :3]
        with np.errstate(divide="ignore", invalid="ignore"):
            x, y = FX * pc[:, 0] / -pc[:, 2] + CX, CY - FY * pc[:, 1] / -pc[:, 2]
        seen |= (np.abs(t - dist) < 1e-6) & (pc[:, 2] < 0) & (x >= 0) & (x <= W - 1) & (y >= 0) & (y <= H - 1)
    return pts[seen]


def cloud_stats(points, colours, samples, radius):
    """|sdf| percentiles of exported points, the rms of their colours against the analytic colour at the nearest surface point, and
    the share of ``samples`` (surface points) with an exported point within ``radius``."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    d = np.abs(sdf(p))
    near = np.array([((p - s) ** 2).sum(-1).min() for s in samples]) if len(p) else np.full(len(samples), np.inf)
    rms = float(np.sqrt(((np.asarray(colours, np.float64).reshape(-1, 3) - surface_colour(p)) ** 2).mean()))
    return dict(sdf_p50=float(np.median(d)), sdf_p95=float(np.percentile(d, 95)), coverage=float((near <= radius ** 2).mean()),
                colour_rms=rms, points=int(len(p)))
