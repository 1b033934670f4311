"""numpy twin of the point-cloud export (include/lse_hip.h, "point-cloud export"): the four stages in float32, every operation in the
order the header states, plus the analytic scene the tests share -- a sphere seen by six pinhole cameras, with planted floaters -- and
a reader for the PLY ``write_ply_points`` writes."""
import functools

import numpy as np

F = np.float32
NO_KEY = np.iinfo(np.int64).max


def _f3(v):
    return np.asarray(v, dtype=F).reshape(3)


def unproject(origins, directions, depth, acc, lo, hi, min_acc):
    """(points [n, 3], keep [n] bool): p = o + d * depth (product rounded, then the sum) for every ray; keep: the validity rule."""
    o, d = np.asarray(origins, F).reshape(-1, 3), np.asarray(directions, F).reshape(-1, 3)
    t, a = np.asarray(depth, F).reshape(-1), np.asarray(acc, F).reshape(-1)
    lo, hi = _f3(lo), _f3(hi)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (d * t[:, None]).astype(F)
        p = (o + prod).astype(F)
        keep = (a >= F(min_acc)) & (t > 0) & (t < np.inf) & (lo <= p).all(-1) & (p <= hi).all(-1)
    return p, keep


def append(views, lo, hi, min_acc, cap=None):
    """The cloud ``lse_unproject_append`` builds over ``views`` = [(origins, directions, depth, acc, colors | None, normals | None)]:
    (points, colors | None, normals | None, total) with the rows at or beyond ``cap`` cut off and ``total`` the true count."""
    pts, cols, nrms = [], [], []
    for o, d, t, a, c, n in views:
        p, keep = unproject(o, d, t, a, lo, hi, min_acc)
        pts.append(p[keep])
        cols.append(None if c is None else np.asarray(c, F).reshape(-1, 3)[keep])
        nrms.append(None if n is None else np.asarray(n, F).reshape(-1, 3)[keep])
    cat = lambda parts: None if parts[0] is None else np.concatenate(parts)[:cap]
    total = sum(len(p) for p in pts)
    return np.concatenate(pts)[:cap], cat(cols), cat(nrms), total


def lattice(lo, hi, voxel):
    """The wrapper's voxel counts: max(1, ceil((hi_k - lo_k) / voxel)) in double."""
    return tuple(max(1, int(np.ceil((float(h) - float(l)) / float(voxel)))) for l, h in zip(lo, hi))


def voxel_keys(points, lo, voxel, res, count=None):
    p = np.asarray(points, F).reshape(-1, 3)
    n = p.shape[0]
    count = n if count is None else max(0, min(n, int(count)))
    lo = _f3(lo)
    keys = np.full(n, NO_KEY, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor(((p - lo).astype(F) / F(voxel)).astype(F))
        v = np.zeros((n, 3), dtype=np.int64)
        for k in range(3):
            top = f[:, k] >= F(res[k] - 1)
            mid = ~top & (f[:, k] > 0)                       # NaN: neither -> 0
            v[:, k] = np.where(top, res[k] - 1, np.where(mid, np.where(mid, f[:, k], 0).astype(np.int64), 0))
    keys[:count] = ((v[:, 0] * res[1] + v[:, 1]) * res[2] + v[:, 2])[:count]
    return keys


def _run_sum(values, idx):
    """s = the first element, then + the others one by one in run order, in float32 (accumulate is strictly sequential)."""
    return np.add.accumulate(values[idx], axis=0, dtype=F)[-1]


def voxel_merge(sorted_keys, order, points, colors=None, normals=None, with_normal_sums=False):
    """(keys, counts int32, points, colors | None, normals | None) per voxel, voxels in ascending key."""
    sk, order = np.asarray(sorted_keys, np.int64), np.asarray(order, np.int64)
    p = np.asarray(points, F).reshape(-1, 3)
    c = None if colors is None else np.asarray(colors, F).reshape(-1, 3)
    nr = None if normals is None else np.asarray(normals, F).reshape(-1, 3)
    n = sk.shape[0]
    head = (sk != NO_KEY) & np.concatenate([[True], sk[1:] != sk[:-1]]) if n else np.zeros(0, bool)
    starts = np.flatnonzero(head)
    valid_end = int((sk != NO_KEY).sum())
    ends = np.concatenate([starts[1:], [valid_end]]) if len(starts) else starts
    m = len(starts)
    keys, counts = sk[starts], (ends - starts).astype(np.int32)
    out_p = np.zeros((m, 3), F)
    out_c = None if c is None else np.zeros((m, 3), F)
    out_n = None if nr is None else np.zeros((m, 3), F)
    sums_n = None if nr is None else np.zeros((m, 3), F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for j, (a, b) in enumerate(zip(starts, ends)):
            idx = order[a:b]
            fc = F(b - a)
            out_p[j] = _run_sum(p, idx) / fc
            if c is not None:
                out_c[j] = _run_sum(c, idx) / fc
            if nr is not None:
                s = _run_sum(nr, idx)
                sq = (s * s).astype(F)
                length = np.sqrt(F(F(sq[0] + sq[1]) + sq[2]), dtype=F)
                div = length if length > F(1e-12) else F(1e-12)
                sums_n[j] = s
                out_n[j] = s / div
    if with_normal_sums:
        return keys, counts, out_p, out_c, out_n, sums_n
    return keys, counts, out_p, out_c, out_n


def merge(points, lo, voxel, res, colors=None, normals=None):
    """keys -> stable sort -> merge, as the export chains them."""
    keys = voxel_keys(points, lo, voxel, res)
    order = np.argsort(keys, kind="stable")
    return voxel_merge(keys[order], order, points, colors, normals)


def coords(keys, res):
    keys = np.asarray(keys, np.int64)
    return keys // (res[2] * res[1]), (keys // res[2]) % res[1], keys % res[2]


def support(keys, counts, res, count=None):
    """int32 [m]: per voxel the sum of the counts of the present voxels of its 3 x 3 x 3 block inside the lattice; 0 beyond ``count``."""
    keys, counts = np.asarray(keys, np.int64), np.asarray(counts, np.int64)
    m = keys.shape[0]
    count = m if count is None else max(0, min(m, int(count)))
    have = {int(k): int(c) for k, c in zip(keys[:count], counts[:count])}
    out = np.zeros(m, dtype=np.int64)
    x, y, z = coords(keys, res)
    for j in range(count):
        s = 0
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    xx, yy, zz = int(x[j]) + dx, int(y[j]) + dy, int(z[j]) + dz
                    if 0 <= xx < res[0] and 0 <= yy < res[1] and 0 <= zz < res[2]:
                        s += have.get((xx * res[1] + yy) * res[2] + zz, 0)
        out[j] = s
    return np.minimum(out, np.iinfo(np.int32).max).astype(np.int32)


def support_filter(keys, counts, res, min_support, count=None):
    """(keep [m] bool, support int32 [m])."""
    m = len(keys)
    count = m if count is None else max(0, min(m, int(count)))
    s = support(keys, counts, res, count)
    return (np.arange(m) < count) & (s.astype(np.int64) >= int(min_support)), s


def ulp_distance(a, b):
    """Largest distance in units in the last place between two float32 arrays of finite values."""
    def ordered(v):
        i = np.ascontiguousarray(v, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(ordered(a) - ordered(b)).max()) if np.size(a) else 0


# ---- the analytic scene ---------------------------------------------------------------------------------------------------------
CENTRE = (0.07, -0.05, 0.11)
RADIUS = 0.6
BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
VOXEL = 0.05
H, W, FOCAL, DISTANCE = 48, 64, 60.0, 2.0
N_PLANTED = 19


def camera_rays(axis, sign):
    """Origins and unit directions [H * W, 3] (float64) of a pinhole camera at ``sign * DISTANCE`` on ``axis`` looking at the origin,
    rays through the pixel centres."""
    pos = np.zeros(3)
    pos[axis] = sign * DISTANCE
    fwd = -pos / DISTANCE
    up = np.zeros(3)
    up[(axis + 1) % 3] = 1.0
    right = np.cross(fwd, up)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x, y = (xs + 0.5 - W / 2) / FOCAL, (ys + 0.5 - H / 2) / FOCAL
    d = x[..., None] * right - y[..., None] * up + fwd
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(pos, d.shape).reshape(-1, 3).copy(), d.reshape(-1, 3)


def sphere_depth(o, d):
    """Exact (float64) depth of the first hit of the sphere per ray, +inf on a miss, and the hit mask."""
    oc = o - np.asarray(CENTRE)
    a, b, c = (d * d).sum(-1), (oc * d).sum(-1), (oc * oc).sum(-1) - RADIUS * RADIUS
    disc = b * b - a * c
    hit = disc > 0
    t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / a, np.inf)
    return t, hit


def planted_points(seed=7):
    """N_PLANTED points uniform in (-0.95, 0.95)^3, at least 0.25 from the sphere's surface (rejection sampling, seeded)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < N_PLANTED:
        p = rng.uniform(-0.95, 0.95, 3)
        if abs(np.linalg.norm(p - np.asarray(CENTRE)) - RADIUS) >= 0.25:
            out.append(p)
    return np.stack(out)


@functools.lru_cache(maxsize=None)
def scene():
    """The scene as seven "views" of float32 rays, ``[(origins, directions, depth, acc)]``: the six cameras (acc = 1 on hits, 0 on
    misses) and one bundle of N_PLANTED rays that end at the planted points.  Read-only: shared between tests."""
    views = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            o, d = camera_rays(axis, sign)
            t, hit = sphere_depth(o, d)
            views.append((o.astype(F), d.astype(F), t.astype(F), hit.astype(F)))
    p = planted_points()
    d = np.tile(np.array([0.0, 0.0, 1.0]), (N_PLANTED, 1))
    views.append(((p - d).astype(F), d.astype(F), np.ones(N_PLANTED, F), np.ones(N_PLANTED, F)))
    for v in views:
        for a in v:
            a.setflags(write=False)
    return tuple(views)


@functools.lru_cache(maxsize=None)
def scene_cloud():
    """The twin's results on the scene, computed once: dict(points, n_sphere, res, keys, counts, merged, support)."""
    views = [(o, d, t, a, None, None) for o, d, t, a in scene()]
    pts, _, _, total = append(views, BOX[0], BOX[1], 0.5)
    res = lattice(BOX[0], BOX[1], VOXEL)
    keys, counts, merged, _, _ = merge(pts, BOX[0], VOXEL, res)
    raw_keys = voxel_keys(pts, BOX[0], VOXEL, res)
    n_sphere = total - N_PLANTED
    sphere_keys = set(raw_keys[:n_sphere].tolist())
    planted_only = np.array([k not in sphere_keys for k in keys.tolist()])
    out = dict(points=pts, total=total, n_sphere=n_sphere, res=res, keys=keys, counts=counts, merged=merged,
               support=support(keys, counts, res), planted_only=planted_only)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def read_ply_points(path):
    """(records, property names) of a vertex-only binary little-endian PLY with float / uchar properties."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    kinds = {"float": "<f4", "uchar": "u1"}
    n_vertex, props = None, []
    for ln in lines[2:]:
        w = ln.split()
        assert w[:2] != ["element", "face"], "a point cloud has no face element"
        if w[:2] == ["element", "vertex"]:
            n_vertex = int(w[2])
        elif w[:1] == ["property"]:
            props.append((w[2], kinds[w[1]]))
    dt = np.dtype(props)
    assert end + n_vertex * dt.itemsize == len(raw)
    return np.frombuffer(raw, dtype=dt, count=n_vertex, offset=end), [p[0] for p in props]
