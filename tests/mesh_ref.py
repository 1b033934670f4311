"""numpy twin of the surface-nets definition in include/lse_hip.h ("mesh export"), the analytic test fields and the mesh invariants
(tests/test_mesh_cpu.py and the GPU tests of csrc/mesh.hip).  Not a test file.

``dtype=np.float32`` restates the kernels operation by operation (every numpy operation on float32 arrays rounds once, as the
kernels built without FMA contraction do); ``dtype=np.float64`` is the same definition in double, on the same float32 inputs."""
from __future__ import annotations

import numpy as np


def _res3(res):
    return (int(res),) * 3 if isinstance(res, int) else tuple(int(v) for v in res)


def lattice_positions(res, lo, hi, first: int = 0, n=None, dtype=np.float32) -> np.ndarray:
    """[n, 3] positions of the points first .. first + n: lo_k + (i_k / n_k) * (hi_k - lo_k)."""
    nx, ny, nz = _res3(res)
    points = (nx + 1) * (ny + 1) * (nz + 1)
    n = points - first if n is None else n
    p = np.arange(first, first + n, dtype=np.int64)
    i = np.stack([p // ((ny + 1) * (nz + 1)), (p // (nz + 1)) % (ny + 1), p % (nz + 1)], axis=1)
    lo, hi = np.asarray(lo, dtype=np.float32).astype(dtype), np.asarray(hi, dtype=np.float32).astype(dtype)
    return lo + (i.astype(dtype) / np.asarray([nx, ny, nz]).astype(dtype)) * (hi - lo)


def surface_nets(sigma, res, lo, hi, level, dtype=np.float32):
    """(vertices [V, 3] ``dtype``, triangles [2 Q, 3] int32) of the lattice ``sigma`` (one value per point, iz fastest)."""
    nx, ny, nz = n3 = _res3(res)
    S = np.asarray(sigma, dtype=np.float32).reshape(nx + 1, ny + 1, nz + 1).astype(dtype)
    lv = dtype(np.float32(level))
    with np.errstate(invalid="ignore"):
        inside = S > lv                                   # NaN is outside
    # ---- vertices: the active cells in ascending cell index
    cnt = np.zeros((nx, ny, nz), dtype=np.int32)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cnt += inside[dx:dx + nx, dy:dy + ny, dz:dz + nz]
    active = (cnt != 0) & (cnt != 8)
    cells = np.flatnonzero(active.ravel())
    cc = np.stack(np.unravel_index(cells, (nx, ny, nz)), axis=1).astype(np.int64)
    acc = np.zeros((cells.shape[0], 3), dtype=dtype)
    count = np.zeros(cells.shape[0], dtype=np.int32)
    eye = np.eye(3, dtype=np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for ob in (0, 1):
                for oc in (0, 1):
                    P = cc + ob * eye[b] + oc * eye[c]
                    Q = P + eye[a]
                    sP, sQ = S[P[:, 0], P[:, 1], P[:, 2]], S[Q[:, 0], Q[:, 1], Q[:, 2]]
                    cross = (sP > lv) != (sQ > lv)
                    t = (lv - sP) / (sQ - sP)
                    t = np.where(np.isnan(t), dtype(0.5), t)
                    t = np.minimum(np.maximum(t, dtype(0)), dtype(1))
                    pt = P.astype(dtype)
                    pt[:, a] = pt[:, a] + t
                    acc = acc + np.where(cross[:, None], pt, dtype(0))      # (x + 0 == x: the sum of the crossings, in order)
                    count += cross
        u = acc / count.astype(dtype)[:, None]
    lo, hi = np.asarray(lo, dtype=np.float32).astype(dtype), np.asarray(hi, dtype=np.float32).astype(dtype)
    vertices = lo + (u / np.asarray(n3).astype(dtype)) * (hi - lo)
    # ---- faces: the sign-changing lattice edges (p, a), interior in the other two axes, in ascending (p, a)
    mark = np.zeros((nx + 1, ny + 1, nz + 1, 3), dtype=bool)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        sl_p, sl_q = [None] * 3, [None] * 3
        sl_p[a], sl_q[a] = slice(0, n3[a]), slice(1, n3[a] + 1)
        sl_p[b] = sl_q[b] = slice(1, n3[b])
        sl_p[c] = sl_q[c] = slice(1, n3[c])
        mark[tuple(sl_p) + (a,)] = inside[tuple(sl_p)] != inside[tuple(sl_q)]
    idx = np.flatnonzero(mark.ravel())
    p, a = idx // 3, idx % 3
    i = np.stack(np.unravel_index(p, (nx + 1, ny + 1, nz + 1)), axis=1).astype(np.int64)
    eb, ec = eye[(a + 1) % 3], eye[(a + 2) % 3]
    vid = np.full(nx * ny * nz, -1, dtype=np.int64)
    vid[cells] = np.arange(cells.shape[0])
    cid = lambda q: vid[(q[:, 0] * ny + q[:, 1]) * nz + q[:, 2]]
    w = np.stack([cid(i - eb - ec), cid(i - ec), cid(i), cid(i - eb)], axis=1)
    w = np.where(inside.ravel()[p][:, None], w, w[:, ::-1])
    assert (w >= 0).all()                                  # all four cells are active by construction
    triangles = np.stack([w[:, 0], w[:, 1], w[:, 2], w[:, 0], w[:, 2], w[:, 3]], axis=1).reshape(-1, 3).astype(np.int32)
    return vertices, triangles


# ---------------------------------------------------------------------------------------------------- fields
UNIT_LO, UNIT_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)


def _grid(res, lo, hi):
    return lattice_positions(res, lo, hi, dtype=np.float64)


def sphere(res, centre=(0.07, -0.05, 0.11), radius=0.6, lo=UNIT_LO, hi=UNIT_HI) -> np.ndarray:
    """radius - |x - centre|: positive inside.  Level 0."""
    x = _grid(res, lo, hi)
    return (radius - np.linalg.norm(x - np.asarray(centre), axis=1)).astype(np.float32)


def torus(res, R=0.55, r=0.25, centre=(0.03, -0.04, 0.05), lo=UNIT_LO, hi=UNIT_HI) -> np.ndarray:
    x = _grid(res, lo, hi) - np.asarray(centre)
    return (r - np.sqrt((np.sqrt(x[:, 0] ** 2 + x[:, 1] ** 2) - R) ** 2 + x[:, 2] ** 2)).astype(np.float32)


def two_spheres(res, lo=UNIT_LO, hi=UNIT_HI) -> np.ndarray:
    return np.maximum(sphere(res, (-0.45, -0.4, -0.35), 0.33, lo, hi), sphere(res, (0.42, 0.4, 0.38), 0.36, lo, hi))


def clipped_sphere(res, lo=UNIT_LO, hi=UNIT_HI) -> np.ndarray:
    return sphere(res, (0.6, 0.1, -0.2), 0.7, lo, hi)


def noise(res, seed=0) -> np.ndarray:
    """Gaussian noise with every point of the lattice's surface set outside (-1).  Level 0."""
    nx, ny, nz = _res3(res)
    s = np.random.default_rng(seed).standard_normal((nx + 1, ny + 1, nz + 1)).astype(np.float32)
    s[0], s[-1], s[:, 0], s[:, -1], s[:, :, 0], s[:, :, -1] = -1, -1, -1, -1, -1, -1
    return s.ravel()


def open_noise(res, seed=2) -> np.ndarray:
    """Gaussian noise up to the lattice's surface: active boundary cells, open edges, a vertex in a single-cell lattice.  Level 0."""
    nx, ny, nz = _res3(res)
    return np.random.default_rng(seed).standard_normal((nx + 1) * (ny + 1) * (nz + 1)).astype(np.float32)


def seeded_nonfinite(res, seed=1) -> np.ndarray:
    """The off-centre sphere with NaN, +inf and -inf entries scattered over it (about 3 % of the points each)."""
    s = sphere(res).copy()
    r = np.random.default_rng(seed).random(s.shape[0])
    s[r < 0.03] = np.nan
    s[(r >= 0.03) & (r < 0.06)] = np.inf
    s[(r >= 0.06) & (r < 0.09)] = -np.inf
    return s


# ---------------------------------------------------------------------------------------------------- invariants
def directed_edges(triangles: np.ndarray) -> np.ndarray:
    t = np.asarray(triangles, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], axis=0)


def quad_directed_edges(triangles: np.ndarray) -> np.ndarray:
    """The four boundary edges of every quad (two consecutive triangles (w0, w1, w2), (w0, w2, w3)): without the diagonal."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 6)
    w = t[:, [0, 1, 2, 5]]
    return np.concatenate([w[:, [0, 1]], w[:, [1, 2]], w[:, [2, 3]], w[:, [3, 0]]], axis=0)


def edge_imbalance(edges: np.ndarray) -> int:
    """Number of directed edges a -> b whose multiplicity differs from that of b -> a (0 on a closed oriented surface)."""
    if edges.shape[0] == 0:
        return 0
    m = int(edges.max()) + 1
    keys = np.concatenate([edges[:, 0] * m + edges[:, 1], edges[:, 1] * m + edges[:, 0]])
    sign = np.concatenate([np.ones(edges.shape[0], dtype=np.int64), -np.ones(edges.shape[0], dtype=np.int64)])
    _, inv = np.unique(keys, return_inverse=True)
    return int((np.bincount(inv.ravel(), weights=sign) != 0).sum())


def undirected_edge_uses(edges: np.ndarray) -> np.ndarray:
    e = np.sort(edges, axis=1)
    return np.unique(e[:, 0] * (int(e.max()) + 1) + e[:, 1], return_counts=True)[1]


def euler_characteristic(n_vertices: int, triangles: np.ndarray) -> int:
    e = np.sort(directed_edges(triangles), axis=1)
    n_edges = np.unique(e[:, 0] * (n_vertices + 1) + e[:, 1]).shape[0]
    return n_vertices - n_edges + np.asarray(triangles).shape[0]


def signed_volume(vertices: np.ndarray, triangles: np.ndarray) -> float:
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def unreferenced(n_vertices: int, triangles: np.ndarray) -> int:
    return n_vertices - np.unique(np.asarray(triangles)).shape[0]


# ---------------------------------------------------------------------------------------------------- PLY
def read_ply(path):
    """A reader for what ``write_ply`` promises: binary little-endian, float / uchar vertex properties, ``uchar int`` face lists."""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    lines = raw[:end].decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    kinds = {"float": "<f4", "uchar": "u1", "int": "<i4"}
    n_vertex = n_face = None
    props, section = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[:2] == ["element", "vertex"]:
            n_vertex, section = int(w[2]), "vertex"
        elif w[:2] == ["element", "face"]:
            n_face, section = int(w[2]), "face"
        elif w[:1] == ["property"] and section == "vertex":
            props.append((w[2], kinds[w[1]]))
        elif w[:1] == ["property"]:
            assert w == ["property", "list", "uchar", "int", "vertex_indices"]
    vdt = np.dtype(props)
    verts = np.frombuffer(raw, dtype=vdt, count=n_vertex, offset=end)
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    faces = np.frombuffer(raw, dtype=fdt, count=n_face, offset=end + n_vertex * vdt.itemsize)
    assert end + n_vertex * vdt.itemsize + n_face * fdt.itemsize == len(raw) and (faces["n"] == 3).all()
    return verts, faces["v"], [p[0] for p in props]
