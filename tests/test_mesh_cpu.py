"""Mesh export without a GPU: the five entry points are declared, bound and exported by both libraries and refuse bad arguments
before any launch; the numpy twin of the surface-nets definition (tests/mesh_ref.py) satisfies the mesh invariants on the analytic
fields; its float32 and float64 variants agree within a stated bound; ``write_ply`` round-trips; and ``world_gradient64`` (the
reference of ``lse_point_normals_world``) equals the closed-form transposed Jacobian of both position maps."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import normals_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lse_lattice_positions", "lse_surface_nets_workspace", "lse_surface_nets_count", "lse_surface_nets_emit",
       "lse_point_normals_world")
LO, HI = mr.UNIT_LO, mr.UNIT_HI
RES = 20


def _libs():
    from lsenerf_amd import _lib
    return [_lib.load(), _lib._load_dev()]


def test_symbols_are_declared_bound_and_exported_by_both_libraries():
    from lsenerf_amd import _lib, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lse_hip.h")).read(), flags=re.S)
    for lib in _libs():
        assert lib.lse_abi_version() == _lib.LSE_ABI_VERSION == 6
        for name in NEW:
            assert re.search(r"\bint " + name + r"\s*\(", hdr), name
            assert name in _lib.SIGNATURES and hasattr(lib, name), name
            n_args = len(re.search(r"\b" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S).group(1).split(","))
            assert n_args == len(_lib.SIGNATURES[name]), name
    assert re.search(r"#define LSE_MESH_SEGMENT\s+1024\b", hdr) and _lib.LSE_MESH_SEGMENT == 1024
    for fn in ("lattice_positions", "surface_nets", "point_normals_world"):
        assert callable(getattr(ops, fn))
    from lsenerf_amd import LSENeRFModel, mesh
    assert callable(mesh.extract_mesh) and callable(mesh.write_ply) and callable(LSENeRFModel.extract_mesh)


def test_workspace_size():
    from lsenerf_amd import ops
    for res in ((1, 1, 1), (5, 4, 3), (33, 32, 31), (160, 160, 160)):
        cells, points = res[0] * res[1] * res[2], (res[0] + 1) * (res[1] + 1) * (res[2] + 1)
        assert ops.lattice_points(res) == points
        assert ops.surface_nets_workspace_bytes(res) == 4 * cells + 8 * (-(-cells // 1024) + -(-points // 1024))
    assert ops.surface_nets_workspace_bytes(7) == ops.surface_nets_workspace_bytes((7, 7, 7))


def test_bad_arguments_are_refused_before_any_launch():
    """Every call below fails a host-side check (LSE_E_INVALID = -1, with a message): none reaches a launch, so the dummy
    addresses are never read."""
    F3 = ctypes.c_float * 3
    lo, hi, box6 = F3(-1, -1, -1), F3(1, 1, 1), (ctypes.c_float * 6)(-1, -1, -1, 1, 1, 1)
    ptr, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    big = 1 << 40
    nbytes = ctypes.c_int64(0)
    for lib in _libs():
        bad = []
        # resolutions: a count below 1, 2^31 points or more
        for res in ((0, 4, 4), (4, -1, 4), (4, 4, 0), (2000, 2000, 2000), (1290, 1290, 1290), (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1)):
            bad += [lib.lse_lattice_positions(lo, hi, *res, 0, 1, ptr, None),
                    lib.lse_surface_nets_workspace(*res, ctypes.byref(nbytes)),
                    lib.lse_surface_nets_count(ptr, *res, 0.0, ptr, big, ptr, None),
                    lib.lse_surface_nets_emit(ptr, *res, lo, hi, 0.0, ptr, big, 1, 1, ptr, ptr, None)]
        assert lib.lse_surface_nets_workspace(4, 4, 4, ctypes.byref(nbytes)) == 0 and nbytes.value == 4 * 64 + 8 * 2
        bad += [lib.lse_surface_nets_workspace(4, 4, 4, None),
                # lattice_positions: a window outside the 125 points, null box, null output
                lib.lse_lattice_positions(lo, hi, 4, 4, 4, -1, 1, ptr, None), lib.lse_lattice_positions(lo, hi, 4, 4, 4, 0, -1, ptr, None),
                lib.lse_lattice_positions(lo, hi, 4, 4, 4, 120, 6, ptr, None), lib.lse_lattice_positions(lo, hi, 4, 4, 4, 126, 0, ptr, None),
                lib.lse_lattice_positions(None, hi, 4, 4, 4, 0, 1, ptr, None), lib.lse_lattice_positions(lo, None, 4, 4, 4, 0, 1, ptr, None),
                lib.lse_lattice_positions(lo, hi, 4, 4, 4, 0, 1, None, None),
                # count: null pointers, a short or misaligned workspace, misaligned totals
                lib.lse_surface_nets_count(None, 4, 4, 4, 0.0, ptr, big, ptr, None),
                lib.lse_surface_nets_count(ptr, 4, 4, 4, 0.0, None, big, ptr, None),
                lib.lse_surface_nets_count(ptr, 4, 4, 4, 0.0, ptr, big, None, None),
                lib.lse_surface_nets_count(ptr, 4, 4, 4, 0.0, ptr, nbytes.value - 1, ptr, None),
                lib.lse_surface_nets_count(ptr, 4, 4, 4, 0.0, odd, big, ptr, None),
                lib.lse_surface_nets_count(ptr, 4, 4, 4, 0.0, ptr, big, odd, None),
                # emit: null pointers, a short or misaligned workspace, negative capacities, a capacity without a buffer
                lib.lse_surface_nets_emit(None, 4, 4, 4, lo, hi, 0.0, ptr, big, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, None, hi, 0.0, ptr, big, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, None, 0.0, ptr, big, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, hi, 0.0, None, big, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, hi, 0.0, ptr, nbytes.value - 1, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, hi, 0.0, odd, big, 1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, hi, 0.0, ptr, big, -1, 1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, hi, 0.0, ptr, big, 1, -1, ptr, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, hi, 0.0, ptr, big, 1, 1, None, ptr, None),
                lib.lse_surface_nets_emit(ptr, 4, 4, 4, lo, hi, 0.0, ptr, big, 1, 1, ptr, None, None),
                # point normals: a negative count, aabb normalisation without a box, null pointers
                lib.lse_point_normals_world(ptr, ptr, 1, None, -1, None, ptr, None),
                lib.lse_point_normals_world(ptr, ptr, 0, None, 8, None, ptr, None),
                lib.lse_point_normals_world(None, ptr, 1, None, 8, None, ptr, None),
                lib.lse_point_normals_world(ptr, None, 0, box6, 8, None, ptr, None),
                lib.lse_point_normals_world(ptr, ptr, 1, box6, 8, None, None, None)]
        assert bad == [-1] * len(bad), bad
        assert lib.lse_last_error().decode().startswith("lse_point_normals_world")
        # nothing to do is not an error and launches nothing
        assert lib.lse_lattice_positions(lo, hi, 4, 4, 4, 125, 0, None, None) == 0
        assert lib.lse_point_normals_world(None, None, 1, None, 0, None, None, None) == 0


def test_ops_refuse_mismatched_tensors_on_the_host():
    from lsenerf_amd import ops
    with pytest.raises(ValueError, match="resolution"):
        ops.lattice_points((4, 4))
    with pytest.raises(ValueError, match="sigma has"):
        ops.surface_nets_count(torch.zeros(10), (4, 4, 4), 0.0, torch.zeros(1, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="aabb6"):
        ops.point_normals_world(torch.zeros(2, 3), torch.zeros(2, 3), contraction=False)


# ---------------------------------------------------------------------------------------------------- the twin alone
@pytest.mark.parametrize("field,chi,volume", [("sphere", 2, 4.0 / 3.0 * math.pi * 0.6 ** 3), ("torus", 0, 2 * math.pi ** 2 * 0.55 * 0.25 ** 2),
                                               ("two_spheres", 4, 4.0 / 3.0 * math.pi * (0.33 ** 3 + 0.36 ** 3))])
def test_twin_invariants_of_the_closed_surfaces(field, chi, volume):
    v, t = mr.surface_nets(getattr(mr, field)(RES), RES, LO, HI, 0.0)
    assert v.dtype == np.float32 and t.dtype == np.int32 and t.shape[0] % 2 == 0 and v.shape[0] > 100
    assert mr.edge_imbalance(mr.directed_edges(t)) == 0              # every directed edge a -> b is matched by b -> a
    assert (mr.undirected_edge_uses(mr.quad_directed_edges(t)) == 2).all()
    assert mr.euler_characteristic(v.shape[0], t) == chi
    assert mr.unreferenced(v.shape[0], t) == 0
    vol = mr.signed_volume(v, t)
    print("MESH_TWIN", field, "signed volume / analytic:", vol / volume)
    assert 0.85 * volume < vol < volume                               # positive: outward normals; a 20^3 lattice shrinks the solid a little
    assert v.min() > -1 and v.max() < 1


def test_twin_on_noise_clipped_and_nonfinite_fields():
    v, t = mr.surface_nets(mr.noise(RES), RES, LO, HI, 0.0)
    assert mr.edge_imbalance(mr.directed_edges(t)) == 0
    assert set(np.unique(mr.undirected_edge_uses(mr.quad_directed_edges(t))).tolist()) <= {2, 4}       # never an odd number
    assert mr.unreferenced(v.shape[0], t) == 0
    v, t = mr.surface_nets(mr.clipped_sphere(RES), RES, LO, HI, 0.0)
    assert mr.edge_imbalance(mr.directed_edges(t)) > 0                # open where the surface leaves the box
    assert set(np.unique(mr.undirected_edge_uses(mr.quad_directed_edges(t))).tolist()) == {1, 2}
    v, t = mr.surface_nets(mr.open_noise(RES), RES, LO, HI, 0.0)
    assert mr.unreferenced(v.shape[0], t) > 0                         # active boundary cells keep a vertex nobody references
    v, t = mr.surface_nets(mr.seeded_nonfinite(RES), RES, LO, HI, 0.0)
    assert np.isfinite(v).all() and v.shape[0] > 680 and t.max() < v.shape[0]
    for const in (1.0, -1.0, np.nan, np.inf):
        v, t = mr.surface_nets(np.full(21 ** 3, const, dtype=np.float32), RES, LO, HI, 0.0)
        assert v.shape == (0, 3) and t.shape == (0, 3)
    v, t = mr.surface_nets(mr.open_noise((1, 1, 1)), (1, 1, 1), LO, HI, 0.0)
    assert v.shape == (1, 3) and t.shape == (0, 3)


def test_float32_twin_against_float64_twin():
    """Bound: 8 eps of the box's scale, eps = 2^-23, scale = max(|lo|, |hi|, hi - lo).  A sum of at most 12 crossings of magnitude
    <= n carries at most 12 half-ulps of its largest partial sum, 6 eps relative to n after the division by the count; t adds less
    than 2 eps of ONE lattice unit; the two divisions, the product and the final sum one half-ulp each.  Measured on these fields:
    at most 2.9e-7 = 1.2 eps x scale (printed below)."""
    eps = 2.0 ** -23
    cases = [(f, (33, 32, 31), LO, HI) for f in ("sphere", "torus", "two_spheres", "noise", "clipped_sphere", "seeded_nonfinite")]
    cases.append(("sphere", (7, 12, 5), (-2.0, 0.5, -0.25), (1.0, 3.5, 0.75)))
    for field, res, lo, hi in cases:
        s = getattr(mr, field)(res) if lo is LO else mr.sphere(res, (-0.4, 2.0, 0.2), 0.4, lo, hi)
        v32, t32 = mr.surface_nets(s, res, lo, hi, 0.0)
        v64, t64 = mr.surface_nets(s, res, lo, hi, 0.0, np.float64)
        assert v64.dtype == np.float64 and np.array_equal(t32, t64) and v32.shape[0] > 20
        scale = max(max(abs(a) for a in lo), max(abs(a) for a in hi), max(h - l for l, h in zip(lo, hi)))
        err = float(np.abs(v32.astype(np.float64) - v64).max())
        print("MESH_TWIN f32 vs f64", field, res, "max |dv|:", err, "=", err / (eps * scale), "eps x scale")
        assert err <= 8 * eps * scale, (field, err)


def test_twin_lattice_positions():
    res, lo, hi = (5, 4, 3), (-2.0, 0.5, -0.25), (1.0, 3.5, 0.75)
    p = mr.lattice_positions(res, lo, hi)
    assert p.dtype == np.float32 and p.shape == (6 * 5 * 4, 3)
    assert p[0].tolist() == [-2.0, 0.5, -0.25] and p[-1].tolist() == [1.0, 3.5, 0.75]
    assert p[1].tolist() == [-2.0, 0.5, float(np.float32(-0.25) + np.float32(1) / np.float32(3) * np.float32(1.0))]      # iz is fastest
    assert np.array_equal(mr.lattice_positions(res, lo, hi, 17, 50), p[17:67])
    assert np.abs(p - mr.lattice_positions(res, lo, hi, dtype=np.float64)).max() < 4 * 2.0 ** -23 * 3.5


# ---------------------------------------------------------------------------------------------------- PLY
@pytest.mark.parametrize("with_normals,with_colors", [(False, False), (True, False), (False, True), (True, True)])
def test_write_ply_round_trip(tmp_path, with_normals, with_colors):
    from lsenerf_amd.mesh import Mesh, write_ply
    v, t = mr.surface_nets(mr.sphere(8), 8, LO, HI, 0.0)
    rng = np.random.default_rng(0)
    n = rng.standard_normal(v.shape).astype(np.float32) if with_normals else None
    c = rng.random(v.shape).astype(np.float32) if with_colors else None
    if c is not None:
        c[0], c[1] = (0.0, 1.0, 0.5), (-0.2, 1.3, 0.25)         # clipped to [0, 1], rounded to the nearest of 255 steps
    as_t = lambda a: None if a is None else torch.from_numpy(a)
    path = str(tmp_path / "m.ply")
    write_ply(path, Mesh(as_t(v), as_t(t), as_t(n), as_t(c)))
    verts, faces, names = mr.read_ply(path)
    assert names == ["x", "y", "z"] + (["nx", "ny", "nz"] if with_normals else []) + (["red", "green", "blue"] if with_colors else [])
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), v) and np.array_equal(faces, t)
    if with_normals:
        assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), n)
    if with_colors:
        got = np.stack([verts["red"], verts["green"], verts["blue"]], 1)
        assert got.dtype == np.uint8 and np.array_equal(got, np.rint(np.clip(c, 0, 1) * 255).astype(np.uint8))
        assert got[0].tolist() == [0, 255, 128] and got[1].tolist() == [0, 255, 64]
    # an empty mesh is a valid file
    write_ply(path, Mesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)))
    verts, faces, _ = mr.read_ply(path)
    assert verts.shape == (0,) and faces.shape == (0, 3)


# ---------------------------------------------------------------------------------------------------- world normals
def _closed_form_world_gradient(p, g, contraction, aabb6):
    """J^T g in float64 from the formulas of csrc/positions.h, selector-masked."""
    p, g = np.asarray(p, dtype=np.float64), np.asarray(g, dtype=np.float64)
    if contraction:
        mag = np.abs(p).max(1)
        am = np.abs(p).argmax(1)
        m = np.maximum(mag, 1.0)
        s = (2.0 - 1.0 / m) / m
        ds = -2.0 / m ** 2 + 2.0 / m ** 3
        out = 0.25 * s[:, None] * g
        rows = np.arange(p.shape[0])
        out[rows, am] += 0.25 * (g * p).sum(1) * ds * np.sign(p[rows, am])
        out = np.where((mag < 1.0)[:, None], 0.25 * g, out)
        c = np.where((mag < 1.0)[:, None], p, ((2.0 - 1.0 / m) / m)[:, None] * p)
        x = (c + 2.0) / 4.0
    else:
        lo, hi = np.asarray(aabb6[:3], dtype=np.float64), np.asarray(aabb6[3:], dtype=np.float64)
        out = g / (hi - lo)
        x = (p - lo) / (hi - lo)
    return out * ((x > 0) & (x < 1)).all(1)[:, None]


@pytest.mark.parametrize("contraction", [True, False])
def test_world_gradient64_is_the_closed_form_jacobian(contraction):
    rng = np.random.default_rng(3)
    p = (rng.random((400, 3)) - 0.5) * (6.0 if contraction else 2.6)
    g = rng.standard_normal((400, 3))
    aabb6 = None if contraction else [-1.0, -1.2, -0.8, 1.0, 0.9, 1.1]
    ref = nr.world_gradient64(p, g, contraction, aabb6)
    mine = _closed_form_world_gradient(p, g, contraction, aabb6)
    assert np.abs(ref - mine).max() < 1e-12 * max(1.0, np.abs(ref).max())
    inside = (np.abs(ref).sum(1) > 0)
    assert inside.any() and (contraction or (~inside).any())
    n = nr.sample_normals(ref)
    assert np.allclose(np.linalg.norm(n[inside], axis=1), 1.0) and (n[~inside] == 0).all()
