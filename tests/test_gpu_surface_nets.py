"""csrc/mesh.hip through ``ops``: ``surface_nets`` against the float32 numpy twin (tests/mesh_ref.py) -- totals equal, triangles equal
and in order, vertices BIT-equal (every operation of the definition is a single correctly rounded float32 operation in both, so no
bound is needed) -- on lattices from one cell to 160^3 (more segments than scan threads), the mesh invariants on the device output,
capacities below the totals, ``lattice_positions`` windows and ``point_normals_world`` against the float64 Jacobian."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import normals_ref as nr
from tests.util import TOL_FWD, nmax_err

pytestmark = pytest.mark.gpu

LO, HI = mr.UNIT_LO, mr.UNIT_HI
FIELDS = {"sphere": mr.sphere, "torus": mr.torus, "two_spheres": mr.two_spheres, "noise": mr.noise, "clipped": mr.clipped_sphere,
          "open_noise": mr.open_noise, "nonfinite": mr.seeded_nonfinite}
SMALL = [(1, 1, 1), (5, 4, 3), (33, 32, 31)]       # one cell; a few; partial waves and several segments
CLOSED = {"sphere": 2, "torus": 0, "two_spheres": 4}      # Euler characteristic


@functools.lru_cache(maxsize=None)
def _sigma(field, res):
    s = FIELDS[field](res)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _twin(field, res):
    return mr.surface_nets(_sigma(field, res), res, LO, HI, 0.0)


@functools.lru_cache(maxsize=None)
def _device(field, res):
    from lsenerf_amd import ops
    v, t, totals = ops.surface_nets(torch.from_numpy(_sigma(field, res).copy()).cuda(), res, LO, HI, 0.0)
    return v.cpu().numpy(), t.cpu().numpy(), totals.cpu().numpy()


def _assert_equal_to_twin(dev, twin, what):
    (v, t, totals), (rv, rt) = dev, twin
    assert totals.tolist() == [rv.shape[0], rt.shape[0] // 2], what
    assert t.dtype == np.int32 and t.shape == rt.shape and np.array_equal(t, rt), what
    assert v.dtype == np.float32 and v.shape == rv.shape, what
    differ = int((v.view(np.int32) != rv.view(np.int32)).sum())
    print("SURFACE_NETS", what, "vertices", v.shape[0], "quads", t.shape[0] // 2, "coordinates that differ in bits:", differ)
    assert differ == 0, what


@pytest.mark.parametrize("res", SMALL, ids=lambda r: "x".join(map(str, r)))
@pytest.mark.parametrize("field", sorted(FIELDS))
def test_mesh_equals_the_float32_twin(field, res):
    _assert_equal_to_twin(_device(field, res), _twin(field, res), f"{field} {res}")
    if field == "open_noise":
        assert _twin(field, res)[0].shape[0] > 0          # even the single cell has its vertex (and no quad)
    if field == "nonfinite" and res != (1, 1, 1):
        assert np.isfinite(_device(field, res)[0]).all()


@pytest.mark.parametrize("field", ["torus", "two_spheres"])
def test_160_cubed_more_segments_than_scan_threads(field):
    from lsenerf_amd import _lib
    res = (160, 160, 160)
    assert 160 ** 3 // _lib.LSE_MESH_SEGMENT > 256 * 8
    dev = _device(field, res)
    _assert_equal_to_twin(dev, _twin(field, res), f"{field} {res}")
    v, t, _ = dev
    assert mr.edge_imbalance(mr.directed_edges(t)) == 0 and mr.euler_characteristic(v.shape[0], t) == CLOSED[field]


@pytest.mark.parametrize("field", sorted(CLOSED))
def test_invariants_of_the_closed_surfaces_on_the_device_output(field):
    v, t, _ = _device(field, (33, 32, 31))
    assert mr.edge_imbalance(mr.directed_edges(t)) == 0                # every directed edge a -> b is matched by b -> a
    assert mr.euler_characteristic(v.shape[0], t) == CLOSED[field]
    assert mr.unreferenced(v.shape[0], t) == 0
    vol = mr.signed_volume(v, t)
    print("SURFACE_NETS", field, "signed volume", vol)
    assert vol > 0                                                      # normals point from high to low density: outwards


def test_the_clipped_sphere_is_open_where_it_leaves_the_box():
    v, t, _ = _device("clipped", (33, 32, 31))
    assert mr.edge_imbalance(mr.directed_edges(t)) > 0
    assert (mr.undirected_edge_uses(mr.quad_directed_edges(t)) <= 2).all()


@pytest.mark.parametrize("res", SMALL, ids=lambda r: "x".join(map(str, r)))
def test_all_inside_and_all_outside_give_nothing(res):
    from lsenerf_amd import ops
    n = ops.lattice_points(res)
    for value, level in ((1.0, 0.0), (-1.0, 0.0), (0.5, 0.5), (float("nan"), 0.0), (float("inf"), 0.0)):      # sigma == level is outside
        v, t, totals = ops.surface_nets(torch.full((n,), value, device="cuda"), res, LO, HI, level)
        assert totals.tolist() == [0, 0] and v.shape == (0, 3) and t.shape == (0, 3), (value, level)


def test_anisotropic_box_and_resolution_and_a_nonzero_level():
    from lsenerf_amd import ops
    res, lo, hi = (7, 12, 5), (-2.0, 0.5, -0.25), (1.0, 3.5, 0.75)
    s = mr.sphere(res, centre=(-0.4, 2.0, 0.2), radius=0.4, lo=lo, hi=hi) + np.float32(0.3)
    twin = mr.surface_nets(s, res, lo, hi, 0.3)
    assert twin[0].shape[0] > 20 and mr.euler_characteristic(twin[0].shape[0], twin[1]) == 2
    v, t, totals = ops.surface_nets(torch.from_numpy(s).cuda().reshape(8, 13, 6), res, lo, hi, 0.3)
    _assert_equal_to_twin((v.cpu().numpy(), t.cpu().numpy(), totals.cpu().numpy()), twin, "anisotropic")


def test_capacities_below_the_totals_and_a_second_run():
    from lsenerf_amd import ops
    res = (33, 32, 31)
    rv, rt = _twin("noise", res)
    n_v, n_q = rv.shape[0], rt.shape[0] // 2
    sigma = torch.from_numpy(_sigma("noise", res).copy()).cuda()
    ws = torch.empty(ops.surface_nets_workspace_bytes(res), dtype=torch.uint8, device="cuda")
    totals = torch.zeros(2, dtype=torch.int64, device="cuda")
    ops.surface_nets_count(sigma, res, 0.0, ws, totals)
    cap_v, cap_q = n_v // 2 + 3, n_q // 3 + 1
    slack = 64                                                         # rows behind the capacities: nothing may land there
    v = torch.full((cap_v + slack, 3), -7.0, device="cuda")
    t = torch.full((2 * (cap_q + slack), 3), -7, dtype=torch.int32, device="cuda")
    ops.surface_nets_emit(sigma, res, LO, HI, 0.0, ws, v[:cap_v], t[:2 * cap_q])
    assert totals.tolist() == [n_v, n_q]                               # still the true counts
    assert np.array_equal(v[:cap_v].cpu().numpy().view(np.int32), rv[:cap_v].view(np.int32))
    assert np.array_equal(t[:2 * cap_q].cpu().numpy(), rt[:2 * cap_q])
    assert bool((v[cap_v:] == -7.0).all()) and bool((t[2 * cap_q:] == -7).all())
    # fixed capacities above the totals through the public op: the rows beyond the totals are the caller's to ignore
    v2, t2, totals2 = ops.surface_nets(sigma, res, LO, HI, 0.0, caps=(n_v + 10, n_q + 10))
    assert totals2.tolist() == [n_v, n_q] and v2.shape == (n_v + 10, 3) and t2.shape == (2 * (n_q + 10), 3)
    assert np.array_equal(v2[:n_v].cpu().numpy().view(np.int32), rv.view(np.int32)) and np.array_equal(t2[:2 * n_q].cpu().numpy(), rt)
    # a second run gives the same bytes
    v3, t3, _ = ops.surface_nets(sigma, res, LO, HI, 0.0)
    assert torch.equal(v3, v2[:n_v]) and torch.equal(t3, t2[:2 * n_q])


def test_lattice_positions_windows_that_straddle_rows():
    from lsenerf_amd import ops
    res, lo, hi = (5, 4, 3), (-2.0, 0.5, -0.25), (1.0, 3.5, 0.75)
    n = ops.lattice_points(res)
    assert n == 6 * 5 * 4
    ref = mr.lattice_positions(res, lo, hi)
    for first, cnt in ((0, n), (0, 1), (3, 6), (17, 50), (n - 1, 1), (n, 0), (7, 0)):
        got = ops.lattice_positions(res, lo, hi, first, cnt).cpu().numpy()
        assert got.shape == (cnt, 3) and np.array_equal(got.view(np.int32), ref[first:first + cnt].view(np.int32)), (first, cnt)
    res = (33, 32, 31)
    got = ops.lattice_positions(res, LO, HI, 1000, 30000).cpu().numpy()
    assert np.array_equal(got.view(np.int32), mr.lattice_positions(res, LO, HI, 1000, 30000).view(np.int32))
    out = torch.full((12, 3), -7.0, device="cuda")
    ops.lattice_positions((5, 4, 3), lo, hi, 4, 8, out=out[2:10])
    assert bool((out[:2] == -7.0).all()) and bool((out[10:] == -7.0).all())
    assert np.array_equal(out[2:10].cpu().numpy().view(np.int32), ref[4:12].view(np.int32))


@pytest.mark.parametrize("contraction", [True, False])
def test_point_normals_world_against_the_float64_jacobian(contraction):
    """The tolerance tests/test_gpu_eval_normals.py uses for world normals: 5 TOL_FWD of the largest component (1)."""
    from lsenerf_amd import ops
    g = torch.Generator().manual_seed(12)
    n = 777                                                            # several blocks, the last one partial
    pos = (torch.rand(n, 3, generator=g) - 0.5) * (6.0 if contraction else 2.6)      # inside and outside the unit box / the aabb
    d = torch.randn(n, 3, generator=g)
    d[::50] = 0.0                                                      # zero gradients give zero normals
    aabb6 = None if contraction else [-1.0, -1.2, -0.8, 1.0, 0.9, 1.1]
    got = ops.point_normals_world(d.cuda(), pos.cuda(), contraction, aabb6).cpu()
    ref = nr.sample_normals(nr.world_gradient64(pos.numpy(), d.numpy(), contraction, aabb6))
    zero = np.linalg.norm(ref, axis=1) == 0
    assert zero[::50].all() and (contraction or zero.sum() > 16 + 20)      # outside the aabb: selector-masked
    err = nmax_err(got, torch.from_numpy(ref))
    print("POINT_NORMALS", "contraction" if contraction else "aabb", "vs float64:", err, "zero rows", int(zero.sum()))
    assert err < 5 * TOL_FWD, err
    assert bool((got[torch.from_numpy(zero)] == 0).all())
    assert float((got[torch.from_numpy(~zero)].norm(dim=-1) - 1).abs().max()) < 1e-5
    # a device-side count: rows at or beyond it are left alone
    out = torch.full((n, 3), -7.0, device="cuda")
    ops.point_normals_world(d.cuda(), pos.cuda(), contraction, aabb6, out=out, n_dev=torch.tensor([300], device="cuda"))
    assert torch.equal(out[:300].cpu(), got[:300]) and bool((out[300:] == -7.0).all())
