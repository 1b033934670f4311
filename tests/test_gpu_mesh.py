"""``LSENeRFModel.extract_mesh`` on the small model of tests/test_gpu_eval_normals.py, with and without contraction, at resolution
24: every stage of the export against the entry point it is built from, called directly -- all of it bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr

pytestmark = pytest.mark.gpu

RES = 24
LEVEL = 1.0          # trunc_exp of a zero logit: about half of the random field lies inside
BOUNDS = ((-0.9, -0.8, -0.7), (0.8, 0.9, 0.75))


@functools.lru_cache(maxsize=None)
def _model(contraction=True):
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(5)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, log2_hashmap_size=14, disable_scene_contraction=not contraction)
    m = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 8).cuda()
    with torch.no_grad():     # a table large enough for the logit to vary over a cell
        m.field.mlp_base_grid.params.uniform_(-0.5, 0.5, generator=torch.Generator(device="cuda").manual_seed(9))
    return m.train()


@functools.lru_cache(maxsize=None)
def _mesh(contraction=True, bounds=None):
    return _model(contraction).extract_mesh(resolution=RES, level=LEVEL, bounds=bounds, normals=True, colors=True)


def _box(model, bounds):
    aabb = model.field.aabb.cpu().tolist() if bounds is None else bounds
    return [float(v) for v in aabb[0]], [float(v) for v in aabb[1]]


@pytest.mark.parametrize("contraction", [True, False])
@pytest.mark.parametrize("bounds", [None, BOUNDS], ids=["aabb", "box"])
def test_every_stage_equals_its_entry_point_called_directly(contraction, bounds):
    from lsenerf_amd import mesh as lm, ops
    from lsenerf_amd.rays import Frustums, RaySamples
    from lsenerf_amd.field import FieldHeadNames
    model = _model(contraction)
    fld = model.field
    got = _mesh(contraction, bounds)
    lo, hi = _box(model, bounds)
    res = (RES, RES, RES)
    model.eval()
    try:
        with torch.no_grad():
            # the lattice density: the field's density route on all positions at once, whatever the chunk size
            pos = ops.lattice_positions(res, lo, hi)
            assert pos.shape == (25 ** 3, 3)
            want_sigma = fld.density_fn(pos).reshape(-1)
            for chunk in (1000, 4096, 1 << 22):
                assert torch.equal(lm.density_lattice(fld, res, lo, hi, chunk), want_sigma), chunk
            # the mesh: surface nets of that density
            v, t, totals = ops.surface_nets(want_sigma, res, lo, hi, LEVEL)
            assert v.shape[0] > 500 and t.shape[0] > 1000 and totals.tolist() == [v.shape[0], t.shape[0] // 2]
            assert torch.equal(got.vertices, v) and torch.equal(got.triangles, t)
            rv, rt = mr.surface_nets(want_sigma.cpu().numpy(), res, lo, hi, LEVEL)
            assert np.array_equal(v.cpu().numpy().view(np.int32), rv.view(np.int32)) and np.array_equal(t.cpu().numpy(), rt)
            # the normals: normals_packed + point_normals_world; unit vectors or zero
            x01, _, y = fld._encode_packed(v, None, None, None, None, None)
            ctr = fld._contraction == "inf"
            assert ctr == contraction
            n = ops.point_normals_world(fld.normals_packed(x01, y), v, ctr, None if ctr else fld._aabb_list())
            assert torch.equal(got.normals, n) and torch.equal(lm.vertex_normals(fld, v, chunk=333), n)
            length = n.norm(dim=-1)
            assert bool(((length - 1).abs() < 1e-5).logical_or(length == 0).all()) and float((length > 0).float().mean()) > 0.9
            # the colours: the eager field on stock samples at the vertices seen along -normal, then the eval mapping of a ray
            dirs = torch.where((n == 0).all(-1, keepdim=True), n.new_tensor([0.0, 0.0, 1.0]), -n)
            zeros = torch.zeros(v.shape[0], 1, device="cuda")
            rs = RaySamples(frustums=Frustums(origins=v, directions=dirs, starts=zeros, ends=zeros),
                            camera_indices=torch.zeros(v.shape[0], 1, dtype=torch.long, device="cuda"))
            rgb = fld(rs)[FieldHeadNames.RGB]
            want = model.route_outputs({"rgb": torch.clamp(torch.nan_to_num(rgb), 0.0, 1.0)}, None)["rgb"]
            assert tuple(want.shape) == (v.shape[0], 3) and torch.equal(got.colors, want)
            assert torch.equal(lm.vertex_colors(model, v, n, chunk=333), want)
            assert float(want.min()) >= 0.0 and float(want.max()) <= 1.0 and float(want.std()) > 1e-3
    finally:
        model.train()


def test_two_calls_are_bit_identical_and_options_drop_outputs():
    model = _model(True)
    a, b = _mesh(True, None), model.extract_mesh(resolution=RES, level=LEVEL, colors=True, chunk=5000)
    for k in ("vertices", "triangles", "normals", "colors"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    c = model.extract_mesh(resolution=(RES, RES, RES), level=LEVEL, normals=False)
    assert c.normals is None and c.colors is None and torch.equal(c.vertices, a.vertices) and torch.equal(c.triangles, a.triangles)
    d = model.extract_mesh(resolution=RES, level=LEVEL, normals=False, colors=True)
    assert d.normals is None and torch.equal(d.colors, a.colors)
    e = model.extract_mesh(resolution=(12, 24, 6), level=LEVEL)
    assert e.vertices.shape[0] > 50 and e.colors is None and e.normals.shape == e.vertices.shape
    assert int(e.triangles.max()) < e.vertices.shape[0] and int(e.triangles.min()) >= 0


def test_mode_and_parameters_are_untouched():
    model = _model(True)
    model.train()
    model.field.mlp_head.eval()                          # a mixed state: every module gets its own mode back
    try:
        modes = [m.training for m in model.modules()]
        before = {k: v.detach().clone() for k, v in model.state_dict().items()}
        grads = [p.requires_grad for p in model.parameters()]
        with torch.enable_grad():
            mesh = model.extract_mesh(resolution=RES, level=LEVEL, colors=True)
        assert not mesh.vertices.requires_grad and not mesh.normals.requires_grad and not mesh.colors.requires_grad
        assert [m.training for m in model.modules()] == modes and model.training
        assert [p.requires_grad for p in model.parameters()] == grads and all(p.grad is None for p in model.parameters())
        after = model.state_dict()
        assert set(after) == set(before)
        for k, v in before.items():
            assert torch.equal(after[k], v), k
        with pytest.raises(ValueError, match="empty box"):
            model.extract_mesh(resolution=4, bounds=((0.0, 0.0, 0.0), (1.0, 0.0, 1.0)))
        assert [m.training for m in model.modules()] == modes
    finally:
        model.train()


def test_ply_round_trip_of_the_result(tmp_path):
    from lsenerf_amd.mesh import write_ply
    mesh = _mesh(False, BOUNDS)
    path = str(tmp_path / "mesh.ply")
    write_ply(path, mesh)
    verts, faces, names = mr.read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert np.array_equal(np.stack([verts["x"], verts["y"], verts["z"]], 1), mesh.vertices.cpu().numpy())
    assert np.array_equal(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), mesh.normals.cpu().numpy())
    assert np.array_equal(faces, mesh.triangles.cpu().numpy())
    want = np.rint(np.clip(mesh.colors.cpu().numpy(), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), want)


def test_small_grid_base_mlp_is_refused_for_normals():
    from lsenerf_amd import _lib, mesh as lm
    from lsenerf_amd.field import LSEField
    fld = LSEField(torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 4, num_levels=4, log2_hashmap_size=10).cuda().eval()
    with pytest.raises(_lib.LseHipError, match="small-grid base MLP"):
        lm.vertex_normals(fld, torch.zeros(4, 3, device="cuda"))
    sigma = lm.density_lattice(fld, (4, 4, 4), [-1.0] * 3, [1.0] * 3)      # the density lattice itself needs no gradient kernel
    assert sigma.shape == (125,) and bool(torch.isfinite(sigma).all())
