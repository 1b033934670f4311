"""``LSENeRFModel.export_tsdf_mesh`` on the small model of tests/test_gpu_mesh.py, with and without contraction, seen by four cameras
of 32 x 24 pixels at resolution 24: every stage of the export against the entry point it is built from, called directly on
``render_flat``'s outputs of the same bundles, and against the numpy twin -- all of it bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_ref as mr
from tests import tsdf_ref as tr
from tests.util import random_binaries

pytestmark = pytest.mark.gpu

H, W = 24, 32
CHUNK = 200               # four chunks a view, the last one 168 rays
RES = 24
BOUNDS = ((-0.9, -0.8, -0.7), (0.8, 0.9, 0.75))
EYES = [(0.2, 0.1, 2.5), (2.5, -0.1, 0.15), (-0.2, 2.5, 0.1), (-1.5, -1.6, -1.2)]


@functools.lru_cache(maxsize=None)
def _model(contraction=True):
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(5)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, log2_hashmap_size=14, eval_num_rays_per_chunk=CHUNK,
                             disable_scene_contraction=not contraction)
    m = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 8).cuda()
    with torch.no_grad():     # a table large enough for the logit to vary over a cell
        m.field.mlp_base_grid.params.uniform_(-0.5, 0.5, generator=torch.Generator(device="cuda").manual_seed(9))
    b = random_binaries(2, 32, 0.5, 5)
    m.occupancy_grid.binaries.copy_(b.cuda())
    m.occupancy_grid.occs.copy_(b.float().flatten().cuda() * 0.5)
    m.occupancy_grid._invalidate_occ_mean()
    return m.eval()


@functools.lru_cache(maxsize=None)
def _eval_set():
    from lsenerf_amd import EvalSet
    from lsenerf_amd.cameras import EdCameras
    c2w = torch.from_numpy(np.stack([tr.look_at(e) for e in EYES]))
    cams = EdCameras(c2w, fx=30.0, fy=30.0, cx=W / 2, cy=H / 2, width=W, height=H, times=torch.zeros(4))
    return EvalSet("cuda", torch.zeros((4, H, W, 3), dtype=torch.uint8), cams, appearance_ids=[1, 2, 3, 4])


@functools.lru_cache(maxsize=None)
def _renders(contraction):
    """(depth [4, HW], acc [4, HW], rgb [4, HW, 3]) of ``render_flat`` over the four bundles and the median accumulation.  Read-only."""
    from lsenerf_amd import evaluation
    from lsenerf_amd.eval_set import camera_bundle
    model = _model(contraction)
    outs = [evaluation.render_flat(model, evaluation._flatten_bundle(camera_bundle(_eval_set(), i), device="cuda")) for i in range(4)]
    depth = torch.stack([o["depth"].reshape(-1) for o in outs]).contiguous()
    acc = torch.stack([o["accumulation"].reshape(-1) for o in outs]).contiguous()
    rgb = torch.stack([o["rgb"].reshape(-1, 3) for o in outs]).contiguous()
    return depth, acc, rgb, float(acc.median())


def _box(model, bounds):
    aabb = model.field.aabb.cpu().tolist() if bounds is None else bounds
    return [float(np.float32(v)) for v in aabb[0]], [float(np.float32(v)) for v in aabb[1]]      # the box as float32 holds it


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _assert_same_mesh(a, b):
    for k in ("vertices", "triangles", "normals", "colors"):
        assert _same(getattr(a, k), getattr(b, k)), k


@functools.lru_cache(maxsize=None)
def _export(contraction=True, bounds=None, vpl=8):
    return _model(contraction).export_tsdf_mesh(_eval_set(), resolution=RES, bounds=bounds, min_accumulation=_renders(contraction)[3],
                                                views_per_launch=vpl)


@pytest.mark.parametrize("contraction", [True, False])
@pytest.mark.parametrize("bounds", [None, BOUNDS], ids=["aabb", "box"])
def test_every_stage_equals_its_entry_point_called_directly(contraction, bounds, monkeypatch):
    from lsenerf_amd import mesh as lm, ops, tsdf
    model, es = _model(contraction), _eval_set()
    depth, acc, rgb, min_acc = _renders(contraction)
    lo, hi = _box(model, bounds)
    res = (RES,) * 3
    volumes = []

    class Spy(tsdf.TSDFVolume):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            volumes.append(self)
    monkeypatch.setattr(tsdf, "TSDFVolume", Spy)
    got = model.export_tsdf_mesh(es, resolution=RES, bounds=bounds, min_accumulation=min_acc)
    assert len(volumes) == 1
    vol = volumes[0]
    trunc = 3.0 * max((h - l) / RES for l, h in zip(lo, hi))
    assert vol.res == res and vol.truncation == trunc and (vol.lo, vol.hi) == (lo, hi)
    # the volume: one integrate over the four renders, and the twin
    n = ops.lattice_points(res)
    tw, cw = torch.zeros((n, 2), device="cuda"), torch.zeros((n, 4), device="cuda")
    poses = es.poses[torch.as_tensor(es.data.image_idx_host).long().cuda()].contiguous()
    ops.tsdf_integrate(tw, cw, res, lo, hi, es.cam_desc, poses, depth, acc, rgb, trunc, min_acc, True)
    assert torch.equal(vol.tw, tw) and torch.equal(vol.cw, cw)
    cam = tr.Camera(30.0, 30.0, W / 2, H / 2, H, W)
    rtw, rcw = tr.integrate(*tr.new_state(res), res, lo, hi, cam, poses.cpu().numpy(), depth.cpu().numpy(), acc.cpu().numpy(),
                            rgb.cpu().numpy(), trunc, min_acc, True)
    assert _same(tw, rtw) and _same(cw, rcw)
    w = tw[:, 1]
    assert int((w == 0).sum()) > 0 and int((w >= 2).sum()) > 100 and int((cw[:, 3] > 0).sum()) > 100
    # the field and the mesh: masked surface nets at level 0
    fld = torch.where(w >= 1, -tw[:, 0], torch.full_like(w, float("nan")))
    assert _same(vol.field(1), fld) and _same(fld, tr.field(rtw))
    v, t, totals = ops.surface_nets(fld, res, lo, hi, 0.0, skip_nan=True)
    assert v.shape[0] > 100 and t.shape[0] > 100 and totals.tolist() == [v.shape[0], t.shape[0] // 2]
    assert torch.equal(got.vertices, v) and torch.equal(got.triangles, t)
    rv, rt = tr.surface_nets(tr.field(rtw), res, lo, hi, 0.0)
    assert _same(v, rv) and _same(t, rt)
    assert v.shape[0] < ops.surface_nets(fld, res, lo, hi, 0.0)[0].shape[0]            # the mask drops the shell against unobserved space
    # fused colours and normals
    col = ops.tsdf_vertex_colors(cw, res, lo, hi, v)
    assert torch.equal(got.colors, col) and _same(col, tr.vertex_colors(rcw, res, lo, hi, rv))
    assert float(col.min()) >= 0.0 and float(col.max()) <= 1.0 and float(col.std()) > 1e-3
    assert torch.equal(got.normals, lm.vertex_normals(model.field, v))


def test_views_per_launch_and_repeated_calls_give_the_same_bytes():
    base = _export(True, None, 8)
    assert base.vertices.shape[0] > 100
    for vpl in (1, 3):
        _assert_same_mesh(_export(True, None, vpl), base)
    _assert_same_mesh(_model(True).export_tsdf_mesh(_eval_set(), resolution=RES, min_accumulation=_renders(True)[3]), base)


def test_image_indices_select_and_order_and_a_pose_pair_is_the_eval_set():
    model, es = _model(True), _eval_set()
    min_acc = _renders(True)[3]
    kw = dict(resolution=RES, min_accumulation=min_acc)
    picked = model.export_tsdf_mesh(es, image_indices=[2, 0, 3], **kw)
    _assert_same_mesh(picked, model.export_tsdf_mesh(es, image_indices=[2, 0, 3], views_per_launch=2, **kw))
    assert picked.vertices.shape[0] > 50 and picked.vertices.shape != _export(True, None, 8).vertices.shape
    _assert_same_mesh(model.export_tsdf_mesh(es, image_indices=[0, 1, 2, 3], **kw), _export(True, None, 8))
    # the same views as (cameras, poses): the geometry needs no appearance id (the fused colours may: they come from the renders)
    pair = model.export_tsdf_mesh((es.cameras, es.poses[[2, 0, 3]]), colors=None, normals=False, **kw)
    again = model.export_tsdf_mesh((es.cameras, es.poses), image_indices=[2, 0, 3], colors=None, normals=False, **kw)
    _assert_same_mesh(pair, again)
    assert pair.vertices.shape[0] > 50
    with pytest.raises(ValueError, match="image index"):
        model.export_tsdf_mesh(es, image_indices=[4], **kw)


def test_colour_modes_fill_exactly_their_output():
    from lsenerf_amd import mesh as lm
    model, es = _model(True), _eval_set()
    base = _export(True, None, 8)
    kw = dict(resolution=RES, min_accumulation=_renders(True)[3])
    bare = model.export_tsdf_mesh(es, colors=None, normals=False, **kw)
    assert bare.colors is None and bare.normals is None and _same(bare.vertices, base.vertices) and _same(bare.triangles, base.triangles)
    only_n = model.export_tsdf_mesh(es, colors=None, **kw)
    assert only_n.colors is None and _same(only_n.normals, base.normals)
    fld = model.export_tsdf_mesh(es, colors="field", normals=False, **kw)
    assert fld.normals is None and _same(fld.vertices, base.vertices)
    assert _same(fld.colors, lm.vertex_colors(model, base.vertices, base.normals)) and not _same(fld.colors, base.colors)
    fused = model.export_tsdf_mesh(es, colors="fused", normals=False, **kw)
    assert fused.normals is None and _same(fused.colors, base.colors)
    with pytest.raises(ValueError, match="colors"):
        model.export_tsdf_mesh(es, colors="vertex", **kw)


def test_modes_parameters_and_config_are_untouched(monkeypatch):
    from lsenerf_amd import evaluation
    model, es = _model(True), _eval_set()
    cfg = model.config
    min_acc = _renders(True)[3]
    before = _export(True, None, 8)
    seen, writes, fail_at = [], [], [None]
    render_flat = evaluation.render_flat

    def spy(m, rb, check_overflow=True):
        if len(seen) == fail_at[0]:
            raise RuntimeError("no more views")
        seen.append((m.config.eval_normals, m.training, check_overflow, torch.is_grad_enabled()))
        return render_flat(m, rb, check_overflow=check_overflow)
    monkeypatch.setattr(evaluation, "render_flat", spy)
    monkeypatch.setattr(type(cfg), "__setattr__", lambda self, k, v: (writes.append(k), object.__setattr__(self, k, v))[1], raising=False)
    model.train()
    model.field.mlp_head.eval()                          # a mixed state: every module gets its own mode back
    try:
        modes = [m.training for m in model.modules()]
        grads = [p.requires_grad for p in model.parameters()]
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        fields = dict(vars(cfg))
        with torch.enable_grad():
            mesh = model.export_tsdf_mesh(es, resolution=RES, min_accumulation=min_acc)
        assert seen == [("off", False, False, False)] * 4 and writes == []
        _assert_same_mesh(mesh, before)
        assert not mesh.vertices.requires_grad and all(p.grad is None for p in model.parameters())

        def untouched():
            assert [m.training for m in model.modules()] == modes and model.training
            assert [p.requires_grad for p in model.parameters()] == grads and dict(vars(cfg)) == fields
            for k, v in model.state_dict().items():
                assert torch.equal(v, state[k]), k
        untouched()
        # a refusal in the middle of the argument checks, and a failure in the middle of the views
        del seen[:]
        for kw, match in ((dict(image_indices=[0, 7]), "image index"), (dict(truncation=-1.0), "truncation"),
                          (dict(views_per_launch=0), "views_per_launch"), (dict(resolution=0), "resolution"),
                          (dict(bounds=[[0, 0, 0], [0, 1, 1]]), "empty box"), (dict(colors="rgb"), "colors")):
            with pytest.raises(ValueError, match=match):
                model.export_tsdf_mesh(es, **{**dict(resolution=RES), **kw})
        assert seen == [] and writes == []
        untouched()
        fail_at[0] = 2
        with pytest.raises(RuntimeError, match="no more views"):
            model.export_tsdf_mesh(es, resolution=RES, min_accumulation=min_acc)
        assert len(seen) == 2
        untouched()
        model.occupancy_grid.check_deferred_overflow()
        # with the normals pass configured, it is switched off for the renders and put back
        del seen[:]
        fail_at[0] = None
        object.__setattr__(cfg, "eval_normals", "world")
        mesh = model.export_tsdf_mesh(es, resolution=RES, min_accumulation=min_acc)
        assert [s[0] for s in seen] == ["off"] * 4 and cfg.eval_normals == "world" and sorted(set(writes)) == ["eval_normals"]
        _assert_same_mesh(mesh, before)
    finally:
        object.__setattr__(cfg, "eval_normals", "off")
        model.eval()


def test_ply_of_the_result_reads_back(tmp_path):
    from lsenerf_amd.mesh import write_ply
    mesh = _export(True, None, 8)
    path = str(tmp_path / "tsdf.ply")
    write_ply(path, mesh)
    verts, faces, names = mr.read_ply(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert _same(np.stack([verts["x"], verts["y"], verts["z"]], 1), mesh.vertices) and _same(faces, mesh.triangles)
    assert _same(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), mesh.normals)
    want = np.rint(np.clip(mesh.colors.cpu().numpy(), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(np.stack([verts["red"], verts["green"], verts["blue"]], 1), want)


from tests.test_scene_io_cpu import scene  # noqa: E402,F401  (the fixture: a tiny scene directory with both camera sets)


def test_the_tool_writes_the_mesh_of_a_checkpoint(scene, tmp_path, capsys):  # noqa: F811
    """tools/export_tsdf_mesh.py on a saved checkpoint and the scene's four val cameras (8 x 6 px): the file holds the mesh the
    same model gives when called directly."""
    import importlib.util
    import os
    from lsenerf_amd import checkpoint
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("export_tsdf_mesh_tool", os.path.join(root, "tools", "export_tsdf_mesh.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from tests.test_scene_io_cpu import _write_cam
    for i in range(9):                                   # the scene's colour cameras, moved onto a ring around the box, looking at it
        ang = 2 * np.pi * i / 9
        pose = tr.look_at((2.4 * np.cos(ang), 2.4 * np.sin(ang), 0.6 * np.sin(3 * ang))).astype(np.float64)
        w2c_rot = np.diag([1.0, -1.0, -1.0]) @ pose[:, :3].T            # OpenCV world -> camera: rows right, down, forward
        _write_cam(os.path.join(scene["root"], "colcam_set", "camera", f"{i:05d}.json"), w2c_rot, pose[:, 3], t=0.5 * i, f=8.0)
    model = _model(True)
    ckpt = str(tmp_path / "nerfstudio_models")
    checkpoint.save_nerfstudio_checkpoint(ckpt, model, step=7)
    out = str(tmp_path / "out.ply")
    min_acc = _renders(True)[3]
    tool.main([ckpt, scene["root"], out, "--resolution", "16", "--min-accumulation", repr(min_acc), "--split", "val",
               "--config", "grid_levels=2", "--config", "grid_resolution=32", "--config", "log2_hashmap_size=14",
               "--config", f"eval_num_rays_per_chunk={CHUNK}"])
    assert "from 4 views" in capsys.readouterr().out
    es = tool.scene_eval_set(scene["root"], "val", 1.0, 1.0)
    want = model.export_tsdf_mesh(es, resolution=16, min_accumulation=min_acc)
    verts, faces, names = mr.read_ply(out)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]
    assert _same(np.stack([verts["x"], verts["y"], verts["z"]], 1), want.vertices) and _same(faces, want.triangles)
    assert _same(np.stack([verts["nx"], verts["ny"], verts["nz"]], 1), want.normals)
    print("TSDF_TOOL vertices", want.vertices.shape[0], "triangles", want.triangles.shape[0])
    assert want.vertices.shape[0] > 50 and want.triangles.shape[0] > 50 and float((es.poses[:, :, 3].norm(dim=-1) - 2.4).abs().max()) < 0.7
