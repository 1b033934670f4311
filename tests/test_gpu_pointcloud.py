"""``LSENeRFModel.export_point_cloud`` on the small model of tests/test_gpu_eval_normals.py / tests/test_gpu_mesh.py seen by three
cameras of 24 x 40 pixels: every stage of the export against the entry point it is built from, called directly on ``render_flat``'s
outputs of the same bundles, and against the numpy twin -- bit for bit (merged normals: 3 ulp, tests/test_gpu_pointcloud_kernels.py)."""
import functools

import numpy as np
import pytest
import torch

from tests import pointcloud_ref as pr
from tests.util import random_binaries

pytestmark = pytest.mark.gpu

H, W = 24, 40             # 960 rays a view
CHUNK = 100               # ten chunks, the last one 60 rays
VOXEL = 0.11
LO, HI = [-1.0] * 3, [1.0] * 3


@functools.lru_cache(maxsize=None)
def _model():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(5)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, eval_num_rays_per_chunk=CHUNK, log2_hashmap_size=14)
    m = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 8).cuda()
    with torch.no_grad():     # a table large enough for the logit to vary over a cell: gradients of ordinary size
        m.field.mlp_base_grid.params.uniform_(-0.5, 0.5, generator=torch.Generator(device="cuda").manual_seed(9))
    b = random_binaries(2, 32, 0.5, 5)
    m.occupancy_grid.binaries.copy_(b.cuda())
    m.occupancy_grid.occs.copy_(b.float().flatten().cuda() * 0.5)
    m.occupancy_grid._invalidate_occ_mean()
    return m.eval()


@functools.lru_cache(maxsize=None)
def _eval_set():
    """Three cameras 2.5 from the centre, on +z, +x and +y, looking at it (OpenGL frame: -z forward)."""
    from lsenerf_amd import EvalSet
    from lsenerf_amd.cameras import EdCameras
    c2w = torch.tensor([[[1.0, 0, 0, 0.2], [0, 1, 0, 0.1], [0, 0, 1, 2.5]],
                        [[0.0, 0, 1, 2.5], [0, 1, 0, -0.1], [-1, 0, 0, 0.15]],
                        [[1.0, 0, 0, -0.2], [0, 0, 1, 2.5], [0, -1, 0, 0.1]]])
    cams = EdCameras(c2w, fx=30.0, fy=30.0, cx=W / 2, cy=H / 2, width=W, height=H, times=torch.zeros(3))
    images = torch.zeros((3, H, W, 3), dtype=torch.uint8)
    return EvalSet("cuda", images, cams, appearance_ids=[1, 2, 3])


def _bundles():
    from lsenerf_amd.eval_set import camera_bundle
    return [camera_bundle(_eval_set(), i) for i in range(3)]


@functools.lru_cache(maxsize=None)
def _renders():
    """``render_flat`` of the three bundles with world normals on the full route, and the median accumulation.  Read-only."""
    from lsenerf_amd import evaluation
    model = _model()
    cfg = model.config
    saved = cfg.eval_normals, cfg.eval_early_stop_eps
    cfg.eval_normals, cfg.eval_early_stop_eps = "world", 0.0
    try:
        outs = []
        for b in _bundles():
            rb = evaluation._flatten_bundle(b, device="cuda")
            out = evaluation.render_flat(model, rb)
            outs.append((rb.origins.contiguous(), rb.directions.contiguous(), out["depth"].reshape(-1).contiguous(),
                         out["accumulation"].reshape(-1).contiguous(), out["rgb"].contiguous(), out["normals"].contiguous()))
    finally:
        cfg.eval_normals, cfg.eval_early_stop_eps = saved
    acc = torch.cat([o[3] for o in outs])
    return tuple(outs), float(acc.median())


def _host(views):
    return [tuple(t.cpu().numpy() for t in v) for v in views]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def _assert_same_cloud(a, b):
    for k in ("points", "colors", "normals", "counts"):
        assert _same(getattr(a, k), getattr(b, k)), k


@functools.lru_cache(maxsize=None)
def _export(voxel=None, min_support=0):
    _, min_acc = _renders()
    return _model().export_point_cloud(_eval_set(), min_accumulation=min_acc, voxel_size=voxel, min_support=min_support)


def test_every_stage_equals_its_entry_point_and_the_twin():
    from lsenerf_amd import ops
    views, min_acc = _renders()
    n_rays = 3 * H * W
    # the raw cloud: three appends in view order
    pts, col, nrm = (torch.full((n_rays, 3), -7.0, device="cuda") for _ in range(3))
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    for o, d, t, a, c, n in views:
        ops.unproject_append(o, d, t, a, LO, HI, min_acc, pts, total, colors=c, normals=n, out_colors=col, out_normals=nrm)
    kept = int(total.item())
    assert 0.15 * n_rays < kept < 0.75 * n_rays              # about half of the rays pass the median; some of them leave the box
    raw = _export()
    assert raw.counts is None and raw.points.shape == (kept, 3)
    assert _same(raw.points, pts[:kept]) and _same(raw.colors, col[:kept]) and _same(raw.normals, nrm[:kept])
    wp, wc, wn, wtotal = pr.append(_host(views), LO, HI, min_acc)
    assert wtotal == kept and _same(raw.points, wp) and _same(raw.colors, wc) and _same(raw.normals, wn)
    length = raw.normals.norm(dim=-1)
    assert bool(((length - 1).abs() < 1e-4).logical_or(length == 0).all()) and float((length > 0).float().mean()) > 0.9
    assert float(raw.colors.min()) >= 0.0 and float(raw.colors.max()) <= 1.0
    # merged: keys, a stable sort, the merge
    res = ops.voxel_lattice(LO, HI, VOXEL)
    assert res == (19, 19, 19)
    keys = ops.voxel_keys(pts, LO, VOXEL, res, n_dev=total)
    sorted_keys, order = torch.sort(keys, stable=True)
    mk, mc, mp, mcol, mn, mt = ops.voxel_merge(sorted_keys, order, pts, col, nrm)
    m = int(mt.item())
    merged = _export(VOXEL)
    assert 50 < m < kept and merged.points.shape == (m, 3) and int(merged.counts.sum()) == kept
    assert _same(merged.points, mp[:m]) and _same(merged.colors, mcol[:m]) and _same(merged.normals, mn[:m])
    assert _same(merged.counts, mc[:m])
    tk, tc, tp, tcol, tn = pr.merge(wp, LO, VOXEL, res, wc, wn)
    assert np.array_equal(mk[:m].cpu().numpy(), tk) and _same(merged.counts, tc)
    assert _same(merged.points, tp) and _same(merged.colors, tcol)
    ok = np.isfinite(tn).all(-1)
    assert ok.mean() > 0.99
    ulps = pr.ulp_distance(merged.normals.cpu().numpy()[ok], tn[ok])
    print(f"merged normals of {m} voxels differ from the twin by at most {ulps} ulp")
    assert ulps <= 3
    # filtered: a support threshold that removes some voxels and keeps others
    sup = pr.support(tk, tc, res)
    thr = int(np.median(sup))
    keep, _ = pr.support_filter(tk, tc, res, thr)
    assert 0 < keep.sum() < m
    fk, fc, fp, fcol, fn, ft, _ = ops.voxel_support_filter(mk, mc, mp, res, thr, mcol, mn, m_dev=mt)
    f = int(ft.item())
    filtered = _export(VOXEL, thr)
    assert f == int(keep.sum()) and np.array_equal(fk[:f].cpu().numpy(), tk[keep])
    assert _same(filtered.points, fp[:f]) and _same(filtered.colors, fcol[:f]) and _same(filtered.normals, fn[:f])
    assert _same(filtered.counts, fc[:f]) and _same(filtered.points, tp[keep]) and _same(filtered.counts, tc[keep])
    assert _same(filtered.normals, merged.normals[torch.from_numpy(keep).cuda()])


def test_routes_views_and_options():
    model = _model()
    _, min_acc = _renders()
    bundles = _bundles()
    es = _eval_set()
    raw = _export()
    _assert_same_cloud(model.export_point_cloud(bundles, min_accumulation=min_acc), raw)             # a list of [H, W] bundles
    _assert_same_cloud(model.export_point_cloud(iter(bundles), min_accumulation=min_acc), raw)       # any iterable
    picked = model.export_point_cloud(es, image_indices=[2, 0], min_accumulation=min_acc, voxel_size=VOXEL)
    _assert_same_cloud(picked, model.export_point_cloud([bundles[2], bundles[0]], min_accumulation=min_acc, voxel_size=VOXEL))
    assert picked.points.shape[0] < _export(VOXEL).points.shape[0]
    bare = model.export_point_cloud(es, min_accumulation=min_acc, normals=False, colors=False)
    assert bare.normals is None and bare.colors is None and _same(bare.points, raw.points)
    _assert_same_cloud(model.export_point_cloud(es, min_accumulation=min_acc, voxel_size=VOXEL, min_support=3), _export(VOXEL, 3))
    # a capacity below the total trims, in order, without an error
    cut = model.export_point_cloud(es, min_accumulation=min_acc, max_points=500)
    assert cut.points.shape == (500, 3) and _same(cut.points, raw.points[:500]) and _same(cut.normals, raw.normals[:500])
    box = ((-0.5, -0.6, -0.4), (0.6, 0.5, 0.7))
    inside = model.export_point_cloud(es, min_accumulation=min_acc, bounds=box)
    p = raw.points
    want = ((p >= p.new_tensor(box[0])) & (p <= p.new_tensor(box[1]))).all(-1)
    assert 0 < int(want.sum()) < p.shape[0] and _same(inside.points, p[want])
    with pytest.raises(ValueError, match="image index"):
        model.export_point_cloud(es, image_indices=[3])


def test_settings_and_modes_are_restored(monkeypatch):
    from lsenerf_amd import evaluation
    model = _model()
    cfg = model.config
    _, min_acc = _renders()
    es = _eval_set()
    before = _export()
    eps0 = cfg.eval_early_stop_eps
    seen, writes, fail_at = [], [], [None]
    render_flat = evaluation.render_flat

    def spy(m, rb, check_overflow=True):
        if len(seen) == fail_at[0]:
            raise RuntimeError("no more views")
        out = render_flat(m, rb, check_overflow=check_overflow)
        seen.append((m.config.eval_normals, m.config.eval_early_stop_eps, m.training, check_overflow, "normals" in out))
        return out
    monkeypatch.setattr(evaluation, "render_flat", spy)
    cls = type(cfg)
    monkeypatch.setattr(cls, "__setattr__", lambda self, k, v: (writes.append(k), object.__setattr__(self, k, v))[1], raising=False)
    model.train()
    model.field.mlp_head.eval()                          # a mixed state: every module gets its own mode back
    object.__setattr__(cfg, "eval_early_stop_eps", 1e-4)
    try:
        modes = [m.training for m in model.modules()]
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        with torch.enable_grad():
            cloud = model.export_point_cloud(es, min_accumulation=min_acc)
        assert seen == [("world", 0.0, False, False, True)] * 3                  # the override holds during the renders ...
        assert (cfg.eval_normals, cfg.eval_early_stop_eps) == ("off", 1e-4)      # ... and is undone
        assert sorted(set(writes)) == ["eval_early_stop_eps", "eval_normals"]
        assert [m.training for m in model.modules()] == modes and model.training
        assert not cloud.points.requires_grad and all(p.grad is None for p in model.parameters())
        _assert_same_cloud(cloud, before)
        for k, v in model.state_dict().items():
            assert torch.equal(v, state[k]), k
        # without normals the configuration is never written and no normals are rendered: the early-stop route stays on
        del seen[:], writes[:]
        bare = model.export_point_cloud(es, min_accumulation=min_acc, normals=False)
        assert writes == [] and seen == [("off", 1e-4, False, False, False)] * 3
        assert bare.normals is None and bare.points.shape[0] > 0 and [m.training for m in model.modules()] == modes

        # a failure inside the export still restores everything
        del seen[:], writes[:]
        fail_at[0] = 1                                   # the second render raises
        with pytest.raises(RuntimeError, match="no more views"):
            model.export_point_cloud(es, min_accumulation=min_acc)
        assert len(seen) == 1 and seen[0][:2] == ("world", 0.0)
        assert (cfg.eval_normals, cfg.eval_early_stop_eps) == ("off", 1e-4) and [m.training for m in model.modules()] == modes
        model.occupancy_grid.check_deferred_overflow()
    finally:
        object.__setattr__(cfg, "eval_early_stop_eps", eps0)
        model.eval()


def test_two_calls_are_bit_identical_and_renders_are_unchanged():
    model = _model()
    _, min_acc = _renders()
    b = _bundles()[1]
    before = model.get_outputs_for_camera_ray_bundle(b)
    a = model.export_point_cloud(_eval_set(), min_accumulation=min_acc, voxel_size=VOXEL, min_support=3)
    c = model.export_point_cloud(_eval_set(), min_accumulation=min_acc, voxel_size=VOXEL, min_support=3)
    _assert_same_cloud(a, c)
    assert a.points.shape[0] > 20
    after = model.get_outputs_for_camera_ray_bundle(b)
    assert set(before) == set(after) and "normals" not in after
    for k in before:
        assert torch.equal(before[k], after[k]), k


def test_ply_of_the_result_reads_back(tmp_path):
    from lsenerf_amd.pointcloud import write_ply_points
    cloud = _export(VOXEL, 3)
    path = str(tmp_path / "cloud.ply")
    write_ply_points(path, cloud)
    rec, names = pr.read_ply_points(path)
    assert names == ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"] and rec.shape[0] == cloud.points.shape[0]
    assert np.array_equal(np.stack([rec["x"], rec["y"], rec["z"]], 1), cloud.points.cpu().numpy())
    assert np.array_equal(np.stack([rec["nx"], rec["ny"], rec["nz"]], 1), cloud.normals.cpu().numpy())
    want = np.rint(np.clip(cloud.colors.cpu().numpy(), 0, 1) * 255).astype(np.uint8)
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], 1), want)
