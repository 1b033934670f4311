"""Quantile depths in the eval render and the exporters, on the small model of tests/test_gpu_tsdf.py seen by four cameras of
32 x 24 pixels: the two new keys on both count-free routes, every other key untouched, and ``depth="median"`` of the two exporters
against the same pipeline assembled by hand from ``render_flat`` and the existing ``ops`` calls -- all of it bit for bit."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import tsdf_ref as tr
from tests.util import random_binaries

pytestmark = pytest.mark.gpu

H, W = 24, 32
CHUNK = 200               # four chunks a view, the last one 168 rays
RES = 24
QS = (0.25, 0.5, 0.75)
EPS = 1e-4
OPAQUE_SCALE = 30.0
_MIN_ACC = 0.5
EYES = [(0.2, 0.1, 2.5), (2.5, -0.1, 0.15), (-0.2, 2.5, 0.1), (-1.5, -1.6, -1.2)]


@functools.lru_cache(maxsize=None)
def _model():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(5)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, log2_hashmap_size=14, eval_num_rays_per_chunk=CHUNK)
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


def _bundle(i):
    from lsenerf_amd import evaluation
    from lsenerf_amd.eval_set import camera_bundle
    return evaluation._flatten_bundle(camera_bundle(_eval_set(), i), device="cuda")


@contextlib.contextmanager
def _settings(**kw):
    """Config fields of the shared model for the duration."""
    cfg = _model().config
    saved = {k: getattr(cfg, k) for k in kw}
    try:
        for k, v in kw.items():
            setattr(cfg, k, v)
        yield
    finally:
        for k, v in saved.items():
            setattr(cfg, k, v)


def _render(i, depth_select=None, **kw):
    from lsenerf_amd import evaluation
    with _settings(**kw):
        more = {} if depth_select is None else {"depth_select": depth_select}
        return {k: v.clone() for k, v in evaluation.render_flat(_model(), _bundle(i), **more).items()}


@functools.lru_cache(maxsize=None)
def _views(eps=0.0, normals="off"):
    """The four renders with the exporters' quantile settings.  Read-only."""
    return [_render(i, eval_depth_quantiles=QS, eval_depth_interpolate=True, eval_early_stop_eps=eps, eval_normals=normals)
            for i in range(4)]


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                                                                       np.ascontiguousarray(b).view(np.uint8))


def _selected(out, max_spread=None):
    """``depth_sel`` of the definition from the render's two keys, by torch: the 0.5 column where it was reached (and, with
    ``max_spread``, the 0.75 one too, at most that far behind the 0.25 one); NaN elsewhere."""
    dq, reached = out["depth_quantiles"], out["depth_reached"].reshape(-1)
    ok = (reached & 2) != 0
    if max_spread is not None:
        ok = ok & ((reached & 4) != 0) & ((dq[:, 2] - dq[:, 0]) <= np.float32(max_spread))
    return torch.where(ok, dq[:, 1], torch.full_like(dq[:, 1], float("nan"))).contiguous()


@pytest.mark.parametrize("eps", [0.0, EPS], ids=["count_free", "early_stop"])
@pytest.mark.parametrize("interpolate", [False, True], ids=["mid", "interpolated"])
def test_two_new_keys_and_every_other_key_as_before(eps, interpolate):
    off = _render(0, eval_early_stop_eps=eps)
    on = _render(0, eval_early_stop_eps=eps, eval_depth_quantiles=QS, eval_depth_interpolate=interpolate)
    assert set(on) == set(off) | {"depth_quantiles", "depth_reached"} and "depth_quantiles" not in off
    for k in off:
        assert _same(on[k], off[k]), k
    dq, reached = on["depth_quantiles"], on["depth_reached"]
    assert dq.shape == (H * W, 3) and dq.dtype == torch.float32 and reached.shape == (H * W, 1) and reached.dtype == torch.uint8
    assert bool(torch.isfinite(dq).all()) and int(reached.max()) <= 7
    hit = ((reached >> torch.arange(3, device="cuda")[None, :]) & 1) == 1
    assert bool(((dq[:, 1:] >= dq[:, :-1]) | ~hit[:, 1:]).all())
    n_median = int(hit[:, 1].sum())
    print(f"DEPTHQ_EVAL eps {eps:g} interpolate {interpolate}: median reached on {n_median} of {H * W} rays")
    assert n_median > 0
    # where the weights reach one half the median lies inside the ray's sampled range; "depth" stays the expected depth
    acc = on["accumulation"].reshape(-1)
    assert bool((acc[hit[:, 1]] >= 0.5 - 1e-4).all()) and bool((acc[~hit[:, 2]] < 0.75 + 1e-4).all())
    with_sel = _render(0, depth_select=(1, None), eval_early_stop_eps=eps, eval_depth_quantiles=QS, eval_depth_interpolate=interpolate)
    assert set(with_sel) == set(on) | {"depth_selected"}
    assert _same(with_sel["depth_selected"].reshape(-1), _selected(on)) and _same(with_sel["depth_quantiles"], dq)
    tight = _render(0, depth_select=(1, 0.02), eval_early_stop_eps=eps, eval_depth_quantiles=QS, eval_depth_interpolate=interpolate)
    assert _same(tight["depth_selected"].reshape(-1), _selected(on, 0.02))
    assert int(torch.isnan(tight["depth_selected"]).sum()) > int(torch.isnan(with_sel["depth_selected"]).sum())


def test_routes_agree_bit_for_bit_and_normals_ride_along():
    full, early = _views(0.0), _views(EPS)
    for a, b in zip(full, early):
        assert _same(a["depth_quantiles"], b["depth_quantiles"]) and _same(a["depth_reached"], b["depth_reached"])
    stopped = sum(int((a["num_samples_per_ray"] > b["num_samples_per_ray"]).sum()) for a, b in zip(full, early))
    print(f"DEPTHQ_EVAL early stop: {stopped} of {4 * H * W} rays were stopped before their end")
    # the same with surfaces: the hash table times OPAQUE_SCALE (found with one render: 10 stops no ray of view 0, 30 stops 698 of its
    # 768) -- the early-stop route then leaves most rays before their end, and the quantiles found by then are the full route's
    table = _model().field.mlp_base_grid.params
    saved = table.detach().clone()
    try:
        with torch.no_grad():
            table.mul_(OPAQUE_SCALE)
        kw = dict(eval_depth_quantiles=QS, eval_depth_interpolate=True)
        a, b = _render(0, **kw), _render(0, eval_early_stop_eps=EPS, **kw)
    finally:
        with torch.no_grad():
            table.copy_(saved)
    stopped = int((a["num_samples_per_ray"] > b["num_samples_per_ray"]).sum())
    print(f"DEPTHQ_EVAL early stop, opaque field: {stopped} of {H * W} rays were stopped before their end")
    assert stopped > H * W // 2 and int((a["depth_reached"] == 7).sum()) > H * W // 2
    assert _same(a["depth_quantiles"], b["depth_quantiles"]) and _same(a["depth_reached"], b["depth_reached"])
    with_normals = _views(0.0, "world")
    for a, b in zip(full, with_normals):
        assert "normals" in b and _same(a["depth_quantiles"], b["depth_quantiles"]) and _same(a["depth_reached"], b["depth_reached"])
    with _settings(eval_depth_quantiles=(0.5, 1 - EPS / 2), eval_early_stop_eps=EPS):
        from lsenerf_amd import evaluation
        with pytest.raises(ValueError, match="1 - q >= eps"):
            evaluation.render_flat(_model(), _bundle(0))
    _model().occupancy_grid.check_deferred_overflow()


def _min_acc():
    return float(torch.cat([o["accumulation"].reshape(-1) for o in _views(0.0)]).median())


def _median_spread():
    """The median distance between the 0.25 and 0.75 depths over the four views: a ``max_depth_spread`` that drops half the rays."""
    return float(torch.cat([o["depth_quantiles"][:, 2] - o["depth_quantiles"][:, 0] for o in _views(0.0)]).median())


@pytest.mark.parametrize("spread", [False, True], ids=["median", "spread"])
def test_point_cloud_median_equals_the_pipeline_by_hand(spread):
    from lsenerf_amd import ops
    max_spread = _median_spread() if spread else None
    model, es = _model(), _eval_set()
    min_acc = _min_acc()
    lo, hi = [-1.0] * 3, [1.0] * 3
    got = model.export_point_cloud(es, min_accumulation=min_acc, depth="median", max_depth_spread=max_spread)
    n = 4 * H * W
    pts, col, nrm = (torch.empty((n, 3), device="cuda") for _ in range(3))
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    for i, out in enumerate(_views(0.0, "world")):
        rb = _bundle(i)
        ops.unproject_append(rb.origins.contiguous(), rb.directions.contiguous(), _selected(out, max_spread),
                             out["accumulation"].reshape(-1).contiguous(), lo, hi, min_acc, pts, total, colors=out["rgb"].contiguous(),
                             normals=out["normals"].contiguous(), out_colors=col, out_normals=nrm)
    kept = int(total.item())
    assert got.points.shape == (kept, 3) and kept > 100
    assert _same(got.points, pts[:kept]) and _same(got.colors, col[:kept]) and _same(got.normals, nrm[:kept])
    expected = model.export_point_cloud(es, min_accumulation=min_acc)
    print(f"DEPTHQ_EVAL point cloud: expected {expected.points.shape[0]} points, median (max_spread {max_spread}) {kept}")
    assert not _same(got.points, expected.points)
    # without normals the exporter keeps the configured route: the early-stop render gives the same cloud
    with _settings(eval_early_stop_eps=EPS):
        early = model.export_point_cloud(es, min_accumulation=min_acc, depth="median", max_depth_spread=max_spread, normals=False)
    assert early.normals is None and _same(early.points, got.points)


@pytest.mark.parametrize("spread", [False, True], ids=["median", "spread"])
def test_tsdf_mesh_median_equals_the_pipeline_by_hand(spread):
    from lsenerf_amd import ops
    max_spread = _median_spread() if spread else None
    model, es = _model(), _eval_set()
    min_acc = _min_acc()
    lo, hi = [-1.0] * 3, [1.0] * 3
    res = (RES,) * 3
    trunc = 3.0 * max((h - l) / RES for l, h in zip(lo, hi))
    got = model.export_tsdf_mesh(es, resolution=RES, min_accumulation=min_acc, normals=False, depth="median", max_depth_spread=max_spread)
    views = _views(0.0)
    depth = torch.stack([_selected(o, max_spread) for o in views]).contiguous()
    acc = torch.stack([o["accumulation"].reshape(-1) for o in views]).contiguous()
    rgb = torch.stack([o["rgb"].reshape(-1, 3) for o in views]).contiguous()
    n = ops.lattice_points(res)
    tw, cw = torch.zeros((n, 2), device="cuda"), torch.zeros((n, 4), device="cuda")
    poses = es.poses[torch.as_tensor(es.data.image_idx_host).long().cuda()].contiguous()
    ops.tsdf_integrate(tw, cw, res, lo, hi, es.cam_desc, poses, depth, acc, rgb, trunc, min_acc, True)
    fld = torch.where(tw[:, 1] >= 1, -tw[:, 0], torch.full_like(tw[:, 1], float("nan")))
    v, t, _ = ops.surface_nets(fld, res, lo, hi, 0.0, skip_nan=True)
    assert v.shape[0] > 50 and _same(got.vertices, v) and _same(got.triangles, t)
    assert _same(got.colors, ops.tsdf_vertex_colors(cw, res, lo, hi, v))
    expected = model.export_tsdf_mesh(es, resolution=RES, min_accumulation=min_acc, normals=False)
    n_nan = int(torch.isnan(depth).sum())
    print(f"DEPTHQ_EVAL tsdf: expected {expected.vertices.shape[0]} vertices, median (max_spread {max_spread}) {v.shape[0]}; "
          f"{n_nan} of {depth.numel()} pixels without a usable depth")
    assert (n_nan > 0 or not spread) and not _same(got.vertices, expected.vertices)


def test_expected_is_the_call_without_the_argument():
    model, es = _model(), _eval_set()
    min_acc = _min_acc()
    a = model.export_point_cloud(es, min_accumulation=min_acc, voxel_size=0.1, min_support=2)
    b = model.export_point_cloud(es, min_accumulation=min_acc, voxel_size=0.1, min_support=2, depth="expected")
    for k in ("points", "colors", "normals", "counts"):
        assert _same(getattr(a, k), getattr(b, k)), k
    a = model.export_tsdf_mesh(es, resolution=RES, min_accumulation=min_acc)
    b = model.export_tsdf_mesh(es, resolution=RES, min_accumulation=min_acc, depth="expected")
    for k in ("vertices", "triangles", "normals", "colors"):
        assert _same(getattr(a, k), getattr(b, k)), k
    assert a.vertices.shape[0] > 50


@pytest.mark.parametrize("which", ["point_cloud", "tsdf_mesh"])
def test_config_and_modes_come_back_also_behind_an_exception(which, monkeypatch):
    from lsenerf_amd import evaluation
    model, es = _model(), _eval_set()
    cfg = model.config
    export = model.export_point_cloud if which == "point_cloud" else functools.partial(model.export_tsdf_mesh, resolution=RES)
    seen, fail_at = [], [None]
    render_flat = evaluation.render_flat

    def spy(m, rb, check_overflow=True, **kw):
        if len(seen) == fail_at[0]:
            raise RuntimeError("no more views")
        seen.append((m.config.eval_depth_quantiles, m.config.eval_depth_interpolate, m.training, kw.get("depth_select")))
        return render_flat(m, rb, check_overflow=check_overflow, **kw)
    monkeypatch.setattr(evaluation, "render_flat", spy)
    object.__setattr__(cfg, "eval_depth_quantiles", (0.5,))          # the user's own setting: it comes back, not the default
    model.train()
    model.field.mlp_head.eval()
    try:
        modes = [m.training for m in model.modules()]
        fields = dict(vars(cfg))
        export(es, min_accumulation=_MIN_ACC, depth="median", max_depth_spread=0.05)
        assert seen == [(QS, True, False, (1, 0.05))] * 4
        assert [m.training for m in model.modules()] == modes and dict(vars(cfg)) == fields
        del seen[:]
        fail_at[0] = 2
        with pytest.raises(RuntimeError, match="no more views"):
            export(es, min_accumulation=_MIN_ACC, depth="median")
        assert len(seen) == 2 and seen[0][3] == (1, None)
        assert [m.training for m in model.modules()] == modes and dict(vars(cfg)) == fields
        model.occupancy_grid.check_deferred_overflow()
    finally:
        object.__setattr__(cfg, "eval_depth_quantiles", ())
        model.eval()

