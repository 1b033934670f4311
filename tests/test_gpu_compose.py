"""The batch composer on the GPU (lsenerf_amd.data, csrc/compose.hip): the device draw against its host twin, the composed step
against the host composition built from the scene_io datasets and the cameras.py generators, the pose-table backward against
float64 autograd, and the composer inside the eager and the captured training step."""
import copy

import numpy as np
import pytest
import torch

from tests.test_compose_cpu import (COL_APP, COL_HW, COL_TIMES, EVS_HW, N_COL, N_FRAMES, host_batch, host_compose, make_scene,
                                    random_indices)
from tests.util import TOL_FWD, TOL_GRAD, nmax_err, random_binaries

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

NUM_EMBD = 8


def _scene(tmp_path, **kw):
    from lsenerf_amd.data import DeviceScene
    col_ds, evs_ds = make_scene(tmp_path, **kw)
    return col_ds, evs_ds, DeviceScene.from_datasets(col_ds, evs_ds, "cuda", rgb_times=torch.tensor(COL_TIMES))


def _spline(cams, device="cpu", exp_t=0.3):
    from lsenerf_amd import cameras as cam
    return cam.CameraOptimizerConfig(mode="SO3xR3", optim_type="spline", exp_t=exp_t).setup(num_cameras=len(cams), device=device,
                                                                                            cameras=cams, dM=torch.eye(4))


def _indices(n_col, n_evs, seed):
    """Given pixels; the first rows pin the cases the comparison must see: both clip ends of the deblur appearance offsets (colour
    images 0 and 5) and the event cameras whose closest colour camera is a tie / lies beyond either end."""
    col = random_indices(n_col, N_COL, COL_HW, seed)
    evs = random_indices(n_evs, N_FRAMES, EVS_HW, seed + 1)
    col[0, 0], col[1, 0] = 0, N_COL - 1
    evs[:4, 0] = torch.tensor([0, 1, N_FRAMES - 1, N_FRAMES - 2])
    return col, evs


# ---------------------------------------------------------------------------------------------------- 5. the draw
def test_device_draw_equals_the_host_twin_and_given_indices_are_honoured(tmp_path):
    from lsenerf_amd.data import BatchComposer
    _, _, scene = _scene(tmp_path)
    comp = BatchComposer(scene, 300, 200, seed=2 ** 40 + 7, num_embd=NUM_EMBD)
    for step in (0, 3, 2 ** 32 + 11):
        _, batch = comp.compose(step=step)
        want_col, want_evs = comp.indices_host(step)
        assert np.array_equal(batch["col_batch"]["indices"].cpu().numpy(), want_col)
        assert np.array_equal(batch["evs_batch"]["indices"].cpu().numpy(), want_evs)
        assert int(comp.step_dev) == 0                                  # an explicit step leaves the counter alone
    assert not np.array_equal(comp.indices_host(0)[0][:200], comp.indices_host(0)[1])      # the streams differ
    for k in range(3):                                                  # the device counter: used, then advanced
        _, batch = comp.compose()
        assert np.array_equal(batch["col_batch"]["indices"].cpu().numpy(), comp.indices_host(k)[0])
        assert int(comp.step_dev) == k + 1
    col_i, evs_i = _indices(300, 200, 4)
    (col, prev, nxt), batch = comp.compose(indices=(col_i, evs_i))
    assert torch.equal(batch["col_batch"]["indices"].cpu().long(), col_i) and torch.equal(batch["evs_batch"]["indices"].cpu().long(), evs_i)
    assert torch.equal(col.metadata["coords"].cpu().long(), col_i) and torch.equal(nxt.metadata["coords"].cpu().long(), evs_i)
    # one stream given, the other drawn
    _, batch = comp.compose(step=9, indices=(None, evs_i))
    assert np.array_equal(batch["col_batch"]["indices"].cpu().numpy(), comp.indices_host(9)[0])
    assert torch.equal(batch["evs_batch"]["indices"].cpu().long(), evs_i)


# ---------------------------------------------------------------------------------------------------- 6. the composed step
def _same(a, b, what):
    a, b = a.detach().cpu(), b.detach().cpu()
    assert a.numel() == b.numel(), (what, a.shape, b.shape)
    assert torch.equal(a.reshape(-1).to(b.dtype), b.reshape(-1)), what


@pytest.mark.parametrize("pairing,deblur,distort,masks", [("consec", False, False, False), ("prevnext", False, True, True),
                                                          ("consec", True, False, True), ("consec", False, True, False)])
def test_composed_step_equals_the_host_composition(tmp_path, pairing, deblur, distort, masks):
    from lsenerf_amd.data import BatchComposer, spline_tables
    col_ds, evs_ds, scene = _scene(tmp_path, distort=distort, masks=masks, prevnext=pairing == "prevnext")
    n_col, n_evs = 150, 90
    comp = BatchComposer(scene, n_col, n_evs, deblur=deblur, seed=1, event_pairing=pairing, num_embd=NUM_EMBD)
    col_i, evs_i = _indices(n_col, n_evs, 10)
    if pairing == "prevnext":
        assert comp.pose_tables[2] is not None
    else:
        assert comp.pose_tables[2] is None
    spl = None
    if deblur:
        spl = _spline(col_ds.cameras)
        comp.set_poses(col=spline_tables(spl, col_ds.cameras, "deblur").detach().cuda())
    (col, prev, nxt), batch = comp.compose(indices=(col_i, evs_i))
    (h_col, h_prev, h_nxt), h_batch = host_compose(col_ds, evs_ds, col_i, evs_i, pairing, spl, NUM_EMBD, torch.tensor(COL_TIMES))
    G = 4 if deblur else 1
    assert len(col) == n_col * G and len(prev) == len(nxt) == n_evs
    # -- batch: bit-equal
    for key, b, hb in (("col_batch", batch["col_batch"], h_batch["col_batch"]), ("evs_batch", batch["evs_batch"], h_batch["evs_batch"])):
        for k in ("image", "appearance_id", "indices"):
            _same(b[k], hb[k], (key, k))
        assert ("msk" in b) == masks
        if masks:
            _same(b["msk"], hb["msk"], (key, "msk"))
            assert 0.0 < float(b["msk"].mean()) < 1.0
    e = batch["evs_batch"]["e_thresh"]
    assert e.is_cuda and e.shape == (n_evs, 1) and bool((e.cpu() == evs_ds.e_thresh).all())
    # -- rays and metadata
    slots = {"col": (col_i[:, :1] * G + torch.arange(G)[None]).reshape(-1), "prev": evs_i[:, 0],
             "nxt": evs_i[:, 0] + (1 if pairing == "consec" else 0)}
    errs = {}
    for name, rb, hb, table in (("col", col, h_col, comp.pose_tables[0]), ("prev", prev, h_prev, comp.pose_tables[1]),
                                ("nxt", nxt, h_nxt, comp.pose_tables[2] if pairing == "prevnext" else comp.pose_tables[1])):
        for k in ("appearance_id", "cam_type", "coords"):
            _same(rb.metadata[k], hb.metadata[k], (name, k))
        _same(rb.times, hb.times, (name, "times"))
        _same(rb.camera_indices, hb.camera_indices, (name, "camera_indices"))
        assert torch.equal(rb.origins, table.reshape(-1, 3, 4)[slots[name].cuda(), :, 3]), (name, "origins")
        errs[name] = {"origins": nmax_err(rb.origins, hb.origins), "directions": nmax_err(rb.directions, hb.directions),
                      "pixel_area": nmax_err(rb.pixel_area, hb.pixel_area),
                      "directions_norm": nmax_err(rb.metadata["directions_norm"], hb.metadata["directions_norm"])}
    print(pairing, deblur, distort, errs)
    for name, d in errs.items():
        for k, v in d.items():
            assert v < TOL_FWD, (name, k, v)
    # what the fixed rows were chosen for
    if deblur:
        app = col.metadata["appearance_id"].cpu().reshape(-1, 4)
        assert app[0].tolist() == [0, 0, 0, 1] and app[1].tolist() == [5, 6, 7, 7]      # ids 0 and 7: both clip ends
    ci = prev.camera_indices.cpu().reshape(-1)
    assert ci[:2].tolist() == [0, 1] and int(nxt.camera_indices[2]) == 5                  # before the first / a tie / past the last
    assert int(col.metadata["cam_type"].max()) == 0 and int(prev.metadata["cam_type"].min()) == 1


# ---------------------------------------------------------------------------------------------------- 7. the backward kernel
@pytest.mark.parametrize("pairing,deblur,distort", [("consec", False, True), ("prevnext", True, False)])
def test_pose_table_gradients_equal_float64_autograd(tmp_path, pairing, deblur, distort):
    from lsenerf_amd.data import BatchComposer, spline_tables
    col_ds, evs_ds, scene = _scene(tmp_path, distort=distort, prevnext=pairing == "prevnext")
    n_col, n_evs = 150, 90
    comp = BatchComposer(scene, n_col, n_evs, deblur=deblur, seed=1, event_pairing=pairing, num_embd=NUM_EMBD)
    col_i, evs_i = _indices(n_col, n_evs, 20)
    col_i[col_i[:, 0] == 3, 0] = 2                      # colour camera 3 and event camera 6 (and 7, consecutive) see no ray
    evs_i[evs_i[:, 0] == 6, 0] = 4
    if pairing == "consec":
        evs_i[evs_i[:, 0] == 5, 0] = 4
    G = 4 if deblur else 1
    if deblur:
        comp.set_poses(col=spline_tables(_spline(col_ds.cameras), col_ds.cameras, "deblur").detach().cuda())
    comp.compose(indices=(col_i, evs_i))
    g = torch.Generator().manual_seed(5)
    d_o, d_d = torch.randn(comp.n_rays, 3, generator=g), torch.randn(comp.n_rays, 3, generator=g)
    got = [None if t is None else t.clone() for t in comp.pose_grads((d_o.cuda(), d_d.cuda()))]
    again = comp.pose_grads((d_o.cuda(), d_d.cuda()))
    for a, b in zip(got, again):
        assert (a is None and b is None) or torch.equal(a, b)          # fixed-order sums
    # float64 autograd through EdCameras.generate_rays with get_c2w_fn = table[slot]
    tabs = [None if t is None else t.detach().cpu().double().requires_grad_(True) for t in comp.pose_tables]
    ecams = (evs_ds.cameras, evs_ds.cameras) if pairing == "consec" else (evs_ds.out.prev_cameras, evs_ds.out.next_cameras)
    plan = [(col_ds.cameras, tabs[0], (col_i[:, :1] * G + torch.arange(G)[None]).reshape(-1), col_i, G),
            (ecams[0], tabs[1], evs_i[:, 0], evs_i, 1),
            (ecams[1], tabs[1] if pairing == "consec" else tabs[2], evs_i[:, 0] + (1 if pairing == "consec" else 0), evs_i, 1)]
    loss, lo = 0.0, 0
    for cams, table, slot, idx, rep in plan:
        old = cams.get_c2w_fn
        cams.get_c2w_fn = lambda ci, table=table, slot=slot: table.reshape(-1, 3, 4)[slot]
        rb = cams.generate_rays(idx[:, :1].repeat_interleave(rep, 0), idx[:, 1:].float().repeat_interleave(rep, 0))
        cams.get_c2w_fn = old
        hi = lo + len(rb)
        loss = loss + (rb.origins * d_o[lo:hi].double()).sum() + (rb.directions * d_d[lo:hi].double()).sum()
        lo = hi
    assert lo == comp.n_rays
    loss.backward()
    for name, a, t in zip(("col", "prev", "nxt"), got, tabs):
        if t is None:
            assert a is None
            continue
        err = nmax_err(a, t.grad, 1e-12)
        print(name, "d pose table", err)
        assert err < TOL_GRAD, (name, err)
        untouched = t.grad.reshape(-1, 12).abs().amax(1) == 0
        assert bool(untouched.any()) and float(a.reshape(-1, 12)[untouched.cuda()].abs().max()) == 0.0, name
    # the eager autograd route (compose(tables=...)) ends in the same kernel
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in comp.pose_tables]
    (col, prev, nxt), _ = comp.compose(indices=(col_i, evs_i), tables=leaves)
    o, d = torch.cat([col.origins, prev.origins, nxt.origins]), torch.cat([col.directions, prev.directions, nxt.directions])
    ((o * d_o.cuda()).sum() + (d * d_d.cuda()).sum()).backward()
    for a, leaf in zip(got, leaves):
        assert (a is None and leaf is None) or torch.equal(a, leaf.grad)


# ---------------------------------------------------------------------------------------------------- models for 8 - 10
def _models(n=2, **cfg_kw):
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd.optim import FlatAdam, FlatParams
    torch.manual_seed(96)
    kw = dict(grid_levels=2, grid_resolution=32, log2_hashmap_size=15, use_mapping=True, mapping_method="identity", map_mode="co_map",
              evs_mapping_method="powpow")
    kw.update(cfg_kw)
    base = LSENeRFModel(LSENeRFModelConfig(**kw), torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), NUM_EMBD)
    with torch.no_grad():
        base.field.mlp_base_grid.params.mul_(300.0)
    models, opts = [], []
    for _ in range(n):
        m = copy.deepcopy(base).cuda().train()
        m.occupancy_grid.binaries.copy_(random_binaries(2, 32, 0.5, 3).cuda())
        m.occupancy_grid.occs.copy_(m.occupancy_grid.binaries.flatten().float() * 0.5)
        models.append(m)
        opts.append(FlatAdam(FlatParams(m.get_param_groups()["fields"]), lr=1e-2, eps=1e-15, lr_final=1e-4, max_steps=50))
    return models, opts


def _to_cuda(bundles, batch):
    from lsenerf_amd import RayBundle
    mv = lambda t: t.cuda() if torch.is_tensor(t) else t
    bs = [None if b is None else RayBundle(origins=mv(b.origins), directions=mv(b.directions), pixel_area=mv(b.pixel_area),
                                           camera_indices=mv(b.camera_indices), times=mv(b.times),
                                           metadata={k: mv(v) for k, v in b.metadata.items()}) for b in bundles]
    return bs, {k: (None if v is None else {kk: mv(vv) for kk, vv in v.items()}) for k, v in batch.items()}


# ---------------------------------------------------------------------------------------------------- 8. end to end, eager
def test_eager_step_on_a_composed_batch_equals_the_step_on_the_host_built_batch(tmp_path):
    """The host-built batch carries the composer's origins / directions / pixel_area (the comparison isolates the plumbing from ray
    rounding).  Losses: the forward has no atomics, so they are held to the host-built side's own run-to-run difference (zero:
    bit-equal).  Flat gradient: bit-equal when the host-built side reproduces itself run to run; otherwise by the rule of
    tests/test_gpu_dp.py, max|g - g_ref| <= max(6e-6 max|g_ref|, 4 x the spread of two host-built runs).  The fixed term is that
    test's: the hash backward sums with float atomics, the maximum over all elements of such a difference is not bounded by ONE
    run-to-run sample of itself (two GPU runs of this test measured a spread of 1.2e-7 and of 1.5e-8 for the same composed-vs-host
    difference of 1.2e-7, one ulp of the largest element), and a plumbing error (a wrong target, id or ray) is off by O(1)."""
    from lsenerf_amd.data import BatchComposer
    col_ds, evs_ds, scene = _scene(tmp_path, masks=True)
    n_col, n_evs = 200, 50
    comp = BatchComposer(scene, n_col, n_evs, seed=3, num_embd=NUM_EMBD)
    col_i, evs_i = _indices(n_col, n_evs, 30)
    (m,), (opt,) = _models(1)
    jit = torch.rand(comp.n_rays, generator=torch.Generator().manual_seed(2)).cuda()

    def run(bundles, batch):
        opt.zero_grad()
        _, losses, _ = m.train_step_bundles(*bundles, batch, jitter=jit)
        sum(losses.values()).backward()
        return {k: float(v) for k, v in losses.items()}, opt.flat.grad.clone()
    bundles, batch = comp.compose(indices=(col_i, evs_i))
    l_dev, g_dev = run(bundles, batch)
    h_bundles, h_batch = _to_cuda(*host_compose(col_ds, evs_ds, col_i, evs_i, "consec", None, NUM_EMBD, torch.tensor(COL_TIMES)))
    for hb, rb in zip(h_bundles, bundles):
        hb.origins, hb.directions, hb.pixel_area = rb.origins.clone(), rb.directions.clone(), rb.pixel_area.clone()
    l_h1, g_h1 = run(h_bundles, h_batch)
    l_h2, g_h2 = run(h_bundles, h_batch)
    assert set(l_dev) == set(l_h1) == {"rgb_loss", "event_loss"} and all(np.isfinite(v) and v > 0 for v in l_dev.values())
    assert float(g_h1.abs().max()) > 0
    spread = float((g_h1 - g_h2).abs().max())
    diff = float((g_dev - g_h1).abs().max())
    print("losses", l_dev, l_h1, "gradient: max", float(g_h1.abs().max()), "run-to-run spread", spread, "composed vs host-built", diff)
    for k in l_h1:
        assert abs(l_dev[k] - l_h1[k]) <= 4 * abs(l_h1[k] - l_h2[k]), (k, l_dev[k], l_h1[k], l_h2[k])
    if spread == 0.0:
        assert diff == 0.0, diff
    else:
        assert diff <= max(6e-6 * float(g_h1.abs().max()), 4 * spread), (diff, spread, float(g_h1.abs().max()))


# ---------------------------------------------------------------------------------------------------- 9. graphed
@pytest.mark.parametrize("event_loss_type", ["log_loss", "enerf_norm_loss"])
def test_graphed_step_with_a_composer_equals_eager_steps_on_composed_batches(tmp_path, event_loss_type):
    """(enerf_norm_loss: the per-ray device ``e_thresh`` of the composed batch lets the capture succeed.)"""
    from lsenerf_amd import ops
    from lsenerf_amd.data import BatchComposer
    from lsenerf_amd.graph import GraphedTrainStep
    _, _, scene = _scene(tmp_path)
    n_col, n_evs, k0 = 200, 50, 5
    c_e, c_g = (BatchComposer(scene, n_col, n_evs, seed=11, num_embd=NUM_EMBD) for _ in range(2))
    (m_e, m_g), (o_e, o_g) = _models(2, event_loss_type=event_loss_type)
    assert m_g._epilogue_desc() is not None
    c_g.step_dev.fill_(k0)
    with pytest.raises(ValueError, match="prefetch_march"):
        GraphedTrainStep(m_g, o_g, composer=c_g, prefetch_march=True)
    step = GraphedTrainStep(m_g, o_g, composer=c_g, jitter="input")
    assert int(c_g.step_dev) == k0 and o_g.step_count == 0 and torch.equal(o_g.flat.data, o_e.flat.data)   # building trains and draws nothing
    spans = [(o, o + p.numel()) for p, o in zip(o_e.flat.params, o_e.flat.offsets)]
    g = torch.Generator().manual_seed(7)
    ops.SYNC_STATS.update(seconds=0.0, count=0)
    for it in range(4):
        jit = torch.rand(c_g.n_rays, generator=g).cuda()
        sync_before = ops.SYNC_STATS["count"]
        l_g = step(jitter=jit)
        assert ops.SYNC_STATS["count"] == sync_before
        l_g = {k: float(v) for k, v in l_g.items()}
        g_g = o_g.flat.grad.clone()
        want_col, want_evs = c_g.indices_host(k0 + it)                 # replay `it` drew what an eager call with step k0 + it draws
        assert np.array_equal(step.col.metadata["coords"].cpu().numpy(), want_col)
        assert np.array_equal(step.prev.metadata["coords"].cpu().numpy(), want_evs)
        assert np.array_equal(step.nxt.metadata["coords"].cpu().numpy(), want_evs)
        bundles, batch = c_e.compose(step=k0 + it)
        o_e.zero_grad()
        _, losses, _ = m_e.train_step_bundles(*bundles, batch, jitter=jit)
        sum(losses.values()).backward()
        g_e = o_e.flat.grad.clone()
        o_e.step()
        l_e = {k: float(v) for k, v in losses.items()}
        assert set(l_g) == set(l_e) == {"rgb_loss", "event_loss"}
        for k in l_e:
            assert abs(l_g[k] - l_e[k]) <= 2e-5 * max(1.0, abs(l_e[k])), (it, k, l_g[k], l_e[k])
        if it == 0:
            for a, b in spans:
                assert nmax_err(g_g[a:b], g_e[a:b], 1e-12) < 3e-5, (a, b)
        assert o_g.step_count == o_e.step_count == it + 1
    assert int(c_g.step_dev) == k0 + 4 and int(c_e.step_dev) == 0
    step.check_overflow()
    d = (o_g.flat.data - o_e.flat.data).abs()
    assert float((d > 1e-5 * float(o_e.flat.data.abs().max())).float().mean()) < 0.02
    with pytest.raises(ValueError, match="composer"):
        step(*c_e.bundles, c_e.batch)
    step.close()


# ---------------------------------------------------------------------------------------------------- 10. poses through the graph
def test_pose_gradients_of_a_graphed_composer_step_equal_the_ray_gradient_route(tmp_path):
    """Config-4 style (deblur, spline tables, ray_grads=True): ``step.pose_grads`` back-propagated into the spline's control
    tangents against the existing route (generate_deblur_rays -> graphed step -> backward from ``step.ray_grads``) for the same
    pixels and jitter."""
    from lsenerf_amd import cameras as cam
    from lsenerf_amd.data import BatchComposer, DeviceScene, spline_tables
    from lsenerf_amd.graph import GraphedTrainStep
    col_ds, _ = make_scene(tmp_path)
    scene = DeviceScene.from_datasets(col_ds, None, "cuda")
    n_px, k0 = 48, 2
    comp = BatchComposer(scene, n_px, 0, deblur=True, seed=21, num_embd=NUM_EMBD)
    idx = torch.from_numpy(comp.indices_host(k0)[0])
    jit = torch.rand(n_px * 4, generator=torch.Generator().manual_seed(1)).cuda()
    models, opts = _models(2, rgb_loss_type="deblur", use_mapping=False)
    results = []
    for route, m, opt in zip(("rays", "composer"), models, opts):
        cams = copy.deepcopy(col_ds.cameras)
        spl = _spline(cams).to("cuda")
        spl.device = "cuda"
        cams.times = cams.times.cuda()
        if route == "rays":
            rb = cam.generate_deblur_rays(cams, spl, idx[:, 0].cuda(), idx[:, 1:].float().cuda())
            app = torch.tensor(COL_APP)[idx[:, 0]][:, None] + (torch.arange(4) - 2)[None]
            rb.metadata["appearance_id"] = app.clip(0, NUM_EMBD - 1).reshape(-1, 1).cuda()
            batch = {"col_batch": {"image": host_batch(col_ds, idx, False)["image"].cuda()}, "evs_batch": None}
            step = GraphedTrainStep(m, opt, rb, None, None, batch, ray_grads=True, jitter="input")
            loss = float(step(rb, None, None, batch, jitter=jit)["rgb_loss"])
            torch.autograd.backward([rb.origins, rb.directions], list(step.ray_grads["col"]))
        else:
            tables = spline_tables(spl, cams, "deblur")
            comp.set_poses(col=tables.detach())
            comp.step_dev.fill_(k0)
            step = GraphedTrainStep(m, opt, composer=comp, ray_grads=True, jitter="input")
            loss = float(step(jitter=jit)["rgb_loss"])
            assert np.array_equal(comp.batch["col_batch"]["indices"].cpu().numpy(), idx.numpy()) and int(comp.step_dev) == k0 + 1
            assert step.pose_grads["prev"] is None and step.pose_grads["next"] is None
            torch.autograd.backward([tables], [step.pose_grads["col"]])
        pose = spl.ctrl_tangents.grad.clone()
        assert float(pose.abs().max()) > 0
        results.append((loss, pose, opt.flat.grad.clone()))
        step.close()
    (l0, p0, t0), (l1, p1, t1) = results
    print("loss", l0, l1, "d ctrl_tangents", nmax_err(p1, p0, 1e-12), "d table", nmax_err(t1, t0, 1e-12))
    assert abs(l0 - l1) <= 2e-5 * max(1.0, abs(l0))
    assert nmax_err(t1, t0, 1e-12) < TOL_GRAD
    assert nmax_err(p1, p0, 1e-12) < TOL_GRAD
