"""The device pose deltas on the GPU (csrc/pose_delta.hip, lsenerf_amd.pose_delta_dev, BatchComposer.attach_camera_optimizers) and the
camera parameters' Adam inside the captured step (GraphedTrainStep(camera_opt=...)): both kernels against the float64 restatement
of tests/pose_delta_fixtures.py, the parameters read in place by a captured step, the attached route against the set_poses route,
and the in-graph camera update against an eager FlatAdam.step() on the same gradients."""
import numpy as np
import pytest
import torch

from tests import pose_delta_fixtures as F
from tests.spline_fixtures import make_spline
from tests.test_compose_cpu import N_COL, N_FRAMES
from tests.test_gpu_compose import NUM_EMBD, _models, _scene
from tests.util import TOL_GRAD, nmax_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

BAR_FWD = 1e-5          # max abs error of a pose entry: the bar tests/test_cameras_cpu.py holds this maths to
TINY = 1.1754943508222875e-38        # float32's smallest normal
FLOOR = 2.0 ** -22      # host-route / device-route bar of tests/test_gpu_adam_sizes.py, of the element's scale


def _bwd_bar(p, base, mode, masked, d_table):
    """``(float64 reference, baseline, bar)``: 4 x the nmax_err of cameras.py's own float32 CPU autograd against float64, floor 1e-6
    (the convention of test_gpu_spline_dev._bwd_bars); for SE3 the baseline is taken over the rows with |w| outside (0.01, 0.1)
    only, where float32 cameras.py does not cancel -- ALL rows are then held to that bar."""
    ref = F.autograd_f64(p, base, mode, masked, d_table)
    base32 = F.cameras_py(p, base, mode, masked, d_table, torch.float32)[1]
    rows = F.baseline_rows(p, mode)
    baseline = nmax_err(base32[rows], ref[rows])
    return ref, baseline, max(4.0 * baseline, 1e-6)


def _device_poses(mode, C):
    from lsenerf_amd.pose_delta_dev import DeltaPoses
    p, base, masked = F.make_params(C), F.make_base(C), F.masked_cameras(C)
    F.check_fixture(p)
    opt = F.make_optimizer(p, mode, masked, device="cuda")
    return p, base, masked, opt, DeltaPoses([(opt, base), None, None], [(C, 3, 4), None, None], "cuda")


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("mode,C", F.FIXTURES)
def test_pose_tables_equal_the_float64_tables(mode, C):
    p, base, masked, opt, poses = _device_poses(mode, C)
    table = torch.full((C, 3, 4), float("nan"), device="cuda")
    poses.forward([table, None, None])
    ref = F.tables_f64(p, base, mode, masked)
    err = float((table.cpu().double() - ref).abs().max())
    print(mode, C, "forward: max abs error", err)
    assert err < BAR_FWD, err                                     # (a row the kernel left out is NaN: fails here)
    if masked is not None:
        assert torch.equal(table[masked.cuda()].cpu(), base[masked])
    again = torch.zeros(C, 3, 4, device="cuda")
    poses.forward([again, None, None])
    assert torch.equal(again, table)


# ---------------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("mode,C", F.FIXTURES)
def test_parameter_gradients_equal_float64_autograd(mode, C):
    """Measured (MI355X): DESIGN.md section 9."""
    p, base, masked, opt, poses = _device_poses(mode, C)
    d = F.random_table_grad(C)
    ref, baseline, bar = _bwd_bar(p, base, mode, masked, d)
    g_dev = [d.cuda(), None, None]
    got = poses.backward(g_dev)["col"].clone()
    err = nmax_err(got, ref)
    print(mode, C, "backward: baseline", baseline, "kernel", err, "bar", bar)
    assert bool(torch.isfinite(got).all())
    assert err <= bar, (err, bar)
    zero_rows = p.abs().amax(1) == 0
    if masked is not None:
        zero_rows[masked] = False
    if bool(zero_rows.any()):                                     # the state training starts from: finite, and the reference's
        z = zero_rows.cuda()
        assert float(got[z].abs().max()) > 0
        assert float((got[z].cpu().double() - ref[zero_rows]).abs().max()) <= bar * float(ref.abs().max())
    assert torch.equal(poses.backward(g_dev)["col"], got)        # no atomics
    poses.grads["col"].fill_(float("nan"))                        # every element is written, masked cameras with exact zeros
    third = poses.backward(g_dev)["col"]
    assert torch.equal(third, got)
    if masked is not None:
        assert float(third[masked.cuda()].abs().max()) == 0.0
    # the eager autograd route ends in the same kernel
    tabs = poses.tables()
    assert tabs[0].requires_grad and tabs[1] is None and tabs[2] is None
    (tabs[0] * g_dev[0]).sum().backward()
    assert torch.equal(opt.pose_adjustment.grad, got)


# ---------------------------------------------------------------------------------------------------- 3. one block, two tables
@pytest.mark.parametrize("mode", F.MODES)
def test_a_shared_block_sums_the_rows_of_prev_and_next(mode):
    from lsenerf_amd.pose_delta_dev import DeltaPoses
    C = 65
    p, masked = F.make_params(C), F.masked_cameras(C)
    base_a, base_b = F.make_base(C, seed=1), F.make_base(C, seed=2)
    d_a, d_b = F.random_table_grad(C, seed=11), F.random_table_grad(C, seed=12)
    opt = F.make_optimizer(p, mode, masked, device="cuda")
    poses = DeltaPoses([None, (opt, base_a), (opt, base_b)], [None, (C, 3, 4), (C, 3, 4)], "cuda")
    assert poses.shared and list(poses.blocks) == ["prev"]
    tables = [None, torch.full((C, 3, 4), float("nan"), device="cuda"), torch.full((C, 3, 4), float("nan"), device="cuda")]
    poses.forward(tables)
    for t, b in ((tables[1], base_a), (tables[2], base_b)):
        assert float((t.cpu().double() - F.tables_f64(p, b, mode, masked)).abs().max()) < BAR_FWD
    ref = F.autograd_f64(p, base_a, mode, masked, d_a) + F.autograd_f64(p, base_b, mode, masked, d_b)
    base32 = F.cameras_py(p, base_a, mode, masked, d_a, torch.float32)[1] + F.cameras_py(p, base_b, mode, masked, d_b, torch.float32)[1]
    rows = F.baseline_rows(p, mode)
    baseline = nmax_err(base32[rows], ref[rows])
    bar = max(4.0 * baseline, 1e-6)
    got = poses.backward([None, d_a.cuda(), d_b.cuda()])
    assert list(got) == ["prev"]
    err = nmax_err(got["prev"], ref)
    print(mode, "shared block: baseline", baseline, "kernel", err, "bar", bar)
    assert err <= bar, (err, bar)
    assert float(got["prev"][masked.cuda()].abs().max()) == 0.0
    # equal base poses: the sum does not depend on which table brought which gradient
    same = DeltaPoses([None, (opt, base_a), (opt, base_a)], [None, (C, 3, 4), (C, 3, 4)], "cuda")
    ab = same.backward([None, d_a.cuda(), d_b.cuda()], static=False)["prev"]
    ba = same.backward([None, d_b.cuda(), d_a.cuda()], static=False)["prev"]
    assert torch.equal(ab, ba) and float(ab.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- 4. parameters in place
def _optimizers(prevnext, seed=5, evs_kind=None):
    """A colour ``CameraOptimizer`` (SE3, cameras 0 and 3 frozen) and the event side's optimiser on the GPU, away from zero."""
    from lsenerf_amd import cameras as cam
    g = torch.Generator().manual_seed(seed)
    col = cam.CameraOptimizer(cam.CameraOptimizerConfig(mode="SE3"), N_COL, device="cuda", non_trainable_camera_indices=torch.tensor([0, 3]))
    n_e = N_FRAMES if prevnext else N_FRAMES + 1
    kind = evs_kind or ("prevnext" if prevnext else "ns")
    evs = cam.CameraOptimizerConfig(mode="SO3xR3", optim_type=kind).setup(num_cameras=n_e, device="cuda")
    with torch.no_grad():
        for o in [col] + ([evs.prev_optim, evs.next_optim] if kind == "prevnext" else [evs]):
            o.pose_adjustment.copy_((torch.randn(o.pose_adjustment.shape, generator=g) * 0.02).cuda())
    return col, evs


def _blocks(deltas):
    """Per parameter block of an attached ``DeltaPoses``: (name, optimiser, segment indices it feeds)."""
    return [(name, deltas.optims[i], [i, 2] if (i == 1 and deltas.shared) else [i]) for name, i in deltas.blocks.items()]


def _check_against_float64(comp, step, tag):
    """The tables in the composer against float64, and ``step.camera_grads`` against float64 autograd fed ``step.pose_grads``."""
    deltas = comp.deltas
    keys = ("col", "prev", "next")
    for name, optim, segs in _blocks(deltas):
        p, masked = optim.pose_adjustment.detach().cpu(), optim.non_trainable_camera_indices
        mode = optim.config.mode
        ref, base32 = 0.0, 0.0
        for s in segs:
            base = deltas.base[s].cpu()
            err = float((comp.pose_tables[s].reshape(-1, 3, 4).cpu().double() - F.tables_f64(p, base, mode, masked)).abs().max())
            assert err < BAR_FWD, (tag, name, s, err)
            d = step.pose_grads[keys[s]].reshape(-1, 3, 4).cpu()
            assert float(d.abs().max()) > 0
            ref = ref + F.autograd_f64(p, base, mode, masked, d)
            base32 = base32 + F.cameras_py(p, base, mode, masked, d, torch.float32)[1]
        rows = F.baseline_rows(p, mode)
        baseline = nmax_err(base32[rows], ref[rows])
        bar = max(4.0 * baseline, 1e-6)
        err = nmax_err(step.camera_grads[name], ref)
        print(tag, name, "gradient: baseline", baseline, "kernel", err, "bar", bar)
        assert err <= bar, (tag, name, err, bar)
        if masked is not None:
            assert float(step.camera_grads[name][masked.cuda()].abs().max()) == 0.0


@pytest.mark.parametrize("prevnext", [True, False])
def test_a_captured_step_reads_the_pose_adjustments_in_place(tmp_path, prevnext):
    from lsenerf_amd.data import BatchComposer
    from lsenerf_amd.graph import GraphedTrainStep
    _, _, scene = _scene(tmp_path, prevnext=prevnext)
    comp = BatchComposer(scene, 48, 24, seed=21, event_pairing="prevnext" if prevnext else "consec", num_embd=NUM_EMBD)
    col, evs = _optimizers(prevnext)
    comp.attach_camera_optimizers(col=col, evs=evs)
    assert list(comp.deltas.blocks) == (["col", "prev", "nxt"] if prevnext else ["col", "prev"])
    (m,), (opt,) = _models(1)
    step = GraphedTrainStep(m, opt, composer=comp, ray_grads=True, jitter="input")
    g = torch.Generator().manual_seed(3)
    params = comp.deltas.parameters()
    for it in range(3):
        if it:                                                    # the camera optimiser's update: in place, between replays
            with torch.no_grad():
                for p in params:
                    p.add_((torch.randn(p.shape, generator=g) * 0.004).cuda())
        losses = step(jitter=torch.rand(comp.n_rays, generator=g).cuda())
        assert all(np.isfinite(float(v)) for v in losses.values())
        fresh = [None if t is None else torch.zeros_like(t) for t in comp.pose_tables]
        comp.deltas.forward(fresh)                                # an eager launch on the current parameters
        assert all(f is None or torch.equal(f, t) for f, t in zip(fresh, comp.pose_tables)), it
        assert set(step.camera_grads) == set(comp.deltas.blocks) and step.spline_grads is None
        _check_against_float64(comp, step, f"replay {it}")
        if it:
            assert not torch.equal(comp.pose_tables[1], before)
        before = comp.pose_tables[1].clone()
    step.close()


# ---------------------------------------------------------------------------------------------------- 5. against set_poses
def test_the_attached_route_equals_the_set_poses_route(tmp_path):
    """The optimisers attached against ``set_poses`` in front of the replay fed clones of the kernel's own tables: same model seed,
    draw and jitter.  Bars of test_the_captured_spline_route_equals_the_set_poses_route."""
    from lsenerf_amd.data import BatchComposer, camera_tables
    from lsenerf_amd.graph import GraphedTrainStep
    k0 = 2
    models, opts = _models(2)
    col_ds, evs_ds, scene = _scene(tmp_path)
    comp_c, comp_b = (BatchComposer(scene, 48, 24, seed=21, num_embd=NUM_EMBD) for _ in range(2))
    jit = torch.rand(comp_c.n_rays, generator=torch.Generator().manual_seed(1)).cuda()
    # attached
    col_c, evs_c = _optimizers(False)
    comp_c.attach_camera_optimizers(col=col_c, evs=evs_c)
    comp_c.step_dev.fill_(k0)
    step_c = GraphedTrainStep(models[0], opts[0], composer=comp_c, ray_grads=True, jitter="input")
    loss_c = {k: float(v) for k, v in step_c(jitter=jit).items()}
    grad_c = opts[0].flat.grad.clone()
    tables_c = [None if t is None else t.clone() for t in comp_c.pose_tables]
    assert int(comp_c.step_dev) == k0 + 1
    # set_poses
    col_b, evs_b = _optimizers(False)
    assert torch.equal(col_b.pose_adjustment, col_c.pose_adjustment)
    comp_b.step_dev.fill_(k0)
    step_b = GraphedTrainStep(models[1], opts[1], composer=comp_b, ray_grads=True, jitter="input")
    comp_b.set_poses(col=tables_c[0].clone(), prev=tables_c[1].clone())
    loss_b = {k: float(v) for k, v in step_b(jitter=jit).items()}
    grad_b = opts[1].flat.grad.clone()
    assert torch.equal(comp_b.batch["col_batch"]["indices"], comp_c.batch["col_batch"]["indices"])
    tabs = [camera_tables(col_ds.cameras, col_b), camera_tables(evs_ds.cameras, evs_b)]
    torch.autograd.backward(tabs, [step_b.pose_grads["col"].reshape(-1, 3, 4), step_b.pose_grads["prev"]])
    errs = {"flat grad": nmax_err(grad_c, grad_b, 1e-12),
            "d col": nmax_err(step_c.camera_grads["col"], col_b.pose_adjustment.grad, 1e-12),
            "d evs": nmax_err(step_c.camera_grads["prev"], evs_b.pose_adjustment.grad, 1e-12)}
    print("losses attached", loss_c, "set_poses", loss_b, errs)
    assert set(loss_c) == set(loss_b) == {"rgb_loss", "event_loss"}
    for k in loss_b:
        assert abs(loss_c[k] - loss_b[k]) <= 2e-5 * max(1.0, abs(loss_b[k])), (k, loss_c[k], loss_b[k])
    assert float(col_b.pose_adjustment.grad.abs().max()) > 0 and float(evs_b.pose_adjustment.grad.abs().max()) > 0
    for k, v in errs.items():
        assert v < TOL_GRAD, (k, v)
    step_b.close()
    step_c.close()


# ---------------------------------------------------------------------------------------------------- 6. the camera Adam
CAM_ADAM = dict(lr=1e-3, eps=1e-15, lr_final=1e-4, max_steps=8)      # the reference's camera_opt group, its decay ending inside the test


def _setup_camera_adam(tmp_path, kind):
    """``(composer, model, opt, camera_opt, masked flat positions)``: FlatParams first, then attach."""
    from lsenerf_amd.data import BatchComposer
    from lsenerf_amd.optim import FlatAdam, FlatParams
    col_ds, _, scene = _scene(tmp_path)
    if kind in ("spline", "mixed"):
        comp = BatchComposer(scene, 48, 24, deblur=True, seed=21, num_embd=NUM_EMBD)
        spl = make_spline(col_ds.cameras, factor=3).to("cuda")
        spl.device = "cuda"
        if kind == "spline":
            flat = FlatParams([spl.ctrl_tangents, spl.scale])
            comp.attach_spline(spl)
        else:               # what the reference builds when only col_cam_optimizer is a spline
            _, evs = _optimizers(False)
            flat = FlatParams([spl.ctrl_tangents, spl.scale, evs.pose_adjustment])
            comp.attach_spline(spl, tables=("col",))
            comp.attach_camera_optimizers(evs=evs)
        frozen = torch.zeros(flat.numel, dtype=torch.bool)
        (m,), (opt,) = _models(1, rgb_loss_type="deblur")
    else:
        comp = BatchComposer(scene, 48, 24, seed=21, num_embd=NUM_EMBD)
        col, evs = _optimizers(False)
        flat = FlatParams([col.pose_adjustment, evs.pose_adjustment])
        comp.attach_camera_optimizers(col=col, evs=evs)
        frozen = torch.zeros(flat.numel, dtype=torch.bool)
        for c in (0, 3):
            frozen[flat.offsets[0] + 6 * c:flat.offsets[0] + 6 * c + 6] = True
        (m,), (opt,) = _models(1)
    return comp, m, opt, FlatAdam(flat, **CAM_ADAM), frozen


def _fresh_tables(comp):
    fresh = [None if t is None else torch.zeros_like(t) for t in comp.pose_tables]
    if comp.spline is not None:
        comp.spline.forward(fresh)
    if comp.deltas is not None:
        comp.deltas.forward(fresh)
    return fresh


@pytest.mark.parametrize("kind", ["spline", "deltas", "mixed"])
def test_the_camera_adam_inside_the_graph_equals_an_eager_step_on_the_same_gradients(tmp_path, kind):
    from lsenerf_amd.graph import GraphedTrainStep
    from lsenerf_amd.optim import FlatAdam, FlatParams
    comp, m, opt, cam_opt, frozen = _setup_camera_adam(tmp_path, kind)
    flat = cam_opt.flat
    live = torch.zeros(flat.numel, dtype=torch.bool)
    for p, o in zip(flat.params, flat.offsets):
        live[o:o + p.numel()] = True
    assert int((~live).sum()) > 0
    state = lambda: (flat.data.clone(), cam_opt.exp_avg.clone(), cam_opt.exp_avg_sq.clone())
    before, field_before = state(), opt.flat.data.clone()
    p_start = flat.data.clone()
    step = GraphedTrainStep(m, opt, composer=comp, ray_grads=True, jitter="input", camera_opt=cam_opt)
    # building trains nothing
    assert all(torch.equal(a, b) for a, b in zip(before, state())) and cam_opt.step_count == 0 and opt.step_count == 0
    assert torch.equal(field_before, opt.flat.data) and int(comp.step_dev) == 0
    # the gradients are written straight into the views of the flat gradient
    for p in flat.params:
        assert any(g.data_ptr() == p.grad.data_ptr() for g in step.camera_grads.values())
    assert len(step.camera_grads) == len(flat.params)
    if kind != "deltas":
        assert step.spline_grads["ctrl_tangents"].data_ptr() == flat.grad.data_ptr()
    # the eager twin: same layout, same hyper-parameters and schedule, the host-scalar route
    twin_flat = FlatParams([torch.nn.Parameter(torch.zeros_like(p)) for p in flat.params])
    assert twin_flat.offsets == flat.offsets and twin_flat.numel == flat.numel
    twin = FlatAdam(twin_flat, **CAM_ADAM)
    g = torch.Generator().manual_seed(3)
    expected_tables, count = None, 0
    for it in range(5):
        if it == 3:                                               # a step count set from outside: the device clock follows it,
            cam_opt.step_count = count = 7                        # across the end of the decay (max_steps = 8)
        pre = state()
        step(jitter=torch.rand(comp.n_rays, generator=g).cuda())
        count += 1
        assert cam_opt.step_count == count and int(cam_opt._step_dev.item()) == count
        assert opt.step_count == it + 1
        if expected_tables is not None:                           # this replay's tables: those of the parameters the last one left
            assert all(e is None or torch.equal(e, t) for e, t in zip(expected_tables, comp.pose_tables)), it
        grads = flat.grad.clone()
        assert float(grads.abs().max()) > 0 and int((grads[(~live).cuda()] != 0).sum()) == 0
        with torch.no_grad():
            twin_flat.data.copy_(pre[0]); twin.exp_avg.copy_(pre[1]); twin.exp_avg_sq.copy_(pre[2]); twin_flat.grad.copy_(grads)
        twin.step_count = count - 1
        lr = twin.current_lr()
        twin.step()
        assert (abs(lr - 1e-4) <= 1e-15) == (count - 1 >= 8) and twin.step_count == count
        cpu = lambda t: t.detach().double().cpu()
        dp = (cpu(twin_flat.data) - cpu(pre[0])).abs()
        scales = (cpu(pre[0]).abs() + dp, 0.9 * cpu(pre[1]).abs() + 0.1 * cpu(grads).abs(), cpu(twin.exp_avg_sq))
        ratios = []
        for k, (a, b, s) in enumerate(zip(state(), (twin_flat.data, twin.exp_avg, twin.exp_avg_sq), scales)):
            ok = (s >= TINY) | (s == 0) if k == 2 else torch.ones_like(s, dtype=torch.bool)
            ratios.append(float(((cpu(a) - cpu(b)).abs()[ok] / s[ok].clamp_min(TINY)).max()))
        print(kind, "replay", it, "step count", count, "lr", lr, "device / host (p, exp_avg, exp_avg_sq) of the scale:", ratios)
        assert float(dp.max()) > 0
        assert max(ratios) <= FLOOR, (it, ratios)
        now = state()
        for t in now:                                             # the padding never moves; neither does a frozen camera
            assert int((t[(~live).cuda()] != 0).sum()) == 0
        assert torch.equal(now[0][frozen.cuda()], p_start[frozen.cuda()])
        if bool(frozen.any()):
            assert float(now[1][frozen.cuda()].abs().max()) == 0.0 and float(now[2][frozen.cuda()].abs().max()) == 0.0
        expected_tables = _fresh_tables(comp)
    step.close()


# ---------------------------------------------------------------------------------------------------- 7. refusals
def test_camera_opt_is_refused_where_it_cannot_work(tmp_path):
    from lsenerf_amd.data import BatchComposer
    from lsenerf_amd.graph import GraphedTrainStep
    from lsenerf_amd.optim import FlatAdam, FlatParams
    col_ds, _, scene = _scene(tmp_path)
    (m,), (opt,) = _models(1)
    deferred = (m.deferred_counts, m.deferred_max_slots)
    col, evs = _optimizers(False)
    cam_opt = FlatAdam(FlatParams([col.pose_adjustment, evs.pose_adjustment]), **CAM_ADAM)
    comp = BatchComposer(scene, 48, 24, seed=21, num_embd=NUM_EMBD)
    with pytest.raises(ValueError, match="camera_opt= belongs to a step built with composer="):
        GraphedTrainStep(m, opt, camera_opt=cam_opt)
    with pytest.raises(ValueError, match="nothing attached"):
        GraphedTrainStep(m, opt, composer=comp, ray_grads=True, camera_opt=cam_opt)
    comp.attach_camera_optimizers(col=col, evs=evs)
    with pytest.raises(ValueError, match="needs ray_grads=True"):
        GraphedTrainStep(m, opt, composer=comp, camera_opt=cam_opt)
    # not exactly the attached parameters: one missing, one foreign
    col2, evs2 = _optimizers(False)
    part = FlatAdam(FlatParams([col2.pose_adjustment]), **CAM_ADAM)
    comp2 = BatchComposer(scene, 48, 24, seed=21, num_embd=NUM_EMBD)
    comp2.attach_camera_optimizers(col=col2, evs=evs2)
    with pytest.raises(ValueError, match="exactly the parameters attached"):
        GraphedTrainStep(m, opt, composer=comp2, ray_grads=True, camera_opt=part)
    with pytest.raises(ValueError, match="exactly the parameters attached"):
        GraphedTrainStep(m, opt, composer=comp2, ray_grads=True, camera_opt=cam_opt)
    # attached first, flattened afterwards: the kernels would read where the parameters no longer are
    col3, evs3 = _optimizers(False)
    comp3 = BatchComposer(scene, 48, 24, seed=21, num_embd=NUM_EMBD)
    comp3.attach_camera_optimizers(col=col3, evs=evs3)
    late = FlatAdam(FlatParams([col3.pose_adjustment, evs3.pose_adjustment]), **CAM_ADAM)
    with pytest.raises(ValueError, match="have moved since attach_camera_optimizers"):
        GraphedTrainStep(m, opt, composer=comp3, ray_grads=True, camera_opt=late)
    with pytest.raises(ValueError, match="have moved since attach_camera_optimizers"):
        comp3.compose()
    comp_s = BatchComposer(scene, 48, 24, deblur=True, seed=21, num_embd=NUM_EMBD)
    spl = make_spline(col_ds.cameras, factor=3).to("cuda")
    spl.device = "cuda"
    comp_s.attach_spline(spl)
    late_s = FlatAdam(FlatParams([spl.ctrl_tangents, spl.scale]), **CAM_ADAM)
    with pytest.raises(ValueError, match="have moved since attach_spline"):
        GraphedTrainStep(m, opt, composer=comp_s, ray_grads=True, camera_opt=late_s)
    assert (m.deferred_counts, m.deferred_max_slots) == deferred and opt.step_count == 0      # every refusal came before anything changed
