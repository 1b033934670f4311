"""The device spline poses on the GPU (csrc/spline.hip, lsenerf_amd.spline_dev, BatchComposer.attach_spline): both kernels against
the float64 restatement of cameras.py over the fixtures of tests/spline_fixtures.py, the parameters read in place by a captured
step, and the captured route against the existing set_poses route."""
import copy

import numpy as np
import pytest
import torch

from tests.test_compose_cpu import COL_TIMES, EVS_TIMES
from tests.test_gpu_compose import NUM_EMBD, _models, _scene
from tests.spline_fixtures import (FIXTURES, autograd_f32, autograd_f64, check_fixture, double_copy, make_spline, random_table_grads,
                                       tables_f64)
from tests.util import TOL_GRAD, nmax_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

BAR_FWD = 1e-5          # max abs error of a pose entry: the bar tests/test_cameras_cpu.py holds this maths to


def _device_poses(name):
    from lsenerf_amd.spline_dev import SplinePoses
    spl, segments, shapes = FIXTURES[name]()
    check_fixture(spl)
    dev = copy.deepcopy(spl).to("cuda")
    return spl, dev, segments, shapes, SplinePoses(dev, segments, shapes, "cuda")


def _fwd_err(tables, spl, segments):
    """max abs error of the fed tables against the float64 tables of the (float32) parameters of ``spl``."""
    ref = tables_f64(double_copy(spl), segments)
    return max(float((t.detach().cpu().double() - r.detach().reshape(t.shape)).abs().max()) for t, r in zip(tables, ref) if r is not None)


def _bwd_bars(spl, segments, d_tables):
    """``(reference (d ctrl, d scale), bars (ctrl, scale))``: the bar is 4 x the error of cameras.py's own float32 CPU autograd against
    float64 on the same fixture (nmax_err), floor 1e-6 -- the factor covers the device's sin / cos / acos being a few ulp where the
    CPU's are about one, and another summation order over at most a few hundred terms."""
    ref = autograd_f64(spl, segments, d_tables)
    base = autograd_f32(spl, segments, d_tables)
    baseline = [nmax_err(b, r) for b, r in zip(base, ref)]
    return ref, baseline, [max(4.0 * b, 1e-6) for b in baseline]


# ---------------------------------------------------------------------------------------------------- 1. forward
@pytest.mark.parametrize("name", list(FIXTURES))
def test_pose_tables_equal_the_float64_tables(name):
    spl, dev, segments, shapes, poses = _device_poses(name)
    tables = [None if s is None else torch.full(s, float("nan"), device="cuda") for s in shapes]
    poses.forward(tables)
    err = _fwd_err(tables, spl, segments)
    print(name, "forward: max abs error", err)
    assert err < BAR_FWD, err                                     # (a row the kernel left out is NaN: fails here)
    again = [None if s is None else torch.zeros(s, device="cuda") for s in shapes]
    poses.forward(again)
    assert all(a is None or torch.equal(a, b) for a, b in zip(again, tables))


# ---------------------------------------------------------------------------------------------------- 2. backward
@pytest.mark.parametrize("name", list(FIXTURES))
def test_parameter_gradients_equal_float64_autograd(name):
    """Measured (MI355X; baseline = cameras.py float32 CPU autograd vs float64, then the kernel; d ctrl_tangents / d scale): see
    DESIGN.md section 9."""
    spl, dev, segments, shapes, poses = _device_poses(name)
    d_tables = random_table_grads(shapes, seed=7)
    (ref_c, ref_s), baseline, bars = _bwd_bars(spl, segments, d_tables)
    g_dev = [None if d is None else d.cuda() for d in d_tables]
    got = {k: v.clone() for k, v in poses.backward(g_dev).items()}
    errs = [nmax_err(got["ctrl_tangents"], ref_c), nmax_err(got["scale"], ref_s)]
    print(name, "backward: baseline (ctrl, scale)", baseline, "kernel", errs, "bars", bars)
    assert errs[0] <= bars[0] and errs[1] <= bars[1], (errs, bars)
    again = poses.backward(g_dev)
    assert torch.equal(again["ctrl_tangents"], got["ctrl_tangents"]) and torch.equal(again["scale"], got["scale"])      # fixed-order sums
    # control points on no list: exactly zero, also over stale contents of the output; their neighbours are undisturbed
    empty = torch.diff(poses.plan.csr_start) == 0
    assert bool(empty.any()) or name != "k70_q130"
    poses.grads["ctrl_tangents"].fill_(float("nan"))
    third = poses.backward(g_dev)["ctrl_tangents"]
    assert torch.equal(third, got["ctrl_tangents"])
    if bool(empty.any()):
        assert float(got["ctrl_tangents"][empty.cuda()].abs().max()) == 0.0 and float(ref_c[empty].abs().max()) == 0.0
        edge = torch.zeros_like(empty)
        edge[1:] |= empty[:-1] & ~empty[1:]
        edge[:-1] |= empty[1:] & ~empty[:-1]
        assert int(edge.sum()) >= 2 and float(ref_c[edge].abs().max()) > 0
        assert float((got["ctrl_tangents"].cpu().double()[edge] - ref_c[edge]).abs().max()) <= bars[0] * float(ref_c.abs().max())
    # a rotation vector that is exactly zero gets a zero rotation gradient, like torch's
    zero = spl.ctrl_tangents.detach()[:, 3:].abs().amax(1) == 0
    if bool(zero.any()):
        assert float(got["ctrl_tangents"][zero.cuda(), 3:].abs().max()) == 0.0 and float(ref_c[zero, 3:].abs().max()) == 0.0
        assert float(got["ctrl_tangents"][zero.cuda(), :3].abs().max()) > 0
    # the eager autograd route ends in the same kernel
    tabs = poses.tables()
    assert all((t is None) == (s is None) for t, s in zip(tabs, shapes)) and all(t is None or t.requires_grad for t in tabs)
    sum((t * g).sum() for t, g in zip(tabs, g_dev) if t is not None).backward()
    assert torch.equal(dev.ctrl_tangents.grad, got["ctrl_tangents"]) and torch.equal(dev.scale.grad, got["scale"])


# ---------------------------------------------------------------------------------------------------- 3. parameters in place
def _composer_with_spline(tmp_path, n_col=48, n_evs=24, factor=3, seed=21):
    from lsenerf_amd.data import BatchComposer
    col_ds, evs_ds, scene = _scene(tmp_path)
    comp = BatchComposer(scene, n_col, n_evs, deblur=True, seed=seed, num_embd=NUM_EMBD)
    spl = make_spline(col_ds.cameras, factor=factor).to("cuda")
    spl.device = "cuda"
    segments = [("deblur", torch.tensor(COL_TIMES)), ("evs", torch.tensor(EVS_TIMES)), None]
    return col_ds, evs_ds, comp, spl, segments


def test_a_captured_step_reads_the_spline_parameters_in_place(tmp_path):
    from lsenerf_amd.graph import GraphedTrainStep
    _, _, comp, spl, segments = _composer_with_spline(tmp_path)
    comp.attach_spline(spl)
    (m, m2), (opt, opt2) = _models(2, rgb_loss_type="deblur")
    step = GraphedTrainStep(m, opt, composer=comp, ray_grads=True, jitter="input")
    g = torch.Generator().manual_seed(3)
    for it in range(3):
        if it:                                                    # the camera optimiser's update: in place, between replays
            with torch.no_grad():
                spl.ctrl_tangents.add_((torch.randn(spl.ctrl_tangents.shape, generator=g) * 0.002).cuda())
                spl.scale.mul_(1.07)
        check_fixture(copy.deepcopy(spl).cpu())
        losses = step(jitter=torch.rand(comp.n_rays, generator=g).cuda())
        assert all(np.isfinite(float(v)) for v in losses.values())
        fresh = [None if t is None else torch.zeros_like(t) for t in comp.pose_tables]
        comp.spline.forward(fresh)                                # an eager launch on the current parameters
        assert all(f is None or torch.equal(f, t) for f, t in zip(fresh, comp.pose_tables)), it
        err = _fwd_err(comp.pose_tables, spl, segments)
        d_tables = [step.pose_grads["col"], step.pose_grads["prev"], None]
        assert float(d_tables[0].abs().max()) > 0 and float(d_tables[1].abs().max()) > 0
        (ref_c, ref_s), baseline, bars = _bwd_bars(spl, segments, d_tables)
        errs = [nmax_err(step.spline_grads["ctrl_tangents"], ref_c), nmax_err(step.spline_grads["scale"], ref_s)]
        print("replay", it, "tables: max abs error", err, "gradients: baseline", baseline, "kernel", errs, "bars", bars)
        assert err < BAR_FWD, (it, err)
        assert errs[0] <= bars[0] and errs[1] <= bars[1], (it, errs, bars)
        if it:
            assert not torch.equal(comp.pose_tables[0], before)
        before = comp.pose_tables[0].clone()
    step.close()
    # ray_grads=False: only the pose evaluation is captured
    _, _, comp2, spl2, _ = _composer_with_spline(tmp_path)
    comp2.attach_spline(spl2)
    step2 = GraphedTrainStep(m2, opt2, composer=comp2)
    with torch.no_grad():
        spl2.ctrl_tangents.add_(0.001)
    step2()
    fresh = [None if t is None else torch.zeros_like(t) for t in comp2.pose_tables]
    comp2.spline.forward(fresh)
    assert all(f is None or torch.equal(f, t) for f, t in zip(fresh, comp2.pose_tables))
    assert step2.spline_grads is None and step2.pose_grads is None
    step2.close()


# ---------------------------------------------------------------------------------------------------- 4. against set_poses
def test_the_captured_spline_route_equals_the_set_poses_route(tmp_path):
    """Route (c), the spline attached, against route (b), ``set_poses`` in front of the replay fed clones of the kernel's own tables:
    same model seed, draw and jitter.  Bars of test_pose_gradients_of_a_graphed_composer_step_equal_the_ray_gradient_route."""
    from lsenerf_amd.data import spline_tables
    from lsenerf_amd.graph import GraphedTrainStep
    k0 = 2
    models, opts = _models(2, rgb_loss_type="deblur")
    col_ds, evs_ds, comp_c, spl_c, _ = _composer_with_spline(tmp_path)
    jit = torch.rand(comp_c.n_rays, generator=torch.Generator().manual_seed(1)).cuda()
    # (c)
    comp_c.attach_spline(spl_c)
    comp_c.step_dev.fill_(k0)
    step_c = GraphedTrainStep(models[0], opts[0], composer=comp_c, ray_grads=True, jitter="input")
    loss_c = {k: float(v) for k, v in step_c(jitter=jit).items()}
    grad_c = opts[0].flat.grad.clone()
    tables_c = [None if t is None else t.clone() for t in comp_c.pose_tables]
    assert int(comp_c.step_dev) == k0 + 1
    # (b)
    _, _, comp_b, spl_b, _ = _composer_with_spline(tmp_path)
    comp_b.step_dev.fill_(k0)
    step_b = GraphedTrainStep(models[1], opts[1], composer=comp_b, ray_grads=True, jitter="input")
    comp_b.set_poses(col=tables_c[0].clone(), prev=tables_c[1].clone())
    loss_b = {k: float(v) for k, v in step_b(jitter=jit).items()}
    grad_b = opts[1].flat.grad.clone()
    assert torch.equal(comp_b.batch["col_batch"]["indices"], comp_c.batch["col_batch"]["indices"])
    tabs = [spline_tables(spl_b, col_ds.cameras, "deblur"), spline_tables(spl_b, evs_ds.cameras, "evs")]
    torch.autograd.backward(tabs, [step_b.pose_grads["col"], step_b.pose_grads["prev"]])
    errs = {"flat grad": nmax_err(grad_c, grad_b, 1e-12),
            "d ctrl_tangents": nmax_err(step_c.spline_grads["ctrl_tangents"], spl_b.ctrl_tangents.grad, 1e-12),
            "d scale": nmax_err(step_c.spline_grads["scale"], spl_b.scale.grad, 1e-12)}
    print("losses (c)", loss_c, "(b)", loss_b, errs)
    assert set(loss_c) == set(loss_b) == {"rgb_loss", "event_loss"}
    for k in loss_b:
        assert abs(loss_c[k] - loss_b[k]) <= 2e-5 * max(1.0, abs(loss_b[k])), (k, loss_c[k], loss_b[k])
    assert float(spl_b.ctrl_tangents.grad.abs().max()) > 0 and float(spl_b.scale.grad.abs().max()) > 0
    for k, v in errs.items():
        assert v < TOL_GRAD, (k, v)
    step_b.close()
    step_c.close()
