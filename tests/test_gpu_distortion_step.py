"""The distortion term inside the training step (LSENeRFModelConfig.distortion_loss_mult): the eager step against the same step with
the float64 twin in the kernels' place, the captured step against the eager one, and the cases in which the term must be absent."""
import pytest
import torch

from tests import distortion_ref as dr
from tests.test_gpu_graph import _eager_step, _setup
from tests.util import TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, nmax_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

MULT = 0.01
KEYS = {"rgb_loss", "event_loss", "distortion_loss"}


def _twin_loss(t_starts, t_ends, sigmas, weights, packed_info, t_scale=1.0):
    """ops.distortion_loss restated: the float64 double sum of tests/distortion_ref.py on the weights of
    ops.render_weight_from_density (differentiable down to ``sigmas`` through lse_render_weight_bwd).  Host-synchronising."""
    from lsenerf_amd import ops
    w = ops.render_weight_from_density(t_starts, t_ends, sigmas, packed_info)[0]
    return dr.loss64(w.double(), t_starts, t_ends, packed_info, t_scale).float()


def _models(mult=MULT):
    (m_a, m_b), (o_a, o_b), batch_of = _setup(False)
    for m in (m_a, m_b):
        m.config.distortion_loss_mult = mult
    return (m_a, m_b), (o_a, o_b), batch_of


def _step_grad(m, opt, bundles, batch, jit, only=None):
    """One eager forward and backward without the optimiser step: (out_dict, losses as floats, flat gradient).  ``only``: the one
    loss key that is back-propagated (default: their sum)."""
    opt.zero_grad()
    out, losses, _ = m.train_step_bundles(*bundles, batch, jitter=jit)
    (sum(losses.values()) if only is None else losses[only]).backward()
    return out, {k: float(v.detach()) for k, v in losses.items()}, opt.flat.grad.clone()


@pytest.mark.parametrize("deferred", (True, False), ids=("count-free", "synced"))
def test_eager_step_against_the_float64_twin(deferred, monkeypatch):
    """Three loss keys; the distortion loss and the flat gradient of the whole step agree with the step whose distortion term is the
    float64 twin: over the whole gradient at TOL_GRAD, per parameter tensor (each scaled by its own maximum) at TOL_GRAD_BLOCK.  On
    the count-free path (capacity-extent arrays, ``n_dev``) and on the synchronising one.  At this multiplier the term moves the
    step's gradient by 1.7e-4 of its maximum -- less than TOL_GRAD, so the comparison of whole steps alone could not tell a wrong
    term from a right one: the gradient of the distortion loss ALONE is held to the same two bars."""
    from lsenerf_amd import ops
    (m_k, m_t), (o_k, o_t), batch_of = _models()
    for m in (m_k, m_t):
        m.deferred_counts = deferred
    bundles, batch, jit = batch_of(60)
    out, l_k, g_k = _step_grad(m_k, o_k, bundles, batch, jit)
    assert set(l_k) == KEYS
    assert [out[k]["distortion"].shape for k in ("col_out", "prev_out", "next_out")] == [(200, 1), (50, 1), (50, 1)]
    with monkeypatch.context() as mp:
        mp.setattr(ops, "distortion_loss", _twin_loss)
        _, l_t, g_t = _step_grad(m_t, o_t, bundles, batch, jit)
    assert set(l_t) == KEYS and l_t["distortion_loss"] > 0
    assert abs(l_k["distortion_loss"] - l_t["distortion_loss"]) <= 2e-5 * l_t["distortion_loss"]
    bounds = list(o_t.flat.offsets) + [o_t.flat.grad.numel()]
    e, eb = nmax_err(g_k, g_t, 1e-12), blockwise_nmax_err(g_k, g_t, bounds)
    _, _, d_k = _step_grad(m_k, o_k, bundles, batch, jit, only="distortion_loss")
    with monkeypatch.context() as mp:
        mp.setattr(ops, "distortion_loss", _twin_loss)
        _, _, d_t = _step_grad(m_t, o_t, bundles, batch, jit, only="distortion_loss")
    te, teb = nmax_err(d_k, d_t, 1e-12), blockwise_nmax_err(d_k, d_t, bounds)
    m_t.config.distortion_loss_mult = 0.0
    _, l_0, g_0 = _step_grad(m_t, o_t, bundles, batch, jit)
    print(f"DISTORTION step deferred={deferred}: losses {l_k} gradient nmax {e:.2e} per tensor {eb:.2e}; the term alone nmax {te:.2e} "
          f"per tensor {teb:.2e}; it moves the step's gradient by {nmax_err(g_k, g_0, 1e-12):.2e}")
    assert set(l_0) == KEYS - {"distortion_loss"}
    assert e < TOL_GRAD and eb < TOL_GRAD_BLOCK
    assert float(d_t.abs().max()) > 0 and te < TOL_GRAD and teb < TOL_GRAD_BLOCK


def test_graphed_step_equals_eager_step_with_the_distortion_term():
    """tests/test_gpu_graph.py's comparison with the third loss: four replays with an occupancy refresh in between, 2e-5 on the
    losses, 3e-5 per parameter tensor on the first step's gradients, and no sample count visits the host."""
    from lsenerf_amd import ops
    from lsenerf_amd.graph import GraphedTrainStep
    (m_e, m_g), (o_e, o_g), batch_of = _models()
    b0, batch0, jit0 = batch_of(50)
    step = GraphedTrainStep(m_g, o_g, *b0, batch0, jitter="input")
    assert o_g.step_count == 0 and torch.equal(o_g.flat.data, o_e.flat.data)
    ops.SYNC_STATS.update(seconds=0.0, count=0)
    spans = [(o, o + p.numel()) for p, o in zip(o_e.flat.params, o_e.flat.offsets)]
    for it in range(4):
        if it == 2:
            for m in (m_e, m_g):
                m.update_occupancy_grid(0)
        bundles, batch, jit = batch_of(60 + 10 * it)
        sync_before = ops.SYNC_STATS["count"]
        l_g = {k: float(v) for k, v in step(*bundles, batch, jitter=jit).items()}
        assert ops.SYNC_STATS["count"] == sync_before
        g_g = o_g.flat.grad.clone()
        l_e, g_e, _ = _eager_step(m_e, o_e, bundles, batch, jit, False)
        assert set(l_g) == set(l_e) == KEYS and l_e["distortion_loss"] > 0
        for k in l_e:
            assert abs(l_g[k] - l_e[k]) <= 2e-5 * max(1.0, abs(l_e[k])), (it, k, l_g[k], l_e[k])
        if it == 0:
            for a, b in spans:
                assert nmax_err(g_g[a:b], g_e[a:b], 1e-12) < 3e-5, (a, b)
        assert o_g.step_count == o_e.step_count == it + 1
    step.check_overflow()
    step.close()


def test_the_term_is_absent_without_a_multiplier_and_under_a_frozen_field():
    (m, _), (o, _), batch_of = _models(mult=0.0)
    bundles, batch, jit = batch_of(60)
    out, losses, _ = m.train_step_bundles(*bundles, batch, jitter=jit)
    assert set(losses) == {"rgb_loss", "event_loss"}
    assert all("distortion" not in v for v in out.values())
    m.config.distortion_loss_mult = MULT
    m.freeze_field()
    out, losses, _ = m.train_step_bundles(*bundles, batch, jitter=jit)
    assert set(losses) == {"rgb_loss", "event_loss"} and all("distortion" not in v for v in out.values())
    m.unfreeze_field()
    out, losses, _ = m.train_step_bundles(*bundles, batch, jitter=jit)
    assert set(losses) == {"rgb_loss", "event_loss", "distortion_loss"}
    m.eval()
    with torch.no_grad():
        assert "distortion" not in m.exec_get_outputs(bundles[0])
