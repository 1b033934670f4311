"""The frozen-field refinement step with ``freeze_field(input_only_mlp=True)``: both frozen MLPs differentiate through
``lse_mlp_bwd_input`` (d(input) and d(row_bias) alone) instead of the training kernel with its weight-gradient products parked in
a scratch.  The launch census, the gradients against the default frozen route on a twin model and against the unfrozen model, and
the captured phases 1 (embedding) and 2 (cameras, ``opt=None``) without an eager step before the capture."""
import pytest
import torch

from tests.test_gpu_refine import HASH_BWD, _adam, _batch_of, _frozen_snapshot, _models
from tests.util import nmax_err

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

BAR = 3e-5          # tests/test_gpu_refine.py: frozen step against the unfrozen model (nmax_err, floor 1e-12)


@pytest.fixture(autouse=True)
def _every_stream_mismatch_counts():
    before = torch.is_warn_always_enabled()
    torch.set_warn_always(True)
    yield
    torch.set_warn_always(before)


@pytest.fixture
def is_eval():
    from lsenerf_amd import model as M
    M.gbconfig.IS_EVAL = True
    try:
        yield
    finally:
        M.gbconfig.IS_EVAL = False


def _with_ray_grads(bundles):
    from lsenerf_amd import RayBundle
    return [RayBundle(origins=b.origins.clone().requires_grad_(True), directions=b.directions.clone().requires_grad_(True),
                      camera_indices=b.camera_indices, metadata=b.metadata) for b in bundles]


def _no_scratch(m):
    return [n for n, p in m.named_parameters() if not p.requires_grad and hasattr(p, "_lse_wgrad_scratch")] == []


# ---------------------------------------------------------------------------------------------------- 1. launch census
@pytest.mark.parametrize("ray_grads", [True, False])
def test_launch_census_with_the_flag_and_after_taking_it_back(ray_grads, monkeypatch):
    from lsenerf_amd import _lib
    (m,) = _models(1)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])

    def backward_calls():
        bundles, batch, jit = _batch_of(50)
        if ray_grads:
            bundles = _with_ray_grads(bundles)
        for p in m.parameters():
            p.grad = None
        del calls[:]
        _, losses, _ = m.train_step_bundles(*bundles, batch, jitter=jit)
        fwd = len(calls)
        sum(losses.values()).backward()
        if ray_grads:
            assert all(float(b.origins.grad.abs().max()) > 0 for b in bundles)
        return calls[fwd:]

    left = m.freeze_field(input_only_mlp=True)
    assert len(left) == 1 and left[0] is m.field.embedding_appearance.embedding.weight
    assert m.field.mlp_head.input_only_bwd and m.field.mlp_base_mlp.input_only_bwd and _no_scratch(m)
    bwd = backward_calls()
    print("REFINE input-only census", "ray grads" if ray_grads else "no ray grads", bwd)
    assert bwd.count("lse_mlp_bwd_input") == (2 if ray_grads else 1)
    assert bwd.count("lse_mlp_bwd") == 0 and bwd.count("lse_mlp_wgrad") == 0
    assert not [c for c in bwd if c in ("lse_hash_bwd", "lse_hash_bwd_levels", "lse_hash_bwd_ex")]
    assert bwd.count("lse_hash_bwd_input") == (1 if ray_grads else 0)
    assert float(left[0].grad.abs().max()) > 0
    assert all(p.grad is None for p in m.parameters() if not p.requires_grad)
    assert _no_scratch(m)                                           # never allocated, never touched
    # the flag taken back: the default frozen route again
    m.unfreeze_field()
    assert not m.field.mlp_head.input_only_bwd and not m.field.mlp_base_mlp.input_only_bwd
    assert all(p.requires_grad for p in (m.field.mlp_head.params, m.field.mlp_base_mlp.params))
    m.freeze_field()
    bwd = backward_calls()
    assert bwd.count("lse_mlp_bwd_input") == 0 and bwd.count("lse_mlp_bwd") == (2 if ray_grads else 1)
    if not ray_grads:
        assert not [c for c in bwd if c in HASH_BWD]


# ---------------------------------------------------------------------------------------------------- 2. against the twins (eager)
def test_eager_gradients_against_the_default_frozen_route_and_the_unfrozen_model():
    """Three copies of one model on the same rays and jitter: unfrozen, frozen (default route), frozen with the flag.  The forward is
    untouched, so the flag's losses are those of the default route bit for bit; ray gradients and the embedding gradient within the
    3e-5 bar against both."""
    m_u, m_d, m_n = _models(3)
    left_d, left_n = m_d.freeze_field(), m_n.freeze_field(input_only_mlp=True)
    bundles, batch, jit = _batch_of(50)
    res = {}
    for key, m in (("u", m_u), ("d", m_d), ("n", m_n)):
        bs = _with_ray_grads(bundles)
        _, losses, _ = m.train_step_bundles(*bs, batch, jitter=jit)
        sum(losses.values()).backward()
        res[key] = ({k: v.detach().clone() for k, v in losses.items()}, [(b.origins.grad, b.directions.grad) for b in bs],
                    m.field.embedding_appearance.embedding.weight.grad)
    for k, v in res["n"][0].items():
        assert torch.equal(v.view(torch.int32), res["d"][0][k].view(torch.int32)), k
    for other in ("d", "u"):
        for i, ((go, gd), (ro, rd)) in enumerate(zip(res["n"][1], res[other][1])):
            errs = nmax_err(go, ro, 1e-12), nmax_err(gd, rd, 1e-12)
            print("REFINE input-only ray grads vs", other, i, errs)
            assert float(ro.abs().max()) > 0 and max(errs) < BAR, (other, i, errs)
        e = nmax_err(res["n"][2], res[other][2], 1e-12)
        print("REFINE input-only embedding gradient vs", other, e)
        assert float(res[other][2].abs().max()) > 0 and e < BAR, (other, e)
    assert _no_scratch(m_n) and left_d and left_n


# ---------------------------------------------------------------------------------------------------- 3a. phase 1, captured
def test_captured_phase_one_without_an_eager_step(is_eval):
    """The test embedding row trained, rays differentiated, the graph captured on a model no eager step has touched.  First replay
    against the default frozen route (captured twin) and the unfrozen model's eager step; four replays move nothing frozen, read
    no sample count on the host and never create the scratch."""
    from lsenerf_amd import model as M, ops
    from lsenerf_amd.graph import GraphedTrainStep
    from tests.test_gpu_graph import _eager_step
    m_e, m_d, m_n = _models(3, "evs_emb")
    M.gbconfig.IS_EVAL = False
    o_e = _adam(m_e.get_param_groups()["fields"])
    M.gbconfig.IS_EVAL = True
    left_d, left_n = m_d.freeze_field(), m_n.freeze_field(input_only_mlp=True)
    frozen0 = _frozen_snapshot(m_n, left_n)
    assert len(frozen0) >= 6 and _no_scratch(m_n)
    o_d, o_n = _adam(left_d), _adam(left_n)
    b0, batch0, _ = _batch_of(50)
    step_n = GraphedTrainStep(m_n, o_n, *b0, batch0, ray_grads=True, jitter="input")
    step_d = GraphedTrainStep(m_d, o_d, *b0, batch0, ray_grads=True, jitter="input")
    ops.SYNC_STATS.update(seconds=0.0, count=0)
    for it in range(4):
        bundles, batch, jit = _batch_of(60 + 10 * it)
        sync_before = ops.SYNC_STATS["count"]
        l_n = {k: float(v.detach()) for k, v in step_n(*bundles, batch, jitter=jit).items()}
        assert ops.SYNC_STATS["count"] == sync_before
        if it:
            continue
        emb_n, emb_d, emb_e = (m.field.embedding_appearance for m in (m_n, m_d, m_e))
        g_row = emb_n.test_emb.weight.grad.clone()
        rg = {k: (a.clone(), b.clone()) for k, (a, b) in step_n.ray_grads.items()}
        l_d = {k: float(v.detach()) for k, v in step_d(*bundles, batch, jitter=jit).items()}
        assert l_n == l_d                                           # the same forward
        for key in rg:
            errs = [nmax_err(a, b, 1e-12) for a, b in zip(rg[key], step_d.ray_grads[key])]
            print("REFINE input-only captured ray grads vs default", key, errs)
            assert float(rg[key][0].abs().max()) > 0 and max(errs) < BAR, (key, errs)
        e_d = nmax_err(g_row, emb_d.test_emb.weight.grad, 1e-12)
        l_e, _, bs = _eager_step(m_e, o_e, bundles, batch, jit, True)
        for k in l_e:
            assert abs(l_n[k] - l_e[k]) <= 2e-5 * max(1.0, abs(l_e[k])), (k, l_n[k], l_e[k])
        for key, be in zip(("col", "prev", "next"), bs):
            errs = nmax_err(rg[key][0], be.origins.grad, 1e-12), nmax_err(rg[key][1], be.directions.grad, 1e-12)
            print("REFINE input-only captured ray grads vs unfrozen", key, errs)
            assert max(errs) < BAR, (key, errs)
        e_e = nmax_err(g_row, emb_e.test_emb.weight.grad, 1e-12)
        print("REFINE input-only captured embedding row gradient vs default", e_d, "vs unfrozen", e_e)
        assert float(g_row.abs().max()) > 0 and max(e_d, e_e) < BAR
    assert o_n.step_count == 4
    step_n.check_overflow()
    for n, p in m_n.named_parameters():
        if n in frozen0:
            assert not p.requires_grad and p.grad is None, n
            assert torch.equal(p.detach().view(torch.int32), frozen0[n].view(torch.int32)), n
    assert _no_scratch(m_n)
    step_n.close()
    step_d.close()


# ---------------------------------------------------------------------------------------------------- 3b. phase 2, captured
def test_captured_camera_only_phase_without_an_eager_step(tmp_path):
    """``opt=None, camera_opt=``: the whole field frozen with the flag.  Camera gradients of the first replay against the default
    frozen route and against an unfrozen copy; four replays leave every model parameter bit-identical."""
    from lsenerf_amd import ops
    from lsenerf_amd.graph import GraphedTrainStep
    from tests.test_gpu_pose_delta import _setup_camera_adam
    setups = {}
    for key in ("n", "d", "u"):
        (tmp_path / key).mkdir()
        setups[key] = _setup_camera_adam(tmp_path / key, "deltas")
    (comp_n, m_n, _, cam_n, _), (comp_d, m_d, _, cam_d, _), (comp_u, m_u, opt_u, _, _) = (setups[k] for k in ("n", "d", "u"))
    assert m_n.freeze_field(train_embedding=False, input_only_mlp=True) == [] and m_d.freeze_field(train_embedding=False) == []
    params0 = {n: p.detach().clone() for n, p in m_n.named_parameters()}
    assert _no_scratch(m_n)
    jit = torch.rand(comp_n.n_rays, generator=torch.Generator().manual_seed(1)).cuda()
    step_n = GraphedTrainStep(m_n, None, composer=comp_n, ray_grads=True, jitter="input", camera_opt=cam_n)
    step_d = GraphedTrainStep(m_d, None, composer=comp_d, ray_grads=True, jitter="input", camera_opt=cam_d)
    step_u = GraphedTrainStep(m_u, opt_u, composer=comp_u, ray_grads=True, jitter="input", optimizer_in_graph=False)
    ops.SYNC_STATS.update(seconds=0.0, count=0)
    l_n = {k: float(v.detach()) for k, v in step_n(jitter=jit).items()}
    g_n = {k: v.clone() for k, v in step_n.camera_grads.items()}
    l_d = {k: float(v.detach()) for k, v in step_d(jitter=jit).items()}
    l_u = {k: float(v.detach()) for k, v in step_u(jitter=jit).items()}
    assert l_n == l_d and set(g_n) == set(step_d.camera_grads) == set(step_u.camera_grads) and len(g_n) >= 2
    for k in l_u:
        assert abs(l_n[k] - l_u[k]) <= 2e-5 * max(1.0, abs(l_u[k])), (k, l_n[k], l_u[k])
    for k, g in g_n.items():
        errs = nmax_err(g, step_d.camera_grads[k], 1e-12), nmax_err(g, step_u.camera_grads[k], 1e-12)
        print("REFINE input-only camera gradient", k, "vs default, unfrozen:", errs)
        assert float(g.abs().max()) > 0 and max(errs) < BAR, (k, errs)
    sync_before = ops.SYNC_STATS["count"]
    for _ in range(3):
        step_n(jitter=jit)
    assert ops.SYNC_STATS["count"] == sync_before and cam_n.step_count == 4
    for n, p in m_n.named_parameters():
        assert torch.equal(p.detach().view(torch.int32), params0[n].view(torch.int32)), n
    assert _no_scratch(m_n)
    for s in (step_n, step_d, step_u):
        s.close()
