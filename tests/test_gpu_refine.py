"""The frozen-field refinement step (R:scripts/emb_eval.sh: fit the test appearance embedding, then the evaluation cameras, with
the radiance field frozen): ``LSENeRFModel.freeze_field`` + ``GraphedTrainStep``.  The captured frozen step must compute what the
unfrozen eager step computes for everything that still trains, launch no table-gradient scatter and no weight-gradient kernel,
hand no frozen parameter a gradient, and actually refine the embedding row it is given."""
import copy

import pytest
import torch

from tests.util import nmax_err, random_binaries, random_rays

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

SIZES = (200, 50, 50)
HASH_BWD = ("lse_hash_bwd", "lse_hash_bwd_levels", "lse_hash_bwd_ex", "lse_hash_bwd_input")


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


def _models(n, embedding="global_emb"):
    """tests/test_gpu_graph.py::_setup's model (2 occupancy levels of 32^3, log2_hashmap_size 15, the same occupancy), ``n`` deep
    copies on the GPU; ``embedding="evs_emb"``: a per-frame embedding with eval_mode "param" and its test row initialised."""
    from lsenerf_amd import LSEEmbeddingConfig, LSENeRFModel, LSENeRFModelConfig
    torch.manual_seed(96)
    cfg = LSENeRFModelConfig(grid_levels=2, grid_resolution=32, log2_hashmap_size=15, use_mapping=True, mapping_method="identity",
                             map_mode="co_map", evs_mapping_method="powpow",
                             embed_config=LSEEmbeddingConfig(embedding, eval_mode="param" if embedding == "evs_emb" else "zero"))
    base = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), 30)
    with torch.no_grad():
        base.field.mlp_base_grid.params.mul_(300.0)
    if embedding == "evs_emb":
        base.init_test_params()
    out = []
    for _ in range(n):
        m = copy.deepcopy(base).cuda().train()
        m.occupancy_grid.binaries.copy_(random_binaries(2, 32, 0.5, 3).cuda())
        m.occupancy_grid.occs.copy_(m.occupancy_grid.binaries.flatten().float() * 0.012)
        out.append(m)
    return out


def _batch_of(seed, sizes=SIZES):
    from lsenerf_amd import RayBundle
    g = torch.Generator().manual_seed(seed)
    bundles = []
    for i, n in enumerate(sizes):
        o, d = random_rays(n, seed=seed + i)
        bundles.append(RayBundle(origins=o.cuda(), directions=d.cuda(), camera_indices=torch.zeros(n, 1, dtype=torch.long, device="cuda"),
                                 metadata={"appearance_id": torch.randint(0, 16, (n,), generator=g).cuda()}))
    batch = {"col_batch": {"image": torch.rand(sizes[0], 3, generator=g).cuda()}}
    if len(sizes) > 1:
        batch["evs_batch"] = {"image": ((torch.rand(sizes[1], 1, generator=g) - 0.5) * 0.4).cuda()}
    return bundles, batch, torch.rand(sum(sizes), generator=g).cuda()


def _adam(params):
    from lsenerf_amd.optim import FlatAdam, FlatParams
    return FlatAdam(FlatParams(params), lr=1e-2, eps=1e-15)


def _frozen_snapshot(m, trainable):
    keep = {id(p) for p in trainable}
    return {n: p.detach().clone() for n, p in m.named_parameters() if id(p) not in keep}


# ---------------------------------------------------------------------------------------------------- 1. phase 1, captured
def test_captured_frozen_step_equals_the_unfrozen_eager_step(is_eval):
    """Phase 1: the field frozen, the test embedding row trained (evs_emb, eval_mode "param", IS_EVAL routing), rays
    differentiated.  Losses, ray gradients and the embedding's gradient of the first replay against the UNFROZEN copy's eager step
    on the same rays and jitter, within the bars of tests/test_gpu_graph.py; after four replays nothing frozen has moved or
    received a gradient and no sample count visited the host."""
    from lsenerf_amd import model as M, ops
    from lsenerf_amd.graph import GraphedTrainStep
    from tests.test_gpu_graph import _eager_step
    m_e, m_f = _models(2, "evs_emb")
    M.gbconfig.IS_EVAL = False
    o_e = _adam(m_e.get_param_groups()["fields"])            # every parameter a training run optimises, test row included
    M.gbconfig.IS_EVAL = True
    left = m_f.freeze_field()
    emb_f, emb_e = m_f.field.embedding_appearance, m_e.field.embedding_appearance
    assert [id(p) for p in left] == [id(p) for p in emb_f.parameters()] and len(left) == 2
    frozen0 = _frozen_snapshot(m_f, left)
    assert len(frozen0) >= 6
    o_f = _adam(left)
    b0, batch0, _ = _batch_of(50)
    step = GraphedTrainStep(m_f, o_f, *b0, batch0, ray_grads=True, jitter="input")
    assert o_f.step_count == 0
    ops.SYNC_STATS.update(seconds=0.0, count=0)
    for it in range(4):
        bundles, batch, jit = _batch_of(60 + 10 * it)
        sync_before = ops.SYNC_STATS["count"]
        l_f = {k: float(v) for k, v in step(*bundles, batch, jitter=jit).items()}
        assert ops.SYNC_STATS["count"] == sync_before                # no sample count visited the host
        if it:
            continue
        g_row, g_tab = emb_f.test_emb.weight.grad.clone(), emb_f.embedding.weight.grad.clone()
        rg = {k: (a.clone(), b.clone()) for k, (a, b) in step.ray_grads.items()}
        l_e, _, bs = _eager_step(m_e, o_e, bundles, batch, jit, True)
        assert set(l_f) == set(l_e) == {"rgb_loss", "event_loss"}
        for k in l_e:
            assert abs(l_f[k] - l_e[k]) <= 2e-5 * max(1.0, abs(l_e[k])), (k, l_f[k], l_e[k])
        for key, be in zip(("col", "prev", "next"), bs):
            assert float(be.origins.grad.abs().max()) > 0
            errs = nmax_err(rg[key][0], be.origins.grad, 1e-12), nmax_err(rg[key][1], be.directions.grad, 1e-12)
            print("REFINE ray grads", key, errs)
            assert max(errs) < 3e-5, (key, errs)
        e_row = nmax_err(g_row, emb_e.test_emb.weight.grad, 1e-12)
        print("REFINE embedding row gradient", e_row, "losses", l_f, l_e)
        assert float(g_row.abs().max()) > 0 and e_row < 3e-5
        assert float(g_tab.abs().max()) == 0.0 and float(emb_e.embedding.weight.grad.abs().max()) == 0.0      # IS_EVAL: not read
    assert o_f.step_count == 4
    step.check_overflow()
    for n, p in m_f.named_parameters():
        if n in frozen0:
            assert not p.requires_grad and p.grad is None, n
            assert torch.equal(p.detach().view(torch.int32), frozen0[n].view(torch.int32)), n
    step.close()


# ---------------------------------------------------------------------------------------------------- 2. launch census
@pytest.mark.parametrize("ray_grads", [True, False])
def test_launch_census_of_an_eager_frozen_step(ray_grads, monkeypatch):
    from lsenerf_amd import RayBundle, _lib
    (m,) = _models(1)
    left = m.freeze_field()
    assert len(left) == 1 and left[0] is m.field.embedding_appearance.embedding.weight
    bundles, batch, jit = _batch_of(50)
    if ray_grads:
        bundles = [RayBundle(origins=b.origins.clone().requires_grad_(True), directions=b.directions.clone().requires_grad_(True),
                             camera_indices=b.camera_indices, metadata=b.metadata) for b in bundles]
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    _, losses, _ = m.train_step_bundles(*bundles, batch, jitter=jit)
    fwd = len(calls)
    sum(losses.values()).backward()
    bwd = calls[fwd:]
    print("REFINE census", "ray grads" if ray_grads else "no ray grads", bwd)
    assert not [c for c in bwd if c in ("lse_hash_bwd", "lse_hash_bwd_levels", "lse_hash_bwd_ex", "lse_mlp_wgrad")]
    if ray_grads:
        assert bwd.count("lse_hash_bwd_input") == 1 and bwd.count("lse_mlp_bwd") == 2
        assert all(float(b.origins.grad.abs().max()) > 0 for b in bundles)
    else:
        assert not [c for c in bwd if c in HASH_BWD + ("lse_positions_bwd", "lse_ray_grad_from_dx01", "lse_ray_grad_reduce")]
        assert bwd.count("lse_mlp_bwd") == 1                     # the head; the base has nothing to differentiate
    assert float(left[0].grad.abs().max()) > 0
    assert all(p.grad is None for p in m.parameters() if not p.requires_grad)


# ---------------------------------------------------------------------------------------------------- 3. phase 2: opt=None
def test_camera_only_step_without_a_field_optimiser(tmp_path):
    """Phase 2: the whole field frozen, the per-camera optimisers and their Adam inside the captured step, ``opt=None``.  The
    camera gradients of the first replay against an unfrozen copy run with ``optimizer_in_graph=False``."""
    from lsenerf_amd.graph import GraphedTrainStep
    from tests.test_gpu_pose_delta import _setup_camera_adam
    (tmp_path / "frozen").mkdir()
    (tmp_path / "trained").mkdir()
    comp_f, m_f, _, cam_f, _ = _setup_camera_adam(tmp_path / "frozen", "deltas")
    comp_u, m_u, opt_u, _, _ = _setup_camera_adam(tmp_path / "trained", "deltas")
    assert m_f.freeze_field(train_embedding=False) == []
    params0 = {n: p.detach().clone() for n, p in m_f.named_parameters()}
    jit = torch.rand(comp_f.n_rays, generator=torch.Generator().manual_seed(1)).cuda()
    step_f = GraphedTrainStep(m_f, None, composer=comp_f, ray_grads=True, jitter="input", camera_opt=cam_f)
    step_u = GraphedTrainStep(m_u, opt_u, composer=comp_u, ray_grads=True, jitter="input", optimizer_in_graph=False)
    cam0 = cam_f.flat.data.clone()
    l_f = {k: float(v) for k, v in step_f(jitter=jit).items()}
    g_f = {k: v.clone() for k, v in step_f.camera_grads.items()}
    l_u = {k: float(v) for k, v in step_u(jitter=jit).items()}
    assert set(g_f) == set(step_u.camera_grads) and len(g_f) >= 2
    for k in l_u:
        assert abs(l_f[k] - l_u[k]) <= 2e-5 * max(1.0, abs(l_u[k])), (k, l_f[k], l_u[k])
    for k, g in g_f.items():
        err = nmax_err(g, step_u.camera_grads[k], 1e-12)
        print("REFINE camera gradient", k, err)
        assert float(g.abs().max()) > 0 and err < 3e-5, (k, err)
    assert cam_f.step_count == 1 and not torch.equal(cam_f.flat.data, cam0)         # the camera Adam ran inside the graph
    for n, p in m_f.named_parameters():
        assert torch.equal(p.detach().view(torch.int32), params0[n].view(torch.int32)), n
    step_f.close()
    step_u.close()


# ---------------------------------------------------------------------------------------------------- 4. it refines
def test_forty_replays_pull_a_perturbed_test_row_back(is_eval):
    """Targets rendered with a known ``test_emb`` row; the row perturbed; 40 captured phase-1 steps on those targets (colour rays,
    fixed jitter).  The colour loss falls, and the row is the only tensor of the model that changed."""
    from lsenerf_amd.graph import GraphedTrainStep
    (m,) = _models(1, "evs_emb")
    (col,), _, jit = _batch_of(50, sizes=(200,))
    row = m.field.embedding_appearance.test_emb.weight
    with torch.no_grad():
        out, _, _ = m.train_step_bundles(col, None, None, {"col_batch": {"image": torch.zeros(200, 3, device="cuda")}}, jitter=jit)
        target = out["col_out"]["rgb"].clone()
        assert bool(torch.isfinite(target).all()) and float(target.std()) > 0
        row.add_(torch.randn(row.shape, generator=torch.Generator().manual_seed(4)).cuda() * 0.5)
    batch = {"col_batch": {"image": target}}
    left = m.freeze_field()
    opt = _adam(left)                       # (FlatParams re-points the two embedding tensors: snapshot afterwards)
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    step = GraphedTrainStep(m, opt, col, None, None, batch, jitter="input")
    losses = [float(step(col, None, None, batch, jitter=jit)["rgb_loss"]) for _ in range(40)]
    print("REFINE colour loss: first", losses[0], "last", losses[-1])
    assert losses[0] > 0 and losses[-1] < losses[0]
    changed = [k for k, v in m.state_dict().items() if not torch.equal(v, state0[k])]
    assert changed == ["field.embedding_appearance.test_emb.weight"], changed
    step.check_overflow()
    step.close()
