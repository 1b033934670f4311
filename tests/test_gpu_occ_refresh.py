"""Count-free occupancy refresh on the device (csrc/occ_refresh.hip, lsenerf_amd.occ_refresh.DeviceGridRefresher): the occupied-cell
list against torch.nonzero, the cell draw against its numpy twin bit for bit, the refresh against the eager ``_update`` on the same
cells, the field's count-free route against the full-capacity one, graph replays against eager refreshes, and the model switch."""
import copy
from contextlib import contextmanager

import numpy as np
import pytest
import torch

from tests.util import random_binaries

pytestmark = pytest.mark.gpu

OCC_THRE = 0.01


@contextmanager
def no_host_sync():
    """torch raises on every operation that makes the host wait for the device."""
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def _estimator(levels, res, seed=0, frac=0.1, n_negative=0):
    """A seeded grid: ``binaries`` set with probability ``frac``, occs = 0.02 on the set cells, ``n_negative`` cells at -1."""
    from lsenerf_amd import LSEOccGridEstimator
    est = LSEOccGridEstimator([-1, -1, -1, 1, 1, 1], res, levels).cuda().train()
    est.binaries.copy_(random_binaries(levels, res, frac, seed).cuda())
    est.occs.copy_(est.binaries.flatten().float() * 0.02)
    if n_negative:
        g = torch.Generator().manual_seed(seed + 100)
        est.occs[torch.randperm(est.occs.numel(), generator=g)[:n_negative].cuda()] = -1.0
    return est


def analytic_density(scale):
    """``exp(-4 |x|^2) * 0.05`` of tests/test_gpu_golden.py (times ``scale``), written element by element: the value of a row does
    not depend on how many rows the call has."""
    def fn(x):
        r2 = x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]
        return torch.exp(-4 * r2) * 0.05 * scale
    return fn


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ---------------------------------------------------------------------------------------------------- 1. occupied-cell list
@pytest.mark.parametrize("frac", [0.0, 1e-4, 0.05, 0.3, 1.0])
def test_occupied_list_equals_nonzero(frac):
    from lsenerf_amd import ops
    L, res = 4, 128
    C = res ** 3
    binaries = random_binaries(L, res, frac, seed=17).cuda() if 0.0 < frac < 1.0 else torch.full((L, res, res, res), frac == 1.0).cuda()
    cell_list = torch.full((L, C), -7, dtype=torch.int32, device="cuda")
    counts = torch.full((L,), -1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(L * ops.occ_list_tiles(C), dtype=torch.int32, device="cuda")
    with no_host_sync():
        ops.occ_list_occupied(binaries.view(torch.uint8).view(L, C), cell_list, counts, ws)
    counts = counts.tolist()
    for l in range(L):
        want = torch.nonzero(binaries[l].flatten())[:, 0]
        assert counts[l] == want.numel()
        if frac == 0.3:
            assert counts[l] > C // 4                              # the regime in which the refresh draws from the list
        assert torch.equal(cell_list[l, :counts[l]].long(), want)
        assert bool((cell_list[l, counts[l]:] == -7).all())        # nothing written beyond the count


def test_occupied_list_of_a_level_that_is_no_multiple_of_the_tile():
    from lsenerf_amd import ops
    L, C = 3, 5 * 7 * 11 * 13 + 3                                  # 5008 cells: one full tile and a partial one
    g = torch.Generator().manual_seed(3)
    binaries = (torch.rand(L, C, generator=g) < 0.4).cuda()
    cell_list = torch.zeros((L, C), dtype=torch.int32, device="cuda")
    counts = torch.zeros(L, dtype=torch.int64, device="cuda")
    ws = torch.zeros(L * ops.occ_list_tiles(C), dtype=torch.int32, device="cuda")
    ops.occ_list_occupied(binaries.view(torch.uint8), cell_list, counts, ws)
    for l in range(L):
        want = torch.nonzero(binaries[l])[:, 0]
        assert int(counts[l]) == want.numel() and torch.equal(cell_list[l, :want.numel()].long(), want)


# ---------------------------------------------------------------------------------------------------- 2. draw
@pytest.mark.parametrize("seed", [0x15E5EED, (0x9E37 << 32) | 0x79B9])
@pytest.mark.parametrize("step", [272, (1 << 32) + 4112])
def test_draw_equals_the_numpy_twin_bit_for_bit(step, seed):
    """Both branches, every level; level 0 has few occupied cells (cnt <= N: the list as it is), level 1 many (cnt > N: drawn from
    the list); some cells have occs < 0 and must come out as -1 at exactly the twin's slots."""
    from lsenerf_amd.occ_refresh import DeviceGridRefresher, draw_cells_host
    L, res = 2, 32
    C = res ** 3
    est = _estimator(L, res, seed=5, frac=0.1, n_negative=500)
    est.binaries[1].copy_(random_binaries(1, res, 0.6, 9)[0].cuda())
    est.update_seed = seed
    r = DeviceGridRefresher(est, analytic_density(1.0), 0.5)
    occs = est.occs.cpu().numpy()
    aabbs = est.aabbs.cpu().numpy()
    r.step_dev.fill_(step)
    r.list_occupied()
    n_neg_seen = 0
    for warmup in (True, False):
        for level in range(L):
            with no_host_sync():
                ids, pos = r.draw_level(level, warmup)
            n = int(r.n_dev)
            occupied = torch.nonzero(est.binaries[level].flatten())[:, 0].cpu().numpy()
            want_ids, want_pos, want_n = draw_cells_host(seed, step, level, C, (res,) * 3, aabbs[level], warmup,
                                                         occs_level=occs[level * C:(level + 1) * C], occupied=occupied)
            assert n == want_n == (C if warmup else min(len(occupied), C // 4) + C // 4)
            if not warmup:
                assert (len(occupied) > C // 4) == (level == 1)
            assert np.array_equal(ids[:n].cpu().numpy(), want_ids)
            assert np.array_equal(pos[:n].cpu().numpy().view(np.uint32), want_pos.view(np.uint32))     # bit for bit
            n_neg_seen += int((want_ids < 0).sum())
    assert n_neg_seen > 100


# ---------------------------------------------------------------------------------------------------- 3. refresh, same cells
def _device_cells(refresher, step):
    """The cells and positions the refresher will use at ``step`` on the grid as it is now, per level, in ``_update_samples``'
    format (slots with id -1 are cells ``_update`` would not have listed: dropped)."""
    est = refresher.estimator
    C = est.cells_per_lvl
    warmup = step < refresher.warmup_steps
    refresher.step_dev.fill_(step)
    if not warmup:
        refresher.list_occupied()
    out = []
    for level in range(est.levels):
        ids, pos = refresher.draw_level(level, warmup)
        n = int(refresher.n_dev)
        keep = ids[:n] >= 0
        out.append(((ids[:n][keep] - level * C).clone(), pos[:n][keep].clone()))
    return out


@pytest.mark.parametrize("scale,capped", [(1.0, False), (40.0, True)])
def test_refresh_equals_the_eager_update_on_the_same_cells(scale, capped):
    """scale 1: the mean of the non-negative cells stays below occ_thre (it IS the threshold); scale 40: it exceeds occ_thre, both
    routes binarise at exactly float32(0.01) and the grids are bit-equal."""
    from lsenerf_amd.occ_refresh import DeviceGridRefresher, mean_and_threshold_host
    L, res, step_size = 4, 32, 0.5
    density = analytic_density(scale)
    est_d = _estimator(L, res, seed=2, frac=0.0, n_negative=200)
    est_d.occs.clamp_(max=0.0)                                     # all zero but the negative cells
    est_e = copy.deepcopy(est_d)
    r = DeviceGridRefresher(est_d, density, step_size, occ_thre=OCC_THRE, ema_decay=0.95, warmup_steps=256)
    for step in (0, 256, 272):                                     # the warm-up branch, then the sampled one twice
        samples = _device_cells(r, step)
        est_e._update_samples = lambda step, warmup_steps, generator, s=samples: s
        est_e._update(step, lambda x: density(x) * step_size, occ_thre=OCC_THRE, ema_decay=0.95, warmup_steps=256)
        version = est_d.grid_version
        with no_host_sync():
            r.refresh(step)
        assert est_d.grid_version == version + 1
        assert torch.equal(est_d.occs, est_e.occs), step           # bit-equal
        occs = est_d.occs.cpu().numpy()
        mean64, thre64 = mean_and_threshold_host(occs, OCC_THRE)
        print(f"scale {scale} step {step}: mean of cells >= 0 vs occ_thre -> threshold {thre64!r}, all-cells mean {mean64!r}")
        assert (thre64 == OCC_THRE) == capped
        thre_d = float(r.threshold)
        thre_e = float(torch.clamp(est_e.occs[est_e.occs >= 0].mean(), max=OCC_THRE))
        assert abs(thre_d - thre64) <= ulp32(thre64), (thre_d, thre64)
        assert abs(float(est_d.__dict__["_occ_mean_dev"]) - mean64) <= ulp32(mean64)
        assert est_d._occ_mean_host is None
        bin_d, bin_e = est_d.binaries.flatten().cpu().numpy(), est_e.binaries.flatten().cpu().numpy()
        assert np.array_equal(bin_d, occs > np.float32(thre_d))
        differ = bin_d != bin_e
        lo, hi = min(thre_d, thre_e), max(thre_d, thre_e)
        assert ((occs[differ] >= lo) & (occs[differ] <= hi)).all()
        if capped:
            assert thre_d == thre_e == float(np.float32(OCC_THRE)) and not differ.any()
        assert 0 < bin_d.sum() < bin_d.size
        est_e.binaries.copy_(est_d.binaries)                       # the next round draws from the same occupied list


# ---------------------------------------------------------------------------------------------------- 4. field route
def test_count_free_field_route_equals_the_full_capacity_route():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd.occ_refresh import DeviceGridRefresher
    torch.manual_seed(96)
    cfg = LSENeRFModelConfig()
    model = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=8).cuda().train()
    with torch.no_grad():                                          # tools/bench_context.py: spatially varied, partly opaque
        model.field.mlp_base_grid.params.mul_(3000.0)
        model.field.mlp_base_mlp.params[-16 * 64:-15 * 64].mul_(6.0)
    est_a = model.occupancy_grid
    est_b = copy.deepcopy(est_a)
    field = model.field
    seen = []

    def full_capacity(p):
        seen.append(p.shape[0])
        return field.density_fn(p)

    r_a = DeviceGridRefresher(est_a, field, cfg.render_step_size)
    r_b = DeviceGridRefresher(est_b, full_capacity, cfg.render_step_size)
    C = est_a.cells_per_lvl
    for step in (0, 16, 256, 272):
        with no_host_sync():
            r_a.refresh(step)
            r_b.refresh(step)
        assert torch.equal(est_a.occs, est_b.occs), step
        assert torch.equal(est_a.binaries, est_b.binaries), step
        assert float(est_a.__dict__["_occ_mean_dev"]) == float(est_b.__dict__["_occ_mean_dev"])
        frac = float(est_a.binaries.float().mean())
        assert 0.0 < frac < 1.0, frac
    assert seen == [C] * 8 + [2 * (C // 4)] * 8                    # the callable always sees the whole capacity


# ---------------------------------------------------------------------------------------------------- 5. graph
@pytest.mark.parametrize("first_step", [0, 256])
def test_graph_replays_reproduce_eager_refreshes(first_step):
    from lsenerf_amd.occ_refresh import DeviceGridRefresher
    L, res = 2, 32
    density = analytic_density(3.0)
    est_g = _estimator(L, res, seed=4, frac=0.4, n_negative=100)
    est_e = copy.deepcopy(est_g)
    hooks = []
    est_g.after_update_hook = lambda: hooks.append(est_g.grid_version)
    r_g = DeviceGridRefresher(est_g, density, 0.5)
    r_e = DeviceGridRefresher(est_e, density, 0.5)
    state = lambda est: (est.occs.clone(), est.binaries.clone(), est.__dict__["_occ_mean_dev"].clone())
    before, got, want = state(est_g), [], []
    version = est_g.grid_version
    with no_host_sync():
        r_g.capture()
        after_capture = state(est_g)
        for k in range(3):
            r_g.refresh(first_step + 16 * k)
            got.append(state(est_g))
            r_e.refresh(first_step + 16 * k)
            want.append(state(est_e))
    assert r_g.captured and not r_e.captured
    for a, b in zip(before, after_capture):
        assert torch.equal(a, b)                                   # capturing refreshed nothing
    assert est_g.grid_version == version + 3 and hooks == [version + 1, version + 2, version + 3]
    for k in range(3):
        for a, b in zip(got[k], want[k]):
            assert torch.equal(a, b), k
    assert not torch.equal(got[0][0], before[0]) and not torch.equal(got[1][0], got[0][0]) and not torch.equal(got[2][0], got[1][0])
    # the graph draws afresh at every replay: the same state refreshed as another step gives another grid
    est_g.occs.copy_(before[0]); est_g.binaries.copy_(before[1])
    r_g.refresh(first_step + 48)
    assert not torch.equal(est_g.occs, got[0][0])


# ---------------------------------------------------------------------------------------------------- 6. model switch
def test_model_switch_routes_the_refresh_and_the_graphed_step_follows_it():
    from lsenerf_amd.graph import GraphedTrainStep
    from tests.test_gpu_graph import _eager_step, _setup
    (m_e, m_g), (o_e, o_g), batch_of = _setup(False)
    for m in (m_e, m_g):
        assert m.config.device_grid_refresh is False               # the default: nothing changes
        m.config.device_grid_refresh = True
    hooks = []
    m_g.occupancy_grid.after_update_hook = lambda: hooks.append(1)
    eager_updates = []
    for m in (m_e, m_g):
        m.occupancy_grid._update = lambda *a, **k: eager_updates.append(1)
    b0, batch0, jit0 = batch_of(50)
    step = GraphedTrainStep(m_g, o_g, *b0, batch0, jitter="input")
    est = m_g.occupancy_grid
    for it in range(4):
        if it == 2:
            snap = (est.occs.clone(), est.binaries.clone(), est.grid_version)
            m_g.update_occupancy_grid(5)                           # not a refresh step: nothing changes
            assert torch.equal(est.occs, snap[0]) and torch.equal(est.binaries, snap[1]) and est.grid_version == snap[2]
            assert hooks == []
            for m in (m_e, m_g):
                m.update_occupancy_grid(0)                         # a refresh step, through the device route
            assert est.grid_version == snap[2] + 1 and hooks == [1] and eager_updates == []
            assert not torch.equal(est.occs, snap[0])
            # the device-side cap of the alpha threshold is the new mean already (torch sums in float32: 1e-6 relative)
            mean_now = float(est.occs.double().mean())
            assert mean_now > 0.0 and abs(float(est.__dict__["_occ_mean_dev"]) - mean_now) <= ulp32(mean_now)
        bundles, batch, jit = batch_of(60 + 10 * it)
        l_g = {k: float(v) for k, v in step(*bundles, batch, jitter=jit).items()}
        l_e, _, _ = _eager_step(m_e, o_e, bundles, batch, jit, False)
        for k in l_e:
            assert abs(l_g[k] - l_e[k]) <= 2e-5 * max(1.0, abs(l_e[k])), (it, k, l_g[k], l_e[k])
    step.check_overflow()
    step.close()
    # outside training the switch raises like update_every_n_steps does
    m_g.eval()
    with pytest.raises(RuntimeError, match="only during training"):
        m_g.update_occupancy_grid(16)
    m_g.train()
    # with the switch off, `_update` is the code path taken
    m_g.config.device_grid_refresh = False
    version = est.grid_version
    m_g.update_occupancy_grid(16)
    assert eager_updates == [1] and est.grid_version == version    # (the stand-in did nothing)
