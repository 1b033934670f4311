"""Early ray termination of the whole-image eval render on the GPU.

Kernel level (hand-built slots, no marcher, no field): the segment loop driven through the ``ops`` wrappers against
``ops.eval_composite`` on the same arrays with every ray cut at the count the route returns (bit for bit), the termination rule
against float64 prefix sums, reproducibility.  Model level: ``get_outputs_for_camera_ray_bundle`` with ``eval_early_stop_eps > 0``
against the full march + one field evaluation + ``ops.eval_composite`` with the counts replaced (bit for bit), that rays are stopped
at all, closeness to the full render, no host synchronisation, ``eps = 0`` unchanged, and the fallback in training mode."""
import math

import numpy as np
import pytest
import torch

from tests.test_eval_early_stop_cpu import composite_first_m_numpy, schedule_boundaries, stop_count_numpy, tau_prefix64
from tests.test_gpu_eval import CHUNK, H, W, _bundle, _model

pytestmark = pytest.mark.gpu

# ----------------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------------
R, CAP, DT = 131, 320, 1.0 / 256             # 131 rays: the last workgroup of four waves is partial
COUNTS = (0, 1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 300, 320)
N_PATTERNS = 10                              # (a) transparent, (b) x 7 finite walls, (c) infinite wall, (d) linear rise


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bit patterns: NaN outputs (NaN colours composited without nan_to_num) must agree too."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _pattern_of(r: int) -> int:
    return (r % len(COUNTS) + r // len(COUNTS)) % N_PATTERNS      # every count meets (nearly) every pattern over the 131 rays


def _wall_positions(S: int):
    return (0, 63, 64, S - 1, S, S + 1, 2 * S)


def _scene(S: int, tau_stop: float):
    """Slots [R, CAP] (host, float32): interval ends, densities, colours [.., 4]; per ray its count, pattern and wall position."""
    g = np.random.default_rng(1234 + S)
    cnts = np.array([COUNTS[r % len(COUNTS)] for r in range(R)], dtype=np.int64)
    k = np.arange(CAP, dtype=np.float32)
    ts = np.broadcast_to(np.float32(0.25) + k * np.float32(DT), (R, CAP)).copy()
    te = ts + np.float32(DT)
    sigma = (g.random((R, CAP)) * 0.3).astype(np.float32)            # tau of the whole row < 320 * 0.3 / 256 = 0.375 < 0.5
    wall = np.full(R, -1, dtype=np.int64)
    pat = np.array([_pattern_of(r) for r in range(R)])
    for r in range(R):
        p = pat[r]
        if 1 <= p <= 7:                                              # (b) sigma * dt = 1e3 at k0
            wall[r] = _wall_positions(S)[p - 1]
            sigma[r, wall[r]] = np.float32(1e3 / DT)
        elif p == 8:                                                 # (c) sigma = +inf
            wall[r] = (r * 37) % 300
            sigma[r, wall[r]] = np.inf
        elif p == 9:                                                 # (d) tau rises linearly and crosses tau_stop in mid-segment 1
            sigma[r, :] = np.float32(tau_stop / ((S + S // 2) * DT) * (1.0 + 0.01 * (r % 5)))
    rgb = g.random((R, CAP, 4)).astype(np.float32)
    rgb[:, :, 3] = np.nan                                            # the pad column is never read
    for i, (r, kk, c, v) in enumerate([(3, 0, 0, np.inf), (5, 70, 1, -np.inf), (12, 3, 2, np.nan), (27, 63, 0, np.nan),
                                       (40, 64, 1, np.inf), (77, 128, 2, -np.inf), (130, 5, 0, np.nan), (96, 200, 1, np.nan)]):
        rgb[r, kk, c] = v
    return ts, te, sigma, rgb, cnts, pat, wall


def _gather(packed, ri, n, off, slots):
    """Values of the slot rows for the n packed samples of a segment that starts at slot ``off`` of every row."""
    r = ri[:n].long()
    pos = torch.arange(n, device=ri.device) - packed[r, 0]
    return slots[r, off + pos]


def _run_segments(scene, S, tau_stop, nan_to_num):
    """The route of evaluation._render_early_stop with a look-up in place of the field.  Returns the state buffer."""
    from lsenerf_amd import ops
    from lsenerf_amd.evaluation import segment_schedule
    ts_h, te_h, sg_h, rgb_h, cnts_h = scene[:5]
    dev = "cuda"
    ts_slots, te_slots = torch.from_numpy(ts_h).to(dev), torch.from_numpy(te_h).to(dev)
    sg_slots, rgb_slots, cnts = torch.from_numpy(sg_h).to(dev), torch.from_numpy(rgb_h).to(dev), torch.from_numpy(cnts_h).to(dev)
    sched = segment_schedule(CAP, S)
    longest = max(length for _, length in sched)
    state = torch.empty(ops.eval_segment_state_bytes(R), dtype=torch.uint8, device=dev)
    seg_cnts = torch.empty(R, dtype=torch.int64, device=dev)
    ri_b = torch.empty(R * longest, dtype=torch.int32, device=dev)
    ts_b, te_b = torch.empty(R * longest, device=dev), torch.empty(R * longest, device=dev)
    ops.eval_segment_begin(cnts, sched[0][1], state, seg_cnts)
    evaluated = 0
    for k, (off, length) in enumerate(sched):
        packed, total = ops.pack_info_from_counts(seg_cnts)
        C = R * length
        ri, ts, te = ri_b[:C], ts_b[:C], te_b[:C]
        ops.compact_ray_slots(ts_slots.view(-1), te_slots.view(-1), CAP, packed, ri, ts, te, slot_offset=off)
        n = int(total.item())
        evaluated += n
        sigma = torch.full((C,), float("nan"), device=dev)               # beyond the count: never read
        head = torch.full((C, 4), float("nan"), device=dev)
        sigma[:n] = _gather(packed, ri, n, off, sg_slots)
        head[:n] = _gather(packed, ri, n, off, rgb_slots)
        assert torch.equal(ts[:n], _gather(packed, ri, n, off, ts_slots))   # compact_ray_slots(slot_offset=...) itself
        next_len = sched[k + 1][1] if k + 1 < len(sched) else 0
        ops.eval_composite_segment(ts, te, sigma, head, packed, cnts, off + length, next_len, tau_stop, state,
                                   seg_cnts if next_len else None, nan_to_num=nan_to_num)
    return state, evaluated


def _finish(state, background, clamp):
    from lsenerf_amd import ops
    out = (torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda"),
           torch.empty(R, dtype=torch.int64, device="cuda"))
    ops.eval_composite_finish(state, *out, background=background, clamp=clamp)
    return out


def _full_arrays(scene):
    """The full route's packed arrays of the same scene: (ts, te, sigma, rgb [N, 4], packed_info)."""
    from lsenerf_amd import ops
    ts_h, te_h, sg_h, rgb_h, cnts_h = scene[:5]
    cnts = torch.from_numpy(cnts_h).cuda()
    packed, total = ops.pack_info_from_counts(cnts)
    n = int(total.item())
    ri = torch.empty(n, dtype=torch.int32, device="cuda")
    ts, te = torch.empty(n, device="cuda"), torch.empty(n, device="cuda")
    ops.compact_ray_slots(torch.from_numpy(ts_h).cuda().view(-1), torch.from_numpy(te_h).cuda().view(-1), CAP, packed, ri, ts, te)
    sigma = _gather(packed, ri, n, 0, torch.from_numpy(sg_h).cuda()).contiguous()
    rgb = _gather(packed, ri, n, 0, torch.from_numpy(rgb_h).cuda()).contiguous()
    return ts, te, sigma, rgb, packed


@pytest.mark.parametrize("eps", [1e-4, 1e-2, 0.5])
@pytest.mark.parametrize("S", [64, 128])
def test_segment_kernels_truncated_equality_termination_and_reproducibility(S, eps):
    from lsenerf_amd import ops
    tau_stop = ops.eval_tau_stop(eps)
    scene = _scene(S, tau_stop)
    ts_h, te_h, sg_h, rgb_h, cnts_h, pat, wall = scene
    bounds = schedule_boundaries(CAP, S)
    ts, te, sigma, rgb, packed = _full_arrays(scene)
    total = int(cnts_h.sum())
    counts = {}
    for nan_to_num in (False, True):
        state, evaluated = _run_segments(scene, S, tau_stop, nan_to_num)
        state2, _ = _run_segments(scene, S, tau_stop, nan_to_num)
        for background, clamp in ((None, False), (1.0, True), (0.0, False)):
            got = _finish(state, background, clamp)
            # -- reproducibility: a second run, bit for bit
            for a, b in zip(got, _finish(state2, background, clamp)):
                assert torch.equal(a, b) if a.dtype == torch.int64 else bits_equal(a, b)
            # -- truncated equality: lse_eval_composite on the same arrays, every ray cut at the returned count
            cut = packed.clone()
            cut[:, 1] = got[3]
            want = (torch.empty(R, 3, device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda"),
                    torch.empty(R, dtype=torch.int64, device="cuda"))
            ops.eval_composite(ts, te, sigma, rgb, cut, *want, nan_to_num=nan_to_num, background=background, clamp=clamp)
            for name, a, b in zip(("rgb", "acc", "depth"), got, want):
                assert bits_equal(a, b), (name, nan_to_num, background, clamp, (a - b).abs().nan_to_num().max().item())
            assert torch.equal(got[3], want[3])
            # -- rays without a sample: nothing accumulated, the background alone
            empty = torch.from_numpy(cnts_h == 0).cuda()
            assert torch.all(got[1][empty] == 0) and torch.all(got[0][empty] == (background or 0.0)) and torch.all(got[3][empty] == 0)
        m_all = _finish(state, None, False)[3].cpu().numpy()
        counts[nan_to_num] = m_all
        assert evaluated == sum(int(np.minimum(np.maximum(m_all - off, 0), length).sum())
                                for off, length in zip([0] + bounds[:-1], np.diff([0] + bounds)))   # exactly the samples composited
        assert evaluated < total                                      # the walls stop rays at every eps used here
        # an independent look at the values: float64, finite colours only (nan_to_num run), no epilogue.  4e-6: the weights of a
        # ray sum to at most 1 and the colours lie in [0, 1]; a weight's relative error is that of its transmittance -- the f32
        # optical depth in front of it, at most tau_stop + 0.4 < 10 before the stop, known to 7e-7 relative (the figure the
        # termination slack rests on) plus the roundings of two expf -- about 1e-6 of a sum <= 1, and 320 f32 additions add 320 * 2^-24
        if nan_to_num:
            rgb_out, acc_out, _, _ = _finish(state, None, False)
            for r in range(0, R, 7):
                c, a, _, _, _ = composite_first_m_numpy(ts_h[r], te_h[r], sg_h[r], rgb_h[r], int(m_all[r]), nan_to_num=True)
                if np.all(np.abs(c) < 1e30):
                    assert abs(acc_out[r].item() - a) <= 4e-6 and np.abs(rgb_out[r].cpu().numpy() - c).max() <= 4e-6, r
    assert np.array_equal(counts[False], counts[True])              # colours never decide where a ray stops
    # -- termination property against float64 prefix sums; no ray excluded
    m_all = counts[True]
    stopped_walls = 0
    for r in range(R):
        n, m = int(cnts_h[r]), int(m_all[r])
        tau = tau_prefix64(ts_h[r, :n], te_h[r, :n], sg_h[r, :n])
        assert m == n or m in bounds, (r, m, n)
        assert m <= n
        if m < n:
            assert tau[m] >= tau_stop * (1 - 1e-4), (r, m, tau[m])
        for b in bounds:
            if b < m:
                assert tau[b] <= tau_stop * (1 + 1e-4), (r, b, tau[b])
        if 1 <= pat[r] <= 8 and wall[r] < n:                         # a wall inside the ray: it stops where the wall's segment ends
            end = min(b for b in bounds if b > wall[r])
            assert m == min(end, n), (r, pat[r], wall[r], m, n)
            stopped_walls += m < n
        if pat[r] == 0 or (1 <= pat[r] <= 8 and wall[r] >= n):       # transparent: rendered in full
            assert m == n, (r, m, n)
        assert m == stop_count_numpy(tau, bounds, tau_stop), (r, m)   # (no tau of this scene lies within the slack of tau_stop)
    assert stopped_walls >= 20


# ----------------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------------
SEED_HALF = 5              # eps = 0.5, untrained field: 0.858 of the sampled rays stop early (seeds 1, 2, 3: 0.842, 0.850, 0.857)
OPAQUE_SCALE = 1.0e5       # hash-table parameters times this (the density is exp(logit), logit ~ 1e-5 before): found with one full
                           # render -- 1e4 and 3e4 stop no ray, 1e5 stops 0.844 of them (189670 of 295650 samples evaluated)


def _es_model(eps, seed=SEED_HALF, **kw):
    return _model(seed=seed, eval_early_stop_eps=eps, eval_segment_samples=64, **kw)


def _make_opaque(model):
    with torch.no_grad():
        model.field.mlp_base_grid.params.mul_(OPAQUE_SCALE)
    return model


def _reference_cut(model, bundle, nsamples):
    """The full march of every chunk, the field once over all its samples, then ``ops.eval_composite`` with every ray's count
    replaced by ``nsamples``: what the contract says the early-stop route returns, bit for bit."""
    from lsenerf_amd import ops
    from lsenerf_amd.evaluation import _flatten_bundle, _slice
    from lsenerf_amd.renderer import LinearRenderer
    cfg, fld = model.config, model.field
    rb = _flatten_bundle(bundle)
    n_rays = len(rb)
    rgb, acc, depth = torch.empty(n_rays, 3, device="cuda"), torch.empty(n_rays, device="cuda"), torch.empty(n_rays, device="cuda")
    ns = torch.empty(n_rays, dtype=torch.int64, device="cuda")
    linear = isinstance(model.renderer_rgb, LinearRenderer)
    bg = cfg.background_color
    background = None if bg in ("random", "last_sample") else {"black": 0.0, "white": 1.0}[bg]
    full_counts = []
    with torch.no_grad():
        for lo in range(0, n_rays, CHUNK):
            hi = min(n_rays, lo + CHUNK)
            part = _slice(rb, lo, hi)
            ri, ts, te, packed, n_dev = model.sampler.sample_packed(
                part, near_plane=cfg.near_plane, far_plane=cfg.far_plane, render_step_size=cfg.render_step_size,
                alpha_thre=cfg.alpha_thre, cone_angle=cfg.cone_angle)
            table, eidx = fld._eval_emb(hi - lo, "cuda") if fld.embedding_appearance is not None else (None, None)
            sigma, _, _, head = fld.density_rgb_packed(part.origins.contiguous(), part.directions.contiguous(), ri, ts, te, packed,
                                                       eidx, table, n_dev)
            full_counts.append(packed[:, 1].clone())
            cut = packed.clone()
            cut[:, 1] = nsamples.reshape(-1)[lo:hi]
            ops.eval_composite(ts, te, sigma, head, cut, rgb[lo:hi], acc[lo:hi], depth[lo:hi], ns[lo:hi], nan_to_num=not linear,
                               background=background, clamp=not linear)
        raw = {"rgb": rgb, "accumulation": acc[:, None], "depth": depth[:, None], "num_samples_per_ray": ns}
        out = {k: v for k, v in model.route_outputs(raw, rb).items() if torch.is_tensor(v)}
    return out, torch.cat(full_counts)


def _check_cut_equal(model, bundle, mapper_keys=(), exact=("rgb", "accumulation", "depth", "num_samples_per_ray")):
    from lsenerf_amd.evaluation import uses_count_free_route
    assert uses_count_free_route(model, H * W) and model.config.eval_early_stop_eps > 0
    out = model.get_outputs_for_camera_ray_bundle(bundle)
    ref, full_counts = _reference_cut(model, bundle, out["num_samples_per_ray"])
    assert set(out) == set(ref)
    for k in exact:
        got, want = out[k].reshape(H * W, -1), ref[k].reshape(H * W, -1)
        assert got.dtype == want.dtype
        ok = torch.equal(got, want) if got.dtype == torch.int64 else bits_equal(got, want)
        assert ok, (k, (got.float() - want.float()).abs().max().item())
    for k in mapper_keys:
        assert (out[k].reshape(H * W, -1) - ref[k].reshape(H * W, -1)).abs().max().item() <= 1e-6, k
    ns = out["num_samples_per_ray"].reshape(-1)
    assert torch.all(ns <= torch.maximum(full_counts, torch.ones_like(full_counts)))
    return out, full_counts


@pytest.mark.parametrize("eps", [0.5, 0.1])
def test_early_stop_cut_equal_default_renderer(eps):
    out, full = _check_cut_equal(_es_model(eps), _bundle())
    if eps == 0.5:             # (tau stays below -ln 0.1 = 2.3 on every ray of this untrained field: nothing stops at 0.1)
        assert int((out["num_samples_per_ray"].reshape(-1) < full).sum()) > 0


@pytest.mark.parametrize("eps", [0.5, 0.1])
def test_early_stop_cut_equal_white_background(eps):
    _check_cut_equal(_es_model(eps, background_color="white"), _bundle(seed=4))


@pytest.mark.parametrize("eps", [0.5, 0.1])
def test_early_stop_cut_equal_cone0_linear_co_map(eps, monkeypatch):
    from lsenerf_amd import model as M
    from lsenerf_amd.renderer import LinearRenderer
    monkeypatch.setattr(M.MLP_Mapper, "init_steps", 60)
    monkeypatch.setattr(M.RGB_MLP_Mapper, "init_steps", 60)
    m = _es_model(eps, cone_angle=0.0, use_mapping=True, mapping_method="rgb_mlp", map_mode="co_map", evs_mapping_method="mlp",
                  ev_one_dim="learned")
    assert isinstance(m.renderer_rgb, LinearRenderer)
    _check_cut_equal(m, _bundle(seed=2), mapper_keys=("rgb", "ev_out", "ev_linear"),
                     exact=("linear", "accumulation", "depth", "num_samples_per_ray"))


@pytest.mark.parametrize("eps", [0.5, 0.1])
def test_early_stop_cut_equal_embedding_mode_mean(eps):
    from lsenerf_amd import LSEEmbeddingConfig
    m = _es_model(eps, num_train_data=32, embed_config=LSEEmbeddingConfig(embedding_type="evs_emb", eval_mode="mean"))
    with torch.no_grad():
        m.field.embedding_appearance.embedding.weight.normal_(0.0, 0.5)
    _check_cut_equal(m, _bundle(seed=3))


@pytest.mark.parametrize("eps", [0.5, 0.1])
def test_early_stop_empty_middle_chunk_gets_the_fake_sample(eps):
    out, _ = _check_cut_equal(_es_model(eps), _bundle(seed=5, empty_chunk=1))
    ns = out["num_samples_per_ray"].reshape(-1)
    assert ns[CHUNK].item() == 1 and int(ns[CHUNK + 1:2 * CHUNK].sum().item()) == 0
    assert out["depth"].reshape(-1)[CHUNK].item() == 1.0
    assert int(ns[3 * CHUNK:].gt(0).sum().item()) > 0


def _stopped_share(model, bundle):
    """(share of the rays with samples that return fewer samples than the full route, outputs, full-route outputs)."""
    eps = model.config.eval_early_stop_eps
    out = model.get_outputs_for_camera_ray_bundle(bundle)
    model.config.eval_early_stop_eps = 0.0
    full = model.get_outputs_for_camera_ray_bundle(bundle)
    model.config.eval_early_stop_eps = eps
    n_es, n_full = out["num_samples_per_ray"].reshape(-1), full["num_samples_per_ray"].reshape(-1)
    assert torch.all(n_es <= n_full)
    has = n_full > 0
    return float((n_es < n_full)[has].float().mean().item()), out, full


def _check_close(out, full, eps):
    """The weight left behind a stopped ray is at most its transmittance at the stop, which is below eps (up to the f32 slack of the
    carried optical depth); colours lie in [0, 1] and the background is black."""
    bound = eps * (1 + 1e-3) + 1e-6
    d_rgb = (out["rgb"] - full["rgb"]).abs().max().item()
    d_acc = (full["accumulation"] - out["accumulation"]).reshape(-1)
    print(f"eps {eps}: max |rgb_es - rgb_full| {d_rgb:.3e}, acc_full - acc_es in [{d_acc.min().item():.3e}, {d_acc.max().item():.3e}]")
    assert d_rgb <= bound
    assert d_acc.min().item() >= -1e-6 and d_acc.max().item() <= bound


def test_it_actually_stops_rays_untrained_field_eps_half():
    """An untrained field has sigma ~ 1 and tau ~ 1 - 3 per ray in this scene: at eps = 0.5 (tau_stop = 0.69) a good part of the
    rays stops early, not all of them."""
    m = _es_model(0.5, background_color="black")
    share, out, full = _stopped_share(m, _bundle())
    print(f"seed {SEED_HALF}, eps 0.5: {share:.3f} of the sampled rays stop early")
    assert 0.20 <= share <= 0.95, share
    _check_close(out, full, 0.5)


def test_it_actually_stops_rays_opaque_field():
    """eps = 1e-4 on a field made opaque by scaling its hash-table parameters in place (OPAQUE_SCALE, found with one full render):
    at least half the rays stop before their last segment."""
    m = _make_opaque(_es_model(1e-4, background_color="black"))
    share, out, full = _stopped_share(m, _bundle())
    print(f"OPAQUE_SCALE {OPAQUE_SCALE}, eps 1e-4: {share:.3f} of the sampled rays stop early")
    assert share >= 0.5, share
    _check_close(out, full, 1e-4)
    _check_cut_equal(m, _bundle())


def test_early_stop_makes_no_host_sync(monkeypatch):
    """No sampler read-back per image (ops.SYNC_STATS), and nothing at all that waits for the device up to the one overflow read
    behind the last chunk: the render runs with torch's sync debug mode at "error" until then."""
    from lsenerf_amd import ops
    m, b = _es_model(0.5), _bundle(seed=6)
    m.get_outputs_for_camera_ray_bundle(b)          # warm
    torch.cuda.synchronize()
    grid = m.occupancy_grid
    orig, reached = grid.check_deferred_overflow, []

    def overflow_read():
        reached.append(torch.cuda.get_sync_debug_mode())
        torch.cuda.set_sync_debug_mode("default")
        orig()
    monkeypatch.setattr(grid, "check_deferred_overflow", overflow_read)
    c0 = ops.SYNC_STATS["count"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = m.get_outputs_for_camera_ray_bundle(b)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reached == [2]                            # the overflow read was reached once, with the mode still at "error"
    assert ops.SYNC_STATS["count"] == c0
    assert int(out["num_samples_per_ray"].sum().item()) > 0


def test_eps_zero_is_the_route_as_it_was():
    b = _bundle(seed=7)
    base = _model().get_outputs_for_camera_ray_bundle(b)
    off = _model(eval_early_stop_eps=0.0, eval_segment_samples=64).get_outputs_for_camera_ray_bundle(b)
    assert set(base) == set(off)
    for k in base:
        assert torch.equal(base[k], off[k]), k


def test_eps_is_ignored_where_the_count_free_route_is_not_available():
    """Training mode: ``forward`` per chunk, as with eps = 0 (same seeds: the training sampler draws its jitter)."""
    from lsenerf_amd.evaluation import uses_count_free_route
    b = _bundle(seed=8)
    m = _es_model(0.5, background_color="black").train()
    assert not uses_count_free_route(m, H * W)
    torch.manual_seed(11)
    got = m.get_outputs_for_camera_ray_bundle(b)
    m.config.eval_early_stop_eps = 0.0
    torch.manual_seed(11)
    want = m.get_outputs_for_camera_ray_bundle(b)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    m.occupancy_grid.check_deferred_overflow()
