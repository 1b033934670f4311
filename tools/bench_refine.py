"""The frozen-field refinement step against the only route the package had before it (R:scripts/emb_eval.sh: ~3000 steps that fit the
test appearance embedding, then ~6000 that optimise the evaluation cameras, the radiance field frozen in both).

Two workloads: bench.py's headline (4096 rays x ~1024 samples, constant step, no culling) and the reference's default batch (2316 +
597 + 597 = 3510 rays, cone 0.004, alpha_thre 0.01, carved 4-level grid, per-frame embedding with a test row).  Per workload, ms per
replay of three captured steps, interleaved rounds in one process:
  (i)   the training step with optimizer_in_graph=False (full backward, the field update thrown away),
  (ii)  the frozen camera-only step (freeze_field(train_embedding=False), ray gradients, no field optimiser),
  (iii) the frozen embedding-only step (freeze_field(), FlatAdam over the embedding, no ray gradients);
device time (HIP events) of lse_hash_fwd, lse_hash_bwd_ex and lse_hash_bwd_input on the step's own samples; and the share of (ii)
spent in its two lse_mlp_bwd launches, which still form the weight-gradient products of the frozen networks -- what a
data-gradient-only MLP backward could save at most.

The input-gradient-only MLP backward (freeze_field(input_only_mlp=True), lse_mlp_bwd_input) against that default route, A/B in the same
process with the routes alternating:
  kernels: inside the eager frozen camera-only step, on the very arguments of its two lse_mlp_bwd launches -- the head with d_in +
           d_row_bias, the head with d_row_bias alone (what the embedding-only phase asks for), the base -- lse_mlp_bwd (weight
           gradients into the scratch) and lse_mlp_bwd_input, two repeats of each (median of 8 timed calls);
  steps:   (ii) and (iii) captured once more with the flag, replayed in the same interleaved rounds.
Spread = the larger difference between the repeats (rounds) of either route; bar: new <= old - 2 x spread, for each comparison.

Exit status 1 when lse_hash_bwd_input takes longer than 1.5 x lse_hash_fwd on the same inputs in the same run (the two kernels issue
the same gathers and move the same bytes per sample; the factor covers three times the multiply-adds and the wider register
footprint), or when an A/B bar above is missed.  The other step-level ratios are reported, not barred.

Usage: python tools/bench_refine.py [--out profiles/refine_step.txt] [--replays 20] [--rounds 3]"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import torch

import bench
from lsenerf_amd import _lib, ops
from lsenerf_amd import model as M

BAR = 1.5
EXPECTED_II_OVER_I = 0.7      # 5.43 ms headline step - 2.47 ms scatter + ~0.6 ms for a gather the size of the forward (BENCH_r05.json)


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def headline_workload(device):
    model, sets, counts = bench.build_workload(device, seed=0)
    rb, target, _ = sets[0]
    return model, (rb, None, None), {"col_batch": {"image": target}, "evs_batch": None}, f"{len(rb)} rays, {counts[0]} samples"


def default_batch_workload(device):
    """bench.py's cfg3 composition with eval_mode "param": the presets the reference refines (lsenerf_emb, BADNERF_emb)."""
    from lsenerf_amd import LSEEmbeddingConfig, LSENeRFModel, LSENeRFModelConfig, RayBundle
    torch.manual_seed(96)
    cfg = LSENeRFModelConfig(use_mapping=True, mapping_method="identity", map_mode="co_map", evs_mapping_method="powpow",
                             embed_config=LSEEmbeddingConfig(embedding_type="evs_emb", eval_mode="param"))
    sizes, n_emb = (2316, 597, 597), 512
    model = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=n_emb).to(device).train()
    with torch.no_grad():
        model.field.mlp_base_grid.params.mul_(3000.0)
        model.field.mlp_base_mlp.params[-16 * 64:-15 * 64].mul_(6.0)
    model.init_test_params()
    g = torch.Generator().manual_seed(7)

    def bundle(o, d):
        n = o.shape[0]
        return RayBundle(origins=o.to(device), directions=d.to(device), camera_indices=torch.zeros(n, 1, dtype=torch.long, device=device),
                         metadata={"appearance_id": torch.randint(0, n_emb, (n,), generator=g).to(device)})
    o, d = bench.sphere_rays(sizes[0], g)
    col = bundle(o, d)
    o, d = bench.sphere_rays(sizes[1], g)
    prev = bundle(o, d)
    o2, d2 = o + 0.01 * torch.randn(o.shape, generator=g), d + 0.01 * torch.randn(d.shape, generator=g)
    nxt = bundle(o2, d2 / d2.norm(dim=-1, keepdim=True))
    batch = {"col_batch": {"image": torch.rand(sizes[0], 3, generator=g).to(device)},
             "evs_batch": {"image": ((torch.rand(sizes[1], 1, generator=g) - 0.5) * 0.4).to(device)}}
    for s in range(0, 64, 16):
        model.update_occupancy_grid(s)
    return model, (col, prev, nxt), batch, f"{sum(sizes)} rays ({sizes[0]} + {sizes[1]} + {sizes[2]})"


def step_samples(model, bundles):
    """(x01 [cap, 3], n_dev, count) of the samples the step's field pass sees for these bundles: the sampler with device-side counts
    (visibility pre-pass included) and the position kernel, as ``exec_get_outputs`` runs them."""
    from lsenerf_amd import RayBundle
    cfg, fld = model.config, model.field
    saved = model.deferred_max_slots
    model.deferred_max_slots = 1 << 62
    try:
        with torch.no_grad():
            rb = RayBundle.cat([b for b in bundles if b is not None])
            ri, ts, te, packed, n_dev = model.sampler.sample_packed(rb, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
                                                                    render_step_size=cfg.render_step_size, alpha_thre=cfg.alpha_thre,
                                                                    cone_angle=cfg.cone_angle)
            x01, _ = fld._x01(rb.origins.detach().contiguous(), rb.directions.detach().contiguous(), ri, ts, te, packed, n_dev)
    finally:
        model.deferred_max_slots = saved
        fld._prepass = None
    return x01, n_dev, int(n_dev)


def hash_kernel_times(model, bundles, rounds, iters=8):
    """Median device ms of the three hash kernels on the step's samples, interleaved rounds, one event pair per call."""
    x01, n_dev, count = step_samples(model, bundles)
    grid = model.field.mlp_base_grid
    meta, table = grid.meta, grid.params.detach()
    cap, L = x01.shape[0], meta.n_levels
    desc = meta.desc()
    y = torch.empty((L, cap, 2), device=x01.device)
    dy = torch.randn((L, cap, 2), device=x01.device)
    dt, dx = torch.zeros_like(table), torch.empty_like(x01)
    opts = ops.hash_bwd_opts_with_workspace(desc, x01.device)
    for k, v in meta.bwd_tuning:
        setattr(opts, k, v)
    st = ops._stream
    fns = {
        "lse_hash_fwd": lambda: _lib.call("lse_hash_fwd", ctypes.byref(desc), P(x01), P(table), P(y), cap, P(n_dev), st()),
        "lse_hash_bwd_ex": lambda: _lib.call("lse_hash_bwd_ex", ctypes.byref(desc), P(x01), P(dy), P(table), P(dt), P(dx), 0, 0, L, cap,
                                             P(n_dev), ctypes.byref(opts), st()),
        "lse_hash_bwd_input": lambda: _lib.call("lse_hash_bwd_input", ctypes.byref(desc), P(x01), P(dy), P(table), P(dx), cap, P(n_dev),
                                                st()),
    }
    times = {k: [] for k in fns}
    for f in fns.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for name, f in fns.items():
            for _ in range(iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); f(); e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
    return {k: statistics.median(v) for k, v in times.items()}, count, cap


def mlp_bwd_ms_of_an_eager_frozen_step(model, bundles, batch, steps=5):
    """Device ms per step inside lse_mlp_bwd (both launches) of the eager frozen camera-only step, and the launch count."""
    from lsenerf_amd import RayBundle
    per_step, launches = [], 0
    for it in range(steps):
        bs = [None if b is None else RayBundle(origins=b.origins.detach().clone().requires_grad_(True),
                                               directions=b.directions.detach().clone().requires_grad_(True), camera_indices=b.camera_indices,
                                               fars=b.fars, metadata=b.metadata) for b in bundles]
        _lib.TIMING = {"names": {"lse_mlp_bwd"}, "events": []}
        try:
            _, losses, _ = model.train_step_bundles(*bs, batch)
            sum(losses.values()).backward()
            torch.cuda.synchronize()
            ev = _lib.TIMING["events"]
        finally:
            _lib.TIMING = None
        if it >= 2:
            per_step.append(sum(e0.elapsed_time(e1) for _, e0, e1 in ev))
            launches = len(ev)
    return statistics.median(per_step), launches


def ab_verdict(old, new):
    """(old median, new median, spread, new <= old - 2 x spread) of two routes' repeats."""
    spread = max(max(old) - min(old), max(new) - min(new))
    o, n = statistics.median(old), statistics.median(new)
    return o, n, spread, n <= o - 2.0 * spread


def mlp_bwd_kernel_ab(model, bundles, batch, repeats=2, iters=8):
    """lse_mlp_bwd against lse_mlp_bwd_input on the arguments of the two lse_mlp_bwd launches of ONE eager frozen camera-only step
    (the default route): the launches are intercepted where they happen, so every operand is the step's own.  Returns
    {comparison: {"old": [ms per repeat], "new": [...]}}.  (The step's gradients are garbage afterwards: d_row_bias accumulates.)"""
    from lsenerf_amd import RayBundle
    out, real = {}, _lib.call

    def timed(f):
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); f(); e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts)

    def hook(name, *a):
        if name != "lse_mlp_bwd":
            return real(name, *a)
        (desc, params, x, _act, _tiled, o, oc, d_out, d_sig, sel, scale, _pre, _dact, _dact0, d_in, d_par, rb, idx, d_rb, n, n_dev, st) = a
        head = desc._obj.n_in == 16

        def routes(di):
            old = lambda: real("lse_mlp_bwd", desc, params, x, None, 3, o, oc, d_out, d_sig, sel, scale, None, None, None, di, d_par, rb, idx,
                               d_rb, n, n_dev, st)
            new = lambda: real("lse_mlp_bwd_input", desc, params, x, o, oc, d_out, d_sig, sel, scale, di, rb, idx, d_rb, n, n_dev, st)
            return {"old": old, "new": new}
        todo = {"head, d_in + d_row_bias": routes(d_in), "head, d_row_bias alone": routes(None)} if head else {"base, d_in": routes(d_in)}
        for what, fs in todo.items():
            res = {k: [] for k in fs}
            for f in fs.values():
                f(); f()
            for _ in range(repeats):
                for k, f in fs.items():      # the routes alternate
                    res[k].append(timed(f))
            out[what] = res
        return real(name, *a)

    bs = [None if b is None else RayBundle(origins=b.origins.detach().clone().requires_grad_(True),
                                           directions=b.directions.detach().clone().requires_grad_(True), camera_indices=b.camera_indices,
                                           fars=b.fars, metadata=b.metadata) for b in bundles]
    _lib.call = hook
    try:
        _, losses, _ = model.train_step_bundles(*bs, batch)
        sum(losses.values()).backward()
        torch.cuda.synchronize()
    finally:
        _lib.call = real
    for p in model.parameters():
        p.grad = None
    return out


def replay_ms(step, args, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        step(*args)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def run_workload(name, build, device, replays, rounds, log):
    from lsenerf_amd.graph import GraphedTrainStep
    from lsenerf_amd.optim import FlatAdam, FlatParams
    model, bundles, batch, what = build(device)
    args = (*bundles, batch)
    M.gbconfig.IS_EVAL = False
    opt_full = FlatAdam(FlatParams(model.get_param_groups()["fields"]), lr=1e-3, eps=1e-15)
    M.gbconfig.IS_EVAL = True            # the refinement run's setting: the training path reads the test embedding
    steps = {}
    steps["i"] = GraphedTrainStep(model, opt_full, *args, ray_grads=True, optimizer_in_graph=False)
    assert model.freeze_field(train_embedding=False) == []
    steps["ii"] = GraphedTrainStep(model, None, *args, ray_grads=True)
    mlp_ms, mlp_launches = mlp_bwd_ms_of_an_eager_frozen_step(model, bundles, batch)
    kernel_ab = mlp_bwd_kernel_ab(model, bundles, batch)
    model.unfreeze_field()
    assert model.freeze_field(train_embedding=False, input_only_mlp=True) == []
    steps["ii+"] = GraphedTrainStep(model, None, *args, ray_grads=True)
    model.unfreeze_field()
    left = model.freeze_field()
    opt_emb = FlatAdam(FlatParams(left), lr=1e-3, eps=1e-15)
    steps["iii"] = GraphedTrainStep(model, opt_emb, *args, ray_grads=False)
    model.unfreeze_field()
    assert [id(p) for p in model.freeze_field(input_only_mlp=True)] == [id(p) for p in left]
    steps["iii+"] = GraphedTrainStep(model, opt_emb, *args, ray_grads=False)      # (the same embedding optimiser: timing only)
    for s in steps.values():
        replay_ms(s, args, 5)
    ms = {k: [] for k in steps}
    for _ in range(rounds):
        for k, s in steps.items():
            ms[k].append(replay_ms(s, args, replays))
    for s in steps.values():
        s.check_overflow()
    step_ms = {k: statistics.median(v) for k, v in ms.items()}
    kern, count, cap = hash_kernel_times(model, bundles, rounds)
    for s in steps.values():
        s.close()
    model.unfreeze_field()
    M.gbconfig.IS_EVAL = False
    ratio = kern["lse_hash_bwd_input"] / kern["lse_hash_fwd"]
    log(f"== {name}: {what}; {count} samples in the field pass (capacity {cap}), {len(left)} trainable embedding tensor(s)")
    log(f"  (i)   training step, optimizer_in_graph=False      {step_ms['i']:8.3f} ms per replay   rounds {['%.3f' % v for v in ms['i']]}")
    log(f"  (ii)  frozen, camera-only (ray gradients)          {step_ms['ii']:8.3f} ms per replay   rounds {['%.3f' % v for v in ms['ii']]}")
    log(f"  (iii) frozen, embedding-only                       {step_ms['iii']:8.3f} ms per replay   rounds {['%.3f' % v for v in ms['iii']]}")
    log(f"  (ii)/(i) = {step_ms['ii'] / step_ms['i']:.3f}   (expected near {EXPECTED_II_OVER_I} at the headline size: the recorded 5.43 ms step loses "
        f"its 2.47 ms scatter and gains a gather of about the forward's 0.6 ms)      (iii)/(i) = {step_ms['iii'] / step_ms['i']:.3f}")
    for k in ("lse_hash_fwd", "lse_hash_bwd_ex", "lse_hash_bwd_input"):
        log(f"  {k:20s} {kern[k]:8.4f} ms   (device events, the step's own samples, median of {rounds} interleaved rounds)")
    log(f"  lse_hash_bwd_input / lse_hash_fwd = {ratio:.3f}   (bar {BAR})")
    log(f"  lse_mlp_bwd in the eager frozen camera-only step: {mlp_launches} launches, {mlp_ms:.3f} ms = {100 * mlp_ms / step_ms['ii']:.1f} % of (ii) "
        f"-- the ceiling of what a data-gradient-only MLP backward could save")
    ok = True
    log("  input-gradient-only MLP backward, kernels on the step's own arguments (ms; repeats alternate old, new, old, new):")
    for what, r in kernel_ab.items():
        o, n, spread, good = ab_verdict(r["old"], r["new"])
        ok &= good
        log(f"    {what:26s} lse_mlp_bwd {['%.4f' % v for v in r['old']]}  lse_mlp_bwd_input {['%.4f' % v for v in r['new']]}  "
            f"new/old = {n / o:.3f}  spread {spread:.4f}  bar new <= {o - 2 * spread:.4f}: {'met' if good else 'MISSED'}")
    log("  the same through the captured steps (flag = freeze_field(input_only_mlp=True); rounds interleaved with the ones above):")
    for what, a, b in (("(ii)  camera-only", "ii", "ii+"), ("(iii) embedding-only", "iii", "iii+")):
        o, n, spread, good = ab_verdict(ms[a], ms[b])
        ok &= good
        log(f"    {what:22s} default {['%.3f' % v for v in ms[a]]}  flag {['%.3f' % v for v in ms[b]]}  saved {o - n:.3f} ms "
            f"(new/old = {n / o:.3f})  spread {spread:.3f}  bar: {'met' if good else 'MISSED'}"
            + (f"  = {100 * (o - n) / mlp_ms:.0f} % of this run's {mlp_ms:.3f} ms ceiling" if a == "ii" else ""))
    return ratio, ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_step.txt"))
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_refine.py measures on the GPU: none found")
    device = torch.device("cuda", 0)
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)
    log(f"tools/bench_refine.py --replays {a.replays} --rounds {a.rounds}   ({torch.cuda.get_device_name(0)})")
    ratios, ab_ok = {}, {}
    try:
        for name, build in (("headline workload", headline_workload), ("reference default batch", default_batch_workload)):
            ratios[name], ab_ok[name] = run_workload(name, build, device, a.replays, a.rounds, log)
    finally:
        M.gbconfig.IS_EVAL = False
    ok = all(r <= BAR for r in ratios.values())
    log(("PASS" if ok else "FAIL") + f": lse_hash_bwd_input <= {BAR} x lse_hash_fwd on both workloads: " +
        ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    log(("PASS" if all(ab_ok.values()) else "FAIL") + ": lse_mlp_bwd_input <= lse_mlp_bwd - 2 x spread, kernels and steps: " +
        ", ".join(f"{k} {'met' if v else 'missed'}" for k, v in ab_ok.items()))
    ok = ok and all(ab_ok.values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
