"""What one occupancy-grid refresh costs, by route.  Not the contract benchmark: bench.py stays the number of
record.

On the carved 4-level 128^3 grid of tools/bench_context.py (same model, same field scaling, same carving), in ONE process and
alternating, three routes of the same update rule:
  eager    ``LSEOccGridEstimator._update`` (torch index generation, several host synchronisations)
  device   ``DeviceGridRefresher.refresh`` launched eagerly (csrc/occ_refresh.hip, no synchronisation)
  graphed  the same after ``capture()``: one HIP graph replay
for both branches of the rule (warm-up: every cell; sampled: C/4 uniform + up to C/4 occupied cells per level).  Every route starts
from the same carved state.  Per route: the median device time of a refresh (a HIP event pair around each) and the host time per
refresh (perf_counter around the loop, no synchronise inside it).  The eager route runs twice, first and last: the difference of its
two medians is the run-to-run spread the others are judged against.
BAR (exit status 1 when missed): graphed device time <= eager median + 2 * spread, per branch -- the field inference is the same work;
what the device route buys is host time and capturability.  The host-time ratio is reported, not judged.

Then the default-config training step as one replayed graph (4096 rays, pre-pass on), 64 steps from the same training state with
``update_occupancy_grid`` in front of every step (4 of the 64 refresh), once per refresh route: device time per step (events around
the 64 steps, refreshes included) and host time per step.

Usage: python tools/bench_occ_refresh.py [--refreshes 20] [--warmup 3] [--rays 4096] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def build(dev, rays):
    """Model, optimizer, rays and target of tools/bench_context.py, with the grid carved by the reference's update rule."""
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, RayBundle
    from lsenerf_amd.optim import FlatAdam, FlatParams
    torch.manual_seed(96)
    cfg = LSENeRFModelConfig()
    model = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=64).to(dev)
    model.train()
    with torch.no_grad():
        model.field.mlp_base_grid.params.mul_(3000.0)
        model.field.mlp_base_mlp.params[-16 * 64:-15 * 64].mul_(6.0)
    opt = FlatAdam(FlatParams(model.get_param_groups()["fields"]), lr=1e-3, eps=1e-15)
    g = torch.Generator().manual_seed(7)
    o = torch.randn(rays, 3, generator=g)
    o = 1.5 * o / o.norm(dim=-1, keepdim=True)
    d = torch.rand(rays, 3, generator=g) - 0.5 - o
    d = d / d.norm(dim=-1, keepdim=True)
    rb = RayBundle(origins=o.to(dev), directions=d.to(dev), camera_indices=torch.zeros(rays, 1, dtype=torch.long, device=dev),
                   metadata={"appearance_id": torch.randint(0, 64, (rays,), generator=g).to(dev)})
    target = torch.rand(rays, 3, generator=g).to(dev)
    for step in range(0, 64, 16):
        model.update_occupancy_grid(step)
    return model, opt, rb, target


def snapshot(model, opt):
    est = model.occupancy_grid
    return (opt.flat.data.clone(), opt.exp_avg.clone(), opt.exp_avg_sq.clone(), opt.step_count, est.occs.clone(), est.binaries.clone())


def restore(model, opt, snap):
    est = model.occupancy_grid
    with torch.no_grad():
        opt.flat.data.copy_(snap[0]); opt.exp_avg.copy_(snap[1]); opt.exp_avg_sq.copy_(snap[2])
        opt.step_count = snap[3]
        est.occs.copy_(snap[4]); est.binaries.copy_(snap[5])
    est._bump_grid_version()
    est._invalidate_occ_mean()


def time_route(fn, steps, n_warm):
    """``fn(step)`` over ``steps``: (median device ms of a call, host ms per call); the first ``n_warm`` calls are not timed."""
    for s in steps[:n_warm]:
        fn(s)
    torch.cuda.synchronize()
    pairs = []
    t0 = time.perf_counter()
    for s in steps[n_warm:]:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(s)
        e1.record()
        pairs.append((e0, e1))
    host = time.perf_counter() - t0
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in pairs), host / len(pairs) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--refreshes", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_occ_refresh.py needs the GPU (no CPU fallback for the product path)"
    from lsenerf_amd.graph import GraphedTrainStep
    from lsenerf_amd.occ_refresh import DeviceGridRefresher
    dev = torch.device("cuda", 0)
    model, opt, rb, target = build(dev, args.rays)
    est, rss = model.occupancy_grid, model.config.render_step_size
    occ_frac = float(est.binaries.float().mean())
    snap = snapshot(model, opt)
    eager = lambda s: est._update(step=s, occ_eval_fn=lambda x: model.field.density_fn(x) * rss)
    plain = DeviceGridRefresher(est, model.field, rss)
    graphed = DeviceGridRefresher(est, model.field, rss).capture()
    n = args.warmup + args.refreshes
    result = {"context": "carved 4-level 128^3 grid of tools/bench_context.py", "occupied_fraction": occ_frac,
              "refreshes_per_route": args.refreshes, "branches": {}}
    ok = True
    for branch, steps in (("warmup", [16 * (k % 16) for k in range(n)]), ("sampled", [256 + 16 * k for k in range(n)])):
        rows = {}
        for name, fn in (("eager_first", eager), ("device", plain.refresh), ("graphed", graphed.refresh), ("eager_last", eager)):
            restore(model, opt, snap)
            dev_ms, host_ms = time_route(fn, steps, args.warmup)
            rows[name] = {"device_ms_median": round(dev_ms, 4), "host_ms_per_refresh": round(host_ms, 4)}
        a, b = rows["eager_first"]["device_ms_median"], rows["eager_last"]["device_ms_median"]
        eager_med, spread = statistics.median([a, b]), abs(a - b)
        bar = eager_med + 2 * spread
        met = rows["graphed"]["device_ms_median"] <= bar
        ok = ok and met
        eager_host = (rows["eager_first"]["host_ms_per_refresh"] + rows["eager_last"]["host_ms_per_refresh"]) / 2
        rows["summary"] = {"eager_device_ms": round(eager_med, 4), "eager_spread_ms": round(spread, 4), "bar_ms": round(bar, 4),
                           "graphed_device_ms": rows["graphed"]["device_ms_median"], "bar_met": met,
                           "host_ratio_eager_over_graphed": round(eager_host / rows["graphed"]["host_ms_per_refresh"], 2),
                           "host_ratio_eager_over_device": round(eager_host / rows["device"]["host_ms_per_refresh"], 2)}
        result["branches"][branch] = rows

    # ---- the graphed default-config training step with each refresh route in front of it
    restore(model, opt, snap)
    step = GraphedTrainStep(model, opt, rb, None, None, {"col_batch": {"image": target}, "evs_batch": None})
    train = {}
    for name in ("eager", "device", "graphed", "eager_again"):
        restore(model, opt, snap)
        model.config.device_grid_refresh = not name.startswith("eager")
        model.__dict__["_grid_refresher"] = {"device": plain, "graphed": graphed}.get(name)

        def run(first, count):
            for s in range(first, first + count):
                model.update_occupancy_grid(s)
                step(rb, None, None, {"col_batch": {"image": target}, "evs_batch": None})
        run(256 + 1, 15)                                         # (no refresh among these: warms the replay)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        run(256 + 16, 64)                                        # refreshes at 272, 288, 304, 320
        e1.record()
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        train[name] = {"device_ms_per_step": round(e0.elapsed_time(e1) / 64, 4), "host_ms_per_step": round(host / 64 * 1e3, 4)}
    model.config.device_grid_refresh = False
    step.check_overflow()
    step.close()
    result["graphed_train_step_64_steps_4_refreshes"] = train
    result["bar_met"] = ok
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
