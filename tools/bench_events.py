#!/usr/bin/env python3
"""Event synthesis (lsenerf_amd.events, csrc/events.hip) stage by stage -- count, append (walk + ordered stream) and accumulate into
11 frames -- as (b) the package's entry points against (a) the same stage written with torch ops on the device (they live here, not
in the package): a masked vectorised loop for the counts, ``cumsum`` offsets and one masked scatter per emission index for the
ordered stream, ``bucketize`` + ``index_add_`` for the frames.  Two inputs of 640 x 480 pixels and K = 32 intervals:
  synthetic   a random walk of log intensity, L = -2 + cumsum(normal(0, 0.35))
  rendered    ``log_intensity_planes`` of the bench.py workload's field (the set-up of tools/bench_eval_set.py) along 33 poses of an
              orbit; the time of the renders is reported beside the stages
The threshold comes from the planes -- synthetic: 1.2 x the mean absolute plane-to-plane change, which gives about 0.5 events per
item on such a walk; rendered: the median non-zero plane-to-plane change, as in tests/test_gpu_events.py -- and is printed with the
events per item.  All outputs of the two routes are asserted equal -- counts, levels, totals, the stream bit for bit, the
frames -- before anything is timed.  Then the routes alternate in one process: one warm-up each, REPEATS timed repeats each, HIP
events around every stage; a repeat is the mean of 5 calls back to back.  ``spread`` = the largest difference between two repeats of
a route.

One JSON line per measurement, also appended to ``--out FILE`` when given.  Exit status 1 unless, for every stage of every input,
    package <= torch_ops - 2 spread.
usage: python tools/bench_events.py [--out FILE] [--repeats 2] [--skip-rendered]"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--skip-rendered", action="store_true")
args = ap.parse_args()
sys.argv = sys.argv[:1]                     # (bench_eval_set reads its own argv)
import numpy as np
import torch
from lsenerf_amd import ops

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
H, W, K, FRAMES, CAP_STEP = 480, 640, 32, 11, 127
INNER = 5
P = H * W
STAGES = ("count", "append", "accumulate")


def emit_line(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def timed(fn):
    """ms per call of ``fn``: INNER calls back to back between two HIP events (a stage of a fraction of a millisecond is otherwise
    a measurement of the clock and of the allocator)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(INNER):
        out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b) / INNER


# ---- (a) the stages with torch ops ------------------------------------------------------------------------------------------------
def torch_walk(L, ref_in, c_pos, c_neg, cap_step):
    """``(counts [K, P], ref_out, total, starts [K, P])``: per interval a loop over the emission index, masked."""
    ref = ref_in.clone()
    counts = torch.empty((L.shape[0] - 1, L.shape[1]), dtype=torch.int32, device=L.device)
    starts = torch.empty_like(counts, dtype=torch.float32)
    for k in range(L.shape[0] - 1):
        L1 = L[k + 1]
        starts[k] = ref
        up = (L1 - ref) >= c_pos
        down = ~up & ((ref - L1) >= c_neg)
        n = torch.zeros_like(counts[k])
        for _ in range(cap_step):
            go_up = up & ((L1 - ref) >= c_pos)
            go_down = down & ((ref - L1) >= c_neg)
            go = go_up | go_down
            if not bool(go.any()):
                break
            ref = torch.where(go_up, ref + c_pos, torch.where(go_down, ref - c_neg, ref))
            n += go
        ref = torch.where(n == cap_step, L1, ref)
        counts[k] = torch.where(up, n, -n)
    return counts, ref, counts.abs().sum(dtype=torch.int64), starts


def torch_append(L, times, ref_in, c_pos, c_neg, cap_step):
    """The walk, then the ordered stream: exclusive ``cumsum`` offsets per item, one masked scatter per emission index."""
    counts, ref_out, total, starts = torch_walk(L, ref_in, c_pos, c_neg, cap_step)
    n = counts.reshape(-1).abs().to(torch.int64)
    offs = torch.cumsum(n, 0) - n
    m = int(total)
    x = torch.empty(m, dtype=torch.int16, device=L.device)
    y = torch.empty(m, dtype=torch.int16, device=L.device)
    t = torch.empty(m, dtype=torch.float64, device=L.device)
    p = torch.empty(m, dtype=torch.int8, device=L.device)
    level = starts.reshape(-1).clone()
    sgn = torch.sign(counts.reshape(-1)).to(torch.int8)
    L0, L1 = L[:-1].reshape(-1), L[1:].reshape(-1)
    t0 = times[:-1, None].expand(-1, L.shape[1]).reshape(-1)
    dt = (times[1:] - times[:-1])[:, None].expand(-1, L.shape[1]).reshape(-1)
    idx = torch.nonzero(n > 0)[:, 0]
    e = 0
    while idx.numel():
        up = sgn[idx] > 0
        lv = torch.where(up, level[idx] + c_pos, level[idx] - c_neg)
        level[idx] = lv
        l0 = L0[idx]
        d = L1[idx] - l0
        q = ((lv - l0).double() / d.double()).float()
        frac = torch.where((d == 0) | torch.isnan(q), torch.zeros_like(q), q.clamp(0.0, 1.0))
        rows = offs[idx] + e
        t[rows] = t0[idx] + frac.double() * dt[idx]
        pix = idx % L.shape[1]
        x[rows] = (pix % W).to(torch.int16)
        y[rows] = (pix // W).to(torch.int16)
        p[rows] = sgn[idx]
        e += 1
        idx = idx[n[idx] > e]
    return counts, ref_out, total, (x, y, t, p)


def torch_accumulate(ev, bounds):
    x, y, t, p = ev
    F = bounds.shape[0] - 1
    f = torch.bucketize(t, bounds, right=True) - 1
    ok = (t >= bounds[0]) & (t < bounds[F]) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    flat = ((f * H + y.to(torch.int64)) * W + x.to(torch.int64))[ok]
    acc = torch.zeros(F * H * W, dtype=torch.int32, device=t.device)
    acc.index_add_(0, flat, p[ok].to(torch.int32))
    return acc.view(F, H, W)


# ---- (b) the package --------------------------------------------------------------------------------------------------------------
def package_append(L, times, ref_in, c_pos, c_neg, cap_step, cap, ws):
    bufs = [torch.empty(cap, dtype=dt, device=dev) for dt in (torch.int16, torch.int16, torch.float64, torch.int8)]
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    counts = torch.empty((K, P), dtype=torch.int32, device=dev)
    ref_out = ops.event_append(L, times, W, ref_in, c_pos, c_neg, cap_step, *bufs, total, counts=counts, workspace=ws)
    return counts, ref_out, total, tuple(bufs)


def package_accumulate(ev, bounds):
    acc = torch.zeros((bounds.shape[0] - 1, H, W), dtype=torch.int32, device=dev)
    return ops.event_accumulate(*ev, bounds, acc)


def run_case(name, L, thr, extra):
    times = torch.from_numpy(5.0 + np.arange(K + 1, dtype=np.float64) / 240.0).to(dev)
    bounds = torch.from_numpy(np.linspace(5.0, 5.0 + K / 240.0, FRAMES + 1)).to(dev)
    thr = float(np.float32(thr))
    ref_in = L[0].clone()
    ws = torch.empty(ops.event_workspace_bytes(K, P), dtype=torch.uint8, device=dev)
    # the two routes give the same outputs
    a_counts, a_ref, a_total, a_ev = torch_append(L, times, ref_in, thr, thr, CAP_STEP)
    n = int(a_total)
    b_counts, b_ref, b_total, b_ev = package_append(L, times, ref_in, thr, thr, CAP_STEP, n, ws)
    c_counts, c_ref, c_total = ops.event_count(L, ref_in, thr, thr, CAP_STEP)
    assert int(b_total) == n == int(c_total), (n, int(b_total), int(c_total))
    assert torch.equal(a_counts, b_counts) and torch.equal(a_counts, c_counts), "the routes give different counts"
    assert torch.equal(a_ref.view(torch.int32), b_ref.view(torch.int32)) and torch.equal(b_ref.view(torch.int32), c_ref.view(torch.int32))
    for u, v, what in zip(a_ev, b_ev, "xytp"):
        assert torch.equal(u.view(torch.int64) if what == "t" else u, v.view(torch.int64) if what == "t" else v), f"stream {what}"
    a_acc, b_acc = torch_accumulate(a_ev, bounds), package_accumulate(b_ev, bounds)
    assert torch.equal(a_acc, b_acc), "the routes give different frames"
    routes = {
        "torch_ops": {"count": lambda: torch_walk(L, ref_in, thr, thr, CAP_STEP), "append": lambda: torch_append(L, times, ref_in, thr, thr, CAP_STEP),
                      "accumulate": lambda: torch_accumulate(a_ev, bounds)},
        "package": {"count": lambda: ops.event_count(L, ref_in, thr, thr, CAP_STEP),
                    "append": lambda: package_append(L, times, ref_in, thr, thr, CAP_STEP, n, ws),
                    "accumulate": lambda: package_accumulate(b_ev, bounds)}}
    ms = {r: {s: [] for s in STAGES} for r in routes}
    for rep in range(args.repeats + 1):                  # the first round warms up
        for r, stages in routes.items():
            for s in STAGES:
                _, t = timed(stages[s])
                if rep:
                    ms[r][s].append(t)
    ok = True
    row = {"what": name, "pixels": P, "intervals": K, "frames": FRAMES, "threshold": thr, "events": n,
           "events_per_item": round(n / (K * P), 4), "largest_count": int(a_counts.abs().max()), "repeats": args.repeats,
           "calls_per_repeat": INNER, "outputs_equal": True, **extra}
    for s in STAGES:
        a, b = ms["torch_ops"][s], ms["package"][s]
        spread = max(max(a) - min(a), max(b) - min(b))
        a_ms, b_ms = sum(a) / len(a), sum(b) / len(b)
        passed = bool(b_ms <= a_ms - 2 * spread)
        ok = ok and passed
        row[s] = {"torch_ops_ms": round(a_ms, 3), "package_ms": round(b_ms, 3), "spread_ms": round(spread, 3),
                  "torch_ops_runs": [round(v, 3) for v in a], "package_runs": [round(v, 3) for v in b],
                  "ratio": round(b_ms / a_ms, 4), "bar_b_le_a_minus_2_spread": passed}
    if "render_ms_for_the_planes" in extra:
        pk = sum(row[s]["package_ms"] for s in ("append", "accumulate"))
        row["package_append_and_accumulate_share_of_render_plus_them"] = round(pk / (pk + extra["render_ms_for_the_planes"]), 5)
    emit_line(row)
    return ok


with torch.no_grad():
    g = torch.Generator(device=dev).manual_seed(0)
    walk = (-2.0 + torch.cumsum(torch.randn((K + 1, P), generator=g, device=dev, dtype=torch.float64) * 0.35, dim=0)).float()
    step = lambda planes: (planes[1:] - planes[:-1]).abs().double()
    ok = run_case("synthetic", walk.contiguous(), 1.2 * float(step(walk).mean()), {})
    if not args.skip_rendered:
        from bench_eval_set import H as BH, W as BW, model
        from lsenerf_amd.cameras import EdCameras
        from lsenerf_amd.events import log_intensity_planes
        assert (BH, BW) == (H, W)
        poses = []
        for k in range(K + 1):                           # 33 poses of an orbit: 0.2 rad of the ring of bench_eval_set
            a = 0.2 * k / K
            pos = torch.tensor([2.5 * math.cos(a), 0.6 * math.sin(2 * a), 2.5 * math.sin(a)], dtype=torch.float64)
            back = pos / pos.norm()
            right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), back)
            right = right / right.norm()
            poses.append(torch.stack([right, torch.linalg.cross(back, right), back, pos], dim=1).float())
        poses = torch.stack(poses)
        cams = EdCameras(poses, fx=400.0, fy=400.0, cx=W / 2, cy=H / 2, width=W, height=H)
        render_ms = []
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            planes = log_intensity_planes(model, cams, poses)
            torch.cuda.synchronize()
            render_ms.append((time.perf_counter() - t0) * 1e3)
        moved = step(planes)
        ok = run_case("rendered", planes, float(moved[moved > 0].median()), {"render_ms_for_the_planes": round(render_ms[-1], 1),
                                           "render_ms_runs": [round(v, 1) for v in render_ms]}) and ok
emit_line({"ok": ok})
sys.exit(0 if ok else 1)
