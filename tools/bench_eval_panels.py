#!/usr/bin/env python3
"""Saving the images of an eval set: (a) what a caller of ``evaluate_set(on_image=...)`` had to do -- the reference writer's
conversion (R:lse_nerf/lse_writer.py:32-64: ``clamp(v * 255, 0, 255).cpu().type(uint8)`` per key but "accumulation", one channel
tiled to three, concatenated along the width) inside the callback -- against (b) ``evaluate_set(panels=PanelSet(...))`` without the
overlay column (the same picture, as uint8 from one launch and one asynchronous copy per image) and (b+) with the overlay (Canny
edges of both images; no counterpart in (a): OpenCV is not installed).  Scene and protocol of tools/bench_eval_set.py: 8 cameras of
640 x 480 around the bench.py workload's field; per route a warm-up set and two timed sets, the whole thing twice.

Per route and repeat one JSON line (wall ms per image); then per route the host waits per set (a pass of its own under
``torch.cuda.set_sync_debug_mode("warn")``) and the summed HIP-event time of the new launches per image, split by entry point (a
pass of its own).  The bar: wall(b) <= wall(a) - 2 * spread, spread = the larger difference between a route's two repeats, (a) and
(b) considered.  It is this tool's exit status.
usage: python tools/bench_eval_panels.py"""
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
import bench_eval_set as base          # the field, the cameras and the eval set of that tool
from lsenerf_amd import PanelSet, _lib, ops

model, eval_set, N_CAM = base.model, base.eval_set, base.N_CAM
SKIP = ("accumulation",)
NEW_CALLS = ("lse_gray8_planes", "lse_canny_u8", "lse_eval_panels")
saved = [None] * N_CAM


def writer_callback(i, outputs, images):
    parts = []
    for k, v in images.items():
        if k in SKIP:
            continue
        data = torch.clamp(v * 255, 0, 255).cpu().type(torch.uint8)
        parts.append(data if data.shape[-1] == 3 else torch.tile(data, (1, 1, 3)))
    saved[i] = torch.cat(parts, dim=1)


panels_plain = PanelSet(eval_set, keys=("img", "depth", "err_map", "ev_out"))
panels_overlay = PanelSet(eval_set)
ROUTES = {"a_on_image_writer_conversion": lambda: model.evaluate_set(eval_set, on_image=writer_callback),
          "b_panel_set": lambda: model.evaluate_set(eval_set, panels=panels_plain),
          "b_plus_panel_set_with_overlay": lambda: model.evaluate_set(eval_set, panels=panels_overlay)}


def timed(fn, sets=2):
    fn()                                                      # warm-up set
    wall = []
    for _ in range(sets):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / N_CAM)
    return wall


walls = {name: [] for name in ROUTES}
for repeat in range(2):
    for name, fn in ROUTES.items():
        wall = timed(fn)
        walls[name].append(sum(wall) / len(wall))
        print(json.dumps({"route": name, "repeat": repeat, "wall_ms_per_image": round(walls[name][-1], 3),
                          "wall_ms_per_image_sets": [round(w, 3) for w in wall]}), flush=True)

for name, fn in ROUTES.items():
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fn()
    torch.cuda.set_sync_debug_mode("default")
    waits = sum("synchroniz" in str(w.message).lower() for w in caught)
    _lib.TIMING = {"names": set(NEW_CALLS), "events": []}
    fn()
    torch.cuda.synchronize()
    events, _lib.TIMING = _lib.TIMING["events"], None
    split = {n: round(sum(e0.elapsed_time(e1) for m, e0, e1 in events if m == n) / N_CAM, 4) for n in NEW_CALLS}
    print(json.dumps({"route": name, "waits_per_set": waits, "new_launch_ms_per_image": round(sum(split.values()), 4),
                      "new_launch_ms_per_image_by_call": split}), flush=True)

# the overlay's Canny by stage, on the grey pair of the last image: 20 calls each between two HIP events
gray = panels_overlay._gray
classes = ops.canny_classify(gray)
stage_ms = {}
for stage, call in (("lse_canny_classify", lambda: ops.canny_classify(gray, out=classes)),
                    ("lse_canny_hysteresis", lambda: ops.canny_hysteresis(classes, out=panels_overlay._edges,
                                                                          workspace=panels_overlay._canny_ws))):
    call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        call()
    e1.record()
    torch.cuda.synchronize()
    stage_ms[stage] = round(e0.elapsed_time(e1) / 20, 4)
print(json.dumps({"canny_ms_per_image_pair_by_stage": stage_ms,
                  "edge_fraction_gt_pred": [round(float((e > 0).float().mean()), 4) for e in panels_overlay._edges]}), flush=True)

# the two routes save the same picture (to the rule of tests/test_gpu_panels.py: at most one level apart)
worst = max(int((saved[i].to(torch.int32) - panels_plain.host[i].to(torch.int32)).abs().max()) for i in range(N_CAM))
mean = {name: sum(w) / len(w) for name, w in walls.items()}
spread = max(abs(walls[name][0] - walls[name][1]) for name in ("a_on_image_writer_conversion", "b_panel_set"))
a, b = mean["a_on_image_writer_conversion"], mean["b_panel_set"]
ok = b <= a - 2 * spread
print(json.dumps({"wall_ms_per_image": {k: round(v, 3) for k, v in mean.items()}, "spread_ms": round(spread, 3),
                  "bar_b_le_a_minus_2_spread": bool(ok), "a_minus_b_ms": round(a - b, 3), "max_level_difference_a_vs_b": worst,
                  "overlay_cost_ms_per_image": round(mean["b_plus_panel_set_with_overlay"] - b, 3)}), flush=True)
sys.exit(0 if ok else 1)
