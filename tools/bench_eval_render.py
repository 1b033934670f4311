#!/usr/bin/env python3
"""Whole-image eval render: the eager loop a user writes today (``model(chunk)`` in eval mode, chunk by chunk) against
``LSENeRFModel.get_outputs_for_camera_ray_bundle`` (count-free sampling + lse_eval_composite, no host sync inside the loop), on one
640 x 480 camera of the bench.py workload (bench.build_workload: same seeded parameters and grid, same calibrated step size) at the
chunk sizes 128 / 2048 / 3512 (the reference's eval scripts and its eval_num_rays_per_chunk).  Asserts that both routes give the same
rgb / accumulation / depth / num_samples_per_ray bit for bit, then prints one JSON line per chunk size: ms per image (device events,
after a warm-up image), samples/s, and host syncs per image (ops.SYNC_STATS).  usage: python tools/bench_eval_render.py [images]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from lsenerf_amd import ops
from lsenerf_amd.cameras import EdCameras
from lsenerf_amd.evaluation import _flatten_bundle, _slice, uses_count_free_route

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
IMAGES = int(sys.argv[1]) if len(sys.argv) > 1 else 2
H, W = 480, 640
KEYS = ("rgb", "accumulation", "depth", "num_samples_per_ray")

model, _, _ = bench.build_workload(dev, seed=0)
model.eval()
# a camera 2.5 units from the centre of the [-1, 1]^3 box, looking at it (OpenGL frame: -z forward)
c2w = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.5]]])
cams = EdCameras(c2w, fx=400.0, fy=400.0, cx=W / 2, cy=H / 2, width=W, height=H)
rb = cams.generate_rays(torch.zeros(H * W, dtype=torch.long), cams.get_image_coords().reshape(-1, 2))
flat = _flatten_bundle(rb, device=dev)


def eager(chunk):
    outs = [model(_slice(flat, lo, min(H * W, lo + chunk))) for lo in range(0, H * W, chunk)]
    return {k: torch.cat([o[k] for o in outs]) for k in KEYS}


def fast(chunk):
    out = model.get_outputs_for_camera_ray_bundle(flat)
    return {k: out[k] for k in KEYS}


def timed(fn, chunk):
    fn(chunk)                                          # warm-up image (allocator, first launches)
    torch.cuda.synchronize()
    s0 = ops.SYNC_STATS["count"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(IMAGES):
        out = fn(chunk)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / IMAGES
    return out, ms, (ops.SYNC_STATS["count"] - s0) / IMAGES


with torch.no_grad():
    for chunk in (128, 2048, 3512):
        model.config.eval_num_rays_per_chunk = chunk
        assert uses_count_free_route(model, H * W), "the count-free route is not taken for this configuration"
        ref, ms_e, sync_e = timed(eager, chunk)
        got, ms_f, sync_f = timed(fast, chunk)
        for k in KEYS:
            assert torch.equal(got[k].reshape(ref[k].shape), ref[k]), (chunk, k)
        n = int(ref["num_samples_per_ray"].sum().item())
        print(json.dumps({"chunk": chunk, "rays": H * W, "samples_per_image": n, "images": IMAGES, "bit_equal": True,
                          "eager_ms_per_image": round(ms_e, 2), "eval_route_ms_per_image": round(ms_f, 2),
                          "speedup": round(ms_e / ms_f, 3),
                          "eager_samples_per_s": round(n / (ms_e * 1e-3)), "eval_route_samples_per_s": round(n / (ms_f * 1e-3)),
                          "eager_syncs_per_image": sync_e, "eval_route_syncs_per_image": sync_f}), flush=True)
