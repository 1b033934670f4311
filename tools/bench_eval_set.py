#!/usr/bin/env python3
"""A whole eval set: what a user did per image before ``evaluate_set`` existed -- (a) ``render_camera`` (rays built on the host,
uploaded) + ``get_image_metrics_and_images`` (ground truth uploaded, ``.tolist()``) -- against (b) ``LSENeRFModel.evaluate_set``
(rays, metric planes and the metrics table on the device, one overflow read and one read-back per set), and (b) again with the
event-only metric.  8 cameras of 640 x 480 on a ring around the bench.py workload's field (the model set-up of
tools/bench_eval_render.py restated here: the seeded parameters, the fully occupied one-level grid and the step size calibrated to
~1024 samples per SURVEY 8d ray), chunk = the reference's eval_num_rays_per_chunk.

Per route, one JSON line:
  wall_ms_per_image     host wall clock around the whole set between two device synchronisations, / images (mean of REPEATS sets
                        after a warm-up set)
  device_ms_per_image   sum of the HIP-event brackets around every C-ABI call of the library (_lib.TIMING), / images, from a pass
                        of its own: the library's kernels only -- torch's own copies and elementwise kernels are not in it
  waits_per_set         host waits for the device in one set: the warnings of torch.cuda.set_sync_debug_mode("warn"), from a pass
                        of its own; sampler_syncs_per_set: ops.SYNC_STATS
usage: python tools/bench_eval_set.py [repeats]"""
import json
import math
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from lsenerf_amd import EvalSet, LSENeRFModel, LSENeRFModelConfig, _lib, ops
from lsenerf_amd.cameras import EdCameras
from lsenerf_amd.evaluation import uses_count_free_route

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
REPEATS = int(sys.argv[1]) if len(sys.argv) > 1 else 2
N_CAM, H, W = 8, 480, 640
CHUNK = 3512
RAYS, SAMPLES_PER_RAY = 4096, 1024


def build_field():
    """bench.py's headline workload ("sphere"): parameters seeded with 96, cone 0, no alpha culling, one fully occupied grid level,
    and the step size settled so that 4096 rays from the radius-1.5 sphere (generator seed 0) yield ~1024 samples each."""
    torch.manual_seed(96)
    cfg = LSENeRFModelConfig(cone_angle=0.0, alpha_thre=0.0, grid_levels=1)
    model = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=64).to(dev)
    model.occupancy_grid.mark_all_occupied()
    g = torch.Generator().manual_seed(0)
    o = torch.randn(RAYS, 3, generator=g)
    o = 1.5 * o / o.norm(dim=-1, keepdim=True)
    d = (torch.rand(RAYS, 3, generator=g) - 0.5) - o
    d = d / d.norm(dim=-1, keepdim=True)
    o, d, jitter = o.to(dev), d.to(dev), torch.zeros(RAYS, device=dev)
    for _ in range(3):
        n = model.occupancy_grid.sampling(o, d, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
                                          render_step_size=cfg.render_step_size, stratified=True, jitter=jitter,
                                          return_packed=True)[1].shape[0]
        cfg.render_step_size = float(cfg.render_step_size * n / (RAYS * SAMPLES_PER_RAY))
    cfg.eval_num_rays_per_chunk = CHUNK
    return model.eval()


def ring_cameras():
    """N_CAM cameras 2.5 units from the centre of the [-1, 1]^3 box on a tilted ring, looking at it (OpenGL frame: -z forward)."""
    poses = []
    for k in range(N_CAM):
        a = 2 * math.pi * k / N_CAM
        pos = torch.tensor([2.5 * math.cos(a), 0.6 * math.sin(2 * a), 2.5 * math.sin(a)], dtype=torch.float64)
        back = pos / pos.norm()
        right = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), back)
        right = right / right.norm()
        poses.append(torch.stack([right, torch.linalg.cross(back, right), back, pos], dim=1).float())
    return EdCameras(torch.stack(poses), fx=400.0, fy=400.0, cx=W / 2, cy=H / 2, width=W, height=H)


model = build_field()
cams = ring_cameras()
images = torch.randint(0, 256, (N_CAM, H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8)
host_batches = [{"image": images[i].float() / 255.0} for i in range(N_CAM)]          # what an eval dataloader hands over
eval_set = EvalSet(dev, images, cams)
assert uses_count_free_route(model, H * W), "the count-free route is not taken for this configuration"


def per_image_route():
    rows = []
    for i in range(N_CAM):
        out = model.render_camera(cams, i)
        rows.append(model.get_image_metrics_and_images(out, host_batches[i])[0])
    return rows


ROUTES = {"a_render_camera_plus_image_metrics": per_image_route,
          "b_evaluate_set": lambda: model.evaluate_set(eval_set)[1],
          "b_evaluate_set_events_only": lambda: model.evaluate_set(eval_set, events_only=True)[1]}


def measure(fn):
    fn()                                                      # warm-up set (allocator, first launches)
    wall = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3 / N_CAM)
    _lib.TIMING = {"names": None, "events": []}               # pass 2: the library's own launches
    fn()
    torch.cuda.synchronize()
    events, _lib.TIMING = _lib.TIMING["events"], None
    device_ms = sum(e0.elapsed_time(e1) for _, e0, e1 in events) / N_CAM
    s0 = ops.SYNC_STATS["count"]                              # pass 3: the waits
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fn()
    torch.cuda.set_sync_debug_mode("default")
    waits = sum("synchroniz" in str(w.message).lower() for w in caught)
    return rows, wall, device_ms, len(events) / N_CAM, waits, ops.SYNC_STATS["count"] - s0


if __name__ == "__main__":          # (tools/bench_eval_panels.py imports the scene above)
    results = {}
    for name, fn in ROUTES.items():
        rows, wall, device_ms, calls, waits, sampler = measure(fn)
        results[name] = (rows, sum(wall) / len(wall))
        print(json.dumps({"route": name, "images": N_CAM, "rays_per_image": H * W, "chunk": CHUNK, "repeats": REPEATS,
                          "wall_ms_per_image": round(sum(wall) / len(wall), 2), "wall_ms_per_image_runs": [round(w, 2) for w in wall],
                          "device_ms_per_image": round(device_ms, 2), "library_calls_per_image": round(calls, 1),
                          "waits_per_set": waits, "sampler_syncs_per_set": sampler,
                          "mean_psnr": round(sum(r["psnr"] for r in rows) / N_CAM, 4),
                          "mean_ssim": round(sum(r["ssim"] for r in rows) / N_CAM, 6)}), flush=True)
    rows_a, wall_a = results["a_render_camera_plus_image_metrics"]
    rows_b, wall_b = results["b_evaluate_set"]
    # (a)'s rays come from torch on the host, (b)'s from the device kernel: equal to rounding, so the metrics agree closely, not bit for bit
    diff = {k: max(abs(ra[k] - rb[k]) for ra, rb in zip(rows_a, rows_b)) for k in ("psnr", "ssim")}
    print(json.dumps({"a_vs_b_max_abs_diff": diff, "wall_ratio_a_over_b": round(wall_a / wall_b, 3)}), flush=True)
