#!/usr/bin/env python3
"""Early ray termination of the eval render against the full count-free route, on one 640 x 480 camera of the bench.py workload
(bench.build_workload: same seeded parameters and grid, same calibrated step size; the camera of tools/bench_eval_render.py).

Scenes: (i) the workload as it is -- an untrained field, no ray gets near T = 1e-4, so this prices the segment launches that find
nothing to stop; (ii) the same workload with its hash table scaled (the factor is searched here, with full renders, and printed)
until the median ray of the full render is opaque -- T <= eps -- within the first quarter of its samples (opaque_factor below).  Chunk sizes 3512 (the
reference's eval_num_rays_per_chunk) and 32768; ``deferred_max_slots`` is raised for the run so that the larger one takes the
count-free route at all (the default budget sends it to the ``forward`` loop).

Protocol: both routes alternate in one process; per route one warm-up image, then IMAGES timed images between two device events; the
whole thing twice.  ``spread`` = the larger difference between a route's two repeats.  One JSON line per (scene, chunk): ms per image
of both routes (the mean of the repeats), samples evaluated by each, samples marched, host syncs per image.  Exit status 1 unless,
on scene (ii) at chunk 32768, early_stop_ms <= full_ms - 2 * spread.  usage: python tools/bench_eval_early_stop.py [images]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from lsenerf_amd import ops
from lsenerf_amd.cameras import EdCameras
from lsenerf_amd.evaluation import _flatten_bundle, segment_schedule, uses_count_free_route

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
IMAGES = int(sys.argv[1]) if len(sys.argv) > 1 else 2
H, W = 480, 640
EPS = 1e-4
CHUNKS = (3512, 32768)

model, _, _ = bench.build_workload(dev, seed=0)
model.eval()
model.deferred_max_slots = ops.MAX_SLOT_ELEMS
c2w = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.5]]])
cams = EdCameras(c2w, fx=400.0, fy=400.0, cx=W / 2, cy=H / 2, width=W, height=H)
rb = cams.generate_rays(torch.zeros(H * W, dtype=torch.long), cams.get_image_coords().reshape(-1, 2))
flat = _flatten_bundle(rb, device=dev)
table = model.field.mlp_base_grid.params
table0 = table.detach().clone()


def render(eps):
    model.config.eval_early_stop_eps = eps
    return model.get_outputs_for_camera_ray_bundle(flat)


def timed(eps):
    render(eps)                                        # warm-up image (allocator, first launches)
    torch.cuda.synchronize()
    s0 = ops.SYNC_STATS["count"]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(IMAGES):
        out = render(eps)
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / IMAGES, (ops.SYNC_STATS["count"] - s0) / IMAGES


def opaque_factor():
    """The smallest power of four times the hash table at which the median sampled ray of the full render reaches T <= eps within the
    first quarter of its samples.  Measured with the route itself at 64-sample segments, the finest it has: a ray's count there is an
    upper bound (by less than 64) of the sample at which its transmittance reaches eps, so `count <= full count / 4` is sufficient."""
    cfg = model.config
    cfg.eval_num_rays_per_chunk = CHUNKS[0]
    full = render(0.0)["num_samples_per_ray"].reshape(-1)
    has = full > 0
    base, cfg.eval_segment_samples = cfg.eval_segment_samples, 64
    try:
        factor = 1.0
        while factor <= 4.0 ** 16:  # (the density is exp(logit) and the bias-free ReLU MLP is homogeneous: logit ~ 1e-5 x factor)
            table.copy_(table0 * factor)
            es = render(EPS)["num_samples_per_ray"].reshape(-1)
            ratio = (es[has].float() / full[has].float()).median().item()
            print(f"factor {factor:g}: median stop count / full count {ratio:.4f} (median full count "
                  f"{full[has].float().median().item():.0f})", file=sys.stderr, flush=True)
            if ratio <= 0.25:
                return factor, ratio
            factor *= 4.0
    finally:
        cfg.eval_segment_samples = base
    raise SystemExit("no factor up to 4^16 makes the median ray opaque within its first quarter")


ok = True
with torch.no_grad():
    cfg = model.config
    cap = model.occupancy_grid._cap_per_ray(cfg.near_plane, cfg.far_plane, cfg.render_step_size, cfg.cone_angle)
    n_segments = len(segment_schedule(cap, cfg.eval_segment_samples))
    factor, ratio = opaque_factor()
    print(json.dumps({"opaque_factor": factor, "median_stop_over_full_count": round(ratio, 4), "cap_per_ray": cap,
                      "segments": n_segments, "eps": EPS, "segment_samples": cfg.eval_segment_samples}), flush=True)
    for scene, f in (("i_untrained", 1.0), ("ii_opaque", factor)):
        table.copy_(table0 * f)
        for chunk in CHUNKS:
            cfg.eval_num_rays_per_chunk = chunk
            assert uses_count_free_route(model, H * W), "the count-free route is not taken for this configuration"
            ms = {"full": [], "early_stop": []}
            for _ in range(2):
                full, t, sync_f = timed(0.0)
                ms["full"].append(t)
                es, t, sync_e = timed(EPS)
                ms["early_stop"].append(t)
            spread = max(abs(v[0] - v[1]) for v in ms.values())
            full_ms, es_ms = sum(ms["full"]) / 2, sum(ms["early_stop"]) / 2
            marched = int(full["num_samples_per_ray"].sum().item())
            evaluated = int(es["num_samples_per_ray"].sum().item())
            row = {"scene": scene, "chunk": chunk, "rays": H * W, "images": IMAGES, "full_ms_per_image": round(full_ms, 2),
                   "early_stop_ms_per_image": round(es_ms, 2), "spread_ms": round(spread, 2), "ratio": round(es_ms / full_ms, 3),
                   "samples_marched": marched, "samples_evaluated_full": marched, "samples_evaluated_early_stop": evaluated,
                   "share_evaluated": round(evaluated / max(marched, 1), 4), "full_syncs_per_image": sync_f,
                   "early_stop_syncs_per_image": sync_e}
            if scene == "ii_opaque" and chunk == CHUNKS[-1]:
                row["bar_early_stop_le_full_minus_2_spread"] = bool(es_ms <= full_ms - 2 * spread)
                ok = row["bar_early_stop_le_full_minus_2_spread"]
            print(json.dumps(row), flush=True)
    table.copy_(table0)
sys.exit(0 if ok else 1)
