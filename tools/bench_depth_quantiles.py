#!/usr/bin/env python3
"""Quantile depths of the eval render (LSENeRFModelConfig.eval_depth_quantiles), on the bench.py workload and the 640 x 480 camera
of tools/bench_eval_precision.py.

(a) ``lse_eval_depth_quantiles`` (three quantiles, interpolated, with depth_sel) against ``lse_eval_composite`` on the samples of
    one 32768-ray chunk of that image -- between two device events.  The new kernel reads 12 bytes per sample and does the same
    scan; the compositor reads those and the colour rows.
(b) ms per 640 x 480 image with the setting off and on, at chunks 3512 and 32768, on the full count-free route and on the
    early-stop route (eps 1e-4).
(c) for 8 cameras on a ring (160 x 120): the points ``export_point_cloud`` keeps with ``depth="expected"`` and ``"median"`` --
    raw, merged per voxel, and after the neighbour-support filter.  No bar.

Protocol of (a) and (b): the variants alternate in one process; per variant one warm-up, then a timed batch between two device
events; the whole thing twice.  ``spread`` = the larger difference between a variant's two repeats, over the variants compared.  One
JSON line per measurement.  Exit status 1 unless
    lse_eval_depth_quantiles <= lse_eval_composite + 2 spread.
usage: python tools/bench_depth_quantiles.py [images]"""
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from lsenerf_amd import ops
from lsenerf_amd.cameras import EdCameras
from lsenerf_amd.evaluation import _flatten_bundle, _slice, uses_count_free_route
from lsenerf_amd.renderer import LinearRenderer

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
IMAGES = int(sys.argv[1]) if len(sys.argv) > 1 else 2
H, W = 480, 640
CHUNKS = (3512, 32768)
QS = (0.25, 0.5, 0.75)
EPS = 1e-4
KERNEL_REPS = 50
RING, RING_H, RING_W = 8, 120, 160
VOXEL, SUPPORT, MIN_ACC = 0.02, 4, 0.5

model, sets, counts = bench.build_workload(dev, seed=0)
model.eval()
model.deferred_max_slots = ops.MAX_SLOT_ELEMS
fld, cfg = model.field, model.config
c2w = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.5]]])
cams = EdCameras(c2w, fx=400.0, fy=400.0, cx=W / 2, cy=H / 2, width=W, height=H)
rb = cams.generate_rays(torch.zeros(H * W, dtype=torch.long), cams.get_image_coords().reshape(-1, 2))
flat = _flatten_bundle(rb, device=dev)


def elapsed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps


def alternate(fns, reps):
    """{variant: [ms, ms]}: per variant one warm-up and one timed batch, variants alternating, the whole thing twice."""
    ms = {r: [] for r in fns}
    for _ in range(2):
        for r, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            ms[r].append(elapsed(fn, reps)[1])
    return ms


def render(on, eps):
    cfg.eval_depth_quantiles, cfg.eval_depth_interpolate, cfg.eval_early_stop_eps = (QS if on else ()), on, eps
    return model.get_outputs_for_camera_ray_bundle(flat)


def look_at(eye):
    """[3, 4] camera-to-world of a camera at ``eye`` looking at the origin (columns: right, up, back)."""
    eye = torch.tensor(eye, dtype=torch.float32)
    back = eye / eye.norm()
    right = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0]), back)
    right = right / right.norm()
    return torch.stack([right, torch.linalg.cross(back, right), back, eye], dim=1)


ok = False
with torch.no_grad():
    # ---- (a) the two kernels on one chunk's samples
    cfg.eval_num_rays_per_chunk = CHUNKS[1]
    part = _slice(flat, (H // 2) * W - CHUNKS[1] // 2, (H // 2) * W + CHUNKS[1] // 2)        # the rows around the image centre
    m = len(part)
    fld._prepass = None
    ri, ts, te, packed, n_dev = model.sampler.sample_packed(part, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
                                                            render_step_size=cfg.render_step_size, alpha_thre=cfg.alpha_thre,
                                                            cone_angle=cfg.cone_angle)
    rays_o, rays_d = part.origins.contiguous(), part.directions.contiguous()
    table, eidx = fld._eval_emb(m, dev) if fld.embedding_appearance is not None else (None, None)
    sigma, _, _, head = fld.density_rgb_packed(rays_o, rays_d, ri, ts, te, packed, eidx, table, n_dev)
    rgb, acc, depth = torch.empty((m, 3), device=dev), torch.empty(m, device=dev), torch.empty(m, device=dev)
    nsamples = torch.empty(m, dtype=torch.int64, device=dev)
    ws = torch.empty(3 * m, device=dev)
    dq, reached, dsel = torch.empty((m, 3), device=dev), torch.empty(m, dtype=torch.uint8, device=dev), torch.empty(m, device=dev)
    taus = [ops.depth_tau(q) for q in QS]
    linear = isinstance(model.renderer_rgb, LinearRenderer)
    background = {"black": 0.0, "white": 1.0}.get(cfg.background_color)
    composite = lambda: ops.eval_composite(ts, te, sigma, head, packed, rgb, acc, depth, nsamples, nan_to_num=not linear,
                                           background=background, clamp=not linear, workspace=ws)
    quantiles = lambda: ops.eval_depth_quantiles(ts, te, sigma, packed, taus, dq, reached, dsel, interpolate=True, sel=1)
    ms = alternate({"lse_eval_composite": composite, "lse_eval_depth_quantiles": quantiles}, KERNEL_REPS)
    spread = max(abs(v[0] - v[1]) for v in ms.values())
    old_ms, new_ms = sum(ms["lse_eval_composite"]) / 2, sum(ms["lse_eval_depth_quantiles"]) / 2
    ok = bool(new_ms <= old_ms + 2 * spread)
    n = int(nsamples.sum().item())
    for r, v in ms.items():
        print(json.dumps({"what": r, "rays": m, "samples": n, "ms": round(sum(v) / 2, 4), "repeats_ms": [round(t, 4) for t in v]}),
              flush=True)
    print(json.dumps({"what": "depth_quantiles_vs_composite", "spread_ms": round(spread, 4), "ratio": round(new_ms / old_ms, 3),
                      "rays_median_reached": int(((reached >> 1) & 1).sum().item()),
                      "rays_all_three_reached": int((reached == 7).sum().item()), "bar_le_composite_plus_2_spread": ok}), flush=True)
    del ri, ts, te, packed, sigma, head

    # ---- (b) ms per image
    for chunk in CHUNKS:
        cfg.eval_num_rays_per_chunk = chunk
        assert uses_count_free_route(model, H * W), "the count-free route is not taken for this configuration"
        for route, eps in (("count_free", 0.0), ("early_stop", EPS)):
            ms = alternate({on: (lambda on=on: render(on, eps)) for on in (False, True)}, IMAGES)
            off_ms, on_ms = sum(ms[False]) / 2, sum(ms[True]) / 2
            print(json.dumps({"what": "ms_per_image", "chunk": chunk, "route": route, "rays": H * W, "images": IMAGES,
                              "off_ms": round(off_ms, 2), "on_ms": round(on_ms, 2), "added_ms": round(on_ms - off_ms, 2),
                              "ratio": round(on_ms / off_ms, 3), "repeats_off_ms": [round(v, 2) for v in ms[False]],
                              "repeats_on_ms": [round(v, 2) for v in ms[True]],
                              "spread_ms": round(max(abs(v[0] - v[1]) for v in ms.values()), 2)}), flush=True)
    cfg.eval_depth_quantiles, cfg.eval_depth_interpolate, cfg.eval_early_stop_eps = (), False, 0.0

    # ---- (c) what the exporter keeps, expected against median depth
    cfg.eval_num_rays_per_chunk = CHUNKS[1]
    ring = torch.stack([look_at((2.5 * math.cos(2 * math.pi * i / RING), 2.5 * math.sin(2 * math.pi * i / RING), 0.8 * math.sin(3.0 * i)))
                        for i in range(RING)])
    rcams = EdCameras(ring, fx=100.0, fy=100.0, cx=RING_W / 2, cy=RING_H / 2, width=RING_W, height=RING_H)
    coords = rcams.get_image_coords().reshape(-1, 2)
    bundles = [rcams.generate_rays(torch.full((RING_H * RING_W,), i, dtype=torch.long), coords) for i in range(RING)]
    for mode, spread_arg in (("expected", None), ("median", None), ("median", 0.05)):
        kw = dict(min_accumulation=MIN_ACC, normals=False, colors=False, depth=mode, max_depth_spread=spread_arg)
        raw = model.export_point_cloud(bundles, **kw).points.shape[0]
        merged = model.export_point_cloud(bundles, voxel_size=VOXEL, **kw).points.shape[0]
        kept = model.export_point_cloud(bundles, voxel_size=VOXEL, min_support=SUPPORT, **kw).points.shape[0]
        print(json.dumps({"what": "point_cloud", "depth": mode, "max_depth_spread": spread_arg, "cameras": RING,
                          "rays": RING * RING_H * RING_W, "min_accumulation": MIN_ACC, "raw_points": raw, "voxel_size": VOXEL,
                          "voxels": merged, "min_support": SUPPORT, "voxels_after_filter": kept, "filter_removed": merged - kept,
                          "filter_removed_share": round((merged - kept) / max(merged, 1), 4)}), flush=True)

print(json.dumps({"ok": ok}), flush=True)
sys.exit(0 if ok else 1)
