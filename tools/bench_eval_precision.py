#!/usr/bin/env python3
"""The reduced-piece MLP routes of the eval render (LSENeRFModelConfig.eval_mlp_arith: bf16x3, bf16x1) against bf16x6, on the
bench.py workload and the 640 x 480 camera of tools/bench_eval_early_stop.py (same seeded parameters and grid, same calibrated
step size, same opaque variant: the hash table scaled by the factor that tool searches for, searched here the same way).

(a) ``lse_mlp_fwd_pair`` alone on the bench step's own samples (bench.build_workload's set, about 4.19 M), per route, between two
    device events.
(b) ms per 640 x 480 image at chunks 3512 and 32768, per route.
(c) PSNR and maximum absolute difference of each reduced route's ``rgb`` / ``accumulation`` / ``depth`` against the bf16x6 image of
    the same run, on the workload as it is and on the opaque variant.

Protocol of (a) and (b): the routes alternate in one process; per route one warm-up, then two timed repetitions (images, or batches of
KERNEL_REPS launches) between two device events; the whole thing twice.  ``spread`` = the larger difference between a route's two
repeats, over the routes compared.  One JSON line per measurement.  Exit status 1 unless
    bf16x1: pair kernel <= bf16x6 - 2 spread  AND  ms per image at chunk 32768 <= bf16x6 - 2 spread
    bf16x3: pair kernel <= bf16x6 - 2 spread.
usage: python tools/bench_eval_precision.py [images]"""
import dataclasses
import json
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from lsenerf_amd import ops
from lsenerf_amd.cameras import EdCameras
from lsenerf_amd.evaluation import _flatten_bundle, uses_count_free_route

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
IMAGES = int(sys.argv[1]) if len(sys.argv) > 1 else 2
H, W = 480, 640
EPS = 1e-4
CHUNKS = (3512, 32768)
ROUTES = ("bf16x6", "bf16x3", "bf16x1")
KERNEL_REPS = 20

model, sets, counts = bench.build_workload(dev, seed=0)
model.eval()
model.deferred_max_slots = ops.MAX_SLOT_ELEMS
fld, cfg = model.field, model.config
c2w = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.5]]])
cams = EdCameras(c2w, fx=400.0, fy=400.0, cx=W / 2, cy=H / 2, width=W, height=H)
rb = cams.generate_rays(torch.zeros(H * W, dtype=torch.long), cams.get_image_coords().reshape(-1, 2))
flat = _flatten_bundle(rb, device=dev)
table = fld.mlp_base_grid.params
table0 = table.detach().clone()


def elapsed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps


def alternate(fns, reps):
    """{route: [ms, ms]}: per route one warm-up and one timed batch, routes alternating, the whole thing twice."""
    ms = {r: [] for r in fns}
    for _ in range(2):
        for r, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            ms[r].append(elapsed(fn, reps)[1])
    return ms


def render(route, eps=0.0):
    fld.inference_arith = route
    cfg.eval_early_stop_eps = eps
    return model.get_outputs_for_camera_ray_bundle(flat)


def opaque_factor():
    """tools/bench_eval_early_stop.py: the smallest power of four times the hash table at which the median sampled ray reaches
    T <= eps within the first quarter of its samples (measured with the early-stop route at 64-sample segments, bf16x6)."""
    cfg.eval_num_rays_per_chunk = CHUNKS[0]
    full = render("bf16x6")["num_samples_per_ray"].reshape(-1)
    has = full > 0
    base, cfg.eval_segment_samples = cfg.eval_segment_samples, 64
    try:
        factor = 1.0
        while factor <= 4.0 ** 16:
            table.copy_(table0 * factor)
            es = render("bf16x6", EPS)["num_samples_per_ray"].reshape(-1)
            if (es[has].float() / full[has].float()).median().item() <= 0.25:
                return factor
            factor *= 4.0
    finally:
        cfg.eval_segment_samples = base
        cfg.eval_early_stop_eps = 0.0
        table.copy_(table0)
    raise SystemExit("no factor up to 4^16 makes the median ray opaque within its first quarter")


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return math.inf if mse == 0.0 else 10.0 * math.log10(1.0 / mse)


bars = {}
with torch.no_grad():
    # ---- (a) the pair kernel on the bench step's samples
    brb, _, jit = sets[0]
    rays_o, rays_d = brb.origins.detach().contiguous(), brb.directions.detach().contiguous()
    ri, ts, te, packed = model.occupancy_grid.sampling(rays_o, rays_d, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
                                                       render_step_size=cfg.render_step_size, stratified=True, jitter=jit,
                                                       return_packed=True)
    n = ts.shape[0]
    x01, sel, y = fld._encode_packed(rays_o, rays_d, ri, ts, te, packed)
    emb_table, eidx = fld._eval_emb(rays_o.shape[0], dev) if fld.embedding_appearance is not None else (None, None)
    row_bias, head_meta = fld._head_row_bias(rays_d, eidx, emb_table)
    base, head = fld.mlp_base_mlp, fld.mlp_head

    def pair_of(route):
        arith = ops.MLP_ARITH_ROUTES[route]
        bm, hm = dataclasses.replace(base.meta(), arith=arith), dataclasses.replace(head_meta, arith=arith)
        return lambda: ops.fused_mlp_pair(base.params, y, sel, fld.average_init_density, bm, head.params, hm, n, row_bias, ri, packed,
                                          out_cols=4)
    ms = alternate({r: pair_of(r) for r in ROUTES}, KERNEL_REPS)
    k6 = sum(ms["bf16x6"]) / 2
    for r in ROUTES:
        row = {"what": "lse_mlp_fwd_pair", "route": r, "samples": n, "ms": round(sum(ms[r]) / 2, 4), "repeats_ms": [round(v, 4) for v in ms[r]]}
        if r != "bf16x6":
            spread = max(abs(ms[q][0] - ms[q][1]) for q in ("bf16x6", r))
            row.update(spread_ms=round(spread, 4), ratio=round(row["ms"] / k6, 3),
                       bar_le_bf16x6_minus_2_spread=bool(sum(ms[r]) / 2 <= k6 - 2 * spread))
            bars[(r, "kernel")] = row["bar_le_bf16x6_minus_2_spread"]
        print(json.dumps(row), flush=True)
    del x01, sel, y, row_bias, ri, ts, te, packed

    # ---- (b) ms per image, (c) fidelity against the bf16x6 image of the same run
    factor = opaque_factor()
    print(json.dumps({"opaque_factor": factor, "eps": EPS}), flush=True)
    for scene, f in (("i_untrained", 1.0), ("ii_opaque", factor)):
        table.copy_(table0 * f)
        for chunk in CHUNKS:
            cfg.eval_num_rays_per_chunk = chunk
            assert uses_count_free_route(model, H * W), "the count-free route is not taken for this configuration"
            if scene == "i_untrained":
                ms = alternate({r: (lambda r=r: render(r)) for r in ROUTES}, IMAGES)
                i6 = sum(ms["bf16x6"]) / 2
                for r in ROUTES:
                    row = {"what": "ms_per_image", "scene": scene, "chunk": chunk, "route": r, "rays": H * W, "images": IMAGES,
                           "ms": round(sum(ms[r]) / 2, 2), "repeats_ms": [round(v, 2) for v in ms[r]]}
                    if r != "bf16x6":
                        spread = max(abs(ms[q][0] - ms[q][1]) for q in ("bf16x6", r))
                        row.update(spread_ms=round(spread, 2), ratio=round(row["ms"] / i6, 3),
                                   le_bf16x6_minus_2_spread=bool(sum(ms[r]) / 2 <= i6 - 2 * spread))
                        if chunk == CHUNKS[-1]:
                            bars[(r, "image")] = row["le_bf16x6_minus_2_spread"]
                    print(json.dumps(row), flush=True)
            if chunk == CHUNKS[-1]:
                ref = render("bf16x6")
                for r in ROUTES[1:]:
                    out = render(r)
                    row = {"what": "fidelity_vs_bf16x6", "scene": scene, "chunk": chunk, "route": r,
                           "samples": int(ref["num_samples_per_ray"].sum().item())}
                    for k in ("rgb", "accumulation", "depth"):
                        row[f"{k}_psnr_db"] = round(psnr(out[k], ref[k]), 2)
                        row[f"{k}_max_abs_diff"] = float(f"{float((out[k] - ref[k]).abs().max()):.3e}")
                    row["depth_max"] = float(f"{float(ref['depth'].max()):.3e}")
                    print(json.dumps(row), flush=True)
    table.copy_(table0)
    fld.inference_arith = "bf16x6"

ok = bars.get(("bf16x1", "kernel"), False) and bars.get(("bf16x1", "image"), False) and bars.get(("bf16x3", "kernel"), False)
print(json.dumps({"bars": {f"{r}_{w}": v for (r, w), v in bars.items()}, "ok": bool(ok)}), flush=True)
sys.exit(0 if ok else 1)
