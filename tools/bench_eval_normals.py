#!/usr/bin/env python3
"""Rendered analytic normals of the eval render (LSENeRFModelConfig.eval_normals), on the bench.py workload and the 640 x 480 camera
of tools/bench_eval_precision.py.

(a) ``lse_density_logit_grad`` on the bench step's own samples (bench.build_workload's set, about 4.19 M) against the route it
    replaces: a zero-fill of the [N, 16] seed with column 0 set, then ``lse_mlp_bwd_input`` -- between two device events.
(b) ms per 640 x 480 image at chunks 3512 and 32768 with normals off, "field" and "world".
(c) the HIP-event time of the three launches the option adds (lse_density_logit_grad, lse_hash_bwd_input,
    lse_eval_composite_normals), summed over one image, per chunk size.

Protocol of (a) and (b): the variants alternate in one process; per variant one warm-up, then a timed batch between two device
events; the whole thing twice.  ``spread`` = the larger difference between a variant's two repeats, over the variants compared.  One
JSON line per measurement.  Exit status 1 unless
    lse_density_logit_grad <= seeded lse_mlp_bwd_input route - 2 spread.
usage: python tools/bench_eval_normals.py [images]"""
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from lsenerf_amd import _lib, ops
from lsenerf_amd.cameras import EdCameras
from lsenerf_amd.evaluation import _flatten_bundle, uses_count_free_route

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
IMAGES = int(sys.argv[1]) if len(sys.argv) > 1 else 2
H, W = 480, 640
CHUNKS = (3512, 32768)
MODES = ("off", "field", "world")
KERNEL_REPS = 20
NEW_LAUNCHES = ("lse_density_logit_grad", "lse_hash_bwd_input", "lse_eval_composite_normals")

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


def render(mode):
    cfg.eval_normals = mode
    return model.get_outputs_for_camera_ray_bundle(flat)


ok = False
with torch.no_grad():
    # ---- (a) the gradient kernel against the seeded route, on the bench step's samples
    brb, _, jit = sets[0]
    rays_o, rays_d = brb.origins.detach().contiguous(), brb.directions.detach().contiguous()
    ri, ts, te, packed = model.occupancy_grid.sampling(rays_o, rays_d, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
                                                       render_step_size=cfg.render_step_size, stratified=True, jitter=jit,
                                                       return_packed=True)
    n = ts.shape[0]
    x01, sel, y = fld._encode_packed(rays_o, rays_d, ri, ts, te, packed)
    base = fld.mlp_base_mlp
    meta = base.meta()
    d_y = torch.empty_like(y)
    seed = torch.empty((n, 16), dtype=torch.float32, device=dev)

    def seeded():
        seed.zero_()
        seed[:, 0] = 1.0
        ops.mlp_bwd_input(base.params, y, meta, n, None, 16, seed, d_in=d_y)
        return d_y

    new = lambda: ops.density_logit_grad(base.params, y, meta, n, d_in=d_y)
    same = torch.equal(seeded().clone().view(torch.int32), new().view(torch.int32))
    ms = alternate({"seeded_mlp_bwd_input": seeded, "density_logit_grad": new}, KERNEL_REPS)
    spread = max(abs(v[0] - v[1]) for v in ms.values())
    old_ms, new_ms = sum(ms["seeded_mlp_bwd_input"]) / 2, sum(ms["density_logit_grad"]) / 2
    ok = bool(new_ms <= old_ms - 2 * spread)
    for r, v in ms.items():
        print(json.dumps({"what": r, "samples": n, "ms": round(sum(v) / 2, 4), "repeats_ms": [round(t, 4) for t in v]}), flush=True)
    print(json.dumps({"what": "density_logit_grad_vs_seeded", "spread_ms": round(spread, 4), "ratio": round(new_ms / old_ms, 3),
                      "same_bits": bool(same), "bar_le_seeded_minus_2_spread": ok}), flush=True)
    del x01, sel, y, d_y, seed, ri, ts, te, packed

    # ---- (b) ms per image, (c) the added launches
    for chunk in CHUNKS:
        cfg.eval_num_rays_per_chunk = chunk
        assert uses_count_free_route(model, H * W), "the count-free route is not taken for this configuration"
        ms = alternate({m: (lambda m=m: render(m)) for m in MODES}, IMAGES)
        off = sum(ms["off"]) / 2
        for m in MODES:
            row = {"what": "ms_per_image", "chunk": chunk, "eval_normals": m, "rays": H * W, "images": IMAGES,
                   "ms": round(sum(ms[m]) / 2, 2), "repeats_ms": [round(v, 2) for v in ms[m]]}
            if m != "off":
                row.update(added_ms=round(row["ms"] - off, 2), ratio=round(row["ms"] / off, 3),
                           spread_ms=round(max(abs(ms[q][0] - ms[q][1]) for q in ("off", m)), 2))
            print(json.dumps(row), flush=True)
        for m in MODES[1:]:
            _lib.TIMING = {"names": set(NEW_LAUNCHES), "events": []}
            try:
                out = render(m)
                torch.cuda.synchronize()
                events = _lib.TIMING["events"]
            finally:
                _lib.TIMING = None
            per = {k: round(sum(e0.elapsed_time(e1) for name, e0, e1 in events if name == k), 3) for k in NEW_LAUNCHES}
            unit = out["normals"].reshape(-1, 3).norm(dim=-1)
            print(json.dumps({"what": "added_launches_ms_per_image", "chunk": chunk, "eval_normals": m, "launches": len(events), **per,
                              "total_ms": round(sum(per.values()), 3), "samples": int(out["num_samples_per_ray"].sum().item()),
                              "rays_with_a_normal": int((unit > 0.5).sum().item())}), flush=True)
    cfg.eval_normals = "off"

print(json.dumps({"ok": ok}), flush=True)
sys.exit(0 if ok else 1)
