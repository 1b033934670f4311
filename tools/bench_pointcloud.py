#!/usr/bin/env python3
"""Point-cloud export (lsenerf_amd.pointcloud, csrc/pointcloud.hip) on the field and the 8 cameras of 640 x 480 of
tools/bench_eval_set.py: the four stages BEHIND the renders -- append over 8 images, keys + sort, merge, support filter -- as
(b) the package's entry points, against (a) the same stages written with torch ops on the device (boolean-mask indexing,
``torch.unique(return_inverse, return_counts)`` + ``index_add_``, 27 ``searchsorted`` neighbour lookups; they live here, not in the
package).  The renders (world normals on, the full route) are made once and shared; ``min_accumulation`` is the median accumulation
of the untrained field, voxels of 0.02 over the field's aabb, ``min_support`` 4.

The two routes must give the same point count, the same voxel keys, per-voxel counts and supports and the same surviving keys
(asserted); means are not compared bit for bit: ``index_add_`` sums in no fixed order.  The routes alternate in one process: one
warm-up each, then REPEATS timed exports each.  Per route: wall clock per export between two device synchronisations, HIP-event time
per stage, and the host waits of one export (``torch.cuda.set_sync_debug_mode("warn")``; route (b) ends with the one read of the
final count).  ``spread`` = the largest difference between two repeats of a route.  The renders' time is reported beside it.

One JSON line per measurement, also appended to ``--out FILE`` when given.  Exit status 1 unless
    wall (b) <= wall (a) - 2 spread.
usage: python tools/bench_pointcloud.py [--out FILE] [--repeats 3]"""
import argparse
import json
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=3)
args = ap.parse_args()
sys.argv = sys.argv[:1]                     # (bench_eval_set reads its own argv)
import torch
from bench_eval_set import H, N_CAM, W, dev, eval_set, model
from lsenerf_amd import evaluation, ops
from lsenerf_amd.eval_set import camera_bundle

VOXEL, MIN_SUPPORT = 0.02, 4
aabb = model.field.aabb.cpu().tolist()
LO, HI = [float(v) for v in aabb[0]], [float(v) for v in aabb[1]]
RES = ops.voxel_lattice(LO, HI, VOXEL)
STAGES = ("append", "keys_sort", "merge", "filter")


def emit_line(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def render_views():
    """[(origins, directions, depth, acc, rgb, normals)] of the 8 images and the time of the renders (ms per image)."""
    cfg = model.config
    cfg.eval_normals, cfg.eval_early_stop_eps = "world", 0.0
    views, ms = [], []
    for rep in range(2):
        views = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(N_CAM):
            rb = evaluation._flatten_bundle(camera_bundle(eval_set, i), device=dev)
            out = evaluation.render_flat(model, rb, check_overflow=False)
            views.append((rb.origins.contiguous(), rb.directions.contiguous(), out["depth"].reshape(-1).contiguous(),
                          out["accumulation"].reshape(-1).contiguous(), out["rgb"].contiguous(), out["normals"].contiguous()))
        model.occupancy_grid.check_deferred_overflow()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / N_CAM)
    cfg.eval_normals = "off"
    return views, ms


class Stages:
    """HIP events around the stages of one export."""

    def __init__(self):
        self.marks = [self._mark()]

    @staticmethod
    def _mark():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def done(self):
        self.marks.append(self._mark())

    def ms(self):
        return [a.elapsed_time(b) for a, b in zip(self.marks[:-1], self.marks[1:])]


def torch_route(views, min_acc):
    st = Stages()
    lo, hi = views[0][0].new_tensor(LO), views[0][0].new_tensor(HI)
    pts, cols, nrms = [], [], []
    for o, d, t, a, c, n in views:
        p = o + d * t[:, None]
        keep = (a >= min_acc) & (t > 0) & (t < float("inf")) & ((p >= lo) & (p <= hi)).all(-1)
        pts.append(p[keep]), cols.append(c[keep]), nrms.append(n[keep])          # boolean-mask indexing: a host wait each
    pts, cols, nrms = torch.cat(pts), torch.cat(cols), torch.cat(nrms)
    st.done()
    f = torch.floor((pts - lo) / pts.new_tensor([VOXEL]))       # (a tensor divisor: `/ float` multiplies by the reciprocal on the device)
    top = f.new_tensor([r - 1 for r in RES])
    v = torch.where(f >= top, top, torch.where(f > 0, f, torch.zeros_like(f))).to(torch.int64)
    keys = (v[:, 0] * RES[1] + v[:, 1]) * RES[2] + v[:, 2]
    ukeys, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)      # a sort and a host wait
    st.done()
    m = ukeys.shape[0]
    mean = lambda x: torch.zeros((m, 3), device=dev).index_add_(0, inverse, x)
    mp, mc, mn = mean(pts) / counts[:, None], mean(cols) / counts[:, None], mean(nrms)
    mn = mn / mn.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    st.done()
    x, y, z = ukeys // (RES[2] * RES[1]), (ukeys // RES[2]) % RES[1], ukeys % RES[2]
    support = torch.zeros(m, dtype=torch.int64, device=dev)
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                xx, yy, zz = x + dx, y + dy, z + dz
                inside = (xx >= 0) & (xx < RES[0]) & (yy >= 0) & (yy < RES[1]) & (zz >= 0) & (zz < RES[2])
                nkey = (xx * RES[1] + yy) * RES[2] + zz
                at = torch.searchsorted(ukeys, nkey).clamp_max(m - 1)
                support += torch.where(inside & (ukeys[at] == nkey), counts[at], torch.zeros_like(counts))
    keep = support >= MIN_SUPPORT
    out = (ukeys[keep], counts[keep], mp[keep], mc[keep], mn[keep])
    st.done()
    return dict(n_points=pts.shape[0], keys=ukeys, counts=counts, support=support, kept_keys=out[0], points=out[2]), st


def package_route(views, min_acc):
    st = Stages()
    cap = sum(v[2].shape[0] for v in views)
    pts, cols, nrms = (torch.empty((cap, 3), dtype=torch.float32, device=dev) for _ in range(3))
    total = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = torch.empty(ops.unproject_workspace_bytes(H * W), dtype=torch.uint8, device=dev)
    for o, d, t, a, c, n in views:
        ops.unproject_append(o, d, t, a, LO, HI, min_acc, pts, total, colors=c, normals=n, out_colors=cols, out_normals=nrms,
                             workspace=ws)
    st.done()
    keys = ops.voxel_keys(pts, LO, VOXEL, RES, n_dev=total)
    sorted_keys, order = torch.sort(keys, stable=True)
    st.done()
    mk, mc, mp, mcol, mn, mt = ops.voxel_merge(sorted_keys, order, pts, cols, nrms)
    st.done()
    fk, fc, fp, fcol, fn, ft, sup = ops.voxel_support_filter(mk, mc, mp, RES, MIN_SUPPORT, mcol, mn, m_dev=mt, want_support=True)
    st.done()
    kept = int(ft.item())                                  # the one read of an export: it trims the arrays
    return dict(n_points=total, keys=mk, n_voxels=mt, counts=mc, support=sup, kept_keys=fk[:kept], points=fp[:kept]), st


def count_waits(fn):
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fn()
    torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() for w in caught)


with torch.no_grad():
    views, render_ms = render_views()
    min_acc = float(torch.cat([v[3] for v in views]).median())
    routes = {"torch_ops": lambda: torch_route(views, min_acc), "package": lambda: package_route(views, min_acc)}
    wall = {k: [] for k in routes}
    stage_ms = {k: [] for k in routes}
    results = {}
    for name, fn in routes.items():                       # warm-up (allocator, first launches)
        fn()
    for _ in range(args.repeats):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            results[name], st = fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) * 1e3)
            stage_ms[name].append(st.ms())
    waits = {name: count_waits(fn) for name, fn in routes.items()}

    a, b = results["torch_ops"], results["package"]
    n_points, m = int(b["n_points"].item()), int(b["n_voxels"].item())
    assert a["n_points"] == n_points, (a["n_points"], n_points)
    assert a["keys"].shape[0] == m and torch.equal(a["keys"], b["keys"][:m]), "the two routes give different voxel keys"
    assert torch.equal(a["counts"].to(torch.int32), b["counts"][:m]), "the two routes give different per-voxel counts"
    assert torch.equal(a["support"].to(torch.int32), b["support"][:m]), "the two routes give different supports"
    assert torch.equal(a["kept_keys"], b["kept_keys"]), "the two routes keep different voxels"
    mean_diff = float((a["points"] - b["points"]).abs().max()) if b["points"].shape[0] else 0.0

for name in routes:
    per_stage = [sum(r[k] for r in stage_ms[name]) / args.repeats for k in range(len(STAGES))]
    emit_line({"route": name, "images": N_CAM, "rays_per_image": H * W, "repeats": args.repeats,
               "wall_ms_per_export": round(sum(wall[name]) / args.repeats, 3), "wall_ms_runs": [round(w, 3) for w in wall[name]],
               "event_ms": {k: round(v, 3) for k, v in zip(STAGES, per_stage)}, "event_ms_total": round(sum(per_stage), 3),
               "host_waits_per_export": waits[name]})
spread = max(max(w) - min(w) for w in wall.values())
a_ms, b_ms = sum(wall["torch_ops"]) / args.repeats, sum(wall["package"]) / args.repeats
ok = bool(b_ms <= a_ms - 2 * spread)
emit_line({"what": "torch_ops_vs_package", "min_accumulation": round(min_acc, 6), "voxel": VOXEL, "lattice": list(RES),
           "min_support": MIN_SUPPORT, "points": n_points, "voxels": m, "voxels_kept": int(b["kept_keys"].shape[0]),
           "same_point_count": True, "same_keys": True, "same_counts": True, "same_supports": True, "same_kept_keys": True,
           "max_abs_diff_of_kept_means": mean_diff, "torch_ops_ms": round(a_ms, 3), "package_ms": round(b_ms, 3),
           "spread_ms": round(spread, 3), "ratio": round(b_ms / a_ms, 4), "bar_b_le_a_minus_2_spread": ok})
emit_line({"what": "renders", "ms_per_image": round(render_ms[-1], 2), "ms_per_image_runs": [round(v, 2) for v in render_ms],
           "ms_for_the_set": round(render_ms[-1] * N_CAM, 1), "package_stages_share_of_an_export":
           round(b_ms / (b_ms + render_ms[-1] * N_CAM), 4)})
emit_line({"ok": ok})
sys.exit(0 if ok else 1)
