#!/usr/bin/env python3
"""TSDF mesh export (lsenerf_amd.tsdf, csrc/tsdf.hip, the masked surface nets of csrc/mesh.hip) on the field and the 8 cameras of
640 x 480 of tools/bench_eval_set.py, lattices of 128^3, 256^3 and 512^3 cells over the field's aabb, truncation 3 voxel edges,
``min_accumulation`` = the median accumulation of the untrained field.

(1) HIP-event times of the stages: the 8 renders (made once, shared by every lattice), lse_tsdf_integrate with 1 and with 8 views
    per launch (colours fused), the field, count + emit with LSE_NETS_SKIP_NAN, the fused vertex colours, the vertex normals.  Each
    stage twice in one process.
(2) At 256^3: route (a), the same integration written with torch ops on the device (one elementwise op per operation of the
    definition, the lattice positions precomputed outside the timed region; it lives here, not in the package), against route (b),
    lse_tsdf_integrate at 8 views per launch.  The routes alternate; per route one warm-up and one timed run, the whole thing twice.
    ``spread`` = the larger difference between a route's two repeats.  Torch's float32 `*`, `+`, `-`, `/`, `sqrt` and `round` each
    round once like the definition's (the truncation divides as a device tensor: by a host scalar torch multiplies with the
    reciprocal), so the two routes' ``tw`` and ``cw`` must be equal bit for bit (asserted).

One JSON line per measurement, also appended to ``--out FILE`` when given.  Exit status 1 unless
    (b) <= (a) - 2 spread   at 256^3.
usage: python tools/bench_tsdf.py [--out FILE] [--resolutions 128,256,512]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--resolutions", default="128,256,512")
args = ap.parse_args()
sys.argv = sys.argv[:1]                     # (bench_eval_set reads its own argv)
import torch
from bench_eval_set import H, N_CAM, W, dev, eval_set, model
from lsenerf_amd import evaluation, mesh as lm, ops, tsdf
from lsenerf_amd.eval_set import camera_bundle

RESOLUTIONS = [int(v) for v in args.resolutions.split(",")]
BAR_RES = 256
aabb = model.field.aabb.cpu().tolist()
LO, HI = [float(v) for v in aabb[0]], [float(v) for v in aabb[1]]
DESC = eval_set.cam_desc
R2_MAX = tsdf.border_r2_max(DESC)
model.eval()


def emit_line(row):
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def render_views():
    depth = torch.empty((N_CAM, H * W), dtype=torch.float32, device=dev)
    acc, rgb = torch.empty_like(depth), torch.empty((N_CAM, H * W, 3), dtype=torch.float32, device=dev)
    for i in range(N_CAM):
        out = evaluation.render_flat(model, evaluation._flatten_bundle(camera_bundle(eval_set, i), device=dev), check_overflow=False)
        depth[i].copy_(out["depth"].reshape(-1))
        acc[i].copy_(out["accumulation"].reshape(-1))
        rgb[i].copy_(out["rgb"].reshape(-1, 3))
    model.occupancy_grid.check_deferred_overflow()
    return depth, acc, rgb


def torch_integrate(x, tw, cw, poses, depth, acc, rgb, trunc, min_acc):
    """Route (a): the update of include/lse_hip.h ("TSDF fusion") for a pinhole camera with carving, one torch op per operation."""
    t, w = tw[:, 0].clone(), tw[:, 1].clone()
    c, cwt = cw[:, :3].clone(), cw[:, 3].clone()
    inf = torch.full_like(t, float("inf"))
    trunc_t = torch.full((), trunc, dtype=torch.float32, device=t.device)      # a tensor: torch divides by a host scalar as x * (1 / s)
    for j in range(poses.shape[0]):
        M = poses[j]
        v0, v1, v2 = x[:, 0] - M[0, 3], x[:, 1] - M[1, 3], x[:, 2] - M[2, 3]
        xc = (v0 * M[0, 0] + v1 * M[1, 0]) + v2 * M[2, 0]
        yc = (v0 * M[0, 1] + v1 * M[1, 1]) + v2 * M[2, 1]
        zc = (v0 * M[0, 2] + v1 * M[1, 2]) + v2 * M[2, 2]
        z = -zc
        ok = z > 0
        X, Y = xc / z, yc / z
        u, v = torch.round(X * DESC.fx + DESC.cx), torch.round(DESC.cy - Y * DESC.fy)
        ok &= (u >= 0) & (u < float(W)) & (v >= 0) & (v < float(H))
        pix = torch.where(ok, v, torch.zeros_like(v)).long() * W + torch.where(ok, u, torch.zeros_like(u)).long()
        dp, a = depth[j][pix], acc[j][pix]
        dist = torch.sqrt((v0 * v0 + v1 * v1) + v2 * v2)
        surface = a >= min_acc
        sdf = torch.where(surface, dp - dist, inf)
        ok &= ~surface | ((dp > 0) & (dp < float("inf")))
        ok &= ~(sdf < -trunc)
        tn = torch.clamp(sdf / trunc_t, max=1.0)
        t = torch.where(ok, (t * w + tn) / (w + 1.0), t)
        w = torch.where(ok, w + 1.0, w)
        okc = ok & surface & (sdf <= trunc)
        q = rgb[j][pix]
        c = torch.where(okc[:, None], (c * cwt[:, None] + q) / (cwt[:, None] + 1.0), c)
        cwt = torch.where(okc, cwt + 1.0, cwt)
    return torch.stack([t, w], 1), torch.cat([c, cwt[:, None]], 1)


ok = False
with torch.no_grad():
    (depth, acc, rgb), t0 = timed(render_views)
    (depth, acc, rgb), t1 = timed(render_views)
    min_acc = float(acc.median())
    poses = eval_set.poses[torch.as_tensor(eval_set.data.image_idx_host).long().to(dev)].contiguous()
    emit_line({"what": "renders_ms", "views": N_CAM, "H": H, "W": W, "total_ms": [round(t0, 3), round(t1, 3)],
               "per_view_ms": round((t0 + t1) / 2 / N_CAM, 3), "min_accumulation": round(min_acc, 6)})
    for n in [16] + RESOLUTIONS:                # (16: an untimed pass that takes the first-call costs of every stage)
        res = (n, n, n)
        points = ops.lattice_points(res)
        trunc = 3.0 * max((h - l) / n for l, h in zip(LO, HI))
        ms = {"integrate_1": [], "integrate_8": [], "field": [], "count": [], "emit": [], "colors": [], "normals": []}
        ws = torch.empty(ops.surface_nets_workspace_bytes(res), dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)

        def integrate(vol, per_launch):
            for a in range(0, N_CAM, per_launch):
                b = min(N_CAM, a + per_launch)
                vol.integrate(DESC, poses[a:b], depth[a:b], acc[a:b], rgb[a:b], min_acc, True, R2_MAX)

        for rep in range(2):
            vol1 = tsdf.TSDFVolume(res, LO, HI, trunc, dev)
            ms["integrate_1"].append(timed(lambda: integrate(vol1, 1))[1])
            vol = tsdf.TSDFVolume(res, LO, HI, trunc, dev)
            ms["integrate_8"].append(timed(lambda: integrate(vol, 8))[1])
            assert torch.equal(vol.tw, vol1.tw) and torch.equal(vol.cw, vol1.cw), "1 and 8 views per launch give different bytes"
            del vol1
            fld, t = timed(lambda: vol.field(1))
            ms["field"].append(t)
            ms["count"].append(timed(lambda: ops.surface_nets_count(fld, res, 0.0, ws, totals, skip_nan=True))[1])
            n_v, n_q = totals.tolist()
            v = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
            tri = torch.empty((2 * n_q, 3), dtype=torch.int32, device=dev)
            ms["emit"].append(timed(lambda: ops.surface_nets_emit(fld, res, LO, HI, 0.0, ws, v, tri, skip_nan=True))[1])
            ms["colors"].append(timed(lambda: vol.vertex_colors(v))[1])
            ms["normals"].append(timed(lambda: lm.vertex_normals(model.field, v))[1])
            observed = float((vol.tw[:, 1] > 0).float().mean())
            if rep == 0:
                del vol, fld, v, tri
        mean = {k: sum(x) / 2 for k, x in ms.items()}
        if n == 16:
            del vol, fld, v, tri, ws
            continue
        emit_line({"what": "stages_ms", "resolution": n, "points": points, "truncation": round(trunc, 6), "vertices": n_v, "quads": n_q,
                   "observed_points": round(observed, 4), "state_MiB": round(points * 24 / 2 ** 20, 1),
                   **{k: round(x, 3) for k, x in mean.items()},
                   "integrate_8_GBps_of_48B_per_point": round(points * 48 / (mean["integrate_8"] * 1e-3) / 1e9, 1),
                   "repeats_ms": {k: [round(y, 3) for y in x] for k, x in ms.items()}})
        if n == BAR_RES:
            x = ops.lattice_positions(res, LO, HI, device=dev)
            zero_tw, zero_cw = torch.zeros_like(vol.tw), torch.zeros_like(vol.cw)

            def route_a():
                return torch_integrate(x, zero_tw, zero_cw, poses, depth, acc, rgb, trunc, min_acc)

            def route_b():
                tw, cw = torch.zeros_like(zero_tw), torch.zeros_like(zero_cw)
                ops.tsdf_integrate(tw, cw, res, LO, HI, DESC, poses, depth, acc, rgb, trunc, min_acc, True, R2_MAX)
                return tw, cw
            rms = {"torch_ops": [], "tsdf_integrate": []}
            outs = {}
            for _ in range(2):
                for name, fn in (("torch_ops", route_a), ("tsdf_integrate", route_b)):
                    fn()
                    torch.cuda.synchronize()
                    outs[name], t = timed(fn)
                    rms[name].append(t)
            spread = max(abs(r[0] - r[1]) for r in rms.values())
            a_ms, b_ms = sum(rms["torch_ops"]) / 2, sum(rms["tsdf_integrate"]) / 2
            ok = bool(b_ms <= a_ms - 2 * spread)
            (tw_a, cw_a), (tw_b, cw_b) = outs["torch_ops"], outs["tsdf_integrate"]
            differ = int((tw_a.view(torch.int32) != tw_b.view(torch.int32)).any(1).sum())
            differ_c = int((cw_a.view(torch.int32) != cw_b.view(torch.int32)).any(1).sum())
            emit_line({"what": "torch_ops_vs_tsdf_integrate", "resolution": n, "views": N_CAM, "torch_ops_ms": round(a_ms, 3),
                       "tsdf_integrate_ms": round(b_ms, 3), "repeats_ms": {k: [round(y, 3) for y in r] for k, r in rms.items()},
                       "spread_ms": round(spread, 3), "ratio": round(b_ms / a_ms, 4), "points_with_other_tw_bits": differ,
                       "points_with_other_cw_bits": differ_c, "bar_b_le_a_minus_2_spread": ok})
            assert differ == 0 and differ_c == 0, "the two routes give different bytes"
            del x, zero_tw, zero_cw, outs, tw_a, cw_a, tw_b, cw_b
        del vol, fld, v, tri, ws
        torch.cuda.empty_cache()

emit_line({"ok": ok})
sys.exit(0 if ok else 1)
