#!/usr/bin/env python3
"""Mesh export (lsenerf_amd.mesh, csrc/mesh.hip) on the bench.py workload's field at 128^3, 256^3 and 512^3 cells over the field's aabb,
iso value = the median density of the 128^3 lattice (an untrained field: a noise-like surface, about as many vertices as a lattice
can give).

(1) HIP-event times of the four stages: the density lattice pass (lattice_positions + the field's eval-mode density route, chunks of
    2^22 points), lse_surface_nets_count, lse_surface_nets_emit, and the vertex normals (normals_packed + lse_point_normals_world).
    Each stage twice in one process.
(2) At 256^3: route (a), the same extraction written with torch ops on the device (nonzero / cumsum / advanced indexing; it lives
    here, not in the package), against route (b), count + one read of the totals + emit.  The routes alternate; per route one warm-up
    and one timed run, the whole thing twice.  ``spread`` = the larger difference between a route's two repeats.
    The two routes must give the same vertex count and the same triangle array (asserted).

One JSON line per measurement, also appended to ``--out FILE`` when given.  Exit status 1 unless
    (b) <= (a) - 2 spread   at 256^3.
usage: python tools/bench_mesh.py [--out FILE] [--resolutions 128,256,512]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from lsenerf_amd import mesh as lm, ops

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--resolutions", default="128,256,512")
args = ap.parse_args()
RESOLUTIONS = [int(v) for v in args.resolutions.split(",")]
BAR_RES = 256
CHUNK = 1 << 22

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
model, _, _ = bench.build_workload(dev, seed=0)
model.eval()
fld = model.field
aabb = fld.aabb.cpu().tolist()
LO, HI = [float(v) for v in aabb[0]], [float(v) for v in aabb[1]]


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


def torch_surface_nets(sigma, n, lo, hi, level):
    """Route (a): the definition of include/lse_hip.h ("mesh export") with torch ops -- what the package would do without csrc/mesh.hip."""
    S = sigma.view(n + 1, n + 1, n + 1)
    inside = S > level
    cnt = torch.zeros((n, n, n), dtype=torch.int32, device=sigma.device)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                cnt += inside[dx:dx + n, dy:dy + n, dz:dz + n]
    active = ((cnt != 0) & (cnt != 8)).reshape(-1)
    cells = torch.nonzero(active)[:, 0]
    vid = torch.cumsum(active, 0, dtype=torch.int32) - 1                       # vertex id of every active cell
    cc = torch.stack([cells // (n * n), (cells // n) % n, cells % n], dim=1)
    acc = torch.zeros((cells.shape[0], 3), dtype=torch.float32, device=sigma.device)
    count = torch.zeros(cells.shape[0], dtype=torch.int32, device=sigma.device)
    eye = torch.eye(3, dtype=torch.int64, device=sigma.device)
    flat = sigma.reshape(-1)
    pidx = lambda q: (q[:, 0] * (n + 1) + q[:, 1]) * (n + 1) + q[:, 2]
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        for ob in (0, 1):
            for oc in (0, 1):
                P = cc + ob * eye[b] + oc * eye[c]
                sP, sQ = flat[pidx(P)], flat[pidx(P + eye[a])]
                cross = (sP > level) != (sQ > level)
                t = (level - sP) / (sQ - sP)
                t = torch.where(torch.isnan(t), torch.full_like(t, 0.5), t).clamp(0.0, 1.0)
                pt = P.to(torch.float32)
                pt[:, a] = pt[:, a] + t
                acc = acc + torch.where(cross[:, None], pt, torch.zeros_like(pt))
                count += cross
    u = acc / count.to(torch.float32)[:, None]
    lo_t, hi_t = sigma.new_tensor(lo), sigma.new_tensor(hi)
    vertices = lo_t + (u / float(n)) * (hi_t - lo_t)
    mark = torch.zeros((n + 1, n + 1, n + 1, 3), dtype=torch.bool, device=sigma.device)
    for a in range(3):
        sl_p, sl_q = [slice(1, n)] * 3, [slice(1, n)] * 3
        sl_p[a], sl_q[a] = slice(0, n), slice(1, n + 1)
        mark[tuple(sl_p) + (a,)] = inside[tuple(sl_p)] != inside[tuple(sl_q)]
    idx = torch.nonzero(mark.reshape(-1))[:, 0]
    p, a = idx // 3, idx % 3
    i = torch.stack([p // ((n + 1) * (n + 1)), (p // (n + 1)) % (n + 1), p % (n + 1)], dim=1)
    eb, ec = eye[(a + 1) % 3], eye[(a + 2) % 3]
    cid = lambda q: vid[(q[:, 0] * n + q[:, 1]) * n + q[:, 2]]
    w = torch.stack([cid(i - eb - ec), cid(i - ec), cid(i), cid(i - eb)], dim=1)
    w = torch.where(inside.reshape(-1)[p][:, None], w, w.flip(1))
    triangles = torch.stack([w[:, 0], w[:, 1], w[:, 2], w[:, 0], w[:, 2], w[:, 3]], dim=1).reshape(-1, 3)
    return vertices, triangles


ok = False
with torch.no_grad():
    level = None
    for n in RESOLUTIONS:
        res = (n, n, n)
        points = ops.lattice_points(res)
        ws = torch.empty(ops.surface_nets_workspace_bytes(res), dtype=torch.uint8, device=dev)
        totals = torch.zeros(2, dtype=torch.int64, device=dev)
        ms = {"density": [], "count": [], "emit": [], "normals": []}
        for rep in range(2):
            sigma, t = timed(lambda: lm.density_lattice(fld, res, LO, HI, CHUNK))
            ms["density"].append(t)
            if level is None:
                level = float(sigma.median())
            ms["count"].append(timed(lambda: ops.surface_nets_count(sigma, res, level, ws, totals))[1])
            n_v, n_q = totals.tolist()
            v = torch.empty((n_v, 3), dtype=torch.float32, device=dev)
            tri = torch.empty((2 * n_q, 3), dtype=torch.int32, device=dev)
            ms["emit"].append(timed(lambda: ops.surface_nets_emit(sigma, res, LO, HI, level, ws, v, tri))[1])
            nrm, t = timed(lambda: lm.vertex_normals(fld, v, CHUNK))
            ms["normals"].append(t)
            unit = float((nrm.norm(dim=-1) > 0.5).float().mean()) if n_v else 0.0
            del nrm
            if rep == 0:
                del v, tri
        emit_line({"what": "stages_ms", "resolution": n, "points": points, "level": round(level, 6), "vertices": n_v, "quads": n_q,
                   "workspace_MiB": round(ws.numel() / 2 ** 20, 1), "vertices_with_a_normal": round(unit, 4),
                   **{k: round(sum(x) / 2, 3) for k, x in ms.items()}, "repeats_ms": {k: [round(y, 3) for y in x] for k, x in ms.items()}})
        if n == BAR_RES:
            route_a = lambda: torch_surface_nets(sigma, n, LO, HI, level)
            route_b = lambda: ops.surface_nets(sigma, res, LO, HI, level)[:2]
            rms = {"torch_ops": [], "count_emit": []}
            for _ in range(2):
                for name, fn in (("torch_ops", route_a), ("count_emit", route_b)):
                    fn()
                    torch.cuda.synchronize()
                    out, t = timed(fn)
                    rms[name].append(t)
                    if name == "torch_ops":
                        va, ta = out
                    else:
                        vb, tb = out
            assert va.shape[0] == vb.shape[0] == n_v, (va.shape, vb.shape, n_v)
            assert ta.shape == tb.shape and torch.equal(ta.to(torch.int32), tb), "the two routes give different triangles"
            same_vertices = bool(torch.equal(va, vb))
            spread = max(abs(x[0] - x[1]) for x in rms.values())
            a_ms, b_ms = sum(rms["torch_ops"]) / 2, sum(rms["count_emit"]) / 2
            ok = bool(b_ms <= a_ms - 2 * spread)
            emit_line({"what": "torch_ops_vs_count_emit", "resolution": n, "torch_ops_ms": round(a_ms, 3), "count_emit_ms": round(b_ms, 3),
                       "repeats_ms": {k: [round(y, 3) for y in x] for k, x in rms.items()}, "spread_ms": round(spread, 3),
                       "ratio": round(b_ms / a_ms, 4), "same_vertex_count": True, "same_triangles": True,
                       "same_vertex_bits": same_vertices, "bar_b_le_a_minus_2_spread": ok})
            del va, ta, vb, tb
        del sigma, ws, v, tri
        torch.cuda.empty_cache()

emit_line({"ok": ok})
sys.exit(0 if ok else 1)
