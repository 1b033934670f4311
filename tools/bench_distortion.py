#!/usr/bin/env python3
"""Distortion loss in the training step (LSENeRFModelConfig.distortion_loss_mult), on the bench.py workload (4096 rays x ~1024
samples, one MI355X).

(a) ``lse_distortion_fwd`` against ``lse_volrend_fwd`` and ``lse_distortion_bwd`` (the d_sigmas route with the densities, one
    broadcast upstream scalar: what the step launches) against ``lse_volrend_bwd`` (upstream gradient on the colour, d_rgb written:
    what the step launches), on the samples, densities and colours of the bench step -- between two device events.  The new
    kernels do the same walk over fewer streams.
(b) ms per step of the captured step (bench._graphed_timing) with the multiplier at 0 and at 0.01, from the same training state.
    A number, no bar.

Protocol: the variants alternate in one process; per variant one warm-up, then a timed batch; the whole thing twice.  ``spread`` =
the larger difference between a variant's two repeats, over the two variants compared.  One JSON line per measurement.  Exit status
1 unless each new kernel <= its compositor counterpart + 2 spread.
usage: python tools/bench_distortion.py [steps]"""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
import bench
from lsenerf_amd import _lib
from lsenerf_amd.optim import FlatAdam, FlatParams

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
STEPS = int(sys.argv[1]) if len(sys.argv) > 1 else 30
WARMUP = 6
KERNEL_REPS = 50
MULT = 0.01

model, sets, counts = bench.build_workload(dev, seed=1000)
model.sampler.density_fn = None            # the headline workload: no visibility pre-pass (alpha_thre = 0)
rb, target, jitter = sets[0]
fld, cfg = model.field, model.config
R = len(rb)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def elapsed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def alternate(fns, reps):
    """{variant: [ms, ms]}: per variant one warm-up and one timed batch, variants alternating, the whole thing twice."""
    ms = {r: [] for r in fns}
    for _ in range(2):
        for r, fn in fns.items():
            fn()
            torch.cuda.synchronize()
            ms[r].append(elapsed(fn, reps))
    return ms


# ---- (a) the four kernels on the step's own arrays
with torch.no_grad():
    ri, ts, te, packed, n_dev = model.occupancy_grid.sampling(
        rb.origins.detach(), rb.directions.detach(), sigma_fn=None, near_plane=cfg.near_plane, far_plane=cfg.far_plane,
        render_step_size=cfg.render_step_size, stratified=True, cone_angle=cfg.cone_angle, alpha_thre=cfg.alpha_thre, jitter=jitter,
        deferred=True)
    rays_o, rays_d = rb.origins.detach().contiguous(), rb.directions.detach().contiguous()
    table, eidx = fld._ray_emb(rb.metadata, rb.camera_indices, R, dev)
    sigma, _, _, rgb16 = fld.density_rgb_packed(rays_o, rays_d, ri, ts, te, packed, eidx, table, n_dev)
    n = int(packed[:, 1].sum().item())
    cap = ts.shape[0]
    stride = rgb16.stride(0)
    f = lambda *s: torch.empty(*s, device=dev)          # noqa: E731
    weights, out_rgb, out_acc, out_dep = f(cap), f(R, 3), f(R), f(R)
    d_sigma_vr, d_rgb, g_rgb = f(cap), torch.zeros_like(rgb16), torch.rand(R, 3, device=dev)
    loss, totals, d_sigma, g_one = f(R), f(R, 2), f(cap), torch.full((1,), MULT / R, device=dev)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    kernels = {
        "lse_volrend_fwd": lambda: _lib.call("lse_volrend_fwd", p(ts), p(te), p(sigma), p(rgb16), stride, p(packed), R, p(weights),
                                             p(out_rgb), p(out_acc), p(out_dep), st),
        "lse_distortion_fwd": lambda: _lib.call("lse_distortion_fwd", p(ts), p(te), p(weights), p(packed), R, 1.0, p(loss), p(totals), st),
        "lse_volrend_bwd": lambda: _lib.call("lse_volrend_bwd", p(ts), p(te), p(sigma), p(rgb16), stride, p(packed), R, p(weights),
                                             p(g_rgb), None, None, p(d_sigma_vr), p(d_rgb), st),
        "lse_distortion_bwd": lambda: _lib.call("lse_distortion_bwd", p(ts), p(te), p(sigma), p(weights), p(packed), R, 1.0, p(totals),
                                                p(g_one), 0, None, p(d_sigma), st),
    }
    ms = alternate(kernels, KERNEL_REPS)
    mean = {k: sum(v) / 2 for k, v in ms.items()}
    for k, v in ms.items():
        print(json.dumps({"what": k, "rays": R, "samples": n, "ms": round(mean[k], 4), "repeats_ms": [round(t, 4) for t in v]}), flush=True)
    ok = True
    for new, old in (("lse_distortion_fwd", "lse_volrend_fwd"), ("lse_distortion_bwd", "lse_volrend_bwd")):
        spread = max(abs(ms[k][0] - ms[k][1]) for k in (new, old))
        good = bool(mean[new] <= mean[old] + 2 * spread)
        ok = ok and good
        print(json.dumps({"what": f"{new}_vs_{old}", "spread_ms": round(spread, 4), "ratio": round(mean[new] / mean[old], 3),
                          "bar_le_counterpart_plus_2_spread": good}), flush=True)
    mean_loss = float(loss.mean())
    del ri, ts, te, packed, sigma, rgb16, weights, d_sigma_vr, d_rgb, d_sigma

# ---- (b) the captured step with the multiplier at 0 and at MULT, from the same training state
opt = FlatAdam(FlatParams(model.get_param_groups()["fields"]), lr=1e-2, eps=1e-15, lr_final=1e-4, max_steps=200000)
batch = {"col_batch": {"image": target}, "evs_batch": None}
snap = bench._snapshot(model, opt)
step_ms = {0.0: [], MULT: []}
for _ in range(2):
    for mult in step_ms:
        bench._restore(model, opt, snap)
        cfg.distortion_loss_mult = mult
        step_ms[mult].append(bench._graphed_timing(model, opt, rb, None, None, batch, STEPS, WARMUP)["ms_per_step"])
cfg.distortion_loss_mult = 0.0
off, on = sum(step_ms[0.0]) / 2, sum(step_ms[MULT]) / 2
print(json.dumps({"what": "graphed_step_ms", "rays": R, "samples": n, "steps": STEPS, "mult_0_ms": round(off, 4), f"mult_{MULT}_ms": round(on, 4),
                  "added_ms": round(on - off, 4), "ratio": round(on / off, 4), "repeats_mult_0_ms": [round(v, 4) for v in step_ms[0.0]],
                  f"repeats_mult_{MULT}_ms": [round(v, 4) for v in step_ms[MULT]],
                  "spread_ms": round(max(abs(v[0] - v[1]) for v in step_ms.values()), 4),
                  "mean_distortion_per_ray_at_start": round(mean_loss, 6)}), flush=True)
print(json.dumps({"ok": ok}), flush=True)
sys.exit(0 if ok else 1)
