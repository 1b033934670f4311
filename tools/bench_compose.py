#!/usr/bin/env python3
"""Feeding the captured training step: the route a user writes without the composer against ``BatchComposer`` inside the graph.

  (a) "torch route"  indices from ``torch.randint`` on the device, targets gathered with torch indexing from resident images,
                     rays from the ``cameras.py`` generators on the device (``RayGenerator`` / ``generate_deblur_rays``,
                     ``ConsecRayGenerator``), metadata with torch ops, then ``GraphedTrainStep.__call__`` with its input copies;
  (b) "composer"     ``GraphedTrainStep(model, opt, composer=...)``: one compose launch inside the graph, ``step()`` copies nothing;
                     with spline poses: ``spline_tables`` + ``set_poses`` (torch, ~60 launches) in front of every replay;
  (c) "spline"       (b) with the spline ATTACHED (``composer.attach_spline``): the graph starts with ``lse_spline_poses``, which reads
                     the spline's parameters in place -- nothing runs in front of a replay.  Feeds the table (b) feeds (colour).
                     Default composition only.
  (c+) "spline + torch Adam"  (c) with ``ray_grads=True``, followed per step by what a caller does without ``camera_opt=``: assign
                     ``step.spline_grads`` to ``.grad``, ``torch.optim.Adam`` (lr 1e-3, eps 1e-15) and its exponential decay;
  (d) "camera_opt"   (c) with ``ray_grads=True`` and ``camera_opt=``: the spline backward writes into the flat gradient of a
                     ``FlatAdam`` over ``ctrl_tangents`` + ``scale`` whose update is the last launch of the graph.
  At config 2 the same pair for per-camera optimisers (a ``CameraOptimizer`` on the colour and on the event cameras):
  "set_poses" = ``camera_tables`` + ``set_poses`` in front of the replay, torch autograd over ``step.pose_grads`` and torch Adam behind
  it; "attached" = ``attach_camera_optimizers`` + ``camera_opt=``.
All at the reference's default composition (579 x 4 + 597 + 597 rays, deblur colour bundle, poses from the spline) and at config 2
(2318 + 597 + 597), on a synthetic resident scene (32 colour images 480 x 640, 64 int8 event frames 260 x 346, cameras on a
sphere around the [-1, 1]^3 box).  Per route: ms per step (median of the per-step device-event intervals, 100 steps after 20
warm-up ones) and host ms per step (time.perf_counter around the loop, no synchronisation inside it).

    python tools/bench_compose.py                            # the two compositions, both routes: one JSON line each
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_compose.py trace precomposed|composer [cfg]
    python tools/bench_compose.py analyze DIR_PRECOMPOSED_1 DIR_PRECOMPOSED_2 DIR_COMPOSER
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_compose.py trace composer_poses|spline
    python tools/bench_compose.py analyze_spline DIR_COMPOSER_POSES_1 DIR_COMPOSER_POSES_2 DIR_SPLINE
    python tools/bench_compose.py camera                     # (c+), (d) and the config-2 pair: one JSON line each
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_compose.py trace spline|spline_adam
    python tools/bench_compose.py analyze_camera DIR_SPLINE_1 DIR_SPLINE_2 DIR_SPLINE_ADAM
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_compose.py trace cfg2_set_poses|cfg2_attached cfg2
    python tools/bench_compose.py analyze_cfg2 DIR_SET_POSES_1 DIR_SET_POSES_2 DIR_ATTACHED

``trace``: replays only -- the composer step, or the parent's graphed step fed the SAME batches composed beforehand -- behind a
0.5 s pause that marks the start of the timed region in the kernel trace.  ``analyze``: summed kernel time per step of the three traces, the time of the two
composer kernels, and the bar of the change -- (b) may exceed the mean of the two precomposed runs by no more than the composer
kernels' own time plus twice the spread between those two runs.  ``trace composer_poses`` / ``trace spline``: routes (b) / (c) at the
default composition with ``ray_grads=True`` ((c) then ends with ``lse_spline_poses_bwd``); ``analyze_spline``: the same bar with the two
spline kernels as the change's own.  ``trace spline_adam``: route (d); ``analyze_camera``: the same bar against (c) with the camera
parameters' Adam launches as the change's own (the field's Adam runs the same two kernels: of every pair in a step the second launch
is the camera's).  ``analyze_cfg2``: the attached route against the set_poses route, own kernels = the two pose-delta kernels and the
camera Adam."""
import csv
import glob
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

STEPS, WARMUP = 100, 20
COMPOSE_KERNELS = ("compose_kernel", "advance_kernel", "rays_bwd_kernel")
SPLINE_KERNELS = ("spline_fwd_kernel", "spline_bwd_kernel")
DELTA_KERNELS = ("pose_delta_fwd_kernel", "pose_delta_bwd_kernel")
ADAM_KERNELS = ("adam_schedule_kernel", "adam_kernel")
CAMERA_ADAM = tuple("camera " + k for k in ADAM_KERNELS)


def analyze(dirs, own_kernels=COMPOSE_KERNELS, camera_adam=False):
    def load(d, split_adam=False):
        rows = []
        for f in glob.glob(f"{d}/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
        rows.sort()
        assert rows, f"no kernel trace under {d}"
        last_gap = max(i for i in range(1, len(rows)) if rows[i][0] - rows[i - 1][1] > 200e6)     # the 0.5 s pause
        timed = rows[last_gap:]
        per = {}
        seen = {k: 0 for k in ADAM_KERNELS}
        for s, e, name in timed:
            key = next((k for k in own_kernels if k in name), "other")
            adam = next((k for k in ADAM_KERNELS if k in name), None) if split_adam else None
            if adam is not None:        # field's, camera's, field's, ...: the camera's update is the second of every pair
                seen[adam] += 1
                key = "camera " + adam if seen[adam] % 2 == 0 else "other"
            tot, n = per.get(key, (0, 0))
            per[key] = (tot + (e - s), n + 1)
        if split_adam:
            assert all(n == 2 * STEPS for n in seen.values()), f"{d}: expected two Adam pairs per step, saw {seen}"
        return per
    pre1, pre2, comp = load(dirs[0]), load(dirs[1]), load(dirs[2], split_adam=camera_adam)
    steps = STEPS
    total = lambda per: sum(t for t, _ in per.values()) / steps / 1e6
    a, b, c = total(pre1), total(pre2), total(comp)
    own = sum(comp.get(k, (0, 0))[0] for k in own_kernels) / steps / 1e6
    spread = abs(a - b)
    res = {"precomposed_kernel_ms_per_step": [round(a, 5), round(b, 5)], "run_to_run_spread_ms": round(spread, 5),
           "composer_kernel_ms_per_step": round(c, 5), "composer_kernels_own_ms_per_step": round(own, 5),
           "avg_us": {k: round(comp[k][0] / comp[k][1] / 1e3, 3) for k in own_kernels if k in comp},
           "excess_ms": round(c - (a + b) / 2, 5), "allowed_excess_ms": round(own + 2 * spread, 5),
           "within_bar": bool(c - (a + b) / 2 <= own + 2 * spread)}
    print(json.dumps(res))
    return res


if len(sys.argv) > 1 and sys.argv[1] in ("analyze", "analyze_spline"):
    analyze(sys.argv[2:5], COMPOSE_KERNELS if sys.argv[1] == "analyze" else SPLINE_KERNELS)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] in ("analyze_camera", "analyze_cfg2"):
    # (the set_poses route of config 2 has ONE Adam pair per step, the field's: only the last directory is split by parity)
    analyze(sys.argv[2:5], CAMERA_ADAM if sys.argv[1] == "analyze_camera" else DELTA_KERNELS + CAMERA_ADAM, camera_adam=True)
    sys.exit(0)

import numpy as np
import torch
from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, RayBundle, cameras as cam
from lsenerf_amd.data import BatchComposer, DeviceScene, batch_split, camera_tables, spline_tables
from lsenerf_amd.graph import GraphedTrainStep
from lsenerf_amd.optim import FlatAdam, FlatParams

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
N_COL, N_EVS, N_EMB = 32, 64, 64
COL_HW, EVS_HW = (480, 640), (260, 346)


def look_at_cameras(n, hw, f, seed, t0, t1):
    """n cameras on a sphere of radius 2.2 around the origin, looking at it (OpenGL frame: -z forward), times ascending."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 1.5 * np.pi, n) + rng.normal(0, 0.01, n)
    pos = 2.2 * np.stack([np.cos(ang), 0.3 * np.sin(2 * ang), np.sin(ang)], -1)
    z = pos / np.linalg.norm(pos, axis=-1, keepdims=True)
    x = np.cross(np.array([0.0, 1.0, 0.0])[None], z)
    x /= np.linalg.norm(x, axis=-1, keepdims=True)
    y = np.cross(z, x)
    c2w = np.concatenate([np.stack([x, y, z], -1), pos[..., None]], -1).astype(np.float32)
    return cam.EdCameras(torch.from_numpy(c2w), f, f, hw[1] / 2, hw[0] / 2, hw[1], hw[0],
                         times=torch.linspace(t0, t1, n))


def build(kind):
    torch.manual_seed(96)
    deblur = kind == "default"
    cfg = LSENeRFModelConfig(use_mapping=True, mapping_method="identity", map_mode="co_map", evs_mapping_method="powpow",
                             rgb_loss_type="deblur" if deblur else "linspace")
    model = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=N_EMB).to(dev).train()
    with torch.no_grad():
        model.field.mlp_base_grid.params.mul_(3000.0)
        model.field.mlp_base_mlp.params[-16 * 64:-15 * 64].mul_(6.0)
    opt = FlatAdam(FlatParams(model.get_param_groups()["fields"]), lr=1e-3, eps=1e-15)
    for s in range(0, 64, 16):
        model.update_occupancy_grid(s)
    rng = np.random.default_rng(0)
    col_cams = look_at_cameras(N_COL, COL_HW, 500.0, 1, 0.0, 10.0)
    evs_cams = look_at_cameras(N_EVS + 1, EVS_HW, 300.0, 2, 0.0, 10.0)
    evs_cams.set_hard_cam_type(cam.HardCamType.EVS)
    scene = DeviceScene.from_arrays(
        dev, col_images=rng.integers(0, 256, (N_COL,) + COL_HW + (3,), dtype=np.uint8), col_cameras=col_cams,
        col_appearance_ids=list(range(N_COL)), evs_frames=rng.integers(-4, 5, (N_EVS,) + EVS_HW).astype(np.int8), evs_cameras=evs_cams,
        evs_appearance_ids=[i % N_EMB for i in range(N_EVS)], e_thresh=0.2, rgb_times=col_cams.times.reshape(-1))
    n_col, n_evs = batch_split(3512, 0.66, "deblur" if deblur else "mse")
    spl = None
    if deblur:
        spl = cam.CameraOptimizerConfig(mode="SO3xR3", optim_type="spline", exp_t=0.05).setup(
            num_cameras=N_COL, device="cpu", cameras=col_cams, dM=torch.eye(4)).to(dev)
        spl.device = dev
    return model, opt, scene, n_col, n_evs, spl


class TorchRoute:
    """(a): what a user of the parent commit writes -- everything in front of the graph is torch on the device."""

    def __init__(self, scene, n_col, n_evs, spl):
        self.scene, self.n_col, self.n_evs, self.spl = scene, n_col, n_evs, spl
        mv = lambda c: cam.EdCameras(c.camera_to_worlds.to(dev), c.fx, c.fy, c.cx, c.cy, c.width, c.height, times=c.times.to(dev))
        self.col_cams, self.evs_cams = mv(scene.col.cameras), mv(scene.evs.cameras)
        self.col_gen = cam.RayGenerator(self.col_cams).to(dev)
        self.evs_gen = cam.ConsecRayGenerator(self.evs_cams).to(dev)
        self.e_thresh = torch.full((n_evs, 1), scene.e_thresh, device=dev)

    @torch.no_grad()
    def compose(self):
        sc = self.scene

        def draw(n, s):
            return torch.stack([torch.randint(0, s.n_images, (n,), device=dev), torch.randint(0, s.H, (n,), device=dev),
                                torch.randint(0, s.W, (n,), device=dev)], -1)
        ci, ei = draw(self.n_col, sc.col), draw(self.n_evs, sc.evs)
        app = sc.col.appearance_id[ci[:, 0]].long()
        if self.spl is not None:
            col = cam.generate_deblur_rays(self.col_cams, self.spl, ci[:, 0], self.col_gen.image_coords[ci[:, 1], ci[:, 2]])
            app = torch.clip(app[:, None] + (torch.arange(4, device=dev) - 2)[None], 0, N_EMB - 1).reshape(-1)
        else:
            col = self.col_gen(ci)
        col.metadata["appearance_id"] = app
        prev, nxt = self.evs_gen(ei)
        prev.metadata["appearance_id"] = nxt.metadata["appearance_id"] = sc.evs.appearance_id[ei[:, 0]].long()
        batch = {"col_batch": {"image": sc.col.images[ci[:, 0], ci[:, 1], ci[:, 2]].float() / 255.0},
                 "evs_batch": {"image": (sc.evs.images[ei[:, 0], ei[:, 1], ei[:, 2]].float() * sc.e_scale)[:, None],
                               "e_thresh": self.e_thresh}}
        return (col, prev, nxt), batch


def timed(step_fn):
    for _ in range(WARMUP):
        step_fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(STEPS + 1)]
    ev[0].record()
    t0 = time.perf_counter()
    for i in range(STEPS):
        step_fn()
        ev[i + 1].record()
    host = (time.perf_counter() - t0) / STEPS * 1e3
    torch.cuda.synchronize()
    per = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(STEPS))
    return {"ms_per_step_median": round(per[STEPS // 2], 4), "ms_per_step_mean": round(ev[0].elapsed_time(ev[-1]) / STEPS, 4),
            "host_ms_per_step": round(host, 4)}


def run(kind):
    model, opt, scene, n_col, n_evs, spl = build(kind)
    route = TorchRoute(scene, n_col, n_evs, spl)
    bundles, batch = route.compose()
    step_a = GraphedTrainStep(model, opt, *bundles, batch)

    def a():
        bundles, batch = route.compose()
        step_a(*bundles, batch)
    res_a = timed(a)
    step_a.close()
    del step_a
    # every route starts from the same freshly built model, optimiser and occupancy grid (same seeds): the routes are compared on
    # the same training state, not one after the other on a model the previous route has trained
    del model, opt, route
    model, opt, scene, n_col, n_evs, spl = build(kind)
    comp = BatchComposer(scene, n_col, n_evs, deblur=spl is not None, seed=0, num_embd=N_EMB)
    step_b = GraphedTrainStep(model, opt, composer=comp)

    def b():
        if spl is not None:
            with torch.no_grad():
                comp.set_poses(col=spline_tables(spl, scene.col.cameras, "deblur"))
        step_b()
    res_b = timed(b)
    step_b.check_overflow()
    step_b.close()
    del step_b, model, opt
    res_c = {}
    if spl is not None:          # (c): the table (b) feeds, from the attached spline
        model, opt, scene, n_col, n_evs, spl = build(kind)
        comp_c = BatchComposer(scene, n_col, n_evs, deblur=True, seed=0, num_embd=N_EMB)
        comp_c.attach_spline(spl, tables=("col",))
        step_c = GraphedTrainStep(model, opt, composer=comp_c)
        res_c["spline"] = timed(step_c)
        step_c.check_overflow()
        step_c.close()
    print(json.dumps({"composition": kind, "rays": comp.n_rays, "col_pixels": n_col, "evs_pixels": n_evs, "steps": STEPS,
                      "warmup": WARMUP, "torch_route": res_a, "composer": res_b, **res_c}), flush=True)


CAM_LR, CAM_LR_FINAL, CAM_STEPS = 1e-3, 1e-4, 5000       # the reference's camera_opt group (R:lse_nerf/lse_config.py:29-38)


def torch_camera_adam(params):
    adam = torch.optim.Adam(params, lr=CAM_LR, eps=1e-15)
    return adam, torch.optim.lr_scheduler.ExponentialLR(adam, gamma=(CAM_LR_FINAL / CAM_LR) ** (1.0 / CAM_STEPS))


def flat_camera_adam(params):
    return FlatAdam(FlatParams(params), lr=CAM_LR, eps=1e-15, lr_final=CAM_LR_FINAL, max_steps=CAM_STEPS)


def camera_optimizers(scene):
    mk = lambda n: cam.CameraOptimizerConfig(mode="SO3xR3").setup(num_cameras=n, device=dev)
    return mk(scene.col.n_cameras), mk(scene.evs.n_cameras)


def camera_route(name, kind="default"):
    """``(fn, step)`` of one camera-optimiser route on a freshly built model: "spline_torch_adam" (c+), "spline_adam" (d) at the default
    composition; "cfg2_set_poses", "cfg2_attached" at config 2."""
    model, opt, scene, n_col, n_evs, spl = build(kind)
    comp = BatchComposer(scene, n_col, n_evs, deblur=spl is not None, seed=0, num_embd=N_EMB)
    if name == "spline_torch_adam":
        comp.attach_spline(spl, tables=("col",))
        step = GraphedTrainStep(model, opt, composer=comp, ray_grads=True)
        adam, sched = torch_camera_adam([spl.ctrl_tangents, spl.scale])

        def fn():
            step()
            spl.ctrl_tangents.grad = step.spline_grads["ctrl_tangents"]
            spl.scale.grad = step.spline_grads["scale"]
            adam.step()
            sched.step()
    elif name == "spline_adam":
        cam_opt = flat_camera_adam([spl.ctrl_tangents, spl.scale])            # (FlatParams re-points .data: before attaching)
        comp.attach_spline(spl, tables=("col",))
        step = fn = GraphedTrainStep(model, opt, composer=comp, ray_grads=True, camera_opt=cam_opt)
    elif name == "cfg2_set_poses":
        col_o, evs_o = camera_optimizers(scene)
        step = GraphedTrainStep(model, opt, composer=comp, ray_grads=True)
        adam, sched = torch_camera_adam([col_o.pose_adjustment, evs_o.pose_adjustment])

        def fn():
            tabs = [camera_tables(scene.col.cameras, col_o), camera_tables(scene.evs.cameras, evs_o)]
            comp.set_poses(col=tabs[0].detach(), prev=tabs[1].detach())
            step()
            adam.zero_grad(set_to_none=True)
            torch.autograd.backward(tabs, [step.pose_grads["col"].reshape(-1, 3, 4), step.pose_grads["prev"]])
            adam.step()
            sched.step()
    else:
        assert name == "cfg2_attached", name
        col_o, evs_o = camera_optimizers(scene)
        cam_opt = flat_camera_adam([col_o.pose_adjustment, evs_o.pose_adjustment])
        comp.attach_camera_optimizers(col=col_o, evs=evs_o)
        step = fn = GraphedTrainStep(model, opt, composer=comp, ray_grads=True, camera_opt=cam_opt)
    return fn, step


def run_camera():
    for kind, names in (("default", ("spline_torch_adam", "spline_adam")), ("cfg2", ("cfg2_set_poses", "cfg2_attached"))):
        res = {}
        for name in names:
            fn, step = camera_route(name, kind)
            res[name] = timed(fn)
            step.check_overflow()
            step.close()
            del fn, step
        print(json.dumps({"composition": kind, "camera_optimiser_routes": res, "steps": STEPS, "warmup": WARMUP}), flush=True)


def trace(mode, kind):
    if mode in ("spline_adam", "cfg2_set_poses", "cfg2_attached"):
        fn, step = camera_route(mode, kind)
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        time.sleep(0.5)
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        step.check_overflow()
        print(json.dumps({"trace": mode, "composition": kind, "steps": STEPS}), flush=True)
        return
    model, opt, scene, n_col, n_evs, spl = build(kind)
    comp = BatchComposer(scene, n_col, n_evs, deblur=spl is not None, seed=0, num_embd=N_EMB)
    if mode in ("composer_poses", "spline"):
        assert spl is not None, "the spline routes are measured at the default composition"
    if mode == "spline":
        comp.attach_spline(spl, tables=("col",))
    elif spl is not None:
        with torch.no_grad():
            comp.set_poses(col=spline_tables(spl, scene.col.cameras, "deblur"))
    if mode in ("composer", "spline"):
        step = GraphedTrainStep(model, opt, composer=comp, ray_grads=True)
        fn = step
    elif mode == "composer_poses":
        step = GraphedTrainStep(model, opt, composer=comp, ray_grads=True)

        def fn():
            with torch.no_grad():
                comp.set_poses(col=spline_tables(spl, scene.col.cameras, "deblur"))
            step()
    else:       # the parent's graphed step on precomposed inputs: the batches the composer step draws (steps 0, 1, ...), composed
        #         eagerly beforehand and handed to GraphedTrainStep.__call__ with its copies -- the same work per step on both sides
        cl = lambda t: t.clone() if torch.is_tensor(t) else t
        items = []
        for k in range(WARMUP + STEPS):
            bundles, batch = comp.compose(step=k)
            items.append(([RayBundle(origins=cl(b.origins), directions=cl(b.directions), pixel_area=cl(b.pixel_area),
                                     camera_indices=cl(b.camera_indices), times=cl(b.times),
                                     metadata={n: cl(v) for n, v in b.metadata.items()}) for b in bundles],
                          {n: {kk: cl(vv) for kk, vv in v.items()} for n, v in batch.items()}))
        step = GraphedTrainStep(model, opt, *items[0][0], items[0][1], ray_grads=True)
        it = iter(items)

        def fn():
            bundles, batch = next(it)
            step(*bundles, batch)
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    time.sleep(0.5)
    for _ in range(STEPS):
        fn()
    torch.cuda.synchronize()
    step.check_overflow()
    print(json.dumps({"trace": mode, "composition": kind, "steps": STEPS}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        trace(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else "default")
    elif len(sys.argv) > 1 and sys.argv[1] == "camera":
        run_camera()
    else:
        for kind in ("default", "cfg2"):
            run(kind)
