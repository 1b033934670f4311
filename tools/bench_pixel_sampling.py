#!/usr/bin/env python3
"""Weighted pixel sampling (``BatchComposer(sampling=PixelSampling(...))``), measured on the GPU.

Workload: a synthetic resident scene at the reference's split -- ``batch_split(3512, 0.66, "deblur")`` = 579 colour pixels (x 4 rays)
and 597 event pixels (x 2 rays) per step -- with 32 colour images and 64 int8 event frames of 480 x 640, one event frame pixel in ten
non-zero, and a 16-pixel invalid border in both masks.  Sampling: masks respected, event weights 9 (active) / 1 (idle).

    python tools/bench_pixel_sampling.py draw             # (a) the draw alone against the same draw in torch ops; exit 1: bar missed
    python tools/bench_pixel_sampling.py step             # (b) the captured step with and without sampling, alternating; exit 1: bar missed
    python tools/bench_pixel_sampling.py none [--root T]  # the captured step without sampling only, with the package of the tree T:
                                                          # run on this tree and on the parent commit's, alternating processes

(a) The torch route keeps a flat int64 inclusive cumulative sum of every pixel's weight resident (8 bytes per PIXEL; the kernel's
    table is 8 bytes per image ROW), and per step does ``torch.searchsorted(cum, t, right=True)`` and the unravel to (c, y, x) for
    both streams.  Its positions ``t`` are computed beforehand on the host and resident, so the route pays for no random numbers;
    on steps 0, 1 and the last one it runs on the kernel's own positions and the indices are asserted equal.  Time: HIP events around groups of INNER calls, the two
    routes alternating group by group; per route the median over the groups, spread = the largest difference between the medians
    of the route's REPEATS disjoint thirds.  Bar: new <= torch - 2 x spread.
(b) Two captured steps in one process on models built from the same seeds, blocks of BLOCK replays alternating; per route the
    median block, spread = max - min over the route's blocks after the first.  Bar: with - without <= draw time + 2 x spread, the
    draw time being that of the two draw launches inside a captured graph (INNER steps' draws captured and replayed), measured in
    the same process.  Also reported: the share of event rays whose target is non-zero.
Each mode prints one JSON line."""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
if "--root" in sys.argv:
    ROOT = sys.argv[sys.argv.index("--root") + 1]
sys.path.insert(0, os.path.abspath(ROOT))

import numpy as np
import torch
from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, cameras as cam
from lsenerf_amd import data
from lsenerf_amd.graph import GraphedTrainStep
from lsenerf_amd.optim import FlatAdam, FlatParams

dev = torch.device("cuda", 0)
N_COL, N_EVS, N_EMB, HW, BORDER = 32, 64, 64, (480, 640), 16
W_ACTIVE, W_IDLE = 9, 1
SEED = 0
INNER, GROUPS, REPEATS = 20, 60, 3            # (a): 60 groups of 20 calls per route
BLOCK, BLOCKS, WARMUP = 50, 7, 20            # (b): 7 blocks of 50 replays per route, the first of each is warm-up too


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
    return cam.EdCameras(torch.from_numpy(c2w), f, f, hw[1] / 2, hw[0] / 2, hw[1], hw[0], times=torch.linspace(t0, t1, n))


def make_scene():
    rng = np.random.default_rng(0)
    col_cams = look_at_cameras(N_COL, HW, 500.0, 1, 0.0, 10.0)
    evs_cams = look_at_cameras(N_EVS + 1, HW, 500.0, 2, 0.0, 10.0)
    evs_cams.set_hard_cam_type(cam.HardCamType.EVS)
    frames = (rng.integers(1, 5, (N_EVS,) + HW) * rng.choice([-1, 1], (N_EVS,) + HW) * (rng.random((N_EVS,) + HW) < 0.1)).astype(np.int8)
    msk = np.zeros(HW, np.uint8)
    msk[BORDER:-BORDER, BORDER:-BORDER] = 1
    return data.DeviceScene.from_arrays(
        dev, col_images=rng.integers(0, 256, (N_COL,) + HW + (3,), dtype=np.uint8), col_cameras=col_cams,
        col_appearance_ids=list(range(N_COL)), col_msk=np.broadcast_to(msk, (N_COL,) + HW).copy(), evs_frames=frames,
        evs_cameras=evs_cams, evs_appearance_ids=[i % N_EMB for i in range(N_EVS)],
        evs_msk=np.broadcast_to(msk, (N_EVS,) + HW).copy(), e_thresh=0.2, rgb_times=col_cams.times.reshape(-1))


def make_model():
    torch.manual_seed(96)
    cfg = LSENeRFModelConfig(use_mapping=True, mapping_method="identity", map_mode="co_map", evs_mapping_method="powpow",
                             rgb_loss_type="deblur")
    model = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=N_EMB).to(dev).train()
    with torch.no_grad():
        model.field.mlp_base_grid.params.mul_(3000.0)
        model.field.mlp_base_mlp.params[-16 * 64:-15 * 64].mul_(6.0)
    opt = FlatAdam(FlatParams(model.get_param_groups()["fields"]), lr=1e-3, eps=1e-15)
    for s in range(0, 64, 16):
        model.update_occupancy_grid(s)
    return model, opt


def composer(scene, sampling):
    n_col, n_evs = data.batch_split(3512, 0.66, "deblur")
    kw = {} if sampling is None else {"sampling": sampling}       # (the parent commit's composer has no such argument)
    return data.BatchComposer(scene, n_col, n_evs, deblur=True, seed=SEED, num_embd=N_EMB, **kw)


def median(v):
    return sorted(v)[len(v) // 2]


def group_ms(fn, groups):
    """ms per call of ``fn`` for every group of INNER back-to-back calls (HIP events around the group)."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(groups)]
    for e0, e1 in ev:
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        yield e0, e1


def bench_draw(scene, comp):
    """(a): ``(result dict, ms per step of the draw kernels inside a graph)``; both streams of a step on both routes."""
    streams = [w for w in comp._weighted if w is not None]
    steps = INNER * GROUPS
    # the torch route's resident state: per stream the flat inclusive sums and the positions of every step
    state = []
    for w in streams:
        n_img, H, W = w.shape
        wt = torch.cat([torch.from_numpy(w.row_weights(np.arange(i * H, (i + 1) * H))) for i in range(n_img)]).to(dev)
        cum = torch.cumsum(wt.reshape(-1), 0)
        assert int(cum[-1]) == w.total
        state.append((cum, H, W))
    check_steps = (0, 1, steps - 1)
    t_check = {}
    for w in streams:
        for s in check_steps:
            ctr = np.zeros((w.n, 4), np.uint32)
            ctr[:, 0], ctr[:, 1], ctr[:, 2] = s, np.arange(w.n), w.stream_id
            p = data.philox4x32_10(ctr, (SEED & 0xFFFFFFFF, SEED >> 32))
            t_check[(w.stream_id, s)] = torch.tensor([(((int(a) << 32) | int(b)) * w.total) >> 64 for a, b in p[:, :2]], device=dev)
    # positions of the timed steps: any resident positions cost the same, so uniform integers stand in for all but the checked steps
    g = torch.Generator(device=dev).manual_seed(1)
    pos = [torch.stack([torch.randint(0, w.total, (w.n,), generator=g, device=dev) for _ in range(64)]) for w in streams]
    out_t = [None, None]

    def torch_draw(k, t=None):
        for j, (cum, H, W) in enumerate(state):
            flat = torch.searchsorted(cum, pos[j][k & 63] if t is None else t[j], right=True)
            r = flat // W
            out_t[j] = torch.stack([r // H, r % H, flat - r * W], -1).to(torch.int32)

    def new_draw(k):
        for w in streams:
            w.draw(k, comp.step_dev, SEED)
    for s in check_steps:                                         # the same pixels on both routes
        torch_draw(0, [t_check[(w.stream_id, s)] for w in streams])
        new_draw(s)
        for j, w in enumerate(streams):
            assert torch.equal(out_t[j], w.indices), f"stream {w.stream_id}, step {s}: the torch route and the kernel disagree"
    counter = [0, 0]

    def a():
        torch_draw(counter[0])
        counter[0] += 1

    def b():
        new_draw(counter[1])
        counter[1] += 1
    for _ in range(3 * INNER):
        a()
        b()
    torch.cuda.synchronize()
    ev_a, ev_b = [], []
    ga, gb = group_ms(a, GROUPS), group_ms(b, GROUPS)
    for _ in range(GROUPS):                                       # alternating, group by group
        ev_a.append(next(ga))
        ev_b.append(next(gb))
    torch.cuda.synchronize()
    ms = lambda ev: [e0.elapsed_time(e1) / INNER for e0, e1 in ev]
    ms_a, ms_b = ms(ev_a), ms(ev_b)
    thirds = lambda v: [median(v[i::REPEATS]) for i in range(REPEATS)]
    spread = max(max(thirds(v)) - min(thirds(v)) for v in (ms_a, ms_b))
    new, old = median(ms_b), median(ms_a)
    # the kernels' own time, without the host between them: INNER steps' draws captured as one graph, replayed
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(INNER):
            for w in streams:
                w.draw(None, comp.step_dev, SEED)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    ev_g = []
    for _ in range(GROUPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graph.replay()
        e1.record()
        ev_g.append((e0, e1))
    torch.cuda.synchronize()
    in_graph = median(ms(ev_g))
    res = {"mode": "draw", "pixels_per_step": [w.n for w in streams], "calls_per_route": steps,
           "torch_ms_per_step": round(old, 5), "new_ms_per_step": round(new, 5), "new_in_graph_ms_per_step": round(in_graph, 5),
           "thirds_torch": [round(v, 5) for v in thirds(ms_a)],
           "thirds_new": [round(v, 5) for v in thirds(ms_b)], "spread_ms": round(spread, 5),
           "torch_table_bytes": sum(int(c.numel()) * 8 for c, _, _ in state), "new_table_bytes": sum(int(w.row_off.numel()) * 8 for w in streams),
           "indices_equal_on_steps": list(check_steps), "within_bar": bool(new <= old - 2 * spread)}
    return res, in_graph


def bench_steps(routes):
    """``routes``: name -> (step, composer).  Blocks of BLOCK replays, alternating between the routes; ms per step of every block and
    the share of event rays with a non-zero target over the timed replays."""
    for step, _ in routes.values():
        for _ in range(WARMUP):
            step()
    torch.cuda.synchronize()
    blocks = {k: [] for k in routes}
    nonzero = {k: torch.zeros((), device=dev) for k in routes}
    for _ in range(BLOCKS):
        for name, (step, comp) in routes.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BLOCK):
                step()
            e1.record()
            nonzero[name] += (comp.evs_batch["image"] != 0).float().mean()     # (the last replay of the block, outside the timing)
            blocks[name].append((e0, e1))
    torch.cuda.synchronize()
    out = {}
    for name, ev in blocks.items():
        ms = [e0.elapsed_time(e1) / BLOCK for e0, e1 in ev][1:]
        out[name] = {"ms_per_step_median": round(median(ms), 5), "blocks": [round(v, 5) for v in ms], "spread_ms": round(max(ms) - min(ms), 5),
                     "event_targets_nonzero": round(float(nonzero[name]) / BLOCKS, 4)}
    return out


def main(mode):
    scene = make_scene()
    if mode == "none":
        model, opt = make_model()
        comp = composer(scene, None)
        step = GraphedTrainStep(model, opt, composer=comp)
        res = bench_steps({"none": (step, comp)})["none"]
        step.check_overflow()
        print(json.dumps({"mode": "none", "tree": "--root" in sys.argv and ROOT or "this", **res}), flush=True)
        return 0
    sampling = data.PixelSampling(evs_active_weight=W_ACTIVE, evs_idle_weight=W_IDLE)
    if mode == "draw":
        res, _ = bench_draw(scene, composer(scene, sampling))
        print(json.dumps(res), flush=True)
        return 0 if res["within_bar"] else 1
    assert mode == "step", mode
    routes = {}
    for name, s in (("none", None), ("sampling", sampling)):
        model, opt = make_model()
        comp = composer(scene, s)
        routes[name] = (GraphedTrainStep(model, opt, composer=comp), comp)
    res = bench_steps(routes)
    for step, _ in routes.values():
        step.check_overflow()
    draw, draw_ms = bench_draw(scene, routes["sampling"][1])
    spread = max(r["spread_ms"] for r in res.values())
    excess = res["sampling"]["ms_per_step_median"] - res["none"]["ms_per_step_median"]
    ok = bool(excess <= draw_ms + 2 * spread)
    print(json.dumps({"mode": "step", "replays_per_block": BLOCK, "blocks_timed": BLOCKS - 1, **res, "excess_ms": round(excess, 5),
                      "draw_ms_per_step": round(draw_ms, 5), "spread_ms": round(spread, 5),
                      "allowed_excess_ms": round(draw_ms + 2 * spread, 5), "sampling_totals": routes["sampling"][1].sampling_totals,
                      "within_bar": ok}), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("--") else "step"))
