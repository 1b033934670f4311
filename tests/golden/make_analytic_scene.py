#!/usr/bin/env python3
"""Generator of tests/golden/analytic_scene_oracle.json: trains ``oracle.model.ModelOracle`` on the analytic scene of
tests/analytic_scene.py with the configuration tests/test_gpu_analytic_scene.py trains the HIP model with (one dictionary,
``analytic_scene.CONFIG``), on the pixels the composer draws (``lsenerf_amd.data.draw_indices_host``), for three seeds of the
initialisation -- each the parameters ``LSENeRFModel`` itself starts from under that seed (``hip_initialisation``), so that the HIP
model of the test and the oracle of the same seed begin alike -- and records what the trained oracle scores against the closed form.  The GPU test takes every bar from that file.

CPU only, project code only.  usage:
    python tests/golden/make_analytic_scene.py [--cache DIR] [--threads N] [--parallel P] [--full]
``--cache`` keeps the trained states, so a rerun only measures.  Without ``--full`` contraction off is trained for one seed only
and its margin is the spread measured with contraction on (the JSON says which).  The committed file was made with ``--full
--threads 2 --parallel 4``: torch's CPU sums depend on the thread count, and 400 training steps amplify a last-bit difference into
the spread between two seeds, so only a rerun with two threads reproduces the file to its last digits.  ``--steps N`` tries another
step count without touching ``analytic_scene.CONFIG`` (at 800 steps no score of the oracle moved by more than its spread).
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import analytic_scene as sc  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "analytic_scene_oracle.json")
CFG = sc.CONFIG


def build_model(contraction: bool, seed: int):
    from oracle.field import FieldOracle
    from oracle.model import ModelOracle
    field = FieldOracle("tcnn", log2_hashmap_size=CFG["log2_hashmap_size"], num_embeddings=CFG["num_embeddings"],
                        contraction=contraction, seed=seed)
    for k, v in hip_initialisation(contraction, seed).items():        # the oracle starts where the HIP model of that seed starts
        assert field.params[k].shape == v.shape, k
        field.params[k] = v.clone().requires_grad_(True)
    return ModelOracle(field, grid_resolution=CFG["grid_resolution"], grid_levels=CFG["grid_levels"], alpha_thre=CFG["alpha_thre"],
                       cone_angle=CFG["cone_angle"], near_plane=CFG["near_plane"], render_step_size=CFG["render_step_size"],
                       background=CFG["background"])


def hip_initialisation(contraction: bool, seed: int):
    """The parameters ``LSENeRFModel`` starts from under ``torch.manual_seed(seed)``, built on the CPU the way
    tests/test_gpu_analytic_scene.py builds its model, by the oracle's names (the layouts are those of tests/util.sync_params_to_oracle).
    Oracle seed ``s`` and the HIP model of seed ``s`` so start from the same numbers; what is left between them is the jitter stream,
    the occupancy refresh's draws and the order of floating-point sums."""
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig
    from lsenerf_amd.field import LSEEmbeddingConfig
    torch.manual_seed(seed)
    cfg = LSENeRFModelConfig(grid_resolution=CFG["grid_resolution"], grid_levels=CFG["grid_levels"], log2_hashmap_size=CFG["log2_hashmap_size"],
                             alpha_thre=CFG["alpha_thre"], cone_angle=CFG["cone_angle"], near_plane=CFG["near_plane"],
                             render_step_size=CFG["render_step_size"], background_color=CFG["background"],
                             disable_scene_contraction=not contraction, embed_config=LSEEmbeddingConfig(eval_mode="mean"))
    fld = LSENeRFModel(cfg, torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), CFG["num_embeddings"]).field
    return {"grid": fld.mlp_base_grid.params.detach(), "base": fld.mlp_base_mlp.params.detach(), "head": fld.mlp_head.params.detach(),
            "embedding": fld.embedding_appearance.embedding.weight.detach()}


def init_checksum(params):
    return {k: float(v.double().sum()) for k, v in params.items()}


def state_path(cache, contraction, seed):
    return os.path.join(cache, f"analytic_{'on' if contraction else 'off'}_{seed}.pt")


def train_one(contraction: bool, seed: int, cache: str):
    from lsenerf_amd.data import draw_indices_host
    from oracle.model import adam_step
    torch.manual_seed(seed)
    model = build_model(contraction, seed)
    cams = sc.train_cameras()
    img = sc.images(cams)["rgb8"]
    params, opt = model.field.parameters(), {}
    curve, kept = [], []
    t0 = time.time()
    for k in range(CFG["steps"]):
        if k % CFG["occ_every"] == 0:
            with torch.no_grad():
                model.grid.update(k, lambda x: model.field.density_fn(x) * model.render_step_size, warmup_steps=CFG["occ_warmup_steps"])
        idx = draw_indices_host(CFG["draw_seed"], k, 0, CFG["rays_per_step"], len(cams), sc.H, sc.W)
        o = np.empty((len(idx), 3))
        d = np.empty((len(idx), 3))
        for c in np.unique(idx[:, 0]):
            m = idx[:, 0] == c
            o[m], d[m] = sc.pixel_rays(cams[c], idx[m, 1], idx[m, 2])
        o, d = torch.from_numpy(o).float(), torch.from_numpy(d).float()
        target = torch.from_numpy(img[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.float32) / 255.0)
        with torch.no_grad():
            ri, ts, te = model.sample(o, d)
        if ri.numel() == 0:
            ri, ts, te = torch.zeros(1, dtype=torch.int64), torch.ones(1), torch.ones(1)
        for p in params:
            p.grad = None
        out = model.render_samples(o, d, ri, ts, te)
        loss = ((out["rgb"] - target) ** 2).mean()
        loss.backward()
        adam_step(params, opt, lr=CFG["lr"], eps=CFG["eps"])
        curve.append(float(loss.detach()))
        kept.append(int(ri.numel()))
        if k % 20 == 0 or k == CFG["steps"] - 1:
            print(f"[{'on' if contraction else 'off'} {seed}] step {k} loss {curve[-1]:.3e} samples {kept[-1]} "
                  f"occupied {float(model.grid.binaries.float().mean()):.3f} {time.time() - t0:.0f}s", flush=True)
    torch.save({"params": {k: v.detach() for k, v in model.field.params.items()}, "occs": model.grid.occs,
                "binaries": model.grid.binaries, "curve": curve, "kept": kept, "seconds": time.time() - t0},
               state_path(cache, contraction, seed))


def load_model(contraction, seed, cache):
    st = torch.load(state_path(cache, contraction, seed))
    model = build_model(contraction, seed)
    for k, v in st["params"].items():
        model.field.params[k] = v.clone().requires_grad_(True)
    model.grid.occs, model.grid.binaries = st["occs"], st["binaries"]
    model.training = False
    model.field.training = False
    return model, st


# ---------------------------------------------------------------------------------------------------- measurements
def render(model, c2w, ys=None, xs=None):
    """Eval render of the oracle with the trained embedding row (``eval_emb_mode="mean"``, one row) -> dict of numpy arrays, the
    per-sample packed arrays included."""
    from oracle import volrend as vr
    from oracle.field import frustum_positions
    o, d = sc.pixel_rays(c2w, ys, xs)
    o, d = torch.from_numpy(o).float(), torch.from_numpy(d).float()
    n = o.shape[0]
    with torch.no_grad():
        ri, ts, te = model.sample(o, d)
        pos = frustum_positions(o[ri], d[ri], ts[:, None], te[:, None])
        density, geo = model.field.get_density(pos)
        rgb = model.field.get_outputs(d[ri], geo, None, eval_emb_mode="mean")
        packed = vr.pack_info(ri, n)
        w = vr.render_weight_from_density(ts, te, density[..., 0], packed)[0][..., None]
        out_rgb = vr.render_rgb(rgb, w, ri, n, False, "white")
        depth = vr.render_depth_expected(w, ts, te, ri, n)
        acc = vr.render_accumulation(w, ri, n)
    return dict(rgb=out_rgb.numpy().astype(np.float64), depth=depth.numpy().reshape(-1).astype(np.float64),
                acc=acc.numpy().reshape(-1).astype(np.float64), ri=ri.numpy(), ts=ts.numpy(), te=te.numpy(), w=w.numpy().reshape(-1),
                sigma=density[..., 0].numpy(), pos=pos, packed=packed.numpy(), o=o, d=d)


def composite_normals(model, r):
    """World normals: -grad(density logit) per sample by autograd through ``get_density``, normalised, composited with the render
    weights, renormalised.  -> [n_rays, 3]"""
    pos = r["pos"].clone().requires_grad_(True)
    density, _ = model.field.get_density(pos)
    logit = torch.log(density[..., 0].clamp_min(1e-30))
    (g,) = torch.autograd.grad(logit.sum(), pos)
    nrm = -g / g.norm(dim=-1, keepdim=True).clamp_min(1e-20)
    acc = np.zeros((r["o"].shape[0], 3))
    np.add.at(acc, r["ri"], nrm.numpy().astype(np.float64) * r["w"][:, None])
    return acc / np.maximum(np.linalg.norm(acc, axis=-1, keepdims=True), 1e-20)


def view_metrics(model, c2w, truth, want_normals=True):
    from tests import depth_quantiles_ref as dq
    r = render(model, c2w)
    hit, t = truth["hit"].ravel(), truth["t"].ravel()
    inner = sc.interior(truth["body"]).ravel()
    ih, im = inner & hit, inner & ~hit
    gt = truth["rgb8"].reshape(-1, 3) / 255.0
    m = dict(psnr=sc.psnr(r["rgb"], gt), psnr_interior=sc.psnr(r["rgb"], gt, inner),
             rms_interior=float(np.sqrt(((r["rgb"] - gt)[inner] ** 2).mean())),
             acc_hit_gt_0p9=float((r["acc"][ih] > 0.9).mean()), acc_miss_lt_0p1=float((r["acc"][im] < 0.1).mean()),
             separated=float(np.concatenate([r["acc"][ih] > 0.5, r["acc"][im] < 0.5]).mean()),
             interior_share=float(inner.mean()))
    for k, v in sc.err_stats(r["depth"][ih] - t[ih]).items():
        m["depth_" + k] = v
    med = median_depth(dq, r)
    for k, v in sc.err_stats(med[ih] - t[ih]).items():
        m["median_depth_" + k] = v
    if want_normals:
        nrm = composite_normals(model, r)
        cosang = np.clip((nrm[ih] * truth["normal"].reshape(-1, 3)[ih]).sum(-1), -1, 1)
        ang = np.degrees(np.arccos(cosang))
        m.update(normal_mean_deg=float(ang.mean()), normal_p95_deg=float(np.percentile(ang, 95)), normal_within_90=float((cosang > 0).mean()))
    return m, r, med


def median_depth(dq, r, interpolate=False, select=False):
    """The depth at which a ray's accumulated weight crosses one half (tests/depth_quantiles_ref.reference on the samples the render
    weights come from); ``select``: NaN where it never does, as the exporters' ``depth_selected``."""
    ref = dq.reference(r["ts"], r["te"], r["sigma"], r["packed"], dq.taus_of((0.5,)), interpolate=interpolate)
    d = ref["depth"][:, 0]
    return np.where(ref["reached"] & 1 == 1, d, np.nan) if select else d


def run_metrics(contraction, seed, cache):
    model, st = load_model(contraction, seed, cache)
    held = sc.heldout_cameras()
    truth = sc.images(held)
    res = dict(seconds=st["seconds"], loss_first=float(np.mean(st["curve"][:1])), loss_last=float(st["curve"][-1]),
               loss_ratio=float(st["curve"][-1] / st["curve"][0]), kept_first=st["kept"][0], kept_last=st["kept"][-1], views=[],
               init_checksum=init_checksum(hip_initialisation(contraction, seed)))
    for v in range(len(held)):
        m, _, _ = view_metrics(model, held[v], {k: a[v] for k, a in truth.items()})
        res["views"].append(m)
        print(f"[{'on' if contraction else 'off'} {seed}] view {v}", json.dumps(m), flush=True)
    res.update(occupancy_metrics(model))
    res.update(density_mesh_metrics(model))
    res.update(export_metrics(model))
    res.update(event_metrics(model))
    return res


def occupancy_metrics(model):
    pts, _, _ = sc.surface_samples(4000)
    r = CFG["grid_resolution"]
    ijk = np.clip(np.floor((pts + 1.0) / 2.0 * r).astype(np.int64), 0, r - 1)
    b = model.grid.binaries[0].numpy()
    cells = np.unique(ijk, axis=0)
    return dict(occupied_fraction=float(b.mean()), surface_cells_occupied=float(b[cells[:, 0], cells[:, 1], cells[:, 2]].mean()))


def density_mesh_metrics(model):
    from lsenerf_amd.mesh import DEFAULT_LEVEL
    from tests import mesh_ref as mr
    n = CFG["lattice"]
    res, lo, hi = (n,) * 3, [-1.0] * 3, [1.0] * 3
    pts = torch.from_numpy(mr.lattice_positions(res, lo, hi))
    with torch.no_grad():
        dens = torch.cat([model.field.get_density(pts[i:i + 32768])[0][:, 0] for i in range(0, len(pts), 32768)]).numpy()
    v, t = mr.surface_nets(dens, res, lo, hi, DEFAULT_LEVEL)[:2]
    cell = 2.0 / n
    out = {"density_mesh_" + k: x for k, x in sc.mesh_stats(v, t, mr.signed_volume, near=cell).items()}
    vt = torch.from_numpy(np.asarray(v, np.float32)).requires_grad_(True)      # vertex normals: -grad(density logit), in world coordinates
    (g,) = torch.autograd.grad(torch.log(model.field.get_density(vt)[0][:, 0].clamp_min(1e-30)).sum(), vt)
    facing = (-g.numpy().astype(np.float64) * sc.outward_normal(v)).sum(-1) > 0
    out["density_mesh_normals_within_90"] = float(facing.mean())
    out["density_mesh_normals_within_90_near"] = float(facing[np.abs(sc.sdf(v)) < cell].mean())
    return out


def export_metrics(model):
    """The exporters' twins over the training views' renders: tests/tsdf_ref (fusion, masked surface nets, fused colours) and
    tests/pointcloud_ref.unproject, with the exporters' defaults, for the expected and for the interpolated median depth."""
    from tests import depth_quantiles_ref as dq
    from tests import pointcloud_ref as pr
    from tests import tsdf_ref as tr
    cams = sc.train_cameras()
    truth = sc.images(cams)
    n = CFG["lattice"]
    res, lo, hi = (n,) * 3, [-1.0] * 3, [1.0] * 3
    renders = [render(model, c) for c in cams]
    inner = sc.interior(truth["body"]).reshape(len(cams), -1)
    gt = truth["rgb8"].reshape(len(cams), -1, 3) / 255.0
    rgb = np.stack([r["rgb"] for r in renders])
    out = dict(train_rms_interior=float(np.sqrt(((rgb - gt)[inner] ** 2).mean())))
    samples = sc.visible_surface_samples(cams)
    cam = tr.Camera(sc.FX, sc.FY, sc.CX, sc.CY, sc.H, sc.W)
    for mode in ("expected", "median"):
        depth = np.stack([r["depth"] if mode == "expected" else median_depth(dq, r, interpolate=True, select=True) for r in renders])
        acc = np.stack([r["acc"] for r in renders])
        tw, cw = tr.integrate(*tr.new_state(res), res, lo, hi, cam, cams.astype(np.float32), depth, acc, rgb, 3.0 * 2.0 / n, 0.5, True)
        v, _ = tr.surface_nets(tr.field(tw), res, lo, hi, 0.0)
        col = tr.vertex_colors(cw, res, lo, hi, v)
        for k, x in sc.cloud_stats(v, col, samples, 2 * 2.0 / n).items():
            out[f"tsdf_{mode}_{k}"] = x
        pts, cols = [], []
        for r, dep, c in zip(renders, depth, rgb):
            p, keep = pr.unproject(r["o"].numpy(), r["d"].numpy(), dep, r["acc"], lo, hi, 0.9)
            pts.append(p[keep]), cols.append(c[keep])
        for k, x in sc.cloud_stats(np.concatenate(pts), np.concatenate(cols), samples, 2 * 2.0 / n).items():
            out[f"cloud_{mode}_{k}"] = x
    return out


def event_metrics(model):
    traj = sc.trajectory_cameras()
    truth = sc.images(traj)
    want = sc.event_frames(truth["rgb8"] / 255.0, CFG["event_threshold"])
    from tests import events_ref as er
    c = CFG["event_threshold"]
    lg = np.stack([sc.log_gray(render(model, p)["rgb"]) for p in traj]).astype(np.float32)           # [8, H W] log-intensity planes
    got = np.stack([er.count(lg[k:k + 2], lg[k], c, c, 127)[0][0] for k in range(len(traj) - 1)]).reshape(want.shape).astype(np.float64)
    strong = np.abs(want) >= 2
    return dict(event_sign_agreement=float((np.sign(got[strong]) == np.sign(want[strong])).mean()), event_strong_share=float(strong.mean()),
                event_mean_difference=float((got - want).mean()))


# ---------------------------------------------------------------------------------------------------- driver
def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", default=None)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--parallel", type=int, default=3)
    ap.add_argument("--full", action="store_true", help="three seeds with contraction off as well")
    ap.add_argument("--train", default=None, help="internal: on|off,seed")
    ap.add_argument("--measure", default=None, help="internal: on|off,seed")
    ap.add_argument("--steps", type=int, default=None, help="try another step count (change analytic_scene.CONFIG to keep it)")
    args = ap.parse_args()
    if args.steps is not None:
        CFG["steps"] = args.steps
    torch.set_num_threads(args.threads)
    cache = args.cache or tempfile.mkdtemp(prefix="analytic_scene_")
    os.makedirs(cache, exist_ok=True)
    if args.train or args.measure:
        c, s = (args.train or args.measure).split(",")
        if args.train:
            train_one(c == "on", int(s), cache)
        else:
            with open(state_path(cache, c == "on", int(s)) + ".json", "w") as f:
                json.dump(run_metrics(c == "on", int(s), cache), f)
        return
    seeds = list(CFG["init_seeds"])
    runs = [(True, s) for s in seeds] + [(False, s) for s in (seeds if args.full else seeds[:1])]
    for what in ("--train", "--measure"):
        todo = [r for r in runs if not os.path.exists(state_path(cache, *r) + (".json" if what == "--measure" else ""))] \
            if what == "--train" else runs
        for i in range(0, len(todo), args.parallel):
            procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cache", cache, "--threads", str(args.threads),
                                       "--steps", str(CFG["steps"]), what, f"{'on' if c else 'off'},{s}"])
                     for c, s in todo[i:i + args.parallel]]
            if any(p.wait() != 0 for p in procs):
                raise SystemExit(f"{what} failed")
    doc = dict(config={k: (list(v) if isinstance(v, tuple) else v) for k, v in CFG.items()}, torch_version=torch.__version__,
               contraction_off_seeds=len(seeds) if args.full else 1,
               note=("contraction off: three seeds" if args.full else
                     "contraction off is recorded for one seed; its margin is the spread over the three seeds with contraction on"),
               runs={})
    for c, s in runs:
        with open(state_path(cache, c, s) + ".json") as f:
            doc["runs"].setdefault("contraction_on" if c else "contraction_off", {})[str(s)] = round_floats(json.load(f))
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


def round_floats(x):
    if isinstance(x, float):
        return float(f"{x:.5g}")
    if isinstance(x, dict):
        return {k: round_floats(v) for k, v in x.items()}
    if isinstance(x, list):
        return [round_floats(v) for v in x]
    return x


if __name__ == "__main__":
    main()
