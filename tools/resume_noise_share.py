#!/usr/bin/env python3
"""The figure behind the parameter-update criterion of tests/test_gpu_resume.py: how large a share of one Adam update moves by more
than ``1e-5 * max|parameters|`` when the gradient of that step is off by float-atomic noise.

Trains ``oracle.model.ModelOracle`` on the analytic scene exactly as tests/golden/make_analytic_scene.py does (same configuration,
pixels and initialisation) for steps 0 .. K-1, then takes step K twice from the same parameters and moments: once on the gradient
as computed, once on that gradient perturbed by ``rel`` (uniform in [-1, 1] per element) in three forms: relative to each element;
relative to the tensor's largest element on the elements that received a gradient (what ``tests.util.nmax_err`` < rel, the bar the
GPU tests hold two gradients of identical parameters to, admits at worst); and that on every element.  Prints the share of
elements whose updates differ by more than ``1e-5 * max|parameters|`` -- the criterion of tests/test_gpu_graph.py.  CPU only.

    python tools/resume_noise_share.py [--k 264] [--rel 3e-5] [--threads 4]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests import analytic_scene as sc  # noqa: E402
from tests.golden import make_analytic_scene as gen  # noqa: E402

CFG = sc.CONFIG


def batch_of(k, cams, img):
    from lsenerf_amd.data import draw_indices_host
    idx = draw_indices_host(CFG["draw_seed"], k, 0, CFG["rays_per_step"], len(cams), sc.H, sc.W)
    o, d = np.empty((len(idx), 3)), np.empty((len(idx), 3))
    for c in np.unique(idx[:, 0]):
        m = idx[:, 0] == c
        o[m], d[m] = sc.pixel_rays(cams[c], idx[m, 1], idx[m, 2])
    target = torch.from_numpy(img[idx[:, 0], idx[:, 1], idx[:, 2]].astype(np.float32) / 255.0)
    return torch.from_numpy(o).float(), torch.from_numpy(d).float(), target


def gradient(model, params, o, d, target):
    with torch.no_grad():
        ri, ts, te = model.sample(o, d)
    if ri.numel() == 0:
        ri, ts, te = torch.zeros(1, dtype=torch.int64), torch.ones(1), torch.ones(1)
    for p in params:
        p.grad = None
    loss = ((model.render_samples(o, d, ri, ts, te)["rgb"] - target) ** 2).mean()
    loss.backward()
    return float(loss.detach())


def main():
    from oracle.model import adam_step
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=264)
    ap.add_argument("--rel", type=float, default=3e-5)
    ap.add_argument("--threads", type=int, default=4)
    ap.add_argument("--seed", type=int, default=CFG["init_seeds"][0])
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    torch.manual_seed(args.seed)
    model = gen.build_model(True, args.seed)
    cams = sc.train_cameras()
    img = sc.images(cams)["rgb8"]
    params, opt = model.field.parameters(), {}
    t0 = time.time()
    for k in range(args.k + 1):
        if k % CFG["occ_every"] == 0:
            with torch.no_grad():
                model.grid.update(k, lambda x: model.field.density_fn(x) * model.render_step_size, warmup_steps=CFG["occ_warmup_steps"])
        loss = gradient(model, params, *batch_of(k, cams, img))
        if k == args.k:
            break
        adam_step(params, opt, lr=CFG["lr"], eps=CFG["eps"])
        if k % 20 == 0:
            print(f"step {k} loss {loss:.3e} {time.time() - t0:.0f}s", flush=True)
    # step K, twice, from the same parameters and moments
    grads = [p.grad.detach().clone() for p in params]
    before = [p.detach().clone() for p in params]
    scale = max(float(p.abs().max()) for p in before)

    def update(gs):
        st = {key: (v.clone() if torch.is_tensor(v) else v) for key, v in opt.items()}
        with torch.no_grad():
            for p, b, g in zip(params, before, gs):
                p.copy_(b)
                p.grad = g.clone()
        adam_step(params, st, lr=CFG["lr"], eps=CFG["eps"])
        return torch.cat([(p.detach() - b).reshape(-1) for p, b in zip(params, before)])

    clean = update(grads)
    print(f"RESUME cpu perturbation: step {args.k}, loss {loss:.4e}, elements {clean.numel()}, max|parameters| {scale:.4g}, "
          f"elements with a non-zero update {int((clean != 0).sum())}")
    # "element": every element off by rel of ITSELF (an element no sample touched stays exactly zero, as on the device);
    # "touched": every non-zero element off by rel of its tensor's max (the worst case nmax_err < rel admits);
    # "all": every element, the untouched ones too, off by rel of its tensor's max (no device sum does that: recorded as the ceiling)
    forms = {"element": lambda x, u: x * (1 + args.rel * u),
             "touched": lambda x, u: x + args.rel * float(x.abs().max()) * u * (x != 0),
             "all": lambda x, u: x + args.rel * float(x.abs().max()) * u}
    for form, perturb in forms.items():
        for s in range(2):
            g = torch.Generator().manual_seed(100 + s)
            noisy = [perturb(x, 2 * torch.rand(x.shape, generator=g, dtype=x.dtype) - 1) for x in grads]
            diff = (update(noisy) - clean).abs()
            share = float((diff > 1e-5 * scale).double().mean())
            print(f"RESUME cpu perturbation [{form}, seed {100 + s}]: gradient off by {args.rel:g}: share of the update off by more than "
                  f"1e-5 x {scale:.4g} = {share:.6f}   (criterion: < 0.02)   largest difference {float(diff.max()):.3g}")


if __name__ == "__main__":
    main()
