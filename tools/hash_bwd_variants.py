#!/usr/bin/env python3
"""Whole-kernel time of hash-backward settings (lse_hash_bwd_ex options) on M-march / M-packed positions, interleaved rounds.
usage: python tools/hash_bwd_variants.py "impl=0" "impl=2 second_probe=1" "impl=2 nodx=1 lib=/path/to/other/liblse_hip.so" "fwd=1" ...
A variant is a string of key=value pairs: the fields of lse_hash_bwd_opts, plus
  nodx=1    no d(x) (dx = NULL)
  fwd=1     time lse_hash_fwd instead of the backward
  lib=PATH  make the same call through that library (ctypes.CDLL; its own lse_hash_bwd_default_opts fills the options)"""
import ctypes, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch
from lsenerf_amd import ops, _lib
import bench
dev = torch.device("cuda", 0)
R, S = 4096, 1024
ROUNDS = 12       # the first one is a warm-up: 11 timed
P = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None


def fixed(o, d):
    step = 2 * 3 ** 0.5 / 1000
    ts = (0.05 + step * torch.arange(S, dtype=torch.float32)).repeat(R).to(dev)
    ri = torch.repeat_interleave(torch.arange(R, dtype=torch.int32), S).to(dev)
    cnt = torch.full((R,), S, dtype=torch.long)
    packed = torch.stack([torch.cumsum(cnt, 0) - cnt, cnt], -1).to(dev).contiguous()
    return ops.positions(o.to(dev), d.to(dev), ri, ts, ts + step, packed, True, None)[0]


def default_config_positions():
    from lsenerf_amd import LSENeRFModel, LSENeRFModelConfig, RayBundle
    torch.manual_seed(96)
    model = LSENeRFModel(LSENeRFModelConfig(), torch.tensor([[-1.0, -1, -1], [1, 1, 1]]), num_train_data=64).to(dev).train()
    with torch.no_grad():
        model.field.mlp_base_grid.params.mul_(3000.0)
        model.field.mlp_base_mlp.params[-16 * 64:-15 * 64].mul_(6.0)
    o, d = bench.sphere_rays(R, torch.Generator().manual_seed(7))
    rb = RayBundle(origins=o.to(dev), directions=d.to(dev), camera_indices=torch.zeros(R, 1, dtype=torch.long, device=dev))
    cb = model.update_occupancy_grid
    for s_ in range(0, 64, 16):
        cb(s_)
    rs, _ = model.sampler(ray_bundle=rb, near_plane=0.05, far_plane=1e3, render_step_size=model.config.render_step_size,
                          alpha_thre=0.01, cone_angle=0.004)
    return ops.positions(rb.origins, rb.directions, rs.ray_indices, rs.frustums.starts[..., 0].contiguous(),
                         rs.frustums.ends[..., 0].contiguous(), rs.packed_info, True, None)[0]


def headline_positions():
    """bench.py's headline step (SURVEY 8d exact: sphere rays, one-level grid fully occupied, step chosen for 1024 samples per ray)."""
    model, _sets, _ = bench.build_workload(dev, 1000)      # (one ray set: the round-1..4 fixed draw)
    rb, _, jitter = _sets[0]
    cfg = model.config
    with torch.no_grad():
        ri, ts, te, packed = model.occupancy_grid.sampling(
            rb.origins.detach(), rb.directions.detach(), near_plane=cfg.near_plane, far_plane=cfg.far_plane,
            render_step_size=cfg.render_step_size, stratified=True, jitter=jitter, return_packed=True)[:4]
        return ops.positions(rb.origins.detach(), rb.directions.detach(), ri, ts, te, packed, True, None)[0]


def make_regimes():
    g = torch.Generator().manual_seed(1)
    torch.rand(ops.make_grid_meta().n_params, generator=g)      # (the table's draw comes first from this generator: main)
    o_in = torch.rand(R, 3, generator=g) - 0.5
    d_in = torch.randn(R, 3, generator=g); d_in = d_in / d_in.norm(dim=-1, keepdim=True)
    o_sp, d_sp = bench.sphere_rays(R, torch.Generator().manual_seed(96))
    return {"headline": headline_positions(), "M-march(inside box)": fixed(o_in, d_in), "M-packed": fixed(o_sp, d_sp),
            "default": default_config_positions()}


_other_libs = {}


def other_library(path):
    """A second library of the same ABI, loaded next to the process's own one (its own instance: its own code objects)."""
    if path not in _other_libs:
        lib = ctypes.CDLL(path)
        for name in ("lse_hash_fwd", "lse_hash_bwd_ex", "lse_hash_bwd_input"):
            getattr(lib, name).argtypes = _lib.SIGNATURES[name]
            getattr(lib, name).restype = ctypes.c_int32
        lib.lse_hash_bwd_default_opts.restype = None
        lib.lse_hash_bwd_default_opts.argtypes = [ctypes.POINTER(_lib.HashBwdOpts)]
        lib.lse_hash_bwd_workspace_bytes.restype = ctypes.c_int64
        lib.lse_hash_bwd_workspace_bytes.argtypes = [ctypes.POINTER(_lib.GridDesc), ctypes.POINTER(_lib.HashBwdOpts)]
        lib.lse_last_error.restype = ctypes.c_char_p
        _other_libs[path] = lib
    return _other_libs[path]


def make_call(variant, meta, desc, table, x01, dy, dt, dx, y):
    """variant string -> a function of no arguments that enqueues the call on the current stream"""
    kv = dict(t.split("=", 1) for t in variant.split())
    lib = other_library(kv.pop("lib")) if "lib" in kv else _lib.load()
    nodx, fwd = bool(int(kv.pop("nodx", 0))), bool(int(kv.pop("fwd", 0)))
    n = x01.shape[0]

    def checked(rc):
        if rc != 0:
            raise RuntimeError(f"{variant}: {lib.lse_last_error().decode()}")
    if fwd:
        return lambda: checked(lib.lse_hash_fwd(ctypes.byref(desc), P(x01), P(table), P(y), n, None, ops._stream()))
    o = _lib.HashBwdOpts()
    lib.lse_hash_bwd_default_opts(ctypes.byref(o))
    for k, val in kv.items():
        setattr(o, k, float(val) if k == "interleave_from_scale" else int(val))
    nb = int(lib.lse_hash_bwd_workspace_bytes(ctypes.byref(desc), ctypes.byref(o)))
    if nb:      # the product path's replica workspace (ops.hash_bwd_opts_with_workspace)
        o._ws = torch.zeros(nb // 4, dtype=torch.float32, device=dev)
        o.workspace, o.workspace_bytes = o._ws.data_ptr(), nb
    return lambda: checked(lib.lse_hash_bwd_ex(ctypes.byref(desc), P(x01), P(dy), P(table), P(dt), None if nodx else P(dx), 0, 0,
                                               meta.n_levels, n, None, ctypes.byref(o), ops._stream()))


def time_variants(variants, meta, table, x01, rounds=ROUNDS):
    """{variant: sorted list of the timed rounds, ms}: the variants take turns inside every round"""
    n = x01.shape[0]
    desc = meta.desc()
    dy = torch.randn(meta.n_levels, n, 2, device=dev)
    dt = torch.zeros_like(table); dx = torch.empty_like(x01)
    y = torch.empty(meta.n_levels, n, 2, device=dev)
    fns = [(v, make_call(v, meta, desc, table, x01, dy, dt, dx, y)) for v in variants]
    times = {v: [] for v in variants}
    for rnd in range(rounds):
        for v, fn in fns:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record(); torch.cuda.synchronize()
            if rnd: times[v].append(e0.elapsed_time(e1))
    return {v: sorted(t) for v, t in times.items()}


if __name__ == "__main__":
    meta = ops.make_grid_meta()
    table = ((torch.rand(meta.n_params, generator=torch.Generator().manual_seed(1)) * 2 - 1) * 1e-2).to(dev)
    variants = sys.argv[1:] or ["impl=2", "impl=0"]
    for name, x01 in make_regimes().items():
        for v, t in time_variants(variants, meta, table, x01).items():
            print(f"{name:20s} {v:40s} median {t[len(t)//2]:.3f} ms  min {t[0]:.3f}  max {t[-1]:.3f}", flush=True)
