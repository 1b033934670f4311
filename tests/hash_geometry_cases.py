"""Shared data and helpers of the hash-grid geometry tests (tests/test_hash_geometry_cpu.py, tests/test_gpu_hash_geometry.py).
Not a test file.

The reference is ``oracle/hashgrid.py`` (float32 with the fmaf emulation) and nothing else; tolerances are those of tests/util.py.
Everything here runs on the CPU: the geometry table, the seeded inputs, the oracle's results per geometry (computed once per
process and shared), the run-end counts that decide which path of the batched backward a wave takes, the comparison itself and the
mutated copies of the oracle that show the comparison would notice a subtly wrong kernel."""
from __future__ import annotations

import functools
from typing import Dict, Optional

import numpy as np
import torch

from oracle import hashgrid as ohg
from tests.util import TOL_FWD, TOL_GRAD, TOL_GRAD_BLOCK, blockwise_nmax_err, hash_level_bounds, nmax_err, rel_l2

# name -> keyword arguments of ops.make_grid_meta / oracle.hashgrid.tcnn_grid_meta (everything else: L 16, T 19, 16 -> 2048)
GEOMETRIES: Dict[str, dict] = {
    "L1": dict(n_levels=1),                                             # one level, scale 1, rep_lv = 1 = n_levels
    "L2_T10": dict(n_levels=2, log2_hashmap_size=10),                   # no dense level: replicated HASHED levels, res 16 -> 2048
    "L3_T14": dict(n_levels=3, log2_hashmap_size=14),                   # rep_lv = 3 < 4
    "L5_T12": dict(n_levels=5, log2_hashmap_size=12),                   # odd L, replicated levels at the T cap
    "L12_T17": dict(n_levels=12, log2_hashmap_size=17),                 # 3 dense levels
    "L20_T15_m4096": dict(n_levels=20, log2_hashmap_size=15, max_res=4096),     # more than 16 levels
    "L24_T14": dict(n_levels=24, log2_hashmap_size=14),                 # (L & 7) == 0 beyond 16
    "b64_m4096": dict(base_resolution=64, max_res=4096),                # replica budget met with equality, dense 64^3 = 2^18 exact fit
    "b48_m4096": dict(base_resolution=48, max_res=4096),                # rep_lv = 1 with two dense levels
    "b80_m4096": dict(base_resolution=80, max_res=4096),                # rep_lv = 0: no workspace at all
    "b32_m512": dict(base_resolution=32, max_res=512),                  # rep_lv = 3, growth 1.2
    "b16_m1024": dict(max_res=1024),                                    # Ed_HashEncoding's own default, 6 dense levels
    "b16_m128_L8_T22": dict(n_levels=8, max_res=128, log2_hashmap_size=22),     # every level dense, largest 128^3 = 2^21 exact fit
    "b2_m2048": dict(base_resolution=2),                                # levels of 8, 64, 216, 512 entries
    "b16_m16_L4": dict(n_levels=4, max_res=16),                         # four identical levels, per-level scale exactly 1
    "T4_L4": dict(n_levels=4, log2_hashmap_size=4),                     # 16-entry levels, everything collides
}
DEFAULT = "default"       # the grid every other hash test runs (not a row of the table; the GPU tier uses it as a partner)

# replica_floats() of csrc/hashgrid.hip: the replicated levels stop at min(replica_levels, n_levels) and at the first level that
# pushes one replica past 2 MB.  Pinned per geometry (computed once with the oracle's level table); the CPU tier holds both the
# restated rule below and the library against these numbers.
REP_LV = {"L1": 1, "L2_T10": 2, "L3_T14": 3, "L5_T12": 4, "L12_T17": 4, "L20_T15_m4096": 4, "L24_T14": 4, "b64_m4096": 1, "b48_m4096": 1,
          "b80_m4096": 0, "b32_m512": 3, "b16_m1024": 4, "b16_m128_L8_T22": 4, "b2_m2048": 4, "b16_m16_L4": 4, "T4_L4": 4, DEFAULT: 4}
REPLICA_BUDGET_FLOATS = (2 << 20) // 4


def geometry_kwargs(name: str) -> dict:
    return {} if name == DEFAULT else dict(GEOMETRIES[name])


def oracle_meta(name: str) -> ohg.TcnnGridMeta:
    return ohg.tcnn_grid_meta(**geometry_kwargs(name))


def restated_rep_lv(offsets, n_levels: int, replica_levels: int, replicas: int) -> int:
    lv = min(replica_levels, n_levels)
    while lv > 0 and 2 * offsets[lv] > REPLICA_BUDGET_FLOATS:
        lv -= 1
    return lv if replicas >= 2 else 0


def restated_dense(res: int, size: int) -> bool:
    """level_info() of csrc/hashgrid.hip: the stride loop runs while stride <= size; the level is hashed iff size < final stride."""
    stride, d = 1, 0
    while d < 3 and stride <= size:
        stride *= res
        d += 1
    return not (size < stride)


# ---------------------------------------------------------------------------------------------------- inputs
ZERO_BLOCKS = (1, 63, 64, 65, 130, 317)       # samples at exactly (0, 0, 0), as positions_fwd_kernel writes deselected samples
ZERO_LEAD = 5                                 # random points in front of the first block: no block starts at lane 0
# segment B: (rays, consecutive samples per ray, multiple of the automatic step).  The automatic step alone gives long runs on the
# coarse levels and short ones on the fine levels of a grid that has levels in between; with 8 rays x 256 samples at that step
# L1, L2_T10 and b16_m16_L4 (16^3 levels: 0.8 cells per 64 samples) end 1 .. 4, 8 or 64 runs per wave and never land between
# the thresholds (8, 48), so some rays are faster.  The CPU tier counts the paths for every geometry.
RAY_GROUPS = ((4, 256, 1.0), (2, 256, 4.0), (4, 128, 12.0))


def ray_coherent_points(n_rays, per_ray, seed, step_mult=1.0):
    from tests.test_gpu_parity import _ray_coherent_points
    return _ray_coherent_points(n_rays, per_ray, seed, step=2 * 3 ** 0.5 / 1000 / 4 * step_mult)


def make_points(seed: int = 0):
    """x [N, 3] float32 on the CPU and the index ranges of its segments: A 2048 uniform points (every lane ends a run), B 2048
    ray-coherent ones (``RAY_GROUPS``), C 640 samples at exactly the origin in blocks of ``ZERO_BLOCKS`` separated by single random
    points.  C starts ``ZERO_LEAD`` samples behind a multiple of 64, so its blocks begin at lanes 5, 7, 7, 8, 10 and 13: runs cross
    16-lane rows, 64-sample waves and 512-sample workgroups of the generic kernel.  N = 4746 (74 chunks of 64 + 10)."""
    g = torch.Generator().manual_seed(1000 + seed)
    a = torch.rand(2048, 3, generator=g)
    b = torch.cat([ray_coherent_points(r, per, seed=2000 + 10 * seed + i, step_mult=m) for i, (r, per, m) in enumerate(RAY_GROUPS)])
    parts, blocks = [torch.rand(ZERO_LEAD, 3, generator=g)], []
    pos = a.shape[0] + b.shape[0] + ZERO_LEAD
    for i, n in enumerate(ZERO_BLOCKS):
        if i:
            parts.append(torch.rand(1, 3, generator=g))
            pos += 1
        parts.append(torch.zeros(n, 3))
        blocks.append((pos, pos + n))
        pos += n
    c = torch.cat(parts)
    x = torch.cat([a, b, c]).float().contiguous()
    seg = {"A": (0, a.shape[0]), "B": (a.shape[0], a.shape[0] + b.shape[0]), "C": (a.shape[0] + b.shape[0], x.shape[0]),
           "zero_blocks": blocks}
    assert x.shape[0] == pos and x.shape[0] % 64 != 0 and x.shape[0] % 1024 != 0
    return x, seg


def make_out_of_range_points(seed: int = 0):
    """2048 finite points uniform in [-0.3, 1.3]^3 plus 64 with coordinates in [-4, 4]: tcnn's defined behaviour outside the unit
    cube (wrapping integer coordinates, exact modulo), which Ed_HashEncoding.forward promises as a drop-in."""
    g = torch.Generator().manual_seed(3000 + seed)
    near = torch.rand(2048, 3, generator=g) * 1.6 - 0.3
    far = torch.rand(64, 3, generator=g) * 8.0 - 4.0
    return torch.cat([near, far]).float().contiguous()


def on_face(x: torch.Tensor, scales) -> torch.Tensor:
    """Samples within 1e-4 (in ``pos`` units) of a cell face at some level: floor() there depends on the last bit of the position
    formula, and d(x) jumps across the face.  The only samples the d(x) comparison may skip."""
    m = torch.zeros(x.shape[0], dtype=torch.bool)
    for sc in scales:
        p = x.double() * sc + 0.5
        m |= ((p - p.round()).abs() < 1e-4).any(-1)
    return m


MAX_ON_FACE = 0.02


def oracle_results(meta_o: ohg.TcnnGridMeta, x: torch.Tensor, table: torch.Tensor, w: torch.Tensor) -> dict:
    """Forward, table gradient and d(x) of ``sum(encode(x) * w)`` by the oracle."""
    tc, xc = table.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y = ohg.hash_encode_tcnn(xc, tc, meta_o)                    # [N, L*2]
    (y * w).sum().backward()
    return {"x": x, "table": table, "w": w, "meta_o": meta_o, "y": y.detach(), "dt": tc.grad, "dx": xc.grad,
            "on_face": on_face(x, meta_o.scales)}


def make_case(name: str, x: Optional[torch.Tensor] = None, seed: int = 0):
    """(meta_o, x, segments, table U(-0.1, 0.1), w = randn [N, 2L]) -- the conventions of the existing hash tests."""
    meta_o = oracle_meta(name)
    seg = None
    if x is None:
        x, seg = make_points(seed)
    g = torch.Generator().manual_seed(4000 + seed + sum(map(ord, name)))
    table = (torch.rand(meta_o.n_params, generator=g) * 2 - 1) * 0.1
    w = torch.randn(x.shape[0], 2 * meta_o.n_levels, generator=g)
    return meta_o, x, seg, table, w


@functools.lru_cache(maxsize=None)
def reference(name: str) -> dict:
    """The oracle's results for geometry ``name`` on ``make_points(0)``: computed once per process, shared, never modified."""
    meta_o, x, seg, table, w = make_case(name)
    ref = oracle_results(meta_o, x, table, w)
    ref["segments"] = seg
    return ref


@functools.lru_cache(maxsize=None)
def reference_out_of_range(name: str) -> dict:
    meta_o, x, _, table, w = make_case(name, x=make_out_of_range_points(), seed=1)
    return oracle_results(meta_o, x, table, w)


def truncated(ref: dict, m: int) -> dict:
    """The oracle's results on the first ``m`` samples (forward and d(x) are per sample; the table gradient is summed again)."""
    tc = ref["table"].clone().requires_grad_(True)
    (ohg.hash_encode_tcnn(ref["x"][:m], tc, ref["meta_o"]) * ref["w"][:m]).sum().backward()
    return {**ref, "x": ref["x"][:m], "w": ref["w"][:m], "y": ref["y"][:m], "dx": ref["dx"][:m], "dt": tc.grad,
            "on_face": ref["on_face"][:m]}


def level_major(w: torch.Tensor) -> torch.Tensor:
    """[N, 2L] (tcnn's column order) -> [L, N, 2] (the layout the kernels read and write)."""
    n = w.shape[0]
    return w.reshape(n, -1, 2).permute(1, 0, 2).contiguous()


def sample_major(y: torch.Tensor) -> torch.Tensor:
    """[L, N, 2] -> [N, 2L]."""
    return y.permute(1, 0, 2).reshape(y.shape[1], -1)


# ---------------------------------------------------------------------------------------------------- which path a wave takes
def cell_coords(x: torch.Tensor, scale: float) -> torch.Tensor:
    """[N, 3] integer cell (p0, p1, p2) of the oracle's position formula."""
    pos = (x.double() * float(np.float32(scale)) + 0.5).to(torch.float32)
    return torch.floor(pos).to(torch.int64)


def run_end_counts(x: torch.Tensor, meta_o: ohg.TcnnGridMeta) -> torch.Tensor:
    """[chunks, L]: run ends per 64-sample chunk and level.  A run end is a change of the integer cell between neighbouring samples
    or the last sample of the chunk (the lanes behind the last sample repeat it: they end no run of their own)."""
    n = x.shape[0]
    chunks = (n + 63) // 64
    out = torch.zeros(chunks, meta_o.n_levels, dtype=torch.int64)
    for l in range(meta_o.n_levels):
        c = cell_coords(x, meta_o.scales[l])
        change = torch.zeros(chunks * 64, dtype=torch.bool)
        change[: n - 1] = (c[1:] != c[:-1]).any(-1)
        change = change.view(chunks, 64)
        change[:, 63] = True
        out[:, l] = change.sum(-1)
    return out


# ---------------------------------------------------------------------------------------------------- the comparison
def check_against_oracle(got_y, got_dt, got_dx, ref: dict, meta) -> Dict[str, float]:
    """Forward [N, 2L] level by level, each level on its own scale; table gradient globally, per level and in relative L2; d(x)
    on every sample that is not within 1e-4 of a cell face.  ``meta``: anything with ``offsets`` (GridMeta or TcnnGridMeta).
    Asserts, and returns the figures.  Any of the three may be None (not produced by the call under test)."""
    res: Dict[str, float] = {}
    L = len(meta.offsets) - 1
    if got_y is not None:
        y, y_ref = got_y.detach().cpu(), ref["y"]
        assert y.shape == y_ref.shape, (y.shape, y_ref.shape)
        assert bool(torch.isfinite(y).all())
        res["fwd"] = max(nmax_err(y[:, 2 * l:2 * l + 2], y_ref[:, 2 * l:2 * l + 2]) for l in range(L)) if y.numel() else 0.0
        assert res["fwd"] < TOL_FWD, res
    if got_dt is not None:
        dt, dt_ref = got_dt.detach().cpu(), ref["dt"]
        assert bool(torch.isfinite(dt).all())
        res["dt"] = nmax_err(dt, dt_ref)
        res["dt_blk"] = blockwise_nmax_err(dt, dt_ref, hash_level_bounds(meta))
        res["dt_l2"] = rel_l2(dt, dt_ref)
        assert res["dt"] < TOL_GRAD and res["dt_blk"] < TOL_GRAD_BLOCK and res["dt_l2"] < TOL_GRAD, res
    if got_dx is not None:
        dx, keep = got_dx.detach().cpu(), ~ref["on_face"]
        assert dx.shape == ref["dx"].shape and bool(torch.isfinite(dx).all())
        res["skipped"] = 1.0 - float(keep.float().mean()) if keep.numel() else 0.0
        assert res["skipped"] <= MAX_ON_FACE, res
        res["dx"] = nmax_err(dx[keep], ref["dx"][keep])
        assert res["dx"] < TOL_GRAD, res
    return res


# ---------------------------------------------------------------------------------------------------- mutated copies of the oracle
def encode_level(x, tab, scale: float, res: int, size: int, dense: bool, drop_axis: Optional[int] = None, drop_rows=None):
    """One level of ``oracle.hashgrid.hash_encode_tcnn``, restated so that it can be made wrong on purpose (``tab`` [size', 2]: the
    level's own entries).  ``drop_axis`` / ``drop_rows``: the samples ``drop_rows`` (bool [N]) lose the +1 of their corners along
    ``drop_axis`` in the INDEX (weights untouched) -- a corner read from the wrong entry.  Unmutated it reproduces the oracle bit
    for bit (held in tests/test_hash_geometry_cpu.py)."""
    pos = (x.double() * float(np.float32(scale)) + 0.5).to(x.dtype)
    p0 = torch.floor(pos)
    w = pos - p0
    p0i = p0.detach().to(torch.int64) & 0xFFFFFFFF
    acc = torch.zeros(x.shape[0], 2, dtype=x.dtype)
    for c in range(8):
        wgt = torch.ones(x.shape[0], dtype=x.dtype)
        cs = []
        for d in range(3):
            if (c >> d) & 1:
                wgt = wgt * w[:, d]
                plus = (p0i[:, d] + 1) & 0xFFFFFFFF
                cs.append(torch.where(drop_rows, p0i[:, d], plus) if d == drop_axis else plus)
            else:
                wgt = wgt * (1 - w[:, d])
                cs.append(p0i[:, d])
        idx = ohg._tcnn_index(cs[0], cs[1], cs[2], res, size, dense)
        acc = acc + wgt[:, None] * tab[idx]
    return acc


def results_with_level(ref: dict, level: int, **mut) -> dict:
    """``ref`` with ONE level replaced by ``encode_level`` (keywords: size / dense / drop_axis / drop_rows override the oracle's):
    y columns, table-gradient block and that level's share of d(x).  Without keywords the result equals ``ref``."""
    m: ohg.TcnnGridMeta = ref["meta_o"]
    lo, hi = m.offsets[level], m.offsets[level + 1]
    kw = dict(size=hi - lo, dense=m.is_dense(level), drop_axis=None, drop_rows=None)
    plain = dict(kw)
    kw.update(mut)
    wl = ref["w"][:, 2 * level:2 * level + 2]
    out = {}
    for key, k in (("plain", plain), ("mut", kw)):
        xc = ref["x"].clone().requires_grad_(True)
        tl = ref["table"].reshape(-1, 2)[lo:hi].clone().requires_grad_(True)
        yl = encode_level(xc, tl, m.scales[level], m.resolutions[level], **k)
        (yl * wl).sum().backward()
        out[key] = (yl.detach(), tl.grad.reshape(-1), xc.grad)
    y, dt = ref["y"].clone(), ref["dt"].clone()
    assert torch.equal(out["plain"][0], y[:, 2 * level:2 * level + 2]), "encode_level must restate the oracle bit for bit"
    y[:, 2 * level:2 * level + 2] = out["mut"][0]
    dt[2 * lo:2 * hi] = out["mut"][1]
    dx = ref["dx"] - out["plain"][2] + out["mut"][2]
    return {"y": y, "dt": dt, "dx": dx}


def dense_levels(m: ohg.TcnnGridMeta):
    return [l for l in range(m.n_levels) if m.is_dense(l)]


def padded_dense_levels(m: ohg.TcnnGridMeta):
    """Dense levels whose res^3 is not a multiple of 8: the level is res^3 padded up, and the fold-back of the dense index must use
    the padded size."""
    return [l for l in dense_levels(m) if m.resolutions[l] ** 3 != m.level_size(l)]


def mutation_dense_as_hashed(ref: dict):
    """(a) the finest dense level indexed with the hash."""
    lv = dense_levels(ref["meta_o"])
    return results_with_level(ref, lv[-1], dense=False) if lv else None


def folding_levels(m: ohg.TcnnGridMeta, x: torch.Tensor):
    """The padded dense levels at which some corner of some sample of ``x`` has a raw dense index >= res^3, so that the fold-back
    ``idx % size`` is taken at all.  For inputs in [0, 1] that needs p + 1 == res along z: only levels whose scale has a fractional
    part >= 0.5 get there (res = ceil(scale) + 1); elsewhere a wrong fold-back size computes the same values and is no error."""
    out = []
    for l in padded_dense_levels(m):
        r = m.resolutions[l]
        c = (cell_coords(x, m.scales[l]) & 0xFFFFFFFF) + 1
        c = c & 0xFFFFFFFF
        if bool((((c[:, 0] + c[:, 1] * r + c[:, 2] * r * r) & 0xFFFFFFFF) >= r ** 3).any()):
            out.append(l)
    return out


def mutation_unpadded_size(ref: dict):
    """(b) a dense level's size taken as res^3, without the pad to 8 (the finest level at which that changes an index)."""
    m = ref["meta_o"]
    lv = folding_levels(m, ref["x"])
    return results_with_level(ref, lv[-1], size=m.resolutions[lv[-1]] ** 3) if lv else None


def mutation_lost_corner(ref: dict, axis: int = 0):
    """(c) the last sample of every 64-sample chunk loses the +1 along one axis, at one level only (the finest)."""
    n = ref["x"].shape[0]
    rows = torch.zeros(n, dtype=torch.bool)
    rows[63::64] = True
    return results_with_level(ref, ref["meta_o"].n_levels - 1, drop_axis=axis, drop_rows=rows)


def mutation_lost_replica(ref: dict, rep_lv: int):
    """(d) one of 16 replicas of the last replicated level never reaches the table gradient."""
    if rep_lv <= 0:
        return None
    m = ref["meta_o"]
    dt = ref["dt"].clone()
    dt[2 * m.offsets[rep_lv - 1]:2 * m.offsets[rep_lv]] *= 15.0 / 16.0
    return {"y": ref["y"], "dt": dt, "dx": ref["dx"]}
