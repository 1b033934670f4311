"""The hash-grid kernels at the geometries of tests/hash_geometry_cases.py against oracle/hashgrid.py: every row of the table
through the autograd path training takes (shared replica workspace included) with both threshold pairs, the generic backward
kernel, device-side sample counts, level ranges combined with replicas, several grids sharing one workspace, and positions outside
the unit cube.  tests/test_hash_geometry_cpu.py shows that the shared inputs reach every path of the batched backward at every
geometry and that ``check_against_oracle`` rejects subtly wrong results.  Tolerances: tests/util.py, unchanged."""
import ctypes
import dataclasses

import pytest
import torch

from tests import hash_geometry_cases as hc
from tests.util import nmax_err

pytestmark = pytest.mark.gpu


def _ops():
    from lsenerf_amd import ops
    return ops


def _P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _meta(name, tuning=()):
    return dataclasses.replace(_ops().make_grid_meta(**hc.geometry_kwargs(name)), bwd_tuning=tuple(tuning))


def _workspace_reads_zero():
    """The shared replica workspace(s) of ops.hash_encode's backward, where one exists, read all zero."""
    for ws in _ops()._HASH_BWD_WS.values():
        assert not bool(ws.any()), "the replica workspace must read zero again after a backward"


def _autograd(name, ref, tuning=()):
    """Forward + backward through ops.hash_encode on the GPU: (y [N, 2L], d table, d x)."""
    ops = _ops()
    meta = _meta(name, tuning)
    xg = ref["x"].cuda().requires_grad_(True)
    tg = ref["table"].cuda().requires_grad_(True)
    y = hc.sample_major(ops.hash_encode(xg, tg, meta))
    (y * ref["w"].cuda()).sum().backward()
    _workspace_reads_zero()
    return y.detach(), tg.grad, xg.grad


def _report(tag, res):
    print("HASHGEOM " + tag + " " + " ".join(f"{k}={v:.3e}" for k, v in res.items()))


def _tunings():
    return {"default": (), "dense_steps": _ops().HASH_BWD_DENSE_STEPS}


# ------------------------------------------------------------------------------------------------ 1: every geometry
@pytest.mark.parametrize("name", list(hc.GEOMETRIES))
def test_hash_fwd_bwd_every_geometry(name):
    ref = hc.reference(name)
    meta_o = ref["meta_o"]
    assert list(_meta(name).offsets) == meta_o.offsets
    for tag, tuning in _tunings().items():
        y, dt, dx = _autograd(name, ref, tuning)
        res = hc.check_against_oracle(y, dt, dx, ref, meta_o)
        _report(f"{name} {tag}", res)


# ------------------------------------------------------------------------------------------------ 2: the generic kernel
@pytest.mark.parametrize("name", ["L1", "b2_m2048", "b64_m4096", "T4_L4"])
def test_hash_bwd_generic_kernel(name):
    """impl 0, the 16-lanes-per-sample kernel: the shipped fallback, which had only ever seen the default grid."""
    from tests.test_gpu_parity import _hash_bwd_ex
    ops = _ops()
    ref = hc.reference(name)
    meta = _meta(name)
    xg, tg = ref["x"].cuda(), ref["table"].cuda()
    with torch.no_grad():
        y = hc.sample_major(ops.hash_encode(xg, tg, meta))
    dt, dx = _hash_bwd_ex(ops, meta, xg, hc.level_major(ref["w"]).cuda(), tg, impl=0)
    res = hc.check_against_oracle(y, dt, dx, ref, ref["meta_o"])
    _report(f"{name} generic", res)


# ------------------------------------------------------------------------------------------------ 3: device-side counts
@pytest.mark.parametrize("name", ["L1", "b64_m4096", "T4_L4"])
def test_hash_device_side_counts(name):
    """Arrays of capacity N, the count on the device: rows below the count against the oracle on the truncated arrays, nothing at
    or beyond it written (sentinel-filled outputs through the C ABI)."""
    from lsenerf_amd import _lib
    ops = _ops()
    ref = hc.reference(name)
    meta, meta_o = _meta(name), ref["meta_o"]
    L, cap = meta.n_levels, ref["x"].shape[0]
    xg, tg = ref["x"].cuda(), ref["table"].cuda()
    dy = hc.level_major(ref["w"]).cuda()                      # [L, cap, 2]: the capacity is the level stride
    desc = meta.desc()
    assert not bool(ref["on_face"][0])                        # (the one-sample case compares d(x) of sample 0)
    for n_dev in (0, 1, cap - 777, cap, cap + 5):
        cnt = torch.tensor([n_dev], dtype=torch.int64, device="cuda")
        y = torch.full((L, cap, 2), 7.0, device="cuda")
        _lib.call("lse_hash_fwd", ctypes.byref(desc), _P(xg), _P(tg), _P(y), cap, _P(cnt), ops._stream())
        dt, dx = torch.zeros_like(tg), torch.full_like(xg, 7.0)
        opts = ops.hash_bwd_opts_with_workspace(desc, xg.device)
        _lib.call("lse_hash_bwd_ex", ctypes.byref(desc), _P(xg), _P(dy), _P(tg), _P(dt), _P(dx), 0, 0, L, cap, _P(cnt),
                  ctypes.byref(opts), ops._stream())
        _workspace_reads_zero()
        m = min(n_dev, cap)
        assert bool((y[:, m:] == 7.0).all()) and bool((dx[m:] == 7.0).all()), n_dev
        if m == 0:
            assert not bool(dt.any())
            continue
        sub = ref if m == cap else hc.truncated(ref, m)
        res = hc.check_against_oracle(hc.sample_major(y[:, :m]), dt, dx[:m], sub, meta_o)
        _report(f"{name} n_dev={n_dev}", res)


# ------------------------------------------------------------------------------------------------ 4: level ranges + replicas
@pytest.mark.parametrize("name", [hc.DEFAULT, "b32_m512"])
def test_hash_bwd_level_ranges_with_a_replica_workspace(name):
    """Two lse_hash_bwd_ex calls, [s, L) and then [0, s) accumulating, with the replica workspace: the split below, at and above
    the last replicated level."""
    from lsenerf_amd import _lib
    ops = _ops()
    ref = hc.reference(name)
    meta, meta_o = _meta(name), ref["meta_o"]
    L, n, rep_lv = meta.n_levels, ref["x"].shape[0], hc.REP_LV[name]
    xg, tg = ref["x"].cuda(), ref["table"].cuda()
    dy = hc.level_major(ref["w"]).cuda()
    desc = meta.desc()
    opts = ops.hash_bwd_opts_with_workspace(desc, xg.device)
    assert opts.workspace and opts.workspace_bytes >= opts.replicas * 4 * 2 * meta.offsets[rep_lv]

    def call(dt, dx, acc, lo, hi):
        _lib.call("lse_hash_bwd_ex", ctypes.byref(desc), _P(xg), _P(dy), _P(tg), _P(dt), _P(dx), acc, lo, hi, n, None,
                  ctypes.byref(opts), ops._stream())
        _workspace_reads_zero()

    one_t, one_x = torch.zeros_like(tg), torch.full_like(xg, 7.0)
    call(one_t, one_x, 0, 0, L)
    _report(f"{name} one call", hc.check_against_oracle(None, one_t, one_x, ref, meta_o))
    for s in sorted({1, 2, rep_lv, rep_lv + 1, L - 1}):
        part_t, part_x = torch.zeros_like(tg), torch.full_like(xg, 7.0)       # the first call overwrites d(x)
        call(part_t, part_x, 0, s, L)
        lo = 2 * meta.offsets[s]
        assert float(part_t[:lo].abs().max()) == 0.0 and float(part_t[lo:].abs().max()) > 0, s
        call(part_t, part_x, 1, 0, s)
        # same kernel, the levels dealt to two launches: summation order only
        assert nmax_err(part_t, one_t) < 1e-5 and nmax_err(part_x, one_x) < 1e-5, s
        _report(f"{name} split at {s}", hc.check_against_oracle(None, part_t, part_x, ref, meta_o))


# ------------------------------------------------------------------------------------------------ 5: one workspace, several grids
def test_grids_of_different_geometry_share_one_replica_workspace():
    """One process, one stream: default -> b64_m4096 (a larger workspace, another replica stride) -> b2_m2048 (a tiny one inside
    the same buffer) -> default again.  Each against its own oracle; the second default run equals the first to summation order."""
    runs = []
    for name in (hc.DEFAULT, "b64_m4096", "b2_m2048", hc.DEFAULT):
        ref = hc.reference(name)
        y, dt, dx = _autograd(name, ref)
        _report(f"{name} shared workspace", hc.check_against_oracle(y, dt, dx, ref, ref["meta_o"]))
        runs.append((y, dt, dx))
    assert len(_ops()._HASH_BWD_WS) >= 1
    (y0, dt0, dx0), (y1, dt1, dx1) = runs[0], runs[-1]
    assert torch.equal(y0, y1)
    assert nmax_err(dt1, dt0) < 1e-5 and nmax_err(dx1, dx0) < 1e-5


# ------------------------------------------------------------------------------------------------ 6: outside the unit cube
@pytest.mark.parametrize("name", [hc.DEFAULT, "b16_m128_L8_T22", "L2_T10"])
def test_hash_out_of_range_positions(name):
    """tcnn's behaviour outside [0, 1]: integer coordinates wrap in uint32 and the index is the exact modulo.  Every index producer
    of csrc/hashgrid.hip reduces its result below the level's size for ANY uint32 coordinates -- grid_index() ends in a plain
    modulo on the dense branch and in a mask or modulo on the hashed one, corner_indices() does the same per corner, and no kernel
    (generic, batched, or the development build's cached / coarse / LDS-resident ones) forms a table index any other way; the
    replica offset adds 2 * (level offset + index) < rep_stride.  So these inputs cannot index out of bounds."""
    from tests.test_gpu_parity import _hash_bwd_ex
    ops = _ops()
    ref = hc.reference_out_of_range(name)
    x = ref["x"]
    assert bool(torch.isfinite(x).all()) and float(x.min()) < -3 and float(x.max()) > 3
    y, dt, dx = _autograd(name, ref)
    res = hc.check_against_oracle(y, dt, dx, ref, ref["meta_o"])
    _report(f"{name} out of range", res)
    dt0, dx0 = _hash_bwd_ex(ops, _meta(name), x.cuda(), hc.level_major(ref["w"]).cuda(), ref["table"].cuda(), impl=0)
    _report(f"{name} out of range generic", hc.check_against_oracle(None, dt0, dx0, ref, ref["meta_o"]))
