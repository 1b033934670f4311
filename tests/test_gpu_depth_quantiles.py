"""``lse_eval_depth_quantiles`` and its segmented form through ``ops``, against the float64 reference of
tests/depth_quantiles_ref.py on the trained-scene generator of tests/util.py (ray lengths 0 .. 2000, surfaces on both sides of the
64-lane group border and on the last sample), and against each other bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import depth_quantiles_ref as dr
from tests.test_depth_quantiles_cpu import two_surface_ray
from tests.util import FIXED_RAY_LENGTHS, SURFACE_SIGMAS, select_rays, trained_scene_rays

pytestmark = pytest.mark.gpu

F = np.float32
QS = (0.25, 0.5, 0.75)
QS4 = (0.25, 0.5, 0.75, 1 - 1e-4)          # the last one is the early-stop threshold itself: 1 - q >= 1e-4 just holds
KEYS = ("ts", "te", "sigma", "packed_info")


@functools.lru_cache(maxsize=None)
def _inputs(sg, step="const", onset="abrupt", seed=0):
    """(generator output on the CPU, its four arrays on the device).  Read-only."""
    inp = trained_scene_rays(sg, seed=seed, step=step, onset=onset)
    assert tuple(inp["packed_info"][:len(FIXED_RAY_LENGTHS), 1].tolist()) == FIXED_RAY_LENGTHS
    return inp, tuple(inp[k].cuda() for k in KEYS)


def _run(dev_args, qs, interpolate=False, sel=None, max_spread=None):
    """(depth_q, reached, depth_sel or None) as numpy, from outputs pre-filled with NaN / 0xFF and one guard row behind them."""
    from lsenerf_amd import ops
    n = dev_args[3].shape[0]
    dq = torch.full((n + 1, len(qs)), float("nan"), device="cuda")
    reached = torch.full((n + 1,), 0xFF, dtype=torch.uint8, device="cuda")
    ds = torch.full((n + 1,), 7.0, device="cuda") if sel is not None else None
    ops.eval_depth_quantiles(*dev_args, [ops.depth_tau(q) for q in qs], dq[:n], reached[:n], None if ds is None else ds[:n],
                             interpolate=interpolate, sel=sel or 0, max_spread=max_spread)
    assert bool(torch.isnan(dq[n]).all()) and int(reached[n]) == 0xFF and (ds is None or float(ds[n]) == 7.0)     # the guard row
    assert not bool(torch.isnan(dq[:n]).any())                                                                    # every ray is written
    return dq[:n].cpu().numpy(), reached[:n].cpu().numpy(), None if ds is None else ds[:n].cpu().numpy()


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("sg", SURFACE_SIGMAS, ids=[f"{s:g}" for s in SURFACE_SIGMAS])
def test_against_the_float64_reference(sg):
    taus = dr.taus_of(QS)
    never = worst = 0
    for step in ("const", "cone"):
        for onset in ("abrupt", "ramp"):
            for seed in range(3):
                inp, dev_args = _inputs(sg, step, onset, seed)
                host = tuple(inp[k].numpy() for k in KEYS)
                ref = dr.reference(*host, taus)
                decided = ~ref["undecided"]
                assert 1.0 - decided.mean() <= 0.02
                dq, reached, _ = _run(dev_args, QS)
                # the sample index: the depth IS that sample's float32 mid-point (neighbouring mid-points differ)
                assert np.array_equal(dq[decided].astype(np.float64), ref["depth"][decided])
                assert np.array_equal(reached[decided], ref["reached"][decided])
                assert np.all(np.diff(dq, axis=1) >= 0)                      # non-decreasing in j on every ray
                never += int(sum((((reached >> j) & 1) == 0).sum() for j in range(3)))
                # interpolated
                ref = dr.reference(*host, taus, interpolate=True)
                dqi, reached_i, _ = _run(dev_args, QS, interpolate=True)
                assert np.array_equal(reached_i, reached)
                hit = ((reached[:, None] >> np.arange(3)[None, :]) & 1) == 1
                t = dqi.astype(np.float64)
                use = hit & decided[:, None]
                assert np.all((t >= ref["a"])[use]) and np.all((t <= ref["b"])[use])
                ratio = float((np.abs(t - ref["depth"]) / dr.interp_bound(ref, taus))[decided].max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, ratio
                assert _same_bytes(dqi[~hit], dq[~hit])                      # an unreached quantile is the last mid-point either way
                # non-decreasing over the reached quantiles of every ray (an unreached one is the last sample's MID-point by
                # definition, which may lie in front of a crossing interpolated into that sample's far half)
                assert np.all((t[:, 1:] >= t[:, :-1])[hit[:, 1:]])
                # depth_sel: NaN exactly where the definition says, the selected column elsewhere
                for spread in (None, float("inf"), 0.004, 0.05):
                    got = _run(dev_args, QS, interpolate=True, sel=1, max_spread=spread)
                    assert _same_bytes(got[0], dqi) and _same_bytes(got[1], reached)
                    want = dr.depth_select(dqi, reached, 1, spread)
                    assert np.array_equal(np.isnan(got[2]), np.isnan(want)) and _same_bytes(got[2][~np.isnan(want)], want[~np.isnan(want)])
                    assert int(np.isnan(want).sum()) > 0                     # (the ray without samples, at the least)
    print(f"DEPTHQ sigma {sg:g}: {never} unreached ray-quantile pairs, worst interpolated |t - t_ref| / bound {worst:.3f}")
    assert never > 0


ORDER = (5, 0, 9, 3, 12)       # rays of 65, 0, 1024, 63 and a random number of samples


@pytest.mark.parametrize("n_q", [1, 3, 4])
@pytest.mark.parametrize("n_rays", [1, 3, 4, 5])
def test_ray_counts_around_the_block_of_four_and_quantile_counts(n_rays, n_q):
    qs = {1: (0.5,), 3: QS, 4: (0.1, 0.25, 0.5, 0.9)}[n_q]
    inp, dev_all = _inputs(1e3, "cone", "ramp", 1)
    full = _run(dev_all, qs, interpolate=True, sel=n_q - 1, max_spread=0.05)
    keep = torch.zeros(inp["packed_info"].shape[0], dtype=torch.bool)
    rows = sorted(ORDER[:n_rays])
    keep[rows] = True
    part = select_rays(inp, keep)
    got = _run(tuple(part[k].cuda() for k in KEYS), qs, interpolate=True, sel=n_q - 1, max_spread=0.05)
    for g, f in zip(got, full):
        assert _same_bytes(g, f[rows])             # a ray's result does not depend on its neighbours or its place in the block
    ref = dr.reference(*(part[k].numpy() for k in KEYS), dr.taus_of(qs))
    mid = _run(tuple(part[k].cuda() for k in KEYS), qs)
    decided = ~ref["undecided"]
    assert decided.mean() >= 0.5
    assert np.array_equal(mid[0][decided].astype(np.float64), ref["depth"][decided]) and np.array_equal(mid[1][decided], ref["reached"][decided])


def _segments(inp, schedule, counts_of):
    """Per segment of ``schedule`` the re-packed slices (ts, te, sigma, seg_packed) on the device; ``counts_of(k, off, length)``
    gives the rays' counts for segment k (int64 [R], on the CPU)."""
    s0 = inp["packed_info"][:, 0]
    for k, (off, length) in enumerate(schedule):
        c = counts_of(k, off, length)
        idx = torch.cat([torch.arange(int(a) + off, int(a) + off + int(n)) for a, n in zip(s0, c)] + [torch.zeros(1, dtype=torch.long)])
        packed = torch.stack([torch.cumsum(c, 0) - c, c], -1).contiguous()
        pad = lambda t: torch.cat([t, t.new_zeros(1)])[idx].contiguous().cuda()     # (one spare element: never an empty array)
        yield k, pad(inp["ts"]), pad(inp["te"]), pad(inp["sigma"]), packed.cuda()


def _run_segmented(inp, qs, stop=None, interpolate=True, sel=1, max_spread=0.05):
    """The segment kernel over ``segment_schedule(longest ray, 128)``.  ``stop(k, samples covered, state) -> bool [R]``: rays finished
    behind segment k, whose later counts are zeroed (None: every ray is walked to its end)."""
    from lsenerf_amd import evaluation, ops
    cnt = inp["packed_info"][:, 1]
    R = cnt.shape[0]
    sched = evaluation.segment_schedule(int(cnt.max()), 128)
    assert len(sched) >= 5
    taus = [ops.depth_tau(q) for q in qs]
    state = torch.zeros((R, 2), device="cuda")
    dq = torch.zeros((R, len(qs)), device="cuda")
    reached = torch.zeros(R, dtype=torch.uint8, device="cuda")
    ds = torch.full((R,), float("nan"), device="cuda")
    alive = torch.ones(R, dtype=torch.bool)
    counts = lambda k, off, length: torch.where(alive, (cnt - off).clamp(0, length), torch.zeros_like(cnt))
    for k, ts, te, sg, packed in _segments(inp, sched, counts):
        ops.eval_depth_quantiles_segment(ts, te, sg, packed, taus, state, dq, reached, ds, interpolate=interpolate, sel=sel,
                                         max_spread=max_spread)
        if stop is not None:
            alive &= ~stop(k, sched[k][0] + sched[k][1], state.cpu())
    return dq.cpu().numpy(), reached.cpu().numpy(), ds.cpu().numpy(), alive


SEGMENT_CASES = [(30.0, "cone", "ramp"), (1e4, "const", "abrupt"), (float("inf"), "cone", "abrupt")]


@pytest.mark.parametrize("sg,step,onset", SEGMENT_CASES, ids=[f"{c[0]:g}-{c[1]}" for c in SEGMENT_CASES])
def test_segmented_equals_full_bit_for_bit(sg, step, onset):
    inp, dev_args = _inputs(sg, step, onset, 0)
    for qs in (QS, QS4):
        full = _run(dev_args, qs, interpolate=True, sel=1, max_spread=0.05)
        seg = _run_segmented(inp, qs)
        for f, s in zip(full, seg):
            assert _same_bytes(f, s)
    full = _run(dev_args, QS)
    seg = _run_segmented(inp, QS, interpolate=False, max_spread=None)
    assert _same_bytes(full[0], seg[0]) and _same_bytes(full[1], seg[1])


@pytest.mark.parametrize("sg,step,onset", SEGMENT_CASES, ids=[f"{c[0]:g}-{c[1]}" for c in SEGMENT_CASES])
def test_stopped_rays_behave_as_rays_that_end(sg, step, onset):
    from lsenerf_amd import ops
    inp, dev_args = _inputs(sg, step, onset, 0)
    tau_stop = ops.eval_tau_stop(1e-4)
    s0, cnt = inp["packed_info"][:, 0].tolist(), inp["packed_info"][:, 1].tolist()
    sd = (inp["sigma"].double() * (inp["te"].double() - inp["ts"].double())).numpy()

    def by_float64(k, end, state):
        # the optical depth through `end` samples, in double: at 9.2 it is far beyond the largest of QS (1.39) in any arithmetic
        with np.errstate(invalid="ignore"):
            return torch.tensor([bool(np.sum(sd[a:a + min(end, n)]) >= tau_stop) for a, n in zip(s0, cnt)])

    def by_carry(k, end, state):
        # the rule of lse_eval_composite_segment on the carry this walk keeps (the same bits); QS4's last threshold IS tau_stop, so
        # the carry is kept up to the stop
        return state[:, 0] >= tau_stop

    for qs, stop in ((QS, by_float64), (QS4, by_carry)):
        full = _run(dev_args, qs, interpolate=True, sel=1, max_spread=0.05)
        seg = _run_segmented(inp, qs, stop=stop)
        stopped = int((~seg[3] & (inp["packed_info"][:, 1] > 256)).sum())
        print(f"DEPTHQ_STOP sigma {sg:g} n_q {len(qs)}: {int((~seg[3]).sum())} rays stopped, {stopped} of them with samples left")
        assert stopped > 0
        for f, s in zip(full, seg[:3]):
            assert _same_bytes(f, s)


def test_the_median_of_a_two_surface_ray_is_the_front_surface():
    from lsenerf_amd import ops
    ts, te, sg, packed = two_surface_ray()
    dev_args = tuple(torch.from_numpy(a).cuda() for a in (ts, te, sg, packed))
    dq, reached, _ = _run(dev_args, QS)
    mid = (ts + te) * F(0.5)
    assert reached.tolist() == [7] and dq[0].tolist() == [mid[2], mid[2], mid[7]]
    rgb, acc, depth = torch.empty((1, 3), device="cuda"), torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    ops.eval_composite(*dev_args[:3], torch.rand((10, 3), device="cuda"), dev_args[3], rgb, acc, depth,
                       torch.empty(1, dtype=torch.int64, device="cuda"), nan_to_num=False, background=None, clamp=False)
    assert abs(float(acc) - 1.0) < 1e-6 and te[2] < float(depth) < ts[7]          # the mean lies between the two surfaces
    assert float(depth) > dq[0, 1]
    dqi, _, sel = _run(dev_args, QS, interpolate=True, sel=1, max_spread=1.0)
    assert ts[2] < dqi[0, 0] < dqi[0, 1] < te[2] and abs(dqi[0, 1] - (ts[2] + math.log(2.0) / sg[2])) < 1e-6
    assert sel[0] == dqi[0, 1]
    assert np.isnan(_run(dev_args, QS, interpolate=True, sel=1, max_spread=0.25)[2][0])     # quartiles 0.5 apart: a smeared ray
