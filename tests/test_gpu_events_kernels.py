"""The event synthesis entry points (csrc/events.hip) against the numpy twin (tests/events_ref.py), bit for bit: counts, x, y, p, the
float64 times, ref_out and the totals.  Shapes: one pixel, less than a wave, several waves, planes that are no multiple of 64 or of
the 1024-item segment, segment borders inside an interval and across intervals; a wave without any event and a wave whose every lane
saturates at cap_step; 300 x 300 pixels over 3 intervals are 264 segments, more than the scan block's 256 threads: a second scan step,
in the chained windows behind a non-zero total."""
import functools

import numpy as np
import pytest
import torch

from tests import events_ref as er

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (1, 5, 7), (9, 5, 7), (4, 3, 343), (3, 24, 40), (2, 1, 2050), (3, 300, 300)]
C_POS, C_NEG = 0.2, 0.25
SENTINEL = -77


@functools.lru_cache(maxsize=None)
def _planes(K, P, seed=0):
    """A random walk; from 192 pixels on, pixels 64 .. 127 never change (a wave without an event) and pixels 128 .. 191 climb by
    1000 a plane (a wave whose every lane saturates).  Read-only."""
    L = er.random_walk_planes(K, P, seed)
    if P >= 192:
        L[:, 64:128] = L[0, 64:128]
        L[:, 128:192] = L[0, 128:192] + (np.float32(1000.0) * np.arange(K + 1, dtype=np.float32))[:, None]
    L.setflags(write=False)
    return L


def _times(K):
    return 3.0 + 0.01 * np.arange(K + 1, dtype=np.float64) ** 1.5


@functools.lru_cache(maxsize=None)
def _twin(K, H, W, cap_step, seed=0):
    L = _planes(K, H * W, seed)
    return er.append(L, _times(K), W, L[0], C_POS, C_NEG, cap_step)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))                  # (a copy: the cached inputs are read-only)
    return (t if dtype is None else t.to(dtype)).cuda()


def _same(a, b):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    b = b.detach().cpu().numpy() if torch.is_tensor(b) else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _buffers(cap):
    return [torch.full((cap,), SENTINEL, dtype=dt, device="cuda") for dt in (torch.int16, torch.int16, torch.float64, torch.int8)]


def _append(L, times, W, ref, cap_step, cap, c=(C_POS, C_NEG), counts=True, bufs=None, total=None):
    from lsenerf_amd import ops
    L = _dev(L)
    K, P = L.shape[0] - 1, L.shape[1]
    bufs = _buffers(cap) if bufs is None else bufs
    total = torch.zeros(1, dtype=torch.int64, device="cuda") if total is None else total
    cn = torch.full((K, P), SENTINEL, dtype=torch.int32, device="cuda") if counts else None
    ref_out = ops.event_append(L, _dev(times), W, _dev(ref), c[0], c[1], cap_step, *bufs, total, counts=cn)
    return cn, bufs, ref_out, total


def _assert_stream(bufs, want, n=None):
    n = len(want[2]) if n is None else n
    for got, w, name in zip(bufs, want, "xytp"):
        assert _same(got[:n], w[:n]), name
        assert bool((got[n:] == SENTINEL).all()), f"{name}: rows behind the stream were written"


@pytest.mark.parametrize("cap_step", [1, 3, 127])
@pytest.mark.parametrize("shape", SHAPES)
def test_append_and_count_equal_the_twin(shape, cap_step):
    from lsenerf_amd import ops
    K, H, W = shape
    L = _planes(K, H * W)
    counts, ev, ref = _twin(K, H, W, cap_step)
    n = len(ev[2])
    if H * W >= 192:
        assert not counts[:, 64:128].any() and (counts[:, 128:192] == cap_step).all()
    cn, bufs, ref_out, total = _append(L, _times(K), W, L[0], cap_step, n + 5)
    assert int(total.item()) == n
    assert _same(cn, counts) and _same(ref_out, ref)
    _assert_stream(bufs, ev)
    # the walk without a stream: the same counts, levels and total
    c2, r2, wt = ops.event_count(_dev(L), _dev(L[0]), C_POS, C_NEG, cap_step)
    assert _same(c2, counts) and _same(r2, ref) and int(wt.item()) == n
    # ... also into a counts buffer that is no multiple of 16 bytes into its allocation
    odd = torch.full((K * H * W + 1,), SENTINEL, dtype=torch.int32, device="cuda")
    c4, _, wt4 = ops.event_count(_dev(L), _dev(L[0]), C_POS, C_NEG, cap_step, counts=odd[1:].view(K, H * W))
    assert c4.data_ptr() % 16 == 4 and _same(c4, counts) and int(wt4.item()) == n and int(odd[0]) == SENTINEL
    # two runs give the same bytes
    cn3, bufs3, ref3, total3 = _append(L, _times(K), W, L[0], cap_step, n + 5)
    assert _same(cn3, cn) and _same(ref3, ref_out) and all(_same(a, b) for a, b in zip(bufs, bufs3)) and int(total3.item()) == n


def test_the_random_walks_fire():
    counts, ev, _ = _twin(3, 24, 40, 127)
    walk = np.ones(960, bool)
    walk[64:192] = False
    fired = float((counts[:, walk] != 0).mean())
    assert 0.2 < fired < 0.95, fired                                      # (one of the three intervals is static) neither an empty stream nor one event everywhere
    assert len(ev[2]) > 3 * 64 * 127


@pytest.mark.parametrize("shape", [(9, 5, 7), (2, 1, 2050)])
def test_nan_and_infinite_planes_and_a_far_level(shape):
    K, H, W = shape
    P = H * W
    L = _planes(K, P, seed=1).copy()
    L[1, 0::7] = np.nan
    L[1, 1::7] = np.inf
    L[1, 2::7] = -np.inf
    ref = (L[0] + np.where(np.arange(P) % 2 == 0, np.float32(1.3), np.float32(-0.9))).astype(np.float32)      # far from L[0]
    ref[3] = np.nan
    for cap_step in (3, 127):
        counts, ev, want_ref = er.append(L, _times(K), W, ref, C_POS, C_NEG, cap_step)
        first = np.repeat(np.arange(K), np.abs(counts).sum(1)) == 0
        assert first.any() and (ev[2][first] == _times(K)[0]).sum() > P // 4        # fractions clamped to 0 in the first interval
        assert not counts[:, 3].any() and (counts[0, 1::7] == cap_step).all()
        cn, bufs, ref_out, total = _append(L, _times(K), W, ref, cap_step, len(ev[2]))
        assert int(total.item()) == len(ev[2]) and _same(cn, counts) and _same(ref_out, want_ref)
        _assert_stream(bufs, ev)


@pytest.mark.parametrize("shape", [(9, 5, 7), (4, 3, 343), (6, 300, 300)])        # the last: 3 intervals, 264 segments, per window
def test_windows_chain_behind_one_total(shape):
    from lsenerf_amd import ops
    K, H, W = shape
    L, times = _planes(K, H * W), _times(K)
    counts, ev, ref = _twin(K, H, W, 127)
    n = len(ev[2])
    k1 = K // 2
    bufs = _buffers(n + 3)
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    c_a, _, ref_a, _ = _append(L[:k1 + 1], times[:k1 + 1], W, L[0], 127, n + 3, bufs=bufs, total=total)
    first = int(total.item())
    assert first == int(np.abs(counts[:k1]).sum()) and 0 < first < n
    c_b, _, ref_b, _ = _append(L[k1:], times[k1:], W, ref_a.cpu().numpy(), 127, n + 3, bufs=bufs, total=total)
    assert int(total.item()) == n and _same(torch.cat([c_a, c_b]), counts) and _same(ref_b, ref)
    _assert_stream(bufs, ev)
    # no interval: the levels pass through, nothing is appended
    ref_c = ops.event_append(_dev(L[:1]), _dev(times[:1]), W, ref_b, C_POS, C_NEG, 127, *bufs, total)
    assert _same(ref_c, ref) and int(total.item()) == n and ref_c.data_ptr() != ref_b.data_ptr()
    _assert_stream(bufs, ev)
    c0, r0, wt0 = ops.event_count(_dev(L[:1]), ref_b, C_POS, C_NEG, 127)
    assert c0.shape == (0, H * W) and _same(r0, ref) and int(wt0.item()) == 0


@pytest.mark.parametrize("shape", [(9, 5, 7), (3, 24, 40)])
def test_a_capacity_drops_in_order_and_the_total_stays_true(shape):
    K, H, W = shape
    L = _planes(K, H * W)
    counts, ev, ref = _twin(K, H, W, 3)
    n = len(ev[2])
    for cap in (n - 1, n + 1, n // 2, 0):
        cn, bufs, ref_out, total = _append(L, _times(K), W, L[0], 3, cap, counts=(cap != n // 2))
        assert int(total.item()) == n and _same(ref_out, ref)
        assert cn is None or _same(cn, counts)
        _assert_stream(bufs, ev, min(n, cap))


# ---- accumulate -----------------------------------------------------------------------------------------------------------------
def _accumulate(ev, bounds, H, W, acc=None, n_dev=None):
    from lsenerf_amd import ops
    F = len(bounds) - 1
    acc = torch.zeros((F, H, W), dtype=torch.int32, device="cuda") if acc is None else acc
    nd = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int64, device="cuda")
    return ops.event_accumulate(*(_dev(a) for a in ev), _dev(np.asarray(bounds, np.float64)), acc, n_dev=nd)


def test_accumulate_of_a_stream_is_the_summed_counts_and_the_twin():
    K, H, W = 9, 5, 7
    counts, ev, _ = _twin(K, H, W, 127)
    times = _times(K)
    for step in (9, 3, 1):
        bounds = times[::step]
        assert er.boundary_ties(ev[2], bounds) == 0
        acc = _accumulate(ev, bounds, H, W)
        assert _same(acc, er.accumulate(*ev, bounds, H, W))
        assert _same(acc.reshape(K // step, H * W), counts.reshape(K // step, step, H * W).sum(1).astype(np.int32))
    n = len(ev[2])
    bounds = times[::3]
    whole = _accumulate(ev, bounds, H, W)
    parts = _accumulate([a[:n // 3] for a in ev], bounds, H, W)
    parts = _accumulate([a[n // 3:] for a in ev], bounds, H, W, acc=parts)          # it adds: a stream can arrive in pieces
    assert _same(parts, whole)
    for n_dev in (0, n // 2, n + 10, -4):
        assert _same(_accumulate(ev, bounds, H, W, n_dev=n_dev), er.accumulate(*ev, bounds, H, W, count=n_dev)), n_dev
    assert _same(_accumulate(ev, bounds, H, W), whole)                               # two runs give the same bytes


def test_accumulate_edges_contention_and_many_frames():
    b = np.array([1.0, 2.0, 4.0])
    x = np.array([0, 1, 2, 3, -1, 0, 0, 0, 0], np.int16)
    y = np.array([0, 0, 0, 0, 0, 2, -1, 1, 1], np.int16)
    t = np.array([1.0, 2.0, 4.0, 1.5, 1.5, 1.5, 1.5, np.nextafter(1.0, 0.0), np.nan])
    p = np.array([1, -1, 1, 1, 1, 1, 1, 1, 1], np.int8)
    want = np.zeros((2, 2, 3), np.int32)
    want[0, 0, 0], want[1, 0, 1] = 1, -1
    assert _same(_accumulate((x, y, t, p), b, 2, 3), want) and _same(er.accumulate(x, y, t, p, b, 2, 3), want)
    # 10 000 events on one pixel
    n = 10000
    rng = np.random.default_rng(4)
    ev = (np.full(n, 5, np.int16), np.full(n, 2, np.int16), rng.uniform(0.0, 1.0, n), rng.choice(np.int8([-1, 1]), n, p=[0.3, 0.7]))
    acc = _accumulate(ev, [0.0, 1.0], 4, 9)
    assert int(acc[0, 2, 5]) == int(ev[3].sum()) and int(acc.abs().sum()) == abs(int(ev[3].sum()))
    # F in {1, 3, 257}, bounds of uneven width, events on every bound
    n = 6000
    for F in (1, 3, 257):
        bounds = np.cumsum(rng.uniform(0.01, 1.0, F + 1))
        tt = rng.uniform(bounds[0] - 0.5, bounds[-1] + 0.5, n)
        tt[:F + 1] = bounds
        ev = (rng.integers(-1, 8, n).astype(np.int16), rng.integers(-1, 6, n).astype(np.int16), tt,
              rng.choice(np.int8([-1, 1]), n))
        assert _same(_accumulate(ev, bounds, 5, 7), er.accumulate(*ev, bounds, 5, 7)), F


def test_wrappers_check_their_tensors():
    from lsenerf_amd import ops
    L, ref = torch.zeros((3, 8), device="cuda"), torch.zeros(8, device="cuda")
    times = torch.zeros(3, dtype=torch.float64, device="cuda")
    bufs = _buffers(4)
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError, match="expected torch.float32"):
        ops.event_count(L.double(), ref, 0.2, 0.2, 8)
    with pytest.raises(ValueError, match="contiguous"):
        ops.event_count(torch.zeros((8, 3), device="cuda").t(), ref, 0.2, 0.2, 8)
    with pytest.raises(ValueError, match=r"ref_in: \[8\] expected"):
        ops.event_count(L, ref[:7], 0.2, 0.2, 8)
    with pytest.raises(ValueError, match="must not alias"):
        ops.event_count(L, ref, 0.2, 0.2, 8, ref_out=ref)
    with pytest.raises(ValueError, match=r"times: \[3\] expected"):
        ops.event_append(L, times[:2], 4, ref, 0.2, 0.2, 8, *bufs, total)
    with pytest.raises(ValueError, match="out_p: expected torch.int8"):
        ops.event_append(L, times, 4, ref, 0.2, 0.2, 8, bufs[0], bufs[1], bufs[2], bufs[0], total)
    with pytest.raises(ValueError, match="workspace of 8 bytes"):
        ops.event_append(L, times, 4, ref, 0.2, 0.2, 8, *bufs, total, workspace=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match=r"bounds: \[3\] expected"):
        ops.event_accumulate(*bufs, times[:2], torch.zeros((2, 2, 4), dtype=torch.int32, device="cuda"))
    assert ops.event_workspace_bytes(2, 8) == 8 + 12 * 16
