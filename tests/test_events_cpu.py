"""Event synthesis without a GPU: the numpy twin (tests/events_ref.py) on the random walks it was probed with, the package's host
side (``EventStream``, ``write_event_frames``, the window loop of ``simulate_events`` over an injected twin backend,
``event_frame_metrics``), the ops' refusals and the library's argument checks, which precede any device work."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import events_ref as er

K, HH, WW = 9, 5, 7
P = HH * WW
C_POS, C_NEG, CAP = 0.2, 0.25, 64
TIMES = np.arange(K + 1, dtype=np.float64) * 0.01 + 3.0
SEEDS = range(5)


def _walk(seed):
    return er.random_walk_planes(K, P, seed)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _same_run(a, b):
    return _same(a[0], b[0]) and all(_same(u, v) for u, v in zip(a[1], b[1])) and _same(a[2], b[2])


# ---- twin properties ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_the_walks_give_the_probed_figures(seed):
    L = _walk(seed)
    counts, (x, y, t, p), ref = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    assert 223 <= len(t) <= 276 and int(np.abs(counts).max()) <= 6
    assert len(t) == int(np.abs(counts).sum()) == er.count(L, L[0], C_POS, C_NEG, CAP)[2]
    assert x.dtype == np.int16 and y.dtype == np.int16 and t.dtype == np.float64 and p.dtype == np.int8
    assert set(np.unique(p)) <= {-1, 1} and int(x.max()) < WW and int(y.max()) < HH
    # no event sits on an end of its interval: the frames below have no tie to argue about
    assert er.boundary_ties(t, TIMES) == 0
    assert not counts[2].any()                                              # the static interval emits nothing
    assert float(np.abs(L[-1] - ref).max()) < max(C_POS, C_NEG)            # the cap was never hit


@pytest.mark.parametrize("seed", SEEDS)
def test_the_vectorised_twin_is_the_scalar_definition(seed):
    L = _walk(seed)
    counts, (x, y, t, p), ref = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    level = L[0].copy()
    ts = []
    for k in range(K):
        for pix in range(P):
            n, level[pix], tt = er.walk_scalar(L[k, pix], L[k + 1, pix], level[pix], C_POS, C_NEG, CAP, TIMES[k], TIMES[k + 1])
            assert n == counts[k, pix]
            ts += tt
    assert _same(level, ref) and _same(np.asarray(ts, np.float64), t)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("window", [1, 3, 4])
def test_windows_chain_to_the_same_counts_events_and_levels(seed, window):
    L = _walk(seed)
    assert _same_run(er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP), er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP, window))


@pytest.mark.parametrize("seed", SEEDS)
def test_event_times_do_not_decrease_per_pixel_and_lie_in_their_interval(seed):
    L = _walk(seed)
    counts, (x, y, t, p), _ = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    pix = y.astype(np.int64) * WW + x
    for q in range(P):
        assert (np.diff(t[pix == q]) >= 0).all()
    k = np.repeat(np.arange(K), np.abs(counts).sum(1))
    assert (t >= TIMES[k]).all() and (t <= TIMES[k + 1]).all()


def test_nan_and_infinite_planes():
    L = _walk(0)
    L[4, 3] = np.nan
    L[5:, 8] = np.nan
    counts, (x, y, t, p), ref = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    assert not counts[3, 3] and not counts[4:, 8].any()                             # into a NaN plane: nothing
    assert np.isfinite(t).all()
    ref0 = L[0].copy()
    ref0[5] = np.nan
    c2, _, r2 = er.simulate(L, TIMES, WW, ref0, C_POS, C_NEG, CAP)
    assert not c2[:, 5].any() and np.isnan(r2[5])                                   # a NaN level stays
    M = _walk(1)
    M[2, 0], M[2, 1] = np.inf, -np.inf
    c3, (_, _, t3, _), r3 = er.simulate(M, TIMES, WW, M[0], C_POS, C_NEG, 3)
    assert c3[1, 0] == 3 and c3[2, 0] == -3 and c3[1, 1] == -3 and c3[2, 1] == 3    # saturates, re-arms at L1, comes back
    assert np.isfinite(t3).all()


def test_the_cap_saturates_and_rearms():
    L = np.array([[0.0], [1.0], [1.05], [-2.0]], np.float32)
    counts, (x, y, t, p), ref = er.simulate(L, [0.0, 1.0, 2.0, 3.0], 1, L[0], 0.1, 0.1, 3)
    assert counts[:, 0].tolist() == [3, 0, -3] and p.tolist() == [1, 1, 1, -1, -1, -1]
    assert ref[0] == np.float32(-2.0)
    # the first interval: levels 0.1, 0.2, 0.3 over a rise of 1 in [0, 1]
    want = [np.float64(np.float32(np.float64(lv) / 1.0)) for lv in np.cumsum(np.float32([0.1, 0.1, 0.1]), dtype=np.float32)]
    assert t[:3].tolist() == want
    c1, _, r1 = er.simulate(L, [0.0, 1.0, 2.0, 3.0], 1, L[0], 0.1, 0.1, 127)
    assert c1[0, 0] in (9, 10) and abs(float(r1[0]) + 2.0) < 0.1


def test_a_level_far_from_the_first_plane_clamps_the_fraction():
    L = np.array([[0.0], [0.05]], np.float32)
    _, (_, _, t, p), _ = er.simulate(L, [2.0, 4.0], 1, np.float32([-1.1]), 0.2, 0.2, 64)
    assert len(t) == 5 and p.tolist() == [1] * 5 and t.tolist() == [2.0] * 5       # every level lies below L0: frac = 0


@pytest.mark.parametrize("seed", SEEDS)
def test_accumulate_of_simulate_is_the_summed_counts(seed):
    L = _walk(seed)
    counts, ev, _ = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    bounds = TIMES[::3]
    assert er.boundary_ties(ev[2], bounds) == 0
    acc = er.accumulate(*ev, bounds, HH, WW)
    assert _same(acc.reshape(3, P), counts.reshape(3, 3, P).sum(1).astype(np.int32))
    n = len(ev[2])
    parts = er.accumulate(*(a[:n // 3] for a in ev), bounds, HH, WW)
    parts = er.accumulate(*(a[n // 3:] for a in ev), bounds, HH, WW, acc=parts)
    assert _same(parts, acc)
    assert _same(er.accumulate(*ev, bounds, HH, WW, count=n // 2), er.accumulate(*(a[:n // 2] for a in ev), bounds, HH, WW))


def test_accumulate_edges():
    b = np.array([1.0, 2.0, 4.0])
    x = np.array([0, 1, 2, 3, -1, 0, 0, 0, 0], np.int16)
    y = np.array([0, 0, 0, 0, 0, 2, -1, 1, 1], np.int16)
    t = np.array([1.0, 2.0, 4.0, 1.5, 1.5, 1.5, 1.5, np.nextafter(1.0, 0.0), np.nan])
    p = np.array([1, -1, 1, 1, 1, 1, 1, 1, 1], np.int8)
    acc = er.accumulate(x, y, t, p, b, 2, 3)
    want = np.zeros((2, 2, 3), np.int32)
    want[0, 0, 0] = 1          # t equal to the first bound counts, in frame 0
    want[1, 0, 1] = -1         # t equal to an inner bound belongs to the later frame
    assert _same(acc, want)    # t equal to the last bound, x / y outside, t below the first bound and NaN: skipped


# ---- the package's host side ----------------------------------------------------------------------------------------------------
def _stream(seed=0):
    from lsenerf_amd.events import EventStream
    L = _walk(seed)
    _, (x, y, t, p), _ = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    return EventStream(*(torch.from_numpy(a) for a in (x, y, t, p)), HH, WW)


def test_event_stream_npz_round_trip_and_sort(tmp_path):
    from lsenerf_amd.events import EventStream
    s = _stream()
    path = str(tmp_path / "events.npz")
    s.write_npz(path)
    with np.load(path) as z:
        assert sorted(z.files) == ["H", "W", "p", "t", "x", "y"]
    r = EventStream.read_npz(path)
    assert (r.H, r.W, len(r)) == (HH, WW, len(s))
    for k in ("x", "y", "t", "p"):
        assert getattr(r, k).dtype == getattr(s, k).dtype and torch.equal(getattr(r, k), getattr(s, k)), k
    o = s.sorted_by_time()
    assert bool((o.t[1:] >= o.t[:-1]).all()) and len(o) == len(s)
    order = np.argsort(s.t.numpy(), kind="stable")
    assert torch.equal(o.x, s.x[order]) and torch.equal(o.p, s.p[order]) and torch.equal(o.t, s.t[order])
    tie = EventStream(torch.tensor([3, 1, 2], dtype=torch.int16), torch.zeros(3, dtype=torch.int16),
                      torch.tensor([1.0, 0.5, 1.0], dtype=torch.float64), torch.ones(3, dtype=torch.int8), 1, 4).sorted_by_time()
    assert tie.x.tolist() == [1, 3, 2]                                      # ties keep stream order


def test_event_frames_round_trip_through_the_scene_reader(tmp_path):
    from lsenerf_amd.events import write_event_frames
    from lsenerf_amd.scene_io import EventSceneReader
    frames = torch.tensor([[[0, 5, -7], [127, -128, 1]], [[300, -300, 128], [-129, 2, 0]]], dtype=torch.int32)
    path = write_event_frames(str(tmp_path / "ecam_set"), frames)
    assert path.endswith("eimgs/eimgs_1x.npy") and np.load(path).dtype == np.int8
    reader = EventSceneReader.__new__(EventSceneReader)
    reader.data = str(tmp_path / "ecam_set")
    got = reader.load_events([1, 0])
    assert got.shape == (2, 2, 3, 1) and got.dtype == np.int8
    want = frames.clamp(-128, 127).to(torch.int8).numpy()
    assert np.array_equal(got[..., 0], want[[1, 0]])
    with pytest.raises(ValueError, match=r"\[n, H, W\]"):
        write_event_frames(str(tmp_path / "bad"), torch.zeros(2, 3))


class _TwinBackend:
    """The entry points of ``ops`` the window loop uses, on CPU tensors through the numpy twin; records what it was asked."""

    def __init__(self):
        self.calls = []

    @staticmethod
    def event_workspace_bytes(K, P):
        return 8 * ((K * P + 1023) // 1024) + 12 * K * P

    def event_count(self, planes, ref_in, c_pos, c_neg, cap_step, ref_out=None):
        counts, ref, total = er.count(planes.numpy(), ref_in.numpy(), c_pos, c_neg, cap_step)
        ref_out.copy_(torch.from_numpy(ref))
        self.calls.append(("count", planes.shape[0] - 1, total))
        return torch.from_numpy(counts), ref_out, torch.tensor([total])

    def event_append(self, planes, times, W, ref_in, c_pos, c_neg, cap_step, out_x, out_y, out_t, out_p, total, ref_out=None,
                     workspace=None):
        assert ref_out.data_ptr() != ref_in.data_ptr()
        assert workspace.numel() >= self.event_workspace_bytes(planes.shape[0] - 1, planes.shape[1])
        _, ev, ref = er.append(planes.numpy(), times.numpy(), W, ref_in.numpy(), c_pos, c_neg, cap_step)
        base, cap = int(total), out_t.shape[0]
        for out, src in zip((out_x, out_y, out_t, out_p), ev):
            keep = max(0, min(len(src), cap - base))
            out[base:base + keep] = torch.from_numpy(src[:keep])
        total += len(ev[2])
        ref_out.copy_(torch.from_numpy(ref))
        self.calls.append(("append", planes.shape[0] - 1, cap))
        return ref_out


def _run_windows(L, window, max_events, ref=None):
    from lsenerf_amd import events
    planes = torch.from_numpy(L)
    rendered = []

    def render(i0, i1, out):
        rendered.extend(range(i0, i1))
        out.copy_(planes[i0:i1])
    backend = _TwinBackend()
    arrays, ref_out, total, known = events._simulate_windows(render, torch.from_numpy(TIMES), P, WW, C_POS, C_NEG, window, CAP,
                                                             max_events, ref, backend=backend)
    return arrays, ref_out, int(total), known, rendered, backend.calls


@pytest.mark.parametrize("window", [1, 2, 4, 9, 16])
def test_the_window_loop_grows_exactly_and_renders_every_plane_once(window):
    L = _walk(3)
    counts, ev, ref = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    arrays, ref_out, total, known, rendered, calls = _run_windows(L, window, None)
    assert rendered == list(range(K + 1))                                   # the shared plane of two windows is not rendered twice
    assert total == known == len(ev[2]) and all(a.shape[0] == total for a in arrays)
    for a, want in zip(arrays, ev):
        assert _same(a.numpy(), want)
    assert _same(ref_out.numpy(), ref)
    appends = [c for c in calls if c[0] == "append"]
    counted = [c for c in calls if c[0] == "count"]
    assert [c[1] for c in appends] == [min(window, K - k0) for k0 in range(0, K, window)] == [c[1] for c in counted]
    assert [c[2] for c in appends] == np.cumsum([c[2] for c in counted]).tolist()        # each append saw arrays of exactly its size


@pytest.mark.parametrize("window", [2, 9])
def test_the_window_loop_with_a_capacity_drops_in_order_and_counts_on(window):
    L = _walk(3)
    _, ev, ref = er.simulate(L, TIMES, WW, L[0], C_POS, C_NEG, CAP)
    n = len(ev[2])
    for cap in (0, 100, n, n + 50):
        arrays, ref_out, total, known, _, calls = _run_windows(L, window, cap)
        assert known is None and total == n and not [c for c in calls if c[0] == "count"]        # nothing is read inside the loop
        assert all(a.shape[0] == cap for a in arrays)
        m = min(n, cap)
        for a, want in zip(arrays, ev):
            assert _same(a.numpy()[:m], want[:m])
        assert _same(ref_out.numpy(), ref)


def test_the_window_loop_starts_from_a_given_level_and_checks_its_arguments():
    from lsenerf_amd import events
    L = _walk(2)
    ref0 = (L[0] + np.float32(0.6)).astype(np.float32)
    _, ev, ref = er.simulate(L, TIMES, WW, ref0, C_POS, C_NEG, CAP)
    arrays, ref_out, total, _, _, _ = _run_windows(L, 4, None, ref=torch.from_numpy(ref0))
    assert total == len(ev[2]) and _same(arrays[2].numpy(), ev[2]) and _same(ref_out.numpy(), ref)
    with pytest.raises(ValueError, match="window"):
        events._simulate_windows(lambda *a: None, torch.from_numpy(TIMES), P, WW, C_POS, C_NEG, 0, CAP, None, None)
    with pytest.raises(ValueError, match="max_events"):
        events._simulate_windows(lambda *a: None, torch.from_numpy(TIMES), P, WW, C_POS, C_NEG, 4, CAP, -1, None)


def test_simulate_events_checks_its_arguments_before_anything_runs():
    from lsenerf_amd.events import predict_event_frames, simulate_events

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} was touched")
    model = Untouchable()
    cams = types.SimpleNamespace(height=HH, width=WW)
    poses = torch.zeros(3, 3, 4)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="thresholds"):
            simulate_events(model, cams, poses, [0.0, 1.0, 2.0], bad)
        with pytest.raises(ValueError, match="thresholds"):
            predict_event_frames(model, cams, poses[None], 0.2, threshold_neg=bad)
    for bad in (0, 32768):
        with pytest.raises(ValueError, match="cap_step"):
            simulate_events(model, cams, poses, [0.0, 1.0, 2.0], 0.2, cap_step=bad)


def test_event_frame_metrics_on_hand_made_frames():
    from lsenerf_amd.events import event_frame_metrics
    rec = torch.tensor([[[0, 2, -1], [3, 0, -4]]], dtype=torch.int8)
    pred = torch.tensor([[[1, 1, 1], [5, 0, -4]]], dtype=torch.int32)
    m = event_frame_metrics(pred, rec)
    assert m["mean_abs_diff"] == pytest.approx((1 + 1 + 2 + 2 + 0 + 0) / 6)
    assert m["sign_agreement"] == pytest.approx(3 / 4)                      # of the four recorded pixels, (0, 2) disagrees
    assert event_frame_metrics(rec, rec) == {"mean_abs_diff": 0.0, "sign_agreement": 1.0}
    assert np.isnan(event_frame_metrics(pred, torch.zeros_like(rec))["sign_agreement"])
    with pytest.raises(ValueError, match="recorded"):
        event_frame_metrics(pred, rec[0])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_ops_refuse_bad_tensors_before_the_library(monkeypatch):
    from lsenerf_amd import _lib, ops

    def no_library(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "call", no_library)
    planes, ref = torch.zeros(3, 8), torch.zeros(8)
    times = torch.zeros(3, dtype=torch.float64)
    ev = (torch.zeros(4, dtype=torch.int16), torch.zeros(4, dtype=torch.int16), torch.zeros(4, dtype=torch.float64),
          torch.zeros(4, dtype=torch.int8))
    total = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.event_count(planes, ref, 0.2, 0.2, 8)
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.event_append(planes, times, 4, ref, 0.2, 0.2, 8, *ev, total)
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.event_accumulate(*ev, times, torch.zeros((2, 2, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="thresholds"):
        ops.event_count(planes, ref, 0.0, 0.2, 8)
    with pytest.raises(ValueError, match="cap_step"):
        ops.event_count(planes, ref, 0.2, 0.2, 0)
    with pytest.raises(ValueError, match="width"):
        ops.event_append(planes, times, 3, ref, 0.2, 0.2, 8, *ev, total)
    with pytest.raises(ValueError, match=r"\[K \+ 1, P\]"):
        ops.event_count(ref, ref, 0.2, 0.2, 8)
    with pytest.raises(ValueError, match=r"\[F, H, W\]"):
        ops.event_accumulate(*ev, times, torch.zeros((2, 4), dtype=torch.int32))


def test_the_library_refuses_bad_arguments_before_any_launch():
    """The host-side checks of csrc/events.hip return LSE_E_INVALID without touching a device: callable without a GPU."""
    from lsenerf_amd import _lib
    v = ctypes.c_int64(-1)
    size = lambda k, p: (_lib.call("lse_event_workspace", k, p, ctypes.byref(v)), v.value)[1]
    assert size(0, 35) == 0 and size(3, 0) == 0
    assert size(1, 1) == 8 + 12 and size(1, 1025) == 2 * 8 + 12 * 1025 and size(5, 205) == 2 * 8 + 12 * 1025
    sizes = [[size(k, p) for p in (1, 35, 1024, 1025, 307200)] for k in (1, 2, 9, 32)]
    for row in sizes:
        assert row == sorted(row) and len(set(row)) == len(row)             # monotone in P ...
    for col in zip(*sizes):
        assert list(col) == sorted(col) and len(set(col)) == len(col)       # ... and in K
    for k, p in ((-1, 4), (4, -1), (4, (1 << 30) + 1), (1 << 11, 1 << 30)):
        with pytest.raises(_lib.LseHipError, match="outside|exceeds"):
            size(k, p)
    fake = ctypes.c_void_p(4096)                 # never dereferenced: every call below is refused before a launch
    fake2 = ctypes.c_void_p(8192)
    count = lambda c_pos, c_neg, cap: _lib.call("lse_event_count", fake, 2, 35, fake, c_pos, c_neg, cap, fake, fake2, fake, None)
    append = lambda P=35, W=7, c=(0.2, 0.25), cap_step=64, ws=1 << 20, cap=8, total=fake, ref_out=fake2: _lib.call(
        "lse_event_append", fake, fake, 2, P, W, fake, c[0], c[1], cap_step, fake, ws, cap, fake, fake, fake, fake, None, ref_out,
        total, None)
    for bad in (0.0, -0.2, float("nan"), float("inf")):
        for c in ((bad, 0.2), (0.2, bad)):
            with pytest.raises(_lib.LseHipError, match="thresholds must be positive and finite"):
                count(*c, 64)
            with pytest.raises(_lib.LseHipError, match="thresholds must be positive and finite"):
                append(c=c)
    for bad in (0, 32768, -1):
        with pytest.raises(_lib.LseHipError, match=r"cap_step -?\d+ outside \[1, 32767\]"):
            count(0.2, 0.25, bad)
        with pytest.raises(_lib.LseHipError, match=r"cap_step -?\d+ outside \[1, 32767\]"):
            append(cap_step=bad)
    with pytest.raises(_lib.LseHipError, match="no whole number of rows"):
        append(P=36)
    with pytest.raises(_lib.LseHipError, match=r"width 32768 outside \[1, 32767\]"):
        append(P=32768, W=32768)
    with pytest.raises(_lib.LseHipError, match="width 0"):
        append(W=0)
    with pytest.raises(_lib.LseHipError, match="height 32768 above 32767"):
        append(P=32768, W=1)
    need = size(2, 35)
    with pytest.raises(_lib.LseHipError, match=f"workspace of {need - 1} bytes < {need}"):
        append(ws=need - 1)
    with pytest.raises(_lib.LseHipError, match="negative capacity"):
        append(cap=-1)
    with pytest.raises(_lib.LseHipError, match="total must be"):
        append(total=None)
    with pytest.raises(_lib.LseHipError, match="two non-null buffers"):
        append(ref_out=fake)
    with pytest.raises(_lib.LseHipError, match="window_total must be"):
        _lib.call("lse_event_count", fake, 2, 35, fake, 0.2, 0.2, 8, fake, fake2, None, None)
    acc = lambda n=8, F=2, H=5, W=7: _lib.call("lse_event_accumulate", fake, fake, fake, fake, n, None, fake, F, H, W, fake, None)
    with pytest.raises(_lib.LseHipError, match="extent"):
        acc(n=-1)
    for kw in ({"F": 0}, {"H": 0}, {"W": -3}):
        with pytest.raises(_lib.LseHipError, match="at least 1"):
            acc(**kw)
    acc(n=0)                                      # nothing to add: no launch


def test_the_tool_checks_its_arguments_before_loading_anything(tmp_path):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "simulate_events.py")
    spec = importlib.util.spec_from_file_location("simulate_events_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    missing = str(tmp_path / "no_such_checkpoint")
    out = str(tmp_path / "events.npz")
    with pytest.raises(SystemExit, match="--times or --rate"):
        tool.main([missing, str(tmp_path), out, "--threshold", "0.2"])
    with pytest.raises(SystemExit, match="--times or --rate"):
        tool.main([missing, str(tmp_path), out, "--threshold", "0.2", "--times", "0,1", "--rate", "30"])
    with pytest.raises(SystemExit, match="ascending"):
        tool.main([missing, str(tmp_path), out, "--threshold", "0.2", "--times", "0,2,1"])
    with pytest.raises(SystemExit, match="--threshold"):
        tool.main([missing, str(tmp_path), out, "--threshold", "-1", "--times", "0,1"])
    with pytest.raises(SystemExit, match="--frames needs --frame-every"):
        tool.main([missing, str(tmp_path), out, "--threshold", "0.2", "--times", "0,1", "--frames", str(tmp_path / "ecam")])
    assert not (tmp_path / "events.npz").exists()


from tests.test_scene_io_cpu import scene  # noqa: E402,F401  (the fixture: a tiny scene directory with both camera sets)


def test_the_tools_trajectory_is_the_spline_through_the_scene(scene):  # noqa: F811
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "simulate_events.py")
    spec = importlib.util.spec_from_file_location("simulate_events_tool", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from lsenerf_amd.scene_io import ColorSceneReader
    col = ColorSceneReader(os.path.join(scene["root"], "colcam_set")).outputs("train")
    cams, poses, times, thr = tool.trajectory(scene["root"], None, 4.0, None, None, 1.0, 1.0, None)
    t = col.cameras.times.flatten()
    assert thr == 0.35 and (cams.height, cams.width) == (6, 8)                        # the scene's e_thresh, the event camera's size
    assert times == [float(t[0]) + k / 4.0 for k in range(int((float(t[-1]) - float(t[0])) * 4) + 1)]
    assert poses.shape == (len(times), 3, 4) and poses.dtype == torch.float32 and bool(torch.isfinite(poses).all())
    # at a colour camera's own time the pose is that camera times the colour -> event transform
    c2w = torch.cat([col.cameras.camera_to_worlds[0], torch.tensor([[0.0, 0.0, 0.0, 1.0]])])
    assert float((poses[0] - (c2w @ col.dM)[:3]).abs().max()) < 1e-4
    _, picked, given, thr2 = tool.trajectory(scene["root"], [float(t[0]), float(t[1])], None, None, None, 1.0, 1.0, 0.2)
    assert given == [float(t[0]), float(t[1])] and thr2 == 0.2 and torch.equal(picked[0], poses[0])
    with pytest.raises(SystemExit, match="fewer than two poses"):
        tool.trajectory(scene["root"], None, 0.01, None, None, 1.0, 1.0, None)
