"""numpy twin of the event synthesis entry points (include/lse_hip.h, "event synthesis"): ``count`` / ``append`` (the sensor walk and
the ordered stream) and ``accumulate`` (stream -> frames), written from the header's definition with every float32 operation rounded
on its own (numpy float32 arrays never fuse or widen) and the event times in float64.  ``walk_scalar`` is the definition once more,
one pixel and one ``np.float32`` operation at a time: tests/test_events_cpu.py holds the vectorised twin against it."""
import numpy as np

F32 = np.float32


def random_walk_planes(K, P, seed, static=2, sigma=0.35):
    """``L = -2 + cumsum(normal(0, sigma))`` over K + 1 planes of P pixels, float32; plane ``static + 1`` repeats plane ``static``
    (a static interval) when there are that many."""
    rng = np.random.default_rng(seed)
    L = (-2.0 + np.cumsum(rng.normal(0.0, sigma, size=(K + 1, P)), axis=0)).astype(F32)
    if static is not None and static + 1 <= K:
        L[static + 1] = L[static]
    return L


def walk_scalar(L0, L1, ref, c_pos, c_neg, cap_step, t0=0.0, t1=1.0):
    """One interval at one pixel: ``(signed count, ref, [event times])``."""
    L0, L1, ref, c_pos, c_neg = F32(L0), F32(L1), F32(ref), F32(c_pos), F32(c_neg)
    n, pol, times = 0, 0, []

    def emit(level):
        d = F32(L1 - L0)
        q = F32(np.float64(F32(level - L0)) / np.float64(d))
        frac = F32(0) if (d == 0 or np.isnan(q)) else (F32(0) if q < 0 else (F32(1) if q > 1 else q))
        times.append(np.float64(t0) + np.float64(frac) * (np.float64(t1) - np.float64(t0)))
    with np.errstate(all="ignore"):
        if F32(L1 - ref) >= c_pos:
            pol = 1
            while F32(L1 - ref) >= c_pos and n < cap_step:
                ref = F32(ref + c_pos)
                emit(ref)
                n += 1
        elif F32(ref - L1) >= c_neg:
            pol = -1
            while F32(ref - L1) >= c_neg and n < cap_step:
                ref = F32(ref - c_neg)
                emit(ref)
                n += 1
    if n == cap_step:
        ref = L1
    return pol * n, ref, times


def _interval(L0, L1, ref, c_pos, c_neg, cap_step):
    """One interval over all pixels: ``(signed counts int32 [P], ref [P], levels float32 [n_max, P])`` -- levels[e, p] is the level
    behind event e of pixel p (valid for e < |counts[p]|)."""
    ref = ref.copy()
    with np.errstate(all="ignore"):
        up = (L1 - ref) >= c_pos
        down = ~up & ((ref - L1) >= c_neg)
        n = np.zeros(ref.shape, np.int32)
        levels = []
        for _ in range(cap_step):
            go_up = up & ((L1 - ref) >= c_pos)
            go_down = down & ((ref - L1) >= c_neg)
            go = go_up | go_down
            if not go.any():
                break
            ref = np.where(go_up, ref + c_pos, np.where(go_down, ref - c_neg, ref)).astype(F32)
            n += go
            levels.append(ref.copy())
    ref = np.where(n == cap_step, L1, ref).astype(F32)
    counts = np.where(up, n, -n).astype(np.int32)
    return counts, ref, (np.stack(levels) if levels else np.zeros((0,) + ref.shape, F32))


def _check(c_pos, c_neg, cap_step):
    c_pos, c_neg = F32(c_pos), F32(c_neg)
    assert 0 < c_pos < np.inf and 0 < c_neg < np.inf and 1 <= cap_step <= 32767
    return c_pos, c_neg


def count(L, ref, c_pos, c_neg, cap_step):
    """lse_event_count: ``(counts int32 [K, P], ref_out float32 [P], window_total)``."""
    c_pos, c_neg = _check(c_pos, c_neg, cap_step)
    L = np.asarray(L, F32)
    ref = np.asarray(ref, F32).copy()
    K = L.shape[0] - 1 if L.shape[0] else 0
    counts = np.zeros((K, ref.shape[0]), np.int32)
    for k in range(K):
        counts[k], ref, _ = _interval(L[k], L[k + 1], ref, c_pos, c_neg, cap_step)
    return counts, ref, int(np.abs(counts.astype(np.int64)).sum())


def append(L, times, W, ref, c_pos, c_neg, cap_step):
    """lse_event_append of one window: ``(counts, (x int16, y int16, t float64, p int8), ref_out)`` in stream order."""
    c_pos, c_neg = _check(c_pos, c_neg, cap_step)
    L = np.asarray(L, F32)
    times = np.asarray(times, np.float64)
    ref = np.asarray(ref, F32).copy()
    P = ref.shape[0]
    K = L.shape[0] - 1 if L.shape[0] else 0
    assert P % W == 0 and W <= 32767 and P // W <= 32767
    counts = np.zeros((K, P), np.int32)
    xs, ys, ts, ps = [], [], [], []
    for k in range(K):
        L0, L1 = L[k], L[k + 1]
        counts[k], ref, levels = _interval(L0, L1, ref, c_pos, c_neg, cap_step)
        n = np.abs(counts[k])
        mask = np.arange(levels.shape[0])[None, :] < n[:, None]           # [P, n_max]: pixel ascending, emission order
        pix, e = np.nonzero(mask)
        level = levels[e, pix]
        with np.errstate(all="ignore"):
            d = (L1 - L0)[pix]
            num = level - L0[pix]
            q = (num.astype(np.float64) / d.astype(np.float64)).astype(F32)
            frac = np.where((d == 0) | np.isnan(q), F32(0), np.where(q < 0, F32(0), np.where(q > 1, F32(1), q))).astype(F32)
        dt = times[k + 1] - times[k]
        prod = frac.astype(np.float64) * dt
        ts.append(times[k] + prod)
        xs.append((pix % W).astype(np.int16))
        ys.append((pix // W).astype(np.int16))
        ps.append(np.sign(counts[k])[pix].astype(np.int8))
    cat = lambda parts, dt: np.concatenate(parts).astype(dt) if parts else np.zeros(0, dt)
    return counts, (cat(xs, np.int16), cat(ys, np.int16), cat(ts, np.float64), cat(ps, np.int8)), ref


def simulate(L, times, W, ref, c_pos, c_neg, cap_step, window=None):
    """``append`` over the whole plane set, or chained over windows of ``window`` intervals (the last plane of a window is the first
    of the next, ``ref_out`` of one is ``ref_in`` of the next)."""
    L = np.asarray(L, F32)
    K = L.shape[0] - 1
    window = K if not window else window
    counts, parts = [], []
    ref = np.asarray(ref, F32)
    for k0 in range(0, K, max(window, 1)):
        k1 = min(k0 + window, K)
        c, ev, ref = append(L[k0:k1 + 1], np.asarray(times)[k0:k1 + 1], W, ref, c_pos, c_neg, cap_step)
        counts.append(c)
        parts.append(ev)
    if not parts:
        return append(L, times, W, ref, c_pos, c_neg, cap_step)
    return np.concatenate(counts), tuple(np.concatenate([p[j] for p in parts]) for j in range(4)), ref


def accumulate(x, y, t, p, bounds, H, W, acc=None, count=None):
    """lse_event_accumulate: adds the counted events of ``x, y, t, p`` (the first ``count``) into ``acc`` int32 [F, H, W]."""
    bounds = np.asarray(bounds, np.float64)
    F = bounds.shape[0] - 1
    acc = np.zeros((F, H, W), np.int32) if acc is None else acc.copy()
    m = len(t) if count is None else max(0, min(len(t), int(count)))
    x, y, t, p = (np.asarray(a)[:m] for a in (x, y, t, p))
    with np.errstate(all="ignore"):
        ok = (bounds[0] <= t) & (t < bounds[F]) & (x >= 0) & (x < W) & (y >= 0) & (y < H)
    f = np.searchsorted(bounds, t[ok], side="right") - 1                 # the largest f with bounds[f] <= t
    np.add.at(acc, (f, y[ok].astype(np.int64), x[ok].astype(np.int64)), p[ok].astype(np.int32))
    return acc


def boundary_ties(t, bounds):
    """Events whose time equals a bound: where accumulate's half-open frames and the per-frame counts may differ."""
    return int(np.isin(np.asarray(t, np.float64), np.asarray(bounds, np.float64)).sum())
