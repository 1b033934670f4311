"""The entry points of csrc/pointcloud.hip against the numpy twin (tests/pointcloud_ref.py), bit for bit: counts, keys and supports
as integers, floats through their int32 view.  The one exception is the merged normal (a root and a divide behind the bit-equal
sums): at most 3 ulp per component -- 1 for the root, 1 for a divisor that is off by one, 1 for the divide's own rounding.  Shapes
are the smallest at which the wave (64) / segment (1024) / scan structure can go wrong: sizes around 64 and 1024, several segments,
more than one block."""
import numpy as np
import pytest
import torch

from tests import pointcloud_ref as pr

pytestmark = pytest.mark.gpu

F = np.float32
LO, HI = (-1.0, -0.75, -0.5), (1.0, 0.5, 0.75)
MIN_ACC = 0.6
SENTINEL = -7.0
NORMAL_ULPS = 3


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))           # (a copy: the twin's shared arrays are read-only)
    return (t if dtype is None else t.to(dtype)).cuda()


def bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, F).view(np.int32)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


def ray_field(n, seed):
    """n rays with every edge of the validity rule sprinkled in: origins, directions, depth, acc, colours, normals (float32)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform(-0.4, 0.4, (n, 3)).astype(F)
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    t = rng.uniform(0.05, 1.2, n).astype(F)
    a = rng.uniform(0.0, 1.0, n).astype(F)
    depth_edges = [np.nan, np.inf, 0.0, -0.5, -np.inf, np.finfo(F).tiny]
    acc_edges = [MIN_ACC, down(MIN_ACC), up(MIN_ACC), np.nan, 1.0, 0.0, np.inf]
    for i in range(0, n, 3):                       # every third ray carries an edge; the kind cycles
        kind = (i // 3) % 4
        if kind == 0:
            t[i] = depth_edges[(i // 12) % len(depth_edges)]
        elif kind == 1:
            a[i] = acc_edges[(i // 12) % len(acc_edges)]
        else:                                      # a point exactly on a box face, or one ulp outside it
            k, side, out = (i // 12) % 3, (i // 36) % 2, kind == 3
            o[i] = 0.0
            d[i] = 0.0
            d[i, k] = 1.0 if side else -1.0
            face = F(HI[k] if side else -LO[k])    # the depth that lands on the face: 0 + (+-1) * face is exact
            t[i] = up(face) if out else face
            a[i] = 1.0
    col = rng.uniform(0, 1, (n, 3)).astype(F)
    nrm = rng.normal(size=(n, 3)).astype(F)
    return o, d, t, a, col, nrm


def gpu_append(views, cap, colors=True, normals=True, total0=None, extra=0):
    """``ops.unproject_append`` over ``views`` into sentinel-filled buffers of cap + extra rows (the op sees the first cap)."""
    from lsenerf_amd import ops
    full = lambda on: torch.full((cap + extra, 3), SENTINEL, device="cuda") if on else None
    P, C, N = full(True), full(colors), full(normals)
    total = torch.zeros(1, dtype=torch.int64, device="cuda") if total0 is None else total0
    cut = lambda t: None if t is None else t[:cap]
    for o, d, t, a, c, n in views:
        ops.unproject_append(dev(o), dev(d), dev(t), dev(a), LO, HI, MIN_ACC, cut(P), total, colors=dev(c) if colors else None,
                             normals=dev(n) if normals else None, out_colors=cut(C), out_normals=cut(N))
    return P, C, N, total


def check_append(views, cap, colors, normals, extra=0):
    P, C, N, total = gpu_append(views, cap, colors, normals, extra=extra)
    twin_views = [(o, d, t, a, c if colors else None, n if normals else None) for o, d, t, a, c, n in views]
    wp, wc, wn, wtotal = pr.append(twin_views, LO, HI, MIN_ACC, cap=cap)
    assert int(total.item()) == wtotal
    k = min(wtotal, cap)
    assert len(wp) == k
    for got, want in ((P, wp), (C, wc), (N, wn)):
        assert (got is None) == (want is None)
        if got is not None:
            assert same_bits(got[:k], want)
            assert bool((got[k:] == SENTINEL).all())          # rows at or beyond the total, or the capacity, are untouched
    return wtotal


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 5000])
def test_append_equals_the_twin(n):
    view = ray_field(n, seed=n)
    kept = None
    for colors, normals in ((True, True), (True, False), (False, True), (False, False)):
        kept = check_append([view], n, colors, normals)
    if n >= 63:
        assert 0 < kept < n
    if n == 5000:           # the edges really are there: rays on a face are kept, one ulp outside dropped
        p, keep = pr.unproject(*view[:4], LO, HI, MIN_ACC)
        on_face = [(p[:, k] == F(b[k])) & keep for b in (LO, HI) for k in range(3)]
        assert all(m.any() for m in on_face)
        beyond = [((p[:, k] == up(HI[k])) | (p[:, k] == down(LO[k]))) & ~keep for k in range(3)]
        assert all(m.any() for m in beyond)
        a = view[3]
        assert keep[a == F(MIN_ACC)].any() and keep[a == up(MIN_ACC)].any() and not keep[a == down(MIN_ACC)].any()


def test_append_capacity_below_the_total():
    view = ray_field(3000, seed=11)
    kept = check_append([view], 3000, True, True)
    for cap in (kept // 2, 1, 0, kept, kept + 5):
        assert check_append([view], cap, True, True, extra=16) == kept        # total stays true; rows beyond cap are untouched


def test_three_appends_share_one_total():
    views = [ray_field(n, seed=20 + i) for i, n in enumerate((1000, 65, 2500))]
    total = check_append(views, 3565, True, True)
    assert total > 1000
    check_append(views, total - 7, True, False, extra=8)          # the capacity cuts inside the last view
    # an append behind a total that some other cloud left: rows start there
    start = torch.full((1,), 40, dtype=torch.int64, device="cuda")
    P, _, _, t = gpu_append(views[1:2], 200, False, False, total0=start)
    wp, _, _, wtotal = pr.append([views[1][:4] + (None, None)], LO, HI, MIN_ACC)
    assert int(t.item()) == 40 + wtotal and same_bits(P[40:40 + wtotal], wp) and bool((P[:40] == SENTINEL).all())


def test_append_of_more_segments_than_scan_threads_behind_a_total():
    """263 169 rays are 258 segments: the scan block takes a second step, its last segment holds one ray, and its carry starts at the
    non-zero total the first view left."""
    n = 257 * 1024 + 1
    small, large = ray_field(5000, seed=40), ray_field(n, seed=41)
    total = check_append([small, large], 5000 + n, True, False)
    kept_small = int(pr.unproject(*small[:4], LO, HI, MIN_ACC)[1].sum())
    assert kept_small > 0 and 0 < total - kept_small < n


def test_append_with_every_ray_dropped_and_with_no_ray():
    o, d, t, a, c, n = ray_field(1500, seed=3)
    P, C, N, total = gpu_append([(o, d, t, np.zeros_like(a), c, n)], 1500)
    assert int(total.item()) == 0 and all(bool((b == SENTINEL).all()) for b in (P, C, N))
    empty = tuple(v[:0] for v in (o, d, t, a, c, n))
    P, _, _, total = gpu_append([empty], 4)
    assert int(total.item()) == 0 and bool((P == SENTINEL).all())


def test_append_twice_gives_the_same_bytes():
    views = [ray_field(n, seed=30 + i) for i, n in enumerate((5000, 1025))]
    a, b = gpu_append(views, 6025), gpu_append(views, 6025)
    for x, y in zip(a, b):
        assert torch.equal(x, y) if x.dtype != torch.float32 else same_bits(x, y)


# ---- keys -----------------------------------------------------------------------------------------------------------------------
def key_points(n, lo, hi, seed):
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    p = rng.uniform(lo - 0.2, hi + 0.2, (n, 3)).astype(F)        # inside and outside the box
    p[0] = lo
    if n > 1:
        p[1] = hi
    if n > 8:
        p[2] = [np.nan, 0.0, np.inf]
        p[3] = [-np.inf, np.nan, 0.0]
        p[4] = down(lo[0]), down(lo[1]), down(lo[2])
        p[5] = up(hi[0]), up(hi[1]), up(hi[2])
        p[6] = lo[0], hi[1], lo[2]
    return p


@pytest.mark.parametrize("res,voxel", [((40, 40, 40), 0.05), ((7, 1, 300), 0.1), ((1, 1, 1), 3.0)])
@pytest.mark.parametrize("n", [1, 257, 2000])
def test_keys_equal_the_twin(res, voxel, n):
    from lsenerf_amd import ops
    lo = (-1.0, -0.3, 0.25)
    hi = tuple(l + r * voxel for l, r in zip(lo, res))
    p = key_points(n, lo, hi, seed=n)
    for count in (None, n, n // 2, 0, n + 9):
        n_dev = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
        got = ops.voxel_keys(dev(p), lo, voxel, res, n_dev=n_dev).cpu().numpy()
        want = pr.voxel_keys(p, lo, voxel, res, count=count)
        assert np.array_equal(got, want), count
        c = n if count is None else min(n, count)
        assert (got[c:] == pr.NO_KEY).all() and (got[:c] < res[0] * res[1] * res[2]).all() and (got[:c] >= 0).all()
    if n > 1:
        full = pr.voxel_keys(p, lo, voxel, res)
        assert full[0] == 0                                        # the point on lo
        assert full[1] == res[0] * res[1] * res[2] - 1             # the point on hi is clamped to n_k - 1


def test_keys_lattice_limits():
    from lsenerf_amd import _lib, ops
    big = 1 << 20
    p = dev(np.array([[0, 0, 0], [1, 1, 1], [0.5, 0.25, 2.0]], F))
    got = ops.voxel_keys(p, (0.0, 0.0, 0.0), 2.0 ** -20, (big, big, big)).cpu().numpy()
    assert got.tolist() == pr.voxel_keys(p.cpu().numpy(), (0, 0, 0), 2.0 ** -20, (big, big, big)).tolist()
    assert got[1] == 2 ** 60 - 1 and got[0] == 0
    for res in ((big + 1, 1, 1), (1, big + 1, 1), (1, 1, big + 1), (0, 1, 1), (1, 1, -3)):
        with pytest.raises(_lib.LseHipError, match="every count in"):
            ops.voxel_keys(p, (0.0, 0.0, 0.0), 1.0, res)
    with pytest.raises(_lib.LseHipError, match="voxel size"):
        ops.voxel_keys(p, (0.0, 0.0, 0.0), 0.0, (4, 4, 4))


# ---- merge ----------------------------------------------------------------------------------------------------------------------
def merge_case(run_lengths, seed, tail=0, shuffle=True):
    """A cloud whose voxels have the given run lengths (in key order), its points shuffled; ``tail`` rows without a key behind them.
    Returns keys [n] (INT64_MAX on the tail), points, colours, unit-ish normals."""
    rng = np.random.default_rng(seed)
    lengths = np.asarray(run_lengths, np.int64)
    voxel_key = np.cumsum(rng.integers(1, 5, len(lengths)))      # ascending, with gaps
    keys = np.repeat(voxel_key, lengths)
    n = len(keys)
    perm = rng.permutation(n) if shuffle else np.arange(n)
    keys = np.concatenate([keys[perm], np.full(tail, pr.NO_KEY, np.int64)])
    n += tail
    pts = rng.normal(scale=0.7, size=(n, 3)).astype(F)
    col = rng.uniform(0, 1, (n, 3)).astype(F)
    base = rng.normal(size=(len(lengths) + 1, 3))                # one direction per voxel, jittered: sums far from zero
    owner = np.concatenate([np.repeat(np.arange(len(lengths)), lengths)[perm], np.full(tail, len(lengths))])
    nrm = base[owner] + rng.normal(scale=0.2, size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(F)
    return keys, pts, col, nrm


def check_merge(keys, pts, col, nrm, cap=None):
    """GPU merge of the stable-sorted cloud against the twin; returns (voxels, largest normal distance in ulp)."""
    from lsenerf_amd import ops
    n = len(keys)
    sorted_keys, order = torch.sort(dev(keys), stable=True)
    assert np.array_equal(order.cpu().numpy(), np.argsort(keys, kind="stable"))
    P, C, N = dev(pts), dev(col), dev(nrm)
    gk, gc, gp, gcol, gn, total = ops.voxel_merge(sorted_keys, order, P, C, N, cap=cap)
    wk, wc, wp, wcol, wn, wsum = pr.voxel_merge(sorted_keys.cpu().numpy(), order.cpu().numpy(), pts, col, nrm, with_normal_sums=True)
    m = len(wk)
    assert int(total.item()) == m
    k = m if cap is None else min(m, cap)
    assert gk.shape[0] == (n if cap is None else cap)
    assert np.array_equal(gk[:k].cpu().numpy(), wk[:k]) and np.array_equal(gc[:k].cpu().numpy(), wc[:k])
    assert gc.dtype == torch.int32
    assert same_bits(gp[:k], wp[:k]) and same_bits(gcol[:k], wcol[:k])
    # the normal sums, bit for bit, through the colour path: mean = s_n / (float)c
    _, _, _, gsum, _, _ = ops.voxel_merge(sorted_keys, order, P, N, None, cap=cap)
    assert same_bits(gsum[:k], (wsum / wc[:, None].astype(F)).astype(F)[:k])
    assert float(np.sqrt((wsum.astype(np.float64) ** 2).sum(-1)).min(initial=1.0)) > 1e-12
    ulps = pr.ulp_distance(gn[:k].cpu().numpy(), wn[:k])
    print(f"merge n={n} voxels={m}: normals differ by at most {ulps} ulp")
    assert ulps <= NORMAL_ULPS
    # without attributes
    k2, c2, p2, col2, n2, t2 = ops.voxel_merge(sorted_keys, order, P, cap=cap)
    assert col2 is None and n2 is None and int(t2.item()) == m and same_bits(p2[:k], wp[:k]) and torch.equal(k2[:k], gk[:k])
    return m, ulps


# runs that start and end on, just before and just after the segment borders at 1024, 2048 and 3072; every length the issue names
BORDER_RUNS = [1023, 1, 1024, 2, 63, 64, 65] + [1] * 829 + [3000, 1, 2, 64]


def test_merge_runs_across_segment_borders():
    assert sum(BORDER_RUNS[:1]) == 1023 and sum(BORDER_RUNS[:2]) == 1024 and sum(BORDER_RUNS[:3]) == 2048
    assert sum(BORDER_RUNS[:-4]) == 3071                       # the run of 3000 starts one before a border and spans three
    m, _ = check_merge(*merge_case(BORDER_RUNS, seed=1))
    assert m == len(BORDER_RUNS)
    check_merge(*merge_case(BORDER_RUNS, seed=2, tail=100))     # rows without a key behind the cloud
    check_merge(*merge_case([1025, 1, 1022, 1, 1], seed=3, tail=1))      # just after / just before


@pytest.mark.parametrize("runs", [[2000], [1] * 1500, [1], [64], [65], [1, 1]], ids=["one-voxel", "all-distinct", "1", "64", "65", "2"])
def test_merge_shapes(runs):
    m, _ = check_merge(*merge_case(runs, seed=len(runs)))
    assert m == len(runs)


def test_merge_of_nothing_and_capacity_below_the_voxel_count():
    from lsenerf_amd import ops
    keys, pts, col, nrm = merge_case([], seed=5, tail=70)        # count 0: every row lacks a key
    assert check_merge(keys, pts, col, nrm)[0] == 0
    e64, e3 = torch.empty(0, dtype=torch.int64, device="cuda"), torch.empty((0, 3), device="cuda")
    out = ops.voxel_merge(e64, e64, e3, e3, e3)                  # extent 0: the total is still written
    assert int(out[5].item()) == 0 and out[2].shape == (0, 3)
    case = merge_case([3, 1, 70, 2, 1, 1, 5] * 40, seed=6)
    for cap in (0, 1, 100, 279, 280, 281):
        assert check_merge(*case, cap=cap)[0] == 280
    sorted_keys, order = torch.sort(dev(case[0]), stable=True)
    a = ops.voxel_merge(sorted_keys, order, dev(case[1]), dev(case[2]), dev(case[3]))
    b = ops.voxel_merge(sorted_keys, order, dev(case[1]), dev(case[2]), dev(case[3]))
    for x, y in zip(a, b):
        assert np.array_equal(x[:280].cpu().numpy().view(np.uint8), y[:280].cpu().numpy().view(np.uint8))     # two runs, same bytes


# ---- support filter -------------------------------------------------------------------------------------------------------------
def check_filter(keys, counts, res, min_support, count=None, cap=None, seed=0):
    from lsenerf_amd import ops
    rng = np.random.default_rng(seed)
    m = len(keys)
    pts, col, nrm = (rng.normal(size=(m, 3)).astype(F) for _ in range(3))
    keys, counts = np.asarray(keys, np.int64), np.asarray(counts, np.int32)
    m_dev = None if count is None else torch.tensor([count], dtype=torch.int64, device="cuda")
    gk, gc, gp, gcol, gn, total, sup = ops.voxel_support_filter(dev(keys), dev(counts), dev(pts), res, min_support, dev(col), dev(nrm),
                                                                m_dev=m_dev, cap=cap, want_support=True)
    keep, wsup = pr.support_filter(keys, counts, res, min_support, count=count)
    assert sup.dtype == torch.int32 and np.array_equal(sup.cpu().numpy(), wsup)
    kept = int(keep.sum())
    assert int(total.item()) == kept
    k = kept if cap is None else min(kept, cap)
    assert np.array_equal(gk[:k].cpu().numpy(), keys[keep][:k]) and np.array_equal(gc[:k].cpu().numpy(), counts[keep][:k])
    for got, want in ((gp, pts), (gcol, col), (gn, nrm)):
        assert same_bits(got[:k], want[keep][:k])
    k2, c2, p2, col2, n2, t2, s2 = ops.voxel_support_filter(dev(keys), dev(counts), dev(pts), res, min_support, m_dev=m_dev, cap=cap)
    assert col2 is None and n2 is None and s2 is None and int(t2.item()) == kept and torch.equal(k2[:k], gk[:k])
    return keep, wsup


def key_of(v, res):
    return (v[0] * res[1] + v[1]) * res[2] + v[2]


def test_filter_full_block_and_lattice_borders():
    res = (5, 6, 7)
    block = sorted(key_of((2 + dx, 3 + dy, 1 + dz), res) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for dz in (-1, 0, 1))
    counts = np.arange(1, 28)
    keep, sup = check_filter(block, counts, res, 100)
    centre = block.index(key_of((2, 3, 1), res))
    assert sup[centre] == counts.sum() == 378 and keep.tolist() == (sup >= 100).tolist() and 0 < keep.sum() < 27
    # the whole of a small lattice: corners, edges and faces skip the offsets that leave it
    res = (3, 4, 5)
    rng = np.random.default_rng(4)
    counts = rng.integers(1, 10, 60)
    keep, sup = check_filter(np.arange(60), counts, res, 0)
    assert keep.all() and sup[0] == sum(counts[key_of((x, y, z), res)] for x in (0, 1) for y in (0, 1) for z in (0, 1))
    for thr in (1, int(sup.max()), int(sup.max()) + 1, int(np.median(sup))):
        keep, _ = check_filter(np.arange(60), counts, res, thr)
        assert keep.sum() == (sup >= thr).sum()
    assert not check_filter(np.arange(60), counts, res, int(sup.max()) + 1)[0].any()
    # one voxel per axis: every neighbour but the voxel itself is outside
    assert check_filter([0], [5], (1, 1, 1), 5)[1].tolist() == [5]


def test_filter_adjacent_keys_are_not_neighbours():
    res = (4, 5, 6)
    for a, b in (((1, 2, 5), (1, 3, 0)), ((1, 4, 5), (2, 0, 0))):
        ka, kb = key_of(a, res), key_of(b, res)
        assert kb - ka == 1
        keep, sup = check_filter([ka, kb], [3, 4], res, 4)
        assert sup.tolist() == [3, 4] and keep.tolist() == [False, True]           # each supports only itself
    # while true neighbours across a large key gap do count
    ka, kb = key_of((1, 2, 3), res), key_of((2, 3, 4), res)
    assert check_filter([ka, kb], [3, 4], res, 7)[1].tolist() == [7, 7]


@pytest.mark.parametrize("m", [1, 64, 65, 1025])
def test_filter_sizes_and_device_counts(m):
    res = (12, 11, 13)
    rng = np.random.default_rng(m)
    keys = np.sort(rng.choice(res[0] * res[1] * res[2], m, replace=False))
    counts = rng.integers(1, 10, m)
    _, sup = check_filter(keys, counts, res, 0)
    thr = int(np.median(sup))
    for count in (None, m, m // 2, 0, m + 3):
        for cap in (None, max(m // 3, 1)):
            check_filter(keys, counts, res, thr, count=count, cap=cap, seed=1)
    check_filter(keys, counts, res, 1)
    check_filter(keys, counts, res, int(sup.max()))


def test_the_analytic_scene_end_to_end():
    from lsenerf_amd import ops
    s = pr.scene_cloud()
    views = pr.scene()
    lo, hi = pr.BOX
    cap = sum(len(v[2]) for v in views)
    pts = torch.full((cap, 3), SENTINEL, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    for o, d, t, a in views:
        ops.unproject_append(dev(o), dev(d), dev(t), dev(a), lo, hi, 0.5, pts, total)
    assert int(total.item()) == s["total"] == 6794 and same_bits(pts[:6794], s["points"])
    res = ops.voxel_lattice(lo, hi, pr.VOXEL)
    assert res == s["res"]
    keys = ops.voxel_keys(pts, lo, pr.VOXEL, res, n_dev=total)
    sorted_keys, order = torch.sort(keys, stable=True)
    mk, mc, mp, _, _, mt = ops.voxel_merge(sorted_keys, order, pts)
    assert int(mt.item()) == 2142
    assert np.array_equal(mk[:2142].cpu().numpy(), s["keys"]) and np.array_equal(mc[:2142].cpu().numpy(), s["counts"])
    assert same_bits(mp[:2142], s["merged"])
    fk, fc, fp, _, _, ft, sup = ops.voxel_support_filter(mk, mc, mp, res, 4, m_dev=mt, want_support=True)
    keep = ~s["planted_only"]
    assert int(ft.item()) == 2142 - pr.N_PLANTED == int(keep.sum())
    assert np.array_equal(fk[:2123].cpu().numpy(), s["keys"][keep])              # exactly the twin's surviving keys
    assert np.array_equal(sup[:2142].cpu().numpy(), s["support"]) and bool((sup[2142:] == 0).all())
    assert same_bits(fp[:2123], s["merged"][keep]) and np.array_equal(fc[:2123].cpu().numpy(), s["counts"][keep])
