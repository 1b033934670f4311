"""Host side of the count-free occupancy refresh (lsenerf_amd.occ_refresh): the C-ABI surface, the numpy twin of the cell draw
(``draw_cells_host`` -- the specification tests/test_gpu_occ_refresh.py holds the kernel against) and the float64 restatement of
the mean / threshold reduction against the oracle's ``finish_update``."""
import os
import re
import subprocess

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lse_occ_list_occupied", "lse_occ_draw_cells", "lse_occ_update_cells_dev", "lse_occ_mean_threshold")
SEED = 0x15E5EED
BOX = (-1.0, -0.5, -2.0, 1.0, 1.5, 2.0)


def test_header_library_and_binding_carry_the_refresh_entry_points():
    from lsenerf_amd import _lib
    with open(os.path.join(ROOT, "include", "lse_hip.h")) as fh:
        header = fh.read()
    for path in (_lib.LIB_PATH, _lib.DEV_LIB_PATH):
        nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = set(re.findall(r" T (lse_\w+)", nm))
        for name in NEW_SYMBOLS:
            assert name in exported, (path, name)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
    assert int(re.search(r"#define LSE_OCC_LIST_TILE (\d+)", header).group(1)) == _lib.LSE_OCC_LIST_TILE
    assert int(re.search(r"#define LSE_OCC_MEAN_BLOCKS (\d+)", header).group(1)) == _lib.LSE_OCC_MEAN_BLOCKS
    assert _lib.load().lse_abi_version() == 6 == _lib.LSE_ABI_VERSION          # additive: the ABI number stays
    with open(os.path.join(ROOT, "lsenerf_amd", "csrc", "Makefile")) as fh:
        mk = fh.read()
    assert re.search(r"^SRCS = .*\bocc_refresh\b", mk, re.M)
    strict = re.search(r"^STRICT = (.*)$", mk, re.M).group(1).split()           # the sources built without FMA contraction ...
    assert {"traverse", "compose", "occ_refresh"} <= set(strict) <= set(re.search(r"^SRCS = (.*)$", mk, re.M).group(1).split())
    # ... by one rule, shipped and dev
    assert re.search(r"^\$\(STRICT:%=%\.o\) \$\(STRICT:%=dev/%\.o\): FLAGS \+= -ffp-contract=off$", mk, re.M)


def test_fixed_counters_give_fixed_words():
    """Known-answer vectors of Philox4x32-10 (Random123's kat_vectors), then the draw's use of it: counter (step, slot, level, 0),
    key (seed low, seed high), word 0 -> cell, words 1..3 -> jitter."""
    from lsenerf_amd.data import philox4x32_10
    from lsenerf_amd.occ_refresh import draw_cells_host
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array([ctr], dtype=np.uint32), key)[0]
        assert tuple(int(v) for v in got) == want
    C, res, step, level = 4096, (16, 16, 16), 272, 3
    seed = (0xABCD << 32) | SEED                                  # both key words in use
    ids, pos, n = draw_cells_host(seed, step, level, C, res, BOX, warmup=False, occupied=np.zeros(0, dtype=np.int64))
    assert n == C // 4 == ids.shape[0]
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = step, np.arange(n), level
    w = philox4x32_10(ctr, (SEED, 0xABCD))
    idx = (w[:, 0].astype(np.uint64) * np.uint64(C)) >> np.uint64(32)
    assert np.array_equal(ids, level * C + idx.astype(np.int64))
    u = (w[:, 1:] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    coord = np.stack([idx // 256, (idx // 16) % 16, idx % 16], -1).astype(np.float64)
    lo, hi = np.array(BOX[:3]), np.array(BOX[3:])
    assert np.abs(pos - (lo + (coord + u) / 16.0 * (hi - lo))).max() < 1e-5
    # another step, slot range or level is another draw
    for other in ((step + 16, level), (step, level - 1)):
        ids2, _, _ = draw_cells_host(seed, other[0], other[1], C, res, BOX, warmup=False, occupied=np.zeros(0, dtype=np.int64))
        assert (ids2 - other[1] * C != ids - level * C).mean() > 0.99


def _in_closed_box(ids, pos, level, C, res, box):
    idx = ids - level * C
    rx, ry, rz = res
    coord = np.stack([idx // (rz * ry), (idx // rz) % ry, idx % rz], -1).astype(np.float64)
    lo, hi = np.array(box[:3], dtype=np.float64), np.array(box[3:], dtype=np.float64)
    size = (hi - lo) / np.array(res, dtype=np.float64)
    c_lo, c_hi = lo + coord * size, lo + (coord + 1) * size
    eps = 4 * np.finfo(np.float32).eps * np.abs(np.array(box)).max()       # the float32 roundings of the three operations
    return bool(((pos >= c_lo - eps) & (pos <= c_hi + eps)).all())


def test_slot_layout_and_n_dev_for_every_regime_of_the_occupied_count():
    from lsenerf_amd.occ_refresh import draw_cells_host
    C, res, level = 8 * 6 * 10, (8, 6, 10), 1
    N = C // 4
    rng = np.random.default_rng(5)
    for cnt in (0, 7, N, N + 57, C):
        occupied = np.sort(rng.choice(C, cnt, replace=False)).astype(np.int64)
        ids, pos, n = draw_cells_host(SEED, 256, level, C, res, BOX, warmup=False, occupied=occupied)
        m = min(cnt, N)
        assert n == m + N == ids.shape[0] == pos.shape[0]
        idx = ids - level * C
        assert ((idx >= 0) & (idx < C)).all()
        if cnt <= N:
            assert np.array_equal(idx[:m], occupied)              # the list as it is
        else:
            assert np.isin(idx[:m], occupied).all()
            assert len(np.unique(idx[:m])) > m // 2                # drawn, not a copy of the list's head
        assert pos.dtype == np.float32 and _in_closed_box(ids, pos, level, C, res, BOX)
    # warm-up branch: slot i is cell i; negative occs give id -1 at exactly those slots, position still the cell's
    occs = rng.random(C).astype(np.float32)
    neg = rng.choice(C, 11, replace=False)
    occs[neg] = -1.0
    ids, pos, n = draw_cells_host(SEED, 0, level, C, res, BOX, warmup=True, occs_level=occs)
    assert n == C
    assert np.array_equal(np.nonzero(ids < 0)[0], np.sort(neg))
    keep = ids >= 0
    assert np.array_equal(ids[keep], level * C + np.arange(C)[keep])
    assert _in_closed_box(level * C + np.arange(C), pos, level, C, res, BOX)
    # sampled branch: the same rule, wherever the cell came from
    occupied = np.sort(rng.choice(C, 30, replace=False)).astype(np.int64)
    occs[occupied[:3]] = -1.0
    ids, _, n = draw_cells_host(SEED, 256, level, C, res, BOX, warmup=False, occs_level=occs, occupied=occupied)
    assert np.array_equal(ids[:3], [-1, -1, -1]) and (ids[3:30] == level * C + occupied[3:]).all()
    clean, _, _ = draw_cells_host(SEED, 256, level, C, res, BOX, warmup=False, occupied=occupied)
    assert np.array_equal(ids < 0, occs[clean - level * C] < 0)


def test_uniform_draws_fill_the_octants_evenly():
    """N = 524 288 uniform draws over a 128^3 level: the count per octant of the box is Binomial(N, 1/8), sigma = sqrt(N * 1/8 * 7/8)
    = 239.4; every octant within 6 sigma (derived, not tuned)."""
    from lsenerf_amd.occ_refresh import draw_cells_host
    C = 128 ** 3
    N = C // 4
    assert N == 524288
    ids, pos, n = draw_cells_host(SEED, 256, 0, C, (128, 128, 128), BOX, warmup=False, occupied=np.zeros(0, dtype=np.int64))
    assert n == N
    centre = (np.array(BOX[:3]) + np.array(BOX[3:])) / 2
    octant = ((pos >= centre) * np.array([4, 2, 1])).sum(-1)
    counts = np.bincount(octant, minlength=8)
    sigma = (N * (1 / 8) * (7 / 8)) ** 0.5
    assert abs(sigma - 239.4) < 0.1
    assert np.abs(counts - N / 8).max() <= 6 * sigma, counts
    # and the jitter inside the cells: mean 1/2 with sigma_mean = sqrt(1/12 / N) = 4.0e-4
    idx = ids.astype(np.int64)
    coord = np.stack([idx // (128 * 128), (idx // 128) % 128, idx % 128], -1)
    lo, hi = np.array(BOX[:3]), np.array(BOX[3:])
    u = (pos - lo) / (hi - lo) * 128 - coord
    assert np.abs(u.mean(0) - 0.5).max() <= 6 * (1 / 12 / N) ** 0.5 + 1e-4          # (+ float32 rounding of the positions)


def test_float64_mean_and_threshold_agree_with_the_oracle():
    """``mean_and_threshold_host`` (what lse_occ_mean_threshold rounds to float32) against OccGridOracle.finish_update on a seeded
    grid with negative cells, with the mean below and above ``occ_thre``: the thresholds agree to float32 summation error (the
    oracle sums in float32), the grids everywhere except where ``occs`` lies between the two thresholds."""
    from oracle.sampling import OccGridOracle
    from lsenerf_amd.occ_refresh import mean_and_threshold_host
    g = torch.Generator().manual_seed(11)
    for scale, capped in ((0.012, False), (0.05, True)):
        og = OccGridOracle(torch.tensor([-1.0, -1, -1, 1, 1, 1]), 16, 2)
        og.occs = torch.rand(og.occs.shape, generator=g) ** 2 * scale
        og.occs[torch.randperm(og.occs.numel(), generator=g)[:300]] = -1.0
        occs = og.occs.numpy()
        mean_all, thre = mean_and_threshold_host(occs, 0.01)
        assert abs(mean_all - float(og.occs.double().mean())) <= 1e-15
        og.finish_update(0.01)
        thre_oracle = float(torch.clamp(og.occs[og.occs >= 0].mean(), max=0.01))
        assert (thre == 0.01) == capped
        thre32 = float(np.float32(thre))
        assert abs(thre32 - thre_oracle) <= 2e-6 * thre_oracle
        mine = occs > np.float32(thre)
        differ = mine != og.binaries.flatten().numpy()
        lo, hi = min(thre32, thre_oracle), max(thre32, thre_oracle)
        assert ((occs[differ] >= lo) & (occs[differ] <= hi)).all()
        if capped:
            assert thre32 == thre_oracle and not differ.any()
    assert np.isnan(mean_and_threshold_host(np.full(8, -1.0, dtype=np.float32), 0.01)[1])   # torch: mean of an empty selection
