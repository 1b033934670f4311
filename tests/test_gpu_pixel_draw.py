"""The weighted pixel draw on the GPU (csrc/pixel_draw.hip through ``ops.pixel_rows_build`` / ``ops.pixel_draw``): the row table, the
drawn pixels and their weights are integers, so every check is bit equality with the numpy twin (tests/pixel_draw_ref.py).  The
shapes are the smallest at which each part can go wrong: one pixel, a tail chunk, the chunk borders of the pixel walk, more rows than
two rounds of the 64-ary row search resolve, totals of 1 to 7, and a total beyond 2^32."""
import numpy as np
import pytest
import torch

from tests import pixel_draw_ref as pr

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 65, 597, 2316)
SEED = 2 ** 40 + 7
NP_OF = {"i8": np.int8, "u8": np.uint8, "i16": np.int16, "i32": np.int32, "f32": np.float32}


def _dev(a):
    return None if a is None or isinstance(a, tuple) else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check(images, msk, w_active, w_idle, counts=COUNTS, steps=(3,), stream_id=1, w=None):
    """Table, pixels and weights of the device against the twin.  ``images``: an array, or a shape tuple for a set without them."""
    from lsenerf_amd import ops
    shape = images if isinstance(images, tuple) else images.shape
    w = pr.pixel_weights(images, msk, w_active, w_idle) if w is None else w
    want_off = pr.row_table(w)
    d_img, d_msk = _dev(images), _dev(msk)
    row_off = ops.pixel_rows_build(d_img, d_msk, shape, w_active, w_idle,
                                   row_off=torch.full((len(want_off),), -1, dtype=torch.int64, device="cuda"))
    assert np.array_equal(row_off.cpu().numpy(), want_off)
    total = int(want_off[-1])
    assert total > 0
    for n in counts:
        for step in steps:
            idx, wt = ops.pixel_draw(d_img, d_msk, shape, w_active, w_idle, row_off, SEED, stream_id, n, step=step)
            want_idx, want_wt = pr.draw(w, SEED, step, stream_id, n, row_off=want_off)
            assert idx.dtype == wt.dtype == torch.int32 and tuple(idx.shape) == (n, 3) and tuple(wt.shape) == (n,)
            assert np.array_equal(idx.cpu().numpy(), want_idx), (n, step)
            assert np.array_equal(wt.cpu().numpy(), want_wt), (n, step)
            assert int(wt.min()) > 0                                     # nothing of weight zero is ever drawn
    return w, want_off, (d_img, d_msk, row_off)


def _frames(kind, shape, active, seed):
    """Sparse frames of one pixel type, with negative values where the type has them and a -0.0 for float32."""
    rng = np.random.default_rng(seed)
    on = rng.random(shape) < active
    if kind == "f32":
        v = (rng.standard_normal(shape) * on).astype(np.float32)
        flat = v.reshape(-1)
        flat[np.flatnonzero(flat == 0)[::3]] = -0.0                      # idle, whatever its sign bit says
        assert np.signbit(flat[flat == 0]).any() and (flat < 0).any()
        return v
    dt = NP_OF[kind]
    lo = 0 if kind == "u8" else int(np.iinfo(dt).min)
    mag = rng.integers(lo, int(np.iinfo(dt).max) + 1, shape)
    v = (mag * on).astype(dt)
    assert kind == "u8" or (v < 0).any()
    return v


def test_one_pixel():
    for kind in NP_OF:
        img = np.array([[[3]]]).astype(NP_OF[kind])
        w, off, _ = _check(img, None, 9, 1, counts=(1, 63, 65))
        assert off.tolist() == [0, 9]
    _check((1, 1, 1), np.ones((1, 1, 1), np.uint8), 1, 1, counts=(1, 65), stream_id=0)


@pytest.mark.parametrize("kind", sorted(NP_OF))
@pytest.mark.parametrize("msk_kind", ["u8", "f32"])
def test_tail_chunk_with_masks_activity_and_every_pixel_type(kind, msk_kind):
    """2 x 3 x 70: a full chunk and a tail of 6 pixels per row; half the pixels masked, a tenth active, weights 9 / 1."""
    shape = (2, 3, 70)
    rng = np.random.default_rng(11)
    img = _frames(kind, shape, 0.1, 12)
    msk = (rng.random(shape) < 0.5).astype(np.uint8 if msk_kind == "u8" else np.float32)
    if msk_kind == "f32":
        msk *= rng.choice([0.25, 1.0, -2.0], shape).astype(np.float32)    # any non-zero value keeps the pixel
        msk[msk == 0] = np.where(rng.random(int((msk == 0).sum())) < 0.5, -0.0, 0.0)
    w, _, _ = _check(img, msk, 9, 1)
    assert set(np.unique(w)) == {0, 1, 9}
    _check(img, msk, 9, 0, counts=(65, 597))                              # idle pixels are never drawn
    _check(img, msk, 0, 3, counts=(65, 597))                              # active pixels are never drawn
    _check(img, None, 9, 1, counts=(65, 597))                             # respect_mask=False with a mask present: it is not passed
    _check(shape, msk, 1, 1, counts=(65, 597), stream_id=0)               # the colour stream: the mask alone


def test_the_step_as_an_argument_from_the_device_and_with_bit_32_set():
    from lsenerf_amd import ops
    shape = (2, 3, 70)
    img = _frames("i8", shape, 0.1, 12)
    msk = (np.random.default_rng(11).random(shape) < 0.5).astype(np.uint8)
    hi = 2 ** 32 + 5
    w, off, (d_img, d_msk, row_off) = _check(img, msk, 9, 1, counts=(597,), steps=(0, 5, hi, 2 ** 63 - 1))
    a = pr.draw(w, SEED, 5, 1, 597)[0]
    assert np.array_equal(a, pr.draw(w, SEED, hi, 1, 597)[0]) and not np.array_equal(a, pr.draw(w, SEED, 0, 1, 597)[0])
    step_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    for s in (0, 5, hi):
        step_dev.fill_(s)
        idx, wt = ops.pixel_draw(d_img, d_msk, shape, 9, 1, row_off, SEED, 1, 597, step_dev=step_dev)
        want = pr.draw(w, SEED, s, 1, 597)
        assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(wt.cpu().numpy(), want[1])
        assert int(step_dev) == s                                         # the draw reads the counter, it does not advance it
    # the streams differ, and the outputs may be the caller's static buffers
    idx = torch.zeros(597, 3, dtype=torch.int32, device="cuda")
    wt = torch.zeros(597, dtype=torch.int32, device="cuda")
    got = ops.pixel_draw(d_img, d_msk, shape, 9, 1, row_off, SEED, 0, 597, step=5, indices=idx, weights=wt)
    assert got[0] is idx and got[1] is wt
    assert np.array_equal(idx.cpu().numpy(), pr.draw(w, SEED, 5, 0, 597)[0]) and not np.array_equal(idx.cpu().numpy(), a)
    empty = ops.pixel_draw(d_img, d_msk, shape, 9, 1, row_off, SEED, 1, 0, step=1)
    assert tuple(empty[0].shape) == (0, 3) and tuple(empty[1].shape) == (0,)


@pytest.mark.parametrize("W,x", [(64, 63), (128, 64), (129, 128)])
def test_the_only_drawable_pixel_of_a_row_at_a_chunk_border(W, x):
    shape = (1, 3, W)
    msk = np.zeros(shape, np.uint8)
    msk[0, 1, x] = 1
    img = np.full(shape, -7, np.int16)
    w, off, _ = _check(img, msk, 9, 1, counts=(1, 65))
    assert off.tolist() == [0, 0, 9, 9]
    # ... and as the last of several: the pixels in front of it are drawable too, the rest of the row is not
    msk[0, 1, :x] = 1
    img[0, 1, :x:2] = 0
    _check(img, msk, 9, 1, counts=(65, 597))
    msk[0, 1, :x] = 0
    msk[0, 1, x:] = 1                                                     # the first drawable pixel instead
    _check(img, msk, 9, 1, counts=(65,))


def test_a_third_round_of_the_row_search_and_runs_of_masked_rows():
    """67 x 63 x 5: 4221 rows > 64^2.  The first 100, the last 50 and every third row are fully masked."""
    shape = (67, 63, 5)
    rng = np.random.default_rng(21)
    img = _frames("i8", shape, 0.3, 22)
    msk = (rng.random(shape) < 0.8).astype(np.uint8).reshape(-1, 5)
    msk[:100], msk[-50:], msk[::3] = 0, 0, 0
    msk = msk.reshape(shape)
    w, off, _ = _check(img, msk, 9, 1, counts=(65, 2316), steps=(3, 4))
    idx = pr.draw(w, SEED, 3, 1, 2316, row_off=off)[0]
    r = idx[:, 0] * 63 + idx[:, 1]
    assert r.min() >= 100 and r.max() < 4221 - 50 and (r % 3 != 0).all() and len(np.unique(r)) > 1000
    _check(shape, msk, 1, 1, counts=(2316,), stream_id=0)


def test_a_total_of_one_and_totals_of_two_to_seven():
    shape = (3, 4, 5)
    img = np.zeros(shape, np.int32)
    img[1, 2, 3] = -1
    w, off, (d_img, _, row_off) = _check(img, None, 1, 0, counts=(1, 63, 65), steps=(0, 1))
    assert int(off[-1]) == 1
    from lsenerf_amd import ops
    idx, wt = ops.pixel_draw(d_img, None, shape, 1, 0, row_off, SEED, 1, 65, step=9)
    assert idx.cpu().tolist() == [[1, 2, 3]] * 65 and wt.cpu().tolist() == [1] * 65
    rng = np.random.default_rng(31)
    for total in range(2, 8):
        img = np.zeros(3 * 4 * 5, np.int32)
        img[rng.choice(60, total, replace=False)] = 5
        img = img.reshape(shape)
        seen = set()
        for s in range(8):
            seen |= set(pr.positions(SEED, s, 1, 8, total))
        assert {0, total - 1} <= seen                                     # both ends of [0, total) occur in these steps
        _check(img, None, 1, 0, counts=(8,), steps=tuple(range(8)))


def test_a_total_beyond_32_bits():
    """One uint8 image of 4112 x 4112, all active, weight 255: the total is 255 * 4112^2 > 2^32, so the table's last entries and the
    positions of most draws do not fit 32 bits."""
    shape = (1, 4112, 4112)
    img = np.full(shape, 200, np.uint8)
    w = np.full(shape, 255, np.int64)
    _, off, _ = _check(img, None, 255, 7, counts=(65, 2316), w=w)
    assert int(off[-1]) == 255 * 4112 * 4112 > 2 ** 32
    t = pr.positions(SEED, 3, 1, 2316, int(off[-1]))
    assert max(t) > 2 ** 32 and min(t) < 2 ** 32
