"""Numpy twin of the weighted pixel draw (include/lse_hip.h, "weighted pixel draw"; csrc/pixel_draw.hip): Python integers and int64
arrays only, so every value is exact.  The "count minus one" forms are written literally -- no searchsorted, no shortcut -- so that
the kernels' searches and the package's own host twin (``BatchComposer.indices_host``) are held to the definition itself."""
import numpy as np

from lsenerf_amd.data import philox4x32_10


def pixel_weights(images, msk, w_active, w_idle):
    """int64 [n, H, W].  ``images``: [n, H, W] of any numeric type, or a shape tuple (a set whose pixels differ only by the mask:
    every unmasked pixel weighs ``w_idle``); ``msk``: [n, H, W] or None.  Values are compared after the conversion to float32."""
    if isinstance(images, tuple):
        w = np.full(images, w_idle, dtype=np.int64)
    else:
        w = np.where(np.asarray(images).astype(np.float32) != 0, w_active, w_idle).astype(np.int64)
    if msk is not None:
        w = np.where(np.asarray(msk).astype(np.float32) == 0, 0, w)
    return w


def row_table(w):
    """int64 [rows + 1]: exclusive prefix sums of the row sums, the total last."""
    sums = w.reshape(-1, w.shape[-1]).sum(1, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(sums, dtype=np.int64)]).astype(np.int64)


def mulhi64(a, b):
    return (int(a) * int(b)) >> 64


def pick(w, row_off, t):
    """``(r, x, weight)`` of the position ``t`` in ``[0, total)``: sections 3 to 7 of the definition."""
    w2 = w.reshape(-1, w.shape[-1])
    rows = w2.shape[0]
    r = int((row_off[:rows] <= t).sum()) - 1
    v = int(t) - int(row_off[r])
    excl = np.cumsum(w2[r], dtype=np.int64) - w2[r]
    x = int((excl <= v).sum()) - 1
    return r, x, int(w2[r, x])


def positions(seed, step, stream_id, n, total):
    """``t`` of the pixels 0 .. n - 1: the Philox call of the uniform draw, then ``mulhi64((w0 << 32) | w1, total)``."""
    ctr = np.zeros((n, 4), dtype=np.uint32)
    ctr[:, 0] = int(step) & 0xFFFFFFFF
    ctr[:, 1] = np.arange(n, dtype=np.uint32)
    ctr[:, 2] = stream_id
    p = philox4x32_10(ctr, (int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF))
    return [mulhi64((int(a) << 32) | int(b), total) for a, b in p[:, :2]]


def draw(w, seed, step, stream_id, n, row_off=None):
    """``(indices int64 [n, 3] = (c, y, x), weights int64 [n])`` of a stream whose pixel weights are ``w`` [n_images, H, W]."""
    H = w.shape[1]
    row_off = row_table(w) if row_off is None else row_off
    idx, wt = np.zeros((n, 3), np.int64), np.zeros(n, np.int64)
    for i, t in enumerate(positions(seed, step, stream_id, n, int(row_off[-1]))):
        r, x, wt[i] = pick(w, row_off, t)
        idx[i] = (r // H, r % H, x)
    return idx, wt
