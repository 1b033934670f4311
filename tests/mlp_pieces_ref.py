"""numpy twin of the reduced-piece MLP forwards (include/lse_hip.h: lse_mlp_desc.arith; lsenerf_amd/csrc/mlp_x6.h).

A route with NP pieces per operand cuts weights and activations into bf16 pieces and forms exactly the piece products
``a_i * b_j`` with ``i + j < NP``: NP = 3 is bf16x6 (six products), NP = 2 bf16x3 (hi*hi + hi*mid + mid*hi), NP = 1 bf16x1.
Pieces are cut by round-to-nearest-even, ``p0 = bf16_rn(x)``, ``p1 = bf16_rn(x - p0)`` (the subtraction is exact in f32); the
three-piece WEIGHT images of bf16x6 are cut by truncation instead, as the kernels do.  Every product is exact in f32 (8 x 8
significant bits); the twin sums them in float64, adds the row bias and rounds ONCE to f32, where the kernel accumulates in f32
inside the matrix core -- equal bits wherever every partial sum is exactly representable, f32 summation error apart elsewhere.

Pure numpy: imported by the CPU tests, the GPU tests and tools/mlp_x6_probe.py."""
from __future__ import annotations

import numpy as np

ROUTES = {"bf16x6": 3, "bf16x3": 2, "bf16x1": 1}
# per-multiply relative error of a route: both operands' representation error plus the dropped products
GAMMA = {1: 2 * 2.0 ** -9 + 2.0 ** -18, 2: 2 * 2.0 ** -17 + 2.0 ** -18}


def bf16_rn(x) -> np.ndarray:
    """float32 -> the nearest bf16 value (ties to even), as float32; on the uint32 bit pattern (finite inputs)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def bf16_trunc(x) -> np.ndarray:
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return (b & np.uint32(0xFFFF0000)).view(np.float32)


def pieces(x, n_pieces: int, cut=bf16_rn) -> list:
    """The first ``n_pieces`` bf16 pieces of float32 ``x`` (float32 arrays): p0 = cut(x), p1 = cut(x - p0), ..."""
    r = np.ascontiguousarray(x, dtype=np.float32)
    out = []
    for _ in range(n_pieces):
        p = cut(r)
        out.append(p)
        r = (r - p).astype(np.float32)          # exact in f32
    return out


def piece_product(a: float, b: float, n_pieces: int) -> float:
    """The value a route computes for one product a * b (float64 sum of the kept piece products)."""
    pa, pb = pieces(np.float32([a]), n_pieces), pieces(np.float32([b]), n_pieces)
    return float(sum(np.float64(pa[i][0]) * np.float64(pb[j][0]) for i in range(n_pieces) for j in range(n_pieces) if i + j < n_pieces))


def layer(h, W, n_pieces: int, bias=None, return_abs: bool = False):
    """Pre-activation [N, out] (float32) of one layer: ``h`` [N, k] float32 activations, ``W`` [out, k] float32 weights, ``bias``
    [N, out] float32 or None.  ``return_abs``: also the float64 sum of the products' magnitudes + |bias|, an upper bound of every
    partial sum whatever the order."""
    wp = pieces(W, n_pieces, bf16_trunc if n_pieces == 3 else bf16_rn)
    hp = pieces(h, n_pieces)
    acc = np.zeros((h.shape[0], W.shape[0]), dtype=np.float64)
    mag = np.zeros_like(acc)
    for i in range(n_pieces):
        for j in range(n_pieces - i):
            acc += hp[j].astype(np.float64) @ wp[i].astype(np.float64).T
            if return_abs:
                mag += np.abs(hp[j]).astype(np.float64) @ np.abs(wp[i]).astype(np.float64).T
    if bias is not None:
        acc += bias.astype(np.float64)
        mag += np.abs(bias).astype(np.float64)
    out = acc.astype(np.float32)
    return (out, acc, mag) if return_abs else out


def forward(x, weights, n_pieces: int, bias=None, sigmoid: bool = False, check_exact: bool = False):
    """The network in route ``n_pieces``: ``x`` [N, k0] float32, ``weights`` = [W0 [64, k0], (W1 [64, 64],) Wo [16, 64]], ``bias`` the
    layer-0 row bias already gathered per sample.  ReLU between layers; returns the [N, 16] float32 output (pre-sigmoid unless
    ``sigmoid``).  ``check_exact``: assert that every product is an integer and every partial sum stays below 2^24, i.e. that the
    f32 accumulation of the kernel is exact in any order."""
    h = np.ascontiguousarray(x, dtype=np.float32)
    for li, W in enumerate(weights):
        pre, acc, mag = layer(h, np.asarray(W, dtype=np.float32), n_pieces, bias if li == 0 else None, return_abs=True)
        if check_exact:
            assert np.all(acc == np.rint(acc)) and np.all(mag == np.rint(mag)), f"layer {li}: non-integer sums"
            assert float(mag.max()) < 2.0 ** 24, f"layer {li}: a partial sum can reach {mag.max()} >= 2^24"
        h = np.maximum(pre, np.float32(0)) if li + 1 < len(weights) else pre
    if sigmoid:
        h = (1.0 / (1.0 + np.exp(-h.astype(np.float64)))).astype(np.float32)
    return h


def exact_and_bound(x, weights, n_pieces: int, bias=None, sigmoid: bool = False):
    """(float64 exact network output [N, 16], running forward-error bound E [N, 16]) of route ``n_pieces`` in {1, 2}.  Per layer
        E' = |W| E + gamma |W| (|h| + E) + (k + 2) 2^-24 (|W| (|h| + E) + |bias|)
    ReLU is 1-Lipschitz, the sigmoid 1/4-Lipschitz."""
    gamma = GAMMA[n_pieces]
    h = np.asarray(x, dtype=np.float64)
    E = np.zeros_like(h)
    for li, W in enumerate(weights):
        W64 = np.asarray(W, dtype=np.float64)
        aW = np.abs(W64)
        b = bias.astype(np.float64) if (li == 0 and bias is not None) else 0.0
        spread = (np.abs(h) + E) @ aW.T
        E = E @ aW.T + gamma * spread + (W64.shape[1] + 2) * 2.0 ** -24 * (spread + np.abs(b))
        h = h @ W64.T + b
        if li + 1 < len(weights):
            h = np.maximum(h, 0.0)
    if sigmoid:
        h = 1.0 / (1.0 + np.exp(-h))
        E = E / 4
    return h, E


def random_network(head: bool, n: int, rows: int = 40, seed: int = 31):
    """The random networks of the parity test's scales (weights 0.2 randn, inputs randn, row bias 0.3 randn): returns a dict with
    ``x`` [n, k0], ``weights`` (the head's first layer as the [64, 16] matrix the kernel meets: column 0 unmasked here), ``bias_rows``
    [rows, 64] and ``ridx`` [n] for the head (None for the base)."""
    g = np.random.default_rng(seed + (1 if head else 0))
    f = lambda *s: g.standard_normal(s).astype(np.float32)
    if head:
        return {"x": f(n, 16), "weights": [0.2 * f(64, 16), 0.2 * f(64, 64), 0.2 * f(16, 64)], "bias_rows": 0.3 * f(rows, 64),
                "ridx": (np.arange(n, dtype=np.int64) * rows // n).astype(np.int32)}
    return {"x": f(n, 32), "weights": [0.2 * f(64, 32), 0.2 * f(16, 64)], "bias_rows": None, "ridx": None}
