"""The reduced-piece inference forwards of the two production MLP shapes (lse_mlp_desc.arith = LSE_MLP_ARITH_BF16X3 / _BF16X1;
csrc/mlp_x6.h with NP = 2 / 1) through ``lse_mlp_fwd`` and ``lse_mlp_fwd_pair``, against the numpy twin tests/mlp_pieces_ref.py.

1. Integer networks whose every partial sum is an integer below 2^24 (asserted on the twin's float64 sums): accumulation order
   cannot matter, so each route equals ITS twin bit for bit -- which pins "exactly the products with i + j < NP" and the k-slot
   packing of every layer.
2. Random networks against float64: every element within the twin's running bound E, the kernel's rms error within a factor two
   of the twin's (same rounding model; f32 against float64 accumulation is 2^-10 of the bf16x1 error and under a tenth of the
   bf16x3 error), and a reduced route differs from bf16x6.
3. Edges: tile boundaries, a device-side count, no samples, both row-bias forms, two calls.
4. The pair against two calls, and every refusal with its outputs untouched."""
import ctypes
import dataclasses
import functools

import numpy as np
import pytest
import torch

from tests import mlp_pieces_ref as twin

pytestmark = pytest.mark.gpu

ROUTES = ("bf16x6", "bf16x3", "bf16x1")
REDUCED = ("bf16x3", "bf16x1")
KINDS = ("head", "base_lm", "base_rm")
SENTINEL = -12345.0
SCALE = 0.7
UNSUPPORTED = -3
EDGE_N = (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 8 * 32 * 3 + 1)


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _meta(kind, route, act=None):
    from lsenerf_amd import _lib, ops
    arith = ops.MLP_ARITH_ROUTES[route]
    if kind == "head":       # the head's first-layer view: h[N,16] against columns 15..30 of the [64 x 64] input matrix, column 0 masked
        return ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID if act == "sigmoid" else _lib.LSE_ACT_NONE, _lib.LSE_IN_ROWMAJOR,
                           w0_ld=64, w0_col=15, w0_mask_col0=1, arith=arith)
    return ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_LEVELMAJOR if kind == "base_lm" else _lib.LSE_IN_ROWMAJOR, arith=arith)


def _pack_params(kind, weights):
    """Kernel parameter vector of twin weights.  Head: W0 [64,16] sits in columns 15..30 of a [64,64] matrix full of junk, and the
    junk under the masked column 15 must never be read as a weight."""
    ws = [np.asarray(w, dtype=np.float32) for w in weights]
    if kind == "head":
        full = np.full((64, 64), 77.0, dtype=np.float32)
        full[:, 15:31] = ws[0]
        full[:, 15] = 1234.5
        ws = [full] + ws[1:]
    return torch.from_numpy(np.concatenate([w.reshape(-1) for w in ws])).cuda()


def _twin_weights(kind, weights):
    ws = [np.array(w, dtype=np.float32) for w in weights]
    if kind == "head":
        ws[0][:, 0] = 0.0          # w0_mask_col0
    return ws


def _dev_in(kind, x):
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    if kind == "base_lm":
        t = t.view(x.shape[0], 16, 2).permute(1, 0, 2)
    return t.contiguous().cuda()


def _fwd(kind, route, params, xin, n, *, bias=None, idx=None, out_cols=16, act=None, sigma=False, sel=None, n_dev=None, out=None,
         sig_out=None):
    from lsenerf_amd import _lib, ops
    desc = _meta(kind, route, act).desc()
    out = torch.empty(n, out_cols, device="cuda") if out is None else out
    if sigma and sig_out is None:
        sig_out = torch.empty(n, device="cuda")
    _lib.call("lse_mlp_fwd", ctypes.byref(desc), _P(params), _P(xin), _P(bias), _P(idx), _P(out), out_cols, None, 3, _P(sig_out),
              _P(sel), SCALE if sigma else 0.0, n, _P(n_dev), ops._stream())
    return (out, sig_out) if sigma else out


# ---------------------------------------------------------------------------------------------------- 1. exact networks
BIG_IN = (257.0, 4097.0, 385.0, -259.0, 3.0)        # 9 .. 13 significant bits
BIG_W0 = (257.0, 259.0, 129.0, -257.0)
BIG_W = (257.0, 4097.0, -385.0)


@functools.lru_cache(maxsize=None)
def _exact_net(kind, big, n=97, rows=5):
    """Integer network.  ``big`` False: inputs in [-3, 3], weights in {-1, 0, 1}, at most 4 non-zeros per row -- one piece holds
    every value.  ``big``: values of 9 .. 16 significant bits on sparse paths.  Rows of a layer come in three classes, r mod 4 = 0 / 3
    "small" (weights +-1 on the previous layer's small columns only), 1 "wide" (the same columns, one weight of BIG_W), 2 "large" (in the
    first layer any column, weights +-1 and one weight of BIG_W0 on a column that carries BIG_IN values; behind it at most 3 weights
    +-1 on the previous layer's large rows): large values never meet large weights, so every partial sum stays below 2^24."""
    g = np.random.default_rng(5 + 2 * KINDS.index(kind) + int(big))
    k0 = 16 if kind == "head" else 32
    x = g.integers(-3, 4, size=(n, k0)).astype(np.float32)
    big_cols = np.arange(1, k0, 4)
    if big:
        x[:, big_cols] = np.asarray(BIG_IN, dtype=np.float32)[g.integers(0, len(BIG_IN), size=(n, len(big_cols)))]
    dims = [(64, k0)] + ([(64, 64)] if kind == "head" else []) + [(16, 64)]
    small_prev = np.setdiff1d(np.arange(1 if kind == "head" else 0, k0), big_cols if big else [])
    weights = []
    for li, (m, k) in enumerate(dims):
        W = np.zeros((m, k), dtype=np.float32)
        for r in range(m):
            cls = (0, 1, 2, 0)[r % 4] if big else 2
            pool = small_prev if cls < 2 else (np.arange(2, k, 4) if (big and li > 0) else np.arange(k))
            nnz = int(g.integers(1, (4 if (li == 0 or not big) else 3) + 1))
            cols = g.choice(pool, size=min(nnz, len(pool)), replace=False)
            # (multi-piece set: mostly +1, so that the large values survive the ReLUs down to the output)
            W[r, cols] = g.choice([-1.0, 1.0], size=len(cols), p=[0.2, 0.8] if big else [0.5, 0.5])
            if big and cls == 1:
                W[r, cols[0]] = BIG_W[int(g.integers(0, len(BIG_W)))]
            if big and cls == 2 and li == 0:
                W[r, big_cols[int(g.integers(0, len(big_cols)))]] = BIG_W0[int(g.integers(0, len(BIG_W0)))]
        weights.append(W)
        small_prev = np.asarray([r for r in range(m) if (not big) or r % 4 in (0, 3)])
    bias_rows = g.integers(-2, 3, size=(rows, 64)).astype(np.float32) if kind == "head" else None
    ridx = (np.arange(n) * rows // n).astype(np.int32) if kind == "head" else None
    return dict(x=x, weights=weights, bias_rows=bias_rows, ridx=ridx, n=n)


def _run_exact(kind, route, net):
    params = _pack_params(kind, net["weights"])
    bias = None if net["bias_rows"] is None else torch.from_numpy(net["bias_rows"]).cuda()
    idx = None if net["ridx"] is None else torch.from_numpy(net["ridx"]).cuda()
    return _fwd(kind, route, params, _dev_in(kind, net["x"]), net["n"], bias=bias, idx=idx).cpu().numpy()


@pytest.mark.parametrize("kind", KINDS)
def test_one_piece_integer_network_is_exact_in_every_route(kind):
    net = _exact_net(kind, False)
    ws = _twin_weights(kind, net["weights"])
    bias = None if net["bias_rows"] is None else net["bias_rows"][net["ridx"]]
    ref = net["x"].astype(np.float64)
    for li, W in enumerate(ws):          # the integer network itself
        ref = ref @ W.astype(np.float64).T + (bias if (li == 0 and bias is not None) else 0.0)
        assert float(np.abs(ref).max()) <= 256
        if li + 1 < len(ws):
            ref = np.maximum(ref, 0.0)
    assert float(np.abs(ref).max()) > 8          # not a network of zeros
    for route in ROUTES:
        t = twin.forward(net["x"], ws, twin.ROUTES[route], bias, check_exact=True)
        assert np.array_equal(t.astype(np.float64), ref), route
        got = _run_exact(kind, route, net)
        assert np.array_equal(got.view(np.uint32), t.view(np.uint32)), (kind, route, float(np.abs(got - t).max()))


@pytest.mark.parametrize("kind", KINDS)
def test_each_route_equals_its_own_twin_on_multi_piece_integers(kind):
    net = _exact_net(kind, True)
    ws = _twin_weights(kind, net["weights"])
    bias = None if net["bias_rows"] is None else net["bias_rows"][net["ridx"]]
    twins = {route: twin.forward(net["x"], ws, twin.ROUTES[route], bias, check_exact=True) for route in ROUTES}
    assert not np.array_equal(twins["bf16x1"], twins["bf16x3"]) and not np.array_equal(twins["bf16x3"], twins["bf16x6"])
    for route in ROUTES:
        got = _run_exact(kind, route, net)
        bad = int((got.view(np.uint32) != twins[route].view(np.uint32)).sum())
        print(f"{kind} {route}: {bad} of {got.size} elements differ from the twin, max |diff| {np.abs(got - twins[route]).max()}")
        assert bad == 0, (kind, route)


# ---------------------------------------------------------------------------------------------------- 2. random networks
N_RANDOM = 4099


@functools.lru_cache(maxsize=None)
def _random_case(kind):
    """One random network per shape with everything the tests of it share, computed once: device inputs, the float64 network."""
    head = kind == "head"
    net = twin.random_network(head, N_RANDOM)
    ws = _twin_weights(kind, net["weights"])
    bias = net["bias_rows"][net["ridx"]] if head else None
    c = dict(net=net, ws=ws, bias=bias, params=_pack_params(kind, net["weights"]), xin=_dev_in(kind, net["x"]),
             bias_dev=None if not head else torch.from_numpy(net["bias_rows"]).cuda(),
             idx_dev=None if not head else torch.from_numpy(net["ridx"]).cuda())
    g = torch.Generator().manual_seed(3)
    c["sel"] = (torch.rand(N_RANDOM, generator=g) < 0.7).to(torch.uint8).cuda()
    return c


@pytest.mark.parametrize("route", REDUCED)
@pytest.mark.parametrize("kind,out_cols", [("head", 4), ("head", 16), ("base_lm", 16), ("base_rm", 16)])
def test_random_network_within_the_bound(kind, out_cols, route):
    c = _random_case(kind)
    head, NP = kind == "head", twin.ROUTES[route]
    ref, E = twin.exact_and_bound(c["net"]["x"], c["ws"], NP, c["bias"], sigmoid=head)
    tw = twin.forward(c["net"]["x"], c["ws"], NP, c["bias"], sigmoid=head)
    kw = dict(bias=c["bias_dev"], idx=c["idx_dev"], out_cols=out_cols, act="sigmoid" if head else None)
    if head:
        out = _fwd(kind, route, c["params"], c["xin"], N_RANDOM, **kw)
        out6 = _fwd(kind, "bf16x6", c["params"], c["xin"], N_RANDOM, **kw)
    else:       # the density head on the route's own h: sigma = scale * exp(h[:, 0]) where the selector is set, 0 elsewhere
        out, sigma = _fwd(kind, route, c["params"], c["xin"], N_RANDOM, sigma=True, sel=c["sel"], **kw)
        out6, sigma6 = _fwd(kind, "bf16x6", c["params"], c["xin"], N_RANDOM, sigma=True, sel=c["sel"], **kw)
        on = c["sel"] != 0
        assert bool((sigma[~on] == 0).all()) and bool((sigma[on] > 0).all())
        want = SCALE * torch.exp(out[:, 0].double())
        assert float(((sigma.double() - want).abs() / want)[on].max()) < 4 * 2.0 ** -24      # expf and one multiply, in f32
        assert not torch.equal(sigma, sigma6)
    assert not torch.equal(out, out6)                      # (refused with "bad arith" where the routes do not exist)
    got = out.cpu().numpy().astype(np.float64)
    cols = slice(0, out_cols)
    err, terr = got - ref[:, cols], tw[:, cols].astype(np.float64) - ref[:, cols]
    ratio = float((np.abs(err) / E[:, cols]).max())
    rms, trms = float(np.sqrt((err ** 2).mean())), float(np.sqrt((terr ** 2).mean()))
    print(f"{kind} oc={out_cols} {route}: worst |err|/E {ratio:.3f}, rms kernel {rms:.3e} twin {trms:.3e}, "
          f"max err / scale {np.abs(err).max() / np.abs(ref).max():.2e}")
    assert ratio <= 1.0
    assert 0.5 * trms <= rms <= 2.0 * trms


# ---------------------------------------------------------------------------------------------------- 3. edges
@functools.lru_cache(maxsize=None)
def _edge_ref(kind, route, biased):
    """The longest edge case, run once: shorter runs must reproduce its leading rows (a sample's output depends on nothing else)."""
    c = _random_case(kind)
    n = max(EDGE_N)
    kw = {}
    if biased == "idx":
        kw = dict(bias=c["bias_dev"] if kind == "head" else _edge_bias_rows(), idx=_edge_idx(n))
    elif biased == "rows":
        kw = dict(bias=_edge_bias_per_sample(n))
    out, sigma = _fwd(kind, route, c["params"], _edge_in(kind, n), n, sigma=True, sel=c["sel"][:n].contiguous(), **kw)
    return out, sigma


@functools.lru_cache(maxsize=None)
def _edge_bias_rows():
    return (torch.randn(40, 64, generator=torch.Generator().manual_seed(8)) * 0.3).cuda()


@functools.lru_cache(maxsize=None)
def _edge_idx(n):
    return (torch.arange(n) * 40 // max(EDGE_N)).int().cuda()


@functools.lru_cache(maxsize=None)
def _edge_bias_per_sample(n):
    return (torch.randn(max(EDGE_N), 64, generator=torch.Generator().manual_seed(9)) * 0.3)[:n].contiguous().cuda()


def _edge_in(kind, n):
    return _dev_in(kind, _random_case(kind)["net"]["x"][:n])


@pytest.mark.parametrize("route", REDUCED)
@pytest.mark.parametrize("kind", KINDS)
def test_tile_edges_counts_and_row_bias_forms(kind, route):
    c = _random_case(kind)
    for biased in ("idx", "rows", None):
        ref_out, ref_sigma = _edge_ref(kind, route, biased)
        for n in EDGE_N:
            kw = {}
            if biased == "idx":
                kw = dict(bias=c["bias_dev"] if kind == "head" else _edge_bias_rows(), idx=_edge_idx(max(EDGE_N))[:n].contiguous())
            elif biased == "rows":
                kw = dict(bias=_edge_bias_per_sample(n))
            sel = c["sel"][:n].contiguous()
            out, sigma = _fwd(kind, route, c["params"], _edge_in(kind, n), n, sigma=True, sel=sel, **kw)
            assert torch.equal(out, ref_out[:n]) and torch.equal(sigma, ref_sigma[:n]), (kind, route, biased, n)
    # two calls give the same bits
    n = max(EDGE_N)
    again = _fwd(kind, route, c["params"], _edge_in(kind, n), n, sigma=True, sel=c["sel"][:n].contiguous())
    assert torch.equal(again[0], _edge_ref(kind, route, None)[0]) and torch.equal(again[1], _edge_ref(kind, route, None)[1])
    # a device-side count below n: rows at or beyond it stay untouched
    xin = _edge_in(kind, n)
    for m in (0, 1, 33, 500):
        out = torch.full((n, 16), SENTINEL, device="cuda")
        sig = torch.full((n,), SENTINEL, device="cuda")
        n_dev = torch.tensor([m], dtype=torch.int64, device="cuda")
        _fwd(kind, route, c["params"], xin, n, sigma=True, sel=c["sel"][:n].contiguous(), n_dev=n_dev, out=out, sig_out=sig)
        assert torch.equal(out[:m], again[0][:m]) and torch.equal(sig[:m], again[1][:m]), (kind, route, m)
        assert bool((out[m:] == SENTINEL).all()) and bool((sig[m:] == SENTINEL).all()), (kind, route, m)
    # no samples: no launch, no error
    from lsenerf_amd import _lib, ops
    desc = _meta(kind, route).desc()
    out = torch.full((n, 16), SENTINEL, device="cuda")
    _lib.call("lse_mlp_fwd", ctypes.byref(desc), _P(c["params"]), _P(xin), None, None, _P(out), 16, None, 3, None, None, 0.0, 0, None,
              ops._stream())
    assert bool((out == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- 4. the pair
def _pair(route_b, route_h, bp, y, sel, hp, bias, idx, h, sigma, out, out_cols, n, kind_b="base_lm", n_dev=None):
    from lsenerf_amd import _lib, ops
    bd, hd = _meta(kind_b, route_b).desc(), _meta("head", route_h, "sigmoid").desc()
    return _lib.load().lse_mlp_fwd_pair(ctypes.byref(bd), _P(bp), _P(y), _P(sel), SCALE, ctypes.byref(hd), _P(hp), _P(bias), _P(idx),
                                        _P(h), _P(sigma), _P(out), out_cols, n, _P(n_dev), ops._stream())


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind_b", ["base_lm", "base_rm"])
def test_pair_is_bitwise_two_calls(kind_b, route):
    b, hd = _random_case(kind_b), _random_case("head")
    for n, out_cols in ((N_RANDOM, 4), (769, 16), (33, 4), (1, 4)):
        y = _dev_in(kind_b, b["net"]["x"][:n])
        sel = b["sel"][:n].contiguous()
        idx = (torch.arange(n) * 40 // n).int().cuda()
        h1, s1 = _fwd(kind_b, route, b["params"], y, n, sigma=True, sel=sel)
        o1 = _fwd("head", route, hd["params"], h1, n, bias=hd["bias_dev"], idx=idx, out_cols=out_cols, act="sigmoid")
        h = torch.full((n, 16), SENTINEL, device="cuda")
        sigma = torch.full((n,), SENTINEL, device="cuda")
        out = torch.full((n, out_cols), SENTINEL, device="cuda")
        assert _pair(route, route, b["params"], y, sel, hd["params"], hd["bias_dev"], idx, h, sigma, out, out_cols, n, kind_b) == 0
        assert torch.equal(h, h1) and torch.equal(sigma, s1) and torch.equal(out, o1), (kind_b, route, n)
    # device-side count
    n, m = 769, 100
    y = _dev_in(kind_b, b["net"]["x"][:n])
    idx = (torch.arange(n) * 40 // n).int().cuda()
    h = torch.full((n, 16), SENTINEL, device="cuda")
    sigma = torch.full((n,), SENTINEL, device="cuda")
    out = torch.full((n, 4), SENTINEL, device="cuda")
    n_dev = torch.tensor([m], dtype=torch.int64, device="cuda")
    h1, s1 = _fwd(kind_b, route, b["params"], y, n, sigma=True, sel=b["sel"][:n].contiguous())
    o1 = _fwd("head", route, hd["params"], h1, n, bias=hd["bias_dev"], idx=idx, out_cols=4, act="sigmoid")
    assert _pair(route, route, b["params"], y, b["sel"][:n].contiguous(), hd["params"], hd["bias_dev"], idx, h, sigma, out, 4, n, kind_b,
                 n_dev) == 0
    assert torch.equal(h[:m], h1[:m]) and torch.equal(sigma[:m], s1[:m]) and torch.equal(out[:m], o1[:m])
    assert bool((h[m:] == SENTINEL).all()) and bool((sigma[m:] == SENTINEL).all()) and bool((out[m:] == SENTINEL).all())


@pytest.mark.parametrize("route", REDUCED)
def test_refusals_launch_nothing(route):
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    b, hd = _random_case("base_lm"), _random_case("head")
    n = 257
    other = "bf16x1" if route == "bf16x3" else "bf16x3"
    y = _dev_in("base_lm", b["net"]["x"][:n])
    idx = (torch.arange(n) * 40 // n).int().cuda()
    fresh = lambda *s: torch.full(s, SENTINEL, device="cuda")
    untouched = lambda *ts: all(bool((t == SENTINEL).all()) for t in ts)
    # mixed routes in a pair
    for rb, rh in ((route, "bf16x6"), ("bf16x6", route), (route, other)):
        h, sigma, out = fresh(n, 16), fresh(n), fresh(n, 4)
        assert _pair(rb, rh, b["params"], y, None, hd["params"], hd["bias_dev"], idx, h, sigma, out, 4, n) == UNSUPPORTED, (rb, rh)
        assert b"lse_mlp_fwd_pair" in lib.lse_last_error()
        torch.cuda.synchronize()
        assert untouched(h, sigma, out), (rb, rh)
    # a saved-activation request, another shape
    act = fresh(2, 272, 64)
    for what, meta, tiled in (("act_tiled 0", _meta("head", route), 0), ("act_tiled 1", _meta("base_lm", route), 1),
                              ("act_tiled 2", _meta("head", route), 2),
                              ("width 32", dataclasses.replace(_meta("base_lm", route), width=32), 3),
                              ("64 inputs", ops.MlpMeta(64, 64, 2, arith=ops.MLP_ARITH_ROUTES[route]), 3)):
        out = fresh(n, 16)
        d = meta.desc()
        x = torch.zeros(n * 64, device="cuda")
        rc = lib.lse_mlp_fwd(ctypes.byref(d), _P(hd["params"]), _P(x), None, None, _P(out), 16, _P(act) if tiled < 3 else None, tiled,
                             None, None, 0.0, n, None, ops._stream())
        assert rc == UNSUPPORTED, what
        assert b"reduced-piece" in lib.lse_last_error(), what
        torch.cuda.synchronize()
        assert untouched(out, act), what
    # the backward entry points
    head, x = _meta("head", route), torch.zeros(n, 16, device="cuda")
    d = head.desc()
    d_in, d_par, d_out, outp = fresh(n, 16), fresh(head.n_params), torch.zeros(n, 4, device="cuda"), torch.zeros(n, 4, device="cuda")
    rc = lib.lse_mlp_bwd(ctypes.byref(d), _P(hd["params"]), _P(x), None, 3, _P(outp), 4, _P(d_out), None, None, 0.0, None, None, None,
                         _P(d_in), _P(d_par), None, None, None, n, None, ops._stream())
    assert rc == UNSUPPORTED and b"lse_mlp_bwd" in lib.lse_last_error()
    rc = lib.lse_mlp_bwd_input(ctypes.byref(d), _P(hd["params"]), _P(x), _P(outp), 4, _P(d_out), None, None, 0.0, _P(d_in), None, None,
                               None, n, None, ops._stream())
    assert rc == UNSUPPORTED and b"lse_mlp_bwd_input" in lib.lse_last_error()
    plain = dataclasses.replace(head, w0_ld=0, w0_col=0, w0_mask_col0=0).desc()
    a2 = torch.zeros(2, n, 64, device="cuda")
    rc = lib.lse_mlp_wgrad(ctypes.byref(plain), _P(x), _P(a2), _P(a2), _P(torch.zeros(n, 16, device="cuda")), _P(d_par), n, ops._stream())
    assert rc == UNSUPPORTED and b"lse_mlp_wgrad" in lib.lse_last_error()
    torch.cuda.synchronize()
    assert untouched(d_in, d_par)
    # ops: a call that would need a backward is refused before any launch
    p = hd["params"].clone().requires_grad_()
    with pytest.raises(ValueError, match="forward only"):
        ops.fused_mlp(p, x, head, n, hd["bias_dev"], idx, out_cols=4)
    with torch.no_grad():
        o = ops.fused_mlp(p, x, head, n, hd["bias_dev"], idx, out_cols=4)
    assert o.shape == (n, 4) and not o.requires_grad
