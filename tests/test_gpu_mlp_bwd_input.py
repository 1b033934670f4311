"""``lse_mlp_bwd_input`` (csrc/mlp_x6.h: ``mlp_bwd_input_kernel``): the data gradients of a fused MLP with frozen parameters --
d(input) and d(row_bias) alone -- against ``lse_mlp_bwd`` (act_tiled = 3, weight gradients into a scratch), which issues the same
matrix-core products in the same order, and against a float64 restatement of the network written here.

d_in must carry the bits of ``lse_mlp_bwd``; d_row_bias sums the same f32 terms in another order, so ``lse_mlp_bwd``'s own error
against float64 is its yardstick: e_new <= max(2 e_old, 1e-6) and e_new < TOL_GRAD."""
import ctypes
import functools

import pytest
import torch

from tests.util import TOL_GRAD, nmax_err

pytestmark = pytest.mark.gpu

SCALE = 0.7                                  # density scale
SEGMENTS = (1, 5, 16, 17, 32, 100, 2048)     # samples per bias row, cycled: tiles that straddle rows, a row over many tiles / waves
SENTINEL = -12345.0
BAND = 1e-5                                  # |pre-activation| below which a float32 and a float64 ReLU gate may disagree
KINDS = ("head4", "head16", "base_lm", "base_rm", "base_sigma", "base_bias")      # base_bias: level-major base with a per-row bias
LEVELMAJOR = ("base_lm", "base_sigma", "base_bias")
# the edges of the 16-sample column tiles and 32-sample wave tiles; 4113: many workgroups, ragged last tile; 600017: the launch
# keeps 768 workgroups x 4 waves = 3072 waves in flight, so 18751 tiles make every wave walk 7 (look-ahead, running row sum)
SIZES = (1, 15, 16, 17, 31, 32, 33, 64, 4113, 600017)
# d_row_bias of two correct launches whose waves cut the samples differently: the same <= 2048 f32 terms per entry in another
# order.  A reordered f32 sum of N like-sized terms moves by about sqrt(N) * 2^-24 of its partial sums (1e-6 of the largest entry
# at N = 2048, what the issue's floor for the yardstick allows); ten times that separates an order effect from a lost term, which
# costs 1 / N >= 5e-4.
TOL_ORDER = 1e-5


def _P(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _meta(kind, **kw):
    from lsenerf_amd import _lib, ops
    if kind.startswith("head"):
        return ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR, w0_ld=64, w0_col=15, w0_mask_col0=1, **kw)
    return ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_ROWMAJOR if kind == "base_rm" else _lib.LSE_IN_LEVELMAJOR, **kw)


@functools.lru_cache(maxsize=None)
def _weights():
    g = torch.Generator().manual_seed(11)
    u = lambda m, fan: ((torch.rand(m, generator=g) * 2 - 1) * (6.0 / fan) ** 0.5).cuda()
    base = torch.cat([u(64 * 32, 96), u(16 * 64, 80)])
    head = torch.cat([u(64 * 64, 128), u(64 * 64, 128), u(16 * 64, 80)])
    return base, head


def _rows(n):
    """Sorted row indices of n samples in segments of SEGMENTS (cycled); only the ODD rows are used, the even ones stay untouched."""
    lens, total = [], 0
    while total < n:
        lens.append(min(SEGMENTS[len(lens) % len(SEGMENTS)], n - total))
        total += lens[-1]
    cnt = torch.tensor(lens, dtype=torch.int64)
    idx = torch.repeat_interleave(2 * torch.arange(len(lens), dtype=torch.int32) + 1, cnt).cuda()
    return idx, 2 * len(lens) + 1


def _net64(kind, x_rows, bias_rows):
    """The network in float64 from row-major inputs [n, n_in] (and the gathered bias): (output [n, 16], smallest |pre-activation|)."""
    bp, hp = _weights()
    if kind.startswith("head"):
        w = hp.double()
        w0 = w[:4096].view(64, 64)[:, 15:31].clone()
        w0[:, 0] = 0.0                                          # w0_mask_col0
        pre0 = x_rows @ w0.T + bias_rows
        pre1 = torch.relu(pre0) @ w[4096:8192].view(64, 64).T
        out = torch.relu(pre1) @ w[8192:].view(16, 64).T
        return out, torch.minimum(pre0.abs().amin(1), pre1.abs().amin(1))
    w = bp.double()
    pre0 = x_rows @ w[:2048].view(64, 32).T + (0.0 if bias_rows is None else bias_rows)
    return torch.relu(pre0) @ w[2048:].view(16, 64).T, pre0.abs().amin(1)


def _to_rows(kind, x):
    return x.permute(1, 0, 2).reshape(x.shape[1], 32) if kind in LEVELMAJOR else x


@functools.lru_cache(maxsize=None)
def _case(kind, n):
    """Inputs of one (shape, sample count), the forward's output and the gradients of ``lse_mlp_bwd`` (act_tiled = 3) on them;
    computed once, never modified."""
    from lsenerf_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1000 + n + 7 * KINDS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g, device="cuda")
    meta, head = _meta(kind), kind.startswith("head")
    biased = head or kind == "base_bias"
    params = _weights()[1 if head else 0]
    c = dict(kind=kind, n=n, meta=meta, params=params, oc=4 if kind == "head4" else 16, idx=None, row_bias=None, d_sigma=None, sel=None,
             scale=0.0)
    c["x"] = rn(n, 16) * 0.5 if head else (rn(16, n, 2) * 0.5 if kind in LEVELMAJOR else rn(n, 32) * 0.5)
    if biased:
        c["idx"], rows = _rows(n)
        c["row_bias"] = rn(rows, 64) * 0.3
    with torch.no_grad():
        out = ops.fused_mlp(params, c["x"], meta, n, c["row_bias"], c["idx"], None, out_cols=c["oc"])
        bias_rows = c["row_bias"][c["idx"].long()].double() if biased else None
        _, margin = _net64(kind, _to_rows(kind, c["x"]).double(), bias_rows)
    c["d_out"] = rn(n, c["oc"])
    if kind == "base_sigma":      # density head: a selector with zeros, and logits on both sides of the +-15 clamp
        c["d_sigma"], c["sel"], c["scale"] = rn(n), (torch.rand(n, generator=g, device="cuda") < 0.7).to(torch.uint8), SCALE
        out = out.clone()
        out[:, 0] = torch.linspace(-20.0, 20.0, n, device="cuda")[torch.randperm(n, generator=g, device="cuda")] if n > 1 else 17.0
        assert n < 64 or (float(out[:, 0].max()) > 15 and float(out[:, 0].min()) < -15 and int(c["sel"].sum()) < n)
    # a sample with a pre-activation inside BAND receives no upstream gradient: a float64 gate may then differ from the float32
    # one without consequence (a handful of samples in a million; every kernel under test sees the same inputs)
    near = margin < BAND
    c["d_out"][near] = 0.0
    if c["d_sigma"] is not None:
        c["d_sigma"][near] = 0.0
    c["out"], c["near"] = out, int(near.sum())
    c["old"] = _old(c)
    return c


def _outputs(c, want_d_in=True, want_bias=True):
    d_in = torch.full_like(c["x"], SENTINEL) if want_d_in else None
    d_rb = torch.zeros_like(c["row_bias"]) if (want_bias and c["row_bias"] is not None) else None
    return d_in, d_rb


def _old(c, n=None, n_dev=None):
    """(d_in, d_row_bias) of lse_mlp_bwd, act_tiled = 3, weight gradients into a scratch."""
    from lsenerf_amd import ops
    d_in, d_rb = _outputs(c)
    scratch = torch.zeros_like(c["params"])
    desc = c["meta"].desc()
    ops._call_n("lse_mlp_bwd", n_dev, ctypes.byref(desc), _P(c["params"]), _P(c["x"]), None, 3, _P(c["out"]), c["oc"], _P(c["d_out"]),
                _P(c["d_sigma"]), _P(c["sel"]), c["scale"], None, None, None, _P(d_in), _P(scratch), _P(c["row_bias"]), _P(c["idx"]),
                _P(d_rb), c["n"] if n is None else n, ops._stream())
    return d_in, d_rb


def _new(c, n=None, n_dev=None, want_d_in=True, want_bias=True):
    from lsenerf_amd import ops
    d_in, d_rb = _outputs(c, want_d_in, want_bias)
    ops.mlp_bwd_input(c["params"], c["x"], c["meta"], c["n"] if n is None else n, c["out"], c["oc"], c["d_out"], c["d_sigma"], c["sel"],
                      c["scale"], d_in, c["row_bias"], c["idx"], d_rb, n_dev)
    return d_in, d_rb


def _bits(t):
    return t.view(torch.int32)


@functools.lru_cache(maxsize=None)
def _ref64(kind, n):
    """(d_in, d_row_bias) in float64: autograd through ``_net64`` with the gathered bias, the upstream gradient formed from the
    forward's float32 ``out`` as the kernels form it."""
    c = _case(kind, n)
    head = kind.startswith("head")
    x = c["x"].double().requires_grad_(True)
    rb = c["row_bias"].double().requires_grad_(True) if c["row_bias"] is not None else None
    out, _ = _net64(kind, _to_rows(kind, x), rb[c["idx"].long()] if rb is not None else None)
    o32 = c["out"].double()
    g = torch.zeros(n, 16, dtype=torch.float64, device="cuda")
    if head:
        g[:, : c["oc"]] = c["d_out"].double() * o32 * (1.0 - o32)
    else:
        g += c["d_out"].double()
        if c["d_sigma"] is not None:
            g[:, 0] += torch.where(c["sel"] != 0, c["d_sigma"].double(), 0.0) * SCALE * torch.exp(o32[:, 0].clamp(-15.0, 15.0))
    (out * g).sum().backward()
    return x.grad, (rb.grad if rb is not None else None)


# ---------------------------------------------------------------------------------------------------- 1, 2: bits of d_in, sizes
@pytest.mark.parametrize("n", SIZES)
def test_d_in_carries_the_bits_of_lse_mlp_bwd(n):
    """Every shape, layout and preamble branch at every size: d_in bit for bit (nothing left unwritten), d_row_bias to the order bar."""
    for kind in KINDS:
        c = _case(kind, n)
        d_in, d_rb = _new(c)
        o_in, o_rb = c["old"]
        assert not bool((o_in == SENTINEL).any()) and float(o_in.abs().max()) > 0, (kind, n)
        assert torch.equal(_bits(d_in), _bits(o_in)), (kind, n, int((_bits(d_in) != _bits(o_in)).sum()))
        if d_rb is not None:
            e = nmax_err(d_rb, o_rb, 1e-12)
            assert float(o_rb.abs().max()) > 0 and e < TOL_ORDER, (kind, n, e)
            assert float(d_rb[0::2].abs().max()) == 0.0, (kind, n)                     # rows no sample references


# ---------------------------------------------------------------------------------------------------- 3, 4, 5: float64
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_against_float64(kind):
    """n = 4113 over the segment pattern (1, 5, 16, 17, 32, 100, 2048, ...): d_in under TOL_GRAD; d_row_bias no worse than twice
    lse_mlp_bwd's own error (floor 1e-6) and under TOL_GRAD; unreferenced rows exactly zero.
    Measured (MI355X): see DESIGN.md section 4, "The frozen-field step"."""
    c = _case(kind, 4113)
    r_in, r_rb = _ref64(kind, 4113)
    d_in, d_rb = _new(c)
    e_in = nmax_err(d_in, r_in, 1e-12)
    print("MLP_BWD_INPUT", kind, "samples inside the gate band:", c["near"], "d_in vs float64:", e_in)
    assert e_in < TOL_GRAD, (kind, e_in)
    if d_rb is None:
        return
    e_new, e_old = nmax_err(d_rb, r_rb, 1e-12), nmax_err(c["old"][1], r_rb, 1e-12)
    print("MLP_BWD_INPUT", kind, "d_row_bias vs float64: new", e_new, "lse_mlp_bwd", e_old)
    assert e_new <= max(2.0 * e_old, 1e-6) and e_new < TOL_GRAD, (kind, e_new, e_old)
    assert float(d_rb[0::2].abs().max()) == 0.0 and float(r_rb[0::2].abs().max()) == 0.0
    assert float(d_rb[1::2].abs().amax(1).min()) > 0                                   # every referenced row received its sum


# ---------------------------------------------------------------------------------------------------- 6: device-side count
@pytest.mark.parametrize("short", [0, 1, 33, 4112])
def test_device_side_count(short):
    """Capacity 4113 with n_dev below it: d_in of the prefix as in the full call, the rest keeps its sentinel; d_row_bias is that
    of a call with n = n_dev (other waves, other order)."""
    n_dev = torch.tensor([short], dtype=torch.int64, device="cuda")
    for kind in ("head4", "base_lm", "base_rm"):
        c = _case(kind, 4113)
        d_in, d_rb = _new(c, n_dev=n_dev)
        rows, full = _to_rows(kind, d_in), _to_rows(kind, c["old"][0])
        assert torch.equal(_bits(rows[:short]), _bits(full[:short])), (kind, short)
        assert bool((rows[short:] == SENTINEL).all()), (kind, short)
        if d_rb is not None:
            if short == 0:
                assert float(d_rb.abs().max()) == 0.0
            else:
                _, s_rb = _new(c, n=short)
                assert float(s_rb.abs().max()) > 0 and nmax_err(d_rb, s_rb, 1e-12) < TOL_ORDER, (kind, short)
                last = int(c["idx"][short - 1])
                assert float(d_rb[last + 1:].abs().max()) == 0.0                       # no row beyond the count was touched


# ---------------------------------------------------------------------------------------------------- 7: null outputs
def test_null_outputs():
    """Embedding-only phase: no d_in, d_row_bias within the yardstick of item 4.  The base: no bias at all, d_in alone."""
    c = _case("head4", 4113)
    _, r_rb = _ref64("head4", 4113)
    d_in, d_rb = _new(c, want_d_in=False)
    assert d_in is None
    e_new, e_old = nmax_err(d_rb, r_rb, 1e-12), nmax_err(c["old"][1], r_rb, 1e-12)
    print("MLP_BWD_INPUT d_row_bias alone vs float64: new", e_new, "lse_mlp_bwd", e_old)
    assert e_new <= max(2.0 * e_old, 1e-6) and e_new < TOL_GRAD
    d_in, d_rb = _new(c, want_bias=False)                                                # the head without a bias gradient
    assert d_rb is None and torch.equal(_bits(d_in), _bits(c["old"][0]))
    for kind in ("base_lm", "base_rm", "base_sigma"):
        b = _case(kind, 4113)
        d_in, d_rb = _new(b)
        assert d_rb is None and b["row_bias"] is None and torch.equal(_bits(d_in), _bits(b["old"][0]))


# ---------------------------------------------------------------------------------------------------- 8: repeatability
@pytest.mark.parametrize("kind", ["head4", "base_sigma"])
def test_two_calls_give_the_same_bits(kind):
    c = _case(kind, 4113)
    a, _ = _new(c)
    b, _ = _new(c)
    assert torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------- 9: refusals
def test_refusals_launch_nothing():
    from lsenerf_amd import _lib, ops
    lib = _lib.load()
    c = _case("head4", 64)
    big = torch.zeros(1 << 16, device="cuda")                       # stands in for any operand: nothing may be read or written
    wide = torch.zeros(1 << 16, device="cuda")

    def rc_of(meta, d_in, d_rb, idx=c["idx"]):
        d = meta.desc()
        return lib.lse_mlp_bwd_input(ctypes.byref(d), _P(big), _P(big), _P(big), 4, _P(big), None, None, 0.0, _P(d_in), _P(big), _P(idx),
                                     _P(d_rb), 64, None, ops._stream())

    d_in = torch.full((64, 64), SENTINEL, device="cuda")
    INVALID, UNSUPPORTED = -1, -3                                   # LSE_E_INVALID, LSE_E_UNSUPPORTED (include/lse_hip.h)
    cases = {
        "width 32": (ops.MlpMeta(16, 32, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR), d_in, None, c["idx"], UNSUPPORTED),
        "64 inputs": (ops.MlpMeta(64, 64, 2, _lib.LSE_ACT_SIGMOID, _lib.LSE_IN_ROWMAJOR), d_in, None, c["idx"], UNSUPPORTED),
        "one hidden layer on 16 inputs": (ops.MlpMeta(16, 64, 1, _lib.LSE_ACT_NONE, _lib.LSE_IN_ROWMAJOR), d_in, None, c["idx"],
                                          UNSUPPORTED),
        "f32 arithmetic": (_meta("head4", arith=_lib.LSE_MLP_ARITH_F32_MFMA), d_in, None, c["idx"], UNSUPPORTED),
        "both outputs null": (_meta("head4"), None, None, c["idx"], INVALID),
        "d_row_bias without row_bias_idx": (_meta("head4"), d_in, wide, None, INVALID),
    }
    for what, (meta, di, drb, idx, code) in cases.items():
        rc = rc_of(meta, di, drb, idx)
        msg = lib.lse_last_error().decode()
        assert rc == code and "lse_mlp_bwd_input" in msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert bool((d_in == SENTINEL).all()) and float(wide.abs().max()) == 0.0 and float(big.abs().max()) == 0.0
    with pytest.raises(_lib.LseHipError, match="lse_mlp_bwd_input"):
        ops.mlp_bwd_input(c["params"], c["x"], _meta("head4", arith=_lib.LSE_MLP_ARITH_F32_MFMA), 64, c["out"], 4, c["d_out"],
                          d_in=torch.empty_like(c["x"]))
