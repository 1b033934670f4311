"""``ops.mlp_bwd_route``: what ``fused_mlp`` saves for its backward and which backward runs, without a GPU.  The function is pure
(flags in, ``(act_tiled, input_only_kernel)`` out), so the whole decision is held here over the full cross product of network
shape x every boolean argument x each module switch turned off on its own.

``EXPECTED`` was produced once by evaluating the conditions ``_MlpFn.forward`` spelt out inline, before the route became a
function, on the same cross product: one string per (network, switch that is off), one character per combination of the boolean
arguments in the order of ``itertools.product((False, True), repeat=6)`` over ``ARGS``; ``0`` .. ``3`` = act_tiled with the
``lse_mlp_bwd`` backward, ``I`` = act_tiled 3 with the input-only kernel (``lse_mlp_bwd_input``)."""
import itertools

import pytest

ARGS = ("params_grad", "need_grad", "bias_grad", "bias_sorted", "has_count", "input_only")
SWITCHES = ("FUSED_WGRAD", "ACT_TILED", "RECOMPUTE_FIRST_LAYER", "RECOMPUTE_ALL", "FUSED_BIAS_GRAD")

_ZERO = "0" * 64
_ONE = "1" * 64
_X6 = "11111111111111111I3I1I3I11111I3I11111111111111113333333311113333"          # head / base, every switch on
_X6_NO_BIAS = "11111111111111111I3I1I3I1111111111111111111111113333333311111111"     # FUSED_BIAS_GRAD off
_SECOND_GEN = "1111111111111111111111111111111111111111111111112222222211112222"     # first hidden layer recomputed
_SECOND_GEN_NO_BIAS = "1111111111111111111111111111111111111111111111112222222211111111"
_F32 = "1111111111111111113311331111113311111111111111113333333311113333"
_F32_NO_BIAS = "1111111111111111113311331111111111111111111111113333333311111111"
EXPECTED = {
    "head": {None: _X6, "FUSED_WGRAD": _ZERO, "ACT_TILED": _ZERO, "RECOMPUTE_FIRST_LAYER": _X6, "RECOMPUTE_ALL": _SECOND_GEN,
             "FUSED_BIAS_GRAD": _X6_NO_BIAS},
    "base_row": {None: _X6, "FUSED_WGRAD": _ZERO, "ACT_TILED": _ZERO, "RECOMPUTE_FIRST_LAYER": _X6, "RECOMPUTE_ALL": _ONE,
                 "FUSED_BIAS_GRAD": _X6_NO_BIAS},
    "base_level": {None: _X6, "FUSED_WGRAD": _ZERO, "ACT_TILED": _ZERO, "RECOMPUTE_FIRST_LAYER": _X6, "RECOMPUTE_ALL": _ONE,
                   "FUSED_BIAS_GRAD": _X6_NO_BIAS},
    "width32": {None: _SECOND_GEN, "FUSED_WGRAD": _ZERO, "ACT_TILED": _ZERO, "RECOMPUTE_FIRST_LAYER": _ONE,
                "RECOMPUTE_ALL": _SECOND_GEN, "FUSED_BIAS_GRAD": _SECOND_GEN_NO_BIAS},
    "one_layer": {None: _ONE, "FUSED_WGRAD": _ZERO, "ACT_TILED": _ZERO, "RECOMPUTE_FIRST_LAYER": _ONE, "RECOMPUTE_ALL": _ONE,
                  "FUSED_BIAS_GRAD": _ONE},
    # the head with the f32-MFMA FORWARD (lse_mlp_desc.arith): its trainable / counted backward still recomputes in bf16x6
    # (tests/test_gpu_parity.py runs that pair), only lse_mlp_bwd_input insists on the bf16x6 forward
    "head_f32_fwd": {None: _F32, "FUSED_WGRAD": _ZERO, "ACT_TILED": _ZERO, "RECOMPUTE_FIRST_LAYER": _F32,
                     "RECOMPUTE_ALL": _SECOND_GEN, "FUSED_BIAS_GRAD": _F32_NO_BIAS},
}
AUTO_ARITH = ("head", "base_row", "base_level", "width32", "one_layer")


def _metas():
    from lsenerf_amd import _lib, ops
    row, lev = _lib.LSE_IN_ROWMAJOR, _lib.LSE_IN_LEVELMAJOR
    return {"head": ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID, row), "base_row": ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, row),
            "base_level": ops.MlpMeta(32, 64, 1, _lib.LSE_ACT_NONE, lev), "width32": ops.MlpMeta(16, 32, 2, _lib.LSE_ACT_NONE, row),
            "one_layer": ops.MlpMeta(16, 64, 1, _lib.LSE_ACT_NONE, row),
            "head_f32_fwd": ops.MlpMeta(16, 64, 2, _lib.LSE_ACT_SIGMOID, row, arith=_lib.LSE_MLP_ARITH_F32_MFMA)}


def _routes(name, off, monkeypatch):
    """[(arguments, act_tiled, input_only_kernel)] of network ``name`` with switch ``off`` (or none) turned off."""
    from lsenerf_amd import ops
    for sw in SWITCHES:
        monkeypatch.setattr(ops, sw, sw != off)
    meta, out = _metas()[name], []
    for bits in itertools.product((False, True), repeat=len(ARGS)):
        kw = dict(zip(ARGS, bits))
        tiled, input_only_kernel = ops.mlp_bwd_route(meta, **kw)
        assert tiled in (0, 1, 2, 3) and input_only_kernel in (False, True)
        out.append((kw, tiled, input_only_kernel))
    return out


@pytest.mark.parametrize("off", (None,) + SWITCHES)
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_route_equals_the_table_of_the_inline_logic(name, off, monkeypatch):
    got = "".join("I" if io else str(t) for _, t, io in _routes(name, off, monkeypatch))
    assert got == EXPECTED[name][off]


@pytest.mark.parametrize("off", (None,) + SWITCHES)
@pytest.mark.parametrize("name", AUTO_ARITH)
def test_route_rules(name, off, monkeypatch):
    from lsenerf_amd import ops
    meta = _metas()[name]
    for kw, tiled, input_only_kernel in _routes(name, off, monkeypatch):
        if tiled == 3:          # the two shapes, bf16x6 arithmetic, every switch on, and somebody who needs the recomputing kernels
            assert ops.mlp_input_only_shape(meta) and name in ("head", "base_row", "base_level")
            assert off in (None, "RECOMPUTE_FIRST_LAYER", "FUSED_BIAS_GRAD") and (off != "FUSED_BIAS_GRAD" or not kw["bias_grad"])
            assert kw["need_grad"] and (kw["params_grad"] or kw["has_count"] or kw["input_only"])
        if tiled == 2:          # the head-like case (two hidden layers, row-major) with trainable parameters
            assert meta.n_hidden_layers == 2 and kw["params_grad"] and kw["need_grad"] and off != "RECOMPUTE_FIRST_LAYER"
        if input_only_kernel:   # frozen parameters on route 3, asked for by the caller
            assert tiled == 3 and not kw["params_grad"] and kw["input_only"]
        if off in ("FUSED_WGRAD", "ACT_TILED"):
            assert tiled == 0 and not input_only_kernel
        else:
            assert tiled != 0
        if kw["bias_grad"] and not (kw["bias_sorted"] and off != "FUSED_BIAS_GRAD"):
            assert tiled in (0, 1)      # a needed bias gradient that cannot be reduced in-kernel never recomputes


def test_shape_predicates_share_one_rule():
    from lsenerf_amd import ops
    m = _metas()
    assert [n for n in sorted(m) if ops.mlp_input_only_shape(m[n])] == ["base_level", "base_row", "head"]
    assert ops._mlp_pair_shapes(m["base_row"], m["head"]) and ops._mlp_pair_shapes(m["base_level"], m["head"])
    assert not ops._mlp_pair_shapes(m["head"], m["head"]) and not ops._mlp_pair_shapes(m["base_row"], m["base_row"])
    assert not ops._mlp_pair_shapes(m["base_row"], m["head_f32_fwd"]) and not ops._mlp_pair_shapes(m["base_row"], m["width32"])
