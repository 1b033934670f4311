"""GPU tier of the loss-epilogue size tests: lse_loss_epilogue_fwd / _bwd (csrc/epilogue.hip), called through ops.loss_epilogue and
ops.loss_epilogue_packed, against the float64 reference of tests/epilogue_cases.py at every committed (descriptor, n_col, n_ev):
ray counts below one wave, with a partial last wave, of exactly one workgroup, one more than that and of several trips of the
stride loops, the colour and the event side in different classes.  Per case: losses and every gradient through the shared
comparison; the three-tensor and the packed route bitwise equal; each bundle alone; each loss backpropagated alone; a second run
bit-identical; MLP-mapper gradients added into destinations that already hold values."""
import pytest
import torch

from tests import epilogue_cases as ec

pytestmark = pytest.mark.gpu

CASES = ec.all_cases()
MLP_KEYS = ("mlp_rgb", "mlp_evs")


def _run(name, inp, route="three", bundles="both", upstream=ec.UPSTREAM, preload=None):
    """One forward + backward on the GPU -> the dictionary ``ec.evaluate`` returns (tensors on the device).  ``upstream``: weights
    of (rgb_loss, event_loss) in the backpropagated sum, None = that loss is not backpropagated at all.  ``preload``: {key: [8
    tensors]} put into the MLP parameters' .grad before the backward (the kernel adds into them)."""
    from lsenerf_amd import ops
    fields = ec.DESCRIPTORS[name][1]
    G = fields[4]
    dev = lambda t: t.detach().clone().cuda()
    P = {}
    for k, v in ec.used_params(name, inp).items():
        P[k] = [dev(t).requires_grad_(True) for t in v] if isinstance(v, list) else dev(v).requires_grad_(True)
    for k, gs in (preload or {}).items():
        if k in P:
            for p, g in zip(P[k], gs):
                p.grad = g.detach().clone().cuda()
    has_col, has_ev = bundles in ("both", "col"), bundles in ("both", "ev")
    n_col_rays, n_ev = (inp["col"].shape[0] if has_col else 0), (inp["prev"].shape[0] if has_ev else 0)
    col_gt, evs_gt = (dev(inp["col_gt"]) if has_col else None), (dev(inp["evs_gt"]) if has_ev else None)
    e_thresh = dev(inp["e_thresh"]) if (has_ev and fields[6] == ec.ENERF) else None
    kw = dict(pow_rgb=P.get("pow_rgb"), pow_evs=P.get("pow_evs"), w31=P.get("w31"), mlp_rgb=P.get("mlp_rgb", ()),
              mlp_evs=P.get("mlp_evs", ()), e_thresh=e_thresh)
    if route == "three":
        col = dev(inp["col"]).requires_grad_(True) if has_col else None
        prev = dev(inp["prev"]).requires_grad_(True) if has_ev else None
        nxt = dev(inp["next"]).requires_grad_(True) if has_ev else None
        rgb_loss, event_loss = ops.loss_epilogue(fields, col, col_gt, prev, nxt, evs_gt, **kw)
    else:
        parts = ([inp["col"]] if has_col else []) + ([inp["prev"], inp["next"]] if has_ev else [])
        allr = torch.cat(parts).cuda().requires_grad_(True)
        assert n_col_rays % G == 0
        rgb_loss, event_loss = ops.loss_epilogue_packed(fields, allr, n_col_rays, n_ev, col_gt, evs_gt, **kw)
    terms = [l * w for l, w, has in ((rgb_loss, upstream[0], has_col), (event_loss, upstream[1], has_ev)) if has and w is not None]
    sum(terms).backward()
    if route != "three":
        g = allr.grad
        col = prev = nxt = None
        d_col = g[:n_col_rays] if has_col else None
        d_prev, d_next = (g[n_col_rays:n_col_rays + n_ev], g[n_col_rays + n_ev:]) if has_ev else (None, None)
    else:
        d_col, d_prev, d_next = (t.grad if t is not None else None for t in (col, prev, nxt))
    grad = lambda k: None if k not in P else ([p.grad for p in P[k]] if isinstance(P[k], list) else P[k].grad)
    return {"rgb_loss": rgb_loss.detach(), "event_loss": event_loss.detach(), "d_col": d_col, "d_prev": d_prev, "d_next": d_next,
            "d_pow_rgb": grad("pow_rgb"), "d_pow_evs": grad("pow_evs"), "d_w31": grad("w31"), "d_mlp_rgb": grad("mlp_rgb"),
            "d_mlp_evs": grad("mlp_evs")}


def _tensors(res, keys):
    for k in keys:
        v = res[k]
        for i, t in enumerate(v if isinstance(v, list) else [v]):
            if t is not None:
                yield f"{k}{i if isinstance(v, list) else ''}", t


def _assert_bitwise(a, b, keys=ec.COLOUR_KEYS + ec.EVENT_KEYS):
    ta, tb = dict(_tensors(a, keys)), dict(_tensors(b, keys))
    assert set(ta) == set(tb)
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k


@pytest.mark.parametrize("case", CASES, ids=ec.case_id)
def test_loss_epilogue_at_size(case):
    name, n_col, n_ev, seed, variant = case
    inp, ref = ec.make_inputs(*case), ec.reference(*case)
    # (1) both bundles, three tensors, both losses: everything against float64
    a = _run(name, inp)
    res = ec.compare(a, ref, inp, do_assert=False)
    print(ec.case_id(case), "worst", ec.worst(res), {k: f"{v:.3f}" for k, v in res.items() if v > 0.05})
    ec.compare(a, ref, inp)
    # (2) the same again: fixed-order sums, bit-identical
    _assert_bitwise(_run(name, inp), a)
    # (3) one packed buffer (the event rows start behind n_col * group colour rows: an odd offset for an odd n_col), the MLP
    #     mappers' gradient destinations already holding values: the same bits, added to what was there
    g = torch.Generator().manual_seed(11)
    used = ec.used_params(name, inp)
    noise = {k: [torch.randn(t.shape, generator=g) * 0.37 for t in used[k]] for k in MLP_KEYS if k in used}
    b = _run(name, inp, route="packed", preload=noise)
    _assert_bitwise(b, a, keys=("rgb_loss", "event_loss", "d_col", "d_prev", "d_next", "d_pow_rgb", "d_pow_evs", "d_w31"))
    for k in noise:
        for i in range(8):
            assert torch.equal(b["d_" + k][i], noise[k][i].cuda() + a["d_" + k][i]), (k, i)
    # (4) each bundle alone (a descriptor may take the other kernel pair then: no bitwise statement)
    c = _run(name, inp, bundles="col")
    assert float(c["event_loss"]) == 0.0 and c["d_prev"] is None
    ec.compare(c, ref, inp, keys=ec.COLOUR_KEYS)
    e = _run(name, inp, bundles="ev", route="packed")
    assert float(e["rgb_loss"]) == 0.0 and e["d_col"] is None
    ec.compare(e, ref, inp, keys=ec.EVENT_KEYS)
    # (5) one loss backpropagated alone: the other side's gradients are exactly zero, this side's the same bits
    for upstream, live, dead in (((None, ec.UPSTREAM[1]), ec.EVENT_KEYS, ec.COLOUR_KEYS), ((ec.UPSTREAM[0], None), ec.COLOUR_KEYS, ec.EVENT_KEYS)):
        for route in ("three", "packed"):
            o = _run(name, inp, route=route, upstream=upstream)
            _assert_bitwise(o, a, keys=live)
            for k, t in _tensors(o, [k for k in dead if k.startswith("d_")]):
                assert float(t.abs().max()) == 0.0, (k, route)


def test_packed_route_keeps_preloaded_scalar_gradients():
    """pow_rgb / pow_evs / ThreeToOne gradients reach a preallocated .grad by addition too (ops._scalar_param_grads)."""
    from lsenerf_amd import ops
    name, n_col, n_ev = "co_map_powpow_learned", 1025, 341
    inp = ec.make_inputs(name, n_col, n_ev)
    a = _run(name, inp)
    fields = ec.DESCRIPTORS[name][1]
    P = {k: inp[k].clone().cuda().requires_grad_(True) for k in ("pow_rgb", "pow_evs", "w31")}
    for i, p in enumerate(P.values()):
        p.grad = torch.full_like(p, 0.5 + i)
    allr = torch.cat([inp["col"], inp["prev"], inp["next"]]).cuda().requires_grad_(True)
    l = ops.loss_epilogue_packed(fields, allr, n_col, n_ev, inp["col_gt"].cuda(), inp["evs_gt"].cuda(), P["pow_rgb"], P["pow_evs"], P["w31"])
    (l[0] * ec.UPSTREAM[0] + l[1] * ec.UPSTREAM[1]).backward()
    for i, k in enumerate(P):
        assert torch.equal(P[k].grad, (0.5 + i) + a["d_" + k]), k
