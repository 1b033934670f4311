"""lse_adam_step / lse_adam_step_dev / lse_adam_schedule_dev and the two occupancy-grid kernels of csrc/optim.hip at the sizes
training runs them at: Adam's grid is capped at 2048 workgroups x 256 threads x 4 floats, so its grid-stride loop starts above
2 097 152 floats (training: ~12 M); occ_binarize's starts above 524 288 cells (training: 8.4 M).

Adam's reference is Adam in float64 from the same float32 gradients.  Errors are taken per element on the element's own scale --
for ``p`` S = |p0| + sum_k |delta p_k|, for ``exp_avg`` the same recursion run on |g|, for ``exp_avg_sq`` the value itself (only
where float64 puts it in float32's normal range, or at exactly 0) -- and the worst ratio must not exceed
max(4 x the same figure of torch.optim.Adam in float32 on the CPU, 2^-22): the kernel multiplies by reciprocals where torch
divides, hence the 4."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TINY = 1.1754943508222875e-38        # float32's smallest normal
FLOOR = 2.0 ** -22
SMALL = (1, 2, 3, 4, 5, 7, 1023, 1025)
LOOPING = (2097151, 2097152, 2097157, 4194309)      # one short of the cap, the cap, the first loop trips, two full trips + a tail
REGIMES = ("wide", "eps", "sparse")


def _keep_mask(n, g):
    """Sparse regime: 5 % of the elements ever see a gradient, in runs of 1 .. 6 that cross the 4-float vectors, plus runs laid
    across every 8th multiple of 1024 (one thread's trip to the next)."""
    keep = torch.zeros(n, dtype=torch.bool)
    n_runs = max(1, int(0.05 * n / 3.5))
    starts = torch.randint(0, n, (n_runs,), generator=g)
    lens = torch.randint(1, 7, (n_runs,), generator=g)
    for off in range(6):
        idx = starts[lens > off] + off
        keep[idx[idx < n]] = True
    for b in range(1024, n, 8 * 1024):
        keep[b - 2:b + 3] = True
    return keep


def _grads(regime, n, steps, seed):
    """[steps] float32 CPU gradients.  wide: randn x 10^[-6, 2]; eps: randn x 10^[-20, -11] (eps = 1e-15 decides the step);
    sparse: wide on a fixed 5 % of the elements and exactly 0 elsewhere in every step (the hash table's regime)."""
    g = torch.Generator().manual_seed(1000 * seed + n % 9973 + {"wide": 1, "eps": 2, "sparse": 3}[regime])
    keep = _keep_mask(n, g) if regime == "sparse" else None
    out = []
    for _ in range(steps):
        lo, hi = (-20, -10) if regime == "eps" else (-6, 3)
        x = torch.randn(n, generator=g) * (10.0 ** torch.randint(lo, hi, (n,), generator=g).float())
        if keep is not None:
            x = x * keep
        out.append(x.float())
    return out, keep


def _adam64(p0, grads, lrs, betas, eps, step0=0, grad_scale=1.0):
    """float64 Adam + the per-element scales.  Returns (p, m, v, S_p, S_m)."""
    b1, b2 = betas
    p, m, v = p0.double().clone(), torch.zeros_like(p0, dtype=torch.float64), torch.zeros_like(p0, dtype=torch.float64)
    s_p, s_m = p.abs().clone(), torch.zeros_like(p)
    for k, (g32, lr) in enumerate(zip(grads, lrs)):
        t = step0 + k + 1
        g = g32.double() * grad_scale
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        s_m = b1 * s_m + (1 - b1) * g.abs()
        dp = (lr / (1 - b1 ** t)) * (m / (v.sqrt() / math.sqrt(1 - b2 ** t) + eps))
        p = p - dp
        s_p = s_p + dp.abs()
    return p, m, v, s_p, s_m


def _torch32(p0, grads, lrs, betas, eps, step0=0):
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=lrs[0], betas=betas, eps=eps)
    if step0:
        opt.state[ref] = {"step": torch.tensor(float(step0)), "exp_avg": torch.zeros_like(ref), "exp_avg_sq": torch.zeros_like(ref)}
    for g, lr in zip(grads, lrs):
        opt.param_groups[0]["lr"] = lr
        ref.grad = g.clone()
        opt.step()
    st = opt.state[ref]
    return ref.detach(), st["exp_avg"], st["exp_avg_sq"]


def _ratios(p, m, v, ref64):
    """Worst err / scale of (p, exp_avg, exp_avg_sq) and the share of exp_avg_sq that is compared."""
    p64, m64, v64, s_p, s_m = ref64
    cpu = lambda t: t.detach().double().cpu()
    rp = ((cpu(p) - p64).abs() / s_p.clamp_min(TINY)).max()
    rm = ((cpu(m) - m64).abs() / s_m.clamp_min(TINY)).max()
    ok = (v64 >= TINY) | (v64 == 0)
    rv = ((cpu(v) - v64).abs()[ok] / v64[ok].clamp_min(TINY)).max()
    return {"p": float(rp), "exp_avg": float(rm), "exp_avg_sq": float(rv)}, float(ok.double().mean())


def _check(tag, got, ref64, base32):
    r, share = _ratios(*got, ref64)
    rb, _ = _ratios(*base32, ref64)
    print(tag, "kernel", {k: f"{x:.3e}" for k, x in r.items()}, "torch float32", {k: f"{x:.3e}" for k, x in rb.items()},
          f"exp_avg_sq compared {share:.2f}")
    assert share >= 0.5, share
    for k in r:
        assert r[k] <= max(4.0 * rb[k], FLOOR), (tag, k, r[k], rb[k])
    return r


def _p0(n, kind, seed):
    if kind == "zero":
        return torch.zeros(n)
    return (torch.rand(n, generator=torch.Generator().manual_seed(77 + seed)) * 2 - 1) * 1e-4


def _run_kernel(p0, grads, lrs, betas, eps, grad_scale=1.0):
    from lsenerf_amd import ops
    p = p0.clone().cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for k, (g, lr) in enumerate(zip(grads, lrs)):
        ops.adam_step(p, g.cuda(), m, v, lr, betas[0], betas[1], eps, k + 1, grad_scale)
    return p, m, v


def _case(n, regime, p0_kind, betas=(0.9, 0.999), eps=1e-15, steps=6, seed=0):
    grads, keep = _grads(regime, n, steps, seed)
    p0 = _p0(n, p0_kind, seed)
    lrs = [1e-2] * steps
    ref64 = _adam64(p0, grads, lrs, betas, eps)
    got = _run_kernel(p0, grads, lrs, betas, eps)
    _check(f"adam n={n} {regime} p0={p0_kind} eps={eps:g} betas={betas}", got, ref64, _torch32(p0, grads, lrs, betas, eps))
    if keep is not None:                  # never a gradient: untouched, bit for bit
        assert int((~keep).sum()) > 0 or n < 8
        idle = (~keep).cuda()
        assert torch.equal(got[0][idle], p0.cuda()[idle])
        assert int((got[1][idle] != 0).sum()) == 0 and int((got[2][idle] != 0).sum()) == 0


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("p0_kind", ["small", "zero"])
def test_adam_below_the_grid_cap(regime, p0_kind):
    for n in SMALL:
        _case(n, regime, p0_kind)


@pytest.mark.parametrize("p0_kind", ["small", "zero"])
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("n", LOOPING)
def test_adam_across_the_grid_stride_loop(n, regime, p0_kind):
    _case(n, regime, p0_kind)


def test_adam_other_hyperparameters_in_the_loop():
    _case(2097157, "wide", "small", betas=(0.8, 0.99), eps=1e-8)


def test_adam_grad_scale_is_exact_in_the_loop():
    """grad_scale = 0.25 on 4 g against 1.0 on g: scaling by a power of two is exact, so are the results."""
    n = 2097157
    grads, _ = _grads("wide", n, 2, seed=3)
    p0 = _p0(n, "small", 3)
    a = _run_kernel(p0, [4 * g for g in grads], [1e-2] * 2, (0.9, 0.999), 1e-15, grad_scale=0.25)
    b = _run_kernel(p0, grads, [1e-2] * 2, (0.9, 0.999), 1e-15)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _flat(seed=0):
    from lsenerf_amd.optim import FlatParams
    g = torch.Generator().manual_seed(5 + seed)
    a = torch.nn.Parameter(((torch.rand(37, 29, generator=g) * 2 - 1) * 1e-4).cuda())       # 1073 -> padded to 1088
    b = torch.nn.Parameter(((torch.rand(70, generator=g) * 2 - 1) * 1e-4).cuda())           # 70 -> padded to 128
    flat = FlatParams([a, b])
    assert flat.numel == 1088 + 128 and flat.offsets == [0, 1088]
    return flat


@pytest.mark.parametrize("max_steps,step0", [(8, 0), (200000, 199990)])
def test_flat_adam_host_and_device_clock_follow_the_schedule(max_steps, step0):
    """FlatAdam.step (scalars from the host) and prepare_step + step_staged (scalars derived on the device from a device-side step
    counter) over 12 steps that cross the end of the exponential decay, against float64 Adam driven by current_lr's formula, and
    against each other within 2^-22 of the element's scale (host and device ``pow`` need not agree in the last bit)."""
    from lsenerf_amd.optim import FlatAdam
    steps = 12
    lr_of = lambda done: math.exp(math.log(1e-2) * (1 - min(max(done / max_steps, 0.0), 1.0)) + math.log(1e-4) * min(max(done / max_steps, 0.0), 1.0))
    lrs = [lr_of(step0 + k) for k in range(steps)]
    assert lrs[0] > lrs[1] and lrs[-1] == lrs[-2] == lr_of(10 ** 9)                          # decaying, then clamped at lr_final
    results = {}
    for route in ("host", "device"):
        flat = _flat()
        p0 = flat.data.detach().cpu().clone()
        opt = FlatAdam(flat, lr=1e-2, eps=1e-15, lr_final=1e-4, max_steps=max_steps)
        opt.step_count = step0
        grads, _ = _grads("wide", flat.numel, steps, seed=9)
        live = torch.zeros(flat.numel, dtype=torch.bool)
        live[:1073] = True
        live[1088:1088 + 70] = True
        grads = [g * live for g in grads]                                                    # the alignment padding never has a gradient
        for k, g in enumerate(grads):
            flat.grad.copy_(g.cuda())
            assert abs(opt.current_lr() - lrs[k]) <= 1e-15
            if route == "host":
                opt.step()
            else:
                opt.prepare_step()
                opt.step_staged()
        assert opt.step_count == step0 + steps
        if route == "device":
            assert int(opt._step_dev.item()) == step0 + steps
        got = (flat.data, opt.exp_avg, opt.exp_avg_sq)
        ref64 = _adam64(p0, grads, lrs, (0.9, 0.999), 1e-15, step0=step0)
        _check(f"FlatAdam {route} max_steps={max_steps} step0={step0}", got, ref64, _torch32(p0, grads, lrs, (0.9, 0.999), 1e-15, step0=step0))
        pad = (~live).cuda()
        for t in got:
            assert int((t[pad] != 0).sum()) == 0                                             # padding: p, m, v stay exactly 0
        results[route] = [t.detach().double().cpu() for t in got]
    _, _, v64, s_p, s_m = ref64
    for (a, b), s in zip(zip(results["host"], results["device"]), (s_p, s_m, v64)):
        assert float(((a - b).abs() / s.clamp_min(TINY)).max()) <= FLOOR


def test_adam_refuses_a_misaligned_slice_and_touches_nothing():
    from lsenerf_amd import _lib, ops
    g = torch.Generator().manual_seed(2)
    bufs = [torch.randn(1030, generator=g).cuda() for _ in range(4)]
    bufs[3].abs_()
    before = [b.clone() for b in bufs]
    hyper = torch.tensor([1e-2, 0.1, 1.0, 0.9, 0.999, 1e-15], device="cuda")
    with pytest.raises(_lib.LseHipError, match="16-byte aligned"):
        ops.adam_step(bufs[0][1:], bufs[1][1:], bufs[2][1:], bufs[3][1:], 1e-2, 0.9, 0.999, 1e-15, 1)
    with pytest.raises(_lib.LseHipError, match="16-byte aligned"):
        ops.adam_step_dev(bufs[0][4:], bufs[1][4:], bufs[2][3:-1], bufs[3][4:], hyper)
    torch.cuda.synchronize()
    for a, b in zip(bufs, before):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ occupancy-grid kernels
@pytest.mark.parametrize("n", [1, 524287, 524289, 1048581])
def test_occ_binarize_across_its_grid_stride_loop(n):
    """The grid is capped at 2048 x 256 = 524 288 threads.  The comparison is strict: values equal to the threshold stay 0."""
    from lsenerf_amd import ops
    g = torch.Generator().manual_seed(n % 1000)
    occs = torch.rand(n, generator=g)
    thre = torch.tensor([0.37])
    occs[torch.randint(0, n, (max(1, n // 50),), generator=g)] = thre[0]
    occs[0] = 0.9
    occs[-1] = thre[0] if n in (1, 524289) else 0.9           # the last cell: on the threshold (the only cell of n = 1) / above it
    out = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    ops.occ_binarize(occs.cuda(), thre.cuda(), out)
    want = (occs > thre).to(torch.uint8)
    assert 0 < int(want.sum()) < n or (n == 1 and int(want.sum()) == 0)
    assert int((occs == thre).sum()) >= 1
    assert torch.equal(out.cpu(), want)


def test_occ_update_cells_with_heavy_duplication():
    """300 000 ids drawn from 50 000 of 65 536 cells: every touched cell ends at the maximum over its duplicates of
    max(occs * ema, new), bit for bit (one float32 product and comparisons); the other cells are untouched."""
    from lsenerf_amd import ops
    g = torch.Generator().manual_seed(8)
    cells, n = 65536, 300000
    occs = torch.rand(cells, generator=g)
    occs[torch.randint(0, cells, (3000,), generator=g)] = 0.0
    pool = torch.randperm(cells, generator=g)[:50000]
    ids = pool[(torch.rand(n, generator=g) ** 3 * 50000).long().clamp_max(49999)]           # skewed: some cells hundreds of times
    new = torch.rand(n, generator=g) * (torch.rand(n, generator=g) < 0.7)
    assert int(torch.bincount(ids, minlength=cells).max()) > 50
    upd = torch.maximum(occs[ids] * 0.95, new)
    want = occs.clone().scatter_reduce(0, ids, upd, "amax", include_self=False)
    got = occs.clone().cuda()
    ops.occ_update_cells(got, ids.cuda(), new.cuda(), 0.95)
    untouched = torch.ones(cells, dtype=torch.bool)
    untouched[ids] = False
    assert int(untouched.sum()) >= cells - 50000
    assert torch.equal(got.cpu()[untouched], occs[untouched])
    assert torch.equal(got.cpu(), want)
