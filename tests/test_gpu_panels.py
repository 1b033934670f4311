"""The eval-panel kernels on the GPU (csrc/panels.hip) against the numpy twin of tests/panels_ref.py, bit for bit: the 8-bit grey,
Canny's classification on sizes below, at and across the tile, the host-free hysteresis on hand-built class maps, the uint8 panel
grid for every column subset; then the grid against the torch route on the device, and ``evaluate_set(panels=...)``.

The rule against the torch route (``clamp(v * 255, 0, 255).to(uint8)`` of the float panels): a value whose ``v * 255`` lies more than
1e-3 from an integer must be equal, the rest may differ by one level (the channel-sum order of torch's grey reduction is not the
kernel's).  The dedicated fixture first shows that at least 99 % of the values of every panel are of the first kind, counted on
torch's own values.  One mend of that precondition: "err_map" writes the exact constant 1 wherever the error has the other sign
(about half of its values, with no arithmetic behind them, so ``v * 255`` is exactly 255 on both routes); those count as values that
must be equal and are left out of the 99 % count, which is taken over the values that came from arithmetic."""
import numpy as np
import pytest
import torch

from tests import panels_ref as ref
from tests.test_gpu_eval import CHUNK, H, W, _model
from tests.test_gpu_eval_set import N_IMG, _eval_set

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 3), (5, 7), (37, 53), (64, 96), (97, 130)]          # below one tile, odd, a multiple of the tile, several tiles


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------- grey
def test_gray8_equals_the_twin():
    from lsenerf_amd import ops
    rng = np.random.default_rng(0)
    a = rng.random((3, 37, 53), dtype=np.float32) * 1.2 - 0.1           # some values below 0 and above 1
    b = rng.random((3, 37, 53), dtype=np.float32)
    a[:, 0, 0] = np.nan
    a[:, 0, 1] = (1.0, 1.0, 1.0)
    b[:, 5, 5] = 0.0
    out = ops.gray8_planes(_dev(a), _dev(b)).cpu().numpy()
    assert out.shape == (2, 37, 53) and out[0, 0, 0] == 0
    assert (out[0] == ref.gray8(a)).all() and (out[1] == ref.gray8(b)).all()
    one = ops.gray8_planes(_dev(b)[None]).cpu().numpy()                 # [1, 3, H, W], one image
    assert one.shape == (1, 37, 53) and (one[0] == ref.gray8(b)).all()


# ---------------------------------------------------------------------------------------------------- classification
@pytest.mark.parametrize("hw", SIZES)
def test_classify_equals_the_twin(hw):
    from lsenerf_amd import ops
    fixtures = ref.classify_fixtures(*hw)
    counts = {}
    want = np.stack([ref.canny_classify(img, branches=counts) for _, img in fixtures])
    if hw[0] * hw[1] >= 35:          # (a 1 x 1 image has no gradient at all, a 3 x 3 one too few pixels for every direction)
        assert all(counts[k] > 0 for k in ("horizontal", "vertical", "diagonal_pos", "diagonal_neg")), counts
    got = ops.canny_classify(_dev(np.stack([img for _, img in fixtures]))).cpu().numpy()          # one launch for the stack
    for k, (name, _) in enumerate(fixtures):
        assert (got[k] == want[k]).all(), (name, int((got[k] != want[k]).sum()))
    single = ops.canny_classify(_dev(fixtures[5][1])).cpu().numpy()                                # [H, W] alone
    assert (single == want[5]).all()
    other = ops.canny_classify(_dev(fixtures[6][1]), low=20.5, high=90).cpu().numpy()              # other thresholds, floored
    assert (other == ref.canny_classify(fixtures[6][1], 20, 90)).all()
    assert (ops.canny_classify(_dev(fixtures[6][1]), low=90, high=20).cpu().numpy() == other).all()          # swapped, as OpenCV


# ---------------------------------------------------------------------------------------------------- hysteresis
@pytest.mark.parametrize("hw", [(97, 130), (5, 7)])
def test_hysteresis_equals_the_twin(hw):
    from lsenerf_amd import ops
    fixtures = ref.hysteresis_fixtures(*hw)
    maps = np.stack([m for _, m in fixtures])
    want = np.stack([ref.hysteresis_label(m) for m in maps])
    cls = _dev(maps)
    n_ws = ops.canny_workspace_bytes(hw[0], hw[1], len(fixtures)) // 8
    ws = torch.full((n_ws,), -1, dtype=torch.int64, device="cuda")                                 # every byte 0xFF
    got = ops.canny_hysteresis(cls, workspace=ws).cpu().numpy()
    for k, (name, _) in enumerate(fixtures):
        assert (got[k] == want[k]).all(), (name, int((got[k] != want[k]).sum()))
    if hw == (97, 130):
        spiral, length = ref.spiral_map(*hw)
        assert length > 2000 and (got[0] == (spiral > 0) * 255).all() and not got[1].any()
    again = ops.canny_hysteresis(cls, workspace=torch.zeros_like(ws)).cpu().numpy()                # zero workspace, second run
    assert (again == got).all()
    assert (ops.canny_hysteresis(cls).cpu().numpy() == got).all()                                  # whatever the allocator hands out
    one = ops.canny_hysteresis(_dev(maps[7])).cpu().numpy()                                        # [H, W] alone: random 0.1
    assert (one == want[7]).all()
    inplace = cls.clone()
    assert ops.canny_hysteresis(inplace, out=inplace) is inplace and (inplace.cpu().numpy() == got).all()


@pytest.mark.parametrize("hw", [(37, 53), (97, 130)])
def test_canny_edges_is_classify_then_hysteresis(hw):
    from lsenerf_amd import ops
    imgs = np.stack([ref.noise_image(*hw, r) for r in (0, 1, 3)])
    g = _dev(imgs)
    edges = ops.canny_edges(g)
    assert torch.equal(edges, ops.canny_hysteresis(ops.canny_classify(g)))
    want = np.stack([ref.canny(img) for img in imgs])
    assert (edges.cpu().numpy() == want).all() and 0 < (want > 0).mean() < 1
    assert set(np.unique(want)) <= {0, 255}


# ---------------------------------------------------------------------------------------------------- panels
def _panel_inputs(h, w, masked, seed=0, float_gt=False):
    """Device inputs of ops.eval_panels for a random image pair (through lse_eval_image_prep, as evaluate_set feeds them)."""
    from lsenerf_amd import ops
    g = torch.Generator().manual_seed(seed)
    gt = torch.rand(h, w, 3, generator=g) if float_gt else torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    msk = (torch.rand(h, w, generator=g) > 0.3).to(torch.uint8).cuda() if masked else None
    rgb = torch.rand(h * w, 3, generator=g).cuda()
    gt_pl, pr_pl, _ = ops.eval_image_prep(gt.cuda(), rgb, msk)
    depth = (torch.rand(h, w, 1, generator=g) * 3 + 0.5).cuda()
    acc = (torch.rand(h, w, 1, generator=g) * 0.98 + 0.01).cuda()                  # strictly inside (0, 1)
    edges = ops.canny_edges(ops.gray8_planes(gt_pl, pr_pl))
    ev = {c: torch.rand(h, w, c, generator=g).cuda() * 1.1 for c in (1, 3)}
    return dict(gt_planes=gt_pl, pred_planes=pr_pl, rgb=rgb, depth=depth, accumulation=acc, edges=edges), ev


def _np(inputs, ev=None, pair=None):
    d = {k: v.cpu().numpy() for k, v in inputs.items()}
    d["acc"] = d.pop("accumulation")
    if ev is not None:
        d["ev_out"] = ev.cpu().numpy()
    if pair is not None:
        d["pair"] = tuple(p.cpu().numpy() for p in pair)
    return d


SUBSETS = [("img", "depth", "err_map"), ("img", "depth", "err_map", "overlay"), ("img", "depth", "err_map", "ev_out"),
           ref.PANEL_KEYS, ("overlay",), ("ev_out",), ("depth", "overlay"), ("err_map", "ev_out"), ("img",)]


@pytest.mark.parametrize("hw,masked", [((24, 40), False), ((37, 53), True)])
def test_panels_equal_the_twin_for_every_column_subset(hw, masked):
    from lsenerf_amd import ops
    h, w = hw
    inputs, ev = _panel_inputs(h, w, masked, seed=h)
    assert 0 < float((inputs["edges"] > 0).float().mean()) < 1
    for keys in SUBSETS:
        for c in ((1, 3) if "ev_out" in keys else (None,)):
            e = ev[c] if c else None
            grid = ops.eval_panels(keys, h, w, ev_out=e, **inputs)
            assert tuple(grid.shape) == (h, ref.panel_columns(keys) * w, 3) and grid.dtype == torch.uint8
            want = ref.panels(keys, **_np(inputs, e))
            assert (grid.cpu().numpy() == want).all(), (keys, c)
    # the grey pair of the event-only metric as "img"
    pair = (torch.rand(1, 1, h, w, device="cuda"), torch.rand(1, 1, h, w, device="cuda") * 1.3)
    grid = ops.eval_panels(("img", "overlay"), h, w, pair=pair, **inputs)
    assert (grid.cpu().numpy() == ref.panels(("img", "overlay"), **_np(inputs, pair=pair))).all()
    # the order of the keys does not matter: the columns come in ops.PANEL_KEYS' order
    assert torch.equal(ops.eval_panels(("overlay", "img"), h, w, pair=pair, **inputs), grid)


def test_panels_on_a_flat_depth_plane_and_on_nans():
    from lsenerf_amd import ops
    h, w = 24, 40
    inputs, _ = _panel_inputs(h, w, False, seed=3)
    inputs["depth"] = torch.full((h, w, 1), 1.75, device="cuda")                    # far == near: 0 / 1e-10, no NaN
    ws = torch.empty(ops.eval_panels_workspace_bytes(h, w) // 4, dtype=torch.float32, device="cuda")
    grid = ops.eval_panels(("depth",), h, w, workspace=ws, **inputs)
    assert ws[:2].tolist() == [1.75, 1.75]
    assert (grid.cpu().numpy() == ref.panels(("depth",), **_np(inputs))).all() and int(grid.min()) >= 254
    inputs["depth"] = inputs["depth"].clone()
    inputs["depth"][3, 4] = float("nan")                                            # torch.min hands the NaN on: every value NaN -> 0
    grid = ops.eval_panels(("depth", "err_map"), h, w, workspace=ws, **inputs)
    assert bool(torch.isnan(ws[:2]).all()) and not grid[:, :w].any()
    assert (grid.cpu().numpy() == ref.panels(("depth", "err_map"), **_np(inputs))).all()


def _torch_grid(images, columns):
    """The writer's route on the device: clamp(v * 255, 0, 255).to(uint8) per key, one channel tiled to three, concatenated.  Also
    v * 255 of every value (float32) for the rule."""
    u8, scaled = [], []
    for k in columns:
        v = images[k].to(torch.float32)
        if v.shape[-1] == 1:
            v = v.expand(-1, -1, 3)
        t = v * 255
        scaled.append(t)
        u8.append(torch.clamp(t, 0, 255).to(torch.uint8))
    return torch.cat(u8, dim=1), torch.cat(scaled, dim=1)


def _check_against_torch(grid, images, columns, w, require_99=False):
    """The rule of this module's docstring; ``images["overlay"]`` (values 0 / 1) must match exactly."""
    want, t = _torch_grid(images, columns)
    assert grid.shape == want.shape
    safe = (t - torch.round(t)).abs() > 1e-3
    x = 0
    for k in columns:
        width = (2 if k == "img" else 1) * w
        sl = slice(x, x + width)
        x += width
        g, wt, s = grid[:, sl].to(torch.int32), want[:, sl].to(torch.int32), safe[:, sl]
        if k == "overlay":
            assert torch.equal(g, wt), k
            continue
        exact_const = (images[k] == 1.0) if k == "err_map" else torch.zeros_like(s)
        if require_99:
            arith = ~exact_const
            frac = float((s & arith).sum()) / max(int(arith.sum()), 1)
            assert frac >= 0.99, (k, frac)
        must = s | exact_const
        assert torch.equal(g[must], wt[must]), (k, int((g[must] != wt[must]).sum()))
        assert int((g - wt).abs().max()) <= 1, k


def test_panels_equal_the_torch_route_away_from_rounding_boundaries():
    from lsenerf_amd import eval_set as es, ops
    h, w = 24, 40
    inputs, ev = _panel_inputs(h, w, False, seed=21, float_gt=True)
    outputs = {"rgb": inputs["rgb"].reshape(h, w, 3), "accumulation": inputs["accumulation"], "depth": inputs["depth"],
               "ev_out": ev[1]}
    images = es._image_dict(outputs, inputs["gt_planes"], inputs["pred_planes"])
    columns = ("img", "depth", "err_map", "ev_out")
    grid = ops.eval_panels(columns, h, w, ev_out=ev[1], **inputs)
    _check_against_torch(grid, images, columns, w, require_99=True)


# ---------------------------------------------------------------------------------------------------- the whole set
@pytest.mark.parametrize("events_only,eps", [(False, 0.0), (True, 0.0), (False, 1e-4)], ids=["rgb", "events_only", "early_stop"])
def test_evaluate_set_fills_the_panel_set_without_a_wait_of_its_own(events_only, eps, monkeypatch):
    from lsenerf_amd import PanelSet, ops
    from lsenerf_amd.eval_set import camera_bundle
    from lsenerf_amd.evaluation import uses_count_free_route
    m = _model(eval_overlay=True, eval_early_stop_eps=eps, eval_segment_samples=64)
    assert uses_count_free_route(m, H * W) and CHUNK == 256
    s, gt_images, gt_msk = _eval_set(masked="u8", seed=31)
    ps = PanelSet(s)
    assert ps.keys == ops.PANEL_KEYS and ps.host is None
    seen = []

    def keep(i, outputs, images):
        columns = tuple(k for k in ops.PANEL_KEYS if k in images)
        seen.append((columns, {k: images[k].clone() for k in columns}))
    _, rows_plain = m.evaluate_set(s, events_only=events_only)
    _, rows_cb = m.evaluate_set(s, events_only=events_only, on_image=keep)
    torch.cuda.synchronize()
    grid = m.occupancy_grid
    orig, reached = grid.check_deferred_overflow, []

    def overflow_read():
        reached.append(torch.cuda.get_sync_debug_mode())
        torch.cuda.set_sync_debug_mode("default")
        orig()
    monkeypatch.setattr(grid, "check_deferred_overflow", overflow_read)
    c0 = ops.SYNC_STATS["count"]
    torch.cuda.set_sync_debug_mode("error")
    try:
        _, rows = m.evaluate_set(s, events_only=events_only, panels=ps)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert reached == [2] and ops.SYNC_STATS["count"] == c0          # no wait up to the set's own overflow read
    assert rows == rows_plain == rows_cb                              # the metrics bit for bit
    assert len(seen) == N_IMG
    columns = seen[0][0]
    assert columns == ("img", "depth", "err_map", "overlay") == ps.columns          # this model renders no "ev_out"
    assert tuple(ps.host.shape) == (N_IMG, H, 5 * W, 3) and ps.host.is_pinned() and ps.host.dtype == torch.uint8
    assert len({ps.host[i].numpy().tobytes() for i in range(N_IMG)}) == N_IMG       # three different images
    for i in range(N_IMG):
        images = seen[i][1]
        assert list(k for k in images) == list(columns)
        ov = images["overlay"]
        assert ov.dtype == torch.float32 and set(ov.unique().tolist()) <= {0.0, 1.0}
        host = ps.host[i].cuda()
        assert torch.equal((ov * 255).to(torch.uint8), host[:, 4 * W:5 * W])        # the dictionary's overlay is the grid's column
        _check_against_torch(host, images, columns, W)
    if not events_only:          # the per-image route's dictionary carries the same overlay, after "err_map"
        out = m.get_outputs_for_camera_ray_bundle(camera_bundle(s, 1))
        _, imgs = m.get_image_metrics_and_images(out, {"image": gt_images[1].float() / 255.0, "msk": gt_msk[1]})
        assert list(imgs) == ["img", "accumulation", "depth", "err_map", "overlay"]
        assert torch.equal(imgs["overlay"], seen[1][1]["overlay"])
    # a PanelSet without the overlay column
    ps2 = PanelSet(s, keys=("err_map", "img"))
    m.evaluate_set(s, events_only=events_only, panels=ps2)
    assert ps2.columns == ("img", "err_map") and torch.equal(ps2.host, torch.cat([ps.host[:, :, :2 * W], ps.host[:, :, 3 * W:4 * W]], dim=2))
