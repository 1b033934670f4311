"""``LSENeRFModelConfig.eval_mlp_arith`` / ``LSEField.inference_arith``: the eval render with the two fused MLPs in a reduced-piece
route (bf16x3 / bf16x1).  Every eval route picks the option up through the field, so the equalities the default holds bit for bit
(tests/test_gpu_eval.py, tests/test_gpu_eval_early_stop.py) must hold under each route with no tolerance; training mode must not
see the option at all."""
import ctypes
import math

import pytest
import torch

from tests.test_gpu_eval import H, KEYS, W, _bundle, _check_equal, _model
from tests.test_gpu_eval_early_stop import _check_cut_equal, _es_model, _reference_cut, bits_equal

pytestmark = pytest.mark.gpu

REDUCED = ("bf16x3", "bf16x1")
IMAGE_KEYS = ("rgb", "accumulation", "depth")


def test_default_is_the_explicit_bf16x6():
    bundle = _bundle()
    a = _model().get_outputs_for_camera_ray_bundle(bundle)
    m = _model(eval_mlp_arith="bf16x6")
    assert m.field.inference_arith == "bf16x6"
    b = m.get_outputs_for_camera_ray_bundle(bundle)
    assert set(a) == set(b)
    for k in KEYS:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("route", REDUCED)
def test_count_free_render_equals_eager_loop_and_manual_composition(route):
    bundle = _bundle()
    m = _model(eval_mlp_arith=route)
    out, _ = _check_equal(m, bundle)                          # the eager eval ``forward`` loop over the same chunks, bit for bit
    # the same march, one density_rgb_packed under the route, ops.eval_composite: every ray keeps its own count
    ref, _ = _reference_cut(m, bundle, out["num_samples_per_ray"])
    for k in IMAGE_KEYS:
        assert bits_equal(out[k].reshape(H * W, -1), ref[k].reshape(H * W, -1)), k
    # ... and the route is really taken: the image is not the default's
    base = _model().get_outputs_for_camera_ray_bundle(bundle)
    assert not torch.equal(out["rgb"], base["rgb"])
    print(f"{route}: max |rgb - rgb(bf16x6)| = {float((out['rgb'] - base['rgb']).abs().max()):.3e}")


@pytest.mark.parametrize("route", REDUCED)
@pytest.mark.parametrize("eps", [0.5, 0.1])
def test_early_stop_route_under_a_reduced_route(route, eps):
    out, full = _check_cut_equal(_es_model(eps, eval_mlp_arith=route), _bundle())
    if eps == 0.5:
        assert int((out["num_samples_per_ray"].reshape(-1) < full).sum()) > 0
    base = _es_model(eps).get_outputs_for_camera_ray_bundle(_bundle())
    assert not torch.equal(out["rgb"], base["rgb"])


def _spy_mlp_arith(monkeypatch):
    """Records ``lse_mlp_desc.arith`` of every MLP call that reaches the library."""
    from lsenerf_amd import _lib
    seen = []
    real = _lib.call

    def call(name, *args):
        if name in ("lse_mlp_fwd", "lse_mlp_bwd", "lse_mlp_bwd_input"):
            seen.append((name, ctypes.cast(args[0], ctypes.POINTER(_lib.MlpDesc)).contents.arith))
        elif name == "lse_mlp_fwd_pair":
            seen.append((name, ctypes.cast(args[0], ctypes.POINTER(_lib.MlpDesc)).contents.arith))
            seen.append((name, ctypes.cast(args[5], ctypes.POINTER(_lib.MlpDesc)).contents.arith))
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", call)
    return seen


@pytest.mark.parametrize("route", REDUCED)
def test_training_mode_ignores_the_option(route, monkeypatch):
    """A training step's losses and gradients, and the occupancy refresh, with the option set and unset: the same bits, and no
    call of a training step or a refresh carries a reduced route.

    The gradients of a training step are sums of float atomics (hash table, weight-gradient flushes), so two steps of the SAME
    model state are not bit-reproducible on their own: measured on one MI355X, the flat gradients of two identical unset models
    differ in 63893 of 956608 elements by up to 1.1e-8 (values ~1e-3); an unset and a set one in 64815, by up to 1.1e-8.  The
    step is therefore run on two unset copies as well: where those two agree bit for bit the set copy must agree with them bit for
    bit too; where they do not, the set copy may differ from an unset one only as the unset copies differ from each other -- at
    most twice as many elements, at most twice the root-mean-square difference (over ~6e4 differing elements that statistic is
    steady to a few per cent, and one element wrong by 1e-5 alone would triple it).  Everything that carries no atomics -- the
    losses, the refreshed grid, the descriptors of every MLP launch -- is compared bit for bit."""
    from lsenerf_amd import ops
    from tests.test_gpu_graph import _eager_step, _setup
    (m_a, m_a2), (o_a, o_a2), batch_of = _setup(False)
    (m_b, _), (o_b, _), _ = _setup(False)
    assert torch.equal(o_a.flat.data, o_b.flat.data)              # the same state three times
    m_b.field.inference_arith = route
    m_b.config.eval_mlp_arith = route
    seen = _spy_mlp_arith(monkeypatch)
    # the occupancy refresh, on the three equal states (before any optimiser step: its input would carry the atomics' order)
    before = m_a.occupancy_grid.occs.clone()
    grids = []
    for m in (m_a, m_a2, m_b):
        torch.manual_seed(17)
        m.update_occupancy_grid(0)
        grids.append((m.occupancy_grid.occs.clone(), m.occupancy_grid.binaries.clone()))
    for occs, binaries in grids[1:]:
        assert torch.equal(occs, grids[0][0]) and torch.equal(binaries, grids[0][1])
    assert not torch.equal(grids[0][0], before)
    assert seen and all(arith == 0 for _, arith in seen), seen        # the refresh runs under torch.no_grad(), in training mode
    del seen[:]
    bundles, batch, jit = batch_of(60)
    l_a, g_a, _ = _eager_step(m_a, o_a, bundles, batch, jit, False)
    n_a = len(seen)
    l_a2, g_a2, _ = _eager_step(m_a2, o_a2, bundles, batch, jit, False)
    l_b, g_b, _ = _eager_step(m_b, o_b, bundles, batch, jit, False)
    assert n_a > 0 and len(seen) == 3 * n_a
    assert all(arith == 0 for _, arith in seen), seen
    assert l_a == l_a2 == l_b, (l_a, l_a2, l_b)
    own, got = (g_a != g_a2), (g_a != g_b)
    own_max, got_max = float((g_a - g_a2).abs().max()), float((g_a - g_b).abs().max())
    own_rms, got_rms = float((g_a - g_a2).double().pow(2).mean().sqrt()), float((g_a - g_b).double().pow(2).mean().sqrt())
    print(f"{route}: unset vs unset {int(own.sum())} of {g_a.numel()} elements differ, max {own_max:.3e} rms {own_rms:.3e}; "
          f"unset vs set {int(got.sum())} differ, max {got_max:.3e} rms {got_rms:.3e}")
    if not bool(own.any()):
        assert not bool(got.any()), got_max
    else:
        assert int(got.sum()) <= 2 * int(own.sum()) and got_rms <= 2 * own_rms, (int(got.sum()), int(own.sum()), got_rms, own_rms)
    # the visibility pre-pass and the refresh run under torch.no_grad(), in training mode: bf16x6 all the same
    assert seen and all(arith == 0 for _, arith in seen), seen
    # ... while the same model in eval mode takes the route
    del seen[:]
    m_b.eval()
    with torch.no_grad():
        m_b(bundles[0])
    assert seen and all(arith == ops.MLP_ARITH_ROUTES[route] for _, arith in seen), seen


@pytest.mark.parametrize("route", REDUCED)
def test_evaluate_set_under_a_reduced_route(route):
    from lsenerf_amd.eval_set import camera_bundle
    from tests.test_gpu_eval_set import N_IMG, _eval_set
    m = _model(eval_mlp_arith=route)
    s, images, msk = _eval_set(masked="f32", seed=11)
    average, per_image = m.evaluate_set(s)
    assert len(per_image) == N_IMG
    m6 = _model()
    for i in range(N_IMG):
        out = m.get_outputs_for_camera_ray_bundle(camera_bundle(s, i))
        metrics, _ = m.get_image_metrics_and_images(out, {"image": images[i].float() / 255.0, "msk": msk[i]})
        for k in ("psnr", "ssim"):
            assert math.isfinite(per_image[i][k]) and per_image[i][k] == metrics[k], (i, k, per_image[i], metrics)
        out6 = m6.get_outputs_for_camera_ray_bundle(camera_bundle(s, i))
        assert not torch.equal(out["rgb"], out6["rgb"])
    assert all(math.isfinite(float(v)) for v in average.values())
    # render_camera goes the same way
    from lsenerf_amd.cameras import EdCameras
    c2w = torch.tensor([[[1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 2.5]]])
    cams = EdCameras(c2w, fx=30.0, fy=30.0, cx=W / 2, cy=H / 2, width=W, height=H)
    cam, cam6 = m.render_camera(cams, 0), m6.render_camera(cams, 0)
    rb = cams.generate_rays(torch.zeros(H * W, dtype=torch.long), cams.get_image_coords().reshape(-1, 2))
    same = m.get_outputs_for_camera_ray_bundle(rb)
    assert torch.equal(same["rgb"].reshape(H, W, 3).to(cam["rgb"].device), cam["rgb"]) and not torch.equal(cam["rgb"], cam6["rgb"])
