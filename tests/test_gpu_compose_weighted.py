"""The batch composer with ``sampling=PixelSampling(...)`` on the GPU: the composed step's pixels, targets and ``draw_weights``
against the numpy twin of the weighted draw (tests/pixel_draw_ref.py) on a small two-stream scene with masks, eager and inside a
captured training step; and a composer without ``sampling`` on the same scene, which draws what it always drew."""
import numpy as np
import pytest
import torch

from tests import pixel_draw_ref as pr
from tests.test_pixel_draw_cpu import COL_HW, EVS_HW, N_FRAMES, scene_weights, small_scene

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("error:The AccumulateGrad node's stream")]

N_COL_PIX, N_EVS_PIX, SEED = 200, 65, 2 ** 33 + 11


def _sampling():
    from lsenerf_amd.data import PixelSampling
    return PixelSampling(evs_active_weight=9, evs_idle_weight=1)


def _np(t):
    return t.detach().cpu().numpy()


def _check_step(comp, bundles, batch, arrays, w_col, w_evs, step):
    """Everything the composed step holds about its pixels, against the twin's draw at ``step``."""
    (col, prev, nxt) = bundles
    want_col, wt_col = pr.draw(w_col, comp.seed, step, 0, comp.n_col)
    want_evs, wt_evs = pr.draw(w_evs, comp.seed, step, 1, comp.n_evs)
    cb, eb = batch["col_batch"], batch["evs_batch"]
    assert np.array_equal(_np(cb["indices"]), want_col) and np.array_equal(_np(eb["indices"]), want_evs)     # (camera i = image i here)
    assert np.array_equal(_np(col.metadata["coords"]), want_col)
    assert np.array_equal(_np(prev.metadata["coords"]), want_evs) and np.array_equal(_np(nxt.metadata["coords"]), want_evs)
    assert np.array_equal(_np(comp.draw_weights[0]), wt_col) and np.array_equal(_np(comp.draw_weights[1]), wt_evs)
    assert set(np.unique(wt_col)) == {1} and set(np.unique(wt_evs)) <= {1, 9}
    c, y, x = want_col.T
    assert np.array_equal(_np(cb["image"]), arrays["col_img"][c, y, x].astype(np.float32) / np.float32(255.0))
    assert np.array_equal(_np(cb["msk"]).reshape(-1), arrays["col_msk"][c, y, x].astype(np.float32))
    c, y, x = want_evs.T
    assert np.array_equal(_np(eb["image"]).reshape(-1), arrays["frames"][c, y, x].astype(np.float32) * np.float32(0.25))
    assert np.array_equal(_np(eb["msk"]).reshape(-1), arrays["evs_msk"][c, y, x])
    assert bool((cb["msk"] != 0).all()) and bool((eb["msk"] != 0).all())          # no masked pixel is trained on
    assert np.array_equal(wt_evs == 9, _np(eb["image"]).reshape(-1) != 0)         # the weight says whether the target is an event
    h_col, h_evs = comp.indices_host(step)
    assert np.array_equal(h_col, want_col) and np.array_equal(h_evs, want_evs)
    return want_col, want_evs


def test_eager_compose_draws_the_twins_pixels():
    from lsenerf_amd.data import BatchComposer, draw_indices_host
    scene, arrays = small_scene("cuda")
    s = _sampling()
    comp = BatchComposer(scene, N_COL_PIX, N_EVS_PIX, seed=SEED, sampling=s)
    w_col, w_evs = scene_weights(arrays, s)
    assert comp.sampling_totals == (int(w_col.sum()), int(w_evs.sum()))
    assert float((arrays["frames"] != 0).mean()) < 0.35                            # a uniform draw would mostly meet zeros ...
    active = []
    for step in (0, 3, 2 ** 32 + 3):
        bundles, batch = comp.compose(step=step)
        _check_step(comp, bundles, batch, arrays, w_col, w_evs, step)
        active.append(float((batch["evs_batch"]["image"] != 0).float().mean()))
        assert int(comp.step_dev) == 0                                              # an explicit step leaves the counter alone
    assert min(active) > 0.6                                                        # ... the weighted one mostly meets events
    comp.set_step(7)
    for k in range(3):                                                              # the device counter: used, then advanced
        bundles, batch = comp.compose()
        _check_step(comp, bundles, batch, arrays, w_col, w_evs, 7 + k)
        assert int(comp.step_dev) == 8 + k
    # given pixels win over the draw, for whichever stream they are given
    g = torch.Generator().manual_seed(1)
    given = torch.stack([torch.randint(0, N_FRAMES, (N_EVS_PIX,), generator=g), torch.randint(0, EVS_HW[0], (N_EVS_PIX,), generator=g),
                         torch.randint(0, EVS_HW[1], (N_EVS_PIX,), generator=g)], -1)
    _, batch = comp.compose(step=5, indices=(None, given))
    assert torch.equal(batch["evs_batch"]["indices"].cpu().long(), given)
    assert np.array_equal(_np(batch["col_batch"]["indices"]), pr.draw(w_col, SEED, 5, 0, N_COL_PIX)[0])
    assert not bool((batch["evs_batch"]["msk"] != 0).all())                         # (given pixels are the caller's business)
    # after an edit in place the tables follow on request
    scene.evs.images[1] = 0
    arrays["frames"][1] = 0
    totals = comp.rebuild_sampling()
    w_col2, w_evs2 = scene_weights(arrays, s)
    assert totals == (int(w_col2.sum()), int(w_evs2.sum())) and totals[1] < int(w_evs.sum())
    _check_step(comp, *comp.compose(step=11), arrays, w_col2, w_evs2, 11)
    # a composer without sampling, same scene and seed: the uniform convention, untouched
    plain = BatchComposer(scene, N_COL_PIX, N_EVS_PIX, seed=SEED)
    _, batch = plain.compose(step=3)
    assert np.array_equal(_np(batch["col_batch"]["indices"]), draw_indices_host(SEED, 3, 0, N_COL_PIX, 3, *COL_HW))
    assert np.array_equal(_np(batch["evs_batch"]["indices"]), draw_indices_host(SEED, 3, 1, N_EVS_PIX, N_FRAMES, *EVS_HW))
    assert not bool((batch["evs_batch"]["msk"] != 0).all())


def test_a_uniform_setting_still_takes_the_weighted_route():
    """Equal event weights and no mask to respect: every pixel weighs 1, and the pixels are those of the weighted convention (one
    convention per setting, whatever the data)."""
    from lsenerf_amd.data import BatchComposer, PixelSampling
    scene, arrays = small_scene("cuda", masks=False)
    comp = BatchComposer(scene, 63, 65, seed=5, sampling=PixelSampling())
    assert comp.sampling_totals == (3 * COL_HW[0] * COL_HW[1], N_FRAMES * EVS_HW[0] * EVS_HW[1])
    _, batch = comp.compose(step=2)
    w = np.ones((N_FRAMES,) + EVS_HW, np.int64)
    assert np.array_equal(_np(batch["evs_batch"]["indices"]), pr.draw(w, 5, 2, 1, 65)[0])
    assert np.array_equal(_np(batch["col_batch"]["indices"]), pr.draw(np.ones((3,) + COL_HW, np.int64), 5, 2, 0, 63)[0])
    assert np.array_equal(comp.indices_host(2)[1], pr.draw(w, 5, 2, 1, 65)[0])
    assert "msk" not in batch["evs_batch"] and _np(comp.draw_weights[1]).tolist() == [1] * 65


def test_a_captured_step_replays_the_weighted_draw():
    from lsenerf_amd.data import BatchComposer
    from lsenerf_amd.graph import GraphedTrainStep
    from tests.test_gpu_compose import _models
    scene, arrays = small_scene("cuda")
    s = _sampling()
    comp = BatchComposer(scene, N_COL_PIX, N_EVS_PIX, seed=SEED, sampling=s, num_embd=8)
    w_col, w_evs = scene_weights(arrays, s)
    (m,), (opt,) = _models(1)
    s0 = 5
    comp.set_step(s0)
    step = GraphedTrainStep(m, opt, composer=comp, jitter="input")
    assert int(comp.step_dev) == s0                                                 # building draws nothing that stays
    g = torch.Generator().manual_seed(7)
    for k in range(3):
        losses = step(jitter=torch.rand(comp.n_rays, generator=g).cuda())
        assert all(np.isfinite(float(v.detach())) for v in losses.values()) and set(losses) == {"rgb_loss", "event_loss"}
        _check_step(comp, (step.col, step.prev, step.nxt), step.batch, arrays, w_col, w_evs, s0 + k)
        assert int(comp.step_dev) == s0 + k + 1
    comp.set_step(40)                                                               # a resumed run: the same graph, another position
    losses = step(jitter=torch.rand(comp.n_rays, generator=g).cuda())
    assert all(np.isfinite(float(v.detach())) for v in losses.values())
    _check_step(comp, (step.col, step.prev, step.nxt), step.batch, arrays, w_col, w_evs, 40)
    assert int(comp.step_dev) == 41
    step.check_overflow()
    step.close()
