"""Host side of the batch composer (lsenerf_amd.data): the batch split, the C-ABI surface, the Philox draw's host twin, and the
pose-table helpers against the ray generators of cameras.py.  Also the synthetic scene and the host composition (datasets +
generators + a restatement of add_metadata / CameraIdxFixer) that tests/test_gpu_compose.py compares the device composer with."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests.test_cameras_cpu import gen_data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("lse_compose_batch", "lse_compose_rays_bwd")


# ---------------------------------------------------------------------------------------------------- synthetic scene
COL_HW, EVS_HW = (20, 28), (18, 24)
N_COL, N_FRAMES = 6, 9
COL_APP = [0, 1, 3, 5, 6, 7]          # with num_embd = 8: the deblur offsets (-2 .. +1) clip at both ends
COL_TIMES = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
# event-camera times: before the first colour time, an exact tie (0.5), inside, and beyond the last colour time
EVS_TIMES = [-0.5, 0.5, 0.75, 1.5, 2.25, 3.0, 3.5, 4.6, 5.7, 6.5]


def _cams(n, hw, seed, times, f, dist=None):
    from lsenerf_amd import cameras as cam
    c2w, _ = gen_data(n, seed=seed)
    c2w[:, :3, 3] *= 0.3
    c = cam.EdCameras(torch.from_numpy(c2w), f, f * 1.07, hw[1] / 2 - 0.7, hw[0] / 2 + 0.4, hw[1], hw[0],
                      times=torch.tensor(times, dtype=torch.float32))
    c.distortion_params = None if dist is None else torch.tensor(dist, dtype=torch.float32)
    return c


def make_scene(tmp_path, distort=False, masks=False, prevnext=False, seed=0):
    """``(ColorDataset, EventFrameDataset)`` over a synthetic scene: 6 colour cameras (PNG files in ``tmp_path``), 9 int8 event
    frames under 10 event cameras (or 9 + 9 previous / next cameras), different poses and times, non-square images."""
    from PIL import Image
    from lsenerf_amd import cameras as cam
    from lsenerf_amd.scene_io import ColorDataset, EventFrameDataset, SceneOutputs
    rng = np.random.default_rng(seed)
    dist = (0.08, -0.02, 0.004, 0.0, 0.003, -0.002) if distort else None
    aabb = torch.tensor([[-1.0, -1, -1], [1, 1, 1]])
    files = []
    for i in range(N_COL):
        f = os.path.join(str(tmp_path), f"{i:05d}.png")
        Image.fromarray(rng.integers(0, 256, COL_HW + (3,), dtype=np.uint8)).save(f)
        files.append(f)
    col_cams = _cams(N_COL, COL_HW, 2, COL_TIMES, 31.0, dist)
    col_msk = (rng.random((N_COL,) + COL_HW) < 0.7) if masks else None
    col = ColorDataset(SceneOutputs(cameras=col_cams, scene_aabb=aabb, dataparser_scale=1.0, appearance_ids=list(COL_APP),
                                    image_filenames=files, msk=col_msk))
    n_ecam = N_FRAMES if prevnext else N_FRAMES + 1
    evs_cams = _cams(n_ecam, EVS_HW, 5, EVS_TIMES[:n_ecam], 27.0, dist)
    evs_cams.set_hard_cam_type(cam.HardCamType.EVS)
    prev_c = next_c = None
    if prevnext:
        prev_c = _cams(n_ecam, EVS_HW, 5, EVS_TIMES[:n_ecam], 27.0, dist)
        next_c = _cams(n_ecam, EVS_HW, 7, EVS_TIMES[1:n_ecam + 1], 27.0, dist)
    evs_msk = (rng.random((N_FRAMES,) + EVS_HW) < 0.7).astype(np.float32) if masks else None
    evs = EventFrameDataset(SceneOutputs(cameras=evs_cams, scene_aabb=aabb, dataparser_scale=1.0,
                                         appearance_ids=[7 - (i % 4) for i in range(N_FRAMES)], msk=evs_msk,
                                         events=rng.integers(-5, 6, (N_FRAMES,) + EVS_HW + (1,)).astype(np.int8), e_thresh=0.35,
                                         prev_cameras=prev_c, next_cameras=next_c))
    return col, evs


def find_closest_idxs(ref, srch):
    """R:lse_nerf/data_components.py:5-29, restated."""
    ins = torch.searchsorted(ref, srch).clamp(max=len(ref) - 1)
    prev = (ins - 1).clamp(min=0)
    return torch.where((ref[prev] - srch).abs() < (ref[ins] - srch).abs(), prev, ins)


def add_metadata(rb, batch, cam_id=0, max_app_id=10000000):
    """R:lse_nerf/utils.py:153-194, restated: appearance ids per ray (deblur: id + (k - 2), clipped), cam_type, and the pixel list
    tiled (not interleaved) up to the ray count, as ``fix_datashape`` leaves it."""
    n_rays, n = len(rb), len(batch["indices"])
    factor = n_rays // n
    app = batch["appearance_id"].reshape(-1, 1)
    if factor > 1:
        app = torch.clip(app + (torch.arange(factor) - factor // 2)[None], 0, max_app_id - 1).reshape(-1, 1)
    rb.metadata["appearance_id"] = app
    rb.metadata["cam_type"] = torch.full((n_rays,), cam_id)
    rb.metadata["coords"] = batch["indices"].repeat(factor, 1)
    return rb


def host_batch(ds, idx, is_evs):
    """What the reference's pixel sampler gathers for pixels ``idx`` [n, 3] = (c, y, x) from a dataset with every image cached."""
    c, y, x = idx[:, 0], idx[:, 1], idx[:, 2]
    b = {"image": torch.stack([ds.get_image(int(ci))[int(yi), int(xi)] for ci, yi, xi in idx.tolist()]),
         "appearance_id": torch.tensor([ds.appearance_ids[int(ci)] for ci in c]), "indices": idx.clone()}
    if ds.msk is not None:
        b["msk"] = ds.msk[c, y, x].float().reshape(-1, 1)
    if is_evs:
        b["e_thresh"] = ds.e_thresh
    return b


def host_compose(col_ds, evs_ds, col_idx, evs_idx, pairing="consec", spline=None, num_embd=8, rgb_times=None):
    """The step the reference's ``next_train`` (R:lse_nerf/lse_datamanager.py:337-372) composes for given pixels, from the scene_io
    datasets and the cameras.py generators.  ``spline``: the colour bundle is a deblur bundle (4 rays per pixel)."""
    from lsenerf_amd import cameras as cam
    col = prev = nxt = col_b = evs_b = None
    if col_idx is not None:
        if spline is not None:
            col_ds.cameras.set_interpolator(spline)
            col = cam.DeblurRayGenerator(col_ds.cameras)(col_idx)
            col_ds.cameras.set_interpolator(None)
        else:
            col = cam.RayGenerator(col_ds.cameras)(col_idx)
        col_b = host_batch(col_ds, col_idx, False)
        add_metadata(col, col_b, 0, num_embd)
    if evs_idx is not None:
        gen = cam.ConsecRayGenerator(evs_ds.cameras) if pairing == "consec" else \
            cam.PrevNextRayGenerator(evs_ds.out.prev_cameras, evs_ds.out.next_cameras)
        prev, nxt = gen(evs_idx)
        evs_b = host_batch(evs_ds, evs_idx, True)
        for rb in (prev, nxt):
            add_metadata(rb, evs_b, 1)
            if rgb_times is not None:          # CameraIdxFixer (R:lse_nerf/data_components.py:70-90)
                rb.camera_indices = find_closest_idxs(rgb_times, rb.times)
    return (col, prev, nxt), {"col_batch": col_b, "evs_batch": evs_b}


def random_indices(n, n_images, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, n_images, (n,), generator=g), torch.randint(0, hw[0], (n,), generator=g),
                        torch.randint(0, hw[1], (n,), generator=g)], -1)


# ---------------------------------------------------------------------------------------------------- 1. batch split
def test_batch_split_gives_the_recorded_compositions():
    from lsenerf_amd.data import batch_split
    assert batch_split(3512, 0.66, "deblur") == (579, 597)          # 2316 colour rays
    assert batch_split(3512, 0.66, "mse") == (2318, 597)
    assert batch_split(3512, 1.0, "deblur") == (878, 0)
    assert batch_split(3512, 0.66, "DEBLUR") == (579, 597)


# ---------------------------------------------------------------------------------------------------- 2. C-ABI surface
def test_header_library_and_binding_carry_the_composer_entry_points():
    from lsenerf_amd import _lib
    with open(os.path.join(ROOT, "include", "lse_hip.h")) as fh:
        header = fh.read()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (lse_\w+)", nm))
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
    assert "typedef struct lse_compose_desc" in header
    lib = _lib.load()
    assert lib.lse_abi_version() == 6 == _lib.LSE_ABI_VERSION
    assert int(re.search(r"#define LSE_ABI_VERSION (\d+)", header).group(1)) == 6


def test_binding_structs_have_the_layout_the_header_declares():
    """The ctypes mirrors against the C compiler's view of include/lse_hip.h (sizes and a probe field per struct)."""
    import shutil
    import tempfile
    from lsenerf_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    assert cc is not None, "the build needs a C compiler anyway (oracle/c)"
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "lse_hip.h"\nint main(void){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n",' \
          "sizeof(lse_compose_stream), sizeof(lse_compose_desc), sizeof(lse_compose_scene), sizeof(lse_compose_out)," \
          "offsetof(lse_compose_desc, seed), offsetof(lse_compose_scene, next_pose), offsetof(lse_compose_out, ray_px)," \
          "offsetof(lse_compose_out, evs_batch_appearance_id));return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "p.c"), "w") as fh:
            fh.write(src)
        subprocess.run([cc, "-I", os.path.join(ROOT, "include"), os.path.join(d, "p.c"), "-o", os.path.join(d, "p")], check=True)
        got = [int(v) for v in subprocess.run([os.path.join(d, "p")], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(_lib.ComposeStream), ctypes.sizeof(_lib.ComposeDesc), ctypes.sizeof(_lib.ComposeScene),
            ctypes.sizeof(_lib.ComposeOut), _lib.ComposeDesc.seed.offset, _lib.ComposeScene.next_pose.offset,
            _lib.ComposeOut.ray_px.offset, _lib.ComposeOut.evs_batch_appearance_id.offset]
    assert got == want


# ---------------------------------------------------------------------------------------------------- 3. the draw's host twin
def _philox_reference(ctr, key):
    """Philox4x32-10 in plain Python integers (Salmon et al., SC'11; Random123 philox.h)."""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_core_reproduces_the_published_vectors(ctr, key, want):
    from lsenerf_amd.data import philox4x32_10
    assert tuple(_philox_reference(ctr, key)) == want
    assert tuple(int(v) for v in philox4x32_10(np.array(ctr, dtype=np.uint32), key)) == want
    both = philox4x32_10(np.array([ctr, (1, 2, 3, 4)], dtype=np.uint32), key)          # vectorised over counters
    assert tuple(int(v) for v in both[0]) == want and [int(v) for v in both[1]] == _philox_reference((1, 2, 3, 4), key)


def test_host_draw_is_in_range_reproducible_and_distinct_per_step_and_stream():
    from lsenerf_amd.data import draw_indices_host
    seed = 2 ** 40 + 7
    a = draw_indices_host(seed, 5, 0, 3512, 7, 36, 48)
    assert a.shape == (3512, 3) and a.dtype == np.int64
    assert a.min() >= 0 and (a.max(0) < np.array([7, 36, 48])).all() and (a.max(0) == np.array([6, 35, 47])).all()
    assert np.array_equal(a, draw_indices_host(seed, 5, 0, 3512, 7, 36, 48))
    assert np.array_equal(a[:100], draw_indices_host(seed, 5, 0, 100, 7, 36, 48))       # pixel i does not depend on the batch size
    for other in (draw_indices_host(seed, 6, 0, 3512, 7, 36, 48), draw_indices_host(seed, 5, 1, 3512, 7, 36, 48),
                  draw_indices_host(seed + 1, 5, 0, 3512, 7, 36, 48), draw_indices_host(seed + 2 ** 32, 5, 0, 3512, 7, 36, 48)):
        assert (other != a).any(1).mean() > 0.99
    assert np.array_equal(a, draw_indices_host(seed, 5 + 2 ** 32, 0, 3512, 7, 36, 48))  # the low 32 bits of the step enter
    # pixel i of the draw, word by word, from the scalar restatement
    w = _philox_reference((5, 17, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    assert a[17].tolist() == [(w[0] * 7) >> 32, (w[1] * 36) >> 32, (w[2] * 48) >> 32]


@pytest.mark.parametrize("seed", [0, 96, 12345, 2 ** 40 + 7])
@pytest.mark.parametrize("stream", [0, 1])
def test_host_draw_is_uniform_over_images_and_pixels(seed, stream):
    """8 images of 36 x 48, 64 steps x 3512 draws, K = 128 bins (camera x quarter of the rows x quarter of the columns; 1756
    expected per bin).  Bound: mean + 6 sigma of a chi-square with K - 1 = 127 degrees of freedom = 127 + 6 sqrt(254) = 222.6
    (the draw is deterministic: this cannot flake).  Measured with this convention: 95 - 148 over these eight cases."""
    from lsenerf_amd.data import draw_indices_host
    K = 128
    counts = np.zeros(K)
    for step in range(64):
        i = draw_indices_host(seed, step, stream, 3512, 8, 36, 48)
        counts += np.bincount(i[:, 0] * 16 + (i[:, 1] // 9) * 4 + i[:, 2] // 12, minlength=K)
    expected = 64 * 3512 / K
    chi2 = float(((counts - expected) ** 2 / expected).sum())
    print(f"seed {seed} stream {stream}: chi-square {chi2:.1f}")
    assert chi2 <= (K - 1) + 6 * np.sqrt(2 * (K - 1))


# ---------------------------------------------------------------------------------------------------- 4. pose tables
def _rays_from_table(cameras, table, slots, idx, repeat=1):
    """EdCameras.generate_rays with get_c2w_fn = table[slot]."""
    old = cameras.get_c2w_fn
    cameras.get_c2w_fn = lambda ci: table.reshape(-1, 3, 4)[slots]
    try:
        return cameras.generate_rays(idx[:, :1].repeat_interleave(repeat, 0), idx[:, 1:].float().repeat_interleave(repeat, 0))
    finally:
        cameras.get_c2w_fn = old


def _close(a, b, bar=1e-5):
    for name in ("origins", "directions", "pixel_area"):
        err = float((getattr(a, name) - getattr(b, name)).abs().max())
        assert err < bar, (name, err)


@pytest.mark.parametrize("distort", [False, True])
def test_pose_tables_reproduce_the_ray_generators(tmp_path, distort):
    """Rays from RayGenerator (+ CameraOptimizer.apply_to_raybundle), ConsecRayGenerator, PrevNextRayGenerator and
    DeblurRayGenerator equal EdCameras.generate_rays reading ``table[slot]``, within the bar tests/test_cameras_cpu.py uses for
    pose maths (1e-5)."""
    from lsenerf_amd import cameras as cam
    from lsenerf_amd.data import camera_tables, spline_tables
    col_ds, evs_ds = make_scene(tmp_path, distort=distort, prevnext=True)
    col_idx = random_indices(64, N_COL, COL_HW, 1)
    evs_idx = random_indices(64, N_FRAMES - 1, EVS_HW, 2)
    cams = col_ds.cameras
    # plain cameras, then with a CameraOptimizer's corrections
    _close(cam.RayGenerator(cams)(col_idx), _rays_from_table(cams, camera_tables(cams), col_idx[:, 0], col_idx))
    opt = cam.CameraOptimizerConfig(mode="SO3xR3").setup(num_cameras=N_COL, device="cpu")
    with torch.no_grad():
        opt.pose_adjustment.copy_(torch.randn(N_COL, 6, generator=torch.Generator().manual_seed(3)) * 0.05)
    rb = cam.RayGenerator(cams)(col_idx)
    opt.apply_to_raybundle(rb)
    got = _rays_from_table(cams, camera_tables(cams, opt), col_idx[:, 0], col_idx)
    assert float((rb.origins - got.origins).abs().max()) < 1e-5 and float((rb.directions - got.directions).abs().max()) < 1e-5
    # consecutive event cameras: one table, read at c and c + 1
    ecams = evs_ds.cameras
    prev, nxt = cam.ConsecRayGenerator(ecams)(evs_idx)
    _close(prev, _rays_from_table(ecams, camera_tables(ecams), evs_idx[:, 0], evs_idx))
    _close(nxt, _rays_from_table(ecams, camera_tables(ecams), evs_idx[:, 0] + 1, evs_idx))
    # previous / next camera sets: two tables, both read at c
    pc, nc = evs_ds.out.prev_cameras, evs_ds.out.next_cameras
    prev, nxt = cam.PrevNextRayGenerator(pc, nc)(evs_idx)
    _close(prev, _rays_from_table(pc, camera_tables(pc), evs_idx[:, 0], evs_idx))
    _close(nxt, _rays_from_table(nc, camera_tables(nc), evs_idx[:, 0], evs_idx))
    # the spline: rgb / evs cameras at the cameras' times, and the four deblur cameras of every exposure
    spl = cam.CameraOptimizerConfig(mode="SO3xR3", optim_type="spline", exp_t=0.3).setup(
        num_cameras=N_COL, device="cpu", cameras=cams, dM=torch.eye(4))
    cams.set_interpolator(spl)
    rb = cam.DeblurRayGenerator(cams)(col_idx)
    cams.set_interpolator(None)
    table = spline_tables(spl, cams, "deblur")
    assert table.shape == (N_COL, 4, 3, 4) and table.requires_grad
    slots = (col_idx[:, :1] * 4 + torch.arange(4)[None]).reshape(-1)
    _close(rb, _rays_from_table(cams, table, slots, col_idx, repeat=4))
    assert float((spline_tables(spl, cams, "rgb") - spl.get_rgb_cameras(cams.times)).abs().max()) == 0.0
    assert spline_tables(spl, cams, "evs").shape == (N_COL, 3, 4)


def test_closest_colour_camera_table_follows_camera_idx_fixer():
    """Both ends, an exact tie (the later camera wins: `prev < cur` is strict) and interior times."""
    from lsenerf_amd.data import find_closest_idxs as product
    ref, srch = torch.tensor(COL_TIMES), torch.tensor(EVS_TIMES)
    want = [0, 1, 1, 2, 2, 3, 4, 5, 5, 5]           # 0.5 ties between cameras 0 and 1 -> 1; 1.5 -> 2; 3.5 -> 4
    assert product(ref, srch).tolist() == want == find_closest_idxs(ref, srch).tolist()
