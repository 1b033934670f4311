"""tests/analytic_scene.py against brute force: the closed forms a trained field is held to (tests/test_gpu_analytic_scene.py) are a
dozen lines of ray-sphere and ray-box algebra, and this file is where they are checked -- by marching, by finite differences, and,
in ONE test, against the project's own ray generator.  It also holds the conditions the GPU tests rely on."""
import numpy as np
import torch

from tests import analytic_scene as sc


def _random_rays(n, seed):
    """Rays from eyes on a shell of radius 1.8 .. 2.5 towards points of the cube [-0.9, 0.9]^3: about half of them hit."""
    rng = np.random.default_rng(seed)
    eye = rng.normal(size=(n, 3))
    eye *= (rng.uniform(1.8, 2.5, n) / np.linalg.norm(eye, axis=-1))[:, None]
    d = rng.uniform(-0.9, 0.9, (n, 3)) - eye
    return eye, d / np.linalg.norm(d, axis=-1, keepdims=True)


def test_trace_equals_marching_and_bisection():
    o, d = _random_rays(240, 1)
    t, _, _, body = sc.trace(o, d)
    step = 1e-4
    ts = np.arange(0.0, 4.5, step)
    hits = grazing = 0
    for r in range(len(o)):
        s = sc.sdf(o[r] + ts[:, None] * d[r])
        inside = np.flatnonzero(s <= 0)
        if s.min() > step:                                   # never within a step of a surface: a miss, whatever the sampling
            assert not np.isfinite(t[r]) and body[r] == sc.BODY_NONE, r
            continue
        if inside.size == 0 or s.min() > -step:              # closest approach within 1e-4 of a surface: not decided by marching
            grazing += 1
            continue
        a, b = ts[inside[0] - 1], ts[inside[0]]              # sdf(a) > 0 >= sdf(b)
        for _ in range(60):
            m = 0.5 * (a + b)
            if sc.sdf(o[r] + m * d[r])[0] > 0:
                a = m
            else:
                b = m
        assert abs(t[r] - b) < 1e-6, (r, t[r], b)
        hits += 1
    assert hits > 60 and len(o) - hits - grazing > 60 and grazing < 10, (hits, grazing)
    hit = np.isfinite(t)
    p = o[hit] + t[hit, None] * d[hit]
    assert np.abs(sc.sdf(p)).max() < 1e-12
    # the body is the one whose own distance vanishes there
    assert np.abs(np.where(body[hit] == sc.BODY_SPHERE, sc._sdf_sphere(p), sc._sdf_box(p))).max() < 1e-12


def test_outward_normal_is_the_gradient_of_the_distance():
    rng = np.random.default_rng(2)
    p = rng.uniform(-1, 1, (20000, 3))
    # away from where the distance has a kink: the medial surface between the bodies, the sphere's centre, the planes through the
    # box faces (where the nearest box feature changes between face, edge and corner) and the box's inner medial axis
    ds, db = sc._sdf_sphere(p), sc._sdf_box(p)
    q = np.abs(p - 0.5 * (sc.BOX_LO + sc.BOX_HI)) - 0.5 * (sc.BOX_HI - sc.BOX_LO)
    qs = np.sort(q, axis=-1)
    keep = (np.abs(ds - db) > 1e-2) & (np.linalg.norm(p - sc.SPHERE_C, axis=-1) > 1e-2)
    keep &= (ds < db) | ((np.abs(q) > 1e-2).all(-1) & ((qs[:, 2] > 0) | (qs[:, 2] - qs[:, 1] > 1e-2)))
    p = p[keep]
    assert len(p) > 15000 and int((sc._sdf_box(p) < sc._sdf_sphere(p)).sum()) > 3000
    h = 1e-6
    g = np.stack([(sc.sdf(p + h * e) - sc.sdf(p - h * e)) / (2 * h) for e in np.eye(3)], -1)
    n = sc.outward_normal(p)
    assert np.abs(g - n).max() < 1e-6
    assert np.abs(np.linalg.norm(n, axis=-1) - 1).max() < 1e-12


def test_hit_normals_are_unit_and_face_the_camera_and_colours_follow_the_body():
    for cams in (sc.train_cameras(), sc.heldout_cameras(), sc.trajectory_cameras()):
        for c2w in cams:
            o, d = sc.pixel_rays(c2w)
            t, col, n, body = sc.trace(o, d)
            hit = body != sc.BODY_NONE
            assert np.array_equal(hit, np.isfinite(t))
            assert np.abs(np.linalg.norm(n[hit], axis=-1) - 1).max() < 1e-9 and (n[~hit] == 0).all()
            assert ((n[hit] * d[hit]).sum(-1) < 0).all()
            p = o[hit] + t[hit, None] * d[hit]
            assert ((sc.outward_normal(p) * n[hit]).sum(-1) > 1 - 1e-6).mean() > 0.99       # (all but pixels that land on a box edge)
            assert (col[~hit] == 1.0).all() and col.min() >= 0.09 and col.max() <= 1.0
            s = body == sc.BODY_SPHERE
            assert np.allclose(col[s], 0.5 + 0.4 * n[s], atol=1e-12)
            assert np.allclose(col[hit], sc.surface_colour(p), atol=1e-6)
            b = body == sc.BODY_BOX
            if b.any():
                assert all(any(np.array_equal(c, f) for f in sc.BOX_COLOURS) for c in np.unique(col[b], axis=0))
    assert len({tuple(c) for c in sc.BOX_COLOURS}) == 6


def test_the_bodies_are_asymmetric_apart_and_inside_the_cube():
    lo = np.minimum(sc.SPHERE_C - sc.SPHERE_R, sc.BOX_LO)
    hi = np.maximum(sc.SPHERE_C + sc.SPHERE_R, sc.BOX_HI)
    assert (lo > -1).all() and (hi < 1).all()
    assert sc._sdf_box(sc.SPHERE_C[None])[0] > sc.SPHERE_R + 0.05                       # the two do not touch
    # an axis swap or a sign flip moves the geometry by much more than any depth bar: the signed distance changes by > 0.2 somewhere
    pts, _, _ = sc.surface_samples(600)
    import itertools
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((1, -1), repeat=3):
            if perm == (0, 1, 2) and signs == (1, 1, 1):
                continue
            moved = pts[:, perm] * np.asarray(signs)
            assert np.abs(sc.sdf(moved)).max() > 0.2, (perm, signs)


def test_surface_samples_lie_on_the_surface_with_its_normals():
    p, n, body = sc.surface_samples(1500)
    assert np.abs(sc.sdf(p)).max() < 1e-12
    assert np.abs((sc.outward_normal(p + 1e-9 * n) * n).sum(-1) - 1).max() < 1e-6
    assert (body == sc.BODY_SPHERE).sum() == 1500 and (body == sc.BODY_BOX).sum() >= 1400
    t, _, nrm, seen = sc.trace(p + 0.02 * n, -n)              # from 0.02 above (less than the gap between the bodies), looking back
    assert np.array_equal(seen, body) and np.abs(t - 0.02).max() < 1e-12 and np.abs(nrm - n).max() < 1e-9


def test_rays_equal_the_projects_generator_for_one_camera():
    """The single place where the helper's rays and the project's are tied together, at the bar of tests/test_cameras_cpu.py."""
    from lsenerf_amd.cameras import EdCameras
    c2w = sc.heldout_cameras()[1]
    cams = EdCameras(torch.from_numpy(c2w[None]), fx=sc.FX, fy=sc.FY, cx=sc.CX, cy=sc.CY, width=sc.W, height=sc.H)
    coords = cams.get_image_coords().reshape(-1, 2)
    rb = cams.generate_rays(torch.zeros(len(coords), dtype=torch.long), coords)
    o, d = sc.pixel_rays(c2w)
    assert np.abs(rb.origins.numpy() - o).max() < 1e-5 and np.abs(rb.directions.numpy() - d).max() < 1e-5
    # and a subset of pixels is the same rows of the whole image
    ys, xs = np.array([0, 5, 47]), np.array([63, 0, 31])
    o2, d2 = sc.pixel_rays(c2w, ys, xs)
    assert np.array_equal(d2, d[ys * sc.W + xs]) and np.array_equal(o2, o[ys * sc.W + xs])
    # the optical axis is the centre pixel's ray
    assert np.allclose(sc.pixel_rays(c2w, [sc.CY], [sc.CX])[1][0], sc.optical_axis(c2w), atol=1e-12)


def test_look_at_is_a_rotation_that_looks_at_the_target():
    for c2w in np.concatenate([sc.train_cameras(), sc.heldout_cameras(), sc.trajectory_cameras()]):
        R = c2w[:, :3]
        assert np.allclose(R.T @ R, np.eye(3), atol=1e-12) and np.linalg.det(R) > 0.999
        eye = c2w[:, 3]
        assert np.allclose(sc.optical_axis(c2w), -eye / np.linalg.norm(eye), atol=1e-12)
        assert R[2, 1] > 0                                   # the camera's up has a positive world z
    r = np.linalg.norm(sc.train_cameras()[:, :, 3], axis=-1)
    assert np.allclose(r, 2.2) and len(r) == 24
    r = np.linalg.norm(sc.heldout_cameras()[:, :, 3], axis=-1)
    assert r.min() >= 2.0 - 1e-12 and r.max() <= 2.4 + 1e-12 and len(r) == 4
    # no held-out direction is a training direction, and trajectory poses are a few degrees apart
    unit = lambda c: c[:, :, 3] / np.linalg.norm(c[:, :, 3], axis=-1, keepdims=True)
    assert (unit(sc.heldout_cameras()) @ unit(sc.train_cameras()).T).max() < np.cos(np.deg2rad(8))
    traj = unit(sc.trajectory_cameras())
    ang = np.degrees(np.arccos((traj[1:] * traj[:-1]).sum(-1)))
    assert len(traj) == 8 and ang.min() > 1 and ang.max() < 5


def test_interior_is_the_three_by_three_same_state_mask():
    m = np.zeros((6, 7), int)
    m[2:5, 2:6] = 1
    m[0, 0] = 2
    got = sc.interior(m)
    want = np.zeros_like(got)
    for y in range(6):
        for x in range(7):
            nb = m[max(y - 1, 0):y + 2, max(x - 1, 0):x + 2]
            want[y, x] = (nb == m[y, x]).all()
    assert np.array_equal(got, want) and got[3, 3] and not got[2, 2] and not got[1, 1] and got[5, 0]
    assert np.array_equal(sc.interior(np.stack([m, m.T[:6, :6].repeat(2, 1)[:, :7]]))[0], got)


def test_images_and_event_frames_follow_their_definitions():
    traj = sc.trajectory_cameras()
    im = sc.images(traj)
    assert im["rgb8"].dtype == np.uint8 and im["rgb8"].shape == (8, sc.H, sc.W, 3)
    assert np.array_equal(im["rgb8"], np.rint(255 * im["rgb"]).astype(np.uint8))
    assert np.array_equal(im["hit"], np.isfinite(im["t"]))
    c = sc.CONFIG["event_threshold"]
    fr = sc.event_frames(im["rgb8"] / 255.0, c)
    gray = (im["rgb8"] / 255.0) @ np.array([0.2989, 0.5870, 0.1140])
    assert fr.shape == (7, sc.H, sc.W)
    assert np.allclose(fr, (np.log(gray[1:] + 1e-6) - np.log(gray[:-1] + 1e-6)) / c, atol=1e-12)
    # the frames have enough strong pixels of both polarities for a sign test to mean something
    assert (fr >= 2).mean() > 0.005 and (fr <= -2).mean() > 0.005
    # a pixel that leaves the background for a body darkens: a negative event
    entered = ~im["hit"][:-1] & im["hit"][1:]
    assert (fr[entered] < 0).all()


def test_the_conditions_the_gpu_tests_rely_on():
    held = sc.images(sc.heldout_cameras())
    both = 0
    for v in range(4):
        share = sc.interior(held["body"][v]).mean()
        assert share >= 0.8, (v, share)
        assert sc.interior(held["hit"][v]).mean() >= share                      # (the body map is the stricter of the two)
        vis = [(held["body"][v] == b).sum() for b in (sc.BODY_SPHERE, sc.BODY_BOX)]
        both += min(vis) >= 100
        assert held["hit"][v].mean() > 0.15
    assert both >= 3
    train = sc.images(sc.train_cameras())
    assert 0.25 <= train["hit"].mean() <= 0.5, train["hit"].mean()
    # every ray of every camera crosses the cube the field lives in, so no pixel is outside the sampler's reach
    for c2w in np.concatenate([sc.train_cameras(), sc.heldout_cameras(), sc.trajectory_cameras()]):
        o, d = sc.pixel_rays(c2w)
        t, _, _, _ = sc.trace(o, d)
        assert np.nanmax(np.where(np.isfinite(t), t, np.nan)) < np.linalg.norm(c2w[:, 3]) + 1.0
    assert abs(sc.CONFIG["height"] - sc.H) + abs(sc.CONFIG["width"] - sc.W) == 0
    assert sc.CONFIG["n_train"] == 24 and sc.CONFIG["n_heldout"] == 4 and sc.CONFIG["n_trajectory"] == 8


def test_the_committed_fixture_was_made_with_this_configuration():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "analytic_scene_oracle.json")
    with open(path) as f:
        doc = json.load(f)
    want = {k: (list(v) if isinstance(v, tuple) else v) for k, v in sc.CONFIG.items()}
    assert doc["config"] == want
    on = doc["runs"]["contraction_on"]
    assert sorted(on) == sorted(str(s) for s in sc.CONFIG["init_seeds"])
    for runs in doc["runs"].values():
        for run in runs.values():
            assert len(run["views"]) == 4
            for view in run["views"]:                        # every oracle seed separates hit from miss on every interior pixel
                assert view["separated"] == 1.0 and view["interior_share"] >= 0.8
    assert os.path.getsize(path) < 64 * 1024
