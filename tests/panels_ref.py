"""numpy twin of lsenerf_amd/csrc/panels.hip for the tests: the 8-bit grey, Canny's classification (OpenCV's published
``Canny(image, low, high, apertureSize=3, L2gradient=False)`` up to the hysteresis), the hysteresis in two independent formulations
and the uint8 panel grid, in float32 with one rounding per operation.  Plus the fixtures both test files share.  OpenCV is not a
dependency: parity with cv2 is unpinned, the twin restates the algorithm as include/lse_hip.h words it."""
import numpy as np

F = np.float32
TILE = 32                                    # the Canny kernels' tile edge (csrc/panels.hip kTile): fixtures cross its borders
PANEL_KEYS = ("img", "depth", "err_map", "overlay", "ev_out")


def to_u8(v):
    """(uint8) trunc(min(max(v * 255, 0), 255)); a NaN gives 0 (numpy's own cast of a NaN is undefined, so it is replaced first)."""
    v = np.asarray(v, dtype=F) * F(255.0)
    with np.errstate(invalid="ignore"):
        v = np.where(np.isnan(v), F(0.0), np.minimum(np.maximum(v, F(0.0)), F(255.0)))
    return v.astype(np.uint8)


def gray3(planes):
    p = np.asarray(planes, dtype=F).reshape(3, *np.shape(planes)[-2:])
    return (p[0] * F(0.2989) + p[1] * F(0.5870)) + p[2] * F(0.1140)


def gray8(planes):
    """uint8 [H, W] of float32 planes [3, H, W]: the grey of lse_eval_image_prep, each operation rounded."""
    return to_u8(gray3(planes))


def sobel_mag(gray_u8):
    """(dx, dy, mag) int32 [H, W]: 3 x 3 Sobel with a replicated border, mag = |dx| + |dy|."""
    g = np.pad(np.asarray(gray_u8).astype(np.int32), 1, mode="edge")
    H, W = g.shape[0] - 2, g.shape[1] - 2
    w = lambda dy, dx: g[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    dx = (w(-1, 1) + 2 * w(0, 1) + w(1, 1)) - (w(-1, -1) + 2 * w(0, -1) + w(1, -1))
    dy = (w(1, -1) + 2 * w(1, 0) + w(1, 1)) - (w(-1, -1) + 2 * w(-1, 0) + w(-1, 1))
    return dx, dy, np.abs(dx) + np.abs(dy)


def canny_classify(gray_u8, low=50, high=200, branches=None):
    """Class map uint8 [H, W]: 0 none, 1 weak, 2 strong.  ``branches``: a dict that receives, over the candidates (mag > low), the
    counts of the three non-maximum-suppression directions and of both diagonal signs."""
    low, high = int(np.floor(low)), int(np.floor(high))
    if low > high:
        low, high = high, low
    dx, dy, mag = sobel_mag(gray_u8)
    H, W = mag.shape
    m = np.pad(mag, 1)                                   # 0 outside the image
    at = lambda oy, ox: m[1 + oy:1 + oy + H, 1 + ox:1 + ox + W]
    x = np.abs(dx).astype(np.int64)
    y = np.abs(dy).astype(np.int64) << 15
    tg22x = x * 13573
    tg67x = tg22x + (x << 16)
    horiz = y < tg22x
    vert = ~horiz & (y > tg67x)
    diag = ~horiz & ~vert
    neg = (dx ^ dy) < 0                                  # s = -1
    pass_h = (mag > at(0, -1)) & (mag >= at(0, 1))
    pass_v = (mag > at(-1, 0)) & (mag >= at(1, 0))
    pass_dp = (mag > at(-1, -1)) & (mag > at(1, 1))      # s = +1: up-left and down-right
    pass_dn = (mag > at(-1, 1)) & (mag > at(1, -1))      # s = -1: up-right and down-left
    ok = np.where(horiz, pass_h, np.where(vert, pass_v, np.where(neg, pass_dn, pass_dp)))
    cand = mag > low
    if branches is not None:
        for name, sel in (("horizontal", horiz), ("vertical", vert), ("diagonal_pos", diag & ~neg), ("diagonal_neg", diag & neg)):
            branches[name] = branches.get(name, 0) + int((cand & sel).sum())
    cls = np.zeros((H, W), dtype=np.uint8)
    cls[cand & ok] = 1
    cls[cand & ok & (mag > high)] = 2
    return cls


def hysteresis_flood(cls):
    """OpenCV's formulation: a stack flood from the strong pixels through their 8-neighbours that are weak."""
    cls = np.asarray(cls)
    H, W = cls.shape
    edge = cls == 2
    stack = [tuple(p) for p in np.argwhere(edge)]
    while stack:
        y, x = stack.pop()
        for ny in range(max(y - 1, 0), min(y + 2, H)):
            for nx in range(max(x - 1, 0), min(x + 2, W)):
                if cls[ny, nx] == 1 and not edge[ny, nx]:
                    edge[ny, nx] = True
                    stack.append((ny, nx))
    return edge.astype(np.uint8) * 255


def hysteresis_label(cls):
    """Connected components (8-connected) of the candidates; a component is an edge iff it holds a strong pixel."""
    from scipy import ndimage
    cls = np.asarray(cls)
    lab, n = ndimage.label(cls > 0, structure=np.ones((3, 3), dtype=bool))
    strong = np.zeros(n + 1, dtype=bool)
    strong[np.unique(lab[cls == 2])] = True
    strong[0] = False
    return strong[lab].astype(np.uint8) * 255


def canny(gray_u8, low=50, high=200):
    return hysteresis_label(canny_classify(gray_u8, low, high))


def panel_columns(keys):
    return sum(2 if k == "img" else 1 for k in PANEL_KEYS if k in keys)


def _clip01(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, F(0), np.where(x > 1, F(1), x)).astype(F)          # a NaN stays


def panel_values(keys, gt_planes=None, pred_planes=None, rgb=None, pair=None, depth=None, acc=None, edges=None, ev_out=None):
    """{key: float32 [H, W or 2 W, 3]} of the float panels ("overlay": uint8 already), every operation a float32 one."""
    out = {}
    three = lambda a: np.repeat(np.asarray(a, dtype=F)[..., None], 3, axis=-1)
    if "img" in keys:
        if pair is not None:
            left, right = three(np.asarray(pair[0]).reshape(np.shape(pair[0])[-2:])), three(np.asarray(pair[1]).reshape(np.shape(pair[1])[-2:]))
        else:
            left = np.moveaxis(np.asarray(gt_planes, dtype=F).reshape(3, *np.shape(gt_planes)[-2:]), 0, -1)
            right = np.asarray(rgb, dtype=F).reshape(*left.shape)
        out["img"] = np.concatenate([left, right], axis=1)
    if "depth" in keys:
        d, a = np.asarray(depth, dtype=F), np.asarray(acc, dtype=F)
        d, a = d.reshape(d.shape[:2]), a.reshape(a.shape[:2])
        near, far = d.min(), d.max()                          # numpy's min / max hand a NaN on, as torch's do
        with np.errstate(invalid="ignore", divide="ignore"):
            v = _clip01((d - near) / ((far - near) + F(1e-10)))
            out["depth"] = three((F(1) - _clip01(v)) * a + (F(1) - a))
    if "err_map" in keys:
        err = (gray3(gt_planes) - gray3(pred_planes)) * F(6.0)
        one = np.ones_like(err)
        pos, neg = err > 0, err < 0
        r = np.where(neg, F(1) - np.abs(err), one)
        g = np.where(pos, F(1) - err, np.where(neg, F(1) - np.abs(err), one))
        b = np.where(pos, F(1) - err, one)
        out["err_map"] = np.stack([r, g, b], axis=-1).astype(F)
    if "overlay" in keys:
        ge, pe = np.asarray(edges[0]) != 0, np.asarray(edges[1]) != 0
        o = np.full((*ge.shape, 3), 255, dtype=np.uint8)
        o[ge | pe] = 0
        o[ge, 0] = 255
        o[pe, 2] = 255
        out["overlay"] = o
    if "ev_out" in keys:
        e = np.asarray(ev_out, dtype=F)
        out["ev_out"] = e if e.shape[-1] == 3 else np.repeat(e, 3, axis=-1)
    return out


def panels(keys, **inputs):
    """uint8 [H, columns * W, 3]: the grid of lse_eval_panels."""
    vals = panel_values(keys, **inputs)
    return np.concatenate([vals[k] if k == "overlay" else to_u8(vals[k]) for k in PANEL_KEYS if k in keys], axis=1)


# ---------------------------------------------------------------------------------------------------- fixtures: images
def step_image(H, W, vertical=True, height=255, at=None):
    """0 | height: a vertical step (columns < at dark) or a horizontal one (rows < at dark)."""
    img = np.zeros((H, W), dtype=np.uint8)
    if vertical:
        img[:, (W // 2 if at is None else at):] = height
    else:
        img[(H // 2 if at is None else at):, :] = height
    return img


def box_blur(img, radius):
    if radius == 0:
        return img.copy()
    k = 2 * radius + 1
    g = np.pad(img.astype(np.int64), radius, mode="edge")
    H, W = img.shape
    s = sum(g[dy:dy + H, dx:dx + W] for dy in range(k) for dx in range(k))
    return (s // (k * k)).astype(np.uint8)


def noise_image(H, W, radius, seed=0):
    rng = np.random.default_rng(1000 * seed + 10 * radius + H * W)
    return box_blur(rng.integers(0, 256, (H, W), dtype=np.uint8), radius)


def ramp_image(H, W, sx, sy, slope=6):
    """A diagonal band: clip(128 + slope (sx (x - W/2) + sy (y - H/2)), 0, 255); dx has the sign of sx, dy that of sy."""
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(128 + slope * (sx * (x - W // 2) + sy * (y - H // 2)), 0, 255).astype(np.uint8)


def classify_fixtures(H, W):
    """[(name, uint8 image)]: the steps, blurred noise at three radii, a diagonal ramp per sign combination of dx, dy."""
    out = [("vstep", step_image(H, W, True)), ("hstep", step_image(H, W, False)), ("const", np.full((H, W), 77, dtype=np.uint8)),
           ("vstep12", step_image(H, W, True, 12)), ("vstep13", step_image(H, W, True, 13))]
    out += [(f"noise{r}", noise_image(H, W, r)) for r in (0, 1, 3)]
    out += [(f"ramp{sx:+d}{sy:+d}", ramp_image(H, W, sx, sy)) for sx in (1, -1) for sy in (1, -1)]
    return out


# ---------------------------------------------------------------------------------------------------- fixtures: class maps
def spiral_map(H, W, seeded=True):
    """A one-pixel weak spiral from the corner inwards, arms two pixels apart (never 8-adjacent); ``seeded``: its inner end is
    strong.  Returns (map, length)."""
    m = np.zeros((H, W), dtype=np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = 1
    n = 1
    inside = lambda a, b: 0 <= a < H and 0 <= b < W
    while True:
        for _ in range(2):
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if inside(ny, nx) and not m[ny, nx] and not (inside(ny2, nx2) and m[ny2, nx2]):
                y, x = ny, nx
                m[y, x] = 1
                n += 1
                break
            dy, dx = dx, -dy                     # turn right
        else:
            break
    if seeded:
        m[y, x] = 2
    return m, n


def corner_blobs_map(H, W):
    """Weak 4 x 4 (or smaller) blobs that touch only diagonally across a tile corner: one pair on the diagonal, seeded in the far
    corner of the lower blob; one on the anti-diagonal, not seeded.  Returns (map, mask of what must become an edge)."""
    m = np.zeros((H, W), dtype=np.uint8)
    cy, cx = min(TILE, H // 2), min(TILE, W // 3)
    m[max(cy - 4, 0):cy, max(cx - 4, 0):cx] = 1
    m[cy:cy + 4, cx:cx + 4] = 1
    want = m > 0
    m[min(cy + 3, H - 1), min(cx + 3, W - 1)] = 2
    cx2 = min(2 * TILE, 2 * (W // 3) + 1)
    if cx2 - 1 > cx + 4:                          # the unseeded pair, clear of the first
        m[max(cy - 4, 0):cy, cx2:cx2 + 4] = 1
        m[cy:cy + 4, max(cx2 - 4, cx + 6):cx2] = 1
    return m, want


def border_map(H, W, seeded=True):
    """Weak pixels on all four image borders (the corners included), one strong pixel in the last corner."""
    m = np.zeros((H, W), dtype=np.uint8)
    m[0, :] = m[-1, :] = 1
    m[:, 0] = m[:, -1] = 1
    if seeded:
        m[-1, -1] = 2
    return m


def random_map(H, W, density, strong=0.01, seed=0):
    rng = np.random.default_rng(seed + int(density * 100) + 7 * H * W)
    u = rng.random((H, W))
    m = (u < density).astype(np.uint8)
    m[rng.random((H, W)) < strong] = 2
    return m


def hysteresis_fixtures(H, W):
    """[(name, class map)]."""
    out = [("spiral", spiral_map(H, W, True)[0]), ("spiral_unseeded", spiral_map(H, W, False)[0]),
           ("corner_blobs", corner_blobs_map(H, W)[0]), ("borders", border_map(H, W)), ("borders_unseeded", border_map(H, W, False)),
           ("all_strong", np.full((H, W), 2, dtype=np.uint8)), ("all_weak", np.ones((H, W), dtype=np.uint8))]
    out += [(f"random{d}", random_map(H, W, d)) for d in (0.1, 0.4, 0.9)]
    return out
