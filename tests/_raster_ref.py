"""NumPy restatement of the forward 3DGS rasteriser's rules (include/pixie_hip.h, section D) with a `dtype` argument: the yardstick of
the rasteriser tests on both sides (CPU: raster_math.h built for the host; GPU: the kernels).

It is neither tiled nor sorted.  Per pixel it takes the Gaussians whose tile rectangle contains the pixel's tile, in (depth, index)
order, and blends them front to back.  Run in float64 it is the reference result; run in float32 it is the yardstick: its distance
from the float64 run says what float32 evaluation of this algorithm costs on a scene.

The float64 run also returns the BORDERLINE sets.  A Gaussian is borderline when a decision of its projection sits within
EPS = 64 * 2^-24 (relative) of its threshold: p_view.z against 0.2, det against 0, 3 sqrt(lambda) against an integer, an edge of
its rectangle against a tile boundary.  A pixel is borderline when a decision that shapes it does: alpha against 1/255,
T (1 - alpha) against 1e-4 (both with the tolerance scaled by 1 + mag, mag = the sum of the magnitudes of power's terms: power's
rounding error is relative to that sum, and alpha = o exp(power) carries it as a relative error), power against 0 away from the
centre, two Gaussians that both contribute to it with depths closer than EPS, or a borderline Gaussian that would contribute to it (looked for one tile beyond its rectangle as well; a Gaussian
borderline at the near plane or in det marks every pixel).  Comparisons are made off these sets: on them a float32 evaluation may
legitimately take the other branch.

The scene generators of the tests live here too (seeded; no fixture files).
"""
import numpy as np

EPS = 64.0 * 2.0 ** -24
# What the float32 yardstick y of a scene may be at most.  A pixel is at most 1 and is a sum of weights alpha T that add up to at most
# 1; each alpha carries power's rounding error, a few 2^-24 times (1 + mag) with mag up to ~10 where alpha >= 1/255, i.e. ~1e-6
# relative, and the conic's conditioning can cost an order of magnitude more for the large near-camera Gaussians.  A y beyond
# 2e-5 therefore means a decision flipped between the float32 and float64 runs that the borderline sets failed to mark.
Y_CAP = 2.0e-5
TILE = 16


# ------------------------------------------------------------------------------------------------ cameras and scenes
def look_at_camera(eye, target, fovx_deg, W, H, up=(0.0, 1.0, 0.0), znear=0.01, zfar=100.0):
    """A pinhole camera in the rasteriser's conventions: row-vector matrices ([p, 1] . V), +z forward, y down."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, up)            # +x right with y down
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], axis=1)          # world -> camera as p @ R
    V = np.eye(4)
    V[:3, :3] = R
    V[3, :3] = -eye @ R
    tanx = np.tan(np.radians(fovx_deg) / 2.0)
    tany = tanx * H / W
    Pm = np.zeros((4, 4))                             # row-vector form of the usual perspective matrix
    Pm[0, 0] = 1.0 / tanx
    Pm[1, 1] = 1.0 / tany
    Pm[2, 2] = zfar / (zfar - znear)
    Pm[3, 2] = -(zfar * znear) / (zfar - znear)
    Pm[2, 3] = 1.0
    return dict(V=V.astype(np.float32), P=(V @ Pm).astype(np.float32), tanfovx=float(np.float32(tanx)), tanfovy=float(np.float32(tany)),
                W=int(W), H=int(H), campos=eye.astype(np.float32))


def _cloud(rng, n, centre, spread, scale_lo, scale_hi, aniso=4.0):
    means = (np.asarray(centre) + rng.normal(size=(n, 3)) * np.asarray(spread)).astype(np.float32)
    base = np.exp(rng.uniform(np.log(scale_lo), np.log(scale_hi), size=(n, 1)))
    scales = (base * np.exp(rng.uniform(-np.log(aniso) / 2, np.log(aniso) / 2, size=(n, 3)))).astype(np.float32)
    q = rng.normal(size=(n, 4))
    rots = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.9, 1.1, size=(n, 1))).astype(np.float32)   # used un-normalised
    opacity = rng.uniform(0.05, 1.0, size=n).astype(np.float32)
    colors = rng.uniform(0.0, 1.0, size=(n, 3)).astype(np.float32)
    return dict(means=means, scales=scales, rotations=rots, opacity=opacity, colors=colors)


SCENES = ("a", "b", "c", "d", "e", "f", "g", "h", "i")
CPU_SCENES = ("a", "d", "e", "f", "g", "h", "i")           # <= 128 x 128 and <= 5 000 Gaussians


def scene(name, seed=None):
    """The scenes of tests/test_raster_hip.py: dict(means, scales, rotations, opacity, colors, cam, bg, scale_modifier)."""
    seeds = dict(a=11, b=11, c=23, d=31, e=41, f=51, g=61, h=71, i=81)
    rng = np.random.default_rng(seeds[name] if seed is None else seed)
    bg = np.array([0.1, 0.2, 0.3], np.float32)
    if name in ("a", "b"):      # an anisotropic cloud; (b) sees it with a wide field of view at a size that leaves partial tiles
        s = _cloud(rng, 5000, (0, 0, 0), (1.2, 1.2, 1.2), 0.01, 0.08)
        s["cam"] = look_at_camera((0.3, -0.4, -4.0), (0, 0, 0), 50.0, 128, 128) if name == "a" else \
            look_at_camera((0.2, -0.3, -1.6), (0, 0, 0), 120.0, 250, 187)
    elif name == "c":
        s = _cloud(rng, 20000, (0, 0, 0), (1.5, 1.5, 1.5), 0.005, 0.04)
        s["cam"] = look_at_camera((0.5, 0.6, -4.5), (0, 0, 0), 55.0, 400, 400)
    elif name == "d":           # a stack of nearly opaque Gaussians: pixels terminate in the first batch and mid-batch
        s = _cloud(rng, 700, (0, 0, 0.5), (0.5, 0.5, 1.0), 0.05, 0.3, aniso=2.0)
        s["opacity"][:] = 0.99
        s["cam"] = look_at_camera((0.0, 0.0, -3.0), (0, 0, 0), 45.0, 96, 96)
    elif name == "e":           # one Gaussian covering every tile
        s = _cloud(rng, 1, (0, 0, 0), (0.0, 0.0, 0.0), 1.5, 1.5, aniso=1.5)
        s["opacity"][:] = 0.8
        s["cam"] = look_at_camera((0.1, 0.2, -3.0), (0, 0, 0), 60.0, 112, 80)
    elif name == "f":           # everything behind the near plane
        s = _cloud(rng, 300, (0, 0, -6.0), (1.0, 1.0, 0.5), 0.02, 0.1)
        s["cam"] = look_at_camera((0.0, 0.0, -3.0), (0, 0, 0), 50.0, 64, 64)
    elif name == "g":           # a cloud straddling p_view.z = 0.2
        s = _cloud(rng, 1500, (0, 0, -2.6), (0.6, 0.6, 0.5), 0.004, 0.02)
        s["cam"] = look_at_camera((0.0, 0.0, -3.0), (0, 0, 0), 70.0, 96, 64)
    elif name == "h":           # n = 0
        s = _cloud(rng, 0, (0, 0, 0), (1, 1, 1), 0.01, 0.02)
        s["cam"] = look_at_camera((0.0, 0.0, -3.0), (0, 0, 0), 50.0, 40, 24)
    elif name == "i":           # far more than 256 instances in the central tiles: several LDS batches
        s = _cloud(rng, 2500, (0, 0, 0), (0.12, 0.12, 1.0), 0.004, 0.02)
        s["opacity"] *= 0.15
        s["cam"] = look_at_camera((0.0, 0.0, -3.0), (0, 0, 0), 40.0, 64, 64)
    else:
        raise KeyError(name)
    s["bg"], s["scale_modifier"], s["name"] = bg, 1.0, name
    return s


def cov3d_from_scale_rot(scales, rotations, mod, dtype):
    f = dtype
    s, q = np.asarray(scales).astype(f), np.asarray(rotations).astype(f)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = f(1), f(2)
    R = [one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
         two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
         two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)]
    sm = [f(mod) * s[:, k] for k in range(3)]
    A = [R[3 * i + k] * sm[k] for i in range(3) for k in range(3)]
    dot = lambda i, j: A[3 * i] * A[3 * j] + A[3 * i + 1] * A[3 * j + 1] + A[3 * i + 2] * A[3 * j + 2]
    return np.stack([dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)], axis=1).astype(f)


# ------------------------------------------------------------------------------------------------ projection
def _near_int(v, scale):
    return np.abs(v - np.round(v)) <= EPS * scale


def project(means, cov6, cam, dtype):
    """Per-Gaussian outputs in `dtype` (the order of operations of raster_math.h project()):
    dict(valid, depth, px, py, conic (n,3), cov2d (n,3), radius, rect (n,4) = x0 y0 x1 y1, projectable, borderline)."""
    f = dtype
    W, H = cam["W"], cam["H"]
    tx_n, ty_n = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    V, P = cam["V"].astype(f).reshape(16), cam["P"].astype(f).reshape(16)
    tanx, tany = f(cam["tanfovx"]), f(cam["tanfovy"])
    fx, fy = f(W) / (f(2) * tanx), f(H) / (f(2) * tany)
    m, c = np.asarray(means).astype(f).reshape(-1, 3), np.asarray(cov6).astype(f).reshape(-1, 6)
    n = len(m)
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    with np.errstate(all="ignore"):
        tx = V[0] * x + V[4] * y + V[8] * z + V[12]
        ty = V[1] * x + V[5] * y + V[9] * z + V[13]
        tz = V[2] * x + V[6] * y + V[10] * z + V[14]
        front = tz > f(0.2)
        hx = P[0] * x + P[4] * y + P[8] * z + P[12]
        hy = P[1] * x + P[5] * y + P[9] * z + P[13]
        hw = P[3] * x + P[7] * y + P[11] * z + P[15]
        pw = f(1) / (hw + f(0.0000001))
        limx, limy = f(1.3) * tanx, f(1.3) * tany
        tzs = np.where(front, tz, f(1))
        tx = np.minimum(limx, np.maximum(-limx, tx / tzs)) * tzs
        ty = np.minimum(limy, np.maximum(-limy, ty / tzs)) * tzs
        j00, j02 = fx / tzs, -(fx * tx) / (tzs * tzs)
        j11, j12 = fy / tzs, -(fy * ty) / (tzs * tzs)
        m00, m01, m02 = j00 * V[0] + j02 * V[2], j00 * V[4] + j02 * V[6], j00 * V[8] + j02 * V[10]
        m10, m11, m12 = j11 * V[1] + j12 * V[2], j11 * V[5] + j12 * V[6], j11 * V[9] + j12 * V[10]
        u0 = c[:, 0] * m00 + c[:, 1] * m01 + c[:, 2] * m02
        u1 = c[:, 1] * m00 + c[:, 3] * m01 + c[:, 4] * m02
        u2 = c[:, 2] * m00 + c[:, 4] * m01 + c[:, 5] * m02
        v0 = c[:, 0] * m10 + c[:, 1] * m11 + c[:, 2] * m12
        v1 = c[:, 1] * m10 + c[:, 3] * m11 + c[:, 4] * m12
        v2 = c[:, 2] * m10 + c[:, 4] * m11 + c[:, 5] * m12
        a = m00 * u0 + m01 * u1 + m02 * u2 + f(0.3)
        b = m10 * u0 + m11 * u1 + m12 * u2
        d = m10 * v0 + m11 * v1 + m12 * v2 + f(0.3)
        det = a * d - b * b
        nonsing = det != 0
        dets = np.where(nonsing, det, f(1))
        det_inv = f(1) / dets
        conic = np.stack([d * det_inv, -b * det_inv, a * det_inv], axis=1)
        mid = f(0.5) * (a + d)
        disc = np.sqrt(np.maximum(f(0.1), mid * mid - det))
        lam = np.maximum(mid + disc, mid - disc)
        ext = f(3) * np.sqrt(lam)
        rf = np.ceil(ext)
        rf = np.where(rf < 1.0e9, rf, 1.0e9)
        radius = rf.astype(np.int64)
        px = ((hx * pw + f(1)) * f(W) - f(1)) * f(0.5)
        py = ((hy * pw + f(1)) * f(H) - f(1)) * f(0.5)
        r = radius.astype(f)
        edges = [(px - r) / f(TILE), (py - r) / f(TILE), (px + r + f(TILE - 1)) / f(TILE), (py + r + f(TILE - 1)) / f(TILE)]
        lims = [tx_n, ty_n, tx_n, ty_n]
        rect = np.stack([np.nan_to_num(np.minimum(np.maximum(e, f(0)), f(lim)), nan=0.0).astype(np.int64) for e, lim in zip(edges, lims)], axis=1)
    projectable = front & nonsing
    tiles = (rect[:, 2] - rect[:, 0]) * (rect[:, 3] - rect[:, 1])
    valid = projectable & (tiles > 0)
    out = dict(valid=valid, projectable=projectable, depth=tz, px=px, py=py, conic=conic, cov2d=np.stack([a, b, d], axis=1),
               radius=np.where(valid, radius, 0), rect=np.where(valid[:, None], rect, 0), raw_rect=rect, tiles_x=tx_n, tiles_y=ty_n)
    # borderline decisions (meaningful in the float64 run)
    with np.errstate(all="ignore"):
        b_near = np.abs(tz - 0.2) <= EPS * 0.2
        b_det = front & (np.abs(det) <= EPS * np.maximum(np.abs(a * d), b * b))
        b_rad = projectable & _near_int(ext, np.maximum(ext, 1.0))
        b_rect = np.zeros(n, bool)
        for e, lim, centre in zip(edges, lims, (px, py, px, py)):
            k = np.round(e)
            scale = np.maximum(np.maximum(np.abs(centre), r), max(W, H)) / TILE
            b_rect |= projectable & (k >= 1) & (k <= lim) & (np.abs(e - k) <= EPS * scale)
    out["borderline_global"] = b_near | b_det            # may appear or vanish as a whole
    out["borderline_extent"] = b_rad | b_rect            # may gain or lose a ring of tiles
    out["borderline"] = out["borderline_global"] | out["borderline_extent"]
    return out


# ------------------------------------------------------------------------------------------------ render
def render(s, dtype, cov6=None, tile_mask=None, flags=None):
    """Renders scene dict `s` in `dtype`.  cov6: use these covariances instead of building them from scales / rotations.
    tile_mask: (tiles_y, tiles_x) bool, render only those tiles (the others keep NaN).  flags: compute the borderline sets
    (default: in float64 only).
    Returns dict(color (3,H,W), final_T, n_contrib, radii, proj, borderline_pixels (H,W) bool, borderline_gaussians (n,) bool)."""
    f = dtype
    flags = (f == np.float64) if flags is None else flags
    cam = s["cam"]
    W, H = cam["W"], cam["H"]
    if cov6 is None:
        cov6 = cov3d_from_scale_rot(s["scales"], s["rotations"], s["scale_modifier"], f)
    pr = project(s["means"], cov6, cam, f)
    n = len(pr["valid"])
    tx_n, ty_n = pr["tiles_x"], pr["tiles_y"]
    if tile_mask is None:
        tile_mask = np.ones((ty_n, tx_n), bool)
    sel = np.repeat(np.repeat(tile_mask, TILE, axis=0), TILE, axis=1)[:H, :W]
    T = np.ones((H, W), f)
    Cacc = np.zeros((H, W, 3), f)
    done = ~sel
    seen = np.zeros((H, W), np.int64)
    last = np.zeros((H, W), np.int64)
    bpix = np.zeros((H, W), bool)
    last_run = np.full((H, W), -1, np.int64)
    opacity, colors = np.asarray(s["opacity"]).astype(f).reshape(-1), np.asarray(s["colors"]).astype(f).reshape(-1, 3)
    YY, XX = np.mgrid[0:H, 0:W]
    XX, YY = XX.astype(f), YY.astype(f)

    cand = np.nonzero(pr["valid"] | (pr["projectable"] & pr["borderline_extent"] if flags else False))[0]
    order = cand[np.lexsort((cand, pr["depth"][cand]))]
    run = np.full(n, -1, np.int64)
    if flags and len(order) > 1:
        dd = pr["depth"][order]
        close = (dd[1:] - dd[:-1]) <= EPS * np.abs(dd[1:])
        ids = np.concatenate([[0], np.cumsum(~close)])
        in_run = np.concatenate([[False], close]) | np.concatenate([close, [False]])
        run[order] = np.where(in_run, ids, -1)
    if flags and pr["borderline_global"].any():
        bpix |= sel
    a255, tmin, amax = f(1.0) / f(255.0), f(0.0001), f(0.99)

    for g in order:
        x0, y0, x1, y1 = (int(v) for v in (pr["rect"][g] if pr["valid"][g] else (0, 0, 0, 0)))
        ext = flags and pr["borderline_extent"][g]
        if ext:
            rx0, ry0, rx1, ry1 = (int(v) for v in pr["raw_rect"][g])
            ex0, ey0, ex1, ey1 = max(rx0 - 1, 0), max(ry0 - 1, 0), min(rx1 + 1, tx_n), min(ry1 + 1, ty_n)
        else:
            ex0, ey0, ex1, ey1 = x0, y0, x1, y1
        if ex1 <= ex0 or ey1 <= ey0 or not tile_mask[ey0:ey1, ex0:ex1].any():
            continue
        ys, xs = slice(ey0 * TILE, min(ey1 * TILE, H)), slice(ex0 * TILE, min(ex1 * TILE, W))
        inrect = np.zeros((ys.stop - ys.start, xs.stop - xs.start), bool)
        inrect[(y0 - ey0) * TILE:(y1 - ey0) * TILE, (x0 - ex0) * TILE:(x1 - ex0) * TILE] = True
        live = ~done[ys, xs]
        act = live & inrect
        seen[ys, xs] += act
        dx, dy = pr["px"][g] - XX[ys, xs], pr["py"][g] - YY[ys, xs]
        ca, cb, cc = pr["conic"][g]
        with np.errstate(all="ignore"):
            power = f(-0.5) * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
            alpha = np.minimum(amax, opacity[g] * np.exp(np.minimum(power, f(0))))
        ok = act & ~(power > 0) & ~(alpha < a255)
        test_T = T[ys, xs] * (f(1) - alpha)
        stop = ok & (test_T < tmin)
        add = ok & ~stop
        if flags:
            mag = 0.5 * (np.abs(ca) * dx * dx + np.abs(cc) * dy * dy) + np.abs(cb * dx * dy)
            b = (np.abs(power) <= EPS * mag) & ((dx != 0) | (dy != 0))
            # alpha inherits power's absolute error, which scales with the sum of its terms' magnitudes (mag), not with |power|
            b |= ~(power > 0) & (np.abs(alpha - a255) <= EPS * alpha * (1.0 + mag))
            b |= ok & (np.abs(test_T - tmin) <= EPS * (tmin + T[ys, xs] * alpha * (1.0 + mag)))
            bpix[ys, xs] |= b & act
            if ext:             # its rectangle may differ by a ring of tiles: every live pixel it would reach is borderline
                bpix[ys, xs] |= live & ~(power > EPS * mag) & (alpha >= a255 * (1 - EPS))
            if run[g] >= 0:
                lr = last_run[ys, xs]
                bpix[ys, xs] |= ok & (lr == run[g])
                lr[ok] = run[g]
                last_run[ys, xs] = lr
        w = alpha * T[ys, xs]
        Cacc[ys, xs] += np.where(add[..., None], colors[g] * w[..., None], f(0))
        T[ys, xs] = np.where(add, test_T, T[ys, xs])
        lv = last[ys, xs]
        last[ys, xs] = np.where(add, seen[ys, xs], lv)
        done[ys, xs] |= stop
    bg = np.asarray(s["bg"]).astype(f)
    color = (Cacc + T[..., None] * bg).transpose(2, 0, 1).copy()
    color[:, ~sel] = np.nan
    final_T = np.where(sel, T, np.nan)
    return dict(color=color, final_T=final_T, n_contrib=np.where(sel, last, -1), radii=pr["radius"].astype(np.int32), proj=pr,
                borderline_pixels=bpix, borderline_gaussians=pr["borderline"], selected=sel)


def yardstick(s, cov6=None, tile_mask=None):
    """(float64 run, float32 run, y): y = the largest |float32 - float64| pixel difference off the borderline pixels."""
    r64 = render(s, np.float64, cov6=cov6, tile_mask=tile_mask)
    r32 = render(s, np.float32, cov6=cov6, tile_mask=tile_mask)
    keep = r64["selected"] & ~r64["borderline_pixels"]
    y = float(np.max(np.abs(r32["color"].astype(np.float64) - r64["color"])[:, keep], initial=0.0))
    return r64, r32, y


def eval_sh64(shs, degree, dirs):
    """float64 real spherical harmonics, degree 0..3: shs (n, K, 3), unit dirs (n, 3) -> max(value + 0.5, 0)"""
    shs, d = np.asarray(shs, np.float64), np.asarray(dirs, np.float64)
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    pi = np.pi
    v = 0.5 * np.sqrt(1 / pi) * shs[:, 0]
    if degree > 0:
        c1 = np.sqrt(3 / (4 * pi))
        v = v - c1 * y * shs[:, 1] + c1 * z * shs[:, 2] - c1 * x * shs[:, 3]
    if degree > 1:
        c2 = 0.5 * np.sqrt(15 / pi)
        v = v + c2 * x * y * shs[:, 4] - c2 * y * z * shs[:, 5] + 0.25 * np.sqrt(5 / pi) * (2 * z * z - x * x - y * y) * shs[:, 6] \
            - c2 * x * z * shs[:, 7] + 0.25 * np.sqrt(15 / pi) * (x * x - y * y) * shs[:, 8]
    if degree > 2:
        a, b, c = 0.25 * np.sqrt(35 / (2 * pi)), 0.5 * np.sqrt(105 / pi), 0.25 * np.sqrt(21 / (2 * pi))
        v = v - a * y * (3 * x * x - y * y) * shs[:, 9] + b * x * y * z * shs[:, 10] - c * y * (4 * z * z - x * x - y * y) * shs[:, 11] \
            + 0.25 * np.sqrt(7 / pi) * z * (2 * z * z - 3 * x * x - 3 * y * y) * shs[:, 12] - c * x * (4 * z * z - x * x - y * y) * shs[:, 13] \
            + 0.25 * np.sqrt(105 / pi) * z * (x * x - y * y) * shs[:, 14] - a * x * (x * x - 3 * y * y) * shs[:, 15]
    return np.maximum(v + 0.5, 0.0)
