"""Torch restatement of the rasteriser (include/pixie_hip.h, section D) with a `dtype` argument, whose gradients come from autograd: the
yardstick of the backward-pass tests on both sides (CPU: raster_grad_math.h built for the host; GPU: the kernels).

The projection is vectorised; the blend is a loop over the Gaussians in (depth, index) order, each over the pixels of its tile
rectangle.  Every decision -- culling, radius and rectangle (taken from tests/_raster_ref.project in the same dtype), power > 0, the
1/255 and 1e-4 rules, min(0.99, .), the 1.3 tanfov clamp and the max(., 0) of the colour -- is made on detached values, so autograd
differentiates the forward with every decision held fixed, which is how the library defines its gradient.  dL/dmeans2D is the
retained gradient of the pixel centres times (0.5 W, 0.5 H), with a zero third column.

Loss = sum(w * colour) with `weights(...)`: a seeded uniform(-1, 1) array that is zero on the borderline pixels of
_raster_ref.render(..., np.float64), so no gradient depends on a decision float32 may legitimately take the other way.
Run in float64 it is the reference; run in float32 it is the yardstick y_q of a quantity q: the rel-L2 distance of its float32
gradient from its float64 one over all Gaussians."""
import numpy as np
import torch

from tests import _raster_ref as rr

MAX_ZERO_SHARE = 0.01


def wide_scene():
    """A scene of our own: 1 200 Gaussians at 120 x 72 seen from inside the cloud with a 125 degree field of view, so that the
    1.3 tanfov clamp of the projection is active on some Gaussians whose extent still reaches the image."""
    rng = np.random.default_rng(97)
    s = rr._cloud(rng, 1200, (0, 0, 0.4), (1.6, 1.0, 0.5), 0.03, 0.2, aniso=3.0)
    s["opacity"] *= 0.6
    s["cam"] = rr.look_at_camera((0.05, -0.1, -0.55), (0, 0, 0.4), 125.0, 120, 72)
    s["bg"], s["scale_modifier"], s["name"] = np.array([0.1, 0.2, 0.3], np.float32), 1.0, "w"
    return s


def small_scene():
    """<= 200 Gaussians at 48 x 48 for the finite-difference check: wide field, so both clamps of the projection occur."""
    rng = np.random.default_rng(131)
    s = rr._cloud(rng, 160, (0, 0, 0.3), (1.2, 0.8, 0.4), 0.05, 0.25, aniso=3.0)
    s["opacity"] *= 0.7
    s["cam"] = rr.look_at_camera((0.05, -0.1, -0.6), (0, 0, 0.3), 120.0, 48, 48)
    s["bg"], s["scale_modifier"], s["name"] = np.array([0.1, 0.2, 0.3], np.float32), 1.25, "small"
    return s


def make_shs(n, seed, k=16):
    """SH coefficients for which max(., 0) is active on some channels: a DC term around -0.5 / C0 on a part of the Gaussians"""
    rng = np.random.default_rng(seed)
    shs = (rng.normal(size=(n, k, 3)) * 0.3).astype(np.float32)
    shs[:, 0, :] += rng.uniform(-2.5, 2.0, size=(n, 3)).astype(np.float32)
    return shs


def sh_colors64(s, shs, degree):
    d = s["means"].astype(np.float64) - s["cam"]["campos"].astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rr.eval_sh64(shs, degree, d)


def weights(s, cov6=None, seed=7, r64=None):
    """(w (3, H, W) float64, share of zero-weighted pixels, the float64 helper run)"""
    if r64 is None:
        r64 = rr.render(s, np.float64, cov6=cov6)
    cam = s["cam"]
    w = np.random.default_rng(seed).uniform(-1.0, 1.0, size=(3, cam["H"], cam["W"]))
    bp = r64["borderline_pixels"]
    w[:, bp] = 0.0
    return w, float(bp.mean()) if bp.size else 0.0, r64


def _sh_eval(sh, degree, x, y, z):
    """sh (n, K, 3), x y z (n, 1): the polynomial of raster_math.h sh_to_rgb before the + 0.5"""
    C0, C1 = 0.28209479177387814, 0.4886025119029199
    C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
    C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325616595, -0.4570457994644658, 1.445305721320277,
          -0.5900435899266435)
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    v = C0 * sh[:, 0]
    if degree > 0:
        v = v - C1 * y * sh[:, 1] + C1 * z * sh[:, 2] - C1 * x * sh[:, 3]
    if degree > 1:
        v = v + C2[0] * xy * sh[:, 4] + C2[1] * yz * sh[:, 5] + C2[2] * (2.0 * zz - xx - yy) * sh[:, 6] + C2[3] * xz * sh[:, 7] \
            + C2[4] * (xx - yy) * sh[:, 8]
    if degree > 2:
        v = v + C3[0] * y * (3.0 * xx - yy) * sh[:, 9] + C3[1] * xy * z * sh[:, 10] + C3[2] * y * (4.0 * zz - xx - yy) * sh[:, 11] \
            + C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * sh[:, 12] + C3[4] * x * (4.0 * zz - xx - yy) * sh[:, 13] \
            + C3[5] * z * (xx - yy) * sh[:, 14] + C3[6] * x * (xx - 3.0 * yy) * sh[:, 15]
    return v


def run(s, dtype, w, cov6=None, shs=None, sh_degree=0, grad=True, offsets=None):
    """One render of scene dict `s` in `dtype` (np.float32 / np.float64) and, with grad, the gradients of sum(w * colour).
    cov6: (n, 6) precomputed covariances (the cov3D form); None builds them from scales / rotations (that form).
    shs: (n, K, 3) coefficients evaluated at sh_degree (the SH form); None uses s["colors"].
    offsets: dict of arrays added to the inputs (keys of the returned grads, plus "means2D" (n, 2) added to the pixel centres), for
    finite differences.
    Returns dict(color (3, H, W), loss, grads {name: array}, n_contrib_max, signature (bytes: every decision taken),
    clamped (n,) bool: the 1.3 tanfov clamp is active, sh_clamped (n, 3) bool)."""
    td = torch.float32 if dtype == np.float32 else torch.float64
    f = dtype
    cam = s["cam"]
    W, H = cam["W"], cam["H"]
    n = len(s["means"])
    offsets = offsets or {}

    def leaf(a, key):
        a = np.asarray(a).astype(f)
        if key in offsets:
            a = a + np.asarray(offsets[key]).astype(f)
        return torch.tensor(a, dtype=td, requires_grad=grad)

    means = leaf(s["means"], "means3D")
    opac = leaf(np.asarray(s["opacity"]).reshape(-1), "opacities")
    leaves = {"means3D": means, "opacities": opac}
    mod = float(s["scale_modifier"])
    if cov6 is not None:
        cov = leaf(cov6, "cov3D")
        leaves["cov3D"] = cov
    else:
        sc, q = leaf(s["scales"], "scales"), leaf(s["rotations"], "rotations")
        leaves["scales"], leaves["rotations"] = sc, q
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = [1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
             2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
             2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)]
        sm = [mod * sc[:, k] for k in range(3)]
        A = [R[3 * i + k] * sm[k] for i in range(3) for k in range(3)]
        dot = lambda i, j: A[3 * i] * A[3 * j] + A[3 * i + 1] * A[3 * j + 1] + A[3 * i + 2] * A[3 * j + 2]
        cov = torch.stack([dot(0, 0), dot(0, 1), dot(0, 2), dot(1, 1), dot(1, 2), dot(2, 2)], dim=1)
    sh_clamped = np.zeros((n, 3), bool)
    if shs is not None:
        sh = leaf(shs, "shs")
        leaves["shs"] = sh
        campos = torch.tensor(cam["campos"].astype(f), dtype=td)
        dvec = means - campos
        dvec = dvec / torch.sqrt((dvec * dvec).sum(dim=1, keepdim=True))
        v = _sh_eval(sh, sh_degree, dvec[:, 0:1], dvec[:, 1:2], dvec[:, 2:3]) + 0.5
        on = v.detach() > 0
        sh_clamped = ~on.numpy()
        colors = torch.where(on, v, torch.zeros_like(v))
    else:
        colors = leaf(s["colors"], "colors")
        leaves["colors"] = colors

    # decisions of the projection: from the NumPy helper in the same dtype, on the same values
    pr = rr.project(means.detach().numpy(), cov.detach().numpy(), cam, f)
    valid = pr["valid"]
    idx = np.nonzero(valid)[0]
    ti = torch.from_numpy(idx)
    V, P = torch.tensor(cam["V"].astype(f).reshape(16), dtype=td), torch.tensor(cam["P"].astype(f).reshape(16), dtype=td)
    tanx, tany = f(cam["tanfovx"]), f(cam["tanfovy"])
    fx, fy = float(f(W) / (f(2) * tanx)), float(f(H) / (f(2) * tany))
    limx, limy = float(f(1.3) * tanx), float(f(1.3) * tany)
    m, c = means[ti], cov[ti]
    x, y, z = m[:, 0], m[:, 1], m[:, 2]
    tx = V[0] * x + V[4] * y + V[8] * z + V[12]
    ty = V[1] * x + V[5] * y + V[9] * z + V[13]
    tz = V[2] * x + V[6] * y + V[10] * z + V[14]
    hx = P[0] * x + P[4] * y + P[8] * z + P[12]
    hy = P[1] * x + P[5] * y + P[9] * z + P[13]
    hw = P[3] * x + P[7] * y + P[11] * z + P[15]
    pw = 1.0 / (hw + 0.0000001)
    rx, ry = tx / tz, ty / tz
    with torch.no_grad():
        hi_x, lo_x, hi_y, lo_y = rx > limx, rx < -limx, ry > limy, ry < -limy
    cx = torch.where(hi_x, torch.full_like(rx, limx), torch.where(lo_x, torch.full_like(rx, -limx), rx))
    cy = torch.where(hi_y, torch.full_like(ry, limy), torch.where(lo_y, torch.full_like(ry, -limy), ry))
    txc, tyc = cx * tz, cy * tz
    j00, j02 = fx / tz, -(fx * txc) / (tz * tz)
    j11, j12 = fy / tz, -(fy * tyc) / (tz * tz)
    m00, m01, m02 = j00 * V[0] + j02 * V[2], j00 * V[4] + j02 * V[6], j00 * V[8] + j02 * V[10]
    m10, m11, m12 = j11 * V[1] + j12 * V[2], j11 * V[5] + j12 * V[6], j11 * V[9] + j12 * V[10]
    u0 = c[:, 0] * m00 + c[:, 1] * m01 + c[:, 2] * m02
    u1 = c[:, 1] * m00 + c[:, 3] * m01 + c[:, 4] * m02
    u2 = c[:, 2] * m00 + c[:, 4] * m01 + c[:, 5] * m02
    v0 = c[:, 0] * m10 + c[:, 1] * m11 + c[:, 2] * m12
    v1 = c[:, 1] * m10 + c[:, 3] * m11 + c[:, 4] * m12
    v2 = c[:, 2] * m10 + c[:, 4] * m11 + c[:, 5] * m12
    a = m00 * u0 + m01 * u1 + m02 * u2 + 0.3
    b = m10 * u0 + m11 * u1 + m12 * u2
    d = m10 * v0 + m11 * v1 + m12 * v2 + 0.3
    det_inv = 1.0 / (a * d - b * b)
    conic = torch.stack([d * det_inv, -b * det_inv, a * det_inv], dim=1)
    px = ((hx * pw + 1.0) * float(W) - 1.0) * 0.5
    py = ((hy * pw + 1.0) * float(H) - 1.0) * 0.5
    pxy = torch.stack([px, py], dim=1)
    if "means2D" in offsets:
        pxy = pxy + torch.tensor(np.asarray(offsets["means2D"]).astype(f)[idx], dtype=td)
    if grad:
        pxy.retain_grad()
    clamped = np.zeros(n, bool)
    clamped[idx] = (hi_x | lo_x | hi_y | lo_y).numpy()

    T = torch.ones((H, W), dtype=td)
    Cacc = torch.zeros((H, W, 3), dtype=td)
    done = np.zeros((H, W), bool)
    seen = np.zeros((H, W), np.int64)
    last = np.zeros((H, W), np.int64)
    YY, XX = torch.meshgrid(torch.arange(H, dtype=td), torch.arange(W, dtype=td), indexing="ij")
    seq = np.lexsort((idx, pr["depth"][idx]))                        # the valid Gaussians in blend order
    a255, tmin, amax = float(f(1.0) / f(255.0)), float(f(0.0001)), float(f(0.99))
    sig = [valid.tobytes(), pr["rect"].tobytes(), idx[seq].tobytes(), clamped.tobytes(), sh_clamped.tobytes()]
    col_v, op_v = colors[ti], opac[ti]
    for k in seq:
        x0, y0, x1, y1 = (int(t) for t in pr["rect"][idx[k]])
        ys, xs = slice(y0 * rr.TILE, min(y1 * rr.TILE, H)), slice(x0 * rr.TILE, min(x1 * rr.TILE, W))
        live = ~done[ys, xs]
        seen[ys, xs] += live
        dx, dy = pxy[k, 0] - XX[ys, xs], pxy[k, 1] - YY[ys, xs]
        ca, cb, cc = conic[k, 0], conic[k, 1], conic[k, 2]
        power = -0.5 * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
        Tl = T[ys, xs].clone()
        with torch.no_grad():
            pos = power > 0
        raw = op_v[k] * torch.exp(torch.where(pos, torch.zeros_like(power), power))
        with torch.no_grad():
            capped = raw > amax
        alpha = torch.where(capped, torch.full_like(raw, amax), raw)
        with torch.no_grad():
            ok = torch.from_numpy(live) & ~pos & ~(alpha < a255)
            test_T = Tl * (1.0 - alpha)
            stop = ok & (test_T < tmin)
            add = ok & ~stop
        wgt = alpha * Tl
        Cacc[ys, xs] = Cacc[ys, xs] + torch.where(add[..., None], col_v[k] * wgt[..., None], torch.zeros((), dtype=td))
        T[ys, xs] = torch.where(add, Tl * (1.0 - alpha), Tl)
        addn = add.numpy()
        last[ys, xs] = np.where(addn, seen[ys, xs], last[ys, xs])
        done[ys, xs] |= stop.numpy()
        sig.append(np.packbits(addn).tobytes() + np.packbits((capped & add).numpy()).tobytes())
    bg = torch.tensor(np.asarray(s["bg"]).astype(f), dtype=td)
    color = (Cacc + T[..., None] * bg).permute(2, 0, 1)
    loss = (torch.tensor(np.asarray(w).astype(f), dtype=td) * color).sum()
    out = dict(color=color.detach().numpy().copy(), loss=float(loss.detach()), n_contrib_max=int(last.max(initial=0)), signature=b"".join(sig),
               clamped=clamped, sh_clamped=sh_clamped, valid=valid, grads=None)
    if grad:
        if loss.requires_grad:
            loss.backward()
        g = {k: (t.grad.numpy().astype(np.float64) if t.grad is not None else np.zeros(tuple(t.shape))) for k, t in leaves.items()}
        m2 = np.zeros((n, 3))
        if pxy.grad is not None and len(idx):
            m2[idx, 0] = pxy.grad[:, 0].numpy().astype(np.float64) * (0.5 * W)
            m2[idx, 1] = pxy.grad[:, 1].numpy().astype(np.float64) * (0.5 * H)
        g["means2D"] = m2
        out["grads"] = g
    return out


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = float(np.sqrt((ref * ref).sum()))
    num = float(np.sqrt(((got - ref) ** 2).sum()))
    return num / den if den > 0 else (0.0 if num == 0 else float("inf"))


def bar(y_q, k):
    """What a float32 implementation may be away from the float64 gradient, per quantity: 3 y_q for a different but equally valid
    float32 rounding sequence, plus 2 K 2^-24 for a K-step chain of T / (1 - alpha) recoveries at two roundings a step."""
    return 3.0 * y_q + 2.0 * k * 2.0 ** -24


def case(name, form="cov", degree=None):
    """A test case: scene `name` ("w": wide_scene, "small": small_scene, else a scene of _raster_ref) in the form "cov" (cov3D_precomp,
    the float32 covariances the helper builds) or "sr" (scales / rotations), with precomputed colours (degree None) or SH coefficients
    evaluated at `degree`.  Returns (scene, kwargs of run, w, share of zero-weighted pixels)."""
    s = wide_scene() if name == "w" else small_scene() if name == "small" else rr.scene(name)
    kw = {}
    if form == "cov":
        kw["cov6"] = rr.cov3d_from_scale_rot(s["scales"], s["rotations"], s["scale_modifier"], np.float32)
    if degree is not None:
        kw["shs"], kw["sh_degree"] = make_shs(len(s["means"]), 1000 + degree), degree
        s["colors"] = sh_colors64(s, kw["shs"], degree).astype(np.float32)       # what the NumPy helper blends
    w, share, _ = weights(s, cov6=kw.get("cov6"))
    return s, kw, w, share


_CACHE = {}


def reference(name, form="cov", degree=None):
    """(scene, kwargs of run, w, share, float64 run, {quantity: y_q}) of case(name, form, degree): computed once per process"""
    key = (name, form, degree)
    if key not in _CACHE:
        s, kw, w, share = case(name, form, degree)
        r64 = run(s, np.float64, w, **kw)
        r32 = run(s, np.float32, w, **kw)
        y = {q: rel_l2(r32["grads"][q], r64["grads"][q]) for q in r64["grads"]}
        _CACHE[key] = (s, kw, w, share, r64, y)
    return _CACHE[key]
