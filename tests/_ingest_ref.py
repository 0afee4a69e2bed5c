"""NumPy restatement of the scene ingest (gs_simulation.py:403-438) and the checks the ingest tests share.  TEST INFRASTRUCTURE ONLY.

`reference(...)` follows the reference's torch expressions one by one at a chosen precision; tests/test_scene_ingest_math.py pins it
to tests/golden/scene_ingest.npz (the reference's own code), so that the GPU tests can use it at sizes the golden does not hold.
The bar of every floating quantity is the convention of tests/test_raster_math.py: with y the error of the reference's float32 run
against its float64 run (max-abs over max-abs magnitude), a result lies within 3 y of the float64 run.  y comes from the golden for
the golden cases and from this restatement's float32 and float64 runs of the same input elsewhere; never from the code under test.
"""
import ast
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
CASES = ("deg3", "deg0", "rot3")
FLOATING = ("pos", "cov", "opacity", "scale_origin", "original_mean_pos", "unsel_cov", "unsel_opacity")
BAR = 3.0
MARGIN = 1e-4

_golden = None


def golden():
    global _golden
    if _golden is None:
        _golden = dict(np.load(os.path.join(GOLDEN, "scene_ingest.npz")))
    return _golden


def golden_config(case):
    return ast.literal_eval(str(golden()[f"{case}/config"]))


def golden_ply(case):
    return os.path.join(GOLDEN, f"ingest_{case}.ply")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max()) if a.size else 0.0


def rotation_matrices(degrees, axes, dt):
    """generate_rotation_matrices at precision dt (pi = 3.1415926)"""
    out = []
    for deg, ax in zip(degrees, axes):
        a = dt(deg) / dt(180.0) * dt(3.1415926)
        c, s = np.cos(a), np.sin(a)
        m = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[ax]
        out.append(np.asarray(m, dt))
    return out


def reference(block, columns, k, cfg, dt, mats=None):
    """The span at precision dt (np.float32 / np.float64) on the PLY body `block` (N, A) with the column table of
    GaussianCheckpoint.  `mats`: the rotation matrices to use (default: rotation_matrices at dt).  Returns a dict with the golden's
    keys: sel_index, unsel_index, pos, cov, opacity, shs, unsel_*, scale_origin, original_mean_pos, all_cov, all_opacity."""
    columns = np.asarray(columns)
    col = lambda lo, hi: block[:, columns[lo:hi]].astype(dt)
    n = block.shape[0]
    xyz, raw, ls, q = col(0, 3), col(3, 4), col(4, 7), col(7, 11)
    shs = np.concatenate([block[:, columns[11:14]][:, None, :],
                          block[:, columns[14:11 + 3 * k]].reshape(n, 3, k - 1).transpose(0, 2, 1)], axis=1)
    opacity = dt(1) / (dt(1) + np.exp(-raw))
    s = np.exp(ls)
    qn = q / np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])[:, None]
    r, x, y, z = qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3]
    two, one = dt(2), dt(1)
    R = np.stack([one - two * (y * y + z * z), two * (x * y - r * z), two * (x * z + r * y),
                  two * (x * y + r * z), one - two * (x * x + z * z), two * (y * z - r * x),
                  two * (x * z - r * y), two * (y * z + r * x), one - two * (x * x + y * y)], axis=1).reshape(n, 3, 3)
    L = R * s[:, None, :]
    full = L @ L.transpose(0, 2, 1)
    cov = np.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], axis=1)
    if mats is None:
        mats = rotation_matrices(cfg.get("rotation_degree", []), cfg.get("rotation_axis", []), dt)
    mats = [np.asarray(m, dt) for m in mats]

    kept = np.flatnonzero(opacity[:, 0] > dt(cfg["opacity_threshold"]))
    rp = xyz[kept]
    for m in mats:
        rp = rp @ m.T
    area = cfg.get("sim_area")
    inside = np.ones(len(kept), bool)
    if area is not None:
        for i in range(3):
            inside &= (rp[:, i] > dt(area[2 * i])) & (rp[:, i] < dt(area[2 * i + 1]))
    sel, unsel = kept[inside], kept[~inside]
    out = dict(sel_index=sel, unsel_index=unsel, all_cov=cov, all_opacity=opacity, shs=shs[sel], opacity=opacity[sel],
               unsel_pos=block[:, columns[0:3]][unsel], unsel_cov=cov[unsel], unsel_opacity=opacity[unsel], unsel_shs=shs[unsel],
               rotated_margin=np.inf, opacity_margin=float(np.abs(opacity.astype(np.float64) - cfg["opacity_threshold"]).min()))
    if area is not None and len(kept):
        out["rotated_margin"] = float(np.abs(rp[:, [0, 0, 1, 1, 2, 2]].astype(np.float64) - np.asarray(area, np.float64)).min())
    if len(sel) == 0:
        return out
    rp = rp[inside]
    lo, hi = rp.min(axis=0), rp.max(axis=0)
    mean = (lo + hi) / dt(2)
    with np.errstate(divide="ignore"):
        scale = dt(1) / (hi - lo).max()
    pos = (rp - mean) * scale + dt(1) + np.asarray([0, 0, cfg.get("z_shift_value", 0.0)], dt)
    full = np.stack([cov[sel][:, [0, 1, 2]], cov[sel][:, [1, 3, 4]], cov[sel][:, [2, 4, 5]]], axis=1)
    for m in mats:
        full = m @ (full @ m.T)
    rcov = np.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2], full[:, 2, 2]], axis=1) * (scale * scale)
    out.update(pos=pos, cov=rcov, scale_origin=scale, original_mean_pos=mean)
    return out


def synthetic_block(n, k, seed, cfg, all_selected=False, keep_only=None):
    """(block (n, 11 + 3 + 3 k), names): a random checkpoint in save_ply's column order whose Gaussians all keep MARGIN from cfg's
    thresholds (float64 evaluation; reference() reports the margins it met).  `all_selected`: opacities well above the threshold.
    `keep_only`: that many Gaussians pass the opacity filter, the others fall well below it."""
    from pixie_amd.splat_export import attribute_names
    rng = np.random.default_rng(seed)
    R = np.eye(3)
    for m in rotation_matrices(cfg.get("rotation_degree", []), cfg.get("rotation_axis", []), np.float64):
        R = m @ R
    draw_raw = lambda m: (rng.uniform(2.0, 4.0, m) if all_selected else rng.normal(0.0, 2.0, m)).astype(np.float32)
    xyz = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    raw = draw_raw(n)
    area = cfg.get("sim_area")
    for _ in range(200):
        near = np.abs(1 / (1 + np.exp(-raw.astype(np.float64))) - cfg["opacity_threshold"]) < 10 * MARGIN
        if area is not None:
            near |= (np.abs((xyz.astype(np.float64) @ R.T)[:, [0, 0, 1, 1, 2, 2]] - np.asarray(area, np.float64)) < 10 * MARGIN).any(axis=1)
        if not near.any():
            break
        xyz[near] = rng.uniform(-1, 1, (int(near.sum()), 3)).astype(np.float32)
        raw[near] = draw_raw(int(near.sum()))
    assert not near.any()
    if keep_only is not None:
        raw[:] = -8.0
        raw[rng.choice(n, keep_only, replace=False)] = 3.0
    shs = rng.normal(0, 0.5, (n, k, 3)).astype(np.float32)
    block = np.concatenate([xyz, np.zeros((n, 3), np.float32), shs[:, :1].transpose(0, 2, 1).reshape(n, -1),
                            shs[:, 1:].transpose(0, 2, 1).reshape(n, -1), raw[:, None],
                            rng.normal(-4.0, 0.7, (n, 3)).astype(np.float32), rng.normal(0, 1, (n, 4)).astype(np.float32)], axis=1)
    return np.ascontiguousarray(block), attribute_names(k)


def check_against(got, f64, y, what, report=None):
    """`got`, `f64`: dicts with the golden's keys (got may lack the unselected ones when there are none); `y`: {quantity: the
    reference's float32-vs-float64 error}.  Exact: indices (hence counts and order), shs, unselected pos.  Floating: within BAR * y
    of the float64 run.  Every figure is printed before it is asserted."""
    lines = []
    for key in ("sel_index", "unsel_index"):
        assert np.array_equal(got[key], f64[key]), f"{what}: {key} differs"
    assert np.array_equal(got["shs"], f64["shs"].astype(np.float32)), f"{what}: shs is not a bit-equal copy"
    n_unsel = len(f64["unsel_index"])
    if n_unsel:
        assert np.array_equal(got["unsel_shs"], f64["unsel_shs"].astype(np.float32)), f"{what}: unselected shs is not a bit-equal copy"
        assert np.array_equal(got["unsel_pos"], f64["unsel_pos"].astype(np.float32)), f"{what}: unselected pos is not a bit-equal copy"
    failed = []
    for q in FLOATING:
        if q.startswith("unsel_") and not n_unsel:
            continue
        err = rel(got[q], f64[q])
        lines.append(f"{what} {q}: reference y {y[q]:.3e}, bar {BAR * y[q]:.3e}, ours {err:.3e}")
        if not err <= BAR * y[q]:
            failed.append(lines[-1])
    print("\n".join(lines))
    if report is not None:
        report.extend(lines)
    assert not failed, "outside 3 y of the float64 run:\n" + "\n".join(failed)


def golden_runs(case):
    """(f32 dict, f64 dict, y) of a golden case"""
    g = golden()
    runs = {tag: {k.split("/", 2)[2]: v for k, v in g.items() if k.startswith(f"{case}/{tag}/")} for tag in ("f32", "f64")}
    y = {q: rel(runs["f32"][q], runs["f64"][q]) for q in FLOATING if q in runs["f64"]}
    return runs["f32"], runs["f64"], y
