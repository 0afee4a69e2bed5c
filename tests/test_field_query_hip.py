"""GPU checks of the NeRF feature-field query (pixie_amd.field_query, pixie_amd/csrc/field_query.hip) against the float64 NumPy
restatement of tests/_field_query_ref.py.

Bars.  Every float32 output array: max |got - float64| <= 3 x max |float32 NumPy evaluation of the same restatement - float64| on
the same inputs, plus the floor of _field_query_ref.bar: (sum of the layers' fan-ins + 16) 2^-24 max(1, max|ref|) -- a K-term
float32 dot product carries at most K 2^-24 sum|w x| of rounding error and the encoding a handful of roundings per column; the
floor matters only where the float32 yardstick lands on the float64 value by luck.  The measured ratios are printed;
profiles/field_query_parity.txt is written from the same cases by scripts/field_query_bench.py --parity.

Equalities.  float16 outputs equal the float32 results rounded to nearest even; the density is zero exactly where the float32
restatement's selector is false; the files' dtypes, shapes and .npz keys are voxelize.py's; two runs are bit-identical; the
reference's batch loop (voxelize.py:93-113, here 1000 points per batch so that the last batch is ragged) over FeatureFieldQuery
equals the fused call.

General affine.  The kernel's affine is the float32 chain ((a0 x + a1 y) + a2 z) + a3 and the restatement repeats it bit for bit;
the reference's Transform3d is a float32 matrix product whose order is not specified, so a voxel within a few ulps of a selector
face may fall on the other side there.  The lattices here keep every voxel 1e-4 away from the faces (asserted), as INTEGRATION
section 1a documents for this stage.
"""
import os

import numpy as np
import pytest
import torch

from tests import _field_query_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N_MAX = 257

# name -> (convention, log2_T, F, n_frequencies, n_extra, n_hidden, out_dim, bias, activation); 4 levels from 4 to 32: with the
# tcnn convention level 0 is dense and the others hashed at both table sizes, and 32^3 corners wrap a 2^8 / 2^10 table many times
NETS = {
    "tcnn_T8_F2_h1_o16_bias": ("tcnn", 8, 2, 0, 0, 1, 16, True, "none"),
    "tcnn_T10_F8_freq_h2_o768": ("tcnn", 10, 8, 6, 0, 2, 768, False, "none"),
    "ns_T8_F2_h2_o20_bias": ("nerfstudio", 8, 2, 0, 0, 2, 20, True, "none"),
    "ns_T10_F8_freq_h1_o3_sigmoid": ("nerfstudio", 10, 8, 6, 0, 1, 3, True, "sigmoid"),
    "tcnn_T10_F2_extra5_h2_o16_exp": ("tcnn", 10, 2, 0, 5, 2, 16, True, "exp"),
    "tcnn_T8_F4_extra3_h4_o64": ("tcnn", 8, 4, 0, 3, 4, 64, False, "none"),               # odd input width (19), one full chunk
    "extra15_h2_o3_sigmoid": (None, 0, 0, 0, 15, 2, 3, True, "sigmoid"),                  # the colour head's shape: no grid
}
_cases = {}


def sample_points(rng, n):
    p = rng.random((n, 3)).astype(np.float32)
    p[:8] = [[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [0.25, 0.75, 0.5], [0, 1, 0.5], [0.125, 0.375, 0.875], [1, 0, 0], [0.5, 0, 1]]
    return p                                           # exactly 0, exactly 1, and cell boundaries of both conventions (q integral)


def case(name):
    """net, inputs and both NumPy evaluations: computed once per name, shared and left unchanged"""
    if name not in _cases:
        conv, T, F, nf, ne, nh, out, bias, act = NETS[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        lv, rows = R.levels(conv, 4, 4, 32, T) if conv else (None, 0)
        net = R.random_net(rng, lv, rows, F, nf, ne, nh, out, bias, act)
        p = sample_points(rng, N_MAX)
        extra = rng.standard_normal((N_MAX, ne)).astype(np.float32) if ne else None
        ref = R.hashmlp(net, p, extra)
        f32 = R.hashmlp(net, p, extra, np.float32)
        _cases[name] = (net, p, extra, ref, f32)
    return _cases[name]


def device_net(net, device=DEV):
    from pixie_amd import field_query as FQ
    lv = None
    if net["levels"]:
        lv = np.array([tuple(l[k] for k in FQ.LEVEL_DTYPE.names) for l in net["levels"]], FQ.LEVEL_DTYPE)
    return FQ.HashMLP(lv, net["table"], net["weights"], net["biases"], net["n_frequencies"], net["n_extra"], net["act"], device=device)


def within(got, ref, f32, nets, what):
    err = float(np.abs(got.astype(np.float64) - ref).max())
    yard = float(np.abs(f32.astype(np.float64) - ref).max())
    bar = R.bar(ref, f32, nets)
    print(f"{what}: max|got - f64| {err:.3e}, float32 NumPy {yard:.3e} (ratio {err / yard if yard else float('inf'):.2f}), bar {bar:.3e}")
    assert np.all(np.isfinite(got)) and err <= bar, what


@pytest.mark.parametrize("name", list(NETS))
def test_hashmlp_forward_against_float64(name):
    net, p, extra, ref, f32 = case(name)
    m = device_net(net)
    t = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    got = m(t(p) if net["levels"] else None, t(extra))
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape and got.is_cuda
    within(got.cpu().numpy(), ref, f32, [net], name)
    again = m(t(p) if net["levels"] else None, t(extra))
    assert torch.equal(got, again), "two runs are bit-identical"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["tcnn_T10_F8_freq_h2_o768", "ns_T8_F2_h2_o20_bias", "tcnn_T10_F2_extra5_h2_o16_exp"])
def test_point_counts_around_the_tile(name, n):
    """a point's result does not depend on how many points share its tile: the first n rows equal the rows of the full call"""
    net, p, extra, ref, f32 = case(name)
    m = device_net(net)
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a[:n])).to(DEV)
    full = m(torch.from_numpy(p).to(DEV), None if extra is None else torch.from_numpy(extra).to(DEV))
    got = m(t(p), t(extra))
    assert tuple(got.shape) == (n, ref.shape[1]) and torch.equal(got, full[:n])
    within(got.cpu().numpy(), ref[:n], f32[:n], [net], f"{name} n={n}")


# ---- the voxeliser ---------------------------------------------------------------------------------------------------------
GENERAL = np.array([[0.9, 0.12, -0.05, 0.03969], [-0.1, 0.95, 0.07, -0.02054], [0.04, -0.06, 1.05, -0.01945]], np.float32)
AABB = np.array([[-1, -1, -1], [1, 1, 1]], np.float32)
# name -> (min_bounds, max_bounds, voxel_size, contraction, affine, alpha_weighted, feature_dim)
LATTICES = {
    "5x7x9_contraction_identity": ((-1.0, -0.75, -1.25), (0.25, 1.0, 1.0), 0.25, True, None, True, 768),     # |x|inf exactly 1 and above
    "5x7x9_contraction_general_raw": ((-1.0, -0.75, -1.25), (0.25, 1.0, 1.0), 0.25, True, GENERAL, False, 64),
    "16c_aabb_identity": ((-1.04,) * 3, (1.04,) * 3, 0.13, False, None, True, 64),                          # outside the aabb: selector 0
    "16c_aabb_general": ((-1.04,) * 3, (1.04,) * 3, 0.13, False, GENERAL, True, 24),
}
_fields = {}


def lattice_case(name):
    if name not in _fields:
        from pixie_amd import field_query as FQ
        lo, hi, vs, contraction, A, weighted, C = LATTICES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        fq = R.random_field(rng, "tcnn" if "contraction" in name else "nerfstudio", C, contraction, A, None if contraction else AABB)
        axes = [a.numpy() for a in FQ.lattice_axes(lo, hi, vs)]                       # torch.arange on the host, the reference's line
        x = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        ref = R.field(fq, x, vs)
        f32 = R.field(fq, x, vs, np.float32)
        _fields[name] = (fq, x, tuple(len(a) for a in axes), ref, f32)
    return _fields[name]


def device_field(fq):
    from pixie_amd import field_query as FQ
    return FQ.FeatureFieldQuery(device_net(fq["density"]), device_net(fq["color"]), device_net(fq["feature"]), fq["world_to_nerf"],
                                fq["contraction"], fq.get("aabb"), fq["average_init_density"])


@pytest.mark.parametrize("name", list(LATTICES))
def test_voxelize_against_float64_and_the_batch_loop(name):
    fq, x, shape, ref, f32 = lattice_case(name)
    lo, hi, vs, contraction, A, weighted, C = LATTICES[name]
    n = len(x)
    assert shape == ((5, 7, 9) if name.startswith("5x7x9") else (16, 16, 16))
    margin = np.minimum(np.abs(ref["p"]), np.abs(ref["p"] - 1)).min()
    if A is not None:
        assert margin > 1e-4, "the general-affine lattices stay clear of the selector faces"
    assert contraction or 0 < ref["selector"].sum() < n
    if name == "5x7x9_contraction_identity":
        mag = np.abs(x).max(axis=1)
        assert (mag == 1).any() and (mag > 1).any() and (mag < 1).any()
    field = device_field(fq)
    feats, alphas, rgb, density, alpha32 = field.voxelize(lo, hi, vs, weighted, return_density=True, return_alpha32=True)
    assert feats.dtype == alphas.dtype == rgb.dtype == torch.float16 and density.dtype == alpha32.dtype == torch.float32
    assert tuple(feats.shape) == shape + (C,) and tuple(alphas.shape) == shape + (1,) and tuple(rgb.shape) == shape + (3,)
    # float32 outputs against the restatement
    nets_d, nets_c, nets_f = [fq["density"]], [fq["density"], fq["color"]], [fq["feature"]]
    d = density.cpu().numpy().reshape(-1)
    assert np.array_equal(d == 0, ~ref["selector"]), "selector"
    within(d, ref["density"], f32["density"], nets_d, f"{name} density")
    within(alpha32.cpu().numpy().reshape(-1), ref["alpha"], f32["alpha"], nets_d, f"{name} alpha")
    # the reference's loop over the adapter surface, ragged last batch
    pts = torch.from_numpy(x).to(DEV)
    loop_f, loop_a, loop_c = (np.zeros((n, k), np.float16) for k in (C, 1, 3))
    raw32, rgb32 = np.zeros((n, C), np.float32), np.zeros((n, 3), np.float32)
    for i in range(0, n, 1000):
        batch = pts[i:i + 1000]
        outputs = field(batch)
        alpha = field.get_alpha(batch, vs)
        qp_alpha = 1 - torch.exp(-(outputs["density"] * vs))                        # get_alpha(outputs["density"], delta), optimize.py:226
        feature = qp_alpha * outputs["feature"] if weighted else outputs["feature"]
        colour = field.get_rgb(batch)
        loop_f[i:i + 1000] = feature.cpu().to(torch.float16).numpy()
        loop_a[i:i + 1000] = alpha.cpu().to(torch.float16).numpy()
        loop_c[i:i + 1000] = colour.cpu().to(torch.float16).numpy()
        raw32[i:i + 1000], rgb32[i:i + 1000] = outputs["feature"].cpu().numpy(), colour.cpu().numpy()
        assert torch.equal(outputs["density"].reshape(-1), density.reshape(-1)[i:i + 1000])
        assert torch.equal(alpha.reshape(-1), alpha32.reshape(-1)[i:i + 1000])
        assert torch.equal(field.get_density(batch), outputs["density"])
    within(raw32, ref["feature"], f32["feature"], nets_f, f"{name} feature")
    within(rgb32, ref["rgb"], f32["rgb"], nets_c, f"{name} rgb")
    # float16 outputs: the float32 results rounded to nearest even
    a32 = alpha32.cpu().numpy().reshape(-1, 1)
    assert np.array_equal(alphas.cpu().numpy().reshape(-1, 1), a32.astype(np.float16))
    assert np.array_equal(rgb.cpu().numpy().reshape(-1, 3), rgb32.astype(np.float16))
    want = (a32 * raw32 if weighted else raw32).astype(np.float16)
    assert np.array_equal(feats.cpu().numpy().reshape(-1, C), want)
    # the loop equals the fused call
    assert np.array_equal(loop_a, alphas.cpu().numpy().reshape(-1, 1)) and np.array_equal(loop_c, rgb.cpu().numpy().reshape(-1, 3))
    differ = int((loop_f != feats.cpu().numpy().reshape(-1, C)).sum())
    print(f"{name}: loop features differing from the fused call: {differ} of {loop_f.size}")
    assert differ == 0
    # two runs are bit-identical
    again = field.voxelize(lo, hi, vs, weighted, return_density=True, return_alpha32=True)
    assert all(torch.equal(a, b) for a, b in zip((feats, alphas, rgb, density, alpha32), again))


def test_closed_form_lattice_equals_given_axes_when_the_step_is_exact():
    """without axes the kernel forms float32(min + i voxel_size) in double: the same grids as with torch.arange's axes at a step
    that float32 holds exactly"""
    import ctypes as C
    from pixie_amd import _lib
    fq, _, shape, _, _ = lattice_case("5x7x9_contraction_identity")
    lo, hi, vs = LATTICES["5x7x9_contraction_identity"][:3]
    field = device_field(fq)
    want = field.voxelize(lo, hi, vs)
    outs = [torch.empty_like(t) for t in want]
    scratch = torch.empty(shape, dtype=torch.float32, device=DEV)
    desc = field.desc(lo, vs, shape, True)
    _lib.check(_lib.load().pixie_field_voxelize(C.byref(desc), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), None, scratch.data_ptr(),
                                                _lib.current_stream_ptr()), "pixie_field_voxelize")
    assert all(torch.equal(a, b) for a, b in zip(want, outs))


def test_files_are_the_references(tmp_path):
    from pixie_amd import field_query as FQ
    fq, x, shape, ref, _ = lattice_case("16c_aabb_identity")
    lo, hi, vs = LATTICES["16c_aabb_identity"][:3]
    field = device_field(fq)
    out = str(tmp_path / "grid" / "clip_features.npz")
    bounds = tuple(zip(lo, hi))
    assert FQ.extract_clip_voxel_grid(field, out, bounds, vs, alpha_weighted=True, run_outlier_filter=False) == out
    meta = np.load(out)
    assert sorted(meta.files) == sorted(["min_bounds", "max_bounds", "voxel_size", "feature_dim", "grid_shape", "alpha_weighted", "alpha_threshold_for_mask"])
    assert tuple(meta["grid_shape"]) == shape and int(meta["feature_dim"]) == 64 and bool(meta["alpha_weighted"]) and float(meta["voxel_size"]) == vs
    assert np.array_equal(meta["min_bounds"], np.asarray(lo)) and np.array_equal(meta["max_bounds"], np.asarray(hi))
    feats, alphas, rgb = field.voxelize(lo, hi, vs)
    for suffix, t, last in (("_features.npy", feats, 64), ("_alphas.npy", alphas, 1), ("_rgb.npy", rgb, 3)):
        a = np.load(out.replace(".npz", suffix))
        assert a.dtype == np.float16 and a.shape == shape + (last,) and np.array_equal(a, t.cpu().numpy())
    mask = np.load(out.replace(".npz", "_mask.npy"))
    a32, c32 = alphas.float().cpu().numpy()[..., 0], rgb.float().cpu().numpy()
    assert mask.dtype == np.bool_ and mask.shape == shape
    assert np.array_equal(mask, (a32 > np.float32(0.01)) & (((c32[..., 0] + c32[..., 1]) + c32[..., 2]) / np.float32(3) > np.float32(0.05)))
    grid, dmask, mn, mx = FQ.voxelize_to_device(field, bounds, vs, run_outlier_filter=False)
    assert tuple(grid.shape) == (1, 64) + shape and grid.dtype == torch.float32 and mn == lo and mx == hi
    assert torch.equal(grid[0].permute(1, 2, 3, 0), feats.float()) and np.array_equal(dmask.cpu().numpy(), mask)


def test_state_dict_and_tcnn_constructors_equal_from_arrays():
    """the two loaders against from_arrays on the matrices they should extract (key names per mlp.py:271-292, the tiny-cuda-nn
    layout per split_tcnn_params), both against the float64 restatement through the same lattice"""
    from pixie_amd import field_query as FQ
    rng = np.random.default_rng(99)
    lo, hi, vs = (-0.9,) * 3, (0.9,) * 3, 0.3
    G, A_DIM = 15, 8
    dcfg = dict(num_levels=4, base_res=4, max_res=32, log2_hashmap_size=8)
    fcfg = dict(num_levels=4, start_res=4, max_res=32, log2_hashmap_size=10, features_per_level=8, pe_n_freq=6, num_layers=2, feature_dim=24)
    head = [rng.standard_normal((64, 16 + G + A_DIM)) * 0.2, rng.standard_normal((64, 64)) * 0.2, rng.standard_normal((3, 64)) * 0.2]
    head_b = [rng.standard_normal(64) * 0.1, rng.standard_normal(64) * 0.1, rng.standard_normal(3) * 0.1]
    emb = rng.standard_normal((5, A_DIM)).astype(np.float32)
    # (a) nerfstudio torch keys, average appearance embedding
    dl, drows = R.levels("nerfstudio", 4, 4, 32, 8)
    fl, frows = R.levels("nerfstudio", 4, 4, 32, 10)
    dn = R.random_net(rng, dl, drows, 2, n_hidden=1, out_dim=1 + G)
    fn = R.random_net(rng, fl, frows, 8, n_frequencies=6, n_hidden=2, out_dim=24)
    sd = {"field.mlp_base.model.0.hash_table": dn["table"], "field.embedding_appearance.embedding.weight": emb,
          "feature_field.field.0.hash_table": fn["table"]}
    for prefix, ws, bs in (("field.mlp_base.model.1", dn["weights"], dn["biases"]), ("field.mlp_head", head, head_b),
                           ("feature_field.field.1", fn["weights"], fn["biases"])):
        for i, (w, b) in enumerate(zip(ws, bs)):
            sd[f"{prefix}.layers.{i}.weight"], sd[f"{prefix}.layers.{i}.bias"] = torch.from_numpy(np.asarray(w, np.float32)), torch.from_numpy(np.asarray(b, np.float32))
    cfg = dict(density=dcfg, feature=fcfg, use_average_appearance_embedding=True, contraction=True)
    got = FQ.FeatureFieldQuery.from_nerfstudio_state_dict(sd, cfg, device=DEV)
    cw, cb = FQ.fold_color_head(head, head_b, 16, G, R.sh(4, (0.5, 0.5, 0.5)), emb.astype(np.float64).mean(axis=0))
    fq = dict(density=dn, feature=fn, color=dict(levels=None, table=None, weights=cw, biases=cb, n_frequencies=0, n_extra=G, act="sigmoid"),
              world_to_nerf=np.eye(4, dtype=np.float32)[:3], contraction=True, average_init_density=1.0)
    want = device_field(fq)
    for a, b in zip(got.voxelize(lo, hi, vs), want.voxelize(lo, hi, vs)):
        assert torch.equal(a, b)
    x = np.stack(np.meshgrid(*[a.numpy() for a in FQ.lattice_axes(lo, hi, vs)], indexing="ij"), axis=-1).reshape(-1, 3)
    ref, f32 = R.field(fq, x, vs), R.field(fq, x, vs, np.float32)
    within(got.get_rgb(torch.from_numpy(x).to(DEV)).cpu().numpy(), ref["rgb"], f32["rgb"], [dn, fq["color"]], "state dict rgb")
    # (b) tiny-cuda-nn vectors: no biases, padded first / last layers, padding columns of ones
    dl, drows = R.levels("tcnn", 4, 4, 32, 8)
    fl, frows = R.levels("tcnn", 4, 4, 32, 10)
    dn = R.random_net(rng, dl, drows, 2, n_hidden=1, out_dim=1 + G, bias=False)
    fn = R.random_net(rng, fl, frows, 8, n_frequencies=6, n_hidden=2, out_dim=24, bias=False)

    def padded(w, rows, cols):                       # the matrix in the top-left corner, noise in the padding rows and columns
        out = (rng.standard_normal((rows, cols)) * 0.1).astype(np.float32)
        out[:w.shape[0], :w.shape[1]] = w
        return out

    ones_bias = lambda w, cols: w[:, cols:].astype(np.float64).sum(axis=1).astype(np.float32)
    d_w0, d_w1 = padded(dn["weights"][0], 64, 16), padded(dn["weights"][1], 16, 64)                  # 8 columns -> 16, 16 outputs
    f_w0, f_w2 = padded(fn["weights"][0], 64, 80), padded(fn["weights"][2], 32, 64)                  # 68 columns -> 80, 24 outputs -> 32
    c_w0, c_w2 = padded(head[0][:, :16 + G], 64, 32), padded(head[2], 16, 64)                        # 31 columns -> 32, 3 outputs -> 16
    c_w1 = head[1].astype(np.float32)
    params = dict(density=np.concatenate([d_w0.ravel(), d_w1.ravel(), dn["table"].ravel()]),
                  feature=np.concatenate([f_w0.ravel(), fn["weights"][1].ravel(), f_w2.ravel(), fn["table"].ravel()]),
                  color=np.concatenate([c_w0.ravel(), c_w1.ravel(), c_w2.ravel()]))
    tcfg = dict(density=dict(dcfg, num_layers=1), feature=fcfg, color=dict(num_layers=2), geo_feat_dim=G, contraction=True)
    got = FQ.FeatureFieldQuery.from_tcnn_params({k: torch.from_numpy(v) for k, v in params.items()}, tcfg, device=DEV)
    dn = dict(dn, biases=[ones_bias(d_w0, 8), None])
    fn_b = dict(fn, biases=[ones_bias(f_w0, 68), None, None])
    cw, cb = FQ.fold_color_head([c_w0[:, :31], c_w1, head[2]], [ones_bias(c_w0, 31), None, None], 16, G, R.sh(4, (0, 0, 0)))
    fq = dict(density=dn, feature=fn_b, color=dict(levels=None, table=None, weights=cw, biases=cb, n_frequencies=0, n_extra=G, act="sigmoid"),
              world_to_nerf=np.eye(4, dtype=np.float32)[:3], contraction=True, average_init_density=1.0)
    want = device_field(fq)
    for a, b in zip(got.voxelize(lo, hi, vs), want.voxelize(lo, hi, vs)):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="parameters"):
        FQ.FeatureFieldQuery.from_tcnn_params(dict(params, feature=torch.from_numpy(params["feature"][:-8])), tcfg, device=DEV)


def test_refusals():
    import ctypes as C
    from pixie_amd import _lib, field_query as FQ
    net, p, extra, _, _ = case("tcnn_T8_F2_h1_o16_bias")
    m = device_net(net)
    with pytest.raises(_lib.PixieHipError):
        m(torch.from_numpy(p))                                                       # a host tensor
    with pytest.raises(ValueError):
        FQ.HashMLP(None, None, [np.zeros((32, 3)), np.zeros((3, 32))], n_extra=3, device=DEV)      # hidden width 32
    with pytest.raises(ValueError):
        FQ.HashMLP(None, None, [np.zeros((64, 3)), np.zeros((1025, 64))], n_extra=3, device=DEV)   # output wider than 1024
    with pytest.raises(ValueError):
        FQ.HashMLP(None, None, [np.zeros((64, 3))] + [np.zeros((64, 64))] * 4 + [np.zeros((3, 64))], n_extra=3, device=DEV)   # 5 hidden layers
    with pytest.raises(ValueError):
        FQ.HashMLP(None, None, [np.zeros((64, 161)), np.zeros((3, 64))], n_extra=161, device=DEV)  # input row wider than 160
    lib = _lib.load()
    out = torch.empty((4, 16), dtype=torch.float32, device=DEV)
    pos = torch.from_numpy(p[:4]).to(DEV)

    def refused(change, word):
        d = m.desc()
        change(d)
        assert lib.pixie_hashmlp_forward(C.byref(d), pos.data_ptr(), None, 4, out.data_ptr(), None) != 0
        assert word in lib.pixie_last_error().decode(), lib.pixie_last_error()

    refused(lambda d: setattr(d, "features_per_level", 3), "features_per_level")
    refused(lambda d: setattr(d, "n_levels", 17), "n_levels")
    refused(lambda d: setattr(d, "n_hidden", 5), "hidden")
    refused(lambda d: setattr(d, "out_dim", 1025), "out_dim")
    refused(lambda d: setattr(d, "out_activation", 3), "out_activation")
    refused(lambda d: setattr(d, "table_rows", d.table_rows - 1), "does not fit")
    refused(lambda d: setattr(d, "n_extra", 160), "columns")
