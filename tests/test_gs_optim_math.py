"""CPU checks of pixie_amd/csrc/gs_optim_math.h (compiled for the host by tests/host_harness/gs_optim_math_host.cpp, g++
-ffp-contract=off): the arithmetic the kernels of gs_optim.hip run, with the bars of the GPU tests.

  * adam_element over five steps against torch.optim.Adam on the CPU at float64, yardstick the same optimiser at float32:
    max |header - float64| <= 3 y + 2 * 2^-24 * max |value| for p, exp_avg and exp_avg_sq of every group (the inputs of
    tests/test_gs_adam_hip.py: gradients from 1e-12 to 1e2, exact zeros in step 2, learning rates that change per step);
  * classify against the decisions of the torch restatement on every golden and synthetic case (each keeps its quantities a relative
    1e-3 away from the thresholds, asserted): which rows stay, are cloned, are split, and whose children stay;
  * split_position / split_scaling against the float64 restatement: 3 y + 4 * 2^-24 * max |value|, y the float32 restatement's distance.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _gs_optim_ref as gr
from tests import test_gs_adam_hip as ga

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_harness", "gs_optim_math_host.cpp")
FP, IP = C.POINTER(C.c_float), C.POINTER(C.c_int32)
fp = lambda a: a.ctypes.data_as(FP)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = str(tmp_path_factory.mktemp("gs_optim_host") / "libgs_optim_math_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-shared", SRC, "-o", lib])
    h = C.CDLL(lib)
    h.hh_gs_adam.argtypes = [C.c_int64, FP, FP, FP, FP] + [C.c_double] * 5
    h.hh_gs_classify.argtypes = [C.c_int64, FP, FP, FP, FP] + [C.c_double] * 4 + [C.c_int, IP]
    h.hh_gs_split.argtypes = [C.c_int64, FP, FP, FP, FP, FP, FP]
    h.hh_gs_stats_norm2.argtypes = [C.c_float, C.c_float]
    h.hh_gs_stats_norm2.restype = C.c_float
    return h


@pytest.mark.parametrize("n,degree", [(5, 3), (67, 3), (1000, 0)])
def test_adam_element_within_the_bar(host, n, degree):
    params, grads, ref64, ref32 = ga.reference(n, degree)
    p = {f: params[f].copy() for f in ga.FIELDS}
    m = {f: np.zeros_like(p[f]) for f in ga.FIELDS}
    v = {f: np.zeros_like(p[f]) for f in ga.FIELDS}
    worst = 0.0
    for step in range(ga.N_STEPS):
        t = step + 1
        for f in ga.FIELDS:
            if p[f].size == 0:
                continue
            lr = ga.BASE_LR[f] * ga.LR_FACTOR[step]
            g = np.ascontiguousarray(grads[step][f])
            host.hh_gs_adam(p[f].size, fp(p[f]), fp(g), fp(m[f]), fp(v[f]), 0.9, 0.999, 1e-15, lr / (1 - 0.9 ** t), (1 - 0.999 ** t) ** 0.5)
            for q, arr in enumerate((p[f], m[f], v[f])):
                want = ref64[step][f][q].numpy()
                d = np.abs(arr.astype(np.float64) - want).max()
                y = np.abs(ref32[step][f][q].numpy().astype(np.float64) - want).max()
                bar = 3 * y + 2 * 2.0 ** -24 * np.abs(want).max()
                worst = max(worst, d / bar)
                assert d <= bar, (step, f, q, d, y, bar)
    print(f"adam_element N={n} degree={degree}: worst d / bar {worst:.3f}")


@pytest.mark.parametrize("name", list(gr.CASES))
def test_classify_and_split_against_the_restatement(host, name):
    mss = gr.CASES[name][2]
    state = gr.make_case(name)
    assert min(gr.margins(state).values()) > 1e-3
    n = state["xyz"].shape[0]
    z_all = state.pop("z")
    z = z_all[:2 * gr.split_count(state)]
    args = (gr.MAX_GRAD, gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, mss, z)
    r32, r64 = gr.densify_ref(state, *args, torch.float32), gr.densify_ref(state, *args, torch.float64)
    flags = np.zeros(n, np.int32)
    host.hh_gs_classify(n, fp(state["xyz_gradient_accum"]), fp(state["denom"]), fp(state["scaling"]), fp(state["opacity"]), gr.MAX_GRAD,
                        gr.MIN_OPACITY, gr.EXTENT, gr.PERCENT_DENSE, 1 if mss else 0, flags.ctypes.data_as(IP))
    rows = np.arange(n)
    kept, clone, child, split = (rows[(flags & b) != 0] for b in (1, 2, 4, 8))
    want_src = r32["source_index"].numpy()
    assert np.array_equal(np.concatenate([kept, clone, child, child]), want_src)
    assert len(split) == r32["n_split"] and (len(kept), len(clone), 2 * len(child)) == r32["counts"][:3]
    made = int(((flags & 16) != 0).sum())
    assert (n - len(split) - len(kept)) + (made - len(clone)) + 2 * (len(split) - len(child)) == r32["counts"][3]
    if len(child) == 0:
        return
    # the children: z row copy * n_split + rank among the split
    rank = {int(i): k for k, i in enumerate(split)}
    n_old = len(kept) + len(clone)
    for copy in range(2):
        zz = np.ascontiguousarray(z[[copy * len(split) + rank[int(i)] for i in child]])
        src = [np.ascontiguousarray(state[f][child]) for f in ("xyz", "scaling", "rotation")]
        out_xyz, out_scaling = np.zeros((len(child), 3), np.float32), np.zeros((len(child), 3), np.float32)
        host.hh_gs_split(len(child), fp(src[0]), fp(src[1]), fp(src[2]), fp(zz), fp(out_xyz), fp(out_scaling))
        lo = n_old + copy * len(child)
        for f, got in (("xyz", out_xyz), ("scaling", out_scaling)):
            w64 = r64[f].numpy()[lo:lo + len(child)]
            d = np.abs(got.astype(np.float64) - w64).max()
            y = np.abs(r32[f].numpy()[lo:lo + len(child)].astype(np.float64) - w64).max()
            assert d <= 3 * y + 4 * 2.0 ** -24 * np.abs(w64).max(), (f, copy, d, y)


def test_stats_norm(host):
    assert host.hh_gs_stats_norm2(3.0, 4.0) == 5.0 and host.hh_gs_stats_norm2(0.0, 0.0) == 0.0
    assert abs(host.hh_gs_stats_norm2(1e-4, -2e-4) - np.hypot(1e-4, 2e-4)) <= 2 * np.spacing(np.float32(2.2e-4))
