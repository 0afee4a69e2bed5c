"""Builds pixie_amd/libpixie_hip.so (gfx950) in-tree with hipcc.

`python -m pixie_amd.build` or `__graft_entry__.build()`.  hipcc cross-compiles without a
GPU; the resulting .so is git-ignored but travels with the working tree.
"""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libpixie_hip.so")
LIB_DIAG = os.path.join(HERE, "libpixie_hip_diag.so")   # same sources + -DPIXIE_DIAG (tests, profilers)
ARCH = "gfx950"
SOURCES = ["common.hip", "mpm.hip", "unet_ops.hip", "conv3d_mfma.hip", "conv3d_f16x3.hip", "unet_exec.hip", "projector_fused.hip", "field_transfer.hip", "particle_filling.hip", "raster.hip", "raster_backward.hip", "scene_ingest.hip", "knn.hip", "photometric.hip", "gs_optim.hip", "occupancy.hip", "part_segmentation.hip", "field_query.hip", "field_query_backward.hip", "ray_render.hip", "ray_sample.hip", "density_field.hip"]
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wall",
         "-Wno-unused-function", "-Wno-unused-variable"]
# Per-file flags.  mpm.hip: hipcc's SLP vectoriser turns a third of the fused MPM kernel's fp32 arithmetic into packed
# v_pk_* instructions, each of which needs its operands in aligned register pairs: 168 VGPRs (3 waves per SIMD) and
# ~340 extra v_mov per wave to shuffle values into place.  A packed op issues in ~5.7 cycles against 4.5 for a scalar one
# (scripts/microbench/valu_rate.hip), so the packing saves little even before the moves.  Without it the same kernel needs
# 96 VGPRs (5 waves per SIMD) and no spills.
# raster.hip: no fused multiply-adds, so that the device rounds as raster_math.h does when g++ builds it for tests/test_raster_math.py
# (-ffp-contract=off there too) and as a float32 NumPy evaluation does: what is left between the kernels and that evaluation is
# the device's expf alone, and the scales / rotations route is bit-equal to the cov3D route fed with the helper's covariances
# (tests/test_raster_hip.py).  The price, a mul + add where an fma would do (about four per sample in the render loop), is unmeasured.
# raster_backward.hip: the same, for raster_grad_math.h and tests/test_raster_grad_math.py; its walk also repeats the forward's blend
# operation for operation, which only an unfused build does with the forward's bits.
# scene_ingest.hip: the same, for ingest_math.h and tests/test_scene_ingest_math.py; the kernels move ~480 bytes per Gaussian, so
# the unfused arithmetic is not what bounds them.
# knn.hip: the same, for knn_math.h and tests/test_knn_math.py: distCUDA2 is bit-equal to a float32 brute force in the same order.
# gs_optim.hip: the same, for gs_optim_math.h: the Adam update rounds in the order torch's kernels do; it moves 28 bytes per
# element, so the unfused arithmetic is not what bounds it.
# occupancy.hip: the same, for occupancy_math.h and tests/test_occupancy_math.py: the eps-ball test of the cluster filter is the
# float64 expression ((dx dx + dy dy) + dz dz) < eps eps as written, which decides lattice pairs at exactly eps by its rounding.
# part_segmentation.hip: the same, for part_seg_math.h and tests/test_part_seg_math.py: a lane's share of a dot product is the
# float32 chain acc = acc + f q as written, so the host build of the header carries the device's bits up to expf; the kernel moves
# 2 C bytes per masked voxel against 2 K C flops, so the unfused arithmetic is not what bounds it.
# field_query.hip: the same, for hashgrid_math.h and tests/test_hashgrid_math.py: lattice coordinate, affine, contraction, selector and
# the scaled position of every level round as a float32 NumPy evaluation does, so cells and selectors are equal; the layers run on
# matrix instructions, which fuse regardless.
# field_query_backward.hip: the same: its scatter re-derives the forward's cells and corner weights from hashgrid_math.h and must land
# on the forward's rows with the forward's weights; hashgrid_grad_math.h's fixed-point conversion is exact either way.
# ray_render.hip: the same, for ray_render_math.h and tests/test_ray_render_math.py: weights, depth quotient and median rule round as
# g++ rounds the header (its exp is a double exp rounded once on both sides); the feature kernels move 4 bytes per multiply-add, so the unfused arithmetic is not what bounds them.
# ray_sample.hip: the same, for ray_sample_math.h and tests/test_ray_sampling_math.py: stratified bins, spacing maps, deltas, positions and
# the cdf interpolation round as float32 NumPy does, so a level's bins are bit-equal to torch's on the same random numbers.
# density_field.hip: the same, for hashgrid_math.h (front end, cells, corner weights: the forward and the scatter land on the same rows)
# and density_field_math.h; the layers are explicit fmaf, which the flag leaves alone.
EXTRA_FLAGS = {"mpm.hip": ["-fno-slp-vectorize"], "raster.hip": ["-ffp-contract=off"], "raster_backward.hip": ["-ffp-contract=off"],
               "scene_ingest.hip": ["-ffp-contract=off"], "knn.hip": ["-ffp-contract=off"], "gs_optim.hip": ["-ffp-contract=off"],
               "occupancy.hip": ["-ffp-contract=off"], "part_segmentation.hip": ["-ffp-contract=off"], "field_query.hip": ["-ffp-contract=off"],
               "field_query_backward.hip": ["-ffp-contract=off"], "ray_render.hip": ["-ffp-contract=off"],
               "ray_sample.hip": ["-ffp-contract=off"], "density_field.hip": ["-ffp-contract=off"]}


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP extension cannot be built")
    return exe


def _newer(target: str, deps) -> bool:
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _uses_diag(path: str, seen=None) -> bool:
    """Whether the source, or a csrc/ file it includes with quotes (followed recursively), mentions PIXIE_DIAG."""
    seen = set() if seen is None else seen
    path = os.path.normpath(path)
    if path in seen or not os.path.exists(path):
        return False
    seen.add(path)
    with open(path) as f:
        text = f.read()
    if "PIXIE_DIAG" in text:
        return True
    here = os.path.dirname(path)
    return any(_uses_diag(os.path.join(here, inc), seen) for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M)
               if os.path.normpath(os.path.join(here, inc)).startswith(CSRC + os.sep))


def build(force: bool = False, verbose: bool = False) -> str:
    """Compiles csrc/*.hip into libpixie_hip.so (the product) and libpixie_hip_diag.so (the same sources with -DPIXIE_DIAG:
    + pixie_mpm_phase / pixie_mpm_kernel_times / pixie_conv_kernel_variant and the kernel trace buffer, for tests and
    profilers).  Only the sources that mention PIXIE_DIAG, themselves or in a csrc/ header they include, are compiled twice.  `force` (or PIXIE_FORCE_BUILD=1 in the
    environment) recompiles everything and prints hipcc's wall time per file, so that a cold build is observable."""
    force = force or os.environ.get("PIXIE_FORCE_BUILD", "") not in ("", "0")
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(HERE, "..", "include", "pixie_hip.h"))
    hipcc = _hipcc()
    objs = {False: [], True: []}
    procs = []
    for src in SOURCES:
        sp = os.path.join(CSRC, src)
        if not os.path.exists(sp):
            continue
        for diag in ((False, True) if _uses_diag(sp) else (False,)):
            obj = os.path.join(OBJ, src.replace(".hip", ".diag.o" if diag else ".o"))
            objs[diag].append(obj)
            if not force and _newer(obj, [sp, os.path.abspath(__file__)] + headers):
                continue
            cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + (["-DPIXIE_DIAG"] if diag else []) + ["-c", sp, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((src + (" -DPIXIE_DIAG" if diag else ""), time.time(),
                          subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
        if not _uses_diag(sp):
            objs[True].append(objs[False][-1])
    failed = False
    for src, t0, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            failed = True
            sys.stderr.write(f"--- hipcc failed on {src} ---\n{out}\n")
        else:
            if force or verbose:
                print(f"hipcc {src}: done {time.time() - t0:.0f} s after launch (all files compile in parallel)", flush=True)
            if verbose and out.strip():
                print(out)
    if failed:
        raise RuntimeError("hipcc failed; see messages above")
    for diag, lib in ((False, LIB), (True, LIB_DIAG)):
        if force or procs or not _newer(lib, objs[diag]):
            cmd = [hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib] + objs[diag]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    if force or verbose:
        print(f"built {LIB} ({os.path.getsize(LIB)} bytes) and {LIB_DIAG} ({os.path.getsize(LIB_DIAG)} bytes) from {len(procs)} compilations", flush=True)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
