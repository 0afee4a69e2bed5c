#!/usr/bin/env python
"""Times pixie_amd.occupancy.occupancy_mask on the scene builder of tests/_occupancy_ref.py at 64^3 and 128^3 (float16 arrays
already on the device, default parameters), and the NumPy / scipy restatement of the same file on this host's CPU where
scipy is importable (without scipy the device timing still runs and the table says that the host row is missing).  Device events around one call on torch's current stream; warm-up, then the median of `--reps` calls.
Recorded, not asserted: writes a table (default profiles/occupancy_mask_table.txt) with the slow-path voxel counts.

The reference's own route (Open3D remove_statistical_outlier + cluster_dbscan on the host) cannot be timed where Open3D is not
installed; the table says so instead of quoting a number.

    python scripts/profile_occupancy.py [--scenes scene64 scene128] [--reps 20] [--warmup 5] [--out PATH] [--no-host]
"""
import argparse
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from pixie_amd.occupancy import occupancy_mask  # noqa: E402
from tests import _occupancy_ref as R  # noqa: E402  (the suite's scene builder: numpy only; its restatement imports scipy when called)


def scipy_importable():
    try:
        import scipy.spatial  # noqa: F401
        import scipy.sparse.csgraph  # noqa: F401
        return True
    except ImportError:
        return False


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["scene64", "scene128"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the CPU restatement")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occupancy_mask_table.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("profile_occupancy: no HIP device is visible; this measurement has no CPU form")
    dev = torch.device("cuda:0")
    host = not args.no_host and scipy_importable()
    rows = []
    for name in args.scenes:
        scene = R.build_scene(name)
        alphas, rgb = torch.from_numpy(scene["alphas"]).to(dev), torch.from_numpy(scene["rgb"]).to(dev)
        for keep in ("non_noise", "largest"):
            call = lambda: occupancy_mask(alphas, rgb, scene["voxel_size"], scene["min_bounds"], axes=scene["axes"], keep=keep, return_stats=True)
            times = []
            for it in range(args.warmup + args.reps):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                mask, stats = call()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times.append(e0.elapsed_time(e1))
            c = stats.counts
            rows.append(f"{name:>9} {keep:<10} HIP   median {statistics.median(times):8.3f} ms   min {min(times):8.3f}   max {max(times):8.3f}   "
                        f"candidates {c['after_gray']}, after B {c['after_outlier_removal']}, after C {c['after_cluster_removal']}, "
                        f"slow-path voxels {c['slow_path_voxels']} ({100.0 * c['slow_path_voxels'] / max(c['after_gray'], 1):.1f} %), clusters {c['n_clusters']}")
        if host:
            t0 = time.perf_counter()
            ref = R.reference(scene)
            dt = (time.perf_counter() - t0) * 1e3
            same = bool((mask.cpu().numpy() == ref["largest"]).all())
            rows.append(f"{name:>9} {'both rules':<10} host  one run {dt:10.1f} ms   (cKDTree k-NN + query_pairs + connected_components, single-threaded); "
                        f"masks equal: {same}")
    head = [f"occupancy_mask, default parameters (nb_neighbors 50, std_ratio 4, eps 5 voxels, min_cluster_pts 10), float16 inputs resident on the device;",
            f"{args.reps} timed calls after {args.warmup} warm-up; device events around the whole call (allocations, three memsets, 14 kernel launches, no synchronise inside);",
            "the reference's own route -- Open3D remove_statistical_outlier + cluster_dbscan -- is NOT timed: Open3D is not installed where this ran;",
            f"device: {torch.cuda.get_device_name(0)}"]
    if not host:
        head.append("the NumPy / scipy restatement on the host is not timed either: " + ("--no-host" if args.no_host else "scipy is not importable here"))
    head.append("")
    text = "\n".join(head + rows) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
