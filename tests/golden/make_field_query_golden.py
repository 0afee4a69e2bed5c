#!/usr/bin/env python
"""Writes tests/golden/field_query_ns.npz: the "nerfstudio" grid convention of pixie_amd.field_query pinned to the REFERENCE's own
modules.

Imports nerfstudio's torch fallbacks from the reference tree (third_party/nerfstudio) and records inputs, state-dict arrays and
outputs of `MLPWithHashEncoding(implementation="torch")` (field_components/mlp.py:187-295, i.e. HashEncoding.pytorch_fwd +
MLP.pytorch_fwd) for two small configurations, and of `SHEncoding(levels=4).pytorch_fwd` at a handful of directions.  Nothing of the
reference's text is in this file; it runs on the CPU.

Needs /root/reference and the packages nerfstudio's field components import (jaxtyping, rich).  The build container lacks
jaxtyping, so the fixture has NOT been produced yet and no test reads it: until someone runs this where the import works, the
"nerfstudio" convention is checked against the NumPy restatement of tests/_field_query_ref.py alone.
"""
import os
import sys

import numpy as np
import torch

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REF, "third_party", "nerfstudio"))

from nerfstudio.field_components.encodings import SHEncoding  # noqa: E402
from nerfstudio.field_components.mlp import MLPWithHashEncoding  # noqa: E402

CASES = {"a": dict(num_levels=4, min_res=4, max_res=32, log2_hashmap_size=8, features_per_level=2, num_layers=2, layer_width=64, out_dim=16),
         "b": dict(num_levels=6, min_res=16, max_res=128, log2_hashmap_size=10, features_per_level=8, num_layers=3, layer_width=64, out_dim=20)}


def main():
    out = {}
    rng = np.random.default_rng(0)
    for name, cfg in CASES.items():
        torch.manual_seed(1 + len(out))
        net = MLPWithHashEncoding(implementation="torch", hash_init_scale=1.0, **cfg)
        pts = rng.random((300, 3)).astype(np.float32)
        pts[:4] = [[0, 0, 0], [1, 1, 1], [0.25, 0.5, 0.75], [0.5, 0.5, 0.5]]        # cell boundaries: the scaled position is integral
        with torch.no_grad():
            y = net(torch.from_numpy(pts))
        for k, v in cfg.items():
            out[f"{name}.cfg.{k}"] = np.int64(v)
        out[f"{name}.points"] = pts
        out[f"{name}.out"] = y.numpy()
        out[f"{name}.scalings"] = net.model[0].scalings.numpy()
        for k, v in net.state_dict().items():
            out[f"{name}.sd.{k}"] = v.numpy()
    dirs = np.concatenate([np.full((1, 3), 0.5), np.zeros((1, 3)), rng.standard_normal((6, 3))]).astype(np.float32)
    out["sh.directions"] = dirs
    out["sh.out"] = SHEncoding(levels=4, implementation="torch").pytorch_fwd(torch.from_numpy(dirs)).numpy()
    path = os.path.join(HERE, "field_query_ns.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, keys {sorted(out)[:6]} ...")


if __name__ == "__main__":
    main()
