"""What the hash-grid network modules share on the Python side: field_query (HashMLP), field_training (TrainableHashMLP) and
density_field (HashMLPDensityField) fill the same level table, size and align the same scratch, and bind the same kind of grads struct."""
import ctypes as C

import torch

from . import _lib

SCRATCH_SHIFT_OFFSET = 4                         # bytes into the scratch (pixie_hip.h): int32 shift s,
SCRATCH_STATE_OFFSET = 8                         # int32 state


def fill_levels(desc, levels) -> None:           # desc.level[l] from a LEVEL_DTYPE array
    for l, lv in enumerate(levels):
        d = desc.level[l]
        d.scale, d.shift = float(lv["scale"]), float(lv["shift"])
        d.res, d.size, d.offset, d.dense = int(lv["res"]), int(lv["size"]), int(lv["offset"]), int(lv["dense"])


def train_bytes(entry_name: str, desc, n: int):
    """(saved_bytes, scratch_bytes) of the *_train_bytes entry point `entry_name`"""
    saved, scratch = C.c_int64(), C.c_int64()
    _lib.check(getattr(_lib.load(), entry_name)(C.byref(desc), n, C.byref(saved), C.byref(scratch)), entry_name)
    return saved.value, scratch.value


def aligned_scratch(nbytes: int, device) -> torch.Tensor:      # 256-byte aligned, as the backward entry points require
    scratch = torch.empty(nbytes + 256, dtype=torch.uint8, device=device)
    return scratch[(-scratch.data_ptr()) % 256:][:nbytes]


def bind_layer_grads(g, tensors, need, n_layers: int):
    """tensors: the n_layers weights, then the n_layers biases (None where absent); need[j]: whether tensors[j] wants a gradient.
    Allocates those gradients, puts their addresses into g.d_weight / g.d_bias and returns them (or None) in the order of `tensors`."""
    grads = [torch.empty_like(t) if t is not None and need[j] else None for j, t in enumerate(tensors)]
    for j, gt in enumerate(grads):
        if gt is not None:
            (g.d_weight if j < n_layers else g.d_bias)[j % n_layers] = gt.data_ptr()
    return grads


def bias_list(bias_layers, biases, n_layers: int):             # one bias or None per layer, from the biases that exist and their layers
    out = [None] * n_layers
    for slot, i in enumerate(bias_layers):
        out[i] = biases[slot]
    return out


def require_device_params(module: torch.nn.Module, device, who: str) -> None:
    for p in module.parameters():
        if p.device != device or p.dtype != torch.float32 or not p.is_contiguous():
            raise _lib.PixieHipError(f"{who}: parameters must stay contiguous float32 tensors on {device}")
