"""Dataset ops: the fused batch-assembly kernel (``csrc/kernels/augment.hip``).

``augment`` turns N rows of an int32 table into the stem's input in one pass over the output: gather the source image,
crop (zero padded) or resize (bilinear) to S x S, flip, normalise, round to bf16 and lay out as "nhwc8" or as the
space-to-depth image "s2d" that ``stem_conv_s2d`` reads. A uint8 ``src`` on the GPU runs the HIP kernel; one on the
host runs ``ops.reference.augment``, the same definition in torch (float64), which is also the kernel's oracle.
"""
from __future__ import annotations

import torch

from k8s_amd.ops import reference as ref
from k8s_amd.ops._ext import load as _load_ext

LAYOUTS = ("nhwc8", "s2d")


def norm_constants(mean, std):
    """(a, b) with a_c = fp32(1 / std_c), b_c = fp32(-mean_c / std_c), as Python floats (0..255 scale)."""
    a = [float(torch.tensor(1.0 / float(s), dtype=torch.float32)) for s in std]
    b = [float(torch.tensor(-float(m) / float(s), dtype=torch.float32)) for m, s in zip(mean, std)]
    return a, b


def launches() -> int:
    """Augmentation kernels this process has launched (a rejected call launches none)."""
    return int(_load_ext().augment_launches())


def augment(src: torch.Tensor, table: torch.Tensor, a, b, S: int, layout: str = "s2d") -> torch.Tensor:
    """``src`` uint8 [M, Hs, Ws, 3]; ``table`` int32 [N, 6] on the host, rows (src index, y0, x0, h, w, flip);
    ``a``, ``b``: ``norm_constants``. Returns bf16 [N, S, S, 8] ("nhwc8") or [N, S/2+3, S/2+3, 16] ("s2d"). The GPU
    binding validates every table row on the host before anything is launched and raises on the first bad one."""
    if src.is_cuda:
        return _load_ext().augment(src, table, [float(v) for v in a], [float(v) for v in b], int(S), layout)
    return ref.augment(src, table, a, b, int(S), layout)
