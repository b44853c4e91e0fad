"""The Gaussian window of the composed paths (``structural.ssim_composed``, ``slice_bias.field_composed``,
``evaluate.ssim3d_composed``) and the SSIM map the first and the last share: torch expressions that the kernels of
csrc/window.h, csrc/structural.hip, csrc/slice_bias.hip and csrc/evaluate.hip follow operation for operation.
"""
import math
from typing import Sequence

import torch
import torch.nn.functional as F


def gaussian_taps(sigma: float, radius: int, dtype: torch.dtype = torch.float64, device=None) -> torch.Tensor:
    """g[t] = exp(-(t - radius)^2 / (2 sigma^2)), t = 0 .. 2 radius, normalised to sum 1 in double and rounded to ``dtype`` once
    (what the kernels' host code does)."""
    g = [math.exp(-float((t - radius) * (t - radius)) / (2.0 * sigma * sigma)) for t in range(2 * radius + 1)]
    total = 0.0
    for v in g:
        total += v
    return torch.tensor([v / total for v in g], dtype=torch.float64).to(dtype=dtype, device=device)


def window(a: torch.Tensor, taps: Sequence[float], dims: int = 2) -> torch.Tensor:
    """S(a) with zero padding over the last ``dims`` (2 or 3) dimensions, along x, then y, then z: explicit shifted slices in tap
    order, acc = 0; acc = acc + g[t] a[. + t - radius], so that a kernel can follow it operation for operation."""
    radius = (len(taps) - 1) // 2
    out = a
    for axis in range(-1, -dims - 1, -1):
        n = a.shape[axis]
        pad = [0, 0] * (-axis - 1) + [radius, radius]
        padded = F.pad(out, pad)
        out = torch.zeros_like(a)
        for t, g in enumerate(taps):
            out = out + g * padded.narrow(axis, t, n)
    return out


def ssim_map(i: torch.Tensor, j: torch.Tensor, valid: torch.Tensor, taps: Sequence[float], c1, c2, dims: int = 2) -> torch.Tensor:
    """The SSIM of Wang et al. 2004 with its window renormalised by the mask's share of it (the definition:
    nesvor_amd/structural.py), at ``valid`` and exactly 0 elsewhere.  ``i`` and ``j`` are 0 off ``valid``."""
    zero, one = torch.zeros_like(i), torch.ones_like(i)
    wt = torch.where(valid, window(valid.to(i.dtype), taps, dims), one)
    mu_i, mu_j = window(i, taps, dims) / wt, window(j, taps, dims) / wt
    var_i = window(i * i, taps, dims) / wt - mu_i * mu_i
    var_j = window(j * j, taps, dims) / wt - mu_j * mu_j
    cov = window(i * j, taps, dims) / wt - mu_i * mu_j
    num = (2 * mu_i * mu_j + c1) * (2 * cov + c2)
    den = (mu_i * mu_i + mu_j * mu_j + c1) * (var_i + var_j + c2)
    return torch.where(valid, num / den, zero)
