"""Structural outlier exclusion for the classical reconstruction (the ``svr`` command): the step IRTK / SVRTK and NiftyMIC run
after the EM weights.  The robust statistics (nesvor_amd/robust.py) judge every pixel on its own residual; a slice with
plausible intensities in the wrong place, or a part of a slice that lies over the wrong anatomy, passes that test.  Here a
slice is compared with the structure the volume predicts for it.  The reference project has no counterpart: the definition
is this module's.

Definition.  With sim = A x, y the acquired slices, scale_k the robust slice scales (ones without them) and L the dynamic
range (1: the stacks are normalised by their 0.99 quantile): I = scale_k y and J = sim on the valid pixels, 0 elsewhere, v the
validity as 0 / 1.  S(a) is the separable 11-tap Gaussian window (sigma 1.5, ``gaussian_taps``) with zero padding, along x
first, the taps added in ascending order from 0.  With Wt = S(v) (1 off the mask; at a valid pixel Wt >= g[5]^2 > 0)
    muI = S(I) / Wt,  muJ = S(J) / Wt,  sI = S(I I) / Wt - muI^2,  sJ = S(J J) / Wt - muJ^2,  sIJ = S(I J) / Wt - muI muJ,
    ssim = (2 muI muJ + C1) (2 sIJ + C2) / ((muI^2 + muJ^2 + C1) (sI + sJ + C2)),   C1 = (0.01 L)^2,  C2 = (0.03 L)^2
at valid pixels and exactly 0 elsewhere: the SSIM of Wang et al. 2004 with its window renormalised by the mask's share of it.
Eight sums per slice over its valid pixels, {n, sum ssim, #(ssim < t_local), sum I, sum J, sum I^2, sum J^2, sum I J}, give the
signed correlation r_k = cov / sqrt(varI varJ) (0 where varI varJ <= 1e-12) of a slice with its simulation.

Decisions.  A pixel is kept where it is valid and ssim >= t_local; a slice where it has a valid pixel and r_k >= t_global.  The
weight multiplier is their product.  Decisions are recomputed every round and are not sticky: a pixel dropped against an
early blurry volume comes back.

One round (``StructuralExclusion.update``) needs the map and the sums (``ssim_stats``): on HIP fp32 tensors one pass of
``torch.ops.nesvor.structural_ssim`` (csrc/structural.hip); ``NESVOR_STRUCTURAL=composed``, host tensors and other dtypes take
the same formulas as a torch expression (``ssim_composed``, the fp64 yardstick of tests/test_structural.py).  What follows
the sums is a few operations on n-vectors in fp64, written with ``torch.where``: a round reads nothing back to the host.
"""
import os
from typing import Optional, Tuple

import torch

from . import window as _w

RADIUS = 5
SIGMA = 1.5
N_STATS = 8
MIN_VAR_PRODUCT = 1e-12  # below it a slice (or its simulation) is flat: r = 0


def gaussian_taps(dtype: torch.dtype = torch.float64, device=None) -> torch.Tensor:
    return _w.gaussian_taps(SIGMA, RADIUS, dtype, device)


def _fused(sim: torch.Tensor) -> bool:
    return os.environ.get("NESVOR_STRUCTURAL", "") != "composed" and sim.is_cuda and sim.dtype == torch.float32


def _window(a: torch.Tensor, taps) -> torch.Tensor:
    return _w.window(a, taps, 2)


def ssim_composed(sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], scale: torch.Tensor, threshold: float = 0.4,
                  dynamic_range: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The map (as ``sim``) and the eight sums per slice (n,8) in fp64.  The per-pixel arithmetic is in the tensors' dtype, in
    the order the kernel evaluates it; the sums are taken in fp64."""
    n = sim.shape[0]
    valid = torch.ones_like(sim, dtype=torch.bool) if mask is None else mask.reshape(sim.shape).bool()
    c1, c2 = (0.01 * dynamic_range) ** 2, (0.03 * dynamic_range) ** 2
    taps = gaussian_taps(sim.dtype).tolist()  # host numbers: exactly the dtype's values
    zero = torch.zeros_like(sim)
    i = torch.where(valid, scale.view(n, *([1] * (sim.ndim - 1))) * y, zero)
    j = torch.where(valid, sim, zero)
    v = valid.to(sim.dtype)
    ssim = _w.ssim_map(i, j, valid, taps, c1, c2, 2)
    below = (valid & (ssim < threshold)).to(sim.dtype)
    terms = (v, ssim, below, i, j, i * i, j * j, i * j)
    stats = torch.stack([t.double().flatten(1).sum(1) for t in terms], dim=1)
    return ssim, stats


def ssim_stats(sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], scale: torch.Tensor, threshold: float = 0.4,
               dynamic_range: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    if _fused(sim):
        return torch.ops.nesvor.structural_ssim(sim.contiguous(), y.contiguous(),
                                                None if mask is None else mask.reshape(sim.shape).contiguous(),
                                                scale.contiguous(), float(threshold), float(dynamic_range))
    return ssim_composed(sim, y, mask, scale, threshold, dynamic_range)


def slice_ncc(stats: torch.Tensor) -> torch.Tensor:
    """r_k (n) in fp64 from the sums: the signed correlation of I and J over a slice's valid pixels; 0 for a slice without a
    valid pixel and where varI varJ <= 1e-12."""
    n_k = stats[:, 0]
    n_safe = torch.where(n_k > 0, n_k, torch.ones_like(n_k))
    mean_i, mean_j = stats[:, 3] / n_safe, stats[:, 4] / n_safe
    cov = stats[:, 7] / n_safe - mean_i * mean_j
    var_i = stats[:, 5] / n_safe - mean_i * mean_i
    var_j = stats[:, 6] / n_safe - mean_j * mean_j
    product = var_i * var_j
    ok = product > MIN_VAR_PRODUCT
    return torch.where(ok, cov / torch.sqrt(torch.where(ok, product, torch.ones_like(product))), torch.zeros_like(product))


class StructuralExclusion:
    """The thresholds and, after ``update``, the decisions as device tensors: ``ssim`` (as the slices), ``stats`` (n,8) fp64,
    ``ncc`` (n) fp64, ``pixel_keep`` (as the slices, bool) and ``slice_keep`` (n, bool)."""

    def __init__(self, local_ssim: float = 0.4, global_ncc: float = 0.5, dynamic_range: float = 1.0, rounds: int = 3) -> None:
        self.local_ssim, self.global_ncc, self.dynamic_range = float(local_ssim), float(global_ncc), float(dynamic_range)
        self.rounds = int(rounds)  # of ``svr.reconstruct_volume`` when the robust statistics, which bring their own number, are off
        self.ssim = self.stats = self.ncc = self.pixel_keep = self.slice_keep = None

    def update(self, sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor],
               scale: Optional[torch.Tensor] = None) -> "StructuralExclusion":
        if scale is None:
            scale = torch.ones(sim.shape[0], dtype=sim.dtype, device=sim.device)
        self.ssim, self.stats = ssim_stats(sim, y, mask, scale, self.local_ssim, self.dynamic_range)
        self.ncc = slice_ncc(self.stats)
        keep = self.ssim >= self.local_ssim
        self.pixel_keep = keep if mask is None else keep & mask.reshape(sim.shape).bool()
        self.slice_keep = (self.stats[:, 0] > 0) & (self.ncc >= self.global_ncc)
        return self

    def weights(self) -> torch.Tensor:
        """The multiplier of the data term's pixel weight: pixel_keep times its slice's slice_keep, as the slices' dtype."""
        keep = self.pixel_keep & self.slice_keep.view(-1, *([1] * (self.pixel_keep.ndim - 1)))
        return keep.to(self.ssim.dtype)

    def pixel_share(self) -> torch.Tensor:
        """The share (n, fp64) of a slice's valid pixels with ssim >= the local threshold; 0 for a slice without one."""
        n_k = self.stats[:, 0]
        ok = n_k > 0
        return torch.where(ok, 1 - self.stats[:, 2] / torch.where(ok, n_k, torch.ones_like(n_k)), torch.zeros_like(n_k))
