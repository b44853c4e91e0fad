"""Robust statistics for the classical reconstruction (the ``svr`` command): outlier rejection and per-slice intensity scales
by the EM scheme of Kuklisova-Murgasova et al. 2012 (the one IRTK / SVRTK and NiftyMIC use).  The reference project has no
counterpart - its ``SRR`` accepts a pixel weight ``p`` that something else must supply - so the definition is this module's.

Model.  With x the current volume, sim = A x and y the acquired slices, the residual of a valid pixel of slice k is
e = scale_k y - sim.  It is drawn from a mixture of a Gaussian inlier N(0, sigma2), proportion c, and a uniform outlier of
density m; the posterior of "inlier" is
    p = c g / (c g + (1 - c) m),     g = exp(-e^2 / (2 sigma2)) / sqrt(2 pi sigma2).
A slice's potential pot_k = sqrt(sum (1 - p)^2 / n_k) is in turn drawn from a mixture of two Gaussians (inlier slices, outlier
slices); the posterior of "inlier slice" is the slice weight.  Each slice's scale is the weighted least-squares fit of
scale_k y to sim.

One round (``RobustStatistics.update``) needs p and seven sums per slice, {n, sum p, sum p e^2, sum (1 - p)^2, sum p y sim,
sum p y^2, sum e^2} (``estep``): on HIP fp32 tensors one pass of ``torch.ops.nesvor.robust_estep`` (csrc/robust.hip);
``NESVOR_ROBUST=composed``, host tensors and other dtypes take the same formulas as a torch expression (``estep_composed``,
the fp64 yardstick of tests/test_robust.py).  Everything after the sums is a few dozen operations on n-vectors in fp64,
written with ``torch.where``: the state lives on the device and a round reads nothing back to the host.
"""
import math
import os
from typing import Optional, Tuple

import torch

MIN_SIGMA2 = 1e-6  # floor of the pixel inlier variance
MIN_SLICE_VAR = 1e-4  # floor of both variances of the slice potentials' mixture
N_STATS = 7


def _fused(sim: torch.Tensor) -> bool:
    return os.environ.get("NESVOR_ROBUST", "") != "composed" and sim.is_cuda and sim.dtype == torch.float32


def estep_composed(sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], scale: torch.Tensor,
                   model: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """p (as ``sim``) and the seven sums per slice (n,7) in fp64; ``model`` = {sigma2, c, m}.  The per-pixel arithmetic is in the
    tensors' dtype, in the order the kernel evaluates it; the sums are taken in fp64."""
    n = sim.shape[0]
    valid = torch.ones_like(sim, dtype=torch.bool) if mask is None else mask.reshape(sim.shape).bool()
    sigma2, c, m = model[0], model[1], model[2]
    e = scale.view(n, *([1] * (sim.ndim - 1))) * y - sim
    e2 = e * e
    g = torch.exp(-e2 / (2 * sigma2)) / torch.sqrt(2 * math.pi * sigma2)
    cg = c * g
    zero = torch.zeros_like(sim)
    p = torch.where(valid, cg / (cg + (1 - c) * m), zero)
    q = 1 - p
    py = p * y
    terms = (valid.to(sim.dtype), p, p * e2, q * q, py * sim, py * y, e2)
    stats = torch.stack([torch.where(valid, t, zero).double().flatten(1).sum(1) for t in terms], dim=1)
    return p, stats


def estep(sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], scale: torch.Tensor,
          model: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if _fused(sim):
        return torch.ops.nesvor.robust_estep(sim.contiguous(), y.contiguous(),
                                             None if mask is None else mask.reshape(sim.shape).contiguous(),
                                             scale.contiguous(), model.contiguous())
    return estep_composed(sim, y, mask, scale, model)


def _normal(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor) -> torch.Tensor:
    return torch.exp(-(x - mean) ** 2 / (2 * var)) / torch.sqrt(2 * math.pi * var)


def _safe_ratio(num: torch.Tensor, den: torch.Tensor, otherwise) -> torch.Tensor:
    ok = den > 0
    return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.full_like(num, otherwise))


def _lower_median(values: torch.Tensor, valid: torch.Tensor) -> torch.Tensor:
    """``torch.median`` (the lower of two middle elements) over the valid entries, without reading their number back."""
    ordered = torch.sort(torch.where(valid, values, torch.full_like(values, float("inf")))).values
    middle = ((valid.sum() - 1) // 2).clamp(min=0)
    return ordered.gather(0, middle.view(1))[0]


def slice_weights(pot: torch.Tensor, valid: torch.Tensor, previous: torch.Tensor) -> torch.Tensor:
    """One EM round on the slice potentials (fp64 n-vectors): the posterior of "inlier slice", 0 for a slice that is not valid.

    A first round (nothing rejected so far: sum (1 - w) <= 1e-6) starts robustly: inliers at the median with the MAD's
    spread, outliers at the largest potential.  Later rounds take the classes' weighted moments.  If the classes are closer
    than four inlier standard deviations they overlap, and nothing is rejected."""
    zero, one = torch.zeros_like(pot), torch.ones_like(pot)
    w = torch.where(valid, previous, zero)
    v = valid.to(pot.dtype)
    n_valid = v.sum()
    s_in, s_out = w.sum(), ((1 - w) * v).sum()
    pot0 = torch.where(valid, pot, zero)
    # robust start
    median = _lower_median(pot, valid)
    mad = _lower_median((pot - median).abs(), valid)
    var_rob = (1.4826 * mad) ** 2
    max_pot = torch.where(valid, pot, torch.full_like(pot, -float("inf"))).max()
    # weighted moments
    mean_in_w = _safe_ratio((w * pot0).sum(), s_in, 0.0)
    var_in_w = _safe_ratio((w * (pot0 - mean_in_w) ** 2).sum(), s_in, 0.0)
    mean_out_w = _safe_ratio(((1 - w) * v * pot0).sum(), s_out, 0.0)
    var_out_w = _safe_ratio(((1 - w) * v * (pot0 - mean_out_w) ** 2).sum(), s_out, 0.0)
    mix_w = _safe_ratio(s_in, n_valid, 0.9)
    start = s_out <= 1e-6
    mean_in, mean_out = torch.where(start, median, mean_in_w), torch.where(start, max_pot, mean_out_w)
    var_in = torch.where(start, var_rob, var_in_w).clamp(min=MIN_SLICE_VAR)
    var_out = torch.where(start, var_rob, var_out_w).clamp(min=MIN_SLICE_VAR)
    mix = torch.where(start, torch.full_like(mix_w, 0.9), mix_w).clamp(0.01, 0.99)
    num = mix * _normal(pot0, mean_in, var_in)
    new = _safe_ratio(num, num + (1 - mix) * _normal(pot0, mean_out, var_out), 1.0)
    new = torch.where(pot0 >= mean_out, zero, new)
    new = torch.where(pot0 <= mean_in, one, new)
    new = torch.where(mean_out - mean_in < 4 * torch.sqrt(var_in), one, new)
    return torch.where(valid, new, zero)


class RobustStatistics:
    """The EM state as device tensors: ``model`` = {sigma2, c, m} (also as the 0-d views ``sigma2``, ``c``, ``m``), ``scale`` (n),
    ``slice_weight`` (n) and the pixel posteriors ``p`` (as the slices).  ``init`` once, then ``update`` per round."""

    def __init__(self) -> None:
        self.model = self.scale = self.slice_weight = self.p = self.stats = None

    sigma2 = property(lambda self: self.model[0])
    c = property(lambda self: self.model[1])
    m = property(lambda self: self.model[2])

    def init(self, sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor]) -> "RobustStatistics":
        n = sim.shape[0]
        self.scale = torch.ones(n, dtype=sim.dtype, device=sim.device)
        self.slice_weight = torch.ones(n, dtype=sim.dtype, device=sim.device)
        if mask is None:
            y_max, y_min = y.max(), y.min()
        else:
            valid = mask.reshape(y.shape).bool()
            y_max = torch.where(valid, y, torch.full_like(y, -float("inf"))).max()
            y_min = torch.where(valid, y, torch.full_like(y, float("inf"))).min()
        m = 1 / (2.1 * y_max - 1.9 * y_min)
        # the seventh sum does not depend on the model: sigma2 = 1 is a placeholder for this call
        self.model = torch.stack([torch.ones_like(m), torch.full_like(m, 0.9), m])
        self.p, self.stats = estep(sim, y, mask, self.scale, self.model)
        sigma2 = _safe_ratio(self.stats[:, 6].sum(), self.stats[:, 0].sum(), MIN_SIGMA2).clamp(min=MIN_SIGMA2)
        self.model = torch.stack([sigma2.to(sim.dtype), self.model[1], self.model[2]])
        return self

    def update(self, sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor]) -> "RobustStatistics":
        self.p, st = estep(sim, y, mask, self.scale, self.model)
        self.stats = st
        n_k = st[:, 0]
        valid = n_k > 0
        pot = torch.sqrt(_safe_ratio(st[:, 3], n_k, 0.0))
        self.slice_weight = slice_weights(pot, valid, self.slice_weight.double()).to(sim.dtype)
        sum_p = st[:, 1].sum()
        sigma2 = _safe_ratio(st[:, 2].sum(), sum_p, MIN_SIGMA2).clamp(min=MIN_SIGMA2)
        c = _safe_ratio(sum_p, n_k.sum(), 0.9).clamp(0.01, 0.99)
        self.model = torch.stack([sigma2.to(sim.dtype), c.to(sim.dtype), self.model[2]])
        self.scale = _safe_ratio(st[:, 4], st[:, 5], 1.0).to(sim.dtype)
        return self

    def weights(self) -> torch.Tensor:
        """The pixel weight of the data term: p times its slice's weight."""
        return self.p * self.slice_weight.view(-1, *([1] * (self.p.ndim - 1)))

    def scaled(self, y: torch.Tensor) -> torch.Tensor:
        return self.scale.view(-1, *([1] * (y.ndim - 1))) * y
