"""Slice bias fields for the classical reconstruction (the ``svr`` command): a smooth multiplicative field per slice, the step
IRTK / SVRTK and NiftyMIC run next to the slice scale of the EM scheme (Kuklisova-Murgasova et al. 2012).  The stack-level
correction (nesvor_amd/bias.py) works in a stack's index space, removes each stack's own mean and sees no other stack: fields
that differ from slice to slice (the subject moves in the coil's profile) and inconsistencies between stacks survive it.  Here
every slice is compared with what the volume predicts for it.  The reference project has no counterpart: the definition is
this module's.

Definition of one round.  With sim = A x (n,1,h,w), y the acquired normalised slices, scale_k the robust slice scales (ones
without them), weight the robust and / or structural pixel weights (ones without them), b the current log-field (zeros at
first) and sigma_px = sigma_mm / res_s:
    e = valid & (y > lo) & (sim > lo)            the eligible pixels; lo = MIN_INTENSITY (0.05 of the normalised range, a
                                                 constructor argument) rounded to the tensors' dtype once; the test is on the
                                                 raw inputs, so it is the same in every precision
    I = (scale_k y) exp(-b)
    r = clamp(log(I / sim), -CLAMP, CLAMP)       on eligible pixels, 0 elsewhere; CLAMP = log 2
    u = weight                                   on eligible pixels, 0 elsewhere
S(a) is the separable Gaussian window of radius R = max(1, ceil(3 sigma_px)) with zero padding: taps
exp(-(t - R)^2 / (2 sigma_px^2)), t = 0 .. 2 R, normalised to sum 1 in double and rounded to the dtype once (``gaussian_taps``);
along x first; each pass is acc = 0; acc = acc + g[t] a[. + t - R] in ascending t (``window.window``, which ``structural.py`` shares).
    num = S(u r),  den = S(u),  d = num / den where den > DEN_MIN = 1e-3, else 0,   b_new = b + d    on every pixel of the frame
(off the mask the field is the smooth continuation of what the eligible pixels say).  Five sums per slice in fp64 follow,
{n_eligible, sum u, sum u b_new, sum u r, sum (u r) r}.  After the sums, on fp64 n-vectors with ``torch.where``: a slice with
sum u < MIN_WEIGHT = 64 keeps its old field; every other slice loses its weighted mean, b_new -= sum u b_new / sum u.  A field
therefore carries shape only; the slice's gain stays with scale_k.

One round (``SliceBias.update``) needs b_new and the sums (``field_update``): on HIP fp32 tensors with R <= MAX_RADIUS = 48 two
passes of ``torch.ops.nesvor.slice_bias_update`` (csrc/slice_bias.hip); ``NESVOR_SLICE_BIAS=composed``, host tensors, other dtypes
and larger radii take the same formulas as a torch expression (``field_composed``, the fp64 yardstick of
tests/test_slice_bias.py).  A round reads nothing back to the host.
"""
import math
import os
from typing import Optional, Tuple

import torch

from . import window as _w

MIN_INTENSITY = 0.05
CLAMP = math.log(2.0)
DEN_MIN = 1e-3
MIN_WEIGHT = 64.0
MAX_RADIUS = 48  # of the fused path
N_STATS = 5


def window_radius(sigma_px: float) -> int:
    sigma_px = float(sigma_px)
    if not (sigma_px > 0.0 and math.isfinite(sigma_px)):
        raise ValueError(f"slice bias: sigma_px must be positive and finite, got {sigma_px}")
    return max(1, math.ceil(3.0 * sigma_px))


def gaussian_taps(sigma_px: float, dtype: torch.dtype = torch.float64, device=None) -> torch.Tensor:
    return _w.gaussian_taps(sigma_px, window_radius(sigma_px), dtype, device)


def _rounded(value: float, dtype: torch.dtype) -> float:
    """``value`` rounded to ``dtype`` once, as a host number."""
    return torch.tensor(value, dtype=torch.float64).to(dtype).item()


def _window(a: torch.Tensor, taps) -> torch.Tensor:
    return _w.window(a, taps, 2)


def eligible(sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], min_intensity: float = MIN_INTENSITY) -> torch.Tensor:
    lo = _rounded(min_intensity, sim.dtype)
    e = (y > lo) & (sim > lo)
    return e if mask is None else e & mask.reshape(sim.shape).bool()


def field_composed(sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], scale: torch.Tensor,
                   weight: Optional[torch.Tensor], b: torch.Tensor, sigma_px: float,
                   min_intensity: float = MIN_INTENSITY) -> Tuple[torch.Tensor, torch.Tensor]:
    """b_new (as ``sim``, before the centring) and the five sums per slice (n,5) in fp64.  The per-pixel arithmetic is in the
    tensors' dtype, in the order the kernel evaluates it; the sums are taken in fp64."""
    n = sim.shape[0]
    dtype = sim.dtype
    e = eligible(sim, y, mask, min_intensity)
    clamp, den_min = _rounded(CLAMP, dtype), _rounded(DEN_MIN, dtype)
    taps = gaussian_taps(sigma_px, dtype).tolist()  # host numbers: exactly the dtype's values
    zero, one = torch.zeros_like(sim), torch.ones_like(sim)
    i = (scale.view(n, *([1] * (sim.ndim - 1))) * y) * torch.exp(-b)
    r = torch.where(e, torch.log(torch.where(e, i / sim, one)).clamp(-clamp, clamp), zero)
    u = torch.where(e, one if weight is None else weight.reshape(sim.shape), zero)
    ur = u * r
    num, den = _window(ur, taps), _window(u, taps)
    ok = den > den_min
    b_new = b + torch.where(ok, num / torch.where(ok, den, one), zero)
    terms = (e.to(dtype), u, torch.where(e, u * b_new, zero), ur, ur * r)
    stats = torch.stack([t.double().flatten(1).sum(1) for t in terms], dim=1)
    return b_new, stats


def _fused(sim: torch.Tensor, sigma_px: float) -> bool:
    return (os.environ.get("NESVOR_SLICE_BIAS", "") != "composed" and sim.is_cuda and sim.dtype == torch.float32
            and window_radius(sigma_px) <= MAX_RADIUS)


def field_update(sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], scale: torch.Tensor,
                 weight: Optional[torch.Tensor], b: torch.Tensor, sigma_px: float,
                 min_intensity: float = MIN_INTENSITY) -> Tuple[torch.Tensor, torch.Tensor]:
    if _fused(sim, sigma_px):
        return torch.ops.nesvor.slice_bias_update(sim.contiguous(), y.contiguous(),
                                                  None if mask is None else mask.reshape(sim.shape).contiguous(), scale.contiguous(),
                                                  None if weight is None else weight.reshape(sim.shape).contiguous(), b.contiguous(),
                                                  float(sigma_px), float(min_intensity))
    return field_composed(sim, y, mask, scale, weight, b, sigma_px, min_intensity)


def centred(b: torch.Tensor, b_new: torch.Tensor, stats: torch.Tensor) -> torch.Tensor:
    """What follows the sums: a slice with sum u < MIN_WEIGHT keeps ``b``; every other slice is ``b_new`` minus its weighted
    mean sum u b_new / sum u (fp64, rounded to the field's dtype once)."""
    total = stats[:, 1]
    ok = total >= MIN_WEIGHT
    mean = stats[:, 2] / torch.where(ok, total, torch.ones_like(total))
    shape = (-1, *([1] * (b.ndim - 1)))
    return torch.where(ok.view(shape), b_new - mean.to(b.dtype).view(shape), b)


class SliceBias:
    """The window and the floor and, after ``update``, the state as device tensors: ``b`` (as the slices) the log-fields and
    ``stats`` (n,5) fp64 the sums of the last round (of b_new before its centring)."""

    def __init__(self, sigma_mm: float = 12.0, min_intensity: float = MIN_INTENSITY, rounds: int = 3) -> None:
        self.sigma_mm, self.min_intensity = float(sigma_mm), float(min_intensity)
        self.rounds = int(rounds)  # of ``svr.reconstruct_volume`` when neither the robust statistics nor the structural step bring theirs
        if not (self.sigma_mm > 0.0 and math.isfinite(self.sigma_mm)):
            raise ValueError(f"SliceBias: sigma_mm must be positive and finite, got {sigma_mm}")
        self.b = self.stats = None

    def update(self, sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], scale: Optional[torch.Tensor],
               weight: Optional[torch.Tensor], res_s: float) -> "SliceBias":
        if scale is None:
            scale = torch.ones(sim.shape[0], dtype=sim.dtype, device=sim.device)
        if self.b is None:
            self.b = torch.zeros_like(sim)
        b_new, self.stats = field_update(sim, y, mask, scale, weight, self.b, self.sigma_mm / float(res_s), self.min_intensity)
        self.b = centred(self.b, b_new.view_as(self.b), self.stats)
        return self

    def corrected(self, y: torch.Tensor) -> torch.Tensor:
        """y exp(-b); ``y`` itself before the first round."""
        return y if self.b is None else y * torch.exp(-self.b)

    def rms(self, sim: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
        """The root mean square (n, fp64) of ``b`` over a slice's eligible pixels; 0 for a slice without one."""
        e = eligible(sim, y, mask, self.min_intensity)
        count = e.flatten(1).sum(1).double()
        square = torch.where(e, self.b * self.b, torch.zeros_like(self.b)).double().flatten(1).sum(1)
        return torch.sqrt(square / torch.where(count > 0, count, torch.ones_like(count)))
