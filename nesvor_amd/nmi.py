"""Normalised mutual information for the slice-to-volume registration: the ONE statement of the definition.  The fused kernel
(csrc/svr_nmi.hip, ``torch.ops.nesvor.svr_joint_histogram``) implements it, the composed path of ``SVR`` / ``GroupSVR`` and the
tests call it.

Joint histogram of simulated value I and acquired value J over the valid pixels of a (slice, pose), ``B`` bins per axis
(``MIN_BINS <= B <= MAX_BINS``).  Each axis has an affine map to bin coordinates, computed in fp32 (``axis_map``):
``scale = fp32((B-1) / (hi - lo))``, 0 when ``hi <= lo``.  I takes the min / max of the level's volume; J takes the min / max of the
slice's masked pixels (``SVR``: (0, 0) for an empty mask) or of its group's (``GroupSVR``).  Position of a value v (``axis_place``),
all in fp32, every operation rounded on its own::

    u = clamp((v - lo) * scale, 0, B-1);  b0 = min(int(u), B-2);  f = u - b0;  q = int(f * 256 + 0.5)   # 0 <= q <= 256

v gives weight ``256 - q`` to bin ``b0`` and ``q`` to bin ``b0 + 1``; a valid pixel adds the four integer products of its I weights
and its J weights to the cells (bI, bJ) - ``UNITS`` = 65536 per pixel.  The histogram is integer (row = I bin, column = J bin), so
it does not depend on the order of addition; the linear weights make it continuous in I, which the finite-difference gradient
needs.

Loss (``nmi_loss``), in float64:  N = sum H, p = H / N, entropies with 0 log 0 = 0,  ``loss = 1 - (H_I + H_J) / H_IJ``  in [-1, 0];
0 where N == 0 or H_IJ <= 0 ("no valid pixel" is the worst loss, as the descent assumes); the valid count is N / 65536.  A group's
histogram is the integer sum of its members'.

The stack registration (``VVR`` with ``loss = {"name": "nmi"}``; csrc/vvr_nmi.hip, ``torch.ops.nesvor.vvr_joint_histogram``) uses the
same statement per (pyramid level, pose) over ALL ``M`` points of the level's point list - there is no mask: I is the source sampled
at the moved point (trilinear, zero padding, so a point that leaves the source has I = 0 and still counts, as it does for NCC), J
the target's value at the point; I's map is ``axis_map`` of the min / max of the level's source, J's of the min / max of the point
list's values ((0, 0) for an empty list), both computed once per level.  A histogram's total is ``UNITS * M``; an empty list gives
zeros and loss 0."""
from typing import Tuple

import torch

MIN_BINS, MAX_BINS, DEFAULT_BINS = 2, 64, 32
UNITS = 65536  # what one valid pixel adds to its histogram


def check_bins(bins, what: str = "bins") -> int:
    """``bins`` as an int in [MIN_BINS, MAX_BINS]; ValueError naming ``what`` otherwise."""
    if isinstance(bins, bool) or int(bins) != bins or not MIN_BINS <= int(bins) <= MAX_BINS:
        raise ValueError(f"{what}: an integer in [{MIN_BINS}, {MAX_BINS}] expected, got {bins}")
    return int(bins)


def masked_range(values: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lo, hi) of the masked elements of every row of ``values`` (n, ...): (+inf, -inf) for a row without one, so that ranges
    pool with min / max."""
    v, m = values.flatten(1), mask.flatten(1)
    lo = torch.where(m, v, torch.full_like(v, float("inf"))).amin(1)
    hi = torch.where(m, v, torch.full_like(v, float("-inf"))).amax(1)
    return lo, hi


def axis_map(lo: torch.Tensor, hi: torch.Tensor, bins: int) -> torch.Tensor:
    """(..., 2) fp32 {lo, scale} of an axis whose values span [lo, hi]; (0, 0) for an empty range (hi < lo)."""
    lo, hi = lo.float(), hi.float()
    scale = torch.where(hi > lo, (bins - 1) / (hi - lo), torch.zeros_like(lo))  # fp32: one subtraction, one division
    return torch.stack([torch.where(hi < lo, torch.zeros_like(lo), lo), scale], -1)


def axis_place(v: torch.Tensor, lo, scale, bins: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(b0, q), int64: the lower bin of every fp32 value and the weight, of 256, of the upper one.  ``lo`` / ``scale``: floats
    that fp32 holds exactly, or fp32 tensors that broadcast against ``v``."""
    assert v.dtype == torch.float32
    u = ((v - lo) * scale).clamp(0, bins - 1)
    b0 = u.long().clamp(max=bins - 2)
    f = u - b0.float()
    return b0, (f * 256 + 0.5).long()


def joint_histogram(I: torch.Tensor, J: torch.Tensor, valid: torch.Tensor, i_map, j_map: torch.Tensor, bins: int) -> torch.Tensor:
    """(m, B, B) int64 from I, J (m, P) fp32 and valid (m, P) bool; ``i_map`` = (lo, scale) floats, ``j_map`` (m, 2) fp32.  Integer
    adds only (``index_add_`` of int64): the same on every device and from run to run."""
    m = I.shape[0]
    J = torch.where(valid, J, torch.zeros_like(J))  # (a NaN behind the mask stays out of the integer conversions)
    I = torch.where(valid, I, torch.zeros_like(I))
    bi, qi = axis_place(I, float(i_map[0]), float(i_map[1]), bins)
    bj, qj = axis_place(J, j_map[:, :1], j_map[:, 1:], bins)
    cell = torch.arange(m, device=I.device)[:, None] * (bins * bins) + bi * bins + bj
    on = valid.long()
    out = torch.zeros(m * bins * bins, dtype=torch.int64, device=I.device)
    for di, wi in ((0, 256 - qi), (1, qi)):
        for dj, wj in ((0, 256 - qj), (1, qj)):
            out.index_add_(0, (cell + (di * bins + dj)).reshape(-1), (wi * wj * on).reshape(-1))
    return out.view(m, bins, bins)


def _entropy(p: torch.Tensor, dims) -> torch.Tensor:
    return -(torch.where(p > 0, p * torch.log(torch.where(p > 0, p, torch.ones_like(p))), torch.zeros_like(p))).sum(dims)


def nmi_loss(hist: torch.Tensor) -> torch.Tensor:
    """(..., B, B) int64 histograms -> (...) float64 loss  1 - (H_I + H_J) / H_IJ; 0 for an empty histogram or H_IJ <= 0."""
    h = hist.double()
    n = h.sum((-2, -1))
    p = h / torch.where(n > 0, n, torch.ones_like(n))[..., None, None]
    h_ij, h_i, h_j = _entropy(p, (-2, -1)), _entropy(p.sum(-1), -1), _entropy(p.sum(-2), -1)
    ok = (n > 0) & (h_ij > 0)
    return torch.where(ok, 1 - (h_i + h_j) / torch.where(ok, h_ij, torch.ones_like(h_ij)), torch.zeros_like(h_ij))


def valid_count(hist: torch.Tensor) -> torch.Tensor:
    """The number of valid pixels behind (..., B, B) histograms, float64 (exact: the total is 65536 * count)."""
    return (hist.sum((-2, -1)) // UNITS).double()
