"""Denoising of the input stacks (``--denoise`` on the commands that read stacks, and the ``denoise`` command): 2-D non-local
means (Buades et al. 2005), slice by slice, the step SVRTK runs on every stack before anything else and the N4 literature
recommends before the field is fitted.  2-D on purpose: the slices of a stack move against each other, a 3-D patch would
average across motion.  The reference project has no counterpart: the definition is this module's.

Definition (``nlm_composed``).  y (n,1,h,w) the slices, m the validity as 0 / 1 (the mask, or 1 everywhere; 0 outside the image),
y0 = y on valid pixels and 0 elsewhere (so that no invalid value, a NaN included, reaches a valid pixel), sigma_k the noise
standard deviation of slice k, P the patch radius, S the search radius, beta the strength.  For a valid pixel p of slice k:
    candidates   q = p + t for every shift t in [-S,S]^2 \\ {0} with q inside the image and valid, in ascending (t_y, t_x)
    c_o = m(p+o) m(q+o),  e_o = c_o (y0(p+o) - y0(q+o))^2       o in [-P,P]^2; o = 0 always counts
    num = sum_o e_o,  den = sum_o c_o                            each added along x first, then along y, in ascending order
    d2 = num / max(den, 1)                                       the mean squared difference of the pixels both patches have
    w(p,q) = exp(-(max(d2 - 2 sigma_k^2, 0) / (beta sigma_k)^2)) 2 sigma^2 is what two patches of one signal differ by
    w_c = the largest w(p,q), or 1 without a candidate           the centre weight
    W = w_c + sum_q w(p,q),  V = w_c y(p) + sum_q w(p,q) y(q)    the sums from 0 in candidate order
    out(p) = V / W                                               y(p) where W = 0: every weight underflowed (an outlier at a tiny sigma)
An invalid pixel keeps its value bit for bit, and so does every pixel of a slice whose sigma_k is not positive and finite.
``stats`` (n,2) fp64 holds {number of valid pixels, sum over them of (out - y)^2} per slice; the second is the "method noise":
a denoiser that removes noise and nothing else removes about sigma (``method_noise_rms``).  Everything is evaluated in the
dtype of y, the squares of ``stats`` too; their sum is taken in fp64.

``estimate_noise`` gives one sigma per stack: on the valid pixels whose four in-plane neighbours are inside the image and valid
the pseudo-residual eps = sqrt(4/5) (y - mean of the four) has the noise's variance where the signal is locally linear
(Gasser et al. 1986); sigma = 1.4826 median|eps - median eps|, the MAD, ignores the edges, where it is not.

``denoise_stacks`` is what the command line calls: on HIP fp32 tensors with P <= 3 and S <= 10 one launch per stack of
``torch.ops.nesvor.nlm_denoise`` (csrc/denoise.hip), which follows the expression operation for operation; host tensors, other
dtypes, larger radii and ``NESVOR_DENOISE=composed`` take the expression itself.
"""
import logging
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

MAX_PATCH_RADIUS = 3  # of the fused path
MAX_SEARCH_RADIUS = 10
MIN_NOISE_PIXELS = 64
MAD_TO_SIGMA = 1.4826
N_STATS = 2


def _rounded(value: float, dtype: torch.dtype) -> float:
    """``value`` rounded to ``dtype`` once, as a host number."""
    return torch.tensor(value, dtype=torch.float64).to(dtype).item()


def _check(patch_radius: int, search_radius: int, strength: float) -> Tuple[int, int, float]:
    P, S, beta = int(patch_radius), int(search_radius), float(strength)
    if P < 1 or S < 1:
        raise ValueError(f"denoise: patch and search radius of at least 1 expected, got {patch_radius} and {search_radius}")
    if not (beta > 0.0 and math.isfinite(beta)):
        raise ValueError(f"denoise: strength must be positive and finite, got {strength}")
    return P, S, beta


def _box(a: torch.Tensor, P: int, h: int, w: int) -> torch.Tensor:
    """(.., h + 2 P, w + 2 P) -> (.., h, w): the sum over the (2 P + 1)^2 window, along x first; each pass from its first term
    in ascending order."""
    rows = a[..., :, 0:w]
    for ox in range(1, 2 * P + 1):
        rows = rows + a[..., :, ox:ox + w]
    acc = rows[..., 0:h, :]
    for oy in range(1, 2 * P + 1):
        acc = acc + rows[..., oy:oy + h, :]
    return acc


def nlm_composed(y: torch.Tensor, mask: Optional[torch.Tensor], sigma: torch.Tensor, patch_radius: int = 1, search_radius: int = 3,
                 strength: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """out (as ``y``) and stats (n,2) fp64; the module's definition as a torch expression in the dtype of ``y``, in the order
    the kernel evaluates it."""
    P, S, beta = _check(patch_radius, search_radius, strength)
    shape, dtype = y.shape, y.dtype
    n, h, w = int(shape[0]), int(shape[-2]), int(shape[-1])
    y = y.reshape(n, 1, h, w)
    valid = torch.ones_like(y, dtype=torch.bool) if mask is None else mask.reshape(y.shape).bool()
    zero, one = torch.zeros_like(y), torch.ones_like(y)
    y0 = torch.where(valid, y, zero)
    sig = sigma.to(dtype).reshape(n, 1, 1, 1)
    ok = torch.isfinite(sig) & (sig > 0)
    s = torch.where(ok, sig, torch.ones_like(sig))
    two_s2 = 2.0 * (s * s)
    hs = _rounded(beta, dtype) * s
    h2 = hs * hs
    R = S + P
    yp, mp = F.pad(y0, (R, R, R, R)), F.pad(valid.to(dtype), (R, R, R, R))
    H, W = h + 2 * P, w + 2 * P  # the frame a patch sum reads
    ya, ma = yp[..., S:S + H, S:S + W], mp[..., S:S + H, S:S + W]
    acc_w, acc_wy, wmax = zero, zero, zero
    some = torch.zeros_like(valid)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            if dy == 0 and dx == 0:
                continue
            yb, mb = yp[..., S + dy:S + dy + H, S + dx:S + dx + W], mp[..., S + dy:S + dy + H, S + dx:S + dx + W]
            diff = ya - yb
            c = ma * mb
            num, den = _box(c * (diff * diff), P, h, w), _box(c, P, h, w)
            d2 = num / den.clamp(min=1.0)
            x = (d2 - two_s2).clamp(min=0.0)
            there = mb[..., P:P + h, P:P + w] > 0
            wgt = torch.where(there, torch.exp(-(x / h2)), zero)
            acc_w = acc_w + wgt
            acc_wy = acc_wy + wgt * yb[..., P:P + h, P:P + w]
            wmax = torch.maximum(wmax, wgt)
            some = some | there
    wc = torch.where(some, wmax, one)
    total = wc + acc_w
    value = wc * y0 + acc_wy
    good = valid & ok & (total > 0)
    out = torch.where(good, value / torch.where(good, total, one), y)
    d = torch.where(valid, out - y, zero)
    stats = torch.stack([valid.double().flatten(1).sum(1), (d * d).double().flatten(1).sum(1)], dim=1)
    return out.reshape(shape), stats


def _fused(y: torch.Tensor, patch_radius: int, search_radius: int) -> bool:
    return (os.environ.get("NESVOR_DENOISE", "") != "composed" and y.is_cuda and y.dtype == torch.float32
            and 1 <= patch_radius <= MAX_PATCH_RADIUS and 1 <= search_radius <= MAX_SEARCH_RADIUS)


def nlm(y: torch.Tensor, mask: Optional[torch.Tensor], sigma: torch.Tensor, patch_radius: int = 1, search_radius: int = 3,
        strength: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernel where it applies, else the expression."""
    P, S, beta = _check(patch_radius, search_radius, strength)
    if _fused(y, P, S):
        return torch.ops.nesvor.nlm_denoise(y.contiguous(), None if mask is None else mask.reshape(y.shape).contiguous(),
                                            sigma.to(torch.float32).contiguous(), P, S, beta)
    return nlm_composed(y, mask, sigma, P, S, beta)


def estimate_noise(slices: torch.Tensor, mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, int]:
    """(sigma, n_used): the noise standard deviation of a stack as a 0-dim tensor of the slices' dtype on their device, and the
    number of pixels it was taken from.  With no usable pixel sigma is nan."""
    n, h, w = int(slices.shape[0]), int(slices.shape[-2]), int(slices.shape[-1])
    y = slices.reshape(n, h, w)
    use = torch.zeros_like(y, dtype=torch.bool)
    if h < 3 or w < 3:
        return y.new_full((), float("nan")), 0
    m = torch.ones_like(y, dtype=torch.bool) if mask is None else mask.reshape(y.shape).bool()
    use[:, 1:-1, 1:-1] = m[:, 1:-1, 1:-1] & m[:, :-2, 1:-1] & m[:, 2:, 1:-1] & m[:, 1:-1, :-2] & m[:, 1:-1, 2:]
    eps = torch.zeros_like(y)
    eps[:, 1:-1, 1:-1] = math.sqrt(0.8) * (y[:, 1:-1, 1:-1] - 0.25 * ((y[:, :-2, 1:-1] + y[:, 2:, 1:-1]) + (y[:, 1:-1, :-2] + y[:, 1:-1, 2:])))
    values = eps[use]  # (the count is read here; the values stay on the device)
    n_used = int(values.numel())
    if n_used == 0:
        return y.new_full((), float("nan")), 0
    sigma = MAD_TO_SIGMA * (values - values.median()).abs().median()
    return sigma, n_used


def method_noise_rms(stats: torch.Tensor) -> float:
    """sqrt(sum (out - y)^2 / number of valid pixels) over all slices of ``stats``; 0 without a valid pixel."""
    count, square = float(stats[:, 0].sum()), float(stats[:, 1].sum())
    return math.sqrt(square / count) if count > 0 else 0.0


def denoise_stacks(stacks: Sequence, patch_radius: int = 1, search_radius: int = 3, strength: float = 1.0, sigma: Optional[float] = None,
                   names: Optional[Sequence[str]] = None) -> List[Dict]:
    """Non-local means on every ``Stack`` in place: ``st.slices`` is replaced by the denoised slices in the same dtype; masks,
    poses and geometry are untouched.  ``sigma``: a fixed noise level in the stacks' intensities instead of the estimate.
    Returns per stack ``{"sigma": 0-dim tensor, "n_used": pixels of the estimate (0 with a fixed sigma), "stats": (n,2) fp64 or None,
    "fused": bool}``; a stack whose noise cannot be estimated (fewer than 64 usable pixels) is left as it is with a warning and
    ``stats`` None."""
    P, S, beta = _check(patch_radius, search_radius, strength)
    if sigma is not None and not (float(sigma) > 0.0 and math.isfinite(float(sigma))):
        raise ValueError(f"denoise: a fixed sigma must be positive and finite, got {sigma}")
    reports = []
    for j, st in enumerate(stacks):
        name = names[j] if names is not None else f"stack {j}"
        y = st.slices
        if sigma is None:
            s, n_used = estimate_noise(y, st.mask)
            if n_used < MIN_NOISE_PIXELS:
                logging.warning("Denoising, %s: only %d pixels with four valid neighbours, fewer than %d: the noise cannot be estimated "
                                "and the stack is left as it is", name, n_used, MIN_NOISE_PIXELS)
                reports.append({"sigma": s, "n_used": n_used, "stats": None, "fused": False})
                continue
        else:
            s, n_used = torch.tensor(float(sigma), dtype=y.dtype, device=y.device), 0
        fused = _fused(y, P, S)
        out, stats = nlm(y, st.mask, s.expand(y.shape[0]), P, S, beta)  # the per-slice array: the stack's sigma on every slice
        st.slices = out.to(y.dtype).view_as(y)
        reports.append({"sigma": s, "n_used": n_used, "stats": stats, "fused": fused})
        logging.info("Denoising, %s: sigma %.4g (%s), method noise rms %.4g (%s path)", name, float(s),
                     f"estimated on {n_used} pixels" if sigma is None else "given", method_noise_rms(stats), "fused" if fused else "composed")
    return reports


def report_row(report: Dict) -> Dict:
    """A report of ``denoise_stacks`` as host numbers: sigma, n_used, valid_pixels, method_noise_rms (None for a stack left alone)."""
    s = float(report["sigma"])
    row = {"sigma": s if math.isfinite(s) else None, "n_used": int(report["n_used"]), "denoised": report["stats"] is not None,
           "valid_pixels": None, "method_noise_rms": None, "path": "fused" if report["fused"] else "composed"}
    if report["stats"] is not None:
        row["valid_pixels"] = int(report["stats"][:, 0].sum())
        row["method_noise_rms"] = method_noise_rms(report["stats"])
    return row
