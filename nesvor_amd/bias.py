"""Bias field correction of a stack (the ``correct-bias-field`` command, ``--bias-field-correction``): an N4-style estimate of
the smooth multiplicative coil bias, removed before anything compares intensities across space.

Upstream NeSVoR calls SimpleITK's N4 for this in releases after the one this project models; the definition below is this
module's own.  A stack, (n,1,h,w) or (D,H,W), is a 3-D array in index space; the valid voxels are ``mask & (slices > 0)``.  With
v = log I on the valid voxels and the log field f = 0 at the start, level l fits a cubic B-spline lattice of
S = (n_control_points - 3) 2^l spans and C = S + 3 control points per axis; an iteration is

1. histogram: u = v - f, lo / hi its extremes over the valid voxels, slope = (hi - lo) / (n_bins - 1), c = (u - lo) / slope
   (clamped to [0, n_bins - 1]); with i = min(floor c, n_bins - 2) a voxel adds 1 - (c - i) to bin i and c - i to bin i + 1;
2. sharpening (``sharpen_lut``): Wiener deconvolution of the zero-padded histogram with a Gaussian of ``fwhm``, then the
   conditional expectation E per bin - float64 torch on n_bins-sized arrays, shared by both paths;
3. residual r = u - lerp(E, c) on the valid voxels;
4. fit (Lee, Wolberg and Shin's multilevel B-spline approximation): voxel index i of an axis of n voxels has t = i / (n - 1) S,
   span s = min(floor t, S - 1), tau = t - s and the four uniform cubic basis values on control indices s .. s + 3
   (``axis_table``); with w_k the product of a voxel's three axis weights on control point k,
   Phi_k = sum_p w_kp^3 r_p / (sum_c w_cp^2) / sum_p w_kp^2, 0 where the divisor is 0;
5. update: f += sum_k Phi_k w_k on every voxel; with g = expm1 of the increment over the valid voxels
   cv = sqrt(mean g^2 - (mean g)^2) / (1 + mean g); the level ends when cv < tol or after n_iter iterations.

After the last level f loses its float64 mean over the valid voxels (the stack keeps its brightness) and
corrected = slices / exp(f) on every voxel.  There is no shrink factor: the fit runs at full resolution.

Steps 1, 3 + 4 and 5 are, on HIP fp32 tensors with C <= 16 and n_bins <= 1024, one fused op each
(``torch.ops.nesvor.n4_histogram / n4_fit / n4_update_``, csrc/bias.hip: reproducible sums, the axes contracted one after the
other); ``NESVOR_BIAS=composed``, host tensors and other dtypes take the float64 torch expressions ``histogram_composed``,
``fit_composed`` and ``update_composed`` (three einsums with dense (n, C) weight tables each way; the yardstick of
tests/test_bias.py and tests/test_gpu_bias.py).  Both paths share v, the per-level tables and the sharpening.  The extremes of u
stay on the device (the update returns those of the next u); the ONE host read per iteration is cv.
"""
import logging
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

MAX_CONTROL = 16  # control points per axis the fused ops take
MAX_BINS = 1024   # histogram bins the fused ops take


def _fused(x: torch.Tensor, C: int, n_bins: int) -> bool:
    return (os.environ.get("NESVOR_BIAS", "") != "composed" and x.is_cuda and x.dtype == torch.float32 and C <= MAX_CONTROL
            and 2 <= n_bins <= MAX_BINS)


# ---------------------------------------------------------------------------------------------------------------------
# per-axis tables
# ---------------------------------------------------------------------------------------------------------------------
def axis_table(n: int, S: int, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(span (n) int32, basis (n,4) float64) of the voxel indices 0 .. n - 1 of an axis under S spans: the first control index
    and the uniform cubic B-spline values on control indices span .. span + 3.  tau = 1 only at the last index."""
    i = torch.arange(n, dtype=torch.float64, device=device)
    t = i / (n - 1) * S if n > 1 else torch.zeros(1, dtype=torch.float64, device=device)
    s = torch.clamp(torch.floor(t), max=S - 1)
    tau = t - s
    basis = torch.stack([(1 - tau) ** 3 / 6, (3 * tau ** 3 - 6 * tau ** 2 + 4) / 6, (-3 * tau ** 3 + 3 * tau ** 2 + 3 * tau + 1) / 6,
                         tau ** 3 / 6], 1)
    return s.to(torch.int32), basis


def dense_weights(span: torch.Tensor, basis: torch.Tensor, S: int) -> torch.Tensor:
    """The (n, S + 3) float64 weight matrix of an axis table."""
    idx = span.long()[:, None] + torch.arange(4, device=span.device)[None]
    return torch.zeros(span.shape[0], S + 3, dtype=torch.float64, device=span.device).scatter_(1, idx, basis)


class LevelTables:
    """The tables of one level for a (D,H,W) array, built once in float64: per axis (z, y, x) ``span`` (n) int32, ``basis`` (n,4)
    float64, ``dense`` (n, C) float64 for the composed path and ``basis32`` (n,4) float32 for the kernels."""

    def __init__(self, shape: Sequence[int], S: int, device=None):
        self.S, self.C = int(S), int(S) + 3
        pairs = [axis_table(int(n), self.S, device) for n in shape]
        self.span = [p[0].contiguous() for p in pairs]
        self.basis = [p[1] for p in pairs]
        self.basis32 = [b.float().contiguous() for b in self.basis]
        self._dense: Optional[List[torch.Tensor]] = None

    @property
    def dense(self) -> List[torch.Tensor]:
        if self._dense is None:
            self._dense = [dense_weights(s, b, self.S) for s, b in zip(self.span, self.basis)]
        return self._dense


# ---------------------------------------------------------------------------------------------------------------------
# the composed float64 path
# ---------------------------------------------------------------------------------------------------------------------
def _valid(v: torch.Tensor, mask: Optional[torch.Tensor]) -> torch.Tensor:
    return torch.ones_like(v, dtype=torch.bool) if mask is None else mask.reshape(v.shape) != 0


def _bin_coord(u: torch.Tensor, rng: torch.Tensor, n_bins: int) -> torch.Tensor:
    """c = (u - lo) / slope clamped to [0, n_bins - 1], a NaN (slope 0) counted as 0; rng = {lo, hi}."""
    lo, hi = rng.double()[0], rng.double()[1]
    slope = (hi - lo) / (n_bins - 1)
    return torch.nan_to_num((u - lo) / slope, nan=0.0).clamp(0, n_bins - 1)


def histogram_composed(v: torch.Tensor, f: torch.Tensor, mask: Optional[torch.Tensor], rng: torch.Tensor, n_bins: int) -> torch.Tensor:
    """(n_bins) float64: the fractionally binned histogram of u = v - f over the valid voxels."""
    c = _bin_coord((v.double() - f.double())[_valid(v, mask)], rng, n_bins)
    i0 = torch.floor(c).clamp(max=n_bins - 2).long()
    off = c - i0
    return torch.zeros(n_bins, dtype=torch.float64, device=v.device).index_add_(0, i0, 1 - off).index_add_(0, i0 + 1, off)


def sharpen_lut(hist: torch.Tensor, rng: torch.Tensor, fwhm: float = 0.15, noise: float = 0.01) -> torch.Tensor:
    """(n_bins) float64 E: the conditional expectation of the true log intensity per bin, from the Wiener deconvolution of the
    histogram (zero-padded to 2^(ceil(log2 n_bins) + 1), centred) with a Gaussian of ``fwhm``.  All on ``hist``'s device."""
    n_bins = int(hist.shape[0])
    dev = hist.device
    lo, hi = rng.double()[0], rng.double()[1]
    slope = (hi - lo) / (n_bins - 1)
    P = 2 ** (math.ceil(math.log2(n_bins)) + 1)
    o = (P - n_bins) // 2
    V = torch.zeros(P, dtype=torch.float64, device=dev)
    V[o:o + n_bins] = hist
    sf = fwhm / slope
    k = torch.arange(P, device=dev)
    k = torch.minimum(k, P - k).double()
    F = 2 * math.sqrt(math.log(2) / math.pi) / sf * torch.exp(-k ** 2 * (4 * math.log(2) / sf ** 2))
    Ff = torch.fft.fft(F)
    U = torch.fft.ifft(torch.fft.fft(V) * (Ff.conj() / (Ff.conj() * Ff + noise)).real).real.clamp(min=0)
    x = lo + (torch.arange(P, device=dev) - o) * slope
    num = torch.fft.ifft(torch.fft.fft(x * U) * Ff).real
    den = torch.fft.ifft(torch.fft.fft(U) * Ff).real
    return torch.where(den != 0, num / den, torch.zeros_like(num))[o:o + n_bins].contiguous()


def residual_composed(v: torch.Tensor, f: torch.Tensor, rng: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """r = u - lerp(E, c) on every voxel (the callers mask it), float64."""
    n_bins = int(lut.shape[0])
    u = v.double() - f.double()
    c = _bin_coord(u, rng, n_bins)
    j = torch.floor(c).clamp(max=n_bins - 2).long()
    t = c - j
    return u - (lut[j] * (1 - t) + lut[j + 1] * t)


def fit_composed(v: torch.Tensor, f: torch.Tensor, mask: Optional[torch.Tensor], rng: torch.Tensor, lut: torch.Tensor,
                 tables: LevelTables) -> Tuple[torch.Tensor, torch.Tensor]:
    """(lattice, weight), both (C,C,C) float64: Phi and its divisor, as einsums with the dense weight tables."""
    Wz, Wy, Wx = tables.dense
    m = _valid(v, mask).double()
    s2 = lambda W: (W ** 2).sum(1)
    R = m * residual_composed(v, f, rng, lut) / (s2(Wz)[:, None, None] * s2(Wy)[None, :, None] * s2(Wx)[None, None, :])
    num = torch.einsum("zyx,za,yb,xc->abc", R, Wz ** 3, Wy ** 3, Wx ** 3)
    den = torch.einsum("zyx,za,yb,xc->abc", m, Wz ** 2, Wy ** 2, Wx ** 2)
    return torch.where(den > 0, num / den.clamp(min=1e-300), torch.zeros_like(num)), den


def evaluate_composed(lattice: torch.Tensor, tables: LevelTables) -> torch.Tensor:
    """(D,H,W) float64: sum_k lattice[k] w_k on every voxel."""
    return torch.einsum("abc,za,yb,xc->zyx", lattice.double(), *tables.dense)


def update_composed(lattice: torch.Tensor, tables: LevelTables, f: torch.Tensor, v: torch.Tensor,
                    mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """(f + the lattice's field in float64, stats (5) float64 {count, sum g, sum g^2, min u_new, max u_new} over the valid
    voxels; min / max are +inf / -inf without one).  Not in place."""
    d = evaluate_composed(lattice, tables)
    f_new = f.double() + d
    m = _valid(v, mask)
    g = torch.expm1(d[m])
    u = (v.double() - f_new)[m]
    inf = torch.full((), float("inf"), dtype=torch.float64, device=v.device)
    lo, hi = (u.min(), u.max()) if u.numel() else (inf, -inf)
    count = torch.full((), float(u.numel()), dtype=torch.float64, device=v.device)
    return f_new, torch.stack([count, g.sum(), (g * g).sum(), lo, hi])


# ---------------------------------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------------------------------
def _iteration(v, f, valid, rng, tables: LevelTables, n_bins, fwhm, noise, fused):
    """One iteration on either path: -> (f, stats).  The fused path writes f in place."""
    if fused:
        ops = torch.ops.nesvor
        hist = ops.n4_histogram(v, f, valid, rng, n_bins)
        lut = sharpen_lut(hist, rng, fwhm, noise)
        lattice, _ = ops.n4_fit(v, f, valid, rng, lut, *tables.basis32, *tables.span, tables.S)
        return f, ops.n4_update_(lattice, *tables.basis32, *tables.span, tables.S, f, v, valid)
    hist = histogram_composed(v, f, valid, rng, n_bins)
    lut = sharpen_lut(hist, rng, fwhm, noise)
    lattice, _ = fit_composed(v, f, valid, rng, lut, tables)
    return update_composed(lattice, tables, f, v, valid)


def _cv(stats: torch.Tensor) -> torch.Tensor:
    count, sg, sgg = stats[0], stats[1], stats[2]
    mean = sg / count
    return torch.sqrt((sgg / count - mean * mean).clamp(min=0)) / (1 + mean)


def correct_bias_field(slices: torch.Tensor, mask: Optional[torch.Tensor] = None, *, n_levels: int = 4, n_iter: int = 50,
                       tol: float = 1e-3, n_control_points: int = 4, n_bins: int = 200, fwhm: float = 0.15,
                       noise: float = 0.01) -> Tuple[torch.Tensor, torch.Tensor, Dict]:
    """-> (corrected, log_field, info) for one stack ``slices`` (n,1,h,w) or (D,H,W); ``mask`` of its shape or None.

    ``corrected = slices / exp(log_field)``, both of the shape of ``slices``; the field is float32 from the fused path and
    float64 from the composed one, and has zero mean over the valid voxels ``mask & (slices > 0)``.  ``info``: ``iterations``
    (per level), ``cv`` (the last one), ``fused``.  No valid voxel, or one log intensity only: the input comes back unchanged
    with a zero field and a warning."""
    if n_levels < 1 or n_iter < 1 or n_control_points < 4 or n_bins < 2:
        raise ValueError("correct_bias_field: n_levels >= 1, n_iter >= 1, n_control_points >= 4 and n_bins >= 2 expected")
    if not (slices.ndim == 3 or (slices.ndim == 4 and slices.shape[1] == 1)):
        raise ValueError(f"correct_bias_field: a stack (n,1,h,w) or (D,H,W) expected, got {tuple(slices.shape)}")
    if mask is not None and mask.numel() != slices.numel():
        raise ValueError("correct_bias_field: mask must have the shape of slices")
    img = slices.reshape(slices.shape[0], slices.shape[-2], slices.shape[-1])
    if not img.is_floating_point():
        img = img.float()
    valid = img > 0
    if mask is not None:
        valid = valid & (mask.reshape(img.shape) != 0)
    valid = valid.contiguous()
    C_max = (n_control_points - 3) * 2 ** (n_levels - 1) + 3
    fused = _fused(img, C_max, n_bins)
    info: Dict = {"iterations": [], "cv": float("nan"), "fused": fused}
    # v = log I, computed once and shared by both paths
    v = torch.where(valid, torch.log(img.clamp(min=torch.finfo(img.dtype).tiny)), torch.zeros_like(img)).contiguous()
    if not fused:
        v = v.double()
    f = torch.zeros_like(v)
    degenerate = not bool(valid.any())
    if not degenerate:
        vm = v[valid]
        rng = torch.stack([vm.min(), vm.max()])
        degenerate = bool(rng[0] == rng[1])
    if degenerate:
        logging.warning("Bias field correction: no valid voxel or a constant image; the stack is left unchanged")
        return slices, f.reshape(slices.shape), info
    for level in range(n_levels):
        tables = LevelTables(img.shape, (n_control_points - 3) * 2 ** level, img.device)
        done = 0
        for _ in range(n_iter):
            f, stats = _iteration(v, f, valid, rng, tables, n_bins, fwhm, noise, fused)
            rng = stats[3:5].to(v.dtype)  # the extremes of the next u: they stay on the device
            done += 1
            info["cv"] = float(_cv(stats))  # the one host read of the iteration
            if info["cv"] < tol:
                break
        info["iterations"].append(done)
    f = (f.double() - f[valid].double().mean()).to(f.dtype)
    corrected = (img / torch.exp(f)).to(slices.dtype) if slices.is_floating_point() else img / torch.exp(f).to(img.dtype)
    return corrected.reshape(slices.shape), f.reshape(slices.shape), info


def correct_stacks(stacks: List, **kw) -> List[torch.Tensor]:
    """``correct_bias_field`` on every ``Stack`` in place (``slices`` replaced by the corrected ones); returns the log fields."""
    fields = []
    for j, st in enumerate(stacks):
        corrected, field, info = correct_bias_field(st.slices, st.mask, **kw)
        st.slices = corrected
        fields.append(field)
        logging.info("Bias field correction, stack %d: iterations per level %s, last cv %.2e, field exp(f) %.3f .. %.3f (%s path)", j,
                     info["iterations"], info["cv"], float(torch.exp(field.min())), float(torch.exp(field.max())),
                     "fused" if info["fused"] else "composed")
    return fields
