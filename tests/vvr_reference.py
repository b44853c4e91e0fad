"""Shared reference code of tests/test_gpu_vvr_similarity.py (a plain module, not a conftest): the moment sums of
``nesvor_vvr_similarity`` (csrc/vvr.hip) restated in torch on the CPU, and the accumulation bound of the kernel's fp32 arithmetic.

``vvr_sums`` takes the kernel's own fp32 inputs (CPU tensors) and a dtype for the COORDINATES: float64 is the reference,
float32 is the same expression with the kernel's coordinate precision (the difference of the two is the coordinate-rounding
term of an fp32 kernel, measured between references).  Values and sums are float64 in both.

The accumulation bound (``accumulation_bound``) - what the kernel may differ by when its coordinates are exact:

* a sample  v = sum_c w_c s_c  over the 8 corners: ``wx = fx - floor(fx)`` is exact, ``1 - wx`` rounds once, so a weight - a
  product of three such factors - carries at most 3 + 2 roundings; the 8 ``fmaf`` round the running value once each, the first
  term passes through all 8: |v_kernel - v| <= 13 u V with V = sum_c w_c |s_c| and u = 2^-24;
* a thread adds T = ceil(M / (256 min(ceil(M / 256), 2048))) samples in fp32 (one rounding of the running sum each: ``+=`` or one
  ``fmaf``; the product inside an ``fmaf`` is exact), a wave adds its 64 partials in fp32 (63 additions, any order), everything
  after that is double;
* so, to first order in u and with 1 % for the higher orders,
    |sum I   - ref| <= 1.01 u (13 + T + 63) sum V
    |sum I^2 - ref| <= 1.01 u (26 + T + 63) sum v^2        (v^2 carries twice the sample's error)
    |sum I J - ref| <= 1.01 u (13 + T + 63) sum |v J|
    |sum J   - ref| <= 1.01 u (T + 63) sum |J|,   |sum J^2 - ref| <= 1.01 u (T + 63) sum J^2.
"""
import torch

U = 2.0 ** -24  # unit roundoff of fp32
SAMPLE_ROUNDINGS = 13  # 3 + 2 for a weight, 8 fmaf
WAVE_ADDITIONS = 63
MAX_BLOCKS = 2048  # csrc/vvr.hip: the grid is min(ceil(M / 256), 2048) workgroups of 256


def per_thread(M):
    """Samples one thread of the kernel adds up (at most)."""
    blocks = min((M + 255) // 256, MAX_BLOCKS)
    return -(-M // (256 * blocks))


def _trilinear(src, fx, fy, fz):
    """Zero-padded trilinear sample of src (D,H,W) float64 at index coordinates (M,) -> (v, V) with V the sample of |src|."""
    D, H, W = src.shape
    flat, aflat = src.reshape(-1), src.abs().reshape(-1)
    x0, y0, z0 = torch.floor(fx), torch.floor(fy), torch.floor(fz)
    wx, wy, wz = (fx - x0).double(), (fy - y0).double(), (fz - z0).double()
    x0, y0, z0 = x0.long(), y0.long(), z0.long()
    v = torch.zeros(fx.shape, dtype=torch.float64)
    V = torch.zeros(fx.shape, dtype=torch.float64)
    for c in range(8):
        cx, cy, cz = c & 1, (c >> 1) & 1, c >> 2
        x, y, z = x0 + cx, y0 + cy, z0 + cz
        inside = (x >= 0) & (x < W) & (y >= 0) & (y < H) & (z >= 0) & (z < D)
        idx = (z.clamp(0, D - 1) * H + y.clamp(0, H - 1)) * W + x.clamp(0, W - 1)
        w = (wx if cx else 1 - wx) * (wy if cy else 1 - wy) * (wz if cz else 1 - wz)
        w = torch.where(inside, w, torch.zeros_like(w))
        v += w * flat[idx]
        V += w * aflat[idx]
    return v, V


def vvr_sums(src, points, target, mats, to_unit, dtype, with_abs=False):
    """src (D,H,W), points (M,3) [x, y, z in mm], target (M,), mats (K,3,4) rows of [R | t] applied as R (p + t), to_unit (3,):
    -> sums (K,3) {sum I, sum I^2, sum I J} and target sums (2,) {sum J, sum J^2}, float64.  Coordinates in ``dtype`` in the
    kernel's order  ((m0 qx + m1 qy) + m2 qz) * unit, then (g + 1) * (size - 1) / 2;  F.grid_sample's bilinear mode with zero
    padding and align_corners=True, written out.  ``with_abs``: also the sums of the terms' magnitudes
    (K,3) {sum V, sum v^2, sum |v J|} and (2,) {sum |J|, sum J^2} that the accumulation bound is relative to."""
    D, H, W = src.shape
    s64 = src.double()
    p = points.to(dtype)
    m = mats.to(dtype).reshape(-1, 12)
    u = torch.as_tensor(to_unit).to(dtype)
    J = target.double()
    half = [torch.tensor(0.5 * (n - 1), dtype=dtype) for n in (W, H, D)]
    sums = torch.zeros((m.shape[0], 3), dtype=torch.float64)
    mags = torch.zeros((m.shape[0], 3), dtype=torch.float64)
    for k in range(m.shape[0]):
        r = m[k]
        qx, qy, qz = p[:, 0] + r[3], p[:, 1] + r[7], p[:, 2] + r[11]
        f = [((((r[4 * a] * qx + r[4 * a + 1] * qy) + r[4 * a + 2] * qz) * u[a]) + 1) * half[a] for a in range(3)]
        v, V = _trilinear(s64, *f)
        sums[k] = torch.stack([v.sum(), (v * v).sum(), (v * J).sum()])
        mags[k] = torch.stack([V.sum(), (v * v).sum(), (v * J).abs().sum()])
    tsums = torch.stack([J.sum(), (J * J).sum()])
    if with_abs:
        return sums, tsums, mags, torch.stack([J.abs().sum(), (J * J).sum()])
    return sums, tsums


def sample(src, points, mat, to_unit, dtype=torch.float64):
    """The (M,) samples of one pose [R | t] (3,4), float64."""
    D, H, W = src.shape
    p, r, u = points.to(dtype), mat.to(dtype).reshape(12), torch.as_tensor(to_unit).to(dtype)
    half = [torch.tensor(0.5 * (n - 1), dtype=dtype) for n in (W, H, D)]
    qx, qy, qz = p[:, 0] + r[3], p[:, 1] + r[7], p[:, 2] + r[11]
    f = [((((r[4 * a] * qx + r[4 * a + 1] * qy) + r[4 * a + 2] * qz) * u[a]) + 1) * half[a] for a in range(3)]
    return _trilinear(src.double(), *f)[0]


def accumulation_bound(M, mags, tmags):
    """The bound of the module docstring for M points: -> (K,3) and (2,) float64."""
    T = per_thread(M)
    c = torch.tensor([SAMPLE_ROUNDINGS + T + WAVE_ADDITIONS, 2 * SAMPLE_ROUNDINGS + T + WAVE_ADDITIONS,
                      SAMPLE_ROUNDINGS + T + WAVE_ADDITIONS], dtype=torch.float64)
    return 1.01 * U * c * mags, 1.01 * U * (T + WAVE_ADDITIONS) * tmags
