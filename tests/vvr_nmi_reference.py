"""The yardstick of tests/test_gpu_vvr_nmi.py: the joint histograms of csrc/vvr_nmi.hip built on the CPU from the float64 samples of
tests/vvr_reference.py (``sample``) with the definition of nesvor_amd/nmi.py, with derived per-cell bounds.
tests/test_vvr_nmi_reference.py checks it on the CPU.  Nothing here touches a GPU, and nothing is fitted to the kernel.

The case: a (6, 11, 9) source of 1 mm voxels, 70001 random points over 1.03 x its extent (about a third of them not wholly inside
it under a pose: 26 % to 53 %), random target values, 27 random poses; a test takes the first M points and the first K poses.

Bounds.  A bin's weight is a hat function of the bin coordinate u with slope at most 1 per bin, 256 units high.  The sample I is
off by at most e, which moves u by at most i_scale e and therefore EVERY I-bin weight of the point by at most  256 i_scale e + 1
units (the 1: the roundings of q and of u in fp32, both sides).  The J weights are exact (J and its map are inputs), at most 256.
A point's cell (bI, bJ) may therefore be off by (256 i_scale e + 1) wJ[bJ] in the rows bI its I can reach (those of u -+ (i_scale e
+ 2^-8), and one above); an aggregated cell by the sum of its points' bounds - integer adds add nothing.

e, per point:  min(COORD_TOL x V, COORD_TOL_ABS x max |src|) + 13 u V,  V = sum_c |w_c| |src_c| of the point.  The last term is the
kernel's fp32 VALUE arithmetic (tests/vvr_reference.py: 13 roundings).  The first is its fp32 COORDINATE arithmetic, which cannot be
derived from the formats alone (a sample is Lipschitz, not smooth, in its coordinate) and is measured BETWEEN REFERENCES, as
tests/test_gpu_vvr_similarity.py measures its COORD_TOL: the largest |sample(fp32 coordinates) - sample(fp64 coordinates)| over the
case's points and poses, on the CPU (``measure_coord``), asserted at 4 x that: fp32 coordinate arithmetic in another order.
It is measured on two scales and the smaller bound holds.  Relative to V (COORD_MEASURED): V is taken as the larger of the two
references' (a point within rounding of the zero padding's edge has V = 0 under one of them).  That ratio is ill-conditioned at
the padding's edge, where V -> 0 while the coordinate error does not: its largest value, 1.1e-2, comes from a point with V = 2e-5
(the median ratio is 1.2e-8), and 4 x it says nothing about an interior point.  So also relative to max |src| (COORD_MEASURED_ABS):
a weight moves by at most the coordinate error whatever V is.  The relative bound is the smaller one for the few points at the edge,
the absolute one everywhere else."""
import torch

import vvr_reference as R
from nesvor_amd import nmi

SHAPE = (6, 11, 9)
M_MAX = 70001
POSES = 27
REACH = 1.03  # the cloud's half-extent in units of the source's
MS = [1, 255, 256, 257, 4001, 70001]  # 70001: at least two segments at any legal segment length (at most 16384 points)
KS = [1, 2, 13, 14, 27]
BINS = [2, 5, 32, 64]
_DATA = {}


def case():
    if "case" not in _DATA:
        from oracle import transform_convert as tc

        g = torch.Generator().manual_seed(21)
        D, H, W = SHAPE
        src = (torch.nn.functional.avg_pool3d(torch.rand(1, 1, D + 2, H + 2, W + 2, generator=g), 3, 1)[0, 0] + 0.25).contiguous()
        half = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0])
        points = ((torch.rand(M_MAX, 3, generator=g) * 2 - 1) * REACH * half).contiguous()
        target = torch.rand(M_MAX, generator=g)
        ax = torch.randn(POSES, 6, generator=g) * torch.tensor([0.08, 0.08, 0.08, 0.5, 0.5, 0.5])
        unit = (2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1))
        _DATA["case"] = dict(src=src, points=points, target=target, mats=tc.axisangle2mat_forward(ax).contiguous(), unit=unit)
    return _DATA["case"]


def unit32(c):
    """to_unit as the kernel reads it: three floats."""
    return torch.tensor(c["unit"], dtype=torch.float32)


def samples(c, dtype=torch.float64, magnitudes=False, mats=None):
    """(K, M_MAX) float64: the samples of every pose of ``mats`` (None: the case's 27, computed once) with coordinates in ``dtype``
    (``magnitudes``: of |src|, the V of the module docstring)."""
    src = c["src"].abs() if magnitudes else c["src"]
    if mats is not None:
        return torch.stack([R.sample(src, c["points"], m, unit32(c), dtype) for m in mats])
    key = ("samples", dtype, magnitudes)
    if key not in _DATA:
        _DATA[key] = samples(c, dtype, magnitudes, c["mats"])
    return _DATA[key]


def magnitude(c, mats=None):
    """V per (pose, point): the larger of the two references'."""
    return torch.maximum(samples(c, torch.float64, True, mats), samples(c, torch.float32, True, mats))


def outside_share(c):
    """The share of the points not wholly inside the source under pose 0 (a corner of their cell is zero padding)."""
    ones = torch.ones(SHAPE)
    return float((R.sample(ones, c["points"], c["mats"][0], unit32(c)) < 1).double().mean())


def measure_coord(c):
    """Largest |sample(fp32 coordinates) - sample(fp64 coordinates)| over the case -> (relative to V, relative to max |src|);
    V = 0 implies that both samples are 0."""
    diff = (samples(c, torch.float32) - samples(c, torch.float64)).abs()
    V = magnitude(c)
    assert bool((diff[V == 0] == 0).all())
    return float((diff / V.clamp(min=1e-300)).max()), float(diff.max() / c["src"].abs().max())


# measure_coord(case()) on the CPU (no kernel involved), and the tolerances: 4 x that
COORD_MEASURED, COORD_MEASURED_ABS = 1.148e-2, 1.861e-6
COORD_TOL, COORD_TOL_ABS = 4 * COORD_MEASURED, 4 * COORD_MEASURED_ABS


def sample_bound(c, mats=None):
    """e per (pose, point), float64 (K, M_MAX)."""
    V = magnitude(c, mats)
    return torch.clamp(COORD_TOL * V, max=COORD_TOL_ABS * float(c["src"].abs().max())) + R.SAMPLE_ROUNDINGS * R.U * V


def maps(c, M, bins, j_degenerate=False):
    """((i_lo, i_scale), (j_lo, j_scale)) floats: the source's range, the range of the first M target values."""
    i_map = tuple(nmi.axis_map(c["src"].min(), c["src"].max(), bins).tolist())
    J = c["target"][:M]
    j_map = tuple(nmi.axis_map(J.min(), J.min() if j_degenerate else J.max(), bins).tolist())
    return i_map, j_map


def bin_samples(I, J, i_map, j_map, bins):
    """(K, B, B) int64 of samples I (K, M) fp32 against J (M,) fp32 with nmi.joint_histogram - every point counts."""
    K = I.shape[0]
    Jk = J.view(1, -1).expand(K, -1)
    rows = torch.tensor(j_map, dtype=torch.float32, device=I.device).view(1, 2).expand(K, 2)
    return nmi.joint_histogram(I, Jk, torch.ones_like(Jk, dtype=torch.bool), i_map, rows, bins)


def axis_weights(v, lo, scale, bins):
    """(..., B) int64: the weights (of 256) a value gives to every bin of its axis."""
    b0, q = nmi.axis_place(v, lo, scale, bins)
    w = torch.zeros(v.shape + (bins,), dtype=torch.int64)
    w.scatter_(-1, b0[..., None], (256 - q)[..., None])
    w.scatter_add_(-1, (b0 + 1)[..., None], q[..., None])
    return w


def histograms(c, K, M, bins, mats=None):
    """The yardstick's histograms (K, B, B) int64 - the float64 samples rounded to fp32, binned - and their per-cell bounds
    (K, B, B) float64, of the first K poses (of ``mats``: other poses than the case's) and the first M points."""
    i_map, j_map = maps(c, M, bins)
    J = c["target"][:M]
    v = samples(c, mats=mats)[:K, :M]
    hist = bin_samples(v.float(), J, i_map, j_map, bins)
    e = sample_bound(c, mats)[:K, :M]
    d_i = 256.0 * i_map[1] * e + 1.0  # (K, M)
    w_j = axis_weights(J, j_map[0], j_map[1], bins).double()  # (M, B)
    u = ((v - i_map[0]) * i_map[1]).clamp(0, bins - 1)
    du = i_map[1] * e + 2.0 ** -8
    r_lo = (u - du).clamp(min=0).floor().long()
    r_hi = ((u + du).floor().long() + 1).clamp(max=bins - 1)
    bounds = torch.zeros((K, bins + 1, bins), dtype=torch.float64)
    for k in range(K):  # + over rows r_lo .. r_hi: a difference array along the I axis
        add = d_i[k][:, None] * w_j
        bounds[k].index_add_(0, r_lo[k], add)
        bounds[k].index_add_(0, r_hi[k] + 1, -add)
    return hist, bounds.cumsum(1)[:, :bins].clamp(min=0)
