"""The yardstick of tests/test_gpu_svr_similarity.py: the six moment sums of csrc/svr.hip composed on the CPU from the acquisition
oracle (oracle/slice_acq.py), per pixel and aggregated, with derived bounds.  tests/test_svr_reference.py checks it on the CPU.
Nothing here touches a GPU, and nothing is fitted to the kernel.

A CASE is one geometry of tests/acq_geometry.py with K = 27 distinct poses - the six lattice poses, then 21 generic ones (the
identity ``_generic_poses`` starts with is dropped: it is lattice pose 0) - a ``rand`` volume, five ``rand`` images in [0, 1) and
four masks (none, random about 70 %, slice 1 off, one pixel of the last workgroup alone).  The same 27 poses serve every slice, so the oracle runs once per pose; the tests hand slice i the list rolled by i
(``pose_ids``), so that entry (i, k) is pose (i + k) mod 27 and an index that picks another slice's poses shows.

Values: the oracle in fp32, as in the existing pins of the acquisition operator.  A generic seed is accepted only if, on the CPU,
the fp32 and the fp64 oracle have EQUAL valid sets and their images agree within ``pixel_bounds`` (``seed_report``): the
reference's own boundary flips are kept out of the inputs.

Bounds.  Per pixel the simulated value I is held to the existing bound of the operator, TOL32["slices"]: e = 1e-4 |I_ref| + 1e-5.
It propagates to 2 |I_ref| e + e^2 for I^2 and |J| e for I J.  J and the count are exact; J^2 is the fp32 product J * J, one ulp
allowed.  An aggregated sum may be off by the sum of its pixels' bounds plus SUM_ROUNDINGS 2^-24 |sum|: six levels of the fp32 wave
tree, one product rounding and one spare (all terms are >= 0, so |sum| is the sum of the magnitudes); across waves and workgroups
the kernel adds in double."""
import types

import torch

from acq_geometry import GEOMETRIES, TOL32, _generic_poses, _lattice_poses, _psf

K_POSES = 27
N_LATTICE = 6
SUM_ROUNDINGS = 8
EPS32 = 2.0 ** -24
# seed of the generic poses per geometry; accepted by seed_report on the CPU (asserted in tests/test_svr_reference.py)
SEEDS = {"odd": 3, "tiny": 3, "row": 2, "dense": 3, "sparse": 6, "even": 2}
# PSFs run on the "even" geometry besides its own
SPECIAL_PSFS = ["psf1688", "half_zero", "one_tap", "all_zero"]
MASKS = ["none", "random", "slice_off", "last_pixel"]
_DATA = {}


def special_psf(name):
    """psf1688: 1024 non-zero taps, the last entry of the kernel's LDS list.  half_zero: the (9,5,5) PSF with about half of its
    taps set to exact 0, renormalised.  one_tap: (9,5,5), zero except one tap off centre.  all_zero: (9,5,5) zeros."""
    if name == "psf1688":
        return _psf(name)
    psf = _psf("psf955").clone()
    if name == "half_zero":
        keep = torch.rand(psf.shape, generator=torch.Generator().manual_seed(955)) < 0.5
        psf = psf * keep
        assert 0.3 < float((psf == 0).double().mean()) < 0.7
        return (psf / psf.sum()).contiguous()
    psf.zero_()
    if name == "one_tap":
        psf[2, 3, 1] = 1.0  # tap (ix, iy, iz) = (-1, 1, -2)
    return psf.contiguous()


def case(geom, psf=None):
    """One geometry's inputs, fp32 on the CPU, built once and never written."""
    key = (geom, psf)
    if key in _DATA:
        return _DATA[key]
    dims, shape, res, own_psf = GEOMETRIES[geom]
    poses = torch.cat([_lattice_poses(dims), _generic_poses(K_POSES - N_LATTICE + 1, torch.Generator().manual_seed(SEEDS[geom]))[1:]])
    assert poses.shape == (K_POSES, 3, 4)
    g = torch.Generator().manual_seed(7000 + list(GEOMETRIES).index(geom))
    h, w = shape
    c = types.SimpleNamespace(key=key, geom=geom, dims=dims, shape=shape, res=res, psf=_psf(own_psf) if psf is None else special_psf(psf),
                              poses=poses.contiguous(), vol=torch.rand(dims, generator=g), J=torch.rand((5, h, w), generator=g))
    random = torch.rand((5, h, w), generator=g) < 0.7
    slice_off = torch.ones((5, h, w), dtype=torch.bool)
    slice_off[1] = False
    _DATA[key] = c
    c.last_pixel = last_workgroup_pixel(c)
    last = torch.zeros((5, h * w), dtype=torch.bool)
    last[:, c.last_pixel] = True
    c.masks = {"none": None, "random": random, "slice_off": slice_off, "last_pixel": last.view(5, h, w)}
    _DATA[key] = c
    return c


def last_workgroup_pixel(c):
    """The pixel of a slice's last workgroup of 256 (ragged unless h w is a multiple of 256) that the fp32 oracle finds valid under the
    most poses, the last of them on a tie: a mask that keeps it alone leaves one live thread in that workgroup."""
    h, w = c.shape
    first = 256 * ((h * w - 1) // 256)
    count = (images(c, torch.float32)[1] > 0).view(K_POSES, h * w).sum(0)[first:]
    return first + int(torch.nonzero(count == count.max()).max())


def pose_ids(n, K=K_POSES):
    """(n, K) long: slice i evaluates pose (i + k) mod 27 at position k."""
    return (torch.arange(n)[:, None] + torch.arange(K)[None, :]) % K_POSES


def images(c, dtype):
    """(I, weight), each (K, h, w) in ``dtype``: the oracle's A with need_weight, no interp_psf, no masks, once per pose."""
    from oracle import slice_acq as O

    key = ("images", c.key, dtype)
    if key not in _DATA:
        I, wgt = O.slice_acquisition_forward(c.poses.to(dtype), c.vol.to(dtype)[None, None], None, None, c.psf.to(dtype), c.shape, c.res,
                                             True, False)
        _DATA[key] = (I[:, 0], wgt[:, 0])
    return _DATA[key]


def sums(I, weight, J, mask):
    """(n, K, 6) fp64 {count, sum I, sum I^2, sum I J, sum J, sum J^2} over valid = mask & (weight > 0).  I, weight: (K, h, w), the same
    poses for every slice, or (n, K, h, w); J (n, h, w); mask (n, h, w) bool or None."""
    if I.ndim == 3:
        I, weight = I[None], weight[None]
    n = J.shape[0]
    v = (weight > 0).expand(n, -1, -1, -1)
    if mask is not None:
        v = v & mask[:, None]
    v = v.double()
    Id, Jd = I.double() * v, J.double()[:, None] * v
    return torch.stack([t.sum((2, 3)) for t in (v, Id, Id * Id, Id * Jd, Jd, Jd * Jd)], -1)


def _e(I_ref):
    rtol, atol, _ = TOL32["slices"]
    return rtol * I_ref.double().abs() + atol


def _jj(J):
    """fp32 J * J and one ulp of it, in double."""
    jj = J.float() * J.float()
    return jj.double(), (torch.nextafter(jj, torch.full_like(jj, float("inf"))) - jj).double()


def pixel_values(I_ref, weight, J):
    """(..., h, w, 6) fp64: what an entry whose mask keeps one pixel must hold, {v, v I, v I^2, v I J, v J, v fp32(J J)}."""
    v = (weight > 0).double()
    Id, Jd = I_ref.double(), J.double().expand_as(I_ref)
    return torch.stack([torch.ones_like(Id), Id, Id * Id, Id * Jd, Jd, _jj(J)[0].expand_as(Id)], -1) * v[..., None]


def pixel_bounds(I_ref, J):
    """(..., h, w, 6) fp64 bounds of the six per-pixel values; I_ref (..., h, w), J broadcastable to it."""
    e = _e(I_ref)
    Ia, Ja = I_ref.double().abs(), J.double().abs().expand_as(e)
    zero = torch.zeros_like(e)
    return torch.stack([zero, e, 2 * Ia * e + e * e, Ja * e, zero, _jj(J)[1].expand_as(e)], -1)


def summation_term(ref_sums):
    s = SUM_ROUNDINGS * EPS32 * ref_sums.abs()
    s[..., 0] = 0  # counts are exact
    return s


def sum_bounds(I_ref, weight, J, mask, ref_sums):
    """(n, K, 6) fp64: the per-pixel bounds added over the valid set, plus the summation term of ``ref_sums`` = sums(...)."""
    if I_ref.ndim == 3:
        I_ref, weight = I_ref[None], weight[None]
    n = J.shape[0]
    v = (weight > 0).expand(n, -1, -1, -1)
    if mask is not None:
        v = v & mask[:, None]
    b = pixel_bounds(I_ref.expand(n, -1, -1, -1), J[:, None])
    return (b * v.double()[..., None]).sum((2, 3)) + summation_term(ref_sums)


def seed_report(c):
    """The two CPU conditions on a case's poses: (number of pixels whose validity differs between the fp32 and the fp64 oracle,
    largest |I32 - I64| / bound)."""
    I32, w32 = images(c, torch.float32)
    I64, w64 = images(c, torch.float64)
    flips = int(((w32 > 0) != (w64 > 0)).sum())
    return flips, float(((I32.double() - I64).abs() / _e(I32)).max())
