"""The yardstick of tests/test_gpu_svr_nmi.py: the joint histograms of csrc/svr_nmi.hip built on the CPU from the acquisition oracle
(oracle/slice_acq.py) with the definition of nesvor_amd/nmi.py, per pixel and aggregated, with derived per-cell bounds.
tests/test_nmi_reference.py checks it on the CPU.  Nothing here touches a GPU, and nothing is fitted to the kernel.

Cases, seeds, masks and the 27 poses per geometry are those of tests/svr_reference.py (``case``, ``images``, ``pose_ids``: slice i
evaluates pose (i + k) mod 27 at position k).

Bounds.  A bin's weight is a hat function of the bin coordinate u with slope at most 1 per bin, 256 units high.  The simulated value
I is held to the existing bound of the operator, e = TOL32["slices"] = 1e-4 |I_ref| + 1e-5, which moves u by at most i_scale e and
therefore EVERY I-bin weight of the pixel by at most  256 i_scale e + 1  units (the 1: the roundings of q and of u in fp32, both
sides).  The J weights are exact (J and its map are inputs), at most 256.  A pixel's cell (bI, bJ) may therefore be off by
(256 i_scale e + 1) wJ[bJ]; an aggregated cell by the sum of its pixels' bounds - integer adds add nothing."""
import torch

import svr_reference as R
from acq_geometry import TOL32
from nesvor_amd import nmi

BINS = [2, 5, 32, 64]
PIXEL_BINS = 32  # the per-pixel runs (the default of the registration)


def i_map(c, bins):
    """(lo, scale) floats of the simulated value: the range of the case's volume."""
    return tuple(nmi.axis_map(c.vol.min(), c.vol.max(), bins).tolist())


def j_map(J, mask, bins):
    """(n, 2) fp32 {lo, scale} of the acquired value: every slice's masked range ((0, 0) for an empty mask); J (n, h, w)."""
    return nmi.axis_map(*nmi.masked_range(J, torch.ones_like(J, dtype=torch.bool) if mask is None else mask), bins).contiguous()


def histograms(I, weight, J, mask, imap, jmap, bins, pid):
    """(n, k, B, B) int64: I, weight (27, h, w) by pose, J (n, h, w), mask (n, h, w) bool or None, jmap (n, 2), pid (n, k) the pose of
    every entry."""
    out = []
    for i in range(J.shape[0]):
        Ii, wi = I[pid[i]].flatten(1), weight[pid[i]].flatten(1)  # (k, P)
        valid = wi > 0
        if mask is not None:
            valid = valid & mask[i].flatten()[None]
        out.append(nmi.joint_histogram(Ii, J[i].flatten()[None].expand_as(Ii).contiguous(), valid, imap, jmap[i:i + 1].expand(Ii.shape[0], 2),
                                       bins))
    return torch.stack(out)


def axis_weights(v, lo, scale, bins):
    """(..., B) int64: the weights (of 256) a value gives to every bin of its axis."""
    b0, q = nmi.axis_place(v, lo, scale, bins)
    w = torch.zeros(v.shape + (bins,), dtype=torch.int64)
    w.scatter_(-1, b0[..., None], (256 - q)[..., None])
    w.scatter_add_(-1, (b0 + 1)[..., None], q[..., None])
    return w


def pixel_histograms(c, J, jmap_row, bins):
    """Per (pose, pixel) of one image J (h, w) binned with ONE map jmap_row (2,): values (27, P, B, B) int64, bounds (27, P, B, B)
    float64, valid (27, P) bool - what an entry whose mask keeps that pixel alone must hold."""
    I, wgt = R.images(c, torch.float32)
    K, P = I.shape[0], I[0].numel()
    imap = i_map(c, bins)
    valid = (wgt > 0).view(K, P)
    Iv, Jv = I.reshape(K * P, 1), J.flatten()[None].expand(K, P).reshape(K * P, 1).contiguous()
    values = nmi.joint_histogram(Iv, Jv, valid.reshape(K * P, 1), imap, jmap_row[None].expand(K * P, 2), bins).view(K, P, bins, bins)
    rtol, atol, _ = TOL32["slices"]
    e = rtol * I.double().abs().view(K, P) + atol
    d_i = (256.0 * imap[1] * e + 1.0) * valid.double()
    w_j = axis_weights(J.flatten(), float(jmap_row[0]), float(jmap_row[1]), bins).double()  # (P, B)
    bounds = d_i[..., None, None] * w_j[None, :, None, :].expand(K, P, bins, bins)
    return values, bounds, valid


# ---------------------------------------------------------------------------------------------------------------------
# one synthetic case past the kernel's unit of work
# ---------------------------------------------------------------------------------------------------------------------
# csrc/svr_nmi.hip cuts a slice into segments, one LDS histogram each: as many as it takes to reach 1024 workgroups, of 1024 pixels
# at least (small calls) and 16384 at most (calls of 1024 (slice, pose) entries or more)
MIN_SEGMENT_PIXELS, MAX_SEGMENT_PIXELS, TARGET_WORKGROUPS = 1024, 16384, 1024
SEGMENT_CASES = {"segment": (2, 4 * MIN_SEGMENT_PIXELS + 1), "segment_max": (40, MAX_SEGMENT_PIXELS + 1)}


def segments(entries, pixels):
    """The number of segments the kernel cuts a slice of ``pixels`` into in a call of ``entries`` (slice, pose) pairs."""
    want = -(-TARGET_WORKGROUPS // entries)
    seg = min(max(-(-(-(-pixels // want)) // 256) * 256, MIN_SEGMENT_PIXELS), MAX_SEGMENT_PIXELS)
    return -(-pixels // seg)


def segment_case(name="segment"):
    """A single row of one pixel more than whole segments, the last pixel alone in the last segment: "segment", 2 slices of 4097
    pixels (x 27 poses = 54 entries: segments of 1024, five of them); "segment_max", 40 slices of 16385 pixels (1080 entries: whole
    slices up to 16384 pixels, two segments).  Pixels of a quarter voxel on a (5, 7, W) volume that holds them, the four masks, 27
    poses: the lattice poses of the volume, then generic ones (small translations).  For comparisons with the composed definition
    on the device (no oracle run)."""
    import types

    from acq_geometry import _generic_poses, _lattice_poses, _psf

    if name not in R._DATA:
        n, w = SEGMENT_CASES[name]
        assert segments(n * R.K_POSES, w - 1) + 1 == segments(n * R.K_POSES, w) == {"segment": 5, "segment_max": 2}[name]
        dims = (5, 7, w // 4 + 20)
        g = torch.Generator().manual_seed(w)
        poses = torch.cat([_lattice_poses(dims), _generic_poses(R.K_POSES - R.N_LATTICE + 1, g)[1:] * torch.tensor([1, 1, 1, 0.2])])
        R._DATA[name] = types.SimpleNamespace(key=name, geom=name, dims=dims, shape=(1, w), res=0.25, psf=_psf("psf333"),
                                                   poses=poses.contiguous(), vol=torch.rand(dims, generator=g),
                                                   J=torch.rand((n, 1, w), generator=g),
                                                   masks={"none": None, "random": torch.rand((n, 1, w), generator=g) < 0.7})
        c = R._DATA[name]
        c.masks["slice_off"] = torch.ones((n, 1, w), dtype=torch.bool)
        c.masks["slice_off"][1] = False
        c.masks["last_pixel"] = torch.zeros((n, 1, w), dtype=torch.bool)
        c.masks["last_pixel"][..., -1] = True  # the last segment's only pixel, alone
    return R._DATA[name]
