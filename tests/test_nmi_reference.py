"""The definition of nesvor_amd/nmi.py and the reference of tests/nmi_reference.py, checked on the CPU: what
tests/test_gpu_svr_nmi.py holds the kernel to is itself right."""
import math

import pytest
import torch

import nmi_reference as N
import svr_reference as R
from nesvor_amd import nmi


def _pair(n=3, P=4000, seed=0):
    g = torch.Generator().manual_seed(seed)
    I = torch.rand((n, P), generator=g)
    return I, torch.rand((n, P), generator=g), torch.rand((n, P), generator=g) < 0.8


def _maps(I, J, valid, bins):
    return tuple(nmi.axis_map(I.min(), I.max(), bins).tolist()), nmi.axis_map(*nmi.masked_range(J, valid), bins)


@pytest.mark.parametrize("bins", N.BINS)
@pytest.mark.parametrize("mask", R.MASKS)
def test_total_is_65536_per_valid_pixel_and_the_j_marginal_is_built_from_j_alone(mask, bins):
    """On the oracle's images of "even" (27 rolled poses, five slices): the total of every histogram is 65536 * count with the count of
    svr_reference.sums, and its column sums are 256 * the J weights of the valid pixels - I does not enter them."""
    c = R.case("even")
    I, wgt = R.images(c, torch.float32)
    m = c.masks[mask]
    pid = R.pose_ids(5)
    jm = N.j_map(c.J, m, bins)
    H = N.histograms(I, wgt, c.J, m, N.i_map(c, bins), jm, bins, pid)
    assert H.shape == (5, R.K_POSES, bins, bins) and H.dtype == torch.int64 and int(H.min()) >= 0
    count = R.sums(I, wgt, c.J, m)[torch.arange(5)[:, None], pid][..., 0]
    assert torch.equal(H.sum((2, 3)), (count * nmi.UNITS).long()) and float(count.max()) > 0
    assert torch.equal(nmi.valid_count(H), count)
    wj = N.axis_weights(c.J.flatten(1), jm[:, :1], jm[:, 1:], bins)  # (5, P, B)
    valid = (wgt > 0).flatten(1)[pid]  # (5, K, P)
    if m is not None:
        valid = valid & m.flatten(1)[:, None]
    assert torch.equal(H.sum(2), 256 * (valid.long()[..., None] * wj[:, None]).sum(2))
    if mask == "slice_off":
        assert int(H[1].abs().max()) == 0 and jm[1].tolist() == [0.0, 0.0]
        assert float(nmi.nmi_loss(H[1]).abs().max()) == 0.0


@pytest.mark.parametrize("bins", [5, 32])
def test_a_slice_identical_to_its_simulation(bins):
    """J = I with one map for both axes: the histogram is symmetric (rows equal columns).  With every value on a bin centre a pixel
    lands wholly in a diagonal cell and the loss is -1.  Between centres the linear weights spread a pixel over a 2 x 2 block (the
    price of a histogram that is continuous in I) and the loss stays above -1.  For uniform values and many bins: given the I bin
    b, u has the triangular density of the hat around b, so the J bin is b with probability int hat^2 = 2/3 and b - 1 or b + 1 with
    1/6 each: H(bJ | bI) = c = -(2/3 ln 2/3 + 1/3 ln 1/6) = 0.8676 nats, H_I = H_J = ln B, H_IJ = ln B + c, and the loss is
    -(ln B - c) / (ln B + c) = -0.600 at B = 32 (held to 0.03: the two half-width end bins and the sampling of 3200 pixels)."""
    I, J, valid = _pair()
    centres = torch.round(I * (bins - 1)) / (bins - 1)
    for v, exact in ((centres, True), (I, False)):
        im = tuple(nmi.axis_map(v.min(), v.max(), bins).tolist())
        jm = torch.tensor(im).expand(v.shape[0], 2)
        H = nmi.joint_histogram(v, v.clone(), valid, im, jm, bins)
        assert torch.equal(H, H.transpose(1, 2))
        loss = nmi.nmi_loss(H)
        if exact:
            assert int((H - torch.diag_embed(torch.diagonal(H, dim1=1, dim2=2))).abs().max()) == 0
            assert float((loss + 1).abs().max()) < 1e-12
        elif bins == 32:
            c = -(2 / 3 * math.log(2 / 3) + 1 / 3 * math.log(1 / 6))
            assert float((loss + (math.log(bins) - c) / (math.log(bins) + c)).abs().max()) < 0.03, loss
        independent = nmi.nmi_loss(nmi.joint_histogram(v, J, valid, im, nmi.axis_map(*nmi.masked_range(J, valid), bins), bins))
        assert bool((loss < independent).all())


def test_independent_inputs_have_a_loss_near_zero():
    """20000 independent uniform pairs, 8 bins: the plug-in mutual information of independent data is about (B-1)^2 / (2 N) = 1.2e-3
    nats, H_IJ about ln 64, so the loss is about -6e-4 (the linear weights smooth, which lowers it further): held to [-0.01, 0]."""
    I, J, valid = _pair(2, 20000, 1)
    loss = nmi.nmi_loss(nmi.joint_histogram(I, J, valid, *_maps(I, J, valid, 8), 8))
    assert bool((loss <= 0).all()) and bool((loss > -0.01).all()), loss


def test_loss_is_invariant_to_an_affine_change_of_j_when_the_range_is_recomputed():
    """J -> a J + b with a = 4, b = -1 (exact in fp32 for these J: multiples of 2^-10 below 1) moves lo and hi by the same map and
    leaves every bin coordinate - hence the histogram - unchanged up to fp32 rounding of the scale; a NEGATIVE a mirrors the
    columns.  The loss agrees to 1e-3."""
    g = torch.Generator().manual_seed(2)
    I = torch.rand((3, 3000), generator=g)
    J = torch.randint(0, 1024, (3, 3000), generator=g).float() / 1024
    valid = torch.rand((3, 3000), generator=g) < 0.8
    bins = 32
    base = nmi.nmi_loss(nmi.joint_histogram(I, J, valid, *_maps(I, J, valid, bins), bins))
    assert bool((base < -1e-3).all())
    for a, b in ((4.0, -1.0), (-2.0, 3.0)):
        J2 = a * J + b
        moved = nmi.nmi_loss(nmi.joint_histogram(I, J2, valid, *_maps(I, J2, valid, bins), bins))
        assert float((moved - base).abs().max()) < 1e-3, (a, b, moved, base)


def test_scale_zero_puts_everything_in_column_zero_and_hi_lands_wholly_in_the_last_bin():
    bins = 5
    I, _, valid = _pair(2, 500, 3)
    const = torch.full_like(I, 0.7)
    jm = nmi.axis_map(*nmi.masked_range(const, valid), bins)
    assert jm[:, 1].tolist() == [0.0, 0.0] and jm[:, 0].tolist() == pytest.approx([0.7, 0.7])
    H = nmi.joint_histogram(I, const, valid, tuple(nmi.axis_map(I.min(), I.max(), bins).tolist()), jm, bins)
    assert int(H[:, :, 1:].abs().max()) == 0 and torch.equal(H[:, :, 0].sum(1), valid.sum(1) * nmi.UNITS)
    # the largest value of an axis: b0 = B - 2, q = 256
    v = torch.tensor([0.25, 1.5, 0.9])
    lo, scale = nmi.axis_map(v.min(), v.max(), bins).tolist()
    b0, q = nmi.axis_place(v, lo, scale, bins)
    assert (int(b0[1]), int(q[1])) == (bins - 2, 256) and (int(b0[0]), int(q[0])) == (0, 0)
    w = N.axis_weights(v, lo, scale, bins)
    assert w[1].tolist() == [0, 0, 0, 0, 256] and w.sum(1).tolist() == [256, 256, 256]


def test_empty_histogram_and_single_cell_have_loss_zero():
    H = torch.zeros((3, 4, 4), dtype=torch.int64)
    H[1, 2, 1] = 5 * nmi.UNITS  # H_IJ = 0
    H[2] = nmi.UNITS  # uniform: independent, loss 0 up to rounding
    loss = nmi.nmi_loss(H)
    assert loss[:2].tolist() == [0.0, 0.0] and abs(float(loss[2])) < 1e-12
    assert nmi.valid_count(H).tolist() == [0.0, 5.0, 16.0]
    assert math.isclose(float(nmi.nmi_loss(torch.diag(torch.tensor([3, 3, 3, 3])) * nmi.UNITS)), -1.0, abs_tol=1e-12)


def test_per_pixel_reference_adds_up_to_the_aggregated_one():
    """pixel_histograms (one pixel per entry) added over a mask's pixels is the aggregated histogram; every pixel's bound is at
    least one unit per J weight, and 0 where the pixel is invalid."""
    c = R.case("even")
    bins = N.PIXEL_BINS
    I, wgt = R.images(c, torch.float32)
    m = c.masks["random"]
    jm = N.j_map(c.J[:1], None, bins)[0]
    values, bounds, valid = N.pixel_histograms(c, c.J[0], jm, bins)
    assert torch.equal(values.sum((2, 3)), valid.long() * nmi.UNITS)
    agg = N.histograms(I, wgt, c.J[:1], m[:1], N.i_map(c, bins), jm[None], bins, torch.arange(R.K_POSES)[None])[0]
    assert torch.equal(values[:, m[0].flatten()].sum(1), agg)
    assert float(bounds[~valid].abs().max()) == 0 and bool((bounds[valid].sum((1, 2)) >= 256).all())


@pytest.mark.parametrize("bad", [1, 65, 0, -3, 2.5, True])
def test_bins_outside_the_range_are_refused(bad):
    with pytest.raises(ValueError, match="nmi_bins"):
        nmi.check_bins(bad, "nmi_bins")
    assert nmi.check_bins(2) == 2 and nmi.check_bins(64) == 64 and nmi.DEFAULT_BINS == 32
