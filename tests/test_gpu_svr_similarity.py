"""The similarity sums of csrc/svr.hip (``torch.ops.nesvor.svr_similarity``) against the CPU acquisition oracle, PER PIXEL and
aggregated, on the geometries of tests/acq_geometry.py; reference and bounds: tests/svr_reference.py (derived there, none fitted
to the kernel; its CPU conditions on the seeds: tests/test_svr_reference.py).

Per pixel: h w slices that all hold one image, slice i's mask keeping pixel i alone, so that entry (i, k) is
{v, v I, v I^2, v I J, v J, v J^2} of that pixel under that pose - an error of random sign cannot cancel, and one dropped tap of
1024 shows.  K = 27 distinct poses (6 lattice + 21 generic; passes of 13 + 13 + 1), slice i taking the list rolled by i.  The
aggregated runs are held to the reference and, within the summation term alone, to the kernel's own per-pixel values added up on
the host, which separates the reduction from the per-pixel arithmetic.

Every run prints ``RATIO <case> <what> <largest error / bound>``; DESIGN.md, "Slice-to-volume registration", has the table."""
import pytest
import torch

import svr_reference as R
from acq_geometry import GEOMETRIES, OUTSIDE, _lattice_poses

pytestmark = pytest.mark.gpu

K = R.K_POSES
PIXEL_CASES = [(g, None) for g in GEOMETRIES] + [("even", p) for p in R.SPECIAL_PSFS]
PIXEL_IDS = [p or g for g, p in PIXEL_CASES]
_RUNS = {}


def _svr(device, c, tf, slices, mask, psf=None, vol=None):
    out = torch.ops.nesvor.svr_similarity((c.vol if vol is None else vol).to(device), (c.psf if psf is None else psf).to(device),
                                          tf.contiguous().to(device), slices.contiguous().to(device), None if mask is None else mask.to(device),
                                          c.res)
    assert out.shape == (tf.shape[0], tf.shape[1], 6) and out.dtype == torch.float64
    return out.cpu()


def _one_hot(device, c, k=K):
    """(h w, k, 6): slice i = image 0 with pixel i alone unmasked, under the leading k poses of its rolled list.  Run once."""
    key = (c.key, k)
    if key not in _RUNS:
        h, w = c.shape
        n = h * w
        _RUNS[key] = _svr(device, c, c.poses[R.pose_ids(n, k)], c.J[0].expand(n, h, w), torch.eye(n, dtype=torch.bool).view(n, h, w))
    return _RUNS[key]


def _by_entry(per_pose, pid):
    """(27, n_pix, ...) by pose -> (n_pix, k, ...) by entry of the one-hot run."""
    return per_pose[pid, torch.arange(pid.shape[0])[:, None].expand_as(pid)]


def _by_pose(c, full):
    """The full one-hot run (n_pix, 27, 6) -> (27, n_pix, 6) by pose: pose p stands at position (p - i) mod 27 of slice i."""
    n = full.shape[0]
    pos = (torch.arange(K)[:, None] - torch.arange(n)[None, :]) % K
    return full[torch.arange(n)[None, :].expand_as(pos), pos]


def _hold(got, want, bound, what):
    """|got - want| <= bound element by element (equality where the bound is 0); prints and returns the largest error / bound."""
    err = (got - want).abs()
    free = bound > 0
    ratio = float((err[free] / bound[free]).max()) if bool(free.any()) else 0.0
    print(f"RATIO {what} {ratio:.4f}")
    assert torch.equal(got[~free], want[~free]), (what, "an exact element differs", int((got[~free] != want[~free]).sum()))
    assert ratio <= 1, (what, ratio)
    return ratio


def _check_pixels(c, got, pid, what):
    """A one-hot run's entries against the fp32 oracle: count and J exactly, the rest within pixel_bounds, exact zeros where the
    oracle has no valid pixel."""
    h, w = c.shape
    I, wgt = R.images(c, torch.float32)
    J = c.J[0]
    want = _by_entry(R.pixel_values(I, wgt, J).view(K, h * w, 6), pid)
    bound = _by_entry(R.pixel_bounds(I, J).view(K, h * w, 6), pid)
    valid = _by_entry((wgt > 0).view(K, h * w), pid)
    assert torch.equal(got[..., 0], valid.double()), (what, "validity differs from the fp32 oracle at", int((got[..., 0] != valid.double()).sum()))
    assert float(got[~valid].abs().max() if bool((~valid).any()) else 0) == 0
    assert not bool(valid[pid == OUTSIDE].any()) and float(got[pid == OUTSIDE].abs().max() if bool((pid == OUTSIDE).any()) else 0) == 0
    _hold(got, want, bound * valid[..., None], what)


# ---------------------------------------------------------------------------------------------------------------------
# per pixel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,psf", PIXEL_CASES, ids=PIXEL_IDS)
def test_every_pixel_under_every_pose(device, geom, psf):
    """Every geometry with its own PSF; on "even" also 1024 taps (the last LDS entry), a PSF with half of its taps exactly 0 (the tap
    skip), a single tap off centre and the all-zero PSF (every entry exact zeros).  Lattice poses (decisions exact in fp32) and
    generic ones alike: count equal to the fp32 oracle's validity, values within pixel_bounds, zeros where invalid."""
    c = R.case(geom, psf)
    got = _one_hot(device, c)
    h, w = c.shape
    assert got.shape == (h * w, K, 6)
    if psf == "all_zero":
        assert float(got.abs().max()) == 0
    else:
        assert (c.psf.numel() == 1024 and bool((c.psf != 0).all())) == (psf == "psf1688")
        assert float(got[..., 0].mean()) >= 0.05
    _check_pixels(c, got, R.pose_ids(h * w), f"{psf or geom} pixel")


@pytest.mark.parametrize("geom,psf", PIXEL_CASES, ids=PIXEL_IDS)
def test_valid_set_is_the_acquisition_kernels(device, geom, psf):
    """The header's design claim: valid set and value are the ones slice_acq_fwd produces (both kernels call csrc/acq_taps.h) -
    generic poses too.  All pixels unmasked: the count of every pose equals the number of weight > 0 of
    ``slice_acq_cuda.forward``; and pixel by pixel from the one-hot run, where a single non-zero term enters the wave sum and every
    later add is in double: the validity, and on every valid pixel sum I equal to the operator's ``slices`` BIT FOR BIT under the
    same pose and sum I^2 equal to its fp32 square."""
    from nesvor_amd import slice_acq_cuda as A

    c = R.case(geom, psf)
    e = torch.empty(0, device=device)
    sim, wgt = A.forward(c.poses.to(device), c.vol[None, None].to(device), e, e, c.psf.to(device), c.shape, c.res, True, False)
    valid = (wgt[:, 0] > 0).cpu()
    got = _svr(device, c, c.poses[None], c.J[:1], None)
    assert torch.equal(got[0, :, 0], valid.flatten(1).sum(1).double())
    own = _by_pose(c, _one_hot(device, c))  # (27, h w, 6)
    assert torch.equal(own[..., 0], valid.flatten(1).double())
    I, v = sim[:, 0].cpu().flatten(1), valid.flatten(1)
    assert I.dtype == torch.float32
    for col, want in ((1, I), (2, I * I)):
        differs = (own[..., col] != want.double()) & v
        assert not bool(differs.any()), (col, "first (pose, pixel) that differs", differs.nonzero()[0].tolist(), int(differs.sum()))


# ---------------------------------------------------------------------------------------------------------------------
# aggregated
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask", R.MASKS + ["random_nan"])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_aggregated_sums(device, geom, mask):
    """Five slices with distinct images; masks: none, random about 70 %, slice 1 fully masked, one pixel of the last, ragged
    workgroup alone (the one valid under the most poses).  Against svr_reference.sums within sum_bounds, the count exactly;
    against the kernel's own per-pixel I and validity (the one-hot run) with the products formed in fp32 and added in double on
    the host, within the summation term alone.  ``random_nan``: NaN in ``slices`` wherever the mask is off changes no bit of the
    output."""
    c = R.case(geom)
    h, w = c.shape
    pid = R.pose_ids(5)
    m = c.masks["random" if mask == "random_nan" else mask]
    J = c.J
    if mask == "random_nan":
        J = torch.where(m, c.J, torch.full_like(c.J, float("nan")))
        assert int(torch.isnan(J).sum()) > 0
    key = (c.key, "sums", "random" if mask == "random_nan" else mask)
    got = _svr(device, c, c.poses[pid], J, m)
    if mask == "random_nan":
        assert torch.equal(got, _RUNS[key] if key in _RUNS else _svr(device, c, c.poses[pid], c.J, m))
    _RUNS[key] = got
    rows = torch.arange(5)[:, None]
    I, wgt = R.images(c, torch.float32)
    ref = R.sums(I, wgt, c.J, m)
    bound = R.sum_bounds(I, wgt, c.J, m, ref)
    assert torch.equal(got[..., 0], ref[rows, pid][..., 0])
    if mask == "slice_off":
        assert float(got[1].abs().max()) == 0 and float(got[0, :, 0].max()) > 0
    if mask == "last_pixel":
        assert float(got[..., 0].max()) == 1
    _hold(got, ref[rows, pid], bound[rows, pid], f"{geom} sums/{mask}")
    # the reduction alone: the kernel's own per-pixel values
    own = _by_pose(c, _one_hot(device, c))  # (27, h w, 6)
    Ik, vk = own[..., 1].float().view(1, K, h, w), own[..., 0].view(1, K, h, w)
    if m is not None:
        vk = vk * m[:, None].double()
    Ie, Je = Ik.expand(5, K, h, w), c.J[:, None].expand(5, K, h, w)
    terms = torch.stack([torch.ones_like(Ie), Ie, Ie * Ie, Ie * Je, Je, Je * Je], -1)
    assert terms.dtype == torch.float32
    host = (terms.double() * vk[..., None]).sum((2, 3))
    _hold(got, host[rows, pid], R.summation_term(host)[rows, pid], f"{geom} reduction/{mask}")


# ---------------------------------------------------------------------------------------------------------------------
# pass composition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 12, 13, 14, 25, 26, 27])
def test_pass_composition(device, k):
    """13-pose passes, then singles: 1; 12 singles; 13; 13 + 1; 13 + 12; 13 + 13; 13 + 13 + 1.  The leading k poses of every slice's
    list, per pixel on "even": every entry is the K = 27 run's bit for bit, and holds against the reference."""
    c = R.case("even")
    h, w = c.shape
    full = _one_hot(device, c)
    h_w = h * w
    pid = R.pose_ids(h_w, k)
    tf = c.poses[pid]
    got = _svr(device, c, tf, c.J[0].expand(h_w, h, w), torch.eye(h_w, dtype=torch.bool).view(h_w, h, w))
    assert torch.equal(got, full[:, :k])
    _check_pixels(c, got, pid, f"even passes/{k}")


# ---------------------------------------------------------------------------------------------------------------------
# stack sizes, thin volumes, a one-pixel slice
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 300])
def test_stack_sizes(device, n):
    """One slice of (7,9), and 300 slices of (2,2) (a workgroup per slice, three of its waves idle) on the (5,7,9) volume, 14 poses
    each (a 13-pose pass and a single).  Lattice poses as tests/test_gpu_slice_acq_geometry.py::test_stack_sizes builds them - the
    three rotations in turn, translations from the multiples of 1/4 in [-3, 3], every (slice, pose) its own - so the count is
    exact; masks on (slice 1 fully masked)."""
    from oracle import slice_acq as O

    dims, _, res, _ = GEOMETRIES["odd"]
    c = R.case("odd")
    k = 14
    g = torch.Generator().manual_seed(180 + n)
    shape = (2, 2) if n > 1 else (7, 9)
    rots = _lattice_poses(dims)[:3, :, :3]
    t = torch.randint(-12, 13, (n, k, 3), generator=g).float() / 4
    tf = torch.cat([rots[(torch.arange(n)[:, None] + torch.arange(k)[None, :]) % 3], t[..., None]], -1)
    J = torch.rand((n,) + shape, generator=g)
    m = torch.rand((n,) + shape, generator=g) < 0.7
    if n > 1:
        m[1] = False
    I, wgt = O.slice_acquisition_forward(tf.view(n * k, 3, 4), c.vol[None, None], None, None, c.psf, shape, res, True, False)
    I, wgt = I.view(n, k, *shape), wgt.view(n, k, *shape)
    share = float((wgt > 0).double().mean())
    assert 0.05 <= share < 1, share  # (both kinds of pixel are there)
    ref = R.sums(I, wgt, J, m)
    got = _svr(device, c, tf, J, m)
    assert torch.equal(got[..., 0], ref[..., 0]) and float(ref[..., 0].max()) > 0
    _hold(got, ref, R.sum_bounds(I, wgt, J, m, ref), f"stack/{n}")


@pytest.mark.parametrize("dims", [(1, 7, 9), (5, 1, 9), (5, 7, 1)], ids=lambda d: "x".join(map(str, d)))
def test_volume_one_voxel_thick_has_no_valid_pixel(device, dims):
    """No position satisfies 0 <= coord < dim - 1 along the thin axis: every entry is exact zeros, under lattice and generic poses."""
    c = R.case("odd")
    g = torch.Generator().manual_seed(sum(dims))
    tf = torch.cat([_lattice_poses(dims), c.poses[R.N_LATTICE:]])[None].expand(2, -1, -1, -1)
    got = _svr(device, c, tf, c.J[:2], None, vol=torch.rand(dims, generator=g))
    assert got.shape == (2, K, 6) and float(got.abs().max()) == 0


def test_one_pixel_slice(device):
    """A (1,1) slice: w - 1 = h - 1 = 0 in the pixel's offset; three slices on the "odd" volume under its 27 poses."""
    from oracle import slice_acq as O

    c = R.case("odd")
    J = torch.rand((3, 1, 1), generator=torch.Generator().manual_seed(11))
    pid = R.pose_ids(3)
    I, wgt = O.slice_acquisition_forward(c.poses, c.vol[None, None], None, None, c.psf, (1, 1), c.res, True, False)
    I, wgt = I[:, 0], wgt[:, 0]  # (27,1,1)
    assert 5 <= int((wgt > 0).sum()) < K
    got = _svr(device, c, c.poses[pid], J, None)
    rows = torch.arange(3)[:, None]
    valid = (wgt > 0).view(1, K).expand(3, -1)
    want = R.pixel_values(I[None].expand(3, -1, -1, -1), wgt[None].expand(3, -1, -1, -1), J[:, None]).view(3, K, 6)
    bound = R.pixel_bounds(I[None].expand(3, -1, -1, -1), J[:, None]).view(3, K, 6) * valid[..., None]
    assert torch.equal(got[..., 0], valid[rows, pid].double())
    _hold(got, want[rows, pid], bound[rows, pid], "one-pixel slice")


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: every element written, nothing else
# ---------------------------------------------------------------------------------------------------------------------
def test_every_sum_is_written_and_nothing_past_the_workspace(device):
    """``sums`` pre-filled with -7 (no sum is negative) and a workspace 64 doubles longer than the library asks for, filled with -7:
    after the call no sentinel is left in ``sums``, the tail is untouched, the result is what the op returns, and a second call
    gives the same bits.  "sparse": two workgroups per slice, the second ragged; random mask."""
    from nesvor_amd import _lib

    c = R.case("sparse")
    lib, P = _lib.load(), _lib.ptr
    h, w = c.shape
    n, tail = 5, 64
    pid = R.pose_ids(n)
    vol, psf, tf = c.vol.to(device), c.psf.to(device), c.poses[pid].contiguous().to(device)
    J, m = c.J.to(device), c.masks["random"].to(device)
    nbytes = int(lib.nesvor_svr_similarity_workspace_bytes(n, K, h, w))
    assert nbytes == 8 * 6 * n * K * 2

    def call():
        sums = torch.full((n, K, 6), -7.0, dtype=torch.float64, device=device)
        ws = torch.full((nbytes // 8 + tail,), -7.0, dtype=torch.float64, device=device)
        err = lib.nesvor_svr_similarity(P(vol), *c.dims, P(psf), *c.psf.shape, P(tf), P(J), P(m), n, K, h, w, c.res, P(sums), P(ws),
                                        nbytes + 8 * tail, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert err == 0
        assert bool((ws[nbytes // 8:] == -7.0).all()) and not bool((ws[:nbytes // 8] == -7.0).any())
        return sums

    first = call()
    assert not bool((first == -7.0).any()) and bool(torch.isfinite(first).all())
    assert torch.equal(first, call())
    assert torch.equal(first.cpu(), _svr(device, c, c.poses[pid], c.J, c.masks["random"]))
