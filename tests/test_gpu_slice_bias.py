"""Slice bias fields on the GPU: the kernel (csrc/slice_bias.hip) against the torch expression in fp64, its refusals, the fused
update against the composed one, ``reconstruct_volume(slice_bias=...)`` on the 32^3 phantom and the command line."""
import json
import math
import os

import pytest
import torch

from test_gpu_robust import MIN_PIXELS, _RES_R, _RES_S, _THICK, _moving_stacks, _psnr, _ulp

# (n, h, w): a single pixel; smaller than every radius; exactly one tile; one pixel past a tile edge both ways with three tiles
# across; 2 x 2 ragged tiles without a mask, with a random one, and with that and an empty slice; a row of two 256-pixel
# segments plus one pixel; the shape of tests/test_slice_bias.py (64-pixel segments, four rows to a workgroup)
CASES = [((1, 1, 1), "none"), ((1, 5, 5), "random"), ((3, 16, 16), "random"), ((2, 17, 33), "random"),
         ((5, 19, 23), "none"), ((5, 19, 23), "random"), ((5, 19, 23), "slice"), ((1, 8, 257), "random"), ((2, 40, 44), "random")]
SIGMAS = (0.3, 1.5, 8.0, 16.0)  # R = 1, 5, 24 (larger than most of the slices) and 48 (the fused path's limit)
LO = 0.05
NAMES = ("n eligible", "sum u", "sum u b_new", "sum u r", "sum u r^2")
_DATA = {}


def _data(shape, kind, device):
    """sim in [0.02, 0.9) (a few per cent below the floor), y = sim exp(field) / gain with a rough field of std 0.2 and a few
    pixels times 3 (beyond the clamp), gains in [0.8, 1.2] that are the scales passed, weights in [0, 1], an incoming field of
    std 0.1; shared by the tests and never written."""
    key = (shape, kind)
    if key not in _DATA:
        n, h, w = shape
        g = torch.Generator().manual_seed(1000 * n + 10 * h + w)
        sim = 0.02 + 0.88 * torch.rand(n, 1, h, w, generator=g)
        scale = 0.8 + 0.4 * torch.rand(n, generator=g)
        y = sim * torch.exp(0.2 * torch.randn(n, 1, h, w, generator=g)) / scale.view(n, 1, 1, 1)
        y = y * (1 + 2 * (torch.rand(n, 1, h, w, generator=g) < 0.02))
        weight = torch.rand(n, 1, h, w, generator=g)
        b = 0.1 * torch.randn(n, 1, h, w, generator=g)
        mask = None
        if kind != "none":
            mask = torch.rand(n, 1, h, w, generator=g) < 0.7
            if kind == "slice":
                mask[1] = False
        _DATA[key] = tuple(None if t is None else t.to(device) for t in (sim, y, mask, scale, weight, b))
    return _DATA[key]


def _away_from_decisions(sim, y, mask, weight, sigma_px):
    """Equality is only defined away from decisions: in fp64 no input within 1e-6 of the floor, no den within 1e-6 of DEN_MIN."""
    from nesvor_amd.slice_bias import DEN_MIN, _rounded, _window, eligible, gaussian_taps

    lo, den_min = _rounded(LO, torch.float32), _rounded(DEN_MIN, torch.float32)
    valid = torch.ones_like(sim, dtype=torch.bool) if mask is None else mask
    assert float((y.double() - lo).abs()[valid].min()) > 1e-6 and float((sim.double() - lo).abs()[valid].min()) > 1e-6
    e = eligible(sim, y, mask, LO)
    u = torch.where(e, torch.ones_like(sim) if weight is None else weight, torch.zeros_like(sim)).double()
    den = _window(u, gaussian_taps(sigma_px).tolist())
    assert float((den - den_min).abs().min()) > 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", CASES)
def test_update_against_the_torch_expression_in_fp64(device, shape, kind):
    """For b_new and each of the four float sums the kernel's largest error against the fp64 expression is at most twice that of
    the same expression evaluated per pixel in fp32 (its sums in fp64) plus one fp32 ulp of the largest magnitude; the count of
    eligible pixels is exact and two calls give equal bits.  Every sigma_px with and without weights, on a nonzero incoming
    field (and once on zeros).  Measured on MI355X (largest over the cases): DESIGN.md, "Slice bias fields"."""
    from nesvor_amd.slice_bias import eligible, field_composed

    sim, y, mask, scale, weight, b = _data(shape, kind, device)
    n = shape[0]
    count = eligible(sim, y, mask, LO).flatten(1).sum(1).double()
    combos = [(s, wt, b) for s in SIGMAS for wt in (None, weight)] + [(1.5, None, torch.zeros_like(b))]
    for sigma_px, wt, b_in in combos:
        _away_from_decisions(sim, y, mask, wt, sigma_px)
        b64, s64 = field_composed(sim.double(), y.double(), mask, scale.double(), None if wt is None else wt.double(), b_in.double(),
                                  sigma_px, LO)
        b32, s32 = field_composed(sim, y, mask, scale, wt, b_in, sigma_px, LO)
        bk, sk = torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, wt, b_in, sigma_px, LO)
        assert bk.shape == sim.shape and bk.dtype == torch.float32 and sk.shape == (n, 5) and sk.dtype == torch.float64
        assert torch.equal(sk[:, 0], count) and torch.equal(s64[:, 0], count)
        if kind == "slice":
            assert bool((sk[1] == 0).all()) and torch.equal(bk[1], b_in[1])  # nothing eligible: no update
        err_k, err_c = float((bk.double() - b64).abs().max()), float((b32.double() - b64).abs().max())
        ulp = _ulp(b64.abs().max())
        print(f"{shape} {kind} sigma_px {sigma_px:g} weight {'none' if wt is None else 'random'} b {'zero' if b_in is not b else 'random'}: "
              f"b_new kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e} (bit-equal to composed: {torch.equal(bk, b32)})")
        assert err_k <= 2 * err_c + ulp
        for j in range(1, 5):
            err_k, err_c = float((sk[:, j] - s64[:, j]).abs().max()), float((s32[:, j] - s64[:, j]).abs().max())
            ulp = _ulp(s64[:, j].abs().max())
            print(f"    {NAMES[j]}: kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e} (largest {float(s64[:, j].abs().max()):.4e})")
            assert err_k <= 2 * err_c + ulp, NAMES[j]
        again_b, again_s = torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, wt, b_in, sigma_px, LO)
        assert torch.equal(again_b, bk) and torch.equal(again_s, sk)


@pytest.mark.gpu
def test_update_takes_a_byte_mask_and_flat_slices(device):
    sim, y, mask, scale, weight, b = _data((5, 19, 23), "random", device)
    bk, sk = torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, weight, b, 1.5, LO)
    b8, s8 = torch.ops.nesvor.slice_bias_update(sim[:, 0], y[:, 0], mask[:, 0].to(torch.uint8), scale, weight[:, 0], b[:, 0], 1.5, LO)
    assert b8.shape == (5, 19, 23) and torch.equal(b8, bk[:, 0]) and torch.equal(s8, sk)
    ones = torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, torch.ones_like(sim), b, 1.5, LO)
    none = torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, None, b, 1.5, LO)
    assert torch.equal(ones[0], none[0]) and torch.equal(ones[1], none[1])
    meta = torch.ops.nesvor.slice_bias_update(sim.to("meta"), y.to("meta"), None, scale.to("meta"), None, b.to("meta"), 1.5, LO)
    assert meta[0].shape == sim.shape and meta[0].dtype == torch.float32 and meta[0].device.type == "meta"
    assert meta[1].shape == (5, 5) and meta[1].dtype == torch.float64


@pytest.mark.gpu
def test_update_refusals(device):
    """Every refusal returns before a launch (csrc/slice_bias.hip: the checks are the first statements of
    nesvor_slice_bias_update), so the sentinels in the field and the sums stay."""
    from nesvor_amd import _lib

    lib = _lib.load()
    n, h, w = 5, 19, 23
    sim, y, mask, scale, weight, b = _data((n, h, w), "random", device)
    out = torch.full((n, h, w), -7.0, device=device)
    stats = torch.full((n, 5), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_slice_bias_update_workspace_bytes(n, h, w))
    assert nbytes == 8 * 5 * n * 4 + 2 * 4 * n * h * w  # 2 x 2 tiles per slice, and the two row-filtered intermediates
    assert lib.nesvor_slice_bias_update_workspace_bytes(0, h, w) == 0 and lib.nesvor_slice_bias_update_workspace_bytes(n, 0, w) == 0
    assert lib.nesvor_slice_bias_update_workspace_bytes(1, 65536, 65536) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    P = _lib.ptr

    def call(n_=n, h_=h, w_=w, sim_=sim, y_=y, scale_=scale, b_=b, out_=out, stats_=stats, ws_=ws, nb=nbytes, sigma_=1.5, r_=5, lo_=LO,
             weight_=weight):
        return lib.nesvor_slice_bias_update(P(sim_), P(y_), P(mask), P(scale_), P(weight_), P(b_), n_, h_, w_, sigma_, r_, lo_, P(out_),
                                            P(stats_), P(ws_), nb, _lib.stream_ptr())

    assert call(nb=nbytes - 1) != 0 and call(nb=0) != 0 and call(ws_=None) != 0  # a short or missing workspace
    assert call(nb=8 * 5 * n * 4) != 0  # room for the partial sums alone
    assert call(n_=-1) != 0 and call(h_=0) != 0 and call(w_=0) != 0 and call(w_=-3) != 0
    assert call(h_=65536, w_=65536) != 0 and call(h_=1, w_=2 ** 31 - 256) != 0  # h w > INT_MAX - 256
    for name in ("sim_", "y_", "scale_", "b_", "out_", "stats_"):
        assert call(**{name: None}) != 0
    assert call(out_=b) != 0  # in place: the row pass reads the neighbours' b
    for bad in (0, -1, 49, 1000):
        assert call(r_=bad) != 0
    for bad in (0.0, -1.5, float("inf"), float("-inf"), float("nan")):
        assert call(sigma_=bad) != 0
    assert call(n_=0) == 0 and call(n_=0, ws_=None, nb=0) == 0  # no slices: a no-op
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((stats == -7.0).all())
    assert call() == 0 and call(weight_=None, r_=48, sigma_=16.0) == 0
    assert call() == 0
    torch.cuda.synchronize()
    direct = torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, weight, b, 1.5, LO)
    assert torch.equal(out.view_as(sim), direct[0]) and torch.equal(stats, direct[1])
    empty = torch.ops.nesvor.slice_bias_update(sim[:0], y[:0], None, scale[:0], None, b[:0], 1.5, LO)
    assert empty[0].shape == (0, 1, h, w) and empty[1].shape == (0, 5)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::slice_bias_update'"):
        torch.ops.nesvor.slice_bias_update(sim.cpu(), y.cpu(), mask.cpu(), scale.cpu(), weight.cpu(), b.cpu(), 1.5, LO)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.slice_bias_update(sim.double(), y.double(), mask, scale.double(), None, b.double(), 1.5, LO)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.slice_bias_update(sim, y, mask, scale.double(), None, b, 1.5, LO)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, weight.double(), b, 1.5, LO)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.nesvor.slice_bias_update(sim.transpose(-1, -2), y.transpose(-1, -2), None, scale, None, b.transpose(-1, -2), 1.5, LO)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        torch.ops.nesvor.slice_bias_update(sim, y, mask.float(), scale, None, b, 1.5, LO)
    with pytest.raises(RuntimeError, match="one shape"):
        torch.ops.nesvor.slice_bias_update(sim, y[:4].contiguous(), mask, scale, None, b, 1.5, LO)
    with pytest.raises(RuntimeError, match="one shape"):
        torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, weight[:4].contiguous(), b, 1.5, LO)
    with pytest.raises(RuntimeError, match="scale"):
        torch.ops.nesvor.slice_bias_update(sim, y, mask, scale[:4].contiguous(), None, b, 1.5, LO)
    with pytest.raises((ValueError, RuntimeError), match="sigma_px"):
        torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, None, b, 0.0, LO)
    with pytest.raises(RuntimeError, match="HIP error"):  # R = 49: the library refuses what field_update never sends
        torch.ops.nesvor.slice_bias_update(sim, y, mask, scale, None, b, 16.2, LO)


# ---------------------------------------------------------------------------------------------------------------------
# the update on both paths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_radius_beyond_the_limit_takes_the_expression(device, monkeypatch):
    from nesvor_amd import slice_bias

    sim, y, mask, scale, weight, b = _data((5, 19, 23), "random", device)
    calls = []
    inner = slice_bias.field_composed
    monkeypatch.setattr(slice_bias, "field_composed", lambda *a: calls.append(1) or inner(*a))
    monkeypatch.delenv("NESVOR_SLICE_BIAS", raising=False)
    assert slice_bias.window_radius(16.2) == 49
    got = slice_bias.field_update(sim, y, mask, scale, weight, b, 16.2, LO)
    assert len(calls) == 1
    want = inner(sim, y, mask, scale, weight, b, 16.2, LO)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    slice_bias.field_update(sim, y, mask, scale, weight, b, 16.0, LO)
    assert len(calls) == 1  # R = 48: the kernel


@pytest.mark.gpu
def test_fused_update_follows_the_composed_one(device, monkeypatch):
    """Three rounds on the (5,19,23) case with its random mask at sigma_px = 8 (R = 24), sim held: fused and composed fields
    each within ``bound`` of the same rounds in fp64 and within twice that of each other.  The bound: a round's update is a
    quotient of two sums of (2 R + 1) fp32 products per pass, two passes, each product and add within 2^-24 relative, of terms
    of size <= CLAMP times the weight's share: 2 x 2 (2 R + 1) 2^-24 CLAMP per round, and a round does not amplify what it is
    given (the smoothed residual of an error takes it back), so three rounds at most three times that."""
    from nesvor_amd import slice_bias

    sim, y, mask, scale, weight, _ = _data((5, 19, 23), "random", device)
    calls = []
    inner = slice_bias.field_composed
    monkeypatch.setattr(slice_bias, "field_composed", lambda *a: calls.append(1) or inner(*a))

    def rounds(cast):
        sb = slice_bias.SliceBias(sigma_mm=12.0)
        for _ in range(3):
            sb.update(cast(sim), cast(y), mask, cast(scale), cast(weight), 1.5)
        return sb

    monkeypatch.delenv("NESVOR_SLICE_BIAS", raising=False)
    fused = rounds(lambda t: t)
    assert not calls  # the fused path never evaluates the torch expression
    monkeypatch.setenv("NESVOR_SLICE_BIAS", "composed")
    composed = rounds(lambda t: t)
    assert len(calls) == 3
    monkeypatch.delenv("NESVOR_SLICE_BIAS")
    exact = rounds(lambda t: t.double())
    assert len(calls) == 6 and exact.b.dtype == torch.float64 and fused.b.dtype == composed.b.dtype == torch.float32
    bound = 3 * 2 * 2 * 49 * 2.0 ** -24 * slice_bias.CLAMP
    gap = lambda a, c: float((a.b.double() - c.b.double()).abs().max())
    print(f"fused - composed {gap(fused, composed):.3e}; against fp64: fused {gap(fused, exact):.3e}, composed {gap(composed, exact):.3e}; "
          f"bound {bound:.3e}; field std {float(exact.b.std()):.4f}; sum u {fused.stats[:, 1].tolist()}")
    assert bool((fused.stats[:, 1] >= slice_bias.MIN_WEIGHT).all()) and float(exact.b.std()) > 0.01
    assert gap(fused, exact) <= bound and gap(composed, exact) <= bound and gap(fused, composed) <= 2 * bound
    assert float((fused.stats - exact.stats).abs().max()) <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_an_update_reads_nothing_back_to_the_host(device, monkeypatch, path):
    """``update`` under torch's synchronisation check: any read of a device value (``.item()``, ``nonzero``, a blocking copy)
    raises there."""
    from nesvor_amd import slice_bias

    sim, y, mask, scale, weight, _ = _data((5, 19, 23), "random", device)
    if path == "composed":
        monkeypatch.setenv("NESVOR_SLICE_BIAS", "composed")
    else:
        monkeypatch.delenv("NESVOR_SLICE_BIAS", raising=False)
    sb = slice_bias.SliceBias(sigma_mm=3.0)
    sb.update(sim, y, mask, scale, weight, 1.5)  # (warm: the library is loaded, the allocator has its blocks)
    sb.update(sim, y, None, None, None, 1.5)
    rms = sb.rms(sim, y, mask)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        sb.update(sim, y, mask, scale, weight, 1.5)
        corrected, rms = sb.corrected(y), sb.rms(sim, y, mask)
        sb.update(sim, y, None, None, None, 1.5)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert corrected.shape == sim.shape and rms.shape == (5,) and bool(torch.isfinite(sb.b).all())
    with pytest.raises(RuntimeError):  # the check is live: a read does raise under it
        torch.cuda.set_sync_debug_mode("error")
        try:
            sb.stats[0, 0].item()
        finally:
            torch.cuda.set_sync_debug_mode(before)


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline on the 32^3 phantom: three still stacks, 1.5 mm pixels, 3 mm slices
# ---------------------------------------------------------------------------------------------------------------------
_STILL = {}
_RUNS = {}


def _still32(device):
    """The 32^3 phantom and its three stacks without motion, normalised by the 0.99 quantile of their masked intensities as
    tests/test_gpu_robust.py::_still does; and the same stacks with every slice multiplied by exp(c1 x + c2 y), x and y from -1
    to 1 across the frame, |c| <= 0.6 (seeded), the exponent with zero mean over the slice's pixels.  Built once, never written."""
    if _STILL:
        return _STILL
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=_RES_S, s_thick=_THICK, motion_deg=0, motion_mm=0, seed=0, normalize=False)
    allv = torch.cat([s.image[s.mask] for s in slices])
    q = torch.kthvalue(allv, max(int(0.99 * allv.numel()), 1)).values
    n = len(slices) // 3
    stacks = [(torch.stack([s.image for s in slices[j * n:(j + 1) * n]]) / q).contiguous() for j in range(3)]
    poses = [RigidTransform.cat([s.transformation for s in slices[j * n:(j + 1) * n]]) for j in range(3)]
    h, w = stacks[0].shape[-2:]
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")
    g = torch.Generator().manual_seed(11)
    biased, truth = [], []
    for s in stacks:
        c = (1.2 * torch.rand(s.shape[0], 2, generator=g) - 0.6).to(device)
        f = c[:, 0].view(-1, 1, 1, 1) * xx.to(device) + c[:, 1].view(-1, 1, 1, 1) * yy.to(device)
        on = (s > 0).float()
        f = f - (f * on).flatten(1).sum(1).view(-1, 1, 1, 1) / on.flatten(1).sum(1).clamp(min=1).view(-1, 1, 1, 1)
        biased.append((s * torch.exp(f)).contiguous())
        truth.append(f)
    _STILL.update(phantom=vol / q, stacks=stacks, biased=biased, truth=torch.cat(truth), poses=poses, n=n)
    return _STILL


def _run(device, which, robust_rounds, bias):
    """One reconstruction of the clean or the biased stacks (n_iter 30; three rounds with either switch), cached."""
    from nesvor_amd.slice_bias import SliceBias
    from nesvor_amd.svr import reconstruct_volume

    key = (which, robust_rounds, bias)
    if key not in _RUNS:
        c = _still32(device)
        out = {}
        extra = dict(slice_bias=SliceBias(), slice_bias_out=out) if bias else {}
        vol = reconstruct_volume(c[which], None, c["poses"], _RES_S, _THICK, _RES_R, n_iter=30, beta=0.02, delta=0.1,
                                 robust_rounds=robust_rounds, **extra)
        _RUNS[key] = (vol, out, _psnr(vol, c["phantom"]))
    return _RUNS[key]


def _field_stats(c, which, out):
    """(std of b - b_true, std of b_true, std of b) over the eligible pixels (of the last round) of the slices with >= 200
    pixels; b_true is 0 for the clean stacks."""
    y = torch.cat(c[which])
    pixels = (y > 0).flatten(1).sum(1)
    assert torch.equal(torch.nonzero(pixels > 0).flatten(), out["keep"])
    assert out["b"].shape == y[out["keep"]].shape  # the stacks share one square frame: no padding
    truth = c["truth"][out["keep"]] if which == "biased" else torch.zeros_like(out["b"])
    big = (pixels[out["keep"]] >= MIN_PIXELS).view(-1, 1, 1, 1)
    e = out["eligible"] & big
    assert not bool((e & ~(y[out["keep"]] > LO)).any())
    return float((out["b"] - truth)[e].std()), float(truth[e].std()), float(out["b"][e].std())


@pytest.mark.gpu
@pytest.mark.parametrize("robust_rounds", [0, 3])
def test_pipeline_recovers_the_slices_fields(device, monkeypatch, robust_rounds):
    """Every slice multiplied by a linear log-field: over the eligible pixels of the slices with >= 200 pixels the std of
    b - b_true is at most 0.75 x the std of b_true, and the PSNR is not below that of the plain run on the same slices minus
    0.1 dB (the project's parity margin; no gain is asserted: this phantom's PSNR is set by blur, not by bias).  Measured on
    MI355X: DESIGN.md, "Slice bias fields"."""
    for name in ("NESVOR_SRR", "NESVOR_ROBUST", "NESVOR_SLICE_BIAS"):
        monkeypatch.delenv(name, raising=False)
    c = _still32(device)
    _, _, p_plain = _run(device, "biased", 0, False)
    _, out, p_bias = _run(device, "biased", robust_rounds, True)
    err, true, got = _field_stats(c, "biased", out)
    print(f"robust_rounds {robust_rounds}: field error std {err:.4f} of {true:.4f}: ratio {err / true:.4f} (estimated std {got:.4f}); "
          f"PSNR plain {p_plain:.3f} dB, with fields {p_bias:.3f} dB; largest bias_rms {float(out['bias_rms'].max()):.4f}")
    assert set(out) == {"b", "stats", "bias_rms", "eligible", "keep"} and out["stats"].shape == (out["keep"].numel(), 5)
    assert err <= 0.75 * true
    assert p_bias >= p_plain - 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("robust_rounds", [0, 3])
def test_pipeline_leaves_clean_slices_nearly_alone(device, monkeypatch, robust_rounds):
    """No field: the estimated fields' std is at most 0.05 (the edge mismatch of a blurry A x, the floor of the method) and the
    PSNR is not below the plain run's minus 0.1 dB."""
    for name in ("NESVOR_SRR", "NESVOR_ROBUST", "NESVOR_SLICE_BIAS"):
        monkeypatch.delenv(name, raising=False)
    c = _still32(device)
    _, _, p_plain = _run(device, "stacks", 0, False)
    _, out, p_bias = _run(device, "stacks", robust_rounds, True)
    _, _, got = _field_stats(c, "stacks", out)
    print(f"robust_rounds {robust_rounds}: estimated field std {got:.4f}; PSNR plain {p_plain:.3f} dB, with fields {p_bias:.3f} dB")
    assert got <= 0.05
    assert p_bias >= p_plain - 0.1


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_svr_with_slice_bias_fields(tmp_path, device, monkeypatch):
    from nesvor_amd import cli, svr
    from nesvor_amd.image_io import load_slices
    from nesvor_amd.slice_bias import SliceBias

    for name in ("NESVOR_SRR", "NESVOR_ROBUST", "NESVOR_STRUCTURAL", "NESVOR_SLICE_BIAS"):
        monkeypatch.delenv(name, raising=False)
    paths, nonempty = _moving_stacks(device, tmp_path)
    made = []
    inner = svr.reconstruct_volume

    def spy(*a, **k):
        vol = inner(*a, **k)
        made.append((a, k, vol.image.clone()))  # (the command rescales the volume it gets in place)
        return vol

    monkeypatch.setattr(svr, "reconstruct_volume", spy)
    out, weights, folder = str(tmp_path / "v.nii.gz"), str(tmp_path / "w.json"), str(tmp_path / "corrected")
    common = ["svr", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--registration", "none", "--n-iter-srr", "6",
              "--verbose", "0", "--output-volume", out]
    cli.main(common + ["--slice-bias-fields", "--slice-weights", weights, "--output-corrected-slices", folder])
    assert len(made) == 1 and isinstance(made[0][1]["slice_bias"], SliceBias) and made[0][1]["robust_rounds"] == 0
    assert made[0][1]["slice_bias"].sigma_mm == 12.0 and made[0][1]["slice_bias"].rounds == 3 and made[0][1]["structural"] is None
    rows = json.load(open(weights))
    assert len(rows) == len(nonempty) > 30
    assert all(set(r) == {"stack", "slice", "bias_rms"} for r in rows)
    assert all(0.0 <= r["bias_rms"] < 1.0 and not math.isnan(r["bias_rms"]) for r in rows) and any(r["bias_rms"] > 0 for r in rows)
    assert [(r["stack"], r["slice"]) for r in rows] == nonempty  # every non-empty slice of every input stack, once, in order
    assert len([f for f in os.listdir(folder) if f.endswith(".nii.gz")]) == len(nonempty)
    written = load_slices(folder, device)
    b = made[0][1]["slice_bias_out"]["b"]
    assert len(written) == b.shape[0] and bool(torch.isfinite(written[0].image).all())
    print("largest bias_rms", max(r["bias_rms"] for r in rows), "field std", float(b.std()))
    # every switch: the rows carry all three sets
    cli.main(common + ["--slice-bias-fields", "--bias-sigma", "9", "--structural-exclusion", "--outlier-rejection", "--robust-rounds", "2",
                       "--slice-weights", weights])
    assert len(made) == 2 and made[1][1]["robust_rounds"] == 2 and made[1][1]["slice_bias"].sigma_mm == 9.0
    rows = json.load(open(weights))
    assert all(set(r) == {"stack", "slice", "weight", "scale", "ncc", "pixel_share", "excluded", "bias_rms"} for r in rows)
    assert [(r["stack"], r["slice"]) for r in rows] == nonempty
    # without the switch: today's call, and the plain pipeline bit for bit
    cli.main(common)
    assert len(made) == 3 and "slice_bias" not in made[2][1] and "slice_bias_out" not in made[2][1]
    a, k, image = made[2]
    direct = inner(*a, **k)
    assert torch.equal(direct.image, image)
