"""Stack denoising on the GPU: the kernel (csrc/denoise.hip) against the torch expression in fp64, its canaries and refusals,
``denoise_stacks`` on both paths and the quality on the phantom."""
import pytest
import torch

import denoise_cases as C
import nesvor_amd  # noqa: F401  (registers torch.ops.nesvor)
from test_gpu_robust import _ulp

# (n, h, w): a single pixel; smaller than every search window; exactly one tile; one pixel past a tile edge both ways with three
# tiles across; 2 x 2 ragged tiles without a mask, with a random one, and with that and an empty slice; a row of 17 tiles; 3 x 3
# tiles, the middle one with a full halo at every radius but the largest
CASES = [((1, 1, 1), "none"), ((1, 5, 5), "random"), ((3, 16, 16), "random"), ((2, 17, 33), "random"),
         ((5, 19, 23), "none"), ((5, 19, 23), "random"), ((5, 19, 23), "slice"), ((1, 8, 257), "random"), ((2, 40, 44), "random")]
RADII = ((1, 1), (1, 3), (2, 5), (3, 10))  # (P, S): the smallest, the defaults, a middle one, the fused path's limits
STRENGTHS = (0.7, 1.0)
_DATA = {}


def _data(shape, kind, device):
    """Values in [0, 1] with structure - a smooth ramp, two steps, noise of 0.05 - a random 70 % mask (one slice emptied for
    ``slice``), sigma per slice 0.02 and 0.1 in turn, slice 2 (where there is one) at 0: copied.  Shared, never written."""
    key = (shape, kind)
    if key not in _DATA:
        n, h, w = shape
        g = torch.Generator().manual_seed(1000 * n + 10 * h + w)
        yy, xx = torch.meshgrid(torch.linspace(0, 1, h), torch.linspace(0, 1, w), indexing="ij")
        y = 0.15 + 0.3 * xx * yy + 0.2 * (xx > 0.4) + 0.25 * (yy > 0.6) + 0.05 * torch.randn(n, 1, h, w, generator=g)
        y = y.clamp(0, 1).contiguous()
        sigma = torch.tensor([(0.02, 0.1)[k % 2] for k in range(n)])
        if n >= 3:
            sigma[2] = 0.0
        mask = None
        if kind != "none":
            mask = torch.rand(n, 1, h, w, generator=g) < 0.7
            if kind == "slice":
                mask[1] = False
        _DATA[key] = tuple(None if t is None else t.to(device) for t in (y, mask, sigma))
    return _DATA[key]


def _held_to_the_rule(got, got_stats, y, mask, sigma, P, S, beta, label):
    """``test_gpu_slice_bias.py``'s rule: the largest error against the expression in fp64 is at most twice that of the expression
    in fp32 plus one fp32 ulp of the largest magnitude, for out and for the sum of squares; the count is exact.  Returns the two
    ratios error / bound."""
    from nesvor_amd.denoise import nlm_composed

    o64, s64 = nlm_composed(y.double(), mask, sigma.double(), P, S, beta)
    o32, s32 = nlm_composed(y, mask, sigma, P, S, beta)
    valid = torch.ones_like(y, dtype=torch.bool) if mask is None else mask
    assert torch.equal(got_stats[:, 0], valid.flatten(1).sum(1).double()) and torch.equal(s64[:, 0], got_stats[:, 0])
    ratios = []
    for name, k, c, e in (("out", got.double(), o32.double(), o64), ("sum (out - y)^2", got_stats[:, 1], s32[:, 1], s64[:, 1])):
        err_k, err_c, ulp = float((k - e).abs().max()), float((c - e).abs().max()), _ulp(e.abs().max())
        print(f"{label} {name}: kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e} ratio {err_k / (2 * err_c + ulp):.3f}"
              + (f" (bit-equal to composed: {torch.equal(got, o32)})" if name == "out" else ""))
        assert err_k <= 2 * err_c + ulp, (label, name)
        ratios.append(err_k / (2 * err_c + ulp))
    return ratios


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,kind", CASES)
def test_kernel_against_the_torch_expression_in_fp64(device, shape, kind):
    """Every (P, S) and strength: out and the sum of squares within the rule above, the valid count exact, two calls equal
    bits, invalid pixels and copied slices equal to the input bit for bit.  The function is continuous in its inputs, so no
    case is kept away from a decision.  Measured on MI355X (largest ratios over the cases): DESIGN.md, "Stack denoising"."""
    y, mask, sigma = _data(shape, kind, device)
    n = shape[0]
    worst = [0.0, 0.0]
    for P, S in RADII:
        for beta in STRENGTHS:
            out, stats = torch.ops.nesvor.nlm_denoise(y, mask, sigma, P, S, beta)
            assert out.shape == y.shape and out.dtype == torch.float32 and stats.shape == (n, 2) and stats.dtype == torch.float64
            r = _held_to_the_rule(out, stats, y, mask, sigma, P, S, beta, f"{shape} {kind} P {P} S {S} strength {beta}")
            worst = [max(a, b) for a, b in zip(worst, r)]
            if mask is not None:
                assert torch.equal(out[~mask], y[~mask])
            copied = ~(sigma > 0)
            assert torch.equal(out[copied], y[copied]) and bool((stats[copied, 1] == 0).all())
            if kind == "slice":
                assert stats[1].tolist() == [0.0, 0.0]
            if shape[1] * shape[2] > 1:
                assert not torch.equal(out, y)
            again, again_stats = torch.ops.nesvor.nlm_denoise(y, mask, sigma, P, S, beta)
            assert torch.equal(again, out) and torch.equal(again_stats, stats)
    print(f"{shape} {kind}: largest ratios out {worst[0]:.3f}, sum {worst[1]:.3f}")


@pytest.mark.gpu
def test_kernel_takes_a_byte_mask_and_flat_slices(device):
    y, mask, sigma = _data((5, 19, 23), "random", device)
    out, stats = torch.ops.nesvor.nlm_denoise(y, mask, sigma, 1, 3, 1.0)
    o8, s8 = torch.ops.nesvor.nlm_denoise(y[:, 0], mask[:, 0].to(torch.uint8), sigma, 1, 3, 1.0)
    assert o8.shape == (5, 19, 23) and torch.equal(o8, out[:, 0]) and torch.equal(s8, stats)
    ones = torch.ops.nesvor.nlm_denoise(y, torch.ones_like(mask), sigma, 1, 3, 1.0)
    none = torch.ops.nesvor.nlm_denoise(y, None, sigma, 1, 3, 1.0)
    assert torch.equal(ones[0], none[0]) and torch.equal(ones[1], none[1])
    bad = sigma.clone()
    bad[0], bad[1], bad[3] = float("nan"), float("inf"), -1.0
    out, stats = torch.ops.nesvor.nlm_denoise(y, mask, bad, 2, 5, 1.0)
    assert torch.equal(out[:4], y[:4]) and not torch.equal(out[4], y[4]) and bool((stats[:4, 1] == 0).all())
    empty = torch.ops.nesvor.nlm_denoise(y[:0], None, sigma[:0], 1, 3, 1.0)
    assert empty[0].shape == (0, 1, 19, 23) and empty[1].shape == (0, 2)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.nlm_denoise(y.double(), mask, sigma.double(), 1, 3, 1.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.nesvor.nlm_denoise(y.transpose(-1, -2), None, sigma, 1, 3, 1.0)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        torch.ops.nesvor.nlm_denoise(y, mask.float(), sigma, 1, 3, 1.0)
    with pytest.raises(RuntimeError, match="sigma"):
        torch.ops.nesvor.nlm_denoise(y, mask, sigma[:4].contiguous(), 1, 3, 1.0)
    with pytest.raises(RuntimeError, match="HIP error"):  # the library refuses what denoise.nlm never sends
        torch.ops.nesvor.nlm_denoise(y, mask, sigma, 4, 3, 1.0)


@pytest.mark.gpu
def test_kernel_writes_nothing_outside_out_and_stats(device):
    """out and stats inside larger poisoned buffers, at the limits of the radii and at the defaults."""
    from nesvor_amd import _lib

    lib = _lib.load()
    P_ = _lib.ptr
    pad, poison = 1024, -7.0
    for shape, kind in (((5, 19, 23), "random"), ((2, 17, 33), "random"), ((1, 1, 1), "none")):
        n, h, w = shape
        y, mask, sigma = _data(shape, kind, device)
        nbytes = int(lib.nesvor_nlm_denoise_workspace_bytes(n, h, w))
        for P, S in ((1, 3), (3, 10)):
            big = torch.full((n * h * w + 2 * pad,), poison, device=device)
            big_stats = torch.full((2 * n + 2 * pad,), poison, dtype=torch.float64, device=device)
            big_ws = torch.full((nbytes // 8 + 2 * pad,), poison, dtype=torch.float64, device=device)
            out, stats, ws = big[pad:pad + n * h * w], big_stats[pad:pad + 2 * n], big_ws[pad:pad + nbytes // 8]
            assert lib.nesvor_nlm_denoise(P_(y), P_(mask), P_(sigma), n, h, w, P, S, 1.0, P_(out), P_(stats), P_(ws), nbytes,
                                          _lib.stream_ptr()) == 0
            torch.cuda.synchronize()
            for buf in (big, big_stats, big_ws):
                assert bool((buf[:pad] == poison).all()) and bool((buf[-pad:] == poison).all())
            direct = torch.ops.nesvor.nlm_denoise(y, mask, sigma, P, S, 1.0)
            assert torch.equal(out.view_as(y), direct[0]) and torch.equal(stats.view(n, 2), direct[1])


@pytest.mark.gpu
def test_kernel_refusals(device):
    """Every refusal returns before a launch (csrc/denoise.hip: the checks are the first statements of nesvor_nlm_denoise), so
    the sentinels in out and the sums stay."""
    from nesvor_amd import _lib

    lib = _lib.load()
    n, h, w = 5, 19, 23
    y, mask, sigma = _data((n, h, w), "random", device)
    out = torch.full((n, h, w), -7.0, device=device)
    stats = torch.full((n, 2), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_nlm_denoise_workspace_bytes(n, h, w))
    assert nbytes == 8 * 2 * n * 4  # 2 x 2 tiles per slice
    assert lib.nesvor_nlm_denoise_workspace_bytes(1, 16, 16) == 16 and lib.nesvor_nlm_denoise_workspace_bytes(3, 17, 33) == 8 * 2 * 3 * 6
    assert lib.nesvor_nlm_denoise_workspace_bytes(0, h, w) == 0 and lib.nesvor_nlm_denoise_workspace_bytes(n, 0, w) == 0
    assert lib.nesvor_nlm_denoise_workspace_bytes(1, 65536, 65536) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    P_ = _lib.ptr

    def call(n_=n, h_=h, w_=w, y_=y, sigma_=sigma, out_=out, stats_=stats, ws_=ws, nb=nbytes, p_=1, s_=3, beta_=1.0):
        return lib.nesvor_nlm_denoise(P_(y_), P_(mask), P_(sigma_), n_, h_, w_, p_, s_, beta_, P_(out_), P_(stats_), P_(ws_), nb,
                                      _lib.stream_ptr())

    invalid = 1  # hipErrorInvalidValue
    assert call(nb=nbytes - 1) == invalid and call(nb=0) == invalid and call(ws_=None) == invalid  # a short or missing workspace
    assert call(n_=-1) == invalid and call(h_=0) == invalid and call(w_=0) == invalid and call(w_=-3) == invalid
    assert call(h_=65536, w_=65536) == invalid and call(h_=1, w_=2 ** 31 - 256) == invalid  # h w > INT_MAX - 256
    assert call(n_=2 ** 30 + 1, h_=17, w_=16) == invalid  # two tiles per slice: more than INT_MAX workgroups
    for name in ("y_", "sigma_", "out_", "stats_"):
        assert call(**{name: None}) == invalid
    assert call(out_=y) == invalid  # in place: a tile reads its neighbours' y
    for bad in (0, -1, 4, 1000):
        assert call(p_=bad) == invalid
    for bad in (0, -1, 11, 1000):
        assert call(s_=bad) == invalid
    for bad in (0.0, -1.5, float("inf"), float("-inf"), float("nan")):
        assert call(beta_=bad) == invalid
    assert call(n_=0) == 0 and call(n_=0, ws_=None, nb=0) == 0  # no slices: a no-op
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((stats == -7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    direct = torch.ops.nesvor.nlm_denoise(y, mask, sigma, 1, 3, 1.0)
    assert torch.equal(out.view_as(y), direct[0]) and torch.equal(stats, direct[1])
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::nlm_denoise'"):
        torch.ops.nesvor.nlm_denoise(y.cpu(), mask.cpu(), sigma.cpu(), 1, 3, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# the switches
# ---------------------------------------------------------------------------------------------------------------------
def _stack(device, sigma=0.06):
    from nesvor_amd.image import Stack

    clean, noisy, mask = C.phantom_stack(sigma)
    return clean, noisy, mask, Stack(noisy.to(device), mask.to(device))


@pytest.mark.gpu
def test_denoise_stacks_takes_the_op_and_agrees_with_the_expression(device, monkeypatch):
    from nesvor_amd import denoise

    calls = []
    inner = denoise.nlm_composed
    monkeypatch.setattr(denoise, "nlm_composed", lambda *a: calls.append(1) or inner(*a))
    monkeypatch.delenv("NESVOR_DENOISE", raising=False)
    _, noisy, mask, st = _stack(device)
    pose = st.transformation.axisangle().clone()
    fused = denoise.denoise_stacks([st])[0]
    assert not calls and fused["fused"] and st.slices.dtype == torch.float32 and st.slices.is_cuda
    assert torch.equal(st.mask.cpu(), mask) and torch.equal(st.transformation.axisangle(), pose)
    monkeypatch.setenv("NESVOR_DENOISE", "composed")
    _, _, _, st2 = _stack(device)
    composed = denoise.denoise_stacks([st2])[0]
    assert len(calls) == 1 and not composed["fused"]
    assert torch.equal(fused["sigma"], composed["sigma"]) and fused["n_used"] == composed["n_used"]
    monkeypatch.delenv("NESVOR_DENOISE")
    y, m = noisy.to(device), mask.to(device)
    _held_to_the_rule(st.slices, fused["stats"], y, m, fused["sigma"].expand(12).contiguous(), 1, 3, 1.0, "phantom stack")
    print("fused - composed", float((st.slices - st2.slices).abs().max()))
    # a radius outside the fused limits falls back to the expression
    _, _, _, st3 = _stack(device)
    wide = denoise.denoise_stacks([st3], patch_radius=4, search_radius=2, sigma=0.06)[0]
    assert len(calls) == 4 and not wide["fused"] and wide["n_used"] == 0 and not torch.equal(st3.slices, y)
    _, _, _, st4 = _stack(device)
    denoise.denoise_stacks([st4], patch_radius=3, search_radius=10, sigma=0.06)
    assert len(calls) == 4  # the limits themselves: the kernel
    st5 = _stack(device)[3]
    st5.slices = st5.slices.double()
    assert not denoise.denoise_stacks([st5])[0]["fused"] and st5.slices.dtype == torch.float64 and len(calls) == 5


@pytest.mark.gpu
def test_quality_on_the_phantom_on_the_fused_path(device, monkeypatch):
    """tests/test_denoise.py's quality test on the kernel: at sigma = 0.06 the masked PSNR rises by at least 1 dB and the
    estimate lies within 0.9 .. 1.3 of the truth; at sigma = 0.03 a rise."""
    from nesvor_amd.denoise import denoise_stacks, method_noise_rms

    monkeypatch.delenv("NESVOR_DENOISE", raising=False)
    for sigma, gain in ((0.06, 1.0), (0.03, 0.0)):
        clean, noisy, mask, st = _stack(device, sigma)
        rep = denoise_stacks([st])[0]
        before, after = C.masked_psnr(noisy, clean, mask), C.masked_psnr(st.slices, clean, mask)
        print(f"sigma {sigma}: PSNR {before:.2f} -> {after:.2f} dB, estimate {float(rep['sigma']):.4f} on {rep['n_used']} pixels, "
              f"method noise rms {method_noise_rms(rep['stats']):.4f}")
        assert rep["fused"] and torch.equal(st.slices.cpu()[~mask], noisy[~mask])
        if gain > 0:
            assert after >= before + gain and 0.9 * sigma <= float(rep["sigma"]) <= 1.3 * sigma
        else:
            assert after > before
