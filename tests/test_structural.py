"""Structural exclusion of the classical reconstruction (nesvor_amd/structural.py) on host tensors in fp64 - the composed path,
which is also the yardstick of tests/test_gpu_structural.py -, its routing through ``reconstruct_volume`` and the ``svr``
command's flags."""
import pytest
import torch
import torch.nn.functional as F

from test_robust import EMPTY, N, _dense_pipeline, _synthetic

PERMUTED = {1: (3, 17, 30), 6: (0, 3, 8, 11, 14, 17, 22, 27, 30, 33)}


# ---------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------
def test_taps_sum_to_one_and_are_the_gaussian():
    from nesvor_amd.structural import gaussian_taps

    g = gaussian_taps()
    assert g.shape == (11,) and g.dtype == torch.float64 and float(g.sum()) == pytest.approx(1.0, abs=1e-15)
    t = torch.arange(11, dtype=torch.float64)
    expected = torch.exp(-(t - 5) ** 2 / (2 * 1.5 ** 2))
    assert torch.allclose(g, expected / expected.sum(), rtol=0, atol=1e-15)
    assert torch.equal(g, g.flip(0)) and gaussian_taps(torch.float32).dtype == torch.float32


def test_a_slice_against_itself_is_one_on_the_mask_and_zero_off_it():
    from nesvor_amd.structural import ssim_composed

    sim, _, mask, _, _ = _synthetic(0, ())
    ssim, stats = ssim_composed(sim, sim, mask, torch.ones(N, dtype=torch.float64))
    assert ssim.shape == sim.shape and ssim.dtype == torch.float64 and stats.shape == (N, 8) and stats.dtype == torch.float64
    assert float((ssim[mask] - 1).abs().max()) <= 1e-12
    assert bool((ssim[~mask] == 0).all())
    assert torch.equal(stats[:, 0], mask.flatten(1).sum(1).double())
    assert bool((stats[EMPTY] == 0).all())
    assert torch.equal(stats[:, 2], torch.zeros(N, dtype=torch.float64))  # nothing below the threshold
    assert torch.allclose(stats[:, 1], stats[:, 0], rtol=0, atol=1e-9)


@pytest.mark.parametrize("a,b,L", [(0.5, 0.5, 1.0), (0.8, 0.2, 1.0), (0.3, 0.9, 2.0), (0.0, 0.4, 1.0)])
def test_a_constant_pair_gives_the_luminance_term(a, b, L):
    """Both variances and the covariance vanish (to rounding), so ssim = (2ab + C1) / (a^2 + b^2 + C1), whatever the mask cuts
    out of the window."""
    from nesvor_amd.structural import ssim_composed

    _, _, mask, _, _ = _synthetic(0, ())
    sim = torch.full((N, 1, 19, 23), b, dtype=torch.float64)
    y = torch.full_like(sim, a / 2)
    ssim, stats = ssim_composed(sim, y, mask, torch.full((N,), 2.0, dtype=torch.float64), 0.4, L)
    c1 = (0.01 * L) ** 2
    expected = (2 * a * b + c1) / (a * a + b * b + c1)
    assert float((ssim[mask] - expected).abs().max()) <= 1e-10
    assert bool((ssim[~mask] == 0).all())
    n = mask.flatten(1).sum(1).double()
    assert torch.allclose(stats[:, 3], a * n, rtol=1e-12) and torch.allclose(stats[:, 4], b * n, rtol=1e-12)
    assert torch.allclose(stats[:, 7], a * b * n, rtol=1e-12)
    assert torch.equal(stats[:, 2], n if expected < 0.4 else torch.zeros_like(n))


def test_without_a_mask_the_interior_is_the_conv2d_gaussian_ssim():
    """Away from the border the window is whole (Wt = 1 to rounding): the textbook SSIM, here through ``F.conv2d`` with the
    outer product of the taps."""
    from nesvor_amd.structural import gaussian_taps, ssim_composed

    g = torch.Generator().manual_seed(11)
    n, h, w = 3, 40, 45
    sim = torch.rand(n, 1, h, w, generator=g, dtype=torch.float64)
    y = (sim + 0.1 * torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)).clamp(min=0)
    scale = 0.8 + 0.4 * torch.rand(n, generator=g, dtype=torch.float64)
    ssim, stats = ssim_composed(sim, y, None, scale)
    taps = gaussian_taps()
    kernel = torch.outer(taps, taps)[None, None]
    blur = lambda a: F.conv2d(a, kernel, padding=5)
    i, j = scale.view(n, 1, 1, 1) * y, sim
    mu_i, mu_j = blur(i), blur(j)
    var_i, var_j, cov = blur(i * i) - mu_i ** 2, blur(j * j) - mu_j ** 2, blur(i * j) - mu_i * mu_j
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    expected = (2 * mu_i * mu_j + c1) * (2 * cov + c2) / ((mu_i ** 2 + mu_j ** 2 + c1) * (var_i + var_j + c2))
    inner = (slice(None), slice(None), slice(11, h - 11), slice(11, w - 11))
    gap = float((ssim[inner] - expected[inner]).abs().max())
    print("largest gap to the conv2d SSIM in the interior", gap)
    assert gap <= 1e-10
    assert torch.equal(stats[:, 0], torch.full((n,), float(h * w), dtype=torch.float64))
    assert torch.allclose(stats[:, 1], ssim.flatten(1).sum(1), rtol=1e-14)


# ---------------------------------------------------------------------------------------------------------------------
# the decisions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("true_gains", [True, False])
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6])
def test_decisions_on_permuted_and_clean_slices(seed, true_gains):
    """Permuted slices: r < 0.5 and at most 10 % of their pixels kept; every other non-empty slice: r >= 0.5 and at least 80 %
    kept; with the true gains as scales and with ones (the slices then differ from their simulations by factors 0.7 .. 1.3)."""
    from nesvor_amd.structural import StructuralExclusion

    bad = PERMUTED.get(seed, ())
    sim, y, mask, gain, _ = _synthetic(seed, bad)
    se = StructuralExclusion().update(sim, y, mask, gain if true_gains else None)
    r, share = se.ncc, se.pixel_share()
    good = [k for k in range(N) if k not in bad and k != EMPTY]
    print(f"seed {seed} gains {true_gains}: good r >= {float(r[good].min()):.4f} share >= {float(share[good].min()):.4f}"
          + (f"; permuted r <= {float(r[list(bad)].max()):.4f} share <= {float(share[list(bad)].max()):.4f}" if bad else ""))
    assert r.dtype == share.dtype == torch.float64 and r.shape == share.shape == (N,)
    for k in bad:
        assert float(r[k]) < 0.5 and float(share[k]) <= 0.1 and not bool(se.slice_keep[k])
    for k in good:
        assert float(r[k]) >= 0.5 and float(share[k]) >= 0.8 and bool(se.slice_keep[k])
    assert not bool(se.slice_keep[EMPTY]) and float(share[EMPTY]) == 0.0 and float(r[EMPTY]) == 0.0
    # the state and the multiplier
    assert se.pixel_keep.dtype == torch.bool and torch.equal(se.pixel_keep, mask & (se.ssim >= 0.4))
    weights = se.weights()
    assert weights.dtype == sim.dtype and torch.equal(weights, (se.pixel_keep & se.slice_keep.view(N, 1, 1, 1)).double())
    assert torch.equal(se.stats[:, 0] - se.stats[:, 2], se.pixel_keep.flatten(1).sum(1).double())
    assert torch.equal(share[good], (1 - se.stats[:, 2] / se.stats[:, 0])[good])


def test_thresholds_are_taken_from_the_constructor():
    from nesvor_amd.structural import StructuralExclusion

    sim, y, mask, gain, _ = _synthetic(1, PERMUTED[1])
    strict = StructuralExclusion(local_ssim=0.9, global_ncc=0.99).update(sim, y, mask, gain)
    loose = StructuralExclusion(local_ssim=0.0, global_ncc=-1.0).update(sim, y, mask, gain)
    assert torch.equal(strict.ncc, loose.ncc) and torch.equal(strict.ssim, loose.ssim)
    assert int(strict.pixel_keep.sum()) < int(loose.pixel_keep.sum())
    assert int(strict.slice_keep.sum()) < int(loose.slice_keep.sum()) == N - 1  # all but the empty slice
    assert torch.equal(strict.pixel_keep, mask & (strict.ssim >= 0.9))


def test_a_flat_slice_has_no_correlation():
    from nesvor_amd.structural import StructuralExclusion

    sim, y, mask, gain, _ = _synthetic(2, ())
    y = y.clone()
    y[7] = 0.6  # flat: varI = 0
    sim = sim.clone()
    sim[9] = 0.4  # its simulation flat: varJ = 0
    se = StructuralExclusion().update(sim, y, mask, gain)
    assert float(se.ncc[7]) == 0.0 and float(se.ncc[9]) == 0.0
    assert not bool(se.slice_keep[7]) and not bool(se.slice_keep[9])
    assert bool(torch.isfinite(se.ncc).all()) and bool(torch.isfinite(se.ssim).all())
    assert float(se.ncc[8]) >= 0.5


def test_composed_is_forced_by_the_switch(monkeypatch):
    from nesvor_amd import structural

    sim, y, mask, gain, _ = _synthetic(3, ())
    calls = []
    inner = structural.ssim_composed
    monkeypatch.setattr(structural, "ssim_composed", lambda *a: calls.append(1) or inner(*a))
    monkeypatch.setenv("NESVOR_STRUCTURAL", "composed")
    se = structural.StructuralExclusion().update(sim, y, mask, gain)
    assert len(calls) == 1 and not structural._fused(sim)
    for t in (se.ssim, se.stats, se.ncc, se.pixel_keep, se.slice_keep):
        assert isinstance(t, torch.Tensor)
    monkeypatch.delenv("NESVOR_STRUCTURAL")
    assert not structural._fused(sim)  # host tensors take the expression anyway


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline's routing
# ---------------------------------------------------------------------------------------------------------------------
def _recording(monkeypatch, svr):
    """A ``StructuralExclusion`` that records its weights after every update, and ``svr.RobustStatistics`` replaced by one that
    records the weights and scales it hands out."""
    from nesvor_amd.robust import RobustStatistics
    from nesvor_amd.structural import StructuralExclusion

    seen = {"structural": [], "scales_in": [], "robust": [], "scales": []}

    class Structural(StructuralExclusion):
        def update(self, sim, y, mask, scale=None):
            super().update(sim, y, mask, scale)
            seen["structural"].append(self.weights())
            seen["scales_in"].append(scale)
            return self

    class Robust(RobustStatistics):
        def weights(self):
            seen["robust"].append(super().weights())
            return seen["robust"][-1]

        def scaled(self, y):
            seen["scales"].append(self.scale)
            return super().scaled(y)

    monkeypatch.setattr(svr, "RobustStatistics", Robust)
    return Structural, seen


def test_structural_none_is_todays_pipeline(monkeypatch):
    svr, images, start, calls = _dense_pipeline(monkeypatch)
    out = {}
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=4, structural=None, structural_out=out)
    assert len(calls) == 1 and calls[0]["p"] is None and calls[0]["slices"] is images and calls[0]["volume"] is start
    assert calls[0]["n_iter"] == 4 and out == {}
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=11, robust_rounds=3, structural=None, structural_out=out)
    assert [c["n_iter"] for c in calls] == [3, 3, 5] and out == {}
    plain = [c["p"] for c in calls]
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=11, robust_rounds=3)
    assert all(torch.equal(c["p"], p) for c, p in zip(calls, plain))


def test_structural_rounds_split_the_steps_and_pass_their_weights(monkeypatch):
    svr, images, start, calls = _dense_pipeline(monkeypatch)
    Structural, seen = _recording(monkeypatch, svr)
    out, robust_out = {}, {}
    se = Structural()
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=11, robust_rounds=0, robust_out=robust_out, structural=se,
                           structural_out=out)
    assert [c["n_iter"] for c in calls] == [3, 3, 5] and calls[0]["volume"] is start
    assert len(seen["structural"]) == 3 and not seen["robust"] and robust_out == {}
    for c, weights, scale in zip(calls, seen["structural"], seen["scales_in"]):
        assert scale is None and c["slices"] is images
        assert torch.equal(c["p"], weights) and bool(((c["p"] == 0) | (c["p"] == 1)).all()) and c["p"].dtype == images.dtype
    assert set(out) == {"ncc", "slice_keep", "pixel_share", "keep"}
    assert out["ncc"].shape == out["slice_keep"].shape == out["pixel_share"].shape == (6,) and out["keep"].tolist() == list(range(6))
    assert torch.equal(out["ncc"], se.ncc) and torch.equal(out["pixel_share"], se.pixel_share())


def test_both_switches_multiply_the_weights_and_scale_the_slices(monkeypatch):
    svr, images, start, calls = _dense_pipeline(monkeypatch)
    Structural, seen = _recording(monkeypatch, svr)
    out, robust_out = {}, {}
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=9, robust_rounds=2, robust_out=robust_out, structural=Structural(),
                           structural_out=out)
    assert [c["n_iter"] for c in calls] == [4, 5]
    assert len(seen["structural"]) == len(seen["robust"]) == len(seen["scales"]) == 2
    for c, sw, rw, scale, scale_in in zip(calls, seen["structural"], seen["robust"], seen["scales"], seen["scales_in"]):
        assert torch.equal(c["p"], rw * sw) and bool(((sw == 0) | (sw == 1)).all())
        assert scale_in is scale and torch.equal(c["slices"], scale.view(-1, 1, 1, 1) * images)
    assert set(robust_out) == {"slice_weight", "scale", "keep"} and torch.equal(robust_out["scale"], seen["scales"][-1])
    assert set(out) == {"ncc", "slice_keep", "pixel_share", "keep"}


def test_more_structural_rounds_than_steps_are_cut(monkeypatch):
    from nesvor_amd.structural import StructuralExclusion

    svr, images, start, calls = _dense_pipeline(monkeypatch)
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=2, structural=StructuralExclusion())
    assert [c["n_iter"] for c in calls] == [1, 1]
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=0, structural=StructuralExclusion())
    assert [c["n_iter"] for c in calls] == [0]
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=2, robust_rounds=5, structural=StructuralExclusion())
    assert [c["n_iter"] for c in calls] == [1, 1]
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=8, structural=StructuralExclusion(rounds=4))
    assert [c["n_iter"] for c in calls] == [2, 2, 2, 2]


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_parser_has_the_structural_flags_and_keeps_the_other_defaults():
    from nesvor_amd.cli import build_parser

    p = build_parser()
    base = ["svr", "--input-stacks", "a.nii.gz", "b.nii.gz", "--output-volume", "v.nii.gz"]
    a = p.parse_args(base)
    assert a.structural_exclusion is False and a.local_ssim_threshold == 0.4 and a.global_ncc_threshold == 0.5
    b = p.parse_args(base + ["--structural-exclusion", "--local-ssim-threshold", "0.3", "--global-ncc-threshold", "0.6"])
    assert b.structural_exclusion is True and b.local_ssim_threshold == 0.3 and b.global_ncc_threshold == 0.6
    new = {"structural_exclusion", "local_ssim_threshold", "global_ncc_threshold"}
    va, vb = vars(a), vars(b)
    assert new <= set(va) and {k: v for k, v in va.items() if k not in new} == {k: v for k, v in vb.items() if k not in new}
    assert a.outlier_rejection is False and a.robust_rounds == 3 and a.slice_weights is None
    assert a.n_iter_srr == 30 and a.srr_beta == 0.02 and a.srr_delta == 0.1 and a.registration == "svr"
    assert a.simulated_slices is None and a.output_resolution == 0.8 and a.output_intensity_mean == 700.0
    for command in ("reconstruct", "register"):  # svr only
        with pytest.raises(SystemExit):
            p.parse_args([command, "--input-stacks", "a.nii.gz", "--output-volume", "v.nii.gz", "--output-slices", "s",
                          "--structural-exclusion"])


def test_slice_weights_needs_one_of_the_two_switches(monkeypatch):
    from argparse import Namespace

    from nesvor_amd import image_io
    from nesvor_amd.svr import svr_command

    class Reached(Exception):
        pass

    def load_slices(*a, **k):
        raise Reached()

    monkeypatch.setattr(image_io, "load_slices", load_slices)
    args = dict(input_slices="nowhere", input_stacks=None, stack_masks=None, thicknesses=None, device=torch.device("cpu"),
                outlier_rejection=False, robust_rounds=3, slice_weights="w.json", local_ssim_threshold=0.4, global_ncc_threshold=0.5)
    with pytest.raises(SystemExit, match="--slice-weights needs --outlier-rejection: without it no slice weights are estimated"):
        svr_command(Namespace(structural_exclusion=False, **args))
    with pytest.raises(Reached):  # accepted: the command goes on to load the slices
        svr_command(Namespace(structural_exclusion=True, **args))
