"""Slice bias fields of the classical reconstruction (nesvor_amd/slice_bias.py) on host tensors in fp64 / fp32 - the composed
path, which is also the yardstick of tests/test_gpu_slice_bias.py -, its routing through ``reconstruct_volume`` and the ``svr``
command's flags."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_robust import _dense_pipeline


# ---------------------------------------------------------------------------------------------------------------------
# the window
# ---------------------------------------------------------------------------------------------------------------------
def test_taps_and_radius():
    from nesvor_amd.slice_bias import gaussian_taps, window_radius

    assert [window_radius(s) for s in (0.1, 0.3, 1.0 / 3.0, 0.5, 1.5, 3.0, 8.0, 16.0, 16.1)] == [1, 1, 1, 2, 5, 9, 24, 48, 49]
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            window_radius(bad)
    g = gaussian_taps(1.5)
    assert g.shape == (11,) and g.dtype == torch.float64 and float(g.sum()) == pytest.approx(1.0, abs=1e-15)
    t = torch.arange(11, dtype=torch.float64)
    expected = torch.exp(-(t - 5) ** 2 / (2 * 1.5 ** 2))
    assert torch.allclose(g, expected / expected.sum(), rtol=0, atol=1e-15)
    assert torch.equal(g, g.flip(0)) and gaussian_taps(8.0, torch.float32).shape == (49,)


@pytest.mark.parametrize("sigma_px", [0.5, 3.0])
def test_the_window_is_the_zero_padded_separable_gaussian(sigma_px):
    """Against a plain numpy double loop on (2,7,9); with sigma_px = 3 the radius, 9, is larger than the slice."""
    from nesvor_amd.slice_bias import _window, gaussian_taps, window_radius

    g = torch.Generator().manual_seed(3)
    a = torch.rand(2, 7, 9, generator=g, dtype=torch.float64)
    radius = window_radius(sigma_px)
    taps = gaussian_taps(sigma_px).tolist()
    assert len(taps) == 2 * radius + 1
    got = _window(a, taps).numpy()
    src = a.numpy()
    rows = np.zeros_like(src)
    for k in range(2):
        for i in range(7):
            for j in range(9):
                for t in range(2 * radius + 1):
                    jj = j + t - radius
                    if 0 <= jj < 9:
                        rows[k, i, j] += taps[t] * src[k, i, jj]
    want = np.zeros_like(src)
    for k in range(2):
        for i in range(7):
            for j in range(9):
                for t in range(2 * radius + 1):
                    ii = i + t - radius
                    if 0 <= ii < 7:
                        want[k, i, j] += taps[t] * rows[k, ii, j]
    assert float(np.abs(got - want).max()) <= 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# recovery with sim held true
# ---------------------------------------------------------------------------------------------------------------------
def _fixture(dtype=torch.float64):
    """(5,40,44): sim a bicubic-upsampled random field in [0.1, 0.9], a disc-shaped mask (radius 95 % of the half height),
    per-slice true log-fields c1 x + c2 y + c3 x y with |c| <= 0.3 and zero mean over the mask, noise 0.02, gains in
    [0.8, 1.2] that are passed as ``scale``."""
    n, h, w = 5, 40, 44
    g = torch.Generator().manual_seed(7)
    coarse = torch.rand(n, 1, 6, 6, generator=g, dtype=torch.float64)
    sim = (0.1 + 0.8 * F.interpolate(coarse, size=(h, w), mode="bicubic", align_corners=True)).clamp(0.1, 0.9)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, h, dtype=torch.float64), torch.linspace(-1, 1, w, dtype=torch.float64), indexing="ij")
    mask = ((yy * (h - 1) / 2) ** 2 + (xx * (w - 1) / 2) ** 2 <= (0.95 * (h - 1) / 2) ** 2).expand(n, 1, h, w).contiguous()
    c = 0.6 * torch.rand(n, 3, generator=g, dtype=torch.float64) - 0.3
    truth = c[:, 0].view(n, 1, 1, 1) * xx + c[:, 1].view(n, 1, 1, 1) * yy + c[:, 2].view(n, 1, 1, 1) * (xx * yy)
    truth = truth - (truth * mask).flatten(1).sum(1).view(n, 1, 1, 1) / mask.flatten(1).sum(1).view(n, 1, 1, 1)
    gain = 0.8 + 0.4 * torch.rand(n, generator=g, dtype=torch.float64)
    y = (sim * torch.exp(truth) + 0.02 * torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)) / gain.view(n, 1, 1, 1)
    return tuple(t.to(dtype) if t.is_floating_point() else t for t in (sim, y, mask, gain, truth))


def test_three_rounds_recover_smooth_fields():
    """With sigma_px = 8 and three rounds the error's std over the mask is at most 0.2 x the true fields' std.  Measured here in
    fp64: DESIGN.md, "Slice bias fields"."""
    from nesvor_amd.slice_bias import SliceBias

    sim, y, mask, gain, truth = _fixture()
    sb = SliceBias(sigma_mm=12.0)
    for _ in range(3):
        sb.update(sim, y, mask, gain, None, 1.5)  # sigma_px = 12 / 1.5 = 8
    err = (sb.b - truth)[mask]
    ratio = float(err.std()) / float(truth[mask].std())
    print(f"error std {float(err.std()):.4f} of {float(truth[mask].std()):.4f}: ratio {ratio:.4f}")
    assert ratio <= 0.2
    assert torch.allclose(sb.corrected(y), y * torch.exp(-sb.b))
    assert sb.stats.shape == (5, 5) and sb.stats.dtype == torch.float64
    e = mask & (y > 0.05) & (sim > 0.05)
    assert torch.equal(sb.stats[:, 0], e.flatten(1).sum(1).double()) and int(e.sum()) >= int(mask.sum()) - 5


# ---------------------------------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------------------------------
def test_updated_slices_are_centred_and_light_slices_keep_their_field():
    from nesvor_amd.slice_bias import MIN_WEIGHT, SliceBias, eligible

    sim, y, mask, gain, _ = _fixture()
    mask = mask.clone()
    mask[1] = False
    mask[1, 0, 20, 10:40] = True  # 30 eligible pixels: below MIN_WEIGHT
    mask[3] = False               # none
    sb = SliceBias()
    sb.b = 0.01 * torch.arange(sim.numel(), dtype=torch.float64).view_as(sim) / sim.numel()
    before = sb.b.clone()
    sb.update(sim, y, mask, gain, None, 1.5)
    assert sb.stats[1, 1] == 30.0 and sb.stats[3, 1] == 0.0 and MIN_WEIGHT == 64.0
    assert torch.equal(sb.b[1], before[1]) and torch.equal(sb.b[3], before[3])
    e = eligible(sim, y, mask)
    for k in (0, 2, 4):
        assert not torch.equal(sb.b[k], before[k])
        u = e[k].double()
        assert abs(float((u * sb.b[k]).sum()) / float(u.sum())) <= 1e-12
    # weighted: the mean that is removed is the weighted one
    weight = torch.rand(sim.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    sb.update(sim, y, mask, gain, weight, 1.5)
    for k in (0, 2, 4):
        u = e[k].double() * weight[k]
        assert abs(float((u * sb.b[k]).sum()) / float(u.sum())) <= 1e-12


def test_ineligible_pixels_contribute_nothing():
    from nesvor_amd.slice_bias import field_composed

    sim, y, mask, gain, _ = _fixture()
    y, sim = y.clone(), sim.clone()
    y[:, :, 18:22, 5:9] = 0.04     # below the floor
    sim[:, :, 30:33, 20:30] = 0.03
    b = torch.zeros_like(sim)
    weight = torch.rand(sim.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    ref_b, ref_s = field_composed(sim, y, mask, gain, weight, b, 8.0)
    assert float(ref_s[:, 0].max()) < float(mask[0].sum())
    y2, sim2, w2 = y.clone(), sim.clone(), weight.clone()
    y2[:, :, 18:22, 5:9] = 0.0      # (log of 0 there, were it taken)
    sim2[:, :, 30:33, 20:30] = -1.0
    y2[~mask] = 55.0
    w2[~mask] = 1e6
    w2[:, :, 18:22, 5:9] = 1e6
    got_b, got_s = field_composed(sim2, y2, mask, gain, w2, b, 8.0)
    assert torch.equal(got_b, ref_b) and torch.equal(got_s, ref_s)


def test_no_weight_is_ones_and_a_byte_mask_is_a_bool_mask():
    from nesvor_amd.slice_bias import field_composed, field_update

    sim, y, mask, gain, _ = _fixture()
    b = 0.05 * torch.sin(torch.arange(sim.numel(), dtype=torch.float64)).view_as(sim)
    ref = field_composed(sim, y, mask, gain, None, b, 3.0)
    for other in (field_composed(sim, y, mask, gain, torch.ones_like(sim), b, 3.0),
                  field_composed(sim, y, mask.to(torch.uint8), gain, None, b, 3.0),
                  field_update(sim, y, mask, gain, None, b, 3.0),  # host tensors take the expression
                  field_composed(sim[:, 0], y[:, 0], mask[:, 0], gain, None, b[:, 0], 3.0)):
        assert torch.equal(other[0].view_as(ref[0]), ref[0]) and torch.equal(other[1], ref[1])
    nomask = field_composed(sim, y, None, gain, None, b, 3.0)
    allmask = field_composed(sim, y, torch.ones_like(mask), gain, None, b, 3.0)
    assert torch.equal(nomask[0], allmask[0]) and torch.equal(nomask[1], allmask[1])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_den_min_and_the_clamp_on_hand_made_slices(dtype):
    from nesvor_amd.slice_bias import CLAMP, field_composed

    # one eligible pixel in a 1 x 31 slice, sigma_px 1 (R = 3): den is the tap of the distance, 0 beyond the radius
    sim = torch.full((1, 1, 1, 31), 0.5, dtype=dtype)
    y = torch.full((1, 1, 1, 31), 0.01, dtype=dtype)
    y[..., 15] = 0.5 * math.exp(0.2)
    one = torch.ones(1, dtype=dtype)
    b = torch.zeros_like(sim)
    b_new, stats = field_composed(sim, y, None, one, None, b, 1.0)
    # the window's value at distance d is g[3] g[3 + d] (the row pass on a single row keeps g[3] of it): 0.159, 0.0967, 0.0216, 0.0018
    near, far = b_new[0, 0, 0, 12:19], torch.cat([b_new[0, 0, 0, :12], b_new[0, 0, 0, 19:]])
    assert torch.allclose(near, torch.full_like(near, 0.2), rtol=0, atol=1e-6) and bool((far == 0).all())
    assert stats[0].tolist()[:2] == [1.0, 1.0] and float(stats[0, 3]) == pytest.approx(0.2, abs=1e-6)
    # a weight of 0.3 puts den at distance 3 to 0.3 x 0.0018 < DEN_MIN: that pixel gets no update any more; distance 2 still does
    b_new, _ = field_composed(sim, y, None, one, torch.full_like(sim, 0.3), b, 1.0)
    assert float(b_new[0, 0, 0, 12]) == 0.0 and float(b_new[0, 0, 0, 18]) == 0.0
    assert float(b_new[0, 0, 0, 13]) == pytest.approx(0.2, abs=1e-6) and float(b_new[0, 0, 0, 17]) == pytest.approx(0.2, abs=1e-6)
    # the clamp: ratios of 5 and 1 / 5 count as 2 and 1 / 2
    y = torch.full((1, 1, 1, 31), 0.01, dtype=dtype)
    y[..., 4], y[..., 26] = 2.5, 0.1
    b_new, stats = field_composed(sim, y, None, one, None, b, 1.0)
    assert float(b_new[0, 0, 0, 4]) == pytest.approx(CLAMP, abs=1e-6) and float(b_new[0, 0, 0, 26]) == pytest.approx(-CLAMP, abs=1e-6)
    assert float(stats[0, 3]) == pytest.approx(0.0, abs=1e-6) and float(stats[0, 4]) == pytest.approx(2 * CLAMP * CLAMP, abs=1e-6)
    # an incoming field is divided out before the ratio is taken
    y[..., 4] = 0.5 * math.exp(0.5)
    b = torch.full_like(sim, 0.4)
    b_new, _ = field_composed(sim, y, None, one, None, b, 1.0)
    assert float(b_new[0, 0, 0, 4]) == pytest.approx(0.5, abs=1e-6)


def test_composed_is_forced_by_the_switch_and_by_host_tensors(monkeypatch):
    from nesvor_amd import slice_bias

    sim, y, mask, gain, _ = _fixture(torch.float32)
    calls = []
    inner = slice_bias.field_composed
    monkeypatch.setattr(slice_bias, "field_composed", lambda *a: calls.append(1) or inner(*a))
    monkeypatch.setenv("NESVOR_SLICE_BIAS", "composed")
    slice_bias.SliceBias().update(sim, y, mask, None, None, 1.5)
    monkeypatch.delenv("NESVOR_SLICE_BIAS")
    sb = slice_bias.SliceBias().update(sim, y, mask, None, None, 1.5)
    assert len(calls) == 2 and sb.b.dtype == torch.float32 and sb.stats.dtype == torch.float64
    assert not slice_bias._fused(sim, 8.0)


# ---------------------------------------------------------------------------------------------------------------------
# the pipeline's routing
# ---------------------------------------------------------------------------------------------------------------------
def test_slice_bias_none_is_todays_pipeline(monkeypatch):
    svr, images, start, calls = _dense_pipeline(monkeypatch)
    out = {}
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=4, slice_bias=None, slice_bias_out=out)
    assert len(calls) == 1 and calls[0]["p"] is None and calls[0]["slices"] is images and calls[0]["volume"] is start
    assert calls[0]["n_iter"] == 4 and out == {}


def test_slice_bias_rounds_split_the_steps_and_descend_on_the_corrected_slices(monkeypatch):
    from nesvor_amd.slice_bias import SliceBias

    svr, images, start, calls = _dense_pipeline(monkeypatch)
    seen = []

    class Recording(SliceBias):
        def update(self, sim, y, mask, scale, weight, res_s):
            super().update(sim, y, mask, scale, weight, res_s)
            seen.append((y, scale, weight, res_s, self.b.clone()))
            return self

    out, robust_out = {}, {}
    sb = Recording(sigma_mm=3.0)
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=11, robust_out=robust_out, slice_bias=sb, slice_bias_out=out)
    assert [c["n_iter"] for c in calls] == [3, 3, 5] and calls[0]["volume"] is start and robust_out == {}
    assert len(seen) == 3
    for c, (y, scale, weight, res_s, b) in zip(calls, seen):
        assert y is images and scale is None and weight is None and res_s == 1.5 and c["p"] is None
        assert torch.equal(c["slices"], images * torch.exp(-b))
    assert set(out) == {"b", "stats", "bias_rms", "eligible", "keep"} and out["b"] is sb.b and out["keep"].tolist() == list(range(6))
    assert out["stats"].shape == (6, 5) and out["bias_rms"].shape == (6,) and out["bias_rms"].dtype == torch.float64
    assert out["eligible"].dtype == torch.bool and out["eligible"].shape == images.shape
    del calls[:], seen[:]
    # with the robust statistics: their scales and weights reach the update, and the descent takes the scaled corrected slices
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=9, robust_rounds=2, robust_out=robust_out, slice_bias=Recording(3.0))
    assert [c["n_iter"] for c in calls] == [4, 5] and set(robust_out) == {"slice_weight", "scale", "keep"}
    for c, (y, scale, weight, res_s, b) in zip(calls, seen):
        assert y is images and scale.shape == (6,) and torch.equal(weight, c["p"])
    assert torch.equal(calls[-1]["slices"], robust_out["scale"].view(-1, 1, 1, 1) * (images * torch.exp(-seen[-1][4])))
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=2, slice_bias=SliceBias())
    assert [c["n_iter"] for c in calls] == [1, 1]
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=8, slice_bias=SliceBias(rounds=4))
    assert [c["n_iter"] for c in calls] == [2, 2, 2, 2]
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=8, robust_rounds=2, slice_bias=SliceBias(rounds=4))
    assert [c["n_iter"] for c in calls] == [4, 4]


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def test_parser_has_the_slice_bias_flags_and_keeps_the_other_defaults():
    from nesvor_amd.cli import build_parser

    p = build_parser()
    base = ["svr", "--input-stacks", "a.nii.gz", "b.nii.gz", "--output-volume", "v.nii.gz"]
    a = p.parse_args(base)
    assert a.slice_bias_fields is False and a.bias_sigma == 12.0 and a.output_corrected_slices is None
    b = p.parse_args(base + ["--slice-bias-fields", "--bias-sigma", "9", "--output-corrected-slices", "c"])
    assert b.slice_bias_fields is True and b.bias_sigma == 9.0 and b.output_corrected_slices == "c"
    new = {"slice_bias_fields", "bias_sigma", "output_corrected_slices"}
    va, vb = vars(a), vars(b)
    assert new <= set(va) and {k: v for k, v in va.items() if k not in new} == {k: v for k, v in vb.items() if k not in new}
    assert a.outlier_rejection is False and a.structural_exclusion is False and a.robust_rounds == 3 and a.slice_weights is None
    assert a.bias_field_correction is False  # (the stack-level correction keeps its own switch)
    for command in ("reconstruct", "register"):  # svr only
        with pytest.raises(SystemExit):
            p.parse_args([command, "--input-stacks", "a.nii.gz", "--output-volume", "v.nii.gz", "--output-slices", "s",
                          "--slice-bias-fields"])


def _command(monkeypatch, tmp_path, **flags):
    """``svr_command`` on six host slices with ``reconstruct_volume`` replaced by a recorder."""
    from argparse import Namespace

    from nesvor_amd import image_io, svr
    from nesvor_amd.image import Slice, Volume

    g = torch.Generator().manual_seed(1)
    loaded = [Slice(torch.rand(1, 8, 8, generator=g) + 0.1, None, None, 1.5, 1.5, 3.0) for _ in range(6)]
    monkeypatch.setattr(image_io, "load_slices", lambda *a, **k: loaded)
    # (grouping and framing go through the poses, whose conversions are device operators: the images as they are, no poses)
    images = torch.stack([s.image for s in loaded])
    monkeypatch.setattr(svr, "_group", lambda slices, res_s: ([images], [images > 0], [None], 1.5))
    monkeypatch.setattr(svr, "_frame", lambda slices, mask, poses, res_s: (images, images > 0, [None] * 6))
    made = []

    def reconstruct(*a, **k):
        made.append(k)
        if "slice_bias_out" in k:
            k["slice_bias_out"].update(b=torch.full((6, 1, 8, 8), 0.1), stats=torch.full((6, 5), 64.0, dtype=torch.float64),
                                       bias_rms=torch.full((6,), 0.1, dtype=torch.float64), keep=torch.arange(6))
        return Volume(torch.ones(2, 2, 2), None, None, 1.0, 1.0, 1.0)

    monkeypatch.setattr(svr, "reconstruct_volume", reconstruct)
    args = dict(input_slices="somewhere", input_stacks=None, stack_masks=None, thicknesses=None, device=torch.device("cpu"),
                outlier_rejection=False, structural_exclusion=False, robust_rounds=3, slice_weights=None, local_ssim_threshold=0.4,
                global_ncc_threshold=0.5, output_resolution=1.0, n_iter_srr=3, srr_beta=0.02, srr_delta=0.1, simulated_slices=None,
                slice_bias_fields=False, bias_sigma=12.0, output_corrected_slices=None)
    args.update(flags)
    return svr.svr_command(Namespace(**args)), made


def test_the_command_hands_a_slice_bias_to_the_reconstruction(monkeypatch, tmp_path):
    import json

    from nesvor_amd.slice_bias import SliceBias

    weights = str(tmp_path / "w.json")
    data, made = _command(monkeypatch, tmp_path, slice_bias_fields=True, bias_sigma=9.0, slice_weights=weights,
                          output_corrected_slices=str(tmp_path / "c"))
    assert len(made) == 1 and isinstance(made[0]["slice_bias"], SliceBias)
    assert made[0]["slice_bias"].sigma_mm == 9.0 and made[0]["slice_bias"].min_intensity == 0.05 and made[0]["slice_bias"].rounds == 3
    assert made[0]["robust_rounds"] == 0 and made[0]["structural"] is None
    rows = json.load(open(weights))  # --slice-weights is accepted with the new flag alone
    assert len(rows) == 6 and all(set(r) == {"stack", "slice", "bias_rms"} and r["bias_rms"] == pytest.approx(0.1) for r in rows)
    assert len(data["output_corrected_slices"]) == 6
    first = data["output_corrected_slices"][0]
    assert first.image.shape == (1, 8, 8) and torch.allclose(first.image, data["output_slices"][0].image * math.exp(-0.1))
    # with the other two switches
    _, made = _command(monkeypatch, tmp_path, slice_bias_fields=True, outlier_rejection=True, structural_exclusion=True, robust_rounds=2)
    assert made[0]["robust_rounds"] == 2 and made[0]["structural"].rounds == 2 and isinstance(made[0]["slice_bias"], SliceBias)


def test_without_the_flag_the_command_calls_as_before(monkeypatch, tmp_path):
    data, made = _command(monkeypatch, tmp_path)
    assert len(made) == 1 and made[0] == {} and "output_corrected_slices" not in data
    _, made = _command(monkeypatch, tmp_path, outlier_rejection=True)
    assert set(made[0]) == {"robust_rounds", "robust_out"}
    _, made = _command(monkeypatch, tmp_path, structural_exclusion=True)
    assert set(made[0]) == {"robust_rounds", "robust_out", "structural", "structural_out"}
    with pytest.raises(SystemExit, match="--output-corrected-slices needs --slice-bias-fields"):
        _command(monkeypatch, tmp_path, output_corrected_slices="c")
    with pytest.raises(SystemExit, match="--slice-weights needs --outlier-rejection"):
        _command(monkeypatch, tmp_path, slice_weights="w.json")
    with pytest.raises(SystemExit, match="--bias-sigma must be positive"):
        _command(monkeypatch, tmp_path, slice_bias_fields=True, bias_sigma=0.0)
