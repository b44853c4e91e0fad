"""CPU: the stack denoising definitions (nesvor_amd/denoise.py) on the composed path with host tensors - the properties of the
non-local means rule in fp64, the noise estimate, the quality on the phantom, the command line and the operator's registration."""
import json
import logging
import sys

import pytest
import torch

import denoise_cases as C
from nesvor_amd.image import Stack


def _slices(n=3, h=13, w=11, seed=0, frac=0.7):
    """Structured slices in [0, 1] (a ramp, a step, noise of 0.05) in fp64 with a random mask."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, h, dtype=torch.float64), torch.linspace(0, 1, w, dtype=torch.float64), indexing="ij")
    y = (0.3 * xx + 0.3 * (yy > 0.5) + 0.2).expand(n, 1, h, w) + 0.05 * torch.randn(n, 1, h, w, generator=g, dtype=torch.float64)
    mask = torch.rand(n, 1, h, w, generator=g) < frac
    return y.clamp(0, 1).contiguous(), mask


def _sigma(n, value=0.05):
    return torch.full((n,), value, dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the definition
# ---------------------------------------------------------------------------------------------------------------------
def test_a_constant_slice_comes_back_unchanged():
    """V / W with V the sum of K copies of a v and W = K: each add rounds once, so |out - v| <= K eps v with K <= 49."""
    from nesvor_amd.denoise import nlm_composed

    y = torch.full((2, 1, 9, 10), 0.3, dtype=torch.float64)
    out, stats = nlm_composed(y, None, _sigma(2), 1, 3, 1.0)
    assert float((out - y).abs().max()) <= 49 * 2.0 ** -52 * 0.3
    assert torch.equal(stats[:, 0], torch.full((2,), 90.0, dtype=torch.float64)) and float(stats[:, 1].max()) < 1e-28
    half = torch.full((1, 1, 7, 7), 0.5, dtype=torch.float64)  # every sum exact: bit for bit
    assert torch.equal(nlm_composed(half, None, _sigma(1), 2, 2, 0.7)[0], half)


def test_invalid_pixels_and_slices_without_a_sigma_are_copied():
    from nesvor_amd.denoise import nlm_composed

    y, mask = _slices(n=5)
    y[0, 0, 2, 3] = float("nan")
    mask[0, 0, 2, 3] = False  # an invalid NaN: kept, and reaching no one
    sigma = torch.tensor([0.05, 0.0, -1.0, float("inf"), float("nan")], dtype=torch.float64)
    out, stats = nlm_composed(y, mask, sigma, 1, 3, 1.0)
    assert torch.equal(out[~mask].view(torch.int64), y[~mask].view(torch.int64))  # (as bits: the NaN too)
    assert torch.equal(out[1:], y[1:])
    assert bool(torch.isfinite(out[0][mask[0]]).all()) and not torch.equal(out[0], y[0])
    assert torch.equal(stats[:, 0], mask.flatten(1).sum(1).double()) and bool((stats[1:, 1] == 0).all()) and float(stats[0, 1]) > 0


def test_a_pixel_without_a_candidate_is_copied():
    from nesvor_amd.denoise import nlm_composed

    one = torch.tensor([[[[0.37]]]], dtype=torch.float64)
    out, stats = nlm_composed(one, None, _sigma(1), 1, 3, 1.0)
    assert torch.equal(out, one) and stats.tolist() == [[1.0, 0.0]]
    y, _ = _slices(n=1)
    mask = torch.zeros_like(y, dtype=torch.bool)
    mask[0, 0, 4, 5] = True
    out, stats = nlm_composed(y, mask, _sigma(1), 2, 5, 1.0)
    assert torch.equal(out, y) and stats.tolist() == [[1.0, 0.0]]
    # two valid pixels further apart than the search radius: no candidate either
    mask[0, 0, 4, 0] = True
    assert torch.equal(nlm_composed(y, mask, _sigma(1), 1, 3, 1.0)[0], y)
    assert not torch.equal(nlm_composed(y, mask, _sigma(1), 1, 5, 1.0)[0], y)


def test_an_invalid_value_never_influences_a_valid_pixel():
    from nesvor_amd.denoise import nlm_composed

    y, mask = _slices()
    other = torch.where(mask, y, torch.full_like(y, 1e6))
    other[0, 0][~mask[0, 0]] = float("nan")
    for P, S in ((1, 3), (2, 4)):
        a, sa = nlm_composed(y, mask, _sigma(3), P, S, 1.0)
        b, sb = nlm_composed(other, mask, _sigma(3), P, S, 1.0)
        assert torch.equal(a[mask], b[mask]) and torch.equal(sa, sb)


def test_every_output_lies_in_the_range_of_its_search_window():
    """A weighted mean with non-negative weights; V and W each carry at most K = (2 S + 1)^2 roundings: a margin of K eps."""
    from nesvor_amd.denoise import nlm_composed
    import torch.nn.functional as F

    y, mask = _slices(h=17, w=15)
    S = 3
    out, _ = nlm_composed(y, mask, _sigma(3, 0.08), 1, S, 1.0)
    big = 1e9
    lo = -F.max_pool2d(-torch.where(mask, y, torch.full_like(y, big)), 2 * S + 1, 1, S)  # (the padding is -inf for a max pool)
    hi = F.max_pool2d(torch.where(mask, y, torch.full_like(y, -big)), 2 * S + 1, 1, S)
    margin = 49 * 2.0 ** -52
    assert bool((out[mask] >= lo[mask] - margin).all()) and bool((out[mask] <= hi[mask] + margin).all())
    assert float((out - y).abs().max()) > 1e-3


def test_flips_and_the_transpose_commute_with_the_filter():
    """The rule names no direction; the sums are added in another order, so equality holds to a few roundings of values <= 1."""
    from nesvor_amd.denoise import nlm_composed

    y, mask = _slices()
    out, stats = nlm_composed(y, mask, _sigma(3), 1, 3, 0.7)
    for f in (lambda t: t.flip(-1), lambda t: t.flip(-2), lambda t: t.transpose(-1, -2)):
        o2, s2 = nlm_composed(f(y).contiguous(), f(mask).contiguous(), _sigma(3), 1, 3, 0.7)
        assert float((o2 - f(out)).abs().max()) <= 1e-13 and float((s2 - stats).abs().max()) <= 1e-13


def test_stats_are_the_count_and_the_sum_recomputed_from_out():
    from nesvor_amd.denoise import method_noise_rms, nlm_composed

    y, mask = _slices()
    out, stats = nlm_composed(y, mask, _sigma(3), 1, 3, 1.0)
    assert stats.shape == (3, 2) and stats.dtype == torch.float64
    for k in range(3):
        d = (out[k] - y[k])[mask[k]]
        assert float(stats[k, 0]) == int(mask[k].sum()) and float(stats[k, 1]) == pytest.approx(float((d * d).sum()), rel=1e-12)
    assert method_noise_rms(stats) == pytest.approx(float(((out - y)[mask] ** 2).mean().sqrt()), rel=1e-12)
    o32, s32 = nlm_composed(y.float(), mask, _sigma(3).float(), 1, 3, 1.0)  # the dtype of y is kept
    assert o32.dtype == torch.float32 and s32.dtype == torch.float64 and float((o32.double() - out).abs().max()) < 1e-5
    flat, sflat = nlm_composed(y[:, 0], mask[:, 0].to(torch.uint8), _sigma(3), 1, 3, 1.0)
    assert flat.shape == (3, 13, 11) and torch.equal(flat, out[:, 0]) and torch.equal(sflat, stats)
    for bad in (dict(patch_radius=0), dict(search_radius=0), dict(strength=0.0), dict(strength=float("nan"))):
        with pytest.raises(ValueError):
            nlm_composed(y, mask, _sigma(3), **{"patch_radius": 1, "search_radius": 3, "strength": 1.0, **bad})


# ---------------------------------------------------------------------------------------------------------------------
# the noise estimate
# ---------------------------------------------------------------------------------------------------------------------
def test_estimate_noise_on_pure_noise():
    """12 x 62 x 62 = 46128 samples: the pseudo-residual is exact on a constant, the MAD scatters by well under 1 %."""
    from nesvor_amd.denoise import estimate_noise

    g = torch.Generator().manual_seed(3)
    y = 0.4 + 0.05 * torch.randn(12, 1, 64, 64, generator=g)
    sigma, n_used = estimate_noise(y, None)
    print("estimate", float(sigma), "on", n_used)
    assert n_used == 12 * 62 * 62 and sigma.ndim == 0 and sigma.dtype == torch.float32
    assert abs(float(sigma) - 0.05) <= 0.05 * 0.05
    mask = torch.ones_like(y, dtype=torch.bool)
    mask[:, :, 10, 10] = False  # an invalid pixel takes itself and its four neighbours out
    assert estimate_noise(y, mask)[1] == n_used - 12 * 5


def test_too_few_pixels_leave_the_stack_alone_with_a_warning(caplog):
    from nesvor_amd.denoise import denoise_stacks, estimate_noise

    g = torch.Generator().manual_seed(4)
    y = torch.rand(1, 1, 9, 9, generator=g)  # 7 x 7 = 49 usable pixels
    assert estimate_noise(y, None)[1] == 49
    st = Stack(y.clone())
    with caplog.at_level(logging.WARNING):
        rep = denoise_stacks([st], names=["the small one"])
    assert "the small one" in caplog.text and "49 pixels" in caplog.text and "left as it is" in caplog.text
    assert torch.equal(st.slices, y) and rep[0]["stats"] is None and rep[0]["n_used"] == 49
    assert estimate_noise(torch.rand(2, 1, 2, 9), None)[1] == 0
    rep = denoise_stacks([st], sigma=0.1)  # a given sigma needs no estimate
    assert rep[0]["stats"] is not None and not torch.equal(st.slices, y)


# ---------------------------------------------------------------------------------------------------------------------
# quality on the phantom
# ---------------------------------------------------------------------------------------------------------------------
def test_quality_on_the_phantom():
    """sigma = 0.06 with the defaults: the masked PSNR rises by at least 1 dB and the estimate lies within 0.9 .. 1.3 of the truth
    (a CPU prototype measured 24.41 -> 28.56 dB and 0.0661); at sigma = 0.03 a rise (the prototype: 30.37 -> 32.20 dB)."""
    from nesvor_amd.denoise import denoise_stacks, method_noise_rms

    for sigma, gain in ((0.06, 1.0), (0.03, 0.0)):
        clean, noisy, mask = C.phantom_stack(sigma)
        st = Stack(noisy.clone(), mask.clone())
        rep = denoise_stacks([st])[0]
        before, after = C.masked_psnr(noisy, clean, mask), C.masked_psnr(st.slices, clean, mask)
        print(f"sigma {sigma}: PSNR {before:.2f} -> {after:.2f} dB, estimate {float(rep['sigma']):.4f} on {rep['n_used']} pixels, "
              f"method noise rms {method_noise_rms(rep['stats']):.4f}")
        assert st.slices.dtype == torch.float32 and torch.equal(st.mask, mask) and not rep["fused"]
        assert torch.equal(st.slices[~mask], noisy[~mask])
        if gain > 0:
            assert after >= before + gain and 0.9 * sigma <= float(rep["sigma"]) <= 1.3 * sigma
        else:
            assert after > before


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
HEADS = {"reconstruct": ["--output-volume", "v.nii.gz"], "register": ["--output-slices", "d"], "svr": ["--output-volume", "v.nii.gz"],
         "assess": [], "correct-bias-field": ["--output-corrected-stacks", "c.nii.gz", "d.nii.gz"]}


def test_parser_has_the_denoise_flags_on_the_five_commands():
    from nesvor_amd.cli import build_parser, denoise_options

    flags = ["--denoise", "--denoise-patch-radius", "2", "--denoise-search-radius", "5", "--denoise-strength", "0.7", "--denoise-sigma", "12.5"]
    for command, extra in HEADS.items():
        base = [command, "--input-stacks", "x.nii.gz", "y.nii.gz", *extra]
        args = build_parser().parse_args(base + flags)
        assert args.denoise and denoise_options(args) == {"patch_radius": 2, "search_radius": 5, "strength": 0.7, "sigma": 12.5}
        args = build_parser().parse_args(base)
        assert not args.denoise and denoise_options(args) == {"patch_radius": 1, "search_radius": 3, "strength": 1.0, "sigma": None}
    args = build_parser().parse_args(["denoise", "--input-stacks", "a", "b", "--output-stacks", "c", "d"])
    assert denoise_options(args) == {"patch_radius": 1, "search_radius": 3, "strength": 1.0, "sigma": None}
    assert args.stack_masks is None and args.output_json is None and not hasattr(args, "denoise")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["denoise", "--input-stacks", "a"])  # --output-stacks is required
    with pytest.raises(SystemExit):
        build_parser().parse_args(["sample-volume", "--input-model", "m", "--output-volume", "v", "--denoise"])


def _files(tmp_path, sigma=0.06):
    from nesvor_amd.image_io import save_stack
    from nesvor_amd.transform import RigidTransform

    clean, noisy, mask = C.phantom_stack(sigma)
    paths, masks = [], []
    for j in range(2):
        pose = torch.eye(3, 4).repeat(6, 1, 1)  # (as matrices: the host has no kernel for the axis-angle conversion)
        pose[:, 2, 3] = 2.0 * (torch.arange(6) - 3.0)
        st = Stack(noisy[6 * j:6 * j + 6].clone(), mask[6 * j:6 * j + 6].clone(), RigidTransform(pose, trans_first=True), resolution_x=1.0,
                   resolution_y=1.0, thickness=2.0, gap=2.0)
        paths.append(str(tmp_path / f"s{j}.nii.gz"))
        masks.append(str(tmp_path / f"m{j}.nii.gz"))
        save_stack(paths[-1], st)
        save_stack(masks[-1], st, st.mask.to(st.slices.dtype))
    return paths, masks


def test_denoise_command_round_trips_stacks_and_writes_the_report(tmp_path):
    from nesvor_amd import cli
    from nesvor_amd.denoise import denoise_stacks
    from nesvor_amd.image_io import load_stack

    paths, masks = _files(tmp_path)
    out = [str(tmp_path / f"d{j}.nii.gz") for j in range(2)]
    report = str(tmp_path / "r.json")
    args = cli.build_parser().parse_args(["denoise", "--input-stacks", *paths, "--stack-masks", *masks, "--output-stacks", *out,
                                          "--output-json", report])
    args.device = torch.device("cpu")
    cli.denoise_cmd(args)
    rows = json.load(open(report))
    assert [r["input_stack"] for r in rows] == paths and [r["output_stack"] for r in rows] == out
    for p, m, o, row in zip(paths, masks, out, rows):
        src, got = load_stack(p, m), load_stack(o, m)
        want = load_stack(p, m)
        rep = denoise_stacks([want])[0]
        assert torch.equal(got.slices, want.slices) and not torch.equal(got.slices, src.slices)
        assert torch.equal(got.transformation.matrix(True), src.transformation.matrix(True)) and got.resolution_x == src.resolution_x
        assert row["denoised"] and row["path"] == "composed" and row["n_used"] == rep["n_used"] > 64
        assert row["sigma"] == pytest.approx(float(rep["sigma"])) and 0.9 * 0.06 <= row["sigma"] <= 1.3 * 0.06
        assert row["valid_pixels"] == int(src.mask.sum()) and 0.5 * row["sigma"] < row["method_noise_rms"] < 1.5 * row["sigma"]
    # a given sigma and other radii
    args = cli.build_parser().parse_args(["denoise", "--input-stacks", *paths, "--output-stacks", *out, "--denoise-sigma", "0.05",
                                          "--denoise-patch-radius", "2", "--denoise-search-radius", "2", "--denoise-strength", "0.8"])
    args.device = torch.device("cpu")
    cli.denoise_cmd(args)
    want = load_stack(paths[0])
    denoise_stacks([want], 2, 2, 0.8, sigma=0.05)
    assert torch.equal(load_stack(out[0]).slices, want.slices)


def test_length_mismatches_end_with_the_sibling_commands_messages(tmp_path):
    from nesvor_amd import cli

    paths, masks = _files(tmp_path)
    base = ["denoise", "--input-stacks", *paths]
    for extra, what in ((["--output-stacks", "a.nii.gz"], "output stacks"),
                        (["--output-stacks", "a.nii.gz", "b.nii.gz", "--stack-masks", masks[0]], "stack masks")):
        args = cli.build_parser().parse_args(base + extra)
        args.device = torch.device("cpu")
        with pytest.raises(SystemExit, match=f"The numbers of {what} and input stacks are different!"):
            cli.denoise_cmd(args)


def test_input_slices_ignores_the_flag_with_a_warning(caplog, monkeypatch):
    from nesvor_amd import cli, image_io, svr

    def stop(*a, **k):
        raise KeyboardInterrupt  # the commands are left where they would read the folder

    monkeypatch.setattr(image_io, "load_slices", stop)
    for command, run in (("reconstruct", cli.reconstruct), ("svr", svr.svr_command)):
        for extra, warned in ((["--denoise"], True), (["--denoise", "--denoise-sigma", "3"], True), (["--denoise-sigma", "3"], False), ([], False)):
            args = cli.build_parser().parse_args([command, "--input-slices", "x", "--output-volume", "v.nii.gz", *extra])
            args.device = torch.device("cpu")
            caplog.clear()
            with caplog.at_level(logging.WARNING), pytest.raises(KeyboardInterrupt):
                run(args)
            assert ("--denoise" in caplog.text and "are ignored with --input-slices" in caplog.text) == warned, (command, extra)


def test_load_stacks_without_the_flag_never_touches_the_module(tmp_path, monkeypatch):
    from nesvor_amd import cli
    from nesvor_amd.image_io import load_stack

    paths, masks = _files(tmp_path)

    def refuse(*a, **k):
        raise AssertionError("denoise called")

    monkeypatch.delitem(sys.modules, "nesvor_amd.denoise", raising=False)
    monkeypatch.setattr(cli, "_denoise_stacks", refuse)
    args = cli.build_parser().parse_args(["assess", "--input-stacks", *paths, "--stack-masks", *masks])
    args.device = torch.device("cpu")
    loaded = cli._load_stacks(args)
    assert "nesvor_amd.denoise" not in sys.modules
    for st, p, m in zip(loaded, paths, masks):
        ref = load_stack(p, m)
        assert torch.equal(st.mask, ref.mask) and torch.equal(st.slices, ref.slices)
    args.denoise = True  # the control: the flag, and the step is taken
    with pytest.raises(AssertionError, match="denoise called"):
        cli._load_stacks(args)


def test_assess_with_denoise_runs_on_host_tensors(tmp_path, caplog):
    """The step sits after the masking switches and before the bias correction; ``assess`` scores the denoised stacks higher
    (noise lowers the adjacent-slice NCC)."""
    from nesvor_amd import cli
    from nesvor_amd.assess import assess_stacks

    paths, masks = _files(tmp_path)
    base = ["assess", "--input-stacks", *paths, "--stack-masks", *masks, "--thicknesses", "2", "2"]
    args = cli.build_parser().parse_args(base)
    args.device = torch.device("cpu")
    plain = cli._load_stacks(args)
    args = cli.build_parser().parse_args(base + ["--denoise"])
    args.device = torch.device("cpu")
    with caplog.at_level(logging.INFO):
        loaded = cli._load_stacks(args)
    assert "Denoising, stack 0 (" in caplog.text and "method noise rms" in caplog.text and "Denoising of 2 stacks finished" in caplog.text
    for a, b in zip(plain, loaded):
        assert torch.equal(a.mask, b.mask) and not torch.equal(a.slices, b.slices) and torch.equal(a.slices[~a.mask], b.slices[~b.mask])
    before, after = assess_stacks(plain, "ncc"), assess_stacks(loaded, "ncc")
    print("ncc", [r["score"] for r in before], "->", [r["score"] for r in after])
    assert all(x["score"] > y["score"] for x, y in zip(after, before))
    # the command itself, on the host: its JSON carries the scores of the denoised stacks
    report = str(tmp_path / "assess.json")
    args = cli.build_parser().parse_args(base + ["--denoise", "--output-json", report])
    args.device = torch.device("cpu")
    cli.assess_cmd(args)
    assert [r["score"] for r in json.load(open(report))] == pytest.approx([r["score"] for r in after])


# ---------------------------------------------------------------------------------------------------------------------
# the operator
# ---------------------------------------------------------------------------------------------------------------------
def test_operator_is_registered_with_a_fake_kernel_and_no_cpu_kernel():
    import nesvor_amd.ops as ops

    assert "nlm_denoise" in ops.SCHEMAS
    y = torch.empty(4, 1, 9, 7, device="meta")
    out, stats = torch.ops.nesvor.nlm_denoise(y, None, torch.empty(4, device="meta"), 1, 3, 1.0)
    assert out.shape == (4, 1, 9, 7) and out.dtype == torch.float32 and out.device.type == "meta"
    assert stats.shape == (4, 2) and stats.dtype == torch.float64 and stats.device.type == "meta"
    out, _ = torch.ops.nesvor.nlm_denoise(torch.empty(2, 5, 6, device="meta"), torch.empty(2, 5, 6, dtype=torch.bool, device="meta"),
                                          torch.empty(2, device="meta"), 3, 10, 0.5)
    assert out.shape == (2, 5, 6)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::nlm_denoise'"):
        torch.ops.nesvor.nlm_denoise(torch.zeros(1, 1, 4, 4), None, torch.ones(1), 1, 3, 1.0)
