"""Bias field correction on the CPU (the composed float64 path of nesvor_amd/bias.py): the basis tables, fit and update against a
straight-loop restatement that does not use separability, the histogram, the 32^3 phantom under a known field, degenerate
inputs, the command-line flags, ``_load_stacks`` and ``save_stack``."""
import math
from argparse import Namespace

import numpy as np
import pytest
import torch

N4_DEFAULTS = {"n_levels_n4": 4, "n_iter_n4": 50, "tol_n4": 0.001, "n_control_points_n4": 4, "n_bins_n4": 200, "fwhm_n4": 0.15,
               "noise_n4": 0.01}
MINIMAL = {"reconstruct": ["--input-stacks", "a.nii.gz"], "register": ["--input-stacks", "a.nii.gz", "--output-slices", "out"],
           "svr": ["--input-stacks", "a.nii.gz", "--output-volume", "v.nii.gz"], "assess": ["--input-stacks", "a.nii.gz"],
           "correct-bias-field": ["--input-stacks", "a.nii.gz", "--output-corrected-stacks", "c.nii.gz"]}


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [1, 2, 8, 13])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 40, 257])
def test_basis_tables(n, S):
    from nesvor_amd.bias import axis_table, dense_weights

    span, basis = axis_table(n, S)
    assert span.dtype == torch.int32 and basis.dtype == torch.float64 and basis.shape == (n, 4) and span.shape == (n,)
    assert float((basis.sum(1) - 1).abs().max()) < 1e-15 and bool((basis >= 0).all())
    assert int(span.min()) >= 0 and int(span.max()) <= S - 1
    # tau = 1 (the first basis value is 0) only at the last index, and only there
    t = torch.arange(n, dtype=torch.float64) / max(n - 1, 1) * S
    tau = t - span
    assert bool((tau[:-1] < 1).all()) and bool((tau >= 0).all())
    if n > 1:
        assert float(tau[-1]) == 1.0 and float(basis[-1, 0]) == 0.0 and int(span[-1]) == S - 1
    else:
        assert float(tau[0]) == 0.0 and int(span[0]) == 0
    dense = dense_weights(span, basis, S)
    assert dense.shape == (n, S + 3) and float((dense.sum(1) - 1).abs().max()) < 1e-15
    assert int((dense != 0).sum(1).max()) <= 4


# ---------------------------------------------------------------------------------------------------------------------
# fit and update against straight loops
# ---------------------------------------------------------------------------------------------------------------------
def _axis_weights(i, n, S):
    """(first control index, four weights) of voxel index i: the issue's formulas, restated with python floats."""
    t = i / (n - 1) * S if n > 1 else 0.0
    s = min(math.floor(t), S - 1)
    tau = t - s
    return s, [(1 - tau) ** 3 / 6, (3 * tau ** 3 - 6 * tau ** 2 + 4) / 6, (-3 * tau ** 3 + 3 * tau ** 2 + 3 * tau + 1) / 6, tau ** 3 / 6]


def _loops(r, valid, S):
    """Lattice, divisor and evaluated field by scattering every voxel over its 64 control points."""
    D, H, W = r.shape
    C = S + 3
    num, den = np.zeros((C, C, C)), np.zeros((C, C, C))
    weights = {}
    for z in range(D):
        for y in range(H):
            for x in range(W):
                (sz, bz), (sy, by), (sx, bx) = _axis_weights(z, D, S), _axis_weights(y, H, S), _axis_weights(x, W, S)
                w = {(sz + a, sy + b, sx + c): bz[a] * by[b] * bx[c] for a in range(4) for b in range(4) for c in range(4)}
                weights[z, y, x] = w
                if not valid[z, y, x]:
                    continue
                total = sum(q * q for q in w.values())
                for k, q in w.items():
                    num[k] += q ** 3 * r[z, y, x] / total
                    den[k] += q * q
    phi = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    field = np.zeros((D, H, W))
    for p, w in weights.items():
        field[p] = sum(phi[k] * q for k, q in w.items())
    return phi, den, field


def _first_cell(shape, S):
    """The voxels of the span cell (0, 0, 0)."""
    cell = np.ones(shape, dtype=bool)
    for axis, n in enumerate(shape):
        first = np.array([_axis_weights(i, n, S)[0] == 0 for i in range(n)])
        cell &= first.reshape([-1 if a == axis else 1 for a in range(3)])
    return cell


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("shape", [(3, 4, 5), (1, 2, 7)])
def test_fit_and_update_against_straight_loops(shape, S):
    """With a lookup table of zeros the residual is u = v - f itself.  S = 2: the mask empties the span cell (0, 0, 0), the only
    one control point (0, 0, 0) sees, so the lattice and its divisor are exactly 0 there; S = 1 has one cell: a random mask, and
    with everything masked the whole lattice is exactly 0."""
    from nesvor_amd import bias

    g = torch.Generator().manual_seed(7 * S + sum(shape))
    v = torch.randn(shape, generator=g, dtype=torch.float64)
    f = 0.1 * torch.randn(shape, generator=g, dtype=torch.float64)
    valid = torch.rand(shape, generator=g) < 0.8
    if S == 2:
        valid &= ~torch.tensor(_first_cell(shape, S))
    assert bool(valid.any()) and not bool(valid.all())
    tables = bias.LevelTables(shape, S)
    rng = torch.tensor([-5.0, 5.0], dtype=torch.float64)
    lut = torch.zeros(16, dtype=torch.float64)
    lattice, weight = bias.fit_composed(v, f, valid, rng, lut, tables)
    phi, den, field = _loops((v - f).numpy(), valid.numpy(), S)
    close = lambda a, b: np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert lattice.shape == (S + 3,) * 3 and close(lattice.numpy(), phi) and close(weight.numpy(), den)
    assert np.array_equal(weight.numpy() == 0, den == 0) and bool((lattice[weight == 0] == 0).all())
    if S == 2:
        assert float(lattice[0, 0, 0]) == 0.0 and float(weight[0, 0, 0]) == 0.0 and phi[0, 0, 0] == 0.0
    f_new, stats = bias.update_composed(lattice, tables, f, v, valid)
    assert close((f_new - f).numpy(), field)
    gm = np.expm1(field[valid.numpy()])
    u = (v - f_new)[valid].numpy()
    expected = np.array([valid.sum().item(), gm.sum(), (gm * gm).sum(), u.min(), u.max()])
    assert np.abs(stats.numpy() - expected).max() <= 1e-12 * np.abs(expected).max()
    # every voxel is updated, valid or not
    assert bool(((f_new - f)[~valid] != 0).any())
    empty, w0 = bias.fit_composed(v, f, torch.zeros(shape, dtype=torch.bool), rng, lut, tables)
    assert bool((empty == 0).all()) and bool((w0 == 0).all())


def test_residual_interpolates_the_lookup_table():
    from nesvor_amd import bias

    g = torch.Generator().manual_seed(3)
    v, f = torch.randn(2, 3, 9, generator=g, dtype=torch.float64), torch.zeros(2, 3, 9, dtype=torch.float64)
    rng = torch.tensor([-1.0, 1.5], dtype=torch.float64)  # some u outside on both sides: c is clamped
    lut = torch.randn(12, generator=g, dtype=torch.float64)
    r = bias.residual_composed(v, f, rng, lut).numpy()
    slope = 2.5 / 11
    for idx in np.ndindex(2, 3, 9):
        c = min(max((float(v[idx]) + 1.0) / slope, 0.0), 11.0)
        j = min(math.floor(c), 10)
        assert abs(r[idx] - (float(v[idx]) - (float(lut[j]) * (1 - (c - j)) + float(lut[j + 1]) * (c - j)))) < 1e-12


def test_histogram():
    from nesvor_amd import bias

    g = torch.Generator().manual_seed(11)
    v, f = torch.randn(4, 5, 6, generator=g, dtype=torch.float64), 0.2 * torch.randn(4, 5, 6, generator=g, dtype=torch.float64)
    valid = torch.rand(4, 5, 6, generator=g) < 0.7
    u = (v - f)[valid]
    rng = torch.stack([u.min(), u.max()])
    for n_bins in (2, 7, 200):
        hist = bias.histogram_composed(v, f, valid, rng, n_bins)
        assert hist.shape == (n_bins,) and bool((hist >= 0).all())
        assert abs(float(hist.sum()) - int(valid.sum())) <= 1e-9
        only_hi = torch.zeros_like(valid)
        only_hi.view(-1)[torch.nonzero(valid.view(-1) & ((v - f).view(-1) == rng[1]))[0]] = True
        top = bias.histogram_composed(v, f, only_hi, rng, n_bins)
        assert abs(float(top[-1]) - 1.0) <= 1e-12 and float(top[:-1].abs().sum()) <= 1e-12
        low = bias.histogram_composed(v, f, valid & ((v - f) == rng[0]), rng, n_bins)
        assert float(low[0]) == 1.0 and float(low[1:].abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the 32^3 phantom under exp(0.35 x - 0.25 y^2 + 0.2 z x + 0.15 z)
# ---------------------------------------------------------------------------------------------------------------------
def _phantom_case():
    from nesvor_amd.phantom import phantom3d

    vol = torch.tensor(phantom3d(n=32), dtype=torch.float64)
    ax = torch.linspace(-1, 1, 32, dtype=torch.float64)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    log_field = 0.35 * x - 0.25 * y ** 2 + 0.2 * z * x + 0.15 * z
    return vol, vol * torch.exp(log_field), log_field


def test_phantom_field_is_recovered():
    """The values the definition was prototyped with: 50, 19, 7 and 4 iterations, the field's error std over the mask 0.0041
    against the field's own 0.2430, the CV of the largest tissue class (value 0.2, 6302 voxels) 0.0035 against 0.243."""
    from nesvor_amd.bias import correct_bias_field

    vol, img, log_field = _phantom_case()
    mask = vol > 0
    corrected, f, info = correct_bias_field(img, mask)
    assert info["iterations"] == [50, 19, 7, 4] and info["cv"] < 1e-3 and info["fused"] is False
    assert f.dtype == torch.float64 and f.shape == img.shape and corrected.shape == img.shape
    true = log_field - log_field[mask].mean()
    err_std, true_std = float((f - true)[mask].std()), float(true[mask].std())
    values, counts = torch.unique(vol[mask], return_counts=True)
    cls = vol == values[counts.argmax()]
    cv = lambda a: float(a[cls].std() / a[cls].mean())
    cv_before, cv_after = cv(img), cv(corrected)
    print(f"field error std {err_std:.4f} (field {true_std:.4f}); largest class {float(values[counts.argmax()]):.2f} x "
          f"{int(counts.max())}: CV {cv_before:.4f} -> {cv_after:.4f}")
    assert int(counts.max()) == 6302
    assert err_std <= 0.1 * true_std and cv_after <= 0.1 * cv_before
    assert round(true_std, 4) == 0.2430 and round(err_std, 4) == 0.0041 and round(cv_before, 3) == 0.243 and round(cv_after, 4) == 0.0035
    assert abs(float(f[mask].mean())) < 1e-12
    assert bool((corrected[img == 0] == 0).all()) and torch.equal(corrected == 0, img == 0)
    assert torch.allclose(corrected, img / torch.exp(f), rtol=1e-15, atol=0)
    # a (n,1,h,w) stack and a mask of uint8 are the same thing
    c4, f4, info4 = correct_bias_field(img[:, None], mask[:, None].to(torch.uint8))
    assert c4.shape == (32, 1, 32, 32) and torch.equal(c4[:, 0], corrected) and torch.equal(f4[:, 0], f) and info4 == info


def test_degenerate_inputs(caplog):
    from nesvor_amd.bias import correct_bias_field

    g = torch.Generator().manual_seed(5)
    img = torch.rand(3, 1, 6, 7, generator=g) + 0.5
    with caplog.at_level("WARNING"):
        out, f, info = correct_bias_field(img, torch.zeros_like(img, dtype=torch.bool))
    assert torch.equal(out, img) and bool((f == 0).all()) and f.shape == img.shape and info["iterations"] == []
    assert "unchanged" in caplog.text
    caplog.clear()
    const = torch.full((3, 1, 6, 7), 2.5)
    with caplog.at_level("WARNING"):
        out, f, info = correct_bias_field(const, None)
    assert torch.equal(out, const) and bool((f == 0).all()) and "unchanged" in caplog.text
    zeros = torch.zeros(2, 4, 4)
    out, f, _ = correct_bias_field(zeros)
    assert torch.equal(out, zeros) and bool((f == 0).all())
    single = torch.rand(1, 1, 9, 8, generator=g) + 0.5
    out, f, info = correct_bias_field(single, n_levels=2, n_iter=3)
    assert out.shape == single.shape and bool(torch.isfinite(out).all()) and bool(torch.isfinite(f).all())
    assert len(info["iterations"]) == 2 and all(1 <= k <= 3 for k in info["iterations"])
    with pytest.raises(ValueError):
        correct_bias_field(torch.rand(3, 2, 4, 4))
    with pytest.raises(ValueError):
        correct_bias_field(img, torch.ones(3, 1, 6, 6, dtype=torch.bool))


# ---------------------------------------------------------------------------------------------------------------------
# command line, _load_stacks, save_stack
# ---------------------------------------------------------------------------------------------------------------------
def test_parser_has_the_flags_on_all_five_commands():
    from nesvor_amd import cli

    parser = cli.build_parser()
    for command, argv in MINIMAL.items():
        args = parser.parse_args([command] + argv)
        for name, value in N4_DEFAULTS.items():
            assert getattr(args, name) == value, (command, name)
        assert cli.bias_options(args) == {"n_levels": 4, "n_iter": 50, "tol": 0.001, "n_control_points": 4, "n_bins": 200, "fwhm": 0.15,
                                          "noise": 0.01}
        if command == "correct-bias-field":
            assert not hasattr(args, "bias_field_correction")
            continue
        assert args.bias_field_correction is False
        on = parser.parse_args([command] + argv + ["--bias-field-correction", "--n-levels-n4", "2", "--n-iter-n4", "5", "--tol-n4", "0.01",
                                                   "--n-control-points-n4", "5", "--n-bins-n4", "64", "--fwhm-n4", "0.2", "--noise-n4", "0.1"])
        assert on.bias_field_correction is True
        assert cli.bias_options(on) == {"n_levels": 2, "n_iter": 5, "tol": 0.01, "n_control_points": 5, "n_bins": 64, "fwhm": 0.2, "noise": 0.1}
    for argv in (["sample-volume", "--input-model", "m.pt", "--output-volume", "v"],
                 ["sample-slices", "--input-model", "m.pt", "--input-slices", "d", "--simulated-slices", "s"]):
        assert not hasattr(parser.parse_args(argv), "n_levels_n4")  # the commands without stacks do not have the flags
        with pytest.raises(SystemExit):
            parser.parse_args(argv + ["--bias-field-correction"])
    assert cli.bias_options(Namespace()) == cli.bias_options(parser.parse_args(["assess"] + MINIMAL["assess"]))  # (older Namespaces)
    assert "correct-bias-field" in cli.__doc__ and "--bias-field-correction" in cli.__doc__


def _stack(seed=0, n=5, h=6, w=7):
    """A stack as ``load_stack`` makes them: one rotation (0.3 rad about z) and in-plane offset, slices ``gap`` apart along z."""
    from nesvor_amd.image import Stack
    from nesvor_amd.transform import RigidTransform

    g = torch.Generator().manual_seed(seed)
    img = torch.rand(n, 1, h, w, generator=g) + 0.25
    img[0, 0, :2] = 0
    c, s = math.cos(0.3), math.sin(0.3)
    R = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    gap = 2.5
    t = torch.tensor([[1.5, -2.0, 3.0 + gap * k] for k in range(n)])
    mat = torch.cat((R.expand(n, 3, 3), t[:, :, None]), -1)
    return Stack(img, img > 0, RigidTransform(mat, trans_first=True), resolution_x=1.25, resolution_y=0.75, thickness=gap, gap=gap)


def test_save_stack_round_trip(tmp_path):
    from nesvor_amd.image_io import load_stack, save_stack

    st = _stack()
    path = str(tmp_path / "stack.nii.gz")
    save_stack(path, st)
    back = load_stack(path)
    assert torch.equal(back.slices, st.slices) and back.slices.shape == (5, 1, 6, 7)
    assert abs(back.resolution_x - 1.25) < 1e-6 and abs(back.resolution_y - 0.75) < 1e-6 and abs(back.gap - 2.5) < 1e-6
    assert float((back.transformation.matrix() - st.transformation.matrix()).abs().max()) < 1e-5
    other = torch.rand(5, 1, 6, 7) + 1
    save_stack(path, st, other)
    back = load_stack(path)
    assert torch.equal(back.slices, other)
    assert float((back.transformation.matrix() - st.transformation.matrix()).abs().max()) < 1e-5
    with pytest.raises(ValueError):
        save_stack(path, st, other[:4])


def test_load_stacks_corrects_once_per_run(tmp_path, monkeypatch):
    from nesvor_amd import bias, cli
    from nesvor_amd.image_io import save_stack

    paths = []
    for j in range(2):
        paths.append(str(tmp_path / f"s{j}.nii.gz"))
        save_stack(paths[-1], _stack(seed=j))
    calls = []
    monkeypatch.setattr(bias, "correct_stacks", lambda stacks, **kw: calls.append((len(stacks), kw)) or [])
    base = dict(input_stacks=paths, stack_masks=None, thicknesses=None, device=torch.device("cpu"))
    plain = cli._load_stacks(Namespace(**base))  # an older Namespace: no flag at all
    off = cli._load_stacks(Namespace(**base, bias_field_correction=False))
    assert calls == [] and len(plain) == len(off) == 2
    on = cli._load_stacks(Namespace(**base, bias_field_correction=True, n_iter_n4=3, n_bins_n4=32))
    assert len(on) == 2 and len(calls) == 1 and calls[0][0] == 2
    assert calls[0][1] == {"n_levels": 4, "n_iter": 3, "tol": 0.001, "n_control_points": 4, "n_bins": 32, "fwhm": 0.15, "noise": 0.01}
    monkeypatch.undo()
    # for real, on the composed path: the stacks come back corrected in place, as correct_bias_field corrects them
    real = cli._load_stacks(Namespace(**base, bias_field_correction=True, n_levels_n4=1, n_iter_n4=2))
    expected, _, _ = bias.correct_bias_field(plain[0].slices, plain[0].mask, n_levels=1, n_iter=2)
    assert torch.equal(real[0].slices, expected) and not torch.equal(real[0].slices, plain[0].slices)


def test_mismatched_output_counts_are_refused():
    from nesvor_amd import cli

    parser = cli.build_parser()
    two = ["correct-bias-field", "--input-stacks", "a.nii.gz", "b.nii.gz"]
    with pytest.raises(SystemExit, match="output corrected stacks"):
        cli.correct_bias_field_cmd(parser.parse_args(two + ["--output-corrected-stacks", "c.nii.gz"]))
    with pytest.raises(SystemExit, match="output bias fields"):
        cli.correct_bias_field_cmd(parser.parse_args(two + ["--output-corrected-stacks", "c.nii.gz", "d.nii.gz", "--output-bias-fields", "f.nii.gz"]))
    with pytest.raises(SystemExit, match="stack masks"):
        cli.correct_bias_field_cmd(parser.parse_args(two + ["--output-corrected-stacks", "c.nii.gz", "d.nii.gz", "--stack-masks", "m.nii.gz"]))
