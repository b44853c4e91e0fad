"""Rigid alignment for ``evaluate`` on the CPU (nesvor_amd/align.py, composed path, float64 unless said otherwise): the pose
algebra and its exact zero, the moments against ``resample_composed``, the recovery of a known motion, the cases in which nothing
may change, the pyramid's level rule, the overlap rule and the command."""
import json
import math
import sys

import pytest
import torch

from test_evaluate import _cpu, _pose, _rotation, _volume

# the asserted bound on the target registration error: a quarter and a half of a reference voxel (1 mm)
TRE_MEAN, TRE_MAX = 0.25, 0.5
SHIFT = (2.0, -1.5, 1.0)  # q, mm
_FIXTURES = {}


def fixture(degrees, dtype=torch.float64):
    """(R, X, G_true) shared by the tests and never written.  R: a 48^3 lattice of 1 mm, a textured ellipsoid.  X: a 66^3 lattice
    of 0.8 mm at the identity pose holding 0.9 x (the object at Q^T (p - q)) + noise on the voxels that lie inside R's lattice;
    Q = ``degrees`` about (1,2,3), q = SHIFT.  The truth is G: p -> Q p + q."""
    from nesvor_amd import evaluate
    from nesvor_amd.utils import gaussian_blur

    key = (degrees, dtype)
    if key not in _FIXTURES:
        n, m = 48, 66
        tex = gaussian_blur(torch.randn(1, 1, n, n, n, generator=torch.Generator().manual_seed(11), dtype=torch.float64), 2.0, 4.0)[0, 0]
        tex = tex / tex.std()
        ax = torch.arange(n, dtype=torch.float64) - (n - 1) / 2
        z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
        ellipsoid = torch.sqrt(x ** 2 + (y / 0.8) ** 2 + (z / 0.9) ** 2) < 0.42 * n
        obj = torch.where(ellipsoid, (0.5 + 0.2 * tex).clamp(min=0), torch.zeros_like(tex))
        Q, q = _rotation(degrees, (1.0, 2.0, 3.0)), torch.tensor(SHIFT, dtype=torch.float64)
        # X's lattice seen from R's world frame: world_R = Q^T (world_X - q), i.e. the pose (Q^T, -q) in the world = R (p + t) convention
        seen = _volume(torch.zeros(m, m, m, dtype=torch.float64), _pose(Q.t(), tuple((-q).tolist())), (0.8, 0.8, 0.8))
        J, _, cover = evaluate.interpolate_composed((m, m, m), obj, None, evaluate.index_map(seen, _volume(obj)))
        noise = 0.01 * torch.randn(m, m, m, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        G = torch.eye(4, dtype=torch.float64)
        G[:3, :3], G[:3, 3] = Q, q
        _FIXTURES[key] = (_volume(obj.to(dtype), _pose(), (1.0, 1.0, 1.0), obj > 0),
                          _volume(torch.where(cover, 0.9 * J + noise, torch.zeros_like(J)).to(dtype), _pose(), (0.8, 0.8, 0.8), cover), G)
    return _FIXTURES[key]


def tre(reference, G_est, G_true):
    """(mean, max) of |G_est p - G_true p| over the world positions p of the reference mask's voxel centres."""
    from nesvor_amd.evaluate import _geometry

    Rr, tr, sr, cr = _geometry(reference)
    index = torch.nonzero(reference.mask.cpu()).double().flip(1)  # (x, y, z)
    p = ((index - cr) * sr + tr) @ Rr.t()
    G_est = torch.as_tensor(G_est, dtype=torch.float64)
    e = ((p @ G_est[:3, :3].t() + G_est[:3, 3]) - (p @ G_true[:3, :3].t() + G_true[:3, 3])).norm(dim=1)
    return float(e.mean()), float(e.max())


def _rand(shape, seed):
    return 0.1 + 0.9 * torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ---------------------------------------------------------------------------------------------------------------------
# poses and maps
# ---------------------------------------------------------------------------------------------------------------------
def test_the_zero_pose_is_the_old_map_bit_for_bit():
    from nesvor_amd.align import centroid, pose_maps
    from nesvor_amd.evaluate import index_map

    mask = torch.rand(7, 9, 11, generator=torch.Generator().manual_seed(1)) < 0.6
    for rot, dtype in ((None, torch.float64), (_rotation(10.0, (1.0, 2.0, 3.0)), torch.float64), (_rotation(33.0, (3.0, -1.0, 2.0)), torch.float32)):
        ref = _volume(_rand((7, 9, 11), 0), _pose(rot, (3.0, -2.0, 0.7), dtype), (0.8, 0.9, 1.1), mask)
        vol = _volume(_rand((8, 6, 10), 1), _pose(_rotation(-17.0, (0.0, 1.0, 1.0)), (0.3, 0.1, -4.0), dtype), (1.2, 0.7, 0.8))
        c = centroid(ref)
        assert c.dtype == torch.float64 and c.shape == (3,)
        maps = pose_maps(ref, vol, [[0.0] * 6, [0.0] * 6], c)
        assert maps.shape == (2, 3, 4) and maps.dtype == torch.float64
        assert torch.equal(maps[0], index_map(ref, vol)) and torch.equal(maps[1], maps[0])
    assert pose_maps(ref, vol, [], c).shape == (0, 3, 4)


def test_a_translation_moves_the_offset_and_the_matrix_is_the_correction():
    from nesvor_amd.align import centroid, correction, pose_maps, rotation

    Rx = _rotation(-17.0, (0.0, 1.0, 1.0))
    ref = _volume(_rand((7, 9, 11), 0), _pose(_rotation(10.0, (1.0, 2.0, 3.0)), (3.0, -2.0, 0.7)), (0.8, 0.9, 1.1))
    vol = _volume(_rand((8, 6, 10), 1), _pose(Rx, (0.3, 0.1, -4.0)), (1.2, 0.7, 0.8))
    c = centroid(ref)
    # without a mask the centroid is the lattice's centre: world = R_R t_R
    assert float((c - _rotation(10.0, (1.0, 2.0, 3.0)) @ torch.tensor([3.0, -2.0, 0.7], dtype=torch.float64)).abs().max()) <= 1e-14
    t = torch.tensor([1.5, -0.25, 3.0], dtype=torch.float64)
    zero, moved = pose_maps(ref, vol, [[0.0] * 6, [0.0, 0.0, 0.0, *t.tolist()]], c)
    assert float((moved[:, :3] - zero[:, :3]).abs().max()) == 0  # the rotation part is untouched
    expect = (Rx.t() @ t) / torch.tensor([1.2, 0.7, 0.8], dtype=torch.float64)  # world moves by t: X's index by R_X^T t / s_X
    assert float((moved[:, 3] - zero[:, 3] - expect).abs().max()) <= 1e-13
    theta = [4.0, -3.0, 7.0, 0.5, 1.0, -2.0]
    G, rot = correction(theta, c), rotation(theta[:3])
    assert float((rot @ rot.t() - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-15 and float(torch.linalg.det(rot)) == pytest.approx(1.0, abs=1e-15)
    angle = math.degrees(math.acos((float(rot.trace()) - 1) / 2))
    assert angle == pytest.approx(math.sqrt(4.0 ** 2 + 3.0 ** 2 + 7.0 ** 2), abs=1e-12)
    p = torch.randn(5, 3, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    direct = c + (p - c) @ rot.t() + torch.tensor(theta[3:], dtype=torch.float64)
    assert float((p @ G[:3, :3].t() + G[:3, 3] - direct).abs().max()) <= 1e-13 and G[3].tolist() == [0.0, 0.0, 0.0, 1.0]
    assert torch.equal(correction([0.0] * 6, c), torch.eye(4, dtype=torch.float64))
    # M(theta) is the old map after G: an R voxel's world position p is looked up in X at G p
    from nesvor_amd.evaluate import index_map

    M = pose_maps(ref, vol, [theta], c)[0]
    M0 = index_map(ref, vol)
    # (the old map is affine in the world position: compare through three voxels' positions and the origin)
    from nesvor_amd.evaluate import _geometry

    Rr, tr, sr, cr = _geometry(ref)
    Rxx, tx, sx, cx = _geometry(vol)
    index = torch.tensor([[0.0, 0.0, 0.0], [3.0, 1.0, 2.0], [10.0, 8.0, 6.0], [5.0, 0.0, 1.0]], dtype=torch.float64)
    world = ((index - cr) * sr + tr) @ Rr.t()
    moved_world = world @ G[:3, :3].t() + G[:3, 3]
    expect_u = (moved_world @ Rxx - tx) / sx + cx  # R_X^T world - t_X
    got_u = index @ M[:, :3].t() + M[:, 3]
    assert float((got_u - expect_u).abs().max()) <= 1e-12 and float((index @ M0[:, :3].t() + M0[:, 3] - got_u).abs().max()) > 0.5


def test_moments_are_the_resamplers_sums_bit_for_bit():
    from nesvor_amd.align import centroid, pose_maps, pose_moments, pose_moments_composed
    from nesvor_amd.evaluate import resample_composed

    g = torch.Generator().manual_seed(4)
    ref = _volume(_rand((12, 13, 14), 3), _pose(), (1.0, 1.0, 1.0), torch.rand(12, 13, 14, generator=g) < 0.8)
    vol = _volume(_rand((16, 17, 18), 4), _pose(_rotation(10.0, (1.0, 2.0, 3.0)), (0.4, 0.4, 0.4)), (0.8, 0.8, 0.8), torch.rand(16, 17, 18, generator=g) < 0.8)
    thetas = [[0.0] * 6, [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], [0.0, 0.0, -2.0, 0.5, 0.0, 0.0], [3.0, 1.0, 2.0, -1.0, 0.5, 0.25]]
    maps = pose_maps(ref, vol, thetas, centroid(ref))
    for dtype in (torch.float64, torch.float32):
        args = (ref.image.to(dtype), ref.mask, vol.image.to(dtype), vol.mask)
        sums = pose_moments_composed(*args, maps)
        assert sums.shape == (4, 6) and sums.dtype == torch.float64
        for k in range(4):
            expect = resample_composed(*args, maps[k])[2]
            assert torch.equal(sums[k], expect[[0, 2, 3, 4, 5, 6]]) and float(sums[k, 0]) > 500
        assert torch.equal(pose_moments(*args, maps), sums)  # host tensors take the composed path
        assert len({tuple(row) for row in sums.tolist()}) == 4
    assert pose_moments_composed(*args, maps[:0]).shape == (0, 6)


# ---------------------------------------------------------------------------------------------------------------------
# recovery
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degrees,dof", [(8.0, "rigid"), (15.0, "rigid"), (0.0, "translation")])
def test_recovery_of_a_known_motion(degrees, dof):
    """Measured (float64, CPU): mean / max TRE 0.034 / 0.053 mm at 8 degrees (1681 pose evaluations), 0.032 / 0.041 mm at 15
    degrees (2149), 0.037 / 0.037 mm for the translation alone (193); DESIGN.md, "Rigid alignment"."""
    from nesvor_amd.align import align_volumes

    ref, vol, G = fixture(degrees)
    out = align_volumes(ref, vol, dof)
    mean, worst = tre(ref, out["matrix"], G)
    print(f"{degrees} degrees, {dof}: TRE mean {mean:.4f} max {worst:.4f} mm; ncc {out['ncc_before']:.4f} -> {out['ncc_after']:.4f}; "
          f"{out['evaluations']} pose evaluations on {out['levels']} levels; theta {[round(v, 4) for v in out['theta']]}")
    assert mean <= TRE_MEAN and worst <= TRE_MAX
    assert out["ncc_after"] > out["ncc_before"] and out["accepted"] and out["levels"] == 3
    assert out["rotation_deg"] == pytest.approx(degrees, abs=0.5) and (dof == "rigid" or out["theta"][:3] == [0.0, 0.0, 0.0])
    assert out["matrix"].shape == (4, 4) and out["matrix"].dtype == torch.float64 and out["translation_mm"] == float(out["matrix"][:3, 3].norm())


def test_identical_volumes_stay_where_they_are():
    from nesvor_amd.evaluate import METRICS, compare_volumes

    ref, _, _ = fixture(8.0)
    same = _volume(ref.image.clone(), _pose(), (1.0, 1.0, 1.0), ref.mask.clone())
    plain = compare_volumes(ref, same)
    for dof in ("rigid", "translation"):
        out = compare_volumes(ref, same, align=dof)
        a = out["alignment"]
        assert a["theta"] == [0.0] * 6 and torch.equal(a["matrix"], torch.eye(4, dtype=torch.float64)) and a["levels"] == 3
        assert a["rotation_deg"] == 0 and a["translation_mm"] == 0 and a["ncc_after"] == a["ncc_before"]
        assert all(out[k] == plain[k] for k in METRICS) and "alignment" not in plain
        assert all(torch.equal(out[k], plain[k]) for k in ("resampled", "valid", "ssim_map"))


def test_a_rejected_result_leaves_the_old_comparison(monkeypatch, caplog):
    """``descend`` replaced by one that walks to a worse pose: theta = 0 with the warning, and the report is --align none's."""
    from nesvor_amd import align
    from nesvor_amd.evaluate import METRICS, compare_volumes

    ref = _volume(_rand((16, 16, 16), 5))
    vol = _volume(ref.image * 0.5 + 0.01 * _rand((16, 16, 16), 6))

    def worse(problem, theta, free, step, rounds, max_iter, start=None):
        moved = [0.0, 0.0, 0.0, 1.3, 0.0, 0.0]
        return moved, problem.sums([moved])[0], start[0]

    monkeypatch.setattr(align, "descend", worse)
    with caplog.at_level("WARNING"):
        out = compare_volumes(ref, vol, align="rigid")
    a = out["alignment"]
    assert "did not raise the correlation" in caplog.text and not a["accepted"] and a["theta"] == [0.0] * 6 and a["levels"] == 1
    plain = compare_volumes(ref, vol)
    assert all(out[k] == plain[k] for k in METRICS) and all(torch.equal(out[k], plain[k]) for k in ("resampled", "valid", "ssim_map"))


def test_a_volume_far_away_is_skipped():
    from nesvor_amd.evaluate import compare_volumes

    ref, vol, _ = fixture(8.0)
    far = _volume(vol.image, _pose(None, (0.0, 1000.0, 0.0)), (0.8, 0.8, 0.8), vol.mask)
    out = compare_volumes(ref, far, align="rigid")
    a = out["alignment"]
    assert a["skipped"] and not a["accepted"] and a["theta"] == [0.0] * 6 and a["evaluations"] == 1
    assert out["n"] == 0 and out["coverage"] == 0 and math.isnan(out["psnr"]) and math.isnan(out["ncc"])


def test_the_level_rule():
    from nesvor_amd.align import align_volumes, pyramid_level, usable_levels

    def blank(*shape):
        return _volume(torch.zeros(*shape, dtype=torch.float64))

    assert usable_levels(blank(48, 48, 48), blank(66, 66, 66), 3) == 3 and usable_levels(blank(48, 48, 48), blank(66, 66, 66), 2) == 2
    assert usable_levels(blank(96, 96, 96), blank(96, 96, 96), 3) == 3  # --align-levels is the most that are used
    assert usable_levels(blank(47, 48, 48), blank(66, 66, 66), 3) == 2  # 47 // 4 = 11
    assert usable_levels(blank(16, 16, 16), blank(16, 16, 16), 3) == 1
    assert usable_levels(blank(48, 23, 48), blank(66, 66, 66), 3) == 1 and usable_levels(blank(48, 48, 48), blank(66, 66, 23), 3) == 1
    assert usable_levels(blank(48, 24, 48), blank(66, 66, 24), 3) == 2 and usable_levels(blank(48, 48, 48), blank(48, 48, 48), 0) == 1
    image = _rand((16, 16, 16), 7)
    out = align_volumes(_volume(image), _volume(image.roll(1, 2) * 0.7))
    assert out["levels"] == 1 and out["accepted"] and out["theta"][3] == pytest.approx(1.0, abs=0.1)
    # a level: the pose kept, the voxels 2^l times as large, size // 2^l samples, the mask of the blurred mask
    ref, _, _ = fixture(8.0)
    level = pyramid_level(ref, 2, torch.float64, torch.device("cpu"))
    assert level.image.shape == (12, 12, 12) and level.mask.dtype == torch.bool and level.mask.shape == (12, 12, 12)
    assert (level.resolution_x, level.resolution_y, level.resolution_z) == (4.0, 4.0, 4.0) and level.transformation is ref.transformation
    assert 0 < int(level.mask.sum()) < 12 ** 3 and bool(level.mask[6, 6, 6]) and not bool(level.mask[0, 0, 0])
    same = pyramid_level(ref, 0, torch.float64, torch.device("cpu"))
    assert torch.equal(same.image, ref.image) and torch.equal(same.mask, ref.mask)


def test_the_overlap_rule():
    """12^3 voxels of 1 mm against themselves: a shift of 5 voxels keeps 12 x 12 x 7 of the 1728 (more than half), one of 7 keeps
    12 x 12 x 5 (less): its loss is +inf, and 2 inside a difference quotient."""
    from nesvor_amd import align

    image = _rand((12, 12, 12), 8)
    ref, vol = _volume(image), _volume(image.clone())
    counter = [0]
    problem = align._Problem(ref, vol, align.centroid(ref), counter)
    start, near, far = problem.sums([[0.0] * 6, [0.0, 0.0, 0.0, 5.0, 0.0, 0.0], [0.0, 0.0, 0.0, 7.0, 0.0, 0.0]])
    assert counter == [3] and (start[0], near[0], far[0]) == (1728.0, 12 * 12 * 7.0, 12 * 12 * 5.0)
    assert align.loss(start, start[0]) == pytest.approx(0.0, abs=1e-12) and 0 < align.loss(near, start[0]) < 2
    assert align.loss(far, start[0]) == math.inf and align._finite(align.loss(far, start[0])) == 2.0 and align._finite(0.25) == 0.25
    assert align.loss([863.0, 1, 1, 1, 1, 1], 1728.0) == math.inf and align.loss([864.0, 0, 0, 0, 0, 0], 1728.0) == 1.0  # (r = 0: degenerate)
    assert align.correlation(far) < 1 and align.loss(far, 0.0) == 1 - align.correlation(far)
    # the descent does not leave: from a pose next to the edge of the rule it never accepts a pose beyond it
    theta, sums, n0 = align.descend(problem, [0.0, 0.0, 0.0, 4.0, 0.0, 0.0], (3, 4, 5), 4.0, 2, 5)
    assert n0 == 12 * 12 * 8.0 and sums[0] >= 0.5 * n0


# ---------------------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The 8-degree fixture as float32 NIfTI files with mask files of their own (the input's noise is not positive everywhere)."""
    ref, vol, G = fixture(8.0)
    root = tmp_path_factory.mktemp("align")
    paths = {name: str(root / f"{name}.nii.gz") for name in ("ref", "ref_mask", "vol", "vol_mask", "far", "far_mask")}
    for name, v in (("ref", ref), ("vol", vol)):
        _volume(v.image.float(), _pose(dtype=torch.float32), (v.resolution_x,) * 3, v.mask).save(paths[name])
        _volume(v.mask.float(), _pose(dtype=torch.float32), (v.resolution_x,) * 3).save(paths[name + "_mask"])
    _volume(vol.image.float(), _pose(None, (0.0, 1000.0, 0.0), torch.float32), (0.8,) * 3, vol.mask).save(paths["far"])
    _volume(vol.mask.float(), _pose(None, (0.0, 1000.0, 0.0), torch.float32), (0.8,) * 3).save(paths["far_mask"])
    return paths, root


def test_the_command_without_align_is_todays(files, caplog):
    from nesvor_amd import cli
    from nesvor_amd.evaluate import METRICS, evaluate_command, format_table

    paths, root = files
    parser = cli.build_parser()
    argv = ["evaluate", "--reference-volume", paths["ref"], "--reference-mask", paths["ref_mask"], "--input-volumes", paths["vol"],
            "--input-masks", paths["vol_mask"], "--verbose", "0"]
    args = parser.parse_args(argv)
    assert args.align == "none" and args.align_levels == 3 and args.output_aligned is None
    out = str(root / "plain.json")
    sys.modules.pop("nesvor_amd.align", None)
    rows = evaluate_command(_cpu(parser.parse_args(argv + ["--output-json", out])))
    assert "nesvor_amd.align" not in sys.modules  # the module is not even imported
    assert list(rows[0]) == ["input_volume", *METRICS] and all(list(r) == ["input_volume", *METRICS] for r in json.load(open(out)))
    assert "rot deg" not in format_table(rows)
    with pytest.raises(SystemExit, match="--output-aligned needs --align"):
        evaluate_command(_cpu(parser.parse_args(argv + ["--output-aligned", str(root / "a.nii.gz")])))
    with pytest.raises(SystemExit, match="input volumes are different"):
        evaluate_command(_cpu(parser.parse_args(argv + ["--align", "rigid", "--output-aligned", str(root / "a.nii.gz"), str(root / "b.nii.gz")])))
    with pytest.raises(SystemExit):
        parser.parse_args(argv + ["--align", "affine"])
    assert "--align" in cli.__doc__ and "share a world frame" in cli.__doc__


def test_the_command_with_align(files, caplog):
    """``--align rigid`` through files (float32, CPU): the JSON entry, the aligned ``--output-resampled``, the skipped far volume,
    and ``--output-aligned``: `evaluate` without ``--align`` on that file reproduces the aligned comparison.  Measured: n equal,
    PSNR apart by 4.4e-6 dB (28.309889 against 28.309893) - the file's affine is stored in float32 (the NIfTI header's srow), so the second run's index map
    differs from M(theta*) by a few 1e-6 voxels; the bound is 4 x that, DESIGN.md "Rigid alignment"."""
    from nesvor_amd import cli
    from nesvor_amd.evaluate import METRICS, evaluate_command, format_table
    from nesvor_amd.image_io import load_nii_volume

    paths, root = files
    ref, vol, G = fixture(8.0)
    parser = cli.build_parser()
    out, moved, aligned = str(root / "a.json"), [str(root / "m0.nii.gz"), str(root / "m1.nii.gz")], [str(root / "x0.nii.gz"), str(root / "x1.nii.gz")]
    argv = ["evaluate", "--reference-volume", paths["ref"], "--reference-mask", paths["ref_mask"], "--verbose", "0"]
    args = parser.parse_args(argv + ["--input-volumes", paths["vol"], paths["far"], "--input-masks", paths["vol_mask"], paths["far_mask"],
                                     "--align", "rigid", "--output-json", out, "--output-resampled", *moved, "--output-aligned", *aligned])
    assert args.align == "rigid"
    with caplog.at_level("WARNING"):
        rows = evaluate_command(_cpu(args))
    assert "shares no voxel" in caplog.text and paths["far"] in caplog.text
    written = json.load(open(out))
    assert all(list(r) == ["input_volume", *METRICS, "alignment"] for r in written) and "rot deg" in format_table(rows)
    a = written[0]["alignment"]
    assert sorted(a) == sorted(["theta", "matrix", "rotation_deg", "translation_mm", "ncc_before", "ncc_after", "levels", "evaluations", "accepted"])
    mean, worst = tre(ref, a["matrix"], G)
    print(f"command, float32 files: TRE mean {mean:.4f} max {worst:.4f} mm, {a['evaluations']} evaluations, psnr {written[0]['psnr']:.3f}")
    assert mean <= TRE_MEAN and worst <= TRE_MAX and a["accepted"] and a["levels"] == 3 and a["ncc_after"] > a["ncc_before"]
    assert written[0]["ncc"] == pytest.approx(a["ncc_after"], abs=1e-6) and written[0]["coverage"] > 0.99
    far = written[1]
    assert far["n"] == 0 and far["coverage"] == 0 and far["psnr"] is None and not far["alignment"]["accepted"]
    assert far["alignment"]["theta"] == [0.0] * 6 and far["alignment"]["ncc_before"] is None
    # the resampled file is the aligned volume: against the reference it correlates as the report says, not as the unaligned one
    array = torch.tensor(load_nii_volume(moved[0])[0]).double()
    valid = array != 0
    stack = torch.stack([array[valid], ref.image[valid]])
    assert float(torch.corrcoef(stack)[0, 1]) == pytest.approx(written[0]["ncc"], abs=1e-4) and written[0]["ncc"] > 0.95
    plain = evaluate_command(_cpu(parser.parse_args(argv + ["--input-volumes", paths["vol"], "--input-masks", paths["vol_mask"]])))
    assert plain[0]["ncc"] < 0.6 and plain[0]["psnr"] < written[0]["psnr"] - 5
    # the aligned file: the input's own voxels, another pose
    data, res, affine = load_nii_volume(aligned[0])
    own, own_res, own_affine = load_nii_volume(paths["vol"])
    assert torch.equal(torch.tensor(data), torch.tensor(own)) and abs(res - own_res).max() <= 1e-6 and abs(affine - own_affine).max() > 0.1
    from nesvor_amd.evaluate import load_volume

    mask_path = str(root / "x0_mask.nii.gz")
    loaded = load_volume(aligned[0])
    _volume(vol.mask.float(), loaded.transformation, (0.8,) * 3).save(mask_path)
    again = evaluate_command(_cpu(parser.parse_args(argv + ["--input-volumes", aligned[0], "--input-masks", mask_path])))
    assert "alignment" not in again[0]
    print(f"from the aligned file: n {again[0]['n']} (aligned run {rows[0]['n']}), psnr {again[0]['psnr']:.6f} ({rows[0]['psnr']:.6f}), "
          f"difference {abs(again[0]['psnr'] - rows[0]['psnr']):.3e} dB")
    assert abs(again[0]["n"] - rows[0]["n"]) <= 4 * 0 and abs(again[0]["psnr"] - rows[0]["psnr"]) <= 4 * 4.4e-6
