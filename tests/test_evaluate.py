"""Volume comparison on the CPU (nesvor_amd/evaluate.py, composed path; float64 unless said otherwise): the index map and the
resampling on identical, shifted, oblique, smaller and disjoint lattices, the 3-D SSIM against ``F.conv3d``, the intensity fits
and the ``evaluate`` command."""
import json
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _pose(rot=None, t=(0.0, 0.0, 0.0), dtype=torch.float64):
    from nesvor_amd.transform import RigidTransform

    R = torch.eye(3, dtype=torch.float64) if rot is None else rot
    return RigidTransform(torch.cat([R, torch.tensor(t, dtype=torch.float64).view(3, 1)], 1)[None].to(dtype), trans_first=True)


def _rotation(degrees, axis):
    """Rodrigues: the rotation by ``degrees`` about ``axis``, float64."""
    k = torch.tensor(axis, dtype=torch.float64)
    k = k / k.norm()
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], dtype=torch.float64)
    a = math.radians(degrees)
    return torch.eye(3, dtype=torch.float64) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)


def _volume(image, pose=None, res=(1.0, 1.0, 1.0), mask=None):
    from nesvor_amd.image import Volume

    return Volume(image, mask, pose if pose is not None else _pose(), *res)


def _rand(shape, seed):
    return 0.1 + 0.9 * torch.rand(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_identical_lattices_keep_every_voxel_and_score_one():
    """The case eps exists for: an oblique common pose, so that M carries the roundings of R^T R, and no border voxel is lost."""
    from nesvor_amd.evaluate import compare_volumes, index_map

    g = torch.Generator().manual_seed(1)
    image = _rand((7, 9, 11), 0)
    mask_r, mask_x = torch.rand(7, 9, 11, generator=g) < 0.8, torch.rand(7, 9, 11, generator=g) < 0.8
    for rot in (None, _rotation(10.0, (1.0, 2.0, 3.0))):
        pose = _pose(rot, (3.0, -2.0, 0.7))
        ref, vol = _volume(image, pose, (0.8, 0.8, 0.8), mask_r), _volume(image.clone(), pose, (0.8, 0.8, 0.8), mask_x)
        M = index_map(ref, vol)
        assert M.dtype == torch.float64 and M.shape == (3, 4) and float((M - torch.eye(3, 4, dtype=torch.float64)).abs().max()) < 2.0 ** -20
        out = compare_volumes(ref, vol, intensity_fit="none")
        v = mask_r & mask_x
        assert torch.equal(out["valid"], v)  # no border voxel is lost to the roundings of M
        assert out["n"] == int(v.sum()) and out["coverage"] == pytest.approx(int(v.sum()) / int(mask_r.sum())) and not out["fused"]
        if rot is None:  # M is exact
            assert torch.equal(out["resampled"], torch.where(v, image, torch.zeros_like(image)))  # bit for bit
            assert bool((out["ssim_map"][v] == 1).all()) and bool((out["ssim_map"][~v] == 0).all())
            assert out["mse"] == 0 and out["psnr"] == float("inf") and out["ssim"] == 1 and out["mae"] == 0
        else:
            assert float((out["resampled"] - torch.where(v, image, torch.zeros_like(image))).abs().max()) <= 1e-12 and out["mse"] <= 1e-24
    full = compare_volumes(_volume(image, pose), _volume(image.clone(), pose), intensity_fit="none")
    assert bool(full["valid"].all()) and full["n"] == image.numel() and full["coverage"] == 1.0  # all border voxels are kept


def test_a_whole_voxel_shift_through_the_pose():
    from nesvor_amd.evaluate import compare_volumes

    image = _rand((8, 9, 10), 2)
    res = (0.8, 0.8, 0.8)
    sx, sy, sz = 2, -1, 3
    ref = _volume(image, _pose(None, (1.0, 2.0, 3.0)), res)
    vol = _volume(image.clone(), _pose(None, (1.0 + sx * 0.8, 2.0 + sy * 0.8, 3.0 + sz * 0.8)), res)
    out = compare_volumes(ref, vol, intensity_fit="none")
    d, h, w = image.shape
    z, y, x = torch.meshgrid(torch.arange(d), torch.arange(h), torch.arange(w), indexing="ij")
    uz, uy, ux = z - sz, y - sy, x - sx  # a voxel of R is voxel (index - shift) of X
    overlap = (uz >= 0) & (uz < d) & (uy >= 0) & (uy < h) & (ux >= 0) & (ux < w)
    assert torch.equal(out["valid"], overlap) and out["n"] == int(overlap.sum()) == (d - 3) * (h - 1) * (w - 2)
    expect = image[uz.clamp(0, d - 1), uy.clamp(0, h - 1), ux.clamp(0, w - 1)]
    got = out["resampled"]
    assert float((got[overlap] - expect[overlap]).abs().max()) <= 1e-13 and bool((got[~overlap] == 0).all())


def _oblique(shape_r, shape_x, seed=3):
    """R: 1 mm, identity.  X: 0.8 mm voxels, 10 degrees about (1,2,3)/sqrt(14), half a voxel off the centre."""
    ref = _volume(_rand(shape_r, seed), _pose(), (1.0, 1.0, 1.0))
    vol = _volume(_rand(shape_x, seed + 1), _pose(_rotation(10.0, (1.0, 2.0, 3.0)), (0.4, 0.4, 0.4)), (0.8, 0.8, 0.8))
    return ref, vol


def test_oblique_resampling_agrees_with_sample_points():
    """On ``valid`` both are exact trilinear formulas of the same coordinates; only the rounding order differs (1e-13 after the
    coordinate's amplification), so 1e-9 of the largest magnitude leaves three decades."""
    from nesvor_amd.evaluate import compare_volumes

    before = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)  # (Image.resolution_xyz is a tensor of the default dtype)
    try:
        ref, vol = _oblique((12, 13, 14), (16, 17, 18))
        out = compare_volumes(ref, vol, intensity_fit="none")
        sampled = vol.sample_points(ref.xyz_masked).view(ref.image.shape)
    finally:
        torch.set_default_dtype(before)
    v = out["valid"]
    assert sampled.dtype == torch.float64 and 0.3 * v.numel() < int(v.sum()) < v.numel()
    gap = float((out["resampled"][v] - sampled[v]).abs().max())
    print(f"oblique: {int(v.sum())} of {v.numel()} voxels, largest gap to sample_points {gap:.3e}")
    assert gap <= 1e-9 * float(sampled.abs().max())
    assert 0 < out["coverage"] < 1 and math.isfinite(out["psnr"]) and abs(out["ncc"]) <= 1


def test_a_smaller_volume_partly_outside_is_counted_voxel_by_voxel():
    from nesvor_amd.evaluate import EPS, compare_volumes, index_map

    ref, vol = _oblique((8, 9, 10), (5, 6, 4), seed=5)
    vol.transformation = _pose(_rotation(10.0, (1.0, 2.0, 3.0)), (2.1, 0.4, -1.3))
    M = index_map(ref, vol).tolist()
    count = 0
    for z in range(8):
        for y in range(9):
            for x in range(10):
                u = [((M[a][0] * x + M[a][1] * y) + M[a][2] * z) + M[a][3] for a in range(3)]
                count += all(-EPS <= u[a] <= size - 1 + EPS for a, size in enumerate((4, 6, 5)))
    out = compare_volumes(ref, vol)
    assert 0 < count < 720 and out["n"] == count == int(out["valid"].sum()) and out["coverage"] == pytest.approx(count / 720)
    assert out["coverage"] < 1


def test_disjoint_volumes_give_nan_and_no_exception():
    from nesvor_amd.evaluate import compare_volumes

    ref = _volume(_rand((6, 7, 8), 7))
    vol = _volume(_rand((6, 7, 8), 8), _pose(None, (1000.0, 0.0, 0.0)))
    out = compare_volumes(ref, vol)
    assert out["n"] == 0 and out["coverage"] == 0.0 and not bool(out["valid"].any())
    for key in ("ncc", "dynamic_range", "mse", "rmse", "nrmse", "mae", "psnr", "ssim"):
        assert math.isnan(out[key]), key
    assert all(math.isnan(v) for v in out["fit"]) and bool((out["ssim_map"] == 0).all()) and bool((out["resampled"] == 0).all())


def test_without_a_mask_the_interior_is_the_conv3d_gaussian_ssim():
    """More than 5 voxels from every face the zero padding and the renormalisation play no part: the map is the SSIM built from
    ``F.conv3d`` with the outer product of the taps (after tests/test_structural.py's 2-D test)."""
    from nesvor_amd.evaluate import ssim3d_composed
    from nesvor_amd.structural import gaussian_taps

    i, j = _rand((14, 15, 16), 9), _rand((14, 15, 16), 10)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    params = torch.tensor([1.0, 0.0, c1, c2], dtype=torch.float64)
    got, stats = ssim3d_composed(i, j, torch.ones_like(i, dtype=torch.bool), params)
    g = gaussian_taps(torch.float64)
    kernel = (g[:, None, None] * g[None, :, None] * g[None, None, :])[None, None]

    def S(a):
        return F.conv3d(a[None, None], kernel)[0, 0]

    mu_i, mu_j = S(i), S(j)
    var_i, var_j, cov = S(i * i) - mu_i ** 2, S(j * j) - mu_j ** 2, S(i * j) - mu_i * mu_j
    expect = (2 * mu_i * mu_j + c1) * (2 * cov + c2) / ((mu_i ** 2 + mu_j ** 2 + c1) * (var_i + var_j + c2))
    assert expect.shape == (4, 5, 6)
    assert float((got[5:-5, 5:-5, 5:-5] - expect).abs().max()) <= 1e-10
    assert stats[0] == i.numel() and float(stats[1]) == pytest.approx(float(got.sum()), rel=1e-14)
    assert float(stats[2]) == pytest.approx(float(((i - j) ** 2).sum()), rel=1e-14)
    assert float(stats[3]) == pytest.approx(float((i - j).abs().sum()), rel=1e-14)


def test_the_three_intensity_fits():
    from nesvor_amd.evaluate import compare_volumes

    image = _rand((6, 7, 8), 11)
    ref = _volume(image)
    scaled = compare_volumes(ref, _volume(image / 1.3), intensity_fit="scale")
    assert scaled["fit"][0] == pytest.approx(1.3, abs=1e-12) and scaled["fit"][1] == 0 and scaled["mse"] < 1e-28
    plain = compare_volumes(ref, _volume(image / 1.3), intensity_fit="none")
    assert plain["fit"] == [1.0, 0.0] and plain["mse"] == pytest.approx((1 - 1 / 1.3) ** 2 * float((image ** 2).mean()), rel=1e-12)
    assert plain["dynamic_range"] == float(image.max()) and plain["nrmse"] == pytest.approx(plain["rmse"] / plain["dynamic_range"])
    assert plain["psnr"] == pytest.approx(10 * math.log10(plain["dynamic_range"] ** 2 / plain["mse"]))
    assert plain["ncc"] == pytest.approx(1.0, abs=1e-9) and plain["mae"] == pytest.approx((1 - 1 / 1.3) * float(image.mean()), rel=1e-12)
    affine = compare_volumes(ref, _volume((image - 0.2) / 1.3, mask=torch.ones_like(image, dtype=torch.bool)), intensity_fit="affine")
    assert affine["fit"][0] == pytest.approx(1.3, abs=1e-9) and affine["fit"][1] == pytest.approx(0.2, abs=1e-9)
    fixed = compare_volumes(ref, _volume(image / 1.3), intensity_fit="none", dynamic_range=2.0)
    assert fixed["dynamic_range"] == 2.0 and fixed["psnr"] == pytest.approx(10 * math.log10(4.0 / plain["mse"]))
    flat = compare_volumes(ref, _volume(torch.zeros_like(image), mask=torch.ones_like(image, dtype=torch.bool)), intensity_fit="scale")
    assert flat["fit"] == [1.0, 0.0] and flat["ncc"] == 0.0  # degenerate denominators
    with pytest.raises(ValueError, match="intensity fit"):
        compare_volumes(ref, _volume(image), intensity_fit="gamma")


def test_fp32_follows_fp64():
    """The same expressions in float32: close to the yardstick, and of the images' dtype."""
    from nesvor_amd.evaluate import compare_volumes

    ref, vol = _oblique((12, 13, 14), (16, 17, 18))
    exact = compare_volumes(ref, vol)
    ref32, vol32 = _volume(ref.image.float(), ref.transformation), _volume(vol.image.float(), vol.transformation, (0.8, 0.8, 0.8))
    single = compare_volumes(ref32, vol32)
    assert single["resampled"].dtype == single["ssim_map"].dtype == torch.float32 and single["n"] == exact["n"]
    for key in ("ncc", "mse", "mae", "psnr", "ssim"):
        assert single[key] == pytest.approx(exact[key], rel=1e-4), key


def test_the_command(tmp_path, caplog):
    """The 24^3 phantom written with ``Volume.save``, on the host: the rows, their order and keys, null for a non-finite value,
    the map files on the reference's lattice, the warning for a disjoint volume, the list-length errors."""
    from nesvor_amd import cli
    from nesvor_amd.evaluate import METRICS, evaluate_command
    from nesvor_amd.image_io import load_nii_volume
    from nesvor_amd.phantom import phantom3d

    image = torch.tensor(phantom3d(n=24), dtype=torch.float32).clamp(min=0)
    pose = _pose(None, (1.5, -2.0, 0.5), torch.float32)  # (axis-aligned: the index map of two such files is the identity exactly)
    ref_path, same, dim, far = (str(tmp_path / n) for n in ("ref.nii.gz", "same.nii.gz", "dim.nii.gz", "far.nii.gz"))
    _volume(image, pose, (0.8, 0.8, 0.8), image > 0).save(ref_path)
    _volume(image.clone(), pose, (0.8, 0.8, 0.8), image > 0).save(same)
    noisy = (image / 1.3 + 0.01 * torch.rand(image.shape, generator=torch.Generator().manual_seed(0))) * (image > 0)
    _volume(noisy, pose, (0.8, 0.8, 0.8), image > 0).save(dim)
    _volume(image.clone(), _pose(None, (500.0, 0.0, 0.0), torch.float32), (0.8, 0.8, 0.8), image > 0).save(far)
    maps, moved, out = [str(tmp_path / f"s{k}.nii.gz") for k in range(3)], [str(tmp_path / f"r{k}.nii.gz") for k in range(3)], str(tmp_path / "o.json")
    parser = cli.build_parser()
    argv = ["evaluate", "--reference-volume", ref_path, "--input-volumes", same, dim, far, "--intensity-fit", "none", "--verbose", "0"]
    args = parser.parse_args(argv + ["--output-json", out, "--output-ssim-maps", *maps, "--output-resampled", *moved])
    assert args.dynamic_range is None and args.reference_mask is None and args.input_masks is None and args.device is None
    args.device = torch.device("cpu")
    with caplog.at_level("WARNING"):
        rows = evaluate_command(args)
    assert "shares no voxel" in caplog.text and far in caplog.text
    written = json.load(open(out))
    assert [r["input_volume"] for r in written] == [same, dim, far] == [r["input_volume"] for r in rows]
    assert all(list(r) == ["input_volume", *METRICS] for r in written)
    n = int((image > 0).sum())
    assert written[0]["n"] == n and written[0]["mse"] == 0 and written[0]["psnr"] is None and written[0]["ssim"] == 1  # inf -> null
    assert rows[0]["psnr"] == float("inf")
    assert written[1]["n"] == n and written[1]["psnr"] > 5 and 0 < written[1]["ssim"] < 1 and written[1]["ncc"] > 0.99
    assert written[2]["n"] == 0 and written[2]["coverage"] == 0 and all(written[2][k] is None for k in METRICS[2:] if k != "fit")
    assert written[2]["fit"] == [None, None]
    ref_array, ref_res, ref_affine = load_nii_volume(ref_path)
    for path in maps + moved:
        array, res, affine = load_nii_volume(path)
        assert array.shape == ref_array.shape and np.allclose(res, ref_res, atol=1e-5) and np.allclose(affine, ref_affine, atol=1e-4)
    assert np.array_equal(load_nii_volume(moved[0])[0], ref_array) and float(load_nii_volume(maps[0])[0].max()) == 1.0
    fitted = evaluate_command(_cpu(parser.parse_args(["evaluate", "--reference-volume", ref_path, "--input-volumes", dim, "--verbose", "0"])))
    assert fitted[0]["fit"][0] == pytest.approx(1.3, rel=0.02) and fitted[0]["psnr"] > written[1]["psnr"] + 5  # the default: scale
    for extra in (["--output-ssim-maps", maps[0]], ["--output-resampled", *moved[:2]], ["--input-masks", same, dim]):
        with pytest.raises(SystemExit, match="input volumes are different"):
            evaluate_command(_cpu(parser.parse_args(argv + extra)))
    with pytest.raises(SystemExit):
        parser.parse_args(argv + ["--intensity-fit", "gamma"])
    masked = evaluate_command(_cpu(parser.parse_args(["evaluate", "--reference-volume", ref_path, "--reference-mask", ref_path, "--input-volumes",
                                                      same, "--input-masks", same, "--dynamic-range", "2", "--verbose", "0"])))
    assert masked[0]["n"] == n and masked[0]["dynamic_range"] == 2.0
    assert "evaluate" in cli.__doc__ and "share a world frame" in cli.__doc__
    # the whole command line: `evaluate` alone takes --device cpu, the other commands keep their integer index
    out2 = str(tmp_path / "o2.json")
    cli.main(["evaluate", "--reference-volume", ref_path, "--input-volumes", same, dim, far, "--intensity-fit", "none", "--verbose", "0",
              "--device", "cpu", "--output-json", out2])
    assert json.load(open(out2)) == written
    assert parser.parse_args(["evaluate", "--reference-volume", ref_path, "--input-volumes", same, "--device", "1"]).device == 1
    with pytest.raises(SystemExit):
        parser.parse_args(["assess", "--input-stacks", same, "--device", "cpu"])


def _cpu(args):
    args.device = torch.device("cpu")
    return args
