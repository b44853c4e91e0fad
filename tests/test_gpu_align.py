"""Rigid alignment for ``evaluate`` on the GPU: the multi-pose moments kernel of csrc/evaluate.hip against the torch expressions of
nesvor_amd/evaluate.py in fp32 and fp64 and against ``volume_resample``, its independence of what else is in a call, its
refusals, and whole alignments on both paths and through the command line."""
import json

import pytest
import torch

from test_align import TRE_MAX, TRE_MEAN, fixture, tre
from test_evaluate import _pose, _volume
from test_gpu_evaluate import MASKS, VOLUMES, _case
from test_gpu_robust import _ulp

from nesvor_amd.ops import EVALUATE_POSE_CHUNK as P

# (D,H,W): a single voxel; 5^3; one voxel short of a workgroup's chunk, the chunk, one voxel past it; two chunks and a voxel;
# several chunks with rows that are no multiple of 64
SHAPES = [(1, 1, 1), (5, 5, 5), (3, 11, 31), (4, 16, 16), (5, 5, 41), (3, 1, 683), (7, 9, 70)]
NAMES = ("sum I", "sum J", "sum I^2", "sum J^2", "sum I J")
_MAPS = {}


def test_the_shapes_sit_at_the_chunk_edges():
    sizes = [d * h * w for d, h, w in SHAPES]
    assert P == 1024 and sizes[:6] == [1, 125, P - 1, P, P + 1, 2 * P + 1] and sizes[6] > 4 * P and SHAPES[6][2] % 64


def _maps(shape, kind, x_kind, M):
    """K = 16 maps (16,3,4) float64 on the host: the case's own and 15 small perturbations of it (up to 1 % of an entry of the
    linear part, up to half a voxel of the offset)."""
    key = (shape, kind, x_kind)
    if key not in _MAPS:
        g = torch.Generator().manual_seed(sum(shape) + 13 * MASKS.index(kind) + 101 * VOLUMES.index(x_kind))
        noise = torch.rand(16, 3, 4, generator=g, dtype=torch.float64) * 2 - 1
        noise[:, :, :3] *= 0.01
        noise[:, :, 3] *= 0.5
        noise[0] = 0
        _MAPS[key] = M[None] + noise
    return _MAPS[key]


def _flat(maps):
    return maps.reshape(-1).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("x_kind", VOLUMES)
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_kernel_against_the_torch_expressions(device, shape, kind, x_kind):
    """Per pose: n equals the fp32 expression's count (printed where not) and in any case differs from the fp64 expression's by
    no more than the voxels whose interpolated mask is within the fp32 expression's own error of 0.5 (u is double on every path,
    so the inside test is the same); every float sum by the project's rule - the kernel's error against the fp64 expression is
    at most twice the fp32 expression's plus one fp32 ulp of the magnitude; a disjoint volume gives exact zeros; a second call
    is bit-identical.  Pose 0 is the case's own map: there n is ``volume_resample``'s and the sums follow the same rule."""
    from nesvor_amd.evaluate import interpolate_composed, resample_composed

    i0, mask_r, x0, mask_x, M = _case(shape, kind, x_kind, device)
    maps = _maps(shape, kind, x_kind, M)
    sums = torch.ops.nesvor.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps))
    assert sums.shape == (16, 6) and sums.dtype == torch.float64 and sums.device == i0.device
    again = torch.ops.nesvor.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps))
    assert torch.equal(again, sums)
    got = sums.tolist()
    worst = [0.0, 0.0, 0.0]
    for k in range(16):
        s32 = resample_composed(i0, mask_r, x0, mask_x, maps[k])[2][[0, 2, 3, 4, 5, 6]].tolist()
        s64 = resample_composed(i0.double(), mask_r, x0.double(), mask_x, maps[k])[2][[0, 2, 3, 4, 5, 6]].tolist()
        if got[k][0] != s32[0] or got[k][0] != s64[0]:
            _, m32, inside = interpolate_composed(shape, x0, mask_x, maps[k])
            _, m64, _ = interpolate_composed(shape, x0.double(), mask_x, maps[k])
            near = inside & ((m64 - 0.5).abs() <= (m32.double() - m64).abs())
            if mask_r is not None:
                near = near & mask_r
            print(f"{shape} {kind} {x_kind} pose {k}: n {got[k][0]:.0f}, fp32 expression {s32[0]:.0f}, fp64 {s64[0]:.0f}, {int(near.sum())} voxels near 0.5")
            assert abs(got[k][0] - s64[0]) <= int(near.sum())
        if x_kind == "disjoint":
            assert got[k] == [0.0] * 6
        for j, name in enumerate(NAMES, start=1):
            err_k, err_c, ulp = abs(got[k][j] - s64[j]), abs(s32[j] - s64[j]), _ulp(torch.tensor(abs(s64[j])))
            worst = max(worst, [err_k / max(2 * err_c + ulp, 1e-300), err_k, err_c])
            assert err_k <= 2 * err_c + ulp, (k, name, err_k, err_c, ulp)
    print(f"{shape} {kind} {x_kind}: n {got[0][0]:.0f}; largest kernel error / allowed {worst[0]:.3f} (kernel {worst[1]:.3e}, fp32 expression {worst[2]:.3e})")
    stats = torch.ops.nesvor.volume_resample(i0, mask_r, x0, mask_x, _flat(maps[0]))[2]
    assert got[0][0] == float(stats[0])
    s64 = resample_composed(i0.double(), mask_r, x0.double(), mask_x, maps[0])[2]
    s32 = resample_composed(i0, mask_r, x0, mask_x, maps[0])[2]
    for j, col in enumerate((2, 3, 4, 5, 6), start=1):
        for value in (got[0][j], float(stats[col])):  # the two kernels are held to one rule
            assert abs(value - float(s64[col])) <= 2 * abs(float(s32[col] - s64[col])) + _ulp(s64[col].abs())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "random"])
@pytest.mark.parametrize("shape", SHAPES)
def test_a_poses_sums_do_not_depend_on_the_call(device, shape, kind):
    """Every pose of the K = 16 call, alone (K = 1) and inside a K = 12 call at another position, gives the same bits: the
    descent carries a loss over from one call to the next (nesvor_amd/align.py)."""
    i0, mask_r, x0, mask_x, M = _case(shape, kind, "oblique", device)
    maps = _maps(shape, kind, "oblique", M)
    ops = torch.ops.nesvor
    full = ops.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps))
    for k in range(16):
        alone = ops.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps[k:k + 1]))
        assert alone.shape == (1, 6) and torch.equal(alone[0], full[k]), k
    order = [(5 * i + 3) % 16 for i in range(12)]  # pose order[i] at position i: never its own
    assert all(i != k for i, k in enumerate(order))
    for start in (0, 4):
        picked = [(k + start) % 16 for k in order]
        some = ops.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps[picked]))
        assert some.shape == (12, 6) and all(torch.equal(some[i], full[k]) for i, k in enumerate(picked))
    assert shape == (1, 1, 1) or len({tuple(row) for row in full.tolist()}) > 1  # (the poses do differ)


@pytest.mark.gpu
def test_refusals_and_no_ops(device):
    """Every refusal returns before a launch (csrc/evaluate.hip: the checks are the first statements of the entry point), so the
    sentinels in the output stay; K = 0 returns 0 and writes nothing; the workspace size is the documented one."""
    import ctypes

    from nesvor_amd import _lib

    lib = _lib.load()
    shape = (5, 5, 41)
    d, h, w = shape
    i0, mask_r, x0, mask_x, M = _case(shape, "random", "oblique", device)
    maps = _maps(shape, "random", "oblique", M)
    xd, xh, xw = x0.shape
    ptr = _lib.ptr
    K = 16
    nbytes = int(lib.nesvor_volume_pose_moments_workspace_bytes(d, h, w, K))
    assert nbytes == 48 * K * 2 == 8 * 6 * K * ((d * h * w + P - 1) // P)
    assert lib.nesvor_volume_pose_moments_workspace_bytes(4, 16, 16, 1) == 48 and lib.nesvor_volume_pose_moments_workspace_bytes(3, 1, 683, 12) == 48 * 12 * 3
    assert lib.nesvor_volume_pose_moments_workspace_bytes(1, 1, 2 ** 31 - 257, 16) == 48 * 16 * 2 ** 21
    for bad in ((0, h, w, 1), (d, 0, w, 1), (d, h, -1, 1), (65536, 65536, 1, 1), (1, 1, 2 ** 31 - 256, 1), (d, h, w, 0), (d, h, w, 17), (d, h, w, -1)):
        assert lib.nesvor_volume_pose_moments_workspace_bytes(*bad) == 0, bad
    sums = torch.full((K, 6), -7.0, dtype=torch.float64, device=device)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)

    def run(d_=d, h_=h, w_=w, xd_=xd, xh_=xh, xw_=xw, ref_=i0, vol_=x0, maps_=_flat(maps), K_=K, sums_=sums, ws_=ws, nb=nbytes, no_maps=False):
        m = None if no_maps else (ctypes.c_double * max(len(maps_), 1))(*maps_)
        return lib.nesvor_volume_pose_moments(ptr(ref_), ptr(mask_r), d_, h_, w_, ptr(vol_), ptr(mask_x), xd_, xh_, xw_, m, K_, ptr(sums_),
                                              ptr(ws_), nb, _lib.stream_ptr())

    assert run(K_=17, maps_=_flat(maps) + [0.0] * 12) != 0 and run(K_=-1) != 0
    assert run(nb=nbytes - 1) != 0 and run(nb=0) != 0 and run(ws_=None) != 0  # a short or missing workspace
    assert run(d_=0) != 0 and run(h_=-2) != 0 and run(w_=0) != 0 and run(xd_=0) != 0 and run(xh_=0) != 0 and run(xw_=-1) != 0
    assert run(d_=65536, h_=65536, w_=1) != 0 and run(xd_=1, xh_=1, xw_=2 ** 31 - 256) != 0  # more than INT_MAX - 256 voxels
    for name in ("ref_", "vol_", "sums_"):
        assert run(**{name: None}) != 0, name
    assert run(no_maps=True) != 0
    for bad in (float("inf"), float("-inf"), float("nan")):
        for k in (0, 7, 12 * K - 1):
            entries = _flat(maps)
            entries[k] = bad
            assert run(maps_=entries) != 0, (k, bad)
    assert run(K_=0) == 0 and run(K_=0, ws_=None, nb=0, no_maps=True, sums_=None) == 0  # nothing to do: nothing is needed
    torch.cuda.synchronize()
    assert bool((sums == -7.0).all())
    assert run() == 0
    torch.cuda.synchronize()
    direct = torch.ops.nesvor.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps))
    assert torch.equal(sums, direct)
    sums.fill_(-7.0)
    assert run(K_=3) == 0  # a workspace larger than needed is fine, and only three rows are written
    torch.cuda.synchronize()
    assert torch.equal(sums[:3], direct[:3]) and bool((sums[3:] == -7.0).all())


@pytest.mark.gpu
def test_argument_errors_byte_masks_and_the_meta_kernel(device):
    i0, mask_r, x0, mask_x, M = _case((5, 5, 41), "random", "oblique", device)
    maps = _maps((5, 5, 41), "random", "oblique", M)
    ops = torch.ops.nesvor
    flat = _flat(maps[:2])
    sums = ops.volume_pose_moments(i0, mask_r, x0, mask_x, flat)
    assert torch.equal(ops.volume_pose_moments(i0, mask_r.to(torch.uint8) * 7, x0, mask_x.to(torch.uint8), flat), sums)
    assert ops.volume_pose_moments(i0, mask_r, x0, mask_x, []).shape == (0, 6)
    meta = ops.volume_pose_moments(i0.to("meta"), None, x0.to("meta"), None, flat)
    assert meta.shape == (2, 6) and meta.dtype == torch.float64 and meta.device.type == "meta"
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::volume_pose_moments'"):
        ops.volume_pose_moments(i0.cpu(), mask_r.cpu(), x0.cpu(), mask_x.cpu(), flat)
    with pytest.raises(RuntimeError, match="torch.float32"):
        ops.volume_pose_moments(i0.double(), mask_r, x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.volume_pose_moments(i0.transpose(0, 1), None, x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.volume_pose_moments(i0, mask_r[1:].contiguous(), x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="12 entries"):
        ops.volume_pose_moments(i0, mask_r, x0, mask_x, flat[:13])
    with pytest.raises(RuntimeError, match="12 entries"):
        ops.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps) + flat[:12])  # 17 maps
    with pytest.raises(RuntimeError, match="HIP error"):
        ops.volume_pose_moments(i0, mask_r, x0, mask_x, [float("nan")] + flat[1:])


@pytest.mark.gpu
def test_pose_moments_takes_more_than_one_launch_worth_of_maps(device, monkeypatch):
    from nesvor_amd import align

    monkeypatch.delenv("NESVOR_EVALUATE", raising=False)
    i0, mask_r, x0, mask_x, M = _case((5, 5, 41), "random", "oblique", device)
    maps = _maps((5, 5, 41), "random", "oblique", M)
    many = torch.cat([maps, maps[:5].flip(0)])
    direct = torch.ops.nesvor.volume_pose_moments(i0, mask_r, x0, mask_x, _flat(maps))
    out = align.pose_moments(i0, mask_r, x0, mask_x, many)
    assert out.shape == (21, 6) and torch.equal(out[:16], direct) and torch.equal(out[16:], direct[:5].flip(0))
    monkeypatch.setenv("NESVOR_EVALUATE", "composed")
    composed = align.pose_moments(i0, mask_r, x0, mask_x, many)
    assert torch.equal(composed, align.pose_moments_composed(i0, mask_r, x0, mask_x, many)) and torch.equal(composed[:, 0], out[:, 0])


# ---------------------------------------------------------------------------------------------------------------------
# whole alignments
# ---------------------------------------------------------------------------------------------------------------------
def _on(device, volume):
    return _volume(volume.image.to(device), volume.transformation, (volume.resolution_x, volume.resolution_y, volume.resolution_z), volume.mask.to(device))


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_recovery_on_the_gpu(device, monkeypatch, path):
    """The 15-degree fixture in fp32 on the device, both paths within the bound of tests/test_align.py; the fused run never
    evaluates the torch expressions during the descent.  Measured on MI355X: DESIGN.md, "Rigid alignment"."""
    from nesvor_amd import align, evaluate

    ref, vol, G = fixture(15.0, torch.float32)
    ref, vol = _on(device, ref), _on(device, vol)
    calls = []
    for module, name in ((align, "pose_moments_composed"), (evaluate, "resample_composed")):
        inner = getattr(module, name)
        monkeypatch.setattr(module, name, lambda *a, _inner=inner, _name=name: calls.append(_name) or _inner(*a))
    if path == "composed":
        monkeypatch.setenv("NESVOR_EVALUATE", "composed")
    else:
        monkeypatch.delenv("NESVOR_EVALUATE", raising=False)
    out = align.align_volumes(ref, vol, "rigid")
    mean, worst = tre(ref, out["matrix"], G)
    print(f"{path}: TRE mean {mean:.4f} max {worst:.4f} mm; ncc {out['ncc_before']:.4f} -> {out['ncc_after']:.4f}; {out['evaluations']} pose "
          f"evaluations; {len(calls)} calls of the torch expressions")
    assert mean <= TRE_MEAN and worst <= TRE_MAX and out["accepted"] and out["levels"] == 3 and out["ncc_after"] > out["ncc_before"]
    if path == "fused":
        assert not calls
    else:
        assert calls.count("resample_composed") == out["evaluations"] and "pose_moments_composed" in calls


@pytest.mark.gpu
def test_cli_evaluate_align_rigid(tmp_path, device, monkeypatch):
    from nesvor_amd import align, cli, evaluate

    monkeypatch.delenv("NESVOR_EVALUATE", raising=False)

    def refuse(*a, **k):
        raise AssertionError("the command on the GPU takes the fused path")

    monkeypatch.setattr(evaluate, "resample_composed", refuse)
    monkeypatch.setattr(align, "pose_moments_composed", refuse)
    ref, vol, G = fixture(15.0, torch.float32)
    paths = {name: str(tmp_path / f"{name}.nii.gz") for name in ("ref", "ref_mask", "vol", "vol_mask", "aligned")}
    for name, v in (("ref", ref), ("vol", vol)):
        _volume(v.image, _pose(dtype=torch.float32), (v.resolution_x,) * 3, v.mask).save(paths[name])
        _volume(v.mask.float(), _pose(dtype=torch.float32), (v.resolution_x,) * 3).save(paths[name + "_mask"])
    out = str(tmp_path / "o.json")
    argv = ["evaluate", "--reference-volume", paths["ref"], "--reference-mask", paths["ref_mask"], "--input-volumes", paths["vol"],
            "--input-masks", paths["vol_mask"], "--verbose", "0", "--device", "0"]
    cli.main(argv + ["--align", "rigid", "--output-json", out, "--output-aligned", paths["aligned"]])
    row = json.load(open(out))[0]
    a = row["alignment"]
    mean, worst = tre(ref, a["matrix"], G)
    print(f"command: TRE mean {mean:.4f} max {worst:.4f} mm, rotation {a['rotation_deg']:.3f} degrees, psnr {row['psnr']:.3f}, ncc {row['ncc']:.4f}")
    assert mean <= TRE_MEAN and worst <= TRE_MAX and a["accepted"] and a["rotation_deg"] == pytest.approx(15.0, abs=0.5)
    assert row["ncc"] == pytest.approx(a["ncc_after"], abs=1e-5) and row["ncc"] > 0.95 and row["coverage"] > 0.99
    plain = str(tmp_path / "p.json")
    cli.main(argv + ["--output-json", plain])
    before = json.load(open(plain))[0]
    assert "alignment" not in before and before["ncc"] < 0.6 and before["psnr"] < row["psnr"] - 5
