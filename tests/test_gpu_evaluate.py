"""Volume comparison on the GPU: the two kernels of csrc/evaluate.hip against the torch expressions of nesvor_amd/evaluate.py in
fp32 and fp64, their refusals, ``compare_volumes`` on both paths and the ``evaluate`` command."""
import json
import math

import pytest
import torch

from test_evaluate import _pose, _rotation, _volume
from test_gpu_robust import _ulp

from nesvor_amd.ops import EVALUATE_Z_CHUNK as C

# (D,H,W): a single voxel; below the window's radius; exactly one tile and one window; one past a tile edge both ways; one plane
# past a chunk boundary, once and twice
SHAPES = [(1, 1, 1), (5, 5, 5), (11, 16, 16), (12, 17, 33), (C + 1, 19, 23), (2 * C + 1, 5, 70)]
MASKS = ["none", "random", "plane"]
VOLUMES = ["same", "oblique", "anisotropic", "disjoint"]
_CASES = {}


def _mask(shape, kind, g):
    if kind == "none":
        return None
    m = torch.rand(*shape, generator=g) < 0.7
    if kind == "plane":
        m[shape[0] // 2] = False
    return m


def _case(shape, kind, x_kind, device):
    """(I0, maskR, X0, maskX, M) on the device (M: host); shared by the tests and never written."""
    from nesvor_amd.evaluate import index_map

    key = (shape, kind, x_kind)
    if key not in _CASES:
        d, h, w = shape
        g = torch.Generator().manual_seed(1000 * d + 10 * h + w + 7 * VOLUMES.index(x_kind))
        if x_kind == "same":
            x_shape, x_pose, x_res = shape, _pose(), (1.0, 1.0, 1.0)
        elif x_kind == "oblique":  # 0.8 mm voxels, 10 degrees about (1,2,3)/sqrt(14), half a voxel off the centre
            x_shape, x_pose, x_res = tuple(int(s / 0.8) + 2 for s in shape), _pose(_rotation(10.0, (1.0, 2.0, 3.0)), (0.4, 0.4, 0.4)), (0.8, 0.8, 0.8)
        elif x_kind == "anisotropic":
            x_shape, x_pose, x_res = ((d + 2) // 3 + 1, h, w + 1), _pose(None, (0.25, 0.0, 0.5)), (1.0, 1.0, 3.0)
        else:
            x_shape, x_pose, x_res = shape, _pose(None, (0.0, 1000.0, 0.0)), (1.0, 1.0, 1.0)
        i0 = 0.1 + 0.9 * torch.rand(*shape, generator=g)
        x0 = 0.1 + 0.9 * torch.rand(*x_shape, generator=g)
        if x_kind == "same":
            x0 = (i0 + 0.05 * torch.randn(*shape, generator=g)) / 1.2
        mask_r, mask_x = _mask(shape, kind, g), _mask(x_shape, "none" if kind == "none" else "random", g)
        M = index_map(_volume(i0, _pose(), (1.0, 1.0, 1.0)), _volume(x0, x_pose, x_res))
        _CASES[key] = tuple(None if t is None else t.to(device) for t in (i0, mask_r, x0, mask_x)) + (M,)
    return _CASES[key]


# ---------------------------------------------------------------------------------------------------------------------
# the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("x_kind", VOLUMES)
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("shape", SHAPES)
def test_both_passes_against_the_torch_expressions(device, shape, kind, x_kind):
    """Resampling: ``valid`` and J0 bit-equal to the fp32 expression (printed where not), and in any case held to the fp64
    expression: ``valid`` differs only where |mX64 - 0.5| is within the fp32 expression's own error there (u is double on every
    path, so the inside test is the same), J0's largest error is at most twice the fp32 expression's plus one fp32 ulp of the
    largest magnitude; n, n_ref and max I exact.  SSIM map and every float sum: the project's rule (tests/test_gpu_structural.py):
    the kernel's largest error against the fp64 expression is at most twice the fp32 expression's plus one fp32 ulp of the largest
    magnitude; the map exactly 0 off v; a second call bit-identical.  Measured on MI355X: DESIGN.md, "Volume comparison"."""
    from nesvor_amd.evaluate import fit_from_sums, interpolate_composed, resample_composed, ssim3d_composed

    i0, mask_r, x0, mask_x, M = _case(shape, kind, x_kind, device)
    flat = M.reshape(12).tolist()
    j, v, s = torch.ops.nesvor.volume_resample(i0, mask_r, x0, mask_x, flat)
    assert j.shape == v.shape == i0.shape and j.dtype == torch.float32 and v.dtype == torch.bool and s.shape == (8,) and s.dtype == torch.float64
    j32, v32, s32 = resample_composed(i0, mask_r, x0, mask_x, M)
    j64, v64, s64 = resample_composed(i0.double(), mask_r, x0.double(), mask_x, M)
    equal = torch.equal(v, v32) and torch.equal(j, j32)
    print(f"{shape} {kind} {x_kind}: n {int(s[0])} of {int(s[1])}; valid and J0 bit-equal to the fp32 expression: {equal}")
    _, m32, inside32 = interpolate_composed(shape, x0, mask_x, M)
    _, m64, inside64 = interpolate_composed(shape, x0.double(), mask_x, M)
    assert torch.equal(inside32, inside64)
    near = (m64 - 0.5).abs() <= (m32.double() - m64).abs()
    assert not bool(((v != v64) & ~near).any())
    both = v & v64
    err_k, err_c = (float((a.double() - j64)[both].abs().max()) if bool(both.any()) else 0.0 for a in (j, j32))
    bound = 2 * err_c + _ulp(j64.abs().max())
    print(f"    J0: kernel {err_k:.3e} composed {err_c:.3e} allowed {bound:.3e}")
    assert err_k <= bound and bool((j[~v] == 0).all())
    n_ref = float(i0.numel() if mask_r is None else mask_r.sum())
    assert float(s[0]) == float(v.sum()) and float(s[1]) == n_ref
    assert float(s[7]) == (float(i0[v].max()) if bool(v.any()) else -math.inf)
    if x_kind == "disjoint":
        assert float(s[0]) == 0
    if x_kind == "same":
        assert torch.equal(v, torch.ones_like(v) if mask_r is None else mask_r & mask_x) and torch.equal(j, torch.where(v, x0, torch.zeros_like(x0)))
    names = ("sum I", "sum J", "sum I^2", "sum J^2", "sum I J")
    for k, name in enumerate(names, start=2):
        err_k, err_c, ulp = abs(float(s[k] - s64[k])), abs(float(s32[k] - s64[k])), _ulp(s64[k].abs())
        print(f"    {name}: kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e}")
        assert err_k <= 2 * err_c + ulp, name
    again = torch.ops.nesvor.volume_resample(i0, mask_r, x0, mask_x, flat)
    assert all(torch.equal(a, b) for a, b in zip(again, (j, v, s)))

    # the second pass on the kernel's own J0 and v, so that the three evaluations see the same inputs
    r, a, b, L = fit_from_sums(s, "affine" if x_kind == "oblique" else "scale", None if kind == "none" else 1.0)
    L = torch.where(torch.isfinite(L), L, torch.ones_like(L))  # (no valid voxel: max I = -inf)
    params = torch.stack([a, b, (0.01 * L) ** 2, (0.03 * L) ** 2]).float()
    m, t = torch.ops.nesvor.volume_ssim(i0, j, v, params)
    assert m.shape == i0.shape and m.dtype == torch.float32 and t.shape == (4,) and t.dtype == torch.float64
    m32, t32 = ssim3d_composed(i0, j, v, params)
    m64, t64 = ssim3d_composed(i0.double(), j.double(), v, params.double())
    err_k, err_c = float((m.double() - m64).abs().max()), float((m32.double() - m64).abs().max())
    bound = 2 * err_c + _ulp(m64.abs().max())
    print(f"    ssim map: kernel {err_k:.3e} composed {err_c:.3e} allowed {bound:.3e} (bit-equal to composed: {torch.equal(m, m32)})")
    assert err_k <= bound
    assert bool((m[~v] == 0).all()) and float(t[0]) == float(v.sum())
    for k, name in ((1, "sum ssim"), (2, "sum e^2"), (3, "sum |e|")):
        err_k, err_c, ulp = abs(float(t[k] - t64[k])), abs(float(t32[k] - t64[k])), _ulp(t64[k].abs())
        print(f"    {name}: kernel {err_k:.3e} composed {err_c:.3e} ulp {ulp:.3e} (value {float(t64[k]):.4e})")
        assert err_k <= 2 * err_c + ulp, name
    again = torch.ops.nesvor.volume_ssim(i0, j, v, params)
    assert torch.equal(again[0], m) and torch.equal(again[1], t)


@pytest.mark.gpu
def test_byte_masks_and_meta_kernels(device):
    i0, mask_r, x0, mask_x, M = _case(SHAPES[3], "random", "oblique", device)
    flat = M.reshape(12).tolist()
    j, v, s = torch.ops.nesvor.volume_resample(i0, mask_r, x0, mask_x, flat)
    j8, v8, s8 = torch.ops.nesvor.volume_resample(i0, mask_r.to(torch.uint8) * 7, x0, mask_x.to(torch.uint8), flat)
    assert torch.equal(j8, j) and torch.equal(v8, v) and torch.equal(s8, s)
    params = torch.tensor([1.1, 0.01, 1e-4, 9e-4], device=device)
    m, t = torch.ops.nesvor.volume_ssim(i0, j, v, params)
    m8, t8 = torch.ops.nesvor.volume_ssim(i0, j, v.to(torch.uint8), params)
    assert torch.equal(m8, m) and torch.equal(t8, t)
    meta = torch.ops.nesvor.volume_resample(i0.to("meta"), None, x0.to("meta"), None, flat)
    assert meta[0].shape == i0.shape and meta[0].dtype == torch.float32 and meta[1].dtype == torch.bool and meta[1].shape == i0.shape
    assert meta[2].shape == (8,) and meta[2].dtype == torch.float64 and meta[0].device.type == "meta"
    meta = torch.ops.nesvor.volume_ssim(i0.to("meta"), j.to("meta"), v.to("meta"), params.to("meta"))
    assert meta[0].shape == i0.shape and meta[0].dtype == torch.float32 and meta[1].shape == (4,) and meta[1].dtype == torch.float64


@pytest.mark.gpu
def test_refusals(device):
    """Every refusal returns before a launch (csrc/evaluate.hip: the checks are the first statements of both entry points), so
    the sentinels in the outputs stay; the workspace sizes are the documented ones."""
    import ctypes

    from nesvor_amd import _lib

    lib = _lib.load()
    shape = (C + 1, 19, 23)
    d, h, w = shape
    i0, mask_r, x0, mask_x, M = _case(shape, "random", "oblique", device)
    xd, xh, xw = x0.shape
    P = _lib.ptr
    out = torch.full(shape, -7.0, device=device)
    valid = torch.full(shape, 9, dtype=torch.uint8, device=device)
    stats = torch.full((8,), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_volume_resample_workspace_bytes(d, h, w))
    assert nbytes == 8 * 8 * ((d * h * w + 255) // 256)
    for bad in ((0, h, w), (d, 0, w), (d, h, -1), (65536, 65536, 1), (1, 1, 2 ** 31 - 256)):
        assert lib.nesvor_volume_resample_workspace_bytes(*bad) == 0 and lib.nesvor_volume_ssim_workspace_bytes(*bad) == 0
    assert lib.nesvor_volume_resample_workspace_bytes(1, 1, 2 ** 31 - 257) == 8 * 8 * (2 ** 23 - 1)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)

    def resample(d_=d, h_=h, w_=w, xd_=xd, xh_=xh, xw_=xw, ref_=i0, vol_=x0, M_=M.reshape(12).tolist(), out_=out, valid_=valid, stats_=stats,
                 ws_=ws, nb=nbytes, no_map=False):
        m = None if no_map else (ctypes.c_double * 12)(*M_)
        return lib.nesvor_volume_resample(P(ref_), P(mask_r), d_, h_, w_, P(vol_), P(mask_x), xd_, xh_, xw_, m, P(out_), P(valid_),
                                          P(stats_), P(ws_), nb, _lib.stream_ptr())

    assert resample(nb=nbytes - 1) != 0 and resample(nb=0) != 0 and resample(ws_=None) != 0  # a short or missing workspace
    assert resample(d_=0) != 0 and resample(h_=-2) != 0 and resample(w_=0) != 0 and resample(xd_=0) != 0 and resample(xh_=0) != 0 and resample(xw_=-1) != 0
    assert resample(d_=65536, h_=65536, w_=1) != 0 and resample(xd_=1, xh_=1, xw_=2 ** 31 - 256) != 0  # more than INT_MAX - 256 voxels
    for name in ("ref_", "vol_", "out_", "valid_", "stats_"):
        assert resample(**{name: None}) != 0, name
    assert resample(no_map=True) != 0
    for bad in (float("inf"), float("-inf"), float("nan")):
        for k in (0, 7, 11):
            entries = M.reshape(12).tolist()
            entries[k] = bad
            assert resample(M_=entries) != 0, (k, bad)
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((valid == 9).all()) and bool((stats == -7.0).all())
    assert resample() == 0
    torch.cuda.synchronize()
    direct = torch.ops.nesvor.volume_resample(i0, mask_r, x0, mask_x, M.reshape(12).tolist())
    assert torch.equal(out, direct[0]) and torch.equal(valid.bool(), direct[1]) and torch.equal(stats, direct[2]) and int(valid.max()) == 1

    j, v = direct[0], direct[1]
    params = torch.tensor([1.0, 0.0, 1e-4, 9e-4], device=device)
    ssim = torch.full(shape, -7.0, device=device)
    sums = torch.full((4,), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_volume_ssim_workspace_bytes(d, h, w))
    assert nbytes == 8 * 4 * 2 * 2 * 2  # two chunks of 2 x 2 tiles
    assert lib.nesvor_volume_ssim_workspace_bytes(C, 16, 16) == 32 and lib.nesvor_volume_ssim_workspace_bytes(2 * C + 1, 5, 70) == 32 * 3 * 5
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)

    def run(d_=d, h_=h, w_=w, ref_=i0, res_=j, valid_=v, params_=params, out_=ssim, stats_=sums, ws_=ws, nb=nbytes):
        return lib.nesvor_volume_ssim(P(ref_), P(res_), P(valid_), P(params_), d_, h_, w_, P(out_), P(stats_), P(ws_), nb, _lib.stream_ptr())

    assert run(nb=nbytes - 1) != 0 and run(nb=0) != 0 and run(ws_=None) != 0
    assert run(d_=0) != 0 and run(h_=0) != 0 and run(w_=-3) != 0 and run(d_=65536, h_=65536, w_=1) != 0 and run(d_=1, h_=1, w_=2 ** 31 - 256) != 0
    for name in ("ref_", "res_", "valid_", "params_", "out_", "stats_"):
        assert run(**{name: None}) != 0, name
    torch.cuda.synchronize()
    assert bool((ssim == -7.0).all()) and bool((sums == -7.0).all())
    assert run() == 0
    torch.cuda.synchronize()
    direct = torch.ops.nesvor.volume_ssim(i0, j, v, params)
    assert torch.equal(ssim, direct[0]) and torch.equal(sums, direct[1])


@pytest.mark.gpu
def test_argument_errors(device):
    i0, mask_r, x0, mask_x, M = _case(SHAPES[3], "random", "oblique", device)
    flat = M.reshape(12).tolist()
    ops = torch.ops.nesvor
    j, v, _ = ops.volume_resample(i0, mask_r, x0, mask_x, flat)
    params = torch.tensor([1.0, 0.0, 1e-4, 9e-4], device=device)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::volume_resample'"):
        ops.volume_resample(i0.cpu(), mask_r.cpu(), x0.cpu(), mask_x.cpu(), flat)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::volume_ssim'"):
        ops.volume_ssim(i0.cpu(), j.cpu(), v.cpu(), params.cpu())
    with pytest.raises(RuntimeError, match="torch.float32"):
        ops.volume_resample(i0.double(), mask_r, x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="torch.float32"):
        ops.volume_resample(i0, mask_r, x0.half(), mask_x, flat)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.volume_resample(i0.transpose(0, 1), None, x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        ops.volume_resample(i0, mask_r.float(), x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.volume_resample(i0, mask_r[1:].contiguous(), x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.volume_resample(i0[0], None, x0, mask_x, flat)
    with pytest.raises(RuntimeError, match="12 entries"):
        ops.volume_resample(i0, mask_r, x0, mask_x, flat[:9])
    with pytest.raises(RuntimeError, match="HIP error"):
        ops.volume_resample(i0, mask_r, x0, mask_x, [float("nan")] + flat[1:])
    with pytest.raises(RuntimeError, match="torch.float32"):
        ops.volume_ssim(i0, j.double(), v, params)
    with pytest.raises(RuntimeError, match="torch.float32"):
        ops.volume_ssim(i0, j, v, params.double())
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.volume_ssim(i0, j.transpose(1, 2), v, params)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        ops.volume_ssim(i0, j, v.float(), params)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.volume_ssim(i0, j[1:].contiguous(), v, params)
    with pytest.raises(RuntimeError, match="one shape"):
        ops.volume_ssim(i0, j, v[1:].contiguous(), params)
    with pytest.raises(RuntimeError, match="four floats"):
        ops.volume_ssim(i0, j, v, params[:3].contiguous())


# ---------------------------------------------------------------------------------------------------------------------
# compare_volumes on both paths
# ---------------------------------------------------------------------------------------------------------------------
def _volumes(device, shape=(C + 1, 19, 23)):
    i0, mask_r, x0, mask_x, _ = _case(shape, "random", "oblique", device)
    ref = _volume(i0, _pose(), (1.0, 1.0, 1.0), mask_r)
    vol = _volume(x0, _pose(_rotation(10.0, (1.0, 2.0, 3.0)), (0.4, 0.4, 0.4)), (0.8, 0.8, 0.8), mask_x)
    return ref, vol


@pytest.mark.gpu
def test_fused_compare_follows_the_composed_one(device, monkeypatch):
    from nesvor_amd import evaluate

    ref, vol = _volumes(device)
    calls = []
    for name in ("resample_composed", "ssim3d_composed"):
        inner = getattr(evaluate, name)
        monkeypatch.setattr(evaluate, name, lambda *a, _inner=inner, _name=name: calls.append(_name) or _inner(*a))
    for fit in evaluate.FITS:
        monkeypatch.delenv("NESVOR_EVALUATE", raising=False)
        del calls[:]
        fused = evaluate.compare_volumes(ref, vol, fit)
        assert not calls and fused["fused"]  # the fused path never evaluates the torch expressions
        monkeypatch.setenv("NESVOR_EVALUATE", "composed")
        composed = evaluate.compare_volumes(ref, vol, fit)
        assert calls == ["resample_composed", "ssim3d_composed"] and not composed["fused"]
        assert fused["n"] == composed["n"] > 1000
        print(fit, {k: fused[k] for k in evaluate.METRICS})
        for key in evaluate.METRICS[1:]:
            for a, b in zip(*([fused[key], composed[key]] if key == "fit" else [[fused[key]], [composed[key]]])):
                assert math.isfinite(a) and math.isfinite(b) and abs(a - b) <= 1e-5 * max(abs(b), 1e-30) + (1e-12 if key == "fit" else 0), (fit, key, a, b)
    monkeypatch.delenv("NESVOR_EVALUATE")
    far = _volume(vol.image, _pose(None, (0.0, 1000.0, 0.0)), (0.8, 0.8, 0.8), vol.mask)
    empty = evaluate.compare_volumes(ref, far)
    assert empty["n"] == 0 and empty["coverage"] == 0 and all(math.isnan(empty[k]) for k in ("ncc", "mse", "psnr", "ssim", "mae", "nrmse"))
    same = evaluate.compare_volumes(ref, _volume(ref.image.clone(), _pose(), (1.0, 1.0, 1.0), ref.mask), "none")
    assert same["mse"] == 0 and same["psnr"] == math.inf and same["coverage"] == 1 and same["ssim"] == pytest.approx(1.0, abs=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["fused", "composed"])
def test_a_comparison_reads_nothing_back_before_the_report(device, monkeypatch, path):
    """Both passes and the report's arithmetic under torch's synchronisation check (after
    tests/test_gpu_structural.py::test_an_update_reads_nothing_back_to_the_host); the report itself is the one read."""
    from nesvor_amd import evaluate

    ref, vol = _volumes(device)
    if path == "composed":
        monkeypatch.setenv("NESVOR_EVALUATE", "composed")
    else:
        monkeypatch.delenv("NESVOR_EVALUATE", raising=False)
    M = evaluate.index_map(ref, vol)  # (the poses live on the host)
    args = (ref.image, ref.mask, vol.image, vol.mask, M)
    evaluate.compare_tensors(*args)  # (warm: the library is loaded, the allocator has its blocks)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [evaluate.compare_tensors(*args, fit, L) for fit, L in (("scale", None), ("affine", 1.0), ("none", None))]
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert all(o["packed"].shape == (12,) and bool(torch.isfinite(o["packed"]).all()) for o in outs)
    with pytest.raises(RuntimeError):  # the check is live: the report's read does raise under it
        torch.cuda.set_sync_debug_mode("error")
        try:
            evaluate.compare_volumes(ref, vol)
        finally:
            torch.cuda.set_sync_debug_mode(before)


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_evaluate_two_lattices(tmp_path, device, monkeypatch):
    from nesvor_amd import cli, evaluate
    from nesvor_amd.image_io import load_nii_volume

    monkeypatch.delenv("NESVOR_EVALUATE", raising=False)

    def refuse(*a, **k):
        raise AssertionError("the command on the GPU takes the fused path")

    monkeypatch.setattr(evaluate, "resample_composed", refuse)
    monkeypatch.setattr(evaluate, "ssim3d_composed", refuse)
    # A Gaussian blob (sigma 5 mm) on a 24^3 lattice of 1 mm, taken to two other lattices of the same world frame by
    # ``Volume.resample`` - 0.8 mm world-aligned, and 0.8 mm tilted by 10 degrees, that one also dimmed by 1.25 - and compared on the
    # voxels at least 2 mm from every face (there no corner of either interpolation is off the first lattice).  Trilinear
    # interpolation of f errs by at most sum_axes h^2 / 8 max|f_aa| = 3 h^2 / (8 sigma^2): 0.015 going to the 0.8 mm lattice and
    # 0.0096 + 0.015 coming back (the first error is carried by a convex combination), so |e| <= 0.0246 at every compared voxel
    # for the gain 1 (1.25); the fitted gain only lowers the mean square.
    n, sigma, bound = 24, 5.0, 0.0246
    axis = torch.arange(n, dtype=torch.float32) - (n - 1) / 2
    image = torch.exp(-(axis[:, None, None] ** 2 + axis[None, :, None] ** 2 + axis[None, None, :] ** 2) / (2 * sigma * sigma))
    pose = _pose(None, (1.0, 2.0, -1.0), torch.float32)
    truth = _volume(image, pose, (1.0, 1.0, 1.0))
    interior = torch.zeros_like(image)
    interior[2:-2, 2:-2, 2:-2] = 1
    paths = [str(tmp_path / name) for name in ("ref.nii.gz", "fine.nii.gz", "tilted.nii.gz", "interior.nii.gz")]
    truth.save(paths[0])
    _volume(interior, pose, (1.0, 1.0, 1.0)).save(paths[3])
    fine = truth.resample(0.8, None)
    tilted = truth.resample(0.8, _pose(_rotation(10.0, (1.0, 2.0, 3.0)), (0.0, 0.0, 0.0), torch.float32))
    fine.save(paths[1])
    tilted.image = tilted.image / 1.25
    tilted.save(paths[2])
    out, maps = str(tmp_path / "o.json"), [str(tmp_path / "s0.nii.gz"), str(tmp_path / "s1.nii.gz")]
    cli.main(["evaluate", "--reference-volume", paths[0], "--reference-mask", paths[3], "--input-volumes", *paths[1:3], "--output-json", out,
              "--output-ssim-maps", *maps, "--verbose", "0", "--device", "0"])
    rows = json.load(open(out))
    print(rows)
    assert [r["input_volume"] for r in rows] == paths[1:3]
    inner = image[interior > 0].double()
    L, rms, var = float(inner.max()), float(inner.pow(2).mean().sqrt()), float(inner.var(unbiased=False))
    for r, gain in zip(rows, (1.0, 1.25)):
        assert r["n"] == 20 ** 3 and r["coverage"] == 1 and r["dynamic_range"] == pytest.approx(L, rel=1e-6)
        assert r["mse"] <= bound ** 2 and r["mae"] <= bound and r["nrmse"] <= bound / L * (1 + 1e-6)
        assert r["psnr"] >= 20 * math.log10(L / bound) - 1e-6 and 0 < r["ssim"] <= 1
        assert r["ncc"] ** 2 >= 1 - bound ** 2 / var  # (1 - r^2) var I is the residual of the affine fit, at most the scale fit's
        assert abs(r["fit"][0] / gain - 1) <= bound / (rms - bound) and r["fit"][1] == 0
    ref_array, _, ref_affine = load_nii_volume(paths[0])
    for path in maps:
        array, _, affine = load_nii_volume(path)
        assert array.shape == ref_array.shape and abs(affine - ref_affine).max() <= 1e-4 and 0 < array.max() <= 1 + 1e-6
