"""The 16-bit-operand MLP backward as a dX launch + a dW launch (csrc/mlp.hip: mlp_bwd_dx16_kernel / mlp_bwd_dw16_kernel) - the
modes 1 (bf16) and 3 (fp16) on the shapes the wave-specialised fused backward does not take: three hidden layers, more than 32
inputs at two hidden layers, ragged N, samples per pixel or pixel features.  The reference trains its default bias-free fp16
networks at any --depth and input width (nesvor/nesvor/models.py:28-41)."""
import math

import pytest
import torch

from conftest import small_args
from mlp_reference import emulated_backward as _emulated_backward  # (shared with tests/test_gpu_mlp_steady_state.py)

pytestmark = pytest.mark.gpu

DT16 = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _mode(ht):
    from nesvor_amd import mlp

    return mlp.BF16 if ht == "bf16" else mlp.FP16


def _net(device, depth, k_in, out_dim, biased, seed):
    g = torch.Generator().manual_seed(seed)
    dims = [k_in] + [64] * depth + [out_dim]
    W = [(torch.rand(o, i, generator=g) * 2 - 1) * math.sqrt(6.0 / (i + o)) for i, o in zip(dims, dims[1:])]
    B = [(0.1 * torch.randn(o, generator=g)) if biased else torch.zeros(o) for o in dims[1:]]
    return [w.to(device) for w in W], [b.to(device) for b in B]


def _inputs(device, k_a, rows, N, S, out_dim, seed):
    g = torch.Generator().manual_seed(seed)
    xa = torch.randn(N // S, k_a, generator=g).to(device) if k_a else None
    xb = torch.randn(rows, N, generator=g).to(device)
    dy = torch.randn(out_dim, N, generator=g).to(device)
    return xa, xb, dy


def _run(W, B, xa, xb, dy, b_row0, k_b, S, mode, fused):
    """forward_raw + backward_raw -> (saved, dxb, dxa per pixel, [(dW, db) per layer])"""
    from nesvor_amd import mlp

    N = xb.shape[1]
    _, saved = mlp.forward_raw(W, B, xa, xb, b_row0, k_b, S, True, mode)
    old = mlp.FUSED_BACKWARD
    mlp.FUSED_BACKWARD = fused
    try:
        dxb = torch.empty(k_b, N, device=xb.device)
        dxa, partial = mlp.backward_raw(W, B, xa, xb, dy, saved, b_row0, k_b, S, dxb, xa is not None, mode)
    finally:
        mlp.FUSED_BACKWARD = old
    torch.cuda.synchronize()
    if dxa is not None:
        P = N // S
        dxa = dxa.view(P, -1, dxa.shape[1]).sum(1)  # per sample or per 16-sample group -> per pixel
    flat, off, grads = partial.sum(0), 0, []
    for w, b in zip(W, B):
        dw = flat[off : off + w.numel()].view_as(w)
        off += w.numel()
        grads.append((dw, flat[off : off + b.numel()]))
        off += b.numel()
    return saved, dxb, dxa, grads, partial


def _fused_ok(W, B, k_a, k_b, S, N, mode):
    import ctypes

    from nesvor_amd import _lib, mlp

    d = mlp.dims_desc(len(W) - 1, W[-1].shape[0], k_a, k_b, 0, S, mode)
    return bool(_lib.load().nesvor_mlp_backward_fused_ok(ctypes.byref(d), N))


def _close(a, b, tol, name):
    scale = float(b.abs().max())
    err = float((a.double() - b.double()).abs().max())
    assert scale > 0 and err <= tol * scale, (name, err, scale)


def _close_norm(a, b, tol, name):
    ref = float(b.double().norm())
    err = float((a.double() - b.double()).norm())
    assert ref > 0 and err <= tol * ref, (name, err, ref)


@pytest.mark.parametrize("ht", ["bf16", "fp16"])
@pytest.mark.parametrize("depth,k_a,k_b,S,out_dim", [
    (1, 0, 32, 16, 16),    # density net, one hidden layer
    (2, 0, 32, 16, 16),    # density net, two hidden layers
    (2, 16, 15, 256, 1),   # sigma net: slice embedding | z[1:]
    (1, 16, 4, 256, 1),    # bias net
])
def test_pair_matches_fused_kernel(device, ht, depth, k_a, k_b, S, out_dim):
    """Shapes both paths take: the pair (FUSED_BACKWARD off) against the wave-specialised kernel.  Same operands rounded at the
    same points with the same conversions; the two differ in fp32 summation order only -> dX, dxa (per pixel), dW, db within
    1e-5 of each tensor's max."""
    N = 4096
    mode = _mode(ht)
    W, B = _net(device, depth, k_a + k_b, out_dim, True, 1)
    xa, xb, dy = _inputs(device, k_a, k_b + 1, N, S, out_dim, 2)
    assert _fused_ok(W, B, k_a, k_b, S, N, mode)
    _, dxb_f, dxa_f, g_f, _ = _run(W, B, xa, xb, dy, 1, k_b, S, mode, True)
    _, dxb_p, dxa_p, g_p, _ = _run(W, B, xa, xb, dy, 1, k_b, S, mode, False)
    _close(dxb_p, dxb_f, 1e-5, "dxb")
    if k_a:
        _close(dxa_p, dxa_f, 1e-5, "dxa")
    for li, ((dw_p, db_p), (dw_f, db_f)) in enumerate(zip(g_p, g_f)):
        _close(dw_p, dw_f, 1e-5, f"dW{li}")
        _close(db_p, db_f, 1e-5, f"db{li}")


PAIR_ONLY = [  # (depth, k_a, k_b, S, N, out_dim, biased)
    (3, 0, 24, 16, 2048, 16, True),    # density net at depth 3
    (3, 0, 24, 16, 2048, 16, False),   # ... bias-free (tinycudann.Network)
    (2, 0, 48, 16, 2048, 16, False),   # depth 2, 48 inputs
    (2, 0, 64, 16, 2048, 16, True),    # depth 2, 64 inputs
    (2, 16, 15, 8, 1000, 1, True),     # ragged N, S = 8
    (3, 16, 15, 24, 984, 1, False),    # ragged N, S = 24
    (2, 8, 15, 16, 1024, 1, True),     # k_a = 8
]


@pytest.mark.parametrize("ht", ["bf16", "fp16"])
@pytest.mark.parametrize("depth,k_a,k_b,S,N,out_dim,biased", PAIR_ONLY)
def test_pair_vs_emulated_reference(device, ht, depth, k_a, k_b, S, N, out_dim, biased):
    """Shapes only the pair takes, against a float64 reference that rounds the same operands to the same 16-bit type and gates
    with the forward's saved activations.  What is left is fp32 (kernel) against fp64 (reference) accumulation, and - rarely - a
    pre-activation gradient that sits on a 16-bit rounding boundary and rounds the other way from its fp32 value: bound
    2e-3 (bf16) / 5e-4 (fp16) of each tensor's max, well below the effect of the rounding the emulation models.  Loosely, the
    exact fp64 backward (no operand rounding; the forward's gates and activations, as in the fp32 modes' tests: a plain fp64
    forward gates differently wherever a pre-activation lies within the 16-bit forward's error of 0) within 3e-2 / 5e-3 in norm."""
    mode, dt = _mode(ht), DT16[ht]
    tol, loose = (2e-3, 3e-2) if ht == "bf16" else (5e-4, 5e-3)
    W, B = _net(device, depth, k_a + k_b, out_dim, biased, 3 + depth)
    xa, xb, dy = _inputs(device, k_a, k_b, N, S, out_dim, 4)
    assert not _fused_ok(W, B, k_a, k_b, S, N, mode)
    saved, dxb, dxa, grads, _ = _run(W, B, xa, xb, dy, 0, k_b, S, mode, True)
    assert saved[0].dtype == dt
    dx_ref, g_ref = _emulated_backward(W, B, xa, xb, dy, saved, 0, k_b, S, dt)
    _close(dxb, dx_ref[:, k_a:].t(), tol, "dxb")
    if k_a:
        _close(dxa, dx_ref[:, :k_a].view(N // S, S, k_a).sum(1), tol, "dxa")
    for li, ((dw, db), (dw_r, db_r)) in enumerate(zip(grads, g_ref)):
        _close(dw, dw_r, tol, f"dW{li}")
        _close(db, db_r, tol, f"db{li}")
    # loosely against the exact backward (no operand rounding)
    dx_ex, g_ex = _emulated_backward(W, B, xa, xb, dy, saved, 0, k_b, S, None)
    _close_norm(dxb, dx_ex[:, k_a:].t(), loose, "dxb exact")
    for li, ((dw, db), (dw_r, db_r)) in enumerate(zip(grads, g_ex)):
        _close_norm(dw, dw_r, loose, f"dW{li} exact")
        _close_norm(db, db_r, loose, f"db{li} exact")


@pytest.mark.parametrize("ht", ["bf16", "fp16"])
@pytest.mark.parametrize("depth,k_a,k_b,S,N", [
    (1, 0, 16, 16, 1000),   # one input block
    (2, 0, 32, 8, 2048),    # two
    (2, 0, 48, 16, 2048),   # three
    (3, 16, 48, 24, 984),   # four, three hidden layers, pixel features
    (3, 0, 24, 16, 2048),
])
def test_pair_is_bit_reproducible(device, ht, depth, k_a, k_b, S, N):
    """No floating-point atomics in the result path: three calls give the same bits (dX, dxa, every partial-sum row)."""
    mode = _mode(ht)
    W, B = _net(device, depth, k_a + k_b, 16, True, 7)
    xa, xb, dy = _inputs(device, k_a, k_b, N, S, 16, 8)
    if _fused_ok(W, B, k_a, k_b, S, N, mode):
        pytest.fail("shape meant for the pair")
    runs = [_run(W, B, xa, xb, dy, 0, k_b, S, mode, False) for _ in range(3)]
    for r in runs[1:]:
        assert torch.equal(r[1], runs[0][1]) and torch.equal(r[4], runs[0][4])
        if k_a:
            assert torch.equal(r[2], runs[0][2])


def test_fp16_loss_scaling_depth3_skips_overflowing_steps(device):
    """The reference's default numerics at --depth 3 (fp16 operands + its GradScaler semantics, train.py:161-164, 190-196): the
    networks train through autograd over flat_network on the 16-bit pair.  A step at scale 2^60 overflows fp16, is skipped
    (parameters and moments untouched, gradients dropped) and halves the scale; finite steps grow it every growth_interval."""
    from nesvor_amd import mlp
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.train import Dataset

    vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    args = small_args(device=device, n_iter=300, batch_size=512, n_samples=16, finest_resolution=1.0, log2_hashmap_size=14,
                      no_transformation_optimization=True, depth=3, dtype=torch.float16, single_precision=False,
                      fp16_loss_scaling=True)
    try:
        ds = Dataset(slices, args)
        torch.manual_seed(0)
        model = NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, args)
        tr = FusedTrainer(model, args)
        assert tr.scaler is not None and tr.scaler.scale == 1.0 and tr.direct is None and mlp.HALF_OPERANDS[0] == mlp.FP16
        assert len(model.inr.density_net.shapes) == 4
        batch = ds.get_batch(args.batch_size, device)
        l0 = tr.step(batch["xyz"], batch["v"], batch["slice_idx"])
        assert tr.t == 1 and tr.scaler.growth_tracker == 1 and all(bool(torch.isfinite(v)) for v in l0.values())
        before = tr.flat.param.clone(), tr.flat.exp_avg.clone(), tr.flat.exp_avg_sq.clone()
        tr.scaler.scale = 2.0 ** 60
        tr.step(batch["xyz"], batch["v"], batch["slice_idx"])
        assert tr.t == 1 and tr.scaler.scale == 2.0 ** 59 and tr.scaler.skipped == 1 and tr.scaler.growth_tracker == 0
        assert torch.equal(tr.flat.param, before[0]) and torch.equal(tr.flat.exp_avg, before[1]) and torch.equal(tr.flat.exp_avg_sq, before[2])
        assert float(tr.flat.grad.abs().max()) == 0.0
        tr.scaler.scale, tr.scaler.growth_interval = 4.0, 2
        la = tr.step(batch["xyz"], batch["v"], batch["slice_idx"])
        assert tr.t == 2 and tr.scaler.scale == 4.0
        tr.step(batch["xyz"], batch["v"], batch["slice_idx"])
        assert tr.t == 3 and tr.scaler.scale == 8.0
        for k in l0:
            assert abs(float(la[k].detach())) < 1e3 * (abs(float(l0[k].detach())) + 1e-3), k
        tr.finish()
    finally:
        mlp.HALF_OPERANDS[0] = True


def _psnr(a, b, peak):
    return 10 * math.log10(peak**2 / float(((a - b) ** 2).mean()))


@pytest.mark.parametrize("over", [dict(depth=3), dict(depth=2, n_features_per_level=4)])
def test_train_phantom_half_precision_pair_shapes_keep_psnr(device, over):
    """Default precision (bias-free bf16-operand networks) on shapes only the pair takes - depth 3, and depth 2 with more than 32
    density-net inputs - reaches the fp32 model's PSNR within 0.5 dB (settings of test_train_phantom_half_precision_model_keeps_psnr)."""
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.train import train

    vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    g = (torch.arange(32, dtype=torch.float32) - 15.5)
    zz, yy, xx = torch.meshgrid(g, g, g, indexing="ij")
    pts = torch.stack([xx, yy, zz], -1).reshape(-1, 3).to(device)
    truth = vol.reshape(-1)
    inside = truth > 0
    psnr = {}
    for dtype in (torch.float32, torch.float16):
        args = small_args(device=device, n_iter=300, batch_size=512, n_samples=16, finest_resolution=1.0,
                          log2_hashmap_size=14, no_transformation_optimization=True, dtype=dtype,
                          single_precision=dtype == torch.float32, **over)
        torch.manual_seed(0)
        inr, _, _ = train(slices, args)
        if dtype == torch.float16:
            sh = inr.density_net.shapes
            assert len(sh) == 4 or sh[0][1] > 32, sh  # a shape the fused backward refuses
        with torch.no_grad():
            r = inr(pts[:, None], False).mean(-1).float()
        s = float((r[inside] * truth[inside]).sum() / (r[inside] ** 2).sum())
        psnr[dtype] = _psnr(r[inside] * s, truth[inside], float(truth.max()))
    print(f"{over}: PSNR fp32 model {psnr[torch.float32]:.2f} dB, half-precision structure {psnr[torch.float16]:.2f} dB")
    assert psnr[torch.float16] > 8.0 and abs(psnr[torch.float16] - psnr[torch.float32]) <= 0.5


def test_one_call_step_bf16_operands_ragged_samples(device, golden):
    """--mlp-bf16 with n_samples = 24: the fused backward refuses every network, the one-call step runs them on the 16-bit pair
    through nesvor_step_t.dpre_scratch.  It must now take the step, and match the Python-issued step of the same model within the
    tolerances of tests/test_gpu_model.py::test_one_call_step_equals_python_issued_step."""
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.transform import RigidTransform

    args = small_args(device=device, mlp_bf16=True, n_samples=24)
    tf = RigidTransform(torch.tensor(golden["fw_sd::axisangle_init"]).to(device), trans_first=True)
    res = torch.tensor(golden["ds_resolution"]).to(device)
    bbox = torch.tensor(golden["fw_sd::inr.bounding_box"]).to(device)
    torch.manual_seed(3)
    m1 = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    with torch.no_grad():
        for name, p in m1.named_parameters():
            if name in ("logit_coef", "log_var_slice"):
                p.add_(0.3 * torch.randn_like(p))
            if name == "axisangle":
                p.add_(0.02 * torch.randn_like(p))
            if name == "inr.encoding.params":
                p.mul_(1e3)
    m2 = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    m2.load_state_dict(m1.state_dict())
    t1, t2 = FusedTrainer(m1, args), FusedTrainer(m2, args)
    assert t1.direct is not None and t2.direct is not None and t1.direct.bf16 is True
    t2.direct._native_on = False
    assert not t1.direct._fused_backward_takes_all(args.batch_size * args.n_samples)
    assert t1.direct.native_ready()
    assert not t2.direct.native_ready()
    d = lambda k: torch.tensor(golden[f"fw_{k}"]).to(device)
    torch.manual_seed(11)
    l1 = t1.direct.run(d("xyz"), d("v"), d("idx"))
    l2 = t2.direct.run(d("xyz"), d("v"), d("idx"))
    assert list(l1.keys()) == list(l2.keys())
    for k in l1:
        a, b = float(l1[k]), float(l2[k])
        assert abs(a - b) <= 1e-6 * abs(b) + 1e-9, (k, a, b)
    torch.cuda.synchronize()
    scale = float(t2.flat.grad.abs().max())
    assert scale > 0 and float((t1.flat.grad - t2.flat.grad).abs().max()) <= 1e-5 * scale
    t1.flat.grad.zero_(); t2.flat.grad.zero_()
    t1.direct._noise_calls = t2.direct._noise_calls = 0
    for it in range(3):
        l1 = t1.step(d("xyz"), d("v"), d("idx"))
        l2 = t2.step(d("xyz"), d("v"), d("idx"))
        for k in l1:
            a, b = float(l1[k]), float(l2[k])
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-7, (it, k, a, b)
        assert t1.t == t2.t == it + 1
        apart = ((t1.flat.param - t2.flat.param).abs() > 1e-5 * (1 + t2.flat.param.abs())).float().mean()
        assert float(apart) < 2e-3, (it, float(apart))


def test_cli_reconstruct_depth3_default_precision(tmp_path, device):
    """`nesvor reconstruct --depth 3` without --single-precision (bias-free half-precision networks) runs end to end and writes a
    volume that correlates with the phantom."""
    from nesvor_amd import cli
    from nesvor_amd.image import Volume
    from nesvor_amd.image_io import load_volume
    from nesvor_amd.phantom import phantom3d, simulate_stacks, stack_geometry
    from nesvor_amd.transform import RigidTransform

    vs, res_s, gap = 32, 1.5, 3.0
    vol = torch.tensor(phantom3d(n=vs), dtype=torch.float32, device=device)
    torch.manual_seed(0)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=res_s, s_thick=gap, normalize=False)
    n_slice, _ = stack_geometry(vs, 1.0, res_s, gap)
    paths = []
    for i in range(3):
        ss = slices[i * n_slice : (i + 1) * n_slice]
        img = torch.cat([s.image for s in ss], 0)
        ax = torch.cat([s.transformation.axisangle() for s in ss], 0).mean(0, keepdim=True)
        p = str(tmp_path / f"stack{i}.nii.gz")
        Volume(img, img > 0, RigidTransform(ax), res_s, res_s, gap).save(p, masked=False)
        paths.append(p)
    out_vol = str(tmp_path / "recon.nii.gz")
    cli.main(["reconstruct", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--output-volume", out_vol, "--depth", "3",
              "--n-iter", "150", "--batch-size", "512", "--n-samples", "32", "--log2-hashmap-size", "12", "--finest-resolution", "2.0",
              "--output-resolution", "2.0", "--seed", "0", "--verbose", "0"])
    v = load_volume(out_vol, device=device)
    assert torch.isfinite(v.image).all()
    g = (torch.arange(vs, dtype=torch.float32) - (vs - 1) / 2)
    zz, yy, xx = torch.meshgrid(g, g, g, indexing="ij")
    pts = torch.stack([xx, yy, zz], -1).reshape(-1, 3).to(device)
    r, truth = v.sample_points(pts), vol.reshape(-1)
    c = float(torch.corrcoef(torch.stack([r, truth]))[0, 1])
    print(f"depth 3, default precision: correlation with the phantom {c:.3f}")
    assert c > 0.3
