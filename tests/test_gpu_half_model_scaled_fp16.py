"""The half-precision model structure (bias-free tinycudann networks) in the scaled-fp16 mode (nesvor_mlp_t.bf16_operands = 4 with
NULL biases, ``args.mlp_fp16`` without ``--single-precision``): the kernels' bias-free forms against fp64, the one-call step against
the Python-issued step and against autograd, reconstruction quality, and a checkpoint that carries the mode."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from conftest import small_args

pytestmark = pytest.mark.gpu


def _gate():
    """Every test asks for the export first: on a library without the bias-free kernels it fails here, before any launch with
    NULL biases."""
    from nesvor_amd import _lib

    lib = _lib.load()
    assert hasattr(lib, "nesvor_mlp_bias_free_ok"), "library without the bias-free kernels"
    return lib


def _net(nh, k_in, out_dim, device, seed=1):
    from nesvor_amd import mlp
    from nesvor_amd.tinycudann import Network

    torch.manual_seed(seed)
    net = Network(k_in, out_dim, {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64,
                                  "n_hidden_layers": nh}).to(device)
    mlp.set_network_operands([net], mlp.FP16S)
    return net


def _inputs(k_a, k_b, out_dim, N, S, device, seed=2):
    g = torch.Generator(device="cpu").manual_seed(seed)
    xa = torch.randn(N // S, k_a, generator=g).to(device) if k_a else None
    xb = torch.randn(k_b, N, generator=g).to(device)
    dy = torch.randn(out_dim, N, generator=g).to(device)
    return xa, xb, dy


def _run(p, xa, xb, dy, k_b, S, need_dxa=True):
    from nesvor_amd import mlp

    y, saved = mlp.forward_raw(p.weights, p.biases, xa, xb, 0, k_b, S, True, mlp.FP16S)
    dxb = torch.empty_like(xb)
    dxa, partial = mlp.backward_raw(p.weights, p.biases, xa, xb, dy, saved, 0, k_b, S, dxb, need_dxa, mlp.FP16S)
    return y, saved, dxa, dxb, partial


# (n_hidden, k_a, k_b, out_dim, N, S): one and two hidden layers on the fused kernels (compact save), three hidden layers and ragged
# N / S on the wide dX + dW pair
SHAPES = [
    (1, 0, 32, 15, 1 << 14, 16), (1, 16, 16, 1, 1 << 14, 16), (2, 16, 15, 1, 1 << 14, 16), (2, 0, 32, 15, 1 << 14, 16),
    (3, 0, 32, 15, 1 << 14, 16), (2, 16, 15, 1, 24 * 640, 24), (1, 0, 24, 15, (1 << 14) + 8, 8),
]


@pytest.mark.parametrize("nh,k_a,k_b,out_dim,N,S", SHAPES)
def test_bias_free_kernels_match_fp64(device, nh, k_a, k_b, out_dim, N, S):
    lib = _gate()
    from nesvor_amd import mlp

    net = _net(nh, k_a + k_b, out_dim, device)
    p = mlp.NetParams(net)
    assert p.bias_free and all(b is None for b in p.biases)
    d = mlp._desc(p.weights, p.biases, k_a, k_b, 0, S, mlp.FP16S)
    assert lib.nesvor_mlp_bias_free_ok(ctypes.byref(d), N) == 1
    fused = bool(lib.nesvor_mlp_backward_fused_ok(ctypes.byref(d), N))
    assert fused == (nh <= 2 and N % (16 * S) == 0 and S % 16 == 0)  # (these shapes: the compact save takes them)
    assert fused == bool(lib.nesvor_mlp_compact_save_ok(ctypes.byref(d), N))
    # biased descriptors of other modes with NULL biases are refused
    d0 = mlp._desc(p.weights, p.biases, k_a, k_b, 0, S, mlp.SPLIT)
    assert lib.nesvor_mlp_bias_free_ok(ctypes.byref(d0), N) == 0 and lib.nesvor_mlp_backward_fused_ok(ctypes.byref(d0), N) == 0
    xa, xb, dy = _inputs(k_a, k_b, out_dim, N, S, device)
    y, saved, dxa, dxb, partial = _run(p, xa, xb, dy, k_b, S)
    assert partial.shape[1] == sum(w.numel() for w in p.weights)  # W0 | W1 | ... | W_last (out_dim rows): no b columns
    # fp64 evaluation of the bias-free network
    X = xb.t()
    if xa is not None:
        X = torch.cat([xa.repeat_interleave(S, 0), X], 1)
    X, Wd = X.cpu().double(), [w.cpu().double() for w in p.weights]
    hs, h = [], X
    for l in range(nh):
        h = torch.relu(h @ Wd[l].t())
        hs.append(h)
    yr = h @ Wd[nh].t()
    rel = lambda a, b: float((a.cpu().double() - b).abs().max() / b.abs().max())
    assert rel(y.t(), yr) < 3e-3
    # the gates of the compact save are the forward's sign bits (word (group, lane = 16 q + sample), bit 16 l + 4 b + r = unit
    # 16 b + 4 q + r of layer l): a unit within fp16 rounding of zero may be gated differently from the exact network - either is a
    # valid subgradient there - so the reference backward takes the kernel's gates (as test_gpu_ops.py does for the biased mode)
    gates = [hs[l] > 0 for l in range(nh)]
    if fused:
        words = saved[0].view(torch.int32).view(N // 16, 4, 16).cpu()
        for l in range(nh):
            g_l = torch.zeros(N // 16, 16, 64, dtype=torch.bool)
            for b in range(4):
                for r in range(4):
                    g_l[:, :, [16 * b + 4 * q + r for q in range(4)]] = (((words >> (16 * l + 4 * b + r)) & 1) != 0).permute(0, 2, 1)
            assert float((g_l.view(N, 64) == gates[l]).double().mean()) > 0.99
            gates[l] = g_l.view(N, 64)
    G = dy.t().cpu().double()
    dd, gW = G, [None] * (nh + 1)
    for l in range(nh, -1, -1):
        inp = hs[l - 1] if l > 0 else X
        gW[l] = dd.t() @ inp
        dd = dd @ Wd[l]
        if l > 0:
            dd = dd * gates[l - 1]
    assert rel(dxb.t(), dd[:, k_a:]) < 5e-3
    if xa is not None:
        per_pixel = dxa.view(N // S, -1, k_a).sum(1)
        assert rel(per_pixel, dd[:, :k_a].reshape(N // S, S, k_a).sum(1)) < 5e-3
    flat, off = partial.sum(0).cpu().double(), 0
    for w, gw in zip(Wd, gW):
        assert rel(flat[off : off + w.numel()].view_as(w), gw) < 5e-3
        off += w.numel()
    assert off == flat.numel()
    # the forward equals the biased instantiation fed zero biases, to fp16 rounding
    zeros = [torch.zeros(w.shape[0], device=device) for w in p.weights]
    yb, _ = mlp.forward_raw(p.weights, zeros, xa, xb, 0, k_b, S, True, mlp.FP16S)
    assert float((y - yb).abs().max()) <= 1e-3 * float(yb.abs().max())
    # inference (nothing saved): the same outputs
    yi, _ = mlp.forward_raw(p.weights, p.biases, xa, xb, 0, k_b, S, False, mlp.FP16S)
    assert float((y - yi).abs().max()) <= 2e-3 * float(y.abs().max())


@pytest.mark.parametrize("nh", [1, 2])
@pytest.mark.parametrize("k_a,k_b,out_dim", [(0, 16, 15), (16, 16, 1), (0, 32, 1), (16, 15, 15)])
def test_bias_free_kernels_are_bit_reproducible(device, nh, k_a, k_b, out_dim):
    """Every bias-free instantiation (training forward with the compact save, inference forward, compact backward; one and two
    input blocks, the VALU output layer and the MFMA one) gives the same bits over 20 runs at N = 2^18."""
    _gate()
    from nesvor_amd import mlp

    N, S = 1 << 18, 16
    p = mlp.NetParams(_net(nh, k_a + k_b, out_dim, device))
    xa, xb, dy = _inputs(k_a, k_b, out_dim, N, S, device)
    ref = None
    for _ in range(20):
        y, saved, dxa, dxb, partial = _run(p, xa, xb, dy, k_b, S)
        yi, _ = mlp.forward_raw(p.weights, p.biases, xa, xb, 0, k_b, S, False, mlp.FP16S)
        assert saved[0].numel() == N * 4  # the compact save
        outs = [y, saved[0], dxb, partial, yi] + ([dxa] if dxa is not None else [])
        if ref is None:
            ref = [t.clone() for t in outs]
        else:
            for a, b in zip(outs, ref):  # (bitwise: the saved words viewed as floats hold NaN patterns)
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _mode4_half_args(device, **over):
    return small_args(device=device, dtype=torch.float16, single_precision=False, mlp_fp16=True, **over)


def _perturbed_pair(golden, device, args, table_scale):
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.transform import RigidTransform

    tf = RigidTransform(torch.tensor(golden["fw_sd::axisangle_init"]).to(device), trans_first=True)
    res = torch.tensor(golden["ds_resolution"]).to(device)
    bbox = torch.tensor(golden["fw_sd::inr.bounding_box"]).to(device)
    torch.manual_seed(3)
    m1 = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    with torch.no_grad():  # per-slice parameters start at 0 / identity: move them so every gradient path is live
        for name, p in m1.named_parameters():
            if name in ("logit_coef", "log_var_slice"):
                p.add_(0.3 * torch.randn_like(p))
            if name == "axisangle":
                p.add_(0.02 * torch.randn_like(p))
            if name == "inr.encoding.params":
                p.mul_(table_scale)
    m2 = NeSVoR(tf, res, float(golden["ds_mean"]), bbox, args)
    m2.load_state_dict(m1.state_dict())
    return m1, m2


def _padding_rows(net):
    last = net.shapes[-1][0] * net.shapes[-1][1]
    return net.params[-last:].view(net.shapes[-1])[net.n_output_dims:], net.params.grad[-last:].view(net.shapes[-1])[net.n_output_dims:]


@pytest.mark.parametrize("over", [
    {"depth": 1, "n_samples": 16}, {"depth": 2, "n_samples": 16}, {"n_levels_bias": 2, "depth": 2, "n_samples": 16},
    {"no_pixel_variance": True, "n_samples": 16}, {"n_samples": 24}, {"depth": 2, "n_samples": 16, "n_features_slice": 32},
])
def test_one_call_step_equals_python_issued_step_bias_free(device, golden, over):
    """``nesvor_step_run`` with the bias-free networks against the same launches issued from Python (same kernels, same order, same
    noise stream), compared as tests/test_gpu_model.py::test_one_call_step_equals_python_issued_step compares the other modes:
    losses to 1e-6, the gradient to 1e-5 of its largest entry (the hash-grid owner pass sums in arrival order), three full steps by
    the fraction of parameters that moved apart.  The padding rows of the last layers take no gradient and are never written."""
    _gate()
    from nesvor_amd import direct, mlp
    from nesvor_amd.fused import FusedTrainer

    if os.environ.get("NESVOR_STEP_NATIVE", "1") == "0":
        pytest.skip("the one-call step is switched off (NESVOR_STEP_NATIVE=0)")
    args = _mode4_half_args(device, **over)
    m1, m2 = _perturbed_pair(golden, device, args, 1e3)
    assert direct.half_precision_model(m1) and direct.supported(m1)
    t1, t2 = FusedTrainer(m1, args), FusedTrainer(m2, args)
    assert t1.direct is not None and t1.direct.bf16 == mlp.FP16S and t1.direct.d_net.bias_free and t1.scaler is None
    t2.direct._native_on = False
    assert t1.direct.native_ready() and not t2.direct.native_ready()
    nets = [n for n in direct._nets(m1) if n.shapes[-1][0] > n.n_output_dims]  # (networks with padding rows)
    pad0 = [_padding_rows(n)[0].clone() for n in nets]
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
    for n, p0 in zip(nets, pad0):
        pv, pg = _padding_rows(n)
        assert float(pg.abs().max()) == 0.0 and torch.equal(pv, p0)
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
    assert float(t1.flat.grad.abs().max()) == 0.0


@pytest.mark.parametrize("over", [{}, {"depth": 2}, {"n_levels_bias": 2}])
def test_direct_step_bias_free_against_autograd(device, golden, over, monkeypatch):
    """The one-call step in this mode against autograd over the op-by-op model with the networks in plain fp32 torch on the same
    flat parameters: fp16 operand rounding after power-of-two scaling (2^-11 per operand) - losses 0.5%, gradients 2% in norm
    (pose: 10%), tighter than the bf16 mode's 2% / 5%."""
    import torch.nn.functional as F_

    import nesvor_amd.tinycudann as tcnn

    _gate()

    def fp32_reference_forward(self, x):
        off, h = 0, x.to(self.params.dtype)
        for li, (o, i) in enumerate(self.shapes):
            h = h @ self.params[off : off + o * i].view(o, i).t()
            off += o * i
            if li < len(self.shapes) - 1:
                h = F_.relu(h)
        return h[..., : self.n_output_dims]

    monkeypatch.setattr(tcnn.Network, "forward", fp32_reference_forward)
    from nesvor_amd import mlp
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.train import loss_weights

    args = _mode4_half_args(device, n_samples=16, **over)
    m1, m2 = _perturbed_pair(golden, device, args, 2e3)
    t2 = FusedTrainer(m2, args)
    assert t2.direct is not None and t2.direct.bf16 == mlp.FP16S
    w = loss_weights(args)
    d = lambda k: torch.tensor(golden[f"fw_{k}"]).to(device)
    noise = torch.randn(48, 16, 3, generator=torch.Generator().manual_seed(0)).to(device)
    l1 = m1.forward_with_noise(d("xyz"), d("v"), d("idx"), noise)
    sum(w[k] * l1[k] for k in l1 if k in w and w[k]).backward()
    l2 = t2.direct.run(d("xyz"), d("v"), d("idx"), noise)
    for k in l1:
        assert abs(float(l1[k].detach()) - float(l2[k])) <= 5e-3 * abs(float(l1[k].detach())) + 1e-6, (k, float(l1[k].detach()), float(l2[k]))
    g1 = dict((n, p.grad) for n, p in m1.named_parameters())
    for name, p in m2.named_parameters():
        a, b = g1[name].float().reshape(-1), p.grad.reshape(-1)
        tol = 0.10 if name == "axisangle" else 0.02
        assert float((a - b).norm()) <= tol * float(a.norm()) + 1e-9, (name, float((a - b).norm()), float(a.norm()))
    assert float(_padding_rows(m2.sigma_net)[1].abs().max()) == 0.0
    t2.optimizer_step()


def _psnr(a, b, peak):
    return 10 * math.log10(peak**2 / float(((a - b) ** 2).mean()))


def test_train_phantom_bias_free_scaled_fp16_keeps_psnr(device):
    """train() in this mode reaches the fp32 model's reconstruction quality within 0.5 dB on the 32^3 phantom."""
    _gate()
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
    for name, kw in (("fp32", dict(dtype=torch.float32, single_precision=True)),
                     ("half+fp16s", dict(dtype=torch.float16, single_precision=False, mlp_fp16=True))):
        args = small_args(device=device, n_iter=300, batch_size=512, n_samples=16, finest_resolution=1.0, log2_hashmap_size=14,
                          no_transformation_optimization=True, depth=2, **kw)
        torch.manual_seed(0)
        inr, _, _ = train(slices, args)
        with torch.no_grad():
            r = inr(pts[:, None], False).mean(-1).float()
        s = float((r[inside] * truth[inside]).sum() / (r[inside] ** 2).sum())
        psnr[name] = _psnr(r[inside] * s, truth[inside], float(truth.max()))
    print(f"PSNR fp32 model {psnr['fp32']:.2f} dB, half-precision structure in scaled fp16 {psnr['half+fp16s']:.2f} dB")
    assert psnr["half+fp16s"] > 8.0 and abs(psnr["half+fp16s"] - psnr["fp32"]) <= 0.5


def test_c1_half_precision_structure_in_scaled_fp16(device):
    """BASELINE C1 at the oracle run's configuration (tests/golden/oracle_run_c1.npz: 3 stacks of phantom3d(128), reduced batch,
    200 iterations) with the half-precision structure in this mode, against the fp32 oracle's PSNR.  The oracle trains biased
    networks, so the gap is the structure's as much as the arithmetic's: reported, held within 0.5 dB."""
    _gate()
    from bench import make_args
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.train import train
    from test_gpu_fullsize import _points, _psnr_pair

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_run_c1.npz")
    gold = np.load(path, allow_pickle=False)
    n_iter, B, S = (int(x) for x in gold["config"][:3])
    phantom = torch.tensor(phantom3d(n=128), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(phantom, n_stacks=3)
    args = make_args(device, B, S, 2, n_iter)
    args.dtype, args.single_precision, args.mlp_fp16 = torch.float16, False, True
    torch.manual_seed(0)
    inr, _, _ = train(slices, args)
    pts = _points(device)
    rec = torch.empty(pts.shape[0], device=device)
    with torch.no_grad():
        for i in range(0, pts.shape[0], 1 << 18):
            rec[i : i + (1 << 18)] = inr(pts[i : i + (1 << 18), None], False).mean(-1)
    p_whole, p_int = _psnr_pair(rec, phantom.reshape(-1), float(gold["skull_threshold"]))
    o_whole, o_int = float(gold["psnr_whole_db"]), float(gold["psnr_interior_db"])
    print(f"half-precision structure, scaled fp16: PSNR whole object {p_whole:.3f} / fp32 oracle {o_whole:.3f} dB "
          f"(gap {p_whole - o_whole:+.3f}); interior {p_int:.3f} / {o_int:.3f} dB (gap {p_int - o_int:+.3f})")
    assert abs(p_whole - o_whole) <= 0.5 and abs(p_int - o_int) <= 0.5


def test_checkpoint_carries_the_mode_per_network(device, tmp_path):
    """An fp16-loss-scaling trainer in the same process (its networks - and the process-wide default - take fp16 operands), then a
    model trained in this mode is saved, reloaded and sampled: the reloaded networks evaluate in scaled fp16 with NULL biases and
    give the in-memory model's output bit for bit."""
    _gate()
    from nesvor_amd import mlp
    from nesvor_amd.fused import FusedTrainer
    from nesvor_amd.image_io import load_model, save_model
    from nesvor_amd.models import NeSVoR
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.sample import PsfAveragedDensity, sample_points
    from nesvor_amd.train import Dataset, train

    vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    mk = lambda **kw: small_args(device=device, n_iter=30, batch_size=512, n_samples=16, finest_resolution=1.0, log2_hashmap_size=14,
                                 no_transformation_optimization=True, dtype=torch.float16, single_precision=False, **kw)
    try:
        a_ls = mk(fp16_loss_scaling=True)
        ds = Dataset(slices, a_ls)
        m_ls = NeSVoR(ds.transformation, ds.resolution, ds.mean, ds.bounding_box, a_ls)
        tr = FusedTrainer(m_ls, a_ls)
        assert tr.scaler is not None and mlp.network_operands(m_ls.inr.density_net) == mlp.FP16 and mlp.HALF_OPERANDS[0] == mlp.FP16
        args = mk(mlp_fp16=True)
        torch.manual_seed(0)
        inr, _, mask = train(slices, args)
        assert mlp.network_operands(inr.density_net) == mlp.FP16S
        path = str(tmp_path / "m.pt")
        save_model(path, inr, mask, args)
        inr2, _, stored = load_model(path, device)
        assert stored.mlp_fp16 and mlp.network_operands(inr2.density_net) == mlp.FP16S and mlp.NetParams(inr2.density_net).bias_free
        g = (torch.arange(16, dtype=torch.float32) - 7.5) * 2
        zz, yy, xx = torch.meshgrid(g, g, g, indexing="ij")
        pts = torch.stack([xx, yy, zz], -1).reshape(-1, 3).to(device)
        args.inference_batch_size, args.n_inference_samples = 4096, 32
        stored.inference_batch_size, stored.n_inference_samples = 4096, 32
        # (the same PSF noise for both: the kernels draw it from the seed and a per-chunk counter)
        torch.manual_seed(7)
        PsfAveragedDensity._chunks = 0
        a = sample_points(inr, pts, args)
        torch.manual_seed(7)
        PsfAveragedDensity._chunks = 0
        b = sample_points(inr2, pts, stored)
        assert torch.equal(a, b)
        with torch.no_grad():
            assert torch.equal(inr(pts[:, None], False), inr2(pts[:, None], False))
    finally:
        mlp.HALF_OPERANDS[0] = True
