"""The wide MLP kernels at hidden widths 129 .. 256 (csrc/mlp_wide.hip, the chunked-image kernels: sixteen 16-feature blocks, a
layer streamed through LDS in 32-row chunks, one 16-sample group per wave, dW in passes of four output x eight input blocks).

a. kernels against the float64 chain with the kernel's own gates, through ``mlp.apply_net`` / ``torch.ops.nesvor.wide_mlp``
   (autograd: gradients outside the input rows are exactly zero; inference output = training output bit for bit; the library
   fallback is not reached);
b. 20 repeat runs of the (256, 3) network at N = 2^16 give the same bits;
c. ``tinycudann.Network`` with 256 neurons;
d. the C ABI's limits (256 accepted, 257 refused, sixteen saved blocks above 128);
e. training end to end at (256, 1) and (192, 2) against the oracle's loop - the construction of
   tests/test_gpu_parity.py::test_other_widths_and_depths_match_oracle_losses, restated;
f. the partial-buffer rule (``mlp.wide_partial_rows``): at most 256 MB at 256 x 7, whose gradients - four workgroups per partial
   row - are compared as in a.; 1024 rows at width 128.

Tolerances of a., c., f.: per quantity, FP32_MARGIN = 4 x the error of the SAME gated chain evaluated by torch in float32 on
the same inputs against float64 - the rule and margin of tests/test_gpu_mlp_steady_state.py (both sum the same number of fp32
terms in another order; the bias gradients summed as a GEMM with a column of ones).  Nothing is fixed in advance: an fp32 chain
of k = 256 had not been measured here.  Every case prints both errors.

MEASURED (MI355X, test a; max |error| / max |reference|, smallest .. largest over the cases and both sizes):

=====================  ==================  ==================
quantity               torch fp32 chain    chunked kernels
=====================  ==================  ==================
y                      1.7e-7 .. 6.4e-7    3.2e-7 .. 6.7e-7
saved activations      1.5e-7 .. 6.6e-7    2.0e-7 .. 6.5e-7
dxb                    3.0e-7 .. 4.8e-7    2.9e-7 .. 5.2e-7
dxa (per pixel)        2.7e-7 .. 3.4e-7    2.4e-7 .. 3.1e-7
dW                     4.6e-7 .. 7.7e-6    1.5e-7 .. 5.9e-7
db                     1.8e-7 .. 4.2e-6    5.7e-8 .. 4.9e-7
=====================  ==================  ==================

The largest kernel error / bound over all tests of this file: y 0.63 (256 x 7 at N = 888, test f: 7.2e-7 against the float32
chain's 2.9e-7), saved activations 0.37, dxb 0.28, dxa 0.29, dW 0.21, db 0.20.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import mlp_reference as R
from conftest import small_args

pytestmark = pytest.mark.gpu

FP32_MARGIN = 4.0
REPEATS = 20

CASES = [  # (width, depth, k_a, k_b, b_row0, rows, out_dim, bias)
    (256, 1, 0, 32, 0, 32, 16, True),
    (256, 3, 16, 15, 1, 16, 1, True),
    (192, 2, 0, 32, 0, 32, 16, False),
    (136, 7, 0, 20, 2, 24, 3, True),   # smallest padded width above 128, deepest stack
    (200, 2, 16, 48, 0, 48, 16, True),  # 64 inputs
]
SIZES = [(24, 37), (24, 10923)]  # (S, pixels): N = 888 - ragged in 16 and in the 128-sample tile -, and 262 152: several tiles per workgroup, a ragged tail


def _sequential(W, B, bias):
    layers = []
    for l, w in enumerate(W):
        lin = nn.Linear(w.shape[1], w.shape[0], bias=bias).to(w.device)
        with torch.no_grad():
            lin.weight.copy_(w)
            if bias:
                lin.bias.copy_(B[l])
        layers += [lin] + ([nn.ReLU()] if l < len(W) - 1 else [])
    return nn.Sequential(*layers)


def _compare(name, W, Bk, x64, dy, gates, got, k_a, P, S):
    """``got``: dict(y (out, N), H [(N, width)], dxb (k_b, N), dxa (P, k_a) | None, grads [(dW, db | None)]) against the float64
    gated chain, each quantity within FP32_MARGIN x the float32 chain's own error.  Prints both errors; -> failures."""
    ref = R.gated_chain(W, Bk, x64, dy, gates)
    c32 = R.gated_chain(W, Bk, x64, dy, gates, torch.float32)
    pix = lambda t: t[:, :k_a].reshape(P, S, k_a).sum(1)
    rows, failed = [], []

    def both(q, g, a32, a64):
        e32, ek = R.rel_err(a32, a64), R.rel_err(g, a64)
        rows.append(f"{q} torch-fp32 {e32:.3g} kernel {ek:.3g}")
        if not ek <= FP32_MARGIN * e32:
            failed.append(f"{q}: {ek:.3g} > {FP32_MARGIN} x {e32:.3g}")

    both("y", got["y"].t(), c32["y"], ref["y"])
    for l, h in enumerate(got.get("H", [])):
        both(f"saved{l}", h, c32["pre"][l].relu(), ref["pre"][l].relu())
    if got.get("dxb") is not None:
        both("dxb", got["dxb"].t(), c32["dx"][:, k_a:], ref["dx"][:, k_a:])
    if got.get("dxa") is not None:
        both("dxa", got["dxa"], pix(c32["dx"]), pix(ref["dx"]))
    for l, (dw, db) in enumerate(got["grads"]):
        both(f"dW{l}", dw, c32["grads"][l][0], ref["grads"][l][0])
        if db is not None:
            both(f"db{l}", db, c32["grads"][l][1], ref["grads"][l][1])
    print(f"\n{name}: " + "; ".join(rows))
    return failed


@pytest.mark.parametrize("S,P", SIZES)
@pytest.mark.parametrize("width,depth,k_a,k_b,b_row0,rows,out_dim,bias", CASES)
def test_kernels_vs_float64(device, width, depth, k_a, k_b, b_row0, rows, out_dim, bias, S, P):
    from nesvor_amd import mlp

    N = S * P
    assert N % 16 != 0 and N % 128 != 0
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, bias, 300 + width + depth, width=width)
    Bk = B if bias else []
    xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 13)
    net = _sequential(W, B, bias)
    assert mlp.wide_supported(net) and not mlp.supported(net)
    xb_g = xb.clone().requires_grad_(True)
    xa_g = None if xa is None else xa.clone().requires_grad_(True)
    warned = set(mlp._warned_library)  # (process-global, never cleared: another test may have reached the library path on purpose)
    y = mlp.apply_net(net, xa_g, xb_g, b_row0, k_b, S)
    y.backward(dy)
    assert mlp._warned_library == warned, mlp._warned_library - warned  # the library path stayed unreached
    # the same launches without autograd: the saved activations (the kernel's gates) and the inference launch
    with torch.no_grad():
        y_tr, saved = torch.ops.nesvor.wide_mlp(xa, xb, W, Bk, b_row0, k_b, S, True)
        y_inf, none = torch.ops.nesvor.wide_mlp(xa, xb, W, Bk, b_row0, k_b, S, False)
    assert len(saved) == depth and len(none) == 0 and saved[0].numel() == (N + 15) // 16 * 16 * 256
    assert torch.equal(y_inf, y_tr) and torch.equal(y.detach(), y_tr)
    # gradient isolation: rows of xb outside [b_row0, b_row0 + k_b) get exactly zero
    outside = torch.ones(rows, dtype=torch.bool, device=device)
    outside[b_row0 : b_row0 + k_b] = False
    assert xb_g.grad.shape == xb.shape and not xb_g.grad[outside].any()
    H = [R.saved_rows(s, N, blocks=16)[:, :width] for s in saved]
    lin = [m for m in net if isinstance(m, nn.Linear)]
    got = {"y": y_tr, "H": H, "dxb": xb_g.grad[b_row0 : b_row0 + k_b], "dxa": None if xa is None else xa_g.grad,
           "grads": [(m.weight.grad, m.bias.grad if bias else None) for m in lin]}
    x64 = R.network_input(xa, xb, b_row0, k_b, S)
    failed = _compare(f"width {width} x {depth}, N {N}", W, Bk, x64, dy, [h > 0 for h in H], got, k_a, P, S)
    assert not failed, failed


def test_repeat_runs_give_the_same_bits(device):
    """(256, 3) at N = 2^16 - every workgroup of the forward / dX kernels walks two 128-sample tiles on 256 CUs, so the chunk
    sequence wraps from the output layer to the next tile's first layer, and the dW kernel runs two workgroups per partial row -
    20 times: y, the saved activations, dxb, dxa and the summed dW / db are the same bits in every run.  Each run's outputs are
    filled with NaN once compared (the allocator hands the next run the same buffers)."""
    from nesvor_amd import mlp

    width, depth, k_a, k_b, b_row0, rows, out_dim, S = 256, 3, 16, 15, 1, 16, 1, 16
    N = 1 << 16
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, True, 77, width=width)
    xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 3)
    first = None
    for rep in range(REPEATS):
        y, saved = mlp.wide_forward_raw(W, B, xa, xb, b_row0, k_b, S, True)
        dxb = torch.full((k_b, N), float("nan"), device=device)
        dxa, partial = mlp.wide_backward_raw(W, B, xa, xb, dy, saved, b_row0, k_b, S, dxb, True)
        cur = [y, dxb, dxa, partial.sum(0)] + list(saved)
        if first is None:
            first = cur
            assert all(torch.isfinite(t).all() for t in cur)
            continue
        for i, (a_, b_) in enumerate(zip(first, cur)):
            assert R.bits_equal(a_, b_), f"run {rep}: tensor {i} differs from run 0"
        for t in (y, dxb, dxa, partial, *saved):
            t.fill_(float("nan"))


def test_tinycudann_network_256(device):
    """``tinycudann.Network`` (bias-free, flat parameters, output rows padded to 16) with 256 neurons takes the wide kernels
    through ``wide_supported``: y, dx and dparams against the float64 matmul chain (the kernel's gates, read from a saving
    launch on the same parameters), the 4 x rule."""
    from nesvor_amd import mlp
    from nesvor_amd.tinycudann import Network

    n_in, n_out, N = 20, 5, 1000
    net = Network(n_in, n_out, {"otype": "CutlassMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 256,
                                "n_hidden_layers": 2}).to(device)
    assert mlp.wide_supported(net) and not mlp.supported(net)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, n_in, generator=g).to(device).requires_grad_(True)
    dy = torch.randn(N, n_out, generator=g).to(device)
    warned = Network._warned
    y = net(x)
    assert y.shape == (N, n_out) and Network._warned == warned  # (the module's own library fallback stayed unreached)
    y.backward(dy)
    W, off = [], 0
    for o, i in net.shapes:
        W.append(net.params.detach()[off : off + o * i].view(o, i))
        off += o * i
    xb = x.detach().t().contiguous()
    with torch.no_grad():
        y_tr, saved = torch.ops.nesvor.wide_mlp(None, xb, W, [], 0, n_in, 1, True)
    assert torch.equal(y_tr[:n_out].t(), y.detach())
    H = [R.saved_rows(s, N, blocks=16) for s in saved]
    dy16 = torch.zeros(16, N, device=device)
    dy16[:n_out] = dy.t()
    grads = list(R.split_partial(net.params.grad, W, []))
    assert not grads[-1][0][n_out:].any()  # the padding rows of the last layer keep a zero gradient
    got = {"y": y_tr, "H": H, "dxb": x.grad.t(), "grads": grads}
    # (y rows n_out .. 15 of the launch are the padded outputs: part of the same chain; the module returns the first n_out)
    failed = _compare("tinycudann.Network 256 x 2", W, [], R.network_input(None, xb, 0, n_in, 1), dy16, [h > 0 for h in H], got, 0, N, 1)
    assert not failed, failed


def test_c_abi_limits(device):
    """Width 256 is inside the limits (parameter count in nn.Linear order), 257 outside (-1; a launch: hipErrorInvalidValue);
    the saved buffers have sixteen blocks above width 128 and eight at 128.  One tiny forward at width 256."""
    from nesvor_amd import _lib, mlp

    lib = _lib.load()
    k_b, out_dim, N = 20, 3, 40
    n_pad = (N + 15) // 16 * 16
    W, B = R.make_net(device, 2, k_b, out_dim, True, 1, width=256)
    d = mlp._wide_desc(W, B, 0, k_b, 0, 1)
    assert lib.nesvor_mlp_wide_param_count(ctypes.byref(d)) == sum(w.numel() + b.numel() for w, b in zip(W, B))
    assert lib.nesvor_mlp_wide_saved_floats(ctypes.byref(d), N) == n_pad * 256
    for width, floats, count_ok in ((257, None, False), (129, n_pad * 256, True), (128, n_pad * 128, True)):
        d.width = width  # (the queries read the shape only)
        assert (lib.nesvor_mlp_wide_param_count(ctypes.byref(d)) > 0) == count_ok
        if floats is not None:
            assert lib.nesvor_mlp_wide_saved_floats(ctypes.byref(d), N) == floats
    d.width = 257
    assert lib.nesvor_mlp_wide_param_count(ctypes.byref(d)) == -1
    xb = torch.randn(k_b, N, device=device)
    y = torch.empty(out_dim, N, device=device)
    with torch.cuda.device(device):
        assert lib.nesvor_mlp_wide_forward(ctypes.byref(d), None, _lib.ptr(xb), _lib.ptr(y), None, N, _lib.stream_ptr()) == 1  # hipErrorInvalidValue
        d.width = 256
        assert lib.nesvor_mlp_wide_forward(ctypes.byref(d), None, _lib.ptr(xb), _lib.ptr(y), None, N, _lib.stream_ptr()) == 0
    _, y_ref = R.forward_chain(W, B, xb.t())
    assert R.rel_err(y.t(), y_ref) < 1e-5  # (a smoke check of the launch; test_kernels_vs_float64 holds the accuracy)


@pytest.mark.parametrize("width,depth", [(256, 1), (192, 2)])
def test_training_matches_oracle_losses(device, width, depth):
    """``--width`` 256 / 192 train through the autograd path on the chunked kernels: every loss of the first 10 iterations against
    the oracle's restatement of the reference loop from the same random stream (rtol 1e-4 plus the absolute floors of
    test_other_widths_and_depths_match_oracle_losses, whose construction this is); the library fallback is not reached;
    ``sample_points`` against the module path."""
    from nesvor_amd import mlp as mlp_mod
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.sample import sample_points
    from nesvor_amd.train import Dataset, train
    from oracle import train_loop as otl

    vol = torch.tensor(phantom3d(n=24), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3)
    args = small_args(device=device, n_iter=10, batch_size=256, n_samples=16, finest_resolution=1.0, log2_hashmap_size=14,
                      host_rng=True, width=width, depth=depth)
    ds = Dataset(slices, args)
    cds = otl.ArrayDataset(ds.xyz.cpu(), ds.v.cpu(), ds.slice_idx.cpu(), ds.transformation.matrix().cpu(), ds.resolution.cpu())
    hist = []
    warned = set(mlp_mod._warned_library)  # (process-global and never cleared: compared, not required to be empty)
    torch.manual_seed(0)
    inr, _, _ = train(slices, args, on_iteration=lambda i, losses: hist.append(torch.stack([losses[k].detach() for k in losses])))
    assert [l.out_features for l in inr.density_net if hasattr(l, "out_features")][:-1] == [width] * depth
    assert mlp_mod.wide_supported(inr.density_net) and not mlp_mod.supported(inr.density_net)
    assert mlp_mod._warned_library == warned, mlp_mod._warned_library - warned  # the library-GEMM fallback stayed unreachable
    torch.manual_seed(0)
    _, _, _, info = otl.train(cds, small_args(**{**vars(args), "device": torch.device("cpu")}))
    keys = list(info["history"][0].keys())
    got = torch.stack(hist).cpu().double().numpy()
    ref = np.array([[h[k] for k in keys] for h in info["history"]])
    assert got.shape == ref.shape
    for j, k in enumerate(keys):
        tol = 1e-4 * np.abs(ref[:, j]) + (1e-6 if k in ("transReg", "imageReg") else 1e-7)
        assert (np.abs(got[:, j] - ref[:, j]) <= tol).all(), (k, got[:, j], ref[:, j])
    args.no_output_psf = True
    pts = inr.bounding_box[0] + (inr.bounding_box[1] - inr.bounding_box[0]) * torch.rand(4096, 3, device=device)
    with torch.no_grad():
        ref_v = inr(pts[:, None], False).mean(-1)
    torch.testing.assert_close(sample_points(inr, pts, args), ref_v, rtol=1e-5, atol=1e-6)
    assert mlp_mod._warned_library == warned, mlp_mod._warned_library - warned


def test_partial_buffer_rule(device):
    """``wide_backward_raw``'s partial tensor: at most 256 MB at 256 x 7 hidden (1024 rows would be 1.7 GB) and not fewer rows
    than half the CUs (the library runs up to four workgroups per row there, two per CU - whose sums are compared with the float64
    chain here, at N = 888); 1024 rows at width 128, as before."""
    from nesvor_amd import mlp

    S, P, k_b, out_dim = 24, 37, 32, 16
    N = S * P
    for width, depth in ((256, 7), (128, 2)):
        W, B = R.make_net(device, depth, k_b, out_dim, True, 40 + width, width=width)
        _, xb, dy = R.make_inputs(device, 0, k_b, N, S, out_dim, 21)
        y, saved = mlp.wide_forward_raw(W, B, None, xb, 0, k_b, S, True)
        dxb = torch.empty(k_b, N, device=device)
        _, partial = mlp.wide_backward_raw(W, B, None, xb, dy, saved, 0, k_b, S, dxb, False)
        assert partial.shape[1] == sum(w.numel() + b.numel() for w, b in zip(W, B))
        if width == 128:
            assert partial.shape[0] == mlp.N_PARTIAL_WIDE == 1024
            continue
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        assert partial.numel() * 4 <= 256 << 20 and partial.numel() * 4 <= mlp.WIDE_PARTIAL_BYTES
        assert -(-2 * cus // mlp.WIDE_DW_MAX_PARTS) <= partial.shape[0] < 1024  # (two dW workgroups per CU at four per row)
        H = [R.saved_rows(s, N, blocks=16) for s in saved]
        got = {"y": y, "H": H, "dxb": dxb, "grads": R.split_partial(partial.sum(0), W, B)}
        failed = _compare("256 x 7 partial sums", W, B, R.network_input(None, xb, 0, k_b, S), dy, [h > 0 for h in H], got, 0, P, S)
        assert not failed, failed
