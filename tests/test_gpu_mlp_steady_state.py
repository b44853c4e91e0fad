"""Every MLP kernel instantiation the launchers take, at the steady state of its software pipeline.

The kernels of csrc/mlp.hip and csrc/mlp_wide.hip are persistent: a workgroup prefetches tile t + 1 while it computes tile t,
reuses its LDS images across tiles, and (the wave-specialised backward) hands groups through a ring between two wave roles.  The
hand-placed waits of those pipelines are exercised only when a workgroup iterates, so every case runs at a size where each
workgroup walks at least three tiles (prologue, steady state, epilogue) - asserted per case from the device's CU count and the
grid rule of every kernel the case took (``_assert_steady_state``) - and checks

1. bit reproducibility: 20 x (training forward, inference forward, backward) give the same bits in y, every saved buffer, dxb,
   dxa and every partial-sum row (each run's outputs are filled with NaN once compared, so that the next run, which gets the same
   buffers back from the allocator, cannot pass by leaving them alone); the inference output equals the training output bit for bit where both launches evaluate the
   same arithmetic, and within the scaled-fp16 test's 2e-3 where they do not by design (the compact kernels' VALU output
   layer for one output row; mode 4's training launch with a FULL save, which evaluates the full split where its inference
   launch evaluates the leading term alone - include/nesvor_hip.h, ``bf16_operands``);
2. accuracy against the same network in float64, the backward with the gates the kernel itself used (no cap on "bad"
   samples: a gate may differ from the float64 network's only where the pre-activation is below the mode's forward bound);
3. that the comparison of 2. FAILS when one 16-sample group of the kernel's own y / dxb is swapped with its neighbour (the
   signature of a stale register) - which keeps the tolerances honest.

Case -> kernels (``path`` is computed from the library's queries nesvor_mlp_backward_fused_ok / nesvor_mlp_compact_save_ok and
the saved-buffer sizes, printed, and asserted where the case is about a path; KB = input blocks, NH = hidden layers):

* fast shapes (S = 256; N = 2^18, and 2^19 where the backward is the wide pair: 256-sample tiles), fused backward on:
  - SPLIT / FP16S, KB <= 2: compact save - mlp_fwd_pf_kernel<KB, NH, split | leading term, save bits, compact[, VALU out]> +
    mlp_bwd_ws_kernel<KB, NH, ., split, compact[, VALU out]>; inference mlp_fwd_pf_kernel<KB, NH, ., no save>;
  - SPLIT / FP16S, KB = 3, 4: full save mlp_fwd_pf_kernel<3|4, NH, split, save>; NH = 1: mlp_bwd_ws_kernel<3|4, 1, ., split>;
    NH = 2 (refused by the fused kernel): wide_bwd_dx_kernel<4> + wide_bwd_dw_kernel<4>;
  - MFMA_FP32: mlp_fwd_pf_kernel<KB, NH, fp32, save | no save> + mlp_bwd_ws_kernel<KB, NH> (KB <= 2 or NH = 1), else the wide pair;
  - BF16 / FP16: mlp_fwd_kernel<KB, 1 | 2> + mlp_bwd_ws_kernel<KB, NH, 1 | 2> (KB <= 2 or NH = 1), else mlp_bwd_dx16_kernel<1 | 2>
    + mlp_bwd_dw16_kernel<1 | 2>;
  - S = 48 (3 groups per pixel, no power of two: ``spg_shift`` = -1) with pixel features: the same kernels' general pixel index;
* fast shapes with ``mlp.FUSED_BACKWARD = False``: full save, then the pair - wide_bwd_dx/dw<4> (MFMA_FP32, SPLIT, FP16S; N = 2^19;
  with pixel features these are the cases that run that kernel's dxa, row offset and single output row at steady state) or
  mlp_bwd_dx16 / dw16 (BF16, FP16);
* ragged / refused shapes: mlp_fwd_kernel<KB[, 1 | 2]> (any N, S, k_a; three hidden layers) + the same pairs (MFMA_FP32: at
  twice the N, for the wide pair's tiles);
* wide: wide_fwd_kernel<4 | 8>, wide_bwd_dx_kernel<4 | 8>, wide_bwd_dw_kernel<4 | 8> (width <= 64: 4; above: 8).  The
  width-64 / 40 cases come first, so that in a process that runs this module alone an HB = 4 launch precedes the first HB = 8
  one: the dynamic-LDS limit of wide_fwd_kernel<8> and wide_bwd_dx_kernel<8> is raised per (device, function) - it used to be
  one flag per kernel pointer TYPE, which the <4> and <8> instantiations share.  (A second device in the process is the
  other half of that fix; a one-GPU machine cannot test it.)

Tolerances.  16-bit modes: the bounds of the project's small-N tests of the same kernels, against the same reference
constructions (tests/test_gpu_ops.py::test_fused_mlp_bf16_operand_mode: 2e-3 of max; tests/test_gpu_mlp_half_pair.py::
test_pair_vs_emulated_reference: 2e-3 bf16 / 5e-4 fp16 for the pair; test_fused_mlp_scaled_fp16_mode: 3e-3 for y, 5e-3 for
gradients).  fp32-accuracy modes (MFMA_FP32, SPLIT, wide): per quantity, 4 x the error of the SAME gated chain evaluated by
torch in float32 on these inputs against the float64 chain (both sum the same number of fp32 terms in another order;
random-walk errors differ by a small constant).  The yardstick sums the bias gradients as a GEMM with a column of ones, like
dW: ``torch.sum`` is a pairwise tree whose error does not grow like a chain's (5e-9 at 2^18 terms, where a healthy chain sum
has 2e-8).  Every case prints both errors.

MEASURED (MI355X, this module's cases; max |error| / max |reference|, smallest .. largest over the cases):

=====================  ==================  ==================  ==================  ==================
quantity               torch fp32 chain    MFMA_FP32 kernels   SPLIT kernels       wide kernels
=====================  ==================  ==================  ==================  ==================
y                      2.2e-7 .. 3.6e-7    2.1e-7 .. 3.4e-7    1.5e-7 .. 2.8e-7    3.2e-7 .. 6.1e-7
                       (wide 3.2 .. 5.2)
hidden pre-activation  1.9e-7 .. 3.9e-7    1.9e-7 .. 4.0e-7    1.0e-7 .. 2.3e-7    1.9e-7 .. 5.2e-7
dxb                    1.8e-7 .. 2.8e-7    1.6e-7 .. 3.5e-7    1.5e-7 .. 2.8e-7    2.4e-7 .. 4.0e-7
                       (wide 2.4 .. 3.9)
dxa (per pixel)        1.1e-7 .. 2.6e-7    1.0e-7 .. 2.1e-7    8.5e-8 .. 3.0e-7    2.4e-7 .. 2.7e-7
dW                     1.8e-6 .. 7.0e-6    1.2e-7 .. 5.0e-7    1.2e-7 .. 1.6e-6    1.9e-7 .. 6.5e-7
                       (wide 2.3e-6 .. 1.2e-5)
db                     9.3e-8 .. 9.9e-6    2.2e-8 .. 2.9e-6    2.2e-8 .. 4.3e-6    2.6e-8 .. 4.5e-7
=====================  ==================  ==================  ==================  ==================

The largest kernel error / bound over all cases: y, pre-activations, dxb, dxa 0.26 .. 0.38; dW 0.14; db 0.48 (SPLIT).  The
16-bit modes against their fixed bounds: FP16S y <= 7.2e-4 (3e-3), gradients <= 6.6e-4 (5e-3); BF16 dxb <= 1.3e-3, dxa 5e-4,
dW 7e-5 (2e-3); FP16 dxb <= 2.9e-4, dxa 1.2e-4, dW 1.6e-5 (5e-4 pair / 2e-3 fused); y against the layer-wise emulation 1.7e-7.
Gates that differ from the reference network's: at most 2091 of 2^24 per layer (FP16S), the largest |pre-activation| among them
2.6e-4 of the layer's maximum; the fp32-accuracy modes: a handful per layer, below 5e-8.

One finding of these measurements is written down in include/nesvor_hip.h (``bf16_operands`` = 2): the hidden layers' bias
gradients of the SPLIT kernels carry a ONE-SIDED error (every entry too small, -1.2e-6 .. -1.9e-6 of max |db| on average at
N = 2^18 where the fp32-MFMA kernels have +-1e-7).  That is what was measured; the cause has not been isolated.  A hypothesis
that fits the sign and the growth with N - a one-signed error per term, as from accumulators that are not rounded to nearest in
the 16-bit MFMAs, adds up like N against a result that grows like sqrt(N) - has not been probed.  The error stays within 4 x the
float32 GEMM's here (0.48 of the bound at most).
"""
import ctypes

import pytest
import torch

import mlp_reference as R

pytestmark = pytest.mark.gpu

REPEATS = 20
MODES = ["MFMA_FP32", "SPLIT", "FP16S", "BF16", "FP16"]
DT16 = {"BF16": torch.bfloat16, "FP16": torch.float16}
FP32_MARGIN = 4.0


def _tiles_per_workgroup(N, samples_per_tile, max_workgroups):
    """The launchers' grid rule: min(tiles, max_workgroups) persistent workgroups striding over the tiles."""
    n_tiles = -(-N // samples_per_tile)
    return n_tiles // min(n_tiles, max_workgroups)  # (the least any workgroup walks)


def _assert_steady_state(device, N, forward, backward):
    """Every kernel the case launched walks at least three tiles per workgroup.  ``forward``: "64" (mlp.hip) | "wide";
    ``backward``: "fused" | "pair16" (mlp_bwd_dx16 / dw16) | "wide4" | "wide8" (wide_bwd_dx / dw) - what the caller read off the
    library's queries and the saved buffers.  The grid rules are the launchers':

    * mlp.hip forwards and mlp_bwd_dx16: 128-sample tiles; the plain kernels on min(tiles, 512) workgroups, the pipelined ones on
      CUs x min(occupancy, 2).  max(2 x CUs, 512) is neither launch's grid but a deliberately conservative bound for both;
    * wide forward and wide_bwd_dx<4 | 8>: 256-sample tiles on min(tiles, 2 x CUs) workgroups;
    * fused backward: 64 samples (one group per wave pair) per iteration on N_PARTIAL_FUSED workgroups;
    * dW kernels of both pairs: 64 samples (one group per wave) per iteration on N_PARTIAL (= N_PARTIAL_WIDE) workgroups."""
    from nesvor_amd import mlp

    cus = torch.cuda.get_device_properties(device).multi_processor_count
    assert mlp.N_PARTIAL == mlp.N_PARTIAL_WIDE
    t = {"forward": _tiles_per_workgroup(N, 128, max(2 * cus, 512)) if forward == "64" else _tiles_per_workgroup(N, 256, 2 * cus)}
    if backward == "fused":
        t["fused backward"] = _tiles_per_workgroup(N, 64, mlp.N_PARTIAL_FUSED)
    else:
        t["dW"] = _tiles_per_workgroup(N, 64, mlp.N_PARTIAL)
        t["dX"] = _tiles_per_workgroup(N, 128, max(2 * cus, 512)) if backward == "pair16" else _tiles_per_workgroup(N, 256, 2 * cus)
    assert min(t.values()) >= 3, (t, cus, N)
    return t


def _same_bits(first, cur, N, rep):
    """``cur`` (one run's outputs) has the bits of ``first``; then ``cur`` is filled with NaN.  The caching allocator hands a
    run the buffers the run before it gave back, so without the fill a kernel that skips some stores would find the right
    values already there.  Full-save buffers of a ragged N are compared without the padding lanes of their last 16-sample
    group (samples >= N: no kernel reads them, and no contract says what they hold)."""
    rem, G = N % 16, (N + 15) // 16
    for i, (a_, b_) in enumerate(zip(first, cur)):
        p, q = a_, b_
        if rem and a_.dim() == 1 and a_.numel() % (G * 256) == 0:
            p, q = a_.clone(), b_.clone()
            for t in (p, q):
                t.view(G, -1, 4, 16, 4)[-1, :, :, rem:, :] = 0  # [group][block][q][sample j][r]
        assert R.bits_equal(p, q), f"run {rep}: tensor {i} differs from run 0"
        b_.fill_(float("nan"))


def _queries(d, N):
    from nesvor_amd import _lib

    lib = _lib.load()
    return bool(lib.nesvor_mlp_backward_fused_ok(ctypes.byref(d), N)), bool(lib.nesvor_mlp_compact_save_ok(ctypes.byref(d), N))


class _Check:
    """Collects failed comparisons instead of raising: the sensitivity self-check needs the comparison to FAIL."""

    def __init__(self):
        self.failed, self.log = [], []

    def le(self, name, err, bound):
        self.log.append(f"{name} {err:.3g} <= {bound:.3g}")
        if not err <= bound:
            self.failed.append(f"{name}: {err:.3g} > {bound:.3g}")


def _swap_group(t, N):
    """A copy of the feature-major tensor t (rows, N) with ONE 16-sample group swapped with its neighbour."""
    g = (N // 16) // 2 + 1
    out = t.clone()
    out[:, 16 * g : 16 * g + 16], out[:, 16 * g + 16 : 16 * g + 32] = t[:, 16 * g + 16 : 16 * g + 32], t[:, 16 * g : 16 * g + 16]
    return out


def _gate_rule(chk, name, gates, pre, bound, first=0):
    """The kernel's gate may differ from the reference network's only where |pre-activation| < bound x max |pre-activation|."""
    for l, (g, p) in enumerate(zip(gates, pre), first):
        differ = g != (p > 0)
        worst = float((p.abs() * differ).max() / p.abs().max())
        chk.log.append(f"{name} layer {l}: {int(differ.sum())} gates differ")
        chk.le(f"{name} layer {l}: largest |pre| with another gate / max|pre|", worst, bound)


def _run_case(device, mode_name, depth, k_a, k_b, b_row0, rows, out_dim, S, N, fused_backward=True, expect=None):
    from nesvor_amd import mlp

    mode = getattr(mlp, mode_name)
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, True, 11 + depth + k_b)
    xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 5 + k_a)
    old = mlp.FUSED_BACKWARD
    mlp.FUSED_BACKWARD = fused_backward
    try:
        d = mlp.dims_desc(depth, out_dim, k_a, k_b, b_row0, S, mode)
        fused_ok, compact_ok = _queries(d, N)
        fused = fused_backward and fused_ok
        first = None
        for rep in range(REPEATS):
            y, saved = mlp.forward_raw(W, B, xa, xb, b_row0, k_b, S, True, mode)
            y_inf, _ = mlp.forward_raw(W, B, xa, xb, b_row0, k_b, S, False, mode)
            dxb = torch.full((k_b, N), float("nan"), device=device)
            dxa, partial = mlp.backward_raw(W, B, xa, xb, dy, saved, b_row0, k_b, S, dxb, xa is not None, mode)
            # (compact save: saved[1:] are 16-element placeholders no kernel touches)
            kept = saved[:1] if saved[0].numel() == (N + 15) // 16 * 16 * 4 else saved
            cur = [y, y_inf, dxb, partial] + list(kept) + ([dxa] if dxa is not None else [])
            if first is None:
                first = cur
            else:
                _same_bits(first, cur, N, rep)
    finally:
        mlp.FUSED_BACKWARD = old
    y, y_inf, dxb, partial = first[:4]
    n_pad = (N + 15) // 16 * 16
    compact = first[4].numel() == n_pad * 4
    saved = first[4 : 4 + (1 if compact else depth)]
    dxa = first[-1] if xa is not None else None
    assert compact == (fused_backward and compact_ok) and partial.shape[0] == (mlp.N_PARTIAL_FUSED if fused else mlp.N_PARTIAL)
    kb1 = (k_a + k_b + 15) // 16
    # the backward this case took: the fused kernel, else the 16-bit pair on 16-bit saved activations, else (fp32 data) the wide
    # kernels at width 64 - mlp_wide.hip's grid rule, not mlp.hip's
    backward = "fused" if fused else "pair16" if first[4].dtype != torch.float32 else "wide4"
    tiles = _assert_steady_state(device, N, "64", backward)
    path = f"{'compact' if compact else 'full'} save, {backward} backward, KB {kb1}, NH {depth}, out {out_dim}"
    print(f"\n{mode_name}: {path}; tiles per workgroup >= {tiles}")
    if expect is not None:
        assert (compact, fused) == expect, (path, expect)

    # inference launch against the training launch
    valu_out = compact and out_dim == 1
    # mode 4 on a shape the library saves compactly (its own query), asked for a FULL save: the training launch evaluates the full
    # split, the inference launch the leading term alone
    full_split_training = mode_name == "FP16S" and compact_ok and not compact
    if valu_out or full_split_training:
        assert float((y - y_inf).abs().max()) < 2e-3 * float(y.abs().max())
    else:
        assert torch.equal(y, y_inf)

    x64 = R.network_input(xa, xb, b_row0, k_b, S)
    P = N // S
    dxa_pix = None if dxa is None else dxa.double().view(P, -1, k_a).sum(1)
    flat = partial.double().sum(0)
    got_grads = R.split_partial(flat, W, B)

    if mode_name in DT16:
        dt, u = DT16[mode_name], R.UNIT_ROUNDOFF[DT16[mode_name]]
        assert saved[0].dtype == dt and not compact
        H = [R.saved_rows(s, N) for s in saved]
        pre, y_ref = R.emulated_forward_layers(W, B, x64, H, dt)
        dx_ref, g_ref = R.emulated_backward(W, B, xa, xb, dy, saved, b_row0, k_b, S, dt)
        tol_b = 2e-3 if (fused or mode_name == "BF16") else 5e-4

        def compare(y_, dxb_):
            chk = _Check()
            chk.le("y", R.rel_err(y_.t(), y_ref), 2e-3)
            _gate_rule(chk, "gate", [h > 0 for h in H], pre, 2e-3)
            for l, (h, p) in enumerate(zip(H, pre)):
                # saved = round16(fp32 sum): the sum within 2e-3 of max (the bound the project holds), the rounding within u |value|
                m = float(p.abs().max())
                excess = ((h - p.relu()).abs() - u * (p.relu() + 2e-3 * m)).max()
                chk.le(f"saved {l}", float(excess) / m, 2e-3)
            chk.le("dxb", R.rel_err(dxb_.t(), dx_ref[:, k_a:]), tol_b)
            if dxa_pix is not None:
                chk.le("dxa", R.rel_err(dxa_pix, dx_ref[:, :k_a].view(P, S, k_a).sum(1)), tol_b)
            for l, ((dw, db), (dw_r, db_r)) in enumerate(zip(got_grads, g_ref)):
                chk.le(f"dW{l}", R.rel_err(dw, dw_r), tol_b)
                chk.le(f"db{l}", R.rel_err(db, db_r), tol_b)
            return chk
    else:
        gates = R.compact_gates(saved[0], N, depth) if compact else [R.saved_rows(s, N) > 0 for s in saved]
        ref = R.gated_chain(W, B, x64, dy, gates)
        if mode_name == "FP16S":
            bound = {"y": 3e-3, "pre": 3e-3, "grad": 5e-3}
            e32 = None
        else:
            c32 = R.gated_chain(W, B, x64, dy, gates, torch.float32)
            e32 = {"y": R.rel_err(c32["y"], ref["y"]), "dxb": R.rel_err(c32["dx"][:, k_a:], ref["dx"][:, k_a:]),
                   "pre": [R.rel_err(a_, b_) for a_, b_ in zip(c32["pre"], ref["pre"])]}
            if k_a:
                e32["dxa"] = R.rel_err(c32["dx"][:, :k_a].view(P, S, k_a).sum(1), ref["dx"][:, :k_a].view(P, S, k_a).sum(1))
            for l, ((dw, db), (dw_r, db_r)) in enumerate(zip(c32["grads"], ref["grads"])):
                e32[f"dW{l}"], e32[f"db{l}"] = R.rel_err(dw, dw_r), R.rel_err(db, db_r)
            print("torch fp32 chain vs fp64:", {k: (f"{v:.3g}" if not isinstance(v, list) else [f"{x:.3g}" for x in v]) for k, v in e32.items()})

        def compare(y_, dxb_):
            chk = _Check()
            b_ = (lambda k: FP32_MARGIN * e32[k]) if e32 is not None else (lambda k: bound["y"] if k == "y" else bound["grad"])
            chk.le("y", R.rel_err(y_.t(), ref["y"]), b_("y"))
            for l, (g, p) in enumerate(zip(gates, ref["pre"])):
                pb = FP32_MARGIN * e32["pre"][l] if e32 is not None else bound["pre"]
                _gate_rule(chk, "gate", [g], [p], pb, l)
                if not compact:
                    chk.le(f"saved {l}", R.rel_err(R.saved_rows(saved[l], N), p.relu()), pb)
            chk.le("dxb", R.rel_err(dxb_.t(), ref["dx"][:, k_a:]), b_("dxb"))
            if dxa_pix is not None:
                chk.le("dxa", R.rel_err(dxa_pix, ref["dx"][:, :k_a].view(P, S, k_a).sum(1)), b_("dxa"))
            for l, ((dw, db), (dw_r, db_r)) in enumerate(zip(got_grads, ref["grads"])):
                chk.le(f"dW{l}", R.rel_err(dw, dw_r), b_(f"dW{l}"))
                chk.le(f"db{l}", R.rel_err(db, db_r), b_(f"db{l}"))
            return chk

    chk = compare(y, dxb)
    print("kernel vs reference:", "; ".join(chk.log))
    assert not chk.failed, chk.failed
    # sensitivity self-check: one swapped group in y, then in dxb, must be noticed
    assert compare(_swap_group(y, N), dxb).failed, "a swapped group of y passes the comparison"
    assert compare(y, _swap_group(dxb, N)).failed, "a swapped group of dxb passes the comparison"


def _n_64(mode, fused):
    """N of a fast-shape case: 2^18 - 2048 tiles of 128 samples, 4 per workgroup in the 64-wide forwards and mlp_bwd_dx16, 16
    iterations of the fused backward - except where the backward is the pair in an fp32-data mode: that pair is the WIDE kernels
    at width 64, whose dX kernel walks 256-sample tiles on 2 x CUs workgroups (2 tiles each at 2^18 on 256 CUs: a prologue and an
    epilogue, no steady state), so those cases run at 2^19 (4 tiles each).  _run_case asserts the count for the kernels it took."""
    return 1 << 19 if (not fused and mode not in DT16) else 1 << 18


FAST_INPUTS = [  # (k_a, k_b, b_row0, rows, out_dim)
    (0, 16, 0, 16, 16), (0, 16, 0, 16, 1),
    (0, 32, 0, 32, 16), (0, 32, 0, 32, 1),
    (16, 15, 1, 16, 16), (16, 15, 1, 16, 1),   # pixel features, row offset
    (0, 48, 0, 48, 16),                        # three input blocks
    (16, 48, 0, 48, 16),                       # four, pixel features
]


@pytest.mark.parametrize("k_a,k_b,b_row0,rows,out_dim", FAST_INPUTS)
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("mode", MODES)
def test_fast_shapes_at_steady_state(device, mode, depth, k_a, k_b, b_row0, rows, out_dim):
    """N = 2^18, S = 256, biased networks, the library's default switches: the pipelined / plain forward and the fused backward
    (the pair where the fused kernel refuses: more than two input blocks at two hidden layers).  Measured errors behind the
    bounds: MEASURED in the module docstring (fp32-accuracy modes: y 1.5e-7 .. 3.4e-7 against a torch-fp32 chain's 2.2e-7 .. 3.6e-7)."""
    kb1 = (k_a + k_b + 15) // 16
    fused = kb1 <= 2 or depth == 1
    compact = mode in ("SPLIT", "FP16S") and kb1 <= 2
    _run_case(device, mode, depth, k_a, k_b, b_row0, rows, out_dim, 256, _n_64(mode, fused), expect=(compact, fused))


@pytest.mark.parametrize("mode", MODES)
def test_fast_shape_whose_pixel_is_no_power_of_two_groups(device, mode):
    """Pixel features at S = 48: three 16-sample groups per pixel, so the kernels cannot shift to get a group's pixel
    (``spg_shift`` = -1) and take the general index.  N = 48 x 5464 = 2049 whole 128-sample tiles."""
    assert (48 // 16) & (48 // 16 - 1) != 0
    _run_case(device, mode, 2, 16, 15, 1, 16, 1, 48, 48 * 5464, expect=(mode in ("SPLIT", "FP16S"), True))


@pytest.mark.parametrize("k_a,k_b,b_row0,rows,out_dim", FAST_INPUTS[2:6])
@pytest.mark.parametrize("mode", MODES)
def test_fast_shapes_pair_backward_at_steady_state(device, mode, k_a, k_b, b_row0, rows, out_dim):
    """``mlp.FUSED_BACKWARD = False`` at two hidden layers: the full-save forward and the dX + dW pair (the wide kernels at width 64
    in the fp32-data modes - which therefore run at N = 2^19, ``_n_64`` -, the 16-bit pair in BF16 / FP16) at steady state.  The
    fp32-data cases with pixel features are the only ones that run wide_bwd_dx_kernel<4>'s pixel-feature gradient, row offset and
    single output row at steady state: test_wide_kernels_at_steady_state has no pixel features at width <= 64."""
    _run_case(device, mode, 2, k_a, k_b, b_row0, rows, out_dim, 256, _n_64(mode, False), fused_backward=False, expect=(False, False))


RAGGED = [  # (depth, k_a, k_b, S, pixels at 128-sample dX tiles (BF16 / FP16), pixels at 256-sample dX tiles (MFMA_FP32: wide pair))
    (2, 16, 15, 8, 32771, 65539),   # N = 262 168 / 524 312: 8 samples into a last 16-group
    (3, 16, 15, 24, 10923, 21847),  # N = 262 152 / 524 328
    (3, 0, 24, 16, 1 << 14, 1 << 15),
    (2, 8, 15, 16, 1 << 14, 1 << 15),
    (2, 0, 64, 16, 1 << 14, 1 << 15),
]


@pytest.mark.parametrize("depth,k_a,k_b,S,P,P_wide", RAGGED)
@pytest.mark.parametrize("mode", ["MFMA_FP32", "BF16", "FP16"])
def test_ragged_and_refused_shapes_at_steady_state(device, mode, depth, k_a, k_b, S, P, P_wide):
    """Shapes the pipelined forward and / or the fused backward refuse (N not a multiple of 16, S or k_a no multiple of 16, three
    hidden layers, four input blocks at two hidden layers): the plain forward (the pipelined one where it takes the shape: fp32
    data, whole tiles, at most two hidden layers) and the dX + dW pair.  N = 8 x 32771, 24 x 10923 and 2^18 in BF16 / FP16; in
    MFMA_FP32 the pair is the wide kernels' (256-sample tiles, two per workgroup at those sizes), so N = 8 x 65539, 24 x 21847 and
    2^19 there - as ragged in 16 as the smaller ones."""
    N = S * (P_wide if mode not in DT16 else P)
    assert N % 16 == (S * P) % 16
    _run_case(device, mode, depth, k_a, k_b, 0, k_b, 16 if k_a == 0 else 1, S, N, expect=(False, False))


WIDE = [  # (width, depth, k_a, k_b, b_row0, rows, out_dim, bias): the shapes of test_wide_mlp_vs_fp64_reference, HB = 4 first
    (64, 4, 0, 32, 0, 32, 16, True), (40, 7, 0, 20, 2, 24, 3, True),
    (128, 1, 0, 32, 0, 32, 16, True), (128, 2, 0, 32, 0, 32, 16, False), (128, 4, 16, 15, 1, 16, 1, True), (96, 5, 16, 8, 0, 8, 1, True)]


@pytest.mark.parametrize("width,depth,k_a,k_b,b_row0,rows,out_dim,bias", WIDE)
def test_wide_kernels_at_steady_state(device, width, depth, k_a, k_b, b_row0, rows, out_dim, bias):
    """csrc/mlp_wide.hip through ``wide_forward_raw`` / ``wide_backward_raw`` at N = 24 x 21847 = 524 328 (S = 24, ragged in 16:
    2049 tiles of 256 samples, the last one 40 samples): wide_fwd_kernel / wide_bwd_dx_kernel / wide_bwd_dw_kernel <4> (width <= 64)
    and <8>.  The HB = 4 cases run first: the <8> kernels must get their own dynamic-LDS limit although a <4> launch of the same
    pointer type came before them (raise_lds is keyed per device and function; the second device of that key cannot be tested on a
    one-GPU machine).  Bounds: 4 x the torch-fp32 chain's error, per quantity (module docstring; measured: y 3.2e-7 .. 6.1e-7 against the
    torch-fp32 chain's 3.2e-7 .. 5.2e-7, dxb 2.4e-7 .. 4.0e-7 against 2.4e-7 .. 3.9e-7, dW 1.9e-7 .. 6.5e-7 against 2.3e-6 .. 1.2e-5)."""
    from nesvor_amd import _lib, mlp

    S, P = 24, 21847
    N = S * P
    assert N % 16 != 0
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, bias, 100 + width + depth, width=width)
    Bk = B if bias else []
    xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 9)
    hb = 4 if width <= 64 else 8
    d = mlp._wide_desc(W, Bk, k_a, k_b, b_row0, S)
    assert _lib.load().nesvor_mlp_wide_saved_floats(ctypes.byref(d), N) == (N + 15) // 16 * 16 * 16 * hb  # (the library's own HB)
    tiles = _assert_steady_state(device, N, "wide", f"wide{hb}")
    print(f"\nwide kernels <{hb}>: width {width}, NH {depth}, {'biased' if bias else 'bias-free'}; tiles per workgroup >= {tiles}")
    first = None
    for rep in range(REPEATS):
        y, saved = mlp.wide_forward_raw(W, Bk, xa, xb, b_row0, k_b, S, True)
        y_inf, _ = mlp.wide_forward_raw(W, Bk, xa, xb, b_row0, k_b, S, False)
        dxb = torch.full((k_b, N), float("nan"), device=device)
        dxa, partial = mlp.wide_backward_raw(W, Bk, xa, xb, dy, saved, b_row0, k_b, S, dxb, xa is not None)
        cur = [y, y_inf, dxb, partial] + list(saved) + ([dxa] if dxa is not None else [])
        if first is None:
            first = cur
        else:
            _same_bits(first, cur, N, rep)
    y, y_inf, dxb, partial = first[:4]
    saved = first[4 : 4 + depth]
    dxa = first[4 + depth] if xa is not None else None
    assert torch.equal(y, y_inf)
    x64 = R.network_input(xa, xb, b_row0, k_b, S)
    H = [R.saved_rows(s, N, hb)[:, :width] for s in saved]
    gates = [h > 0 for h in H]
    ref = R.gated_chain(W, Bk, x64, dy, gates)
    c32 = R.gated_chain(W, Bk, x64, dy, gates, torch.float32)
    dxa_pix = None if dxa is None else dxa.double().view(P, S, k_a).sum(1)
    got_grads = R.split_partial(partial.double().sum(0), W, Bk)
    pix = lambda t: t[:, :k_a].view(P, S, k_a).sum(1)

    def compare(y_, dxb_):
        chk = _Check()
        both = lambda name, got, a32, a64: (chk.log.append(f"[torch fp32 {name} {R.rel_err(a32, a64):.3g}]"),
                                            chk.le(name, R.rel_err(got, a64), FP32_MARGIN * R.rel_err(a32, a64)))
        both("y", y_.t(), c32["y"], ref["y"])
        for l in range(depth):
            pb = FP32_MARGIN * R.rel_err(c32["pre"][l], ref["pre"][l])
            _gate_rule(chk, "gate", [gates[l]], [ref["pre"][l]], pb, l)
            chk.le(f"saved {l}", R.rel_err(H[l], ref["pre"][l].relu()), pb)
        both("dxb", dxb_.t(), c32["dx"][:, k_a:], ref["dx"][:, k_a:])
        if dxa_pix is not None:
            both("dxa", dxa_pix, pix(c32["dx"]), pix(ref["dx"]))
        for l in range(depth + 1):
            both(f"dW{l}", got_grads[l][0], c32["grads"][l][0], ref["grads"][l][0])
            if bias:
                both(f"db{l}", got_grads[l][1], c32["grads"][l][1], ref["grads"][l][1])
        return chk

    chk = compare(y, dxb)
    print("kernel vs reference:", "; ".join(chk.log))
    assert not chk.failed, chk.failed
    assert compare(_swap_group(y, N), dxb).failed, "a swapped group of y passes the comparison"
    assert compare(y, _swap_group(dxb, N)).failed, "a swapped group of dxb passes the comparison"
