"""The operand bounds the producing kernels publish are EXACT at their producers.

The scaled MLP modes (SPLIT, FP16S) pick their power-of-two operand scales from bounds that the kernel which WROTE the operand
publishes: the hash-grid forward max |pe|, the MLP forwards ``y_absmax``, the loss kernel ``dz0_absmax`` / ``dlog_var_absmax`` /
``dlog_bias_absmax``, the MLP backwards ``dx_absmax`` (which also scales the hash-grid backward's fixed-point sums).  ``pow2_scale``
leaves a factor of two below fp16 overflow, so a producer that skips a tail group, a masked lane or a last row under-reports, and
its consumer saturates - on the batches whose extreme value sits in the skipped place only.

Contract checked here: after zero-filling, the published value EQUALS ``tensor.abs().max()`` - it is a maximum of the very floats
that were stored (slotted bounds: the maximum over the 16 slots, 64 floats apart; ``dx_absmax``: the scalar).  And the maximum is
MOVED to the places a kernel can skip: the argmax sample of a first run is swapped with the sample at the first / last position,
in the last partially filled 16-sample group (ragged N), at the end of the first tile and at the start of the last tile (which some
workgroup handles in its last iteration) - whole pixels where pixel features or the loss's pixel structure apply (the loss: plus
the reversal of the pixel's samples, which keeps its s <-> S - 1 - s pairs) - the argmax is asserted to have landed there, and
the bound must still be exact.  One variant per producer has a negative extremum.

Planted values stay finite and moderate; nothing here feeds inf / NaN or makes a consumer overflow.
"""
import ctypes

import pytest
import torch

import mlp_reference as R

pytestmark = pytest.mark.gpu


def _slotted():
    from nesvor_amd import mlp

    return mlp.ABSMAX_FLOATS


def _slot_max(buf):
    """A slotted bound: the maximum over the 16 slots, 64 floats apart."""
    return float(buf.view(16, 64)[:, 0].max())


def _targets(N, tile, pixel=None):
    """Sample positions a kernel can skip.  ``tile``: samples per workgroup iteration of the producer."""
    n_tiles = -(-N // tile)
    t = {"first sample": 0, "last sample": N - 1, "last sample of the first tile": min(tile, N) - 1,
         "first sample of the last tile": (n_tiles - 1) * tile}
    if N % 16:
        t["first sample of the partial 16-group"] = N - N % 16
    return t


def _move(N, S, src, dst, pixels, device):
    """Sample permutation (new[:, i] = old[:, perm[i]]) that brings sample ``src`` to position ``dst`` by a swap - with ``pixels``:
    a swap of the two whole pixels, then of two samples inside the target pixel - and the pixel permutation (or None)."""
    perm = torch.arange(N)
    pp = None
    if pixels:
        pp = torch.arange(N // S)
        ps, pd = src // S, dst // S
        pp[ps], pp[pd] = pd, ps
        perm = (pp[:, None] * S + torch.arange(S)[None]).reshape(-1)
        a = pd * S + src % S
        va, vb = int(perm[a]), int(perm[dst])
        perm[a], perm[dst] = vb, va
        pp = pp.to(device)
    else:
        perm[src], perm[dst] = dst, src
    return perm.to(device), pp


def _check_everywhere(run, xa, xb, dy, S, N, tile, negative=None):
    """run(xa, xb, dy) -> (tensor (rows, N), published bound).  Exact as given, and with the extreme sample moved to every target."""
    t, b = run(xa, xb, dy)
    assert b == float(t.abs().max()) and b > 0, ("as given", b, float(t.abs().max()))
    src = int(t.abs().amax(0).argmax())
    if negative is not None:
        col = t[:, src]
        assert float(col[col.abs().argmax()]) < 0, "the extremum was meant to be negative"
    seen = []
    for name, dst in _targets(N, tile).items():
        perm, pp = _move(N, S, src, dst, xa is not None, xb.device)
        t, b = run(None if xa is None else xa[pp].contiguous(), xb[:, perm].contiguous(), None if dy is None else dy[:, perm].contiguous())
        assert int(t.abs().amax(0).argmax()) == dst, (name, dst, int(t.abs().amax(0).argmax()))
        assert b == float(t.abs().max()), (name, b, float(t.abs().max()))
        seen.append(name)
    return seen


def _queries(mode, depth, out_dim, k_a, k_b, b_row0, S, N):
    from nesvor_amd import _lib, mlp

    d = mlp.dims_desc(depth, out_dim, k_a, k_b, b_row0, S, mode)
    lib = _lib.load()
    return bool(lib.nesvor_mlp_backward_fused_ok(ctypes.byref(d), N)), bool(lib.nesvor_mlp_compact_save_ok(ctypes.byref(d), N))


# ------------------------------------------------------------------------------------------------ y_absmax (MLP forwards)
Y_CASES = [
    # id, mode, depth, (k_a, k_b, b_row0, rows), out_dim, S, N, fused_backward, bias_free, expected save ("compact" | "full")
    ("pf-compact-split-out16", "SPLIT", 2, (0, 32, 0, 32), 16, 256, 1 << 17, True, False, "compact"),
    ("pf-compact-split-out1", "SPLIT", 2, (16, 15, 1, 16), 1, 256, 1 << 17, True, False, "compact"),
    ("pf-compact-fp16s-out16", "FP16S", 1, (0, 16, 0, 16), 16, 256, 1 << 17, True, False, "compact"),
    ("pf-compact-fp16s-out1", "FP16S", 2, (16, 15, 1, 16), 1, 256, 1 << 17, True, False, "compact"),
    ("pf-full-split-out16", "SPLIT", 1, (0, 48, 0, 48), 16, 256, 1 << 17, True, False, "full"),
    ("pf-full-split-out1", "SPLIT", 2, (16, 15, 1, 16), 1, 256, 1 << 17, False, False, "full"),
    ("pf-full-fp16s-out16", "FP16S", 2, (0, 32, 0, 32), 16, 256, 1 << 17, False, False, "full"),
    ("pf-full-fp16s-out1", "FP16S", 1, (16, 48, 0, 48), 1, 256, 1 << 17, True, False, "full"),
    ("pf-mfma-out16", "MFMA_FP32", 2, (0, 32, 0, 32), 16, 256, 1 << 17, True, False, "full"),
    ("pf-mfma-out1", "MFMA_FP32", 1, (16, 15, 1, 16), 1, 256, 1 << 17, True, False, "full"),
    ("plain-ragged-fp32", "MFMA_FP32", 2, (16, 15, 1, 16), 1, 8, 8 * 16389, True, False, "full"),
    ("plain-ragged-split", "SPLIT", 3, (0, 24, 0, 24), 16, 8, 8 * 16389, True, False, "full"),
    ("plain-ragged-bf16", "BF16", 2, (16, 15, 1, 16), 1, 8, 8 * 16389, True, False, "full"),
    ("plain-ragged-fp16", "FP16", 3, (0, 24, 0, 24), 16, 8, 8 * 16389, True, False, "full"),
    ("plain-bf16-fast", "BF16", 2, (0, 32, 0, 32), 16, 256, 1 << 17, True, False, "full"),
    ("bias-free-full-save", "FP16S", 2, (0, 32, 0, 32), 16, 256, 1 << 17, False, True, "full"),
    ("bias-free-ragged", "FP16S", 2, (16, 15, 1, 16), 1, 8, 8 * 16389, True, True, "full"),
]


# (a negative extremum: once per kernel family)
Y_NEGATIVE = ("pf-compact-split-out16", "pf-compact-fp16s-out1", "pf-full-split-out16", "pf-mfma-out1", "plain-ragged-fp32",
              "plain-ragged-bf16", "bias-free-full-save")
Y_PARAMS = [(c, False) for c in Y_CASES] + [(c, True) for c in Y_CASES if c[0] in Y_NEGATIVE]


@pytest.mark.parametrize("case,negative", Y_PARAMS, ids=[c[0] + ("-negative" if n else "") for c, n in Y_PARAMS])
def test_mlp_forward_publishes_exact_y_absmax(device, case, negative):
    """``nesvor_mlp_t.y_absmax`` from every forward: the pipelined kernel with a compact and with a full save and without a save
    (SPLIT, FP16S, fp32 MFMAs; MFMA and VALU output layer), the plain kernel at ragged N (fp32 data, BF16, FP16), and the
    bias-free full-save path (the wide kernels at width 64 plus one pass over y).  The training and the inference launch both
    publish."""
    from nesvor_amd import _lib, mlp

    _, mode_name, depth, (k_a, k_b, b_row0, rows), out_dim, S, N, fused_backward, bias_free, expect = case
    mode = getattr(mlp, mode_name)
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, not bias_free, 21 + depth)
    Bk = [None] * len(W) if bias_free else B
    xa, xb, _dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 3 + k_a)
    fused_ok, compact_ok = _queries(mode, depth, out_dim, k_a, k_b, b_row0, S, N)
    print(f"\n{case[0]}: fused_ok {fused_ok}, compact_ok {compact_ok}, bias-free {bias_free}")
    if bias_free:
        d = mlp._desc(W, Bk, k_a, k_b, b_row0, S, mode)
        assert _lib.load().nesvor_mlp_bias_free_ok(ctypes.byref(d), N)
    sign = [1.0]
    old = mlp.FUSED_BACKWARD
    mlp.FUSED_BACKWARD = fused_backward
    try:
        for need_saved in (True, False):
            def run(xa_, xb_, dy_):
                buf = torch.zeros(_slotted(), device=device)
                Wk = W[:-1] + [W[-1] * sign[0]]
                Bq = Bk if bias_free else B[:-1] + [B[-1] * sign[0]]
                y, saved = mlp.forward_raw(Wk, Bq, xa_, xb_, b_row0, k_b, S, need_saved, mode, y_absmax=buf)
                if need_saved:
                    assert (saved[0].numel() == (N + 15) // 16 * 16 * 4) == (expect == "compact"), case[0]
                return y, _slot_max(buf)

            if negative:  # make the extremum negative: flip the output layer if it is positive
                y, _b = run(xa, xb, None)
                col = y[:, int(y.abs().amax(0).argmax())]
                if float(col[col.abs().argmax()]) > 0:
                    sign[0] = -sign[0]
            _check_everywhere(run, xa, xb, None, S, N, 128, negative=True if negative else None)
    finally:
        mlp.FUSED_BACKWARD = old


# ------------------------------------------------------------------------------------------------ dx_absmax (MLP backwards)
DX_CASES = [
    # id, mode, depth, (k_a, k_b, b_row0, rows), out_dim, S, N, fused_backward, expected (compact, fused), samples per iteration
    ("ws-compact-split", "SPLIT", 2, (0, 32, 0, 32), 16, 256, 1 << 17, True, (True, True), 64),
    ("ws-compact-fp16s", "FP16S", 1, (16, 15, 1, 16), 16, 256, 1 << 17, True, (True, True), 64),
    ("ws-compact-out1", "SPLIT", 2, (16, 15, 1, 16), 1, 256, 1 << 17, True, (True, True), 64),
    ("ws-full-mfma", "MFMA_FP32", 2, (16, 15, 1, 16), 1, 256, 1 << 17, True, (False, True), 64),
    ("ws-full-split-kb3", "SPLIT", 1, (0, 48, 0, 48), 16, 256, 1 << 17, True, (False, True), 64),
    ("ws-full-bf16", "BF16", 2, (0, 32, 0, 32), 16, 256, 1 << 17, True, (False, True), 64),
    ("ws-full-fp16", "FP16", 1, (16, 48, 0, 48), 16, 256, 1 << 17, True, (False, True), 64),
    ("dx16-bf16-ragged", "BF16", 3, (16, 15, 1, 16), 1, 24, 24 * 5463, True, (False, False), 128),
    ("dx16-fp16-ragged", "FP16", 2, (0, 64, 0, 64), 16, 8, 8 * 16389, True, (False, False), 128),
    ("wide64-fp32-ragged", "MFMA_FP32", 3, (16, 15, 1, 16), 1, 24, 24 * 10923, True, (False, False), 256),
    ("wide64-split-refused", "SPLIT", 2, (0, 48, 0, 48), 16, 256, 1 << 18, True, (False, False), 256),
]


DX_NEGATIVE = ("ws-compact-split", "ws-full-bf16", "dx16-bf16-ragged", "wide64-fp32-ragged")
DX_PARAMS = [(c, False) for c in DX_CASES] + [(c, True) for c in DX_CASES if c[0] in DX_NEGATIVE]


@pytest.mark.parametrize("case,negative", DX_PARAMS, ids=[c[0] + ("-negative" if n else "") for c, n in DX_PARAMS])
def test_mlp_backward_publishes_exact_dx_absmax(device, case, negative):
    """``dxb_absmax`` of ``nesvor_mlp_backward_bounded``: the fused backward with a compact save (SPLIT, FP16S, VALU output layer)
    and with a full save (fp32 MFMAs, SPLIT with three input blocks, BF16, FP16), the 16-bit dX + dW pair, and the wide dX kernel at
    width 64 (shapes the fused kernel refuses).  With pixel features the first-layer columns of xa are scaled up so that dxa
    exceeds dxb everywhere: the bound is max |dxb|, not max |dX|."""
    from nesvor_amd import mlp

    name, mode_name, depth, (k_a, k_b, b_row0, rows), out_dim, S, N, fused_backward, expect, tile = case
    mode = getattr(mlp, mode_name)
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, True, 31 + depth)
    if k_a:
        W[0][:, :k_a] *= 16.0
    xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 7 + k_a)
    if k_a:
        xa = xa / 16.0  # (the forward sees the same products)
    fused_ok, compact_ok = _queries(mode, depth, out_dim, k_a, k_b, b_row0, S, N)
    assert (compact_ok, fused_ok) == expect, (name, compact_ok, fused_ok)
    print(f"\n{name}: fused_ok {fused_ok}, compact_ok {compact_ok}")
    sign = [1.0]

    def run(xa_, xb_, dy_):
        _, saved = mlp.forward_raw(W, B, xa_, xb_, b_row0, k_b, S, True, mode)
        assert (saved[0].numel() == (N + 15) // 16 * 16 * 4) == expect[0]
        dxb = torch.full((k_b, N), float("nan"), device=device)
        bound = torch.zeros(1, device=device)
        dxa, partial = mlp.backward_raw(W, B, xa_, xb_, dy_ * sign[0], saved, b_row0, k_b, S, dxb, xa_ is not None, mode, dxb_absmax=bound)
        assert partial.shape[0] == (mlp.N_PARTIAL_FUSED if expect[1] else mlp.N_PARTIAL)
        if dxa is not None:
            assert float(dxa.abs().max()) > float(dxb.abs().max())
        return dxb, float(bound)

    if negative:
        dxb, _b = run(xa, xb, dy)
        col = dxb[:, int(dxb.abs().amax(0).argmax())]
        if float(col[col.abs().argmax()]) > 0:
            sign[0] = -1.0
    _check_everywhere(run, xa, xb, dy, S, N, tile, negative=True if negative else None)


@pytest.mark.parametrize("k_a,k_b,b_row0,rows,out_dim,bias", [(0, 32, 0, 32, 16, True), (16, 15, 1, 16, 1, True), (0, 32, 0, 32, 16, False)])
def test_wide_backward_publishes_exact_dx_absmax(device, k_a, k_b, b_row0, rows, out_dim, bias):
    """``nesvor_mlp_wide_backward_bounded`` at width 128 (wide_bwd_dx_kernel<8>), ragged N = 24 x 10923 (1025 tiles of 256 samples,
    the last one 8 samples)."""
    from nesvor_amd import _lib, mlp

    S, N, depth, width = 24, 24 * 10923, 2, 128
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, bias, 41, width=width)
    Bk = B if bias else []
    if k_a:
        W[0][:, :k_a] *= 16.0
    xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 13)
    if k_a:
        xa = xa / 16.0
    lib = _lib.load()

    def run(xa_, xb_, dy_):
        _, saved = mlp.wide_forward_raw(W, Bk, xa_, xb_, b_row0, k_b, S, True)
        d = mlp._wide_desc(W, Bk, k_a, k_b, b_row0, S)
        dpre = [torch.empty_like(s) for s in saved]
        dxa = torch.empty((N, k_a), device=device) if k_a else None
        dxb = torch.full((k_b, N), float("nan"), device=device)
        partial = torch.empty((mlp.N_PARTIAL_WIDE, lib.nesvor_mlp_wide_param_count(ctypes.byref(d))), device=device)
        bound = torch.zeros(1, device=device)
        with torch.cuda.device(device):
            err = lib.nesvor_mlp_wide_backward_bounded(ctypes.byref(d), _lib.ptr(xa_), _lib.ptr(xb_), _lib.ptr(dy_), mlp._ptr_array8(saved),
                                                       mlp._ptr_array8(dpre), _lib.ptr(dxa), _lib.ptr(dxb), _lib.ptr(partial),
                                                       mlp.N_PARTIAL_WIDE, N, _lib.ptr(bound), _lib.stream_ptr())
        _lib.check(err, "wide backward")
        if dxa is not None:
            assert float(dxa.abs().max()) > float(dxb.abs().max())
        return dxb, float(bound)

    _check_everywhere(run, xa, xb, dy, S, N, 256)


def test_all_zero_dy_leaves_the_bound_zero(device):
    """An all-zero upstream gradient through the scaled-mode backward: every bound stays 0 (``pow2_scale`` clamps instead of
    dividing by it), dxb and the partial sums are exact zeros and finite."""
    from nesvor_amd import mlp

    N, S = 1 << 14, 256
    for mode, (k_a, k_b, b_row0, rows, out_dim) in ((mlp.SPLIT, (0, 32, 0, 32, 16)), (mlp.FP16S, (16, 15, 1, 16, 1))):
        W, B = R.make_net(device, 2, k_a + k_b, out_dim, True, 51)
        xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 17)
        dy.zero_()
        _, saved = mlp.forward_raw(W, B, xa, xb, b_row0, k_b, S, True, mode)
        dxb = torch.full((k_b, N), float("nan"), device=device)
        bound = torch.zeros(1, device=device)
        dxa, partial = mlp.backward_raw(W, B, xa, xb, dy, saved, b_row0, k_b, S, dxb, xa is not None, mode, dxb_absmax=bound)
        assert float(bound) == 0.0
        for t in (dxb, partial) + ((dxa,) if dxa is not None else ()):
            assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------ nesvor_mlp_prepare
@pytest.mark.parametrize("k_a,k_b,b_row0,rows,out_dim,S,N", [(16, 15, 1, 18, 1, 8, 8 * 1237), (0, 32, 0, 32, 16, 256, 1 << 16), (32, 20, 2, 24, 3, 32, 32 * 999)])
def test_mlp_prepare_against_torch(device, k_a, k_b, b_row0, rows, out_dim, S, N):
    """``nesvor_mlp_prepare``: the XA / XB / DY bounds are exact maxima - a large value planted in a row of xb OUTSIDE
    [b_row0, b_row0 + k_b) must not count - and the four numbers per layer (max |W|, largest row L1 norm, largest column L1 norm,
    max |b|) agree with float64 within rtol 1e-5 (an fp32 sum of <= 64 terms errs by <= 64 x 2^-24 = 4e-6: inside the consumer's
    1.0001 slack); the maxima exactly."""
    from nesvor_amd import mlp

    depth = 2
    W, B = R.make_net(device, depth, k_a + k_b, out_dim, True, 61)
    xa, xb, dy = R.make_inputs(device, k_a, rows, N, S, out_dim, 19)
    outside = [r for r in range(rows) if not b_row0 <= r < b_row0 + k_b]
    for r in outside:
        xb[r, N // 3] = 1e3
    xb[b_row0 + k_b - 1, N - 1] = -7.5  # the extremum of the rows that count: last row, last sample, negative
    dy[out_dim - 1, N - 1] = -9.25
    if xa is not None:
        xa[-1, -1] = -6.5
    d = mlp._desc(W, B, k_a, k_b, b_row0, S, mlp.SPLIT)
    prep = mlp.prepare(d, xa, xb, dy, N, mlp.PREP_INPUT | mlp.PREP_DY | mlp.PREP_WEIGHTS)
    A = mlp.ABSMAX_FLOATS
    assert _slot_max(prep[0:A]) == (float(xa.abs().max()) if xa is not None else 0.0) == (6.5 if xa is not None else 0.0)
    assert _slot_max(prep[A : 2 * A]) == float(xb[b_row0 : b_row0 + k_b].abs().max()) == 7.5
    assert _slot_max(prep[2 * A : 3 * A]) == float(dy.abs().max()) == 9.25
    for l, (w, b) in enumerate(zip(W, B)):
        got = prep[3 * A + 4 * l : 3 * A + 4 * l + 4].double().cpu()
        w64 = w.double().abs()
        ref = torch.tensor([float(w64.max()), float(w64.sum(1).max()), float(w64.sum(0).max()), float(b.double().abs().max())], dtype=torch.float64)
        assert float(got[0]) == float(ref[0]) and float(got[3]) == float(ref[3]), (l, got, ref)
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=0.0)


# ------------------------------------------------------------------------------------------------ hash-grid forward
def _hashgrid_bounded(spec, u, table, layout, hints, unclustered_entry, buf):
    from nesvor_amd import _lib

    lib = _lib.load()
    N, E = u.shape[0], spec.n_output_dims
    pe = torch.full((N, E) if layout == _lib.LAYOUT_ROW_MAJOR else (E, N), float("nan"), device=u.device)
    with torch.cuda.device(u.device):
        if unclustered_entry:
            lay = layout | _lib.LAYOUT_UNCLUSTERED
            nbytes = lib.nesvor_hashgrid_forward_workspace_bytes(ctypes.byref(spec.c_struct), N, lay)
            ws = torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=u.device)
            err = lib.nesvor_hashgrid_forward_unclustered(ctypes.byref(spec.c_struct), _lib.ptr(u), _lib.ptr(table), _lib.ptr(pe), N, lay,
                                                          _lib.ptr(buf), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        else:
            err = lib.nesvor_hashgrid_forward_bounded(ctypes.byref(spec.c_struct), _lib.ptr(u), _lib.ptr(table), _lib.ptr(pe), N,
                                                      layout | hints, _lib.ptr(buf), _lib.stream_ptr())
    _lib.check(err, "hashgrid forward")
    return pe


@pytest.mark.parametrize("N", [1000, 1 << 16])
@pytest.mark.parametrize("entry", ["clustered", "plain", "unclustered-entry"])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("F", [1, 2, 4, 8])
def test_hashgrid_forward_publishes_exact_pe_absmax(device, F, layout, entry, N):
    """``nesvor_hashgrid_forward_bounded`` with and without the clustered hint and ``nesvor_hashgrid_forward_unclustered``, both
    layouts, F = 1, 2, 4, 8, N = 1000 (ragged in the 256-point blocks) and 2^16: the published max |pe| is exact, wherever the
    extreme point sits, also when the extremum is negative."""
    from nesvor_amd import _lib
    from nesvor_amd.grid import HashGridSpec

    spec = HashGridSpec(8, F, 12, 5, 1.6)
    g = torch.Generator().manual_seed(F + 10 * layout + N)
    table = torch.randn(spec.n_params, generator=g).to(device)
    u = torch.rand(N, 3, generator=g).to(device)
    hints = _lib.LAYOUT_CLUSTERED if entry == "clustered" else 0
    for sign in (1.0, -1.0):
        def run(xa_, u_t, dy_):
            buf = torch.zeros(_slotted(), device=device)
            pe = _hashgrid_bounded(spec, u_t.t().contiguous(), table * sign, layout, hints, entry == "unclustered-entry", buf)
            return (pe.t() if layout == 0 else pe), _slot_max(buf)

        _check_everywhere(run, None, u.t().contiguous(), None, 1, N, 256)


# ------------------------------------------------------------------------------------------------ loss kernel
def _loss_backward_bounded(z0, lv, lb, x, v, idx, c, lvs, reg, delta, gw, bufs):
    from nesvor_amd import _lib
    from nesvor_amd import loss as L

    lb_mean = lb.mean().reshape(1) if lb is not None else None
    a = L._fill(z0, lv, lb, x, v, idx, c, lvs, lb_mean, reg, delta)
    out = {"dz0": torch.full_like(z0, float("nan")), "dlog_var": None if lv is None else torch.full_like(lv, float("nan")),
           "dlog_bias": None if lb is None else torch.full_like(lb, float("nan"))}
    a.gw = gw.data_ptr()
    for k, t in out.items():
        setattr(a, k, None if t is None else t.data_ptr())
    a.dz0_absmax, a.dlog_var_absmax, a.dlog_bias_absmax = (b.data_ptr() for b in bufs)
    with torch.cuda.device(z0.device):
        _lib.check(_lib.load().nesvor_imaging_loss(ctypes.byref(a), _lib.stream_ptr()), "imaging loss backward")
    return out


@pytest.mark.parametrize("reg", [0, 1, 2], ids=["edge", "TV", "L2"])
@pytest.mark.parametrize("S", [24, 64, 256])
def test_loss_kernel_publishes_exact_gradient_bounds(device, S, reg):
    """``dz0_absmax`` / ``dlog_var_absmax`` / ``dlog_bias_absmax`` of the loss kernel's backward launch: S = 24 (the general
    two-pass kernel), 64 and 256 (the cached single-pass one), B = 37 (the last workgroup partly empty), every regulariser.  The
    pixel that holds the extreme gradient is swapped into the first and the last place, with and without reversing its samples
    (which keeps the regulariser's s <-> S - 1 - s pairs); both signs of the upstream gradients."""
    B, n = 37, 5
    g = torch.Generator().manual_seed(7 + S + reg)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    z0, lv, lb = (rn(B, S) * 2).to(device), (rn(B, S) * 0.3).to(device), (rn(B, S) * 0.1).to(device)
    x = (rn(B, 1, 3) * 20 + rn(B, S, 3)).to(device)
    v, idx = torch.rand(B, generator=g).to(device), torch.randint(0, n, (B,), generator=g).to(device)
    c, lvs = (torch.rand(n, generator=g) + 0.5).to(device), (rn(n) * 0.2).to(device)
    names = ("dz0", "dlog_var", "dlog_bias")
    for sign in (1.0, -1.0):
        gw = (sign * torch.tensor([1.0, 1.0, 2.0, 100.0])).to(device)

        def run(pix, reverse_pixel=None):
            Z, LV, LB, X = z0[pix].clone(), lv[pix].clone(), lb[pix].clone(), x[pix].clone()
            if reverse_pixel is not None:
                for t in (Z, LV, LB, X):
                    t[reverse_pixel] = t[reverse_pixel].flip(0)
            bufs = [torch.zeros(_slotted(), device=device) for _ in range(3)]
            out = _loss_backward_bounded(Z.reshape(-1), LV.reshape(-1), LB.reshape(-1), X.contiguous(), v[pix].contiguous(),
                                         idx[pix].contiguous(), c, lvs, reg, 0.13, gw, bufs)
            for k, b in zip(names, bufs):
                assert _slot_max(b) == float(out[k].abs().max()) > 0, (k, _slot_max(b), float(out[k].abs().max()))
            return out

        ident = torch.arange(B, device=device)
        out = run(ident)
        for k in names:
            src = int(out[k].abs().argmax())
            p, s = src // S, src % S
            for dst_p in (0, B - 1):
                pix = ident.clone()
                pix[p], pix[dst_p] = dst_p, p
                for rev in (None, dst_p):
                    got = run(pix, rev)
                    want = dst_p * S + (s if rev is None else S - 1 - s)
                    assert int(got[k].abs().argmax()) == want, (k, dst_p, rev, int(got[k].abs().argmax()), want)


def test_loss_and_sigma_backward_share_one_slotted_bound(device):
    """The bound of the density network's upstream gradient dz is raised by TWO producers: the loss kernel (max |dz_0|, slotted)
    and sigma_net's backward (max |dz_1..| = its dxb, a scalar publish into slot 0 - csrc/step.hip).  The maximum over the slots
    must be max(max |dz_0|, max |dz_1..|) whichever of the two is larger and whichever ran first."""
    from nesvor_amd import mlp

    B_, S, n = 64, 256, 5
    N = B_ * S
    g = torch.Generator().manual_seed(3)
    z0 = (torch.randn(B_, S, generator=g) * 2).to(device)
    x = (torch.randn(B_, 1, 3, generator=g) * 20 + torch.randn(B_, S, 3, generator=g)).to(device)
    v, idx = torch.rand(B_, generator=g).to(device), torch.randint(0, n, (B_,), generator=g).to(device)
    gw = torch.tensor([1.0, 1.0, 2.0, 100.0], device=device)
    W, Bs = R.make_net(device, 2, 31, 1, True, 71)
    xa, xb, dy = R.make_inputs(device, 16, 16, N, S, 1, 23)
    for dy_scale in (1e-4, 1e2):  # sigma_net's share far below / far above the loss kernel's
        for loss_first in (True, False):
            buf = torch.zeros(_slotted(), device=device)
            other = [torch.zeros(_slotted(), device=device) for _ in range(2)]

            def loss():
                return _loss_backward_bounded(z0.reshape(-1), None, None, x, v, idx, None, None, 0, 0.13, gw, [buf] + other)["dz0"]

            def sigma():
                _, saved = mlp.forward_raw(W, Bs, xa, xb, 1, 15, S, True, mlp.SPLIT)
                dxb = torch.empty(15, N, device=device)
                mlp.backward_raw(W, Bs, xa, xb, dy * dy_scale, saved, 1, 15, S, dxb, True, mlp.SPLIT, dxb_absmax=buf[:1])
                return dxb

            dz0, dz1 = (loss(), sigma()) if loss_first else tuple(reversed((sigma(), loss())))
            want = max(float(dz0.abs().max()), float(dz1.abs().max()))
            assert _slot_max(buf) == want, (dy_scale, loss_first, _slot_max(buf), want)
            assert (float(dz1.abs().max()) > float(dz0.abs().max())) == (dy_scale > 1)


# ------------------------------------------------------------------------------------------------ wiring
def test_producer_filled_prep_equals_prepare(device):
    """A scaled-mode forward whose ``prep`` input bounds were filled by the PRODUCERS - the hash-grid forward into the density
    network's XB slots, the density forward's ``y_absmax`` into sigma_net's XB slots - equals the same forward on
    ``nesvor_mlp_prepare``'s ``prep``, bit for bit (the slots, and therefore the scales, are the same numbers)."""
    from nesvor_amd import _lib, mlp
    from nesvor_amd.grid import HashGridSpec

    A = mlp.ABSMAX_FLOATS
    S, N = 256, 1 << 16
    spec = HashGridSpec(16, 2, 14, 9, 1.26)
    g = torch.Generator().manual_seed(5)
    table = (torch.randn(spec.n_params, generator=g) * 0.3).to(device)
    u = torch.rand(N, 3, generator=g).to(device)
    Wd, Bd = R.make_net(device, 2, 32, 16, True, 81)
    Wd[-1][0] *= 0.25  # (row 0 of z - the density - is not fed to sigma_net: keep the maximum of z in the rows that are)
    Bd[-1][0] *= 0.25
    Ws, Bs = R.make_net(device, 2, 31, 1, True, 82)
    xa = torch.randn(N // S, 16, generator=g).to(device)
    for mode in (mlp.SPLIT, mlp.FP16S):
        # density network: XB bound from the hash-grid forward
        dd = mlp._desc(Wd, Bd, 0, 32, 0, S, mode)
        prep_ref = mlp.prepare(dd, None, torch.zeros(1, device=device), None, N, mlp.PREP_WEIGHTS)  # weight norms only
        prep_d = prep_ref.clone()
        pe = _hashgrid_bounded(spec, u, table, _lib.LAYOUT_FEATURE_MAJOR, _lib.LAYOUT_CLUSTERED, False, prep_d[A : 2 * A])
        prep_full = mlp.prepare(dd, None, pe, None, N, mlp.PREP_INPUT | mlp.PREP_WEIGHTS)
        assert _slot_max(prep_d[A : 2 * A]) == _slot_max(prep_full[A : 2 * A]) == float(pe.abs().max())
        # ... and the density forward publishes max |z| into sigma_net's XB slots
        ds = mlp._desc(Ws, Bs, 16, 15, 1, S, mode)
        prep_s = mlp.prepare(ds, xa, torch.zeros(16, N, device=device), None, N, mlp.PREP_INPUT | mlp.PREP_WEIGHTS)  # XA bound, weight norms
        prep_s[A : 2 * A].zero_()
        z_a, _ = mlp.forward_raw(Wd, Bd, None, pe, 0, 32, S, False, mode, prep=prep_d, y_absmax=prep_s[A : 2 * A])
        z_b, _ = mlp.forward_raw(Wd, Bd, None, pe, 0, 32, S, False, mode, prep=prep_full)
        assert torch.equal(z_a, z_b)
        assert float(z_a[1:].abs().max()) == float(z_a.abs().max())
        prep_s_full = mlp.prepare(ds, xa, z_a, None, N, mlp.PREP_INPUT | mlp.PREP_WEIGHTS)
        assert _slot_max(prep_s[A : 2 * A]) == _slot_max(prep_s_full[A : 2 * A])
        y_a, _ = mlp.forward_raw(Ws, Bs, xa, z_a, 1, 15, S, False, mode, prep=prep_s)
        y_b, _ = mlp.forward_raw(Ws, Bs, xa, z_a, 1, 15, S, False, mode, prep=prep_s_full)
        assert torch.equal(y_a, y_b)
