"""The small kernels of the one-call training step (csrc/step.hip runs them between the MLP, hash-grid and loss kernels), each
driven through the C ABI at wave and block edges and compared with a float64 restatement on the CPU (tests/step_reference.py):

* nesvor_step_prologue / nesvor_step_prologue_pose   - softmax, pose matrices, zero-fill, pose regulariser
* nesvor_step_epilogue / nesvor_step_epilogue_scaled - softmax backward, pose backward, loss values
* nesvor_sum_rows / nesvor_sum_rows_multi            - column sums of the MLP partial gradients
* nesvor_psf_transform_forward_rng / _forward_rng_gather / _backward_rng / _backward_rng_slices (+ nesvor_psf_noise)
* nesvor_adamw_step

Two acceptance rules, neither taken from what the kernels return (tests/step_reference.py):

* pure sums: |err| <= (T + 2) 2^-24 sum|terms|, per output element;
* transcendental / pose math: err_kernel <= 4 err_torch_fp32 + 8 2^-24 scale, where err_torch_fp32 is the error of the fp32 torch
  composition the kernel replaces, evaluated on the CPU from the same inputs against the same float64 reference.
  Each such comparison prints err_kernel / err_torch_fp32.

"Bit for bit" and "untouched" are torch.equal.
"""
import ctypes

import numpy as np
import pytest
import torch

import step_reference as R

pytestmark = pytest.mark.gpu

N_SLICES = [1, 63, 64, 65, 255, 256, 257, 700]
CANARY = -7.25


def _api():
    from nesvor_amd import _lib

    return _lib, _lib.load(), _lib.stream_ptr()


def _gen(*seed):
    return torch.Generator().manual_seed(int(sum(s * 1000003 ** i for i, s in enumerate(seed))) % (2 ** 31))


def _canary(*shape, device, value=CANARY):
    return torch.full(shape, value, dtype=torch.float32, device=device)


# ================================================================================================================ prologue
def _prologue_inputs(n, offset):
    g = _gen(n, 90 + int(offset))
    logit = R.overflow_logits(n, offset, g)
    ax, kind = R.pose_rows(n, g)
    c64 = R.softmax_n(logit, torch.float64)
    # what the test relies on: the reference is finite and non-zero, although exp(logit) alone is not representable in fp32
    assert bool(torch.isfinite(c64).all()) and float(c64.min()) > 1e-30
    e32 = torch.exp(logit)
    if n > 1 or offset > 0:  # (overflow of the largest, or terms below the smallest normal number)
        assert bool(torch.isinf(e32).any()) or float(e32.min()) < 2.0 ** -126, "the offset does not stress the max subtraction"
    return logit, ax, kind, c64


@pytest.mark.parametrize("n", N_SLICES)
def test_prologue_softmax_matrices_zero_fill(device, n):
    """nesvor_step_prologue: c = n softmax(logit) with logits randn * 3 +- 90 and the largest at index n - 1, mat = axisangle2mat
    over rows of mixed magnitude, zero-fill of exactly n_zero floats; the NULL switches leave their outputs untouched.

    Largest err_kernel / err_torch_fp32 on the MI355X: c 14.6, mat 1.89 (RATIO_LOG at the end of this module explains the 14.6)."""
    _lib, lib, st = _api()
    P = _lib.ptr
    for trial, n_zero in enumerate((0, 1, 255, 256, 257, 13 * 700 + 1 + 300)):
        offset = 90.0 if trial % 2 == 0 else -90.0
        logit, ax, kind, c64 = _prologue_inputs(n, offset)
        d_logit, d_ax = logit.to(device), ax.to(device)
        c, mat, zb = _canary(n, device=device), _canary(n, 3, 4, device=device), torch.ones(n_zero + 1, device=device)
        assert lib.nesvor_step_prologue(P(d_logit), P(c), P(d_ax), P(mat), P(zb), n_zero, n, st) == 0
        R.calibrated(c, c64, R.softmax_n(logit, torch.float32), f"c n={n} offset={offset:+.0f}", "softmax")
        m64, m32 = R.ax2mat(ax, torch.float64), R.ax2mat(ax, torch.float32)
        for k, name in enumerate(("x2.5", "x1e-4", "x0.5", "zero")):
            sel = kind == k
            R.calibrated(mat.cpu()[sel][:, :, :3], m64[sel][:, :, :3], m32[sel][:, :, :3], f"mat[{name}, R] n={n}", "axisangle2mat")
            R.calibrated(mat.cpu()[sel][:, :, 3], m64[sel][:, :, 3], m32[sel][:, :, 3], f"mat[{name}, t] n={n}", "axisangle2mat")
        zb = zb.cpu()
        assert float(zb[:n_zero].abs().max() if n_zero else 0.0) == 0.0 and float(zb[n_zero]) == 1.0, (n, n_zero)

    # NULL switches: no slice scale (logit_coef NULL) leaves c alone, no pose optimisation (axisangle NULL) leaves mat alone
    c, mat, zb = _canary(n, device=device), _canary(n, 3, 4, device=device), torch.ones(9, device=device)
    assert lib.nesvor_step_prologue(None, P(c), P(d_ax), P(mat), P(zb), 8, n, st) == 0
    assert torch.equal(c, _canary(n, device=device))
    R.calibrated(mat[:, :, :3], m64[:, :, :3], m32[:, :, :3], f"mat[R] (no logit_coef) n={n}", "axisangle2mat")
    R.calibrated(mat[:, :, 3], m64[:, :, 3], m32[:, :, 3], f"mat[t] (no logit_coef) n={n}", "axisangle2mat")
    c2, mat2 = _canary(n, device=device), _canary(n, 3, 4, device=device)
    assert lib.nesvor_step_prologue(P(d_logit), P(c2), None, P(mat2), P(zb), 8, n, st) == 0
    assert torch.equal(mat2, _canary(n, 3, 4, device=device))
    R.calibrated(c2, c64, R.softmax_n(logit, torch.float32), f"c (no axisangle) n={n}", "softmax")
    assert float(zb[:8].abs().max()) == 0.0 and float(zb[8]) == 1.0


def _pose_inputs(n):
    """Initial poses and current poses a perturbation away: most by ~0.05 rad / 1 mm, every fourth by ~1e-5 rad (the small-angle
    branch of mat2axisangle), every seventh not at all (zero error, zero gradient)."""
    g = _gen(n, 17)
    ax0 = torch.randn(n, 6, generator=g) * torch.tensor([0.5, 0.5, 0.5, 20.0, 20.0, 20.0])
    d = torch.randn(n, 6, generator=g) * torch.tensor([0.05, 0.05, 0.05, 1.0, 1.0, 1.0])
    i = torch.arange(n)
    d[i % 4 == 1, :3] *= 2e-4
    d[i % 7 == 3] = 0.0
    ax = (ax0 + d).float()
    # no row sits at a branch threshold of the pose conversion (|q_xyz|^2 = 1e-6 <=> error angle 2e-3; |a|^2 = 1e-6), where fp32
    # and fp64 could take different branches
    err = R.tc.mat2axisangle_forward(R.nm.mat_compose(R.nm.mat_inv(R.ax2mat(ax0, torch.float64)), R.ax2mat(ax, torch.float64)))
    ang = err[:, :3].norm(dim=-1)
    assert not bool(((ang > 1e-3) & (ang < 4e-3)).any())
    for a in (ax, ax0):
        th2 = (a[:, :3].double() ** 2).sum(-1)
        assert not bool(((th2 > 0.25e-6) & (th2 < 4e-6)).any())
    return ax, ax0


@pytest.mark.parametrize("n", N_SLICES)
def test_prologue_pose_variant(device, n):
    """nesvor_step_prologue_pose: c, mat and the zero buffer are the plain prologue's, bit for bit; trans_terms and g_trans are
    nesvor_trans_loss's, bit for bit (the same trans_loss_one, built without contraction), and match the oracle's trans_loss under
    autograd in float64; an incomplete set of pose pointers is refused before anything is written.

    Largest err_kernel / err_torch_fp32 on the MI355X: 1.41."""
    _lib, lib, st = _api()
    P = _lib.ptr
    ax, ax0 = _pose_inputs(n)
    logit = R.overflow_logits(n, 90.0, _gen(n, 5))
    d_logit, d_ax, d_ax0 = logit.to(device), ax.to(device), ax0.to(device)
    n_zero = 13 * n + 1 + 300

    def outputs():
        return [_canary(n, device=device), _canary(n, 3, 4, device=device), torch.ones(n_zero + 1, device=device),
                _canary(n, device=device), _canary(n, 6, device=device)]

    plain = outputs()
    assert lib.nesvor_step_prologue(P(d_logit), P(plain[0]), P(d_ax), P(plain[1]), P(plain[2]), n_zero, n, st) == 0
    pose = outputs()
    assert lib.nesvor_step_prologue_pose(P(d_logit), P(pose[0]), P(d_ax), P(pose[1]), P(pose[2]), n_zero, n, P(d_ax0), P(pose[3]),
                                         P(pose[4]), st) == 0
    for a, b in zip(plain[:3], pose[:3]):
        assert torch.equal(a, b)
    assert float(pose[2][:n_zero].abs().max()) == 0.0 and float(pose[2][n_zero]) == 1.0
    assert not bool((pose[0] == CANARY).any()) and not bool((pose[1] == CANARY).any())

    terms, grad = _canary(n, device=device), _canary(n, 6, device=device)
    assert lib.nesvor_trans_loss(P(d_ax), P(d_ax0), P(terms), P(grad), n, st) == 0
    assert torch.equal(pose[3], terms), "trans_terms: the prologue's fourth workgroup != nesvor_trans_loss"
    assert torch.equal(pose[4], grad), "g_trans: the prologue's fourth workgroup != nesvor_trans_loss"

    t64, g64, loss64 = R.trans_loss_parts(ax, ax0, torch.float64)
    t32, g32, _ = R.trans_loss_parts(ax, ax0, torch.float32)
    assert float(loss64) > 0 and abs(float(t64.sum()) - float(loss64)) <= 1e-12 * float(loss64)
    R.calibrated(pose[3], t64, t32, f"trans_terms n={n}", "trans_loss")
    R.calibrated(pose[4][:, :3], g64[:, :3], g32[:, :3], f"g_trans[rotation] n={n}", "trans_loss")
    R.calibrated(pose[4][:, 3:], g64[:, 3:], g32[:, 3:], f"g_trans[translation] n={n}", "trans_loss")

    # refusal: axisangle_init given, one of axisangle / trans_terms / g_trans missing
    for miss in range(3):
        o = outputs()
        a = [P(d_ax), P(o[3]), P(o[4])]
        a[miss] = None
        assert lib.nesvor_step_prologue_pose(P(d_logit), P(o[0]), a[0], P(o[1]), P(o[2]), n_zero, n, P(d_ax0), a[1], a[2], st) != 0
        for got, fresh in zip(o, outputs()):
            assert torch.equal(got, fresh)


# ================================================================================================================ epilogue
EPILOGUE_B = [1, 255, 256, 257, 1000]


def _epilogue_inputs(n, B):
    g = _gen(n, B, 3)
    c = R.softmax_n(torch.randn(n, generator=g) * 3.0, torch.float64).float()
    dc = torch.randn(n, generator=g)
    ax, kind = R.pose_rows(n, g)
    dmat = torch.randn(n, 3, 4, generator=g)
    dtrans = torch.randn(n, 6, generator=g)
    terms = torch.rand(n, generator=g) * 10.0 ** torch.randint(-3, 1, (n,), generator=g).float()
    loss_pix = torch.randn(B, 3, generator=g) * 10.0 ** torch.randint(-2, 2, (B, 3), generator=g).float()
    loss_pix[:, 0].abs_()
    return c, dc, ax, kind, dmat, dtrans, terms, loss_pix


def _check_losses(losses, loss_pix, terms, B, n, img_scale, img_offset, pose=True):
    lp, lp_abs = loss_pix.double().sum(0), loss_pix.double().abs().sum(0)
    inv_B = float(np.float32(1.0) / np.float32(B))  # (the launcher's 1.f / (float)B; its rounding is one of the T + 2)
    s, o = float(np.float32(img_scale)), float(np.float32(img_offset))
    ref = torch.stack([lp[0] / B, lp[1] / B, (lp[0] + lp[1]) / B, terms.double().sum(), lp[2] * s + o])
    mag = torch.stack([lp_abs[0] * inv_B, lp_abs[1] * inv_B, (lp_abs[0] + lp_abs[1]) * inv_B, terms.double().abs().sum(),
                       lp_abs[2] * abs(s) + abs(o)])
    T = torch.tensor([B, B, B, n, B + 1], dtype=torch.float64)
    got = losses.double().cpu()
    if not pose:
        assert float(got[3]) == 0.0
        ref, mag, T, got = ref[[0, 1, 2, 4]], mag[[0, 1, 2, 4]], T[[0, 1, 2, 4]], got[[0, 1, 2, 4]]
    else:
        assert float(ref[3]) != 0.0
    err, bound = (got[: ref.numel()] - ref).abs(), (T + 2) * R.U * mag + 1e-30
    assert bool((err <= bound).all()), ("losses", n, B, (err / bound).tolist())
    assert float(losses[5]) == CANARY


@pytest.mark.parametrize("n", N_SLICES)
def test_epilogue_gradients_and_losses(device, n):
    """nesvor_step_epilogue: dlogit = c (dc - <dc, c> / n) (error against max|dlogit|: the subtraction cancels), daxisangle =
    axisangle2mat_backward(dmat) + w_trans dtrans over rows of mixed magnitude, losses[0..4] as sums of B (or n) terms with
    losses[5] left alone; dc NULL leaves dlogit alone, dmat NULL leaves daxisangle alone and reports transReg 0.

    Largest err_kernel / err_torch_fp32 on the MI355X: dlogit 8.75 (RATIO_LOG at the end of this module), daxisangle 2.19."""
    _lib, lib, st = _api()
    P = _lib.ptr
    w_trans, img_scale, img_offset = 0.1, 0.25, -0.5
    for B in EPILOGUE_B:
        c, dc, ax, kind, dmat, dtrans, terms, loss_pix = _epilogue_inputs(n, B)
        d = [t.to(device) for t in (dc, c, dmat, ax, dtrans, loss_pix, terms)]
        dlogit, dax, losses = _canary(n, device=device), _canary(n, 6, device=device), _canary(6, device=device)
        assert lib.nesvor_step_epilogue(P(d[0]), P(d[1]), P(dlogit), P(d[2]), P(d[3]), P(d[4]), w_trans, P(dax), P(d[5]), P(d[6]),
                                        P(losses), n, B, img_scale, img_offset, st) == 0
        R.calibrated(dlogit, R.softmax_backward(c, dc, torch.float64), R.softmax_backward(c, dc, torch.float32),
                     f"dlogit n={n}", "softmax_backward")
        a64 = R.pose_backward(dmat, ax, dtrans, w_trans, torch.float64)
        a32 = R.pose_backward(dmat, ax, dtrans, w_trans, torch.float32)
        for k, name in enumerate(("x2.5", "x1e-4", "x0.5", "zero")):
            sel = kind == k
            R.calibrated(dax.cpu()[sel][:, :3], a64[sel][:, :3], a32[sel][:, :3], f"daxisangle[{name}, rotation] n={n}", "axisangle2mat_backward")
            R.calibrated(dax.cpu()[sel][:, 3:], a64[sel][:, 3:], a32[sel][:, 3:], f"daxisangle[{name}, translation] n={n}", "axisangle2mat_backward")
        _check_losses(losses, loss_pix, terms, B, n, img_scale, img_offset)

    # NULL switches (the last B)
    dlogit2, dax2, losses2 = _canary(n, device=device), _canary(n, 6, device=device), _canary(6, device=device)
    assert lib.nesvor_step_epilogue(None, P(d[1]), P(dlogit2), P(d[2]), P(d[3]), P(d[4]), w_trans, P(dax2), P(d[5]), P(d[6]),
                                    P(losses2), n, B, img_scale, img_offset, st) == 0
    assert torch.equal(dlogit2, _canary(n, device=device)) and torch.equal(dax2, dax) and torch.equal(losses2, losses)
    dlogit3, dax3, losses3 = _canary(n, device=device), _canary(n, 6, device=device), _canary(6, device=device)
    assert lib.nesvor_step_epilogue(P(d[0]), P(d[1]), P(dlogit3), None, P(d[3]), P(d[4]), w_trans, P(dax3), P(d[5]), P(d[6]),
                                    P(losses3), n, B, img_scale, img_offset, st) == 0
    assert torch.equal(dax3, _canary(n, 6, device=device)) and torch.equal(dlogit3, dlogit)
    assert float(losses3[3]) == 0.0
    _check_losses(losses3, loss_pix, terms, B, n, img_scale, img_offset, pose=False)


@pytest.mark.parametrize("scale", [1.0, 1024.0, 2.0 ** -3])
def test_epilogue_scaled_equals_host_product(device, scale):
    """nesvor_step_epilogue_scaled with a device scale == nesvor_step_epilogue given the host product w_trans * scale: same bits,
    at every slice count of the list."""
    _lib, lib, st = _api()
    P = _lib.ptr
    w_trans, B = 0.1, 257
    host_w = float(np.float32(w_trans) * np.float32(scale))
    d_scale = torch.tensor([scale], dtype=torch.float32, device=device)
    for n in N_SLICES:
        c, dc, ax, kind, dmat, dtrans, terms, loss_pix = _epilogue_inputs(n, B)
        d = [t.to(device) for t in (dc, c, dmat, ax, dtrans, loss_pix, terms)]
        a = [_canary(n, device=device), _canary(n, 6, device=device), _canary(6, device=device)]
        b = [_canary(n, device=device), _canary(n, 6, device=device), _canary(6, device=device)]
        assert lib.nesvor_step_epilogue_scaled(P(d[0]), P(d[1]), P(a[0]), P(d[2]), P(d[3]), P(d[4]), w_trans, P(d_scale), P(a[1]), P(d[5]),
                                               P(d[6]), P(a[2]), n, B, 0.25, -0.5, st) == 0
        assert lib.nesvor_step_epilogue(P(d[0]), P(d[1]), P(b[0]), P(d[2]), P(d[3]), P(d[4]), host_w, P(b[1]), P(d[5]), P(d[6]), P(b[2]),
                                        n, B, 0.25, -0.5, st) == 0
        for x, y in zip(a, b):
            assert torch.equal(x, y), (n, scale)
        assert not bool((a[1] == CANARY).any())
        # (and the scale is applied at all: against float64 with the scaled weight)
        a64 = R.pose_backward(dmat, ax, dtrans, host_w, torch.float64)
        a32 = R.pose_backward(dmat, ax, dtrans, host_w, torch.float32)
        R.calibrated(a[1], a64, a32, f"daxisangle scale={scale} n={n}", "axisangle2mat_backward")


# ================================================================================================================ row sums
SUM_ROWS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 256]
SUM_COLS = [1, 63, 64, 65, 200]


def _sum_matrix(rows, ld, seed):
    g = _gen(rows, ld, seed)
    return torch.randn(rows, ld, generator=g) * 10.0 ** torch.randint(-2, 2, (rows, ld), generator=g).float()


@pytest.mark.parametrize("rows", SUM_ROWS)
def test_sum_rows_at_row_group_edges(device, rows):
    """nesvor_sum_rows around the 16 row groups and their unroll by two, at column counts around the 64-column workgroup, with a
    row pitch equal to and larger than the column count; out[cols] is left alone."""
    _lib, lib, st = _api()
    for cols in SUM_COLS:
        for ld in (cols, cols + 37):
            m = _sum_matrix(rows, ld, 1)
            d_m, out = m.to(device), _canary(cols + 1, device=device)
            assert lib.nesvor_sum_rows(_lib.ptr(d_m), _lib.ptr(out), rows, cols, ld, st) == 0
            assert float(out[cols]) == CANARY, (rows, cols, ld)
            m64 = m[:, :cols].double()
            ref = m64.sum(0)
            assert bool((ref != 0).all())
            R.assert_sum(out[:cols], ref, m64.abs().sum(0), rows, f"sum_rows rows={rows} cols={cols} ld={ld}")


def _ptr_array(tensors_or_ints):
    return (ctypes.c_void_p * len(tensors_or_ints))(*[t if isinstance(t, int) else t.data_ptr() for t in tensors_or_ints])


def _int_array(v):
    return (ctypes.c_int * len(v))(*v)


@pytest.mark.parametrize("rows", [1, 17, 256])
@pytest.mark.parametrize("n_jobs", [1, 2, 3, 4])
def test_sum_rows_multi_equals_single_jobs(device, rows, n_jobs):
    """nesvor_sum_rows_multi: every job's output == nesvor_sum_rows of that job, bit for bit, and the float64 column sums; the
    second job sums a column range of a wider matrix."""
    _lib, lib, st = _api()
    cols = [65, 1, 64, 200][:n_jobs]
    ld = [65, 90, 64, 237][:n_jobs]
    first_col = [0, 41, 0, 0][:n_jobs]
    mats = [_sum_matrix(rows, ld[k], 10 + k) for k in range(n_jobs)]
    d_mats = [m.to(device) for m in mats]
    outs = [_canary(cols[k] + 1, device=device) for k in range(n_jobs)]
    in_ptrs = [d_mats[k].data_ptr() + 4 * first_col[k] for k in range(n_jobs)]
    assert lib.nesvor_sum_rows_multi(_ptr_array(in_ptrs), _ptr_array(outs), _int_array(cols), _int_array(ld), n_jobs, rows, st) == 0
    for k in range(n_jobs):
        single = _canary(cols[k] + 1, device=device)
        assert lib.nesvor_sum_rows(ctypes.c_void_p(in_ptrs[k]), _lib.ptr(single), rows, cols[k], ld[k], st) == 0
        assert torch.equal(outs[k], single), (rows, n_jobs, k)
        assert float(outs[k][cols[k]]) == CANARY
        m64 = mats[k][:, first_col[k]:first_col[k] + cols[k]].double()
        R.assert_sum(outs[k][:cols[k]], m64.sum(0), m64.abs().sum(0), rows, f"sum_rows_multi rows={rows} job {k} of {n_jobs}")


def test_sum_rows_multi_refusals(device):
    """Five jobs, a job without columns and a row pitch below the column count are refused before anything is written; no job is
    a no-op that succeeds."""
    _lib, lib, st = _api()
    rows = 17
    mats = [_sum_matrix(rows, 80, 20 + k).to(device) for k in range(5)]

    def outputs():
        return [_canary(81, device=device) for _ in range(5)]

    for cols, ld, n_jobs, want_zero in (([8] * 5, [80] * 5, 5, False), ([8, 0, 8], [80] * 3, 3, False), ([8, 80], [80, 79], 2, False),
                                        ([8, 8], [80, 80], 0, True)):
        outs = outputs()
        k = max(n_jobs, len(cols))
        err = lib.nesvor_sum_rows_multi(_ptr_array(mats[:k]), _ptr_array(outs[:k]), _int_array(cols), _int_array(ld), n_jobs, rows, st)
        assert (err == 0) == want_zero, (cols, ld, n_jobs, err)
        for o, fresh in zip(outs, outputs()):
            assert torch.equal(o, fresh), (cols, ld, n_jobs)


# ================================================================================================================= sampler
SAMPLER_RNG = (20240607, 11)


def _psf_noise(lib, _lib, B, S, device):
    out = torch.empty(B * S, 3, dtype=torch.float32, device=device)
    assert lib.nesvor_psf_noise(SAMPLER_RNG[0], SAMPLER_RNG[1], _lib.ptr(out), B * S, _lib.stream_ptr()) == 0
    return out.view(B, S, 3)


def _sampler_inputs(B, S, mode):
    """Small poses and sigmas; n slices of which one (``empty``, in the middle) owns no pixel and every other owns at least one
    ("spread"), or of which one owns every pixel ("one")."""
    g = _gen(B, S, 7)
    n = min(B + 1, 7)
    empty = n // 2
    mat = R.ax2mat(torch.randn(n, 6, generator=g) * torch.tensor([0.3, 0.3, 0.3, 5.0, 5.0, 5.0]), torch.float32)
    if mode == "one":
        owner = (empty + 1) % n
        idx = torch.full((B,), owner, dtype=torch.int64)
    else:
        owners = torch.tensor([k for k in range(n) if k != empty])
        idx = owners[torch.randint(0, len(owners), (B,), generator=g)]
        idx[: len(owners)] = owners[torch.randperm(len(owners), generator=g)][: B]
        assert sorted(set(idx.tolist())) == owners.tolist()
    assert not bool((idx == empty).any())
    xyz = torch.randn(B, 3, generator=g) * 20
    sigma = torch.rand(n, 3, generator=g) + 0.5
    bb = torch.tensor([[-60.0, -65, -70], [62, 66, 75]])
    dx, du = torch.randn(B, S, 3, generator=g), torch.randn(B, S, 3, generator=g) * 50
    return n, empty, mat, idx, xyz, sigma, bb, dx, du


SAMPLER_CASES = [(1, 1, "spread"), (3, 63, "spread"), (4, 64, "spread"), (5, 65, "spread"), (203, 130, "spread"), (4, 64, "one"),
                 (203, 130, "one")]


@pytest.mark.parametrize("B,S,mode", SAMPLER_CASES)
def test_sampler_rng_forward_backward(device, B, S, mode):
    """nesvor_psf_transform_forward_rng / _backward_rng at sample counts around one wave: x, u and the per-pixel pose gradient
    against float64 on the draws nesvor_psf_noise materialises; x NULL, and dx NULL / du NULL / both in the backward (each the
    float64 result of that term alone).

    Largest err_kernel / err_torch_fp32 on the MI355X: forward 1.00, backward 1.03."""
    _lib, lib, st = _api()
    P = _lib.ptr
    n, empty, mat, idx, xyz, sigma, bb, dx, du = _sampler_inputs(B, S, mode)
    d_mat, d_idx, d_xyz, d_sigma, d_bb, d_dx, d_du = (t.to(device) for t in (mat, idx, xyz, sigma, bb, dx, du))
    noise = _psf_noise(lib, _lib, B, S, device).cpu()
    assert bool(torch.isfinite(noise).all())
    x, u = _canary(B, S, 3, device=device), _canary(B, S, 3, device=device)
    assert lib.nesvor_psf_transform_forward_rng(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), P(x), P(u), B, S, st) == 0
    x64, u64, _ = R.psf_forward(mat, idx, xyz, sigma, noise, bb, torch.float64)
    x32, u32, _ = R.psf_forward(mat, idx, xyz, sigma, noise, bb, torch.float32)
    R.calibrated(x, x64, x32, f"x B={B} S={S} {mode}", "sampler forward")
    R.calibrated(u, u64, u32, f"u B={B} S={S} {mode}", "sampler forward")
    u_only = _canary(B, S, 3, device=device)
    assert lib.nesvor_psf_transform_forward_rng(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), None, P(u_only), B, S, st) == 0
    assert torch.equal(u_only, u)

    for name, a, b in (("dx+du", dx, du), ("dx", dx, None), ("du", None, du)):
        dpix = _canary(B, 3, 4, device=device)
        assert lib.nesvor_psf_transform_backward_rng(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb),
                                                     P(d_dx) if a is not None else None, P(d_du) if b is not None else None, P(dpix), B, S, st) == 0
        g64, _ = R.psf_backward_pix(mat, idx, xyz, sigma, noise, bb, a, b, torch.float64)
        g32, _ = R.psf_backward_pix(mat, idx, xyz, sigma, noise, bb, a, b, torch.float32)
        R.calibrated(dpix[:, :, :3], g64[:, :, :3], g32[:, :, :3], f"dpix[R] {name} B={B} S={S} {mode}", "sampler backward")
        R.calibrated(dpix[:, :, 3], g64[:, :, 3], g32[:, :, 3], f"dpix[t] {name} B={B} S={S} {mode}", "sampler backward")


@pytest.mark.parametrize("B,S,mode", SAMPLER_CASES)
def test_sampler_backward_slices_adds_per_slice(device, B, S, mode):
    """nesvor_psf_transform_backward_rng_slices: dmat_slice afterwards == what it held + the float64 index_add of the per-pixel
    gradients (a sum over the slice's pixels x S samples, T = pixels + S deep; its terms are |g_i q_j| and |(R^T g)_j| per sample
    and what dmat_slice held), with dpix given and with dpix NULL; dpix == nesvor_psf_transform_backward_rng's, bit for bit; the
    row of the slice without a pixel keeps its bits."""
    _lib, lib, st = _api()
    P = _lib.ptr
    n, empty, mat, idx, xyz, sigma, bb, dx, du = _sampler_inputs(B, S, mode)
    d_mat, d_idx, d_xyz, d_sigma, d_bb, d_dx, d_du = (t.to(device) for t in (mat, idx, xyz, sigma, bb, dx, du))
    noise = _psf_noise(lib, _lib, B, S, device).cpu()
    g64, terms_abs = R.psf_backward_pix(mat, idx, xyz, sigma, noise, bb, dx, du, torch.float64)
    prefill = torch.randn(n, 3, 4, generator=_gen(B, S, 9)) * 10 + 3.0
    ref = prefill.double().index_add(0, idx, g64)
    mag = prefill.double().abs().index_add(0, idx, terms_abs)
    count = torch.bincount(idx, minlength=n)
    assert int(count[empty]) == 0 and (mode == "one" or bool((count[torch.arange(n) != empty] > 0).all()))
    T = (count + S).double()[:, None, None].expand(n, 3, 4)
    assert bool((ref != 0).all())

    plain = _canary(B, 3, 4, device=device)
    assert lib.nesvor_psf_transform_backward_rng(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), P(d_dx), P(d_du), P(plain),
                                                 B, S, st) == 0
    for with_dpix in (True, False):
        acc = prefill.to(device)
        dpix = _canary(B, 3, 4, device=device)
        assert lib.nesvor_psf_transform_backward_rng_slices(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), P(d_dx), P(d_du),
                                                            P(dpix) if with_dpix else None, P(acc), B, S, st) == 0
        assert torch.equal(dpix, plain if with_dpix else _canary(B, 3, 4, device=device))
        acc = acc.cpu()
        assert torch.equal(acc[empty], prefill[empty])
        err, bound = (acc.double() - ref).abs(), (T + 2) * R.U * mag + 1e-30
        assert bool((err <= bound).all()), (B, S, mode, with_dpix, float((err / bound).max()))
        assert not torch.equal(acc[idx[0]], prefill[idx[0]])


@pytest.mark.parametrize("ks", [0, 1, 16, 64, 65, 100])
def test_sampler_forward_gather(device, ks):
    """nesvor_psf_transform_forward_rng_gather: x and u are nesvor_psf_transform_forward_rng's, bit for bit; se[b] ==
    embedding[slice_idx[b]] exactly over ks columns around one wave, the row after the last pixel left alone; ks = 0 leaves se
    alone; ks > 0 without an embedding or without se is refused."""
    _lib, lib, st = _api()
    P = _lib.ptr
    for B, S in ((3, 63), (203, 130)):
        n, empty, mat, idx, xyz, sigma, bb, _, _ = _sampler_inputs(B, S, "spread")
        d_mat, d_idx, d_xyz, d_sigma, d_bb = (t.to(device) for t in (mat, idx, xyz, sigma, bb))
        x0, u0 = _canary(B, S, 3, device=device), _canary(B, S, 3, device=device)
        assert lib.nesvor_psf_transform_forward_rng(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), P(x0), P(u0), B, S, st) == 0
        kw = max(ks, 1)
        emb = torch.randn(n, kw, generator=_gen(B, ks, 1))
        d_emb = emb.to(device)
        x, u, se = _canary(B, S, 3, device=device), _canary(B, S, 3, device=device), _canary(B + 1, kw, device=device)
        assert lib.nesvor_psf_transform_forward_rng_gather(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), P(x), P(u), B, S,
                                                           P(d_emb), P(se), ks, st) == 0
        assert torch.equal(x, x0) and torch.equal(u, u0)
        assert not bool((x == CANARY).any()) and not bool((u == CANARY).any())
        if ks == 0:
            assert torch.equal(se, _canary(B + 1, kw, device=device))
            x2, u2 = _canary(B, S, 3, device=device), _canary(B, S, 3, device=device)  # (and NULL is fine there)
            assert lib.nesvor_psf_transform_forward_rng_gather(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), P(x2), P(u2), B, S,
                                                               None, None, 0, st) == 0
            assert torch.equal(x2, x0) and torch.equal(u2, u0)
        else:
            assert torch.equal(se[:B].cpu(), emb[idx])
            assert torch.equal(se[B], _canary(kw, device=device))
            for e_ptr, s_ptr in ((None, P(se)), (P(d_emb), None)):
                x3, se3 = _canary(B, S, 3, device=device), se.clone()
                assert lib.nesvor_psf_transform_forward_rng_gather(P(d_mat), P(d_idx), P(d_xyz), P(d_sigma), *SAMPLER_RNG, P(d_bb), P(x3), None, B, S,
                                                                   e_ptr, s_ptr if s_ptr is None else P(se3), ks, st) != 0
                assert torch.equal(x3, _canary(B, S, 3, device=device)) and torch.equal(se3, se)


# =================================================================================================================== AdamW
# 262147 / 262148: 256 / 257 workgroups, the two sides of the launch's priority switch (blocks <= 256); 3 * 2^20 + 3: more than
# 2048 * 256 float4, so the grid-stride loop takes a second trip, and a three-element tail
ADAMW_N = [1, 2, 3, 4, 5, 1023, 262147, 262148, 262149, 3 * 2 ** 20 + 3]


@pytest.mark.parametrize("grad_scale", [1.0, 1.0 / 1024])
@pytest.mark.parametrize("n", ADAMW_N)
def test_adamw_moments_tail_and_guards(device, n, grad_scale):
    """nesvor_adamw_step, three steps: p, exp_avg and exp_avg_sq against a float64 transcription of torch.optim.AdamW fed
    g * grad_scale (and, at grad_scale 1, p against torch.optim.AdamW itself); zero_grad 1 clears the gradient, zero_grad 0 leaves
    its bits and gives the same p and moments; the element past n of each buffer is left alone.

    The entry point takes lr, the betas, eps and the weight decay as floats, so the optimiser under test IS the one with those
    fp32 values: the references are given the same (rounded) hyper-parameters - 1 - beta is then exact on both sides.

    Largest err_kernel / err_torch_fp32 on the MI355X: 7.08 (exp_avg_sq at n = 3; RATIO_LOG at the end of this module)."""
    _lib, lib, st = _api()
    P = _lib.ptr
    f32 = lambda v: float(np.float32(v))
    lr, b1, b2, eps, wd = f32(5e-3), f32(0.9), f32(0.99), f32(1e-15), f32(1e-2)
    g = _gen(n, 31)
    p0 = torch.randn(n, generator=g)
    guard = torch.tensor([CANARY])
    p_t = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p_t], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    p64, m64, v64 = p0.double(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    bufs = [torch.cat([t, guard]).to(device) for t in (p0, torch.zeros(n), torch.zeros(n), torch.zeros(n))]  # p, g, m, v
    for t in (1, 2, 3):
        grad = torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, 2, (n,), generator=g).float()
        grad[3::7] = 0.0  # entries no step touches: the weight decay still applies (not element 0: n = 1 has a gradient)
        if t == 2:
            grad[1::3] = 0.0
        bufs[1][:n] = grad.to(device)
        p_t.grad = grad * torch.tensor(grad_scale)
        opt.step()
        R.adamw_step(p64, grad.double(), m64, v64, t, lr, b1, b2, eps, wd, grad_scale)

        keep = [b.clone() for b in bufs]  # zero_grad = 0 on a copy of the same state
        args = (n, lr, b1, b2, eps, wd, 1 - b1 ** t, 1 - b2 ** t, grad_scale)
        assert lib.nesvor_adamw_step(P(keep[0]), P(keep[1]), P(keep[2]), P(keep[3]), *args, 0, st) == 0
        g_before = bufs[1].clone()
        assert lib.nesvor_adamw_step(P(bufs[0]), P(bufs[1]), P(bufs[2]), P(bufs[3]), *args, 1, st) == 0
        assert float(bufs[1][:n].abs().max()) == 0.0
        assert torch.equal(keep[1], g_before)
        for k in (0, 2, 3):
            assert torch.equal(keep[k], bufs[k]), (n, t, k)
        for b in bufs + keep:
            assert float(b[n]) == CANARY, (n, t)

        st_t = opt.state[p_t]
        tag = f"n={n} grad_scale={grad_scale:g} t={t}"
        R.calibrated(bufs[0][:n], p64, p_t.data, f"p {tag}", "adamw")
        R.calibrated(bufs[2][:n], m64, st_t["exp_avg"], f"exp_avg {tag}", "adamw")
        R.calibrated(bufs[3][:n], v64, st_t["exp_avg_sq"], f"exp_avg_sq {tag}", "adamw")
        if grad_scale == 1.0:
            # torch.optim.AdamW itself: two fp32 evaluations, each within its error of the float64 one, differ by at most the sum of
            # the two errors - with the rule above, 5 err_torch_fp32 + 8 2^-24 scale
            e_t = float((p_t.data.double() - p64).abs().max())
            direct = float((bufs[0][:n].cpu() - p_t.data).abs().max())
            assert direct <= 5.0 * e_t + 8.0 * R.U * float(p64.abs().max()), (tag, direct, e_t)
    assert not torch.equal(bufs[0][:n].cpu(), p0)


# RATIO_LOG - the largest err_kernel / err_torch_fp32 per group on the MI355X, with the kernel's error there in units of 2^-24 scale
# (the rule: err_kernel <= 4 err_torch_fp32 + 8 2^-24 scale):
#   softmax (prologue c)              14.6   n = 257, +90: 1.65 x 2^-24 scale - 1.07 ulp of the largest c, which torch rounds to 0.07 ulp
#   axisangle2mat (prologue mat)       1.89
#   trans_loss (terms, g_trans)        1.41
#   softmax backward (dlogit)          8.75  n = 64, B = 257: 4.2 x 2^-24 scale
#   axisangle2mat backward             2.19
#   sampler forward (x, u)             1.00
#   sampler backward (per pixel)       1.03
#   AdamW (p, exp_avg, exp_avg_sq)     7.08  n = 3, step 2, exp_avg_sq: 1.55 x 2^-24 scale (2.0 at most from n = 1023 up)
# Two of the groups above 4 (softmax: n = 63 / -90, 255 / +90, 257 / +90; its backward: n = 64 and 65) are sums over the slices taken
# in another order than torch's, in cases where torch's own error happens to be a fraction of a unit in the last place: an fp32
# evaluation on the CPU, operation by operation in the kernels' order (block-stride partial sums, xor butterfly over the wave, the
# four wave totals in turn), gives the very same errors - 1.638e-5, 1.955e-5, 1.721e-6 for c, 6.461e-6 and 1.878e-6 for dlogit.
# The third, exp_avg_sq of a three-element tensor, is 1.55 x 2^-24 of the largest v after the three roundings of
# fma(1 - beta2, g g, beta2 v) (each up to half a unit in the last place), where torch's result lands within 0.22 x 2^-24.
# All of them are inside the rule through its floor, the largest at 0.42 of the bound.
