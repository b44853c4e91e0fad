"""Shared reference code of the step-kernel tests (a plain module, not a conftest): the small kernels of the one-call training
step - prologue, epilogue, row sums, sampler, AdamW - restated in torch on the CPU, in float64 (the reference) and in float32
(the yardstick an fp32 kernel is measured against), and the two acceptance rules of tests/test_gpu_step_kernels.py.

Every function takes the kernel's own fp32 inputs (CPU tensors) and a dtype; the float64 result is the reference, the float32
result is "the torch composition the kernel replaces".

Acceptance rules:

* pure sums (``sum_bound``): an fp32 sum of T terms, in any order, is off by at most (T + 2) 2^-24 sum|terms| (T - 1 additions
  of relative error 2^-24 each on the running sum, three more roundings for what is done to the total), floor 1e-30;
* transcendental / pose math (``calibrated``): err_kernel <= 4 err_torch_fp32 + 8 2^-24 scale, both errors the largest absolute
  deviation from the float64 reference over the tensor, scale the reference's largest magnitude.
"""
import math

import torch

from oracle import nesvor_model as nm
from oracle import transform_convert as tc

U = 2.0 ** -24  # unit roundoff of fp32


def sum_bound(abs_terms_sum, T):
    """Largest error of an fp32 sum of T terms whose magnitudes add up to ``abs_terms_sum`` (float64 tensor or number)."""
    return (T + 2) * U * abs_terms_sum + 1e-30


def assert_sum(got, ref64, abs_terms_sum, T, what):
    err = (got.double().cpu() - ref64).abs()
    bound = sum_bound(abs_terms_sum, T)
    bad = err > bound
    assert not bool(bad.any()), (what, "T", T, "worst err/bound", float((err / bound).max()), "first bad", int(bad.reshape(-1).nonzero()[0]))


def calibrated(got, ref64, torch32, what, group):
    """Assert the calibrated rule on one tensor; prints err_kernel / err_torch_fp32."""
    if ref64.numel() == 0:
        return
    assert got.shape == ref64.shape == torch32.shape, (what, got.shape, ref64.shape, torch32.shape)
    assert bool(torch.isfinite(ref64).all()), what
    d_k = (got.double().cpu() - ref64).abs().reshape(-1)
    e_k = float(d_k.max())
    e_t = float((torch32.double() - ref64).abs().max())
    scale = float(ref64.abs().max())
    bound = 4.0 * e_t + 8.0 * U * scale
    ratio = e_k / e_t if e_t > 0 else (0.0 if e_k == 0 else float("inf"))
    # (where the kernel's largest error sits, in units in the last place of that element: tells a lucky rounding of torch's
    #  from an error of the kernel's when the ratio is large)
    at = float(ref64.reshape(-1)[int(d_k.argmax())].abs()) if e_k == e_k else float("nan")
    ulps = e_k / 2.0 ** (math.floor(math.log2(at)) - 23) if at > 0 and e_k == e_k else 0.0
    print(f"[{group}] {what}: err_kernel {e_k:.3e} err_torch_fp32 {e_t:.3e} ratio {ratio:.3g} scale {scale:.3e} bound {bound:.3e}"
          f" | worst at |ref| = {at:.3e}: {ulps:.2f} ulp")
    assert e_k == e_k and e_k <= bound, (what, "err_kernel", e_k, "err_torch_fp32", e_t, "ratio", ratio, "bound", bound)


# ---------------------------------------------------------------------------------------------------------------- inputs
def pose_rows(n, gen):
    """Axis-angle rows (n, 6) of mixed magnitude and the row kind: 0 = rotation x 2.5, 1 = rotation x 1e-4 (the first-order
    branch, |a|^2 <= 1e-6), 2 = rotation x 0.5, 3 = an all-zero row (one, in the middle, when n >= 3)."""
    kind = torch.tensor([(0, 1, 2, 0)[i % 4] for i in range(n)])
    ax = torch.randn(n, 6, generator=gen)
    ax[:, :3] *= torch.tensor([2.5, 1e-4, 0.5])[kind][:, None]
    ax[:, 3:] *= 3.0
    if n >= 3:
        kind[n // 2] = 3
        ax[n // 2] = 0.0
    return ax, kind


def overflow_logits(n, offset, gen):
    """randn * 3 + offset with the largest logit moved to index n - 1 (the last wave, the last block-stride trip)."""
    l = torch.randn(n, generator=gen) * 3.0
    j = int(l.argmax())
    l[[j, n - 1]] = l[[n - 1, j]]
    l = (l + offset).float()
    assert int(l.argmax()) == n - 1 or float(l.max()) == float(l[n - 1])
    return l


# -------------------------------------------------------------------------------------------------------------- prologue
def softmax_n(logit, dtype):
    return torch.softmax(logit.to(dtype), 0) * logit.numel()


def ax2mat(ax, dtype):
    return tc.axisangle2mat_forward(ax.to(dtype))


def trans_loss_parts(ax, ax_init, dtype):
    """NeSVoR.trans_loss per slice -> (terms (n), grad (n, 6), loss): the oracle's own functions under autograd; ``loss`` is
    oracle.nesvor_model.trans_loss itself, ``terms`` its per-slice shares (they add up to it)."""
    a = ax.to(dtype).clone().requires_grad_(True)
    a0 = ax_init.to(dtype)
    loss = nm.trans_loss(a, a0)
    (grad,) = torch.autograd.grad(loss, a)
    with torch.no_grad():
        err = nm.mat2axisangle(nm.mat_compose(nm.mat_inv(nm.axisangle2mat(a0)), nm.axisangle2mat(a)))
        n = ax.shape[0]
        terms = (err[:, :3] ** 2).sum(-1) / (3 * n) + 1e-3 * (err[:, 3:] ** 2).sum(-1) / (3 * n)
    return terms, grad, loss.detach()


# -------------------------------------------------------------------------------------------------------------- epilogue
def softmax_backward(c, dc, dtype):
    c, dc = c.to(dtype), dc.to(dtype)
    return c * (dc - (dc * c).sum() / c.numel())


def pose_backward(dmat, ax, dtrans, w_trans, dtype):
    w = torch.tensor(w_trans, dtype=torch.float32).to(dtype)  # (the entry point takes a float)
    return tc.axisangle2mat_backward(dmat.to(dtype), ax.to(dtype)) + w * dtrans.to(dtype)


# --------------------------------------------------------------------------------------------------------------- sampler
def psf_forward(mat, idx, xyz, sigma, noise, bb, dtype):
    """-> x (B, S, 3), u (B, S, 3), q (B, S, 3) = (xyz + noise sigma_k) + t_k (what R_k multiplies)."""
    mat, xyz, sigma, noise, bb = (t.to(dtype) for t in (mat, xyz, sigma, noise, bb))
    m = mat[idx]
    x = nm.transform_points_trans_first(m[:, None], xyz[:, None] + noise * sigma[idx][:, None])
    u = (x - bb[0]) / (bb[1] - bb[0])
    q = (xyz[:, None] + noise * sigma[idx][:, None]) + m[:, None, :, 3]
    return x, u, q


def psf_backward_pix(mat, idx, xyz, sigma, noise, bb, dx, du, dtype):
    """Per-pixel gradient of the slice matrix (B, 3, 4) = sum_s [ g q^T | R^T g ], g = dx + du / (bb1 - bb0); dx or du None:
    that term alone.  Also sum_s of the absolute per-sample contributions to each entry, |g_i q_j| and |(R^T g)_j| (the terms of
    the sum bound)."""
    _, _, q = psf_forward(mat, idx, xyz, sigma, noise, bb, dtype)
    R = mat.to(dtype)[idx][:, :, :3]
    e = (bb[1] - bb[0]).to(dtype)
    g = torch.zeros_like(q)
    if dx is not None:
        g = g + dx.to(dtype)
    if du is not None:
        g = g + du.to(dtype) / e
    dR = torch.einsum("bsi,bsj->bij", g, q)
    dt = torch.einsum("bij,bsi->bj", R, g)
    dR_abs = torch.einsum("bsi,bsj->bij", g.abs(), q.abs())
    dt_abs = torch.einsum("bij,bsi->bsj", R, g).abs().sum(1)
    return torch.cat([dR, dt[:, :, None]], -1), torch.cat([dR_abs, dt_abs[:, :, None]], -1)


# ----------------------------------------------------------------------------------------------------------------- AdamW
def adamw_step(p, g, m, v, t, lr, beta1, beta2, eps, wd, grad_scale):
    """torch.optim.AdamW's single-tensor update (amsgrad off, maximize off) transcribed, in the dtype of the tensors (float64),
    in place; the gradient is g * grad_scale."""
    g = g * grad_scale
    p.mul_(1 - lr * wd)
    m.lerp_(g, 1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1, bc2 = 1 - beta1 ** t, 1 - beta2 ** t
    denom = (v.sqrt() / bc2 ** 0.5).add_(eps)
    p.addcdiv_(m, denom, value=-(lr / bc1))
