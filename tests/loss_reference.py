"""Shared reference code of the loss-kernel tests (a plain module, not a conftest): csrc/loss.hip - the imaging model with its
three losses and every gradient (nesvor_imaging_loss), and the per-pixel -> per-slice gradient sums (nesvor_slice_grads,
nesvor_slice_grads_by_slice) - restated in torch on the CPU, dtype-generic: float64 is the reference, float32 "the torch
composition the kernel replaces".  The acceptance rules are those of tests/step_reference.py.

Conventions, as the header of loss.hip states them: bias and c enter ``var`` detached; var starts from 1 without pixel variance;
logVar is 0 without any variance; the global mean of log_bias is an INPUT (one number, as for the kernel), so the biasReg
gradient is 2 gw3 lb_mean / (B S) per sample.
"""
import torch

from oracle import nesvor_model as nm
from step_reference import U, assert_sum, calibrated, sum_bound  # noqa: F401  (the tests take the rules from here)

OUTPUTS = ("dz0", "dlog_var", "dlog_bias", "dx", "dc_pix", "dlvs_pix")


def reg_pixel_sums(density, x, reg, delta):
    """Per pixel, the sum over its samples of the regulariser term whose batch mean oracle.nesvor_model.IMAGE_REG[reg] takes,
    summed directly as the kernel does (tests/test_loss_reference.py holds each pixel's sum to IMAGE_REG on that pixel alone).
    The gradients of loss_parts go through IMAGE_REG itself."""
    dd = density - torch.flip(density, (1,))
    dx2 = ((x - torch.flip(x, (1,))) ** 2).sum(-1) + 1e-6
    term = {"edge": lambda: (1 + dd ** 2 / dx2 / (delta * delta)).sqrt(), "TV": lambda: torch.abs(dd / dx2.sqrt()), "L2": lambda: dd ** 2 / dx2}[reg]()
    return term.sum(-1)


def loss_parts(z0, lv, lb, x, v, idx, c, lvs, lb_mean, reg, delta, gw, dtype):
    """-> dict: ``loss_pix`` (B, 3) = (e^2 / (2 var), 0.5 log var | 0, sum_s regulariser term) and the gradients of
    gw . (MSE, logVar, imageReg, biasReg): ``dz0``, ``dlog_var``, ``dlog_bias`` (B, S), ``dx`` (B, S, 3), and per PIXEL ``dc_pix``,
    ``dlvs_pix`` (B) - c[idx] and log_var_slice[idx] are leaves of shape (B).  None where the input is absent (lv, lb, c, lvs).
    z0, lv, lb: (B, S); x: (B, S, 3); v, idx: (B); c, lvs: (n); lb_mean: one number (tensor) or None; gw: four numbers."""
    B, S = z0.shape
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    z0, lv, lb, x = leaf(z0), leaf(lv), leaf(lb), leaf(x)
    c_pix = leaf(None if c is None else c[idx])
    lvs_pix = leaf(None if lvs is None else lvs[idx])
    v, gw = v.to(dtype), torch.as_tensor(gw).to(dtype)

    density = torch.nn.functional.softplus(z0)  # (threshold 20, as the reference)
    bias = lb.exp() if lb is not None else 1
    bias_d = bias.detach() if lb is not None else 1
    v_out = (c_pix if c is not None else 1) * (bias * density).mean(-1)
    var = torch.ones(B, dtype=dtype)
    if lv is not None:
        var = ((c_pix.detach() if c is not None else 1) * (bias_d * lv.exp()).mean(-1)) ** 2
    if lvs is not None:
        var = var + lvs_pix.exp()
    has_var = lv is not None or lvs is not None
    mse_pix = (v_out - v) ** 2 / (2 * var)
    logvar_pix = 0.5 * var.log() if has_var else torch.zeros(B, dtype=dtype)
    total = gw[0] * mse_pix.mean() + gw[1] * logvar_pix.mean() + gw[2] * nm.IMAGE_REG[reg](density, x, delta)
    if lb is not None:  # d (mean lb)^2 = 2 lb_mean d mean lb, the mean itself held as the number the kernel is handed
        total = total + gw[3] * 2 * lb_mean.detach().to(dtype).reshape(()) * lb.mean()
    leaves = {"dz0": z0, "dlog_var": lv, "dlog_bias": lb, "dx": x, "dc_pix": c_pix, "dlvs_pix": lvs_pix}
    present = [k for k in OUTPUTS if leaves[k] is not None]
    grads = torch.autograd.grad(total, [leaves[k] for k in present], allow_unused=True)
    out = {k: None for k in OUTPUTS}
    for k, g in zip(present, grads):
        out[k] = g if g is not None else torch.zeros_like(leaves[k])
    with torch.no_grad():
        out["loss_pix"] = torch.stack([mse_pix, logvar_pix, reg_pixel_sums(density, x, reg, delta)], -1)
    return out


def dlvs_pix_means_term(z0, lv, lb, v, idx, c, lvs, gw):
    """dlvs_pix is a function of the pixel's two means over S - m1 = mean_s(bias density) and m2 = mean_s(bias exp(log_var)):
    dlvs_pix = (gw0 (-e^2 / (2 var^2)) + gw1 / (2 var)) / B  exp(lvs),  e = c m1 - v,  var = (c m2)^2 + exp(lvs)
    -> (dlvs_pix (B), term (B)) in float64, term = |d dlvs_pix / d m1| level(m1) + |d dlvs_pix / d m2| level(m2), where level(m) is
    the calibrated rule's own bound for the mean taken as an output, 4 err_torch_fp32(m) + 8 2^-24 max|m| over the case's pixels:
    what an error of the means WITHIN that rule moves dlvs_pix by (first order).  lvs is present; lv, lb, c may be None."""
    B, S = z0.shape

    def means(dtype):
        bias = lb.to(dtype).exp() if lb is not None else torch.ones(B, S, dtype=dtype)
        return ((bias * torch.nn.functional.softplus(z0.to(dtype))).mean(-1),
                (bias * lv.to(dtype).exp()).mean(-1) if lv is not None else None)

    level = lambda m64, m32: 4.0 * float((m32.double() - m64).abs().max()) + 8.0 * U * float(m64.abs().max())
    (m1, m2), (m1_32, m2_32) = means(torch.float64), means(torch.float32)
    m1 = m1.requires_grad_(True)
    m2 = m2.requires_grad_(True) if lv is not None else None
    v, lvs, gw = v.double(), lvs.double(), torch.as_tensor(gw).double()
    c_pix = c.double()[idx] if c is not None else 1
    e = c_pix * m1 - v
    var = ((c_pix * m2) ** 2 if lv is not None else 1) + lvs[idx].exp()
    out = (gw[0] * (-e * e / (2 * var * var)) + gw[1] * 0.5 / var) / B * lvs[idx].exp()
    g = torch.autograd.grad(out.sum(), [m1] + ([m2] if lv is not None else []))
    term = g[0].abs() * level(m1.detach(), m1_32)
    if lv is not None:
        term = term + g[1].abs() * level(m2.detach(), m2_32)
    return out.detach(), term


def calibrated_or_means_term(got, ref64, torch32, what, group, term):
    """The calibrated rule; where a comparison misses it, the rule with ``term`` (dlvs_pix_means_term) added per element - and a
    printed line that says so, with the size of the term in units of 2^-24 |ref|."""
    try:
        calibrated(got, ref64, torch32, what, group)
    except AssertionError:
        d_k = (got.double().cpu() - ref64).abs()
        bound = 4.0 * float((torch32.double() - ref64).abs().max()) + 8.0 * U * float(ref64.abs().max())
        print(f"[{group}] {what}: MISSES the bare rule; with the means' term, up to {float((term / (U * ref64.abs())).max()):.1f} x 2^-24 |ref|, "
              f"err / bound = {float((d_k / (bound + term)).max()):.3f}")
        assert bool((d_k <= bound + term).all()), (what, "err_kernel", float(d_k.max()), "bare bound", bound, "means' term up to", float(term.max()))


def slice_sums(idx, dc_pix, dlvs_pix, dxa, dpix, n, rows, ks, dtype):
    """Per-slice sums of the per-pixel terms -> (sums, abs_sums, counts): ``sums`` = (dc (n), dlvs (n), dse (n, ks), dmat (n, 12)),
    ``abs_sums`` the same of the terms' magnitudes (the sum rule's sum|terms|), ``counts`` (n) the pixels of each slice - an element
    of dc, dlvs, dmat has counts[k] terms, one of dse counts[k] * rows.  dxa: (B, rows, ks).  None where the input is absent."""
    B = idx.shape[0]

    def add(t, width):
        if t is None:
            return None, None
        t = t.to(dtype).reshape(B, width)
        return (torch.zeros(n, width, dtype=dtype).index_add_(0, idx, t), torch.zeros(n, width, dtype=dtype).index_add_(0, idx, t.abs()))

    dc, dc_abs = add(dc_pix, 1)
    dlvs, dlvs_abs = add(dlvs_pix, 1)
    dmat, dmat_abs = add(dpix, 12)
    dse = dse_abs = None
    if dxa is not None and ks > 0:
        d = dxa.to(dtype).reshape(B, rows, ks)
        dse, dse_abs = add(d.sum(1), ks)[0], add(d.abs().sum(1), ks)[0]
    sq = lambda t: None if t is None else t[:, 0]
    return (sq(dc), sq(dlvs), dse, dmat), (sq(dc_abs), sq(dlvs_abs), dse_abs, dmat_abs), torch.bincount(idx, minlength=n)


# ---------------------------------------------------------------------------------------------------------------- inputs
RAMP, TIED, COINCIDENT = 0, 1, 2  # the pixels of edge_inputs that are not generic, where B and S leave room for them


def edge_inputs(B, S, gen, n=3):
    """fp32 inputs of the imaging loss that both precisions read: z0 = 2 randn, log_var = 0.3 randn, log_bias = 0.1 randn,
    log_var_slice = 0.2 randn, c in [0.5, 1.5], v in [0, 1), x = 20 randn per pixel + randn per sample, delta = 0.13, and
    * pixel RAMP (B >= 1): z0 a ramp from -30 to +30 - both branches of softplus' threshold 20, large dd across the mirror;
    * pixel TIED (B >= 2): z0[s] == z0[S-1-s] exactly for the pairs s = 0, 1 (as many as S // 2 allows): dd == 0, TV's sign(0);
    * pixel COINCIDENT (B >= 3, S >= 2): x[0] == x[S-1] with different z0: dx2 == 1e-6 exactly.
    Every other pixel is generic; at odd S the middle sample of every pixel is its own mirror."""
    r = lambda *sh: torch.randn(*sh, generator=gen)
    d = {"z0": r(B, S) * 2, "lv": r(B, S) * 0.3, "lb": r(B, S) * 0.1, "x": r(B, 1, 3) * 20 + r(B, S, 3),
         "v": torch.rand(B, generator=gen), "idx": torch.randint(0, n, (B,), generator=gen),
         "c": torch.rand(n, generator=gen) + 0.5, "lvs": r(n) * 0.2, "delta": 0.13}
    z0, x = d["z0"], d["x"]
    z0[RAMP] = torch.linspace(-30.0, 30.0, S)
    if B > TIED:
        for s in range(min(2, S // 2)):
            z0[TIED, S - 1 - s] = z0[TIED, s]
    if B > COINCIDENT and S >= 2:
        x[COINCIDENT, S - 1] = x[COINCIDENT, 0]
        assert float(z0[COINCIDENT, 0]) != float(z0[COINCIDENT, S - 1])
    d["lb_mean"] = d["lb"].mean().reshape(1)
    return d


def mirror_signs_agree(z0):
    """TV's precondition: for every mirror pair, sign(dd) of the fp32 torch composition equals sign(dd) in fp64 (TV's gradient
    is discontinuous at dd = 0: a pair that straddles it says nothing about a kernel)."""
    dd = lambda t: torch.nn.functional.softplus(t) - torch.flip(torch.nn.functional.softplus(t), (1,))
    return bool(torch.equal(torch.sign(dd(z0.float())).double(), torch.sign(dd(z0.double()))))
