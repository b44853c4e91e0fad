"""tests/loss_reference.py against the formulas the suite already trusts (test_imaging_loss_vs_reference_math in
tests/test_gpu_ops.py: models.py:286-325, 366-384 under autograd, per-SLICE leaves c and log_var_slice): in float64 the per-pixel
parts add up to the four loss values and the gradients are autograd's of those formulas - the same operations regrouped, hence
rtol 1e-12 - so that the new reference cannot drift from the old one.  Also that its edge inputs are what they claim to be."""
import pytest
import torch

import loss_reference as L
from oracle import nesvor_model as nm

FLAGS = [(True, True, False, True), (True, True, True, True), (False, True, False, False), (True, False, True, True),
         (False, False, False, True)]  # pix_var, slice_var, bias, scale: the combinations of the existing test


def _existing_formulas(z0, lv, lb, x, v, idx, c, lvs, reg, delta, w):
    """The body of test_imaging_loss_vs_reference_math; the inputs are float64 leaves (or None)."""
    bias, scale, pix_var, slice_var = lb is not None, c is not None, lv is not None, lvs is not None
    density = torch.nn.functional.softplus(z0)
    bias_t = lb.exp() if bias else 1
    bias_d = bias_t.detach() if bias else 1
    cc = c[idx] if scale else 1
    v_out = cc * (bias_t * density).mean(-1)
    var = lv.exp() if pix_var else 1
    if pix_var:
        var = ((cc.detach() if scale else 1) * (bias_d * var).mean(-1)) ** 2
    if slice_var:
        var = var + lvs.exp()[idx]
    mse = ((v_out - v) ** 2 / (2 * var)).mean()
    logvar = 0.5 * var.log().mean() if (pix_var or slice_var) else torch.zeros((), dtype=torch.float64)
    ireg = nm.IMAGE_REG[reg](density, x, delta)
    breg = lb.mean() ** 2 if bias else torch.zeros((), dtype=torch.float64)
    (w[0] * mse + w[1] * logvar + w[2] * ireg + w[3] * breg).backward()
    return mse, logvar, ireg, breg


@pytest.mark.parametrize("reg", ["edge", "TV", "L2"])
@pytest.mark.parametrize("pix_var,slice_var,bias,scale", FLAGS)
@pytest.mark.parametrize("S", [3, 24, 64])
def test_loss_parts_regroup_the_existing_formulas(reg, pix_var, slice_var, bias, scale, S):
    torch.manual_seed(7)
    B, n = 37, 5
    idx = torch.randint(0, n, (B,))
    f64 = lambda *sh: torch.randn(*sh, dtype=torch.float64)
    z0 = (f64(B, S) * 2).requires_grad_(True)
    lv = (f64(B, S) * 0.3).requires_grad_(True) if pix_var else None
    lb = (f64(B, S) * 0.1).requires_grad_(True) if bias else None
    x = (f64(B, 1, 3) * 20 + f64(B, S, 3)).requires_grad_(True)
    v = torch.rand(B, dtype=torch.float64)
    c = (torch.rand(n, dtype=torch.float64) + 0.5).requires_grad_(True) if scale else None
    lvs = (f64(n) * 0.2).requires_grad_(True) if slice_var else None
    delta, w = 0.13, [1.0, -1.0, 2.0, 100.0]
    mse, logvar, ireg, breg = _existing_formulas(z0, lv, lb, x, v, idx, c, lvs, reg, delta, w)

    det = lambda t: None if t is None else t.detach()
    lb_mean = lb.detach().mean() if bias else None
    p = L.loss_parts(det(z0), det(lv), det(lb), det(x), v, idx, det(c), det(lvs), lb_mean, reg, delta, torch.tensor(w, dtype=torch.float64),
                     torch.float64)
    close = lambda a, b, what: torch.testing.assert_close(a, b, rtol=1e-12, atol=0.0, msg=lambda m: f"{what}: {m}")
    sums = p["loss_pix"].sum(0)
    close(sums[0] / B, mse.detach(), "MSE")
    close(sums[1] / B, logvar.detach(), "logVar")
    close(delta * (sums[2] / (B * S) - 1) if reg == "edge" else sums[2] / (B * S), ireg.detach(), "imageReg")
    if bias:
        close(lb_mean ** 2, breg.detach(), "biasReg")
    dens = torch.nn.functional.softplus(z0.detach())
    for b in range(B):  # each pixel's direct sum against IMAGE_REG on that pixel alone
        one = nm.IMAGE_REG[reg](dens[b:b + 1], x.detach()[b:b + 1], delta)
        close(p["loss_pix"][b, 2], (one / delta + 1) * S if reg == "edge" else one * S, f"regulariser sum of pixel {b}")
    for name, leaf in (("dz0", z0), ("dlog_var", lv), ("dlog_bias", lb), ("dx", x)):
        if leaf is None:
            assert p[name] is None
        else:
            close(p[name], leaf.grad if leaf.grad is not None else torch.zeros_like(leaf), name)
    for name, leaf in (("dc_pix", c), ("dlvs_pix", lvs)):  # per pixel here, per slice there
        if leaf is None:
            assert p[name] is None
        else:
            close(torch.zeros(n, dtype=torch.float64).index_add_(0, idx, p[name]), leaf.grad, name)
    if slice_var:  # the closed form whose sensitivity to the two means over S may widen dlvs_pix's bound (test_gpu_loss_kernels.py)
        closed, term = L.dlvs_pix_means_term(det(z0), det(lv), det(lb), v, idx, det(c), det(lvs), w)
        close(closed, p["dlvs_pix"], "dlvs_pix in closed form")
        assert term.shape == (B,) and bool((term > 0).all())


@pytest.mark.parametrize("S", [1, 2, 3, 4, 65, 1024])
def test_edge_inputs_are_what_they_claim(S):
    d = L.edge_inputs(5, S, torch.Generator().manual_seed(S))
    z0, x = d["z0"], d["x"]
    assert all(t.dtype == torch.float32 for t in (z0, d["lv"], d["lb"], x, d["v"], d["c"], d["lvs"], d["lb_mean"]))
    assert float(z0[L.RAMP, 0]) == -30.0 and (S == 1 or float(z0[L.RAMP, -1]) == 30.0)
    tied = (z0[L.TIED] == torch.flip(z0[L.TIED], (0,))).sum()
    assert int(tied) == 2 * min(2, S // 2) + S % 2
    if S >= 2:
        dx2 = ((x - torch.flip(x, (1,))) ** 2).sum(-1) + 1e-6
        assert float(dx2[L.COINCIDENT, 0]) == float(torch.tensor(1e-6)) and z0[L.COINCIDENT, 0] != z0[L.COINCIDENT, -1]
    assert L.mirror_signs_agree(z0)
    assert not L.mirror_signs_agree(torch.tensor([[1.0, 1.0 + 1e-9]], dtype=torch.float64))  # a pair fp32 cannot tell apart
