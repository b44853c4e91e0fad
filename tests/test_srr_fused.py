"""Classical reconstruction (the ``svr`` command): the fused descent step (csrc/srr.hip) against ``edge_prior_gradient`` in
fp64, the step bound and ``srr_descent`` on both of its paths, the ``reconstruct_volume`` pipeline and its command line."""
import os
from argparse import Namespace

import pytest
import torch

ALPHA = 0.5  # the reference's fixed step: exact in fp32


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_parser_has_svr_and_keeps_the_other_defaults():
    from nesvor_amd.cli import build_parser

    p = build_parser()
    a = p.parse_args(["svr", "--input-stacks", "a.nii.gz", "b.nii.gz", "--output-volume", "v.nii.gz"])
    assert a.registration == "svr" and a.output_resolution == 0.8 and a.output_intensity_mean == 700.0
    assert a.n_iter_srr == 30 and a.srr_beta == 0.02 and a.srr_delta == 0.1
    assert a.input_slices is None and a.output_slices is None and a.simulated_slices is None and a.verbose == 1
    b = p.parse_args(["svr", "--input-slices", "dir", "--output-volume", "v.nii.gz", "--registration", "none", "--n-iter-srr", "5"])
    assert b.input_slices == "dir" and b.registration == "none" and b.n_iter_srr == 5
    with pytest.raises(SystemExit):
        p.parse_args(["svr", "--input-stacks", "a.nii.gz"])  # no --output-volume
    assert p.parse_args(["reconstruct", "--input-stacks", "a.nii.gz", "--output-volume", "v.nii.gz"]).registration == "none"
    assert p.parse_args(["register", "--input-stacks", "a.nii.gz", "--output-slices", "out"]).registration == "stack"


def test_input_slices_of_mixed_pixel_sizes_are_refused(tmp_path):
    from nesvor_amd.image import Slice
    from nesvor_amd.image_io import save_slices
    from nesvor_amd.svr import MIXED_SLICES_MESSAGE, svr_command
    from nesvor_amd.transform import RigidTransform

    g = torch.Generator().manual_seed(0)
    pose = lambda: RigidTransform(torch.eye(3, 4)[None].clone())  # (as a matrix: the axis-angle conversion is a HIP kernel)
    for name, sizes in (("pixel", [(1.5, 1.5, 3.0), (1.0, 1.0, 3.0)]), ("thickness", [(1.5, 1.5, 3.0), (1.5, 1.5, 4.0)])):
        folder = str(tmp_path / name)
        os.makedirs(folder)
        save_slices(folder, [Slice(torch.rand(1, 6, 7, generator=g) + 0.5, None, pose(), *s) for s in sizes])
        args = Namespace(input_slices=folder, input_stacks=None, stack_masks=None, thicknesses=None, device=torch.device("cpu"),
                         output_resolution=0.8, n_iter_srr=1, srr_beta=0.02, srr_delta=0.1, simulated_slices=None)
        with pytest.raises(SystemExit) as e:
            svr_command(args)
        assert str(e.value) == MIXED_SLICES_MESSAGE and "one pixel size and one thickness" in MIXED_SLICES_MESSAGE


class _DenseOp:
    """A small dense acquisition operator given as two closures: A (m x n) on the flattened volume."""

    def __init__(self, A, volume_shape, slices_shape):
        self.forward = lambda x: (A @ x.reshape(-1)).reshape(slices_shape)
        self.adjoint = lambda y: (A.t() @ y.reshape(-1)).reshape(volume_shape)


def test_step_bound_dominates_the_spectrum_and_descent_never_increases_the_misfit(monkeypatch):
    from nesvor_amd.srr import PRIOR_SLOPE_BOUND, descent_step_bound, srr_descent

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    g = torch.Generator().manual_seed(7)
    A = torch.rand(20, 12, generator=g, dtype=torch.float64)
    p = torch.rand(1, 1, 4, 5, generator=g, dtype=torch.float64)
    op = _DenseOp(A, (1, 1, 2, 2, 3), (1, 1, 4, 5))
    x0 = torch.rand(1, 1, 2, 2, 3, generator=g, dtype=torch.float64)
    lam = float(torch.linalg.eigvalsh(A.t() @ torch.diag(p.reshape(-1)) @ A).max())
    assert PRIOR_SLOPE_BOUND == pytest.approx(2 * (6 + 6 + 8 / 3))
    for beta in (0.0, 0.02):
        L = descent_step_bound(op, p, beta, like=x0)
        assert L.ndim == 0 and L.dtype == torch.float64
        assert float(L) >= lam + PRIOR_SLOPE_BOUND * beta
        assert float(L) == pytest.approx(float((A.t() @ (p.reshape(-1) * (A @ torch.ones(12, dtype=torch.float64)))).max())
                                         + PRIOR_SLOPE_BOUND * beta)
    assert float(descent_step_bound(op, None, 0.0, like=x0)) >= float(torch.linalg.eigvalsh(A.t() @ A).max())

    # ten steps (eleven iterates pass through A before the final clamp) at alpha = 1 / L, far from the start
    y = op.forward(torch.rand(1, 1, 2, 2, 3, generator=g, dtype=torch.float64)) + 0.1 * torch.rand(1, 1, 4, 5, generator=g, dtype=torch.float64)
    seen = []

    def forward(x):
        out = A @ x.reshape(-1)
        seen.append(float((p.reshape(-1) * (out - y.reshape(-1)) ** 2).sum()))
        return out.reshape(1, 1, 4, 5)

    op.forward = forward
    srr_descent(op, y, 5.0 * x0, 11, 0.0, 0.1, p=p)
    assert len(seen) == 12  # (one more: the volume of ones of the bound)
    misfit = seen[1:]
    assert all(b <= a for a, b in zip(misfit[:-1], misfit[1:])), misfit
    assert misfit[-1] < 0.5 * misfit[0]


def test_composed_descent_is_the_reference_loop():
    """fp64 host tensors take the torch expression: the same numbers as the reference's loop written out (srr.py:117-131)."""
    from nesvor_amd.srr import edge_prior_gradient, srr_descent

    g = torch.Generator().manual_seed(11)
    shape = (1, 1, 4, 5, 6)
    A = torch.rand(30, 120, generator=g, dtype=torch.float64) / 30
    op = _DenseOp(A, shape, (3, 1, 2, 5))
    p = torch.rand(3, 1, 2, 5, generator=g, dtype=torch.float64)
    y = torch.rand(3, 1, 2, 5, generator=g, dtype=torch.float64)
    volume = torch.rand(shape, generator=g, dtype=torch.float64) - 0.2
    start = volume.clone()
    n_iter, alpha, beta, delta = 4, 0.3, 0.02, 0.1
    x = volume.clone()
    for _ in range(n_iter):  # the reference, literally
        err = op.forward(x) - y
        err = err * p
        grad = op.adjoint(err)
        grad.add_(edge_prior_gradient(x, delta), alpha=beta * delta * delta)
        x.add_(grad, alpha=-alpha)
    x.clamp_(min=0.0)
    out = srr_descent(op, y, volume, n_iter, beta, delta, p=p, alpha=alpha)
    assert torch.equal(volume, start)  # the input is left alone
    torch.testing.assert_close(out, x, rtol=0, atol=1e-15)
    assert float(out.min()) == 0.0 and float((out - start).abs().max()) > 1e-3
    every = srr_descent(op, y, volume, n_iter, beta, delta, p=p, alpha=alpha, clamp_every=True)
    assert float(every.min()) == 0.0 and not torch.equal(every, out)
    assert torch.equal(srr_descent(op, y, volume, 0, beta, delta, alpha=alpha), volume.clamp(min=0))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against edge_prior_gradient
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [(3, 3, 3), (2, 7, 65), (7, 2, 9), (5, 9, 33), (4, 8, 64), (17, 8, 65), (11, 19, 70),
          (1, 1, 1), (1, 9, 33), (9, 1, 33), (9, 33, 1), (2, 2, 2),  # no interior along one axis, or along any
          (16, 3, 34), (32, 9, 33), (33, 3, 3)]  # z-march seams: 16 planes per workgroup, a last workgroup of one plane, halos across
_INPUTS = {}


def _inputs(shape, device):
    """Seeded x in [0, 1) and a normal gradient, shared by every test of the shape and never written."""
    if shape not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + shape[0] * 10007 + shape[1] * 101 + shape[2])
        _INPUTS[shape] = (torch.rand(shape, generator=g).to(device), torch.randn(shape, generator=g).to(device))
    return _INPUTS[shape]


def _border(shape, device):
    m = torch.ones(shape, dtype=torch.bool, device=device)
    if min(shape) >= 3:
        m[1:-1, 1:-1, 1:-1] = False
    return m


def _ulp(value: torch.Tensor) -> float:
    v = value.float()
    return float(torch.nextafter(v, torch.full_like(v, float("inf"))) - v)


@pytest.mark.gpu
@pytest.mark.parametrize("beta_rel", [0.0, 0.02])
@pytest.mark.parametrize("delta", [0.1, 1.0])
@pytest.mark.parametrize("shape", SHAPES)
def test_step_against_the_prior_gradient_in_fp64(device, shape, delta, beta_rel):
    """The kernel's largest error against fp64 is at most twice that of the fp32 torch expression plus one ulp of the largest
    |out| (the factor two: another order of the 26 terms).  Border voxels equal x - alpha g bit for bit.  Measured on MI355X
    (largest over the cases): DESIGN.md, "Classical reconstruction"."""
    from nesvor_amd.srr import edge_prior_gradient

    x, grad = _inputs(shape, device)
    beta = beta_rel * delta * delta
    expect = x.double() - ALPHA * (grad.double() + beta * edge_prior_gradient(x.double(), delta))
    composed = x - ALPHA * (grad + beta * edge_prior_gradient(x, delta))
    out = torch.ops.nesvor.srr_step(x, grad, ALPHA, beta, delta, False)
    assert out.shape == x.shape and out.dtype == torch.float32 and out.data_ptr() not in (x.data_ptr(), grad.data_ptr())
    err_kernel = float((out.double() - expect).abs().max())
    err_composed = float((composed.double() - expect).abs().max())
    ulp = _ulp(expect.abs().max())
    print(f"shape {shape} delta {delta} beta {beta:g}: kernel {err_kernel:.3e} composed {err_composed:.3e} ulp {ulp:.3e}")
    assert err_kernel <= 2 * err_composed + ulp
    border = _border(shape, device)
    plain = x - ALPHA * grad
    assert torch.equal(out[border], plain[border])
    if min(shape) < 3:
        assert bool(border.all())
    elif beta:
        assert not torch.equal(out[~border], plain[~border])  # the prior did act on the interior


@pytest.mark.gpu
def test_clamp_zeroes_negatives_and_keeps_nan(device):
    shape = (5, 9, 33)
    x, grad = _inputs(shape, device)
    delta, beta = 0.1, 0.02 * 0.01
    free = torch.ops.nesvor.srr_step(x, grad, ALPHA, beta, delta, False)
    clamped = torch.ops.nesvor.srr_step(x, grad, ALPHA, beta, delta, True)
    neg = free < 0
    assert int(neg.sum()) > 100 and int((~neg).sum()) > 100
    assert bool((clamped[neg] == 0).all()) and torch.equal(clamped[~neg], free[~neg])
    # a NaN in x: NaN there and at its interior neighbours only (a border voxel takes no neighbour into account)
    xn = x.clone()
    z, y, c = 1, 4, 10  # next to the z = 0 border
    xn[z, y, c] = float("nan")
    expect = torch.zeros(shape, dtype=torch.bool, device=device)
    expect[z - 1:z + 2, y - 1:y + 2, c - 1:c + 2] = True
    expect &= ~_border(shape, device)
    assert int(expect.sum()) == 18
    for clamp in (False, True):
        out = torch.ops.nesvor.srr_step(xn, grad, ALPHA, beta, delta, clamp)
        assert torch.equal(torch.isnan(out), expect)
        ref = clamped if clamp else free
        assert torch.equal(out[~expect], ref[~expect])
    xb = x.clone()
    xb[0, 4, 10] = float("nan")  # on the border: that voxel alone, and the interior voxels that see it
    out = torch.ops.nesvor.srr_step(xb, grad, ALPHA, beta, delta, True)
    expect = torch.zeros(shape, dtype=torch.bool, device=device)
    expect[0:2, 3:6, 9:12] = True
    expect &= ~_border(shape, device)
    expect[0, 4, 10] = True
    assert torch.equal(torch.isnan(out), expect) and int(expect.sum()) == 10


@pytest.mark.gpu
def test_out_may_be_the_gradient_and_the_step_is_reproducible(device):
    from nesvor_amd.ops import srr_step_into

    for shape in ((11, 19, 70), (17, 8, 65)):
        x, grad = _inputs(shape, device)
        first = torch.ops.nesvor.srr_step(x, grad, ALPHA, 2e-4, 0.1, True)
        assert torch.equal(first, torch.ops.nesvor.srr_step(x, grad, ALPHA, 2e-4, 0.1, True))
        g1 = grad.clone()
        assert srr_step_into(x, g1, g1, ALPHA, 2e-4, 0.1, True) is g1 and torch.equal(g1, first)
        g2 = grad.clone()
        assert torch.ops.nesvor.srr_step_(x, g2, ALPHA, 2e-4, 0.1, True) is None and torch.equal(g2, first)


@pytest.mark.gpu
def test_step_refusals(device):
    """Every refusal returns before a launch (csrc/srr.hip: the checks are the first statements of nesvor_srr_step), so the
    sentinel in ``out`` stays."""
    from nesvor_amd import _lib
    from nesvor_amd.ops import srr_step_into

    lib = _lib.load()
    shape = (5, 9, 33)
    n = 5 * 9 * 33
    x, grad = _inputs(shape, device)
    buf = torch.full((2 * n + 64,), -7.0, device=device)
    out = buf[:n]
    call = lambda xp, gp, op, D, H, W: lib.nesvor_srr_step(xp, gp, op, D, H, W, ALPHA, 2e-4, 0.1, 1, _lib.stream_ptr())
    P = lambda t: _lib.ptr(t)
    assert call(None, P(grad), P(out), 5, 9, 33) != 0 and call(P(x), None, P(out), 5, 9, 33) != 0
    assert call(P(x), P(grad), None, 5, 9, 33) != 0
    for dims in ((0, 9, 33), (5, 0, 33), (5, 9, 0), (-1, 9, 33)):
        assert call(P(x), P(grad), P(out), *dims) != 0
    assert call(P(x), P(grad), P(out), 2048, 2048, 2048) != 0  # D H W > INT_MAX
    xs = buf[n + 32:2 * n + 32]  # x, out and grad inside one buffer: every overlap below is inside allocated memory
    assert call(P(xs), P(grad), P(xs), 5, 9, 33) != 0  # out == x
    assert call(P(xs), P(grad), P(buf[n + 40:2 * n + 40]), 5, 9, 33) != 0  # out overlaps x
    assert call(P(x), P(buf[8:n + 8]), P(out), 5, 9, 33) != 0  # out overlaps grad partially
    torch.cuda.synchronize()
    assert bool((buf == -7.0).all())
    with pytest.raises(RuntimeError, match="srr step"):
        srr_step_into(x, grad, x, ALPHA, 2e-4, 0.1, True)
    with pytest.raises(RuntimeError, match="srr step"):
        srr_step_into(x, buf[8:n + 8].view(shape), buf[:n].view(shape), ALPHA, 2e-4, 0.1, True)
    with pytest.raises(RuntimeError, match="srr step"):
        torch.ops.nesvor.srr_step(torch.empty((0, 3, 3), device=device), torch.empty((0, 3, 3), device=device), ALPHA, 2e-4, 0.1, True)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::srr_step'"):
        torch.ops.nesvor.srr_step(x.cpu(), grad.cpu(), ALPHA, 2e-4, 0.1, True)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.srr_step(x.double(), grad.double(), ALPHA, 2e-4, 0.1, True)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.nesvor.srr_step(x.transpose(0, 1), grad.transpose(0, 1), ALPHA, 2e-4, 0.1, True)
    with pytest.raises(RuntimeError, match="one shape"):
        torch.ops.nesvor.srr_step(x, grad[:4].contiguous(), ALPHA, 2e-4, 0.1, True)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: solver and pipeline on the 48^3 phantom (three stacks, 1.5 mm pixels, 3 mm slices, as tests/test_svr.py builds them)
# ---------------------------------------------------------------------------------------------------------------------
_RES_S, _THICK, _RES_R = 1.5, 3.0, 1.0
_STILL = {}


def _still(device):
    """The phantom, its three stacks WITHOUT motion (so the world frame is the phantom's) in the phantom's intensities, the
    acquisition operator on a 1 mm volume and the equalised back-projection; built once, never written."""
    if _STILL:
        return _STILL
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.registration import _cover_shape
    from nesvor_amd.srr import PSFreconstruction
    from nesvor_amd.svr import _frame, _operator
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=48), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=_RES_S, s_thick=_THICK, motion_deg=0, motion_mm=0, seed=0, normalize=False)
    n = len(slices) // 3
    stacks = [torch.stack([s.image for s in slices[j * n:(j + 1) * n]]).contiguous() for j in range(3)]
    poses = [RigidTransform.cat([s.transformation for s in slices[j * n:(j + 1) * n]]) for j in range(3)]
    images, m, frame_poses = _frame(stacks, None, poses, _RES_S)
    shape = _cover_shape(frame_poses, m, _RES_S, _THICK, _RES_R)
    op, params = _operator(images, m, frame_poses, _RES_S, _THICK, _RES_R, shape)
    _STILL.update(phantom=vol, stacks=stacks, poses=poses, images=images, mask=m, op=op, params=params,
                  start=PSFreconstruction(op.transforms, images, m, None, params))
    return _STILL


@pytest.mark.gpu
def test_fused_descent_follows_the_composed_one(device, monkeypatch):
    """Five steps from one start.  The yardstick is the same descent in fp64: the fused path may be off it by at most twice
    the drift of the composed fp32 path plus one ulp of the largest voxel - the kernel's bound, accumulated over the steps."""
    from nesvor_amd.srr import AcquisitionOperator, descent_step_bound, srr_descent

    c = _still(device)
    op, images, start = c["op"], c["images"], c["start"]
    beta, delta = 0.02, 0.1
    alpha = 1.0 / float(descent_step_bound(op, None, beta, like=start))
    monkeypatch.delenv("NESVOR_SRR", raising=False)
    fused = srr_descent(op, images, start, 5, beta, delta, alpha=alpha)
    again = srr_descent(op, images, start, 5, beta, delta, alpha=alpha)
    monkeypatch.setenv("NESVOR_SRR", "composed")
    composed = srr_descent(op, images, start, 5, beta, delta, alpha=alpha)
    monkeypatch.delenv("NESVOR_SRR")
    op64 = AcquisitionOperator(op.transforms.double(), {**c["params"], "psf": c["params"]["psf"].double()}, None, c["mask"])
    exact = srr_descent(op64, images.double(), start.double(), 5, beta, delta, alpha=alpha)
    assert exact.dtype == torch.float64 and fused.dtype == composed.dtype == torch.float32
    drift_fused = float((fused.double() - exact).abs().max())
    drift_composed = float((composed.double() - exact).abs().max())
    moved = float((exact - start.double()).abs().max())
    ulp = _ulp(exact.abs().max())
    print(f"alpha {alpha:.4e}; 5 steps moved the volume by up to {moved:.3e}; against fp64: fused {drift_fused:.3e}, "
          f"composed {drift_composed:.3e}; fused - composed {float((fused - composed).abs().max()):.3e}; ulp {ulp:.3e}")
    assert moved > 1e-3
    assert drift_fused <= 2 * drift_composed + ulp
    assert torch.equal(fused, again)
    assert fused.data_ptr() != start.data_ptr() and float(fused.min()) == 0.0


@pytest.mark.gpu
def test_descent_lowers_the_misfit_monotonically_without_a_prior(device, monkeypatch):
    """beta = 0, alpha = 1 / L: the weighted data misfit of eleven successive iterates (ten steps) never increases (relative
    slack 1e-5 for fp32 rounding)."""
    from nesvor_amd.srr import AcquisitionOperator, srr_descent

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    c = _still(device)
    inner, images = c["op"], c["images"]
    seen = []

    class Recording(AcquisitionOperator):
        def forward(self, volume):
            y = AcquisitionOperator.forward(self, volume)
            seen.append(((y - images).double() ** 2).sum())  # (the operator zeroes the pixels outside the mask; so is `images`)
            return y

    op = Recording(inner.transforms, c["params"], None, c["mask"])
    srr_descent(op, images, c["start"], 11, 0.0, 0.1)
    misfit = torch.stack(seen[1:]).tolist()  # (the first pass is the volume of ones of the step bound)
    print("misfit per iterate:", " ".join(f"{v:.6e}" for v in misfit))
    assert len(misfit) == 11
    assert all(b <= a * (1 + 1e-5) for a, b in zip(misfit[:-1], misfit[1:]))
    assert misfit[-1] < misfit[0]


@pytest.mark.gpu
def test_reconstruction_is_closer_to_the_phantom_than_its_start(device, monkeypatch):
    """The premise of SRR: thirty steps with the prior (beta 0.02, delta 0.1) end closer to the phantom - sampled at the voxel
    centres, inside the coverage mask - than the equalised back-projection they start from.  Measured on MI355X: DESIGN.md."""
    from nesvor_amd.image import Volume
    from nesvor_amd.svr import reconstruct_volume
    from nesvor_amd.transform import RigidTransform
    from nesvor_amd.utils import meshgrid

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    c = _still(device)
    rec = reconstruct_volume(c["stacks"], None, c["poses"], _RES_S, _THICK, _RES_R, n_iter=30, beta=0.02, delta=0.1)
    assert tuple(rec.image.shape) == tuple(c["start"].shape[-3:]) and float(rec.resolution_x) == _RES_R
    assert rec.mask.dtype == torch.bool and 0 < int(rec.mask.sum()) < rec.mask.numel()
    identity = RigidTransform(torch.eye(3, 4, device=device)[None])
    truth = Volume(c["phantom"], None, identity, 1.0, 1.0, 1.0).sample_points(rec.xyz_masked)
    peak = float(c["phantom"].max())
    psnr = lambda v: 10 * torch.log10(peak * peak / ((v[rec.mask].double() - truth.double()) ** 2).mean())
    p_start, p_rec = float(psnr(c["start"][0, 0])), float(psnr(rec.image))
    print(f"PSNR inside the mask ({int(rec.mask.sum())} voxels): back-projection {p_start:.3f} dB, 30 descent steps {p_rec:.3f} dB")
    assert p_rec > p_start


def _moving_stacks(device, tmp_path):
    """The three 48^3-phantom stacks with inter-slice motion of tests/test_svr.py as NIfTI files; also the number of non-empty slices."""
    from nesvor_amd.image import Volume
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=48), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, n_stacks=3, res_s=_RES_S, s_thick=_THICK, motion_deg=2, motion_mm=1, seed=0)
    n = len(slices) // 3
    paths, n_nonempty = [], 0
    for j in range(3):
        ss = slices[j * n:(j + 1) * n]
        img = torch.stack([s.image for s in ss])[:, 0].contiguous()
        n_nonempty += int((img > 0).flatten(1).any(1).sum())
        ax = RigidTransform.cat([s.transformation for s in ss]).axisangle().mean(0, keepdim=True)  # stack centre pose
        p = str(tmp_path / f"stack{j}.nii.gz")
        Volume(img, img > 0, RigidTransform(ax), _RES_S, _RES_S, _THICK).save(p, masked=False)
        paths.append(p)
    return paths, n_nonempty


@pytest.mark.gpu
def test_cli_svr(tmp_path, device, monkeypatch):
    from nesvor_amd import cli, svr
    from nesvor_amd.image_io import load_volume

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    paths, n_nonempty = _moving_stacks(device, tmp_path)
    made = []
    inner = svr.reconstruct_volume

    def spy(*a, **k):
        made.append(inner(*a, **k))
        return made[-1]

    monkeypatch.setattr(svr, "reconstruct_volume", spy)
    out, sim = str(tmp_path / "v.nii.gz"), str(tmp_path / "sim")
    cli.main(["svr", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--output-volume", out, "--simulated-slices", sim,
              "--n-iter-srr", "5", "--verbose", "0"])
    assert len(made) == 1
    vol = made[0]  # the object the command rescaled and wrote
    assert int(vol.mask.sum()) > 1000
    mean = float(vol.v_masked.double().mean())
    print(f"volume {tuple(vol.image.shape)}, {int(vol.mask.sum())} voxels in the mask, masked mean {mean:.4f}")
    assert mean == pytest.approx(700.0, rel=1e-5)
    back = load_volume(out, device=device)
    assert tuple(back.image.shape) == tuple(vol.image.shape)
    for r in (back.resolution_x, back.resolution_y, back.resolution_z):
        assert float(r) == pytest.approx(0.8, abs=1e-6)
    torch.testing.assert_close(back.image, vol.image * vol.mask, rtol=1e-6, atol=1e-4)
    assert float(back.image.max()) > 700.0 and float(back.image.min()) == 0.0
    assert len([f for f in os.listdir(sim) if f.endswith(".nii.gz")]) == n_nonempty > 30
    with pytest.raises(NotImplementedError, match="svr"):
        cli.main(["svr", "--input-stacks", *paths, "--registration", "svort", "--output-volume", str(tmp_path / "never.nii.gz"),
                  "--verbose", "0"])


@pytest.mark.gpu
def test_cli_svr_from_registered_slices(tmp_path, device, monkeypatch):
    """``--input-slices`` on what ``register`` wrote reconstructs the same object as the stacks themselves.  The poses come back
    from the files' affines within fp32 rounding; that can flip a pixel's "PSF weight >= 0.5" decision at the rim of the volume or
    a ``ceil`` of the covering shape, so the volumes are compared on their common centre by correlation, not bit by bit: a wrong
    pixel size, thickness, slice order or pose convention moves the object by a voxel or more and costs far more than 1e-3."""
    from nesvor_amd import cli
    from nesvor_amd.image_io import load_volume

    monkeypatch.delenv("NESVOR_SRR", raising=False)
    paths, n_nonempty = _moving_stacks(device, tmp_path)
    folder, a, b = str(tmp_path / "slices"), str(tmp_path / "a.nii.gz"), str(tmp_path / "b.nii.gz")
    common = ["--thicknesses", "3", "3", "3", "--registration", "none", "--verbose", "0"]
    cli.main(["register", "--input-stacks", *paths, "--output-slices", folder, *common])
    assert len([f for f in os.listdir(folder) if f.endswith(".nii.gz")]) == n_nonempty
    cli.main(["svr", "--input-slices", folder, "--output-volume", a, "--n-iter-srr", "3", "--verbose", "0"])
    cli.main(["svr", "--input-stacks", *paths, "--output-volume", b, "--n-iter-srr", "3", *common])
    va, vb = load_volume(a, device=device), load_volume(b, device=device)
    for v in (va, vb):
        assert float(v.resolution_x) == pytest.approx(0.8, abs=1e-6) and float(v.image.max()) > 700.0
        assert all(s % 2 == 1 for s in v.image.shape)  # centred at the origin with a voxel on it: central crops line up
    size = [min(p, q) for p, q in zip(va.image.shape, vb.image.shape)]
    crop = lambda t: t[tuple(slice((n - s) // 2, (n - s) // 2 + s) for n, s in zip(t.shape, size))].double()
    x, y = crop(va.image), crop(vb.image)
    x, y = x - x.mean(), y - y.mean()
    ncc = float((x * y).sum() / (x.norm() * y.norm()))
    print(f"volumes {tuple(va.image.shape)} / {tuple(vb.image.shape)}: correlation of the two routes 1 - {1 - ncc:.3e}")
    assert ncc > 1 - 1e-3
