"""The joint histograms of the stack registration's mutual-information similarity (csrc/vvr_nmi.hip: ``nesvor_vvr_joint_histogram``,
``nesvor_vvr_sample``) and what ``VVR`` / ``register_stacks`` / the command line do with them.

1. Bit for bit: the fused histogram equals ``nmi.joint_histogram`` of the kernel's own samples over point counts at wave / workgroup /
   segment edges, pose counts, bin counts, degenerate maps; nothing outside ``hist`` and the workspace's stated size is written; two
   runs agree.
2. Correctness: a cell above 2^32; the samples per point and the histogram per cell against the float64 yardstick of
   tests/vvr_nmi_reference.py within its derived bounds; the samples' sums against ``nesvor_vvr_similarity``; the refusals.
3. Paths and outcome: the three evaluation paths of ``VVR`` on one level; the registration of a stack pair whose intensities are
   related by the non-monotone J -> 4 J (1 - J), in both directions, against NCC from the same start; ``register_stacks`` and the
   ``register`` command."""
import ctypes
import math
import os
import types

import pytest
import torch

import vvr_nmi_reference as N
import vvr_reference as R
from nesvor_amd import nmi

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
CANARY = 64  # sentinel words on either side of hist and past the workspace
_DEV = {}


def _on(device):
    """The yardstick's case on the device, uploaded once."""
    if "case" not in _DEV:
        c = N.case()
        _DEV["case"] = {k: c[k].to(device) for k in ("src", "points", "target", "mats")}
    return _DEV["case"]


def _unit(c):
    return (ctypes.c_float * 3)(*c["unit"])


def _raw(device, src, points, target, mats, unit, M, K, bins, i_map, j_map, workspace_bytes=None, null_workspace=False, dims=None):
    """nesvor_vvr_joint_histogram through ctypes between canaries -> (error code, hist (K,B,B) on the device, canaries intact)."""
    from nesvor_amd import _lib

    lib = _lib.load()
    D, H, W = src.shape[-3:] if dims is None else dims
    cells = max(K, 0) * bins * bins
    buf = torch.full((cells + 2 * CANARY,), -7, dtype=torch.int64, device=device)
    need = int(lib.nesvor_vvr_joint_histogram_workspace_bytes(M, K, bins))
    nbytes = need if workspace_bytes is None else workspace_bytes
    ws = torch.full((max(need, 8) // 4 + CANARY,), 0x5A5A5A5A, dtype=torch.int32, device=device)
    err = lib.nesvor_vvr_joint_histogram(_lib.ptr(src), D, H, W, _lib.ptr(points), _lib.ptr(target), _lib.ptr(mats), unit, M, K,
                                         *(float(v) for v in (*i_map, *j_map)), bins, ctypes.c_void_p(buf.data_ptr() + 8 * CANARY),
                                         None if null_workspace else _lib.ptr(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    intact = bool((buf[:CANARY] == -7).all()) and bool((buf[CANARY + cells:] == -7).all()) and bool((ws[need // 4:] == 0x5A5A5A5A).all())
    return err, buf[CANARY:CANARY + cells].view(max(K, 0), bins, bins), intact, need


# ---------------------------------------------------------------------------------------------------------------------
# 1. bit for bit against the composed definition
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", N.MS)
def test_fused_equals_composed_bit_for_bit(device, M):
    """Every K in KS and B in BINS at this M: the kernel's histogram is ``nmi.joint_histogram`` of ``vvr_sample``'s values; its total
    is 65536 M per pose; the canaries around ``hist`` and past the workspace's stated size are untouched; a second run agrees; the
    op gives the same.  M = 70001 takes more than one segment for every K (a segment holds at most 16384 points)."""
    from nesvor_amd import ops  # noqa: F401

    c, d = N.case(), _on(device)
    points, J = d["points"][:M].contiguous(), d["target"][:M].contiguous()
    unit = _unit(c)
    I = torch.ops.nesvor.vvr_sample(d["src"], points, d["mats"], list(c["unit"]))
    assert I.shape == (N.POSES, M) and I.dtype == torch.float32
    assert torch.equal(torch.ops.nesvor.vvr_sample(d["src"], points, d["mats"][5:7].contiguous(), list(c["unit"])), I[5:7])
    for bins in N.BINS:
        i_map, j_map = N.maps(c, M, bins)
        for K in N.KS:
            err, hist, intact, need = _raw(device, d["src"], points, J, d["mats"], unit, M, K, bins, i_map, j_map)
            assert err == 0 and intact, (K, bins)
            if M == 70001:
                assert need >= 2 * 4 * K * bins * bins  # at least two segments
            assert torch.equal(hist, N.bin_samples(I[:K], J, i_map, j_map, bins)), (K, bins)
            assert hist.sum((1, 2)).tolist() == [nmi.UNITS * M] * K
            if K in (1, 13):
                again = _raw(device, d["src"], points, J, d["mats"], unit, M, K, bins, i_map, j_map)[1]
                via_op = torch.ops.nesvor.vvr_joint_histogram(d["src"], points, J, d["mats"][:K].contiguous(), list(c["unit"]), *i_map, *j_map, bins)
                assert torch.equal(again, hist) and torch.equal(via_op, hist)


@pytest.mark.parametrize("M", [257, 70001])
def test_degenerate_maps(device, M):
    """A J range of one value (scale 0): every point lands in column 0.  A constant source (i_scale 0): every point lands in row 0,
    the points outside the source included.  Both equal the composed definition."""
    c, d = N.case(), _on(device)
    points, J = d["points"][:M].contiguous(), d["target"][:M].contiguous()
    K, bins = 13, 32
    i_map, j_map = N.maps(c, M, bins, j_degenerate=True)
    assert j_map[1] == 0.0
    I = torch.ops.nesvor.vvr_sample(d["src"], points, d["mats"][:K].contiguous(), list(c["unit"]))
    err, hist, intact, _ = _raw(device, d["src"], points, J, d["mats"], _unit(c), M, K, bins, i_map, j_map)
    assert err == 0 and intact and torch.equal(hist, N.bin_samples(I, J, i_map, j_map, bins))
    assert bool((hist[:, :, 1:] == 0).all()) and hist[:, :, 0].sum(1).tolist() == [nmi.UNITS * M] * K
    flat = torch.full(N.SHAPE, 0.7, device=device)
    i_map = tuple(nmi.axis_map(flat.min(), flat.max(), bins).tolist())
    assert i_map[1] == 0.0
    j_map = N.maps(c, M, bins)[1]
    I = torch.ops.nesvor.vvr_sample(flat, points, d["mats"][:K].contiguous(), list(c["unit"]))
    assert bool((I == 0).any()) and bool((I > 0.69).any())
    err, hist, intact, _ = _raw(device, flat, points, J, d["mats"], _unit(c), M, K, bins, i_map, j_map)
    assert err == 0 and intact and torch.equal(hist, N.bin_samples(I, J, i_map, j_map, bins))
    assert bool((hist[:, 1:] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 2. correctness
# ---------------------------------------------------------------------------------------------------------------------
def test_a_cell_above_two_to_the_32(device):
    """A constant source and a constant target: both scales are 0 and all 70001 points put their 65536 units into cell (0, 0) -
    4.59e9, more than a 32-bit cell holds, so the segments are added in 64 bits."""
    c, d = N.case(), _on(device)
    M, bins = 70001, 32
    flat, J = torch.full(N.SHAPE, 0.7, device=device), torch.full((M,), 0.3, device=device)
    i_map = tuple(nmi.axis_map(flat.min(), flat.max(), bins).tolist())
    j_map = tuple(nmi.axis_map(J.min(), J.max(), bins).tolist())
    assert i_map[1] == 0.0 and j_map[1] == 0.0
    for K in (1, 13):
        err, hist, intact, _ = _raw(device, flat, d["points"], J, d["mats"], _unit(c), M, K, bins, i_map, j_map)
        assert err == 0 and intact
        assert hist[:, 0, 0].tolist() == [M * nmi.UNITS] * K and M * nmi.UNITS > 2 ** 32
        assert int(hist.sum()) == K * M * nmi.UNITS


def test_samples_and_cells_against_the_float64_yardstick(device):
    """``vvr_sample`` per point within the yardstick's bound e (tests/vvr_nmi_reference.py: 4 x the measured coordinate term, plus the
    13 roundings of the value arithmetic), all 27 poses and 70001 points.  The histogram's J marginal equals the yardstick's exactly
    (J and its map are inputs); every cell lies within its derived bound."""
    c, d = N.case(), _on(device)
    I = torch.ops.nesvor.vvr_sample(d["src"], d["points"], d["mats"], list(c["unit"])).cpu().double()
    err = (I - N.samples(c)).abs()
    e = N.sample_bound(c)
    worst = float((err / e.clamp(min=1e-300)).max())
    print(f"vvr_sample: worst |kernel - fp64| / bound {worst:.3f}; largest |kernel - fp64| {float(err.max()):.3e}, largest bound {float(e.max()):.3e}")
    assert bool((err <= e).all())
    assert bool((I[N.magnitude(c) == 0] == 0).all())
    for K, M, bins in ((13, 4001, 32), (2, 70001, 64), (14, 257, 5)):
        ref, bounds = N.histograms(c, K, M, bins)
        i_map, j_map = N.maps(c, M, bins)
        got = torch.ops.nesvor.vvr_joint_histogram(d["src"], d["points"][:M].contiguous(), d["target"][:M].contiguous(),
                                                   d["mats"][:K].contiguous(), list(c["unit"]), *i_map, *j_map, bins).cpu()
        assert torch.equal(got.sum(1), ref.sum(1))
        diff = (got - ref).abs().double()
        print(f"K = {K}, M = {M}, B = {bins}: worst |cell - yardstick| / bound {float((diff / bounds.clamp(min=1e-300)).max()):.3f}, "
              f"cells that differ {int((diff > 0).sum())} of {diff.numel()}")
        assert bool((diff <= bounds).all())


def test_the_samples_sums_agree_with_the_moment_kernel(device):
    """sum I, sum I^2 and sum I J of ``vvr_sample``'s output (added in float64) against ``nesvor_vvr_similarity`` on the same
    inputs, at the tolerance of tests/test_gpu_vvr_similarity.py: its accumulation bound plus COORD_TOL, relative to the sums of the
    terms' magnitudes."""
    from test_gpu_vvr_similarity import COORD_TOL
    from nesvor_amd import _lib

    c, d = N.case(), _on(device)
    M, K = N.M_MAX, N.POSES
    I = torch.ops.nesvor.vvr_sample(d["src"], d["points"], d["mats"], list(c["unit"])).double()
    J = d["target"].double()
    mine = torch.stack([I.sum(1), (I * I).sum(1), (I * J).sum(1)], 1).cpu()
    sums = torch.full((K, 3), -7.0, dtype=torch.float64, device=device)
    D, H, W = N.SHAPE
    err = _lib.load().nesvor_vvr_similarity(_lib.ptr(d["src"]), D, H, W, _lib.ptr(d["points"]), _lib.ptr(d["target"]), _lib.ptr(d["mats"]),
                                            _unit(c), M, K, _lib.ptr(sums), None, _lib.stream_ptr())
    assert err == 0
    torch.cuda.synchronize()
    mags = torch.stack([N.samples(c, torch.float64, True).sum(1), (I * I).sum(1).cpu(), (I * J).abs().sum(1).cpu()], 1)
    b, _ = R.accumulation_bound(M, mags, torch.zeros(2, dtype=torch.float64))
    tol = b + COORD_TOL * mags
    diff = (sums.cpu() - mine).abs()
    print(f"sums of vvr_sample against nesvor_vvr_similarity: worst difference / tolerance {float((diff / tol).max()):.3e}")
    assert bool((diff <= tol).all())


def test_refusals_leave_hist_alone(device):
    """hipErrorInvalidValue without a launch - a size below 1, bins outside [2, 64], a NULL or too small workspace, an M or a grid
    that does not fit an int - and the no-ops K <= 0, M <= 0: ``hist`` keeps its sentinels.  M = 0 through the op gives zeros."""
    from nesvor_amd import _lib

    c, d = N.case(), _on(device)
    M, K, bins = 4001, 2, 8
    points, J = d["points"][:M].contiguous(), d["target"][:M].contiguous()
    i_map, j_map = N.maps(c, M, bins)
    args = (device, d["src"], points, J, d["mats"], _unit(c))
    need = int(_lib.load().nesvor_vvr_joint_histogram_workspace_bytes(M, K, bins))
    assert need >= 4 * K * bins * bins
    cases = {"D = 0": dict(dims=(0, 11, 9)), "W = 0": dict(dims=(6, 11, 0)), "NULL workspace": dict(null_workspace=True),
             "small workspace": dict(workspace_bytes=need - 1)}
    for what, kw in cases.items():
        err, hist, intact, _ = _raw(*args, M, K, bins, i_map, j_map, **kw)
        assert err == INVALID and intact and bool((hist == -7).all()), what
    lib = _lib.load()
    sentinel = torch.full((K * 64 * 64,), -7, dtype=torch.int64, device=device)
    ws = torch.zeros(1 << 16, dtype=torch.int32, device=device)

    def call(M_, K_, bins_):
        return lib.nesvor_vvr_joint_histogram(_lib.ptr(d["src"]), 6, 11, 9, _lib.ptr(points), _lib.ptr(J), _lib.ptr(d["mats"]), _unit(c), M_, K_,
                                              *(float(v) for v in (*i_map, *j_map)), bins_, _lib.ptr(sentinel), _lib.ptr(ws), ws.numel() * 4,
                                              _lib.stream_ptr())

    for bad in (1, 0, 65, -3):
        assert call(M, K, bad) == INVALID and lib.nesvor_vvr_joint_histogram_workspace_bytes(M, K, bad) == 0, bad
    assert call(2 ** 31, 1, bins) == INVALID  # M does not fit an int
    assert call(2 ** 31 - 1, 16385, bins) == INVALID  # 131072 segments x 16385 poses: the grid does not fit an int
    assert call(M, 0, bins) == 0 and call(M, -1, bins) == 0 and call(0, K, bins) == 0 and call(-5, K, bins) == 0  # no-ops
    torch.cuda.synchronize()
    assert bool((sentinel == -7).all())
    empty = torch.ops.nesvor.vvr_joint_histogram(d["src"], points[:0], J[:0], d["mats"][:3].contiguous(), list(c["unit"]), *i_map, 0.0, 0.0, bins)
    assert empty.shape == (3, bins, bins) and empty.dtype == torch.int64 and int(empty.abs().sum()) == 0
    assert torch.ops.nesvor.vvr_sample(d["src"], points[:0], d["mats"][:3].contiguous(), list(c["unit"])).shape == (3, 0)


# ---------------------------------------------------------------------------------------------------------------------
# 3. paths and outcome
# ---------------------------------------------------------------------------------------------------------------------
def test_the_three_paths_give_one_loss(device, monkeypatch):
    """``VVR`` on one level (the yardstick's case as the level: its source, its first 4001 points and their values), the 13 poses of a
    gradient and a K = 1 call: fused equals composed exactly.  Generic (``grid_sample``) differs by fp32 sampling in another order:
    both it and the kernel lie within the yardstick's per-cell bounds b of the float64 histogram, so their cells differ by at most
    2 b, and to first order  |d loss| <= sum_c |d loss / d h_c| 2 b_c  with the derivative taken by autograd in fp64 at the yardstick's
    histogram, 1 % for the higher orders (b_c is about 1 % of a populated cell), plus the two roundings of the losses to fp32."""
    from nesvor_amd.registration import VVR
    from nesvor_amd.transform import RigidTransform

    c, d = N.case(), _on(device)
    M, bins = 4001, 32
    lv = types.SimpleNamespace(source=d["src"][None, None], points=d["points"][:M].contiguous(), values=d["target"][:M].contiguous(),
                               to_unit=N.unit32(c).to(device), to_unit_host=_unit(c), target_sums=None, i_map=None, j_map=None)
    vvr = VVR(1, 1, 1, 1, {"name": "gd"}, {"name": "nmi", "bins": bins}, False)
    vvr.trans_first = True
    vvr.theta_t = RigidTransform(torch.tensor([[0.05, -0.03, 0.04, 0.4, -0.3, 0.2]], device=device))
    g = torch.Generator().manual_seed(31)
    thetas = (torch.randn(13, 6, generator=g) * torch.tensor([4.0, 4.0, 4.0, 0.5, 0.5, 0.5])).to(device)  # degrees, mm
    assert vvr._fused(thetas[:1], lv)
    monkeypatch.delenv("NESVOR_VVR_NMI", raising=False)
    fused, fused1 = vvr._objective_fused(thetas, lv), vvr._objective_fused(thetas[4:5], lv)
    assert (lv.i_map, lv.j_map) == N.maps(c, M, bins)
    monkeypatch.setenv("NESVOR_VVR_NMI", "composed")
    composed, composed1 = vvr._objective_fused(thetas, lv), vvr._objective_fused(thetas[4:5], lv)
    assert torch.equal(fused, composed) and torch.equal(fused1, composed1) and torch.equal(fused1, fused[4:5])
    assert fused.shape == (13,) and fused.dtype == torch.float32 and bool((fused < 0).all())
    generic = vvr._objective(thetas, lv)
    mats = RigidTransform(thetas * vvr._unit(thetas), trans_first=True).inv().compose(vvr.theta_t).matrix().cpu()
    ref, bounds = N.histograms(c, 13, M, bins, mats=mats)
    h = ref.double().requires_grad_(True)
    loss = _loss64(h)
    assert torch.allclose(loss.detach(), nmi.nmi_loss(ref), rtol=1e-12, atol=0)
    tol = torch.zeros(13, dtype=torch.float64)
    for k in range(13):
        (gk,) = torch.autograd.grad(loss[k], h, retain_graph=True)
        tol[k] = 1.01 * (gk[k].abs() * 2 * bounds[k]).sum() + 2 * R.U * float(loss[k].detach().abs())
    diff = (fused.double().cpu() - generic.double().cpu()).abs()
    print(f"PATHS: loss {float(fused[0]):.6f}; largest |fused - generic| {float(diff.max()):.3e}, tolerance {float(tol.min()):.3e} .. {float(tol.max()):.3e}; "
          f"|fused - yardstick| {float((fused.double().cpu() - loss.detach()).abs().max()):.3e}")
    assert bool((diff <= tol).all())
    assert bool(((fused.double().cpu() - loss.detach()).abs() <= tol).all())


def _loss64(h):
    """nmi.nmi_loss on float64 histograms that carry a gradient (the module's takes integers)."""
    n = h.sum((-2, -1))
    p = h / n[..., None, None]
    ent = lambda q, dims: -(torch.where(q > 0, q * torch.log(torch.where(q > 0, q, torch.ones_like(q))), torch.zeros_like(q))).sum(dims)
    return 1 - (ent(p.sum(-1), -1) + ent(p.sum(-2), -1)) / ent(p, (-2, -1))


def _pose_error(ax, truth, trans_first):
    """(rotation error in degrees, translation error in mm) between two poses given as axis-angle rows."""
    from nesvor_amd.transform import RigidTransform

    a = RigidTransform(ax, trans_first=trans_first).matrix()[0].double().cpu()
    b = truth.matrix()[0].double().cpu()
    cos = ((a[:, :3].T @ b[:, :3]).trace() - 1) / 2
    return math.degrees(math.acos(float(cos.clamp(-1, 1)))), float((a[:, 3] - b[:, 3]).norm())


@pytest.mark.parametrize("remapped", ["source", "target"])
def test_registration_across_a_non_monotone_intensity_map(device, remapped):
    """The 64^3 phantom, every other slice (32 slices: 1 mm in-plane, 2 mm through-plane), against itself with one side's
    intensities remapped by J -> 4 J (1 - J), from (6, 2, -4 deg; 4, -3, 2 mm) off the truth; 3 levels, 4 rounds, momentum 0.1,
    32 bins.  With nmi the pose comes back within 0.5 deg and 0.5 mm, and its translation error is below half of what global NCC
    reaches from the same start."""
    from nesvor_amd.phantom import phantom3d
    from nesvor_amd.registration import VVR
    from nesvor_amd.transform import RigidTransform

    plain = torch.tensor(phantom3d(n=64), dtype=torch.float32, device=device)[::2][None, None].contiguous()
    other = (4 * plain * (1 - plain)).contiguous()
    source, target = (other, plain) if remapped == "source" else (plain, other)
    trans_first = False
    truth = RigidTransform(torch.zeros((1, 6), device=device), trans_first=trans_first)
    offset = torch.tensor([[math.radians(6.0), math.radians(2.0), math.radians(-4.0), 4.0, -3.0, 2.0]], device=device)
    start = truth.axisangle(trans_first=trans_first) + offset
    result = {}
    for name, loss in (("nmi", {"name": "nmi"}), ("ncc", {"name": "ncc", "win": None})):
        vvr = VVR(num_levels=3, num_steps=4, step_size=2, max_iter=20, optimizer={"name": "gd", "momentum": 0.1}, loss=loss, auto_grad=False)
        out, value = vvr(start.clone(), source, target, {"res_s": 1.0, "s_thick": 2.0}, truth, trans_first)
        result[name] = _pose_error(out, truth, trans_first) + (float(value),)
    rot0, tr0 = _pose_error(start, truth, trans_first)
    print(f"OUTCOME {remapped} remapped: start {rot0:.2f} deg {tr0:.2f} mm; nmi {result['nmi'][0]:.3f} deg {result['nmi'][1]:.3f} mm "
          f"(loss {result['nmi'][2]:.4f}); ncc {result['ncc'][0]:.3f} deg {result['ncc'][1]:.3f} mm (loss {result['ncc'][2]:.4f})")
    assert result["nmi"][0] < 0.5 and result["nmi"][1] < 0.5
    assert result["nmi"][1] < 0.5 * result["ncc"][1]


def _remapped_stacks(device):
    """The two stacks of tests/test_registration.py::test_register_stacks_removes_a_rigid_offset - the same content, the second one's
    poses off by 4 deg / 3 mm - with the second stack's intensities remapped by J -> 4 J (1 - J)."""
    from nesvor_amd.image import Stack
    from nesvor_amd.phantom import phantom3d
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=64), dtype=torch.float32, device=device)
    n = 32
    slices = vol[::2][:, None].contiguous()  # (32,1,64,64): 1 mm in-plane, 2 mm through-plane

    def poses(offset):
        t = torch.zeros((n, 6), dtype=torch.float32, device=device)
        t[:, -1] = (torch.arange(n, dtype=torch.float32, device=device) - (n - 1) / 2) * 2.0
        return offset.compose(RigidTransform(t))

    ident = RigidTransform(torch.zeros((1, 6), device=device))
    off = RigidTransform(torch.tensor([[math.radians(4.0), 0.0, math.radians(-2.0), 3.0, -2.0, 1.0]], device=device))
    return [Stack(slices.clone(), slices > 0, poses(ident), resolution_x=1.0, resolution_y=1.0, thickness=2.0, gap=2.0),
            Stack((4 * slices * (1 - slices)).contiguous(), slices > 0, poses(off), resolution_x=1.0, resolution_y=1.0, thickness=2.0, gap=2.0)]


def test_register_stacks_with_nmi_removes_a_rigid_offset_across_the_remap(device):
    """``register_stacks(stacks, similarity="nmi")``: after registration both stacks sit at the same place again, at the pose
    tolerances of the same-contrast test (rotation entries within 6e-3, translation within 0.3 mm)."""
    from nesvor_amd.registration import register_stacks

    stacks = register_stacks(_remapped_stacks(device), similarity="nmi")
    a, b = stacks[0].transformation.matrix(), stacks[1].transformation.matrix()
    print(f"REGISTER_STACKS nmi: largest rotation entry difference {float((a[:, :, :3] - b[:, :, :3]).abs().max()):.2e}, "
          f"largest translation difference {float((a[:, :, 3] - b[:, :, 3]).abs().max()):.3f} mm")
    assert float((a[:, :, :3] - b[:, :, :3]).abs().max()) < 6e-3
    assert float((a[:, :, 3] - b[:, :, 3]).abs().max()) < 0.3


def test_cli_register_stack_with_nmi(tmp_path, device):
    """``register --registration stack --stack-similarity nmi`` end to end on those stacks, written as files: every non-empty slice
    comes out and loads again (the poses are the test's above)."""
    from nesvor_amd import cli
    from nesvor_amd.image import Volume
    from nesvor_amd.image_io import load_slices
    from nesvor_amd.transform import RigidTransform

    paths, n_nonempty = [], 0
    for j, st in enumerate(_remapped_stacks(device)):
        img = st.slices[:, 0]
        n_nonempty += int((img > 0).flatten(1).any(1).sum())
        ax = st.transformation.axisangle().mean(0, keepdim=True)  # stack centre pose
        p = str(tmp_path / f"stack{j}.nii.gz")
        Volume(img, img > 0, RigidTransform(ax), 1.0, 1.0, 2.0).save(p, masked=False)
        paths.append(p)
    out = str(tmp_path / "slices")
    cli.main(["register", "--input-stacks", *paths, "--thicknesses", "2", "2", "--registration", "stack", "--stack-similarity", "nmi",
              "--nmi-bins", "32", "--output-slices", out, "--verbose", "0"])
    files = [f for f in os.listdir(out) if not f.startswith("mask")]
    assert len(files) == n_nonempty > 40
    assert len(load_slices(out)) == n_nonempty
