"""The moment sums of the volume-to-volume registration kernel (csrc/vvr.hip, ``nesvor_vvr_similarity``) against the float64
restatement of tests/vvr_reference.py: every sum of every pose - not the loss - at both instantiations (13 poses per pass and
single poses), mixed passes, the ``target_sums`` hand-over, wave / workgroup / grid-stride edges of the point count, thin and
one-voxel volumes, clouds partly and wholly outside the source, and the loss ``VVR._objective_fused`` forms from the sums.

Two kinds of case.  LATTICE: every coordinate is exact in fp32 (dyadic voxel sizes, points, translations; rotations with entries
0 and +-1), so the kernel can differ from the reference only by its fp32 value arithmetic and partial sums - the derived
accumulation bound of tests/vvr_reference.py, asserted as it stands.  GENERIC: random points and poses; the kernel's fp32
coordinates add a term that cannot be derived from the formats alone (a sample is Lipschitz, not smooth, in its coordinate) and
is measured BETWEEN REFERENCES - ``vvr_sums(float32)`` against ``vvr_sums(float64)`` on the generic inputs, on the CPU
(COORD_MEASURED) - and asserted at 4 x that rounded up to a power of ten (COORD_TOL, the SCORE_TOL convention of
tests/test_gpu_assess.py), relative to the sum of the terms' magnitudes.  Nothing is fitted to the kernel's output."""
import ctypes
import types

import pytest
import torch

import vvr_reference as R

pytestmark = pytest.mark.gpu

# ---- lattice case: source (D,H,W) = (5,9,17) of 2 x 1 x 0.5 mm voxels, so to_unit = 2 / (size - 1) / voxel = 1/4 on every axis
# and the volume is the cube |x|, |y|, |z| <= 4 mm; points every 0.25 / 0.5 / 0.5 mm from -4 to +6 mm (1.5 x beyond the volume on
# the positive side): index coordinates 2 x + 8, y + 4, z / 2 + 2 with fractions in {0, 1/4, 1/2, 3/4}
LATTICE_SHAPE = (5, 9, 17)
LATTICE_UNIT = (0.25, 0.25, 0.25)
LATTICE_STEP = (0.25, 0.5, 0.5)
LATTICE_ROTATIONS = [[[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[0, -1, 0], [1, 0, 0], [0, 0, 1]], [[0, 1, 0], [0, 0, 1], [1, 0, 0]]]
LATTICE_TRANSLATIONS = [(0.0, 0.0, 0.0), (0.25, -1.5, 2.0), (-8.0, 4.0, 0.125)]  # share of the cloud that touches the volume: about 68 %, 53 %, 12 %
LATTICE_KS = [1, 2, 9]
# ---- generic case: a 3 x 3 x 3-averaged random source of 1 mm voxels, random points over 1.5 x its extent, 27 random poses
GENERIC_SHAPE = (21, 32, 30)
GENERIC_M = 70001
GENERIC_POSES = 27
GENERIC_KS = [1, 13, 14, 26, 27]  # 13 poses per pass, then single poses: 1, 13, 13 + 1, 13 + 13, 13 + 13 + 1
# largest |vvr_sums(float32) - vvr_sums(float64)| / sum |terms| over the 27 poses and the three sums of the generic case,
# measured on the CPU (no kernel involved); asserted at 4 x that, rounded up to a power of ten
COORD_MEASURED, COORD_TOL = 3.394e-8, 1e-6
M_EDGES = [1, 63, 64, 65, 255, 256, 257]  # inside / at / past one wave and one workgroup
M_STRIDE = 2048 * 256 + 257  # past the largest grid: the first 257 threads take a second trip of the grid-stride loop
THIN_SHAPES = [(1, 1, 1), (1, 5, 7), (2, 3, 4)]
_DATA = {}


def _lattice_mats():
    mats = []
    for rot in LATTICE_ROTATIONS:
        for t in LATTICE_TRANSLATIONS:
            mats.append(torch.cat([torch.tensor(rot, dtype=torch.float32), torch.tensor(t, dtype=torch.float32)[:, None]], 1))
    order = [0, 3, 6, 1, 4, 7, 2, 5, 8]  # translation-major: the first three poses have translation 0
    return torch.stack([mats[i] for i in order])


def _lattice():
    if "lattice" not in _DATA:
        g = torch.Generator().manual_seed(11)
        src = torch.rand(LATTICE_SHAPE, generator=g)
        axes = [torch.arange(-4.0, 6.0 + 1e-6, s) for s in LATTICE_STEP]
        z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
        points = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
        target = torch.rand(points.shape[0], generator=g)
        _DATA["lattice"] = dict(src=src, points=points, target=target, mats=_lattice_mats(), unit=LATTICE_UNIT)
    return _DATA["lattice"]


def _generic():
    if "generic" not in _DATA:
        from oracle import transform_convert as tc

        g = torch.Generator().manual_seed(12)
        D, H, W = GENERIC_SHAPE
        src = torch.nn.functional.avg_pool3d(torch.rand(1, 1, D + 2, H + 2, W + 2, generator=g), 3, 1)[0, 0].contiguous()
        half = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0])
        points = ((torch.rand(GENERIC_M, 3, generator=g) * 2 - 1) * 1.5 * half).contiguous()
        target = torch.rand(GENERIC_M, generator=g)
        ax = torch.randn(GENERIC_POSES, 6, generator=g) * torch.tensor([0.3, 0.3, 0.3, 3.0, 3.0, 3.0])
        unit = (2.0 / (W - 1), 2.0 / (H - 1), 2.0 / (D - 1))
        _DATA["generic"] = dict(src=src, points=points, target=target, mats=tc.axisangle2mat_forward(ax).contiguous(), unit=unit)
    return _DATA["generic"]


def _unit32(c):
    """to_unit as the kernel reads it: three floats."""
    return torch.tensor(c["unit"], dtype=torch.float32)


def _reference(c, name):
    """(sums, tsums, mags, tmags) of a case in float64, computed once."""
    key = ("ref", name)
    if key not in _DATA:
        _DATA[key] = R.vvr_sums(c["src"], c["points"], c["target"], c["mats"], _unit32(c), torch.float64, with_abs=True)
    return _DATA[key]


def _is_lattice(c):
    """The case's fp32 coordinates are its fp64 coordinates: the two references agree to the last bit."""
    a = R.vvr_sums(c["src"], c["points"], c["target"], c["mats"], _unit32(c), torch.float32)
    b = R.vvr_sums(c["src"], c["points"], c["target"], c["mats"], _unit32(c), torch.float64)
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def _launch(device, c, K=None):
    """nesvor_vvr_similarity through ctypes, as nesvor_amd/registration.py calls it -> (sums (K,3), target sums (2,)) on
    the CPU.  The outputs start as sentinels: the entry point zeroes what it accumulates into."""
    from nesvor_amd import _lib

    mats = c["mats"].to(device).contiguous()
    K = mats.shape[0] if K is None else K
    M = c["points"].shape[0]
    src, points, target = c["src"].to(device), c["points"].to(device), c["target"].to(device)
    D, H, W = src.shape
    sums = torch.full((K, 3), -7.0, dtype=torch.float64, device=device)
    ts = torch.full((2,), -7.0, dtype=torch.float64, device=device)
    err = _lib.load().nesvor_vvr_similarity(_lib.ptr(src), D, H, W, _lib.ptr(points), _lib.ptr(target), _lib.ptr(mats),
                                            (ctypes.c_float * 3)(*c["unit"]), M, K, _lib.ptr(sums), _lib.ptr(ts), _lib.stream_ptr())
    assert err == 0
    torch.cuda.synchronize()
    return sums.cpu(), ts.cpu()


def _assert_sums(got, tgot, ref, M, coord_tol, what):
    """|kernel - reference| <= accumulation bound + coord_tol x sum |terms| for every sum; prints the worst ratio."""
    sums, tsums, mags, tmags = ref
    K = got.shape[0]
    b, tb = R.accumulation_bound(M, mags[:K], tmags)
    b = b + coord_tol * mags[:K]
    err = (got - sums[:K]).abs()
    worst = float((err / b.clamp(min=1e-300)).max())
    print(f"{what}: K = {K}, M = {M}, T = {R.per_thread(M)}: worst |kernel - fp64| / bound {worst:.3f}")
    assert bool((err <= b).all()), (what, worst)
    if tgot is not None:
        assert bool(((tgot - tsums).abs() <= tb).all()), (what, tgot, tsums)


# ---------------------------------------------------------------------------------------------------------------------
# lattice and generic cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", LATTICE_KS)
def test_lattice_sums_within_the_accumulation_bound(device, K):
    """Exact coordinates (asserted: the fp32 and fp64 references agree bit for bit), so only the derived bound of
    tests/vvr_reference.py stands between kernel and reference: M = 41 x 21 x 21 = 18081 points, 71 workgroups, T = 1, so
    c = 77 (sum I, sum I J), 90 (sum I^2), 64 (target sums) in units of 2^-24 sum |terms|.  The poses leave between 5 % and 70 %
    of the cloud in touch with the volume (asserted on the reference: no case is silently empty or trivial)."""
    c = _lattice()
    assert c["points"].shape[0] == 18081 and R.per_thread(18081) == 1 and _is_lattice(c)
    ones = torch.ones(LATTICE_SHAPE)
    for m in c["mats"]:
        share = float((R.sample(ones, c["points"], m, _unit32(c)) > 0).double().mean())
        assert 0.05 <= share <= 0.70, share
    got, tgot = _launch(device, c, K=K)
    _assert_sums(got, tgot, _reference(c, "lattice"), 18081, 0.0, "lattice")


def test_generic_sums_and_pass_offsets(device):
    """Random points and poses: accumulation bound (M = 70001: 274 workgroups, T = 1) plus the coordinate term COORD_TOL.  Every K
    in GENERIC_KS must also reproduce the first K rows of the K = 27 launch within twice that tolerance (both are within one of
    the reference): a pass that read ``mats + 12 k`` or wrote ``sums + 3 k`` at a wrong offset would be off by whole sums."""
    c = _generic()
    ref = _reference(c, "generic")
    assert R.per_thread(GENERIC_M) == 1
    full, tfull = _launch(device, c, K=GENERIC_POSES)
    _assert_sums(full, tfull, ref, GENERIC_M, COORD_TOL, "generic")
    b, _ = R.accumulation_bound(GENERIC_M, ref[2], ref[3])
    tol = 2 * (b + COORD_TOL * ref[2])
    for K in GENERIC_KS:
        got, tgot = _launch(device, c, K=K)
        _assert_sums(got, tgot, ref, GENERIC_M, COORD_TOL, "generic")
        assert bool(((got - full[:K]).abs() <= tol[:K]).all()), K


# ---------------------------------------------------------------------------------------------------------------------
# point counts
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", M_EDGES)
def test_point_count_edges_on_the_lattice(device, M):
    """The first M points of a fixed shuffle of the lattice cloud under 14 lattice poses (the nine and the first five again: one
    13-pose pass and one single pass), coordinates exact: the derived bound alone, T = 1."""
    base = _lattice()
    key = ("edges", M)
    if key not in _DATA:
        perm = torch.randperm(base["points"].shape[0], generator=torch.Generator().manual_seed(13))[:M]
        c = dict(base, points=base["points"][perm].contiguous(), target=base["target"][perm].contiguous(),
                 mats=torch.cat([base["mats"], base["mats"][:5]]))
        _DATA[key] = c
    c = _DATA[key]
    assert _is_lattice(c)
    got, tgot = _launch(device, c)
    _assert_sums(got, tgot, _reference(c, key), M, 0.0, "edge")


@pytest.mark.parametrize("K", [1, 13])
def test_grid_stride_trip(device, K):
    """M = 2048 x 256 + 257 random points in the generic source: the grid is capped at 2048 workgroups and T = 2.  Generic
    tolerance (the points and poses are drawn like the generic case's)."""
    base = _generic()
    if "stride" not in _DATA:
        g = torch.Generator().manual_seed(14)
        D, H, W = GENERIC_SHAPE
        half = torch.tensor([(W - 1) / 2.0, (H - 1) / 2.0, (D - 1) / 2.0])
        points = ((torch.rand(M_STRIDE, 3, generator=g) * 2 - 1) * 1.5 * half).contiguous()
        _DATA["stride"] = dict(base, points=points, target=torch.rand(M_STRIDE, generator=g), mats=base["mats"][:13].contiguous())
    c = _DATA["stride"]
    assert R.per_thread(M_STRIDE) == 2
    got, tgot = _launch(device, c, K=K)
    _assert_sums(got, tgot, _reference(c, "stride"), M_STRIDE, COORD_TOL, "grid stride")


# ---------------------------------------------------------------------------------------------------------------------
# volumes and clouds
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", THIN_SHAPES)
def test_thin_volumes(device, shape):
    """(1,1,1) - which the Python level never builds (its to_unit divides by size - 1) -, one slice and the smallest volume with
    an interior, through the C entry: an axis of one voxel has half-extent 0, so every finite coordinate lands on index 0 with
    weight 1, as F.grid_sample(align_corners=True) does.  Dyadic to_unit and points, identity and one translated pose: exact
    coordinates (asserted), the derived bound alone."""
    key = ("thin", shape)
    if key not in _DATA:
        g = torch.Generator().manual_seed(15 + shape[2])
        ax = torch.arange(-3.0, 3.0 + 1e-6, 0.25)
        z, y, x = torch.meshgrid(ax[::4], ax[::2], ax, indexing="ij")
        points = torch.stack([x, y, z], -1).reshape(-1, 3).contiguous()
        eye = torch.eye(3)
        mats = torch.stack([torch.cat([eye, torch.zeros(3, 1)], 1), torch.cat([eye, torch.tensor([[0.25], [-1.5], [2.0]])], 1)])
        _DATA[key] = dict(src=torch.rand(shape, generator=g) + 0.5, points=points, target=torch.rand(points.shape[0], generator=g),
                          mats=mats, unit=(0.25, 0.5, 1.0))
    c = _DATA[key]
    assert _is_lattice(c)
    ref = _reference(c, key)
    assert bool((ref[0][:, 0] > 0).all())
    if shape == (1, 1, 1):  # every point samples the one voxel
        assert float(ref[0][0, 0]) == pytest.approx(c["points"].shape[0] * float(c["src"][0, 0, 0].double()), rel=1e-14)
    got, tgot = _launch(device, c)
    _assert_sums(got, tgot, ref, c["points"].shape[0], 0.0, f"volume {shape}")


def test_cloud_wholly_outside(device):
    """Poses that move the cloud 10^6 mm away give exactly 0 for their three sums - inside a 13-pose pass (row 5) and as a
    single pass (row 13) - and their neighbours in the same launch are unaffected."""
    base = _lattice()
    if "outside" not in _DATA:
        mats = torch.cat([base["mats"], base["mats"][:5]]).clone()
        mats[5, :, 3] = torch.tensor([1e6, 0.0, 0.0])
        mats[13, :, 3] = torch.tensor([0.0, -1e6, 1e6])
        _DATA["outside"] = dict(base, mats=mats)
    c = _DATA["outside"]
    ref = _reference(c, "outside")
    assert bool((ref[0][[5, 13]] == 0).all()) and bool((ref[0][[4, 6, 12], 0] > 0).all())
    got, tgot = _launch(device, c)
    assert bool((got[[5, 13]] == 0).all())
    # (rows 5 and 13 aside, the coordinates are the lattice's)
    _assert_sums(got, tgot, ref, c["points"].shape[0], 0.0, "outside")


# ---------------------------------------------------------------------------------------------------------------------
# target sums
# ---------------------------------------------------------------------------------------------------------------------
def test_target_sums_handover(device):
    """With a buffer: {sum J, sum J^2} within the derived bound (c = T + 63 = 64), for K = 1, 13 and 27 alike - only the first
    pass adds to it (a second pass adding too would double it).  With a null pointer the call succeeds, computes the same pose
    sums, and writes nothing beyond them: the (K,3) sums sit inside a sentinel-filled buffer."""
    from nesvor_amd import _lib

    c = _generic()
    ref = _reference(c, "generic")
    _, tb = R.accumulation_bound(GENERIC_M, ref[2], ref[3])
    for K in (1, 13, 27):
        _, tgot = _launch(device, c, K=K)
        assert bool(((tgot - ref[1]).abs() <= tb).all()), (K, tgot, ref[1])
    K = 14
    with_t, _ = _launch(device, c, K=K)
    buf = torch.full((3 * K + 64,), -7.0, dtype=torch.float64, device=device)
    src, points, target, mats = (c[k].to(device) for k in ("src", "points", "target", "mats"))
    D, H, W = src.shape
    err = _lib.load().nesvor_vvr_similarity(_lib.ptr(src), D, H, W, _lib.ptr(points), _lib.ptr(target), _lib.ptr(mats),
                                            (ctypes.c_float * 3)(*c["unit"]), GENERIC_M, K, _lib.ptr(buf), None, _lib.stream_ptr())
    assert err == 0
    torch.cuda.synchronize()
    assert bool((buf[3 * K:] == -7.0).all())
    without = buf[:3 * K].view(K, 3).cpu()
    _assert_sums(without, None, ref, GENERIC_M, COORD_TOL, "null target_sums")
    b, _ = R.accumulation_bound(GENERIC_M, ref[2], ref[3])
    assert bool(((without - with_t).abs() <= 2 * (b + COORD_TOL * ref[2])[:K]).all())


# ---------------------------------------------------------------------------------------------------------------------
# the loss VVR forms from the sums
# ---------------------------------------------------------------------------------------------------------------------
def _loss64(kind, sums, tsums, M, eps=1e-6):
    sI, sII, sIJ = sums[..., 0] / M, sums[..., 1] / M, sums[..., 2] / M
    sJ, sJJ = tsums[0] / M, tsums[1] / M
    if kind == "mse":
        return sII - 2 * sIJ + sJJ
    cross = sIJ - sI * sJ
    return -(cross * cross) / ((sII - sI * sI) * (sJJ - sJ * sJ) + eps)


def _level(c, device, target=None):
    """What VVR._objective_fused reads of a pyramid level, for a case of this module."""
    return types.SimpleNamespace(source=c["src"].to(device)[None, None], points=c["points"].to(device),
                                 values=(c["target"] if target is None else target).to(device),
                                 to_unit_host=(ctypes.c_float * 3)(*c["unit"]), target_sums=None)


@pytest.mark.parametrize("kind", ["ncc", "mse"])
def test_loss_of_the_fused_objective(device, kind):
    """``VVR._objective_fused`` on the generic source and cloud, the target being the source's samples at one pose plus noise:
    the 13 poses of a gradient (first call on the level: fills the level's target sums), then a K = 1 call that reuses them.
    Reference: the fp64 formula on the reference sums of the very matrices the method built.  Tolerance: the loss is a smooth
    function of the five sums, so to first order  |d loss| <= sum_i |d loss / d s_i| b_i  with b_i the sums' tolerance
    (accumulation bound + COORD_TOL) and the derivatives taken by autograd in fp64 at the reference sums, 1 % for the higher
    orders, plus the result's rounding to fp32 (2^-24 |loss|)."""
    from nesvor_amd.registration import VVR
    from nesvor_amd.transform import RigidTransform

    c = dict(_generic())
    g = torch.Generator().manual_seed(16)
    c["target"] = (R.sample(c["src"], c["points"], c["mats"][0], _unit32(c)) + 0.1 * torch.rand(GENERIC_M, generator=g).double()).float()
    vvr = VVR(num_levels=1, num_steps=1, step_size=1, max_iter=1, optimizer={"name": "gd"},
              loss={"name": "ncc", "win": None} if kind == "ncc" else {"name": "mse"}, auto_grad=False)
    assert vvr._fused_kind == kind
    vvr.trans_first = True
    vvr.theta_t = RigidTransform(torch.tensor([[0.1, -0.05, 0.08, 1.0, -0.5, 0.25]], device=device))
    thetas = (torch.randn(13, 6, generator=g) * torch.tensor([6.0, 6.0, 6.0, 2.0, 2.0, 2.0])).to(device)  # degrees, mm
    lv = _level(c, device)
    unit = vvr._unit(thetas)
    for rows in (slice(0, 13), slice(3, 4)):
        first = lv.target_sums is None
        got = vvr._objective_fused(thetas[rows], lv).double().cpu()
        assert first == (rows.stop == 13) and lv.target_sums is not None
        mats = RigidTransform(thetas[rows] * unit, trans_first=True).inv().compose(vvr.theta_t).matrix().cpu()
        sums, tsums, mags, tmags = R.vvr_sums(c["src"], c["points"], c["target"], mats, _unit32(c), torch.float64, with_abs=True)
        b, tb = R.accumulation_bound(GENERIC_M, mags, tmags)
        b = b + COORD_TOL * mags
        s, t = sums.clone().requires_grad_(True), tsums.clone().requires_grad_(True)
        ref = _loss64(kind, s, t, GENERIC_M)
        tol = torch.zeros_like(ref)
        for k in range(ref.shape[0]):
            gs, gt = torch.autograd.grad(ref[k], (s, t), retain_graph=True)
            tol[k] = 1.01 * ((gs[k].abs() * b[k]).sum() + (gt.abs() * tb).sum()) + R.U * ref[k].detach().abs()
        err = (got - ref.detach()).abs()
        print(f"{kind}, K = {ref.shape[0]}: loss {float(ref[0].detach()):.6f}, worst |fused - fp64| / tolerance {float((err / tol).max()):.3f}, "
              f"tolerance / |loss| {float((tol / ref.detach().abs()).max()):.2e}")
        assert bool((err <= tol).all())


def test_mse_noise_floor_at_the_exact_pose(device):
    """Self-registration on the lattice case: the target is the source's samples at the pose under test (fp64 samples rounded
    to fp32), so the true MSE is that rounding alone (<= 2^-48 / 4 mean J^2) and what the fused MSE returns is the noise of its
    three sums:  |MSE| <= (b_II + 2 b_IJ + b_JJ) / M  with the derived bounds, c = 90, 77 and 64 (T = 1) on sum I^2, sum |I J| and
    sum J^2 - about (90 + 2 x 77 + 64) 2^-24 = 1.8e-5 of mean(J^2).  This is the floor under which the descent's
    ``trial < loss`` test compares rounding, not images.  The pose (zero rotation, dyadic translations) keeps the coordinates
    exact: asserted on the matrices the method built."""
    from nesvor_amd.registration import VVR
    from nesvor_amd.transform import RigidTransform

    c = dict(_lattice())
    M = c["points"].shape[0]
    vvr = VVR(num_levels=1, num_steps=1, step_size=1, max_iter=1, optimizer={"name": "gd"}, loss={"name": "mse"}, auto_grad=False)
    vvr.trans_first = True
    vvr.theta_t = RigidTransform(torch.tensor([[0.0, 0.0, 0.0, 0.25, -1.5, 2.0]], device=device))
    theta = torch.tensor([[0.0, 0.0, 0.0, -0.5, 0.25, 1.0]], device=device)
    mats = RigidTransform(theta * vvr._unit(theta), trans_first=True).inv().compose(vvr.theta_t).matrix().cpu()
    expect = torch.cat([torch.eye(3), torch.tensor([[0.75], [-1.75], [1.0]])], 1)[None]
    assert torch.equal(mats, expect)
    c["mats"] = mats
    c["target"] = R.sample(c["src"], c["points"], mats[0], _unit32(c)).float()
    assert _is_lattice(c)
    sums, tsums, mags, tmags = R.vvr_sums(c["src"], c["points"], c["target"], mats, _unit32(c), torch.float64, with_abs=True)
    true = float(_loss64("mse", sums, tsums, M)[0])
    mean_jj = float(tsums[1]) / M
    assert 0 <= true <= 2.0 ** -48 / 4 * mean_jj * 1.01 and mean_jj > 0.01
    b, tb = R.accumulation_bound(M, mags, tmags)
    floor = float(b[0, 1] + 2 * b[0, 2] + tb[1]) / M
    got = float(vvr._objective_fused(theta, _level(c, device))[0])
    print(f"exact pose: fused MSE {got:.3e}, true {true:.3e}, floor {floor:.3e} = {floor / mean_jj:.2e} mean(J^2)")
    assert abs(got) <= floor + true + R.U * floor  # (the result is rounded to fp32)
    assert floor <= 2e-5 * mean_jj
