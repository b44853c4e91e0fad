"""CPU: the product's HOST logic (no native compute) against fixtures captured from the
reference's Python.  The native transform ops are stood in by the oracle (fixture
`oracle_backend`) — the product itself has no CPU path."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, scipy_table, small_args


def _t(a):
    return torch.tensor(a)


def test_phantom_bit_exact(golden):
    from nesvor_amd.phantom import phantom3d

    for n in (32, 64):
        sha = hashlib.sha1(phantom3d(n=n).astype(np.float32).tobytes()).digest()
        assert np.frombuffer(sha, dtype=np.uint8).tolist() == golden[f"phantom_sha1_{n}"].tolist()


def test_psf_and_utils(golden):
    from nesvor_amd.utils import gaussian_blur, get_PSF, meshgrid, resolution2sigma

    psf = get_PSF(res_ratio=(1.5, 1.5, 3.0))
    assert tuple(psf.shape) == (9, 5, 5) and int((psf > 0).sum()) == 153
    np.testing.assert_array_equal(psf.numpy(), golden["psf_15_15_3"])
    np.testing.assert_array_equal(get_PSF(res_ratio=(1.0, 1.0, 1.0)).numpy(), golden["psf_1_1_1"])
    np.testing.assert_array_equal(
        resolution2sigma(torch.tensor([[1.5, 1.5, 3.0], [0.8, 0.8, 0.8]])).numpy(), golden["sigma_aniso"])
    assert resolution2sigma(0.8, isotropic=True) == float(golden["sigma_iso"])
    np.testing.assert_array_equal(gaussian_blur(_t(golden["blur_in"]), 1.5, 3).numpy(), golden["blur_out"])
    np.testing.assert_array_equal(meshgrid((4, 3, 2), (1.5, 1.5, 3.0)).numpy(), golden["meshgrid"])


def test_rigid_transform_algebra(golden, oracle_backend):
    from nesvor_amd.transform import (RigidTransform, euler2mat, mat2euler, mat2point, mat_update_resolution,
                                      point2mat, transform_points)

    ax = _t(golden["tf_ax"])
    A = RigidTransform(ax, trans_first=True)
    B = RigidTransform(ax.flip(0).clone(), trans_first=False)
    close = lambda a, k: np.testing.assert_allclose(a.numpy(), golden[k], rtol=1e-6, atol=1e-6, err_msg=k)
    close(A.matrix(True), "tf_mat_first")
    close(A.matrix(False), "tf_mat_last")
    close(A.axisangle(False), "tf_ax_last")
    close(A.inv().matrix(True), "tf_inv")
    close(A.compose(B).matrix(True), "tf_compose")
    close(B.axisangle(True), "tf_B_first_ax")
    close(transform_points(A, _t(golden["tf_pts"])), "tf_pts_out")
    close(mat2euler(A.matrix(True)), "tf_euler")
    close(euler2mat(mat2euler(A.matrix(True))), "tf_euler2mat")
    close(mat2point(A.matrix(True), 128, 96, 0.8), "tf_mat2point")
    close(point2mat(mat2point(A.matrix(True), 128, 96, 0.8)), "tf_point2mat")
    close(mat_update_resolution(A.matrix(True), 1.0, 0.8), "tf_update_res")
    assert len(A[2:5]) == 3 and len(A[3]) == 1 and len(RigidTransform.cat([A, B])) == 22


def test_compose_inv_reference_test(oracle_backend):
    """tests/transform/test_transform.py:7-23, verbatim in structure (mixed trans_first)."""
    from nesvor_amd.transform import RigidTransform

    ax, mat = scipy_table()
    zeros = torch.zeros(1, 6)
    n = len(ax)
    for i in range(n):
        ax_a, mat_a = ax[i : i + 1], mat[i : i + 1]
        ax_b, mat_b = ax[n - 1 - i : n - i], mat[n - 1 - i : n - i]
        ab = RigidTransform(ax_a, trans_first=i % 2 == 0).compose(RigidTransform(mat_b, trans_first=i % 2 == 1))
        inv_b_inv_a = RigidTransform(ax_b, trans_first=i % 2 == 1).inv().compose(
            RigidTransform(mat_a, trans_first=i % 2 == 0).inv())
        err = ab.compose(inv_b_inv_a).axisangle()
        # reference tolerance on the rotation; the translations of this table reach 300 mm, where one
        # fp32 ulp of an intermediate is 3.05e-5 (CPU matmul rounding differs from the GPU's FMA order)
        torch.testing.assert_close(err[:, :3], zeros[:, :3], atol=2e-5, rtol=1e-3)
        torch.testing.assert_close(err[:, 3:], zeros[:, 3:], atol=1e-4, rtol=1e-3)


def test_roundtrips_reference_tests():
    """tests/transform/test_transform_convert.py:23-33 (pure-PyTorch helpers)."""
    from nesvor_amd.transform import euler2mat, mat2euler, mat2point, point2mat

    _, mat = scipy_table()
    for i in range(len(mat)):
        m = mat[i : i + 1]
        torch.testing.assert_close(point2mat(mat2point(m, 128 + 2 * i, 128 + 4 * i, 0.5 + 0.1 * i)), m)
        torch.testing.assert_close(euler2mat(mat2euler(m)), m)


def _golden_slices(golden):
    from nesvor_amd.image import Slice
    from nesvor_amd.transform import RigidTransform

    vs, res, res_s, s_thick, gap, n_slice, ss = golden["sim_geom"]
    imgs = _t(golden["sim_stacks"])
    tf = RigidTransform(_t(golden["sim_transforms"]), trans_first=True)
    return [Slice(imgs[k], imgs[k] > 0, tf[k], float(res_s), float(res_s), float(s_thick)) for k in range(imgs.shape[0])]


def test_dataset_fields_bbox_mean_mask(golden, oracle_backend):
    from nesvor_amd.train import Dataset

    args = small_args()
    ds = Dataset(_golden_slices(golden), args)
    np.testing.assert_array_equal(ds.xyz.numpy(), golden["ds_xyz"])
    np.testing.assert_array_equal(ds.v.numpy(), golden["ds_v"])
    np.testing.assert_array_equal(ds.slice_idx.numpy(), golden["ds_slice_idx"])
    np.testing.assert_allclose(ds.transformation.matrix().numpy(), golden["ds_transformation"], atol=1e-6)
    np.testing.assert_array_equal(ds.resolution.numpy(), golden["ds_resolution"])
    np.testing.assert_allclose(ds.bounding_box.numpy(), golden["ds_bounding_box"], rtol=1e-6, atol=1e-5)
    assert abs(ds.mean - float(golden["ds_mean"])) < 1e-6
    m = ds.mask
    np.testing.assert_array_equal(m.mask.numpy(), golden["ds_mask"])
    np.testing.assert_allclose(m.transformation.matrix().numpy(), golden["ds_mask_tf"], rtol=1e-6, atol=1e-5)
    assert abs(float(m.resolution_x) - float(golden["ds_mask_res"])) < 1e-7
    # first get_batch shuffles (count starts at len) and the epoch counter becomes 1
    torch.manual_seed(0)
    ds2 = Dataset(_golden_slices(golden), args)
    b = ds2.get_batch(64, "cpu")
    np.testing.assert_array_equal(b["xyz"].numpy(), golden["ds_batch_xyz"])
    np.testing.assert_array_equal(b["slice_idx"].numpy(), golden["ds_batch_idx"])
    assert [ds2.epoch, ds2.count] == golden["ds_epoch_count"].tolist()


def test_dataset_partial_batch_dropped(golden, oracle_backend):
    from nesvor_amd.train import Dataset

    ds = Dataset(_golden_slices(golden)[:4], small_args())
    M = ds.v.shape[0]
    bs = M // 2 + 1  # two batches do not fit -> second call must reshuffle, never return a short batch
    a = ds.get_batch(bs, "cpu")
    b = ds.get_batch(bs, "cpu")
    assert a["v"].shape[0] == bs and b["v"].shape[0] == bs and ds.epoch == 2


def test_grid_spec_and_inr_hyperparameters(golden):
    from nesvor_amd.grid import HashGridSpec
    from nesvor_amd.models import grid_hyperparameters
    from oracle import hashgrid as hg

    for ext, scale, n_levels, base in golden["inr_levels_table"]:
        a = small_args(level_scale=float(scale), finest_resolution=0.5)
        bb = torch.tensor([[0.0, 0, 0], [ext, ext * 0.8, ext * 0.5]])
        assert grid_hyperparameters(bb, a) == (int(base), int(n_levels))
    # defaults give L=12; --level-scale 1.26 gives L=16 for a 130 mm box
    bb = torch.tensor([[0.0, 0, 0], [130.0, 130, 130]])
    assert grid_hyperparameters(bb, small_args(finest_resolution=0.5))[1] == 12
    assert grid_hyperparameters(bb, small_args(finest_resolution=0.5, level_scale=1.26)) == (9, 16)
    spec = HashGridSpec(16, 2, 19, 9, 1.26)
    ref = hg.make_levels(16, 19, 9, 1.26)
    assert spec.n_params == 7854240 == hg.n_params(ref, 2)
    for a_, b_ in zip(spec.levels, ref):
        assert (a_.res, a_.size, a_.offset, a_.hashed) == (b_.res, b_.size, b_.offset, b_.hashed)
        assert np.float32(a_.scale) == np.float32(b_.scale)


def test_hashgrid_plan_limits_on_the_tested_grids():
    """The grids of tests/test_gpu_hashgrid_grids.py sit where their table says - chunks per level and buckets (chunks over all
    levels) under the plan's chunking rule - and the size query of the owner method (host code: the library loads without a GPU)
    draws the line there: 256 chunks per level and 3968 of 4064 buckets are inside, 512 chunks and 4096 buckets are not."""
    import ctypes

    import hashgrid_reference as R
    from nesvor_amd import _lib
    from nesvor_amd.grid import HashGridSpec

    lib = _lib.load()
    for name, (spec_tuple, most, buckets, inside) in R.GRIDS.items():
        assert R.chunk_counts(spec_tuple) == (most, buckets), name
        assert inside == (most <= R.MAX_CHUNKS and buckets <= R.MAX_BUCKETS), name
        spec = HashGridSpec(*spec_tuple)
        for N in (1000, 1024):
            nbytes = lib.nesvor_hashgrid_backward_workspace_bytes(ctypes.byref(spec.c_struct), N, None)
            assert (nbytes > 0) if inside else (nbytes == -1), (name, nbytes)
            for layout in (0, 1, 1 | _lib.LAYOUT_UNCLUSTERED | _lib.LAYOUT_DY_SCRATCH):
                ex = lib.nesvor_hashgrid_backward_workspace_bytes_ex(ctypes.byref(spec.c_struct), N, None, layout)
                assert (0 < ex <= nbytes + 256 + 1024 * 4 * spec.n_output_dims) if inside else (ex == -1), (name, layout, ex)
            assert (lib.nesvor_hashgrid_backward_order_offset(ctypes.byref(spec.c_struct), N, None) > 0) == inside, name
    for name in ("near_bucket_limit", "T20_256chunks"):
        assert R.GRIDS[name][3]
    for name in ("T21_512chunks", "many_buckets"):
        assert not R.GRIDS[name][3]
    # the re-ordered copy of a feature-major dpe exists only where its rows fit the copy kernel's LDS: E = 256 never does,
    # E = 24 does whatever the device (without one the query assumes 64 KiB)
    wide, narrow = HashGridSpec(*R.GRIDS["L32_F8"][0]), HashGridSpec(*R.GRIDS["cli_130mm"][0])
    hinted = 1 | _lib.LAYOUT_UNCLUSTERED | _lib.LAYOUT_DY_SCRATCH
    q = lambda s, lay: lib.nesvor_hashgrid_backward_workspace_bytes_ex(ctypes.byref(s.c_struct), 1000, None, lay)
    assert q(wide, hinted) == q(wide, 1 | _lib.LAYOUT_UNCLUSTERED)
    assert q(narrow, hinted) == q(narrow, 1 | _lib.LAYOUT_UNCLUSTERED) + 256 + 1024 * 4 * narrow.n_output_dims
    fq = lambda s, lay: lib.nesvor_hashgrid_forward_workspace_bytes(ctypes.byref(s.c_struct), 1000, lay | _lib.LAYOUT_UNCLUSTERED)
    assert fq(wide, 1) == -1 and fq(wide, 0) > 0 and fq(narrow, 1) > fq(narrow, 0) > 0


def _hg_sort_bytes(N):
    """csrc/hashgrid.hip's sort_bytes(N) from its sort_plan rule: 2^b cells per axis with b = (floor(log2 N) - 5) / 3 clamped to
    [1, 6], strips of twice the mean occupancy rounded up to a power of two (at least 2) - the formula of
    tests/test_cabi.py::test_backward_workspace_size_queries_follow_the_layout_hints for any N."""
    n_pad = (N + 255) // 256 * 256
    b = min(max((N.bit_length() - 1 - 5) // 3, 1), 6)
    n_cells = 1 << (3 * b)
    mean, cap = -(-N // n_cells), 2
    while cap < 2 * mean:
        cap *= 2
    return (n_pad * 2 + 2 * ((1 << 18) + 2)) * 4 + n_pad * 8 + n_cells * cap * 4


def test_hashgrid_workspace_layout_identities():
    """What the size and offset queries of the hash-grid launches say about one workspace, as identities between them (host code:
    no GPU), on every tested grid inside the plan's limits, at point counts around the 256-point padding, with and without
    queue scales: two zero-filled tail regions and the tickets | records of 4 (1 + F) bytes | cloud order (n_pad) | 256 bytes of
    alignment slack | the point order's scratch (whole 256s) | optionally dpe as rows."""
    import ctypes

    import hashgrid_reference as R
    from nesvor_amd import _lib
    from nesvor_amd.grid import HashGridSpec

    lib = _lib.load()
    U, S = _lib.LAYOUT_UNCLUSTERED, _lib.LAYOUT_DY_SCRATCH
    zero = lib.nesvor_hashgrid_backward_workspace_zero_bytes()
    assert zero == (2 * 8 + 1) * 4096 * 4  # two regions of 8 sub-queue counter sets, one set of tickets
    assert lib.nesvor_hashgrid_backward_overflow_offset(ctypes.c_void_p(0x7000)) == (4096 - 32) * 4  # (a workspace not seen before)
    assert lib.nesvor_hashgrid_cloud_order_bytes(0) == 0
    checked = 0
    for name, (spec_tuple, _, _, inside) in R.GRIDS.items():
        if not inside:
            continue
        spec = HashGridSpec(*spec_tuple)
        g, L, F = ctypes.byref(spec.c_struct), spec.n_levels, spec.n_features
        E = L * F
        for N in (1, 255, 256, 257, 1000, (1 << 20) - 77):
            n_pad = (N + 255) // 256 * 256
            sort = (_hg_sort_bytes(N) + 255) // 256 * 256
            # the rows -> columns kernels' LDS decides whether the re-ordered copies exist; the forward's query says so
            fwd_fm = lib.nesvor_hashgrid_forward_workspace_bytes(g, N, 1 | U)
            fits = fwd_fm != -1
            assert fits or E > 62, (name, N)  # 256 rows of E + 1 floats + 1 KiB <= 64 KiB, what every device has
            assert not fits or E < 159, (name, N)
            for scale in (None, (ctypes.c_float * L)(*([1.0 / 16] * L))):
                tag = (name, N, scale is not None)
                base = lib.nesvor_hashgrid_backward_workspace_bytes(g, N, scale)
                order = lib.nesvor_hashgrid_backward_order_offset(g, N, scale)
                assert base > 0 and order > zero, tag
                assert base - order == n_pad + 256 + sort, tag
                assert (order - zero) % (4 * (1 + F)) == 0, tag
                for lay in (0, 1):
                    for u in (0, U):
                        for s in (0, S):
                            want = base - (0 if u else sort) + (256 + n_pad * E * 4 if (lay == 1 and u and s and fits) else 0)
                            assert lib.nesvor_hashgrid_backward_workspace_bytes_ex(g, N, scale, lay | u | s) == want, tag + (lay, u, s)
                checked += 1
            assert lib.nesvor_hashgrid_cloud_order_bytes(N) == n_pad
            plan_words = 8 + 14 * ((L + 4) & ~3)
            assert lib.nesvor_hashgrid_cloud_plan_bytes(g, N) == (n_pad // 256 * plan_words * 4 if F <= 2 else 0), (name, N)
            for hint in (0, _lib.LAYOUT_CLUSTERED, S):
                assert lib.nesvor_hashgrid_forward_workspace_bytes(g, N, hint) == lib.nesvor_hashgrid_forward_workspace_bytes(g, N, 1 | hint) == 0
            assert lib.nesvor_hashgrid_forward_workspace_bytes(g, N, 0 | U) == 256 + sort, (name, N)
            assert fwd_fm == (256 + sort + n_pad * E * 4 if fits else -1), (name, N)
        assert lib.nesvor_hashgrid_forward_workspace_bytes(g, 0, 1 | U) == 0 == lib.nesvor_hashgrid_backward_workspace_bytes(g, 0, None)
        assert lib.nesvor_hashgrid_backward_workspace_bytes_ex(g, 0, None, 1 | U | S) == 0
        assert lib.nesvor_hashgrid_backward_order_offset(g, 0, None) == -1
    assert checked == 2 * 6 * sum(1 for v in R.GRIDS.values() if v[3])


def test_hashgrid_entry_points_refuse_before_any_launch():
    """The refusal rules of the hash-grid entry points, row by row (ctypes calls that return before anything is launched: the
    grid is real, the other pointers are dummies).  An empty batch is a no-op - except for the backward with the AdamW step,
    which refuses it; every other row is hipErrorInvalidValue."""
    import ctypes

    from nesvor_amd import _lib
    from nesvor_amd.grid import HashGridSpec

    lib = _lib.load()
    INVALID, P, Q, NULL = 1, ctypes.c_void_p(0x1000), ctypes.c_void_p(0x1008), ctypes.c_void_p(0)  # (Q: not 16-byte aligned)
    AGG, OWN, KEEP, ACC = _lib.HG_STAGE_AGGREGATE, _lib.HG_STAGE_OWNER, _lib.HG_STAGE_KEEP, _lib.HG_STAGE_ACCUMULATE_U
    BOTH = AGG | OWN
    U = _lib.LAYOUT_UNCLUSTERED
    spec = HashGridSpec(6, 2, 10, 4, 1.5)
    L = spec.n_levels
    adam = _lib.AdamwT()

    def grid(**kw):
        c = type(spec.c_struct)()
        ctypes.memmove(ctypes.byref(c), ctypes.byref(spec.c_struct), ctypes.sizeof(c))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    # every entry point as f(grid struct, **overrides) over one set of named defaults
    base = dict(N=1000, layout=0, ws=P, stages=BOTH, l0=0, l1=L, dy_bound=NULL, order=NULL, plan=NULL, fwd_order=P, table=P, gt=P,
                m=P, v=P, adam=ctypes.byref(adam))

    def entry(fn):
        def call(g, **kw):
            a = dict(base, **kw)
            return fn(ctypes.byref(g), a)
        return call

    E = {
        "backward": entry(lambda g, a: lib.nesvor_hashgrid_backward(g, P, P, P, P, P, a["N"], a["layout"], a["ws"], a["stages"], None, NULL)),
        "levels": entry(lambda g, a: lib.nesvor_hashgrid_backward_levels(g, P, P, P, P, P, a["N"], a["layout"], a["ws"], a["stages"],
                                                                          a["l0"], a["l1"], None, NULL)),
        "bounded": entry(lambda g, a: lib.nesvor_hashgrid_backward_bounded(g, P, P, P, P, P, a["N"], a["layout"], a["ws"], a["stages"],
                                                                            a["l0"], a["l1"], None, a["dy_bound"], NULL)),
        "plan": entry(lambda g, a: lib.nesvor_hashgrid_backward_plan(g, P, P, P, P, P, a["N"], a["layout"], a["ws"], a["stages"],
                                                                      a["l0"], a["l1"], None, a["dy_bound"], a["order"], a["plan"], NULL)),
        "adamw": entry(lambda g, a: lib.nesvor_hashgrid_backward_adamw(g, P, a["table"], P, a["gt"], P, a["N"], a["layout"], a["ws"],
                                                                        a["stages"], None, a["dy_bound"], a["m"], a["v"], a["adam"], NULL)),
        "atomic": entry(lambda g, a: lib.nesvor_hashgrid_backward_atomic(g, P, P, P, P, P, a["N"], a["layout"], NULL)),
        "forward": entry(lambda g, a: lib.nesvor_hashgrid_forward(g, P, P, P, a["N"], a["layout"], NULL)),
        "forward_bounded": entry(lambda g, a: lib.nesvor_hashgrid_forward_bounded(g, P, P, P, a["N"], a["layout"], NULL, NULL)),
        "forward_unclustered": entry(lambda g, a: lib.nesvor_hashgrid_forward_unclustered(g, P, P, P, a["N"], a["layout"] | U, NULL, a["ws"],
                                                                                          1 << 40, NULL)),
        "forward_plan": entry(lambda g, a: lib.nesvor_hashgrid_forward_plan(g, P, P, P, a["N"], a["layout"], NULL,
                                                                            a["fwd_order"], a["plan"], None, NULL)),
    }
    owner, ranged = ("backward", "levels", "bounded", "plan"), ("levels", "bounded", "plan")
    rows = []  # (entry, grid overrides, argument overrides, expected)
    for e in E:
        rows.append((e, {}, dict(N=0), INVALID if e == "adamw" else 0))
        rows += [(e, dict(n_levels=0), {}, INVALID), (e, dict(n_levels=33), {}, INVALID), (e, dict(n_features=3), {}, INVALID),
                 (e, {}, dict(layout=2), INVALID)]
    for e in owner + ("adamw", "forward_unclustered"):
        rows.append((e, {}, dict(ws=NULL), INVALID))
    for e in owner + ("adamw",):
        rows += [(e, {}, dict(stages=0), INVALID), (e, {}, dict(stages=KEEP | ACC), INVALID)]
    for e in ranged:
        rows += [(e, {}, dict(l0=-1), INVALID), (e, {}, dict(l1=L + 1), INVALID), (e, {}, dict(l0=3, l1=3), INVALID),
                 (e, {}, dict(l0=4, l1=2), INVALID)]
    rows += [("plan", {}, dict(order=P, plan=Q), INVALID), ("forward_plan", {}, dict(plan=Q), INVALID)]
    rows.append(("forward_plan", {}, dict(fwd_order=NULL), INVALID))
    rows += [("plan", {}, dict(order=P, layout=U), INVALID), ("plan", {}, dict(order=P, plan=P, layout=U), INVALID),
             ("plan", {}, dict(plan=P, layout=U), INVALID),
             ("plan", {}, dict(plan=P), INVALID),  # a plan without the order
             ("plan", dict(n_features=4), dict(order=P, plan=P), INVALID),
             ("plan", {}, dict(order=P, plan=P, l0=1), INVALID), ("plan", {}, dict(order=P, plan=P, l1=L - 1), INVALID)]
    rows += [("adamw", {}, dict(stages=BOTH | KEEP), INVALID), ("adamw", {}, dict(stages=BOTH | ACC), INVALID),
             ("adamw", {}, dict(stages=AGG | KEEP | ACC), INVALID)]
    rows += [("adamw", {}, {k: NULL}, INVALID) for k in ("table", "gt", "m", "v")] + [("adamw", {}, dict(adam=None), INVALID)]
    for e, gkw, akw, want in rows:
        assert E[e](grid(**gkw), **akw) == want, (e, gkw, {k: getattr(v, "value", v) for k, v in akw.items()})
    assert len(rows) == 10 * 5 + 6 + 10 + 12 + 3 + 7 + 3 + 5


def test_state_dict_layout_matches_reference(golden):
    """INR.state_dict() keys/shapes (checkpoint contract, cli/io.py:24-46) without touching the GPU."""
    from nesvor_amd.models import INR

    args = small_args()
    bb = _t(golden["fw_sd::inr.bounding_box"])
    inr = INR(bb, args)
    ref_keys = [str(k)[4:] for k in golden["fw_state_keys"] if str(k).startswith("inr.")]
    sd = inr.state_dict()
    assert list(sd.keys()) == ref_keys
    for k in ref_keys:
        assert tuple(sd[k].shape) == golden["fw_sd::inr." + k].shape, k


def test_moving_average_semantics():
    from nesvor_amd.utils import MovingAverage

    ema = MovingAverage(0.999)
    for x in (1.0, 2.0, 4.0):
        ema("k", x)
    v = ((1.0 * 0.001) * 0.999 + 2.0 * 0.001) * 0.999 + 4.0 * 0.001
    assert abs(ema["k"] - v / (1 - 0.999**3)) < 1e-12 and ema["missing"] == 0


def test_moving_average_update_all_matches_per_key_calls():
    from nesvor_amd.utils import MovingAverage

    a, b = MovingAverage(0.999), MovingAverage(0.999)
    g = torch.Generator().manual_seed(0)
    for _ in range(5):
        vals = {"x": torch.rand((), generator=g, dtype=torch.float64), "y": torch.rand((), generator=g, dtype=torch.float64)}
        for k, v in vals.items():
            a(k, v)
        b.update_all(vals)
    for k in ("x", "y"):
        assert abs(float(a[k]) - float(b[k])) < 1e-12
    assert a.value[0] == b.value[0] == 5


def test_cg_vs_scipy_reference_test():
    """tests/svort/test_cg.py:9-20 — CG on a 5x5 Hankel system against scipy.sparse.linalg.cg (pure host logic)."""
    import scipy.linalg
    import scipy.sparse.linalg

    from nesvor_amd.srr import CG

    n = 5
    A = scipy.linalg.hankel(np.arange(1, n + 1, dtype=np.float64)) + np.eye(n) * 20  # SPD, as the reference builds it
    b = np.arange(n, dtype=np.float64)
    x_ref, _ = scipy.sparse.linalg.cg(A, b, np.zeros_like(b), maxiter=n, atol=1e-12)
    At = torch.tensor(A)
    x = CG(lambda v: At @ v, torch.tensor(b), torch.zeros(n, dtype=torch.float64), n, 0.0)
    np.testing.assert_allclose(x.numpy(), x_ref, rtol=1e-8, atol=1e-10)
    # started at the exact solution the residual is exactly zero: no NaN (deterministic operators)
    x2 = CG(lambda v: At @ v, At @ torch.tensor(x_ref), torch.tensor(x_ref), 3, 0.0)
    assert torch.isfinite(x2).all()


def test_volume_resample_vs_reference_fixture(golden, oracle_backend):
    """``Volume.resample`` (image/image.py:134-177) as ``sample_volume`` uses it: the reference resampled the mask of
    its trained data set (slices at the optimised poses, ``train_out_tf``) to ``output_resolution`` = 2 mm; lattice
    shape, boolean mask and pose of the result are fixtures (``train_volume*``)."""
    from nesvor_amd.image import Slice
    from nesvor_amd.train import Dataset
    from nesvor_amd.transform import RigidTransform

    vs, res, res_s, s_thick, gap, n_slice, ss = golden["sim_geom"]
    imgs = _t(golden["sim_stacks"])
    tf = RigidTransform(_t(golden["train_out_tf"]), trans_first=True)
    slices = [Slice(imgs[k], imgs[k] > 0, tf[k], float(res_s), float(res_s), float(s_thick)) for k in range(imgs.shape[0])]
    args = small_args()
    out = Dataset(slices, args).mask.resample(args.output_resolution, None)
    assert tuple(out.image.shape) == golden["train_volume"].shape
    np.testing.assert_array_equal(out.mask.numpy(), golden["train_volume_mask"])
    np.testing.assert_allclose(out.transformation.matrix().numpy(), golden["train_volume_tf"], rtol=1e-6, atol=1e-5)
    assert float(out.resolution_x) == float(out.resolution_y) == float(out.resolution_z) == 2.0
    # an explicit target orientation: the lattice is rebuilt in that frame and still covers every masked voxel
    rot = RigidTransform(torch.tensor([[0.3, -0.2, 0.5, 0.0, 0.0, 0.0]]), trans_first=True)
    turned = out.resample(None, rot)
    np.testing.assert_allclose(turned.transformation.matrix()[0, :, :3].numpy(), rot.matrix()[0, :, :3].numpy(), atol=1e-6)
    back = turned.sample_points(out.xyz_masked)
    assert float((back > 0).float().mean()) > 0.95


def test_edge_prior_gradient_is_the_derivative_of_the_charbonnier_penalty():
    """``SRR.dR`` (svort/srr.py:134-160): for every interior voxel a, sum over the 26 neighbours o of
    d/dv_a sqrt(1 + (v_a - v_(a+o))^2 / (|o|^2 delta^2)) with the neighbour held fixed; border voxels get 0.
    Checked against autograd of exactly that expression in fp64."""
    from nesvor_amd.srr import SRR, edge_prior_gradient

    torch.manual_seed(0)
    v = torch.rand(2, 1, 6, 7, 8, dtype=torch.float64)
    delta = 0.3
    g = edge_prior_gradient(v, delta)
    va = v.clone().requires_grad_(True)
    D, H, W = v.shape[-3:]
    energy = 0
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dz, dy, dx) == (0, 0, 0):
                    continue
                w = 1.0 / ((dz * dz + dy * dy + dx * dx) * delta * delta)
                nb = v[..., 1 + dz : D - 1 + dz, 1 + dy : H - 1 + dy, 1 + dx : W - 1 + dx]  # constant
                energy = energy + torch.sqrt(1 + w * (va[..., 1:-1, 1:-1, 1:-1] - nb) ** 2).sum()
    energy.backward()
    torch.testing.assert_close(g, va.grad, rtol=1e-12, atol=1e-12)
    assert float(g[..., 0, :, :].abs().max()) == 0.0 and float(g[..., :, :, -1].abs().max()) == 0.0
    torch.testing.assert_close(SRR.dR(v, delta), g)


def test_committed_bench_line_carries_the_contract_fields():
    """The JSON line `bench.py` printed for the committed round profile (profiles/r03_bench_n1.json, produced by
    tools/gpu_check.sh on the GPU box): every field the measurement contract names, with consistent arithmetic."""
    import json

    path = os.path.join(ROOT, "profiles", "r03_bench_n1.json")
    d = json.load(open(path))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-6)  # 2^20-point iterations per second on one GPU
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9)
    assert r["achieved"] == pytest.approx(r["algorithmic_bytes_per_launch"] / (r["launch_ms"] * 1e-3) / 1e9, rel=1e-6)
    assert 0 < r["traffic"] < r["algorithmic_bytes_per_launch"]  # PMC bytes: the table is cache-resident, the scatter merged on chip
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0


def test_bench_dump_outputs_writes_each_steps_losses():
    """``bench.py --dump-outputs``: one float64 scalar file per step and loss, names made file-safe (host logic only)."""
    import tempfile

    import bench

    steps = [{"MSE": torch.tensor(0.5), "MSE+logVar": torch.tensor(-0.25, requires_grad=True)},
             {"MSE": torch.tensor(0.375), "MSE+logVar": torch.tensor(-0.5)}]
    with tempfile.TemporaryDirectory() as d:
        bench.dump_outputs(d, steps)
        assert sorted(os.listdir(d)) == ["step1_loss_MSE.npy", "step1_loss_MSE_logVar.npy", "step2_loss_MSE.npy", "step2_loss_MSE_logVar.npy"]
        for i, losses in enumerate(steps, 1):
            for k, f in (("MSE", "MSE"), ("MSE+logVar", "MSE_logVar")):
                a = np.load(os.path.join(d, f"step{i}_loss_{f}.npy"))
                assert a.dtype == np.float64 and a.shape == () and float(a) == float(losses[k])


def test_queue_capacities_saved_by_one_process_are_loaded_by_the_next(tmp_path, monkeypatch):
    """``save_queue_scales`` / ``NESVOR_HASHGRID_QUEUE=load:<file>`` (encoding.QueueSizer): a sizer made under the load policy
    starts from the capacities written for its key (clamped to [START, 1]), any other key from START; no GPU involved."""
    import torch

    from nesvor_amd import encoding
    from nesvor_amd.encoding import QueueSizer
    from nesvor_amd.grid import HashGridSpec

    spec = HashGridSpec(16, 2, 19, 9, 1.26)
    dev = torch.device("cpu")
    monkeypatch.setattr(encoding, "_SIZERS", {})
    monkeypatch.setattr(QueueSizer, "policy", "adaptive")
    sz = encoding.queue_sizer(spec, 1 << 20, dev)
    assert all(abs(sz.scale[l] - QueueSizer.START) < 1e-9 for l in range(16))
    sz.scale[3], sz.scale[15] = 0.25, 1.0
    path = str(tmp_path / "scales.json")
    encoding.save_queue_scales(path)
    monkeypatch.setattr(encoding, "_SIZERS", {})
    monkeypatch.setattr(QueueSizer, "policy", "load:" + path)
    again = encoding.queue_sizer(spec, 1 << 20, dev)
    assert [round(float(again.scale[l]), 4) for l in (0, 3, 15)] == [round(QueueSizer.START, 4), 0.25, 1.0]
    other = encoding.queue_sizer(spec, 1 << 17, dev)  # another batch size: nothing saved for it
    assert all(abs(other.scale[l] - QueueSizer.START) < 1e-9 for l in range(16))
    monkeypatch.setattr(QueueSizer, "policy", "load:" + str(tmp_path / "missing.json"))
    monkeypatch.setattr(encoding, "_SIZERS", {})
    assert abs(encoding.queue_sizer(spec, 1 << 20, dev).scale[3] - QueueSizer.START) < 1e-9
