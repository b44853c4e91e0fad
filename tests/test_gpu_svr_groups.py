"""The grouped similarity sums of csrc/svr.hip (``torch.ops.nesvor.svr_similarity_groups`` and its ``_bank`` twin) BIT FOR BIT
against their definition: the composition ``correction o base`` written out element by element in numpy in the stated order
(double, every sum of products left to right, rounded once to fp32), fed to ``torch.ops.nesvor.svr_similarity`` - which
tests/test_gpu_svr_similarity.py pins per pixel against the CPU acquisition oracle - and its per-slice sums added per group in CSR
order in a host loop in double.  One pin goes round the sibling kernel: a geometry of tests/acq_geometry.py through
tests/svr_reference.py (the oracle's sums and derived bounds, added over the group).

Shapes where the kernels can go wrong: 5 x 7 slices (one partly filled workgroup) and 17 x 19 (two workgroups, the last
ragged); PSFs of 27 taps, one tap and 1024 (the LDS list's last entry); K = 1 (single-pose kernel), 13 (one pass), 14 (a pass
and a single), 27 (two passes and a single); with and without a mask; groupings with interleaving, empty groups, unlisted and
doubly listed slices and a group wholly outside the volume."""
import numpy as np
import pytest
import torch

import nesvor_amd.ops  # noqa: F401  (registers torch.ops.nesvor)

pytestmark = pytest.mark.gpu

DIMS = (9, 10, 11)
N = 7  # slice 6 lies 100 voxels outside the volume
RES = 1.25
SHAPES = {"5x7": (5, 7), "17x19": (17, 19)}
PSFS = {"psf333": (3, 3, 3), "psf111": (1, 1, 1), "psf1024": (4, 16, 16)}
GROUPINGS = {
    "P2": [[0, 2, 4, 6], [1, 3, 5]],
    "P3": [[0, 3, 6], [1, 4], [2, 5]],
    "all": [[0, 1, 2, 3, 4, 5, 6]],
    "singles": [[0], [1], [2], [3], [4], [5], [6]],
    "empty_between": [[4, 1], [], [0, 5]],  # an empty group; slices 2, 3, 6 in no group; members out of order
    "twice": [[0, 1, 2], [2, 3], []],  # slice 2 in two groups, a trailing empty group
    "outside": [[0, 1], [6], [2]],  # group 1: every pixel outside the volume
}
_CACHE = {}


def _rigid(g, n, angle, shift):
    """n translation-first [R | t] fp32 matrices: rotation vectors ~ angle N(0,1) rad, translations ~ shift N(0,1) voxels."""
    r = torch.randn(n, 3, generator=g, dtype=torch.float64) * angle
    t = torch.randn(n, 3, generator=g, dtype=torch.float64) * shift
    th = r.norm(dim=-1).clamp(min=1e-12)[:, None, None]
    k = torch.zeros(n, 3, 3, dtype=torch.float64)
    k[:, 0, 1], k[:, 0, 2], k[:, 1, 0], k[:, 1, 2], k[:, 2, 0], k[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
    R = torch.eye(3, dtype=torch.float64) + torch.sin(th) / th * k + (1 - torch.cos(th)) / (th * th) * (k @ k)
    return torch.cat([R, t[:, :, None]], -1).float().contiguous()


def _inputs(shape, psf):
    key = (shape, psf)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1234 + 17 * list(SHAPES).index(shape) + list(PSFS).index(psf))
        h, w = SHAPES[shape]
        p = 0.2 + torch.rand(PSFS[psf], generator=g)
        base = _rigid(g, N, 0.4, 1.5)
        base[6, 2, 3] += 100.0
        _CACHE[key] = dict(vol=torch.rand(DIMS, generator=g), psf=(p / p.sum()).contiguous(), base=base,
                           slices=torch.rand((N, h, w), generator=g), mask=torch.rand((N, h, w), generator=g) < 0.7,
                           corr=_rigid(g, 7 * 27, 0.15, 1.0).view(7, 27, 3, 4))
    return _CACHE[key]


def _csr(groups):
    off = [0]
    for m in groups:
        off.append(off[-1] + len(m))
    return torch.tensor(off, dtype=torch.int32), torch.tensor([k for m in groups for k in m], dtype=torch.int32)


def compose_numpy(corr, base):
    """correction o base, (..., 3, 4) fp32 each -> fp32: in double, element by element, every sum of products left to right."""
    c, b = corr.numpy().astype(np.float64), base.numpy().astype(np.float64)
    out = np.empty(np.broadcast_shapes(c.shape, b.shape), dtype=np.float64)
    for r in range(3):
        for col in range(3):
            out[..., r, col] = c[..., r, 0] * b[..., 0, col] + c[..., r, 1] * b[..., 1, col] + c[..., r, 2] * b[..., 2, col]
        rtu = b[..., 0, r] * c[..., 0, 3] + b[..., 1, r] * c[..., 1, 3] + b[..., 2, r] * c[..., 2, 3]
        out[..., r, 3] = b[..., r, 3] + rtu
    return torch.from_numpy(out.astype(np.float32))


def _yardstick(device, x, corr, groups, mask, per_slice):
    """(G,K,6) fp64 on the host.  per_slice(mats (E,K,3,4), ids) -> (E,K,6): the sibling op on the listed slices."""
    G, K = corr.shape[:2]
    want = torch.zeros((G, K, 6), dtype=torch.float64)
    listed = [k for m in groups for k in m]
    if not listed or K == 0:
        return want
    entry_group = [g for g, m in enumerate(groups) for _ in m]
    mats = compose_numpy(corr[entry_group], x["base"][listed][:, None])
    per = per_slice(mats.contiguous().to(device), listed).cpu()
    e = 0
    for g, m in enumerate(groups):
        s = torch.zeros((K, 6), dtype=torch.float64)
        for _ in m:
            s = s + per[e]
            e += 1
        want[g] = s
    return want


def _one_psf(device, x, mask):
    def per_slice(mats, ids):
        return torch.ops.nesvor.svr_similarity(x["vol"].to(device), x["psf"].to(device), mats, x["slices"][ids].contiguous().to(device),
                                               None if mask is None else mask[ids].contiguous().to(device), RES)
    return per_slice


def _groups(device, x, corr, groups, mask):
    off, listed = _csr(groups)
    out = torch.ops.nesvor.svr_similarity_groups(x["vol"].to(device), x["psf"].to(device), corr.contiguous().to(device), x["base"].to(device),
                                                 off, listed, x["slices"].to(device), None if mask is None else mask.to(device), RES)
    assert out.shape == (len(groups), corr.shape[1], 6) and out.dtype == torch.float64
    return out.cpu()


@pytest.mark.parametrize("K", [1, 13, 14, 27])
@pytest.mark.parametrize("psf", list(PSFS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_groups_equal_composed_per_slice_sums_in_csr_order(device, shape, psf, K):
    x = _inputs(shape, psf)
    for masked in (True, False):
        mask = x["mask"] if masked else None
        for name, groups in GROUPINGS.items():
            corr = x["corr"][:len(groups), :K]
            got = _groups(device, x, corr, groups, mask)
            want = _yardstick(device, x, corr, groups, mask, _one_psf(device, x, mask))
            assert torch.equal(got, want), (name, masked, float((got - want).abs().max()))
            for g, m in enumerate(groups):
                if not m:
                    assert float(got[g].abs().max()) == 0, (name, "an empty group is not exact zeros")
            if name == "outside":
                assert float(got[1].abs().max()) == 0 and float(got[0, :, 0].min()) > 0
            if name == "all" and not masked and K == 1:
                assert float(got[0, 0, 0]) > 0  # (the poses do hit the volume)


def test_singles_with_identity_corrections_are_the_sibling_at_the_base_poses(device):
    """n groups of one slice, identity corrections: correction o base is base exactly, so the sums are svr_similarity(base)'s."""
    x = _inputs("17x19", "psf333")
    eye = torch.eye(3, 4).expand(N, 13, 3, 4).contiguous()
    got = _groups(device, x, eye, GROUPINGS["singles"], x["mask"])
    want = torch.ops.nesvor.svr_similarity(x["vol"].to(device), x["psf"].to(device), x["base"][:, None].expand(N, 13, 3, 4).contiguous().to(device),
                                           x["slices"].to(device), x["mask"].to(device), RES).cpu()
    assert torch.equal(got, want)
    assert float(got[:6, :, 0].min()) > 0


def test_no_entry_gives_zeros_and_two_calls_agree(device):
    x = _inputs("5x7", "psf333")
    got = _groups(device, x, x["corr"][:3, :13], [[], [], []], None)
    assert got.shape == (3, 13, 6) and float(got.abs().max()) == 0
    a = _groups(device, x, x["corr"][:3, :27], GROUPINGS["P3"], x["mask"])
    b = _groups(device, x, x["corr"][:3, :27], GROUPINGS["P3"], x["mask"])
    assert torch.equal(a, b)


def test_bad_groupings_are_python_errors_before_a_launch(device):
    x = _inputs("5x7", "psf333")
    args = lambda off, listed: torch.ops.nesvor.svr_similarity_groups(
        x["vol"].to(device), x["psf"].to(device), x["corr"][:2, :1].contiguous().to(device), x["base"].to(device),
        torch.tensor(off, dtype=torch.int32), torch.tensor(listed, dtype=torch.int32), x["slices"].to(device), None, RES)
    for off, listed in (([0, 2, 1], [0, 1]), ([0, 1, 3], [0, 1]), ([0, 1, 2], [0, -1]), ([0, 1, 2], [0, N]), ([1, 1, 2], [0, 1])):
        with pytest.raises(RuntimeError, match="group_"):
            args(off, listed)
    with pytest.raises(RuntimeError, match="host memory"):
        torch.ops.nesvor.svr_similarity_groups(x["vol"].to(device), x["psf"].to(device), x["corr"][:2, :1].contiguous().to(device),
                                               x["base"].to(device), torch.tensor([0, 1, 2], dtype=torch.int32).to(device),
                                               torch.tensor([0, 1], dtype=torch.int32), x["slices"].to(device), None, RES)


def test_library_refusals_and_canaries(device):
    """The C entry point: refusals as hipErrorInvalidValue without a launch, and sums written between untouched canaries."""
    from nesvor_amd import _lib

    lib, P = _lib.load(), _lib.ptr
    x = _inputs("17x19", "psf333")
    h, w = SHAPES["17x19"]
    groups = GROUPINGS["P2"]
    off, listed = (t.to(device) for t in _csr(groups))
    G, E, K = 2, 7, 14
    vol, psf, base = (x[k].to(device) for k in ("vol", "psf", "base"))
    corr = x["corr"][:G, :K].contiguous().to(device)
    J, m = x["slices"].to(device), x["mask"].to(device)
    nbytes = int(lib.nesvor_svr_similarity_groups_workspace_bytes(E, K, h, w))
    assert nbytes == 8 * 6 * E * K * 2 and lib.nesvor_svr_similarity_groups_workspace_bytes(0, K, h, w) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    buf = torch.full((16 + G * K * 6 + 16,), -7.0, dtype=torch.float64, device=device)
    sums = buf[16:16 + G * K * 6]
    INVALID = 1  # hipErrorInvalidValue

    def call(psf_shape=(3, 3, 3), G_=G, E_=E, off_=off, listed_=listed, n_=N, K_=K, nb=nbytes):
        with torch.cuda.device(device):
            return lib.nesvor_svr_similarity_groups(P(vol), *DIMS, P(psf), *psf_shape, P(base), P(corr), P(off_), P(listed_), G_, E_, P(J), P(m),
                                                    n_, K_, h, w, RES, P(sums), P(ws), nb, _lib.stream_ptr())

    assert call(G_=0) == INVALID and call(listed_=None) == INVALID and call(off_=None) == INVALID and call(E_=-1) == INVALID
    assert call(psf_shape=(0, 3, 3)) == INVALID and call(psf_shape=(5, 15, 15)) == INVALID and call(nb=nbytes - 8) == INVALID
    assert call(n_=0) == INVALID
    assert call(K_=0) == 0 and call(E_=0, listed_=None) == 0
    torch.cuda.synchronize(device)
    assert float((buf + 7.0).abs().max()) == 0  # nothing was written by any of them
    assert call() == 0
    torch.cuda.synchronize(device)
    assert float((buf[:16] + 7.0).abs().max()) == 0 and float((buf[-16:] + 7.0).abs().max()) == 0
    want = _groups(device, x, x["corr"][:G, :K], groups, x["mask"])
    assert torch.equal(sums.view(G, K, 6).cpu(), want)


def test_group_sums_against_the_acquisition_oracle(device):
    """Independent of the sibling kernel: geometry "sparse" (17 x 19 pixels, (9,5,5) PSF) with identity base poses, so that the
    composed pose IS the correction (products with exact 0 and 1), its 27 poses as corrections of one group of all five slices.
    Reference: the CPU oracle's sums added over the group, bound: its derived per-slice bounds added (tests/svr_reference.py)."""
    import svr_reference as R

    c = R.case("sparse")
    I, wgt = R.images(c, torch.float32)
    n = c.J.shape[0]
    eye = torch.eye(3, 4).expand(n, 3, 4).contiguous()
    for mask_name in ("none", "random"):
        mask = c.masks[mask_name]
        ref = R.sums(I, wgt, c.J, mask)
        bound = R.sum_bounds(I, wgt, c.J, mask, ref).sum(0)
        want = ref.sum(0)
        off, listed = _csr([list(range(n))])
        got = torch.ops.nesvor.svr_similarity_groups(c.vol.to(device), c.psf.to(device), c.poses[None].contiguous().to(device), eye.to(device),
                                                     off, listed, c.J.to(device), None if mask is None else mask.to(device), c.res).cpu()[0]
        err = (got - want).abs()
        free = bound > 0
        ratio = float((err[free] / bound[free]).max())
        print(f"RATIO sparse groups {mask_name} {ratio:.4f}")
        assert torch.equal(got[~free], want[~free]) and ratio <= 1, (mask_name, ratio)
        assert float(want[:, 0].max()) > 100


def _bank_groups(device, x, bank, corr, groups, mask):
    off, listed = _csr(groups)
    return torch.ops.nesvor.svr_similarity_groups_bank(x["vol"].to(device), bank.flat, bank.table, bank.ids, corr.contiguous().to(device),
                                                       x["base"].to(device), off, listed, x["slices"].to(device),
                                                       None if mask is None else mask.to(device), RES).cpu()


def test_bank_twin(device):
    """Two members of different thickness with ids mixed inside every group, against the bank sibling per slice; a bank of one
    member gives the one-PSF twin's bits."""
    from nesvor_amd.psf_bank import PsfBank
    from nesvor_amd.utils import get_PSF

    x = _inputs("17x19", "psf333")
    thin, thick = get_PSF(res_ratio=(1.0, 1.0, 1.0), device=device), get_PSF(res_ratio=(1.0, 1.0, 3.0), device=device)
    assert thin.shape != thick.shape
    bank = PsfBank([thin, thick], [0, 1, 1, 0, 1, 0, 0])
    for K in (1, 14):
        for name in ("P2", "empty_between", "twice"):
            groups = GROUPINGS[name]
            corr = x["corr"][:len(groups), :K]

            def per_slice(mats, ids):
                sub = PsfBank([thin, thick], [bank.host_ids[i] for i in ids])
                return torch.ops.nesvor.svr_similarity_bank(x["vol"].to(device), sub.flat, sub.table, sub.ids, mats,
                                                            x["slices"][ids].contiguous().to(device), x["mask"][ids].contiguous().to(device), RES)

            got = _bank_groups(device, x, bank, corr, groups, x["mask"])
            assert torch.equal(got, _yardstick(device, x, corr, groups, x["mask"], per_slice)), (K, name)
    one = PsfBank([x["psf"].to(device)], [0] * N)
    corr = x["corr"][:3, :14]
    assert torch.equal(_bank_groups(device, x, one, corr, GROUPINGS["P3"], None), _groups(device, x, corr, GROUPINGS["P3"], None))


def test_group_descent_fused_equals_composed(device, monkeypatch):
    """GroupSVR on one small level: the fused op and NESVOR_PACKAGES=composed give bit-equal losses and corrections."""
    from nesvor_amd.registration import GroupSVR, package_groups
    from nesvor_amd.transform import RigidTransform

    g = torch.Generator().manual_seed(5)
    vol = torch.rand((1, 1, 20, 22, 24), generator=g).to(device)
    vol = torch.nn.functional.avg_pool3d(vol, 3, 1, 1) * 3
    n, hw = 8, 21
    theta = torch.zeros((n, 6))
    theta[:, 5] = (torch.arange(n) - (n - 1) / 2) * 2.0
    theta[:, :3] = 0.05 * torch.randn((n, 3), generator=g)
    theta = theta.to(device)
    params = {"res_s": 1.0, "s_thick": 2.0, "res_r": 1.0}
    from nesvor_amd.slice_acquisition import slice_acquisition
    from nesvor_amd.utils import get_PSF

    psf = get_PSF(res_ratio=(1.0, 1.0, 2.0), device=device)
    moved = theta.clone()
    moved[::2, 3] += 1.0  # package 0 acquired one voxel off
    slices = slice_acquisition(RigidTransform(moved).matrix(), vol, None, None, psf, (hw, hw), 1.0, False, False)
    mask = slices > 0
    groups = package_groups([n], [2])
    out = {}
    for mode in ("fused", "composed"):
        if mode == "composed":
            monkeypatch.setenv("NESVOR_PACKAGES", "composed")
        gsvr = GroupSVR(num_levels=1, num_steps=2, step_size=1, max_iter=5, optimizer={"name": "gd", "momentum": 0.1}, loss={"name": "ncc"})
        before = gsvr.evaluate(theta, groups, slices, mask, vol, params)
        theta_out, loss = gsvr(theta, groups, slices, mask, vol, params)
        out[mode] = (before.cpu(), loss.cpu(), gsvr.corrections.cpu(), theta_out.cpu())
        level, start, end = gsvr.history[0]
        assert level == 0 and bool((end <= start).all()) and torch.equal(start.cpu(), before.cpu())
    for a, b in zip(out["fused"], out["composed"]):
        assert torch.equal(a, b)
    before, loss = out["fused"][:2]
    assert float(loss[0]) < float(before[0])  # the displaced package improved
