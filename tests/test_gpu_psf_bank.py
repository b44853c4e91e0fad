"""Per-slice PSFs: the PSF-bank entry points of csrc/slice_acq.hip and csrc/svr.hip (``nesvor_slice_acq_forward_bank``,
``nesvor_slice_acq_adjoint_forward_bank``, ``nesvor_svr_similarity_bank``; ops ``torch.ops.nesvor.*_bank``).

What a bank must be BIT FOR BIT: a bank of one is the one-PSF entry point; a member padded with zero taps (to a larger odd size, to
an even size, stored at a non-zero offset) is the member itself; the rows of member g in a mixed bank are the one-PSF call on those
slices alone with member g (forward and similarity sums).  The ids are interleaved in every case, so nothing passes by grouping.
The adjoint of a mixed bank sums over members inside one voxel's accumulation, so it is compared against oracle/slice_acq.py in
fp64, composed per member, at the project's bounds of the adjoint (``TOL32`` of tests/acq_geometry.py; not fitted here).

Geometries of tests/acq_geometry.py: "odd", "tiny", "dense" (exactly 256 pixels per slice) and "row" (one pixel more)."""
import ctypes
import types

import pytest
import torch
import torch.nn.functional as F

from acq_geometry import GEOMETRIES, OUTSIDE, TOL32, _generic_poses, _lattice_poses, _psf

pytestmark = pytest.mark.gpu

GEOMS = ["odd", "tiny", "dense", "row"]
INVALID = 1  # hipErrorInvalidValue
K_POSES = 14  # one 13-pose pass and one single-pose pass of the similarity kernel
# generic poses: seed per (geometry, masks); for the adjoint of the mixed bank they are checked on the CPU: the composition of the
# oracle in fp32 agrees with the one in fp64 within TOL32 on every element (asserted in the test)
SEEDS = {(g, m): 700 + 10 * i + int(m) for i, g in enumerate(GEOMS) for m in (False, True)}
SEEDS[("row", False)] = 731  # (730 puts a boundary flip of the oracle's own into the equalised adjoint)
_DATA = {}


def _case(geom, poses, masks, n=6):
    """fp32 inputs on the CPU, made once and never written: n poses (lattice: the six of acq_geometry, the slice 100 voxels
    outside among them), a volume, acquired slices, masks of about 70 % with slice 1 fully masked, K_POSES poses per slice for
    the similarity sums (the pose itself, then small moves of it)."""
    key = (geom, poses, masks, n)
    if key not in _DATA:
        dims, shape, res, psf = GEOMETRIES[geom]
        g = torch.Generator().manual_seed(SEEDS[(geom, masks)] + n)
        tf = _lattice_poses(dims) if poses == "lattice" else _generic_poses(n, g)
        if tf.shape[0] < n:
            tf = torch.cat([tf, _generic_poses(n - tf.shape[0], g)])
        tf = tf[:n].contiguous()
        c = types.SimpleNamespace(key=key, dims=dims, shape=shape, res=res, psf=_psf(psf), tf=tf, n=n,
                                  vol=torch.rand((1, 1) + dims, generator=g), y=torch.rand((n, 1) + shape, generator=g), vm=None, sm=None)
        if masks:
            c.vm = torch.rand((1, 1) + dims, generator=g) < 0.7
            c.sm = torch.rand((n, 1) + shape, generator=g) < 0.7
            if n > 1:
                c.sm[1] = False
        moves = torch.zeros(K_POSES, 3, 4)
        moves[1:, :, 3] = torch.randint(-4, 5, (K_POSES - 1, 3), generator=g).float() / 8
        c.tfk = (tf[:, None] + moves[None]).contiguous()
        _DATA[key] = c
    return _DATA[key]


def _bank(psfs, ids, device):
    from nesvor_amd.psf_bank import PsfBank

    return PsfBank([p.to(device) for p in psfs], ids)


def _dev(t, device):
    return torch.empty(0, device=device) if t is None else t.to(device)


def _one(device, c, psf, idx=None):
    """The one-PSF ops on the slices ``idx`` (all): slices, weight, A^T with and without equalisation, the similarity sums (None
    for a PSF the similarity kernel refuses)."""
    from nesvor_amd import slice_acq_cuda as K

    sel = slice(None) if idx is None else idx
    tf, y, tfk = c.tf[sel].contiguous().to(device), c.y[sel].contiguous().to(device), c.tfk[sel].contiguous().to(device)
    sm = None if c.sm is None else c.sm[sel].contiguous()
    psf = psf.to(device)
    out = {}
    out["slices"], out["weight"] = K.forward(tf, c.vol.to(device), _dev(c.vm, device), _dev(sm, device), psf, c.shape, c.res, True, False)
    for eq in (False, True):
        out["vol", eq], out["vol_weight", eq] = K.adjoint_forward(tf, psf, y, _dev(sm, device), _dev(c.vm, device), c.dims, c.res, False, eq)
    out["sums"] = None
    if psf.numel() <= 1024:
        out["sums"] = torch.ops.nesvor.svr_similarity(c.vol.to(device), psf, tfk, y, None if sm is None else sm.to(device), c.res)
    return out


def _banked(device, c, bank, adjoint=True, sums=True):
    out = {}
    tf, y = c.tf.to(device), c.y.to(device)
    out["slices"], out["weight"] = torch.ops.nesvor.slice_acq_forward_bank(
        tf, c.vol.to(device), _dev(c.vm, device), _dev(c.sm, device), bank.flat, bank.table, bank.ids, list(c.shape), c.res, True)
    if adjoint:
        for eq in (False, True):
            out["vol", eq], out["vol_weight", eq] = torch.ops.nesvor.slice_acq_adjoint_forward_bank(
                tf, bank.flat, bank.table, bank.ids, y, _dev(c.sm, device), _dev(c.vm, device), list(c.dims), c.res, eq)
    if sums:
        out["sums"] = torch.ops.nesvor.svr_similarity_bank(c.vol.to(device), bank.flat, bank.table, bank.ids, c.tfk.to(device), y,
                                                           None if c.sm is None else c.sm.to(device), c.res)
    return out


def _same(got, ref, what):
    for name, r in ref.items():
        if r is None or name not in got:
            continue
        assert got[name].shape == r.shape and torch.equal(got[name], r), (what, name)


def _not_vacuous(c, out):
    """A case must simulate something and, but for the (2,2,2) volume (at most the centre tap of a pixel falls inside it: no pixel
    reaches A^T's weight of 0.5 under every pose set), back-project something."""
    assert float((out["weight"] > 0).float().mean()) > 0.02 and float(out["sums"][..., 0].max()) > 0, c.key
    assert c.key[0] == "tiny" or float(out["vol_weight", True].abs().max()) > 0, c.key


PARAMS = [pytest.param(g, p, m, id=f"{g}-{p}-{'masks' if m else 'nomask'}") for g in GEOMS for p in ("lattice", "generic") for m in (False, True)]


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: what must be the one-PSF entry points bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,poses,masks", PARAMS)
def test_bank_of_one_is_the_one_psf_entry_point(device, geom, poses, masks):
    """P = 1: A (slices and weights), A^T (vol, vol_weight, equalize 0 and 1) and the similarity sums equal the one-PSF entry
    points bit for bit."""
    c = _case(geom, poses, masks)
    ref = _one(device, c, c.psf)
    _not_vacuous(c, ref)
    _same(_banked(device, c, _bank([c.psf], [0] * c.n, device)), ref, c.key)


@pytest.mark.parametrize("twin", ["odd", "even"])
@pytest.mark.parametrize("geom,poses,masks", PARAMS)
def test_zero_padded_twin_changes_no_bit(device, geom, poses, masks, twin):
    """{A, A'}: A' is A zero-padded to a larger odd size (other margins per axis) or to an even size (one plane in front of every
    axis: the tap range -d/2 .. (d+1)/2 - 1 of an even size keeps A's centre), stored behind A, so at a non-zero offset; the ids
    alternate.  Same non-zero taps in the same order, other extents in the gather's box bounds: all outputs are the one-PSF
    call's with A, bit for bit."""
    c = _case(geom, poses, masks)
    pad = (1, 1, 2, 2, 1, 1) if twin == "odd" else (1, 0, 1, 0, 1, 0)
    twin_psf = F.pad(c.psf, pad).contiguous()
    assert all(s % 2 == (1 if twin == "odd" else 0) for s in twin_psf.shape) and twin_psf.numel() <= 1024
    bank = _bank([c.psf, twin_psf], [k % 2 for k in range(c.n)], device)
    assert int(bank.table[1, 0]) == c.psf.numel()
    _same(_banked(device, c, bank), _one(device, c, c.psf), (c.key, twin))


# ---------------------------------------------------------------------------------------------------------------------
# 3: a mixed bank, forward and similarity sums, against the one-PSF calls per member
# ---------------------------------------------------------------------------------------------------------------------
def _members(big=False):
    from nesvor_amd.utils import get_PSF

    m = [get_PSF(res_ratio=(1.5, 1.5, 3.0)), get_PSF(res_ratio=(1.5, 1.5, 4.5)), _psf("psf426")]
    assert not torch.equal(m[0], m[1])  # (both (9,5,5): the second profile is wider inside the same support)
    return m + [_psf("psf1788")] if big else m


@pytest.mark.parametrize("geom,poses,masks", PARAMS)
def test_mixed_bank_rows_are_their_members_calls(device, geom, poses, masks):
    """Three members (two thicknesses of get_PSF and an even-sized one), ids 0, 1, 0, 2, 1, 2: the rows of member g - slices,
    weights, similarity sums - equal, bit for bit, the one-PSF call on those slices alone with member g.  For the forward a
    fourth member of 1088 elements walks global memory in the same launch (ids 0, 1, 3, 2, 3, 0, 1, 2 on eight slices); the
    similarity entry refuses that bank and leaves the canaries around its output untouched."""
    from nesvor_amd import _lib

    c = _case(geom, poses, masks)
    ids = [0, 1, 0, 2, 1, 2]
    got = _banked(device, c, _bank(_members(), ids, device), adjoint=False)
    for g, psf in enumerate(_members()):
        idx = torch.tensor([k for k, i in enumerate(ids) if i == g])
        ref = _one(device, c, psf, idx)
        for name in ("slices", "weight", "sums"):
            assert torch.equal(got[name][idx.to(device)], ref[name]), (c.key, g, name)
    c8 = _case(geom, poses, masks, n=8)
    ids8 = [0, 1, 3, 2, 3, 0, 1, 2]
    bank8 = _bank(_members(big=True), ids8, device)
    assert bank8.max_elements() == 1088
    got8 = _banked(device, c8, bank8, adjoint=False, sums=False)
    for g, psf in enumerate(_members(big=True)):
        idx = torch.tensor([k for k, i in enumerate(ids8) if i == g])
        ref = _one(device, c8, psf, idx)
        for name in ("slices", "weight"):
            assert torch.equal(got8[name][idx.to(device)], ref[name]), (c8.key, g, name)
    assert float(got8["weight"][torch.tensor([2, 4]).to(device)].max()) > 0  # (the dense walk simulated something)
    # the similarity sums refuse a bank with a member of more than 1024 elements: nothing launched, nothing written
    lib, P = _lib.load(), _lib.ptr
    h, w = c8.shape
    nbytes = int(lib.nesvor_svr_similarity_workspace_bytes(8, K_POSES, h, w))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)
    buf = torch.full((3, 8, K_POSES, 6), -7.0, dtype=torch.float64, device=device)  # the output in the middle, canaries around
    vol, tfk, y = c8.vol.to(device), c8.tfk.to(device), c8.y.to(device)
    err = lib.nesvor_svr_similarity_bank(P(vol), *c8.dims, P(bank8.flat), ctypes.c_void_p(bank8.table.data_ptr()), 4, P(bank8.ids), P(tfk),
                                         P(y), None, 8, K_POSES, h, w, c8.res, P(buf[1]), P(ws), nbytes, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert err == INVALID and bool((buf == -7.0).all())
    with pytest.raises(RuntimeError):
        _banked(device, c8, bank8, adjoint=False, sums=True)


# ---------------------------------------------------------------------------------------------------------------------
# 4: the adjoint of a mixed bank against the oracle in fp64, composed per member
# ---------------------------------------------------------------------------------------------------------------------
def _oracle_adjoint(c, psfs, ids, dtype):
    """sum over members of the oracle's unequalised A^T (and weights) on the member's slices -> {(vol, eq), (vol_weight, True)}."""
    from oracle import slice_acq as O

    key = ("oracle", c.key, tuple(ids), dtype)
    if key in _DATA:
        return _DATA[key]
    vol = torch.zeros((1, 1) + c.dims, dtype=dtype)
    wgt = torch.zeros((1, 1) + c.dims, dtype=dtype)
    for g, psf in enumerate(psfs):
        idx = torch.tensor([k for k, i in enumerate(ids) if i == g])
        sm = None if c.sm is None else c.sm[idx]
        args = (c.tf[idx].to(dtype), psf.to(dtype), c.y[idx].to(dtype), sm, c.vm, c.dims, c.res, False)
        vol += O.slice_acquisition_adjoint_forward(*args, False)[0]
        wgt += O.slice_acquisition_adjoint_forward(*args, True)[1]
    pos = wgt > 0
    out = {("vol", False): vol, ("vol_weight", True): wgt, ("vol", True): torch.where(pos, vol / torch.where(pos, wgt, torch.ones_like(wgt)), vol)}
    _DATA[key] = out
    return out


def _within(got, ref, tol):
    rtol, atol, arel = tol
    bound = rtol * ref.abs() + atol + arel * float(ref.abs().max())
    err = (got.double() - ref.double()).abs()
    return bool((err <= bound).all()), float((err - bound).max())


def _check_adjoint(got, ref, what):
    for name, tol in ((("vol", False), "adjoint"), (("vol", True), "adjoint"), (("vol_weight", True), "adjoint_weight")):
        ok, excess = _within(got[name].cpu(), ref[name], TOL32[tol])
        assert ok, (what, name, "excess over the bound", excess)


@pytest.mark.parametrize("geom,poses,masks", PARAMS)
def test_mixed_bank_adjoint_against_the_oracle(device, geom, poses, masks, monkeypatch):
    """A^T (vol with and without equalisation, vol_weight) of the three-member bank, ids 0, 1, 0, 2, 1, 2, against the fp64 oracle
    called once per member on that member's slices - unequalised adjoints and weights summed, then divided - at TOL32's
    ``adjoint`` / ``adjoint_weight`` bounds.  The seeds are fixed so that the same composition of the oracle in fp32 agrees
    with fp64 within that bound on every element (asserted).  The composed path (NESVOR_PSF_BANK=composed) agrees within the
    same bound.  Through the C ABI every element of NaN-filled vol / vol_weight is written and the results are the op's.  Without
    masks: <A x, y keep> = <x, A^T (y keep)> to 1e-4 relative (tests/test_gpu_ops.py::test_slice_acq_adjointness_gpu's bound),
    keep = the pixels of PSF weight >= 0.5."""
    from nesvor_amd import _lib
    from nesvor_amd.slice_acquisition import slice_acquisition_adjoint_bank, slice_acquisition_bank

    c = _case(geom, poses, masks)
    ids = [0, 1, 0, 2, 1, 2]
    psfs = _members()
    ref = _oracle_adjoint(c, psfs, ids, torch.float64)
    assert (geom == "tiny") == (float(ref["vol_weight", True].max()) == 0)  # (the (2,2,2) volume: A^T of these PSFs is the zero volume)
    _check_adjoint(_oracle_adjoint(c, psfs, ids, torch.float32), ref, "fp32 oracle against fp64 oracle")
    bank = _bank(psfs, ids, device)
    got = _banked(device, c, bank, sums=False)
    _check_adjoint(got, ref, c.key)
    if poses == "lattice":
        assert torch.equal(got["vol_weight", True].cpu() > 0, ref["vol_weight", True] > 0)
    if masks:
        assert float(got["vol", True][~c.vm.to(device)].abs().max()) == 0
    # the wrappers: fused (what the ops gave) and composed
    tf, y, sm, vm = c.tf.to(device), c.y.to(device), (None if c.sm is None else c.sm.to(device)), (None if c.vm is None else c.vm.to(device))
    for mode in ("", "composed"):
        monkeypatch.setenv("NESVOR_PSF_BANK", mode)
        w = {}
        for eq in (False, True):
            w["vol", eq], vw = slice_acquisition_adjoint_bank(tf, bank, y, sm, vm, c.dims, c.res, False, eq, need_weight=True)
            if eq:
                w["vol_weight", True] = vw
        s, sw = slice_acquisition_bank(tf, c.vol.to(device), vm, sm, bank, c.shape, c.res, True)
        if mode == "":
            _same(w, {k: got[k] for k in w}, (c.key, "wrapper"))
        else:
            _check_adjoint(w, ref, (c.key, "composed"))
        assert torch.equal(s, got["slices"]) and torch.equal(sw, got["weight"]), mode  # (the forward composes bit for bit)
    # the C ABI overwrites: NaN-filled outputs come back fully written
    lib, P = _lib.load(), _lib.ptr
    D, H, W = c.dims
    h, w_ = c.shape
    scratch = torch.empty(2 * c.n * h * w_, dtype=torch.float32, device=device)
    for eq in (0, 1):
        vol = torch.full((1, 1, D, H, W), float("nan"), device=device)
        vw = torch.full((1, 1, D, H, W), float("nan"), device=device)
        err = lib.nesvor_slice_acq_adjoint_forward_bank(P(tf), P(bank.flat), ctypes.c_void_p(bank.table.data_ptr()), 3, P(bank.ids), P(y), P(sm),
                                                        P(vm), P(vol), P(vw), P(scratch), D, H, W, c.n, h, w_, c.res, eq, _lib.stream_ptr())
        torch.cuda.synchronize()
        assert err == 0 and bool(torch.isfinite(vol).all()) and bool(torch.isfinite(vw).all())
        assert torch.equal(vol, got["vol", bool(eq)]) and torch.equal(vw, got["vol_weight", True])
    if not masks:
        keep = (got["weight"] >= 0.5).float()
        Aty = slice_acquisition_adjoint_bank(tf, bank, y * keep, None, None, c.dims, c.res)
        lhs, rhs = float((got["slices"] * y * keep).double().sum()), float((c.vol.to(device) * Aty).double().sum())
        assert (lhs != 0 or geom == "tiny") and abs(lhs - rhs) <= 1e-4 * abs(lhs), (lhs, rhs)


# ---------------------------------------------------------------------------------------------------------------------
# 5: edges
# ---------------------------------------------------------------------------------------------------------------------
def _abi(device, c, bank, n=None, P_members=None, table=None):
    """The three entry points on sentinel-filled outputs (-7) -> (errors, outputs)."""
    from nesvor_amd import _lib

    lib, P = _lib.load(), _lib.ptr
    n = c.n if n is None else n
    D, H, W = c.dims
    h, w = c.shape
    table = bank.table if table is None else table
    pm = bank.n_members if P_members is None else P_members
    tp = ctypes.c_void_p(table.data_ptr())
    tf, y, vol, tfk = c.tf.to(device), c.y.to(device), c.vol.to(device), c.tfk.to(device)
    full = lambda *s, dtype=torch.float32: torch.full(s, -7.0, dtype=dtype, device=device)
    o = types.SimpleNamespace(slices=full(c.n, 1, h, w), weight=full(c.n, 1, h, w), vol=full(1, 1, D, H, W), vol_weight=full(1, 1, D, H, W),
                              sums=full(c.n, K_POSES, 6, dtype=torch.float64))
    scratch = torch.empty(max(2 * c.n * h * w, 1), dtype=torch.float32, device=device)
    nbytes = int(lib.nesvor_svr_similarity_workspace_bytes(c.n, K_POSES, h, w))
    ws = torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)
    errs = (lib.nesvor_slice_acq_forward_bank(P(tf), P(vol), None, None, P(bank.flat), tp, pm, P(bank.ids), P(o.slices), P(o.weight), D, H, W, n,
                                              h, w, c.res, _lib.stream_ptr()),
            lib.nesvor_slice_acq_adjoint_forward_bank(P(tf), P(bank.flat), tp, pm, P(bank.ids), P(y), None, None, P(o.vol), P(o.vol_weight),
                                                      P(scratch), D, H, W, n, h, w, c.res, 1, _lib.stream_ptr()),
            lib.nesvor_svr_similarity_bank(P(vol), D, H, W, P(bank.flat), tp, pm, P(bank.ids), P(tfk), P(y), None, n, K_POSES, h, w, c.res,
                                           P(o.sums), P(ws), nbytes, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return errs, o


def test_single_slice_and_empty_stack(device):
    """n = 1: the bank's one slice is the one-PSF call.  n = 0: every entry point returns 0 and launches nothing - the slices and
    the sums keep their sentinels (they have no element to write), A^T of the empty stack is the zero volume."""
    c1 = _case("odd", "generic", False, n=1)
    members = _members()
    _same(_banked(device, c1, _bank(members, [1], device)), _one(device, c1, members[1]), "n = 1")
    c = _case("odd", "generic", False)
    errs, o = _abi(device, c, _bank(members, [0, 1, 0, 2, 1, 2], device), n=0)
    assert errs == (0, 0, 0)
    assert bool((o.slices == -7).all()) and bool((o.weight == -7).all()) and bool((o.sums == -7).all())
    assert float(o.vol.abs().max()) == 0 and float(o.vol_weight.abs().max()) == 0


def test_outside_and_fully_masked_slices(device):
    """The lattice's slice 100 voxels outside the volume and the fully masked slice 1 give exact zeros in slices, weights and sums,
    whatever their member; acquired alone, the outside slice back-projects to the zero volume."""
    c = _case("dense", "lattice", True)
    members = _members()
    ids = [0, 1, 0, 2, 1, 2]
    got = _banked(device, c, _bank(members, ids, device))
    for k in (OUTSIDE, 1):
        for name in ("slices", "weight", "sums"):
            assert float(got[name][k].abs().max()) == 0, (k, name)
    assert float(got["weight"][0].max()) > 0
    one = types.SimpleNamespace(**{**vars(c), "tf": c.tf[OUTSIDE:OUTSIDE + 1], "y": c.y[OUTSIDE:OUTSIDE + 1], "tfk": c.tfk[OUTSIDE:OUTSIDE + 1],
                                   "sm": None, "vm": None, "n": 1})
    alone = _banked(device, one, _bank(members, [ids[OUTSIDE]], device))
    assert float(alone["vol", True].abs().max()) == 0 and float(alone["vol_weight", True].abs().max()) == 0


def test_ids_outside_the_bank_have_no_taps(device):
    """The C ABI's guard (Python refuses such ids on the host): slices with id -1 and id P are simulated as empty and contribute
    nothing to A^T - the other slices' rows and the volume are those of the stack without them."""
    c = _case("odd", "generic", False)
    members = _members()
    ids = [0, 1, 0, 2, 1, 2]
    bank = _bank(members, ids, device)
    bank.ids = torch.tensor([0, -1, 0, 2, 3, 2], dtype=torch.int32, device=device)  # (slices 1 and 4 lose their member)
    errs, o = _abi(device, c, bank)
    assert errs == (0, 0, 0)
    keep = torch.tensor([0, 2, 3, 5])
    sub = types.SimpleNamespace(**{**vars(c), "tf": c.tf[keep], "y": c.y[keep], "tfk": c.tfk[keep], "n": 4})
    ref = _banked(device, sub, _bank(members, [0, 0, 2, 2], device))
    for k in (1, 4):  # (the forward writes only pixels of positive weight: the sentinels stay; their sums are exact zeros)
        assert bool((o.slices[k] == -7).all()) and bool((o.weight[k] == -7).all()) and float(o.sums[k].abs().max()) == 0
    kd = keep.to(device)
    written = ref["weight"] > 0
    assert torch.equal(o.slices[kd][written], ref["slices"][written]) and torch.equal(o.sums[kd], ref["sums"])
    assert torch.equal(o.vol, ref["vol", True]) and torch.equal(o.vol_weight, ref["vol_weight", True])


def test_refusals_before_launch(device):
    """hipErrorInvalidValue with every sentinel-filled output untouched: P = 0, a zero dimension in the table, a volume of more than
    INT_MAX voxels (only the dimensions lie).  A legal call then succeeds."""
    from nesvor_amd import _lib

    c = _case("odd", "generic", False)
    bank = _bank(_members(), [0, 1, 0, 2, 1, 2], device)
    zero_dim = bank.table.clone()
    zero_dim[1, 2] = 0
    for kw in (dict(P_members=0), dict(table=zero_dim)):
        errs, o = _abi(device, c, bank, **kw)
        assert errs == (INVALID,) * 3, kw
        for out in vars(o).values():
            assert bool((out == -7).all()), kw
    lib, P = _lib.load(), _lib.ptr
    s = torch.full((c.n, 1) + c.shape, -7.0, device=device)
    big = (2048, 1024, 1024)
    tp = ctypes.c_void_p(bank.table.data_ptr())
    tf, vol, y = c.tf.to(device), c.vol.to(device), c.y.to(device)
    h, w = c.shape
    assert lib.nesvor_slice_acq_forward_bank(P(tf), P(vol), None, None, P(bank.flat), tp, 3, P(bank.ids), P(s), None, *big, c.n, h, w, c.res,
                                             _lib.stream_ptr()) == INVALID
    assert lib.nesvor_slice_acq_adjoint_forward_bank(P(tf), P(bank.flat), tp, 3, P(bank.ids), P(y), None, None, P(s), None, P(s), *big, c.n, h, w,
                                                     c.res, 0, _lib.stream_ptr()) == INVALID
    assert lib.nesvor_svr_similarity_bank(P(vol), *big, P(bank.flat), tp, 3, P(bank.ids), P(c.tfk.to(device)), P(y), None, c.n, K_POSES, h, w,
                                          c.res, P(s), P(s), 0, _lib.stream_ptr()) == INVALID
    torch.cuda.synchronize()
    assert bool((s == -7).all())
    errs, o = _abi(device, c, bank)
    assert errs == (0, 0, 0) and not bool((o.vol == -7).any()) and not bool((o.sums == -7).any())


# ---------------------------------------------------------------------------------------------------------------------
# 6 - 8: the pipeline under --per-stack-thickness: two stacks of a 32^3 phantom, 2 mm and 4 mm thick
# ---------------------------------------------------------------------------------------------------------------------
_RES_S, _THICKS, _RES_R = 1.5, (2.0, 4.0), 1.0
_STACKS = {}


def _two_stacks(device):
    """The phantom and its two still stacks of unequal thickness (each simulated with the PSF of its own), normalised together by
    the 0.99 quantile q of their masked intensities; built once, never written."""
    if not _STACKS:
        from nesvor_amd.phantom import phantom3d, simulate_stacks
        from nesvor_amd.transform import RigidTransform

        vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
        slices, _ = simulate_stacks(vol, n_stacks=2, res_s=_RES_S, s_thick=list(_THICKS), seed=0, normalize=False)
        groups = [[s for s in slices if s.stack_idx == j] for j in range(2)]
        assert len(groups[0]) > len(groups[1]) > 4 and all(float(s.resolution_z) == _THICKS[j] for j in range(2) for s in groups[j])
        allv = torch.cat([s.image[s.mask] for s in slices])
        q = torch.kthvalue(allv, max(int(0.99 * allv.numel()), 1)).values
        _STACKS.update(phantom=vol, q=q, raw=[torch.stack([s.image for s in g]).contiguous() for g in groups],
                       poses=[RigidTransform.cat([s.transformation for s in g]) for g in groups],
                       per_slice=[_THICKS[j] for j in range(2) for _ in groups[j]])
    return _STACKS


def test_bank_operator_reproduces_stacks_of_unequal_thickness(device):
    """The stacks were simulated per stack with the one-PSF operator of their own thickness.  The operator of the pipeline
    (``svr._operator``) with one thickness per slice - a bank of two members - reproduces them exactly: the misfit A x - y is 0
    on every pixel, bit for bit.  The mean-thickness operator, what the pipeline uses without the switch, does not."""
    from nesvor_amd.psf_bank import PsfBank
    from nesvor_amd.svr import _frame_keep, _kept_thickness, _operator

    c = _two_stacks(device)
    images, m, frame_poses, keep = _frame_keep(c["raw"], None, c["poses"], _RES_S)
    thick = _kept_thickness(c["per_slice"], len(c["per_slice"]), keep)
    assert set(thick) == set(_THICKS) and images.shape[0] == len(thick) > 10
    x = c["phantom"][None, None].contiguous()
    op, _ = _operator(images, m, frame_poses, _RES_S, thick, _RES_R, c["phantom"].shape)
    assert isinstance(op.psf, PsfBank) and op.psf.n_members == 2
    assert float((op.forward(x) - images).abs().max()) == 0
    mean_op, _ = _operator(images, m, frame_poses, _RES_S, sum(_THICKS) / 2, _RES_R, c["phantom"].shape)
    assert torch.is_tensor(mean_op.psf) and float((mean_op.forward(x) - images).abs().max()) > 0


def test_register_stacks_spaces_every_stack_by_its_own_gap(device):
    """Gaps 2 and 4 mm: under the switch the consecutive slices of each output stack are its own gap apart (within 1e-4 mm);
    without it both are spaced by the mean thickness, 3 mm, as before."""
    from nesvor_amd.image import Stack
    from nesvor_amd.registration import register_stacks

    c = _two_stacks(device)

    def dataset():
        return [Stack((c["raw"][j] / c["q"]).clone(), c["raw"][j] > 0, c["poses"][j].clone(), 0.0, _RES_S, _RES_S, _THICKS[j], _THICKS[j])
                for j in range(2)]

    for switch, expected in ((True, _THICKS), (False, (3.0, 3.0))):
        out = register_stacks(dataset(), res_s=_RES_S, per_stack_thickness=switch)
        for j in range(2):
            d = _slice_distances(out[j].transformation)
            assert d.shape[0] == c["raw"][j].shape[0] - 1 and float((d - expected[j]).abs().max()) <= 1e-4, (switch, j, d)


def _slice_distances(t):
    """Distances between the world positions of consecutive slice centres (pixel (0, 0, 0) of every slice through its pose)."""
    from nesvor_amd.transform import mat_transform_points

    origin = torch.zeros((len(t), 3), device=t.device)
    centres = mat_transform_points(t.matrix(), origin, True)
    return (centres[1:] - centres[:-1]).norm(dim=1)


def test_cli_svr_per_stack_thickness_end_to_end(tmp_path, device):
    """``svr --per-stack-thickness --registration none`` on the two stacks: it runs, writes a volume, and the simulated slices
    carry the thickness of their own stack.  ``evaluate``'s PSNR against the phantom with and without the switch is printed (and
    recorded in DESIGN.md); no order is asserted: the measured gain is below the 0.1 dB the project asserts PSNRs at."""
    import json
    import os

    from nesvor_amd import cli
    from nesvor_amd.image import Volume
    from nesvor_amd.image_io import load_slices, load_volume
    from nesvor_amd.transform import RigidTransform

    c = _two_stacks(device)
    paths = []
    for j in range(2):
        img = (c["raw"][j] / c["q"])[:, 0].contiguous()
        ax = c["poses"][j].axisangle().mean(0, keepdim=True)  # stack centre pose
        paths.append(str(tmp_path / f"stack{j}.nii.gz"))
        Volume(img, img > 0, RigidTransform(ax), _RES_S, _RES_S, _THICKS[j]).save(paths[-1], masked=False)
    ref = str(tmp_path / "phantom.nii.gz")
    identity = RigidTransform(torch.eye(3, 4, device=device)[None])
    Volume(c["phantom"] / c["q"], c["phantom"] > 0, identity, 1.0, 1.0, 1.0).save(ref, masked=False)
    common = ["svr", "--input-stacks", *paths, "--thicknesses", *[str(t) for t in _THICKS], "--registration", "none", "--n-iter-srr", "30",
              "--output-resolution", str(_RES_R), "--verbose", "0"]
    with_, without, sim = str(tmp_path / "with.nii.gz"), str(tmp_path / "without.nii.gz"), str(tmp_path / "sim")
    cli.main(common + ["--output-volume", with_, "--per-stack-thickness", "--simulated-slices", sim])
    cli.main(common + ["--output-volume", without])
    vol = load_volume(with_, device=device)
    assert vol.image.ndim == 3 and float(vol.image.max()) > 0 and bool(torch.isfinite(vol.image).all())
    written = load_slices(sim, device)
    thick = [round(float(s.resolution_z), 3) for s in written]
    n = [int((c["raw"][j] > 0).flatten(1).any(1).sum()) for j in range(2)]
    assert thick == [_THICKS[0]] * n[0] + [_THICKS[1]] * n[1]
    out = str(tmp_path / "o.json")
    cli.main(["evaluate", "--reference-volume", ref, "--input-volumes", with_, without, "--output-json", out, "--verbose", "0", "--device", "0"])
    rows = json.load(open(out))
    print(f"PSNR against the phantom: with --per-stack-thickness {rows[0]['psnr']:.3f} dB, without {rows[1]['psnr']:.3f} dB "
          f"(SSIM {rows[0]['ssim']:.4f} / {rows[1]['ssim']:.4f}, NCC {rows[0]['ncc']:.5f} / {rows[1]['ncc']:.5f})")
    assert os.path.exists(without) and all(r["psnr"] > 10 for r in rows)


def test_slice_registration_takes_one_thickness_per_slice(device, monkeypatch):
    """``SVR`` with ``params["s_thick"]`` as one value per slice builds a bank per pyramid level: the loss of every slice is, bit
    for bit, the loss the one-PSF path gives that slice with its own thickness (levels 0 and 1); the composed path
    (NESVOR_SVR=composed) agrees to 1e-5; a short descent over a subset of the slices runs and returns finite poses."""
    from nesvor_amd.registration import SVR, PsfBank
    from nesvor_amd.svr import _frame_keep, _kept_thickness

    monkeypatch.delenv("NESVOR_SVR", raising=False)
    monkeypatch.delenv("NESVOR_PSF_BANK", raising=False)
    c = _two_stacks(device)
    images, m, frame_poses, keep = _frame_keep([r / c["q"] for r in c["raw"]], None, c["poses"], _RES_S)
    thick = _kept_thickness(c["per_slice"], len(c["per_slice"]), keep)
    volume = (c["phantom"] / c["q"])[None, None].contiguous()
    theta = frame_poses.axisangle().clone()
    theta[:, 3:] += 0.7  # (off the optimum: the losses differ from slice to slice)
    svr = SVR(num_levels=2, num_steps=1, step_size=2, max_iter=2, optimizer={"name": "gd", "momentum": 0.1}, loss={"name": "ncc"})
    params = {"res_s": _RES_S, "res_r": _RES_R, "s_thick": thick}
    for level in (0, 1):
        assert isinstance(SVR._level(level, images, m, volume, params).psf, PsfBank)
        got = svr.evaluate(theta, images, m, volume, params, level=level)
        assert float(got.abs().max()) > 0
        for t in _THICKS:
            idx = torch.tensor([k for k, v in enumerate(thick) if v == t], device=device)
            one = svr.evaluate(theta[idx], images[idx].contiguous(), m[idx].contiguous(), volume, dict(params, s_thick=t), level=level)
            assert torch.equal(got[idx], one), (level, t)
        monkeypatch.setenv("NESVOR_SVR", "composed")
        composed = svr.evaluate(theta, images, m, volume, params, level=level)
        monkeypatch.delenv("NESVOR_SVR")
        assert float((got - composed).abs().max()) <= 1e-5
    m2 = m.clone()
    m2[::3] = False  # (a third of the slices have no valid pixel: the descent runs on a subset of the bank's ids)
    out, loss = svr(theta, images, m2, volume, params)
    assert out.shape == theta.shape and bool(torch.isfinite(out).all()) and bool(torch.isfinite(loss).all())
    assert torch.equal(out[::3], theta[::3]) and not torch.equal(out, theta)
