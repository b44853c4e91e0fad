"""The acquisition operators of csrc/slice_acq.hip - A, A^T and both backwards, fp32 and fp64 - against oracle/slice_acq.py
evaluated in the same dtype, at geometric edges: odd / tiny / one-row volumes and slices, pixel sizes below and above one voxel,
exactly one workgroup of pixels and one pixel more, PSFs with even dimensions and with 1024 / 1088 taps, slices wholly and half
outside the volume, many small slices and a single one, empty stacks; every output element written; refusals before a launch.

Two sets of poses per geometry.  LATTICE: matrix entries 0 or +-1 and dyadic translations, so every coordinate is exact in fp32:
kernel and oracle take identical ``floor`` and bounds decisions, tap positions fall exactly on voxel boundaries, and the sets
of valid pixels / voxels must be EQUAL.  GENERIC: seeded random poses as in tests/test_gpu_ops.py::_sa_setup; the seeds are
fixed so that the oracle in fp32 agrees with the oracle in fp64 within the asserted tolerance on every element (asserted: a
boundary flip of the reference's own is kept out of the inputs).

Every tolerance is that of the existing test of the same operator in tests/test_gpu_ops.py (TOL32, TOL64 below); none is
fitted to the kernels."""
import types

import pytest
import torch

from acq_geometry import BIG_PSFS, GEOMETRIES, OUTSIDE, TOL32, _generic_poses, _lattice_poses, _psf

pytestmark = pytest.mark.gpu

# generic poses: seed per (geometry, masks); checked on the CPU: the fp32 oracle agrees with the fp64 oracle within TOL32
GENERIC_SEEDS = {(g, m): 100 + 10 * i + int(m) for i, g in enumerate(GEOMETRIES) for m in (False, True)}
BIG_SEEDS = {"psf1688": 171, "psf1788": 172}
MANY = 300  # slices of (2,2) on the "odd" volume: one workgroup per slice in the per-slice kernels, three of its waves idle
INVALID = 1  # hipErrorInvalidValue

# TOL32: (rtol, atol as a fraction of 1, atol as a fraction of the reference's largest magnitude), from tests/test_gpu_ops.py
# (tests/acq_geometry.py); TOL64: test_slice_acq_double_precision_all_four_entry_points (fp64)
TOL64 = {"slices": (1e-10, 1e-12, 0), "weight": (1e-10, 1e-12, 0), "adjoint": (1e-10, 1e-12, 0), "adjoint_weight": (1e-10, 1e-12, 0),
         "grad_vol": (1e-9, 1e-11, 0), "grad_transforms": (0, 0, 1e-9), "grad_slices": (1e-9, 1e-11, 0), "adjoint_grad_transforms": (0, 0, 1e-9)}
_DATA = {}


def _inputs(dims, shape, tf, psf, masks, g):
    """fp32 inputs on the CPU, shared by both dtypes (the fp64 runs take them converted) and never written.  Masks: about 70 %
    each, slice 1 fully masked.  grad_slices carries exact zeros (skipped by the reference)."""
    n = tf.shape[0]
    c = dict(dims=dims, shape=shape, tf=tf.contiguous(), psf=psf, vol=torch.rand((1, 1) + dims, generator=g),
             y=torch.rand((n, 1) + shape, generator=g), g=torch.randn((n, 1) + shape, generator=g), G=torch.randn((1, 1) + dims, generator=g),
             vm=None, sm=None)
    c["g"][0, 0, 0, :3] = 0
    if masks:
        c["vm"] = torch.rand((1, 1) + dims, generator=g) < 0.7
        c["sm"] = torch.rand((n, 1) + shape, generator=g) < 0.7
        if n > 1:
            c["sm"][1] = False
    return c


def _case(geom, poses, masks):
    key = ("case", geom, poses, masks)
    if key not in _DATA:
        dims, shape, res, psf = GEOMETRIES[geom]
        g = torch.Generator().manual_seed(GENERIC_SEEDS[(geom, masks)])
        tf = _lattice_poses(dims) if poses == "lattice" else _generic_poses(6, g)
        _DATA[key] = dict(_inputs(dims, shape, tf, _psf(psf), masks, g), res=res, key=key)
    return _DATA[key]


def _to(c, dtype):
    f = lambda t: t.to(dtype)
    return dict(c, tf=f(c["tf"]), psf=f(c["psf"]), vol=f(c["vol"]), y=f(c["y"]), g=f(c["g"]), G=f(c["G"]))


def _oracle(c, dtype, forward_only=False):
    """All four operators of the oracle in ``dtype`` (the adjoint and its backward with and without equalisation), once per case."""
    from oracle import slice_acq as O

    key = ("oracle", c["key"], dtype, forward_only)
    if key in _DATA:
        return _DATA[key]
    d = _to(c, dtype)
    tf, psf, vm, sm, res, dims = d["tf"], d["psf"], d["vm"], d["sm"], d["res"], d["dims"]
    out = {}
    out["slices"], out["weight"] = O.slice_acquisition_forward(tf, d["vol"], vm, sm, psf, d["shape"], res, True, False)
    if not forward_only:
        out["grad_vol"], out["grad_transforms"] = O.slice_acquisition_backward(tf, d["vol"], vm, psf, d["g"], sm, res)
        for eq in (False, True):
            v, w = O.slice_acquisition_adjoint_forward(tf, psf, d["y"], sm, vm, dims, res, False, eq)
            gs, gt = O.slice_acquisition_adjoint_backward(tf, d["G"], w if eq else None, vm, psf, d["y"], sm, v if eq else None, res, False, eq)
            out["adjoint", eq], out["adjoint_weight", eq], out["grad_slices", eq], out["adjoint_grad_transforms", eq] = v, w, gs, gt
        R, _, centre = O._geometry(tf, dims, d["shape"], res, dtype)
        out["psf_weight"] = O._psf_weight(R, centre, psf, dims).view(-1, 1, *d["shape"])
    _DATA[key] = out
    return out


def _kernels(device, c, dtype, oracle, forward_only=False):
    """The same through nesvor_amd.slice_acq_cuda.  The backward of A^T takes the oracle's vol / vol_weight when equalising, as
    the existing tests do."""
    from nesvor_amd import slice_acq_cuda as K

    d = _to(c, dtype)
    e = torch.empty(0, device=device)
    dev = lambda t: e if t is None else t.to(device)
    tf, psf, vm, sm, res, dims = dev(d["tf"]), dev(d["psf"]), dev(d["vm"]), dev(d["sm"]), d["res"], d["dims"]
    out = {}
    s, w = K.forward(tf, dev(d["vol"]), vm, sm, psf, d["shape"], res, True, False)
    assert s.dtype == dtype
    out["slices"], out["weight"] = s.cpu(), w.cpu()
    if not forward_only:
        gv, gt = K.backward(tf, dev(d["vol"]), vm, psf, dev(d["g"]), sm, res, False, True, True)
        out["grad_vol"], out["grad_transforms"] = gv.cpu(), gt.cpu()
        for eq in (False, True):
            v, w = K.adjoint_forward(tf, psf, dev(d["y"]), sm, vm, dims, res, False, eq)
            assert (w.numel() > 0) == eq
            gs, gt = K.adjoint_backward(tf, dev(d["G"]).clone(), dev(oracle["adjoint_weight", eq]) if eq else None, vm, psf, dev(d["y"]), sm,
                                        dev(oracle["adjoint", eq]) if eq else None, res, False, eq, True, True)
            out["adjoint", eq], out["adjoint_weight", eq] = v.cpu(), (w.cpu() if eq else None)
            out["grad_slices", eq], out["adjoint_grad_transforms", eq] = gs.cpu(), gt.cpu()
    return out


def _within(got, ref, tol):
    rtol, atol, arel = tol
    bound = rtol * ref.abs() + atol + arel * float(ref.abs().max()) if ref.numel() else ref.abs()
    err = (got - ref).abs()
    return bool((err <= bound).all()), (float((err - bound).max()) if ref.numel() else 0.0)


def _compare(got, ref, tols, what):
    for name, r in ref.items():
        if r is None or name == "psf_weight":
            continue
        base = name[0] if isinstance(name, tuple) else name
        ok, excess = _within(got[name].double(), r.double(), tols[base])
        assert ok, (what, name, "excess over the bound", excess, "range", float(r.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# all four operators on every geometry
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("masks", [False, True], ids=["nomask", "masks"])
@pytest.mark.parametrize("poses", ["lattice", "generic"])
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_operators_on_every_geometry(device, geom, poses, masks, dtype):
    """A (with weight), its backward, A^T with and without ``equalize`` and its backward against the oracle in ``dtype``, at the
    bounds of the existing tests (TOL64 / TOL32).
    Lattice poses: the slice 100 voxels outside has no valid pixel and - asserted on the oracle so that a case cannot
    silently become empty - the other slices together keep at least 5 % of theirs and identity, rotation, permutation and the
    half-outside slice each keep some (the rotated one-row slice keeps 3 %); in fp32 the valid sets
    (weight > 0, A^T's vol_weight > 0) are EQUAL to the oracle's, and the outside slice gives exact zeros in slices, weight,
    grad_slices and both grad_transforms rows and, acquired alone, a zero A^T, vol_weight and grad_vol.
    Generic poses in fp32: the oracle in fp32 must itself agree with the oracle in fp64 within TOL32 (a fixed seed keeps the
    reference's own boundary flips out of the inputs).
    Without masks, in fp64: <A x, y keep> = <x, A^T (y keep)> on the device to 1e-10, keep = the oracle's PSF weight >= 0.5."""
    c = _case(geom, poses, masks)
    ref = _oracle(c, dtype)
    tols = TOL64 if dtype == torch.float64 else TOL32
    if poses == "lattice":
        valid = (_oracle(c, torch.float64)["psf_weight"] > 0).flatten(1).double().mean(1)
        others = [k for k in range(6) if k != OUTSIDE]
        some = [0, 1, 2, 5]  # (the (0.5, -1, 2) move leaves the (2,2,2) volume: z = 2.5 >= D - 1)
        assert float(valid[OUTSIDE]) == 0 and float(valid[others].mean()) >= 0.05 and bool((valid[some] > 0).all()), valid
    elif dtype == torch.float32:
        _compare(ref, _oracle(c, torch.float64), TOL32, "fp32 oracle against fp64 oracle")
    got = _kernels(device, c, dtype, ref)
    _compare(got, ref, tols, (geom, poses, masks))
    if masks:
        assert float(got["slices"][~c["sm"]].abs().max()) == 0 and float(got["grad_slices", False][~c["sm"]].abs().max()) == 0
    if poses == "lattice":
        for name in ("slices", "weight", ("grad_slices", False), ("grad_slices", True), "grad_transforms", ("adjoint_grad_transforms", False),
                     ("adjoint_grad_transforms", True)):
            assert float(got[name][OUTSIDE].abs().max()) == 0, name
        if dtype == torch.float32:
            assert torch.equal(got["weight"] > 0, ref["weight"] > 0)
            assert torch.equal(got["adjoint_weight", True] > 0, ref["adjoint_weight", True] > 0)
        # the outside slice alone: A^T and the volume's gradient are the zero volume
        from nesvor_amd import slice_acq_cuda as K

        d = _to(c, dtype)
        e = torch.empty(0, device=device)
        one = slice(OUTSIDE, OUTSIDE + 1)
        tf1, psf, vol = d["tf"][one].to(device), d["psf"].to(device), d["vol"].to(device)
        v1, w1 = K.adjoint_forward(tf1, psf, d["y"][one].to(device), e, e, d["dims"], d["res"], False, True)
        gv1, gt1 = K.backward(tf1, vol, e, psf, d["g"][one].to(device), e, d["res"], False, True, True)
        for out in (v1, w1, gv1, gt1):
            assert float(out.abs().max()) == 0
    if not masks and dtype == torch.float64:
        from nesvor_amd import slice_acq_cuda as K

        d = _to(c, dtype)
        e = torch.empty(0, device=device)
        keep = (ref["psf_weight"] >= 0.5).to(dtype)
        Ax = got["slices"]
        Aty = K.adjoint_forward(d["tf"].to(device), d["psf"].to(device), (d["y"] * keep).to(device), e, e, d["dims"], d["res"], False, False)[0].cpu()
        lhs, rhs = float((Ax * d["y"] * keep).sum()), float((d["vol"] * Aty).sum())
        assert abs(lhs - rhs) <= 1e-10 * abs(lhs), (lhs, rhs)
        assert lhs != 0


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("psf", BIG_PSFS)
def test_forward_at_the_tap_list_limit(device, psf, dtype):
    """(16,8,8) = 1024 taps fill the forward's LDS tap list to its last entry; (17,8,8) = 1088 take the global-memory walk.  Forward
    only (the oracle's other operators cost seconds at this size), the six lattice and six generic poses in one stack."""
    key = ("case", "big", psf)
    if key not in _DATA:
        dims, shape, res, _ = GEOMETRIES["even"]
        g = torch.Generator().manual_seed(BIG_SEEDS[psf])
        tf = torch.cat([_lattice_poses(dims), _generic_poses(6, g)])
        _DATA[key] = dict(_inputs(dims, shape, tf, _psf(psf), False, g), res=res, key=key)
    c = _DATA[key]
    assert (c["psf"].numel() <= 1024) == (psf == "psf1688") and bool((c["psf"] != 0).all())
    ref = _oracle(c, dtype, forward_only=True)
    assert float(ref["weight"][OUTSIDE].abs().max()) == 0 and float((ref["weight"] > 0).double().mean()) > 0.3
    if dtype == torch.float32:
        _compare(ref, _oracle(c, torch.float64, forward_only=True), TOL32, "fp32 oracle against fp64 oracle")
    got = _kernels(device, c, dtype, ref, forward_only=True)
    _compare(got, ref, TOL64 if dtype == torch.float64 else TOL32, psf)
    assert float(got["slices"][OUTSIDE].abs().max()) == 0 and float(got["weight"][OUTSIDE].abs().max()) == 0
    if dtype == torch.float32:
        assert torch.equal(got["weight"][:6] > 0, ref["weight"][:6] > 0)


# ---------------------------------------------------------------------------------------------------------------------
# stack sizes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [1, MANY])
def test_stack_sizes(device, n, dtype):
    """One slice, and 300 slices of (2,2) on the (5,7,9) volume (a workgroup per slice with three idle waves in the per-slice
    kernels; more slices than pixels per slice in the voxel gather).  Lattice poses - the three rotations in turn, translations
    drawn from the multiples of 1/4 in [-3, 3] - so that fp32 decisions are the oracle's; masks on."""
    key = ("case", "stack", n)
    if key not in _DATA:
        dims, _, res, psf = GEOMETRIES["odd"]
        g = torch.Generator().manual_seed(180 + n)
        rots = _lattice_poses(dims)[:3, :, :3]
        t = torch.randint(-12, 13, (n, 3), generator=g).float() / 4
        tf = torch.cat([rots[torch.arange(n) % 3], t[:, :, None]], 2)
        _DATA[key] = dict(_inputs(dims, (2, 2) if n > 1 else (7, 9), tf, _psf(psf), True, g), res=res, key=key)
    c = _DATA[key]
    ref = _oracle(c, dtype)
    share = float((ref["weight"] > 0).double().mean())
    assert 0.05 <= share <= 0.9, share
    got = _kernels(device, c, dtype, ref)
    _compare(got, ref, TOL64 if dtype == torch.float64 else TOL32, ("stack", n))
    if dtype == torch.float32:
        assert torch.equal(got["weight"] > 0, ref["weight"] > 0)


# ---------------------------------------------------------------------------------------------------------------------
# the C ABI: every element written, empty stacks, refusals
# ---------------------------------------------------------------------------------------------------------------------
def _abi(device, c, dtype):
    """The linear-mode entry points of one dtype as closures over a case's device tensors; outputs and dimensions by keyword."""
    from nesvor_amd import _lib

    lib, P = _lib.load(), _lib.ptr
    sfx = "_f64" if dtype == torch.float64 else ""
    d = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in _to(c, dtype).items()}
    D, H, W = c["dims"]
    dp, hp, wp = c["psf"].shape
    n, (h, w) = c["tf"].shape[0], c["shape"]
    scratch = torch.empty(max(2 * n * h * w, 1), dtype=dtype, device=device)
    vw, v = torch.rand((1, 1, D, H, W), dtype=dtype, device=device) + 0.5, torch.rand((1, 1, D, H, W), dtype=dtype, device=device)
    res = float(c["res"])

    def forward(slices, weight, D=D, H=H, W=W, n=n, h=h, w=w):
        return getattr(lib, "nesvor_slice_acq_forward" + sfx)(P(d["tf"]), P(d["vol"]), P(d["vm"]), P(d["sm"]), P(d["psf"]), P(slices), P(weight),
                                                              D, H, W, dp, hp, wp, n, h, w, res, 0, _lib.stream_ptr())

    def adjoint_forward(vol, vol_weight, equalize=1, D=D, H=H, W=W, n=n, h=h, w=w):
        return getattr(lib, "nesvor_slice_acq_adjoint_forward" + sfx)(P(d["tf"]), P(d["psf"]), P(d["y"]), P(d["sm"]), P(d["vm"]), P(vol),
                                                                      P(vol_weight), P(scratch), D, H, W, dp, hp, wp, n, h, w, res, equalize,
                                                                      _lib.stream_ptr())

    def backward(grad_vol, grad_tf, D=D, H=H, W=W, n=n, h=h, w=w):
        return getattr(lib, "nesvor_slice_acq_backward" + sfx)(P(d["tf"]), P(d["vol"]), P(d["vm"]), P(d["psf"]), P(d["g"]), P(d["sm"]),
                                                               P(grad_vol), P(grad_tf), P(scratch), D, H, W, dp, hp, wp, n, h, w, res,
                                                               _lib.stream_ptr())

    def adjoint_backward(grad_slices, grad_tf, equalize=0, D=D, H=H, W=W, n=n, h=h, w=w):
        G = d["G"].clone()
        return getattr(lib, "nesvor_slice_acq_adjoint_backward" + sfx)(P(d["tf"]), P(G), P(vw if equalize else None), P(d["vm"]), P(d["psf"]),
                                                                       P(d["y"]), P(d["sm"]), P(v if equalize else None), P(grad_slices),
                                                                       P(grad_tf), D, H, W, dp, hp, wp, n, h, w, res, equalize,
                                                                       _lib.stream_ptr())

    # interp_psf mode: same arguments without the scratch buffer
    def adjoint_forward_interp(vol, vol_weight, D=D, H=H, W=W):
        return getattr(lib, "nesvor_slice_acq_adjoint_forward_interp" + sfx)(P(d["tf"]), P(d["psf"]), P(d["y"]), P(d["sm"]), P(d["vm"]), P(vol),
                                                                             P(vol_weight), D, H, W, dp, hp, wp, n, h, w, res, 1, _lib.stream_ptr())

    def backward_interp(grad_vol, grad_tf, D=D, H=H, W=W):
        return getattr(lib, "nesvor_slice_acq_backward_interp" + sfx)(P(d["tf"]), P(d["vol"]), P(d["vm"]), P(d["psf"]), P(d["g"]), P(d["sm"]),
                                                                      P(grad_vol), P(grad_tf), D, H, W, dp, hp, wp, n, h, w, res, _lib.stream_ptr())

    def adjoint_backward_interp(grad_slices, grad_tf, D=D, H=H, W=W):
        G = d["G"].clone()
        return getattr(lib, "nesvor_slice_acq_adjoint_backward_interp" + sfx)(P(d["tf"]), P(G), P(vw), P(d["vm"]), P(d["psf"]), P(d["y"]), P(d["sm"]),
                                                                              P(v), P(grad_slices), P(grad_tf), D, H, W, dp, hp, wp, n, h, w, res,
                                                                              1, _lib.stream_ptr())

    full = lambda *shape: torch.full(shape, -7.0, dtype=dtype, device=device)
    return types.SimpleNamespace(forward=forward, adjoint_forward=adjoint_forward, backward=backward, adjoint_backward=adjoint_backward,
                           adjoint_forward_interp=adjoint_forward_interp, backward_interp=backward_interp,
                           adjoint_backward_interp=adjoint_backward_interp, full=full, n=n, h=h, w=w, dims=(D, H, W), tensors=d)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_every_output_element_is_written(device, dtype):
    """Linear mode through the C ABI with the outputs pre-filled with -7: after a legal call no sentinel is left in grad_vol,
    vol, vol_weight or either grad_transforms (``ops`` allocates them uninitialised), and they are what the ops return.  On
    the "sparse" geometry with generic poses and masks: masked voxels, voxels no slice reaches and a fully masked slice."""
    from nesvor_amd import slice_acq_cuda as K

    c = _case("sparse", "generic", True)
    a = _abi(device, c, dtype)
    t = a.tensors
    D, H, W = a.dims
    gv, gt = a.full(1, 1, D, H, W), a.full(a.n, 3, 4)
    assert a.backward(gv, gt) == 0
    vol, vw = a.full(1, 1, D, H, W), a.full(1, 1, D, H, W)
    assert a.adjoint_forward(vol, vw) == 0
    vol0 = a.full(1, 1, D, H, W)
    assert a.adjoint_forward(vol0, None, equalize=0) == 0
    gs, gt2 = torch.zeros((a.n, 1, a.h, a.w), dtype=dtype, device=device), a.full(a.n, 3, 4)  # (grad_slices: zero-filled by the caller)
    assert a.adjoint_backward(gs, gt2) == 0
    torch.cuda.synchronize()
    for name, out in (("grad_vol", gv), ("grad_transforms", gt), ("vol", vol), ("vol_weight", vw), ("vol, not equalised", vol0),
                      ("adjoint grad_transforms", gt2)):
        assert not bool((out == -7.0).any()), name
        assert bool(torch.isfinite(out).all()), name
    assert float(gt[1].abs().max()) == 0 and float(gt2[1].abs().max()) == 0  # the fully masked slice
    assert float(gv[~t["vm"]].abs().max()) == 0 and float(vol[~t["vm"]].abs().max()) == 0
    gv_op, gt_op = K.backward(t["tf"], t["vol"], t["vm"], t["psf"], t["g"], t["sm"], c["res"], False, True, True)
    assert torch.equal(gv, gv_op) and torch.equal(gt, gt_op)
    v_op, w_op = K.adjoint_forward(t["tf"], t["psf"], t["y"], t["sm"], t["vm"], c["dims"], c["res"], False, True)
    assert torch.equal(vol, v_op) and torch.equal(vw, w_op)
    gs_op, gt2_op = K.adjoint_backward(t["tf"], t["G"].clone(), None, t["vm"], t["psf"], t["y"], t["sm"], None, c["res"], False, False, True, True)
    assert torch.equal(gs, gs_op) and torch.equal(gt2, gt2_op)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_empty_stack_gives_zero_gradients(device, dtype):
    """No launch happens for n h w = 0, and what the gradients' buffers held must not reach autograd: through the C ABI the
    sentinel-filled grad_vol / grad_transforms come back as exact zeros (n = 0; h = 0 with n = 6 for both grad_transforms);
    A^T of an empty stack is the zero volume; through the ops and through autograd (``slice_acquisition`` with
    ``transforms[:0]``) the volume's gradient is all zero - the allocator is first handed a block of sevens to give back."""
    from nesvor_amd import slice_acq_cuda as K
    from nesvor_amd.slice_acquisition import slice_acquisition

    c = _case("odd", "generic", False)
    a = _abi(device, c, dtype)
    t = a.tensors
    D, H, W = a.dims
    gv, gt = a.full(1, 1, D, H, W), a.full(a.n, 3, 4)
    assert a.backward(gv, gt, n=0) == 0
    torch.cuda.synchronize()
    assert float(gv.abs().max()) == 0 and bool((gt == -7.0).all())  # (n = 0: grad_transforms has no row)
    gv, gt = a.full(1, 1, D, H, W), a.full(a.n, 3, 4)
    assert a.backward(gv, gt, h=0) == 0
    gt2 = a.full(a.n, 3, 4)
    assert a.adjoint_backward(None, gt2, h=0) == 0
    gt3 = a.full(a.n, 3, 4)
    assert a.adjoint_backward(None, gt3, w=0, equalize=1) == 0
    vol, vw = a.full(1, 1, D, H, W), a.full(1, 1, D, H, W)
    assert a.adjoint_forward(vol, vw, n=0) == 0
    torch.cuda.synchronize()
    for out in (gv, gt, gt2, gt3, vol, vw):
        assert float(out.abs().max()) == 0
    # the ops and autograd
    e = torch.empty(0, device=device)
    sevens = lambda: [torch.full_like(t["vol"], 7.0) for _ in range(8)]
    junk = sevens()
    del junk
    g0 = torch.zeros((0, 1) + c["shape"], dtype=dtype, device=device)
    gv_op, gt_op = K.backward(t["tf"][:0].contiguous(), t["vol"], e, t["psf"], g0, e, c["res"], False, True, True)
    assert gv_op.shape == t["vol"].shape and float(gv_op.abs().max()) == 0 and (gt_op is None or gt_op.numel() == 0)
    junk = sevens()
    del junk
    y0 = torch.zeros((6, 1, 0, 4), dtype=dtype, device=device)
    gs_op, gt_op = K.adjoint_backward(t["tf"], t["G"].clone(), None, e, t["psf"], y0, e, None, c["res"], False, False, True, True)
    assert gt_op.shape == (6, 3, 4) and float(gt_op.abs().max()) == 0
    junk = sevens()
    del junk
    vol = t["vol"].clone().requires_grad_(True)
    tf0 = t["tf"][:0].contiguous().requires_grad_(True)
    out = slice_acquisition(tf0, vol, None, None, t["psf"], c["shape"], c["res"], False, False)
    assert out.shape == (0, 1) + c["shape"]
    out.sum().backward()
    assert vol.grad is not None and float(vol.grad.abs().max()) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_refusals_before_launch(device, dtype):
    """The kernels index voxels with int, so every entry point - linear and interp_psf mode - returns hipErrorInvalidValue for
    D H W > INT_MAX before anything is launched or cleared: small real buffers, only the dimensions lie (as
    tests/test_gpu_bias.py::test_refusals), and the sentinel-filled outputs are untouched.  A legal call then succeeds."""
    c = _case("odd", "generic", True)
    a = _abi(device, c, dtype)
    D, H, W = a.dims
    outs = {name: a.full(1, 1, D, H, W) for name in ("gv", "vol", "vw", "gvi", "voli", "vwi")}
    outs.update({name: a.full(a.n, 3, 4) for name in ("gt", "gt2", "gti", "gt2i")})
    outs.update({name: a.full(a.n, 1, a.h, a.w) for name in ("s", "sw", "gs", "gsi")})
    big = [dict(D=2048, H=1024, W=1024), dict(D=1, H=2, W=2 ** 30), dict(D=65536, H=65536, W=1)]
    for bad in big:
        assert a.forward(outs["s"], outs["sw"], **bad) == INVALID, bad
        assert a.adjoint_forward(outs["vol"], outs["vw"], **bad) == INVALID, bad
        assert a.backward(outs["gv"], outs["gt"], **bad) == INVALID, bad
        assert a.adjoint_backward(outs["gs"], outs["gt2"], **bad) == INVALID, bad
        assert a.adjoint_backward(outs["gs"], outs["gt2"], equalize=1, **bad) == INVALID, bad
        assert a.adjoint_forward_interp(outs["voli"], outs["vwi"], **bad) == INVALID, bad
        assert a.backward_interp(outs["gvi"], outs["gti"], **bad) == INVALID, bad
        assert a.adjoint_backward_interp(outs["gsi"], outs["gt2i"], **bad) == INVALID, bad
        # ... also where nothing would be launched
        assert a.backward(outs["gv"], outs["gt"], n=0, **bad) == INVALID and a.adjoint_backward(outs["gs"], outs["gt2"], h=0, **bad) == INVALID
    torch.cuda.synchronize()
    for name, out in outs.items():
        assert bool((out == -7.0).all()), name
    assert a.forward(outs["s"], outs["sw"]) == 0 and a.adjoint_forward(outs["vol"], outs["vw"]) == 0
    assert a.backward(outs["gv"], outs["gt"]) == 0 and a.adjoint_backward(outs["gs"], outs["gt2"]) == 0
    torch.cuda.synchronize()
    for name in ("vol", "vw", "gv", "gt", "gt2"):
        assert not bool((outs[name] == -7.0).any()), name
