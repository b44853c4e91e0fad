"""Bias field correction on the GPU: the three fused ops (csrc/bias.hip) against the composed float64 expressions of
nesvor_amd/bias.py on the same fp32 inputs at wave and row edges, their reproducibility and refusals, the wrapper's choice of
path, a whole correction on both paths, and the command line."""
import math
import os

import pytest
import torch

# (D, H, W): rows of 1, 63, 64, 65 voxels (inside / at / past one wave), 257 (five chunks), several rows per workgroup and more
# rows than one workgroup takes (four); 22 x 40 x 40 is the stack of the end-to-end test
SHAPES = [(1, 1, 1), (2, 3, 63), (2, 3, 64), (2, 3, 65), (3, 4, 257), (5, 7, 33), (22, 40, 40)]
SPANS = [1, 2, 8]
KINDS = ["none", "bool", "uint8"]
N_BINS = 200
# |fused - composed fp64| of the fitted lattice and of the updated field f on the cases above (the lattice passes through the
# lookup table and a division of two sums, f through the fp32 tables and its own fp32 rounding).  Measured on MI355X (DESIGN.md
# §4, "Bias field correction"): the largest differences over all cases are LATTICE_MEASURED and F_MEASURED; asserted at 4 x
# that, rounded up to a power of ten (the SCORE_TOL convention of tests/test_gpu_assess.py).
LATTICE_MEASURED, LATTICE_TOL = 5.251e-9, 1e-7  # (5, 7, 33), S = 8, bool / uint8 mask
F_MEASURED, F_TOL = 1.505e-8, 1e-7  # (3, 4, 257), S = 8, bool / uint8 mask
# the same for the field of a whole correction (40 iterations, tol = 0) of the (22,1,40,40) stack below
E2E_MEASURED, E2E_TOL = 3.462e-8, 1e-6
_DATA = {}


def _case(shape, S, kind, device, n_bins=N_BINS):
    """v = 1 + 0.5 randn, f = 0.1 randn, a mask of about 70 % with an empty row, an empty slice (D >= 2) and, for S >= 2, an empty
    span cell (0, 0, 0); a range a little inside the extremes of u (so c is clamped at both ends), the sharpened lookup table of
    the composed histogram, the level's tables, and the composed results.  Shared by the tests and never written."""
    key = (shape, S, kind, n_bins)
    if key in _DATA:
        return _DATA[key]
    from nesvor_amd import bias

    g = torch.Generator().manual_seed(1000 * shape[0] + 10 * shape[2] + S)
    v = (1 + 0.5 * torch.randn(shape, generator=g)).to(device)
    f = (0.1 * torch.randn(shape, generator=g)).to(device)
    tables = bias.LevelTables(shape, S, device)
    mask = None
    if kind != "none":
        mask = (torch.rand(shape, generator=g) < 0.7).to(device)
        mask[0, 0, :] = False
        if shape[0] >= 2:
            mask[-1] = False
        if S >= 2:
            sz, sy, sx = tables.span
            mask &= ~((sz == 0)[:, None, None] & (sy == 0)[None, :, None] & (sx == 0)[None, None, :])
        if kind == "uint8":
            mask = mask.to(torch.uint8) * 3  # any set byte counts
    u = v.double() - f.double()
    width = u.max() - u.min()
    rng = torch.stack([u.min() + 0.02 * width - 0.01, u.max() - 0.02 * width + 0.01]).float()
    hist = bias.histogram_composed(v, f, mask, rng, n_bins)
    lut = bias.sharpen_lut(hist, rng)
    lattice, weight = bias.fit_composed(v, f, mask, rng, lut, tables)
    f_new, stats = bias.update_composed(lattice, tables, f, v, mask)
    _DATA[key] = dict(v=v, f=f, mask=mask, rng=rng, tables=tables, hist=hist, lut=lut, lattice=lattice, weight=weight, f_new=f_new,
                      stats=stats, n_bins=n_bins)
    return _DATA[key]


def _fit(c):
    t = c["tables"]
    return torch.ops.nesvor.n4_fit(c["v"], c["f"], c["mask"], c["rng"], c["lut"], *t.basis32, *t.span, t.S)


def _update(c, f):
    t = c["tables"]
    return torch.ops.nesvor.n4_update_(c["lattice"], *t.basis32, *t.span, t.S, f, c["v"], c["mask"])


# ---------------------------------------------------------------------------------------------------------------------
# the ops against the composed expressions
# ---------------------------------------------------------------------------------------------------------------------
def _check_histogram(c):
    """The kernel forms u, slope and c in double exactly as the expression does; a voxel's two weights are rounded to the
    fixed-point quantum 2^-32 (at most 2^-33 each) and added as integers, the per-workgroup bins as integers too, so a bin is
    within 2^-33 x (voxels that touch it) <= 2^-33 count of the fp64 sum, plus the expression's own fp64 rounding; asserted at
    2^-32 count.  Every voxel adds exactly 2^32 quanta: the total is the count (exactly, below 2^53 quanta per bin)."""
    got = torch.ops.nesvor.n4_histogram(c["v"], c["f"], c["mask"], c["rng"], c["n_bins"])
    ref, count = c["hist"], float(c["stats"][0])
    assert got.shape == (c["n_bins"],) and got.dtype == torch.float64 and bool((got >= 0).all())
    worst = float((got - ref).abs().max())
    assert worst <= 2.0 ** -32 * max(count, 1.0)
    assert abs(float(got.sum()) - count) <= 1e-9 * max(count, 1.0) and abs(float(ref.sum()) - count) <= 1e-9 * max(count, 1.0)
    return worst


def _check_fit(c):
    """The divisor ``weight`` = sum_p wz^2 wy^2 wx^2 has non-negative terms.  The fp32 tables carry one rounding per weight (2^-24
    relative), so six for the product of three squares; the kernel squares wx in fp32 (one more) and adds at most 64 such terms
    in fp32 inside a wave (at most 64 x 2^-24 of the sum); everything else is double.  71 x 2^-24 < 2^-17 of the sum itself.
    Where the composed divisor is 0 no valid voxel reaches the control point and both are exactly 0.  The lattice is a ratio of
    two such sums whose numerator cancels: measured (LATTICE_TOL)."""
    lattice, weight = _fit(c)
    C = c["tables"].C
    assert lattice.shape == weight.shape == (C, C, C) and lattice.dtype == weight.dtype == torch.float64
    assert bool(((weight - c["weight"]).abs() <= 2.0 ** -17 * c["weight"]).all())
    empty = c["weight"] == 0
    assert bool((weight[empty] == 0).all()) and bool((lattice[empty] == 0).all())
    if c["mask"] is not None and c["tables"].S >= 2:
        assert bool(empty[0, 0, 0])  # the empty span cell
    return float((lattice - c["lattice"]).abs().max())


def _check_update(c):
    """count exactly.  With d the increment of a voxel, A = sum_k |lattice_k| w_k (the composed evaluation of the absolute
    lattice) and g = expm1(d): the fp32 tables perturb d by at most 3 x 2^-24 A (asserted with 4, which also covers the double
    rounding), so g by e^d times that, plus 2^-24 |g| for its rounding to fp32; a wave adds 64 such terms in fp32.
      |sum g   - ref| <= 2^-24 sum_p (65 |g| + 4 e^d A)
      |sum g^2 - ref| <= 2^-24 sum_p (67 g^2 + 8 |g| e^d A)     (2 |g| |delta g|, the product's rounding, the wave's sum)
    each with 1 % for the second-order terms.  f and the extremes of u_new = v - f_new differ by the field's difference: measured
    (F_TOL)."""
    from nesvor_amd import bias

    f = c["f"].clone()
    stats = _update(c, f)
    ref = c["stats"]
    assert stats.shape == (5,) and stats.dtype == torch.float64 and f.dtype == torch.float32
    assert float(stats[0]) == float(ref[0])
    valid = bias._valid(c["v"], c["mask"])
    d = bias.evaluate_composed(c["lattice"], c["tables"])[valid]
    A = bias.evaluate_composed(c["lattice"].abs(), c["tables"])[valid]
    g, e = torch.expm1(d).abs(), torch.exp(d)
    bound_g = 1.01 * 2.0 ** -24 * float((65 * g + 4 * e * A).sum())
    bound_gg = 1.01 * 2.0 ** -24 * float((67 * g * g + 8 * g * e * A).sum())
    assert abs(float(stats[1] - ref[1])) <= bound_g and abs(float(stats[2] - ref[2])) <= bound_gg
    worst = float((f.double() - c["f_new"]).abs().max())
    if float(ref[0]) == 0:
        assert float(stats[3]) == math.inf and float(stats[4]) == -math.inf and float(ref[3]) == math.inf
    else:
        assert abs(float(stats[3] - ref[3])) <= F_TOL and abs(float(stats[4] - ref[4])) <= F_TOL
        # ... and they are the extremes of v - f for the f the kernel wrote
        u_new = (c["v"].double() - f.double())[valid]
        assert float(stats[3]) == float(u_new.min()) and float(stats[4]) == float(u_new.max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", SPANS)
@pytest.mark.parametrize("shape", SHAPES)
def test_ops_against_the_composed_expressions_in_fp64(device, shape, S, kind):
    c = _case(shape, S, kind, device)
    h, l, f = _check_histogram(c), _check_fit(c), _check_update(c)
    print(f"{shape} S={S} {kind}: count {int(c['stats'][0])}, largest |fused - composed|: histogram {h:.3e}, lattice {l:.3e}, f {f:.3e}")
    assert l <= LATTICE_TOL and f <= F_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("n_bins", [2, 37, 1024])
def test_ops_at_other_histogram_sizes(device, n_bins):
    c = _case((5, 7, 33), 2, "bool", device, n_bins)
    _check_histogram(c)
    assert _check_fit(c) <= LATTICE_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("S", SPANS)
@pytest.mark.parametrize("shape", SHAPES)
def test_ops_are_reproducible(device, shape, S, kind):
    c = _case(shape, S, kind, device)
    hist = lambda: torch.ops.nesvor.n4_histogram(c["v"], c["f"], c["mask"], c["rng"], c["n_bins"])
    assert torch.equal(hist(), hist())
    (l1, w1), (l2, w2) = _fit(c), _fit(c)
    assert torch.equal(l1, l2) and torch.equal(w1, w2)
    f1, f2 = c["f"].clone(), c["f"].clone()
    s1, s2 = _update(c, f1), _update(c, f2)
    assert torch.equal(f1, f2) and torch.equal(s1, s2)
    assert not torch.equal(f1, c["f"]) or float(c["lattice"].abs().max()) == 0  # in place


# ---------------------------------------------------------------------------------------------------------------------
# refusals through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(device):
    """Every refusal returns before a launch (csrc/bias.hip: the checks are the first statements of the entry points), so the
    sentinels in the outputs stay; a legal call then matches the op."""
    from nesvor_amd import _lib

    lib = _lib.load()
    INVALID = 1  # hipErrorInvalidValue
    D, H, W, S, n_bins = 5, 7, 33, 2, N_BINS
    c = _case((D, H, W), S, "bool", device)
    t = c["tables"]
    P, C = _lib.ptr, S + 3
    hist = torch.full((n_bins,), -7.0, dtype=torch.float64, device=device)
    lattice = torch.full((C, C, C), -7.0, dtype=torch.float64, device=device)
    weight = torch.full((C, C, C), -7.0, dtype=torch.float64, device=device)
    stats = torch.full((5,), -7.0, dtype=torch.float64, device=device)
    f = c["f"].clone()
    nb_h = int(lib.nesvor_n4_histogram_workspace_bytes(D, H, W, n_bins))
    nb_f = int(lib.nesvor_n4_fit_workspace_bytes(D, H, W, S))
    nb_u = int(lib.nesvor_n4_update_workspace_bytes(D, H, W))
    assert nb_h == 8 * n_bins * 5  # ceil(1155 / 256) workgroups
    assert nb_f == 8 * 2 * C * (D * H + D * C) and nb_u == 8 * 5 * 9  # ceil(35 rows / 4) workgroups
    assert lib.nesvor_n4_histogram_workspace_bytes(0, H, W, n_bins) == 0 and lib.nesvor_n4_histogram_workspace_bytes(D, H, W, 1) == 0
    assert lib.nesvor_n4_fit_workspace_bytes(D, H, W, 0) == 0 and lib.nesvor_n4_fit_workspace_bytes(D, H, W, 14) == 0
    assert lib.nesvor_n4_update_workspace_bytes(D, 0, W) == 0
    ws = torch.empty(max(nb_h, nb_f, nb_u) // 8, dtype=torch.float64, device=device)
    tabs = dict(tz=t.basis32[0], ty=t.basis32[1], tx=t.basis32[2], sz=t.span[0], sy=t.span[1], sx=t.span[2])

    def histogram(v=c["v"], f_=c["f"], mask=c["mask"], D_=D, H_=H, W_=W, rng=c["rng"], bins=n_bins, out=hist, ws_=ws, nb=nb_h):
        return lib.nesvor_n4_histogram(P(v), P(f_), P(mask), D_, H_, W_, P(rng), bins, P(out), P(ws_), nb, _lib.stream_ptr())

    def fit(v=c["v"], f_=c["f"], mask=c["mask"], rng=c["rng"], lut=c["lut"], bins=n_bins, D_=D, H_=H, W_=W, S_=S, lat=lattice, wgt=weight,
            ws_=ws, nb=nb_f, **k):
        a = {**tabs, **k}
        return lib.nesvor_n4_fit(P(v), P(f_), P(mask), P(rng), P(lut), bins, P(a["tz"]), P(a["ty"]), P(a["tx"]), P(a["sz"]), P(a["sy"]),
                                 P(a["sx"]), D_, H_, W_, S_, P(lat), P(wgt), P(ws_), nb, _lib.stream_ptr())

    def update(lat=c["lattice"], S_=S, f_=f, v=c["v"], mask=c["mask"], D_=D, H_=H, W_=W, out=stats, ws_=ws, nb=nb_u, **k):
        a = {**tabs, **k}
        return lib.nesvor_n4_update(P(lat), P(a["tz"]), P(a["ty"]), P(a["tx"]), P(a["sz"]), P(a["sy"]), P(a["sx"]), S_, P(f_), P(v),
                                    P(mask), D_, H_, W_, P(out), P(ws_), nb, _lib.stream_ptr())

    big = [dict(D_=2048, H_=1024, W_=1024), dict(D_=1, H_=1, W_=2 ** 31 - 256), dict(D_=65536, H_=65536, W_=1)]  # D H W > INT_MAX - 256
    dims = [dict(D_=0), dict(H_=0), dict(W_=0), dict(D_=-1), dict(W_=-3)] + big
    for call, nb in ((histogram, nb_h), (fit, nb_f), (update, nb_u)):
        assert call(nb=nb - 1) == INVALID and call(nb=0) == INVALID and call(ws_=None) == INVALID  # a short or missing workspace
        for bad in dims:
            assert call(**bad) == INVALID, bad
    for call in (fit, update):
        assert call(S_=0) == INVALID and call(S_=-1) == INVALID and call(S_=14) == INVALID  # C = 17
        for name in tabs:
            assert call(**{name: None}) == INVALID, name
    for call in (histogram, fit):
        assert call(bins=1) == INVALID and call(bins=0) == INVALID and call(bins=1025) == INVALID
        assert call(v=None) == INVALID and call(f_=None) == INVALID and call(rng=None) == INVALID
    assert histogram(out=None) == INVALID
    assert fit(lut=None) == INVALID and fit(lat=None) == INVALID and fit(wgt=None) == INVALID
    assert update(lat=None) == INVALID and update(f_=None) == INVALID and update(v=None) == INVALID and update(out=None) == INVALID
    torch.cuda.synchronize()
    for out in (hist, lattice, weight, stats):
        assert bool((out == -7.0).all())
    assert torch.equal(f, c["f"])
    assert histogram() == 0 and fit() == 0 and update() == 0
    torch.cuda.synchronize()
    assert torch.equal(hist, torch.ops.nesvor.n4_histogram(c["v"], c["f"], c["mask"], c["rng"], n_bins))
    l2, w2 = _fit(c)
    assert torch.equal(lattice, l2) and torch.equal(weight, w2)
    f2 = c["f"].clone()
    assert torch.equal(stats, _update(c, f2)) and torch.equal(f, f2)
    assert histogram(mask=None) == 0 and fit(mask=None) == 0 and update(mask=None) == 0  # (a NULL mask is legal)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# the wrapper
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wrapper_paths_and_fake_kernels(device, monkeypatch):
    from nesvor_amd import bias

    calls = []
    for name in ("histogram_composed", "fit_composed", "update_composed"):
        inner = getattr(bias, name)
        monkeypatch.setattr(bias, name, lambda *a, _inner=inner, _name=name: calls.append(_name) or _inner(*a))
    g = torch.Generator().manual_seed(2)
    img = (torch.rand(6, 1, 12, 20, generator=g) + 0.5).to(device)
    monkeypatch.delenv("NESVOR_BIAS", raising=False)
    kw = dict(n_levels=2, n_iter=3, tol=0.0)
    out, f, info = bias.correct_bias_field(img, None, **kw)
    assert calls == [] and info["fused"] is True and info["iterations"] == [3, 3]
    assert f.dtype == torch.float32 and out.dtype == torch.float32 and out.shape == f.shape == img.shape and out.device == img.device
    assert bias.correct_bias_field(img, None, n_control_points=17, **kw)[2]["fused"] is False  # C > 16: composed
    assert bias.correct_bias_field(img, None, n_bins=2048, **kw)[2]["fused"] is False
    assert bias.correct_bias_field(img.double(), None, **kw)[2]["fused"] is False
    assert bias.correct_bias_field(img.cpu(), None, **kw)[2]["fused"] is False
    calls.clear()
    monkeypatch.setenv("NESVOR_BIAS", "composed")
    out_c, f_c, info_c = bias.correct_bias_field(img, None, **kw)
    assert calls == ["histogram_composed", "fit_composed", "update_composed"] * 6 and info_c["fused"] is False
    assert f_c.dtype == torch.float64 and out_c.dtype == torch.float32 and f_c.device == img.device
    print(f"wrapper: largest |fused - composed| field difference after 6 iterations {float((f.double() - f_c).abs().max()):.3e}")
    assert float((f.double() - f_c).abs().max()) <= E2E_TOL
    monkeypatch.undo()
    # fake kernels
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    tabs = [m(4, 4), m(5, 4), m(6, 4), m(4, dtype=torch.int32), m(5, dtype=torch.int32), m(6, dtype=torch.int32)]
    hist = torch.ops.nesvor.n4_histogram(m(4, 5, 6), m(4, 5, 6), None, m(2), 50)
    assert hist.shape == (50,) and hist.dtype == torch.float64
    lattice, weight = torch.ops.nesvor.n4_fit(m(4, 5, 6), m(4, 5, 6), None, m(2), m(50, dtype=torch.float64), *tabs, 2)
    assert lattice.shape == weight.shape == (5, 5, 5) and lattice.dtype == weight.dtype == torch.float64
    stats = torch.ops.nesvor.n4_update_(m(5, 5, 5, dtype=torch.float64), *tabs, 2, m(4, 5, 6), m(4, 5, 6), None)
    assert stats.shape == (5,) and stats.dtype == torch.float64
    # the ops' own argument checks
    c = _case((5, 7, 33), 2, "bool", device)
    t = c["tables"]
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::n4_histogram'"):
        torch.ops.nesvor.n4_histogram(c["v"].cpu(), c["f"].cpu(), None, c["rng"].cpu(), 50)
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.n4_histogram(c["v"].double(), c["f"], None, c["rng"], 50)
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.nesvor.n4_histogram(c["v"].transpose(0, 1), c["f"].transpose(0, 1), None, c["rng"], 50)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        torch.ops.nesvor.n4_histogram(c["v"], c["f"], c["mask"].float(), c["rng"], 50)
    with pytest.raises(RuntimeError, match="one shape"):
        torch.ops.nesvor.n4_histogram(c["v"], c["f"][:4].contiguous(), None, c["rng"], 50)
    with pytest.raises(RuntimeError, match="n_bins"):
        torch.ops.nesvor.n4_histogram(c["v"], c["f"], None, c["rng"], 1025)
    with pytest.raises(RuntimeError, match="S \\+ 3 <= 16"):
        torch.ops.nesvor.n4_fit(c["v"], c["f"], None, c["rng"], c["lut"], *t.basis32, *t.span, 14)
    with pytest.raises(RuntimeError, match=r"\(n, 4\)"):
        torch.ops.nesvor.n4_fit(c["v"], c["f"], None, c["rng"], c["lut"], t.basis32[1], t.basis32[1], t.basis32[2], *t.span, 2)
    with pytest.raises(RuntimeError, match=r"\(C, C, C\)"):
        torch.ops.nesvor.n4_update_(c["lattice"][:4].contiguous(), *t.basis32, *t.span, 2, c["f"].clone(), c["v"], None)


# ---------------------------------------------------------------------------------------------------------------------
# a whole correction: the 32^3 phantom as a (22,1,40,40) stack under exp(0.35 x - 0.25 y^2 + 0.2 z x + 0.15 z) in index space
# ---------------------------------------------------------------------------------------------------------------------
_RES_S, _THICK = 1.5, 3.0
_STACKS = {}


def _log_field(shape, device):
    axes = [torch.linspace(-1, 1, n, dtype=torch.float64, device=device) for n in shape]
    z, y, x = torch.meshgrid(*axes, indexing="ij")
    return 0.35 * x - 0.25 * y ** 2 + 0.2 * z * x + 0.15 * z


def _biased_stacks(device):
    """Three (22,1,40,40) stacks of the phantom: ``clean`` images, ``biased`` = clean x the field, ``poses``; built once."""
    if not _STACKS:
        from nesvor_amd.phantom import phantom3d, simulate_stacks
        from nesvor_amd.transform import RigidTransform

        vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
        slices, _ = simulate_stacks(vol, 3, res_s=_RES_S, s_thick=_THICK, normalize=False)
        n = len(slices) // 3
        _STACKS["clean"] = [torch.stack([s.image for s in slices[j * n:(j + 1) * n]]).contiguous() for j in range(3)]
        _STACKS["poses"] = [RigidTransform.cat([s.transformation for s in slices[j * n:(j + 1) * n]]) for j in range(3)]
        assert tuple(_STACKS["clean"][0].shape) == (22, 1, 40, 40)
        field = _log_field((22, 40, 40), device)
        _STACKS["field"] = field
        _STACKS["biased"] = [(c.double() * torch.exp(field)[:, None]).float().contiguous() for c in _STACKS["clean"]]
    return _STACKS


def _quality(clean, image, f, true):
    """(std of the field's error over the valid voxels, CV of ``image`` over the largest class, its size).  The class: the voxels
    whose clean value is within 2 % of 0.2, the phantom's largest tissue class (the slices are blurred, not rescaled)."""
    valid = clean > 0
    centred = true - true[valid].mean()
    err = float(((f.double() - f.double()[valid].mean()) - centred)[valid].std())
    cls = (clean - 0.2).abs() <= 0.004
    x = image.double()[cls]
    return err, float(x.std() / x.mean()), int(cls.sum())


@pytest.mark.gpu
def test_whole_correction_on_both_paths(device, monkeypatch):
    """Measured on MI355X: 40 iterations, fused against composed field 3.46e-8 (E2E_TOL); with the defaults
    1, 1, 50 and 32 iterations, the field's error std 0.1305 -> 0.0817, the class's CV 0.1401 -> 0.0608 (185 voxels; 0.0109 on
    the clean stack).  The last two are asserted as relative conditions only: smaller after than before."""
    from nesvor_amd.bias import correct_bias_field

    s = _biased_stacks(device)
    clean, img, true = s["clean"][0], s["biased"][0], s["field"][:, None]
    monkeypatch.delenv("NESVOR_BIAS", raising=False)
    # tol = 0: forty iterations on either path, no stop decision that could flip between precisions
    _, f_fused, info = correct_bias_field(img, None, tol=0.0, n_iter=10)
    assert info["fused"] is True and info["iterations"] == [10] * 4
    monkeypatch.setenv("NESVOR_BIAS", "composed")
    _, f_composed, info_c = correct_bias_field(img, None, tol=0.0, n_iter=10)
    monkeypatch.delenv("NESVOR_BIAS")
    assert info_c["fused"] is False and info_c["iterations"] == [10] * 4 and f_composed.dtype == torch.float64
    worst = float((f_fused.double() - f_composed).abs().max())
    print(f"whole correction, 40 iterations: largest |fused - composed| field difference {worst:.3e} (asserted at {E2E_TOL:g})")
    assert worst <= E2E_TOL
    # defaults: the field is removed
    corrected, f, info = correct_bias_field(img, None)
    again, f2, _ = correct_bias_field(img, None)
    assert torch.equal(corrected, again) and torch.equal(f, f2)
    zero = torch.zeros_like(f)
    err_before, cv_before, size = _quality(clean, img, zero, true)
    err_after, cv_after, _ = _quality(clean, corrected, f, true)
    _, cv_clean, _ = _quality(clean, clean, zero, true)
    print(f"defaults: iterations {info['iterations']}, last cv {info['cv']:.2e}; field error std {err_before:.4f} -> {err_after:.4f}; "
          f"largest class ({size} voxels) CV {cv_before:.4f} -> {cv_after:.4f} (clean stack {cv_clean:.4f})")
    assert err_after < err_before and cv_after < cv_before
    valid = img > 0
    assert abs(float(f.double()[valid].mean())) < 1e-6 and torch.equal(corrected == 0, img == 0)


# ---------------------------------------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------------------------------------
def _nifti_stacks(device, tmp_path):
    from nesvor_amd.image import Stack
    from nesvor_amd.image_io import save_stack
    from nesvor_amd.transform import RigidTransform

    s = _biased_stacks(device)
    paths = []
    for j, (img, pose) in enumerate(zip(s["biased"], s["poses"])):
        st = Stack(img.clone(), img > 0, RigidTransform(pose.matrix().clone()), resolution_x=_RES_S, resolution_y=_RES_S, thickness=_THICK,
                   gap=_THICK)
        paths.append(str(tmp_path / f"stack{j}.nii.gz"))
        save_stack(paths[-1], st)
    return paths


@pytest.mark.gpu
def test_cli_correct_bias_field(tmp_path, device, monkeypatch):
    from nesvor_amd import cli
    from nesvor_amd.bias import correct_bias_field
    from nesvor_amd.image_io import load_stack

    monkeypatch.delenv("NESVOR_BIAS", raising=False)
    paths = _nifti_stacks(device, tmp_path)
    outs = [str(tmp_path / f"corrected{j}.nii.gz") for j in range(3)]
    fields = [str(tmp_path / f"field{j}.nii.gz") for j in range(3)]
    cli.main(["correct-bias-field", "--input-stacks", *paths, "--output-corrected-stacks", *outs, "--output-bias-fields", *fields,
              "--n-levels-n4", "2", "--n-iter-n4", "8", "--verbose", "0"])
    for p, o, fpath in zip(paths, outs, fields):
        st = load_stack(p, device=device)
        corrected, f, _ = correct_bias_field(st.slices, st.mask, n_levels=2, n_iter=8)
        got, got_field = load_stack(o, device=device), load_stack(fpath, device=device)
        assert torch.equal(got.slices, corrected) and torch.equal(got_field.slices, torch.exp(f))
        assert float((got.transformation.matrix() - st.transformation.matrix()).abs().max()) < 1e-5
        assert not torch.equal(got.slices, st.slices)
    cli.main(["correct-bias-field", "--input-stacks", *paths[:1], "--output-corrected-stacks", str(tmp_path / "only.nii.gz"),
              "--n-levels-n4", "1", "--n-iter-n4", "2", "--verbose", "0"])
    assert os.path.exists(str(tmp_path / "only.nii.gz"))
    with pytest.raises(SystemExit, match="output corrected stacks"):
        cli.main(["correct-bias-field", "--input-stacks", *paths, "--output-corrected-stacks", *outs[:2], "--verbose", "0"])


@pytest.mark.gpu
def test_cli_register_with_and_without_the_switch(tmp_path, device, monkeypatch):
    """``register --registration stack``: with ``--bias-field-correction`` the correction is logged and as many slices are
    written; without it the files are, bit for bit, what the command's steps before this switch existed produce - ``load_stack``
    per file, ``cli.register``, ``save_slices`` - restated here."""
    from argparse import Namespace

    from nesvor_amd import bias, cli
    from nesvor_amd.image_io import load_slices, load_stack, save_slices

    monkeypatch.delenv("NESVOR_BIAS", raising=False)
    paths = _nifti_stacks(device, tmp_path)
    corrected = []
    inner = bias.correct_stacks
    monkeypatch.setattr(bias, "correct_stacks", lambda stacks, **kw: corrected.append(len(stacks)) or inner(stacks, **kw))
    common = ["register", "--input-stacks", *paths, "--registration", "stack"]
    on, off, old, log = str(tmp_path / "on"), str(tmp_path / "off"), str(tmp_path / "old"), str(tmp_path / "log.txt")
    cli.main(common + ["--output-slices", on, "--bias-field-correction", "--n-levels-n4", "2", "--n-iter-n4", "8", "--output-log", log])
    text = open(log).read()
    assert corrected == [3] and "Bias field correction, stack 2" in text and "Bias field correction of 3 stacks finished" in text
    cli.main(common + ["--output-slices", off, "--verbose", "0"])
    assert corrected == [3]
    stacks = [load_stack(p, None, device=device) for p in paths]
    slices = cli.register(Namespace(registration="stack", template_stack="0", template_metric="ncc"), stacks)
    os.makedirs(old)
    save_slices(old, slices)
    names = sorted(os.listdir(off))
    assert names == sorted(os.listdir(old)) == sorted(os.listdir(on)) and len(names) > 30
    got_off, got_old, got_on = load_slices(off, device), load_slices(old, device), load_slices(on, device)
    for a, b in zip(got_off, got_old):
        assert torch.equal(a.image, b.image) and torch.equal(a.transformation.matrix(), b.transformation.matrix())
    assert any(not torch.equal(a.image, b.image) for a, b in zip(got_off, got_on))
