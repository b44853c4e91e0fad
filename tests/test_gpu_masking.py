"""GPU: the fused stack masking ops (csrc/masking.hip) against the composed float64 path of nesvor_amd/masking.py, with EXACT
equality of masks, counts, extremes, histograms and thresholds.

Equality is only defined away from decision boundaries, so every comparison first evaluates the boundary condition of
tests/masking_cases.py in float64 on its fixture (no voxel within 1e-3 mm of the boundary of another stack's slabs, no
interpolated mask value within 1e-4 of 0.5, no bin coordinate within 1e-9 of an interior bin edge, no intensity within one fp32
ulp of a threshold, the best Otsu split ahead of the runner-up by more than 1e-9 relative) and ASSERTS that no voxel violates
it: nothing is skipped.  The fixtures were chosen on the CPU so that it holds (tests/test_masking.py asserts the same there).

Shapes: stacks of (1,1,1), (1,16,16), (1,1,257), (2,1,65), (3,33,31) and (4,40,52) pixels - the 255 / 256 / 257-pixel and one-row
edges of the ordered reduction - in scenes of 1, 2 and 3 stacks with different pixel sizes; other stacks of 1, 64, 65 and 130
slices (the 64-row LDS chunks of the slab table), one with per-slice motion; gap > thickness and thickness > gap; a stack wholly
outside the other; a (5,6,7) mask volume at 1.7 mm under a rotated pose with stack voxels off its lattice."""
import json

import numpy as np
import pytest
import torch

import masking_cases as C

_CACHE = {}


def _scene(name, device):
    """The stacks of a scene on the device with their tables; built once, never written."""
    from nesvor_amd.masking import slab_tables

    if name not in _CACHE:
        stacks = C.scene(name, device)
        out = []
        for j, st in enumerate(stacks):
            slabs = dict(zip(("slabs", "slab_extents", "slab_offsets"), slab_tables(stacks, j))) if len(stacks) > 1 else {}
            out.append((st, st.transformation.matrix(True).float().contiguous(), slabs))
        _CACHE[name] = out
    return _CACHE[name]


def _volume(device):
    from nesvor_amd.masking import volume_tables

    if "volume" not in _CACHE:
        _CACHE["volume"] = dict(zip(("volume", "volume_geometry"), volume_tables(C.ball_volume(), device)))
    return _CACHE["volume"]


def _both(slices, mask, T, rx, ry, **rules):
    """One rule set on both paths after the boundary condition; -> the fused (mask, stats), asserted equal to the composed."""
    from nesvor_amd.masking import stack_mask_composed

    violations = C.rule_violations(slices, mask, T, rx, ry, **rules)
    assert not any(violations.values()), violations
    fused = torch.ops.nesvor.stack_mask(slices, mask, T, rx, ry, **rules)
    composed = stack_mask_composed(slices, mask, T, rx, ry, **rules)
    assert fused[0].dtype == torch.uint8 and fused[0].shape == slices.shape and fused[1].dtype == torch.float64
    assert torch.equal(fused[0], composed[0])
    assert torch.equal(fused[1], composed[1]), (fused[1], composed[1])
    again = torch.ops.nesvor.stack_mask(slices, mask, T, rx, ry, **rules)
    assert torch.equal(again[0], fused[0]) and torch.equal(again[1].view(torch.int64), fused[1].view(torch.int64))  # bit-identical runs
    return fused


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(C.SCENES))
def test_rules_equal_the_composed_path(device, name):
    thr = torch.tensor([C.THRESHOLD], dtype=torch.float32, device=device)
    for j, (st, T, slabs) in enumerate(_scene(name, device)):
        rx, ry = st.resolution_x, st.resolution_y
        n_valid = int(st.mask.sum())
        alone, _ = _both(st.slices, st.mask, T, rx, ry, threshold=thr)
        assert 0 < int(alone.sum()) < n_valid or n_valid <= 1
        vol, _ = _both(st.slices, st.mask, T, rx, ry, **_volume(device))
        assert int(vol.sum()) < n_valid
        if slabs:
            both, stats = _both(st.slices, st.mask, T, rx, ry, threshold=thr, **slabs)
            only, _ = _both(st.slices, st.mask, T, rx, ry, **slabs)
            assert int(both.sum()) <= int(only.sum()) < n_valid
            if name == "apart":
                assert int(only.sum()) == 0 and stats[:, 0].sum() == 0 and bool(torch.isinf(stats[:, 1:]).all())
            else:
                assert int(both.sum()) > 0
        if name == "solo":  # all three rules at once are the three rules one after the other
            a, _ = _both(st.slices, st.mask, T, rx, ry, threshold=thr, **_volume(device))
            assert torch.equal(a, alone & vol) and 0 < int(a.sum())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["none", "bool", "uint8"])
def test_incoming_mask_kinds_and_nan_intensities(device, kind):
    st, T, _ = _scene("trio", device)[2]
    _, _, slabs = _scene("trio", device)[2]
    slices = st.slices.clone()
    slices.view(-1)[[5, 300, 1023, 1024, 2000]] = float("nan")
    mask = {"none": None, "bool": st.mask, "uint8": st.mask.to(torch.uint8) * 7}[kind]
    thr = torch.tensor([C.THRESHOLD], dtype=torch.float32, device=device)
    out, stats = _both(slices, mask, T, st.resolution_x, st.resolution_y, threshold=thr, **slabs)
    assert not out.view(-1)[[5, 300, 1023, 1024, 2000]].any() and bool(torch.isfinite(stats[:, 1:]).all())
    # without a threshold a NaN voxel of the mask stays, is counted, and enters neither extreme
    out, stats = _both(slices, mask, T, st.resolution_x, st.resolution_y, **_volume(device))
    assert stats[:, 0].sum() == out.sum() > 0 and not torch.isnan(stats).any()  # (a slice outside the ball: +inf / -inf)
    plain, stats = _both(slices, mask, T, st.resolution_x, st.resolution_y)
    expect = torch.ones_like(plain) if mask is None else (mask != 0).to(torch.uint8)
    assert torch.equal(plain, expect) and bool(torch.isfinite(stats[:, 1:]).all()) and stats[:, 0].sum() == plain.sum()
    assert int(plain.view(-1)[[5, 300, 1023, 1024, 2000]].sum()) == int(expect.view(-1)[[5, 300, 1023, 1024, 2000]].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("name,j,n_bins", C.OTSU_CASES)
def test_otsu_equals_the_composed_path_and_numpy(device, name, j, n_bins):
    from nesvor_amd.masking import otsu_histogram_composed, otsu_threshold_composed, stack_range

    st, T, _ = _scene(name, device)[j]
    violations = C.otsu_violations(st.slices, st.mask, n_bins)
    assert not any(violations.values()), violations
    _, stats = torch.ops.nesvor.stack_mask(st.slices, st.mask, T, st.resolution_x, st.resolution_y)
    rng = stack_range(stats)
    v = st.slices[st.mask].double().cpu().numpy()
    assert rng.tolist() == [v.min(), v.max()]
    hist = torch.ops.nesvor.otsu_histogram(st.slices, st.mask, rng, n_bins)
    t64, counts, _ = C.otsu_numpy(v, n_bins)
    assert hist.dtype == torch.int64 and hist.tolist() == counts.tolist() == otsu_histogram_composed(st.slices, st.mask, rng, n_bins).tolist()
    assert torch.equal(hist, torch.ops.nesvor.otsu_histogram(st.slices, st.mask.to(torch.uint8), rng, n_bins))
    t = torch.ops.nesvor.otsu_threshold(hist, rng)
    assert t.dtype == torch.float32 and t.tolist() == [float(np.float32(t64))] == otsu_threshold_composed(hist, rng).tolist()
    assert torch.equal(t, torch.ops.nesvor.otsu_threshold(hist, rng))
    applied, after = _both(st.slices, st.mask, T, st.resolution_x, st.resolution_y, threshold=t)  # the device float goes back in
    assert int(applied.sum()) == int((v > np.float32(t64)).sum()) and after[:, 0].sum() == applied.sum()
    if np.isfinite(t64):
        assert 0 < int(applied.sum()) < v.size
    else:
        assert v.size < 2 and int(applied.sum()) == v.size


@pytest.mark.gpu
def test_mask_stacks_fused_equals_composed_and_honours_the_switch(device, monkeypatch):
    from nesvor_amd import masking

    def run(**kw):
        stacks = C.scene("trio", device)
        return stacks, masking.mask_stacks(stacks, **kw)

    kw = dict(stacks_intersection=True, background_threshold=C.THRESHOLD, otsu_thresholding=True, n_bins_otsu=64)
    # the boundary condition of the Otsu step on what the first three steps keep (theirs is asserted per scene above)
    thr = torch.tensor([C.THRESHOLD], dtype=torch.float32, device=device)
    for st, T, slabs in _scene("trio", device):
        kept, _ = masking.stack_mask_composed(st.slices, st.mask, T, st.resolution_x, st.resolution_y, threshold=thr, **slabs)
        violations = C.otsu_violations(st.slices, kept, 64)
        assert not any(violations.values()), violations
    calls = []
    inner = masking.stack_mask_composed
    monkeypatch.setattr(masking, "stack_mask_composed", lambda *a, **k: calls.append(1) or inner(*a, **k))
    monkeypatch.delenv("NESVOR_MASKING", raising=False)
    fused, rep_f = run(**kw)
    assert not calls and all(r["fused"] for r in rep_f)
    monkeypatch.setenv("NESVOR_MASKING", "composed")
    composed, rep_c = run(**kw)
    assert len(calls) == 6 and not any(r["fused"] for r in rep_c)
    for a, b, ra, rb in zip(fused, composed, rep_f, rep_c):
        assert a.mask.dtype == torch.bool and torch.equal(a.mask, b.mask) and 0 < int(a.mask.sum())
        assert {k: v for k, v in ra.items() if k != "fused"} == {k: v for k, v in rb.items() if k != "fused"}
    monkeypatch.delenv("NESVOR_MASKING")
    # a stack emptied on the fused path: the exit names the switch
    with pytest.raises(SystemExit, match="--stacks-intersection"):
        masking.mask_stacks(C.scene("apart", device), stacks_intersection=True)
    # host tensors take the composed path whatever the switch says
    host = C.scene("trio")
    rep_h = masking.mask_stacks(host, **kw)
    assert not any(r["fused"] for r in rep_h) and all(torch.equal(h.mask, f.mask.cpu()) for h, f in zip(host, fused))


@pytest.mark.gpu
def test_ops_meta_kernels_and_argument_checks(device):
    st, T, slabs = _scene("pair", device)[0]
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")
    out, stats = torch.ops.nesvor.stack_mask(m(4, 1, 5, 6), None, m(4, 3, 4), 1.0, 1.0)
    assert tuple(out.shape) == (4, 1, 5, 6) and out.dtype == torch.uint8 and tuple(stats.shape) == (4, 3) and stats.dtype == torch.float64
    hist = torch.ops.nesvor.otsu_histogram(m(4, 1, 5, 6), None, m(2, dtype=torch.float64), 50)
    assert tuple(hist.shape) == (50,) and hist.dtype == torch.int64
    t = torch.ops.nesvor.otsu_threshold(m(50, dtype=torch.int64), m(2, dtype=torch.float64))
    assert tuple(t.shape) == (1,) and t.dtype == torch.float32
    rx, ry = st.resolution_x, st.resolution_y
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::stack_mask'"):
        torch.ops.nesvor.stack_mask(st.slices.cpu(), None, T.cpu(), rx, ry)
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.nesvor.stack_mask(st.slices.double(), None, T, rx, ry)
    with pytest.raises(RuntimeError, match=r"transforms \(n, 3, 4\)"):
        torch.ops.nesvor.stack_mask(st.slices, None, T[:1].contiguous(), rx, ry)
    with pytest.raises(RuntimeError, match="bool or torch.uint8"):
        torch.ops.nesvor.stack_mask(st.slices, st.mask.float(), T, rx, ry)
    with pytest.raises(RuntimeError, match="go together"):
        torch.ops.nesvor.stack_mask(st.slices, None, T, rx, ry, slab_offsets=slabs["slab_offsets"])
    with pytest.raises(RuntimeError, match="float64"):
        torch.ops.nesvor.stack_mask(st.slices, None, T, rx, ry, **{**slabs, "slabs": slabs["slabs"].float()})
    with pytest.raises(RuntimeError, match="volume_geometry"):
        torch.ops.nesvor.stack_mask(st.slices, None, T, rx, ry, volume=_volume(device)["volume"])
    rng = torch.tensor([0.0, 1.0], dtype=torch.float64, device=device)
    with pytest.raises(RuntimeError, match="n_bins"):
        torch.ops.nesvor.otsu_histogram(st.slices, None, rng, 1025)
    with pytest.raises(RuntimeError, match="float64"):
        torch.ops.nesvor.otsu_histogram(st.slices, None, rng.float(), 16)
    with pytest.raises(RuntimeError, match="n_bins"):
        torch.ops.nesvor.otsu_threshold(torch.zeros(1, dtype=torch.int64, device=device), rng)


@pytest.mark.gpu
def test_refusals_through_the_c_abi(device):
    """Every refusal returns before a launch (the checks are the first statements of the entry points), so the outputs keep the
    value they were given."""
    from nesvor_amd import _lib

    lib = _lib.load()
    st, T, slabs = _scene("pair", device)[0]
    n, h, w = 2, 1, 65
    INVALID = 1  # hipErrorInvalidValue
    P = _lib.ptr
    out = torch.full((n, 1, h, w), 9, dtype=torch.uint8, device=device)
    stats = torch.full((n, 3), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_stack_mask_workspace_bytes(n, h, w))
    assert nbytes == 8 * 3 * n * 1
    assert lib.nesvor_stack_mask_workspace_bytes(0, h, w) == 0 and lib.nesvor_stack_mask_workspace_bytes(n, h, 0) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    vol = _volume(device)
    n_slabs = int(slabs["slabs"].shape[0])

    def call(slices_=st.slices, T_=T, n_=n, h_=h, w_=w, rx=0.8, ry=0.8, volume=None, dims=(0, 0, 0), geom=None, table=slabs["slabs"],
             extents=slabs["slab_extents"], offsets=slabs["slab_offsets"], n_others=1, n_slabs_=n_slabs, out_=out, stats_=stats, ws_=ws,
             nb=nbytes):
        return lib.nesvor_stack_mask(P(slices_), P(st.mask), P(T_), n_, h_, w_, rx, ry, None, P(volume), *dims, P(geom), P(table), P(extents),
                                     P(offsets), n_others, n_slabs_, P(out_), P(stats_), P(ws_), nb, _lib.stream_ptr())

    for bad in (dict(slices_=None), dict(T_=None), dict(out_=None), dict(stats_=None), dict(n_=0), dict(h_=0), dict(w_=-1),
                dict(h_=46341, w_=46341), dict(rx=0.0), dict(ry=float("nan")), dict(ws_=None), dict(nb=nbytes - 1),
                dict(volume=vol["volume"], dims=(5, 6, 7)), dict(volume=vol["volume"], dims=(5, 0, 7), geom=vol["volume_geometry"]),
                dict(table=None), dict(extents=None), dict(offsets=None), dict(n_others=-1), dict(n_slabs_=-1)):
        assert call(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((stats == -7.0).all())
    assert call() == 0
    ref = torch.ops.nesvor.stack_mask(st.slices, st.mask, T, 0.8, 0.8, **slabs)
    assert torch.equal(out, ref[0]) and torch.equal(stats, ref[1])

    rng = torch.tensor([0.05, 1.0], dtype=torch.float64, device=device)
    hist = torch.full((16,), -3, dtype=torch.int64, device=device)
    hb = int(lib.nesvor_otsu_histogram_workspace_bytes(n, h, w, 16))
    assert hb == 4 * 16 * 1 and lib.nesvor_otsu_histogram_workspace_bytes(n, h, w, 1) == 0 == lib.nesvor_otsu_histogram_workspace_bytes(n, h, w, 1025)
    assert lib.nesvor_otsu_threshold_workspace_bytes(16) == 0
    hws = torch.empty(max(hb // 8, 1), dtype=torch.float64, device=device)

    def hcall(slices_=st.slices, n_=n, h_=h, w_=w, rng_=rng, bins=16, hist_=hist, ws_=hws, nb=hb):
        return lib.nesvor_otsu_histogram(P(slices_), P(st.mask), n_, h_, w_, P(rng_), bins, P(hist_), P(ws_), nb, _lib.stream_ptr())

    for bad in (dict(slices_=None), dict(rng_=None), dict(hist_=None), dict(n_=0), dict(h_=0), dict(w_=0), dict(h_=46341, w_=46341),
                dict(bins=1), dict(bins=1025), dict(ws_=None), dict(nb=hb - 1)):
        assert hcall(**bad) == INVALID, bad
    t = torch.full((1,), 5.0, dtype=torch.float32, device=device)
    tcall = lambda hist_=hist, rng_=rng, bins=16, t_=t: lib.nesvor_otsu_threshold(P(hist_), P(rng_), bins, P(t_), None, 0, _lib.stream_ptr())
    for bad in (dict(hist_=None), dict(rng_=None), dict(t_=None), dict(bins=1), dict(bins=1025)):
        assert tcall(**bad) == INVALID, bad
    torch.cuda.synchronize()
    assert bool((hist == -3).all()) and t.item() == 5.0
    assert hcall() == 0 and tcall() == 0
    want = torch.ops.nesvor.otsu_histogram(st.slices, st.mask, rng, 16)
    assert torch.equal(hist, want) and torch.equal(t, torch.ops.nesvor.otsu_threshold(want, rng))


# ---------------------------------------------------------------------------------------------------------------------
# end to end: the 32^3 phantom as three stacks of 22 slices of 40^2 (1.5 mm pixels, 3 mm slices) in NIfTI files
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def phantom_files(device, tmp_path_factory):
    from nesvor_amd.image import Volume
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.transform import RigidTransform

    folder = tmp_path_factory.mktemp("masking")
    vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
    slices, _ = simulate_stacks(vol, 3, res_s=1.5, s_thick=3.0, normalize=False)
    n = len(slices) // 3
    paths = []
    for j in range(3):
        img = torch.cat([s.image for s in slices[j * n:(j + 1) * n]], 0)
        ax = torch.cat([s.transformation.axisangle() for s in slices[j * n:(j + 1) * n]], 0).mean(0, keepdim=True)
        paths.append(str(folder / f"stack{j}.nii.gz"))
        Volume(img, img > 0, RigidTransform(ax), 1.5, 1.5, 3.0).save(paths[-1], masked=False)
    # a ball of 9 mm around (1, -1, 2) on a 2 mm lattice under a rotated pose
    z, y, x = np.meshgrid(*[np.arange(16) - 7.5] * 3, indexing="ij")
    ball = torch.tensor(((x ** 2 + y ** 2 + z ** 2) * 4.0 <= 81.0).astype(np.float32), device=device)
    pose = torch.tensor([[0.3, -0.2, 0.25, 1.0, -1.0, 2.0]], dtype=torch.float32, device=device)
    mask_path = str(folder / "ball.nii.gz")
    Volume(ball, ball > 0, RigidTransform(pose), 2.0, 2.0, 2.0).save(mask_path, masked=False)
    return paths, mask_path, folder


@pytest.mark.gpu
def test_cli_volume_mask_and_output_stack_masks(device, phantom_files, monkeypatch):
    from nesvor_amd import cli, masking
    from nesvor_amd.image_io import load_stack, load_volume

    monkeypatch.delenv("NESVOR_MASKING", raising=False)
    paths, mask_path, folder = phantom_files
    out = [str(folder / f"mask{j}.nii.gz") for j in range(3)]
    cli.main(["register", "--input-stacks", *paths, "--registration", "none", "--output-slices", str(folder / "slices"), "--volume-mask",
              mask_path, "--output-stack-masks", *out, "--verbose", "0"])
    vol, geom = masking.volume_tables(load_volume(mask_path, device=device), device)
    for p, m in zip(paths, out):
        st = load_stack(p, device=device)
        T = st.transformation.matrix(True).float().contiguous()
        violations = C.rule_violations(st.slices, st.mask, T, st.resolution_x, st.resolution_y, volume=vol, volume_geometry=geom)
        assert not any(violations.values()), violations
        want, _ = masking.stack_mask_composed(st.slices, st.mask, T, st.resolution_x, st.resolution_y, volume=vol, volume_geometry=geom)
        written = load_stack(m, device=device)  # the round trip: a mask file is its own mask, and a --stack-masks input
        assert torch.equal(written.mask, want.bool()) and torch.equal(load_stack(p, m, device=device).mask, want.bool())
        assert 0 < int(want.sum()) < int(st.mask.sum())
    with pytest.raises(SystemExit, match="output stack masks and input stacks are different"):
        cli.main(["assess", "--input-stacks", *paths, "--otsu-thresholding", "--output-stack-masks", *out[:2], "--verbose", "0"])


@pytest.mark.gpu
def test_cli_assess_and_svr_see_fewer_voxels(device, phantom_files, monkeypatch):
    from nesvor_amd import cli
    from nesvor_amd.image_io import load_volume

    paths, _, folder = phantom_files
    seen = []
    inner = cli._load_stacks
    monkeypatch.setattr(cli, "_load_stacks", lambda args: seen.append(inner(args)) or seen[-1])
    flags = ["--stacks-intersection", "--otsu-thresholding"]
    report = str(folder / "assess.json")
    cli.main(["assess", "--input-stacks", *paths, "--output-json", report, "--verbose", "0"])
    cli.main(["assess", "--input-stacks", *paths, "--output-json", report, "--verbose", "0", *flags])
    assert len(json.load(open(report))) == 3
    svr = ["svr", "--input-stacks", *paths, "--registration", "none", "--n-iter-srr", "3", "--verbose", "0"]
    cli.main(svr + ["--output-volume", str(folder / "svr_plain.nii.gz")])
    cli.main(svr + ["--output-volume", str(folder / "svr_masked.nii.gz"), *flags])
    counts = [[int(st.mask.sum()) for st in stacks] for stacks in seen]
    assert len(counts) == 4 and counts[0] == counts[2] and counts[1] == counts[3]
    assert all(0 < b < a for a, b in zip(counts[0], counts[1]))
    plain, masked = (load_volume(str(folder / f"svr_{k}.nii.gz"), device=device) for k in ("plain", "masked"))
    assert bool(torch.isfinite(masked.image).all()) and 0 < int((masked.image > 0).sum())


@pytest.mark.gpu
def test_cli_reconstruct_with_a_sample_mask(device, phantom_files):
    from nesvor_amd import cli
    from nesvor_amd.image import Volume
    from nesvor_amd.image_io import load_volume

    paths, mask_path, folder = phantom_files
    out = str(folder / "recon.nii.gz")
    cli.main(["reconstruct", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--output-volume", out, "--sample-mask", mask_path,
              "--single-precision", "--n-iter", "20", "--batch-size", "512", "--n-samples", "32", "--log2-hashmap-size", "12",
              "--finest-resolution", "2.0", "--output-resolution", "2.0", "--seed", "0", "--verbose", "0"])
    v = load_volume(out, device=device)
    given = load_volume(mask_path, device=device)
    everywhere = Volume(v.image, torch.ones_like(v.mask), v.transformation, v.resolution_x, v.resolution_y, v.resolution_z)
    xyz = everywhere.xyz_masked  # all voxel centres of the written volume, in the order of image.flatten()
    # "outside the given mask": the mask interpolates to 0 there and 0.01 mm to every side (the file's float32 affine moves the
    # re-computed positions by some 1e-5 mm against the ones the command sampled at)
    shifts = torch.tensor([[a, b, c] for a in (-0.01, 0.01) for b in (-0.01, 0.01) for c in (-0.01, 0.01)], device=device)
    value = torch.stack([given.sample_points(xyz + s) for s in shifts]).amax(0).view(v.image.shape)
    assert 0 < int((v.image > 0).sum()) and bool((v.image[value == 0] == 0).all()) and int((value == 0).sum()) > 0
    # inside the given mask the model was sampled: the slices' own mask (a box around all stacks) would be far larger
    assert int((v.image > 0).sum()) <= int((value > 0).sum())
