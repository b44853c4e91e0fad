"""CPU: the stack masking definitions (nesvor_amd/masking.py) on the composed float64 path with host tensors - each of the four
rules against a plain numpy loop (tests/masking_cases.py), the order of the steps, Otsu's special cases, the warnings, the exit
for an emptied stack, the parser, and ``_load_stacks`` with and without the flags.  Also here, because it needs no GPU: the
fixtures of tests/test_gpu_masking.py meet the boundary condition of their bit-for-bit comparison in float64."""
import logging
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import masking_cases as C


def _tiny_scene():
    specs = [((2, 4, 5), 1.0, 1.2, 3.0, 2.0, [0.1, 0.1, 0.1, 0.1, 0.1, 0.1]), ((3, 3, 4), 1.5, 1.0, 1.0, 1.6, [-0.1, 0.0, -0.4, 0.1, 0.5, 0.1]),
             ((1, 5, 5), 0.9, 0.9, 4.0, 4.0, [-0.12, -0.01, 0.1, -0.3, 0.2, 0.4])]
    return [C.make_stack(shape, rx, ry, th, gap, pose, seed=i) for i, (shape, rx, ry, th, gap, pose) in enumerate(specs)]


def _rule(st, **kw):
    from nesvor_amd.masking import stack_mask_composed

    T = st.transformation.matrix(True).float().contiguous()
    return stack_mask_composed(st.slices, st.mask, T, st.resolution_x, st.resolution_y, **kw)


def test_background_threshold_against_a_loop_and_drops_nan():
    st = _tiny_scene()[0]
    st.slices[0, 0, 1, 2] = float("nan")
    st.mask = torch.ones_like(st.mask)
    got, stats = _rule(st, threshold=torch.tensor([0.4]))
    v = st.slices.numpy()
    want = np.zeros(v.shape, dtype=bool)
    for idx in np.ndindex(*v.shape):
        want[idx] = bool(v[idx] > np.float32(0.4))
    assert np.array_equal(got.numpy().astype(bool), want) and not want[0, 0, 1, 2]
    for s in range(v.shape[0]):
        kept = v[s][want[s]]
        assert stats[s].tolist() == [float(kept.size), float(kept.min()), float(kept.max())]
    # no threshold: the NaN voxel stays in the mask and in the count, and enters neither extreme
    got, stats = _rule(st)
    assert bool(got.all()) and stats[0, 0] == 20 and stats[0, 1] == np.nanmin(v[0]) and stats[0, 2] == np.nanmax(v[0])


def test_volume_mask_against_a_loop():
    from nesvor_amd.masking import volume_tables

    vol = C.ball_volume()
    arr, geom = volume_tables(vol, "cpu")
    assert arr.dtype == torch.uint8 and tuple(arr.shape) == (5, 6, 7) and geom.dtype == torch.float64 and geom.numel() == 15
    inside = outside = 0
    for st in _tiny_scene():
        want = C.volume_loop(st, vol)
        assert np.abs(want - 0.5).min() > 1e-6
        got, _ = _rule(st, volume=arr, volume_geometry=geom)
        expect = (want >= 0.5) & st.mask[:, 0].numpy()
        assert np.array_equal(got[:, 0].numpy().astype(bool), expect)
        inside, outside = inside + int(expect.sum()), outside + int((~expect).sum())
    assert inside > 10 and outside > 10
    # the same interpolation as Volume.sample_points (grid_sample, zeros outside), which works in float32
    from nesvor_amd.masking import pixel_positions, volume_value_composed

    st = C.scene("solo")[0]
    p = pixel_positions(st.transformation.matrix(True), 33, 31, st.resolution_x, st.resolution_y)
    assert (volume_value_composed(p, arr, geom) == 0).any()  # voxels off the lattice
    assert torch.allclose(volume_value_composed(p, arr, geom).float(), vol.sample_points(p.float()), atol=1e-4)
    thin = C.ball_volume()
    thin.image = thin.image[:1]
    with pytest.raises(SystemExit, match="at least 2 voxels"):
        volume_tables(thin, "cpu")


def test_stacks_intersection_against_a_loop():
    from nesvor_amd.masking import slab_tables

    stacks = _tiny_scene()
    kept = 0
    for j, st in enumerate(stacks):
        slabs, extents, offsets = slab_tables(stacks, j)
        assert tuple(slabs.shape) == (sum(len(s) for k, s in enumerate(stacks) if k != j), 3, 4) and offsets[0] == 0
        got, stats = _rule(st, slabs=slabs, slab_extents=extents, slab_offsets=offsets)
        want = C.intersection_loop(stacks, j) & st.mask[:, 0].numpy()
        assert np.array_equal(got[:, 0].numpy().astype(bool), want)
        assert stats[:, 0].tolist() == want.reshape(want.shape[0], -1).sum(1).tolist()
        kept += int(want.sum())
        assert 0 < want.sum() < st.mask.sum()
    # gap > thickness (stack 1) and thickness > gap (stack 0): the slab is max(thickness, gap) thick either way
    assert slab_tables(stacks, 2)[1][:, 2].tolist() == [1.5, 0.8]
    # the slabs are geometry: emptying another stack's mask changes nothing
    stacks[1].mask[:] = False
    slabs, extents, offsets = slab_tables(stacks, 0)
    again, _ = _rule(stacks[0], slabs=slabs, slab_extents=extents, slab_offsets=offsets)
    assert np.array_equal(again[:, 0].numpy().astype(bool), C.intersection_loop(stacks, 0) & stacks[0].mask[:, 0].numpy())


def test_otsu_on_hand_made_histograms():
    from nesvor_amd.masking import otsu_histogram_composed, otsu_threshold_composed, slice_stats_composed, stack_range

    # two classes of four voxels in the first and the last of four bins: the splits after bins 0, 1 and 2 tie, the first wins
    v = torch.tensor([0.0, 0.0, 0.0, 0.1, 0.9, 1.0, 1.0, 1.0]).reshape(1, 1, 2, 4)
    rng = stack_range(slice_stats_composed(v, torch.ones_like(v, dtype=torch.bool)))
    assert rng.tolist() == [0.0, 1.0]
    hist = otsu_histogram_composed(v, None, rng, 4)
    assert hist.dtype == torch.int64 and hist.tolist() == [4, 0, 0, 4]
    t = otsu_threshold_composed(hist, rng)
    assert t.dtype == torch.float32 and t.tolist() == [0.125]
    # a known split: 5 + 1 voxels low, 2 + 6 high over [0, 5): the best split is after bin 1
    hist = torch.tensor([5, 1, 0, 2, 6])
    rng = torch.tensor([0.0, 5.0], dtype=torch.float64)
    assert otsu_threshold_composed(hist, rng).tolist() == [1.5]
    values = np.repeat([0.0, 1.2, 3.5, 5.0, 4.1], [5, 1, 2, 5, 1])
    t64, counts, var = C.otsu_numpy(values, 5)
    assert counts.tolist() == [5, 1, 0, 2, 6] and t64 == 1.5 and int(np.argmax(var)) == 1
    # the maximum sits in the last bin, the mask is honoured
    v = torch.tensor([1.0, 2.0, 3.0, 4.0, 100.0]).reshape(1, 1, 1, 5)
    m = torch.tensor([1, 1, 1, 1, 0], dtype=torch.bool).reshape(v.shape)
    assert otsu_histogram_composed(v, m, torch.tensor([1.0, 4.0], dtype=torch.float64), 3).tolist() == [1, 1, 2]


def test_order_of_the_steps_and_the_report():
    from nesvor_amd.masking import mask_stacks

    stacks = C.scene("trio")
    before = [st.mask.clone() for st in stacks]
    reports = mask_stacks(stacks, stacks_intersection=True, background_threshold=C.THRESHOLD, otsu_thresholding=True, n_bins_otsu=64)
    fresh = C.scene("trio")
    for j, (st, rep) in enumerate(zip(stacks, reports)):
        v = fresh[j].slices[:, 0].numpy()
        kept = before[j][:, 0].numpy() & (v > np.float32(C.THRESHOLD))
        if j == 2:  # (the loop is slow: one stack; the others through the composed rule, tested above)
            assert np.array_equal(kept & C.intersection_loop(fresh, j), _steps_123(fresh, j))
        kept = _steps_123(fresh, j)
        t64, _, _ = C.otsu_numpy(v[kept], 64)  # Otsu sees the voxels the first three steps kept, and only them
        assert rep["otsu_threshold"] == float(np.float32(t64)) != float(np.float32(C.otsu_numpy(v[before[j][:, 0].numpy()], 64)[0]))
        final = kept & (v > np.float32(t64))
        assert np.array_equal(st.mask[:, 0].numpy(), final) and st.mask.dtype == torch.bool and st.mask.shape == before[j].shape
        assert not (st.mask & ~before[j]).any()  # every step only removes voxels
        assert rep["voxels_before"] == int(before[j].sum()) and rep["voxels_after"] == int(final.sum()) and not rep["fused"]
        assert rep["slices_before"] == int(before[j].flatten(1).any(1).sum()) and rep["slices_after"] == int(final.reshape(len(v), -1).any(1).sum())
        assert rep["kept_share"] == rep["voxels_after"] / rep["voxels_before"]


def _steps_123(stacks, j):
    from nesvor_amd.masking import slab_tables

    slabs, extents, offsets = slab_tables(stacks, j)
    got, _ = _rule(stacks[j], threshold=torch.tensor([C.THRESHOLD]), slabs=slabs, slab_extents=extents, slab_offsets=offsets)
    return got[:, 0].numpy().astype(bool)


def test_otsu_without_a_range_thresholds_nothing(caplog):
    from nesvor_amd.masking import mask_stacks

    flat = C.make_stack((2, 3, 3), 1.0, 1.0, 2.0, 2.0, [0.1, 0.1, 0.1, 0, 0, 0])
    flat.slices = torch.full_like(flat.slices, 0.7)
    flat.mask = torch.ones_like(flat.mask)
    single = C.make_stack((1, 2, 2), 1.0, 1.0, 2.0, 2.0, [0.1, 0.1, 0.1, 0, 0, 0])
    single.mask = torch.zeros_like(single.mask)
    single.mask[0, 0, 1, 1] = True
    single.slices[0, 0, 1, 1] = 0.5
    with caplog.at_level(logging.WARNING):
        reports = mask_stacks([flat, single], otsu_thresholding=True)
    assert [r["otsu_threshold"] for r in reports] == [-float("inf")] * 2
    assert bool(flat.mask.all()) and int(single.mask.sum()) == 1
    assert sum("nothing is thresholded" in r.getMessage() for r in caplog.records) == 2


def test_intersection_is_ignored_with_one_stack_or_a_volume_mask(caplog):
    from nesvor_amd.masking import mask_stacks

    solo = C.scene("solo")
    before = solo[0].mask.clone()
    with caplog.at_level(logging.WARNING):
        mask_stacks(solo, stacks_intersection=True)
    assert torch.equal(solo[0].mask, before) and "more than one stack" in caplog.text
    caplog.clear()
    apart = C.scene("apart")[:1] + C.scene("solo")  # their intersection is empty: it must not be taken
    vol = C.ball_volume()
    with caplog.at_level(logging.WARNING):
        reports = mask_stacks(apart, stacks_intersection=True, volume_mask=vol)
    assert "--volume-mask is given" in caplog.text and all(r["voxels_after"] > 0 for r in reports)
    assert np.array_equal(apart[1].mask[:, 0].numpy(), (C.volume_loop(C.scene("solo")[0], vol) >= 0.5) & before[:, 0].numpy())


def test_an_emptied_stack_ends_the_program_naming_the_switch():
    from nesvor_amd.masking import mask_stacks

    with pytest.raises(SystemExit, match=r"no voxel of second.*--stacks-intersection"):
        mask_stacks(C.scene("apart")[::-1], stacks_intersection=True, background_threshold=0.06, names=["second", "first"])
    with pytest.raises(SystemExit, match=r"no voxel of stack 0.*--background-threshold"):
        mask_stacks(C.scene("solo"), background_threshold=10.0, otsu_thresholding=True)
    far = C.ball_volume()
    far.transformation = type(far.transformation)(far.transformation.matrix(True) + torch.tensor([0, 0, 0, 500.0]), trans_first=True)
    with pytest.raises(SystemExit, match=r"--volume-mask"):
        mask_stacks(C.scene("solo"), volume_mask=far)
    empty = C.scene("solo")
    empty[0].mask[:] = False
    with pytest.raises(SystemExit, match=r"its own mask"):
        mask_stacks(empty, background_threshold=0.1)


def test_parser_has_the_masking_flags_on_the_five_commands():
    from nesvor_amd.cli import build_parser, masking_requested

    flags = ["--volume-mask", "m.nii.gz", "--stacks-intersection", "--background-threshold", "0.5", "--otsu-thresholding", "--n-bins-otsu",
             "128", "--output-stack-masks", "a.nii.gz", "b.nii.gz"]
    heads = {"reconstruct": ["--output-volume", "v.nii.gz"], "register": ["--output-slices", "d"], "svr": ["--output-volume", "v.nii.gz"],
             "assess": [], "correct-bias-field": ["--output-corrected-stacks", "c.nii.gz", "d.nii.gz"]}
    for command, extra in heads.items():
        base = [command, "--input-stacks", "x.nii.gz", "y.nii.gz", *extra]
        args = build_parser().parse_args(base + flags)
        assert (args.volume_mask, args.stacks_intersection, args.background_threshold, args.otsu_thresholding, args.n_bins_otsu,
                args.output_stack_masks) == ("m.nii.gz", True, 0.5, True, 128, ["a.nii.gz", "b.nii.gz"])
        assert masking_requested(args)
        args = build_parser().parse_args(base)
        assert (args.volume_mask, args.stacks_intersection, args.background_threshold, args.otsu_thresholding, args.n_bins_otsu,
                args.output_stack_masks) == (None, False, None, False, 256, None)
        assert not masking_requested(args)
    assert masking_requested(Namespace(background_threshold=0.0)) and not masking_requested(Namespace())
    assert build_parser().parse_args(["reconstruct", "--input-stacks", "x", "--sample-mask", "s.nii.gz"]).sample_mask == "s.nii.gz"
    assert build_parser().parse_args(["sample-volume", "--input-model", "m.pt", "--output-volume", "v", "--sample-mask", "s"]).sample_mask == "s"
    assert build_parser().parse_args(["sample-volume", "--input-model", "m.pt", "--output-volume", "v"]).sample_mask is None
    with pytest.raises(SystemExit):
        build_parser().parse_args(["sample-slices", "--input-model", "m", "--input-slices", "d", "--simulated-slices", "e", "--volume-mask", "m"])


def test_input_slices_ignores_the_flags_with_a_warning(caplog, monkeypatch):
    from nesvor_amd import cli, image_io, svr

    def stop(*a, **k):
        raise KeyboardInterrupt  # the commands are left where they would read the folder

    monkeypatch.setattr(image_io, "load_slices", stop)
    for command, run in (("reconstruct", cli.reconstruct), ("svr", svr.svr_command)):
        for extra, warned in ((["--otsu-thresholding"], True), (["--background-threshold", "0"], True), ([], False)):
            args = cli.build_parser().parse_args([command, "--input-slices", "x", "--output-volume", "v.nii.gz", *extra])
            args.device = torch.device("cpu")
            caplog.clear()
            with caplog.at_level(logging.WARNING), pytest.raises(KeyboardInterrupt):
                run(args)
            assert ("stack masking flags" in caplog.text and "are ignored with --input-slices" in caplog.text) == warned, (command, extra)


def _files(tmp_path):
    from nesvor_amd.image_io import save_stack

    stacks = C.scene("trio")[::2]
    paths = [str(tmp_path / f"s{j}.nii.gz") for j in range(len(stacks))]
    for p, st in zip(paths, stacks):
        save_stack(p, st)
    return paths


def test_load_stacks_without_flags_never_touches_masking(tmp_path, monkeypatch):
    from nesvor_amd import cli
    from nesvor_amd.image_io import load_stack

    paths = _files(tmp_path)
    from nesvor_amd import masking

    def refuse(*a, **k):
        raise AssertionError("masking called")

    # a first import raises, the module's entry point raises if it was imported before, and so does the command's own step
    monkeypatch.setitem(sys.modules, "nesvor_amd.masking", None)
    monkeypatch.setattr(masking, "mask_stacks", refuse)
    monkeypatch.setattr(cli, "_mask_stacks", refuse)
    args = cli.build_parser().parse_args(["assess", "--input-stacks", *paths])
    args.device = torch.device("cpu")
    loaded = cli._load_stacks(args)
    for st, p in zip(loaded, paths):
        ref = load_stack(p)
        assert torch.equal(st.mask, ref.mask) and torch.equal(st.slices, ref.slices)
    args.background_threshold = 0.0  # the control: one flag, and the step is taken
    with pytest.raises(AssertionError, match="masking called"):
        cli._load_stacks(args)


def test_load_stacks_applies_the_flags_and_writes_the_masks(tmp_path, caplog):
    from nesvor_amd import cli
    from nesvor_amd.image_io import load_stack

    paths = _files(tmp_path)
    out = [str(tmp_path / f"m{j}.nii.gz") for j in range(2)]
    args = cli.build_parser().parse_args(["register", "--input-stacks", *paths, "--output-slices", "d", "--background-threshold", "0.3",
                                          "--stacks-intersection", "--otsu-thresholding", "--output-stack-masks", *out])
    args.device = torch.device("cpu")
    with caplog.at_level(logging.INFO):
        loaded = cli._load_stacks(args)
    assert "Stack masking, stack 0 (" in caplog.text
    for st, p, m in zip(loaded, paths, out):
        ref = load_stack(p)
        assert 0 < int(st.mask.sum()) < int(ref.mask.sum()) and not (st.mask & ~ref.mask).any()
        assert torch.equal(load_stack(m).mask, st.mask) and torch.equal(load_stack(p, m).mask, st.mask)  # the round trip
    args.output_stack_masks = out[:1]
    with pytest.raises(SystemExit, match="output stack masks and input stacks are different"):
        cli._load_stacks(args)


def test_gpu_fixtures_meet_the_boundary_condition():
    """The float64 restatement alone, on the CPU: no voxel of a fixture of tests/test_gpu_masking.py sits near a decision."""
    from nesvor_amd.masking import slab_tables, volume_tables

    vol, geom = volume_tables(C.ball_volume(), "cpu")
    thr = torch.tensor([C.THRESHOLD])
    for name in C.SCENES:
        stacks = C.scene(name)
        for j, st in enumerate(stacks):
            T = st.transformation.matrix(True).float().contiguous()
            kw = dict(zip(("slabs", "slab_extents", "slab_offsets"), slab_tables(stacks, j))) if len(stacks) > 1 else {}
            for rules in ({"threshold": thr, **kw}, {"volume": vol, "volume_geometry": geom}):
                assert not any(C.rule_violations(st.slices, st.mask, T, st.resolution_x, st.resolution_y, **rules).values()), (name, j)
    for name, j, n_bins in C.OTSU_CASES:
        st = C.scene(name)[j]
        assert not any(C.otsu_violations(st.slices, st.mask, n_bins).values()), (name, j, n_bins)
