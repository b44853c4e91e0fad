"""Stack assessment on the GPU: the pair-moments kernel (csrc/assess.hip) against the torch expression in fp64 at wave and
block edges, its reproducibility, symmetry and refusals, the scores on a moved and two still stacks, and the template stack
through ``register_stacks`` and the command line."""
import json
import os

import pytest
import torch

# (n, h, w): 1, 63, 64, 65 pixels (inside / at / past one wave), 255, 256, 257 (one workgroup), 1023, 1024, 2080 (several)
SHAPES = [(2, 1, 1), (3, 1, 63), (3, 1, 64), (3, 1, 65), (2, 5, 51), (2, 16, 16), (2, 257, 1), (4, 33, 31), (3, 32, 32), (3, 40, 52)]
KINDS = ["none", "bool", "uint8"]
SWAP = [0, 2, 1, 4, 3, 5]  # the columns of (b, a) in terms of (a, b)
# |fused score - composed fp64 score| of ncc and matrix-rank on the same tensors.  Measured on MI355X ("Stack
# assessment"): the largest difference over Set A and the three still / three moved stacks is 1.85e-8 (matrix-rank, still stack 1);
# 4 x that, rounded up to a power of ten.  The margin is for data-dependent cancellation in the variances.
SCORE_TOL = 1e-7
_DATA = {}


def _data(shape, kind, device):
    """Slices 1 + 0.5 randn (a non-zero mean), a mask of about 60 % with slice 1 fully masked, and the pair list: every i <= j,
    one reversed pair, one duplicate.  Shared by the tests and never written."""
    key = (shape, kind)
    if key not in _DATA:
        n, h, w = shape
        g = torch.Generator().manual_seed(100 * n + 10 * h + w)
        x = 1 + 0.5 * torch.randn(n, 1, h, w, generator=g)
        mask = None
        if kind != "none":
            mask = torch.rand(n, 1, h, w, generator=g) < 0.6
            mask[1] = False
            if kind == "uint8":
                mask = mask.to(torch.uint8) * 3  # any set byte counts
        pairs = [(i, j) for i in range(n) for j in range(i, n)]
        pairs += [(n - 1, 0), (0, n - 1)]  # (0, n-1) is in the list already: its reversal and its duplicate
        _DATA[key] = (x.to(device), None if mask is None else mask.to(device), pairs)
    return _DATA[key]


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_pair_moments_against_the_torch_expression_in_fp64(device, shape, kind):
    """count exactly; every other sum S within 2^-17 sum |term| of the fp64 expression: one product rounding plus at most 64 fp32
    additions are at most 65 * 2^-24 < 2^-17 of the absolute sum, everything beyond a wave is added in double."""
    from nesvor_amd.assess import pair_moments_composed

    x, mask, pairs = _data(shape, kind, device)
    dev_pairs = torch.tensor(pairs, dtype=torch.int32, device=device)
    got = torch.ops.nesvor.pair_moments(x, mask, dev_pairs)
    ref = pair_moments_composed(x, mask, dev_pairs)
    absolute = pair_moments_composed(x.abs(), mask, dev_pairs)  # sum |a|, sum |b|, sum a^2, sum b^2, sum |a b| in fp64
    assert got.shape == (len(pairs), 6) and got.dtype == torch.float64 and ref.dtype == torch.float64
    assert torch.equal(got[:, 0], ref[:, 0])
    if mask is None:
        assert bool((got[:, 0] == shape[1] * shape[2]).all())
    else:
        masked = torch.tensor([1 in p for p in pairs], device=device)
        assert bool((got[masked] == 0).all()) and bool((ref[masked] == 0).all())
    err = (got - ref).abs()
    bound = 2.0 ** -17 * absolute
    worst = float((err[:, 1:] / absolute[:, 1:].clamp(min=1e-300)).max())
    print(f"{shape} {kind}: largest |S - S64| / sum |term| = {worst:.3e} (bound {2.0 ** -17:.3e})")
    assert bool((err[:, 1:] <= bound[:, 1:]).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(2, 1, 1), (3, 1, 65), (4, 33, 31), (3, 40, 52)])
def test_pair_moments_are_reproducible_and_symmetric(device, shape, kind):
    from nesvor_amd import assess

    x, mask, pairs = _data(shape, kind, device)
    dev_pairs = torch.tensor(pairs, dtype=torch.int32, device=device)
    first = torch.ops.nesvor.pair_moments(x, mask, dev_pairs)
    second = torch.ops.nesvor.pair_moments(x, mask, dev_pairs)
    assert torch.equal(first, second)
    n = shape[0]
    at = pairs.index((0, n - 1))
    assert pairs[-2] == (n - 1, 0) and pairs[-1] == (0, n - 1) and at < len(pairs) - 2
    assert torch.equal(first[-1], first[at])  # the duplicate
    assert torch.equal(first[-2], first[at][SWAP])  # the reversed pair
    flipped = torch.ops.nesvor.pair_moments(x, mask, dev_pairs.flip(1).contiguous())
    assert torch.equal(flipped, first[:, SWAP])
    # the public entry takes host pairs, flat slices and either mask type to the same kernel
    public = assess.pair_moments(x[:, 0], None if mask is None else mask[:, 0], pairs)
    assert torch.equal(public, first)


@pytest.mark.gpu
def test_pair_moments_wrapper(device, monkeypatch):
    """``assess.pair_moments``: the index check on the host before anything is launched, the fused path without the torch
    expression, ``NESVOR_ASSESS=composed`` with it; the op's own refusals and its fake kernel."""
    from nesvor_amd import assess

    x, mask, pairs = _data((4, 33, 31), "bool", device)
    calls = []
    inner = assess.pair_moments_composed
    monkeypatch.setattr(assess, "pair_moments_composed", lambda *a: calls.append(1) or inner(*a))
    launched = []
    op = torch.ops.nesvor.pair_moments
    monkeypatch.delenv("NESVOR_ASSESS", raising=False)
    monkeypatch.setattr(assess.torch.ops.nesvor, "pair_moments", lambda *a: launched.append(1) or op(*a))
    for bad in ([(0, 4)], [(-1, 0)], torch.tensor([[0, 1], [4, 0]])):
        with pytest.raises(ValueError):
            assess.pair_moments(x, mask, bad)
    assert not launched and not calls
    fused = assess.pair_moments(x, mask, pairs)
    assert launched == [1] and not calls
    monkeypatch.setenv("NESVOR_ASSESS", "composed")
    composed = assess.pair_moments(x, mask, pairs)
    assert launched == [1] and calls == [1] and composed.device == x.device
    assert torch.equal(fused[:, 0], composed[:, 0])
    monkeypatch.undo()
    dev_pairs = torch.tensor(pairs, dtype=torch.int32, device=device)
    meta = torch.ops.nesvor.pair_moments(x.to("meta"), None, dev_pairs.to("meta"))
    assert meta.shape == (len(pairs), 6) and meta.dtype == torch.float64
    assert torch.ops.nesvor.pair_moments(x, mask, dev_pairs[:0]).shape == (0, 6)
    with pytest.raises(NotImplementedError, match="Could not run 'nesvor::pair_moments'"):
        torch.ops.nesvor.pair_moments(x.cpu(), mask.cpu(), dev_pairs.cpu())
    with pytest.raises(RuntimeError, match="torch.float32"):
        torch.ops.nesvor.pair_moments(x.double(), mask, dev_pairs)
    with pytest.raises(RuntimeError, match="torch.int32"):
        torch.ops.nesvor.pair_moments(x, mask, dev_pairs.long())
    with pytest.raises(RuntimeError, match="contiguous"):
        torch.ops.nesvor.pair_moments(x.transpose(-1, -2), None, dev_pairs)
    with pytest.raises(RuntimeError, match="torch.bool or torch.uint8"):
        torch.ops.nesvor.pair_moments(x, mask.float(), dev_pairs)
    with pytest.raises(RuntimeError, match="one shape"):
        torch.ops.nesvor.pair_moments(x, mask[:3].contiguous(), dev_pairs)
    with pytest.raises(RuntimeError, match=r"\(P, 2\)"):
        torch.ops.nesvor.pair_moments(x, mask, dev_pairs.flatten())


@pytest.mark.gpu
def test_pair_moments_refusals(device):
    """Every refusal returns before a launch (csrc/assess.hip: the checks are the first statements of nesvor_pair_moments), so the
    sentinel in the moments stays."""
    from nesvor_amd import _lib

    lib = _lib.load()
    INVALID = 1  # hipErrorInvalidValue
    n, h, w = 4, 33, 31
    x, mask, pairs = _data((n, h, w), "bool", device)
    pairs = torch.tensor(pairs, dtype=torch.int32, device=device)
    count = int(pairs.shape[0])
    moments = torch.full((count, 6), -7.0, dtype=torch.float64, device=device)
    nbytes = int(lib.nesvor_pair_moments_workspace_bytes(count, h, w))
    assert nbytes == 8 * 6 * count * 4  # four workgroups per pair
    assert lib.nesvor_pair_moments_workspace_bytes(0, h, w) == 0 and lib.nesvor_pair_moments_workspace_bytes(count, 0, w) == 0
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
    P = _lib.ptr

    def call(n_=n, h_=h, w_=w, x_=x, mask_=mask, pairs_=pairs, count_=count, moments_=moments, ws_=ws, nb=nbytes):
        return lib.nesvor_pair_moments(P(x_), P(mask_), n_, h_, w_, P(pairs_), count_, P(moments_), P(ws_), nb, _lib.stream_ptr())

    assert call(nb=nbytes - 1) == INVALID and call(nb=0) == INVALID and call(ws_=None) == INVALID  # a short or missing workspace
    assert call(count_=-1) == INVALID and call(n_=0) == INVALID and call(n_=-2) == INVALID
    assert call(h_=0) == INVALID and call(w_=0) == INVALID and call(w_=-3) == INVALID
    assert call(h_=65536, w_=65536) == INVALID and call(h_=1, w_=2 ** 31 - 256) == INVALID  # h w > INT_MAX - 256
    assert call(h_=1, w_=2 ** 31 - 257, count_=300) == INVALID  # h w passes, 300 x 8388607 workgroups do not
    for name in ("x_", "pairs_", "moments_"):
        assert call(**{name: None}) == INVALID
    assert call(count_=0) == 0 and call(count_=0, ws_=None, nb=0) == 0 and call(count_=0, n_=0) == 0  # no pairs: a no-op
    torch.cuda.synchronize()
    assert bool((moments == -7.0).all())
    assert call() == 0 and call(mask_=None) == 0  # (a NULL mask is legal)
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(moments, torch.ops.nesvor.pair_moments(x, mask, pairs))


# ---------------------------------------------------------------------------------------------------------------------
# scores: the 32^3 phantom as three stacks of 22 slices of 40^2 (1.5 mm pixels, 3 mm slices), still and with motion
# ---------------------------------------------------------------------------------------------------------------------
_RES_S, _THICK = 1.5, 3.0
_SETS = {}


def _sets(device):
    """``still`` and ``moved``: three (22,1,40,40) image tensors each (4 deg / 2 mm of inter-slice motion, seed 0) with their
    nominal poses; built once, never written."""
    if _SETS:
        return _SETS
    from nesvor_amd.phantom import phantom3d, simulate_stacks
    from nesvor_amd.transform import RigidTransform

    vol = torch.tensor(phantom3d(n=32), dtype=torch.float32, device=device)
    for name, motion in (("still", {}), ("moved", {"motion_deg": 4, "motion_mm": 2, "seed": 0})):
        slices, _ = simulate_stacks(vol, 3, res_s=_RES_S, s_thick=_THICK, normalize=False, **motion)
        n = len(slices) // 3
        _SETS[name] = [torch.stack([s.image for s in slices[j * n:(j + 1) * n]]).contiguous() for j in range(3)]
        _SETS["poses"] = [RigidTransform.cat([s.transformation for s in slices[j * n:(j + 1) * n]]) for j in range(3)]
    assert tuple(_SETS["still"][0].shape) == (22, 1, 40, 40)
    return _SETS


def _stacks(images, poses):
    """Fresh ``Stack`` objects (the registration writes into them) on copies of the shared tensors."""
    from nesvor_amd.image import Stack
    from nesvor_amd.transform import RigidTransform

    return [Stack(img.clone(), img > 0, RigidTransform(t.axisangle().clone()), resolution_x=_RES_S, resolution_y=_RES_S, thickness=_THICK,
                  gap=_THICK) for img, t in zip(images, poses)]


def _set_a(device):
    c = _sets(device)
    return _stacks([c["moved"][0], c["still"][1], c["still"][2]], c["poses"])


def _both_paths(stacks, metric, monkeypatch):
    from nesvor_amd.assess import assess_stacks

    monkeypatch.delenv("NESVOR_ASSESS", raising=False)
    fused = assess_stacks(stacks, metric)
    monkeypatch.setenv("NESVOR_ASSESS", "composed")
    composed = assess_stacks(stacks, metric)
    monkeypatch.delenv("NESVOR_ASSESS")
    return fused, composed


@pytest.mark.gpu
def test_scores_rank_the_moved_stack_last(device, monkeypatch):
    """Set A = [moved stack 0, still stack 1, still stack 2]: ``ncc`` ranks them [2, 1, 0] (CPU-oracle scores 0.054, 0.654,
    0.759), so ``auto`` picks stack 2; ``matrix-rank`` is compared within an orientation - the still stack beats the moved one
    for stacks 1 and 2 (-0.636 against -0.773, -0.607 against -0.835; stack 0's two scores are within 0.05 of each other on
    this sheared phantom and are not asserted).  Fused and composed give the same ranks and scores within ``SCORE_TOL``."""
    from nesvor_amd.assess import choose_template

    c = _sets(device)
    stacks = _set_a(device)
    worst = 0.0
    fused, composed = _both_paths(stacks, "ncc", monkeypatch)
    print("ncc, Set A: fused", [r["score"] for r in fused], "composed", [r["score"] for r in composed])
    assert [r["rank"] for r in fused] == [2, 1, 0] and [r["rank"] for r in composed] == [2, 1, 0]
    assert [r["stack_idx"] for r in fused] == [0, 1, 2] and [r["n_slices"] for r in fused] == [r["n_slices"] for r in composed]
    assert all(r["n_slices"] <= 22 for r in fused)
    for s, oracle in zip([r["score"] for r in composed], (0.054, 0.654, 0.759)):
        assert abs(s - oracle) < 2e-3  # the values recorded from the CPU oracle, to their printed digits
    assert choose_template(stacks, "auto", "ncc") == 2
    results = {"ncc": [(fused, composed)], "matrix-rank": [], "volume": []}
    for metric in ("matrix-rank", "volume"):
        results[metric].append(_both_paths(stacks, metric, monkeypatch))
    still, moved = _stacks(c["still"], c["poses"]), _stacks(c["moved"], c["poses"])
    for metric in ("ncc", "matrix-rank"):
        results[metric].append(_both_paths(still, metric, monkeypatch))
        results[metric].append(_both_paths(moved, metric, monkeypatch))
    for metric, runs in results.items():
        for f, g in runs:
            assert [r["rank"] for r in f] == [r["rank"] for r in g], metric
            diffs = [abs(a["score"] - b["score"]) for a, b in zip(f, g)]
            print(f"{metric}: fused {[r['score'] for r in f]} |fused - composed| {diffs}")
            if metric == "volume":
                assert diffs == [0.0, 0.0, 0.0]  # counts are exact
            else:
                worst = max(worst, *diffs)
    print(f"largest |fused - composed| score difference (ncc, matrix-rank): {worst:.3e} (asserted at {SCORE_TOL:g})")
    assert worst <= SCORE_TOL
    (s_f, _), (m_f, _) = results["matrix-rank"][1], results["matrix-rank"][2]
    print("matrix-rank still", [r["score"] for r in s_f], "moved", [r["score"] for r in m_f])
    for j, (oracle_still, oracle_moved) in ((1, (-0.636, -0.773)), (2, (-0.607, -0.835))):
        assert s_f[j]["score"] > m_f[j]["score"]
        assert abs(s_f[j]["score"] - oracle_still) < 2e-3 and abs(m_f[j]["score"] - oracle_moved) < 2e-3
    vol = results["volume"][0][0]
    masks = [int((s.slices > 0).sum()) for s in stacks]
    assert [r["score"] for r in vol] == [m * _RES_S * _RES_S * _THICK for m in masks]


# ---------------------------------------------------------------------------------------------------------------------
# the template stack
# ---------------------------------------------------------------------------------------------------------------------
_DEFAULT = {}


def _registered_default(device):
    """Set A after ``register_stacks`` as every caller had it so far (no ``template``); run once."""
    if not _DEFAULT:
        from nesvor_amd.registration import register_stacks

        _DEFAULT["stacks"] = register_stacks(_set_a(device), res_s=_RES_S)
    return _DEFAULT["stacks"]


@pytest.mark.gpu
def test_template_zero_is_the_old_path(device):
    from nesvor_amd.registration import register_stacks

    old = _registered_default(device)
    new = register_stacks(_set_a(device), res_s=_RES_S, template=0)
    for a, b in zip(old, new):
        assert torch.equal(a.transformation.matrix(), b.transformation.matrix())
    with pytest.raises(ValueError):
        register_stacks(_set_a(device), res_s=_RES_S, template=3)


@pytest.mark.gpu
def test_template_two_centres_the_frame_on_stack_two(device):
    """The list keeps its order and its objects; stack 2's poses are  centre o its own mean pose o slice offsets, what
    ``stack_registration`` builds for its target (stack 0 so far)."""
    from nesvor_amd.registration import register_stacks
    from nesvor_amd.transform import RigidTransform

    c = _sets(device)
    stacks = _set_a(device)
    before = [s.slices.clone() for s in stacks]
    out = register_stacks(stacks, res_s=_RES_S, template=2)
    assert out is stacks and len(out) == 3
    for s, img in zip(out, before):
        assert torch.equal(s.slices, img)

    def target_poses(nominal, n):
        mean = RigidTransform(nominal.axisangle().mean(0, keepdim=True))
        centre = mean.axisangle(trans_first=False).clone()
        centre[..., :3] = 0
        centre[..., 3:] *= -1
        t = torch.zeros((n, 6), dtype=torch.float32, device=device)
        t[:, -1] = (torch.arange(n, dtype=torch.float32, device=device) - (n - 1) / 2) * _THICK
        return RigidTransform(centre).compose(mean).compose(RigidTransform(t)).matrix()

    torch.testing.assert_close(out[2].transformation.matrix(), target_poses(c["poses"][2], 22), rtol=0, atol=1e-5)
    old = _registered_default(device)
    torch.testing.assert_close(old[0].transformation.matrix(), target_poses(c["poses"][0], 22), rtol=0, atol=1e-5)  # the same check, stack 0
    assert not torch.allclose(out[0].transformation.matrix(), old[0].transformation.matrix(), atol=1e-3)  # another world frame


def _nifti_stacks(device, tmp_path):
    """Set A as NIfTI files (written as tests/test_gpu_robust.py::_moving_stacks writes its stacks); also the (stack, slice)
    pairs of the non-empty slices."""
    from nesvor_amd.image import Volume
    from nesvor_amd.transform import RigidTransform

    paths, nonempty = [], []
    for j, st in enumerate(_set_a(device)):
        img = st.slices[:, 0].contiguous()
        nonempty += [(j, k) for k in torch.nonzero((img > 0).flatten(1).any(1)).flatten().tolist()]
        ax = st.transformation.axisangle().mean(0, keepdim=True)  # stack centre pose
        p = str(tmp_path / f"stack{j}.nii.gz")
        Volume(img, img > 0, RigidTransform(ax), _RES_S, _RES_S, _THICK).save(p, masked=False)
        paths.append(p)
    return paths, nonempty


@pytest.mark.gpu
def test_cli_template_stack_auto_and_assess(tmp_path, device, monkeypatch):
    from nesvor_amd import cli, registration

    monkeypatch.delenv("NESVOR_ASSESS", raising=False)
    paths, nonempty = _nifti_stacks(device, tmp_path)
    templates, written = [], []
    inner_register, inner_outputs = registration.register_stacks, cli._outputs
    # (the command passes ``template=``; the call register_stacks makes on the re-ordered list does not)
    monkeypatch.setattr(registration, "register_stacks",
                        lambda ds, *a, **k: ("template" in k and templates.append(k["template"])) or inner_register(ds, *a, **k))
    monkeypatch.setattr(cli, "_outputs", lambda data, args: written.append(data) or inner_outputs(data, args))
    common = ["register", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--registration", "stack"]
    auto, first, log = str(tmp_path / "auto"), str(tmp_path / "first"), str(tmp_path / "log.txt")
    cli.main(common + ["--output-slices", auto, "--template-stack", "auto", "--output-log", log])
    text = open(log).read()
    assert "Template stack: 2" in text and "Stack assessment (ncc" in text
    cli.main(common + ["--output-slices", first, "--template-stack", "0", "--verbose", "0"])
    assert templates == [2, 0]
    count = lambda d: len([f for f in os.listdir(d) if f.endswith(".nii.gz") and not f.startswith("mask")])
    assert count(auto) == count(first) == len(nonempty) > 30
    for data in written:
        assert [(s.stack_idx, s.slice_idx) for s in data["output_slices"]] == nonempty  # input order, whatever the template
    # --registration none: the flags are ignored with a warning
    none, log2 = str(tmp_path / "none"), str(tmp_path / "log2.txt")
    cli.main(["register", "--input-stacks", *paths, "--registration", "none", "--template-stack", "auto", "--output-slices", none,
              "--output-log", log2])
    assert templates == [2, 0] and "ignored" in open(log2).read() and count(none) == len(nonempty)
    with pytest.raises(SystemExit, match="3 input stacks"):
        cli.main(common + ["--output-slices", str(tmp_path / "never"), "--template-stack", "7", "--verbose", "0"])
    # the assess command
    out = str(tmp_path / "assess.json")
    cli.main(["assess", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--output-json", out, "--verbose", "0"])
    rows = json.load(open(out))
    assert len(rows) == 3 and {r["rank"] for r in rows} == {0, 1, 2} and [r["rank"] for r in rows] == [2, 1, 0]
    assert [r["input_stack"] for r in rows] == paths and [r["stack_idx"] for r in rows] == [0, 1, 2]
    assert all(set(r) == {"stack_idx", "n_slices", "metric", "score", "rank", "input_stack"} and r["metric"] == "ncc" for r in rows)
    cli.main(["assess", "--input-stacks", *paths, "--metric", "volume", "--output-json", out, "--verbose", "0"])
    assert {r["rank"] for r in json.load(open(out))} == {0, 1, 2}
