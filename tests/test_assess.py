"""Stack assessment, host side (no GPU): the torch expression of the pair moments against a plain numpy loop, the scores
from hand-made moments, the index validation of ``pair_moments``, the parser and ``choose_template``."""
import math

import numpy as np
import pytest
import torch

PAIRS = [(0, 1), (1, 2), (2, 2), (0, 1), (1, 0), (3, 4), (2, 3), (4, 0), (3, 3)]  # a self-pair, a repeat, a reversal; slice 3 is empty


def _stack(seed=0):
    g = torch.Generator().manual_seed(seed)
    x = 1 + 0.5 * torch.randn(5, 7, 9, generator=g)
    mask = torch.rand(5, 7, 9, generator=g) < 0.6
    mask[3] = False
    return x, mask


def _loop(x, mask, pairs):
    """{count, sum a, sum b, sum a^2, sum b^2, sum a b} pixel by pixel in fp64."""
    x = x.double().numpy().reshape(x.shape[0], -1)
    m = None if mask is None else mask.numpy().reshape(x.shape[0], -1) != 0
    out = np.zeros((len(pairs), 6))
    for p, (ia, ib) in enumerate(pairs):
        for k in range(x.shape[1]):
            if m is not None and not (m[ia, k] and m[ib, k]):
                continue
            a, b = x[ia, k], x[ib, k]
            out[p] += (1.0, a, b, a * a, b * b, a * b)
    return out


@pytest.mark.parametrize("kind", ["none", "bool", "uint8"])
def test_composed_moments_against_a_numpy_loop(kind):
    from nesvor_amd.assess import pair_moments, pair_moments_composed

    x, mask = _stack()
    mask = {"none": None, "bool": mask, "uint8": mask.to(torch.uint8)}[kind]
    ref = _loop(x, mask, PAIRS)
    got = pair_moments_composed(x, mask, torch.tensor(PAIRS))
    assert got.dtype == torch.float64 and got.shape == (len(PAIRS), 6)
    assert np.array_equal(got[:, 0].numpy(), ref[:, 0])
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-12, atol=0)
    if mask is not None:  # every pair with the empty slice: count 0 and all sums exactly 0
        for p, pair in enumerate(PAIRS):
            if 3 in pair:
                assert bool((got[p] == 0).all())
    else:
        assert bool((got[:, 0] == 63).all())
    assert torch.equal(got[0], got[3])  # the repeated pair
    assert torch.equal(got[4], got[0][[0, 2, 1, 4, 3, 5]])  # the reversed pair: columns 1 <-> 2, 3 <-> 4
    # host tensors take the composed path through the public entry, (n, 1, h, w) and lists included
    again = pair_moments(x[:, None], None if mask is None else mask[:, None], PAIRS)
    assert torch.equal(again, got)
    assert pair_moments(x, mask, []).shape == (0, 6)


def _moments(a, b, mask=None):
    from nesvor_amd.assess import pair_moments_composed

    x = torch.stack([torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)])[:, None]
    m = None if mask is None else torch.stack([torch.as_tensor(mask), torch.as_tensor(mask)])[:, None]
    return pair_moments_composed(x, m, torch.tensor([[0, 1]]))


def test_ncc_from_hand_made_moments():
    from nesvor_amd.assess import MIN_OVERLAP, ncc_of_pairs, ncc_score, rank_scores

    assert MIN_OVERLAP == 16
    a = torch.arange(20.0)
    same, opposite = _moments(a, a), _moments(a, -a)
    assert torch.equal(same, torch.tensor([[20.0, 190.0, 190.0, 2470.0, 2470.0, 2470.0]], dtype=torch.float64))
    assert ncc_score(same) == pytest.approx(1.0, abs=1e-12)
    assert ncc_score(opposite) == pytest.approx(-1.0, abs=1e-12)
    assert ncc_score(_moments(a, 3 * a + 2)) == pytest.approx(1.0, abs=1e-12)
    constant = _moments(a, torch.full((20,), 2.0))
    assert not bool(ncc_of_pairs(constant)[1].any()) and math.isnan(ncc_score(constant))
    few = torch.zeros(20, dtype=torch.bool)
    few[:MIN_OVERLAP - 1] = True
    small = _moments(a, a, few)
    assert small[0, 0] == MIN_OVERLAP - 1 and math.isnan(ncc_score(small))
    few[MIN_OVERLAP - 1] = True
    assert ncc_score(_moments(a, a, few)) == pytest.approx(1.0, abs=1e-12)
    # skipped pairs do not enter the mean
    assert ncc_score(torch.cat([same, constant, small, opposite, same])) == pytest.approx(1.0 / 3.0, abs=1e-12)
    assert math.isnan(ncc_score(torch.zeros((0, 6))))
    # nan ranks last, ties go to the lower index
    assert rank_scores([float("nan"), 0.5, 0.7]) == [2, 1, 0]
    assert rank_scores([0.5, 0.5, float("nan"), 0.9]) == [1, 2, 3, 0]
    assert rank_scores([float("nan"), float("nan")]) == [0, 1]


def test_matrix_rank_and_volume_from_hand_made_moments():
    from nesvor_amd.assess import (effective_rank, matrix_rank_score, pair_moments_composed, score_from_moments, stack_pairs,
                                   volume_score)

    k = 4
    assert effective_rank(3.0 * torch.eye(k, dtype=torch.float64)) == pytest.approx(k, rel=1e-12)
    assert matrix_rank_score(3.0 * torch.eye(k, dtype=torch.float64)) == pytest.approx(-1.0, rel=1e-12)
    # k mutually orthogonal equal-norm slices, through the moments of all pairs i <= j
    x = torch.zeros(k, 1, 2, 4)
    for i in range(k):
        x[i, 0, i // 4, i % 4] = 2.0
    pairs = stack_pairs(k, "matrix-rank")
    assert pairs == [(i, j) for i in range(k) for j in range(i, k)]
    m = pair_moments_composed(x, None, torch.tensor(pairs))
    assert score_from_moments(m, k, "matrix-rank") == pytest.approx(-1.0, rel=1e-12)
    # a rank-1 stack: every slice a multiple of one image
    g = torch.Generator().manual_seed(1)
    base = torch.rand(5, 6, generator=g)
    x = torch.stack([c * base for c in (1.0, 0.5, 2.0, 1.5)])[:, None]
    m = pair_moments_composed(x, None, torch.tensor(pairs))
    assert -k * score_from_moments(m, k, "matrix-rank") == pytest.approx(1.0, abs=1e-6)
    # two independent directions of equal weight: effective rank 2
    assert effective_rank(torch.diag(torch.tensor([4.0, 4.0, 0.0], dtype=torch.float64))) == pytest.approx(2.0, rel=1e-12)
    assert math.isnan(effective_rank(torch.zeros(3, 3)))
    # volume: masked pixels times the voxel volume
    mask = torch.zeros(3, 1, 5, 6, dtype=torch.bool)
    mask[0, 0, :2] = True
    mask[2, 0, 1:4, 2:5] = True
    m = pair_moments_composed(torch.ones(3, 1, 5, 6), mask, torch.tensor(stack_pairs(3, "volume")))
    assert m[:, 0].tolist() == [12.0, 0.0, 9.0]
    assert volume_score(m, 1.5 * 1.5 * 3.0) == pytest.approx(21 * 6.75, rel=1e-12)
    assert stack_pairs(4, "ncc") == [(0, 1), (1, 2), (2, 3)] and stack_pairs(1, "ncc") == []


def test_pair_moments_refuses_indices_out_of_range():
    from nesvor_amd.assess import pair_moments

    x, mask = _stack()
    for bad in ([(0, 5)], [(5, 0)], [(0, 1), (-1, 2)], torch.tensor([[0, 1], [2, 7]]), [(0, 1, 2)], [(0.5, 1.0)]):
        with pytest.raises(ValueError):
            pair_moments(x, mask, bad)
    assert pair_moments(x, mask, [(4, 4)]).shape == (1, 6)


def _cpu_stack(slices, mask=None, **kw):
    from nesvor_amd.image import Stack

    kw = {"resolution_x": 1.5, "resolution_y": 1.5, "thickness": 3.0, "gap": 3.0, **kw}
    return Stack(slices, slices > 0 if mask is None else mask, **kw)


def test_assess_stacks_on_host_tensors():
    """Stacks of different sizes with empty slices: non-empty slices in stack order, one dict per stack in input order."""
    from nesvor_amd.assess import assess_stacks, ncc_score, pair_moments_composed

    g = torch.Generator().manual_seed(3)
    smooth = torch.linspace(0, 1, 12 * 10).reshape(1, 1, 12, 10) + 0.1 * torch.arange(6).reshape(6, 1, 1, 1) + 0.5
    smooth[2] = 0  # an empty slice in the middle: its neighbours become an adjacent pair
    noisy = torch.rand(5, 1, 9, 14, generator=g) + 0.5
    stacks = [_cpu_stack(noisy), _cpu_stack(smooth)]
    rows = assess_stacks(stacks, "ncc")
    assert [r["stack_idx"] for r in rows] == [0, 1] and [r["n_slices"] for r in rows] == [5, 5]
    assert [r["rank"] for r in rows] == [1, 0] and all(r["metric"] == "ncc" for r in rows)
    kept = smooth[[0, 1, 3, 4, 5]]
    assert rows[1]["score"] == pytest.approx(ncc_score(pair_moments_composed(kept, kept > 0, torch.tensor([(i, i + 1) for i in range(4)]))), abs=1e-12)
    vol = assess_stacks(stacks, "volume")
    assert vol[0]["score"] == pytest.approx(5 * 9 * 14 * 6.75) and vol[1]["score"] == pytest.approx(5 * 12 * 10 * 6.75)
    rank = assess_stacks(stacks, "matrix-rank")
    assert rank[1]["score"] > rank[0]["score"]  # the smooth stack is of lower rank than noise
    with pytest.raises(ValueError):
        assess_stacks(stacks, "sharpness")


def test_parser_and_choose_template():
    from nesvor_amd import cli
    from nesvor_amd.assess import choose_template

    parser = cli.build_parser()
    a = parser.parse_args(["assess", "--input-stacks", "a.nii.gz", "b.nii.gz"])
    assert a.metric == "ncc" and a.output_json is None and a.stack_masks is None and a.thicknesses is None and a.verbose == 1
    a = parser.parse_args(["assess", "--input-stacks", "a.nii.gz", "--stack-masks", "m.nii.gz", "--thicknesses", "3", "--metric", "matrix-rank",
                           "--output-json", "o.json", "--device", "0"])
    assert a.metric == "matrix-rank" and a.output_json == "o.json" and a.thicknesses == [3.0]
    with pytest.raises(SystemExit):
        parser.parse_args(["assess", "--input-stacks", "a.nii.gz", "--metric", "sharpness"])
    for argv in (["reconstruct", "--input-stacks", "a.nii.gz"], ["register", "--input-stacks", "a.nii.gz", "--output-slices", "d"],
                 ["svr", "--input-stacks", "a.nii.gz", "--output-volume", "v.nii.gz"]):
        a = parser.parse_args(argv)
        assert a.template_stack == "0" and a.template_metric == "ncc"
        a = parser.parse_args(argv + ["--template-stack", "auto", "--template-metric", "volume"])
        assert a.template_stack == "auto" and a.template_metric == "volume"
    g = torch.Generator().manual_seed(0)
    img = torch.rand(4, 1, 8, 8, generator=g) + 0.5
    stacks = [_cpu_stack(img.clone()) for _ in range(3)]
    assert choose_template(stacks, "0", "ncc") == 0 and choose_template(stacks, "2", "ncc") == 2
    with pytest.raises(SystemExit, match="3 input stacks"):
        choose_template(stacks, "7", "ncc")
    with pytest.raises(SystemExit):
        choose_template(stacks, "-1", "ncc")
    with pytest.raises(SystemExit):
        choose_template(stacks, "best", "ncc")
    for metric in ("ncc", "matrix-rank", "volume"):
        assert choose_template(stacks, "auto", metric) == 0  # three equal stacks: the tie goes to the lower index
    stacks[1] = _cpu_stack(torch.cat([img, img[:1]]))  # one more slice: the largest volume
    assert choose_template(stacks, "auto", "volume") == 1
