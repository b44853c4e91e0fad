"""Robust statistics of the classical reconstruction (nesvor_amd/robust.py) on host tensors in fp64 - the composed path, which
is also the yardstick of tests/test_gpu_robust.py -, the ``svr`` command's flags and ``reconstruct_volume``'s plain path."""
import math

import pytest
import torch

N, H, W = 36, 19, 23
EMPTY = 5  # the fully masked slice
NOISE = 0.02


def _synthetic(seed, corrupted):
    """36 slices of 19 x 23: sim = 0.5 + 0.4 sin(3x + phi_k) cos(2y + phi_k), y = (sim + noise) / gain_k with +0.8 on 1 % of the
    pixels, a random mask of 80 %, slice 5 fully masked; the slices in ``corrupted`` have their pixels permuted.  x and y run
    over [0, pi], so every slice shows more than a full period in both directions whatever its phase: a permutation of a slice
    that is nearly flat would be no outlier."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, math.pi, H, dtype=torch.float64), torch.linspace(0, math.pi, W, dtype=torch.float64), indexing="ij")
    phi = 2 * math.pi * torch.rand(N, generator=g, dtype=torch.float64)
    sim = 0.5 + 0.4 * torch.sin(3 * xx[None] + phi[:, None, None]) * torch.cos(2 * yy[None] + phi[:, None, None])
    gain = 0.7 + 0.6 * torch.rand(N, generator=g, dtype=torch.float64)
    y = (sim + NOISE * torch.randn(N, H, W, generator=g, dtype=torch.float64)) / gain[:, None, None]
    spikes = torch.rand(N, H, W, generator=g) < 0.01
    y = y + 0.8 * spikes
    mask = torch.rand(N, H, W, generator=g) < 0.8
    mask[EMPTY] = False
    for k in corrupted:
        y[k] = y[k].flatten()[torch.randperm(H * W, generator=g)].view(H, W)
    return sim[:, None].contiguous(), y[:, None].contiguous(), mask[:, None].contiguous(), gain, spikes[:, None]


def _five_rounds(sim, y, mask):
    from nesvor_amd.robust import RobustStatistics

    rs = RobustStatistics().init(sim, y, mask)
    assert float(rs.c) == 0.9 and bool((rs.scale == 1).all()) and bool((rs.slice_weight == 1).all())
    history = []
    for _ in range(5):
        rs.update(sim, y, mask)
        history.append(rs.slice_weight.clone())
    return rs, history


def test_parser_has_the_robust_flags_and_keeps_the_other_defaults():
    from nesvor_amd.cli import build_parser

    p = build_parser()
    base = ["svr", "--input-stacks", "a.nii.gz", "b.nii.gz", "--output-volume", "v.nii.gz"]
    a = p.parse_args(base)
    assert a.outlier_rejection is False and a.robust_rounds == 3 and a.slice_weights is None
    b = p.parse_args(base + ["--outlier-rejection", "--robust-rounds", "5", "--slice-weights", "w.json"])
    assert b.outlier_rejection is True and b.robust_rounds == 5 and b.slice_weights == "w.json"
    new = {"outlier_rejection", "robust_rounds", "slice_weights"}
    va, vb = vars(a), vars(b)
    assert new <= set(va) and {k: v for k, v in va.items() if k not in new} == {k: v for k, v in vb.items() if k not in new}
    assert a.n_iter_srr == 30 and a.srr_beta == 0.02 and a.srr_delta == 0.1 and a.registration == "svr"
    assert a.simulated_slices is None and a.output_resolution == 0.8


def test_init_follows_its_definition():
    from nesvor_amd.robust import RobustStatistics

    sim, y, mask, _, _ = _synthetic(0, ())
    rs = RobustStatistics().init(sim, y, mask)
    yv = y[mask]
    assert float(rs.m) == pytest.approx(1 / (2.1 * float(yv.max()) - 1.9 * float(yv.min())), rel=1e-12)
    assert float(rs.sigma2) == pytest.approx(float(((y - sim)[mask] ** 2).mean()), rel=1e-12)
    assert rs.p.shape == sim.shape and rs.p.dtype == torch.float64 and bool((rs.p[~mask] == 0).all())
    assert rs.stats.shape == (N, 7) and torch.equal(rs.stats[:, 0], mask.flatten(1).sum(1).double())
    assert bool((rs.stats[EMPTY] == 0).all())


def test_em_rejects_three_permuted_slices_and_recovers_the_gains():
    bad = (3, 17, 30)
    sim, y, mask, gain, spikes = _synthetic(1, bad)
    rs, history = _five_rounds(sim, y, mask)
    w = rs.slice_weight
    good = [k for k in range(N) if k not in bad and k != EMPTY]
    print("weights", [round(float(v), 4) for v in w], "sigma", float(rs.sigma2) ** 0.5, "c", float(rs.c))
    print("largest scale error", float((rs.scale - gain)[good].abs().max()))
    assert all(float(w[k]) < 0.05 for k in bad)
    assert all(float(w[k]) > 0.99 for k in good)
    assert float(w[EMPTY]) == 0.0
    assert float((rs.scale - gain)[good].abs().max()) < 0.02
    assert 0.018 <= math.sqrt(float(rs.sigma2)) <= 0.025
    on_good = torch.zeros_like(mask)
    on_good[good] = True
    spiked = spikes & mask & on_good
    assert int(spiked.sum()) > 50 and float(rs.p[spiked].mean()) < 0.1
    assert torch.equal(rs.weights(), rs.p * w[:, None, None, None]) and torch.equal(rs.scaled(y), rs.scale[:, None, None, None] * y)


@pytest.mark.parametrize("seed", [2, 3, 4, 5])
def test_em_rejects_nothing_on_clean_slices(seed):
    sim, y, mask, _, _ = _synthetic(seed, ())
    _, history = _five_rounds(sim, y, mask)
    valid = torch.ones(N, dtype=torch.bool)
    valid[EMPTY] = False
    for w in history:
        assert bool((w[valid] == 1).all()) and float(w[EMPTY]) == 0.0


def test_em_rejects_ten_permuted_slices():
    bad = (0, 3, 8, 11, 14, 17, 22, 27, 30, 33)
    sim, y, mask, _, _ = _synthetic(6, bad)
    rs, _ = _five_rounds(sim, y, mask)
    w = rs.slice_weight
    print("weights", [round(float(v), 4) for v in w])
    assert all(float(w[k]) < 0.05 for k in bad)
    assert all(float(w[k]) > 0.99 for k in range(N) if k not in bad and k != EMPTY)


def test_composed_is_forced_by_the_switch_and_the_state_stays_tensors(monkeypatch):
    """The switch routes through ``estep_composed`` (host tensors take it anyway); the statistics are tensors throughout.  That
    a round reads nothing back to the host is checked on the GPU (tests/test_gpu_robust.py)."""
    from nesvor_amd import robust

    sim, y, mask, _, _ = _synthetic(7, (3,))
    calls = []
    inner = robust.estep_composed
    monkeypatch.setattr(robust, "estep_composed", lambda *a: calls.append(1) or inner(*a))
    monkeypatch.setenv("NESVOR_ROBUST", "composed")
    rs = robust.RobustStatistics().init(sim, y, mask).update(sim, y, mask)
    assert len(calls) == 2
    for t in (rs.sigma2, rs.c, rs.m):
        assert isinstance(t, torch.Tensor) and t.ndim == 0 and t.dtype == torch.float64
    assert rs.scale.shape == rs.slice_weight.shape == (N,)


class _DenseOp:
    """A small dense acquisition operator given as two closures: A (m x n) on the flattened volume."""

    def __init__(self, A, volume_shape, slices_shape):
        self.transforms = None
        self.forward = lambda x: (A @ x.reshape(-1)).reshape(slices_shape)
        self.adjoint = lambda y, equalize=False: (A.t() @ y.reshape(-1)).reshape(volume_shape)


def _dense_pipeline(monkeypatch):
    """``reconstruct_volume`` with its geometry replaced by a dense operator; records what ``srr_descent`` receives."""
    from nesvor_amd import svr

    g = torch.Generator().manual_seed(13)
    vshape, sshape = (1, 1, 3, 4, 5), (6, 1, 4, 5)
    A = torch.rand(120, 60, generator=g, dtype=torch.float64) / 60
    op = _DenseOp(A, vshape, sshape)
    images = torch.rand(sshape, generator=g, dtype=torch.float64) + 0.1
    m = torch.ones(sshape, dtype=torch.bool)
    start = torch.rand(vshape, generator=g, dtype=torch.float64)
    monkeypatch.setattr(svr, "_frame_keep", lambda slices, mask, poses, res_s: (images, m, None, torch.arange(6)))
    monkeypatch.setattr(svr, "_cover_shape", lambda *a: vshape[-3:])
    monkeypatch.setattr(svr, "_operator", lambda *a: (op, {}))
    monkeypatch.setattr(svr, "PSFreconstruction", lambda *a: start)
    calls = []
    inner = svr.srr_descent

    def spy(op_, slices, volume, n_iter, beta, delta, p=None, **k):
        calls.append({"slices": slices, "volume": volume, "n_iter": n_iter, "p": p})
        return inner(op_, slices, volume, n_iter, beta, delta, p=p, **k)

    monkeypatch.setattr(svr, "srr_descent", spy)
    return svr, images, start, calls


def test_robust_rounds_zero_is_the_plain_pipeline(monkeypatch):
    svr, images, start, calls = _dense_pipeline(monkeypatch)
    out = {}
    vol = svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=4, robust_rounds=0, robust_out=out)
    assert len(calls) == 1 and calls[0]["p"] is None and calls[0]["slices"] is images and calls[0]["volume"] is start
    assert calls[0]["n_iter"] == 4 and out == {}
    default = svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=4)
    assert len(calls) == 2 and calls[1]["p"] is None and torch.equal(default.image, vol.image)


def test_robust_rounds_split_the_steps_and_pass_weights_and_scaled_slices(monkeypatch):
    svr, images, start, calls = _dense_pipeline(monkeypatch)
    out = {}
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=11, robust_rounds=3, robust_out=out)
    assert [c["n_iter"] for c in calls] == [3, 3, 5]
    assert calls[0]["volume"] is start
    for c in calls:
        assert c["p"] is not None and c["p"].shape == images.shape and float(c["p"].min()) >= 0 and float(c["p"].max()) <= 1
        assert c["slices"].shape == images.shape
    assert out["slice_weight"].shape == out["scale"].shape == (6,) and out["keep"].tolist() == list(range(6))
    assert torch.equal(calls[-1]["slices"], out["scale"].view(-1, 1, 1, 1) * images)


def test_more_rounds_than_steps_are_cut_to_the_steps(monkeypatch):
    svr, images, start, calls = _dense_pipeline(monkeypatch)
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=2, robust_rounds=5)
    assert [c["n_iter"] for c in calls] == [1, 1]
    del calls[:]
    svr.reconstruct_volume(None, None, None, 1.5, 3.0, 1.0, n_iter=0, robust_rounds=3)
    assert [c["n_iter"] for c in calls] == [0]


def test_slice_weights_without_outlier_rejection_is_refused():
    from argparse import Namespace

    from nesvor_amd.svr import svr_command

    args = Namespace(input_slices="nowhere", input_stacks=None, stack_masks=None, thicknesses=None, device=torch.device("cpu"),
                     outlier_rejection=False, robust_rounds=3, slice_weights="w.json")
    with pytest.raises(SystemExit, match="--slice-weights needs --outlier-rejection"):
        svr_command(args)


def test_stacks_to_slices_carries_stack_and_slice_indices():
    from nesvor_amd.cli import stacks_to_slices
    from nesvor_amd.image import Stack
    from nesvor_amd.transform import RigidTransform

    g = torch.Generator().manual_seed(3)
    stacks = []
    for n, empty in ((4, (0,)), (5, (2, 4))):
        img = torch.rand(n, 1, 6, 7, generator=g) + 0.5
        mask = torch.ones_like(img, dtype=torch.bool)
        for k in empty:
            mask[k] = False
        pose = RigidTransform(torch.eye(3, 4)[None].repeat(n, 1, 1))  # (as matrices: the axis-angle conversion is a HIP kernel)
        stacks.append(Stack(img, mask, pose, resolution_x=1.5, resolution_y=1.5, thickness=3.0, gap=3.0))
    slices = stacks_to_slices(stacks)
    assert [(s.stack_idx, s.slice_idx) for s in slices] == [(0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 3)]
