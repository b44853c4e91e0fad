"""CPU: tests/hashgrid_reference.py (the yardstick of tests/test_gpu_hashgrid_grids.py) against the oracle it restates -
``oracle.hashgrid.encode``, its autograd (``encode_backward``) and the published formulas (``encode_backward_explicit``) - on three
small grids with dense and hashed levels, at one, two and eight features per entry.

The oracle forms the corner weights in the dtype of its positions, float32 for float32 points, whatever the table's dtype.  To
compare at float64 accuracy the tests hand it the SAME positions - ``_pos``'s value, rounded once to float32 - as float64 numbers:
cells and indices are then those of float32 points, and everything behind them is float64 on both sides.
"""
import pytest
import torch

import hashgrid_reference as R
from oracle import hashgrid as O

GRIDS = [(6, 1, 9, 4, 1.6), (8, 2, 10, 5, 1.5), (5, 8, 8, 3, 1.7)]


@pytest.fixture()
def float64_behind_the_position(monkeypatch):
    pos32 = O._pos

    def pos(u, scale):
        p = pos32(u, scale)
        assert p.dtype == torch.float32
        return p.double()

    monkeypatch.setattr(O, "_pos", pos)


def _case(spec):
    L, F = spec[0], spec[1]
    lv = R.levels_of(spec)
    assert any(l.hashed for l in lv) and not all(l.hashed for l in lv)
    g = torch.Generator().manual_seed(L * 10 + F)
    u = torch.rand(700, 3, generator=g)
    u[0], u[1], u[2] = 0.0, 1.0, torch.tensor([0.0, 0.3, 1.0])
    table = torch.randn(O.n_params(lv, F), generator=g, dtype=torch.float64)
    dy = torch.randn(700, L * F, generator=g, dtype=torch.float64)
    return lv, u, table, dy


@pytest.mark.parametrize("spec", GRIDS, ids=lambda s: "L%d_F%d" % (s[0], s[1]))
def test_reference_equals_the_oracle_in_float64(spec, float64_behind_the_position):
    L, F = spec[0], spec[1]
    lv, u, table, dy = _case(spec)
    pos = O._pos(u, lv[-1].scale)
    assert pos.dtype == torch.float64 and torch.equal(pos, pos.float().double())
    pe, gt, gu = R.reference(spec, u, table, dy)
    assert pe.dtype == gt.dtype == gu.dtype == torch.float64
    assert tuple(pe.shape) == (700, L, F) and tuple(gt.shape) == tuple(table.shape) and tuple(gu.shape) == (L, 700, 3)
    pe_o = O.encode(u, table, lv, F)
    assert pe_o.dtype == torch.float64
    torch.testing.assert_close(pe.reshape(700, L * F), pe_o, rtol=1e-12, atol=0)
    gt_a, gu_a = O.encode_backward(u, table, lv, F, dy)
    gt_e, gu_e = O.encode_backward_explicit(u, table, lv, F, dy)
    assert gt_a.dtype == gt_e.dtype == torch.float64
    torch.testing.assert_close(gt, gt_e, rtol=1e-12, atol=0)
    torch.testing.assert_close(gt, gt_a, rtol=1e-12, atol=0)
    # the oracle's input gradient is float32 (the dtype of u): the finest levels dominate the sum
    assert gu_a.dtype == gu_e.dtype == torch.float32
    total = gu.sum(0)
    torch.testing.assert_close(total, gu_a.double(), rtol=1e-6, atol=1e-6 * float(total.abs().max()))
    torch.testing.assert_close(total, gu_e.double(), rtol=1e-6, atol=1e-6 * float(total.abs().max()))


def test_reference_positions_are_the_float32_ones():
    """Without the patch above: the helper's cells are the oracle's for float32 points (a float64 product would put points that
    round up onto a lattice plane into the cell below), and its values agree with the all-float32 oracle to float32 accuracy."""
    spec = GRIDS[1]
    lv, u, table, dy = _case(spec)
    pe, gt, gu = R.reference(spec, u, table, dy)
    pe32 = O.encode(u, table.float(), lv, spec[1])
    torch.testing.assert_close(pe.reshape(700, -1).float(), pe32, rtol=1e-5, atol=1e-5)
    gt32, gu32 = O.encode_backward(u, table.float(), lv, spec[1], dy.float())
    torch.testing.assert_close(gt.float(), gt32, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gu.sum(0).float(), gu32, rtol=1e-4, atol=1e-4 * float(gu32.abs().max()))
    # per level: a level's share is what dy restricted to that level's columns gives, and nothing else
    F = spec[1]
    for li in range(len(lv)):
        only = torch.zeros_like(dy)
        only[:, li * F : (li + 1) * F] = dy[:, li * F : (li + 1) * F]
        _, _, gu_l = R.reference(spec, u, table, only)
        assert torch.equal(gu_l[li], gu[li]) and int(torch.count_nonzero(gu_l)) == int(torch.count_nonzero(gu_l[li])) > 0
