"""CPU self-checks of tests/vvr_nmi_reference.py, the yardstick of tests/test_gpu_vvr_nmi.py: its constants are what its own
measurement gives, its case is what its docstring says, and its histograms and bounds are consistent.  No kernel involved."""
import pytest
import torch

import vvr_nmi_reference as N
from nesvor_amd import nmi


def test_the_recorded_coordinate_terms_are_what_the_measurement_gives():
    """COORD_MEASURED / COORD_MEASURED_ABS: the largest difference of the helper with fp32 and with fp64 coordinates over the case,
    relative to the point's V and to max |src|, re-measured here; the tolerances are 4 x the recorded values."""
    rel, absolute = N.measure_coord(N.case())
    print(f"largest |sample(fp32 coordinates) - sample(fp64 coordinates)|: {rel:.4e} V, {absolute:.4e} max |src|")
    assert rel == pytest.approx(N.COORD_MEASURED, rel=2e-3) and absolute == pytest.approx(N.COORD_MEASURED_ABS, rel=2e-3)
    assert N.COORD_TOL == 4 * N.COORD_MEASURED and N.COORD_TOL_ABS == 4 * N.COORD_MEASURED_ABS
    assert rel <= N.COORD_TOL / 3.99 and absolute <= N.COORD_TOL_ABS / 3.99


def test_the_case_is_what_the_docstring_says():
    c = N.case()
    assert tuple(c["src"].shape) == (6, 11, 9) and c["points"].shape == (70001, 3) and c["mats"].shape == (27, 3, 4)
    assert 0.30 <= N.outside_share(c) <= 0.40  # about a third of the points not wholly inside the source
    ones = torch.ones(N.SHAPE)
    for m in c["mats"]:
        share = float((N.R.sample(ones, c["points"], m, N.unit32(c)) < 1).double().mean())
        assert 0.25 <= share <= 0.55, share
    assert float(c["src"].min()) > 0.25  # no zero in the source: V = 0 is the zero padding alone
    assert max(N.MS) > 4 * 16384  # more than one segment at the longest segment the kernel takes


@pytest.mark.parametrize("bins", N.BINS)
def test_the_yardsticks_histograms_total_65536_m(bins):
    c = N.case()
    for K, M in ((3, 4001), (1, 257), (2, 1)):
        hist, bounds = N.histograms(c, K, M, bins)
        assert hist.shape == (K, bins, bins) and hist.dtype == torch.int64 and bounds.shape == (K, bins, bins)
        assert hist.sum((1, 2)).tolist() == [nmi.UNITS * M] * K
        assert bool((bounds >= 0).all())
        # the J marginal is the J weights' sum, whatever I is
        i_map, j_map = N.maps(c, M, bins)
        w_j = N.axis_weights(c["target"][:M], j_map[0], j_map[1], bins)
        assert torch.equal(hist.sum(1), (256 * w_j.sum(0))[None].expand(K, -1))
        # a cell with content has a bound, and the bound of a column is at least one unit per J weight of its points
        assert bool((bounds[hist > 0] > 0).all())


def test_the_bounds_cover_the_difference_of_the_two_references():
    """The fp32-coordinate reference stands in for a kernel: its histograms lie within the yardstick's bounds of the fp64 one
    (its samples differ by at most COORD_MEASURED V: a quarter of the tolerance)."""
    c = N.case()
    K, M = 5, 4001
    for bins in (5, 32):
        hist, bounds = N.histograms(c, K, M, bins)
        i_map, j_map = N.maps(c, M, bins)
        other = N.bin_samples(N.samples(c, torch.float32)[:K, :M].float(), c["target"][:M], i_map, j_map, bins)
        assert bool(((other - hist).abs().double() <= bounds).all())
