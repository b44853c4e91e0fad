"""tests/svr_reference.py on the CPU: the accepted seeds meet their two conditions, no case is silently empty, and ``sums`` is
the plain loop."""
import pytest
import torch

import svr_reference as R
from acq_geometry import GEOMETRIES, OUTSIDE

CASES = [(g, None) for g in GEOMETRIES] + [("even", p) for p in R.SPECIAL_PSFS if p != "all_zero"]


@pytest.mark.parametrize("geom,psf", CASES, ids=[p or g for g, p in CASES])
def test_seeds_meet_the_cpu_conditions_and_no_case_is_empty(geom, psf):
    """Generic poses: the fp32 and the fp64 oracle have equal valid sets and their images agree within the per-pixel bound.
    Lattice poses: the OUTSIDE pose has no valid pixel; identity, rotation, permutation and the half-outside pose keep some and
    the set as a whole keeps at least 5 % (the (0.5, -1, 2) move leaves the (2,2,2) volume, and a single off-centre tap leaves it
    under some poses)."""
    c = R.case(geom, psf)
    flips, ratio = R.seed_report(c)
    _, w32 = R.images(c, torch.float32)
    valid = (w32 > 0).flatten(1).double().mean(1)
    print(f"{geom} {psf}: validity flips {flips}, largest |I32 - I64| / bound {ratio:.3f}, valid share per pose {[round(float(v), 2) for v in valid]}")
    assert flips == 0 and ratio <= 1
    assert len({tuple(p.flatten().tolist()) for p in c.poses}) == R.K_POSES  # every pose distinct
    others = [k for k in range(R.N_LATTICE) if k != OUTSIDE]
    assert float(valid[OUTSIDE]) == 0 and float(valid[others].mean()) >= 0.05
    assert bool((valid[[0, 1, 2, 5]] > 0).all())
    assert float(valid[R.N_LATTICE:].mean()) >= 0.05  # the generic poses see the volume
    h, w = c.shape
    assert 256 * ((h * w - 1) // 256) <= c.last_pixel < h * w and int((w32.view(R.K_POSES, -1)[:, c.last_pixel] > 0).sum()) >= 2
    assert int(c.masks["last_pixel"].sum()) == 5 and bool(c.masks["last_pixel"].view(5, -1)[:, c.last_pixel].all())
    if geom not in ("tiny", "odd") and psf is None:  # (a volume 2 or 5 voxels thick: a 3-voxel move along z can leave it)
        assert bool((valid[R.N_LATTICE:] > 0).all())
    else:
        assert int((valid[R.N_LATTICE:] > 0).sum()) >= 7


def test_all_zero_psf_has_no_valid_pixel():
    c = R.case("even", "all_zero")
    I, w = R.images(c, torch.float32)
    assert float(w.abs().max()) == 0 and float(I.abs().max()) == 0


def test_sums_equal_the_plain_loop():
    c = R.case("tiny")
    I, w = R.images(c, torch.float32)
    h, wd = c.shape
    for name in R.MASKS:
        mask = c.masks[name]
        got = R.sums(I, w, c.J, mask)
        assert got.shape == (5, R.K_POSES, 6) and got.dtype == torch.float64
        for i in range(5):
            for k in range(R.K_POSES):
                acc = [0.0] * 6
                for y in range(h):
                    for x in range(wd):
                        if (mask is None or bool(mask[i, y, x])) and float(w[k, y, x]) > 0:
                            a, b = float(I[k, y, x]), float(c.J[i, y, x])
                            for j, t in enumerate((1.0, a, a * a, a * b, b, b * b)):
                                acc[j] += t
                torch.testing.assert_close(got[i, k], torch.tensor(acc, dtype=torch.float64), rtol=1e-13, atol=0)
    assert float(R.sums(I, w, c.J, None)[..., 0].max()) > 0
    assert torch.equal(R.sums(I, w, c.J, c.masks["slice_off"])[1], torch.zeros(R.K_POSES, 6, dtype=torch.float64))


def test_bounds_are_the_derived_ones():
    """One pixel by hand: I = 0.5, J = 0.25 -> e = 6e-5; bounds {0, e, 2 I e + e^2, J e, 0, ulp(1/16)}; an aggregated bound is the
    pixels' bounds added plus 8 x 2^-24 of the sum."""
    I, J, w = torch.full((1, 1, 2), 0.5), torch.full((1, 1, 2), 0.25), torch.tensor([[[1.0, 0.0]]])
    e = 1e-4 * 0.5 + 1e-5
    b = R.pixel_bounds(I, J)
    expect = torch.tensor([0, e, 2 * 0.5 * e + e * e, 0.25 * e, 0, 2.0 ** -27], dtype=torch.float64)
    torch.testing.assert_close(b[0, 0, 0], expect, rtol=1e-12, atol=0)
    v = R.pixel_values(I, w, J)
    assert torch.equal(v[0, 0, 0], torch.tensor([1, 0.5, 0.25, 0.125, 0.25, 0.0625], dtype=torch.float64)) and float(v[0, 0, 1].abs().max()) == 0
    s = R.sums(I, w, J, None)
    assert torch.equal(s[0, 0], v[0, 0, 0])
    sb = R.sum_bounds(I, w, J, None, s)
    term = 8 * 2.0 ** -24 * s[0, 0]
    term[0] = 0
    torch.testing.assert_close(sb[0, 0], expect + term, rtol=1e-12, atol=0)
    assert torch.equal(R.pose_ids(3, 2), torch.tensor([[0, 1], [1, 2], [2, 3]]))
