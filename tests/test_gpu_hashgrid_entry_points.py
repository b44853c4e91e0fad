"""The raw C entry points of the owner-computes hash-grid backward against each other.

``nesvor_amd.encoding`` reaches every backward through ``nesvor_hashgrid_backward_plan``; the thinner forms - ``_backward``,
``_levels``, ``_bounded`` - are called by csrc/step.hip and the tools only, so an argument that one of them forwards wrongly would
show late.  Here each is called through ctypes on one workspace, as a caller of the C ABI would: the smallest tested grid with a
dense and a hashed level, PSF-cloud points at N = 257 (one full workgroup and one of a single point) and N = 512, both layouts of
dpe.  All of them compute one backward, so they must agree within what the owner pass's summation order leaves open: the
tolerances of test_hashgrid_backward_split_by_levels on clustered points.
"""
import ctypes

import pytest
import torch

import hashgrid_reference as R

pytestmark = pytest.mark.gpu

GT_TOL = dict(rtol=1e-5, atol=1e-6)
GU_TOL = dict(rtol=1e-4, atol=1e-5)


def _grid():
    from nesvor_amd.grid import HashGridSpec

    specs = [HashGridSpec(*g[0]) for g in R.GRIDS.values() if g[3]]
    mixed = [s for s in specs if len({lv.hashed for lv in s.levels}) == 2]
    return min(mixed, key=lambda s: s.n_params)


def _psf_cloud(n_pix, S, seed):  # as tests/test_gpu_ops.py builds them
    g = torch.Generator().manual_seed(seed)
    c = torch.rand(n_pix, 1, 3, generator=g) * 110 + 10
    x = c + torch.randn(n_pix, S, 3, generator=g) * torch.tensor([0.77, 0.77, 1.27])
    return (x.reshape(-1, 3) / 130.0).clamp(0, 1).contiguous()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("N", [257, 512])
def test_backward_entry_points_agree(device, N, layout):
    from nesvor_amd import _lib

    lib = _lib.load()
    spec = _grid()
    L, F = spec.n_levels, spec.n_features
    split = next(i for i, lv in enumerate(spec.levels) if lv.hashed)  # [0, split) dense, [split, L) hashed
    assert 0 < split < L
    g = torch.Generator().manual_seed(5)
    u = _psf_cloud(2, 256, 9)[:N].contiguous().to(device)
    table = (torch.randn(spec.n_params, generator=g) * 0.1).to(device)
    dy = torch.randn((L * F, N) if layout else (N, L * F), generator=g).to(device)
    bound = dy.abs().max().reshape(1)
    grid = ctypes.byref(spec.c_struct)
    ws = torch.empty(lib.nesvor_hashgrid_backward_workspace_bytes(grid, N, None), dtype=torch.uint8, device=device)
    ws[: lib.nesvor_hashgrid_backward_workspace_zero_bytes()].zero_()
    AGG, OWN, ALL = _lib.HG_STAGE_AGGREGATE, _lib.HG_STAGE_OWNER, _lib.HG_STAGE_ALL
    LATER = _lib.HG_STAGE_KEEP | _lib.HG_STAGE_ACCUMULATE_U
    NULL = ctypes.c_void_p(0)

    def run(*calls):
        """-> (grad_table, grad_u) of the launches ``calls``, each f(the nine leading arguments, stream) -> error code."""
        gt = torch.zeros_like(table)
        gu = torch.full_like(u, float("nan"))  # (overwritten by the first launch)
        lead = (grid, _lib.ptr(u), _lib.ptr(table), _lib.ptr(dy), _lib.ptr(gt), _lib.ptr(gu), N, layout, _lib.ptr(ws))
        with torch.cuda.device(device):
            for f in calls:
                assert f(lead, _lib.stream_ptr()) == 0
        return gt, gu

    with torch.cuda.device(device):
        ref = run(lambda a, st: lib.nesvor_hashgrid_backward(*a, ALL, None, st))
        runs = {
            "stage 1 then 2": run(lambda a, st: lib.nesvor_hashgrid_backward(*a, AGG, None, st),
                                  lambda a, st: lib.nesvor_hashgrid_backward(*a, OWN, None, st)),
            "levels(0, L)": run(lambda a, st: lib.nesvor_hashgrid_backward_levels(*a, ALL, 0, L, None, st)),
            "bounded, no bound": run(lambda a, st: lib.nesvor_hashgrid_backward_bounded(*a, ALL, 0, L, None, NULL, st)),
            "bounded, true bound": run(lambda a, st: lib.nesvor_hashgrid_backward_bounded(*a, ALL, 0, L, None, _lib.ptr(bound), st)),
            "plan without a hand-over": run(lambda a, st: lib.nesvor_hashgrid_backward_plan(*a, ALL, 0, L, None, NULL, NULL, NULL, st)),
            "levels [s, L) then [0, s)": run(lambda a, st: lib.nesvor_hashgrid_backward_levels(*a, ALL, split, L, None, st),
                                             lambda a, st: lib.nesvor_hashgrid_backward_levels(*a, ALL | LATER, 0, split, None, st)),
        }
    assert float(ref[0].abs().max()) > 0.1 and bool(torch.isfinite(ref[1]).all())
    for what, (gt, gu) in runs.items():
        print(f"{what}: grad_table max |diff| {float((gt - ref[0]).abs().max()):.3e} of {float(ref[0].abs().max()):.3e}, "
              f"grad_u {float((gu - ref[1]).abs().max()):.3e} of {float(ref[1].abs().max()):.3e}")
        torch.testing.assert_close(gt, ref[0], msg=lambda m: f"{what}: grad_table: {m}", **GT_TOL)
        torch.testing.assert_close(gu, ref[1], msg=lambda m: f"{what}: grad_u: {m}", **GU_TOL)
