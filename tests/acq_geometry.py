"""Geometries, PSFs, poses and fp32 tolerances shared by the tests that pin the acquisition arithmetic at geometric edges:
tests/test_gpu_slice_acq_geometry.py (csrc/slice_acq.hip), tests/test_gpu_svr_similarity.py (csrc/svr.hip) and the CPU reference
tests/svr_reference.py.  Nothing here touches a GPU.

Two sets of poses.  LATTICE: matrix entries 0 or +-1 and dyadic translations, so every coordinate is exact in fp32: a kernel and
the oracle take identical ``floor`` and bounds decisions, and their sets of valid pixels must be EQUAL.  GENERIC: seeded random
poses as in tests/test_gpu_ops.py::_sa_setup; the callers fix the seeds and assert what they need of them."""
import torch

# name: volume (D,H,W), slice (h,w), res_slice, PSF
GEOMETRIES = {
    "odd": ((5, 7, 9), (7, 9), 1.0, "psf333"),  # all sizes odd: with lattice poses every tap position is an integer
    "tiny": ((2, 2, 2), (3, 5), 1.0, "psf333"),  # the smallest volume with an interior (x < W - 1)
    "row": ((5, 7, 300), (1, 257), 1.0, "psf955"),  # one row, one pixel past a workgroup
    "dense": ((9, 11, 13), (16, 16), 0.5, "psf955"),  # exactly 256 pixels; several pixels per voxel
    "sparse": ((18, 20, 22), (17, 19), 2.5, "psf955"),  # 323 pixels: second trip of the per-slice loops; sparse pixels
    "even": ((9, 11, 13), (6, 6), 1.0, "psf426"),  # even PSF dimensions: tap ranges -d/2 .. (d+1)/2 - 1 are asymmetric
}
BIG_PSFS = ["psf1688", "psf1788"]  # forward only, on the "even" volume: 1024 taps fill the LDS list exactly, 1088 walk global memory
OUTSIDE = 4  # index of the lattice pose 100 voxels outside the volume

# (rtol, atol as a fraction of 1, atol as a fraction of the reference's largest magnitude), from tests/test_gpu_ops.py:
# test_slice_acq_vs_oracle / _adjoint_vs_oracle / _backward_vs_oracle / _adjoint_backward_vs_oracle (fp32)
TOL32 = {"slices": (1e-4, 1e-5, 0), "weight": (1e-4, 1e-5, 0), "adjoint": (1e-4, 1e-5, 0), "adjoint_weight": (1e-4, 1e-5, 0),
         "grad_vol": (1e-4, 1e-5, 0), "grad_transforms": (0, 0, 2e-4), "grad_slices": (2e-4, 0, 2e-5), "adjoint_grad_transforms": (0, 0, 3e-4)}


def _psf(name):
    """(9,5,5): the PSF of 1.5 x 1.5 x 3 mm slices on a 1 mm grid; (3,3,3): get_PSF((1,1,1)); the others hand-made, every tap
    non-zero, normalised."""
    from nesvor_amd.utils import get_PSF

    if name == "psf955":
        psf = get_PSF(res_ratio=(1.5, 1.5, 3.0))
    elif name == "psf333":
        psf = get_PSF(res_ratio=(1.0, 1.0, 1.0))
    else:
        shape = {"psf426": (4, 2, 6), "psf1688": (16, 8, 8), "psf1788": (17, 8, 8)}[name]
        g = torch.Generator().manual_seed(sum(shape))
        psf = 0.2 + torch.rand(shape, generator=g)
        psf = psf / psf.sum()
    assert tuple(psf.shape) == {"psf955": (9, 5, 5), "psf333": (3, 3, 3), "psf426": (4, 2, 6), "psf1688": (16, 8, 8),
                                "psf1788": (17, 8, 8)}[name]
    return psf.contiguous()


def _lattice_poses(dims):
    """Six poses [R | t] (x = R (p + t) + centre, t in voxels): identity, 90 degrees about z, a cyclic axis permutation, identity
    moved by (0.5, -1, 2), identity 100 voxels outside (OUTSIDE), identity moved by (W - 1) / 2 along x (half in, half out)."""
    eye = [[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]
    rz = [[0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]]
    perm = [[0, 1.0, 0], [0, 0, 1.0], [1.0, 0, 0]]
    W = dims[2]
    poses = [(eye, (0, 0, 0)), (rz, (0, 0, 0)), (perm, (0, 0, 0)), (eye, (0.5, -1.0, 2.0)), (eye, (0, 0, 100.0)), (eye, ((W - 1) / 2.0, 0, 0))]
    return torch.stack([torch.cat([torch.tensor(r), torch.tensor(t, dtype=torch.float32)[:, None]], 1) for r, t in poses])


def _generic_poses(n, g):
    from oracle import transform_convert as tc

    ax = torch.randn(n, 6, generator=g) * torch.tensor([0.6, 0.6, 0.6, 3.0, 3.0, 3.0])
    ax[0] = 0
    return tc.axisangle2mat_forward(ax)
