"""Package registration end to end (``register_slices(..., packages=...)``, ``--packages``) on the 48^3 phantom: three stacks of
1.5 mm pixels and 3 mm slices acquired in P = 2 interleaved packages, every package at its own rigid perturbation (rotation
vector ~ N(0, 4 deg), translation ~ N(0, 2 mm), fixed seed), no per-slice motion, handed over at the nominal poses.

The runs are made once per session and shared by the tests.  Every figure is printed before it is asserted; DESIGN.md,
"Package registration", has the values measured on MI355X."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_RES_S, _THICK, _P = 1.5, 3.0, 2
_RUNS = {}


def _package_stacks(device):
    """(stacks at nominal poses, per stack the two package perturbations as world transforms)."""
    import numpy as np

    from nesvor_amd.image import Stack
    from nesvor_amd.phantom import STACK_ANGLES, phantom3d, stack_geometry, stack_transforms
    from nesvor_amd.slice_acquisition import slice_acquisition
    from nesvor_amd.transform import RigidTransform
    from nesvor_amd.utils import get_PSF

    vol = torch.tensor(phantom3d(n=48), dtype=torch.float32, device=device)
    n_slice, ss = stack_geometry(48, 1.0, _RES_S, _THICK)
    psf = get_PSF(res_ratio=(_RES_S, _RES_S, _THICK), device=device)
    g = torch.Generator().manual_seed(0)
    images, nominals, moves = [], [], []
    for si in range(3):
        nominal = stack_transforms(STACK_ANGLES[si], n_slice, _THICK, device)
        d = torch.cat([torch.randn(_P, 3, generator=g) * (4 * np.pi / 180), torch.randn(_P, 3, generator=g) * 2.0], -1).to(device)
        actual = RigidTransform(d[torch.arange(n_slice) % _P], trans_first=True).compose(nominal)
        images.append(slice_acquisition(actual.matrix(), vol[None, None].contiguous(), None, None, psf, (ss, ss), _RES_S, False, False))
        nominals.append(nominal)
        moves.append(RigidTransform(d, trans_first=True))
    allv = torch.cat([im[im > 0] for im in images])
    q = torch.kthvalue(allv, max(int(0.99 * allv.numel()), 1)).values
    stacks = [Stack((im / q).contiguous(), im > 0, nom, resolution_x=_RES_S, resolution_y=_RES_S, thickness=_THICK, gap=_THICK)
              for im, nom in zip(images, nominals)]
    return stacks, nominals, moves


def _simulated_ncc(stacks):
    """Mean over the non-empty slices of the global NCC between the acquired slices and the slices simulated from the volume
    reconstructed at the stacks' poses (the definition of tests/test_svr.py::_simulated_ncc); lower = better."""
    from nesvor_amd.registration import _cover_shape, reconstruct_from_slices
    from nesvor_amd.slice_acquisition import slice_acquisition
    from nesvor_amd.transform import RigidTransform, mat_update_resolution
    from nesvor_amd.utils import get_PSF, ncc_loss

    img = torch.cat([s.slices * s.mask for s in stacks]).contiguous()
    poses = RigidTransform.cat([s.transformation for s in stacks])
    m = img > 0
    keep = m.flatten(1).any(1)
    img, m, poses = img[keep].contiguous(), m[keep].contiguous(), poses[keep]
    mats = mat_update_resolution(poses.matrix(), 1, _RES_S)
    volume = reconstruct_from_slices(mats, img, _RES_S, _THICK, _RES_S, _cover_shape(poses, m, _RES_S, _THICK, _RES_S))
    sim = slice_acquisition(mats, volume, None, m, get_PSF(res_ratio=(1, 1, _THICK / _RES_S), device=img.device), img.shape[-2:], 1.0,
                            False, False)
    return float(ncc_loss(sim, img, m, win=None, reduction="none").mean())


def _relative_pose_errors(stacks, nominals, moves):
    """Per stack (rotation error in degrees, translation error of the stack centre in mm) of the relative pose between package 0
    and package 1.  A package's slices sit at  M_p o nominal  for one world transform M_p; the relative pose  inv(M_1) o M_0  does
    not change when the whole scene is moved (a registration's gauge), and is  inv(d_1) o d_0  in truth."""
    out = []
    for s, nominal, d in zip(stacks, nominals, moves):
        k = len(nominal) // 2
        k0, k1 = (k, k + 1) if k % _P == 0 else (k + 1, k)
        M = [s.transformation[kp].compose(nominal[kp].inv()) for kp in (k0, k1)]
        rel = M[1].inv().compose(M[0])
        err = rel.compose(d[1].inv().compose(d[0]).inv()).matrix()[0].double()
        R, t = err[:, :3], err[:, 3]
        angle = float(torch.rad2deg(torch.acos(((R.trace() - 1) / 2).clamp(-1, 1))))
        out.append((angle, float((R @ t).norm())))  # the centre (the world origin) goes to R (0 + t)
    return out


def _run(device, what):
    """The shared runs: 'nominal', 'stack' (register_stacks), 'packages' / 'packages2' (two identical runs of the package stage
    alone, n_outer = 0), 'composed' (the same under NESVOR_PACKAGES=composed)."""
    if what in _RUNS:
        return _RUNS[what]
    from nesvor_amd import registration as R

    stacks, nominals, moves = _package_stacks(device)
    history = []
    if what == "stack":
        stacks = R.register_stacks(stacks, res_s=_RES_S)
    elif what != "nominal":
        call = R.GroupSVR.__call__

        def recording(self, *args, **kwargs):
            out = call(self, *args, **kwargs)
            history.extend(self.history)
            return out

        old = os.environ.get("NESVOR_PACKAGES")
        R.GroupSVR.__call__ = recording
        try:
            if what == "composed":
                os.environ["NESVOR_PACKAGES"] = "composed"
            stacks = R.register_slices(stacks, res_s=_RES_S, n_outer=0, packages=[_P] * 3)
        finally:
            R.GroupSVR.__call__ = call
            if what == "composed":
                os.environ.pop("NESVOR_PACKAGES")
                if old is not None:
                    os.environ["NESVOR_PACKAGES"] = old
    _RUNS[what] = (stacks, _relative_pose_errors(stacks, nominals, moves), history)
    return _RUNS[what]


def test_the_package_stage_improves_on_stack_registration(device):
    ncc_stack = _simulated_ncc(_run(device, "stack")[0])
    ncc_packages = _simulated_ncc(_run(device, "packages")[0])
    print(f"mean simulated NCC: stack registration {ncc_stack:.4f}, package stage {ncc_packages:.4f}")
    assert ncc_packages < ncc_stack


def test_the_relative_pose_of_the_packages_is_recovered(device):
    start = _run(device, "nominal")[1]
    end = _run(device, "packages")[1]
    for j, ((r0, t0), (r1, t1)) in enumerate(zip(start, end)):
        print(f"stack {j}: relative pose of its packages off by {r0:.3f} deg / {t0:.3f} mm at the start, {r1:.3f} deg / {t1:.3f} mm after")
    for (r0, t0), (r1, t1) in zip(start, end):
        assert r1 < r0 and t1 < t0


def test_no_group_ends_a_level_above_its_start_and_two_runs_agree(device):
    stacks, _, history = _run(device, "packages")
    assert len(history) == 2 * 3  # two rounds of three levels
    for level, start, end in history:
        assert start.shape == (3 * _P,) and bool((end <= start).all()), (level, start, end)
    assert any(bool((end < start).any()) for _, start, end in history)
    again = _run(device, "packages2")[0]
    for a, b in zip(stacks, again):
        assert torch.equal(a.transformation.matrix(), b.transformation.matrix())


def test_fused_within_a_quarter_of_composed(device):
    """25 %, as tests/test_svr.py holds the slice descent: accept / reject decisions that flip on near-ties.  (The two paths
    have ONE definition and are bit-equal per call - tests/test_gpu_svr_groups.py - so the runs are expected to agree.)"""
    fused, composed = _run(device, "packages")[1], _run(device, "composed")[1]
    rot_f, tr_f = (sum(e[i] for e in fused) / 3 for i in (0, 1))
    rot_c, tr_c = (sum(e[i] for e in composed) / 3 for i in (0, 1))
    print(f"mean relative-pose error: fused {rot_f:.3f} deg / {tr_f:.3f} mm, composed {rot_c:.3f} deg / {tr_c:.3f} mm")
    assert rot_f <= 1.25 * rot_c and tr_f <= 1.25 * tr_c


def test_full_pipeline_with_and_without_packages_is_recorded(device):
    """Printed and recorded, not asserted: on this clean phantom the three slice rounds recover part of the package
    motion on their own.  Measured once on MI355X: mean simulated NCC -0.9002 with packages, -0.8984 without."""
    import math

    from nesvor_amd import registration as R

    for packages in (None, [_P] * 3):
        stacks, nominals, moves = _package_stacks(device)
        out = R.register_slices(stacks, res_s=_RES_S, packages=packages)
        ncc = _simulated_ncc(out)
        errors = ", ".join(f"{r:.2f} deg / {t:.2f} mm" for r, t in _relative_pose_errors(out, nominals, moves))
        print(f"full pipeline, packages {packages}: mean simulated NCC {ncc:.4f}; relative pose of the packages off by {errors}")
        assert math.isfinite(ncc)


def test_without_packages_nothing_of_the_stage_is_touched(device, monkeypatch):
    from nesvor_amd import registration as R

    def boom(*args, **kwargs):
        raise AssertionError("the package stage ran without --packages")

    for name in ("svr_similarity_groups", "svr_similarity_groups_bank"):
        getattr(torch.ops.nesvor, name)
        monkeypatch.setattr(torch.ops.nesvor, name, boom)
    monkeypatch.setattr(R.GroupSVR, "__call__", boom)
    monkeypatch.setattr(R.GroupSVR, "_group_sums", boom)
    monkeypatch.setattr(R, "package_groups", boom)
    stacks, nominals, _ = _package_stacks(device)
    out = R.register_slices(stacks, res_s=_RES_S, n_outer=1)
    assert any(not torch.equal(s.transformation.matrix(), n.matrix()) for s, n in zip(out, nominals))
    with pytest.raises(AssertionError, match="package stage"):
        R.register_slices(_package_stacks(device)[0], res_s=_RES_S, n_outer=0, packages=[2])


def test_too_many_packages_are_refused_before_any_work(device):
    from nesvor_amd import registration as R

    stacks = _package_stacks(device)[0]
    with pytest.raises(ValueError, match="fewer than its"):
        R.register_slices(stacks, res_s=_RES_S, packages=[2, 2, stacks[2].slices.shape[0] + 1])


def test_cli_register_with_packages(tmp_path, device):
    from nesvor_amd import cli
    from nesvor_amd.image import Volume
    from nesvor_amd.transform import RigidTransform

    paths, n_nonempty = [], 0
    for j, st in enumerate(_package_stacks(device)[0]):
        img = st.slices[:, 0]
        n_nonempty += int((img > 0).flatten(1).any(1).sum())
        ax = st.transformation.axisangle().mean(0, keepdim=True)  # stack centre pose
        p = str(tmp_path / f"stack{j}.nii.gz")
        Volume(img, img > 0, RigidTransform(ax), _RES_S, _RES_S, _THICK).save(p, masked=False)
        paths.append(p)
    out = str(tmp_path / "slices")
    cli.main(["register", "--input-stacks", *paths, "--thicknesses", "3", "3", "3", "--registration", "svr", "--packages", "2",
              "--package-rounds", "1", "--output-slices", out, "--verbose", "0"])
    assert len([f for f in os.listdir(out) if not f.startswith("mask")]) == n_nonempty > 30
    with pytest.raises(SystemExit, match="--packages"):
        cli.main(["register", "--input-stacks", *paths, "--registration", "svr", "--packages", "2", "2", "--output-slices",
                  str(tmp_path / "never"), "--verbose", "0"])
