"""Stack-to-stack rigid registration (the reference's ``nesvor/svort/registration.py:189-284``
``VVR`` + ``resample`` and the registration-only branch of ``svort/inference.py``: ``parse_data`` :176-248,
``stack_registration`` :308-367, ``run_svort`` :447-552 with ``svort=False, vvr=True`` = ``--registration stack``).

Volume-to-volume registration by normalised gradient descent on a similarity loss over a coarse-to-fine pyramid:

* level l (num_levels-1 .. 0): both volumes are blurred (sigma = 0.5 * 2^l voxels of the finest axis) and resampled
  to isotropic voxels of size ``min(res) * 2^l``; the target's non-zero voxels become a point list in physical
  coordinates, the source is sampled at the rigidly moved points (trilinear);
* a level runs ``num_steps`` rounds, round r with step length ``step_size * 2^l / 2^r``; a round repeats up to
  ``max_iter`` times: gradient (autograd, or central differences with the step length as offset), momentum
  buffer, normalise the direction, move by the step length, keep the move only where the loss decreased - the
  first rejected move ends the round for that batch entry;
* the parameter vector is (rotation vector in DEGREES, translation in mm) during the descent, so one step length
  serves both parts.

Written for this code base (explicit pyramid level object, one objective function); behaviour follows the reference,
whose own test (``tests/svort/test_vvr.py``) is re-stated in ``tests/test_registration.py``.

Two evaluation paths.  Generic (any loss callable, autograd gradients, any device the transform ops support):
PyTorch ``grid_sample`` + the loss, as the reference does - one objective evaluation is ~25 small launches and a
finite-difference gradient needs 13 of them.  Fused (HIP, ``nesvor_vvr_similarity``): when the loss is given by name
(global NCC or MSE) and the gradient is by finite differences, ONE launch samples the source under all 13 poses and
returns the moment sums the loss is a function of (fp64); ``stack_registration`` uses it.

``loss = {"name": "nmi", "bins": B}`` (not in the reference; ``--stack-similarity nmi``): normalised mutual information of the
sampled source and the target over ALL points of the level (nesvor_amd/nmi.py has the definition; I is binned on the range of the
level's source, J on the range of the level's point list), for stacks whose intensities are not linearly related.  Three
evaluation paths with that one definition: fused (``torch.ops.nesvor.vvr_joint_histogram``, csrc/vvr_nmi.hip: the 13 poses of a
gradient in one call, the accept test a K = 1 call) under the conditions of the fused path above; composed (the kernel's own
samples, ``torch.ops.nesvor.vvr_sample``, binned by ``nmi.joint_histogram`` - bit-equal to the fused one), forced with
``NESVOR_VVR_NMI=composed``; generic (``grid_sample`` + ``nmi.joint_histogram``) for batches and devices without the kernels.  The
histogram is integer, so the gradient is by finite differences only.

Slice-to-volume registration (``SVR``, ``register_slices`` = ``--registration svr``; no counterpart in the reference, whose
slice-level choices need the pretrained SVoRT transformer): the same descent with one pose per slice, the objective being
the similarity of the acquired slice and the slice simulated from the volume by the acquisition operator.

Package registration (``GroupSVR``, ``register_slices(..., packages=...)`` = ``--packages``): the stage between the two - one
rigid correction per interleaved package of a stack, the objective being the similarity over all slices of the package.
"""
import ctypes
import logging
import math
import os
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F

from . import _lib
from . import nmi as _nmi
from .psf_bank import SAME_THICKNESS, PsfBank, bank_for
from .slice_acquisition import bank_fused, slice_acquisition, slice_acquisition_bank
from .transform import RigidTransform, mat_transform_points, mat_update_resolution
from .utils import gaussian_blur, get_PSF, meshgrid, ncc_loss


def resample(x: torch.Tensor, res_xyz_old: Sequence[float], res_xyz_new: Sequence[float]) -> torch.Tensor:
    """Linear resampling of (N,C,*spatial) from voxel size ``res_xyz_old`` to ``res_xyz_new`` (both listed x first),
    keeping the first and the last sample position fixed relative to the centre (registration.py:267-284)."""
    nd = x.ndim - 2
    assert len(res_xyz_old) == len(res_xyz_new) == nd
    axes = []
    for d in range(nd):  # d = 0 is x = the last tensor dimension
        size = x.shape[-1 - d]
        fac = res_xyz_old[d] / res_xyz_new[d]
        size_new = int(size * fac)
        reach = (size_new - 1) / fac / (size - 1)  # normalised half-extent covered by the new samples
        axes.append(torch.linspace(-reach, reach, size_new, dtype=x.dtype, device=x.device))
    mesh = torch.meshgrid(*axes[::-1], indexing="ij")[::-1]  # each of shape (..., ny, nx); element order x, y, (z)
    grid = torch.stack(mesh, -1)[None].expand(x.shape[0], *([-1] * (nd + 1)))
    return F.grid_sample(x, grid, align_corners=True)


class _Level:
    """One pyramid level: the source volume on the level's grid, the target as a masked point list."""

    def __init__(self, source: torch.Tensor, target: torch.Tensor, voxel: float):
        self.source = source
        keep = (target > 0).reshape(-1)
        shape_xyz = (target.shape[-1], target.shape[-2], target.shape[-3])
        self.points = meshgrid(shape_xyz, (voxel, voxel, voxel), device=target.device).reshape(-1, 3)[keep]
        self.values = target.reshape(-1)[keep]
        # physical (mm, centred) -> grid_sample's normalised coordinates of the source
        unit = [2.0 / (source.shape[-1] - 1) / voxel, 2.0 / (source.shape[-2] - 1) / voxel, 2.0 / (source.shape[-3] - 1) / voxel]
        self.to_unit = torch.tensor(unit, dtype=source.dtype, device=source.device)
        self.to_unit_host = (ctypes.c_float * 3)(*unit)
        self.target_sums = None  # (sum J, sum J^2) of the fused path, filled by its first call
        self.i_map, self.j_map = None, None  # nmi: the affine maps to bin coordinates, filled by the first evaluation


class VVR:
    """``VVR(num_levels, num_steps, step_size, max_iter, optimizer, loss, auto_grad)`` then
    ``theta_out, loss = vvr(theta, source, target, params, transform_t, trans_first)``:

    theta (B,6) axis-angle [rad | mm] of the source in the ``trans_first`` convention, source / target volumes
    (1,1,D,H,W), ``params = {"res_s": in-plane, "s_thick": through-plane}`` voxel sizes, ``transform_t`` the target's
    pose.  ``optimizer = {"name": "gd", "momentum": m}``; ``loss`` = {"name": "mse" | "ncc", ...} or a callable
    ``loss(self, warped, target) -> per-element or per-batch loss``, or ``{"name": "nmi", "bins": B}`` (2 <= B <= 64, default
    32; no other key; ``auto_grad=True`` raises): the module docstring has its paths.
    """

    def __init__(self, num_levels: int, num_steps: int, step_size: float, max_iter: int, optimizer: Dict,
                 loss: Union[Dict, Callable], auto_grad: bool) -> None:
        self.num_levels, self.num_steps, self.step_size, self.max_iter = num_levels, num_steps, step_size, max_iter
        self.auto_grad = auto_grad
        self.current_level = num_levels - 1
        if optimizer.get("name") != "gd":
            raise Exception("unknown optimizer")
        self.momentum = float(optimizer.get("momentum", 0))
        self._fused_kind, self._eps = None, 1e-6
        if isinstance(loss, dict):
            kw = dict(loss)
            name = kw.pop("name")
            if name == "mse":
                self._loss = lambda x, y: F.mse_loss(x, y, reduction="none", **kw)
                self._fused_kind = "mse" if not kw else None
            elif name == "ncc":
                self._loss = lambda x, y: ncc_loss(x, y, reduction="none", level=self.current_level, **kw)
                if kw.get("win", 9) is None and set(kw) <= {"win", "eps"}:  # global NCC: a function of five moment sums
                    self._fused_kind, self._eps = "ncc", float(kw.get("eps", 1e-6))
            elif name == "nmi":  # a statistic of the whole point list, not a loss per element: `_objective` takes its own way
                if set(kw) - {"bins"}:
                    raise Exception("unknown loss")
                if auto_grad:
                    raise ValueError("loss nmi: an integer histogram has no gradient; auto_grad=False (finite differences) expected")
                self._bins = _nmi.check_bins(kw.get("bins", _nmi.DEFAULT_BINS), "loss bins")
                self._loss, self._fused_kind = None, "nmi"
            else:
                raise Exception("unknown loss")
        elif callable(loss):
            self._loss = lambda x, y: loss(self, x, y)
        else:
            raise Exception("unknown loss")
        self.theta_t: Optional[RigidTransform] = None
        self.trans_first = True

    # ---- units: the descent works on (degrees, mm) -----------------------------------------------------------
    @staticmethod
    def _unit(theta: torch.Tensor) -> torch.Tensor:
        d = math.pi / 180
        return torch.tensor([d, d, d, 1, 1, 1], dtype=theta.dtype, device=theta.device).view(1, 6)

    # ---- pyramid -------------------------------------------------------------------------------------------
    def _level(self, level: int, source: torch.Tensor, target: torch.Tensor) -> _Level:
        f = 2.0**level
        sigma = [0.5 * f / r for r in self.relative_res]  # per tensor dimension (z, y, x)
        vols = []
        for v in (source, target):
            v = gaussian_blur(v, sigma, truncated=4.0)
            vols.append(resample(v, self.relative_res[::-1], [f] * 3))
        return _Level(vols[0], vols[1], self.res * f)

    # ---- objective -------------------------------------------------------------------------------------------
    def _warp(self, theta_deg: torch.Tensor, lv: _Level) -> torch.Tensor:
        """Source sampled at the target's points moved by  inv(T(theta)) o T_target  ->  (B, M)."""
        pose = RigidTransform(theta_deg * self._unit(theta_deg), trans_first=self.trans_first)
        mat = pose.inv().compose(self.theta_t).matrix()  # (B,3,4), translation-first convention
        moved = mat_transform_points(mat[:, None], lv.points[None], True)  # (B,M,3)
        grid = (moved * lv.to_unit).view(moved.shape[0], -1, 1, 1, 3)
        src = lv.source.expand(moved.shape[0], -1, -1, -1, -1)
        return F.grid_sample(src, grid, align_corners=True).view(moved.shape[0], -1)

    def _objective(self, theta_deg: torch.Tensor, lv: _Level) -> torch.Tensor:
        warped = self._warp(theta_deg, lv)
        if self._fused_kind == "nmi":
            return _nmi.nmi_loss(self._bin(warped, lv)).to(theta_deg.dtype)
        loss = self._loss(warped[:, None], lv.values.view(1, 1, -1).expand(warped.shape[0], -1, -1))
        return loss.reshape(loss.shape[0], -1).mean(1)

    def _fused(self, theta: torch.Tensor, lv: _Level) -> bool:
        return (self._fused_kind is not None and not self.auto_grad and theta.shape[0] == 1 and lv.source.is_cuda
                and lv.source.dtype == torch.float32 and lv.source.shape[0] == 1)

    def _objective_fused(self, thetas_deg: torch.Tensor, lv: _Level) -> torch.Tensor:
        """Losses of K poses of ONE registration problem in one launch -> (K,)."""
        K = thetas_deg.shape[0]
        pose = RigidTransform(thetas_deg * self._unit(thetas_deg), trans_first=self.trans_first)
        mats = pose.inv().compose(self.theta_t).matrix().contiguous()
        if self._fused_kind == "nmi":
            return _nmi.nmi_loss(self._level_histograms(mats, lv, os.environ.get("NESVOR_VVR_NMI", "") != "composed")).to(thetas_deg.dtype)
        dev = lv.source.device
        sums = torch.empty((K, 3), dtype=torch.float64, device=dev)
        first = lv.target_sums is None
        if first:
            lv.target_sums = torch.empty(2, dtype=torch.float64, device=dev)
        src = lv.source.contiguous()
        D, H, W = src.shape[-3:]
        M = lv.values.numel()
        with torch.cuda.device(dev):
            err = _lib.load().nesvor_vvr_similarity(_lib.ptr(src), D, H, W, _lib.ptr(lv.points), _lib.ptr(lv.values), _lib.ptr(mats),
                                                    lv.to_unit_host, M, K, _lib.ptr(sums),
                                                    _lib.ptr(lv.target_sums) if first else None, _lib.stream_ptr())
        _lib.check(err, "vvr similarity")
        sI, sII, sIJ = sums[:, 0] / M, sums[:, 1] / M, sums[:, 2] / M
        sJ, sJJ = lv.target_sums[0] / M, lv.target_sums[1] / M
        if self._fused_kind == "mse":
            return (sII - 2 * sIJ + sJJ).float()
        cross = sIJ - sI * sJ
        return (-(cross * cross) / ((sII - sI * sI) * (sJJ - sJ * sJ) + self._eps)).float()

    # ---- nmi: the statistic of a pose is a joint histogram (nesvor_amd/nmi.py) over ALL points of the level, (K,B,B) int64 ----
    def _level_maps(self, lv: _Level) -> Tuple[Tuple[float, float], Tuple[float, float]]:
        """The level's affine maps to bin coordinates, (lo, scale) each: of the sampled value from the source's range, of the
        target's value from the range of the point list ((0, 0) for an empty one).  Computed once per level."""
        if lv.i_map is None:
            lv.i_map = tuple(_nmi.axis_map(lv.source.min(), lv.source.max(), self._bins).tolist())
            empty = lv.values.numel() == 0
            lv.j_map = (0.0, 0.0) if empty else tuple(_nmi.axis_map(lv.values.min(), lv.values.max(), self._bins).tolist())
        return lv.i_map, lv.j_map

    def _bin(self, samples: torch.Tensor, lv: _Level) -> torch.Tensor:
        """Samples (K,M) of K poses binned against the level's values with the torch integer ops of the definition."""
        i_map, j_map = self._level_maps(lv)
        K = samples.shape[0]
        J = lv.values.float().view(1, -1).expand(K, -1)
        j_rows = torch.tensor(j_map, dtype=torch.float32, device=samples.device).view(1, 2).expand(K, 2)
        return _nmi.joint_histogram(samples.float(), J, torch.ones_like(J, dtype=torch.bool), i_map, j_rows, self._bins)

    def _level_histograms(self, mats: torch.Tensor, lv: _Level, fused: bool) -> torch.Tensor:
        """Joint histograms at mats (K,3,4) on a HIP device: ``fused`` - one call of the kernel; else composed - the kernel's own
        samples (``vvr_sample``) binned by ``nmi.joint_histogram``, bit-equal to it."""
        from . import ops  # noqa: F401  (registers torch.ops.nesvor)

        i_map, j_map = self._level_maps(lv)
        src, unit = lv.source.contiguous(), list(lv.to_unit_host)
        if fused:
            return torch.ops.nesvor.vvr_joint_histogram(src, lv.points, lv.values, mats, unit, *i_map, *j_map, self._bins)
        return self._bin(torch.ops.nesvor.vvr_sample(src, lv.points, mats, unit), lv)

    def _gradient(self, theta: torch.Tensor, lv: _Level, h: float) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._fused(theta, lv):  # the pose and its 12 perturbations in one launch
            e = torch.zeros((13, 6), dtype=theta.dtype, device=theta.device)
            idx = torch.arange(6, device=theta.device)
            e[1 + 2 * idx, idx] = h
            e[2 + 2 * idx, idx] = -h
            l = self._objective_fused(theta + e, lv)
            return l[:1], (l[1::2] - l[2::2]).view(1, 6)
        if self.auto_grad:
            with torch.enable_grad():
                t = theta.detach().requires_grad_(True)
                loss = self._objective(t, lv)
                (grad,) = torch.autograd.grad([loss.sum()], [t])
            return loss.detach(), grad
        loss = self._objective(theta, lv)
        grad = torch.zeros_like(theta)
        for j in range(theta.shape[1]):  # central differences with the step length as offset, not divided by it
            e = torch.zeros_like(theta)
            e[:, j] = h
            grad[:, j] = self._objective(theta + e, lv) - self._objective(theta - e, lv)
        return loss, grad

    # ---- descent -----------------------------------------------------------------------------------------------
    # `_round` names the batch entries it evaluates (`idx`, rows of its `theta`); here every entry is a whole problem on the
    # level's one (source, target) pair and the index is not needed - SVR picks each entry's slice by it
    def _gradient_at(self, idx: torch.Tensor, cur: torch.Tensor, lv, step: float) -> Tuple[torch.Tensor, torch.Tensor]:
        return self._gradient(cur, lv, step)

    def _trial_at(self, idx: torch.Tensor, theta: torch.Tensor, lv) -> torch.Tensor:
        return self._objective_fused(theta, lv) if self._fused(theta, lv) else self._objective(theta, lv)

    def _round(self, theta: torch.Tensor, lv: _Level, step: float, state: Dict) -> Tuple[torch.Tensor, torch.Tensor]:
        """Up to max_iter accepted moves of length `step`; an entry leaves the active set at its first rejected move."""
        active = torch.ones(theta.shape[0], dtype=torch.bool, device=theta.device)
        loss_all = torch.zeros(theta.shape[0], dtype=theta.dtype, device=theta.device)
        for _ in range(self.max_iter):
            idx = torch.nonzero(active).flatten()
            cur = theta[idx]
            loss, grad = self._gradient_at(idx, cur, lv, step)
            loss_all[idx] = loss
            if self.momentum:
                if "buf" not in state:
                    state["buf"] = grad.clone()  # (first use: all entries are active)
                else:
                    state["buf"][idx] = state["buf"][idx] * self.momentum + grad
                direction = state["buf"][idx]
            else:
                direction = grad
            move = direction / (torch.linalg.norm(direction, dim=-1, keepdim=True) + 1e-6) * (-step)
            better = self._trial_at(idx, cur + move, lv) < loss
            active[idx] = better
            if not bool(better.any()):
                break
            theta[idx[better]] += move[better]
        return theta, loss_all

    @torch.no_grad()
    def __call__(self, theta: torch.Tensor, source: torch.Tensor, target: torch.Tensor, params: Dict,
                 transform_t: RigidTransform, trans_first: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        self.theta_t, self.trans_first = transform_t, trans_first
        res = [params["s_thick"], params["res_s"], params["res_s"]]  # voxel size per tensor dimension (z, y, x)
        self.res = min(res)
        self.relative_res = [r / self.res for r in res]
        unit = self._unit(theta)
        theta0 = theta.clone()
        cur = (theta.detach() / unit).clone()
        loss = torch.zeros(theta.shape[0], dtype=theta.dtype, device=theta.device)
        for level in range(self.num_levels - 1, -1, -1):
            self.current_level = level
            lv = self._level(level, source, target)
            step = self.step_size * 2**level
            state: Dict = {}  # the momentum buffer lives for one level
            for _ in range(self.num_steps):
                cur, loss = self._round(cur, lv, step, state)
                step /= 2
        return theta0 + (cur * unit - theta0), loss


# ---------------------------------------------------------------------------------------------------------------------
# slice-to-volume registration
# ---------------------------------------------------------------------------------------------------------------------
class _SliceLevel:
    """One pyramid level of ``SVR``: the volume on the level's grid, the slices and their masks at the level's pixel size,
    the PSF of a slice in the level's voxels (a ``PsfBank`` for slices of unequal thickness)."""

    def __init__(self, volume: torch.Tensor, slices: torch.Tensor, mask: torch.Tensor, psf, res_slice: float,
                 voxel: float):
        self.volume, self.slices, self.mask, self.psf = volume, slices, mask, psf  # (D,H,W), (n,h,w), (n,h,w) bool, (d,h,w)
        self.res_slice, self.voxel = res_slice, voxel  # pixel size in voxels; voxel size in mm
        self.index: Optional[torch.Tensor] = None  # batch entry of the descent -> slice (the slices that take part in this level)
        self.i_map, self.j_map = None, None  # nmi: the affine maps to bin coordinates, filled by the first evaluation


def _psf_op(name: str, psf, ids: Optional[torch.Tensor] = None):
    """The fused op of a statistic and what it takes in the place of the PSF: ``torch.ops.nesvor.<name>`` and ``(psf,)`` for a plain
    PSF, the ``_bank`` twin and the bank's ``op_args(ids)`` (``ids``: the slices of the call, None for all) for a ``PsfBank``."""
    if isinstance(psf, PsfBank):
        return getattr(torch.ops.nesvor, name + "_bank"), psf.op_args(ids)
    return getattr(torch.ops.nesvor, name), (psf,)


def _composed_pixels(mats: torch.Tensor, lv: _SliceLevel, ids: Optional[torch.Tensor]):
    """The composed path's pixels: for every pose k of mats (m,K,3,4), (simulated (m,h,w), valid (m,h,w) bool) of slices ``ids``
    (None: all) from the acquisition operator - valid: mask set and PSF weight > 0, the fused kernels' valid set."""
    mask = lv.mask if ids is None else lv.mask[ids]
    bank = isinstance(lv.psf, PsfBank)
    psf = lv.psf.subset(ids) if bank and ids is not None else lv.psf
    acquire = slice_acquisition_bank if bank else slice_acquisition
    for k in range(mats.shape[1]):
        sim, weight = acquire(mats[:, k], lv.volume[None, None], None, mask[:, None], psf, mask.shape[-2:], lv.res_slice, True, False)
        yield sim[:, 0], mask & (weight[:, 0] > 0)


def _stencil_gradient(cur: torch.Tensor, step: float, losses: Callable) -> Tuple[torch.Tensor, torch.Tensor]:
    """One finite-difference gradient at cur (m,6): ``losses`` maps the 13-pose stencil (m,13,6) - row 0 the pose, rows 1 + 2 j and
    2 + 2 j the pose with +step and -step on axis j - to (m,13) -> (the loss at the pose (m,), the central differences (m,6), not
    divided by the step)."""
    e = torch.zeros((13, 6), dtype=cur.dtype, device=cur.device)
    j = torch.arange(6, device=cur.device)
    e[1 + 2 * j, j] = step
    e[2 + 2 * j, j] = -step
    l = losses(cur[:, None] + e[None])
    return l[:, 0], l[:, 1::2] - l[:, 2::2]


class SVR(VVR):
    """``SVR(num_levels, num_steps, step_size, max_iter, optimizer, loss, min_valid=32)`` then
    ``theta_out, loss = svr(theta, slices, slices_mask, volume, params, trans_first)``: every slice registered rigidly to
    the volume by simulating it through the acquisition operator A (``slice_acquisition`` forward: PSF-weighted sampling at
    the slice's pose) and descending on the similarity of simulated and acquired slice - ``VVR``'s descent, one pose per slice.

    theta (n,6) axis-angle [rad | mm], slices / slices_mask (n,1,h,w), volume (1,1,D,H,W) at ``params["res_r"]``,
    ``params = {"res_s": pixel size, "s_thick": slice thickness, "res_r": voxel size}``.  ``loss = {"name": "ncc" | "mse"}``:
    global masked NCC  -(cov^2) / (var_I var_J + eps)  or the mean squared difference per slice, both functions of the six
    moment sums {count, sum I, sum I^2, sum I J, sum J, sum J^2} over the valid pixels (mask set, PSF weight > 0), in double.

    Level l: volume blurred (sigma 0.5 * 2^l voxels) and resampled to ``res_r * 2^l``; slices blurred in-plane and resampled
    to ``res_s * 2^l``, the mask resampled and thresholded at 0.5; the PSF is that of a slice on the level's grid.  A slice
    with fewer than ``min_valid`` valid pixels at its pose when a level starts keeps its pose for that level (loss 0).

    ``loss = {"name": "nmi", "bins": B}`` (2 <= B <= 64, default 32): normalised mutual information  1 - (H_I + H_J) / H_IJ  of a
    joint histogram of (simulated, acquired) intensity per (slice, pose), for slices whose intensities are not linearly related to
    the volume's (other contrast, other coil bias, saturation).  nesvor_amd/nmi.py states the definition; the simulated value is
    binned on the range of the level's volume, the acquired value on the range of the slice's masked pixels at the level.

    Two evaluation paths with one definition of the loss.  Fused (``torch.ops.nesvor.svr_similarity``, csrc/svr.hip; nmi:
    ``svr_joint_histogram``, csrc/svr_nmi.hip): the 13 poses of a finite-difference gradient of all active slices in one call, the
    accept test a K = 1 call.  Composed: one ``slice_acquisition`` per pose and fp64 torch sums (nmi: the torch integer ops of
    ``nmi.joint_histogram``, bit-equal to the kernel) - used for PSFs the kernel refuses (more than 1024 elements) and forced with
    ``NESVOR_SVR=composed``."""

    def __init__(self, num_levels: int, num_steps: int, step_size: float, max_iter: int, optimizer: Dict, loss: Dict,
                 min_valid: int = 32) -> None:
        self.num_levels, self.num_steps, self.step_size, self.max_iter = num_levels, num_steps, step_size, max_iter
        self.auto_grad = False
        self.current_level = num_levels - 1
        if optimizer.get("name") != "gd":
            raise Exception("unknown optimizer")
        self.momentum = float(optimizer.get("momentum", 0))
        if not isinstance(loss, dict) or loss.get("name") not in ("ncc", "mse", "nmi"):
            raise Exception("unknown loss")
        if not set(loss) <= ({"name", "bins"} if loss["name"] == "nmi" else {"name", "eps"}):
            raise Exception("unknown loss")
        self._kind, self._eps = loss["name"], float(loss.get("eps", 1e-6))
        self._bins = _nmi.check_bins(loss.get("bins", _nmi.DEFAULT_BINS), "loss bins") if self._kind == "nmi" else None
        self.min_valid = min_valid
        self.trans_first = True

    # ---- pyramid -------------------------------------------------------------------------------------------
    @staticmethod
    def _level(level: int, slices: torch.Tensor, slices_mask: torch.Tensor, volume: torch.Tensor, params: Dict) -> _SliceLevel:
        f = 2.0**level
        res_s, res_r, s_thick = params["res_s"], params["res_r"], params["s_thick"]
        sigma = 0.5 * f
        vol = resample(gaussian_blur(volume, sigma, truncated=4.0), [1.0] * 3, [f] * 3)
        sl = resample(gaussian_blur(slices, sigma, truncated=4.0), [1.0] * 2, [f] * 2)
        mask = resample(slices_mask.to(slices.dtype), [1.0] * 2, [f] * 2) > 0.5
        if isinstance(s_thick, (int, float)):
            psf = get_PSF(res_ratio=(res_s / res_r, res_s / res_r, s_thick / (res_r * f)), device=volume.device)
        else:  # one thickness per slice: a PSF bank on the level's grid (a plain PSF if they all agree)
            psf = bank_for(s_thick, res_s, res_r, volume.device, scale=f)
        return _SliceLevel(vol[0, 0].contiguous(), sl[:, 0].contiguous(), mask[:, 0].contiguous(), psf, res_s / res_r, res_r * f)

    # ---- objective -------------------------------------------------------------------------------------------
    @staticmethod
    def _fused_path(lv: _SliceLevel) -> bool:
        from .ops import SVR_MAX_PSF_ELEMENTS

        if isinstance(lv.psf, PsfBank):
            return os.environ.get("NESVOR_SVR", "") != "composed" and bank_fused() and lv.psf.max_elements() <= SVR_MAX_PSF_ELEMENTS
        return os.environ.get("NESVOR_SVR", "") != "composed" and lv.psf.numel() <= SVR_MAX_PSF_ELEMENTS

    def _sums(self, thetas_deg: torch.Tensor, lv: _SliceLevel, ids: Optional[torch.Tensor]) -> torch.Tensor:
        """Moment sums of slices ``ids`` (None: all) under K poses each: thetas_deg (m,K,6) -> (m,K,6) float64."""
        m, K = thetas_deg.shape[:2]
        pose = RigidTransform(thetas_deg.reshape(-1, 6) * self._unit(thetas_deg), trans_first=self.trans_first)
        return self._sums_at(mat_update_resolution(pose.matrix(), 1, lv.voxel).view(m, K, 3, 4).contiguous(), lv, ids)

    def _sums_at(self, mats: torch.Tensor, lv: _SliceLevel, ids: Optional[torch.Tensor]) -> torch.Tensor:
        """The same sums at given matrices: mats (m,K,3,4) fp32 in the level's voxels, row j the poses of slice ``ids[j]``."""
        if self._kind == "nmi":
            return self._histograms_at(mats, lv, ids, self._fused_path(lv))
        slices = lv.slices if ids is None else lv.slices[ids]
        if self._fused_path(lv):
            op, psf = _psf_op("svr_similarity", lv.psf, ids)
            return op(lv.volume, *psf, mats, slices, lv.mask if ids is None else lv.mask[ids], lv.res_slice)
        out = torch.empty((*mats.shape[:2], 6), dtype=torch.float64, device=mats.device)
        J = slices.double()
        for k, (sim, valid) in enumerate(_composed_pixels(mats, lv, ids)):
            valid = valid.double()
            Ik, Jk = sim.double() * valid, J * valid
            out[:, k] = torch.stack([t.sum((1, 2)) for t in (valid, Ik, Ik * Ik, Ik * Jk, Jk, Jk * Jk)], -1)
        return out

    # ---- nmi: the statistic is a joint histogram (nesvor_amd/nmi.py), (m,K,B,B) int64 in the place of the six sums ----
    def _axis_maps(self, lv: _SliceLevel) -> Tuple[Tuple[float, float], torch.Tensor]:
        """The level's affine maps to bin coordinates: (lo, scale) of the simulated value from the volume's range, and
        ``j_map`` (n,2) fp32 of the acquired value from every slice's masked range (``GroupSVR._prepare`` pools it per group)."""
        if lv.i_map is None:
            lv.i_map = tuple(_nmi.axis_map(lv.volume.min(), lv.volume.max(), self._bins).tolist())
        if lv.j_map is None:
            lv.j_map = _nmi.axis_map(*_nmi.masked_range(lv.slices, lv.mask), self._bins).contiguous()
        return lv.i_map, lv.j_map

    def _histograms_at(self, mats: torch.Tensor, lv: _SliceLevel, ids: Optional[torch.Tensor], fused: bool) -> torch.Tensor:
        """Joint histograms of slices ``ids`` (None: all) at mats (m,K,3,4) -> (m,K,B,B) int64; ``fused``: the kernel, else the same
        definition with torch integer ops on the acquisition operator's output."""
        i_map, j_map = self._axis_maps(lv)
        slices = lv.slices if ids is None else lv.slices[ids]
        j_map = j_map if ids is None else j_map[ids].contiguous()
        if fused:
            op, psf = _psf_op("svr_joint_histogram", lv.psf, ids)
            return op(lv.volume, *psf, mats, slices, lv.mask if ids is None else lv.mask[ids], lv.res_slice, *i_map, j_map, self._bins)
        out = torch.empty((*mats.shape[:2], self._bins, self._bins), dtype=torch.int64, device=mats.device)
        for k, (sim, valid) in enumerate(_composed_pixels(mats, lv, ids)):
            out[:, k] = _nmi.joint_histogram(sim.flatten(1), slices.flatten(1), valid.flatten(1), i_map, j_map, self._bins)
        return out

    def _count_of(self, sums: torch.Tensor) -> torch.Tensor:
        """The valid pixels behind the statistics of ``_sums`` (``min_valid`` is held against it)."""
        return _nmi.valid_count(sums) if self._kind == "nmi" else sums[..., 0]

    def _loss_of(self, sums: torch.Tensor) -> torch.Tensor:
        """(..., 6) moment sums (nmi: (..., B, B) histograms) -> loss; an entry without a valid pixel has loss 0."""
        if self._kind == "nmi":
            return _nmi.nmi_loss(sums).float()
        cnt = sums[..., 0]
        ok = cnt > 0
        sI, sII, sIJ, sJ, sJJ = ((sums[..., j] / torch.where(ok, cnt, torch.ones_like(cnt))) for j in range(1, 6))
        if self._kind == "mse":
            loss = sII - 2 * sIJ + sJJ
        else:
            cross = sIJ - sI * sJ
            loss = -(cross * cross) / ((sII - sI * sI) * (sJJ - sJ * sJ) + self._eps)
        return torch.where(ok, loss, torch.zeros_like(loss)).float()

    @staticmethod
    def _ids(idx: torch.Tensor, lv: _SliceLevel) -> Optional[torch.Tensor]:
        """The slices behind batch entries ``idx`` of the level's descent (None: all of them, in order)."""
        ids = lv.index[idx]
        return None if ids.shape[0] == lv.slices.shape[0] else ids  # (an increasing subset of full length is the identity)

    def _trial_at(self, idx: torch.Tensor, theta: torch.Tensor, lv: _SliceLevel) -> torch.Tensor:
        return self._loss_of(self._sums(theta[:, None], lv, self._ids(idx, lv)))[:, 0]

    def _gradient_at(self, idx: torch.Tensor, cur: torch.Tensor, lv: _SliceLevel, step: float) -> Tuple[torch.Tensor, torch.Tensor]:
        return _stencil_gradient(cur, step, lambda thetas: self._loss_of(self._sums(thetas, lv, self._ids(idx, lv))))

    @torch.no_grad()
    def evaluate(self, theta: torch.Tensor, slices: torch.Tensor, slices_mask: torch.Tensor, volume: torch.Tensor,
                 params: Dict, trans_first: bool = True, level: int = 0) -> torch.Tensor:
        """The loss of every slice at pose ``theta`` (n,6) [rad | mm] on pyramid level ``level`` -> (n,)."""
        self.trans_first = trans_first
        lv = self._level(level, slices, slices_mask, volume, params)
        return self._loss_of(self._sums((theta / self._unit(theta))[:, None], lv, None))[:, 0]

    @torch.no_grad()
    def __call__(self, theta: torch.Tensor, slices: torch.Tensor, slices_mask: torch.Tensor, volume: torch.Tensor,
                 params: Dict, trans_first: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        self.trans_first = trans_first
        unit = self._unit(theta)
        theta0 = theta.clone()
        cur = (theta.detach() / unit).clone()
        n = theta.shape[0]
        loss = torch.zeros(n, dtype=theta.dtype, device=theta.device)
        for level in range(self.num_levels - 1, -1, -1):
            self.current_level = level
            lv = self._level(level, slices, slices_mask, volume, params)
            count = self._count_of(self._sums(cur[:, None], lv, None)[:, 0])
            lv.index = torch.nonzero(count >= self.min_valid).flatten()
            loss = torch.zeros(n, dtype=theta.dtype, device=theta.device)
            if lv.index.numel() == 0:
                continue
            sub = cur[lv.index]
            step = self.step_size * 2**level
            state: Dict = {}  # the momentum buffer lives for one level
            for _ in range(self.num_steps):
                sub, sub_loss = self._round(sub, lv, step, state)
                step /= 2
            cur[lv.index] = sub
            loss[lv.index] = sub_loss
        return theta0 + (cur * unit - theta0), loss


# ---------------------------------------------------------------------------------------------------------------------
# package registration: groups of slices that move together (the interleaved sub-stacks of an acquisition)
# ---------------------------------------------------------------------------------------------------------------------
def package_groups(counts: Sequence[int], packages: Sequence[int], keep: Optional[Sequence[int]] = None
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The CSR grouping of interleaved packages -> (group_offsets (G+1), group_slices (E)), int32 host tensors.

    Stack s has ``counts[s]`` slices in file order and ``packages[s]`` packages (one value serves every stack): slice k of stack
    s belongs to package ``k mod P_s``, and packages of different stacks are different groups, numbered stack by stack
    (G = sum of P_s).  ``keep``: the increasing indices, into the concatenation of all stacks, of the slices that remain (the
    empty ones are dropped AFTER the assignment); ``group_slices`` then indexes the kept slices.  A group whose slices were all
    dropped stays, empty."""
    packages = [int(p) for p in packages]
    if len(packages) == 1:
        packages = packages * len(counts)
    if len(packages) != len(counts):
        raise ValueError(f"packages: one count per stack ({len(counts)}) or one for all expected, got {len(packages)}")
    for s, (c, P) in enumerate(zip(counts, packages)):
        if P < 1:
            raise ValueError(f"packages: stack {s} has {P} packages; at least 1 expected")
        if P > c:
            raise ValueError(f"packages: stack {s} has {c} slices, fewer than its {P} packages")
    new_index = {int(k): j for j, k in enumerate(range(sum(counts)) if keep is None else keep)}
    members: List[List[int]] = []
    start = 0
    for c, P in zip(counts, packages):
        for p in range(P):
            members.append([new_index[k] for k in range(start + p, start + c, P) if k in new_index])
        start += c
    offsets = [0]
    for m in members:
        offsets.append(offsets[-1] + len(m))
    return torch.tensor(offsets, dtype=torch.int32), torch.tensor([k for m in members for k in m], dtype=torch.int32)


def compose_mats(correction: torch.Tensor, base: torch.Tensor) -> torch.Tensor:
    """``correction o base`` of (...,3,4) translation-first matrices with the meaning of ``RigidTransform.compose``
    (R' = Rc R, t' = t + R^T uc), written out element by element in the order csrc/svr.hip's grouped kernel uses: in float64,
    every sum of products added left to right, so that rounding the result to fp32 gives that kernel's matrices bit for bit."""
    c, b = correction.double(), base.double()
    rows = []
    for r in range(3):
        row = [c[..., r, 0] * b[..., 0, col] + c[..., r, 1] * b[..., 1, col] + c[..., r, 2] * b[..., 2, col] for col in range(3)]
        rtu = b[..., 0, r] * c[..., 0, 3] + b[..., 1, r] * c[..., 1, 3] + b[..., 2, r] * c[..., 2, 3]
        row.append(b[..., r, 3] + rtu)
        rows.append(torch.stack(row, -1))
    return torch.stack(rows, -2)


def centroid_corrections(x: torch.Tensor, centroid: torch.Tensor, voxel: float = 1.0) -> torch.Tensor:
    """The rigid correction  p -> Rc (p - c) + c + d  as a (...,3,4) translation-first matrix [Rc | Rc^T (c + d) - c], float64.
    x (...,6): rotation vector in DEGREES and d in mm; centroid c (...,3) in voxels of ``voxel`` mm (broadcast against x).
    Rotating about the group's centroid keeps rotation and translation decoupled: the centroid moves by d alone."""
    x, c = x.double(), centroid.double()
    r = x[..., :3] * (math.pi / 180)
    d = x[..., 3:] / voxel
    t2 = (r * r).sum(-1)
    small = t2 < 1e-16
    t = torch.sqrt(torch.where(small, torch.ones_like(t2), t2))
    a = torch.where(small, 1 - t2 / 6, torch.sin(t) / t)  # sin t / t
    bq = torch.where(small, 0.5 - t2 / 24, (1 - torch.cos(t)) / (t * t))  # (1 - cos t) / t^2
    rx, ry, rz = r.unbind(-1)
    zero = torch.zeros_like(rx)
    Kx = torch.stack([torch.stack([zero, -rz, ry], -1), torch.stack([rz, zero, -rx], -1), torch.stack([-ry, rx, zero], -1)], -2)
    R = torch.eye(3, dtype=x.dtype, device=x.device) + a[..., None, None] * Kx + bq[..., None, None] * (Kx @ Kx)
    u = (R.transpose(-2, -1) @ (c + d)[..., None])[..., 0] - c
    return torch.cat([R, u[..., None]], -1)


def _sub_grouping(offsets: torch.Tensor, listed: torch.Tensor, groups: Sequence[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The CSR of the named groups, in that order (host tensors)."""
    off, parts = [0], []
    for g in groups:
        part = listed[int(offsets[g]):int(offsets[g + 1])]
        parts.append(part)
        off.append(off[-1] + int(part.numel()))
    return torch.tensor(off, dtype=torch.int32), (torch.cat(parts) if parts else listed[:0])


class GroupSVR(SVR):
    """``GroupSVR(...)`` (the arguments of ``SVR``) then ``theta_out, loss = gsvr(theta, groups, slices, slices_mask, volume,
    params, trans_first)``: ``SVR`` with one rigid correction per GROUP of slices - the package stage between one pose per
    stack and one pose per slice.  ``groups = (group_offsets, group_slices)``: a CSR grouping in host memory
    (``package_groups``); a slice listed nowhere keeps its pose.

    The unknown is one 6-vector per group (rotation vector in degrees, translation in mm): slice i of group g moves to
    ``correction_g o pose_i``, the correction rotating about the centroid of the group's masked pixel centres at the stage's
    starting poses (``centroid_corrections``).  Pyramid, losses and descent (``_round``: momentum, accept test) are ``SVR``'s; the
    loss of a group is the loss of the sums over all its slices; a group whose valid count at the start of a level is below
    ``min_valid`` sits that level out.  ``theta_out`` (n,6): the corrections folded into the slices' poses in float64.  After a
    call ``corrections`` holds the (G,6) result and ``history`` one ``(level, loss at the level's start, loss at its end)`` per
    level, (G,) each - the accept test keeps the end at or below the start.

    Two evaluation paths with one definition.  Fused (``torch.ops.nesvor.svr_similarity_groups``, csrc/svr.hip): the corrections
    go to the kernel, which composes them with every slice's pose and adds a group's sums in CSR order (nmi: no grouped kernel -
    the per-slice histograms of ``svr_joint_histogram`` at the matrices ``compose_mats`` gives, added per group in integers; every
    slice of a group bins its acquired value on the group's pooled range, ``NESVOR_PACKAGES=composed`` takes the torch definition).  Composed: the same
    composition in float64 here (``compose_mats``), rounded to fp32, then ``SVR``'s per-slice sums (fused or composed themselves:
    ``NESVOR_SVR`` keeps its meaning) added per group in CSR order - taken for PSFs the kernel refuses and forced with
    ``NESVOR_PACKAGES=composed``."""

    def _packages_fused(self, lv: _SliceLevel) -> bool:
        return os.environ.get("NESVOR_PACKAGES", "") != "composed" and self._fused_path(lv)

    def _group_sums(self, x: torch.Tensor, lv: _SliceLevel, gids: Optional[torch.Tensor]) -> torch.Tensor:
        """Moment sums of groups ``gids`` (None: all) under K corrections each: x (m,K,6) [deg | mm] -> (m,K,6) float64."""
        offsets, listed = lv.groups if gids is None else _sub_grouping(*lv.groups, gids.tolist())
        centroid = lv.centroid if gids is None else lv.centroid[gids]
        corr = centroid_corrections(x, centroid[:, None], lv.voxel).float().contiguous()
        m, K = corr.shape[:2]
        nmi = self._kind == "nmi"  # (no grouped kernel: the per-slice histograms at the composed matrices)
        if not nmi and self._packages_fused(lv):
            op, psf = _psf_op("svr_similarity_groups", lv.psf)
            return op(lv.volume, *psf, corr, lv.base, offsets, listed, lv.slices, lv.mask, lv.res_slice)
        out = (torch.zeros((m, K, self._bins, self._bins), dtype=torch.int64, device=corr.device) if nmi else
               torch.zeros((m, K, 6), dtype=torch.float64, device=corr.device))
        if listed.numel() == 0:
            return out
        sizes = (offsets[1:] - offsets[:-1]).long()
        entry_group = torch.repeat_interleave(torch.arange(m), sizes).to(corr.device)
        ids = listed.long().to(corr.device)
        mats = compose_mats(corr[entry_group], lv.base[ids][:, None]).float().contiguous()  # (E,K,3,4)
        if nmi:  # added per group in integers: no order to keep
            return out.index_add_(0, entry_group, self._histograms_at(mats, lv, ids, self._packages_fused(lv)))
        per_entry = self._sums_at(mats, lv, ids)
        for j in range(int(sizes.max())):  # a group's entries one after the other from 0, in CSR order
            has = torch.nonzero(sizes > j).flatten()
            rows = (offsets[:-1].long()[has] + j).to(corr.device)
            has = has.to(corr.device)
            out[has] = out[has] + per_entry[rows]
        return out

    def _gids(self, idx: torch.Tensor, lv: _SliceLevel) -> Optional[torch.Tensor]:
        gids = lv.index[idx]
        return None if gids.shape[0] == lv.centroid.shape[0] else gids

    def _trial_at(self, idx: torch.Tensor, theta: torch.Tensor, lv: _SliceLevel) -> torch.Tensor:
        return self._loss_of(self._group_sums(theta[:, None], lv, self._gids(idx, lv)))[:, 0]

    def _gradient_at(self, idx: torch.Tensor, cur: torch.Tensor, lv: _SliceLevel, step: float) -> Tuple[torch.Tensor, torch.Tensor]:
        return _stencil_gradient(cur, step, lambda x: self._loss_of(self._group_sums(x, lv, self._gids(idx, lv))))

    @staticmethod
    def group_centroids(base_mm: torch.Tensor, slices_mask: torch.Tensor, res_s: float, groups) -> torch.Tensor:
        """(G,3) float64, mm: the mean world position of the masked pixel centres of every group's slices at poses ``base_mm``
        (n,3,4); the origin for a group without a masked pixel.  The per-group adds run on the host, in CSR order."""
        offsets, listed = groups
        m = slices_mask.reshape(slices_mask.shape[0], slices_mask.shape[-2], slices_mask.shape[-1]).double()
        h, w = m.shape[-2:]
        qx = (torch.arange(w, dtype=torch.float64, device=m.device) - (w - 1) / 2) * res_s
        qy = (torch.arange(h, dtype=torch.float64, device=m.device) - (h - 1) / 2) * res_s
        cnt = m.sum((1, 2))
        sq = torch.stack([(m * qx).sum((1, 2)), (m * qy[:, None]).sum((1, 2)), torch.zeros_like(cnt)], -1)  # sum of q per slice
        R, t = base_mm[..., :3].double(), base_mm[..., 3].double()
        world = (R @ (sq + cnt[:, None] * t)[..., None])[..., 0]  # sum over the slice's masked pixels of R (q + t)
        per = torch.cat([world, cnt[:, None]], -1).cpu()
        G = offsets.numel() - 1
        acc = torch.zeros((G, 4), dtype=torch.float64)
        for g in range(G):
            for k in listed[int(offsets[g]):int(offsets[g + 1])].tolist():
                acc[g] += per[k]
        return (acc[:, :3] / acc[:, 3:].clamp(min=1)).to(base_mm.device)

    def _prepare(self, lv: _SliceLevel, base_mm: torch.Tensor, centroid_mm: torch.Tensor, groups) -> None:
        lv.base = mat_update_resolution(base_mm, 1, lv.voxel).contiguous()  # (n,3,4) fp32, the level's voxels
        lv.centroid = centroid_mm / lv.voxel
        lv.groups = groups
        if self._kind == "nmi":  # every slice of a group bins J on the group's pooled range; a slice listed nowhere keeps its own
            lo, hi = _nmi.masked_range(lv.slices, lv.mask)
            offsets, listed = groups
            if listed.numel() > 0:
                G = offsets.numel() - 1
                entry_group = torch.repeat_interleave(torch.arange(G), (offsets[1:] - offsets[:-1]).long()).to(lo.device)
                ids = listed.long().to(lo.device)
                g_lo = torch.full((G,), float("inf"), dtype=lo.dtype, device=lo.device).scatter_reduce_(0, entry_group, lo[ids], "amin")
                g_hi = torch.full((G,), float("-inf"), dtype=hi.dtype, device=hi.device).scatter_reduce_(0, entry_group, hi[ids], "amax")
                lo, hi = lo.index_copy(0, ids, g_lo[entry_group]), hi.index_copy(0, ids, g_hi[entry_group])
            lv.j_map = _nmi.axis_map(lo, hi, self._bins).contiguous()

    @torch.no_grad()
    def evaluate(self, theta: torch.Tensor, groups, slices: torch.Tensor, slices_mask: torch.Tensor, volume: torch.Tensor,
                 params: Dict, trans_first: bool = True, level: int = 0) -> torch.Tensor:
        """The loss of every group at the slice poses ``theta`` (n,6) [rad | mm] on pyramid level ``level`` -> (G,)."""
        base_mm = RigidTransform(theta, trans_first=trans_first).matrix()
        lv = self._level(level, slices, slices_mask, volume, params)
        self._prepare(lv, base_mm, self.group_centroids(base_mm, slices_mask, params["res_s"], groups), groups)
        x = torch.zeros((groups[0].numel() - 1, 1, 6), dtype=theta.dtype, device=theta.device)
        return self._loss_of(self._group_sums(x, lv, None))[:, 0]

    @torch.no_grad()
    def __call__(self, theta: torch.Tensor, groups, slices: torch.Tensor, slices_mask: torch.Tensor, volume: torch.Tensor,
                 params: Dict, trans_first: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        G = groups[0].numel() - 1
        base_mm = RigidTransform(theta, trans_first=trans_first).matrix()
        centroid_mm = self.group_centroids(base_mm, slices_mask, params["res_s"], groups)
        cur = torch.zeros((G, 6), dtype=theta.dtype, device=theta.device)
        loss = torch.zeros(G, dtype=theta.dtype, device=theta.device)
        self.history: List[Tuple[int, torch.Tensor, torch.Tensor]] = []
        for level in range(self.num_levels - 1, -1, -1):
            self.current_level = level
            lv = self._level(level, slices, slices_mask, volume, params)
            self._prepare(lv, base_mm, centroid_mm, groups)
            sums = self._group_sums(cur[:, None], lv, None)[:, 0]
            start = self._loss_of(sums)
            enough = self._count_of(sums) >= self.min_valid
            lv.index = torch.nonzero(enough).flatten()
            loss = torch.zeros(G, dtype=theta.dtype, device=theta.device)
            if lv.index.numel() > 0:
                sub = cur[lv.index]
                step = self.step_size * 2**level
                state: Dict = {}  # the momentum buffer lives for one level
                for _ in range(self.num_steps):
                    sub, _ = self._round(sub, lv, step, state)
                    step /= 2
                cur[lv.index] = sub
                loss[lv.index] = self._loss_of(self._group_sums(cur[:, None], lv, None))[lv.index, 0]
            self.history.append((level, start, torch.where(enough, loss, start)))
        self.corrections = cur
        # fold: every listed slice's pose becomes correction_g o pose, in float64 (mm), then back to the input's form
        offsets, listed = groups
        corr = centroid_corrections(cur, centroid_mm, 1.0)
        mats = base_mm.double().clone()
        sizes = (offsets[1:] - offsets[:-1]).long()
        if listed.numel() > 0:
            entry_group = torch.repeat_interleave(torch.arange(G), sizes).to(theta.device)
            ids = listed.long().to(theta.device)
            mats[ids] = compose_mats(corr[entry_group], mats[ids])
        out = RigidTransform(mats.to(theta.dtype)).axisangle(trans_first=trans_first)
        moved = torch.zeros(theta.shape[0], dtype=torch.bool, device=theta.device)
        if listed.numel() > 0:
            moved[ids] = True
        return torch.where(moved[:, None], out, theta), loss


# ---------------------------------------------------------------------------------------------------------------------
# --registration stack
# ---------------------------------------------------------------------------------------------------------------------
def _mean_pose(t: RigidTransform) -> RigidTransform:
    return RigidTransform(t.axisangle().mean(0, keepdim=True))


def stack_registration(transforms_list: List[List[RigidTransform]], transform_target: RigidTransform,
                       stacks: List[torch.Tensor], res_s: float, s_thick: float,
                       gaps: Optional[Sequence[float]] = None, loss: Optional[Dict] = None) -> List[RigidTransform]:
    """Register every stack (as a volume of its slices) to stack 0 and return per-slice poses
    (svort/inference.py:308-367): stack j starts from each candidate in ``transforms_list`` (mean pose of its
    slices, expressed relative to the target's), the best final NCC wins; the output poses put the slices of stack
    j at  centre o registered_j o (0,0,(i - (n-1)/2) * s_thick).

    ``loss``: the similarity ``VVR`` descends on, ``None`` = global NCC (``{"name": "ncc", "win": None}``, the reference's);
    ``{"name": "nmi", "bins": B}`` = normalised mutual information, for stacks whose intensities are not linearly related.

    ``gaps`` (per-stack slice profiles), one slice spacing per stack: every other stack is resampled along z from its own gap to
    stack 0's before it is registered (``s_thick`` is then that gap), and the output poses of stack j are ``gaps[j]`` apart."""
    device = transform_target.device
    t_target = _mean_pose(transform_target)
    candidates = [[_mean_pose(t) for t in ts] for ts in transforms_list]
    # the loss given by name (global NCC unless told otherwise): on a HIP device VVR then evaluates a gradient's 13 poses in one launch
    vvr = VVR(num_levels=3, num_steps=4, step_size=2, max_iter=20, optimizer={"name": "gd", "momentum": 0.1},
              loss={"name": "ncc", "win": None} if loss is None else loss, auto_grad=False)
    trans_first = False
    registered = [t_target]
    target = stacks[0].squeeze(1)[None, None]
    for j in range(1, len(stacks)):
        source = stacks[j].squeeze(1)[None, None]
        if gaps is not None and abs(gaps[j] - gaps[0]) > SAME_THICKNESS:
            source = resample(source, (1.0, 1.0, gaps[j]), (1.0, 1.0, gaps[0]))
        best, best_ax = float("inf"), None
        for cand in candidates:
            ax = t_target.compose(cand[0].inv()).compose(cand[j]).axisangle(trans_first=trans_first)
            ax, ncc = vvr(ax, source, target, {"res_s": res_s, "s_thick": s_thick}, t_target, trans_first)
            if float(ncc) < best:
                best, best_ax = float(ncc), ax
        registered.append(RigidTransform(best_ax, trans_first=trans_first))
    centre = registered[0].axisangle(trans_first=False).clone()
    centre[..., :3] = 0
    centre[..., 3:] *= -1
    centre = RigidTransform(centre)
    out = []
    for j, stack in enumerate(stacks):
        n = stack.shape[0]
        t = torch.zeros((n, 6), dtype=torch.float32, device=device)
        t[:, -1] = (torch.arange(n, dtype=torch.float32, device=device) - (n - 1) / 2) * (s_thick if gaps is None else gaps[j])
        out.append(centre.compose(registered[j]).compose(RigidTransform(t)))
    return out


def _unequal(values: Sequence[float]) -> bool:
    return max(values) - min(values) > SAME_THICKNESS


def _stack_loss(similarity: str, nmi_bins, what: str = "similarity") -> Optional[Dict]:
    """The ``loss`` of ``stack_registration`` behind a similarity's name (None: its default, global NCC); ValueError otherwise."""
    if similarity not in ("ncc", "nmi"):
        raise ValueError(f"{what}: 'ncc' or 'nmi' expected, got {similarity!r}")
    return None if similarity == "ncc" else {"name": "nmi", "bins": _nmi.check_bins(nmi_bins, "nmi_bins")}


def register_stacks(dataset: List, res_s: float = 1.0, template: int = 0, per_stack_thickness: bool = False,
                    similarity: str = "ncc", nmi_bins: int = _nmi.DEFAULT_BINS) -> List:
    """``--registration stack``: in-plane resampling of the masked stacks to ``res_s`` mm (parse_data), stack
    registration to the first stack, new per-slice poses written into the stacks (run_svort with svort=False, vvr=True).
    As in the reference, the slice spacing of the output poses is the MEAN thickness of the input stacks.

    ``template`` (not in the reference; ``--template-stack``, nesvor_amd/assess.py) names the stack the others are registered
    to and the world frame is centred on: that stack is moved to the front for the registration, the poses land in the stacks
    themselves, and the list comes back in input order.  ``template=0`` is the reference's behaviour.

    ``per_stack_thickness`` (``--per-stack-thickness``) and stacks whose thicknesses or gaps differ by more than 1e-3 mm: every
    stack is registered on the template's slice spacing (resampled along z from its own gap) and its output poses are its own
    gap apart.  Stacks that agree take the path above, bit for bit.

    ``similarity`` (``--stack-similarity``): ``"ncc"`` (global NCC, the reference's, as before) or ``"nmi"`` - normalised mutual
    information on a joint histogram of ``nmi_bins`` bins per axis over the template's points (nesvor_amd/nmi.py; ``VVR``), for
    stacks whose intensities are not linearly related to the template's."""
    loss = _stack_loss(similarity, nmi_bins)  # (refusals before any work)
    if template != 0:
        if not 0 <= template < len(dataset):
            raise ValueError(f"template stack {template} out of range: {len(dataset)} stacks")
        register_stacks([dataset[template]] + [s for j, s in enumerate(dataset) if j != template], res_s,
                        per_stack_thickness=per_stack_thickness, similarity=similarity, nmi_bins=nmi_bins)
        return dataset
    t0 = time.time()
    stacks = [resample(s.slices * s.mask, (s.resolution_x, s.resolution_y), (res_s, res_s)) for s in dataset]
    transforms = [s.transformation for s in dataset]
    s_thick = float(sum(s.thickness for s in dataset) / len(dataset))
    gaps = [float(s.gap) for s in dataset]
    if per_stack_thickness and (_unequal(gaps) or _unequal([float(s.thickness) for s in dataset])):
        out = stack_registration([transforms], transforms[0], stacks, res_s, gaps[0], gaps, loss=loss)
    else:
        out = stack_registration([transforms], transforms[0], stacks, res_s, s_thick, loss=loss)
    logging.debug("time for stack registration: %f s", time.time() - t0)
    for s, t in zip(dataset, out):
        s.transformation = t
    return dataset


# ---------------------------------------------------------------------------------------------------------------------
# --registration svr
# ---------------------------------------------------------------------------------------------------------------------
def _pad_to(stack: torch.Tensor, size: int) -> Tuple[torch.Tensor, Tuple[float, float]]:
    """(n,1,h,w) zero-padded to (n,1,size,size); also the padded frame's centre relative to the old one, in pixels (x, y)."""
    dx1 = (size - stack.shape[-1]) // 2
    dx2 = (size - stack.shape[-1]) - dx1
    dy1 = (size - stack.shape[-2]) // 2
    dy2 = (size - stack.shape[-2]) - dy1
    return F.pad(stack, (dx1, dx2, dy1, dy2)), ((dx2 - dx1) / 2, (dy2 - dy1) / 2)


def _in_plane_shift(n: int, shift_xy: Tuple[float, float], device) -> RigidTransform:
    mat = torch.eye(3, 4, dtype=torch.float32, device=device).repeat(n, 1, 1)
    mat[:, 0, 3], mat[:, 1, 3] = shift_xy
    return RigidTransform(mat)


def _common_frame(stacks: List[torch.Tensor], transforms: List[RigidTransform], res_s: float
                  ) -> Tuple[torch.Tensor, RigidTransform, List[RigidTransform]]:
    """Stacks (n_j,1,h_j,w_j) of ``res_s`` pixels padded to one square size and concatenated, with the poses of the padded
    frames.  A padded frame's centre may sit half a pixel off the slice's, so  pose of the frame = pose o in-plane shift:
    every pixel keeps its place in the world.  Also returns the shifts per stack, to take a frame's pose back to its slice's
    (``frame_pose.compose(shift.inv())``)."""
    size = max(max(s.shape[-2:]) for s in stacks)
    padded, shifts = zip(*[_pad_to(s, size) for s in stacks])
    to_frame = [_in_plane_shift(s.shape[0], (sx * res_s, sy * res_s), s.device) for s, (sx, sy) in zip(stacks, shifts)]
    poses = RigidTransform.cat([p.compose(t) for p, t in zip(transforms, to_frame)])
    return torch.cat(padded).contiguous(), poses, to_frame


def reconstruct_from_slices(mats: torch.Tensor, slices: torch.Tensor, res_s: float, s_thick, res_r: float,
                            volume_shape: Sequence[int]) -> torch.Tensor:
    """The volume the slice registration aligns to (svort/inference.py:370-406): equalised back-projection, then one CG
    step on the normal equations over the non-zero pixels.  mats (n,3,4) in voxels of ``res_r``, slices (n,1,h,w); ``s_thick``: a
    float, or one thickness per slice (a PSF bank)."""
    from .srr import SRR, PSFreconstruction

    if isinstance(s_thick, (int, float)):
        psf = get_PSF(res_ratio=(res_s / res_r, res_s / res_r, s_thick / res_r), device=slices.device)
    else:  # one thickness per slice
        psf = bank_for(s_thick, res_s, res_r, slices.device)
    params = {"psf": psf, "slice_shape": slices.shape[-2:], "interp_psf": False, "res_s": res_s, "res_r": res_r, "s_thick": s_thick,
              "volume_shape": tuple(int(s) for s in volume_shape)}
    volume = PSFreconstruction(mats, slices, None, None, params)
    return SRR(n_iter=1, use_CG=True)(mats, slices, volume, params, slices_mask=slices > 0)


def _cover_shape(poses: RigidTransform, mask: torch.Tensor, res_s: float, s_thick, res_r: float) -> Tuple[int, int, int]:
    """(D,H,W) of a volume of ``res_r`` voxels, centred at the origin, that holds every masked pixel of the posed slices
    (mask (n,1,h,w)) with the slice thickness (the largest, for one thickness per slice) and a few voxels to spare."""
    if not isinstance(s_thick, (int, float)):
        s_thick = max(float(t) for t in s_thick)
    h, w = mask.shape[-2:]
    grid = meshgrid((w, h), (res_s, res_s), device=mask.device)  # (h,w,2), centred
    pts = torch.cat([grid, torch.zeros_like(grid[..., :1])], -1)[None].expand(mask.shape[0], -1, -1, -1)
    world = mat_transform_points(poses.matrix()[:, None, None], pts, True)[mask[:, 0]]
    half = world.abs().amax(0) + s_thick  # x, y, z
    size = [2 * int(math.ceil(float(v) / res_r)) + 5 for v in half.tolist()]
    return size[2], size[1], size[0]


def register_slices(dataset: List, res_s: float = 1.0, res_r: Optional[float] = None, n_outer: int = 3, template: int = 0,
                    per_stack_thickness: bool = False, packages: Optional[Sequence[int]] = None, package_rounds: int = 2,
                    similarity: str = "ncc", nmi_bins: int = _nmi.DEFAULT_BINS, stack_similarity: str = "ncc") -> List:
    """``--registration svr``: stack registration (``register_stacks``, to the stack ``template``), then ``n_outer`` rounds of
    reconstruct a volume from all slices at their current poses  /  register every non-empty slice rigidly to it (``SVR``,
    global NCC); the per-slice poses are written back into the stacks.  ``res_r``: voxel size of the intermediate volume
    (default ``res_s``).  ``per_stack_thickness`` and stacks of unequal thickness: the stack registration above runs under the
    switch, and the volume and the slice registration take every slice's own thickness (a PSF bank).

    ``packages`` (``--packages``; one count per stack, or one for all): between the stack registration and the slice rounds,
    ``package_rounds`` rounds of reconstruct a volume from all slices  /  register every interleaved package rigidly to it
    (``GroupSVR``).  Slice k of stack s belongs to package ``k mod P_s``, counted in file order before the empty slices are
    dropped; ``P_s = 1`` registers the whole stack against the joint volume.  ``None``: no package stage, as before.

    ``similarity`` (``--svr-similarity``): the metric of the package and the slice stage, ``"ncc"`` (global NCC, as before) or
    ``"nmi"`` - normalised mutual information on a joint histogram of ``nmi_bins`` bins per axis (``--nmi-bins``; nesvor_amd/nmi.py),
    for stacks whose intensities are not linearly related.  ``stack_similarity`` (``--stack-similarity``): the same choice for the
    stack registration in front (``register_stacks``), which keeps its NCC unless told otherwise; ``nmi_bins`` serves both."""
    if similarity not in ("ncc", "nmi"):
        raise ValueError(f"similarity: 'ncc' or 'nmi' expected, got {similarity!r}")
    _stack_loss(stack_similarity, nmi_bins, "stack_similarity")  # (refusals before any work)
    loss_spec = {"name": "ncc"} if similarity == "ncc" else {"name": "nmi", "bins": _nmi.check_bins(nmi_bins, "nmi_bins")}
    metric = similarity.upper()
    if packages is not None:  # (refusals before any work)
        package_groups([s.slices.shape[0] for s in dataset], packages)
    dataset = register_stacks(dataset, res_s, template, per_stack_thickness, similarity=stack_similarity, nmi_bins=nmi_bins)
    t0 = time.time()
    res_r = res_s if res_r is None else res_r
    s_thick = float(sum(s.thickness for s in dataset) / len(dataset))
    stacks = [resample(s.slices * s.mask, (s.resolution_x, s.resolution_y), (res_s, res_s)) for s in dataset]
    slices, poses, to_frame = _common_frame(stacks, [s.transformation for s in dataset], res_s)
    mask = slices > 0
    keep = torch.nonzero(mask.flatten(1).any(1)).flatten()
    slices, mask = slices[keep].contiguous(), mask[keep].contiguous()
    if per_stack_thickness and _unequal([float(s.thickness) for s in dataset]):
        per_slice = [float(s.thickness) for s in dataset for _ in range(s.slices.shape[0])]
        s_thick = [per_slice[k] for k in keep.tolist()]
    theta = poses.axisangle()[keep].clone()
    svr = SVR(num_levels=3, num_steps=4, step_size=2, max_iter=20, optimizer={"name": "gd", "momentum": 0.1}, loss=loss_spec)
    params = {"res_s": res_s, "s_thick": s_thick, "res_r": res_r}
    if packages is not None:
        groups = package_groups([s.slices.shape[0] for s in dataset], packages, keep.tolist())
        gsvr = GroupSVR(num_levels=3, num_steps=4, step_size=2, max_iter=20, optimizer={"name": "gd", "momentum": 0.1},
                        loss=loss_spec)
        for it in range(package_rounds):
            current = RigidTransform(theta)
            shape = _cover_shape(current, mask, res_s, s_thick, res_r)
            volume = reconstruct_from_slices(mat_update_resolution(current.matrix(), 1, res_r), slices, res_s, s_thick, res_r, shape)
            theta, loss = gsvr(theta, groups, slices, mask, volume, params, True)
            logging.debug("package registration round %d: volume %s, mean %s %f", it, shape, metric, -float(loss.mean()))
            if logging.getLogger().isEnabledFor(logging.DEBUG):
                for g, c in enumerate(gsvr.corrections.tolist()):
                    logging.debug("  package %d: rotation (%.3f, %.3f, %.3f) deg, translation (%.3f, %.3f, %.3f) mm", g, *c)
    for it in range(n_outer):
        current = RigidTransform(theta)
        shape = _cover_shape(current, mask, res_s, s_thick, res_r)
        volume = reconstruct_from_slices(mat_update_resolution(current.matrix(), 1, res_r), slices, res_s, s_thick, res_r, shape)
        theta, loss = svr(theta, slices, mask, volume, params, True)
        logging.debug("slice registration round %d: volume %s, mean %s %f", it, shape, metric, -float(loss.mean()))
    full = poses.axisangle().clone()
    full[keep] = theta
    start = 0
    for s, t in zip(dataset, to_frame):
        n = s.slices.shape[0]
        s.transformation = RigidTransform(full[start:start + n]).compose(t.inv())
        start += n
    logging.debug("time for slice registration: %f s", time.time() - t0)
    return dataset
