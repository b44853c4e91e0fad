"""Volume comparison (the ``evaluate`` command): which of several reconstructions of one set of slices is closer to a reference
volume.  ``svr`` writes a world-aligned lattice and ``reconstruct`` the model's own, so a volume is first put onto the
reference's lattice through the two NIfTI poses; PSNR, NRMSE, MAE, correlation and a 3-D SSIM are then taken over the voxels
both volumes cover.  Without ``--align`` nothing is aligned: the volumes must share a world frame (the reconstructions of one set
of registered slices, or of one ``--input-slices`` folder, do).  ``--align translation|rigid`` first finds the rigid correction of
the volume's pose that maximises its correlation with the reference (nesvor_amd/align.py, imported only then) and compares
through the corrected index map; everything below is unchanged by it.  The reference project has no counterpart: the definition
is this module's.

Definition.  R is the reference (image I0 (D,H,W), mask, pose, voxel sizes), X the volume under test (X0 (D',H',W'), mask,
pose, voxel sizes); everything is evaluated on R's lattice.

Index map.  M (3,4) takes an R voxel index (x,y,z) to the continuous X voxel index u:
    M = index_X <- lattice frame of X <- world <- lattice frame of R <- index_R
with the centred lattice frames of ``Image.xyz_masked_untransformed`` (p = (index - (shape - 1) / 2) resolution) and the poses
applied as ``transform_points`` does (world = R_R (p + t_R); back: R_X^T world - t_X).  M is composed in float64 on the host;
u_a = ((M[a,0] x + M[a,1] y) + M[a,2] z) + M[a,3] is evaluated in double in this order.

Inside test.  eps = 2^-20 voxels; on each axis u is inside X where -eps <= u <= size - 1 + eps, and is then clamped to
[0, size - 1] (eps: two identical lattices do not lose their border voxels to a rounding of M).

Resampling.  Trilinear in the images' dtype: i0 = floor(u), f = dtype(u - floor(u)), the upper index min(i0 + 1, size - 1) (its
weight is 0 where it was clamped), lerp(a, b, f) = a + f (b - a) along x, then y, then z.  J0 interpolates X0, mX X's mask as
0 / 1.  v = maskR and inside and mX >= 0.5 (the rule of ``--volume-mask``); J0 = 0 off v.

First sums (fp64 sums of the dtype's terms over v; I = I0 on v, J = J0): {n, n_ref = #maskR, sum I, sum J, sum I^2, sum J^2,
sum I J, max I}.  From them, in fp64 on the device with ``torch.where``: the signed correlation r (0 where varI varJ <= 1e-12,
as ``structural.slice_ncc``); the intensity fit (a, b): ``none`` (1, 0), ``scale`` a = sum IJ / sum JJ, ``affine`` the least
squares of I on J, (1, 0) for a degenerate denominator; L = the given dynamic range or max I; c1 = (0.01 L)^2, c2 = (0.03 L)^2.
(a, b, c1, c2) are rounded to the images' dtype once.

Second pass.  J' = a J + b on v (a multiply, then an add) and 0 elsewhere, e = I - J'.  The SSIM is ``structural.py``'s in three
dimensions: S the separable 11-tap Gaussian window (sigma 1.5 voxels of R's lattice, ``structural.gaussian_taps``), zero
padding, along x, then y, then z, the taps added in ascending order from 0; Wt = S(v) (1 off v),
    muI = S(I) / Wt,  muJ = S(J') / Wt,  sI = S(I I) / Wt - muI^2,  sJ = S(J' J') / Wt - muJ^2,  sIJ = S(I J') / Wt - muI muJ,
    ssim = (2 muI muJ + c1) (2 sIJ + c2) / ((muI^2 + muJ^2 + c1) (sI + sJ + c2))      on v, exactly 0 elsewhere.
Second sums in fp64: {n, sum ssim, sum e^2, sum |e|}.

Report (fp64, ONE host read at the very end): n, coverage = n / n_ref, ncc = r, fit = [a, b], dynamic_range = L, mse, rmse,
nrmse = rmse / L, mae, psnr = 10 log10(L^2 / mse), ssim (the mean).  With n == 0 every metric but n and coverage is NaN;
mse == 0 gives psnr = inf.

Two paths.  On HIP fp32 tensors ``resample_moments`` and ``ssim3d`` are one pass each of ``torch.ops.nesvor.volume_resample`` /
``volume_ssim`` (csrc/evaluate.hip); ``NESVOR_EVALUATE=composed``, host tensors and other dtypes take the same formulas as torch
expressions (``resample_composed``, ``ssim3d_composed``: explicit gathers and shifted slices, no ``grid_sample`` or ``conv3d``,
so that the kernels follow them operation for operation; their float64 evaluation is the yardstick of tests/test_evaluate.py and
tests/test_gpu_evaluate.py).
"""
import json
import logging
import math
import os
from typing import Dict, List, Optional, Tuple

import torch

from . import window as _w
from .structural import MIN_VAR_PRODUCT, gaussian_taps

EPS = 2.0 ** -20  # voxels: the slack of the inside test
FITS = ("none", "scale", "affine")
METRICS = ("n", "coverage", "ncc", "fit", "dynamic_range", "mse", "rmse", "nrmse", "mae", "psnr", "ssim")


def _fused(x: torch.Tensor) -> bool:
    return os.environ.get("NESVOR_EVALUATE", "") != "composed" and x.is_cuda and x.dtype == torch.float32


# ---------------------------------------------------------------------------------------------------------------------
# the index map
# ---------------------------------------------------------------------------------------------------------------------
def _geometry(volume) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(R (3,3), t (3), voxel sizes (3), (shape_xyz - 1) / 2 (3)) of a posed lattice, float64 on the host."""
    mat = volume.transformation.matrix(True)
    if mat.shape[0] != 1:
        raise ValueError("evaluate: a volume with one pose expected")
    mat = mat[0].detach().double().cpu()
    d, h, w = volume.image.shape
    res = torch.tensor([float(volume.resolution_x), float(volume.resolution_y), float(volume.resolution_z)], dtype=torch.float64)
    return mat[:, :3], mat[:, 3], res, torch.tensor([w - 1, h - 1, d - 1], dtype=torch.float64) / 2


def index_map(reference, volume) -> torch.Tensor:
    """M (3,4) float64 on the host: R voxel index (x,y,z,1) -> continuous X voxel index (module docstring)."""
    Rr, tr, sr, cr = _geometry(reference)
    Rx, tx, sx, cx = _geometry(volume)
    rot = Rx.t() @ Rr  # lattice frame of X <- lattice frame of R, up to the translations
    A = rot * sr[None, :] / sx[:, None]
    # u = (rot ((index - cr) sr + tr) - tx) / sx + cx, with the terms grouped so that two identical axis-aligned lattices give the
    # identity exactly (rot = 1: rot tr - tx = 0, A = 1, cx - A cr = 0)
    b = (rot @ tr - tx) / sx + (cx - A @ cr)
    return torch.cat([A, b[:, None]], 1)


# ---------------------------------------------------------------------------------------------------------------------
# the composed path
# ---------------------------------------------------------------------------------------------------------------------
def _lerp(a: torch.Tensor, b: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    return a + f * (b - a)


def interpolate_composed(shape, volume: torch.Tensor, mask: Optional[torch.Tensor], M, dtype=None):
    """(J (D,H,W), mX (D,H,W), inside (D,H,W) bool): X0 and X's mask interpolated at the voxels of a (D,H,W) lattice and the
    inside test, before any validity rule."""
    dtype = volume.dtype if dtype is None else dtype
    dev = volume.device
    m = [[float(v) for v in row] for row in torch.as_tensor(M).reshape(3, 4).tolist()]
    D, H, W = (int(s) for s in shape)
    x = torch.arange(W, dtype=torch.float64, device=dev).view(1, 1, W)
    y = torch.arange(H, dtype=torch.float64, device=dev).view(1, H, 1)
    z = torch.arange(D, dtype=torch.float64, device=dev).view(D, 1, 1)
    inside = torch.ones((D, H, W), dtype=torch.bool, device=dev)
    i0, i1, f = [], [], []
    for a, size in enumerate((volume.shape[2], volume.shape[1], volume.shape[0])):
        u = ((m[a][0] * x + m[a][1] * y) + m[a][2] * z) + m[a][3]
        top = float(size - 1)
        inside = inside & (u >= -EPS) & (u <= top + EPS)
        c = u.clamp(min=0.0, max=top)
        fl = torch.floor(c)
        lo = fl.long().clamp(min=0, max=size - 1)
        i0.append(lo)
        i1.append((lo + 1).clamp(max=size - 1))
        f.append((c - fl).to(dtype))
    (x0, y0, z0), (x1, y1, z1), (fx, fy, fz) = i0, i1, f

    def trilinear(a: torch.Tensor) -> torch.Tensor:
        c00, c01 = _lerp(a[z0, y0, x0], a[z0, y0, x1], fx), _lerp(a[z0, y1, x0], a[z0, y1, x1], fx)
        c10, c11 = _lerp(a[z1, y0, x0], a[z1, y0, x1], fx), _lerp(a[z1, y1, x0], a[z1, y1, x1], fx)
        return _lerp(_lerp(c00, c01, fy), _lerp(c10, c11, fy), fz)

    J = trilinear(volume.to(dtype))
    mX = torch.ones_like(J) if mask is None else trilinear((mask != 0).to(dtype))
    return J, mX, inside


def resample_composed(reference: torch.Tensor, reference_mask: Optional[torch.Tensor], volume: torch.Tensor,
                      volume_mask: Optional[torch.Tensor], M) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (J0 as ``reference``, v (D,H,W) bool, the eight first sums (8) fp64), with the arguments of
    ``torch.ops.nesvor.volume_resample``.  The per-voxel arithmetic is in the reference's dtype (coordinates: float64)."""
    J, mX, inside = interpolate_composed(reference.shape, volume, volume_mask, M, reference.dtype)
    in_ref = torch.ones_like(inside) if reference_mask is None else reference_mask != 0
    v = in_ref & inside & (mX >= 0.5)
    zero = torch.zeros_like(reference)
    i, j = torch.where(v, reference, zero), torch.where(v, J, zero)
    top = torch.where(v, reference, torch.full_like(reference, -float("inf"))).amax().double()
    sums = [t.double().sum() for t in (v, in_ref, i, j, i * i, j * j, i * j)]
    return j, v, torch.stack(sums + [top])


def _window3(a: torch.Tensor, taps) -> torch.Tensor:
    return _w.window(a, taps, 3)


def ssim3d_composed(reference: torch.Tensor, resampled: torch.Tensor, valid: torch.Tensor,
                    params: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (the SSIM map as ``reference``, the four second sums (4) fp64), with the arguments of ``torch.ops.nesvor.volume_ssim``:
    ``params`` = {a, b, c1, c2} as a tensor of the reference's dtype on its device (never read on the host)."""
    v = valid != 0
    a, b, c1, c2 = params.to(reference.dtype).unbind(0)
    taps = gaussian_taps(reference.dtype).tolist()  # host numbers: exactly the dtype's values
    zero = torch.zeros_like(reference)
    i = torch.where(v, reference, zero)
    j = torch.where(v, a * resampled + b, zero)
    ssim = _w.ssim_map(i, j, v, taps, c1, c2, 3)
    e = i - j
    stats = torch.stack([t.double().sum() for t in (v, ssim, e * e, e.abs())])
    return ssim, stats


# ---------------------------------------------------------------------------------------------------------------------
# the two passes on either path, and what lies between them
# ---------------------------------------------------------------------------------------------------------------------
def resample_moments(reference, reference_mask, volume, volume_mask, M):
    if _fused(reference) and volume.is_cuda and volume.dtype == torch.float32:
        flat = [float(v) for v in torch.as_tensor(M).reshape(12).tolist()]
        return torch.ops.nesvor.volume_resample(reference.contiguous(), None if reference_mask is None else reference_mask.contiguous(),
                                                volume.contiguous(), None if volume_mask is None else volume_mask.contiguous(), flat)
    return resample_composed(reference, reference_mask, volume, volume_mask, M)


def ssim3d(reference, resampled, valid, params):
    if _fused(reference):
        return torch.ops.nesvor.volume_ssim(reference.contiguous(), resampled.contiguous(), valid.contiguous(),
                                            params.to(torch.float32).contiguous())
    return ssim3d_composed(reference, resampled, valid, params)


def _ratio(num: torch.Tensor, den: torch.Tensor, ok: torch.Tensor, otherwise: float) -> torch.Tensor:
    return torch.where(ok, num / torch.where(ok, den, torch.ones_like(den)), torch.full_like(num, otherwise))


def fit_from_sums(stats: torch.Tensor, intensity_fit: str = "scale", dynamic_range: Optional[float] = None):
    """The first sums (8) fp64 -> (r, a, b, L), fp64 scalars on the sums' device; no host read."""
    if intensity_fit not in FITS:
        raise ValueError(f"intensity fit {intensity_fit!r}: one of {', '.join(FITS)} expected")
    n, _, s_i, s_j, s_ii, s_jj, s_ij, top = stats.unbind(0)
    one, zero = torch.ones_like(n), torch.zeros_like(n)
    n_safe = torch.where(n > 0, n, one)
    mean_i, mean_j = s_i / n_safe, s_j / n_safe
    cov = s_ij / n_safe - mean_i * mean_j
    var_i, var_j = s_ii / n_safe - mean_i * mean_i, s_jj / n_safe - mean_j * mean_j
    product = var_i * var_j
    ok = product > MIN_VAR_PRODUCT
    r = _ratio(cov, torch.sqrt(torch.where(ok, product, one)), ok, 0.0)
    if intensity_fit == "none":
        a, b = one, zero
    elif intensity_fit == "scale":
        a, b = _ratio(s_ij, s_jj, s_jj > 0, 1.0), zero
    else:
        ok = (n > 0) & (var_j > 0)
        a = _ratio(cov, var_j, ok, 1.0)
        b = torch.where(ok, mean_i - a * mean_j, zero)
    L = top if dynamic_range is None else torch.full_like(top, float(dynamic_range))
    return r, a, b, L


def compare_tensors(reference: torch.Tensor, reference_mask: Optional[torch.Tensor], volume: torch.Tensor,
                    volume_mask: Optional[torch.Tensor], M, intensity_fit: str = "scale", dynamic_range: Optional[float] = None) -> Dict:
    """Both passes and the report as device tensors: ``resampled``, ``valid`` (bool), ``ssim_map`` and ``packed`` (12) fp64 =
    {n, coverage, ncc, a, b, L, mse, rmse, nrmse, mae, psnr, ssim}.  Reads nothing back to the host."""
    resampled, valid, first = resample_moments(reference, reference_mask, volume, volume_mask, M)
    r, a, b, L = fit_from_sums(first, intensity_fit, dynamic_range)
    params = torch.stack([a, b, (0.01 * L) ** 2, (0.03 * L) ** 2]).to(reference.dtype)
    ssim_map, second = ssim3d(reference, resampled, valid, params)
    n, n_ref = first[0], first[1]
    some = n > 0
    nan, one = torch.full_like(n, float("nan")), torch.ones_like(n)
    n_safe = torch.where(some, n, one)
    a_used, b_used = params[0].double(), params[1].double()  # (the rounded values: what the second pass applied)
    mse = torch.where(some, second[2] / n_safe, nan)
    rmse = torch.sqrt(mse)
    psnr = torch.where(mse > 0, 10 * torch.log10(L * L / torch.where(mse > 0, mse, one)),
                       torch.where(mse == 0, torch.full_like(mse, float("inf")), nan))
    packed = torch.stack([n, _ratio(n, n_ref, n_ref > 0, float("nan")), torch.where(some, r, nan), torch.where(some, a_used, nan),
                          torch.where(some, b_used, nan), torch.where(some, L, nan), mse, rmse, rmse / L,
                          torch.where(some, second[3] / n_safe, nan), psnr, torch.where(some, second[1] / n_safe, nan)])
    return {"resampled": resampled, "valid": valid != 0, "ssim_map": ssim_map, "packed": packed}


def compare_volumes(reference, volume, intensity_fit: str = "scale", dynamic_range: Optional[float] = None, align: str = "none",
                    align_levels: int = 3) -> Dict:
    """The report of the module docstring for the ``Volume`` ``volume`` against the ``Volume`` ``reference`` (python numbers), plus
    the device tensors ``resampled`` (J0), ``valid`` (bool) and ``ssim_map`` on the reference's lattice and ``fused``, the path.
    The poses are read where they live (the command keeps them on the host); everything else stays on the device up to the one
    ``tolist`` of the report.  ``align`` = "translation" | "rigid": the comparison runs through M(theta*) of nesvor_amd/align.py
    and the report has an ``alignment`` entry (``align_volumes``'s result)."""
    ref = reference.image if reference.image.is_floating_point() else reference.image.float()
    vol = volume.image.to(device=ref.device, dtype=ref.dtype)
    M, alignment = index_map(reference, volume), None
    if align != "none":
        from . import align as _align

        alignment = _align.align_volumes(reference, volume, dof=align, levels=align_levels)
        M = _align.pose_maps(reference, volume, [alignment["theta"]], alignment["centre"])[0]
    out = compare_tensors(ref.contiguous(), (reference.mask != 0).contiguous(), vol.contiguous(),
                          (volume.mask != 0).to(ref.device).contiguous(), M, intensity_fit, dynamic_range)
    values = out.pop("packed").tolist()  # the one host read
    report = {"n": int(values[0]), "coverage": values[1], "ncc": values[2], "fit": [values[3], values[4]], "dynamic_range": values[5],
              "mse": values[6], "rmse": values[7], "nrmse": values[8], "mae": values[9], "psnr": values[10], "ssim": values[11]}
    report.update(out, fused=_fused(ref))
    if alignment is not None:
        report["alignment"] = alignment
    return report


# ---------------------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------------------
def load_volume(path: str, path_mask: Optional[str] = None, device=torch.device("cpu")):
    """``image_io.load_volume`` for this command: the same array, mask (``> 0`` without a mask file) and voxel sizes; the pose is
    kept as the matrix the file's affine gives (the slices' common rotation, the mean of their offsets), not taken through the
    axis-angle conversion, which the index map has no use for."""
    from .image import Volume
    from .image_io import _load_with_mask, affine2transformation
    from .transform import RigidTransform

    vol, mask, resolutions, affine = _load_with_mask(path, path_mask)
    t, m, transformation = affine2transformation(torch.tensor(vol), torch.tensor(mask), resolutions, affine)
    mat = transformation.matrix(True)
    pose = torch.cat([mat[:1, :, :3], mat[:, :, 3:].double().mean(0, keepdim=True).to(mat.dtype)], -1)
    return Volume(image=t.to(device), mask=m.to(device), transformation=RigidTransform(pose, trans_first=True),  # (the pose: on the host)
                  resolution_x=float(resolutions[0]), resolution_y=float(resolutions[1]), resolution_z=float(resolutions[2]))


def _finite(v):
    """JSON has no NaN or infinity: a non-finite number is written as null."""
    if isinstance(v, float):
        return v if math.isfinite(v) else None
    if isinstance(v, (list, tuple)):
        return [_finite(x) for x in v]
    if isinstance(v, dict):  # (the ``alignment`` entry)
        return {k: _finite(x) for k, x in v.items()}
    return v


def format_table(rows: List[Dict]) -> str:
    aligned = any("alignment" in r for r in rows)  # (with --align: the rotation and translation of the correction)
    head = f"{'volume':<32} {'n':>10} {'cover':>7} {'PSNR':>8} {'NRMSE':>8} {'MAE':>10} {'NCC':>7} {'SSIM':>7}"
    head += f" {'rot deg':>8} {'shift mm':>8}  fit" if aligned else "  fit"
    lines = [head]
    for r in rows:
        name = os.path.basename(str(r["input_volume"]))
        line = (f"{name[-32:]:<32} {r['n']:>10d} {r['coverage']:>7.4f} {r['psnr']:>8.3f} {r['nrmse']:>8.5f} {r['mae']:>10.4g} "
                f"{r['ncc']:>7.4f} {r['ssim']:>7.4f}")
        if aligned:
            line += f" {r['alignment']['rotation_deg']:>8.3f} {r['alignment']['translation_mm']:>8.3f}"
        lines.append(line + f"  {r['fit'][0]:.5g} x + {r['fit'][1]:.5g}")
    return "\n".join(lines)


def evaluate_command(args) -> List[Dict]:
    """``evaluate``: every ``--input-volumes`` file against ``--reference-volume``; returns the rows it logs and writes."""
    from .image import Volume

    inputs = list(args.input_volumes)
    for name in ("input_masks", "output_ssim_maps", "output_resampled", "output_aligned"):
        if getattr(args, name, None) is not None and len(getattr(args, name)) != len(inputs):
            raise SystemExit(f"The numbers of {name.replace('_', ' ')} and input volumes are different!")
    align = getattr(args, "align", None) or "none"
    if align == "none" and getattr(args, "output_aligned", None):
        raise SystemExit("--output-aligned needs --align translation or --align rigid!")
    device = getattr(args, "device", None) or torch.device("cpu")
    reference = load_volume(args.reference_volume, getattr(args, "reference_mask", None), device)
    rows = []
    for k, path in enumerate(inputs):
        volume = load_volume(path, args.input_masks[k] if getattr(args, "input_masks", None) else None, device)
        extra = {} if align == "none" else {"align": align, "align_levels": getattr(args, "align_levels", 3)}
        report = compare_volumes(reference, volume, getattr(args, "intensity_fit", "scale"), getattr(args, "dynamic_range", None), **extra)
        if report["n"] == 0:
            logging.warning("evaluate: %s shares no voxel with the reference (do the volumes share a world frame?)", path)
        for name, key in (("output_ssim_maps", "ssim_map"), ("output_resampled", "resampled")):
            if getattr(args, name, None):
                Volume(report[key].cpu(), report["valid"].cpu(), reference.transformation, reference.resolution_x, reference.resolution_y,
                       reference.resolution_z).save(getattr(args, name)[k], masked=False)
        rows.append({"input_volume": path, **{key: report[key] for key in METRICS}})
        if align != "none":
            from . import align as _align

            result = report["alignment"]
            rows[-1]["alignment"] = _align.report_entry(result)
            if getattr(args, "output_aligned", None):  # the input's own voxels and mask with the pose G^-1 o T_X: nothing is resampled
                Volume(volume.image.cpu(), volume.mask.cpu(), _align.aligned_pose(volume, result["theta"], result["centre"]),
                       volume.resolution_x, volume.resolution_y, volume.resolution_z).save(args.output_aligned[k])
    logging.info("Volume comparison against %s (intensity fit: %s):\n%s", args.reference_volume, getattr(args, "intensity_fit", "scale"),
                 format_table(rows))
    if getattr(args, "output_json", None):
        with open(args.output_json, "w") as f:
            json.dump([{k: _finite(v) for k, v in row.items()} for row in rows], f, indent=1)
    return rows
