"""Classical slice-to-volume reconstruction (the ``svr`` command): motion-corrected slices -> a volume, without training
an INR.  The pipeline the survey's row f1 calls "a classical SRR baseline": the slices of all stacks on one padded frame
(``registration._common_frame``), a world-aligned volume that covers them (``registration._cover_shape``), the equalised
back-projection ``PSFreconstruction`` as start and ``srr.srr_descent`` - gradient descent on the weighted data term with the
edge-preserving prior, one fused HIP launch per update (csrc/srr.hip) - to refine it.

Optional robust statistics (``--outlier-rejection``; ``reconstruct_volume(robust_rounds=R)``, nesvor_amd/robust.py): the EM
scheme of Kuklisova-Murgasova et al. 2012 gives every pixel a posterior weight, every slice a weight and an intensity scale;
the descent is split into R rounds, each on the weights and scaled slices the statistics of the current A x give.  One pass
of a fused HIP kernel per round (csrc/robust.hip).  Without the flag the pipeline is the plain one, bit for bit.

Optional structural exclusion (``--structural-exclusion``; ``reconstruct_volume(structural=StructuralExclusion())``,
nesvor_amd/structural.py): after the EM round, if any, every round compares each slice with its simulation - a local SSIM map
drops pixels, the slice's correlation drops whole slices - and the descent runs on what is kept.  One pass of a fused HIP
kernel per round (csrc/structural.hip).  Without the flag nothing changes.

Optional slice bias fields (``--slice-bias-fields``; ``reconstruct_volume(slice_bias=SliceBias())``, nesvor_amd/slice_bias.py):
every round estimates a smooth multiplicative field per slice from the log-ratio of the slice to its simulation, after the EM
round and the structural step, if any, and the descent runs on the corrected slices.  Two passes of a fused HIP kernel per
round (csrc/slice_bias.hip).  Without the flag nothing changes.

Optional per-stack slice profiles (``--per-stack-thickness``; ``s_thick`` as one value per slice, nesvor_amd/psf_bank.py): every
slice is simulated with the PSF of its own thickness - a PSF bank, looked up per slice inside the one launch of A and of A^T
(csrc/slice_acq.hip, csrc/svr.hip) - in the descent, the statistics above and the registration.  Without the flag the mean
thickness is used for every stack, and nothing changes.

Out of scope here: a gauge for the robust scales, robust weights and bias fields inside the ``--registration svr`` rounds.  A volume mask, the stacks' intersection and intensity
thresholds narrow the stacks' masks as they are loaded (``--volume-mask`` and the other stack masking flags, nesvor_amd/masking.py).
"""
import json
import logging
import time
from argparse import Namespace
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .image import Slice, Volume
from .psf_bank import SAME_THICKNESS, as_thickness_list, bank_for, group_thicknesses
from .registration import _common_frame, _cover_shape, resample
from .robust import RobustStatistics
from .slice_bias import MIN_WEIGHT, SliceBias, eligible
from .srr import AcquisitionOperator, PSFreconstruction, srr_descent
from .structural import StructuralExclusion
from .transform import RigidTransform, mat_update_resolution
from .utils import get_PSF

MIXED_SLICES_MESSAGE = ("--input-slices needs slices of one pixel size and one thickness (what the `register` command writes); "
                        "pass the stacks through --input-stacks instead")


def _as_list(v) -> List:
    return list(v) if isinstance(v, (list, tuple)) else [v]


def _frame_keep(slices, mask, poses, res_s: float) -> Tuple[torch.Tensor, torch.Tensor, RigidTransform, torch.Tensor]:
    """Stacks (n_j,1,h_j,w_j) (or one), their masks (or None: the non-zero pixels) and poses -> the non-empty slices on one
    padded frame (n,1,s,s), their masks (the non-zero masked pixels), the frames' poses and the kept slices' indices in the
    concatenated input."""
    stacks, poses = _as_list(slices), _as_list(poses)
    if mask is not None:
        stacks = [s * m.to(s.dtype) for s, m in zip(stacks, _as_list(mask))]
    images, frame_poses, _ = _common_frame(stacks, poses, res_s)
    m = images > 0
    keep = torch.nonzero(m.flatten(1).any(1)).flatten()
    return images[keep].contiguous(), m[keep].contiguous(), frame_poses[keep], keep


def _frame(slices, mask, poses, res_s: float) -> Tuple[torch.Tensor, torch.Tensor, RigidTransform]:
    """``_frame_keep`` without the indices."""
    return _frame_keep(slices, mask, poses, res_s)[:3]


def _kept_thickness(s_thick, slices, keep: torch.Tensor):
    """``s_thick`` of the kept slices: the float as it is, or the entries of the list - one per slice of the concatenated input
    ``slices`` (stacks, or their number of slices) - at ``keep``."""
    if isinstance(s_thick, (int, float)):
        return s_thick
    n_input = slices if isinstance(slices, int) else sum(s.shape[0] for s in _as_list(slices))
    per_slice = as_thickness_list(s_thick, n_input)
    return [per_slice[k] for k in keep.tolist()]


def _operator(images: torch.Tensor, m: torch.Tensor, frame_poses: RigidTransform, res_s: float, s_thick, res_r: float,
              volume_shape: Sequence[int]) -> Tuple[AcquisitionOperator, Dict]:
    """``s_thick``: a float (one PSF), or one thickness per slice of ``images`` (a PSF bank; one PSF if they all agree)."""
    if isinstance(s_thick, (int, float)):
        psf = get_PSF(res_ratio=(res_s / res_r, res_s / res_r, s_thick / res_r), device=images.device)
    else:
        psf = bank_for(s_thick, res_s, res_r, images.device)
    params = {"psf": psf,
              "slice_shape": images.shape[-2:], "interp_psf": False, "res_s": res_s, "res_r": res_r, "s_thick": s_thick,
              "volume_shape": tuple(int(s) for s in volume_shape)}
    mats = mat_update_resolution(frame_poses.matrix(), 1, res_r).contiguous()
    return AcquisitionOperator(mats, params, None, m), params


def reconstruct_volume(slices, mask, poses, res_s: float, s_thick, res_r: float, n_iter: int = 30, beta: float = 0.02,
                       delta: float = 0.1, robust_rounds: int = 0, robust_out: Optional[Dict] = None,
                       structural: Optional[StructuralExclusion] = None, structural_out: Optional[Dict] = None,
                       slice_bias: Optional[SliceBias] = None, slice_bias_out: Optional[Dict] = None) -> Volume:
    """Slices at their poses -> the reconstructed ``Volume``: world-aligned (identity pose, centred at the origin), voxel size
    ``res_r``, large enough for every masked pixel; its mask is the set of voxels a masked pixel's PSF reaches (A^T 1 > 0).

    slices: a stack (n,1,h,w) of ``res_s`` pixels or a list of stacks; mask: the same of bool, or None (the non-zero pixels);
    poses: a ``RigidTransform`` per stack (one pose per slice).  ``s_thick``: the slice thickness, a float - or one value per slice
    of the concatenated input (per-stack slice profiles: every slice takes the PSF of its own thickness, the volume covers the
    largest).  ``beta`` / ``delta``: the prior's weight and edge scale as the
    reference's ``SRR`` takes them; ``n_iter`` descent steps of length 1 / L (``srr.descent_step_bound``) from the equalised
    back-projection.

    ``robust_rounds`` R > 0: outlier rejection and slice scales (nesvor_amd/robust.py).  The statistics are initialised on A x
    of the back-projection; then R times: one EM round on the current A x, and ``n_iter // R`` descent steps (the remainder
    goes to the last round) on the scaled slices with the pixel weights p * slice weight; the step length is bounded anew
    for every round's weights (one scalar read per round).  ``robust_out``, a dict, then receives ``slice_weight`` and
    ``scale`` (n, one entry per non-empty slice, in the order of the concatenated input) and ``keep`` (their indices there).
    More rounds than descent steps are cut to ``n_iter`` (at least one), so no round runs without a step.
    ``robust_rounds=0`` is the plain pipeline and leaves ``robust_out`` alone.

    ``structural``, a ``StructuralExclusion`` (nesvor_amd/structural.py): the descent is split into ``robust_rounds`` rounds
    (``structural.rounds``, 3 by default, if that is 0; cut to ``n_iter`` as above).  Each round takes A x once, runs the EM round on it if ``robust_rounds`` > 0,
    then ``structural.update`` on the slices with the robust scales (or as they are), and descends with the pixel weights
    ``structural.weights()`` (times the robust ones) on the robustly scaled slices (or as they are).  Decisions are taken anew
    every round.  ``structural_out`` then receives ``ncc``, ``slice_keep`` and ``pixel_share`` (n, as above) and ``keep``.
    ``structural=None`` leaves everything above as it is.

    ``slice_bias``, a ``SliceBias`` (nesvor_amd/slice_bias.py): the descent is split into ``robust_rounds`` rounds (if that is 0:
    ``structural.rounds`` with ``structural``, else ``slice_bias.rounds``, 3 by default; cut to ``n_iter`` as above).  Each round takes A x once, runs the EM round,
    if ``robust_rounds`` > 0, and the structural update, if any, on the slices corrected by the current fields, then
    ``slice_bias.update`` on the acquired slices with the robust scales and the round's pixel weights, and descends on the
    (robustly scaled) corrected slices with those weights.  ``slice_bias_out`` then receives ``b`` (the log-fields, as the
    framed slices), ``stats`` (n,5), ``eligible`` (as ``b``, bool: the last round's eligible pixels), ``bias_rms`` (n, the rms of
    ``b`` over them) and ``keep``; ``robust_out`` and ``structural_out`` as above.  ``slice_bias=None`` leaves everything above as
    it is."""
    images, m, frame_poses, keep = _frame_keep(slices, mask, poses, res_s)
    if images.shape[0] == 0:
        raise ValueError("reconstruct_volume: every slice is empty")
    s_thick = _kept_thickness(s_thick, slices, keep)
    shape = _cover_shape(frame_poses, m, res_s, s_thick, res_r)
    op, params = _operator(images, m, frame_poses, res_s, s_thick, res_r, shape)
    start = PSFreconstruction(op.transforms, images, m, None, params)
    if slice_bias is not None:
        x = start
        rounds = robust_rounds if robust_rounds > 0 else (structural.rounds if structural is not None else slice_bias.rounds)
        rounds = max(1, min(rounds, n_iter))
        stats = RobustStatistics().init(op.forward(x), images, m) if robust_rounds > 0 else None
        for r in range(rounds):
            sim = op.forward(x)
            corrected = slice_bias.corrected(images)
            p = None
            if stats is not None:
                stats.update(sim, corrected, m)
                p = stats.weights()
            if structural is not None:
                structural.update(sim, corrected, m, None if stats is None else stats.scale)
                p = structural.weights() if p is None else p * structural.weights()
            slice_bias.update(sim, images, m, None if stats is None else stats.scale, p, res_s)
            corrected = slice_bias.corrected(images)
            steps = n_iter // rounds + (n_iter % rounds if r + 1 == rounds else 0)
            x = srr_descent(op, corrected if stats is None else stats.scaled(corrected), x, steps, beta, delta, p=p)
        if stats is not None and robust_out is not None:
            robust_out.update(slice_weight=stats.slice_weight, scale=stats.scale, keep=keep)
        if structural is not None and structural_out is not None:
            structural_out.update(ncc=structural.ncc, slice_keep=structural.slice_keep, pixel_share=structural.pixel_share(), keep=keep)
        if slice_bias_out is not None:
            slice_bias_out.update(b=slice_bias.b, stats=slice_bias.stats, bias_rms=slice_bias.rms(sim, images, m),
                                  eligible=eligible(sim, images, m, slice_bias.min_intensity), keep=keep)
    elif structural is not None:
        x = start
        rounds = max(1, min(robust_rounds if robust_rounds > 0 else structural.rounds, n_iter))
        stats = RobustStatistics().init(op.forward(x), images, m) if robust_rounds > 0 else None
        for r in range(rounds):
            sim = op.forward(x)
            if stats is not None:
                stats.update(sim, images, m)
            structural.update(sim, images, m, None if stats is None else stats.scale)
            p = structural.weights() if stats is None else stats.weights() * structural.weights()
            steps = n_iter // rounds + (n_iter % rounds if r + 1 == rounds else 0)
            x = srr_descent(op, images if stats is None else stats.scaled(images), x, steps, beta, delta, p=p)
        if stats is not None and robust_out is not None:
            robust_out.update(slice_weight=stats.slice_weight, scale=stats.scale, keep=keep)
        if structural_out is not None:
            structural_out.update(ncc=structural.ncc, slice_keep=structural.slice_keep, pixel_share=structural.pixel_share(), keep=keep)
    elif robust_rounds > 0:
        x = start
        rounds = max(1, min(robust_rounds, n_iter))
        stats = RobustStatistics().init(op.forward(x), images, m)
        for r in range(rounds):
            stats.update(op.forward(x), images, m)
            steps = n_iter // rounds + (n_iter % rounds if r + 1 == rounds else 0)
            x = srr_descent(op, stats.scaled(images), x, steps, beta, delta, p=stats.weights())
        if robust_out is not None:
            robust_out.update(slice_weight=stats.slice_weight, scale=stats.scale, keep=keep)
    else:
        x = srr_descent(op, images, start, n_iter, beta, delta)
    cover = op.adjoint(torch.ones_like(images)) > 0
    return Volume(x[0, 0], cover[0, 0], None, res_r, res_r, res_r)


def _thickness_of(s_thick, k: int) -> float:
    return s_thick if isinstance(s_thick, (int, float)) else s_thick[k]


def simulate_slices(volume: Volume, slices, mask, poses, res_s: float, s_thick) -> List[Slice]:
    """A x at the slices' poses through the acquisition operator: one ``Slice`` (on the padded frame, with the frame's pose and
    the acquired slice's mask) per non-empty input slice.  ``s_thick`` as ``reconstruct_volume`` takes it: with one value per
    slice every written slice carries its own."""
    if isinstance(s_thick, (int, float)):
        images, m, frame_poses = _frame(slices, mask, poses, res_s)
    else:
        images, m, frame_poses, keep = _frame_keep(slices, mask, poses, res_s)
        s_thick = _kept_thickness(s_thick, slices, keep)
    res_r = float(volume.resolution_x)
    op, _ = _operator(images, m, frame_poses, res_s, s_thick, res_r, volume.image.shape)
    sim = op.forward(volume.image[None, None].contiguous())
    return [Slice(sim[k], m[k], frame_poses[k], res_s, res_s, _thickness_of(s_thick, k)) for k in range(sim.shape[0])]


def corrected_slices(b: torch.Tensor, slices, mask, poses, res_s: float, s_thick) -> List[Slice]:
    """y exp(-b) for the log-fields ``b`` that ``reconstruct_volume(slice_bias_out=...)`` returned: one ``Slice`` (on the padded
    frame, with the frame's pose and the acquired slice's mask) per non-empty input slice."""
    if isinstance(s_thick, (int, float)):
        images, m, frame_poses = _frame(slices, mask, poses, res_s)
    else:
        images, m, frame_poses, keep = _frame_keep(slices, mask, poses, res_s)
        s_thick = _kept_thickness(s_thick, slices, keep)
    corrected = images * torch.exp(-b)
    return [Slice(corrected[k], m[k], frame_poses[k], res_s, res_s, _thickness_of(s_thick, k)) for k in range(corrected.shape[0])]


# ---------------------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------------------
def _group(slices: List[Slice], res_s: Optional[float]) -> Tuple[List[torch.Tensor], List[torch.Tensor], List[RigidTransform], float]:
    """Runs of slices with one shape and pixel size -> stacks (n_j,1,h,w) resampled in-plane to ``res_s`` (None: the finest
    pixel size among them), their masks and poses.  ``resample`` keeps the centre of the frame, so the poses stay."""
    if res_s is None:
        res_s = min(min(float(s.resolution_x), float(s.resolution_y)) for s in slices)
    key = lambda s: (tuple(s.image.shape), float(s.resolution_x), float(s.resolution_y))
    runs: List[List[Slice]] = []
    for s in slices:
        if runs and key(runs[-1][0]) == key(s):
            runs[-1].append(s)
        else:
            runs.append([s])
    stacks, masks, poses = [], [], []
    for run in runs:
        img = torch.stack([s.image * s.mask.to(s.image.dtype) for s in run])  # (n,1,h,w)
        rx, ry = float(run[0].resolution_x), float(run[0].resolution_y)
        if abs(rx - res_s) > 1e-3 * res_s or abs(ry - res_s) > 1e-3 * res_s:
            img = resample(img, (rx, ry), (res_s, res_s))
        stacks.append(img.contiguous())
        masks.append(img > 0)
        poses.append(RigidTransform.cat([s.transformation for s in run]))
    return stacks, masks, poses, res_s


def svr_command(args: Namespace) -> Dict:
    """``nesvor_amd.cli svr``: load, register (``cli.register``), reconstruct; returns what ``cli._outputs`` writes."""
    from . import cli
    from .image_io import load_slices

    if args.input_slices is None and args.input_stacks is None:
        raise SystemExit("No image data provided! Use --input-slices or --input-stacks to input data.")
    use_structural = bool(getattr(args, "structural_exclusion", False))
    use_bias = bool(getattr(args, "slice_bias_fields", False))
    per_stack = bool(getattr(args, "per_stack_thickness", False))
    if getattr(args, "slice_weights", None) and not getattr(args, "outlier_rejection", False) and not use_structural and not use_bias:
        raise SystemExit("--slice-weights needs --outlier-rejection: without it no slice weights are estimated")
    if getattr(args, "output_corrected_slices", None) and not use_bias:
        raise SystemExit("--output-corrected-slices needs --slice-bias-fields: without it no field is estimated")
    t0 = time.time()
    if args.input_slices is not None:
        if args.input_stacks or args.stack_masks or args.thicknesses:
            logging.warning("Since <input-slices> is provided, <input-stacks>, <stack_masks> and <thicknesses> would be ignored.")
        cli.warn_template_ignored(args, "--input-slices")
        cli.warn_packages_ignored(args, "--input-slices")
        cli.warn_similarity_ignored(args, "--input-slices")
        cli.warn_masking_ignored(args, "--input-slices")
        cli.warn_denoise_ignored(args, "--input-slices")
        loaded = load_slices(args.input_slices, args.device)
        for i, s in enumerate(loaded):  # the files carry no stack: a slice is known by its place in the folder's numeric order
            s.slice_idx = i
        slices = [s for s in loaded if bool(s.mask.any())]
        if not slices:
            raise SystemExit("No non-empty slice found in --input-slices")
        sizes = [(float(s.resolution_x), float(s.resolution_y), float(s.resolution_z)) for s in slices]
        res_s, s_thick = sizes[0][0], sizes[0][2]
        mixed_thickness = any(abs(rz - s_thick) > SAME_THICKNESS for _, _, rz in sizes)
        if any(abs(rx - res_s) > 1e-3 or abs(ry - res_s) > 1e-3 for rx, ry, _ in sizes) or (mixed_thickness and not per_stack):
            raise SystemExit(MIXED_SLICES_MESSAGE)
        stacks, masks, poses, res_s = _group(slices, res_s)
    else:
        loaded = cli._load_stacks(args)
        thick = [float(s.thickness) for s in loaded]
        s_thick = sum(thick) / len(thick)
        if max(thick) - min(thick) > 0.01 * s_thick and not per_stack:
            logging.warning("The stacks' thicknesses differ (%s): the mean, %.3f mm, is used for all of them", thick, s_thick)
        slices = cli.register(args, loaded)  # non-empty slices, each stack normalised by its 0.99 quantile
        stacks, masks, poses, res_s = _group(slices, None)
    logging.info("Data loading and registration finished in %.1f s (%d slices, pixel size %.3f mm, thickness %.3f mm)",
                 time.time() - t0, len(slices), res_s, s_thick)
    if per_stack:
        # every slice carries its stack's thickness (Slice.resolution_z); slices that agree within 1e-3 mm keep today's path
        per_slice = [float(s.resolution_z) for s in slices]
        members, ids = group_thicknesses(per_slice)
        logging.info("Per-stack slice profiles: %s", ", ".join(f"{t:.3f} mm x {ids.count(g)} slices" for g, t in enumerate(members)))
        if len(members) > 1:
            s_thick = per_slice
    t0 = time.time()
    robust: Dict = {}
    structural: Dict = {}
    fields: Dict = {}
    if use_bias:
        if args.robust_rounds < 1:
            raise SystemExit("--robust-rounds must be at least 1")
        if not args.bias_sigma > 0:
            raise SystemExit("--bias-sigma must be positive")
        exclusion = (StructuralExclusion(args.local_ssim_threshold, args.global_ncc_threshold, rounds=args.robust_rounds)
                     if use_structural else None)
        robust_rounds = args.robust_rounds if getattr(args, "outlier_rejection", False) else 0
        volume = reconstruct_volume(stacks, masks, poses, res_s, s_thick, args.output_resolution, args.n_iter_srr, args.srr_beta,
                                    args.srr_delta, robust_rounds=robust_rounds, robust_out=robust, structural=exclusion,
                                    structural_out=structural, slice_bias=SliceBias(args.bias_sigma, rounds=args.robust_rounds),
                                    slice_bias_out=fields)
    elif use_structural:
        if args.robust_rounds < 1:
            raise SystemExit("--robust-rounds must be at least 1")
        exclusion = StructuralExclusion(args.local_ssim_threshold, args.global_ncc_threshold, rounds=args.robust_rounds)
        robust_rounds = args.robust_rounds if getattr(args, "outlier_rejection", False) else 0
        volume = reconstruct_volume(stacks, masks, poses, res_s, s_thick, args.output_resolution, args.n_iter_srr, args.srr_beta,
                                    args.srr_delta, robust_rounds=robust_rounds, robust_out=robust, structural=exclusion,
                                    structural_out=structural)
    elif getattr(args, "outlier_rejection", False):
        if args.robust_rounds < 1:
            raise SystemExit("--robust-rounds must be at least 1")
        volume = reconstruct_volume(stacks, masks, poses, res_s, s_thick, args.output_resolution, args.n_iter_srr, args.srr_beta,
                                    args.srr_delta, robust_rounds=args.robust_rounds, robust_out=robust)
    else:
        volume = reconstruct_volume(stacks, masks, poses, res_s, s_thick, args.output_resolution, args.n_iter_srr, args.srr_beta,
                                    args.srr_delta)
    if args.device.type == "cuda":
        torch.cuda.synchronize(args.device)
    logging.info("Reconstruction finished in %.1f s (volume %s)", time.time() - t0, tuple(volume.image.shape))
    rows = None
    if robust:
        weight, scale, keep = robust["slice_weight"].tolist(), robust["scale"].tolist(), robust["keep"].tolist()
        logging.info("Outlier rejection: %d of %d slices ended with a weight below 0.5; slice scales %.3f .. %.3f",
                     sum(w < 0.5 for w in weight), len(weight), min(scale), max(scale))
        # stack: the index among --input-stacks, slice: the index inside that stack; with --input-slices stack is null and
        # slice the file's place in the folder's numeric order
        rows = [{"stack": slices[k].stack_idx, "slice": slices[k].slice_idx, "weight": w, "scale": s}
                for k, w, s in zip(keep, weight, scale)]
    if structural:
        ncc, share, kept = structural["ncc"].tolist(), structural["pixel_share"].tolist(), structural["slice_keep"].tolist()
        keep = structural["keep"].tolist()
        logging.info("Structural exclusion: %d of %d slices ended excluded; %.1f %% of the pixels of the others kept",
                     len(kept) - sum(kept), len(kept), 100.0 * sum(s for s, k in zip(share, kept) if k) / max(sum(kept), 1))
        if not any(kept):
            logging.warning("Structural exclusion: every slice ended excluded (no slice correlates with its simulation above %g): "
                            "the last round descended on the prior alone", args.global_ncc_threshold)
        if rows is None:
            rows = [{"stack": slices[k].stack_idx, "slice": slices[k].slice_idx} for k in keep]
        for row, r, s, k in zip(rows, ncc, share, kept):
            row.update(ncc=r, pixel_share=s, excluded=not k)
    if fields:
        rms, updated = fields["bias_rms"].tolist(), (fields["stats"][:, 1] >= MIN_WEIGHT).tolist()
        logging.info("Slice bias fields: the last round updated %d of %d slices (the others have too little weight); rms of the "
                     "log-fields %.3f at most", sum(updated), len(updated), max(rms))
        if rows is None:
            rows = [{"stack": slices[k].stack_idx, "slice": slices[k].slice_idx} for k in fields["keep"].tolist()]
        for row, v in zip(rows, rms):
            row.update(bias_rms=v)
    if rows is not None and getattr(args, "slice_weights", None):
        with open(args.slice_weights, "w") as f:
            json.dump(rows, f, indent=1)
    data = {"output_volume": volume, "output_slices": slices}
    if fields and getattr(args, "output_corrected_slices", None):
        data["output_corrected_slices"] = corrected_slices(fields["b"], stacks, masks, poses, res_s, s_thick)
    if args.simulated_slices:
        data["simulated_slices"] = simulate_slices(volume, stacks, masks, poses, res_s, s_thick)
    return data
