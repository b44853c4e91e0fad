"""Command-line front end with the flag names and defaults of ``nesvor`` (nesvor/cli/main.py:27-326,
nesvor/cli/commands.py:64-146) for the commands that sit on the built path:

    python -m nesvor_amd.cli reconstruct   --input-stacks a.nii.gz b.nii.gz [--stack-masks ...] [--thicknesses ...]
                                           | --input-slices DIR   --output-volume v.nii.gz [--output-model m.pt]
                                           [--output-slices DIR] [--simulated-slices DIR]  [training flags]
    python -m nesvor_amd.cli register      --input-stacks a.nii.gz b.nii.gz --output-slices DIR [--registration stack|svr|none]
                                           [--template-stack 0|K|auto] [--template-metric ncc|matrix-rank|volume]
    python -m nesvor_amd.cli svr           --input-stacks a.nii.gz b.nii.gz c.nii.gz [--stack-masks ...] [--thicknesses ...]
                                           | --input-slices DIR   --output-volume v.nii.gz [--output-slices DIR]
                                           [--simulated-slices DIR] [--registration svr|stack|none] [--output-resolution 0.8]
                                           [--n-iter-srr 30] [--srr-beta 0.02] [--srr-delta 0.1]
                                           [--outlier-rejection] [--structural-exclusion [--local-ssim-threshold 0.4]
                                           [--global-ncc-threshold 0.5]] [--robust-rounds 3] [--slice-weights FILE.json]
                                           [--slice-bias-fields [--bias-sigma 12] [--output-corrected-slices DIR]]
                                           [--template-stack 0|K|auto] [--template-metric ncc|matrix-rank|volume]
    python -m nesvor_amd.cli assess        --input-stacks a.nii.gz b.nii.gz c.nii.gz [--stack-masks ...] [--thicknesses ...]
                                           [--metric ncc|matrix-rank|volume] [--output-json FILE.json]
    python -m nesvor_amd.cli correct-bias-field --input-stacks a.nii.gz b.nii.gz [--stack-masks ...]
                                           --output-corrected-stacks ca.nii.gz cb.nii.gz [--output-bias-fields fa.nii.gz fb.nii.gz]
    python -m nesvor_amd.cli denoise       --input-stacks a.nii.gz b.nii.gz [--stack-masks ...] --output-stacks da.nii.gz db.nii.gz
                                           [--output-json FILE.json]
    python -m nesvor_amd.cli evaluate      --reference-volume r.nii.gz [--reference-mask ...] --input-volumes a.nii.gz b.nii.gz
                                           [--input-masks ...] [--intensity-fit none|scale|affine] [--dynamic-range L]
                                           [--output-json FILE.json] [--output-ssim-maps ...] [--output-resampled ...]
    python -m nesvor_amd.cli sample-volume --input-model m.pt --output-volume v.nii.gz [--output-resolution 0.8] ...
    python -m nesvor_amd.cli sample-slices --input-model m.pt --input-slices DIR --simulated-slices DIR

Differences from the reference, all because the SVoRT transformer (pretrained weights, torchvision) is out of scope
here: ``--registration`` accepts the reference's choices, of which ``none`` (the default; the reference defaults to
``svort``), ``stack`` (stack-to-stack rigid registration) and ``svr`` (stack registration, then every slice registered
rigidly to a volume reconstructed from all of them; not a choice of the reference; both in nesvor_amd/registration.py)
are implemented; the ``register`` command offers the same three.  Precision follows the reference's switch
(``--single-precision`` = the fp32 model with biased Linear layers; the default is the reference's half-precision
structure - bias-free networks - which the HIP path evaluates with bf16 matrix operands and fp32 accumulation;
``--mlp-fp16`` without ``--single-precision`` trains that structure with power-of-two-scaled fp16 operands instead, on
the kernels' bias-free forms, and ``--fp16-loss-scaling`` with fp16 operands under the reference's loss scaler).

Not in the reference (it is single-process): ``torchrun --nproc-per-node N -m nesvor_amd.cli reconstruct ...`` trains data-parallel,
one process per GPU (nesvor_amd/ddp.py); rank 0 samples and writes the outputs.  The other commands stay single-process.

Also not in the reference: ``svr``, the classical pipeline without an INR - registration (default ``svr``), then a
super-resolution reconstruction by gradient descent with the edge-preserving prior (nesvor_amd/svr.py, csrc/srr.hip).
``--outlier-rejection`` adds the EM pixel and slice weights and slice scales (nesvor_amd/robust.py), ``--structural-exclusion``
drops slices whose correlation with their simulation is below ``--global-ncc-threshold`` and pixels whose local SSIM is
below ``--local-ssim-threshold`` (nesvor_amd/structural.py, csrc/structural.hip); ``--robust-rounds`` splits the descent for
either, ``--slice-weights`` writes what either decided per slice.  ``--slice-bias-fields`` estimates, in the same rounds, a
smooth multiplicative field per slice from the log-ratio of the slice to its simulation (Gaussian window of ``--bias-sigma`` mm;
nesvor_amd/slice_bias.py, csrc/slice_bias.hip) and descends on the corrected slices; ``--output-corrected-slices`` writes them,
and the rows of ``--slice-weights`` gain ``bias_rms``, the rms of a slice's log-field.

Also not in the reference (upstream added an ``assess`` command in later releases): ``assess`` scores every input stack for
motion (nesvor_amd/assess.py, csrc/assess.hip; ``ncc`` of adjacent slices, ``matrix-rank`` = effective rank of the stack's
data matrix, ``volume`` of the mask; higher is better) and ranks them; ``--template-stack`` on ``reconstruct``, ``register`` and
``svr`` names the stack that ``--registration stack`` / ``svr`` align the others to and centre the world frame on - an index
(default 0, the first file, as before) or ``auto`` = the best stack under ``--template-metric``.  The output slices keep the
input order.  With ``--registration none`` or ``--input-slices`` the two flags are ignored with a warning.

Also not in the reference: ``--packages P [P ...]`` and ``--package-rounds N`` (default 2) on ``svr``, ``register`` and
``reconstruct``: a stack acquired in P interleaved packages (package p holds slices p, p+P, p+2P, ...) gets a stage between one
pose per stack and one pose per slice - after the stack registration, N rounds of reconstruct a volume / register every package
rigidly to it (``GroupSVR``, nesvor_amd/registration.py; one count per input stack, or one for all).  Only with
``--registration svr``: with another choice, or with ``--input-slices``, the flags are ignored with a warning; a count that matches
neither 1 nor the number of stacks, or a ``P`` below 1, ends the command.  ``--debug`` logs every package's correction per round.

Also not in the reference: ``--svr-similarity ncc|nmi`` (default ``ncc``) and ``--nmi-bins B`` (default 32, 2 <= B <= 64) on
``svr``, ``register`` and ``reconstruct`` choose the metric ``--registration svr`` steers its package and slice stages on: the global
NCC of a slice and its simulation, or their normalised mutual information on a joint histogram of B bins per axis
(nesvor_amd/nmi.py, csrc/svr_nmi.hip) - for stacks of different contrast, of different coil bias, or with saturated slices, where
the linear intensity relation NCC assumes fails.  With another registration, or with ``--input-slices``, the flags are ignored
with a warning; a ``B`` outside [2, 64] ends the command.

Also not in the reference: ``--stack-similarity ncc|nmi`` (default ``ncc``) on ``svr``, ``register`` and ``reconstruct`` chooses the
metric of the stage in front of those: the stack registration of ``--registration stack``, which is also the first stage of
``--registration svr``.  ``nmi`` registers every stack to the template on the normalised mutual information of a joint histogram of
``--nmi-bins`` bins per axis over the template's points (the same definition, nesvor_amd/nmi.py; csrc/vvr_nmi.hip), so that
stacks of another contrast reach the slice stage from a stack pose NCC would have got wrong.  ``--nmi-bins`` serves both flags and
is checked when either asks for ``nmi``.  With ``--registration none`` or ``--input-slices`` the flag is ignored with a warning.

Also not in the reference: ``--per-stack-thickness`` on ``svr``, ``register`` and ``reconstruct`` (there for the registration stage
only) lets stacks of unequal slice thickness keep their own (``--thicknesses``, or the files' z spacing): ``--registration stack``
registers every stack on the template's slice spacing and spaces its slices by its own gap, and ``svr`` / ``--registration svr``
simulate every slice with the PSF of its own thickness (a PSF bank, nesvor_amd/psf_bank.py, looked up per slice inside one
launch of A and A^T); ``svr --input-slices`` then accepts a folder of mixed thickness (not of mixed pixel size).  Without the flag
the mean thickness serves all stacks, with a warning, as before; with it and equal thicknesses nothing changes either.

Also not in the reference (upstream added both in later releases, on SimpleITK's N4): ``correct-bias-field`` estimates the smooth
multiplicative coil bias of every input stack (nesvor_amd/bias.py, csrc/bias.hip: histogram sharpening and a multilevel
B-spline fit of the log field, this project's own definition) and writes the corrected stacks and, with
``--output-bias-fields``, the fields ``exp(f)``; ``--bias-field-correction`` on ``reconstruct``, ``register``, ``svr`` and
``assess`` applies the same correction to the stacks as they are loaded, before assessment, template choice and registration.
The ``--*-n4`` flags (levels, iterations, tolerance, control points, bins, FWHM, noise) are shared by the five commands.

Also not in the reference (upstream added the four switches in later releases; the definitions are nesvor_amd/masking.py's,
csrc/masking.hip): on the five commands that read stacks

    [--volume-mask FILE] [--stacks-intersection] [--background-threshold T] [--otsu-thresholding [--n-bins-otsu 256]]
    [--output-stack-masks FILE ...]

narrow every stack's mask as the stacks are loaded, before bias correction, assessment, template choice and registration, in
this order: intensity above ``T``; the world-space mask volume, interpolated at the voxel, at least 0.5; some slice of every
other stack contains the voxel (ignored with a warning beside ``--volume-mask`` and with one stack); intensity above Otsu's
threshold of the voxels kept so far.  ``--output-stack-masks`` writes the final masks, one file per stack.  A stack left without
a voxel ends the command; with ``--input-slices`` the flags are ignored with a warning.  ``--sample-mask FILE`` on ``reconstruct``
and ``sample-volume`` samples the model on that mask volume instead of the stored one.

Also not in the reference (SVRTK denoises every stack by default): on the five commands that read stacks

    [--denoise [--denoise-patch-radius 1] [--denoise-search-radius 3] [--denoise-strength 1.0] [--denoise-sigma X]]

denoises every stack as it is loaded, after the masking switches and before ``--bias-field-correction``: 2-D non-local means,
slice by slice (nesvor_amd/denoise.py, csrc/denoise.hip), with the noise level estimated per stack or given by ``--denoise-sigma``
in the intensities of the stacks as loaded; the log shows sigma and the rms of what was removed.  ``denoise`` writes the denoised
stacks and, with ``--output-json``, the per-stack report.  With ``--input-slices`` the flags are ignored with a warning.

Also not in the reference: ``evaluate`` compares volumes with a reference volume (nesvor_amd/evaluate.py, csrc/evaluate.hip): every
input volume is put onto the reference's lattice through the two files' poses (trilinear; ``svr`` writes a world-aligned lattice,
``reconstruct`` the model's own) and PSNR, NRMSE, MAE, correlation and the mean of a 3-D SSIM are taken over the voxels both
volumes cover, after the ``--intensity-fit`` of the volume to the reference.  Without ``--align`` the volumes must
share a world frame - the reconstructions of one set of registered slices, or of one ``--input-slices`` folder, do.
``--align translation|rigid``
(nesvor_amd/align.py) first finds the rigid correction of each input volume's pose that maximises its correlation with the
reference - a coarse-to-fine descent over ``--align-levels`` pyramid levels whose dozen candidate poses per step are one fused
pass over the reference - for a ground truth, another tool's output or a run with another ``--template-stack``; every report then
carries an ``alignment`` entry, and ``--output-aligned`` writes each input's own voxels with the corrected pose.  It logs
a table, ``--output-json`` writes the reports (a non-finite value as null), ``--output-ssim-maps`` / ``--output-resampled`` the maps
on the reference's lattice.  A volume that shares no voxel with the reference is reported with a warning.
``--device cpu``, which this command alone takes, runs the same definition as torch expressions on the host.
"""
import argparse
import logging
import os
import sys
import time
from argparse import Namespace
from typing import Dict, List, Optional

import torch


def _training_flags(p: argparse.ArgumentParser) -> None:
    g = p.add_argument_group("model architecture")
    g.add_argument("--n-features-per-level", default=2, type=int)
    g.add_argument("--log2-hashmap-size", default=19, type=int)
    g.add_argument("--level-scale", default=1.3819, type=float)
    g.add_argument("--coarsest-resolution", default=16.0, type=float)
    g.add_argument("--finest-resolution", default=0.5, type=float)
    g.add_argument("--n-levels-bias", default=0, type=int)
    g.add_argument("--depth", default=1, type=int)
    g.add_argument("--width", default=64, type=int)
    g.add_argument("--n-features-z", default=15, type=int)
    g.add_argument("--n-features-slice", default=16, type=int)
    g.add_argument("--no-transformation-optimization", action="store_true")
    g.add_argument("--no-slice-scale", action="store_true")
    g.add_argument("--no-pixel-variance", action="store_true")
    g.add_argument("--no-slice-variance", action="store_true")
    g.add_argument("--single-precision", action="store_true")
    g.add_argument("--fp16-loss-scaling", action="store_true",
                   help="(not a flag of the reference: it is the reference's DEFAULT behaviour) without --single-precision: fp16 MLP "
                        "operands and torch.cuda.amp.GradScaler semantics (init_scale 1, growth 2 every 2000 finite steps, backoff 0.5, "
                        "steps with non-finite gradients skipped) instead of this package's bf16 operands without loss scaling")
    g.add_argument("--mlp-fp16", action="store_true",
                   help="(not in the reference) power-of-two-scaled fp16 MLP matrix operands (one MFMA per product, no loss scaler "
                        "needed), fp32 accumulation / weights: with --single-precision for the fp32 model, without it for the "
                        "half-precision model structure (bias-free networks; excludes --fp16-loss-scaling and --mlp-bf16)")
    g.add_argument("--mlp-bf16", action="store_true",
                   help="(not in the reference) with --single-precision: bf16 MLP matrix operands, fp32 accumulation / weights")
    g.add_argument("--mlp-fp32-mfma", action="store_true",
                   help="(not in the reference) with --single-precision: evaluate the MLP products with fp32 MFMAs instead of the "
                        "default split-fp16 evaluation of the same fp32 products (same accuracy, slower)")
    g = p.add_argument_group("loss function")
    g.add_argument("--weight-transformation", default=0.1, type=float)
    g.add_argument("--weight-bias", default=100.0, type=float)
    g.add_argument("--image-regularization", default="edge", type=str, choices=["TV", "edge", "L2"])
    g.add_argument("--weight-image", default=2.0, type=float)
    g.add_argument("--delta", default=0.2, type=float)
    g = p.add_argument_group("training")
    g.add_argument("--learning-rate", default=5e-3, type=float)
    g.add_argument("--gamma", default=0.33, type=float)
    g.add_argument("--milestones", nargs="+", type=float, default=[0.5, 0.75, 0.9])
    g.add_argument("--n-iter", default=6000, type=int)
    g.add_argument("--batch-size", default=4096, type=int)
    g.add_argument("--n-samples", default=256, type=int)


def _output_volume_flags(g) -> None:
    g.add_argument("--output-resolution", default=0.8, type=float)
    g.add_argument("--output-intensity-mean", default=700.0, type=float)
    g.add_argument("--inference-batch-size", type=int)
    g.add_argument("--n-inference-samples", type=int)
    g.add_argument("--no-output-psf", action="store_true")


def _device_or_host(value: str):
    return "cpu" if value == "cpu" else int(value)


def _common_flags(p: argparse.ArgumentParser, host: bool = False) -> None:
    """``host``: the command has a host path of its own, ``--device cpu`` selects it."""
    g = p.add_argument_group("common")
    if host:
        g.add_argument("--device", default=None, type=_device_or_host,
                       help="HIP device index (default 0), or 'cpu': the same definition as torch expressions on the host")
    else:
        g.add_argument("--device", default=None, type=int, help="HIP device index (default 0; under a launcher: the rank's own device)")
    g.add_argument("--verbose", type=int, default=1, choices=[0, 1, 2])
    g.add_argument("--output-log", type=str)
    g.add_argument("--seed", type=int, default=None)
    g.add_argument("--debug", action="store_true")


def _template_flags(g) -> None:
    g.add_argument("--template-stack", default="0", type=str,
                   help="(not in the reference) the stack the registration aligns the others to and centres the world frame on: an "
                        "index among --input-stacks, or 'auto' = the best stack under --template-metric (nesvor_amd/assess.py)")
    g.add_argument("--template-metric", default="ncc", type=str, choices=["ncc", "matrix-rank", "volume"],
                   help="the score --template-stack auto ranks the stacks by")


def _bias_flags(p: argparse.ArgumentParser, switch: bool = True) -> None:
    g = p.add_argument_group("bias field correction (not in the reference; nesvor_amd/bias.py)")
    if switch:
        g.add_argument("--bias-field-correction", action="store_true",
                       help="remove the smooth multiplicative bias of every input stack as it is loaded (N4-style)")
    g.add_argument("--n-levels-n4", default=4, type=int, help="B-spline levels; level l has (n-control-points - 3) 2^l spans per axis")
    g.add_argument("--n-iter-n4", default=50, type=int, help="iterations per level at most")
    g.add_argument("--tol-n4", default=0.001, type=float, help="a level ends when the field's relative change falls below this")
    g.add_argument("--n-control-points-n4", default=4, type=int, help="control points per axis on the first level")
    g.add_argument("--n-bins-n4", default=200, type=int, help="histogram bins")
    g.add_argument("--fwhm-n4", default=0.15, type=float, help="FWHM of the Gaussian the histogram is deconvolved with (log intensity)")
    g.add_argument("--noise-n4", default=0.01, type=float, help="Wiener filter noise")


def _mask_flags(p: argparse.ArgumentParser) -> None:
    g = p.add_argument_group("stack masking (not in the reference; nesvor_amd/masking.py)")
    g.add_argument("--volume-mask", type=str,
                   help="a 3-D mask in world space: a stack voxel is kept where the mask, interpolated at its position, is >= 0.5")
    g.add_argument("--stacks-intersection", action="store_true",
                   help="keep a stack voxel only where every other stack has a slice that contains it (ignored with --volume-mask)")
    g.add_argument("--background-threshold", type=float, help="keep a stack voxel only where its intensity is above this")
    g.add_argument("--otsu-thresholding", action="store_true",
                   help="per stack, keep a voxel only where its intensity is above Otsu's threshold of the voxels kept so far")
    g.add_argument("--n-bins-otsu", default=256, type=int, help="histogram bins of --otsu-thresholding")
    g.add_argument("--output-stack-masks", nargs="+", type=str, help="write the final mask of every input stack, one file per stack")


def _denoise_flags(p: argparse.ArgumentParser, switch: bool = True) -> None:
    g = p.add_argument_group("stack denoising (not in the reference; nesvor_amd/denoise.py)")
    if switch:
        g.add_argument("--denoise", action="store_true",
                       help="denoise every input stack as it is loaded: 2-D non-local means, slice by slice, after the masking "
                            "switches and before --bias-field-correction")
    g.add_argument("--denoise-patch-radius", default=1, type=int, help="patches of (2 r + 1)^2 pixels are compared")
    g.add_argument("--denoise-search-radius", default=3, type=int, help="every pixel is compared with those at most this far away")
    g.add_argument("--denoise-strength", default=1.0, type=float, help="the filter parameter h in units of sigma: h = strength x sigma")
    g.add_argument("--denoise-sigma", type=float, metavar="X",
                   help="the noise standard deviation, in the intensities of the stacks as loaded, instead of the per-stack estimate")


def denoise_options(args: Namespace) -> Dict:
    """The keyword arguments of ``denoise.denoise_stacks`` from the ``--denoise-*`` flags (defaults where a Namespace lacks them)."""
    return {"patch_radius": getattr(args, "denoise_patch_radius", 1), "search_radius": getattr(args, "denoise_search_radius", 3),
            "strength": getattr(args, "denoise_strength", 1.0), "sigma": getattr(args, "denoise_sigma", None)}


def warn_denoise_ignored(args: Namespace, why: str) -> None:
    if getattr(args, "denoise", False):
        logging.warning("--denoise and the --denoise-* flags are ignored with %s: no stack is loaded", why)


MASK_FLAGS = ("volume_mask", "stacks_intersection", "background_threshold", "otsu_thresholding", "output_stack_masks")


def masking_requested(args: Namespace) -> bool:
    """One of the stack masking switches (or ``--output-stack-masks``) is set."""
    values = [getattr(args, name, None) for name in MASK_FLAGS]
    return any(v is not None and v is not False for v in values)  # (a threshold of 0.0 is a request)


def warn_masking_ignored(args: Namespace, why: str) -> None:
    if masking_requested(args):
        logging.warning("The stack masking flags (--volume-mask, --stacks-intersection, --background-threshold, --otsu-thresholding, "
                        "--output-stack-masks) are ignored with %s: no stack is loaded", why)


def bias_options(args: Namespace) -> Dict:
    """The keyword arguments of ``bias.correct_bias_field`` from the ``--*-n4`` flags (defaults where a Namespace lacks them)."""
    return {"n_levels": getattr(args, "n_levels_n4", 4), "n_iter": getattr(args, "n_iter_n4", 50), "tol": getattr(args, "tol_n4", 1e-3),
            "n_control_points": getattr(args, "n_control_points_n4", 4), "n_bins": getattr(args, "n_bins_n4", 200),
            "fwhm": getattr(args, "fwhm_n4", 0.15), "noise": getattr(args, "noise_n4", 0.01)}


def _thickness_flags(g) -> None:
    g.add_argument("--per-stack-thickness", action="store_true",
                   help="stacks of unequal slice thickness keep their own: the stack registration spaces every stack by its own gap, "
                        "and svr / --registration svr simulate every slice with the PSF of its own thickness (nesvor_amd/psf_bank.py); "
                        "without the flag the mean thickness is used for all stacks")


def _package_flags(g) -> None:
    g.add_argument("--packages", nargs="+", type=int, default=None, metavar="P",
                   help="(not in the reference) interleaved packages per stack, one count per input stack or one for all: with "
                        "--registration svr every package (slices p, p+P, p+2P, ...) is registered rigidly to the joint volume "
                        "between the stack registration and the slice rounds (nesvor_amd/registration.py: GroupSVR)")
    g.add_argument("--package-rounds", type=int, default=2, metavar="N", help="reconstruct / register-packages rounds of --packages")
    g.add_argument("--svr-similarity", choices=["ncc", "nmi"], default="ncc",
                   help="(not in the reference) the metric of --registration svr's package and slice stages: global NCC, or normalised "
                        "mutual information on a joint histogram (nesvor_amd/nmi.py) for stacks whose intensities are not linearly related")
    g.add_argument("--nmi-bins", type=int, default=32, metavar="B",
                   help="bins per axis of --svr-similarity nmi and --stack-similarity nmi, 2 <= B <= 64")
    g.add_argument("--stack-similarity", choices=["ncc", "nmi"], default="ncc",
                   help="(not in the reference) the metric of --registration stack and of the stack stage of --registration svr: global "
                        "NCC, or normalised mutual information on a joint histogram (nesvor_amd/nmi.py, csrc/vvr_nmi.hip)")


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(prog="nesvor_amd.cli", description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = parser.add_subparsers(dest="command", required=True)

    p = sub.add_parser("reconstruct")
    g = p.add_argument_group("input")
    g.add_argument("--input-stacks", nargs="+", type=str)
    g.add_argument("--thicknesses", nargs="+", type=float)
    g.add_argument("--stack-masks", nargs="+", type=str)
    g.add_argument("--input-slices", type=str)
    g = p.add_argument_group("output")
    g.add_argument("--output-volume", type=str)
    _output_volume_flags(g)
    g.add_argument("--output-slices", type=str)
    g.add_argument("--simulated-slices", type=str)
    g.add_argument("--output-model", type=str)
    g.add_argument("--mask-threshold", type=float, default=1.0)
    g.add_argument("--sample-mask", type=str, help="a 3-D mask the output volume is sampled on, instead of the mask of the slices")
    g = p.add_argument_group("registration")
    g.add_argument("--registration", default="none", type=str, choices=["svort", "svort-stack", "stack", "svr", "none"])
    g.add_argument("--svort-version", default="v1", type=str, choices=["v1", "v2"])
    _template_flags(g)
    _thickness_flags(g)
    _package_flags(g)
    _training_flags(p)
    _bias_flags(p)
    _mask_flags(p)
    _denoise_flags(p)
    _common_flags(p)

    p = sub.add_parser("register")
    g = p.add_argument_group("input")
    g.add_argument("--input-stacks", nargs="+", type=str, required=True)
    g.add_argument("--thicknesses", nargs="+", type=float)
    g.add_argument("--stack-masks", nargs="+", type=str)
    g = p.add_argument_group("output")
    g.add_argument("--output-slices", type=str, required=True)
    g = p.add_argument_group("registration")
    g.add_argument("--registration", default="stack", type=str, choices=["svort", "svort-stack", "stack", "svr", "none"])
    g.add_argument("--svort-version", default="v1", type=str, choices=["v1", "v2"])
    _template_flags(g)
    _thickness_flags(g)
    _package_flags(g)
    _bias_flags(p)
    _mask_flags(p)
    _denoise_flags(p)
    _common_flags(p)

    p = sub.add_parser("svr")
    g = p.add_argument_group("input")
    g.add_argument("--input-stacks", nargs="+", type=str)
    g.add_argument("--thicknesses", nargs="+", type=float)
    g.add_argument("--stack-masks", nargs="+", type=str)
    g.add_argument("--input-slices", type=str)
    g = p.add_argument_group("output")
    g.add_argument("--output-volume", type=str, required=True)
    g.add_argument("--output-resolution", default=0.8, type=float)
    g.add_argument("--output-intensity-mean", default=700.0, type=float)
    g.add_argument("--output-slices", type=str)
    g.add_argument("--simulated-slices", type=str)
    g = p.add_argument_group("registration")
    g.add_argument("--registration", default="svr", type=str, choices=["svort", "svort-stack", "stack", "svr", "none"])
    g.add_argument("--svort-version", default="v1", type=str, choices=["v1", "v2"])
    _template_flags(g)
    _thickness_flags(g)
    _package_flags(g)
    g = p.add_argument_group("super-resolution reconstruction")
    g.add_argument("--n-iter-srr", default=30, type=int, help="descent steps")
    g.add_argument("--srr-beta", default=0.02, type=float, help="weight of the edge-preserving prior")
    g.add_argument("--srr-delta", default=0.1, type=float, help="edge scale of the prior, in normalised intensities")
    g.add_argument("--outlier-rejection", action="store_true",
                   help="robust statistics: EM pixel and slice weights and per-slice intensity scales (nesvor_amd/robust.py)")
    g.add_argument("--robust-rounds", default=3, type=int,
                   help="rounds the descent steps are split into (with --outlier-rejection, --structural-exclusion and / or "
                        "--slice-bias-fields)")
    g.add_argument("--slice-weights", type=str,
                   help="JSON file with one row per slice: the final weight and scale (with --outlier-rejection), ncc, pixel_share "
                        "and excluded (with --structural-exclusion)")
    g.add_argument("--structural-exclusion", action="store_true",
                   help="drop slices that do not correlate with their simulation and pixels of low local SSIM (nesvor_amd/structural.py)")
    g.add_argument("--local-ssim-threshold", default=0.4, type=float, help="a pixel is kept where its local SSIM is at least this")
    g.add_argument("--global-ncc-threshold", default=0.5, type=float,
                   help="a slice is kept where its correlation with its simulation is at least this")
    g.add_argument("--slice-bias-fields", action="store_true",
                   help="estimate a smooth multiplicative bias field per slice against its simulation (nesvor_amd/slice_bias.py)")
    g.add_argument("--bias-sigma", default=12.0, type=float, metavar="MM",
                   help="standard deviation of the Gaussian window of --slice-bias-fields, in mm")
    g.add_argument("--output-corrected-slices", type=str, metavar="DIR",
                   help="folder for the slices divided by their fields (with --slice-bias-fields)")
    _bias_flags(p)
    _mask_flags(p)
    _denoise_flags(p)
    _common_flags(p)

    p = sub.add_parser("assess")
    g = p.add_argument_group("input")
    g.add_argument("--input-stacks", nargs="+", type=str, required=True)
    g.add_argument("--thicknesses", nargs="+", type=float)
    g.add_argument("--stack-masks", nargs="+", type=str)
    g = p.add_argument_group("assessment")
    g.add_argument("--metric", default="ncc", type=str, choices=["ncc", "matrix-rank", "volume"],
                   help="per-stack score, higher is better (nesvor_amd/assess.py)")
    g.add_argument("--output-json", type=str, help="JSON file for the list of per-stack results")
    _bias_flags(p)
    _mask_flags(p)
    _denoise_flags(p)
    _common_flags(p)

    p = sub.add_parser("correct-bias-field")
    g = p.add_argument_group("input")
    g.add_argument("--input-stacks", nargs="+", type=str, required=True)
    g.add_argument("--stack-masks", nargs="+", type=str)
    g = p.add_argument_group("output")
    g.add_argument("--output-corrected-stacks", nargs="+", type=str, required=True)
    g.add_argument("--output-bias-fields", nargs="+", type=str, help="the estimated fields exp(f), one file per input stack")
    _bias_flags(p, switch=False)
    _mask_flags(p)
    _denoise_flags(p)
    _common_flags(p)

    p = sub.add_parser("denoise")
    g = p.add_argument_group("input")
    g.add_argument("--input-stacks", nargs="+", type=str, required=True)
    g.add_argument("--stack-masks", nargs="+", type=str)
    g = p.add_argument_group("output")
    g.add_argument("--output-stacks", nargs="+", type=str, required=True, help="the denoised stacks, one file per input stack")
    g.add_argument("--output-json", type=str, help="JSON file for the list of per-stack reports (sigma, method noise)")
    _denoise_flags(p, switch=False)
    _common_flags(p)

    p = sub.add_parser("evaluate")
    g = p.add_argument_group("input (without --align the volumes must share a world frame: nothing is aligned)")
    g.add_argument("--reference-volume", type=str, required=True, help="the volume the others are compared with, on its lattice")
    g.add_argument("--reference-mask", type=str, help="a mask on the reference's lattice instead of its positive voxels")
    g.add_argument("--input-volumes", nargs="+", type=str, required=True,
                   help="the volumes under test, on any lattice of the reference's world frame (the reconstructions of one set of "
                        "registered slices, or of one --input-slices folder, share it), or any rigid motion away from it with --align")
    g.add_argument("--input-masks", nargs="+", type=str, help="one mask per input volume instead of its positive voxels")
    g = p.add_argument_group("comparison (nesvor_amd/evaluate.py)")
    g.add_argument("--intensity-fit", default="scale", type=str, choices=["none", "scale", "affine"],
                   help="fitted to the reference before the errors are taken: nothing, a gain, or a gain and an offset")
    g.add_argument("--dynamic-range", type=float, metavar="L", help="the peak value of PSNR, NRMSE and SSIM (default: the reference's "
                                                                    "largest intensity on the compared voxels)")
    g.add_argument("--align", default="none", type=str, choices=["none", "translation", "rigid"],
                   help="before the comparison, correct each input volume's pose by the translation or rigid motion that maximises its "
                        "correlation with the reference (nesvor_amd/align.py); none: the files' poses are taken as they are")
    g.add_argument("--align-levels", default=3, type=int, metavar="N",
                   help="with --align: at most N pyramid levels (a level needs 12 samples on every axis of both volumes)")
    g = p.add_argument_group("output")
    g.add_argument("--output-json", type=str, help="JSON file for the list of per-volume reports")
    g.add_argument("--output-ssim-maps", nargs="+", type=str, help="the SSIM map of every input volume, on the reference's lattice")
    g.add_argument("--output-resampled", nargs="+", type=str, help="every input volume on the reference's lattice")
    g.add_argument("--output-aligned", nargs="+", type=str,
                   help="with --align: every input volume's own voxels with the corrected pose (nothing is resampled); `evaluate` "
                        "without --align reproduces the aligned comparison from such a file")
    _common_flags(p, host=True)

    p = sub.add_parser("sample-volume")
    p.add_argument("--input-model", type=str, required=True)
    g = p.add_argument_group("output")
    g.add_argument("--output-volume", type=str, required=True)
    _output_volume_flags(g)
    g.add_argument("--mask-threshold", type=float, default=1.0)
    g.add_argument("--sample-mask", type=str, help="a 3-D mask the volume is sampled on, instead of the mask stored with the model")
    _common_flags(p)

    p = sub.add_parser("sample-slices")
    p.add_argument("--input-model", type=str, required=True)
    p.add_argument("--input-slices", type=str, required=True)
    g = p.add_argument_group("output")
    g.add_argument("--simulated-slices", type=str, required=True)
    g.add_argument("--mask-threshold", type=float, default=1.0)
    _common_flags(p)
    return parser


def merge_args(args_old: Namespace, args_new: Namespace) -> Namespace:
    """Stored (checkpoint) arguments overridden by the command line (utils/misc.py:22-26)."""
    d = dict(vars(args_old))
    d.update(vars(args_new))
    return Namespace(**d)


def stacks_to_slices(stacks) -> List:
    """``--registration none``: every non-empty slice of every stack at its nominal pose, each stack normalised by
    the 0.99 quantile of its masked intensities (svort/inference.py:553-560).  Every slice carries the index of its stack in
    ``stacks`` and its own index inside that stack (``stack_idx``, ``slice_idx``)."""
    slices = []
    for j, stack in enumerate(stacks):
        nonempty = stack.mask.flatten(1).any(1)
        stack.slices /= torch.quantile(stack.slices[stack.mask], 0.99)
        kept = stack[nonempty]
        for s, k in zip(kept, torch.nonzero(nonempty).flatten().tolist()):
            s.stack_idx, s.slice_idx = j, k
        slices.extend(kept)
    return slices


def _setup(args: Namespace) -> None:
    level = {0: logging.WARNING, 1: logging.INFO, 2: logging.DEBUG}[args.verbose]
    handlers = [logging.StreamHandler(sys.stderr)]
    launched = _under_launcher() and args.command == "reconstruct"
    if args.output_log and not (launched and int(os.environ.get("RANK", "0")) > 0):  # (data parallel: ONE writer of the log file, rank 0)
        handlers.append(logging.FileHandler(args.output_log, mode="w"))
    logging.basicConfig(level=level, format="%(asctime)s %(levelname)s %(message)s", handlers=handlers, force=True)
    args.rank, args.distributed = 0, False
    if launched:
        # data parallel, one process per GPU (torchrun's environment, or NESVOR_DDP_FORCE=1: a group of one rank)
        import torch.distributed as dist

        from . import ddp

        args.distributed = not dist.is_initialized()  # (a group the caller made is the caller's to destroy)
        args.rank, local_rank, _ = ddp.init_distributed()
        if args.device is not None:
            logging.warning("--device %d ignored under a launcher: rank %d runs on its own device", args.device, args.rank)
        args.device = ddp.local_device(local_rank)
        torch.cuda.set_device(args.device)
        # every rank starts from the SAME seed (train() derives the per-rank PSF-noise seed from it): without --seed, rank 0's draw
        # (torch.seed() is an unsigned 64-bit value: its low 63 bits travel as an int64)
        seed = args.seed if args.seed is not None else (torch.seed() & (2**63 - 1) if args.rank == 0 else 0)
        seed = torch.tensor([seed], dtype=torch.int64, device=args.device if dist.get_backend() == "nccl" else "cpu")
        dist.broadcast(seed, src=0)
        torch.manual_seed(int(seed.item()))
        return
    if args.seed is not None:
        torch.manual_seed(args.seed)
    if args.device == "cpu":  # (`evaluate` alone offers it)
        args.device = torch.device("cpu")
        return
    args.device = torch.device("cuda", args.device or 0)
    torch.cuda.set_device(args.device)


def _under_launcher() -> bool:
    """torchrun's environment (WORLD_SIZE > 1), or a forced group of one rank (NESVOR_DDP_FORCE=1)."""
    from . import ddp

    return int(os.environ.get("WORLD_SIZE", "1")) > 1 or ddp.forced()


def _load_model(args: Namespace):
    from .image_io import load_model

    inr, mask, stored = load_model(args.input_model, args.device)
    return inr, mask, merge_args(stored, args)


def _outputs(data: Dict, args: Namespace) -> None:
    """cli/io.py:33-50"""
    from .image_io import save_model, save_slices

    if getattr(args, "output_volume", None) and "output_volume" in data:
        if args.output_intensity_mean:
            data["output_volume"].rescale(args.output_intensity_mean)
        data["output_volume"].save(args.output_volume)
    if getattr(args, "output_model", None) and "output_model" in data:
        save_model(args.output_model, data["output_model"], data["mask"], args)
    for key in ("output_slices", "simulated_slices", "output_corrected_slices"):
        if getattr(args, key, None) and key in data:
            os.makedirs(getattr(args, key), exist_ok=True)
            save_slices(getattr(args, key), data[key])


def _load_stacks(args: Namespace) -> List:
    from .image_io import load_stack

    for name in ("stack_masks", "thicknesses"):
        if getattr(args, name, None) is not None and len(getattr(args, name)) != len(args.input_stacks):
            raise SystemExit(f"The numbers of {name.replace('_', ' ')} and input stacks are different!")
    stacks = []
    for i, f in enumerate(args.input_stacks):
        st = load_stack(f, args.stack_masks[i] if args.stack_masks is not None else None, device=args.device)
        if args.thicknesses is not None:
            st.thickness = args.thicknesses[i]
        stacks.append(st)
    if masking_requested(args):
        _mask_stacks(args, stacks)
    if getattr(args, "denoise", False):
        _denoise_stacks(args, stacks)
    if getattr(args, "bias_field_correction", False):
        from . import bias

        t0 = time.time()
        bias.correct_stacks(stacks, **bias_options(args))
        logging.info("Bias field correction of %d stacks finished in %.1f s", len(stacks), time.time() - t0)
    return stacks


def _mask_stacks(args: Namespace, stacks: List) -> None:
    """The stack masking switches on the loaded stacks (nesvor_amd/masking.py), and ``--output-stack-masks``."""
    from . import masking
    from .image_io import load_volume, save_stack

    out = getattr(args, "output_stack_masks", None)
    if out is not None and len(out) != len(args.input_stacks):
        raise SystemExit("The numbers of output stack masks and input stacks are different!")
    t0 = time.time()
    volume = load_volume(args.volume_mask, device=args.device) if getattr(args, "volume_mask", None) else None
    masking.mask_stacks(stacks, volume_mask=volume, stacks_intersection=bool(getattr(args, "stacks_intersection", False)),
                        background_threshold=getattr(args, "background_threshold", None),
                        otsu_thresholding=bool(getattr(args, "otsu_thresholding", False)), n_bins_otsu=getattr(args, "n_bins_otsu", 256),
                        names=[f"stack {i} ({f})" for i, f in enumerate(args.input_stacks)])
    logging.info("Stack masking of %d stacks finished in %.1f s", len(stacks), time.time() - t0)
    if out is not None:
        for path, st in zip(out, stacks):
            save_stack(path, st, st.mask.to(st.slices.dtype))


def _denoise_stacks(args: Namespace, stacks: List) -> List[Dict]:
    """``--denoise`` on the loaded stacks (nesvor_amd/denoise.py); returns the per-stack reports as host numbers."""
    from . import denoise

    t0 = time.time()
    reports = denoise.denoise_stacks(stacks, names=[f"stack {i} ({f})" for i, f in enumerate(args.input_stacks)], **denoise_options(args))
    rows = [denoise.report_row(r) for r in reports]  # (reads the sums: the device has finished when the time is taken)
    logging.info("Denoising of %d stacks finished in %.1f s", len(stacks), time.time() - t0)
    return rows


def _sample_mask(args: Namespace, mask):
    """``--sample-mask``: the mask volume of a file instead of ``mask``."""
    if not getattr(args, "sample_mask", None):
        return mask
    from .image_io import load_volume

    return load_volume(args.sample_mask, device=args.device)


def register(args: Namespace, stacks: List) -> List:
    """Stacks -> motion-corrected slices (cli/commands.py:171-176): ``none`` keeps the nominal poses, ``stack``
    registers every stack to the template (``--template-stack``: the first one by default, ``auto`` = the best stack under
    ``--template-metric``, nesvor_amd/assess.py), ``svr`` then registers every slice to a volume reconstructed from all of
    them (``register_slices``); the SVoRT-based choices need the pretrained transformer (out of scope)."""
    if args.registration not in ("none", "stack", "svr"):
        raise NotImplementedError(f"--registration {args.registration}: the SVoRT transformer is out of scope of this "
                                  "build; register with the reference and pass the result through --input-slices, or use "
                                  "--registration svr / stack / none")
    packages = package_options(args, len(stacks))  # (a bad count ends the command before any registration)
    similarity = similarity_options(args)
    if args.registration == "none":
        warn_template_ignored(args, "--registration none")
        return stacks_to_slices(stacks)
    from .assess import choose_template

    # the template only names the registration's target: the stacks, and stack_idx / slice_idx of the slices, stay in input order
    template = choose_template(stacks, getattr(args, "template_stack", "0"), getattr(args, "template_metric", "ncc"))
    per_stack = bool(getattr(args, "per_stack_thickness", False))
    if args.registration == "stack":
        from .registration import register_stacks

        t1 = time.time()
        stacks = register_stacks(stacks, template=template, per_stack_thickness=per_stack, **similarity)
        logging.info("Stack registration finished in %.1f s", time.time() - t1)
    elif args.registration == "svr":
        from .registration import register_slices

        t1 = time.time()
        if packages is None:
            stacks = register_slices(stacks, template=template, per_stack_thickness=per_stack, **similarity)
        else:
            stacks = register_slices(stacks, template=template, per_stack_thickness=per_stack, packages=packages,
                                     package_rounds=int(getattr(args, "package_rounds", 2)), **similarity)
        logging.info("Slice-to-volume registration finished in %.1f s", time.time() - t1)
    return stacks_to_slices(stacks)


def warn_template_ignored(args: Namespace, why: str) -> None:
    """``--template-stack`` / ``--template-metric`` only act where stacks are registered."""
    if str(getattr(args, "template_stack", "0")) != "0" or getattr(args, "template_metric", "ncc") != "ncc":
        logging.warning("--template-stack / --template-metric are ignored with %s: no stack is registered to a template", why)


def warn_packages_ignored(args: Namespace, why: str) -> None:
    """``--packages`` / ``--package-rounds`` only act in the package stage of ``--registration svr``."""
    if getattr(args, "packages", None) is not None or getattr(args, "package_rounds", 2) != 2:
        logging.warning("--packages / --package-rounds are ignored with %s: packages are registered by --registration svr only", why)


def warn_similarity_ignored(args: Namespace, why: str) -> None:
    """``--svr-similarity`` / ``--nmi-bins`` only act in the package and slice stages of ``--registration svr``, ``--stack-similarity``
    where stacks are registered."""
    if getattr(args, "svr_similarity", "ncc") != "ncc" or getattr(args, "nmi_bins", 32) != 32:
        logging.warning("--svr-similarity / --nmi-bins are ignored with %s: the metric is that of --registration svr only", why)
    if getattr(args, "stack_similarity", "ncc") != "ncc":
        logging.warning("--stack-similarity is ignored with %s: no stack is registered", why)


def _nmi_bins(args: Namespace) -> int:
    bins = getattr(args, "nmi_bins", 32)
    if not 2 <= int(bins) <= 64:
        raise SystemExit(f"--nmi-bins: a number of bins in [2, 64] expected, got {bins}")
    return int(bins)


def similarity_options(args: Namespace) -> Dict:
    """``--svr-similarity`` / ``--stack-similarity`` / ``--nmi-bins`` as keyword arguments of the registration the command runs (none
    for the defaults, NCC): of ``register_slices`` with ``--registration svr`` (``similarity``, ``stack_similarity``, ``nmi_bins``), of
    ``register_stacks`` with ``--registration stack --stack-similarity nmi`` (``similarity``, ``nmi_bins``).  Flags that do not act
    are ignored with a warning; ``--nmi-bins`` outside [2, 64] ends the command."""
    registration = getattr(args, "registration", "none")
    stack_nmi = getattr(args, "stack_similarity", "ncc") == "nmi"
    if registration == "stack" and stack_nmi:
        if getattr(args, "svr_similarity", "ncc") != "ncc":
            logging.warning("--svr-similarity is ignored with --registration stack: it is the metric of --registration svr's package "
                            "and slice stages")
        return {"similarity": "nmi", "nmi_bins": _nmi_bins(args)}
    if registration != "svr":
        warn_similarity_ignored(args, f"--registration {registration}")  # (stack: --stack-similarity is at its default here)
        return {}
    bins = _nmi_bins(args)
    out: Dict = {}
    if getattr(args, "svr_similarity", "ncc") == "nmi":
        out["similarity"] = "nmi"
    if stack_nmi:
        out["stack_similarity"] = "nmi"
    if out:
        out["nmi_bins"] = bins
    return out


def package_options(args: Namespace, n_stacks: int) -> Optional[List[int]]:
    """``--packages`` as one count per stack, or None (no package stage).  With a registration other than ``svr`` the flags are
    ignored with a warning; a count that matches neither 1 nor the number of stacks, a ``P < 1`` or ``--package-rounds`` below 0
    ends the command."""
    if getattr(args, "registration", "none") != "svr":
        warn_packages_ignored(args, f"--registration {getattr(args, 'registration', 'none')}")
        return None
    if int(getattr(args, "package_rounds", 2)) < 0:
        raise SystemExit(f"--package-rounds: a number of rounds >= 0 expected, got {args.package_rounds}")
    packages = getattr(args, "packages", None)
    if packages is None:
        return None
    if len(packages) not in (1, n_stacks):
        raise SystemExit(f"--packages: one count per input stack ({n_stacks}) or one for all expected, got {len(packages)}")
    if min(packages) < 1:
        raise SystemExit(f"--packages: every stack has at least 1 package, got {min(packages)}")
    return [int(p) for p in packages] * (n_stacks if len(packages) == 1 else 1)


def register_cmd(args: Namespace) -> None:
    _outputs({"output_slices": register(args, _load_stacks(args))}, args)


def assess_cmd(args: Namespace) -> None:
    import json

    from .assess import assess_stacks, format_table

    rows = assess_stacks(_load_stacks(args), args.metric)
    logging.info("Stack assessment (%s, higher is better):\n%s", args.metric, format_table(rows))
    for row, path in zip(rows, args.input_stacks):
        row["input_stack"] = path
    if args.output_json:
        with open(args.output_json, "w") as f:  # (a score of nan - no countable pair - is written as null)
            json.dump([{k: None if isinstance(v, float) and v != v else v for k, v in row.items()} for row in rows], f, indent=1)


def correct_bias_field_cmd(args: Namespace) -> None:
    from . import bias
    from .image_io import save_stack

    for name in ("output_corrected_stacks", "output_bias_fields", "stack_masks"):
        if getattr(args, name, None) is not None and len(getattr(args, name)) != len(args.input_stacks):
            raise SystemExit(f"The numbers of {name.replace('_', ' ')} and input stacks are different!")
    args.thicknesses = None
    args.bias_field_correction = False  # (the stacks are corrected below, where the fields are at hand)
    stacks = _load_stacks(args)
    fields = bias.correct_stacks(stacks, **bias_options(args))
    for i, (st, field) in enumerate(zip(stacks, fields)):
        save_stack(args.output_corrected_stacks[i], st)
        if args.output_bias_fields is not None:
            save_stack(args.output_bias_fields[i], st, torch.exp(field).to(st.slices.dtype))


def denoise_cmd(args: Namespace) -> None:
    import json

    from .image_io import save_stack

    for name in ("output_stacks", "stack_masks"):
        if getattr(args, name, None) is not None and len(getattr(args, name)) != len(args.input_stacks):
            raise SystemExit(f"The numbers of {name.replace('_', ' ')} and input stacks are different!")
    args.thicknesses = None
    args.denoise = False  # (the stacks are denoised below, where the reports are at hand)
    stacks = _load_stacks(args)
    rows = _denoise_stacks(args, stacks)
    for path, st, row, source in zip(args.output_stacks, stacks, rows, args.input_stacks):
        save_stack(path, st)
        row["input_stack"], row["output_stack"] = source, path
    if args.output_json:
        with open(args.output_json, "w") as f:
            json.dump(rows, f, indent=1)


def evaluate_cmd(args: Namespace) -> None:
    from .evaluate import evaluate_command

    evaluate_command(args)


def reconstruct(args: Namespace) -> None:
    from .image_io import load_slices, load_stack
    from .sample import sample_slices, sample_volume
    from .train import train

    if args.input_slices is None and args.input_stacks is None:
        raise SystemExit("No image data provided! Use --input-slices or --input-stacks to input data.")
    if args.input_slices is not None and (args.input_stacks or args.stack_masks or args.thicknesses):
        logging.warning("Since <input-slices> is provided, <input-stacks>, <stack_masks> and <thicknesses> would be ignored.")
        args.input_stacks = args.stack_masks = args.thicknesses = None
    if args.input_slices is not None:
        warn_template_ignored(args, "--input-slices")
        warn_packages_ignored(args, "--input-slices")
        warn_similarity_ignored(args, "--input-slices")
        warn_masking_ignored(args, "--input-slices")
        warn_denoise_ignored(args, "--input-slices")
    for name in ("stack_masks", "thicknesses"):
        if getattr(args, name) is not None and len(getattr(args, name)) != len(args.input_stacks):
            raise SystemExit(f"The numbers of {name.replace('_', ' ')} and input stacks are different!")
    if args.output_volume is None and args.output_model is None:
        logging.warning("Both <output-volume> and <output-model> are not provided.")
    if not args.inference_batch_size:
        args.inference_batch_size = 8 * args.batch_size
    if not args.n_inference_samples:
        args.n_inference_samples = 2 * args.n_samples
    args.dtype = torch.float32 if args.single_precision else torch.float16
    if args.mlp_bf16 and not args.single_precision:
        raise SystemExit("--mlp-bf16 is a variant of the fp32 model: pass --single-precision too")
    if getattr(args, "mlp_fp16", False) and getattr(args, "fp16_loss_scaling", False):
        raise SystemExit("--mlp-fp16 needs no loss scaler: drop --fp16-loss-scaling")
    if getattr(args, "fp16_loss_scaling", False) and args.single_precision:
        raise SystemExit("--fp16-loss-scaling is the reference's DEFAULT numerics (fp16 operands + GradScaler): drop --single-precision")
    if not args.single_precision:
        logging.info("half-precision model structure (bias-free networks): %s matrix operands, fp32 accumulation",
                     "power-of-two-scaled fp16 (no loss scaler)" if getattr(args, "mlp_fp16", False) else
                     "fp16 (with the reference's loss scaler: init 1, growth 2 / 2000 steps, backoff 0.5)" if getattr(args, "fp16_loss_scaling", False) else "bf16")
    t0 = time.time()
    if args.input_slices is not None:
        slices = load_slices(args.input_slices, args.device)
    else:
        slices = register(args, _load_stacks(args))
    logging.info("Data loading finished in %.1f s (%d slices)", time.time() - t0, len(slices))
    t0 = time.time()
    model, output_slices, mask = train(slices, args)
    logging.info("Reconstruction finished in %.1f s", time.time() - t0)
    t0 = time.time()
    try:
        if getattr(args, "rank", 0) == 0:  # (data parallel: the replicas are identical; the other ranks wait below)
            data = {"mask": mask, "output_model": model, "output_slices": output_slices}
            if args.output_volume:
                data["output_volume"] = sample_volume(model, _sample_mask(args, mask), args)
            if args.simulated_slices:
                data["simulated_slices"] = sample_slices(model, output_slices, mask, args)
            _outputs(data, args)
            logging.info("Results saving finished in %.1f s", time.time() - t0)
    finally:
        if getattr(args, "distributed", False):  # (set by _setup when it made the group; also when rank 0 failed above: the others must leave)
            import torch.distributed as dist

            dist.barrier()
            dist.destroy_process_group()


def svr_cmd(args: Namespace) -> None:
    from .svr import svr_command

    _outputs(svr_command(args), args)


def sample_volume_cmd(args: Namespace) -> None:
    from .sample import sample_volume

    model, mask, args = _load_model(args)
    if not getattr(args, "inference_batch_size", None):
        args.inference_batch_size = 8 * args.batch_size
    if not getattr(args, "n_inference_samples", None):
        args.n_inference_samples = 2 * args.n_samples
    _outputs({"output_volume": sample_volume(model, _sample_mask(args, mask), args)}, args)


def sample_slices_cmd(args: Namespace) -> None:
    from .image_io import load_slices
    from .sample import sample_slices

    model, mask, args = _load_model(args)
    slices = load_slices(args.input_slices, args.device)
    _outputs({"simulated_slices": sample_slices(model, slices, mask, args)}, args)


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    if args.command != "reconstruct" and int(os.environ.get("RANK", "0")) > 0:
        return  # under a launcher only `reconstruct` is data-parallel: one process does the rest
    _setup(args)
    t0 = time.time()
    {"reconstruct": reconstruct, "register": register_cmd, "svr": svr_cmd, "assess": assess_cmd,
     "correct-bias-field": correct_bias_field_cmd, "denoise": denoise_cmd, "evaluate": evaluate_cmd, "sample-volume": sample_volume_cmd,
     "sample-slices": sample_slices_cmd}[args.command](args)
    logging.info("Command 'nesvor %s' finished, overall time: %.1f s", args.command, time.time() - t0)


if __name__ == "__main__":
    main()
