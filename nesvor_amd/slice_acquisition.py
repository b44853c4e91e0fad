"""Differentiable slice acquisition A and its adjoint A^T: the functions of ``nesvor.slice_acquisition``
(slice_acquisition/slice_acq.py:22-211) on the dispatcher ops ``torch.ops.nesvor.slice_acq_forward`` /
``slice_acq_adjoint_forward``, whose autograd formulas (``nesvor_amd.ops``) call the matching backward ops.
float32 / float64, both interpolation modes.
"""
import os

import torch

from . import ops as _ops  # noqa: F401  (registers torch.ops.nesvor)


def _or_empty(mask, like):
    return mask if mask is not None else torch.empty(0, device=like.device)


def slice_acquisition(transforms, vol, vol_mask, slices_mask, psf, slice_shape, res_slice, need_weight, interp_psf):
    """(n,3,4) poses in voxel units, (1,1,D,H,W) volume, (d,h,w) PSF -> slices (n,1,h,w) [, PSF weight per pixel]."""
    out = torch.ops.nesvor.slice_acq_forward(
        transforms.contiguous(), vol.contiguous(), _or_empty(vol_mask, vol), _or_empty(slices_mask, vol), psf.contiguous(),
        [int(s) for s in slice_shape], float(res_slice), bool(need_weight), bool(interp_psf))
    return (out[0], out[1]) if need_weight else out[0]


def slice_acquisition_adjoint(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf, equalize):
    """Back-projection of slices into a (1,1,D,H,W) volume; ``equalize`` divides by the back-projected PSF weight."""
    vol, _ = torch.ops.nesvor.slice_acq_adjoint_forward(
        transforms.contiguous(), psf.contiguous(), slices.contiguous(), _or_empty(slices_mask, slices), _or_empty(vol_mask, slices),
        [int(s) for s in vol_shape], float(res_slice), bool(interp_psf), bool(equalize))
    return vol


# ---------------------------------------------------------------------------------------------------------------------
# per-slice PSFs: A and A^T with a ``PsfBank`` (nesvor_amd/psf_bank.py).  fp32, linear mode, no autograd.
# ---------------------------------------------------------------------------------------------------------------------
def bank_fused() -> bool:
    """NESVOR_PSF_BANK=composed forces the composed expression: one one-PSF launch per member."""
    return os.environ.get("NESVOR_PSF_BANK", "") != "composed"


def _no_gradient(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f"{what}: no gradient flows through a PSF bank (the backward kernels take one PSF); detach the inputs")


def _bank_checks(what, bank, n, interp_psf):
    if interp_psf:
        raise NotImplementedError(f"{what}: a PSF bank has no interp_psf mode")
    if len(bank) != n:
        raise ValueError(f"{what}: the bank holds ids for {len(bank)} slices, the stack has {n}")


def slice_acquisition_bank(transforms, vol, vol_mask, slices_mask, bank, slice_shape, res_slice, need_weight, interp_psf=False):
    """``slice_acquisition`` with slice k blurred by ``bank.psfs[bank.host_ids[k]]``: one launch for all members."""
    _no_gradient("slice_acquisition_bank", transforms, vol)
    n = transforms.shape[0]
    _bank_checks("slice_acquisition_bank", bank, n, interp_psf)
    transforms = transforms.contiguous()
    if bank_fused():
        out = torch.ops.nesvor.slice_acq_forward_bank(
            transforms, vol.contiguous(), _or_empty(vol_mask, vol), _or_empty(slices_mask, vol), bank.flat, bank.table, bank.ids,
            [int(s) for s in slice_shape], float(res_slice), bool(need_weight))
        return (out[0], out[1]) if need_weight else out[0]
    # composed: one existing forward per member on that member's slices, written into their rows
    h, w = int(slice_shape[0]), int(slice_shape[1])
    slices = torch.zeros((n, 1, h, w), dtype=vol.dtype, device=vol.device)
    weight = torch.zeros_like(slices) if need_weight else None
    for _, psf, idx in bank.members():
        sm = None if slices_mask is None else slices_mask[idx].contiguous()
        out = slice_acquisition(transforms[idx], vol, vol_mask, sm, psf, slice_shape, res_slice, need_weight, False)
        if need_weight:
            slices[idx], weight[idx] = out
        else:
            slices[idx] = out
    return (slices, weight) if need_weight else slices


def slice_acquisition_adjoint_bank(transforms, bank, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf=False,
                                   equalize=False, need_weight=False):
    """``slice_acquisition_adjoint`` with a bank; ``need_weight`` (with ``equalize``): also the back-projected weight."""
    _no_gradient("slice_acquisition_adjoint_bank", transforms, slices)
    n = slices.shape[0]
    _bank_checks("slice_acquisition_adjoint_bank", bank, n, interp_psf)
    transforms, slices = transforms.contiguous(), slices.contiguous()
    if bank_fused():
        vol, vol_weight = torch.ops.nesvor.slice_acq_adjoint_forward_bank(
            transforms, bank.flat, bank.table, bank.ids, slices, _or_empty(slices_mask, slices), _or_empty(vol_mask, slices),
            [int(s) for s in vol_shape], float(res_slice), bool(equalize))
        return (vol, vol_weight) if need_weight else vol
    # composed: the sum of the members' unequalised adjoints (and weights), divided where the weight is positive
    shape = (1, 1) + tuple(int(s) for s in vol_shape)
    vol = torch.zeros(shape, dtype=slices.dtype, device=slices.device)
    vol_weight = torch.zeros_like(vol) if equalize else None
    for _, psf, idx in bank.members():
        sm = None if slices_mask is None else slices_mask[idx].contiguous()
        vol += slice_acquisition_adjoint(transforms[idx], psf, slices[idx], sm, vol_mask, vol_shape, res_slice, False, False)
        if equalize:
            # A^T of the member's slices is linear in them: its weight is the adjoint of 1 / (PSF weight) on the active pixels,
            # which the equalised one-PSF op returns next to the volume
            _, wgt = torch.ops.nesvor.slice_acq_adjoint_forward(
                transforms[idx].contiguous(), psf.contiguous(), slices[idx].contiguous(), _or_empty(sm, slices), _or_empty(vol_mask, slices),
                [int(s) for s in vol_shape], float(res_slice), False, True)
            vol_weight += wgt
    if equalize:
        pos = vol_weight > 0
        vol = torch.where(pos, vol / torch.where(pos, vol_weight, torch.ones_like(vol_weight)), vol)
    return (vol, vol_weight) if need_weight else vol
