"""PyTorch-ROCm custom operators of the NeSVoR path (dispatcher namespace ``nesvor``).

Every native kernel family of ``libnesvor_hip.so`` is registered with ``torch.library``:

* a schema (``torch.ops.nesvor.<op>``), so the ops are visible to the dispatcher, ``torch.compile`` and profilers;
* ONE backend kernel, under the ``CUDA`` dispatch key (PyTorch-ROCm files HIP tensors under that key).  No CPU kernel is
  registered: a host tensor fails in the dispatcher ("Could not run 'nesvor::...' with arguments from the 'CPU' backend") -
  the product has no CPU path, by construction;
* a fake (meta) kernel: output shapes / dtypes without touching data;
* an autograd formula (``register_autograd``) for the differentiable ops, built from the matching ``*_backward`` op.

The backend kernels are the C ABI of ``include/nesvor_hip.h`` (plain pointers + sizes + ``hipStream_t``) called through
``ctypes`` on torch's current stream; this module is the "thin torch-extension layer" of SURVEY.md 8(b): validate
device / dtype / contiguity, allocate outputs, launch.  The reference's two pybind modules keep their names
(``nesvor_amd.transform_convert_cuda``, ``nesvor_amd.slice_acq_cuda``) and forward here; the fused training step
(``nesvor_amd.direct``) calls the same C entry points back-to-back without going through the dispatcher.

Replaces: ``nesvor/transform/transform_convert_cuda.cpp:64-69`` and ``nesvor/slice_acquisition/slice_acq_cuda.cpp:156-161``
(PYBIND11_MODULE tables), ``tinycudann``'s autograd Functions (``nesvor/nesvor/models.py:25,31``).
"""
import ctypes
from typing import List, Optional

import torch
from torch.library import Library, register_autograd, register_fake

from . import _lib
from . import encoding as _enc
from . import loss as _loss
from . import mlp as _mlp
from . import sampler as _sampler
from .grid import HashGridSpec

NAMESPACE = "nesvor"
_LIBRARY = Library(NAMESPACE, "DEF")
SCHEMAS = {}


def _op(schema: str, kernel, fake=None, backward=None, setup_context=None):
    name = schema.split("(", 1)[0]
    _LIBRARY.define(schema)
    _LIBRARY.impl(name, kernel, "CUDA")
    if fake is not None:
        register_fake(f"{NAMESPACE}::{name}")(fake)
    if backward is not None:
        register_autograd(f"{NAMESPACE}::{name}", backward, setup_context=setup_context)
    SCHEMAS[name] = schema


def _empty(like: torch.Tensor) -> torch.Tensor:
    """Stand-in for an output that was not requested (the reference returns an undefined Tensor there)."""
    return torch.empty(0, dtype=like.dtype, device=like.device)


def _opt(t: torch.Tensor) -> Optional[torch.Tensor]:
    return t if t.numel() > 0 else None


def _workspace(nbytes: int, device) -> torch.Tensor:
    """``nbytes`` of 8-byte aligned scratch (at least one element, so that its pointer is never null)."""
    return torch.empty(max(nbytes, 8) // 8, dtype=torch.float64, device=device)


def _launch(name: str, device, sizes, *args, query: Optional[str] = None) -> None:
    """``nesvor_<name>(*args, workspace, nbytes, stream)`` on ``device`` with the scratch ``nesvor_<query>_workspace_bytes(*sizes)``
    asks for (``query``: ``name`` unless given - a ``_bank`` twin has no size query of its own and names its sibling's).  A size
    of 0 (a shape the library refuses) still reaches the library: the refusal is its own."""
    lib = _lib.load()
    nbytes = int(getattr(lib, f"nesvor_{query or name}_workspace_bytes")(*sizes))
    workspace = _workspace(nbytes, device)
    with torch.cuda.device(device):
        err = getattr(lib, f"nesvor_{name}")(*args, _lib.ptr(workspace), nbytes, _lib.stream_ptr())
    _lib.check(err, name.replace("_", " "))


def _n_bins(what: str, n_bins: int) -> None:
    if not 2 <= n_bins <= 1024:
        raise RuntimeError(f"{what}: 2 <= n_bins <= 1024 expected, got {n_bins}")


def _byte_mask(what: str, mask: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The optional validity mask of the classical-pipeline ops: bool or uint8 (any set byte counts), empty means none."""
    if mask is None or mask.numel() == 0:
        return None
    if mask.dtype not in (torch.bool, torch.uint8):
        raise RuntimeError(f"{what} mask must be torch.bool or torch.uint8, got {mask.dtype}")
    _lib.require_device(mask, name=f"{what} mask")
    return mask


def _and(names) -> str:
    return ", ".join(names[:-1]) + " and " + names[-1]


def _slice_stack(what: str, stacks: dict, mask, others: dict):
    """The checks of a slice stack: the named ``stacks`` and the mask are (n, ..., h, w) of one shape holding n x h x w
    elements, on one device with the named ``others``; -> (mask or None, n, h, w)."""
    m = _byte_mask(what, mask)
    tensors = [*stacks.values()] + ([] if m is None else [m])
    first = tensors[0]
    if first.ndim < 3 or any(t.shape != first.shape for t in tensors):
        raise RuntimeError(f"{what}: {_and([*stacks, 'mask'])} (n, ..., h, w) of one shape expected")
    if any(t.device != first.device for t in (*tensors, *others.values())):
        raise RuntimeError(f"{what}: {_and([*stacks, 'mask', *others])} must be on one device")
    n, h, w = int(first.shape[0]), int(first.shape[-2]), int(first.shape[-1])
    if first.numel() != n * h * w:
        raise RuntimeError(f"{what}: {' / '.join([*stacks, 'mask'])} must hold n x h x w elements")
    return m, n, h, w


# =====================================================================================================================
# rigid-transform conversions (reference module nesvor.transform_convert_cuda; float32 and float64)
# =====================================================================================================================
def _tc_suffix(t):
    if t.dtype == torch.float32:
        return ""
    if t.dtype == torch.float64:
        return "_f64"
    raise RuntimeError(f"transform_convert: unsupported dtype {t.dtype}")


def _tc_launch(symbol, what, n, *tensors):
    fn = getattr(_lib.load(), symbol)
    with torch.cuda.device(tensors[0].device):
        _lib.check(fn(*[_lib.ptr(t) for t in tensors], n, _lib.stream_ptr()), what)


def _ax2mat_fwd(axisangle):
    _lib.require_device(axisangle, name="axisangle")
    mat = torch.zeros((axisangle.shape[0], 3, 4), dtype=axisangle.dtype, device=axisangle.device)
    _tc_launch("nesvor_axisangle2mat_forward" + _tc_suffix(axisangle), "axisangle2mat_forward", axisangle.shape[0], axisangle, mat)
    return mat


def _ax2mat_bwd(grad_mat, axisangle):
    _lib.require_device(grad_mat, axisangle, name="grad_mat/axisangle")
    grad = torch.zeros((axisangle.shape[0], 6), dtype=axisangle.dtype, device=axisangle.device)
    _tc_launch("nesvor_axisangle2mat_backward" + _tc_suffix(axisangle), "axisangle2mat_backward", axisangle.shape[0], grad_mat, axisangle, grad)
    return grad


def _mat2ax_fwd(mat):
    _lib.require_device(mat, name="mat")
    ax = torch.zeros((mat.shape[0], 6), dtype=mat.dtype, device=mat.device)
    _tc_launch("nesvor_mat2axisangle_forward" + _tc_suffix(mat), "mat2axisangle_forward", mat.shape[0], mat, ax)
    return ax


def _mat2ax_bwd(mat, grad_axisangle):
    _lib.require_device(mat, grad_axisangle, name="mat/grad_axisangle")
    grad = torch.zeros((mat.shape[0], 3, 4), dtype=mat.dtype, device=mat.device)
    _tc_launch("nesvor_mat2axisangle_backward" + _tc_suffix(mat), "mat2axisangle_backward", mat.shape[0], mat, grad_axisangle, grad)
    return grad


_op("axisangle2mat_backward(Tensor grad_mat, Tensor axisangle) -> Tensor", _ax2mat_bwd,
    fake=lambda g, ax: ax.new_empty((ax.shape[0], 6)))
_op("axisangle2mat_forward(Tensor axisangle) -> Tensor", _ax2mat_fwd,
    fake=lambda ax: ax.new_empty((ax.shape[0], 3, 4)),
    backward=lambda ctx, g: torch.ops.nesvor.axisangle2mat_backward(g.contiguous(), ctx.saved_tensors[0]),
    setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0]))
_op("mat2axisangle_backward(Tensor mat, Tensor grad_axisangle) -> Tensor", _mat2ax_bwd,
    fake=lambda mat, g: mat.new_empty((mat.shape[0], 3, 4)))
_op("mat2axisangle_forward(Tensor mat) -> Tensor", _mat2ax_fwd,
    fake=lambda mat: mat.new_empty((mat.shape[0], 6)),
    backward=lambda ctx, g: torch.ops.nesvor.mat2axisangle_backward(ctx.saved_tensors[0], g.contiguous()),
    setup_context=lambda ctx, inputs, output: ctx.save_for_backward(inputs[0]))


# pose regulariser: value and gradient in one launch (models.py:357-363)
def _trans_loss(axisangle, axisangle_init):
    from .transform import trans_loss_raw

    per, grad = trans_loss_raw(axisangle, axisangle_init)
    return per.sum(), grad


def _trans_loss_setup(ctx, inputs, output):
    ctx.save_for_backward(output[1])
    ctx.set_materialize_grads(False)


_op("trans_loss(Tensor axisangle, Tensor axisangle_init) -> (Tensor, Tensor)", _trans_loss,
    fake=lambda ax, ax0: (ax.new_empty(()), torch.empty_like(ax)),
    backward=lambda ctx, g, g_unused: (None if g is None else ctx.saved_tensors[0] * g, None),
    setup_context=_trans_loss_setup)


# =====================================================================================================================
# slice acquisition A / A^T (reference module nesvor.slice_acq_cuda); "None" masks are empty tensors, as in
# slice_acq.py:36-39; outputs that were not requested come back as empty tensors
# =====================================================================================================================
def _mask(m):
    m = m if (m is not None and m.numel() > 0) else None
    if m is not None:
        _lib.require_device(m, dtype=torch.bool, name="mask")
    return m


def _sa_dims(vol_shape, psf):
    return tuple(int(s) for s in vol_shape[-3:]) + tuple(int(s) for s in psf.shape)


def _sa_symbol(name, t, interp_psf=False):
    """float32 / float64 (the reference's AT_DISPATCH_FLOATING_TYPES, slice_acq_cuda_kernel.cu:970-1114).  The
    PSF-interpolating mode of the backward / adjoint operators (:229-279, :526-572, :754) has its own entry points
    (``*_interp``: per-pixel scatter as the reference formulates it; no caller in the reference tree uses the mode)."""
    if t.dtype not in (torch.float32, torch.float64):
        raise NotImplementedError(f"slice_acq: float32 or float64 expected, got {t.dtype}")
    return getattr(_lib.load(), name + ("_interp" if interp_psf else "") + ("_f64" if t.dtype == torch.float64 else ""))


def _sa_forward(transforms, vol, vol_mask, slices_mask, psf, slice_shape, res_slice, need_weight, interp_psf):
    _lib.require_device(transforms, vol, psf, dtype=vol.dtype, name="transforms/vol/psf")
    vm, sm = _mask(vol_mask), _mask(slices_mask)
    n, (h, w) = transforms.shape[0], (int(slice_shape[0]), int(slice_shape[1]))
    slices = torch.zeros((n, 1, h, w), dtype=vol.dtype, device=vol.device)
    weight = torch.zeros((n, 1, h, w), dtype=vol.dtype, device=vol.device) if need_weight else None
    with torch.cuda.device(vol.device):
        err = _sa_symbol("nesvor_slice_acq_forward", vol)(
            _lib.ptr(transforms), _lib.ptr(vol), _lib.ptr(vm), _lib.ptr(sm), _lib.ptr(psf), _lib.ptr(slices), _lib.ptr(weight),
            *_sa_dims(vol.shape, psf), n, h, w, float(res_slice), int(bool(interp_psf)), _lib.stream_ptr())
    _lib.check(err, "slice_acq forward")
    return [slices, weight] if need_weight else [slices]


def _sa_backward(transforms, vol, vol_mask, psf, grad_slices, slices_mask, res_slice, interp_psf, need_vol_grad, need_transforms_grad):
    _lib.require_device(transforms, vol, psf, grad_slices, dtype=vol.dtype, name="slice_acq backward input")
    vm, sm = _mask(vol_mask), _mask(slices_mask)
    n, h, w = grad_slices.shape[0], grad_slices.shape[-2], grad_slices.shape[-1]
    # the interp kernels accumulate (atomics) into their outputs; the linear ones write every element, and the entry point
    # zero-fills both gradients itself when the stack is empty (n h w = 0: nothing is launched)
    new = torch.zeros_like if interp_psf else torch.empty_like
    grad_vol = new(vol) if need_vol_grad else None
    grad_tf = new(transforms) if need_transforms_grad else None
    scratch = () if interp_psf else (_lib.ptr(torch.empty(n * h * w, dtype=vol.dtype, device=vol.device)),)
    with torch.cuda.device(vol.device):
        err = _sa_symbol("nesvor_slice_acq_backward", vol, interp_psf)(
            _lib.ptr(transforms), _lib.ptr(vol), _lib.ptr(vm), _lib.ptr(psf), _lib.ptr(grad_slices), _lib.ptr(sm),
            _lib.ptr(grad_vol), _lib.ptr(grad_tf), *scratch, *_sa_dims(vol.shape, psf), n, h, w, float(res_slice),
            _lib.stream_ptr())
    _lib.check(err, "slice_acq backward")
    return [grad_vol if need_vol_grad else _empty(vol), grad_tf if need_transforms_grad else _empty(vol)]


def _sa_adjoint_forward(transforms, psf, slices, slices_mask, vol_mask, vol_shape, res_slice, interp_psf, equalize):
    _lib.require_device(transforms, psf, slices, dtype=slices.dtype, name="slice_acq adjoint input")
    vm, sm = _mask(vol_mask), _mask(slices_mask)
    n, h, w = slices.shape[0], slices.shape[-2], slices.shape[-1]
    D, H, W = (int(s) for s in vol_shape)
    new = torch.zeros if interp_psf else torch.empty  # the interp kernel accumulates (atomics) into its outputs
    vol = new((1, 1, D, H, W), dtype=slices.dtype, device=slices.device)
    vol_weight = new((1, 1, D, H, W), dtype=slices.dtype, device=slices.device) if equalize else None
    scratch = () if interp_psf else (_lib.ptr(torch.empty(2 * n * h * w, dtype=slices.dtype, device=slices.device)),)
    with torch.cuda.device(slices.device):
        err = _sa_symbol("nesvor_slice_acq_adjoint_forward", slices, interp_psf)(
            _lib.ptr(transforms), _lib.ptr(psf), _lib.ptr(slices), _lib.ptr(sm), _lib.ptr(vm), _lib.ptr(vol), _lib.ptr(vol_weight),
            *scratch, *_sa_dims((D, H, W), psf), n, h, w, float(res_slice), int(bool(equalize)), _lib.stream_ptr())
    _lib.check(err, "slice_acq adjoint_forward")
    return [vol, vol_weight if equalize else _empty(slices)]


def _sa_adjoint_backward(transforms, grad_vol, vol_weight, vol_mask, psf, slices, slices_mask, vol, res_slice, interp_psf,
                         equalize, need_slices_grad, need_transforms_grad):
    _lib.require_device(transforms, grad_vol, psf, slices, dtype=slices.dtype, name="slice_acq adjoint_backward input")
    if equalize:
        _lib.require_device(vol_weight, vol, dtype=slices.dtype, name="slice_acq adjoint_backward vol/vol_weight")
    vm, sm = _mask(vol_mask), _mask(slices_mask)
    n, h, w = slices.shape[0], slices.shape[-2], slices.shape[-1]
    grad_slices = torch.zeros_like(slices) if need_slices_grad else None
    grad_tf = (torch.zeros_like if interp_psf else torch.empty_like)(transforms) if need_transforms_grad else None
    with torch.cuda.device(slices.device):
        err = _sa_symbol("nesvor_slice_acq_adjoint_backward", slices, interp_psf)(
            _lib.ptr(transforms), _lib.ptr(grad_vol), _lib.ptr(vol_weight if equalize else None), _lib.ptr(vm), _lib.ptr(psf),
            _lib.ptr(slices), _lib.ptr(sm), _lib.ptr(vol if equalize else None), _lib.ptr(grad_slices), _lib.ptr(grad_tf),
            *_sa_dims(grad_vol.shape, psf), n, h, w, float(res_slice), int(bool(equalize)), _lib.stream_ptr())
    _lib.check(err, "slice_acq adjoint_backward")
    return [grad_slices if need_slices_grad else _empty(slices), grad_tf if need_transforms_grad else _empty(slices)]


def _sa_forward_setup(ctx, inputs, output):
    transforms, vol, vol_mask, slices_mask, psf, _, res_slice, _, interp_psf = inputs
    # what the kernel actually read (the op requires contiguous inputs, so these are the caller's tensors)
    ctx.save_for_backward(transforms, vol, vol_mask, slices_mask, psf)
    ctx.res_slice, ctx.interp_psf = res_slice, interp_psf


def _sa_forward_backward(ctx, grads):
    transforms, vol, vol_mask, slices_mask, psf = ctx.saved_tensors
    gv, gt = torch.ops.nesvor.slice_acq_backward(
        transforms, vol, vol_mask, psf, grads[0].contiguous(), slices_mask, ctx.res_slice, ctx.interp_psf,
        ctx.needs_input_grad[1], ctx.needs_input_grad[0])
    return _opt(gt), _opt(gv), None, None, None, None, None, None, None


def _sa_adjoint_setup(ctx, inputs, output):
    transforms, psf, slices, slices_mask, vol_mask, _, res_slice, interp_psf, equalize = inputs
    ctx.save_for_backward(transforms, psf, slices, slices_mask, vol_mask, output[0], output[1])
    ctx.res_slice, ctx.interp_psf, ctx.equalize = res_slice, interp_psf, equalize


def _sa_adjoint_backward_formula(ctx, grads):
    transforms, psf, slices, slices_mask, vol_mask, vol, vol_weight = ctx.saved_tensors
    # the native op equalises grad_vol in place (as the reference does): work on a private contiguous copy
    grad_vol = grads[0].contiguous().clone() if ctx.equalize else grads[0].contiguous()
    gs, gt = torch.ops.nesvor.slice_acq_adjoint_backward(
        transforms, grad_vol, vol_weight, vol_mask, psf, slices, slices_mask, vol, ctx.res_slice, ctx.interp_psf, ctx.equalize,
        ctx.needs_input_grad[2], ctx.needs_input_grad[0])
    return _opt(gt), None, _opt(gs), None, None, None, None, None, None


def _fake_slices(transforms, vol, vol_mask, slices_mask, psf, slice_shape, res_slice, need_weight, interp_psf):
    out = vol.new_empty((transforms.shape[0], 1, int(slice_shape[0]), int(slice_shape[1])))
    return [out, torch.empty_like(out)] if need_weight else [out]


_op("slice_acq_backward(Tensor transforms, Tensor vol, Tensor vol_mask, Tensor psf, Tensor grad_slices, Tensor slices_mask, "
    "float res_slice, bool interp_psf, bool need_vol_grad, bool need_transforms_grad) -> Tensor[]", _sa_backward,
    fake=lambda tf, vol, vm, psf, gs, sm, r, i, nv, nt: [torch.empty_like(vol) if nv else vol.new_empty(0),
                                                         torch.empty_like(tf) if nt else vol.new_empty(0)])
_op("slice_acq_forward(Tensor transforms, Tensor vol, Tensor vol_mask, Tensor slices_mask, Tensor psf, int[] slice_shape, "
    "float res_slice, bool need_weight, bool interp_psf) -> Tensor[]", _sa_forward, fake=_fake_slices,
    backward=_sa_forward_backward, setup_context=_sa_forward_setup)
_op("slice_acq_adjoint_backward(Tensor transforms, Tensor(a!) grad_vol, Tensor vol_weight, Tensor vol_mask, Tensor psf, "
    "Tensor slices, Tensor slices_mask, Tensor vol, float res_slice, bool interp_psf, bool equalize, bool need_slices_grad, "
    "bool need_transforms_grad) -> Tensor[]", _sa_adjoint_backward,
    fake=lambda tf, gv, vw, vm, psf, s, sm, vol, r, i, e, ns, nt: [torch.empty_like(s) if ns else s.new_empty(0),
                                                                   torch.empty_like(tf) if nt else s.new_empty(0)])
_op("slice_acq_adjoint_forward(Tensor transforms, Tensor psf, Tensor slices, Tensor slices_mask, Tensor vol_mask, "
    "int[] vol_shape, float res_slice, bool interp_psf, bool equalize) -> Tensor[]", _sa_adjoint_forward,
    fake=lambda tf, psf, s, sm, vm, shape, r, i, e: [s.new_empty((1, 1) + tuple(int(v) for v in shape)),
                                                     s.new_empty((1, 1) + tuple(int(v) for v in shape)) if e else s.new_empty(0)],
    backward=_sa_adjoint_backward_formula, setup_context=_sa_adjoint_setup)


# =====================================================================================================================
# similarity sums of the slice-to-volume registration (csrc/svr.hip): A under K poses per slice, reduced in one call
# =====================================================================================================================
SVR_MAX_PSF_ELEMENTS = 1024  # larger PSFs are refused by the kernel (its LDS tap list); compose from slice_acq_forward


def _svr_stack(what, ok, expected, vol, slices, slices_mask, n):
    """What every svr statistic checks about the inputs they share: the shapes (``ok``: those of the op's own inputs, named in
    ``expected``), vol (..., D, H, W) holding one volume, slices and the mask holding n x h x w elements
    -> (mask or None, h, w, the volume's arguments (pointer, D, H, W))."""
    sm = _mask(slices_mask)
    if not ok or vol.ndim < 3 or slices.ndim < 3:
        raise RuntimeError(f"{what}: vol (..., D, H, W), {expected}, slices (n, ..., h, w)")
    h, w = int(slices.shape[-2]), int(slices.shape[-1])
    if slices.numel() != n * h * w or (sm is not None and sm.numel() != n * h * w):
        raise RuntimeError(f"{what}: slices / slices_mask must hold n x h x w elements")
    D, H, W = (int(s) for s in vol.shape[-3:])
    if vol.numel() != D * H * W:
        raise RuntimeError(f"{what}: one volume expected")
    return sm, h, w, (_lib.ptr(vol), D, H, W)


def _svr_poses(what, vol, transforms, slices, slices_mask):
    """The inputs of the statistics per (slice, pose): ``_svr_stack`` with transforms (n, K, 3, 4) -> (n, K, mask or None, h, w,
    the volume's arguments)."""
    ok = transforms.ndim == 4 and tuple(transforms.shape[2:]) == (3, 4)
    n, K = (int(transforms.shape[0]), int(transforms.shape[1])) if ok else (-1, -1)
    return (n, K, *_svr_stack(what, ok, "transforms (n, K, 3, 4)", vol, slices, slices_mask, n))


def _one_psf(what, psf):
    """One PSF for every slice, as the entry points of the family take it: (pointer, d_p, h_p, w_p)."""
    _lib.require_device(psf, dtype=torch.float32, name=f"{what} psf")
    if psf.ndim != 3:
        raise RuntimeError(f"{what}: psf (d, h, w) expected")
    return (_lib.ptr(psf), *(int(s) for s in psf.shape))


def _svr_sums(what, vol, psf_args, transforms, slices, slices_mask, res_slice):
    """``psf_args(n)``: the entry point's PSF arguments (``_one_psf``, or ``_bank`` for a ``_bank`` twin) - here and below."""
    _lib.require_device(vol, transforms, slices, dtype=torch.float32, name=f"{what} vol/transforms/slices")
    n, K, sm, h, w, volume = _svr_poses(what, vol, transforms, slices, slices_mask)
    psf = psf_args(n)
    sums = torch.empty((n, K, 6), dtype=torch.float64, device=vol.device)
    _launch(what, vol.device, (n, K, h, w), *volume, *psf, _lib.ptr(transforms), _lib.ptr(slices), _lib.ptr(sm), n, K, h, w,
            float(res_slice), _lib.ptr(sums), query="svr_similarity")
    return sums


def _svr_similarity(vol, psf, transforms, slices, slices_mask, res_slice):
    return _svr_sums("svr_similarity", vol, lambda n: _one_psf("svr_similarity", psf), transforms, slices, slices_mask, res_slice)


_op("svr_similarity(Tensor vol, Tensor psf, Tensor transforms, Tensor slices, Tensor? slices_mask, float res_slice) -> Tensor",
    _svr_similarity, fake=lambda vol, psf, tf, s, sm, r: vol.new_empty((tf.shape[0], tf.shape[1], 6), dtype=torch.float64))


# =====================================================================================================================
# per-slice PSFs (nesvor_amd/psf_bank.py): A, A^T and the similarity sums with a PSF bank - psf_bank the members concatenated,
# psf_table (P,4) int32 on the HOST {offset, d_p, h_p, w_p}, psf_id (n) int32 on the device.  fp32, linear mode, no autograd
# formula (slice_acquisition.py raises when a gradient is asked for)
# =====================================================================================================================
def _bank(what, psf_bank, psf_table, psf_id, n):
    _lib.require_device(psf_bank, dtype=torch.float32, name=f"{what} psf_bank")
    _lib.require_device(psf_id, dtype=torch.int32, name=f"{what} psf_id")
    if psf_table.is_cuda or psf_table.dtype != torch.int32 or psf_table.ndim != 2 or psf_table.shape[1] != 4 or not psf_table.is_contiguous():
        raise RuntimeError(f"{what}: psf_table, (P, 4) int32 in host memory, expected")
    if psf_id.numel() != n:
        raise RuntimeError(f"{what}: psf_id must hold one id per slice ({n}), got {psf_id.numel()}")
    P = int(psf_table.shape[0])
    if P > 0 and int((psf_table[:, 0] + psf_table[:, 1:].prod(1)).max()) > psf_bank.numel():
        raise RuntimeError(f"{what}: a row of psf_table reaches past the end of psf_bank")
    return _lib.ptr(psf_bank), ctypes.c_void_p(psf_table.data_ptr()), P, _lib.ptr(psf_id)


def _sa_forward_bank(transforms, vol, vol_mask, slices_mask, psf_bank, psf_table, psf_id, slice_shape, res_slice, need_weight):
    _lib.require_device(transforms, vol, dtype=torch.float32, name="slice_acq_forward_bank transforms/vol")
    vm, sm = _mask(vol_mask), _mask(slices_mask)
    n, (h, w) = transforms.shape[0], (int(slice_shape[0]), int(slice_shape[1]))
    bank = _bank("slice_acq_forward_bank", psf_bank, psf_table, psf_id, n)
    slices = torch.zeros((n, 1, h, w), dtype=vol.dtype, device=vol.device)
    weight = torch.zeros((n, 1, h, w), dtype=vol.dtype, device=vol.device) if need_weight else None
    with torch.cuda.device(vol.device):
        err = _lib.load().nesvor_slice_acq_forward_bank(
            _lib.ptr(transforms), _lib.ptr(vol), _lib.ptr(vm), _lib.ptr(sm), *bank, _lib.ptr(slices), _lib.ptr(weight),
            *(int(s) for s in vol.shape[-3:]), n, h, w, float(res_slice), _lib.stream_ptr())
    _lib.check(err, "slice_acq forward_bank")
    return [slices, weight] if need_weight else [slices]


def _sa_adjoint_forward_bank(transforms, psf_bank, psf_table, psf_id, slices, slices_mask, vol_mask, vol_shape, res_slice, equalize):
    _lib.require_device(transforms, slices, dtype=torch.float32, name="slice_acq_adjoint_forward_bank transforms/slices")
    vm, sm = _mask(vol_mask), _mask(slices_mask)
    n, h, w = slices.shape[0], slices.shape[-2], slices.shape[-1]
    bank = _bank("slice_acq_adjoint_forward_bank", psf_bank, psf_table, psf_id, n)
    D, H, W = (int(s) for s in vol_shape)
    vol = torch.empty((1, 1, D, H, W), dtype=slices.dtype, device=slices.device)
    vol_weight = torch.empty((1, 1, D, H, W), dtype=slices.dtype, device=slices.device) if equalize else None
    scratch = torch.empty(max(2 * n * h * w, 1), dtype=slices.dtype, device=slices.device)
    with torch.cuda.device(slices.device):
        err = _lib.load().nesvor_slice_acq_adjoint_forward_bank(
            _lib.ptr(transforms), *bank, _lib.ptr(slices), _lib.ptr(sm), _lib.ptr(vm), _lib.ptr(vol), _lib.ptr(vol_weight),
            _lib.ptr(scratch), D, H, W, n, h, w, float(res_slice), int(bool(equalize)), _lib.stream_ptr())
    _lib.check(err, "slice_acq adjoint_forward_bank")
    return [vol, vol_weight if equalize else _empty(slices)]


def _svr_similarity_bank(vol, psf_bank, psf_table, psf_id, transforms, slices, slices_mask, res_slice):
    return _svr_sums("svr_similarity_bank", vol, lambda n: _bank("svr_similarity_bank", psf_bank, psf_table, psf_id, n), transforms,
                     slices, slices_mask, res_slice)


_op("slice_acq_forward_bank(Tensor transforms, Tensor vol, Tensor vol_mask, Tensor slices_mask, Tensor psf_bank, Tensor psf_table, "
    "Tensor psf_id, int[] slice_shape, float res_slice, bool need_weight) -> Tensor[]", _sa_forward_bank,
    fake=lambda tf, vol, vm, sm, pb, pt, pi, shape, r, nw: _fake_slices(tf, vol, vm, sm, pb, shape, r, nw, False))
_op("slice_acq_adjoint_forward_bank(Tensor transforms, Tensor psf_bank, Tensor psf_table, Tensor psf_id, Tensor slices, "
    "Tensor slices_mask, Tensor vol_mask, int[] vol_shape, float res_slice, bool equalize) -> Tensor[]", _sa_adjoint_forward_bank,
    fake=lambda tf, pb, pt, pi, s, sm, vm, shape, r, e: [s.new_empty((1, 1) + tuple(int(v) for v in shape)),
                                                         s.new_empty((1, 1) + tuple(int(v) for v in shape)) if e else s.new_empty(0)])
_op("svr_similarity_bank(Tensor vol, Tensor psf_bank, Tensor psf_table, Tensor psf_id, Tensor transforms, Tensor slices, "
    "Tensor? slices_mask, float res_slice) -> Tensor", _svr_similarity_bank,
    fake=lambda vol, pb, pt, pi, tf, s, sm, r: vol.new_empty((tf.shape[0], tf.shape[1], 6), dtype=torch.float64))


# =====================================================================================================================
# joint histograms of the slice-to-volume registration (csrc/svr_nmi.hip; the definition: nesvor_amd/nmi.py): what svr_similarity
# sums into moments, binned - (n, K, B, B) int64, row = bin of the simulated value.  i_lo / i_scale: floats fp32 holds exactly
# =====================================================================================================================
def _svr_histogram(what, vol, psf_args, transforms, slices, slices_mask, res_slice, i_lo, i_scale, j_map, bins):
    _lib.require_device(vol, transforms, slices, j_map, dtype=torch.float32, name=f"{what} vol/transforms/slices/j_map")
    n, K, sm, h, w, volume = _svr_poses(what, vol, transforms, slices, slices_mask)
    if tuple(j_map.shape) != (n, 2):
        raise RuntimeError(f"{what}: j_map (n, 2) = ({n}, 2) expected, got {tuple(j_map.shape)}")
    bins = int(bins)
    if not 2 <= bins <= 64:
        raise RuntimeError(f"{what}: 2 <= bins <= 64 expected, got {bins}")
    psf = psf_args(n)
    hist = torch.empty((n, K, bins, bins), dtype=torch.int64, device=vol.device)
    _launch(what, vol.device, (n, K, h, w, bins), *volume, *psf, _lib.ptr(transforms), _lib.ptr(slices), _lib.ptr(sm), n, K, h, w,
            float(res_slice), float(i_lo), float(i_scale), _lib.ptr(j_map), bins, _lib.ptr(hist), query="svr_joint_histogram")
    return hist


def _svr_joint_histogram(vol, psf, transforms, slices, slices_mask, res_slice, i_lo, i_scale, j_map, bins):
    return _svr_histogram("svr_joint_histogram", vol, lambda n: _one_psf("svr_joint_histogram", psf), transforms, slices, slices_mask,
                          res_slice, i_lo, i_scale, j_map, bins)


def _svr_joint_histogram_bank(vol, psf_bank, psf_table, psf_id, transforms, slices, slices_mask, res_slice, i_lo, i_scale, j_map, bins):
    return _svr_histogram("svr_joint_histogram_bank", vol, lambda n: _bank("svr_joint_histogram_bank", psf_bank, psf_table, psf_id, n),
                          transforms, slices, slices_mask, res_slice, i_lo, i_scale, j_map, bins)


def _fake_histogram(vol, tf, bins):
    return vol.new_empty((tf.shape[0], tf.shape[1], bins, bins), dtype=torch.int64)


_op("svr_joint_histogram(Tensor vol, Tensor psf, Tensor transforms, Tensor slices, Tensor? slices_mask, float res_slice, float i_lo, "
    "float i_scale, Tensor j_map, int bins) -> Tensor", _svr_joint_histogram,
    fake=lambda vol, psf, tf, s, sm, r, lo, sc, jm, bins: _fake_histogram(vol, tf, bins))
_op("svr_joint_histogram_bank(Tensor vol, Tensor psf_bank, Tensor psf_table, Tensor psf_id, Tensor transforms, Tensor slices, "
    "Tensor? slices_mask, float res_slice, float i_lo, float i_scale, Tensor j_map, int bins) -> Tensor", _svr_joint_histogram_bank,
    fake=lambda vol, pb, pt, pi, tf, s, sm, r, lo, sc, jm, bins: _fake_histogram(vol, tf, bins))


# =====================================================================================================================
# joint histograms of the stack registration (csrc/vvr_nmi.hip; the definition: nesvor_amd/nmi.py) and the samples they bin: what
# nesvor_vvr_similarity sums into moments - source (..., D, H, W), points (M, 3), target (M), mats (K, 3, 4), to_unit three floats
# =====================================================================================================================
def _vvr_cloud(what, source, points, mats, to_unit, target=None):
    """The checks of a stack registration's call -> (D, H, W, M, K, to_unit as the library reads it)."""
    names = "source/points/mats" + ("" if target is None else "/target")
    _lib.require_device(source, points, mats, target, dtype=torch.float32, name=f"{what} {names}")
    if source.ndim < 3 or source.numel() != source.shape[-3] * source.shape[-2] * source.shape[-1]:
        raise RuntimeError(f"{what}: source must hold one (D, H, W) volume, got {tuple(source.shape)}")
    if points.ndim != 2 or points.shape[1] != 3 or mats.ndim != 3 or tuple(mats.shape[1:]) != (3, 4) or len(to_unit) != 3:
        raise RuntimeError(f"{what}: points (M, 3), mats (K, 3, 4) and three to_unit factors expected")
    if target is not None and target.numel() != points.shape[0]:
        raise RuntimeError(f"{what}: target must hold one value per point ({points.shape[0]}), got {target.numel()}")
    if any(t.device != source.device for t in (points, mats) + (() if target is None else (target,))):
        raise RuntimeError(f"{what}: {names} must be on one device")
    D, H, W = (int(s) for s in source.shape[-3:])
    return D, H, W, int(points.shape[0]), int(mats.shape[0]), (ctypes.c_float * 3)(*(float(u) for u in to_unit))


def _vvr_joint_histogram(source, points, target, mats, to_unit, i_lo, i_scale, j_lo, j_scale, bins):
    what = "vvr_joint_histogram"
    D, H, W, M, K, unit = _vvr_cloud(what, source, points, mats, to_unit, target)
    bins = int(bins)
    if not 2 <= bins <= 64:
        raise RuntimeError(f"{what}: 2 <= bins <= 64 expected, got {bins}")
    if M == 0 or K == 0:  # (a no-op of the library: an empty point list has an empty histogram)
        return torch.zeros((K, bins, bins), dtype=torch.int64, device=source.device)
    hist = torch.empty((K, bins, bins), dtype=torch.int64, device=source.device)
    _launch(what, source.device, (M, K, bins), _lib.ptr(source), D, H, W, _lib.ptr(points), _lib.ptr(target), _lib.ptr(mats), unit, M, K,
            float(i_lo), float(i_scale), float(j_lo), float(j_scale), bins, _lib.ptr(hist))
    return hist


def _vvr_sample(source, points, mats, to_unit):
    D, H, W, M, K, unit = _vvr_cloud("vvr_sample", source, points, mats, to_unit)
    out = torch.empty((K, M), dtype=torch.float32, device=source.device)
    with torch.cuda.device(source.device):
        err = _lib.load().nesvor_vvr_sample(_lib.ptr(source), D, H, W, _lib.ptr(points), _lib.ptr(mats), unit, M, K, _lib.ptr(out),
                                            _lib.stream_ptr())
    _lib.check(err, "vvr sample")
    return out


_op("vvr_joint_histogram(Tensor source, Tensor points, Tensor target, Tensor mats, float[] to_unit, float i_lo, float i_scale, "
    "float j_lo, float j_scale, int bins) -> Tensor", _vvr_joint_histogram,
    fake=lambda src, pts, tgt, mats, u, ilo, isc, jlo, jsc, bins: src.new_empty((mats.shape[0], bins, bins), dtype=torch.int64))
_op("vvr_sample(Tensor source, Tensor points, Tensor mats, float[] to_unit) -> Tensor", _vvr_sample,
    fake=lambda src, pts, mats, u: src.new_empty((mats.shape[0], pts.shape[0])))


# =====================================================================================================================
# grouped similarity sums (package registration, csrc/svr.hip): one correction per (group, pose), composed with every slice's
# base pose in the kernel, sums per (group, pose) in CSR order.  The grouping arrives in HOST memory, is checked there and
# uploaded: a bad index is a Python exception, never a device read, and no call reads the device back
# =====================================================================================================================
def check_grouping(what: str, group_offsets: torch.Tensor, group_slices: torch.Tensor, n: int):
    """The CSR grouping of ``svr_similarity_groups``, checked on the host -> (offsets int32, slices int32, G, E).  Offsets
    (G+1) start at 0, do not decrease and end at ``len(group_slices)``; every slice index lies in [0, n)."""
    for name, t in (("group_offsets", group_offsets), ("group_slices", group_slices)):
        if t.is_cuda or t.dtype not in (torch.int32, torch.int64) or t.ndim != 1:
            raise RuntimeError(f"{what}: {name}, a 1-D int32 / int64 tensor in host memory, expected")
    G, E = int(group_offsets.numel()) - 1, int(group_slices.numel())
    if G < 1:
        raise RuntimeError(f"{what}: group_offsets must hold G + 1 >= 2 entries, got {G + 1}")
    if int(group_offsets[0]) != 0 or bool((group_offsets[1:] < group_offsets[:-1]).any()):
        raise RuntimeError(f"{what}: group_offsets must start at 0 and must not decrease")
    if int(group_offsets[-1]) != E:
        raise RuntimeError(f"{what}: the last of group_offsets ({int(group_offsets[-1])}) must equal len(group_slices) ({E})")
    if E > 0 and (int(group_slices.min()) < 0 or int(group_slices.max()) >= n):
        raise RuntimeError(f"{what}: group_slices must lie in [0, {n}), got [{int(group_slices.min())}, {int(group_slices.max())}]")
    return group_offsets.to(torch.int32).contiguous(), group_slices.to(torch.int32).contiguous(), G, E


def _svr_groups(what, vol, psf_args, corrections, base, group_offsets, group_slices, slices, slices_mask, res_slice):
    n = int(base.shape[0]) if base.ndim == 3 else -1
    offsets, listed, G, E = check_grouping(what, group_offsets, group_slices, n)  # first: nothing is launched on a bad grouping
    _lib.require_device(vol, corrections, base, slices, dtype=torch.float32, name=f"{what} vol/corrections/base/slices")
    ok = (corrections.ndim == 4 and tuple(corrections.shape[2:]) == (3, 4) and base.ndim == 3 and tuple(base.shape[1:]) == (3, 4)
          and int(corrections.shape[0]) == G)
    sm, h, w, volume = _svr_stack(what, ok, "corrections (G, K, 3, 4), base (n, 3, 4), group_offsets (G + 1)", vol, slices, slices_mask, n)
    K = int(corrections.shape[1])
    psf = psf_args(n)
    if E == 0 or K == 0:  # (the library returns without a launch and without writing)
        return torch.zeros((G, K, 6), dtype=torch.float64, device=vol.device)
    sums = torch.empty((G, K, 6), dtype=torch.float64, device=vol.device)
    offsets, listed = offsets.to(vol.device), listed.to(vol.device)
    _launch(what, vol.device, (E, K, h, w), *volume, *psf, _lib.ptr(base), _lib.ptr(corrections), _lib.ptr(offsets), _lib.ptr(listed),
            G, E, _lib.ptr(slices), _lib.ptr(sm), n, K, h, w, float(res_slice), _lib.ptr(sums), query="svr_similarity_groups")
    return sums


def _svr_similarity_groups(vol, psf, corrections, base, group_offsets, group_slices, slices, slices_mask, res_slice):
    return _svr_groups("svr_similarity_groups", vol, lambda n: _one_psf("svr_similarity_groups", psf), corrections, base, group_offsets,
                       group_slices, slices, slices_mask, res_slice)


def _svr_similarity_groups_bank(vol, psf_bank, psf_table, psf_id, corrections, base, group_offsets, group_slices, slices,
                                slices_mask, res_slice):
    return _svr_groups("svr_similarity_groups_bank", vol, lambda n: _bank("svr_similarity_groups_bank", psf_bank, psf_table, psf_id, n),
                       corrections, base, group_offsets, group_slices, slices, slices_mask, res_slice)


_op("svr_similarity_groups(Tensor vol, Tensor psf, Tensor corrections, Tensor base, Tensor group_offsets, Tensor group_slices, "
    "Tensor slices, Tensor? slices_mask, float res_slice) -> Tensor", _svr_similarity_groups,
    fake=lambda vol, psf, c, b, go, gs, s, sm, r: vol.new_empty((c.shape[0], c.shape[1], 6), dtype=torch.float64))
_op("svr_similarity_groups_bank(Tensor vol, Tensor psf_bank, Tensor psf_table, Tensor psf_id, Tensor corrections, Tensor base, "
    "Tensor group_offsets, Tensor group_slices, Tensor slices, Tensor? slices_mask, float res_slice) -> Tensor",
    _svr_similarity_groups_bank,
    fake=lambda vol, pb, pt, pi, c, b, go, gs, s, sm, r: vol.new_empty((c.shape[0], c.shape[1], 6), dtype=torch.float64))


# =====================================================================================================================
# one descent step of the classical reconstruction with the edge-preserving prior (csrc/srr.hip):
# out = x - alpha (grad + beta dR(x)), dR = srr.edge_prior_gradient, in one launch
# =====================================================================================================================
def srr_step_into(x, grad, out, alpha, beta, delta, clamp):
    """``out`` <- the step; ``out`` may be ``grad`` itself, must not overlap ``x`` (the library refuses it).  Returns ``out``."""
    _lib.require_device(x, grad, out, dtype=torch.float32, name="srr_step x/grad/out")
    if x.ndim < 3 or x.numel() != int(x.shape[-3]) * int(x.shape[-2]) * int(x.shape[-1]):
        raise RuntimeError("srr_step: one volume (..., D, H, W) expected")
    if grad.shape != x.shape or out.shape != x.shape:
        raise RuntimeError("srr_step: x, grad and out must have one shape")
    with torch.cuda.device(x.device):
        err = _lib.load().nesvor_srr_step(_lib.ptr(x), _lib.ptr(grad), _lib.ptr(out), *(int(s) for s in x.shape[-3:]), float(alpha),
                                          float(beta), float(delta), int(bool(clamp)), _lib.stream_ptr())
    _lib.check(err, "srr step")
    return out


def _srr_step(x, grad, alpha, beta, delta, clamp):
    return srr_step_into(x, grad, torch.empty_like(x), alpha, beta, delta, clamp)


def _srr_step_inplace(x, grad, alpha, beta, delta, clamp):
    srr_step_into(x, grad, grad, alpha, beta, delta, clamp)


_op("srr_step(Tensor x, Tensor grad, float alpha, float beta, float delta, bool clamp) -> Tensor", _srr_step,
    fake=lambda x, grad, alpha, beta, delta, clamp: torch.empty_like(x))
# the same step written over the gradient (out == grad): the solver's loop needs no third volume
_op("srr_step_(Tensor x, Tensor(a!) grad, float alpha, float beta, float delta, bool clamp) -> ()", _srr_step_inplace,
    fake=lambda *a: None)


# =====================================================================================================================
# E-step of the robust statistics of the classical reconstruction (csrc/robust.hip): pixel posteriors p and the seven
# per-slice sums of one EM round in one pass over (sim, y, mask); the host logic is nesvor_amd/robust.py
# =====================================================================================================================
def _robust_estep(sim, y, mask, scale, model):
    _lib.require_device(sim, y, scale, model, dtype=torch.float32, name="robust_estep sim/y/scale/model")
    m, n, h, w = _slice_stack("robust_estep", {"sim": sim, "y": y}, mask, {"scale": scale, "model": model})
    if scale.numel() != n or model.numel() != 3:
        raise RuntimeError("robust_estep: scale (n) and model {sigma2, c, m} (3) expected")
    p = torch.empty_like(sim)
    stats = torch.empty((n, 7), dtype=torch.float64, device=sim.device)
    _launch("robust_estep", sim.device, (n, h, w), _lib.ptr(sim), _lib.ptr(y), _lib.ptr(m), _lib.ptr(scale), _lib.ptr(model), n, h, w,
            _lib.ptr(p), _lib.ptr(stats))
    return p, stats


_op("robust_estep(Tensor sim, Tensor y, Tensor? mask, Tensor scale, Tensor model) -> (Tensor p, Tensor stats)", _robust_estep,
    fake=lambda sim, y, mask, scale, model: (torch.empty_like(sim), sim.new_empty((sim.shape[0], 7), dtype=torch.float64)))


# =====================================================================================================================
# structural exclusion of the classical reconstruction (csrc/structural.hip): the local SSIM map of scale_k y against sim and
# the eight per-slice sums of the slice similarity in one pass; the definition and the decisions are nesvor_amd/structural.py
# =====================================================================================================================
def _structural_ssim(sim, y, mask, scale, threshold, dynamic_range):
    _lib.require_device(sim, y, scale, dtype=torch.float32, name="structural_ssim sim/y/scale")
    m, n, h, w = _slice_stack("structural_ssim", {"sim": sim, "y": y}, mask, {"scale": scale})
    if scale.numel() != n:
        raise RuntimeError("structural_ssim: scale (n) expected")
    ssim = torch.empty_like(sim)
    stats = torch.empty((n, 8), dtype=torch.float64, device=sim.device)
    c1, c2 = (0.01 * dynamic_range) ** 2, (0.03 * dynamic_range) ** 2
    _launch("structural_ssim", sim.device, (n, h, w), _lib.ptr(sim), _lib.ptr(y), _lib.ptr(m), _lib.ptr(scale), n, h, w, c1, c2,
            float(threshold), _lib.ptr(ssim), _lib.ptr(stats))
    return ssim, stats


_op("structural_ssim(Tensor sim, Tensor y, Tensor? mask, Tensor scale, float threshold, float dynamic_range) -> (Tensor ssim, Tensor stats)",
    _structural_ssim,
    fake=lambda sim, y, mask, scale, threshold, dynamic_range: (torch.empty_like(sim),
                                                                sim.new_empty((sim.shape[0], 8), dtype=torch.float64)))


# =====================================================================================================================
# volume comparison (csrc/evaluate.hip): a volume on a reference volume's lattice with the first sums, and the 3-D SSIM map of
# the two with the sums of the error measures; the definition, the fit between the two and the report are nesvor_amd/evaluate.py
# =====================================================================================================================
EVALUATE_Z_CHUNK = 32  # planes per workgroup of volume_ssim (kZChunk of csrc/evaluate.hip): a chunk warms up on the 10 planes before it


def _volume(what, name, t, mask):
    """A (D,H,W) fp32 volume and its optional mask; -> (mask or None, D, H, W)."""
    _lib.require_device(t, dtype=torch.float32, name=f"{what} {name}")
    m = _byte_mask(f"{what} {name}", mask)
    if t.ndim != 3 or (m is not None and m.shape != t.shape):
        raise RuntimeError(f"{what}: {name} and its mask (D, H, W) of one shape expected")
    if m is not None and m.device != t.device:
        raise RuntimeError(f"{what}: {name} and its mask must be on one device")
    return m, int(t.shape[0]), int(t.shape[1]), int(t.shape[2])


def _volume_resample(reference, reference_mask, volume, volume_mask, index_map):
    mr, d, h, w = _volume("volume_resample", "reference", reference, reference_mask)
    mx, vd, vh, vw = _volume("volume_resample", "volume", volume, volume_mask)
    if volume.device != reference.device:
        raise RuntimeError("volume_resample: reference and volume must be on one device")
    if len(index_map) != 12:
        raise RuntimeError("volume_resample: index_map, the 12 entries of a (3, 4) matrix, expected")
    resampled = torch.empty_like(reference)
    valid = torch.empty(reference.shape, dtype=torch.bool, device=reference.device)
    stats = torch.empty(8, dtype=torch.float64, device=reference.device)
    M = (ctypes.c_double * 12)(*[float(v) for v in index_map])
    _launch("volume_resample", reference.device, (d, h, w), _lib.ptr(reference), _lib.ptr(mr), d, h, w, _lib.ptr(volume), _lib.ptr(mx),
            vd, vh, vw, M, _lib.ptr(resampled), _lib.ptr(valid), _lib.ptr(stats))
    return resampled, valid, stats


def _volume_ssim(reference, resampled, valid, params):
    _lib.require_device(params, dtype=torch.float32, name="volume_ssim params")
    m, d, h, w = _volume("volume_ssim", "reference", reference, valid)
    _lib.require_device(resampled, dtype=torch.float32, name="volume_ssim resampled")
    if m is None or resampled.shape != reference.shape:
        raise RuntimeError("volume_ssim: reference, resampled and valid (D, H, W) of one shape expected")
    if params.numel() != 4 or any(t.device != reference.device for t in (resampled, params)):
        raise RuntimeError("volume_ssim: params, four floats {a, b, c1, c2}, and resampled on the device of reference expected")
    ssim = torch.empty_like(reference)
    stats = torch.empty(4, dtype=torch.float64, device=reference.device)
    _launch("volume_ssim", reference.device, (d, h, w), _lib.ptr(reference), _lib.ptr(resampled), _lib.ptr(m), _lib.ptr(params), d, h, w,
            _lib.ptr(ssim), _lib.ptr(stats))
    return ssim, stats


_op("volume_resample(Tensor reference, Tensor? reference_mask, Tensor volume, Tensor? volume_mask, float[] index_map) -> "
    "(Tensor resampled, Tensor valid, Tensor stats)",
    _volume_resample,
    fake=lambda reference, reference_mask, volume, volume_mask, index_map: (
        torch.empty_like(reference), reference.new_empty(reference.shape, dtype=torch.bool), reference.new_empty((8,), dtype=torch.float64)))
_op("volume_ssim(Tensor reference, Tensor resampled, Tensor valid, Tensor params) -> (Tensor ssim, Tensor stats)", _volume_ssim,
    fake=lambda reference, resampled, valid, params: (torch.empty_like(reference), reference.new_empty((4,), dtype=torch.float64)))

EVALUATE_POSE_CHUNK = 1024  # voxels per workgroup of volume_pose_moments (kPoseChunk of csrc/evaluate.hip): four per thread
EVALUATE_MAX_POSES = 16  # index maps per call (they travel as kernel arguments)


def _volume_pose_moments(reference, reference_mask, volume, volume_mask, index_maps):
    mr, d, h, w = _volume("volume_pose_moments", "reference", reference, reference_mask)
    mx, vd, vh, vw = _volume("volume_pose_moments", "volume", volume, volume_mask)
    if volume.device != reference.device:
        raise RuntimeError("volume_pose_moments: reference and volume must be on one device")
    K, rest = divmod(len(index_maps), 12)
    if rest or K > EVALUATE_MAX_POSES:
        raise RuntimeError(f"volume_pose_moments: index_maps, the 12 entries of up to {EVALUATE_MAX_POSES} (3, 4) matrices, expected")
    sums = torch.empty((K, 6), dtype=torch.float64, device=reference.device)
    M = (ctypes.c_double * max(12 * K, 1))(*[float(v) for v in index_maps])
    _launch("volume_pose_moments", reference.device, (d, h, w, K), _lib.ptr(reference), _lib.ptr(mr), d, h, w, _lib.ptr(volume),
            _lib.ptr(mx), vd, vh, vw, M, K, _lib.ptr(sums))
    return sums


_op("volume_pose_moments(Tensor reference, Tensor? reference_mask, Tensor volume, Tensor? volume_mask, float[] index_maps) -> Tensor",
    _volume_pose_moments,
    fake=lambda reference, reference_mask, volume, volume_mask, index_maps: reference.new_empty((len(index_maps) // 12, 6),
                                                                                                dtype=torch.float64))


# =====================================================================================================================
# slice bias fields of the classical reconstruction (csrc/slice_bias.hip): one round of the smoothed log-ratio of scale_k y to
# sim - b_new on every pixel and the five per-slice sums - in two passes; the definition, the centring of a field and the rule
# for slices of little weight are nesvor_amd/slice_bias.py
# =====================================================================================================================
def _slice_bias_update(sim, y, mask, scale, weight, b, sigma_px, min_intensity):
    from .slice_bias import window_radius

    _lib.require_device(sim, y, scale, b, dtype=torch.float32, name="slice_bias_update sim/y/scale/b")
    stacks = {"sim": sim, "y": y, "b": b}
    if weight is not None:
        _lib.require_device(weight, dtype=torch.float32, name="slice_bias_update weight")
        stacks["weight"] = weight
    m, n, h, w = _slice_stack("slice_bias_update", stacks, mask, {"scale": scale})
    if scale.numel() != n:
        raise RuntimeError("slice_bias_update: scale (n) expected")
    radius = window_radius(sigma_px)  # (raises for a sigma_px that is not positive and finite)
    b_new = torch.empty_like(sim)
    stats = torch.empty((n, 5), dtype=torch.float64, device=sim.device)
    _launch("slice_bias_update", sim.device, (n, h, w), _lib.ptr(sim), _lib.ptr(y), _lib.ptr(m), _lib.ptr(scale), _lib.ptr(weight),
            _lib.ptr(b), n, h, w, float(sigma_px), radius, float(min_intensity), _lib.ptr(b_new), _lib.ptr(stats))
    return b_new, stats


_op("slice_bias_update(Tensor sim, Tensor y, Tensor? mask, Tensor scale, Tensor? weight, Tensor b, float sigma_px, "
    "float min_intensity) -> (Tensor b_new, Tensor stats)",
    _slice_bias_update,
    fake=lambda sim, y, mask, scale, weight, b, sigma_px, min_intensity: (torch.empty_like(sim),
                                                                          sim.new_empty((sim.shape[0], 5), dtype=torch.float64)))


# =====================================================================================================================
# stack denoising (csrc/denoise.hip): 2-D non-local means of every slice of a stack and the two per-slice sums in one pass;
# the definition, the noise estimate and the choice of the path are nesvor_amd/denoise.py
# =====================================================================================================================
def _nlm_denoise(y, mask, sigma, patch_radius, search_radius, strength):
    _lib.require_device(y, sigma, dtype=torch.float32, name="nlm_denoise y/sigma")
    m, n, h, w = _slice_stack("nlm_denoise", {"y": y}, mask, {"sigma": sigma})
    if sigma.numel() != n:
        raise RuntimeError("nlm_denoise: sigma (n) expected")
    out = torch.empty_like(y)
    stats = torch.empty((n, 2), dtype=torch.float64, device=y.device)
    _launch("nlm_denoise", y.device, (n, h, w), _lib.ptr(y), _lib.ptr(m), _lib.ptr(sigma), n, h, w, int(patch_radius), int(search_radius),
            float(strength), _lib.ptr(out), _lib.ptr(stats))
    return out, stats


_op("nlm_denoise(Tensor y, Tensor? mask, Tensor sigma, int patch_radius, int search_radius, float strength) -> (Tensor out, Tensor stats)",
    _nlm_denoise,
    fake=lambda y, mask, sigma, patch_radius, search_radius, strength: (torch.empty_like(y),
                                                                        y.new_empty((y.shape[0], 2), dtype=torch.float64)))


# =====================================================================================================================
# masked moments of slice pairs for the stack quality assessment (csrc/assess.hip): {count, sum a, sum b, sum a^2, sum b^2,
# sum a b} per pair over the pixels valid in both slices; the host logic (and the range check of the pair indices, which the
# kernel does not repeat) is nesvor_amd/assess.py
# =====================================================================================================================
def _pair_moments(slices, mask, pairs):
    _lib.require_device(slices, dtype=torch.float32, name="pair_moments slices")
    _lib.require_device(pairs, dtype=torch.int32, name="pair_moments pairs")
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise RuntimeError("pair_moments: pairs (P, 2) expected")
    m, n, h, w = _slice_stack("pair_moments", {"slices": slices}, mask, {"pairs": pairs})
    P = int(pairs.shape[0])
    moments = torch.empty((P, 6), dtype=torch.float64, device=slices.device)
    _launch("pair_moments", slices.device, (P, h, w), _lib.ptr(slices), _lib.ptr(m), n, h, w, _lib.ptr(pairs), P, _lib.ptr(moments))
    return moments


_op("pair_moments(Tensor slices, Tensor? mask, Tensor pairs) -> Tensor", _pair_moments,
    fake=lambda slices, mask, pairs: slices.new_empty((pairs.shape[0], 6), dtype=torch.float64))


# =====================================================================================================================
# the three per-iteration passes of the bias field correction (csrc/bias.hip) over a stack as a (D,H,W) array: the histogram
# of u = v - f, the B-spline lattice fitted to the residual, and f += the lattice's field with the statistics of the step; the
# host logic (tables, sharpening, levels, stop test) is nesvor_amd/bias.py
# =====================================================================================================================
def _n4_volume(what, v, f, mask):
    """The argument checks the three ops share; -> (mask or None, D, H, W)."""
    _lib.require_device(v, f, dtype=torch.float32, name=f"{what} v/f")
    m = _byte_mask(what, mask)
    if v.ndim != 3 or f.shape != v.shape or (m is not None and m.shape != v.shape):
        raise RuntimeError(f"{what}: v, f and mask (D, H, W) of one shape expected")
    if f.device != v.device or (m is not None and m.device != v.device):
        raise RuntimeError(f"{what}: v, f and mask must be on one device")
    return m, int(v.shape[0]), int(v.shape[1]), int(v.shape[2])


def _n4_tables(what, v, tables, spans, S):
    """tz, ty, tx (n,4) fp32 and sz, sy, sx (n) int32 for the axes of v."""
    _lib.require_device(*tables, dtype=torch.float32, name=f"{what} basis tables")
    _lib.require_device(*spans, dtype=torch.int32, name=f"{what} span tables")
    for n, t, s in zip(v.shape, tables, spans):
        if tuple(t.shape) != (n, 4) or tuple(s.shape) != (n,):
            raise RuntimeError(f"{what}: per axis a basis table (n, 4) and a span table (n) expected")
        if t.device != v.device or s.device != v.device:
            raise RuntimeError(f"{what}: the tables must be on the device of v")
    if S < 1 or S + 3 > 16:
        raise RuntimeError(f"{what}: S spans with 1 <= S and S + 3 <= 16 control points per axis expected, got S = {S}")


def _n4_range(what, v, rng, n_bins):
    _lib.require_device(rng, dtype=torch.float32, name=f"{what} range")
    if rng.numel() != 2 or rng.device != v.device:
        raise RuntimeError(f"{what}: range, two floats {{lo, hi}} on the device of v, expected")
    _n_bins(what, n_bins)


def _n4_histogram(v, f, mask, rng, n_bins):
    m, D, H, W = _n4_volume("n4_histogram", v, f, mask)
    _n4_range("n4_histogram", v, rng, n_bins)
    hist = torch.empty(n_bins, dtype=torch.float64, device=v.device)
    _launch("n4_histogram", v.device, (D, H, W, n_bins), _lib.ptr(v), _lib.ptr(f), _lib.ptr(m), D, H, W, _lib.ptr(rng), n_bins,
            _lib.ptr(hist))
    return hist


def _n4_fit(v, f, mask, rng, lut, tz, ty, tx, sz, sy, sx, S):
    m, D, H, W = _n4_volume("n4_fit", v, f, mask)
    _lib.require_device(lut, dtype=torch.float64, name="n4_fit lut")
    if lut.ndim != 1 or lut.device != v.device:
        raise RuntimeError("n4_fit: lut (n_bins) on the device of v expected")
    n_bins = int(lut.shape[0])
    _n4_range("n4_fit", v, rng, n_bins)
    _n4_tables("n4_fit", v, (tz, ty, tx), (sz, sy, sx), S)
    C = S + 3
    lattice = torch.empty((C, C, C), dtype=torch.float64, device=v.device)
    weight = torch.empty((C, C, C), dtype=torch.float64, device=v.device)
    _launch("n4_fit", v.device, (D, H, W, S), _lib.ptr(v), _lib.ptr(f), _lib.ptr(m), _lib.ptr(rng), _lib.ptr(lut), n_bins, _lib.ptr(tz),
            _lib.ptr(ty), _lib.ptr(tx), _lib.ptr(sz), _lib.ptr(sy), _lib.ptr(sx), D, H, W, S, _lib.ptr(lattice), _lib.ptr(weight))
    return lattice, weight


def _n4_update(lattice, tz, ty, tx, sz, sy, sx, S, f, v, mask):
    m, D, H, W = _n4_volume("n4_update_", v, f, mask)
    _n4_tables("n4_update_", v, (tz, ty, tx), (sz, sy, sx), S)
    _lib.require_device(lattice, dtype=torch.float64, name="n4_update_ lattice")
    if tuple(lattice.shape) != (S + 3,) * 3 or lattice.device != v.device:
        raise RuntimeError("n4_update_: lattice (C, C, C) with C = S + 3 on the device of v expected")
    stats = torch.empty(5, dtype=torch.float64, device=v.device)
    _launch("n4_update", v.device, (D, H, W), _lib.ptr(lattice), _lib.ptr(tz), _lib.ptr(ty), _lib.ptr(tx), _lib.ptr(sz), _lib.ptr(sy),
            _lib.ptr(sx), S, _lib.ptr(f), _lib.ptr(v), _lib.ptr(m), D, H, W, _lib.ptr(stats))
    return stats


_op("n4_histogram(Tensor v, Tensor f, Tensor? mask, Tensor range, int n_bins) -> Tensor", _n4_histogram,
    fake=lambda v, f, mask, rng, n_bins: v.new_empty((n_bins,), dtype=torch.float64))
_op("n4_fit(Tensor v, Tensor f, Tensor? mask, Tensor range, Tensor lut, Tensor tz, Tensor ty, Tensor tx, Tensor sz, Tensor sy, Tensor sx, "
    "int S) -> (Tensor lattice, Tensor weight)", _n4_fit,
    fake=lambda v, f, mask, rng, lut, tz, ty, tx, sz, sy, sx, S: (v.new_empty((S + 3,) * 3, dtype=torch.float64),
                                                                 v.new_empty((S + 3,) * 3, dtype=torch.float64)))
# f += the lattice's field, in place; returns {count, sum g, sum g^2, min u_new, max u_new}
_op("n4_update_(Tensor lattice, Tensor tz, Tensor ty, Tensor tx, Tensor sz, Tensor sy, Tensor sx, int S, Tensor(a!) f, Tensor v, "
    "Tensor? mask) -> Tensor", _n4_update,
    fake=lambda lattice, tz, ty, tx, sz, sy, sx, S, f, v, mask: v.new_empty((5,), dtype=torch.float64))


# =====================================================================================================================
# stack masking (csrc/masking.hip): the per-voxel rules of one stack in one pass - intensity threshold, world-space mask
# volume, intersection with the other stacks' slabs - with the per-slice {count, min, max} of the kept intensities, and Otsu's
# threshold from an integer histogram without a host read; the definitions and the tables are nesvor_amd/masking.py
# =====================================================================================================================
def _f64(what, t, numel, like):
    _lib.require_device(t, dtype=torch.float64, name=what)
    if t.numel() != numel or t.device != like.device:
        raise RuntimeError(f"{what}: {numel} doubles on the device of slices expected")


def _stack_mask(slices, mask, transforms, resolution_x, resolution_y, threshold=None, volume=None, volume_geometry=None, slabs=None,
                slab_extents=None, slab_offsets=None):
    _lib.require_device(slices, transforms, threshold, dtype=torch.float32, name="stack_mask slices/transforms/threshold")
    m, n, h, w = _slice_stack("stack_mask", {"slices": slices}, mask, {"transforms": transforms})
    if tuple(transforms.shape) != (n, 3, 4):
        raise RuntimeError("stack_mask: transforms (n, 3, 4) expected")
    if threshold is not None and (threshold.numel() != 1 or threshold.device != slices.device):
        raise RuntimeError("stack_mask: threshold, one float on the device of slices, expected")
    vd = vh = vw = 0
    if volume is not None:
        if volume.dtype not in (torch.bool, torch.uint8) or volume.ndim != 3:
            raise RuntimeError("stack_mask: volume (D, H, W) of torch.bool or torch.uint8 expected")
        _lib.require_device(volume, name="stack_mask volume")
        if volume.device != slices.device or volume_geometry is None:
            raise RuntimeError("stack_mask: volume on the device of slices, with volume_geometry, expected")
        _f64("stack_mask volume_geometry", volume_geometry, 15, slices)
        vd, vh, vw = (int(s) for s in volume.shape)
    n_others = n_slabs = 0
    if slab_offsets is not None and slab_offsets.numel() > 1:
        if slabs is None or slab_extents is None:
            raise RuntimeError("stack_mask: slabs, slab_extents and slab_offsets go together")
        _lib.require_device(slab_offsets, dtype=torch.int32, name="stack_mask slab_offsets")
        n_others = int(slab_offsets.numel()) - 1
        if slabs.ndim != 3 or tuple(slabs.shape[1:]) != (3, 4) or slab_offsets.device != slices.device:
            raise RuntimeError("stack_mask: slabs (n_slabs, 3, 4) and slab_offsets on the device of slices expected")
        n_slabs = int(slabs.shape[0])
        _f64("stack_mask slabs", slabs, 12 * n_slabs, slices)
        _f64("stack_mask slab_extents", slab_extents, 3 * n_others, slices)
    out = torch.empty(slices.shape, dtype=torch.uint8, device=slices.device)
    stats = torch.empty((n, 3), dtype=torch.float64, device=slices.device)
    _launch("stack_mask", slices.device, (n, h, w), _lib.ptr(slices), _lib.ptr(m), _lib.ptr(transforms), n, h, w, float(resolution_x),
            float(resolution_y), _lib.ptr(threshold), _lib.ptr(volume), vd, vh, vw,
            _lib.ptr(volume_geometry if volume is not None else None), _lib.ptr(slabs if n_others else None),
            _lib.ptr(slab_extents if n_others else None), _lib.ptr(slab_offsets if n_others else None), n_others, n_slabs, _lib.ptr(out),
            _lib.ptr(stats))
    return out, stats


def _otsu_range(what, slices, rng, n_bins):
    _f64(f"{what} range", rng, 2, slices)
    _n_bins(what, n_bins)


def _otsu_histogram(slices, mask, rng, n_bins):
    _lib.require_device(slices, dtype=torch.float32, name="otsu_histogram slices")
    m, n, h, w = _slice_stack("otsu_histogram", {"slices": slices}, mask, {"range": rng})
    _otsu_range("otsu_histogram", slices, rng, n_bins)
    hist = torch.empty(n_bins, dtype=torch.int64, device=slices.device)
    _launch("otsu_histogram", slices.device, (n, h, w, n_bins), _lib.ptr(slices), _lib.ptr(m), n, h, w, _lib.ptr(rng), n_bins,
            _lib.ptr(hist))
    return hist


def _otsu_threshold(hist, rng):
    _lib.require_device(hist, dtype=torch.int64, name="otsu_threshold hist")
    if hist.ndim != 1:
        raise RuntimeError("otsu_threshold: hist (n_bins) expected")
    n_bins = int(hist.shape[0])
    _otsu_range("otsu_threshold", hist, rng, n_bins)
    out = torch.empty(1, dtype=torch.float32, device=hist.device)
    lib = _lib.load()
    with torch.cuda.device(hist.device):
        err = lib.nesvor_otsu_threshold(_lib.ptr(hist), _lib.ptr(rng), n_bins, _lib.ptr(out), None, 0, _lib.stream_ptr())
    _lib.check(err, "otsu threshold")
    return out


_op("stack_mask(Tensor slices, Tensor? mask, Tensor transforms, float resolution_x, float resolution_y, Tensor? threshold=None, "
    "Tensor? volume=None, Tensor? volume_geometry=None, Tensor? slabs=None, Tensor? slab_extents=None, Tensor? slab_offsets=None) "
    "-> (Tensor mask, Tensor stats)",
    _stack_mask,
    fake=lambda slices, mask, transforms, rx, ry, threshold=None, volume=None, vgeom=None, slabs=None, extents=None, offsets=None: (
        slices.new_empty(slices.shape, dtype=torch.uint8), slices.new_empty((slices.shape[0], 3), dtype=torch.float64)))
_op("otsu_histogram(Tensor slices, Tensor? mask, Tensor range, int n_bins) -> Tensor", _otsu_histogram,
    fake=lambda slices, mask, rng, n_bins: slices.new_empty((n_bins,), dtype=torch.int64))
_op("otsu_threshold(Tensor hist, Tensor range) -> Tensor", _otsu_threshold,
    fake=lambda hist, rng: hist.new_empty((1,), dtype=torch.float32))


# =====================================================================================================================
# multi-resolution hash-grid encoding (tinycudann.Encoding "HashGrid"; the scalars are its encoding_config)
# =====================================================================================================================
_SPECS = {}


def grid_spec(n_levels, n_features_per_level, log2_hashmap_size, base_resolution, per_level_scale) -> HashGridSpec:
    key = (int(n_levels), int(n_features_per_level), int(log2_hashmap_size), int(base_resolution), float(per_level_scale))
    if key not in _SPECS:
        _SPECS[key] = HashGridSpec(*key)
    return _SPECS[key]


def _hg_encode(u, table, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale, layout):
    return _enc.hashgrid_forward(grid_spec(n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale), u, table, layout)


def _hg_backward(u, table, dpe, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale, layout, need_input_grad, method):
    spec = grid_spec(n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale)
    grad_table, grad_u = _enc.hashgrid_backward(spec, u, table, dpe, None, need_input_grad, layout, method)
    return grad_table, grad_u if need_input_grad else _empty(u)


def _hg_accumulate(u, table, dpe, grad_table, n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale, layout, need_input_grad):
    spec = grid_spec(n_levels, n_features, log2_hashmap_size, base_resolution, per_level_scale)
    _, grad_u = _enc.hashgrid_backward(spec, u, table, dpe, grad_table, need_input_grad, layout)
    return grad_u if need_input_grad else _empty(u)


def _hg_setup(ctx, inputs, output):
    ctx.save_for_backward(inputs[0], inputs[1])
    ctx.cfg = inputs[2:]


def _hg_backward_formula(ctx, dpe):
    u, table = ctx.saved_tensors
    gt, gu = torch.ops.nesvor.hashgrid_encode_backward(u, table, dpe.contiguous(), *ctx.cfg, ctx.needs_input_grad[0], "owner")
    return (_opt(gu) if ctx.needs_input_grad[0] else None, gt if ctx.needs_input_grad[1] else None) + (None,) * 6


def _hg_out_shape(u, n_levels, n_features, layout):
    e = n_levels * n_features
    return (u.shape[0], e) if layout == _lib.LAYOUT_ROW_MAJOR else (e, u.shape[0])


_op("hashgrid_encode_backward(Tensor u, Tensor table, Tensor dpe, int n_levels, int n_features_per_level, int log2_hashmap_size, "
    "int base_resolution, float per_level_scale, int layout, bool need_input_grad, str method) -> (Tensor, Tensor)", _hg_backward,
    fake=lambda u, t, d, L, F, T, b, s, lay, need, m: (torch.empty_like(t), torch.empty_like(u) if need else u.new_empty(0)))
_op("hashgrid_encode_backward_(Tensor u, Tensor table, Tensor dpe, Tensor(a!) grad_table, int n_levels, int n_features_per_level, "
    "int log2_hashmap_size, int base_resolution, float per_level_scale, int layout, bool need_input_grad) -> Tensor", _hg_accumulate,
    fake=lambda u, t, d, g, L, F, T, b, s, lay, need: torch.empty_like(u) if need else u.new_empty(0))
_op("hashgrid_encode(Tensor u, Tensor table, int n_levels, int n_features_per_level, int log2_hashmap_size, int base_resolution, "
    "float per_level_scale, int layout) -> Tensor", _hg_encode,
    fake=lambda u, t, L, F, T, b, s, lay: u.new_empty(_hg_out_shape(u, L, F, lay)),
    backward=_hg_backward_formula, setup_context=_hg_setup)


# =====================================================================================================================
# fused MLP (build_network's Linear/ReLU stacks and tinycudann.Network): feature-major input rows + per-pixel features
# =====================================================================================================================
def _mlp_forward(xa, xb, weights, biases, b_row0, k_b, samples_per_pixel, operands, save):
    y, saved = _mlp.forward_raw(list(weights), list(biases), xa, xb, b_row0, k_b, samples_per_pixel, save, _operands(operands))
    return y, saved


def _operands(code: int):
    """int of the schema -> the `bf16` argument of the raw calls: -1 = the fp32 default, else an explicit mode constant."""
    return False if code < 0 else (True if code == _mlp.BF16 else code)


def _mlp_backward(xa, xb, dy, weights, biases, saved, b_row0, k_b, samples_per_pixel, operands, need_dxa, need_dxb):
    dxb = torch.empty((k_b, xb.shape[1]), dtype=torch.float32, device=xb.device) if need_dxb else None
    dxa, partial = _mlp.backward_raw(list(weights), list(biases), xa, xb, dy, list(saved), b_row0, k_b, samples_per_pixel, dxb,
                                     need_dxa, _operands(operands))
    return (dxa if dxa is not None else _empty(xb), dxb if dxb is not None else _empty(xb), partial)


def _mlp_setup(ctx, inputs, output):
    xa, xb, weights, biases, b_row0, k_b, S, operands, save = inputs
    ctx.n_layers = len(weights)
    ctx.has_xa = xa is not None
    ctx.save_for_backward(*([xa] if xa is not None else []), xb, *weights, *biases, *output[1])
    ctx.cfg = (b_row0, k_b, S, operands)
    ctx.set_materialize_grads(False)


def _mlp_backward_formula(ctx, dy, d_saved):
    if dy is None:
        return (None,) * 9
    t = list(ctx.saved_tensors)
    xa = t.pop(0) if ctx.has_xa else None
    xb = t.pop(0)
    n = ctx.n_layers
    weights, biases, saved = t[:n], t[n : 2 * n], t[2 * n :]
    if len(saved) != n - 1:
        raise RuntimeError("fused_mlp was called with save=False but a gradient is requested: pass save=True")
    b_row0, k_b, S, operands = ctx.cfg
    need_xa, need_xb = ctx.has_xa and ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    dxa, dxb, partial = torch.ops.nesvor.fused_mlp_backward(xa, xb, dy.contiguous(), weights, biases, saved, b_row0, k_b, S, operands,
                                                            need_xa, need_xb)
    g_xb = None
    if need_xb:  # the kernel produced rows [b_row0, b_row0 + k_b) of the input gradient; the other rows get none
        g_xb = torch.zeros_like(xb)
        g_xb[b_row0 : b_row0 + k_b] = dxb
    g_xa = dxa.view(xa.shape[0], -1, dxa.shape[1]).sum(1) if need_xa else None
    flat = partial.sum(0)
    gw, gb, off = [], [], 0
    for w, b in zip(weights, biases):
        gw.append(flat[off : off + w.numel()].view_as(w))
        off += w.numel()
        gb.append(flat[off : off + b.numel()].view_as(b))
        off += b.numel()
    return g_xa, g_xb, gw, gb, None, None, None, None, None


def _mlp_fake(xa, xb, weights, biases, b_row0, k_b, S, operands, save):
    # the saved buffers' sizes follow from SHAPE fields alone (csrc/mlp.hip::compact_ok reads n_hidden, k_a, k_b, b_row0,
    # out_dim, samples_per_pixel, the operand mode and N through fill_args - no pointer of the descriptor), so this
    # pointer-less descriptor and forward_raw's real one always agree (tests/test_cabi.py::test_mlp_fake_sizes_match_forward)
    n = xb.shape[1]
    n_pad = (n + 15) // 16 * 16
    sdt = {_mlp.BF16: torch.bfloat16, _mlp.FP16: torch.float16}.get(operands, torch.float32)
    saved = []
    if save:
        d = _mlp.dims_desc(len(weights) - 1, weights[-1].shape[0], 0 if xa is None else xa.shape[1], k_b, b_row0, S, _operands(operands))
        saved = [xb.new_empty(m, dtype=sdt) for m in _mlp.saved_sizes(d, n, len(weights) - 1)]
    return xb.new_empty((weights[-1].shape[0], n)), saved


_op("fused_mlp_backward(Tensor? xa, Tensor xb, Tensor dy, Tensor[] weights, Tensor[] biases, Tensor[] saved, int b_row0, int k_b, "
    "int samples_per_pixel, int operands, bool need_dxa, bool need_dxb) -> (Tensor, Tensor, Tensor)", _mlp_backward)
_op("fused_mlp(Tensor? xa, Tensor xb, Tensor[] weights, Tensor[] biases, int b_row0, int k_b, int samples_per_pixel, int operands, "
    "bool save) -> (Tensor, Tensor[])", _mlp_forward, fake=_mlp_fake, backward=_mlp_backward_formula, setup_context=_mlp_setup)


# ---- the same networks at width <= 256 / up to seven hidden layers (csrc/mlp_wide.hip); `biases` empty = bias-free
def _wide_forward(xa, xb, weights, biases, b_row0, k_b, samples_per_pixel, save):
    return _mlp.wide_forward_raw(list(weights), list(biases), xa, xb, b_row0, k_b, samples_per_pixel, save)


def _wide_backward(xa, xb, dy, weights, biases, saved, b_row0, k_b, samples_per_pixel, need_dxa, need_dxb):
    dxb = torch.empty((k_b, xb.shape[1]), dtype=torch.float32, device=xb.device) if need_dxb else None
    dxa, partial = _mlp.wide_backward_raw(list(weights), list(biases), xa, xb, dy, list(saved), b_row0, k_b, samples_per_pixel, dxb, need_dxa)
    return (dxa if dxa is not None else _empty(xb), dxb if dxb is not None else _empty(xb), partial)


def _wide_setup(ctx, inputs, output):
    xa, xb, weights, biases, b_row0, k_b, S, save = inputs
    ctx.n_layers, ctx.n_bias = len(weights), len(biases)
    ctx.has_xa = xa is not None
    ctx.save_for_backward(*([xa] if xa is not None else []), xb, *weights, *biases, *output[1])
    ctx.cfg = (b_row0, k_b, S)
    ctx.set_materialize_grads(False)


def _wide_backward_formula(ctx, dy, d_saved):
    if dy is None:
        return (None,) * 8
    t = list(ctx.saved_tensors)
    xa = t.pop(0) if ctx.has_xa else None
    xb = t.pop(0)
    n, nb = ctx.n_layers, ctx.n_bias
    weights, biases, saved = t[:n], t[n : n + nb], t[n + nb :]
    if len(saved) != n - 1:
        raise RuntimeError("wide_mlp was called with save=False but a gradient is requested: pass save=True")
    b_row0, k_b, S = ctx.cfg
    need_xa, need_xb = ctx.has_xa and ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    dxa, dxb, partial = torch.ops.nesvor.wide_mlp_backward(xa, xb, dy.contiguous(), weights, biases, saved, b_row0, k_b, S, need_xa, need_xb)
    g_xb = None
    if need_xb:
        g_xb = torch.zeros_like(xb)
        g_xb[b_row0 : b_row0 + k_b] = dxb
    g_xa = dxa.view(xa.shape[0], -1, dxa.shape[1]).sum(1) if need_xa else None
    flat = partial.sum(0)
    gw, gb, off = [], [], 0
    for i, w in enumerate(weights):
        gw.append(flat[off : off + w.numel()].view_as(w))
        off += w.numel()
        if nb:
            gb.append(flat[off : off + biases[i].numel()].view_as(biases[i]))
            off += biases[i].numel()
    return g_xa, g_xb, gw, gb, None, None, None, None


def _wide_fake(xa, xb, weights, biases, b_row0, k_b, S, save):
    n = xb.shape[1]
    n_pad = (n + 15) // 16 * 16
    hb = 4 if weights[0].shape[0] <= 64 else 8 if weights[0].shape[0] <= 128 else 16
    saved = [xb.new_empty(n_pad * 16 * hb) for _ in range(len(weights) - 1)] if save else []
    return xb.new_empty((weights[-1].shape[0], n)), saved


_op("wide_mlp_backward(Tensor? xa, Tensor xb, Tensor dy, Tensor[] weights, Tensor[] biases, Tensor[] saved, int b_row0, int k_b, "
    "int samples_per_pixel, bool need_dxa, bool need_dxb) -> (Tensor, Tensor, Tensor)", _wide_backward)
_op("wide_mlp(Tensor? xa, Tensor xb, Tensor[] weights, Tensor[] biases, int b_row0, int k_b, int samples_per_pixel, bool save) -> "
    "(Tensor, Tensor[])", _wide_forward, fake=_wide_fake, backward=_wide_backward_formula, setup_context=_wide_setup)


# =====================================================================================================================
# PSF sampling + rigid transform + box normalisation (models.py:267-278, transform.py:259-280, models.py:143)
# =====================================================================================================================
def _psf_fwd(mat, slice_idx, xyz, psf_sigma, noise, bounding_box):
    return _sampler.forward_raw(mat, slice_idx, xyz, psf_sigma, noise, bounding_box)


def _psf_bwd(mat, slice_idx, xyz, psf_sigma, noise, bounding_box, dx, du):
    return _sampler.backward_raw(mat, slice_idx, xyz, psf_sigma, noise, bounding_box, dx, du)


def _psf_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)
    ctx.set_materialize_grads(False)


def _psf_backward_formula(ctx, dx, du):
    mat, slice_idx, xyz, psf_sigma, noise, bb = ctx.saved_tensors
    if not ctx.needs_input_grad[0] or (dx is None and du is None):
        return (None,) * 6
    dpix = torch.ops.nesvor.psf_transform_backward(mat, slice_idx, xyz, psf_sigma, noise, bb,
                                                   None if dx is None else dx.contiguous(), None if du is None else du.contiguous())
    return torch.zeros_like(mat).index_add_(0, slice_idx, dpix), None, None, None, None, None


_op("psf_transform_backward(Tensor mat, Tensor slice_idx, Tensor xyz, Tensor psf_sigma, Tensor noise, Tensor bounding_box, "
    "Tensor? dx, Tensor? du) -> Tensor", _psf_bwd,
    fake=lambda mat, idx, xyz, sig, noise, bb, dx, du: noise.new_empty((noise.shape[0], 3, 4)))
_op("psf_transform(Tensor mat, Tensor slice_idx, Tensor xyz, Tensor psf_sigma, Tensor noise, Tensor bounding_box) -> (Tensor, Tensor)",
    _psf_fwd, fake=lambda mat, idx, xyz, sig, noise, bb: (torch.empty_like(noise), noise.new_empty((noise.shape[0] * noise.shape[1], 3))),
    backward=_psf_backward_formula, setup_context=_psf_setup)


# =====================================================================================================================
# imaging model + losses (models.py:286-325, 366-384): values, and all input gradients in one launch
# =====================================================================================================================
def _loss_forward(z0, log_var, log_bias, x, v, slice_idx, c, log_var_slice, reg_type, delta):
    _lib.require_device(z0, log_var, log_bias, x, v, c, log_var_slice, dtype=torch.float32, name="imaging loss input")
    _lib.require_device(slice_idx, dtype=torch.int64, name="slice_idx")
    B, S = x.shape[0], x.shape[1]
    lb_mean = log_bias.mean().reshape(1) if log_bias is not None else torch.zeros(1, dtype=torch.float32, device=x.device)
    if log_bias is not None:
        from . import ddp

        if ddp.active():  # biasReg = (mean log_bias)^2 is not a mean of per-sample terms (models.py:322-323): take the GLOBAL
            # mean, so that value and averaged gradients are those of the undivided batch (as nesvor_amd.direct does)
            torch.distributed.all_reduce(lb_mean)
            lb_mean /= torch.distributed.get_world_size()
    loss_pix = torch.empty((B, 3), dtype=torch.float32, device=x.device)
    a = _loss._fill(z0, log_var, log_bias, x, v, slice_idx, c, log_var_slice, lb_mean if log_bias is not None else None, reg_type, delta)
    a.loss_pix = loss_pix.data_ptr()
    with torch.cuda.device(x.device), _lib.kernel_timer.span("imaging_loss_fwd"):
        err = _lib.load().nesvor_imaging_loss(ctypes.byref(a), _lib.stream_ptr())
    _lib.check(err, "imaging loss forward")
    sums = loss_pix.sum(0)
    mean_term = sums[2] / (B * S)
    ireg = delta * (mean_term - 1) if reg_type == 0 else mean_term
    return sums[0] / B, sums[1] / B, ireg, lb_mean[0] ** 2, lb_mean


def _loss_backward(z0, log_var, log_bias, x, v, slice_idx, c, log_var_slice, lb_mean, gw, reg_type, delta, need_dx):
    dev, B = x.device, x.shape[0]
    dz0 = torch.empty_like(z0)
    dlv = torch.empty_like(log_var) if log_var is not None else None
    dlb = torch.empty_like(log_bias) if log_bias is not None else None
    dx = torch.empty_like(x) if need_dx else None
    dc_pix = torch.empty(B, dtype=torch.float32, device=dev) if c is not None else None
    dlvs_pix = torch.empty(B, dtype=torch.float32, device=dev) if log_var_slice is not None else None
    a = _loss._fill(z0, log_var, log_bias, x, v, slice_idx, c, log_var_slice, lb_mean if log_bias is not None else None, reg_type, delta)
    a.gw = gw.data_ptr()
    for name, t in (("dz0", dz0), ("dlog_var", dlv), ("dlog_bias", dlb), ("dx", dx), ("dc_pix", dc_pix), ("dlvs_pix", dlvs_pix)):
        setattr(a, name, None if t is None else t.data_ptr())
    with torch.cuda.device(dev), _lib.kernel_timer.span("imaging_loss_bwd"):
        err = _lib.load().nesvor_imaging_loss(ctypes.byref(a), _lib.stream_ptr())
    _lib.check(err, "imaging loss backward")
    dc = torch.zeros_like(c).index_add_(0, slice_idx, dc_pix) if c is not None else _empty(x)
    dlvs = torch.zeros_like(log_var_slice).index_add_(0, slice_idx, dlvs_pix) if log_var_slice is not None else _empty(x)
    # (a fresh empty tensor per absent output: custom-op outputs must not alias each other)
    return (dz0, dlv if dlv is not None else _empty(x), dlb if dlb is not None else _empty(x),
            dx if dx is not None else _empty(x), dc, dlvs)


def _loss_setup(ctx, inputs, output):
    z0, log_var, log_bias, x, v, slice_idx, c, log_var_slice, reg_type, delta = inputs
    ctx.present = [t is not None for t in (log_var, log_bias, c, log_var_slice)]
    ctx.save_for_backward(z0, x, v, slice_idx, output[4], *[t for t in (log_var, log_bias, c, log_var_slice) if t is not None])
    ctx.cfg = (reg_type, delta)


def _loss_backward_formula(ctx, g_mse, g_logvar, g_ireg, g_breg, g_unused):
    z0, x, v, slice_idx, lb_mean, *rest = ctx.saved_tensors
    opt = [rest.pop(0) if p else None for p in ctx.present]
    log_var, log_bias, c, log_var_slice = opt
    gw = torch.stack([g_mse, g_logvar, g_ireg, g_breg]).to(torch.float32).contiguous()
    dz0, dlv, dlb, dx, dc, dlvs = torch.ops.nesvor.imaging_loss_backward(
        z0, log_var, log_bias, x, v, slice_idx, c, log_var_slice, lb_mean, gw, *ctx.cfg, ctx.needs_input_grad[3])
    return dz0, _opt(dlv), _opt(dlb), _opt(dx), None, None, _opt(dc), _opt(dlvs), None, None


_op("imaging_loss_backward(Tensor z0, Tensor? log_var, Tensor? log_bias, Tensor x, Tensor v, Tensor slice_idx, Tensor? c, "
    "Tensor? log_var_slice, Tensor log_bias_mean, Tensor gw, int reg_type, float delta, bool need_dx) -> "
    "(Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)", _loss_backward)
_op("imaging_loss(Tensor z0, Tensor? log_var, Tensor? log_bias, Tensor x, Tensor v, Tensor slice_idx, Tensor? c, "
    "Tensor? log_var_slice, int reg_type, float delta) -> (Tensor, Tensor, Tensor, Tensor, Tensor)", _loss_forward,
    fake=lambda z0, lv, lb, x, v, idx, c, lvs, r, d: tuple(x.new_empty(()) for _ in range(4)) + (x.new_empty(1),),
    backward=_loss_backward_formula, setup_context=_loss_setup)


# =====================================================================================================================
# AdamW + zero_grad over one flat buffer (train.py:144-152, 195-197)
# =====================================================================================================================
def _adamw_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, step, grad_scale, zero_grad):
    _lib.require_device(param, grad, exp_avg, exp_avg_sq, dtype=torch.float32, name="adamw buffers")
    with torch.cuda.device(param.device):
        err = _lib.load().nesvor_adamw_step(
            _lib.ptr(param), _lib.ptr(grad), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), param.numel(), lr, beta1, beta2, eps,
            weight_decay, 1 - beta1**step, 1 - beta2**step, grad_scale, int(bool(zero_grad)), _lib.stream_ptr())
    _lib.check(err, "adamw step")


_op("adamw_step_(Tensor(a!) param, Tensor(b!) grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, float lr, float beta1, float beta2, "
    "float eps, float weight_decay, int step, float grad_scale, bool zero_grad) -> ()", _adamw_step,
    fake=lambda *a: None)


# =====================================================================================================================
# the loss scaler of the fp16 mode on the device (train.py:161-164, 190-196; csrc/scaler.hip).  ``state``: the 32 bytes of
# nesvor_loss_scaler_t as an int32 tensor of LOSS_SCALER_WORDS elements (nesvor_amd.fused.LossScaler owns one per trainer)
# =====================================================================================================================
LOSS_SCALER_WORDS = ctypes.sizeof(_lib.LossScalerT) // 4


def _scaler_state(state):
    _lib.require_device(state, dtype=torch.int32, name="loss scaler state")
    if state.numel() != LOSS_SCALER_WORDS:
        raise RuntimeError(f"loss scaler state: {LOSS_SCALER_WORDS} int32 words (nesvor_loss_scaler_t), got {state.numel()}")
    return _lib.ptr(state)


def _grad_found_inf(grad, state):
    _lib.require_device(grad, dtype=torch.float32, name="gradient")
    s = _scaler_state(state)
    with torch.cuda.device(grad.device):
        err = _lib.load().nesvor_grad_found_inf(_lib.ptr(grad), grad.numel(), s, _lib.stream_ptr())
    _lib.check(err, "grad found_inf")


_op("grad_found_inf_(Tensor grad, Tensor(a!) state) -> ()", _grad_found_inf, fake=lambda *a: None)


def _adamw_step_scaled(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, world_size, zero_grad, state):
    _lib.require_device(param, grad, exp_avg, exp_avg_sq, dtype=torch.float32, name="adamw buffers")
    if any(t.data_ptr() % 16 for t in (param, grad, exp_avg, exp_avg_sq)):
        raise RuntimeError("adamw_step_scaled_: the buffers must be 16-byte aligned")
    s = _scaler_state(state)
    with torch.cuda.device(param.device):
        err = _lib.load().nesvor_adamw_step_scaled(
            _lib.ptr(param), _lib.ptr(grad), _lib.ptr(exp_avg), _lib.ptr(exp_avg_sq), param.numel(), lr, beta1, beta2, eps,
            weight_decay, int(world_size), int(bool(zero_grad)), s, _lib.stream_ptr())
    _lib.check(err, "adamw step (device loss scaler)")


_op("adamw_step_scaled_(Tensor(a!) param, Tensor(b!) grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, float lr, float beta1, "
    "float beta2, float eps, float weight_decay, int world_size, bool zero_grad, Tensor state) -> ()", _adamw_step_scaled,
    fake=lambda *a: None)


def _loss_scaler_update(state):
    s = _scaler_state(state)
    with torch.cuda.device(state.device):
        err = _lib.load().nesvor_loss_scaler_update(s, _lib.stream_ptr())
    _lib.check(err, "loss scaler update")


_op("loss_scaler_update_(Tensor(a!) state) -> ()", _loss_scaler_update, fake=lambda *a: None)


def op_names() -> List[str]:
    return sorted(SCHEMAS)
