"""CPU: the device loss scaler's C ABI (csrc/scaler.hip) - the ABI version, the exports and their ctypes signatures, the state struct
mirrored by ``_lib.LossScalerT`` - and the host form of ``fused.LossScaler`` that the device form is held to."""
import ctypes
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib_loaded():
    import __graft_entry__ as ge
    from nesvor_amd import _lib

    ge.build()
    return _lib, _lib.load()


def test_abi_version_is_38():
    _lib, lib = _lib_loaded()
    assert _lib.ABI_VERSION == 38 and lib.nesvor_hip_abi_version() == 38


def test_scaler_exports_resolve_with_their_argtypes():
    _lib, lib = _lib_loaded()
    P, i64, f, d, i = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_int
    want = {
        "nesvor_grad_found_inf": [P, i64, P, P],
        "nesvor_adamw_step_scaled": [P, P, P, P, i64, f, d, d, f, f, i, i, P, P],
        "nesvor_loss_scaler_update": [P, P],
        "nesvor_loss_scale_weights": [P, P, i, P, P],
        "nesvor_step_epilogue_scaled": [P] * 6 + [f, P, P, P, P, P, i, i, f, f, P],
    }
    for name, argtypes in want.items():
        fn = getattr(lib, name)
        assert fn.argtypes == argtypes, name
        assert fn.restype == ctypes.c_int, name
    # the old epilogue keeps its signature (the one-call step and every existing caller)
    assert lib.nesvor_step_epilogue.argtypes == [P] * 6 + [f, P, P, P, P, i, i, f, f, P]


def test_state_struct_mirrors_the_header():
    from nesvor_amd import _lib, ops

    text = open(os.path.join(ROOT, "include", "nesvor_hip.h")).read()
    body = re.search(r"typedef struct nesvor_loss_scaler_t \{(.*?)\} nesvor_loss_scaler_t;", text, re.S).group(1)
    names = re.findall(r"\b(\w+)\s*[,;]", re.sub(r"\b(float|int32_t|uint32_t)\b", "", body))
    assert names == [n for n, _ in _lib.LossScalerT._fields_]
    assert ctypes.sizeof(_lib.LossScalerT) == 32 and ops.LOSS_SCALER_WORDS == 8
    from nesvor_amd import fused

    assert fused._SCALER_FIELDS == tuple(names)


def test_scaler_ops_have_a_device_kernel_only():
    import nesvor_amd.ops as ops

    for name in ("grad_found_inf_", "adamw_step_scaled_", "loss_scaler_update_"):
        assert name in ops.op_names(), name
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f"nesvor::{name}", "CUDA")
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f"nesvor::{name}", "CPU")


def test_host_loss_scaler_is_gradscaler_update():
    """The reference implementation the device scaler is tested against: GradScaler.update semantics, host floats."""
    from nesvor_amd.fused import LossScaler

    s = LossScaler(growth_interval=3)
    assert not s.on_device and s.state_dict() == {"scale": 1.0, "growth_tracker": 0, "skipped": 0}
    for found in (False, False, False, True, False, False, False, False):
        s.update(found)
    assert s.scale == 2.0 and s.growth_tracker == 1 and s.skipped == 1
    s.scale = 2.0 ** 60
    s.update(True)
    assert s.scale == 2.0 ** 59 and s.growth_tracker == 0 and s.skipped == 2
