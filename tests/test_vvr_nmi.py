"""The mutual-information similarity of the stack registration (``--stack-similarity nmi``), the parts that need no GPU: the command
line, the op registry, the loss name ``VVR`` accepts, what ``register_stacks`` / ``register_slices`` refuse, and the generic
evaluation path on the CPU."""
import logging
import os

import pytest
import torch

from nesvor_amd import _lib, cli, nmi, ops
from nesvor_amd.registration import VVR, _Level, register_slices, register_stacks

GD = {"name": "gd", "momentum": 0.1}
COMMANDS = ["register", "svr", "reconstruct"]


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def _parse(command, *extra):
    base = {"register": ["--input-stacks", "a", "b", "c", "--output-slices", "d"],
            "svr": ["--input-stacks", "a", "b", "c", "--output-volume", "v"],
            "reconstruct": ["--input-stacks", "a", "b", "c", "--output-volume", "v"]}[command]
    return cli.build_parser().parse_args([command, *base, *extra])


@pytest.mark.parametrize("command", COMMANDS)
def test_the_flag_parses_and_defaults_to_ncc(command):
    assert _parse(command).stack_similarity == "ncc"
    assert _parse(command, "--stack-similarity", "nmi").stack_similarity == "nmi"
    with pytest.raises(SystemExit):
        _parse(command, "--stack-similarity", "ssim")
    for registration in ("stack", "svr"):  # the default hands nothing down: today's path
        assert cli.similarity_options(_parse(command, "--registration", registration)) == {}


@pytest.mark.parametrize("command", COMMANDS)
def test_the_options_it_hands_to_the_registration(command):
    """``--registration stack``: the keywords of ``register_stacks``; ``--registration svr``: those of ``register_slices``, next to
    what ``--svr-similarity`` hands down; ``--nmi-bins`` serves both flags."""
    opt = lambda *extra: cli.similarity_options(_parse(command, *extra))
    assert opt("--registration", "stack", "--stack-similarity", "nmi") == {"similarity": "nmi", "nmi_bins": 32}
    assert opt("--registration", "stack", "--stack-similarity", "nmi", "--nmi-bins", "16") == {"similarity": "nmi", "nmi_bins": 16}
    assert opt("--registration", "svr", "--stack-similarity", "nmi") == {"stack_similarity": "nmi", "nmi_bins": 32}
    assert opt("--registration", "svr", "--stack-similarity", "nmi", "--svr-similarity", "nmi", "--nmi-bins", "8") == {
        "similarity": "nmi", "stack_similarity": "nmi", "nmi_bins": 8}
    assert opt("--registration", "svr", "--svr-similarity", "nmi") == {"similarity": "nmi", "nmi_bins": 32}  # (as before)


@pytest.mark.parametrize("registration", ["stack", "svr"])
@pytest.mark.parametrize("bins", ["1", "65", "0", "-4"])
def test_bins_outside_2_to_64_end_the_command_and_name_the_flag(registration, bins):
    with pytest.raises(SystemExit, match="--nmi-bins"):
        cli.similarity_options(_parse("register", "--registration", registration, "--stack-similarity", "nmi", "--nmi-bins", bins))


def test_nmi_bins_is_not_reported_ignored_when_the_stack_stage_uses_it(caplog):
    args = _parse("register", "--registration", "stack", "--stack-similarity", "nmi", "--nmi-bins", "16")
    with caplog.at_level(logging.WARNING):
        assert cli.similarity_options(args) == {"similarity": "nmi", "nmi_bins": 16}
    assert "--nmi-bins" not in caplog.text and caplog.text == ""
    caplog.clear()
    # --svr-similarity has nothing to act on with --registration stack: still said, without naming --nmi-bins
    args = _parse("register", "--registration", "stack", "--stack-similarity", "nmi", "--svr-similarity", "nmi")
    with caplog.at_level(logging.WARNING):
        assert cli.similarity_options(args) == {"similarity": "nmi", "nmi_bins": 32}
    assert "--svr-similarity" in caplog.text and "--nmi-bins" not in caplog.text


def test_what_the_svr_flags_did_at_the_default_stays(caplog):
    args = _parse("register", "--registration", "stack", "--svr-similarity", "nmi")
    with caplog.at_level(logging.WARNING):
        assert cli.similarity_options(args) == {}
    assert "--svr-similarity" in caplog.text and "--registration stack" in caplog.text and "--stack-similarity" not in caplog.text


def test_the_flag_is_ignored_with_a_warning_without_a_stack_registration(caplog):
    args = _parse("register", "--registration", "none", "--stack-similarity", "nmi")
    with caplog.at_level(logging.WARNING):
        assert cli.similarity_options(args) == {}
    assert "--stack-similarity" in caplog.text and "--registration none" in caplog.text
    caplog.clear()
    args = cli.build_parser().parse_args(["svr", "--input-slices", "dir", "--output-volume", "v", "--stack-similarity", "nmi"])
    with caplog.at_level(logging.WARNING):
        cli.warn_similarity_ignored(args, "--input-slices")
    assert "--stack-similarity" in caplog.text and "--input-slices" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.WARNING):  # nothing to say when the flag was not given
        cli.warn_similarity_ignored(cli.build_parser().parse_args(["svr", "--input-slices", "dir", "--output-volume", "v"]), "--input-slices")
    assert caplog.text == ""


def test_the_commands_document_the_flag():
    assert "--stack-similarity" in cli.__doc__
    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    assert "--stack-similarity" in readme


# ---------------------------------------------------------------------------------------------------------------------
# ops, C ABI table
# ---------------------------------------------------------------------------------------------------------------------
def test_the_ops_are_registered_with_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode

    for name in ("vvr_joint_histogram", "vvr_sample"):
        assert name in ops.SCHEMAS and name in ops.op_names() and hasattr(torch.ops.nesvor, name)
    with FakeTensorMode():
        m = lambda *s: torch.empty(s)
        out = torch.ops.nesvor.vvr_joint_histogram(m(1, 1, 8, 9, 10), m(77, 3), m(77), m(13, 3, 4), [0.1, 0.2, 0.3], 0.0, 31.0, 0.0, 31.0, 32)
        assert out.shape == (13, 32, 32) and out.dtype == torch.int64
        out = torch.ops.nesvor.vvr_sample(m(8, 9, 10), m(77, 3), m(13, 3, 4), [0.1, 0.2, 0.3])
        assert out.shape == (13, 77) and out.dtype == torch.float32


def test_the_entry_points_are_in_the_signature_table():
    for name in ("nesvor_vvr_joint_histogram", "nesvor_vvr_joint_histogram_workspace_bytes", "nesvor_vvr_sample"):
        assert name in _lib.exported_symbols()


def test_host_tensors_are_refused_by_the_op_backends():
    m = lambda *s: torch.zeros(s)
    with pytest.raises(RuntimeError, match="device"):
        ops._vvr_joint_histogram(m(8, 9, 10), m(5, 3), m(5), m(2, 3, 4), [1.0, 1.0, 1.0], 0.0, 1.0, 0.0, 1.0, 32)
    with pytest.raises(RuntimeError, match="device"):
        ops._vvr_sample(m(8, 9, 10), m(5, 3), m(2, 3, 4), [1.0, 1.0, 1.0])


# ---------------------------------------------------------------------------------------------------------------------
# registration
# ---------------------------------------------------------------------------------------------------------------------
def test_nmi_is_a_loss_name_of_vvr():
    assert VVR(2, 2, 2, 5, GD, {"name": "nmi"}, False)._bins == 32
    assert VVR(2, 2, 2, 5, GD, {"name": "nmi", "bins": 8}, False)._bins == 8
    for bins in (1, 65, 2.5):
        with pytest.raises(ValueError, match="bins"):
            VVR(2, 2, 2, 5, GD, {"name": "nmi", "bins": bins}, False)
    with pytest.raises(Exception, match="unknown loss"):
        VVR(2, 2, 2, 5, GD, {"name": "nmi", "eps": 1e-6}, False)
    with pytest.raises(ValueError, match="auto_grad"):
        VVR(2, 2, 2, 5, GD, {"name": "nmi"}, True)


def test_unknown_similarities_and_bad_bins_are_refused_before_any_work():
    with pytest.raises(ValueError, match="similarity"):
        register_stacks([], similarity="ssim")
    with pytest.raises(ValueError, match="nmi_bins"):
        register_stacks([], similarity="nmi", nmi_bins=65)
    with pytest.raises(ValueError, match="stack_similarity"):
        register_slices([], stack_similarity="ssim")
    with pytest.raises(ValueError, match="nmi_bins"):
        register_slices([], stack_similarity="nmi", nmi_bins=1)


def test_the_generic_path_on_the_cpu(oracle_backend):
    """``VVR._objective`` on a hand-made level, two poses as a batch: the loss is ``nmi_loss`` of the histogram the definition gives
    for the warped samples, over ALL points (total 65536 M), with the level's maps cached on the level."""
    from nesvor_amd.transform import RigidTransform

    g = torch.Generator().manual_seed(3)
    source = torch.rand((1, 1, 6, 7, 8), generator=g)
    target = torch.rand((1, 1, 6, 7, 8), generator=g) * (torch.rand((1, 1, 6, 7, 8), generator=g) < 0.8)
    lv = _Level(source, target, 1.5)
    M = int((target > 0).sum())
    assert lv.values.numel() == M and lv.i_map is None and lv.j_map is None
    vvr = VVR(1, 1, 1, 1, GD, {"name": "nmi", "bins": 8}, False)
    vvr.theta_t, vvr.trans_first = RigidTransform(torch.zeros(1, 6)), True
    theta = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [5.0, -3.0, 8.0, 2.0, -1.0, 4.0]])  # degrees, mm
    assert not vvr._fused(theta[:1], lv)
    loss = vvr._objective(theta, lv)
    assert lv.i_map == tuple(nmi.axis_map(source.min(), source.max(), 8).tolist())
    assert lv.j_map == tuple(nmi.axis_map(lv.values.min(), lv.values.max(), 8).tolist())
    warped = vvr._warp(theta, lv)
    J = lv.values[None].expand(2, -1)
    hist = nmi.joint_histogram(warped, J, torch.ones_like(J, dtype=torch.bool), lv.i_map, torch.tensor([lv.j_map, lv.j_map]), 8)
    assert hist.sum((1, 2)).tolist() == [nmi.UNITS * M] * 2
    assert torch.equal(loss, nmi.nmi_loss(hist).float()) and loss.shape == (2,) and bool((loss < 0).all())
    assert float(loss[0]) != float(loss[1])
    # the finite-difference gradient and the accept test run on it
    l0, grad = vvr._gradient(theta[1:], lv, 1.0)
    assert torch.equal(l0, loss[1:]) and grad.shape == (1, 6) and bool(grad.abs().sum() > 0)
    # an empty point list: zeros, loss 0, J map (0, 0)
    empty = _Level(source, torch.zeros_like(target), 1.5)
    assert vvr._objective(theta, empty).tolist() == [0.0, 0.0] and empty.j_map == (0.0, 0.0)
