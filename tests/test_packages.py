"""Package registration, the parts that need no GPU: the assignment of slices to interleaved packages and its CSR, the command
line, the host composition and the centroid parametrisation, the op registry and the op's refusals of a bad grouping."""
import logging

import pytest
import torch

from nesvor_amd import cli, ops
from nesvor_amd.registration import centroid_corrections, compose_mats, package_groups
from nesvor_amd.transform import RigidTransform, mat_transform_points


# ---------------------------------------------------------------------------------------------------------------------
# assignment
# ---------------------------------------------------------------------------------------------------------------------
def _members(offsets, listed):
    return [listed[int(offsets[g]):int(offsets[g + 1])].tolist() for g in range(offsets.numel() - 1)]


def test_slices_go_to_k_mod_p_and_stacks_keep_their_own_groups():
    offsets, listed = package_groups([5, 4, 3], [2, 3, 1])
    assert offsets.dtype == torch.int32 and listed.dtype == torch.int32
    assert _members(offsets, listed) == [[0, 2, 4], [1, 3], [5, 8], [6], [7], [9, 10, 11]]
    assert _members(*package_groups([4, 4], [2])) == [[0, 2], [1, 3], [4, 6], [5, 7]]  # one count serves every stack


def test_empty_slices_are_dropped_after_the_assignment():
    # slices 2 and 7 are empty: the others keep the package of their place in the FILE and are renumbered in kept order
    keep = [0, 1, 3, 4, 5, 6, 8]
    offsets, listed = package_groups([5, 4], [2, 3], keep)
    assert _members(offsets, listed) == [[0, 3], [1, 2], [4, 6], [5], []]
    assert offsets.tolist() == [0, 2, 4, 6, 7, 7] and int(offsets[-1]) == listed.numel() == len(keep)


def test_package_counts_are_checked():
    with pytest.raises(ValueError, match="fewer than its 4 packages"):
        package_groups([5, 3], [2, 4])
    with pytest.raises(ValueError, match="at least 1"):
        package_groups([5, 3], [2, 0])
    with pytest.raises(ValueError, match="one count per stack"):
        package_groups([5, 3, 4], [2, 2])
    assert _members(*package_groups([3], [3])) == [[0], [1], [2]]  # as many packages as slices is allowed


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def _parse(command, *extra):
    base = {"register": ["--input-stacks", "a", "b", "c", "--output-slices", "d"],
            "svr": ["--input-stacks", "a", "b", "c", "--output-volume", "v"],
            "reconstruct": ["--input-stacks", "a", "b", "c", "--output-volume", "v"]}[command]
    return cli.build_parser().parse_args([command, *base, *extra])


@pytest.mark.parametrize("command", ["register", "svr", "reconstruct"])
def test_defaults_leave_packages_unset(command):
    args = _parse(command, "--registration", "svr")
    assert args.packages is None and args.package_rounds == 2
    assert cli.package_options(args, 3) is None


def test_packages_parse_per_stack_or_one_for_all():
    assert cli.package_options(_parse("register", "--registration", "svr", "--packages", "2"), 3) == [2, 2, 2]
    args = _parse("svr", "--packages", "2", "3", "4", "--package-rounds", "1")  # (svr registers with svr by default)
    assert cli.package_options(args, 3) == [2, 3, 4] and args.package_rounds == 1


def test_a_bad_count_or_p_ends_the_command_and_names_the_flag():
    with pytest.raises(SystemExit, match="--packages"):
        cli.package_options(_parse("register", "--registration", "svr", "--packages", "2", "2"), 3)
    with pytest.raises(SystemExit, match="--packages"):
        cli.package_options(_parse("register", "--registration", "svr", "--packages", "2", "0", "2"), 3)
    with pytest.raises(SystemExit, match="--package-rounds"):
        cli.package_options(_parse("register", "--registration", "svr", "--packages", "2", "--package-rounds", "-1"), 3)


@pytest.mark.parametrize("registration", ["stack", "none"])
def test_packages_are_ignored_with_a_warning_without_svr(registration, caplog):
    args = _parse("register", "--registration", registration, "--packages", "2")
    with caplog.at_level(logging.WARNING):
        assert cli.package_options(args, 3) is None
    assert "--packages" in caplog.text and f"--registration {registration}" in caplog.text


def test_packages_are_ignored_with_a_warning_with_input_slices(caplog):
    args = cli.build_parser().parse_args(["svr", "--input-slices", "dir", "--output-volume", "v", "--packages", "2"])
    with caplog.at_level(logging.WARNING):
        cli.warn_packages_ignored(args, "--input-slices")
    assert "--packages" in caplog.text and "--input-slices" in caplog.text
    caplog.clear()
    with caplog.at_level(logging.WARNING):  # nothing to say when the flags were not given
        cli.warn_packages_ignored(cli.build_parser().parse_args(["svr", "--input-slices", "dir", "--output-volume", "v"]), "--input-slices")
    assert caplog.text == ""


# ---------------------------------------------------------------------------------------------------------------------
# host composition, centroid parametrisation
# ---------------------------------------------------------------------------------------------------------------------
def _random_poses(n, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 6, generator=g, dtype=torch.float64) * torch.tensor([40.0, 40, 40, 10, 10, 10], dtype=torch.float64)
    return centroid_corrections(x, torch.zeros(n, 3, dtype=torch.float64))


def test_compose_mats_is_rigid_transform_compose_in_float64():
    a, b = _random_poses(50, 1), _random_poses(50, 2)
    want = RigidTransform(a).compose(RigidTransform(b)).matrix()
    got = compose_mats(a, b)
    assert got.dtype == torch.float64
    torch.testing.assert_close(got, want, rtol=0, atol=1e-13)  # (the same products; only the order of the adds may differ)
    eye = torch.eye(3, 4, dtype=torch.float64).expand(50, 3, 4)
    assert torch.equal(compose_mats(eye, b), b)  # identity corrections leave the base pose exactly
    assert torch.equal(compose_mats(a.float(), b.float()), compose_mats(a.float().double(), b.float().double()))  # fp32 inputs, double inside


def test_the_correction_is_a_rotation_about_the_centroid():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(20, 6, generator=g, dtype=torch.float64) * torch.tensor([30.0, 30, 30, 5, 5, 5], dtype=torch.float64)
    x[0, :3] = 0  # the small-angle branch
    c = torch.randn(20, 3, generator=g, dtype=torch.float64) * 40
    for voxel in (1.0, 2.0):
        m = centroid_corrections(x, c, voxel)
        R = m[..., :3]
        torch.testing.assert_close(R @ R.transpose(-2, -1), torch.eye(3, dtype=torch.float64).expand(20, 3, 3), rtol=0, atol=1e-14)
        torch.testing.assert_close(torch.linalg.det(R), torch.ones(20, dtype=torch.float64), rtol=0, atol=1e-14)
        # the centroid moves by d alone, whatever the rotation
        torch.testing.assert_close(mat_transform_points(m, c, True), c + x[:, 3:] / voxel, rtol=0, atol=1e-12)
        # and the rotation angle is |rotation vector| (degrees)
        angle = torch.rad2deg(torch.acos(((R.diagonal(dim1=-2, dim2=-1).sum(-1) - 1) / 2).clamp(-1, 1)))
        torch.testing.assert_close(angle, x[:, :3].norm(dim=-1), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------------------------------
def test_the_grouped_ops_are_registered_with_fake_implementations():
    from torch._subclasses.fake_tensor import FakeTensorMode

    for name in ("svr_similarity_groups", "svr_similarity_groups_bank"):
        assert name in ops.SCHEMAS and hasattr(torch.ops.nesvor, name)
    with FakeTensorMode():
        m = lambda *s: torch.empty(s)
        off, listed = torch.empty(4, dtype=torch.int32), torch.empty(7, dtype=torch.int32)
        out = torch.ops.nesvor.svr_similarity_groups(m(8, 9, 10), m(3, 3, 3), m(3, 13, 3, 4), m(7, 3, 4), off, listed, m(7, 11, 12), None, 1.5)
        assert out.shape == (3, 13, 6) and out.dtype == torch.float64
        out = torch.ops.nesvor.svr_similarity_groups_bank(m(8, 9, 10), m(54), torch.empty((2, 4), dtype=torch.int32),
                                                          torch.empty(7, dtype=torch.int32), m(3, 14, 3, 4), m(7, 3, 4), off, listed,
                                                          m(7, 11, 12), None, 1.5)
        assert out.shape == (3, 14, 6) and out.dtype == torch.float64


def _call(off, listed, n=7):
    """The op's backend function itself on host tensors: the grouping is checked first, before any device is asked for."""
    t = lambda v: torch.tensor(v, dtype=torch.int32)
    m = lambda *s: torch.zeros(s)
    return ops._svr_similarity_groups(m(8, 9, 10), m(3, 3, 3), m(len(off) - 1, 1, 3, 4), m(n, 3, 4), t(off), t(listed), m(n, 5, 6), None, 1.0)


@pytest.mark.parametrize("off,listed,what", [
    ([0, 2, 1], [0, 1], "must not decrease"),
    ([1, 1, 2], [0, 1], "start at 0"),
    ([0, 1, 3], [0, 1], "must equal len"),
    ([0, 1, 2], [0, -1], r"\[0, 7\)"),
    ([0, 1, 2], [0, 7], r"\[0, 7\)"),
])
def test_a_bad_grouping_is_refused_before_any_launch(off, listed, what):
    with pytest.raises(RuntimeError, match=what):
        _call(off, listed)
    with pytest.raises(RuntimeError, match=what):
        ops.check_grouping("svr_similarity_groups", torch.tensor(off), torch.tensor(listed), 7)


def test_a_good_grouping_passes_the_check_and_reaches_the_device_check():
    off, listed, G, E = ops.check_grouping("svr_similarity_groups", torch.tensor([0, 2, 2, 3]), torch.tensor([6, 0, 3]), 7)
    assert (G, E) == (3, 3) and off.dtype == listed.dtype == torch.int32
    with pytest.raises(Exception) as info:  # host tensors: refused by the device check that FOLLOWS the grouping's
        _call([0, 2, 2, 3], [6, 0, 3])
    assert "group_" not in str(info.value)
