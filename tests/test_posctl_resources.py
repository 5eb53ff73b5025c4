"""The position-mode kernels (robot_gym_amd/csrc/rg_posctl.hip) compile for gfx950 without scratch: one device-only
compile with the compiler's resource remarks (tests/kernel_checks.py; no GPU needed).  Parity rests on float64 values kept in
registers, and a one-lane-per-robot kernel that spills would pay for it on every tick."""
import pytest

from tests import kernel_checks

KERNELS = {"rg_posctl_bezier_kernel", "rg_posctl_pose_kernel", "rg_posctl_torque_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_posctl.hip")


def test_every_posctl_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_posctl_kernel_uses_scratch(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)
