"""The go-to-target kernels (robot_gym_amd/csrc/rg_goto.hip) compile for gfx950 without scratch and within their LDS budget:
one device-only compile with the compiler's resource remarks (tests/kernel_checks.py; no GPU needed).  The source must stay
clear of what the kernels have no business with (atomics, inline assembly)."""
import os
import re

import pytest

from tests import kernel_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
KERNELS = {"rg_goto_post_kernel", "rg_goto_pre_kernel", "rg_goto_set_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_goto.hip")


def test_every_goto_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_goto_kernel_uses_scratch(remarks):
    kernel_checks.assert_lean(remarks, KERNELS)


# The tick kernel's budget: five arrays of RG_GOTO_MAX_VISIBLE float64 (visible x / y; chain x / y / cumulative length).
LDS_BUDGET = {"rg_goto_post_kernel": 5 * 128 * 8, "rg_goto_pre_kernel": 0, "rg_goto_set_kernel": 0}


def test_lds_is_within_the_budget(remarks):
    for name, budget in LDS_BUDGET.items():
        assert int(remarks[name]["LDS Size [bytes/block]"]) <= budget, (name, remarks[name])
    header = open(os.path.join(ROOT, "include", "rg_goto.h")).read()
    assert int(re.search(r"#define RG_GOTO_MAX_VISIBLE (\d+)", header).group(1)) == 128


# What the device-only compile reports today (upper bounds).  The tick kernel is one wave per workgroup; at 71 VGPRs seven
# waves fit a SIMD, and at 4096 robots the 4096 waves spread over 1024 SIMDs, four each.
REGISTERS = {"rg_goto_post_kernel": dict(vgprs=71, occupancy=7), "rg_goto_pre_kernel": dict(vgprs=27, occupancy=8),
             "rg_goto_set_kernel": dict(vgprs=12, occupancy=8)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)     # no agprs in the table: none allowed


def test_source_has_no_inline_assembly_no_atomics_and_contraction_off():
    src = open(os.path.join(SRC, "rg_goto.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in src.lower()
    assert code.index("#pragma clang fp contract(off)") < code.index("__global__")
    assert "__launch_bounds__(kWave)" in code   # one wave per workgroup: __syncthreads and every branch are wave-uniform
