"""The simulator kernels (robot_gym_amd/csrc/rg_srb.hip) compile for gfx950 without scratch: one device-only compile with
the compiler's resource remarks (tests/kernel_checks.py; no GPU needed).  Parity rests on float64 values kept in registers, and the
source must stay clear of what the kernels have no business with (LDS, atomics, inline assembly)."""
import os
import re

import pytest

from tests import kernel_checks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
KERNELS = {"rg_srb_step_kernel", "rg_srb_reset_kernel"}


@pytest.fixture(scope="module")
def remarks():
    return kernel_checks.remarks("rg_srb.hip")


def test_every_srb_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_srb_kernel_uses_scratch_or_lds(remarks):
    kernel_checks.assert_lean(remarks, KERNELS, lds=0)


# What the device-only compile reports today.  Both kernels fill the 256 architectural VGPRs a 256-lane workgroup may have
# and park further values in accumulator registers (the float64 chain state of leg_fk / leg_ik next to the 13 body values):
# one wave per SIMD, which at 4096 robots (256 waves on 1024 SIMDs) costs nothing.  More accumulator traffic or scratch
# would: the figures are upper bounds.
REGISTERS = {"rg_srb_step_kernel": dict(vgprs=256, agprs=40), "rg_srb_reset_kernel": dict(vgprs=256, agprs=8)}


def test_register_use_is_pinned(remarks):
    kernel_checks.assert_registers(remarks, REGISTERS)


def test_contraction_is_off_before_the_controller_header_is_included():
    src = open(os.path.join(SRC, "rg_srb.hip")).read()
    assert src.index("#pragma clang fp contract(off)") < src.index('#include "rg_mpc_dev.h"') < src.index('#include "rg_srb_tick.inc"')
    assert src.index('#include "rg_srb_dev.inc"') < src.index('#include "rg_srb_tick.inc"') < src.index("__global__")
    tick = open(os.path.join(SRC, "rg_srb_tick.inc")).read()
    for text in (src, tick):
        assert "asm" not in re.sub(r"//.*", "", text) and "atomic" not in text and "__shared__" not in text
    # the shared body of a tick is under the including file's pragma and brings neither a pragma nor a fused operation of its own
    code = re.sub(r"//.*", "", tick)
    assert "#pragma clang fp" not in code and "fma(" not in tick and "#include" not in code


def test_the_body_of_a_tick_is_typed_once():
    """The four step kernels stand on rg_srb_tick.inc: the quaternion's renormalisation and sum4 are defined in one file."""
    sources = {n: open(os.path.join(SRC, n)).read() for n in sorted(os.listdir(SRC)) if n.endswith((".hip", ".inc", ".h"))}
    for text in ("double sum4(double", "qt[3] = qt[3] / nrm"):
        assert [n for n, src in sources.items() if text in src] == ["rg_srb_tick.inc"], text
    assert sources["rg_srb_tick.inc"].count("double sum4(double") == 1 and sources["rg_srb_tick.inc"].count("qt[3] = qt[3] / nrm") == 1
    for n in ("rg_srb.hip", "rg_srb_terrain.hip", "rg_srb_contact.hip", "rg_srb_friction.hip"):
        assert sources[n].count('#include "rg_srb_tick.inc"') == 1, n
