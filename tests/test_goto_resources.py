"""The go-to-target kernels (robot_gym_amd/csrc/rg_goto.hip) compile for gfx950 without scratch and within their LDS budget:
one device-only compile with the compiler's resource remarks, parsed here (no GPU needed).  The source must stay clear of
what the kernels have no business with (atomics, inline assembly)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = {"rg_goto_post_kernel", "rg_goto_pre_kernel", "rg_goto_set_kernel"}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = tmp_path_factory.mktemp("goto") / "rg_goto.s"
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", str(out),
                          "rg_goto.hip", "-Rpass-analysis=kernel-resource-usage"], cwd=SRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: (?:\S+:\d+:\d+:\s+)?(.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            mangled = text.split(":", 1)[1].strip()
            k = re.search(r"(rg_goto_[a-z_]+_kernel)", mangled)
            name = k.group(1) if k else mangled
            kernels[name] = {}
        elif name and ":" in text:
            key, val = text.split(":", 1)
            kernels[name][key.strip()] = val.strip()
    return kernels


def test_every_goto_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_goto_kernel_uses_scratch(remarks):
    for name in KERNELS:
        r = remarks[name]
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)


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
    for name, want in REGISTERS.items():
        r = remarks[name]
        assert int(r["VGPRs"]) <= want["vgprs"], (name, r)
        assert int(r["AGPRs"]) == 0, (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= want["occupancy"], (name, r)


def test_source_has_no_inline_assembly_no_atomics_and_contraction_off():
    src = open(os.path.join(SRC, "rg_goto.hip")).read()
    code = re.sub(r"//.*", "", src)
    assert "asm" not in code and "atomic" not in src.lower()
    assert code.index("#pragma clang fp contract(off)") < code.index("__global__")
    assert "__launch_bounds__(kWave)" in code   # one wave per workgroup: __syncthreads and every branch are wave-uniform
