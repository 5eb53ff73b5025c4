"""The position-mode kernels (robot_gym_amd/csrc/rg_posctl.hip) compile for gfx950 without scratch: one device-only
compile with the compiler's resource remarks, parsed here (no GPU needed).  Parity rests on float64 values kept in
registers, and a one-lane-per-robot kernel that spills would pay for it on every tick."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = {"rg_posctl_bezier_kernel", "rg_posctl_pose_kernel", "rg_posctl_torque_kernel"}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = tmp_path_factory.mktemp("posctl") / "rg_posctl.s"
    res = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-o", str(out),
                          "rg_posctl.hip", "-Rpass-analysis=kernel-resource-usage"], cwd=SRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    kernels, name = {}, None
    for line in res.stderr.splitlines():
        m = re.search(r"remark: (?:\S+:\d+:\d+:\s+)?(.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1).strip()
        if text.startswith("Function Name:"):
            mangled = text.split(":", 1)[1].strip()
            k = re.search(r"(rg_posctl_[a-z_]+_kernel)", mangled)
            name = k.group(1) if k else mangled
            kernels[name] = {}
        elif name and ":" in text:
            key, val = text.split(":", 1)
            kernels[name][key.strip()] = val.strip()
    return kernels


def test_every_posctl_kernel_is_reported(remarks):
    assert set(remarks) == KERNELS


def test_no_posctl_kernel_uses_scratch(remarks):
    for name in KERNELS:
        r = remarks[name]
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
