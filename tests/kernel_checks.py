"""What the CPU tests of every unit ask of the build, in one place (no GPU needed): the compiler's resource figures for a
unit's kernels, from one device-only compile per source under the flags the library is built with (tools/kernel_report.py,
the Makefile's resource-usage target), and what `make` would compile into the two libraries, from dry runs of make itself.
A unit's test keeps its KERNELS set, its REGISTERS table and its own budgets; the machinery they stand on is here."""
import functools
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "robot_gym_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
LIBRARIES = ("librg_mpc.so", "librg_mpc_stamp.so")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_report  # noqa: E402


def short_name(mangled):
    """The rg_..._kernel identifier inside a mangled name (template arguments and parameter types dropped)."""
    m = re.search(r"rg_[a-z0-9_]+_kernel", mangled)
    return m.group(0) if m else mangled


def by_short_name(rows):
    """{short kernel name: row} of parse_remarks' rows.  Two functions that shorten to one name (the instantiations of a
    templated kernel) are an error naming both: a dict would keep the later row only and hide what the earlier one reports."""
    out = {}
    for r in rows:
        name = short_name(r["mangled"])
        if name in out:
            pytest.fail(f"{out[name]['mangled']} and {r['mangled']} both shorten to {name}: tell them apart before pinning either")
        out[name] = r
    return out


@functools.lru_cache(maxsize=None)
def remarks(source):
    """{short kernel name: the compiler's resource row} for one .hip file of robot_gym_amd/csrc; one compile per source and process."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    try:
        text = kernel_report.compile_device(os.devnull, source)
    except RuntimeError as e:
        pytest.fail(str(e))
    return by_short_name(kernel_report.parse_remarks(text))


def assert_lean(rows, kernels, lds=None):
    """No scratch, no spills, no dynamic stack; with lds=0, no LDS either."""
    for name in sorted(kernels):
        r = rows[name]
        assert int(r["ScratchSize [bytes/lane]"]) == 0, (name, r)
        assert int(r["VGPRs Spill"]) == 0 and int(r["SGPRs Spill"]) == 0, (name, r)
        assert r["Dynamic Stack"] == "False", (name, r)
        if lds is not None:
            assert int(r["LDS Size [bytes/block]"]) == lds, (name, r)


def assert_registers(rows, pins):
    """pins: {kernel: dict(vgprs=, agprs=0, occupancy=1[, sgprs=])}, upper bounds on registers and a lower bound on waves per SIMD."""
    for name, want in pins.items():
        r = rows[name]
        assert int(r["VGPRs"]) <= want["vgprs"], (name, r)
        assert int(r["AGPRs"]) <= want.get("agprs", 0), (name, r)
        assert "sgprs" not in want or int(r["TotalSGPRs"]) <= want["sgprs"], (name, r)
        assert int(r["Occupancy [waves/SIMD]"]) >= want.get("occupancy", 1), (name, r)


def _make(*args):
    res = subprocess.run(["make", *args], cwd=SRC, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    return res.stdout


@functools.lru_cache(maxsize=None)
def library_targets():
    """{library: dict(sources=[...], prerequisites=[...])} as make itself sees the two libraries: the .hip files on the link
    command of a forced dry run, in order, and the expanded prerequisites in make's database.  Nothing is built or written."""
    commands, database = _make("-n", "-B", *LIBRARIES).splitlines(), _make("-pn", *LIBRARIES)
    out = {}
    for lib in LIBRARIES:
        line, = [c.split() for c in commands if f"-shared -o {lib} " in c]
        rule, = re.findall(rf"^{re.escape(lib)}: (.*)$", database, flags=re.M)
        out[lib] = dict(sources=[w for w in line if w.endswith(".hip")], prerequisites=rule.split())
    return out


def assert_built_into_both(source, header=None):
    """The unit's source is compiled into both libraries; with header, source and include/<header> rebuild both when they change."""
    for lib, t in library_targets().items():
        assert t["sources"].count(source) == 1, (lib, source, t["sources"])
        if header is not None:
            assert source in t["prerequisites"] and "../../include/" + header in t["prerequisites"], (lib, source, header, t["prerequisites"])
