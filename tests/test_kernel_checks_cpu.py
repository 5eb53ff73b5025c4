"""tests/kernel_checks.py on literal compiler output (no compiler needed): two kernels' remarks become the two expected rows,
and two functions that shorten to one name are refused naming both, never reduced to one row."""
import pytest

from tests import kernel_checks

TAG = "[-Rpass-analysis=kernel-resource-usage]"


def _remarks(mangled, vgprs, scratch):
    rows = [f"Function Name: {mangled}", "    TotalSGPRs: 74", f"    VGPRs: {vgprs}", "    AGPRs: 0", f"    ScratchSize [bytes/lane]: {scratch}",
            "    Dynamic Stack: False", "    Occupancy [waves/SIMD]: 8", "    SGPRs Spill: 0", "    VGPRs Spill: 0", "    LDS Size [bytes/block]: 0"]
    return "".join(f"rg_unit.hip:59:1: remark: {r} {TAG}\n" for r in rows) + "   59 | __global__ void f() {\n      | ^\n"


def test_two_kernels_parse_into_their_two_rows():
    text = ("clang++: warning: argument unused during compilation: '--hip-link' [-Wunused-command-line-argument]\n"
            + _remarks("_ZN12_GLOBAL__N_122rg_scan_observe_kernelENS_7ScanCfgE13rg_srb_groundPKdPKiPfS6_", 40, 0) + _remarks("_Z17rg_dr_push_kernelPdi", 16, 24))
    rows = kernel_checks.by_short_name(kernel_checks.kernel_report.parse_remarks(text))
    assert sorted(rows) == ["rg_dr_push_kernel", "rg_scan_observe_kernel"]
    common = {"TotalSGPRs": "74", "AGPRs": "0", "Dynamic Stack": "False", "Occupancy [waves/SIMD]": "8", "SGPRs Spill": "0", "VGPRs Spill": "0",
              "LDS Size [bytes/block]": "0"}
    assert rows["rg_scan_observe_kernel"] == {"mangled": "_ZN12_GLOBAL__N_122rg_scan_observe_kernelENS_7ScanCfgE13rg_srb_groundPKdPKiPfS6_", "VGPRs": "40",
                                              "ScratchSize [bytes/lane]": "0", **common}
    assert rows["rg_dr_push_kernel"] == {"mangled": "_Z17rg_dr_push_kernelPdi", "VGPRs": "16", "ScratchSize [bytes/lane]": "24", **common}
    kernel_checks.assert_lean(rows, {"rg_scan_observe_kernel"}, lds=0)
    kernel_checks.assert_registers(rows, {"rg_scan_observe_kernel": dict(vgprs=40, occupancy=8), "rg_dr_push_kernel": dict(vgprs=16, sgprs=74)})
    with pytest.raises(AssertionError, match="rg_dr_push_kernel.*'ScratchSize \\[bytes/lane\\]': '24'"):
        kernel_checks.assert_lean(rows, {"rg_scan_observe_kernel", "rg_dr_push_kernel"})
    with pytest.raises(AssertionError, match="rg_scan_observe_kernel"):
        kernel_checks.assert_registers(rows, {"rg_scan_observe_kernel": dict(vgprs=39)})


def test_two_functions_that_shorten_alike_are_refused_naming_both():
    a, b = "_Z15rg_sweep_kernelILi10EEvPd", "_Z15rg_sweep_kernelILi20EEvPd"      # two instantiations of one templated kernel
    rows = kernel_checks.kernel_report.parse_remarks(_remarks(a, 64, 0) + _remarks(b, 256, 512))
    assert [r["mangled"] for r in rows] == [a, b]
    with pytest.raises(pytest.fail.Exception) as e:
        kernel_checks.by_short_name(rows)
    assert a in str(e.value) and b in str(e.value) and "rg_sweep_kernel" in str(e.value)
