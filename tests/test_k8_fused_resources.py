"""Build-time guard of the fused geometry + SH backward (preprocess_bwd_sh_kernel, csrc/preprocess.hip), no GPU: what the
compiler reports for gfx950 through scripts/kernel_resources.py.  The kernel carries K8a's double chain next to K8b's
output stage: it must not spill, must keep three waves per SIMD by registers and by LDS, and its LDS must be ONE buffer
shared by the run stages and the output stage (declared side by side they take 93 KB: one workgroup per compute unit)."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                                reason="needs hipcc (cross-compiles without a GPU) and c++filt")

STAGE_M16 = 256 * (16 * 3 + 4) * 4        # K8b's output stage at M = 16: 53 248 bytes
SMALL_FIXED = 256                         # room for a few words of static LDS (there are none today)


@pytest.fixture(scope="module")
def fused():
    import kernel_resources
    rows = [r for r in kernel_resources.collect([os.path.join(CSRC, "preprocess.hip")])
            if r["kernel"].split("<")[0] == "preprocess_bwd_sh_kernel"]
    assert rows, "preprocess_bwd_sh_kernel is not in preprocess.hip"
    return rows


def test_name_maps_to_the_preprocess_bwd_stage_only(fused):
    """scripts/make_pmc_json.py maps kernels to bench stages by substring and averages the variants of one kernel."""
    for r in fused:
        assert "preprocess_bwd" in r["kernel"] and "sh_bwd" not in r["kernel"], r["kernel"]


def test_no_scratch(fused):
    for r in fused:
        assert r["scratch"] == 0 and r["spills"] == 0, (r["kernel"], r["scratch"], r["spills"])


def test_carries_the_double_chain(fused):
    for r in fused:
        assert r["mix"]["valu_f64"] > 0, r["kernel"]


def test_lds_is_one_buffer(fused):
    for r in fused:
        assert r["lds_dyn"] > 0, "scripts/kernel_resources.py: DYNAMIC_LDS has no entry for the fused kernel"
        assert r["lds"] + r["lds_dyn"] <= STAGE_M16 + SMALL_FIXED, (r["kernel"], r["lds"], r["lds_dyn"])


def test_three_waves_per_simd(fused):
    for r in fused:
        assert min(r["waves_regs"], r["waves_lds"]) >= 3, (r["kernel"], r["vgpr"] + r["agpr"], r["waves_regs"], r["waves_lds"])
