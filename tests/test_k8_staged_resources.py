"""Build-time guard of K8's staged forms (csrc/preprocess.hip), no GPU: preprocess_bwd_sh_kernel<true> and
preprocess_bwd_staged_kernel<ACC> as the compiler reports them for gfx950 through scripts/kernel_resources.py.

The staging spends LDS, not registers: the kernels must stay at three waves per SIMD by registers (168 at most) and by
LDS (the four stages and the staged inputs are 53 248 bytes, K8b's output stage at M = 16: three workgroups per compute
unit) and must not spill.  The camera's 35 uniform words are loaded in front of the first DMA; behind a write to memory
the compiler takes them by vector loads into 35 registers and the kernels fall to two waves -- that is what this guards."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hierarchical-3d-gaussians_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "scripts"))

pytestmark = pytest.mark.skipif(not (os.path.exists("/opt/rocm/bin/hipcc") and shutil.which("c++filt")),
                                reason="needs hipcc (cross-compiles without a GPU) and c++filt")

LDS_BYTES = 4 * (256 * 40 + 64 * 48)      # four stages of 256 records + four blocks of 64 rows x 48 bytes of inputs
STAGED = ("preprocess_bwd_sh_kernel<true>", "preprocess_bwd_staged_kernel<false>", "preprocess_bwd_staged_kernel<true>")


@pytest.fixture(scope="module")
def rows():
    import kernel_resources
    return {r["kernel"]: r for r in kernel_resources.collect([os.path.join(CSRC, "preprocess.hip")])}


def test_the_lds_budget_is_the_output_stage():
    assert LDS_BYTES == 256 * (16 * 3 + 4) * 4 == 53248


@pytest.mark.parametrize("name", STAGED)
def test_three_waves_no_scratch(rows, name):
    assert name in rows, sorted(rows)
    r = rows[name]
    assert r["scratch"] == 0 and r["spills"] == 0, (name, r["scratch"], r["spills"])
    assert r["vgpr"] + r["agpr"] <= 168, (name, r["vgpr"], r["agpr"])
    assert r["lds"] + r["lds_dyn"] <= LDS_BYTES + 256, (name, r["lds"], r["lds_dyn"])
    assert min(r["waves_regs"], r["waves_lds"]) >= 3, (name, r["waves_regs"], r["waves_lds"])
    assert r["mix"]["valu_f64"] > 0, name                    # (the double chain is in it)


def test_the_register_forms_are_still_built(rows):
    """HGS_K8_STAGE=0 and the LOD route run them."""
    for name in ("preprocess_bwd_sh_kernel<false>", "preprocess_bwd_kernel<false, false>", "preprocess_bwd_kernel<true, false>",
                 "preprocess_bwd_kernel<false, true>"):
        assert name in rows, sorted(rows)
