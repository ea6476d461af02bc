"""The fused Gram kernels (k_schur_gram<..., 1>: the point pass in a prologue of the task, ba_kernels.h) stay in registers: no scratch, no spilled VGPRs, two waves
per SIMD.  Round 5's fused variant spilled 50 registers inside the sub-chunk loop; the prologue runs before the camera sums and the tile accumulators are alive and
must cost the loop nothing (read from the built library's code objects: no GPU needed)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as KR  # noqa: E402

LIB = os.path.join(ROOT, "spherical_sfm_amd", "libssfm_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(KR.READELF)), reason="needs the built library and llvm-readelf")

# every fused instantiation the dispatcher can select (ba_solver.hip: gram_kernel_of<true>); the first two are the bench configurations' (config 2, spherical)
FUSED = ["k_schur_gram<6, 2, 3, 1>", "k_schur_gram<3, 1, 2, 1>", "k_schur_gram<6, 1, 0, 1>", "k_schur_gram<6, 1, 2, 1>", "k_schur_gram<6, 2, 0, 1>",
         "k_schur_gram<3, 1, 0, 1>", "k_schur_gram<3, 2, 0, 1>"]


@pytest.fixture(scope="module")
def kernels():
    ks = {k["short"]: k for k in KR.kernels(LIB).values()}
    assert len(ks) > 100, "the library's gfx950 code objects were not found"
    return ks


@pytest.mark.parametrize("name", FUSED)
def test_fused_gram_kernel_has_no_scratch(kernels, name):
    k = kernels[name]
    assert k["scratch"] == 0 and k["vgpr_spill"] == 0 and not k["dynamic_stack"], k
    assert k["vgpr"] + k["agpr"] <= 256, k


def test_no_other_fused_instantiation_is_shipped(kernels):
    """The three-tile class has no fused form (it would carry more scratch than the unfused kernel): what is not in the list above is not in the library."""
    fused = sorted(n for n in kernels if n.startswith("k_schur_gram<") and n.endswith(", 1>"))
    assert fused == sorted(FUSED), fused
