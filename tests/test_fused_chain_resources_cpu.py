"""CPU: the new kernel of the fused detection chain (kernels.hpp launch_suppress_compact) runs beside
the LK launch like every other helper, so it is held to the budget of test_kernel_resources_cpu.py: at most 104
allocated VGPRs, 18 KB of LDS, no scratch -- read the same way, from the AMDGPU metadata of the built library."""
import os

import pytest

from polychase_amd import build
from test_kernel_resources_cpu import HELPER_LDS_BUDGET, HELPER_VGPR_BUDGET, _code_objects, _kernel_metadata

# substrings of the mangled names not yet covered by HELPERS there ("bucket_sort_kernel" already holds both instantiations
# of the rank sort): the suppression with its own compaction
FUSED_HELPERS = ["suppress_compact_kernel"]


@pytest.fixture(scope="module")
def kernels():
    path = build.hip_library_path()
    if not os.path.exists(path):
        build.build_hip()
    return {k[".name"]: k for elf in _code_objects(path) for k in _kernel_metadata(elf)}


@pytest.mark.parametrize("helper", FUSED_HELPERS)
def test_fused_chain_kernels_fit_beside_three_lk_wavefronts(kernels, helper):
    found = [(n, k) for n, k in kernels.items() if helper in n]
    assert len(found) == 1, f"{helper}: {[n for n, _ in found]}"
    name, k = found[0]
    assert (k[".vgpr_count"] + 7) // 8 * 8 <= HELPER_VGPR_BUDGET, f"{name}: {k['.vgpr_count']} VGPRs"
    assert k.get(".agpr_count", 0) == 0, name
    assert k[".group_segment_fixed_size"] <= HELPER_LDS_BUDGET, f"{name}: {k['.group_segment_fixed_size']} B of LDS"
    assert k.get(".private_segment_fixed_size", 0) == 0, f"{name}: spills to scratch"
