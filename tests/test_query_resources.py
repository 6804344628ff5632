"""Compiled shape of the ray-query kernel (query.hip; CPU only: hipcc cross-compiles gfx950): both instantiations run without scratch
or spills, address every buffer as global memory (no flat_*, scratch_* or buffer_* instructions), and keep at least 7 waves per SIMD
resident."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_block_from

WAVES_PER_SIMD = 7
INSTANTIATIONS = ("_ZN2bm10query_raysILb0EEE", "_ZN2bm10query_raysILb1EEE")  # <REQUEST = false>, <REQUEST = true>


@pytest.mark.parametrize("kernel", INSTANTIATIONS)
def test_query_kernel_resources(kernel):
    block = usage_block_from("query", "Function Name: " + kernel)

    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, r"Occupancy \[waves/SIMD\]") >= WAVES_PER_SIMD
    ops = opcodes(kernel_bodies("query", kernel, lambda l: l.startswith(kernel) and l.split(":")[0].startswith(kernel))[0])
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_") or o.startswith("scratch_") or o.startswith("buffer_")) == 0
    # 16-byte record loads and stores, bricks staged straight into LDS
    assert ops["global_load_dwordx4"] >= 2 and ops["global_store_dwordx4"] >= 2 and ops["global_load_lds_dword"] >= 16
