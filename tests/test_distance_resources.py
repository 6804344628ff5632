"""Compiled shape of the kernels of distance.hip (voxels -> distances; CPU only: hipcc cross-compiles gfx950): every kernel is listed, none
uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions; the two atomics of the file are the 64-bit add of
the source count in the x pass and the 64-bit max of the key in the line pass, and nothing sleeps; the register counts are within the
bounds DESIGN.md 4.17 quotes."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

KERNELS = ("distance_x", "distance_line", "distance_finish", "distance_mask")
# the most VGPRs each kernel may take (DESIGN.md 4.17 quotes the compiled numbers: 33, 22, 4 and 9); 64 or fewer registers are 8 waves
VGPR_BOUND = {"distance_x": 40, "distance_line": 32, "distance_finish": 8, "distance_mask": 16}
LDS_BYTES = {"distance_x": 0, "distance_line": 0, "distance_finish": 0, "distance_mask": 0}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("distance")]
    assert len(names) == len(KERNELS) and all(sum(k in name for name in names) == 1 for k in KERNELS), names


@pytest.mark.parametrize("kernel", KERNELS)
def test_distance_kernel_uses_no_scratch_and_no_flat_accesses(kernel):
    (block,) = [b for b in usage_blocks("distance") if kernel in b.split()[0]]
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") == 8
    assert field(block, r"LDS Size \[bytes/block\]") == LDS_BYTES[kernel]
    (body,) = kernel_bodies("distance", kernel)
    ops = opcodes(body)
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
    assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0


def test_the_count_and_the_key_are_the_only_atomics():
    (body,) = kernel_bodies("distance", "distance_x")
    ops = opcodes(body)
    assert ops["global_atomic_add_x2"] == 1 and sum(c for o, c in ops.items() if "atomic" in o or "cmpswap" in o) == 1 and ops["s_sleep"] == 0
    (body,) = kernel_bodies("distance", "distance_line")
    ops = opcodes(body)
    assert ops["global_atomic_umax_x2"] == 1 and sum(c for o, c in ops.items() if "atomic" in o or "cmpswap" in o) == 1 and ops["s_sleep"] == 0
    for kernel in ("distance_finish", "distance_mask"):
        (body,) = kernel_bodies("distance", kernel)
        assert sum(c for o, c in opcodes(body).items() if "atomic" in o or "cmpswap" in o or o == "s_sleep") == 0


def test_the_mask_stores_a_word_where_four_bytes_are_voxels():
    (body,) = kernel_bodies("distance", "distance_mask")
    ops = opcodes(body)
    assert ops["global_store_dword"] >= 1 and ops["global_store_byte"] >= 1
