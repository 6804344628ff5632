"""Compiled shape of the kernels of water.hip (voxels + drains -> spill levels and the mask of the pools; CPU only: hipcc cross-compiles
gfx950): every kernel is listed, none uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions, none
declares LDS and nothing sleeps; the atomics are the stamp and the list append of water_setup, water_drain and water_relax, the reject
count of water_drain and the two counts and the key of water_finish, and no others; the register counts and occupancies are the ones
DESIGN.md 4.21 quotes."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

KERNELS = ("water_setup", "water_drain", "water_relax", "water_finish", "water_record_out", "water_mask")
# the most VGPRs each kernel may take (DESIGN.md 4.21 quotes the compiled numbers: 25, 14, 79, 29, 6 and 6) and the least occupancy that
# may compile: 64 or fewer registers are 8 waves, 96 or fewer are 5.  water_relax holds the state of travel_relax, whose bounds these are;
# with 80 or fewer registers it compiles to 6 waves.
VGPR_BOUND = {"water_setup": 32, "water_drain": 24, "water_relax": 96, "water_finish": 32, "water_record_out": 16, "water_mask": 16}
OCCUPANCY = {"water_setup": 8, "water_drain": 8, "water_relax": 5, "water_finish": 8, "water_record_out": 8, "water_mask": 8}
LDS_BYTES = {k: 0 for k in KERNELS}   # the file declares none: the rows of a tile meet by lane shuffles
# per kernel: the atomic instructions and how many of each.  setup: the stamp and the list append; drain: the same and the reject count;
# relax: the stamp and the list append once per face; finish: the wet and the closed count and the key
ATOMICS = {"water_setup": {"global_atomic_umax": 1, "global_atomic_add": 1}, "water_drain": {"global_atomic_umax": 1, "global_atomic_add": 2},
           "water_relax": {"global_atomic_umax": 6, "global_atomic_add": 6}, "water_finish": {"global_atomic_add_x2": 2, "global_atomic_umax_x2": 1},
           "water_record_out": {}, "water_mask": {}}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("water")]
    assert len(names) == len(KERNELS) and all(sum(k in name for name in names) == 1 for k in KERNELS), names


@pytest.mark.parametrize("kernel", KERNELS)
def test_water_kernel_uses_no_scratch_and_no_flat_accesses(kernel):
    (block,) = [b for b in usage_blocks("water") if kernel in b.split()[0]]
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") >= OCCUPANCY[kernel]
    assert field(block, r"LDS Size \[bytes/block\]") == LDS_BYTES[kernel]
    (body,) = kernel_bodies("water", kernel)
    ops = opcodes(body)
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
    assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0
    assert ops["s_sleep"] == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_atomics_are_the_named_ones_and_no_others(kernel):
    (body,) = kernel_bodies("water", kernel)
    ops = opcodes(body)
    assert {o: c for o, c in ops.items() if "atomic" in o or "cmpswap" in o} == ATOMICS[kernel]


def test_the_rows_of_a_tile_meet_by_lane_shuffles():
    (body,) = kernel_bodies("water", "water_relax")
    ops = opcodes(body)
    assert ops["ds_bpermute_b32"] == 32, "eight values from each of four neighbouring rows per sweep"
    assert sum(c for o, c in ops.items() if o.startswith("ds_") and o != "ds_bpermute_b32") == 0, "no LDS traffic"
    assert ops["s_barrier"] == 0
