"""Compiled shape of the kernels of travel.hip (voxels + seeds -> travel fields and paths; CPU only: hipcc cross-compiles gfx950): every
kernel is listed, none uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions, none declares LDS and
nothing sleeps; the atomics are the stamp and the list append of travel_seed and travel_relax, the reject count of travel_seed and the
count and the key of travel_finish, and no others; the register counts and occupancies are the ones DESIGN.md 4.18 quotes."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

KERNELS = ("travel_setup", "travel_seed", "travel_relax", "travel_finish", "travel_record_out", "travel_paths")
# the most VGPRs each kernel may take (DESIGN.md 4.18 quotes the compiled numbers: 22, 14, 87, 10, 8 and 18) and the occupancy that compiles:
# 64 or fewer registers are 8 waves, 96 or fewer are 5
VGPR_BOUND = {"travel_setup": 32, "travel_seed": 24, "travel_relax": 96, "travel_finish": 16, "travel_record_out": 16, "travel_paths": 24}
OCCUPANCY = {"travel_setup": 8, "travel_seed": 8, "travel_relax": 5, "travel_finish": 8, "travel_record_out": 8, "travel_paths": 8}
LDS_BYTES = {k: 0 for k in KERNELS}   # the file declares none: the rows of a tile meet by lane shuffles
# per kernel: the atomic instructions and how many of each.  seed: the stamp, the list append, the reject count; relax: the stamp and the
# list append once per face; finish: the count and the key
ATOMICS = {"travel_setup": {}, "travel_seed": {"global_atomic_umax": 1, "global_atomic_add": 2}, "travel_relax": {"global_atomic_umax": 6, "global_atomic_add": 6},
           "travel_finish": {"global_atomic_add_x2": 1, "global_atomic_umax_x2": 1}, "travel_record_out": {}, "travel_paths": {}}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("travel")]
    assert len(names) == len(KERNELS) and all(sum(k in name for name in names) == 1 for k in KERNELS), names


@pytest.mark.parametrize("kernel", KERNELS)
def test_travel_kernel_uses_no_scratch_and_no_flat_accesses(kernel):
    (block,) = [b for b in usage_blocks("travel") if kernel in b.split()[0]]
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") == OCCUPANCY[kernel]
    assert field(block, r"LDS Size \[bytes/block\]") == LDS_BYTES[kernel]
    (body,) = kernel_bodies("travel", kernel)
    ops = opcodes(body)
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
    assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0
    assert ops["s_sleep"] == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_atomics_are_the_named_ones_and_no_others(kernel):
    (body,) = kernel_bodies("travel", kernel)
    ops = opcodes(body)
    assert {o: c for o, c in ops.items() if "atomic" in o or "cmpswap" in o} == ATOMICS[kernel]


def test_the_rows_of_a_tile_meet_by_lane_shuffles():
    (body,) = kernel_bodies("travel", "travel_relax")
    ops = opcodes(body)
    assert ops["ds_bpermute_b32"] == 32, "eight values from each of four neighbouring rows per sweep"
    assert sum(c for o, c in ops.items() if o.startswith("ds_") and o != "ds_bpermute_b32") == 0, "no LDS traffic"
    assert ops["s_barrier"] == 0
