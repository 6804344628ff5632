"""Compiled shape of the kernels of foot.hip (ground navigation; CPU only: hipcc cross-compiles gfx950): every kernel is listed, none
uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions, none declares LDS, none has a barrier and nothing
sleeps; the atomics are the ones the design names -- the stands of foot_setup, the min on W (a swap where the value is 0: foot_seed), the
count of the level appended under (once per height in flight in foot_level) and the rejected seeds, the key of foot_finish -- and no
others; the register counts and occupancies are the ones DESIGN.md 4.20 quotes."""
import re

import pytest

from _compiled import CSRC, field, kernel_bodies, opcodes, usage_blocks

KERNELS = ("foot_room", "foot_setup", "foot_seed", "foot_level", "foot_finish", "foot_record_out", "foot_paths")
# the most VGPRs each kernel may take (DESIGN.md 4.20 quotes the compiled numbers: 16, 8, 11, 28, 10, 6 and 25) and the occupancy that
# compiles: 64 or fewer registers are 8 waves
VGPR_BOUND = {"foot_room": 24, "foot_setup": 16, "foot_seed": 16, "foot_level": 32, "foot_finish": 16, "foot_record_out": 16, "foot_paths": 32}
OCCUPANCY = {k: 8 for k in KERNELS}
HEIGHTS = int(re.search(r"kFootHeights = (\d+);", open(f"{CSRC}/foot.h").read()).group(1))
ATOMICS = {"foot_room": {}, "foot_setup": {"global_atomic_add": 1}, "foot_seed": {"global_atomic_swap": 1, "global_atomic_add": 2},
           "foot_level": {"global_atomic_umin": HEIGHTS, "global_atomic_add": HEIGHTS}, "foot_finish": {"global_atomic_umax_x2": 1}, "foot_record_out": {},
           "foot_paths": {}}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("foot")]
    assert len(names) == len(KERNELS) and all(sum(k in name for name in names) == 1 for k in KERNELS), names


@pytest.mark.parametrize("kernel", KERNELS)
def test_foot_kernel_uses_no_scratch_no_lds_and_no_flat_accesses(kernel):
    (block,) = [b for b in usage_blocks("foot") if kernel in b.split()[0]]
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") == OCCUPANCY[kernel]
    assert field(block, r"LDS Size \[bytes/block\]") == 0
    (body,) = kernel_bodies("foot", kernel)
    ops = opcodes(body)
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_") or o.startswith("ds_read") or o.startswith("ds_write")) == 0
    assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0
    assert ops["s_sleep"] == 0 and ops["s_barrier"] == 0, "nothing waits for another wave"


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_atomics_are_the_named_ones_and_no_others(kernel):
    (body,) = kernel_bodies("foot", kernel)
    ops = opcodes(body)
    assert {o: c for o, c in ops.items() if "atomic" in o or "cmpswap" in o} == ATOMICS[kernel]
