"""Compiled shape of the kernels of settle.hip (labels + chosen records -> the settled volume; CPU only: hipcc cross-compiles gfx950):
every kernel is listed, none uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions, none declares LDS
and nothing sleeps; the atomics are the chosen count of settle_setup, the minimum on D (once per slice in flight), the changes and the
contacts of settle_relax, the 2s of settle_move and the moved pieces and the largest drop of settle_finish, and no others; the register
counts and occupancies are the ones DESIGN.md 4.19 quotes."""
import re

import pytest

from _compiled import CSRC, field, kernel_bodies, opcodes, usage_blocks

KERNELS = ("settle_setup", "settle_relax", "settle_move", "settle_finish", "settle_record_out")
# the most VGPRs each kernel may take (DESIGN.md 4.19 quotes the compiled numbers: 8, 30, 29, 11 and 8) and the occupancy that compiles:
# 64 or fewer registers are 8 waves
VGPR_BOUND = {"settle_setup": 16, "settle_relax": 32, "settle_move": 32, "settle_finish": 16, "settle_record_out": 16}
OCCUPANCY = {k: 8 for k in KERNELS}
LDS_BYTES = {k: 0 for k in KERNELS}   # the file declares none: sums meet by lane shuffles
SLICES = int(re.search(r"kSettleSlices = (\d+);", open(f"{CSRC}/settle.h").read()).group(1))
ATOMICS = {"settle_setup": {"global_atomic_add": 1}, "settle_relax": {"global_atomic_umin": SLICES, "global_atomic_add": 1, "global_atomic_add_x2": 1},
           "settle_move": {"global_atomic_add_x2": 1}, "settle_finish": {"global_atomic_add": 1, "global_atomic_umax": 1}, "settle_record_out": {}}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("settle")]
    assert len(names) == len(KERNELS) and all(sum(k in name for name in names) == 1 for k in KERNELS), names


@pytest.mark.parametrize("kernel", KERNELS)
def test_settle_kernel_uses_no_scratch_and_no_flat_accesses(kernel):
    (block,) = [b for b in usage_blocks("settle") if kernel in b.split()[0]]
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") == OCCUPANCY[kernel]
    assert field(block, r"LDS Size \[bytes/block\]") == LDS_BYTES[kernel]
    (body,) = kernel_bodies("settle", kernel)
    ops = opcodes(body)
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
    assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0
    assert ops["s_sleep"] == 0 and ops["s_barrier"] == 0


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_atomics_are_the_named_ones_and_no_others(kernel):
    (body,) = kernel_bodies("settle", kernel)
    ops = opcodes(body)
    assert {o: c for o, c in ops.items() if "atomic" in o or "cmpswap" in o} == ATOMICS[kernel]
