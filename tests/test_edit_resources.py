"""Compiled shape of the voxel-edit kernels (edit.hip; CPU only: hipcc cross-compiles gfx950): no scratch, no spills, and no flat_*
memory instructions -- every buffer is addressed as global memory."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_block_from

KERNELS = ("edit_scatter", "field_pass_x", "field_pass_y", "field_pass_z")


@pytest.mark.parametrize("kernel", KERNELS)
def test_edit_kernel_uses_no_scratch_and_no_flat_accesses(kernel):
    block = usage_block_from("edit", kernel)

    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    ops = opcodes(kernel_bodies("edit", kernel)[0])
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_store") or o.startswith("buffer_load")) == 0
