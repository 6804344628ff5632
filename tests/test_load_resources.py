"""Compiled shape of the kernels of load.hip (dense voxels -> scene; CPU only: hipcc cross-compiles gfx950): no scratch, no spills, and
no flat_* memory instructions -- every buffer is addressed as global memory."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

# (kernel, number of instantiations): classify and pack exist for 16-byte aligned volumes and for any other
KERNELS = (("load_classify", 2), ("load_number", 1), ("load_scan", 1), ("load_pack", 2))


@pytest.mark.parametrize("kernel,instances", KERNELS)
def test_load_kernel_uses_no_scratch_and_no_flat_accesses(kernel, instances):
    blocks = [b for b in usage_blocks("load") if kernel in b.split()[0]]
    assert len(blocks) == instances

    for block in blocks:
        assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    bodies = kernel_bodies("load", kernel)
    assert len(bodies) == instances
    for body in bodies:
        ops = opcodes(body)
        assert ops, f"no instructions found for {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_store") or o.startswith("buffer_load")) == 0
        assert sum(c for o, c in ops.items() if o.startswith("global_load") or o.startswith("global_store")) > 0


def test_volume_reads_are_16_bytes_wide():
    """the aligned classify and pack kernels read the volume as 16 bytes per lane: eight lanes cover a 128-byte line"""
    for kernel in ("load_classifyILb1", "load_packILb1"):
        assert sum(1 for l in kernel_bodies("load", kernel)[0] if l.strip().startswith("global_load_dwordx4")) == 2
