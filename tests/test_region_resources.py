"""Compiled shape of the kernels of region.hip (dense regions of a live scene; CPU only: hipcc cross-compiles gfx950): no scratch, no
spills and no flat_* memory instructions in any kernel or instantiation, and 16-byte accesses to the volume in the aligned ones."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

# (kernel, number of instantiations): pack and unpack exist for 16-byte aligned volumes and for any other
KERNELS = (("region_pack", 2), ("region_unpack", 2), ("region_patch", 1), ("region_zero", 1))



def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("region")]
    assert len(names) == sum(n for _, n in KERNELS) and all(any(k in name for k, _ in KERNELS) for name in names), names


@pytest.mark.parametrize("kernel,instances", KERNELS)
def test_region_kernel_uses_no_scratch_and_no_flat_accesses(kernel, instances):
    blocks = [b for b in usage_blocks("region") if kernel in b.split()[0]]
    assert len(blocks) == instances
    for block in blocks:
        assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    bodies = kernel_bodies("region", kernel)
    assert len(bodies) == instances
    for body in bodies:
        ops = opcodes(body)
        assert ops, f"no instructions found for {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_store") or o.startswith("buffer_load")) == 0
        assert sum(c for o, c in ops.items() if o.startswith("global_load") or o.startswith("global_store")) > 0


def test_volume_accesses_are_16_bytes_wide_in_the_aligned_instantiations():
    """eight lanes cover a 128-byte line: the aligned pack reads and the aligned unpack writes the volume as 16 bytes per lane, once per
    chunk (two chunks per lane); the general instantiations have no such access"""
    for kernel, op in (("region_pack", "global_load_dwordx4"), ("region_unpack", "global_store_dwordx4")):
        for flag, want in (("ILb1", 2), ("ILb0", 0)):
            (body,) = kernel_bodies("region", kernel + flag)
            assert sum(1 for l in body if l.strip().startswith(op)) == want, (kernel, flag)
