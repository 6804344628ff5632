"""Compiled shape of the kernels of volume.hip (volume queries against a live scene; CPU only: hipcc cross-compiles gfx950): every kernel
is listed, none uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions, and the count kernel adds its
results with global atomics."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

# (kernel, number of instantiations): the count kernel exists with and without BM_VOLUME_ANY
KERNELS = (("volume_plan", 1), ("volume_scan", 1), ("volume_count", 2), ("volume_finish", 1))




def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("volume")]
    assert len(names) == sum(n for _, n in KERNELS) and all(any(k in name for k, _ in KERNELS) for name in names), names


@pytest.mark.parametrize("kernel,instances", KERNELS)
def test_volume_kernel_uses_no_scratch_and_no_flat_accesses(kernel, instances):
    blocks = [b for b in usage_blocks("volume") if kernel in b.split()[0]]
    assert len(blocks) == instances
    for block in blocks:
        assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    bodies = kernel_bodies("volume", kernel)
    assert len(bodies) == instances
    for body in bodies:
        ops = opcodes(body)
        assert ops, f"no instructions found for {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
        assert sum(c for o, c in ops.items() if o.startswith("global_load") or o.startswith("global_store")) > 0


def test_the_count_kernel_adds_with_global_atomics_and_keeps_seven_waves():
    """one 64-bit add for the voxels, one 32-bit add for the unresolved cells, and (without BM_VOLUME_ANY) three signed min and three
    signed max for the bounds -- twice, for the group and the wave form; the register budget leaves at least the ray query's 7 waves per SIMD"""
    for block in (b for b in usage_blocks("volume") if "volume_count" in b.split()[0]):
        assert field(block, r"Occupancy \[waves/SIMD\]") >= 7
    for flag, bounds in (("ILb0", True), ("ILb1", False)):
        (body,) = kernel_bodies("volume", "volume_count" + flag)
        ops = opcodes(body)
        assert ops["global_atomic_add_x2"] >= 1 and ops["global_atomic_add"] >= 1
        assert (ops["global_atomic_smin"] >= 3 and ops["global_atomic_smax"] >= 3) if bounds else (ops["global_atomic_smin"] == 0 and ops["global_atomic_smax"] == 0)
        assert sum(c for o, c in ops.items() if "cmpswap" in o) == 0
