"""Compiled shape of the kernels of voxelize.hip (meshes -> voxels; CPU only: hipcc cross-compiles gfx950): every kernel is listed, none
uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions; the scattered writes are one atomic OR and one
atomic XOR with no compare-and-swap loop; the register counts are within the bounds DESIGN.md 4.15 quotes."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

# (kernel, number of instantiations): voxelize_items exists for surface cells and for solid column tiles
KERNELS = (("voxelize_plan", 1), ("voxelize_scan", 1), ("voxelize_items", 2), ("voxelize_dense", 1))
# the most VGPRs each kernel may take and the waves per SIMD that leaves (DESIGN.md 4.15 quotes the compiled numbers): 64 or fewer registers
# are 8 waves; the surface items carry a triangle, its plane and nine edge functions and may take 96 registers, which are 5 waves
VGPR_BOUND = {"voxelize_plan": 32, "voxelize_scan": 32, "voxelize_items": 96, "voxelize_dense": 32}
WAVES = {"voxelize_plan": (8,), "voxelize_scan": (8,), "voxelize_items": (5, 6, 7, 8), "voxelize_dense": (8,)}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("voxelize")]
    assert len(names) == sum(n for _, n in KERNELS) and all(any(k in name for k, _ in KERNELS) for name in names), names


@pytest.mark.parametrize("kernel,instances", KERNELS)
def test_voxelize_kernel_uses_no_scratch_and_no_flat_accesses(kernel, instances):
    blocks = [b for b in usage_blocks("voxelize") if kernel in b.split()[0]]
    assert len(blocks) == instances
    for block in blocks:
        assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
        assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") in WAVES[kernel]
    bodies = kernel_bodies("voxelize", kernel)
    assert len(bodies) == instances
    for body in bodies:
        ops = opcodes(body)
        assert ops, f"no instructions found for {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
        assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0


def test_solid_items_run_at_full_occupancy():
    (block,) = [b for b in usage_blocks("voxelize") if "voxelize_itemsILb1" in b.split()[0]]
    assert field(block, "VGPRs") <= 64 and field(block, r"Occupancy \[waves/SIMD\]") == 8


def test_scattered_writes_are_one_atomic_or_and_one_atomic_xor():
    """the item kernels write the planes through atomics alone -- no plain store, no compare-and-swap loop, no float instruction after the
    snap's multiply and round, no wait for another workgroup"""
    surface, solid = kernel_bodies("voxelize", "voxelize_itemsILb0"), kernel_bodies("voxelize", "voxelize_itemsILb1")
    assert len(surface) == 1 and len(solid) == 1
    for body, mine, other in ((surface[0], "global_atomic_or", "global_atomic_xor"), (solid[0], "global_atomic_xor", "global_atomic_or")):
        ops = opcodes(body)
        assert ops[mine] == 1 and ops[other] == 0
        assert sum(c for o, c in ops.items() if o.startswith("global_atomic")) == 1
        assert sum(c for o, c in ops.items() if o.startswith("global_store")) == 0
        assert sum(c for o, c in ops.items() if "cmpswap" in o) == 0 and ops["s_sleep"] == 0 and ops["s_barrier"] == 0


def test_dense_pass_stores_sixteen_bytes_per_lane_and_counts_with_one_atomic():
    (body,) = kernel_bodies("voxelize", "voxelize_dense")
    ops = opcodes(body)
    assert ops["global_store_dwordx4"] >= 1 and ops["global_atomic_add_x2"] == 1
    assert sum(c for o, c in ops.items() if "cmpswap" in o) == 0
