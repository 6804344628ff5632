"""Compiled shape of the kernels of mesh.hip (voxels -> quads; CPU only: hipcc cross-compiles gfx950): every kernel is listed, none uses
scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions; mesh_emit has no atomic and never sleeps, and writes
a quad as one 16-byte store; the one atomic of the file is the 64-bit add of the face total; the register counts are within the bounds
DESIGN.md 4.16 quotes."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

KERNELS = ("mesh_count", "mesh_scan", "mesh_emit", "mesh_triangles")
# the most VGPRs each kernel may take (DESIGN.md 4.16 quotes the compiled numbers: 26, 12, 28 and 20); 64 or fewer registers are 8 waves
VGPR_BOUND = {"mesh_count": 40, "mesh_scan": 32, "mesh_emit": 40, "mesh_triangles": 32}
LDS_BYTES = {"mesh_count": 200, "mesh_scan": 2048, "mesh_emit": 200, "mesh_triangles": 0}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("mesh")]
    assert len(names) == len(KERNELS) and all(sum(k in name for name in names) == 1 for k in KERNELS), names


@pytest.mark.parametrize("kernel", KERNELS)
def test_mesh_kernel_uses_no_scratch_and_no_flat_accesses(kernel):
    (block,) = [b for b in usage_blocks("mesh") if kernel in b.split()[0]]
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") == 8
    assert field(block, r"LDS Size \[bytes/block\]") == LDS_BYTES[kernel]
    (body,) = kernel_bodies("mesh", kernel)
    ops = opcodes(body)
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
    assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0


def test_emit_has_no_atomic_and_stores_a_quad_at_once():
    (body,) = kernel_bodies("mesh", "mesh_emit")
    ops = opcodes(body)
    assert sum(c for o, c in ops.items() if "atomic" in o or "cmpswap" in o) == 0 and ops["s_sleep"] == 0
    assert ops["global_store_dwordx4"] >= 1
    assert sum(c for o, c in ops.items() if o.startswith("global_store") and o != "global_store_dwordx4") == 0


def test_the_face_total_is_the_only_atomic():
    (body,) = kernel_bodies("mesh", "mesh_count")
    ops = opcodes(body)
    assert ops["global_atomic_add_x2"] == 1 and sum(c for o, c in ops.items() if "atomic" in o or "cmpswap" in o) == 1 and ops["s_sleep"] == 0
    for kernel in ("mesh_scan", "mesh_triangles"):
        (body,) = kernel_bodies("mesh", kernel)
        assert sum(c for o, c in opcodes(body).items() if "atomic" in o or "cmpswap" in o or o == "s_sleep") == 0
