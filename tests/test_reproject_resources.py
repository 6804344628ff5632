"""Compiled shape of the reprojection kernel (reproject.hip; CPU only: hipcc cross-compiles gfx950): the kernel is in the listing, uses no
scratch, no LDS and spills no register, and every buffer is addressed as global memory with 16-byte accesses for the image, hit and
history words."""
from _compiled import field, kernel_bodies, opcodes, usage_block_from, usage_blocks

KERNEL = "_ZN2bm9reprojectE"


def test_the_kernel_is_listed():
    names = [b.split()[0] for b in usage_blocks("reproject")]
    assert len(names) == 1 and names[0].startswith(KERNEL), names


def test_reproject_kernel_resources():
    block = usage_block_from("reproject", "Function Name: " + KERNEL)
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, r"LDS Size \[bytes/block\]") == 0
    assert field(block, "VGPRs") <= 64  # 8 waves per SIMD as far as registers go
    ops = opcodes(kernel_bodies("reproject", KERNEL, lambda l: l.startswith(KERNEL) and l.split(":")[0].startswith(KERNEL))[0])
    assert ops, "no instructions found for the kernel"
    assert sum(c for o, c in ops.items() if o.startswith("flat_") or o.startswith("scratch_") or o.startswith("buffer_")) == 0
    assert ops["global_load_dwordx4"] >= 1 and ops["global_store_dwordx4"] >= 1
