"""Compiled shape of the denoise kernels (denoise.hip; CPU only: hipcc cross-compiles gfx950): every kernel is in the listing, none uses
scratch or spills a register, the tiled kernels stage their taps in LDS and the others use none, and every buffer is addressed as global
memory with 16-byte accesses for the images."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_block_from, usage_blocks

IMG = "PK15HIP_vector_typeIfLj4EE"
KERNELS = {  # mangled prefix: LDS bytes per workgroup (tile 64 x 16 and its halo; 8 bytes per staged pixel for the moments, 24 for a pass)
    "_ZN2bm15denoise_prepareE": 0,
    "_ZN2bm15denoise_momentsILi64ELi16EEE": 70 * 22 * 8,
    "_ZN2bm20denoise_atrous_tiledILi1ELi64ELi16EEE": 68 * 20 * 24,
    "_ZN2bm20denoise_atrous_tiledILi2ELi64ELi16EEE": 72 * 24 * 24,
    "_ZN2bm18denoise_atrous_farE": 0,
    "_ZN2bm10pixel_raysE": 0,
}


def test_every_kernel_is_listed():
    names = [b.split()[0] for b in usage_blocks("denoise")]
    assert len(names) == len(KERNELS)
    for k in KERNELS:
        assert sum(n.startswith(k) for n in names) == 1, k


@pytest.mark.parametrize("kernel", list(KERNELS))
def test_denoise_kernel_resources(kernel):
    block = usage_block_from("denoise", "Function Name: " + kernel)
    assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
    assert field(block, r"LDS Size \[bytes/block\]") == KERNELS[kernel]
    assert field(block, "VGPRs") <= 64  # 8 waves per SIMD as far as registers go
    ops = opcodes(kernel_bodies("denoise", kernel, lambda l: l.startswith(kernel) and l.split(":")[0].startswith(kernel))[0])
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_") or o.startswith("scratch_") or o.startswith("buffer_")) == 0
    assert ops["global_store_dwordx4"] >= 1
    if "pixel_rays" not in kernel:
        assert ops["global_load_dwordx4"] + ops["global_load_dwordx3"] >= 1  # (the moments read c alone: three words)
    if KERNELS[kernel]:
        assert sum(c for o, c in ops.items() if o.startswith("ds_read") or o.startswith("ds_load")) >= 2 and ops["s_barrier"] >= 1
