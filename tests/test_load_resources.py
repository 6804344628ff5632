"""Compiled shape of the kernels of load.hip (dense voxels -> scene; CPU only: hipcc cross-compiles gfx950): no scratch, no spills, and
no flat_* memory instructions -- every buffer is addressed as global memory."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brickmap_amd", "csrc")
# (kernel, number of instantiations): classify and pack exist for 16-byte aligned volumes and for any other
KERNELS = (("load_classify", 2), ("load_number", 1), ("load_scan", 1), ("load_pack", 2))


@pytest.fixture(scope="module")
def build_dir():
    subprocess.check_call(["make", "-s", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(CSRC, "build")


@pytest.mark.parametrize("kernel,instances", KERNELS)
def test_load_kernel_uses_no_scratch_and_no_flat_accesses(kernel, instances, build_dir):
    usage = open(os.path.join(build_dir, "resource_usage_load.txt")).read()
    blocks = [b for b in usage.split("Function Name: ")[1:] if kernel in b.split()[0]]
    assert len(blocks) == instances

    for block in blocks:
        def field(name):
            return int(re.search(name + r": (\d+)", block).group(1))

        assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
    lines = open(os.path.join(build_dir, "load-hip-amdgcn-amd-amdhsa-gfx950.s")).read().splitlines()
    firsts = [i for i, l in enumerate(lines) if l.startswith("_ZN") and kernel in l.split(":")[0]]  # the kernels' labels
    assert len(firsts) == instances
    for first in firsts:
        end = next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))
        ops = collections.Counter(l.split(";")[0].split()[0] for l in lines[first:end] if l.startswith("\t") and l.split(";")[0].strip())
        assert ops, f"no instructions found for {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_store") or o.startswith("buffer_load")) == 0
        assert sum(c for o, c in ops.items() if o.startswith("global_load") or o.startswith("global_store")) > 0


def test_volume_reads_are_16_bytes_wide(build_dir):
    """the aligned classify and pack kernels read the volume as 16 bytes per lane: eight lanes cover a 128-byte line"""
    lines = open(os.path.join(build_dir, "load-hip-amdgcn-amd-amdhsa-gfx950.s")).read().splitlines()
    for kernel in ("load_classifyILb1", "load_packILb1"):
        first = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and kernel in l.split(":")[0])
        end = next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))
        assert sum(1 for l in lines[first:end] if l.strip().startswith("global_load_dwordx4")) == 2
