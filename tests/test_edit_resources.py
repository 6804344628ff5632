"""Compiled shape of the voxel-edit kernels (edit.hip; CPU only: hipcc cross-compiles gfx950): no scratch, no spills, and no flat_*
memory instructions -- every buffer is addressed as global memory."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brickmap_amd", "csrc")
KERNELS = ("edit_scatter", "field_pass_x", "field_pass_y", "field_pass_z")


@pytest.fixture(scope="module")
def build_dir():
    subprocess.check_call(["make", "-s", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(CSRC, "build")


@pytest.mark.parametrize("kernel", KERNELS)
def test_edit_kernel_uses_no_scratch_and_no_flat_accesses(kernel, build_dir):
    usage = open(os.path.join(build_dir, "resource_usage_edit.txt")).read()
    start = usage.index(kernel)
    block = usage[start:]
    block = block[:block.index("Function Name", 10)] if "Function Name" in block[10:] else block

    def field(name):
        return int(re.search(name + r": (\d+)", block).group(1))

    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
    lines = open(os.path.join(build_dir, "edit-hip-amdgcn-amd-amdhsa-gfx950.s")).read().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and kernel in l.split(":")[0])  # the kernel's label
    end = next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ops = collections.Counter(l.split(";")[0].split()[0] for l in lines[first:end] if l.startswith("\t") and l.split(";")[0].strip())
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_store") or o.startswith("buffer_load")) == 0
