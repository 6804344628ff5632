"""Compiled shape of the ray-query kernel (query.hip; CPU only: hipcc cross-compiles gfx950): both instantiations run without scratch
or spills, address every buffer as global memory (no flat_*, scratch_* or buffer_* instructions), and keep at least 7 waves per SIMD
resident."""
import collections
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brickmap_amd", "csrc")
WAVES_PER_SIMD = 7
INSTANTIATIONS = ("_ZN2bm10query_raysILb0EEE", "_ZN2bm10query_raysILb1EEE")  # <REQUEST = false>, <REQUEST = true>


@pytest.fixture(scope="module")
def build_dir():
    subprocess.check_call(["make", "-s", "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(CSRC, "build")


@pytest.mark.parametrize("kernel", INSTANTIATIONS)
def test_query_kernel_resources(kernel, build_dir):
    usage = open(os.path.join(build_dir, "resource_usage_query.txt")).read()
    start = usage.index("Function Name: " + kernel)
    block = usage[start:]
    block = block[:block.index("Function Name", 10)] if "Function Name" in block[10:] else block

    def field(name):
        return int(re.search(name + r": (\d+)", block).group(1))

    assert field(r"ScratchSize \[bytes/lane\]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
    assert field(r"Occupancy \[waves/SIMD\]") >= WAVES_PER_SIMD
    lines = open(os.path.join(build_dir, "query-hip-amdgcn-amd-amdhsa-gfx950.s")).read().splitlines()
    first = next(i for i, l in enumerate(lines) if l.startswith(kernel) and l.split(":")[0].startswith(kernel))  # the kernel's label
    end = next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))
    ops = collections.Counter(l.split(";")[0].split()[0] for l in lines[first:end] if l.startswith("\t") and l.split(";")[0].strip())
    assert ops, f"no instructions found for {kernel}"
    assert sum(c for o, c in ops.items() if o.startswith("flat_") or o.startswith("scratch_") or o.startswith("buffer_")) == 0
    # 16-byte record loads and stores, bricks staged straight into LDS
    assert ops["global_load_dwordx4"] >= 2 and ops["global_store_dwordx4"] >= 2 and ops["global_load_lds_dword"] >= 16
