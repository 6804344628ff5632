"""What the compiled-shape tests (test_*_resources.py) share: one `make asm` per process, and readers for what it leaves per kernel
file -- the compiler's resource report and the gfx950 listing (CPU only: hipcc cross-compiles without a GPU)."""
import collections
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "brickmap_amd", "csrc")


@functools.lru_cache(maxsize=None)
def build_dir():
    """csrc/build with every kernel file's listing and report up to date (files that are up to date are not compiled again)"""
    subprocess.check_call(["make", "-s", "-j", str(min(os.cpu_count() or 1, 16)), "-C", CSRC, "asm"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return os.path.join(CSRC, "build")


def usage(name):
    """the resource report of csrc/<name>.hip"""
    return open(os.path.join(build_dir(), "resource_usage.txt" if name == "trace" else f"resource_usage_{name}.txt")).read()


def usage_blocks(name):
    """the report's blocks, one per kernel, each starting with the kernel's mangled name"""
    return usage(name).split("Function Name: ")[1:]


def usage_block_from(name, start):
    """the report's block that begins where `start` first occurs"""
    text = usage(name)
    block = text[text.index(start):]
    return block[:block.index("Function Name", 10)] if "Function Name" in block[10:] else block


def field(block, name):
    return int(re.search(name + r": (\d+)", block).group(1))


def listing(name):
    return open(os.path.join(build_dir(), f"{name}-hip-amdgcn-amd-amdhsa-gfx950.s")).read().splitlines()


def kernel_bodies(name, kernel, is_label=None):
    """the listing's lines of every kernel of csrc/<name>.hip whose label contains `kernel` (or satisfies is_label(line))"""
    lines = listing(name)
    is_label = is_label or (lambda l: l.startswith("_ZN") and kernel in l.split(":")[0])
    firsts = [i for i, l in enumerate(lines) if is_label(l)]
    return [lines[first:next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))] for first in firsts]


def opcodes(body):
    return collections.Counter(l.split(";")[0].split()[0] for l in body if l.startswith("\t") and l.split(";")[0].strip())
