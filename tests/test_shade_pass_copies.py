"""Register copies of the shade pass (CPU only: hipcc cross-compiles gfx950 without a GPU).

bm::trace_paths is bound by vector-instruction issue, and a v_mov_b32 computes nothing.  The shade pass (phase C of
csrc/trace.hip) used to hold three quarters of the kernel's copies: "the next ray" was a set of temporaries assigned in six divergent
branches, which the compiler turns into copies in every branch, plus one v_mov per flag such a branch sets.  Now every input of the
ray set-up has one home, a branch only sets the lane's path state, and the set-up block selects among the homes.  This file keeps it
so.  The measure, for each of the twelve production instantiations: v_mov_b32 in the whole kernel (the product's own listing), and in
the six regions of phase C of a listing built with the Makefile's flags plus -DBM_ISA_MARKERS (comment lines only; an instruction
belongs to the region whose marker precedes it in the listing -- block placement moves code between neighbouring regions, so the
regions are bounded as a sum and reported one by one).

PARENT: the same two builds of the commit before the refactor (c122231).  Bounds: the headline instantiation -- <false, false, true, 2>,
what a uniform launch of 1080p production frames runs -- at least 60 copies below the 253 the refactor set out from (C.connect and
C.hand-over alone held 79, nearly all of it traffic of the removed temporaries; this build of the parent counts 254); every other
instantiation not above its parent, in the whole kernel and in phase C.  NOW: the counts of this tree, pinned with a slack of 5."""
import collections
import os
import re
import subprocess

import pytest

from _compiled import CSRC, kernel_bodies, opcodes

# trace_paths<instrumented = false, XCD-aware hand-out, helper lanes, frame ring> (tests/test_kernel_resources.py)
KERNELS = tuple("_ZN2bm11trace_pathsILb0ELb%dELb%dELi%dE" % (x, h, r) for r in (0, 2, 1) for h in (1, 0) for x in (0, 1))
HEADLINE = "_ZN2bm11trace_pathsILb0ELb0ELb1ELi2E"
C_REGIONS = ("C.connect", "C.shade", "C.sky", "C.hand-over", "C.generate", "C.set-up")
#                                        whole kernel, (connect, shade, sky, hand-over, generate, set-up)
PARENT = dict(zip(KERNELS, (
    (257, (49, 43, 32, 30, 22, 14)), (253, (49, 39, 32, 30, 22, 14)), (220, (36, 41, 30, 0, 1, 16)), (216, (36, 37, 30, 0, 1, 16)),    # one frame
    (254, (49, 43, 32, 30, 22, 14)), (249, (47, 38, 31, 30, 22, 15)), (219, (36, 41, 30, 0, 1, 16)), (216, (36, 37, 30, 0, 0, 17)),    # uniform ring
    (261, (49, 43, 12, 30, 22, 25)), (255, (49, 39, 12, 30, 22, 23)), (221, (36, 41, 12, 0, 23, 26)), (218, (36, 37, 12, 0, 23, 26)))))  # frame ring
#                                     whole kernel, phase C
NOW = dict(zip(KERNELS, ((135, 66), (133, 64), (139, 64), (137, 63),
                         (131, 66), (129, 64), (138, 64), (132, 63),
                         (138, 73), (137, 68), (163, 79), (157, 67))))
HEADLINE_BOUND = 253 - 60
SLACK = 5


@pytest.fixture(scope="module")
def marked_listing(tmp_path_factory):
    """csrc/trace.hip compiled by the Makefile's own rule, flags and all, plus -DBM_ISA_MARKERS, into a directory of its own"""
    build = str(tmp_path_factory.mktemp("marked"))
    target = os.path.join(build, "trace-hip-amdgcn-amd-amdhsa-gfx950.s")
    subprocess.check_call(["make", "-s", "-C", CSRC, "BUILD=" + build, "EXTRA=-DBM_ISA_MARKERS", target], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(target).read().splitlines()


def region_copies(lines, kernel):
    first = next(i for i, l in enumerate(lines) if l.startswith(kernel) and ":" in l)
    body = lines[first:next(i for i in range(first, len(lines)) if lines[i].startswith(".Lfunc_end"))]
    region, movs = "prologue", collections.Counter()
    for l in body:
        m = re.search(r"; BM_REGION (\S+)", l)
        if m:
            region = m.group(1)
        elif l.startswith("\t") and l.split(";")[0].split()[:1] and l.split(";")[0].split()[0].startswith("v_mov_b"):
            movs[region] += 1
    return movs


@pytest.mark.parametrize("KERNEL", KERNELS)
def test_copies_of_the_whole_kernel(KERNEL):
    ops = opcodes(kernel_bodies("trace", KERNEL, lambda l: l.startswith(KERNEL) and ":" in l)[0])
    movs = sum(c for o, c in ops.items() if o.startswith("v_mov_b"))
    print(f"{KERNEL}: {movs} copies (parent {PARENT[KERNEL][0]}, pinned {NOW[KERNEL][0]})")
    assert movs <= PARENT[KERNEL][0], "more copies than before the shade pass named its next ray's inputs"
    if KERNEL == HEADLINE:
        assert movs <= HEADLINE_BOUND, f"{movs} copies: fewer than 60 below the parent's 253"
    assert movs <= NOW[KERNEL][0] + SLACK, f"{movs} copies, {NOW[KERNEL][0]} when this was written: a next-ray temporary or a per-branch flag is back in phase C?"


@pytest.mark.parametrize("KERNEL", KERNELS)
def test_copies_of_the_shade_pass(KERNEL, marked_listing):
    movs = region_copies(marked_listing, KERNEL)
    total, whole = sum(movs[r] for r in C_REGIONS), sum(movs.values())
    print(f"{KERNEL}: phase C {total} of {whole} copies " + ", ".join(f"{r} {movs[r]} (parent {p})" for r, p in zip(C_REGIONS, PARENT[KERNEL][1])))
    assert whole <= PARENT[KERNEL][0]
    assert total <= sum(PARENT[KERNEL][1]), "more copies in phase C than before the refactor"
    if KERNEL == HEADLINE:
        assert whole <= HEADLINE_BOUND and sum(PARENT[KERNEL][1]) - total >= 60, "the 60 copies came out of phase C"
    assert total <= NOW[KERNEL][1] + SLACK, f"phase C: {total} copies, {NOW[KERNEL][1]} when this was written"
