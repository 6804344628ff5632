"""Compiled shape of the kernels of label.hip (connected components of a live scene; CPU only: hipcc cross-compiles gfx950): every kernel
is listed, none uses scratch, spills registers or has flat_*, scratch_* or buffer_* memory instructions; merge reaches the label volume
through atomics alone; the register counts and the waves per SIMD they leave are those DESIGN.md 4.14 quotes."""
import pytest

from _compiled import field, kernel_bodies, opcodes, usage_blocks

# (kernel, number of instantiations): label_local exists for the cells of the box and for the staged list
KERNELS = (("label_local", 2), ("label_merge", 1), ("label_flatten", 1), ("label_roots_count", 1), ("label_scan", 1), ("label_roots_write", 1),
           ("label_accumulate", 1), ("label_finish", 1), ("label_mask", 1))
# the most VGPRs each kernel may take (DESIGN.md 4.14 quotes the compiled numbers): all leave 8 waves per SIMD, the most gfx950 runs
VGPR_BOUND = {"label_local": 64, "label_merge": 32, "label_flatten": 32, "label_roots_count": 32, "label_scan": 32, "label_roots_write": 32,
              "label_accumulate": 48, "label_finish": 32, "label_mask": 32}


def test_every_kernel_of_the_file_is_listed():
    names = [b.split()[0] for b in usage_blocks("label")]
    assert len(names) == sum(n for _, n in KERNELS) and all(any(k in name for k, _ in KERNELS) for name in names), names


@pytest.mark.parametrize("kernel,instances", KERNELS)
def test_label_kernel_uses_no_scratch_and_no_flat_accesses(kernel, instances):
    blocks = [b for b in usage_blocks("label") if kernel in b.split()[0]]
    assert len(blocks) == instances
    for block in blocks:
        assert field(block, r"ScratchSize \[bytes/lane\]") == 0 and field(block, "VGPRs Spill") == 0 and field(block, "SGPRs Spill") == 0
        assert field(block, "VGPRs") <= VGPR_BOUND[kernel] and field(block, r"Occupancy \[waves/SIMD\]") == 8
    bodies = kernel_bodies("label", kernel)
    assert len(bodies) == instances
    for body in bodies:
        ops = opcodes(body)
        assert ops, f"no instructions found for {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("flat_")) == 0, f"flat_* accesses in {kernel}"
        assert sum(c for o, c in ops.items() if o.startswith("scratch_") or o.startswith("buffer_")) == 0
        assert sum(c for o, c in ops.items() if o.startswith("global_")) > 0


def test_merge_links_with_atomic_minimum_and_stores_nothing_plainly():
    """every write of merge is the union's atomic minimum (returning the old word), every read of a label an agent-scope load (sc1);
    no compare-and-swap loop and no wait for another workgroup (no s_sleep)"""
    (body,) = kernel_bodies("label", "label_merge")
    ops = opcodes(body)
    assert ops["global_atomic_umin"] >= 1 and sum(c for o, c in ops.items() if o.startswith("global_store")) == 0
    assert sum(c for o, c in ops.items() if "cmpswap" in o) == 0 and ops["s_sleep"] == 0
    loads = [l for l in body if l.startswith("\tglobal_load")]
    assert loads and all(" sc1" in l.split(";")[0] for l in loads), [l for l in loads if " sc1" not in l]


def test_local_labels_in_registers_and_stores_eight_words_per_lane():
    """the in-brick rounds exchange rows by lane permutes, not through memory: no global access inside the loop other than none at all --
    the loads come first, the (at most 8) stores last"""
    for body in kernel_bodies("label", "label_local"):
        ops = opcodes(body)
        assert ops["ds_bpermute_b32"] >= 16 and 1 <= sum(c for o, c in ops.items() if o.startswith("global_store")) <= 8
        assert sum(c for o, c in ops.items() if o.startswith("global_atomic")) == 0


def test_components_add_with_integer_atomics():
    (body,) = kernel_bodies("label", "label_accumulate")
    ops = opcodes(body)
    assert ops["global_atomic_add_x2"] >= 1 and ops["global_atomic_or"] >= 1 and ops["global_atomic_smin"] >= 3 and ops["global_atomic_smax"] >= 3
    assert sum(c for o, c in ops.items() if "cmpswap" in o) == 0
