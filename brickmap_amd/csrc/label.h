// label.h -- the rules of connected-component labelling (bm_scene_label_region, include/brickmap.h), written once for the kernels of
// label.hip and the plain loops of label_host.cpp.  Needs no HIP header: tests/label_check.cpp builds it with a host compiler.
//
// A label volume is its own union-find forest.  The word of voxel i (its index in the box, x fastest) is 0 for an empty voxel, else
// 1 + the index of its parent; a root names itself (word == i + 1).  Two invariants hold from the first store to the last:
//   (a) parent(i) <= i, and every chain of parents stays inside one component;
//   (b) a word only ever decreases.
// So a chain of parents is strictly decreasing and ends at a root after at most i steps, and once nothing is left to join the root of a
// tree is the smallest index of its component: label = 1 + index(first voxel), whatever order the joins ran in.
#pragma once
#include <cstdint>

#include "device_types.h"

namespace bm {

// ---- union-find over the words of a label volume (Playne and Komura's union).  W gives load(i) and fetch_min(i, v) -> the old word.
//
// Stale reads are harmless: by (b) and (a) a value read late is a FORMER parent of i, which is still an ancestor of i in the same
// tree or was linked under one, so following it stays inside the component and only costs steps.  What decides a link is the value
// fetch_min returns, never a value read before it.

// the root of i's tree.  Bounded: every step goes to a strictly smaller index (a).
template <class W>
BM_VHD uint32_t label_find(W& w, uint32_t i) {
	uint32_t word = w.load(i);
	while (word != i + 1) {
		i = word - 1;
		word = w.load(i);
	}
	return i;
}

// join the trees of a and b: the larger root is linked under the smaller one.  Bounded: an attempt that fails found the larger root
// already linked, and goes on from that root's parent, a strictly smaller index; a + b decreases with every failed attempt.
template <class W>
BM_VHD void label_union(W& w, uint32_t a, uint32_t b) {
	a = label_find(w, a);
	b = label_find(w, b);
	while (a != b) {
		if (a < b) { const uint32_t t = a; a = b; b = t; }
		const uint32_t old = w.fetch_min(a, b + 1);
		if (old == a + 1) return; // a was a root until this very operation: linked
		// a had a parent already (old - 1 < a).  If old > b + 1 the minimum moved a under b and a's former parent is still to be joined
		// with b; if old <= b + 1 nothing changed and b is to be joined with that parent.  Either way: the pair (old - 1, b).
		a = label_find(w, old - 1);
		b = label_find(w, b);
	}
}

// ---- labelling inside one brick: 64 x-rows of 8 voxels, row r = y + 8 z; a row's eight labels as 16-bit fields of four words, field x
// of word x >> 1.  A field holds the brick-local index (x + 8 r, < 512) of the smallest voxel known to be connected, 0xFFFF for empty.
struct LabelRow {
	uint32_t w[4];
};
constexpr uint32_t kLabelRowEmpty = 0xFFFFFFFFu;

BM_VHD uint32_t label_min16x2(uint32_t a, uint32_t b) {
	const uint32_t al = a & 0xFFFFu, bl = b & 0xFFFFu, ah = a >> 16, bh = b >> 16;
	return (al < bl ? al : bl) | (ah < bh ? ah : bh) << 16;
}
BM_VHD LabelRow label_row_init(uint32_t bits, uint32_t r) {
	LabelRow row;
	for (int k = 0; k < 4; ++k) {
		const uint32_t lo = (bits >> (2 * k)) & 1u ? 8 * r + 2 * k : 0xFFFFu, hi = (bits >> (2 * k + 1)) & 1u ? 8 * r + 2 * k + 1 : 0xFFFFu;
		row.w[k] = lo | hi << 16;
	}
	return row;
}
BM_VHD LabelRow label_row_min(const LabelRow& a, const LabelRow& b) {
	LabelRow row;
	for (int k = 0; k < 4; ++k) row.w[k] = label_min16x2(a.w[k], b.w[k]);
	return row;
}
BM_VHD uint32_t label_row_get(const LabelRow& row, int x) { return (row.w[x >> 1] >> (16 * (x & 1))) & 0xFFFFu; }

// One round for a row: take the minimum with `near` (the field-wise minimum over the four neighbouring rows, 0xFFFF where a neighbour
// is empty or missing) on the row's solid voxels, then give every run of solid voxels the smallest label in it.  True when a label fell.
BM_VHD bool label_row_settle(LabelRow& row, uint32_t bits, const LabelRow& near) {
	uint32_t l[8];
	for (int x = 0; x < 8; ++x) {
		const uint32_t mine = label_row_get(row, x), other = label_row_get(near, x);
		l[x] = (bits >> x) & 1u ? (other < mine ? other : mine) : 0xFFFFu;
	}
	for (int x = 1; x < 8; ++x)
		if (((bits >> x) & (bits >> (x - 1)) & 1u) && l[x - 1] < l[x]) l[x] = l[x - 1];
	for (int x = 6; x >= 0; --x)
		if (((bits >> x) & (bits >> (x + 1)) & 1u) && l[x + 1] < l[x]) l[x] = l[x + 1];
	bool changed = false;
	for (int k = 0; k < 4; ++k) {
		const uint32_t v = l[2 * k] | l[2 * k + 1] << 16;
		changed = changed || v != row.w[k];
		row.w[k] = v;
	}
	return changed;
}
// The rounds end after at most kLabelBrickRounds of them: after round k every voxel within k face steps of its component's first voxel
// carries that voxel's index, and a path inside a brick has fewer than 512 steps.
constexpr int kLabelBrickRounds = 512;

// ---- the box: index of a voxel (relative coordinates) and the component record's face bits
BM_VHD uint32_t label_index(uint32_t x, uint32_t y, uint32_t z, uint32_t nx, uint32_t ny) { return (z * ny + y) * nx + x; }
constexpr int64_t kLabelMaxVoxels = (int64_t{1} << 31) - 2; // so that every label, 1 + index, is a positive int32

} // namespace bm
