// steps.h -- the two innermost bodies of the walk, in the form the kernels run them: one Amanatides-Woo move (src/voxel.cuh:122-130,
// 249-258) and the packed cell of the 8^3 / 2^3 brick walk with its occupancy test; and what a byte of the cube field means.
// Plain C++ (host + device) like jump.h: tests/step_check.cpp replays these very functions against a literal transcription of the
// reference's move and cell arithmetic.
//
// The move stays in compare / select form.  Its mask form (0 / -1 masks from the sign of fp32 differences, `bits(tdelta) & mask`,
// (sx & mx) | (sy & my) | (sz & mz)) is bit-identical on its domain but not faster: the brick loop is a chain of dependent
// instructions around one LDS read and the mask form makes that chain longer, the single move waits for its cube-field byte either
// way (tools/variants/mask_moves.patch, profiles/r07_inner_steps.txt).
#pragma once
#include "jump.h"

namespace bm {

// The reference's choice of the axis (ties: z before y before x); exactly one flag is set.  Any fp32 input: a NaN compares false,
// -0 equals +0.
struct StepAxis {
	bool x, y, z;
};
BM_JHD StepAxis step_choose(float tx, float ty, float tz) {
	StepAxis m;
	m.x = tx < ty && tx < tz;
	m.y = ty <= tx && ty < tz; // x implies !y
	m.z = !(m.x || m.y);
	return m;
}
// select-style (no per-axis branches)
BM_JHD int step_pick(const StepAxis& m, int sx, int sy, int sz) { return m.x ? sx : (m.y ? sy : sz); }
// `t += mask ? delta : 0` is the reference's `tmax += mask * tdelta` for finite deltas
BM_JHD float step_add(float t, float d, bool mask) { return t + (mask ? d : 0.f); }

// ---- the pair move: two single moves whose cube-field bytes are in flight together.  Where a walk goes depends on tmax and tdelta alone;
// the byte of a cell decides whether the lane stops there, not where the next cell is.  So the address of the cell after next is known
// before the first byte is back, and one wait serves both loads:
//     step_pair_ahead    move 1 in full (the arithmetic of one plain move) and, from the new tmax, move 2's axis, increment and cell
//     (the caller loads the bytes of `p` and of `StepAhead::p`, and reads the first: field_state)
//     step_pair_commit   for a lane that move 1 left ST_OUTER (go): move 2 becomes the lane's state, by the plain move's own operations
// A lane that stops at cell 1 drops the second byte and nothing of it needs rolling back: move 2 lives in the StepAhead until committed.
// The same cells in the same order, the same tmax bits and the same last_step as two plain moves, for any fp32 input
// (tests/step_pair_check.cpp); the cell looked at and not committed may lie one increment outside the planes (field_layout.h).
struct StepAhead {
	StepAxis m;  // move 2's axis
	int step;    // ... its increment
	uint32_t p;  // ... and the cell it reaches
};
BM_JHD StepAhead step_pair_ahead(float& tx, float& ty, float& tz, float dx, float dy, float dz, uint32_t& p, int& last_step, int sx, int sy, int sz) {
	const StepAxis m = step_choose(tx, ty, tz);
	const int step = step_pick(m, sx, sy, sz);
	p += static_cast<uint32_t>(step);
	last_step = step;
	tx = step_add(tx, dx, m.x);
	ty = step_add(ty, dy, m.y);
	tz = step_add(tz, dz, m.z);
	StepAhead a;
	a.m = step_choose(tx, ty, tz);
	a.step = step_pick(a.m, sx, sy, sz);
	a.p = p + static_cast<uint32_t>(a.step);
	return a;
}
// go: the lane commits (false: nothing changes).  Cell and increment by select, written in place; tmax only where the lane goes on -- a lane
// that stops keeps the very bits move 1 left it (`t + 0` is not the identity for every fp32 value).
BM_JHD void step_pair_commit(float& tx, float& ty, float& tz, float dx, float dy, float dz, uint32_t& p, int& last_step, const StepAhead& a, bool go) {
	p = go ? a.p : p;
	last_step = go ? a.step : last_step;
	if (go) {
		tx = step_add(tx, dx, a.m.x);
		ty = step_add(ty, dy, a.m.y);
		tz = step_add(tz, dz, a.m.z);
	}
}

// ---- the cell of the brick walk (N = 8: the 8^3 bitmask of a brick; N = 2: the 2^3 LoD mask of the index word), ONE register:
//     bits 5 ...        the voxel's linear index  v = x + N*y + N*N*z  (9 bits for N = 8, 3 for N = 2)
//     bits 15-19, 20-24, 25-29   guard copies of the coordinates, each as (coordinate + 8)
// A move adds ONE per-axis constant, sign * (linear stride << 5 | 1 << guard field).  A coordinate that leaves [0, N) shows in the
// upper bits of its guard field -- "still inside" is one AND and one XOR for all three axes -- and only then may a carry or borrow
// of the linear part run into its neighbours: the walk is over, nothing reads them.  (A borrow that leaves the linear part ends in
// the x guard field, which holds at least 8; a carry ends in the zero bit above the linear part.  An exit's own guard field is 16 or
// 7, one less at most after such a borrow: outside either way.)
// The bitmask of a brick is sixteen 32-bit words, word w = bits 32w ... 32w + 31 of the linear order: the voxel's bit is bit (v & 31)
// of word (v >> 5).  With v at bit 5 the word number sits at bits 10-13 -- for a staging layout that keeps word w of a thread at
// byte w * 1024 + 4 * thread (traverse.h) `cell & 0x3C00` IS the word's address offset -- and the bit number is the low five bits
// of cell >> 5, which is all a 32-bit shift looks at.
template <int N>
struct BrickCell {
	static constexpr int kLog = N == 8 ? 3 : 1;
	static constexpr uint32_t kLin = 5, kGx = 15, kGy = 20, kGz = 25;
	static constexpr uint32_t kOnes = (1u << kGx) | (1u << kGy) | (1u << kGz);
	static constexpr uint32_t kGuard = (~static_cast<uint32_t>(N - 1) & 0x1Fu) * kOnes, kInside = 8u * kOnes;
	static constexpr int kStepX = static_cast<int>((1u << kLin) | (1u << kGx));
	static constexpr int kStepY = static_cast<int>((1u << (kLin + kLog)) | (1u << kGy));
	static constexpr int kStepZ = static_cast<int>((1u << (kLin + 2 * kLog)) | (1u << kGz));
	static constexpr uint32_t kWordMask = 0xFu << (kLin + 5); // N = 8: the word number, in place

	// start cell of a walk from voxel (px, py, pz) (`% N`, then `& (N - 1)`: the latter only defines what the reference leaves
	// undefined, a negative start cell)
	static BM_JHD uint32_t start(int px, int py, int pz) {
		const uint32_t x = static_cast<uint32_t>(px % N) & (N - 1), y = static_cast<uint32_t>(py % N) & (N - 1), z = static_cast<uint32_t>(pz % N) & (N - 1);
		return ((x | (y << kLog) | (z << (2 * kLog))) << kLin) + ((x << kGx) | (y << kGy) | (z << kGz)) + kInside;
	}
	// 0: still inside the block; otherwise bits of the guard fields only (never bit 0)
	static BM_JHD uint32_t outside(uint32_t cell) { return (cell & kGuard) ^ kInside; }
	static BM_JHD uint32_t linear(uint32_t cell) { return (cell >> kLin) & (N * N * N - 1); }
	static BM_JHD uint32_t word(uint32_t cell) { return (cell >> (kLin + 5)) & 0xFu; }
	// occupancy bit of the cell in `w`: its 32-bit word of the brick (N = 8) or the LoD mask (N = 2)
	static BM_JHD uint32_t bit(uint32_t cell, uint32_t w) { return (w >> ((cell >> kLin) & (N == 8 ? 31u : 7u))) & 1u; }
};

// ---- what a byte of the cube field means (traverse.h "cube-field walk"): 0 = the cell holds a brick, 255 = border cell outside the
// grid, n = edge of the empty cube ahead.  `cube` keeps the byte for the walk pass that follows, with a flag when the current tmax is
// outside the range jump.h handles.
enum : int { ST_NEED = 0, ST_OUTER = 1, ST_CAND = 2, ST_JUMP = 3 };
#ifndef BM_JUMP_MIN
#define BM_JUMP_MIN 4 // smallest cube edge worth a jump (a jump costs about four single steps)
#endif
constexpr uint32_t kCubeNoJump = 0x100u; // RayState::cube flag: tmax is outside the range of jump.h, take single moves

// Is a jump WORTH it here -- which is not "is it valid here" (jump_possible, jump.h).  A jump never looks past the end of the binade
// [2^e, 2^(e+1)) of the smallest tmax, a binade is 2^e long and tdelta is at least one cell: below t = 2^BM_JUMP_WORTH_EXP a jump (about
// six single moves' worth of instructions) buys a few cells at most.  Every ray climbs through those binades first, and the primary
// rays of a refill do it together.  The rule is a floor on that exponent (rule (a) of profiles/r17_jump_room.txt; 3 won the sweep of
// 0 ... 4).  tdelta is in the signature for a rule that weighs the room left in the binade against it: rule (b) of the same file, which
// lost and is tools/variants/jump_worth_ride_room.patch.
// A lane that is not worth a jump is ST_OUTER WITHOUT kCubeNoJump: it takes single moves in a single-move pass, and in a jump pass that
// other lanes asked for it jumps as before (valid: jump_worth implies jump_possible) -- the rule only keeps it from asking for one.
// Single moves and jumps land on the same tmax bits, so the rule changes no result; tests/jump_worth_check.cpp.
#ifndef BM_JUMP_WORTH_EXP
#define BM_JUMP_WORTH_EXP 3
#endif
static_assert(BM_JUMP_WORTH_EXP >= BM_JUMP_TMIN_EXP && BM_JUMP_WORTH_EXP < 19, "jump_worth must imply jump_possible");
constexpr uint32_t kJumpWorthBits = static_cast<uint32_t>(127 + BM_JUMP_WORTH_EXP) << 23;
// (the test itself, on the bit pattern of the smallest tmax: the lookup of traverse.h has that minimum already, for jump_possible)
BM_JHD bool jump_worth_bits(uint32_t min_tmax_bits) { return min_tmax_bits - kJumpWorthBits < kJumpMaxBits - kJumpWorthBits; }
BM_JHD bool jump_worth(float tx, float ty, float tz, float dx, float dy, float dz) {
	(void)dx; (void)dy; (void)dz;
	float m = tx < ty ? tx : ty;
	m = m < tz ? m : tz;
	return jump_worth_bits(jump_bits(m));
}

BM_JHD int field_state(uint32_t v, bool possible, uint32_t& cube, bool worth = true) {
	// select-style, no short-circuit: a branchy version costs its full instruction count in a divergent wave anyway
	cube = possible ? v : (v | kCubeNoJump); // remembered for the walk pass, which may be several scheduler rounds away
	const int jump = static_cast<int>(v >= static_cast<uint32_t>(BM_JUMP_MIN)) & static_cast<int>(possible) & static_cast<int>(worth);
	int st = jump ? ST_JUMP : ST_OUTER;
	st = v == 0u ? ST_CAND : st;
	st = v == 255u ? ST_NEED : st; // left the grid (voxel.cuh:256): a miss
	return st;
}

} // namespace bm
