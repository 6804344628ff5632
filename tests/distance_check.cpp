// distance_check.cpp -- the rules of csrc/distance.h and the host routine of csrc/distance_host.cpp, checked without a device and without
// the rest of the library (tests/test_distance_host.py builds this file with distance_host.cpp alone, plain and under the sanitizers).
//
//   patterns : the line rule against a brute-force 1-D minimum for all 2^12 site patterns of length 12 with f = 0
//   lines    : the same for random lines of length 1 ... 200 with random f that include none (argv[1] of them)
//   short    : every line of length 2 and 3 over f in {0, 1, 4, 9, none}
//   volumes  : a volume walked lane by lane the way the kernels walk it -- rows in chunks of 64 lanes with the carried and the looked-ahead
//              source (short rows as segments of a wave), the line passes with their stacks in one [entry][line] array and the top entry
//              in a LineTop, the border term, the key per wave of 64 lanes -- against bm_host_distance_field's plain loops
//   refused  : what the host routines refuse
//
// Prints the counts and `failures 0`.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../brickmap_amd/csrc/distance.h"
#include "../include/brickmap.h"

using namespace bm;

namespace {

long failures = 0;

void fail(const char* what, long a, long b, long c) {
	if (++failures <= 20) std::printf("FAIL %s %ld %ld %ld\n", what, a, b, c);
}

// the line rule with a stack of its own
std::vector<uint32_t> envelope(const std::vector<uint32_t>& f) {
	const uint32_t n = static_cast<uint32_t>(f.size());
	std::vector<uint32_t> stack(n), out(n);
	auto f_at = [&](uint32_t j) { return f[j]; };
	auto load_entry = [&](uint32_t k) { return stack[k]; };
	auto store_entry = [&](uint32_t k, uint32_t e) { stack[k] = e; };
	LineTop top = {0u, 0u, 0u, 0u};
	for (uint32_t u = 0; u < n; ++u)
		if (f[u] != kDistanceNone) distance_line_push(top, u, f[u], n, load_entry, store_entry, f_at);
	for (uint32_t u = n; u-- > 0;) out[u] = distance_line_emit(top, u, load_entry, f_at);
	return out;
}

std::vector<uint32_t> brute(const std::vector<uint32_t>& f) {
	const int64_t n = static_cast<int64_t>(f.size());
	std::vector<uint32_t> out(f.size());
	for (int64_t u = 0; u < n; ++u) {
		int64_t best = kDistanceNone;
		for (int64_t j = 0; j < n; ++j)
			if (f[j] != kDistanceNone && f[j] + (u - j) * (u - j) < best) best = f[j] + (u - j) * (u - j);
		out[u] = static_cast<uint32_t>(best);
	}
	return out;
}

void check_line(const std::vector<uint32_t>& f, const char* what, long tag) {
	const std::vector<uint32_t> a = envelope(f), b = brute(f);
	for (size_t u = 0; u < f.size(); ++u)
		if (a[u] != b[u]) {
			fail(what, tag, static_cast<long>(u), static_cast<long>(a[u]));
			return;
		}
}

// ---- a volume, lane by lane
struct Walk {
	std::vector<uint32_t> field;
	bm_distance_result result;
};

// the x pass of one wave: rows row0 ... of S lanes each
void wave_x(const uint8_t* volume, const DistanceDims& d, uint32_t shift, uint64_t wave, std::vector<uint32_t>& field, uint64_t& sources) {
	const uint32_t S = 1u << shift, rows = static_cast<uint32_t>(d.extent[1]) * static_cast<uint32_t>(d.extent[2]);
	const int32_t nx = d.extent[0];
	// the ballot of a chunk: lane by lane, the voxel's byte (the kernel's words and single bytes read the same bytes)
	auto ballot = [&](int32_t c0) {
		uint64_t all = 0;
		for (uint32_t lane = 0; lane < 64; ++lane) {
			const uint32_t l = lane & (S - 1u), seg = lane >> shift;
			const uint64_t row = (wave << (6u - shift)) + seg;
			const int32_t x = c0 + static_cast<int32_t>(l);
			if (row >= rows || x >= nx) continue;
			const uint32_t z = static_cast<uint32_t>(row) / static_cast<uint32_t>(d.extent[1]), y = static_cast<uint32_t>(row) - z * static_cast<uint32_t>(d.extent[1]);
			if (distance_is_source(volume[z * d.slice_pitch + y * d.row_pitch + x], d.to_empty)) all |= uint64_t{1} << lane;
		}
		return all;
	};
	auto store = [&](uint32_t lane, int32_t x, int32_t g) {
		const uint32_t seg = lane >> shift;
		const uint64_t row = (wave << (6u - shift)) + seg;
		if (row < rows && x < nx) field[row * static_cast<uint64_t>(nx) + static_cast<uint64_t>(x)] = g < kDistanceMaxExtent ? distance_sq(g) : kDistanceNone;
	};
	if (shift < 6u) {
		const uint64_t all = ballot(0);
		sources += static_cast<uint64_t>(__builtin_popcountll(all));
		for (uint32_t lane = 0; lane < 64; ++lane) {
			const uint32_t l = lane & (S - 1u), seg = lane >> shift;
			const uint64_t m = (all >> (seg << shift)) & ((uint64_t{1} << S) - 1u);
			store(lane, static_cast<int32_t>(l), distance_chunk_nearest(m, l, static_cast<int32_t>(l), -1, -1));
		}
		return;
	}
	const int32_t chunks = (nx + 63) >> 6;
	int32_t left = -1, ahead = -1, scanned = 1, kept_chunk = 0;
	uint64_t kept = ballot(0);
	long reads = 1;
	for (int32_t c = 0; c < chunks; ++c) {
		const int32_t c0 = c << 6;
		if (c >= scanned) fail("a chunk that was not read", c, scanned, 0);
		const uint64_t m = c == kept_chunk ? kept : 0u;
		if (m != ballot(c0)) fail("a chunk's mask", c, kept_chunk, 0);
		sources += static_cast<uint64_t>(__builtin_popcountll(m));
		if (ahead < c0 + 64) {
			ahead = -1;
			while (scanned < chunks && ahead < 0) {
				const uint64_t next = ballot(scanned << 6);
				++reads;
				if (next != 0) {
					ahead = (scanned << 6) + __builtin_ctzll(next);
					kept = next;
					kept_chunk = scanned;
				}
				++scanned;
			}
		}
		for (uint32_t lane = 0; lane < 64; ++lane) store(lane, c0 + static_cast<int32_t>(lane), distance_chunk_nearest(m, lane, c0 + static_cast<int32_t>(lane), left, ahead));
		if (m != 0) left = c0 + 63 - __builtin_clzll(m);
	}
	if (reads != chunks) fail("every chunk is read once", reads, chunks, 0);
}

// a line pass, one lane per line, the lanes' stacks interleaved in `stack`; key: null, or the last pass's
void lanes_line(const std::vector<uint32_t>& in, std::vector<uint32_t>& out, std::vector<uint32_t>& stack, uint64_t* key, const DistanceDims& d, uint32_t lines, uint32_t n,
				uint32_t stride, uint32_t row_step) {
	const uint32_t nx = static_cast<uint32_t>(d.extent[0]);
	uint64_t wave_best = 0;
	for (uint32_t line = 0; line < lines; ++line) {
		const uint32_t r = line / nx, x = line - r * nx;
		const size_t base = static_cast<size_t>(r) * row_step + x;
		auto f_at = [&](uint32_t j) { return in.at(base + static_cast<size_t>(j) * stride); };
		auto load_entry = [&](uint32_t k) { return stack.at(static_cast<size_t>(k) * lines + line); };
		auto store_entry = [&](uint32_t k, uint32_t e) { stack.at(static_cast<size_t>(k) * lines + line) = e; };
		LineTop top = {0u, 0u, 0u, 0u};
		for (uint32_t u = 0; u < n; ++u) {
			const uint32_t f = f_at(u);
			if (f != kDistanceNone) distance_line_push(top, u, f, n, load_entry, store_entry, f_at);
		}
		uint64_t best = 0;
		for (uint32_t u = n; u-- > 0;) {
			uint32_t v = distance_line_emit(top, u, load_entry, f_at);
			const size_t index = base + static_cast<size_t>(u) * stride;
			if (key) {
				if (d.outside) {
					const uint32_t edge = distance_outside_sq(d.extent, static_cast<int32_t>(x), static_cast<int32_t>(r), static_cast<int32_t>(u));
					v = edge < v ? edge : v;
				}
				const uint64_t k = distance_max_key(v, static_cast<uint32_t>(index));
				best = k > best ? k : best;
			}
			out.at(index) = v;
		}
		wave_best = best > wave_best ? best : wave_best;
		if (key && ((line & 63u) == 63u || line + 1 == lines)) { // the wave's butterfly and its one atomic
			if (wave_best > *key) *key = wave_best;
			wave_best = 0;
		}
	}
}

Walk walk(const uint8_t* volume, const bm_distance_params& params) {
	const DistanceDims d = distance_dims(distance_params_view(params));
	const uint32_t nx = static_cast<uint32_t>(d.extent[0]), ny = static_cast<uint32_t>(d.extent[1]), nz = static_cast<uint32_t>(d.extent[2]);
	Walk w;
	w.field.assign(d.voxels, 0xDEADBEEFu);
	std::vector<uint32_t> h(distance_plane_bytes(d) / 4, 0xDEADBEEFu), stack(distance_plane_bytes(d) / 4, 0xDEADBEEFu);
	uint64_t tail[2] = {0, 0};
	const uint32_t shift = distance_row_shift(d.extent[0]);
	const uint64_t rows = static_cast<uint64_t>(ny) * nz, per_wave = 64u >> shift, waves = (rows + per_wave - 1) / per_wave;
	for (uint64_t wave = 0; wave < waves; ++wave) wave_x(volume, d, shift, wave, w.field, tail[1]);
	lanes_line(w.field, h, stack, nullptr, d, nx * nz, ny, nx, nx * ny);
	lanes_line(h, w.field, stack, &tail[0], d, nx * ny, nz, nx * ny, nx);
	const DistanceRecord rec = distance_record(tail[0], tail[1]);
	w.result = {rec.sources, rec.max_sq, rec.reserved0, rec.max_at, rec.reserved1};
	return w;
}

} // namespace

int main(int argc, char** argv) {
	const long rounds = argc > 1 ? std::atol(argv[1]) : 100000;
	std::mt19937_64 rng(12345);
	long patterns = 0, lines = 0, shorts = 0, volumes = 0, refused = 0;

	for (uint32_t bits = 0; bits < 4096; ++bits, ++patterns) {
		std::vector<uint32_t> f(12);
		for (int k = 0; k < 12; ++k) f[k] = (bits >> k) & 1u ? 0u : kDistanceNone;
		check_line(f, "pattern", bits);
	}

	for (long i = 0; i < rounds; ++i, ++lines) {
		const size_t n = 1 + rng() % 200;
		const uint32_t scale = (i % 4 == 0) ? 50u : (i % 4 == 1) ? 2000u : (i % 4 == 2) ? 40000u : (1u << 29);
		const uint32_t holes = static_cast<uint32_t>(rng() % 5); // none for one value in 1 ... 5, or never
		std::vector<uint32_t> f(n);
		for (auto& v : f) v = (holes && rng() % (holes + 1) == 0) ? kDistanceNone : static_cast<uint32_t>(rng() % scale);
		check_line(f, "line", i);
	}

	const uint32_t values[5] = {0u, 1u, 4u, 9u, kDistanceNone};
	for (int a = 0; a < 5; ++a)
		for (int b = 0; b < 5; ++b) {
			check_line({values[a], values[b]}, "short2", 5 * a + b);
			++shorts;
			for (int c = 0; c < 5; ++c, ++shorts) check_line({values[a], values[b], values[c]}, "short3", 25 * a + 5 * b + c);
		}

	// (nx, ny, nz): rows of one lane, of segments, of one chunk exactly, of several chunks with a ragged last one; lines past a wave
	const int shapes[][3] = {{1, 1, 1}, {1, 5, 3}, {2, 3, 40}, {5, 7, 3}, {17, 3, 2}, {31, 2, 3}, {32, 3, 3}, {33, 2, 2}, {64, 2, 3}, {65, 3, 2}, {130, 2, 2}, {200, 3, 2}, {3, 70, 2}, {70, 2, 67}};
	const double densities[] = {0.0, 0.004, 0.05, 0.5, 1.0};
	for (const auto& s : shapes)
		for (double density : densities)
			for (uint32_t flags = 0; flags < 4; ++flags, ++volumes) {
				// a volume with pitches above its extents, at an odd place of its buffer
				const int64_t row = s[0] + 3, slice = row * (s[1] + 1);
				std::vector<uint8_t> buffer(static_cast<size_t>(slice * s[2] + 5), 0);
				for (auto& v : buffer) v = (rng() % 1000000) < density * 1000000 ? static_cast<uint8_t>(1 + rng() % 255) : 0;
				bm_distance_params p{};
				p.extent[0] = s[0], p.extent[1] = s[1], p.extent[2] = s[2];
				p.row_pitch = row, p.slice_pitch = slice, p.flags = flags;
				std::vector<uint32_t> want(static_cast<size_t>(s[0]) * s[1] * s[2], 0xDEADBEEFu);
				bm_distance_result res{};
				if (bm_host_distance_field(&p, buffer.data() + 3, want.data(), &res) != 0) fail("host", s[0], s[1], s[2]);
				const Walk w = walk(buffer.data() + 3, p);
				if (w.field != want) fail("walk field", s[0], s[1] * 1000 + s[2], static_cast<long>(flags));
				if (w.result.sources != res.sources || w.result.max_sq != res.max_sq || w.result.max_at != res.max_at || res.reserved0 != 0 || res.reserved1 != 0)
					fail("walk record", s[0], s[1] * 1000 + s[2], static_cast<long>(flags));
				// the mask of both
				std::vector<uint8_t> mask(want.size(), 7);
				if (bm_host_distance_mask(want.size(), want.data(), 4, flags & 1u, mask.data()) != 0) fail("mask", 0, 0, 0);
				for (size_t i = 0; i < want.size(); ++i)
					if (mask[i] != (((want[i] <= 4) != ((flags & 1u) != 0)) ? 1 : 0)) {
						fail("mask byte", static_cast<long>(i), mask[i], static_cast<long>(want[i]));
						break;
					}
			}

	{ // refusals: nothing is written
		uint8_t v[8] = {1, 0, 0, 0, 0, 0, 0, 1};
		uint32_t f[8];
		uint8_t m[8];
		bm_distance_result r{};
		auto refuse = [&](bm_distance_params p, const uint8_t* vol, uint32_t* field, bm_distance_result* res) {
			for (auto& x : f) x = 77;
			r.sources = 77;
			if (bm_host_distance_field(&p, vol, field, res) != BM_EINVAL) fail("not refused", refused, 0, 0);
			for (auto x : f)
				if (x != 77) fail("refused but written", refused, 0, 0);
			if (r.sources != 77) fail("refused but written", refused, 1, 0);
			++refused;
		};
		bm_distance_params ok{};
		ok.extent[0] = 2, ok.extent[1] = 2, ok.extent[2] = 2;
		bm_distance_params p = ok;
		p.extent[0] = 0; refuse(p, v, f, &r);
		p = ok; p.extent[2] = 16385; refuse(p, v, f, &r);
		p = ok; p.extent[0] = p.extent[1] = 16384; p.extent[2] = 8; refuse(p, v, f, &r);
		p = ok; p.row_pitch = 1; refuse(p, v, f, &r);
		p = ok; p.row_pitch = -2; refuse(p, v, f, &r);
		p = ok; p.slice_pitch = 3; refuse(p, v, f, &r);
		p = ok; p.flags = 4; refuse(p, v, f, &r);
		p = ok; p.reserved = 1; refuse(p, v, f, &r);
		refuse(ok, nullptr, f, &r);
		refuse(ok, v, nullptr, &r);
		refuse(ok, v, f, nullptr);
		if (bm_host_distance_field(nullptr, v, f, &r) != BM_EINVAL) fail("null params", 0, 0, 0);
		++refused;
		if (bm_host_distance_mask(0, f, 1, 0, m) != BM_EINVAL || bm_host_distance_mask(8, f, 1, 2, m) != BM_EINVAL) fail("mask refusals", 0, 0, 0);
		++refused;
		if (bm_host_distance_mask(8, nullptr, 1, 0, m) != BM_EINVAL || bm_host_distance_mask(8, f, 1, 0, nullptr) != BM_EINVAL) fail("mask null", 0, 0, 0);
		++refused;
		if (bm_host_distance_field(&ok, v, f, &r) != 0 || f[0] != 0 || f[1] != 1 || f[6] != 1 || f[3] != 1 || r.sources != 2 || r.max_sq != 1 || r.max_at != 1) fail("the volume that is not refused", f[3], r.max_sq, 0);
	}

	std::printf("patterns %ld lines %ld short %ld volumes %ld refused %ld failures %ld\n", patterns, lines, shorts, volumes, refused, failures);
	return failures == 0 ? 0 : 1;
}
