// label_host.cpp -- bm_host_label_volume: connected-component labelling of a dense host volume by the rules of label.h, as plain loops:
// every solid voxel starts as its own root, is joined with its solid -x, -y and -z neighbours, and at the end takes its root's label.
// Needs nothing else of the library (no HIP header, no scene): tests/label_check.cpp links this file alone.
#include <string>

#include "../../include/brickmap.h"
#include "label.h"

namespace bm {
// the library's error slot (error.h, defined in scene.cpp); absent -- a null address -- in a program that links this file alone
__attribute__((weak)) void set_error(const std::string& msg);
} // namespace bm

namespace {

int refuse(const char* why) {
	if (bm::set_error) bm::set_error(std::string("bm_host_label_volume: ") + why);
	return BM_EINVAL;
}

struct HostWords {
	int32_t* p;
	uint32_t load(uint32_t i) const { return static_cast<uint32_t>(p[i]); }
	uint32_t fetch_min(uint32_t i, uint32_t v) {
		const uint32_t old = static_cast<uint32_t>(p[i]);
		if (v < old) p[i] = static_cast<int32_t>(v);
		return old;
	}
};

} // namespace

extern "C" int bm_host_label_volume(const uint8_t* voxels, int64_t nx, int64_t ny, int64_t nz, int32_t* labels, uint64_t* count) {
	using namespace bm;
	if (!count) return refuse("null count");
	if (nx < 0 || ny < 0 || nz < 0) return refuse("negative extent");
	const int64_t lim = int64_t{1} << 31;
	if (nx >= lim || ny >= lim || nz >= lim || (ny != 0 && nx > kLabelMaxVoxels / ny) || (nz != 0 && nx * ny > kLabelMaxVoxels / nz))
		return refuse("more than 2^31 - 2 voxels");
	*count = 0;
	const uint32_t X = static_cast<uint32_t>(nx), Y = static_cast<uint32_t>(ny), Z = static_cast<uint32_t>(nz);
	if (X == 0 || Y == 0 || Z == 0) return 0;
	if (!voxels || !labels) return refuse("null volume");
	HostWords w{labels};
	for (uint32_t z = 0; z < Z; ++z)
		for (uint32_t y = 0; y < Y; ++y)
			for (uint32_t x = 0; x < X; ++x) {
				const uint32_t i = label_index(x, y, z, X, Y);
				labels[i] = voxels[i] ? static_cast<int32_t>(i + 1) : 0;
				if (!voxels[i]) continue;
				if (x > 0 && voxels[i - 1]) label_union(w, i, i - 1);
				if (y > 0 && voxels[i - X]) label_union(w, i, i - X);
				if (z > 0 && voxels[i - X * Y]) label_union(w, i, i - X * Y);
			}
	const uint32_t n = X * Y * Z;
	uint64_t roots = 0;
	for (uint32_t i = 0; i < n; ++i) {
		if (!labels[i]) continue;
		labels[i] = static_cast<int32_t>(label_find(w, i) + 1);
		roots += static_cast<uint32_t>(labels[i]) == i + 1;
	}
	*count = roots;
	return 0;
}
