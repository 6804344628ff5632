// shadowheight_slice.cpp -- the dark heights of a grid on the CPU, built by brickmap_amd/csrc/shadowheight_host.h with the functions of
// shadowheight.h (tools/shadowheight_sim.py compiles and runs this).
// usage: shadowheight_slice <cells xy> <cells z> <dx> <dy> <dz> <extent> <full cells in: bytes [z][y][x]> <dark cells per column out: int32 [y][x]>
// prints the plan; exit status 2 when the sun gets no shadow heights
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../brickmap_amd/csrc/shadowheight_host.h"

int main(int argc, char** argv) {
	using namespace bm;
	if (argc < 9) return 1;
	const int n[3] = {std::atoi(argv[1]), std::atoi(argv[1]), std::atoi(argv[2])};
	const float dir[3] = {static_cast<float>(std::atof(argv[3])), static_cast<float>(std::atof(argv[4])), static_cast<float>(std::atof(argv[5]))};
	const ShadowPlan p = shadow_plan(dir, static_cast<float>(std::atof(argv[6])));
	std::printf("shadow heights: valid %d dom %d bins_per_slab %d..%d rise %d..%d of %d per slab\n", p.valid, p.sun.dom, p.sun.lo1, p.sun.hi1, p.sun.rise, p.rise_hi, kSunHeightUnit);
	if (!p.valid) return 2;
	std::vector<uint8_t> full(static_cast<size_t>(n[0]) * n[1] * n[2]);
	std::vector<int> zd;
	FILE* f = std::fopen(argv[7], "rb");
	if (!f || std::fread(full.data(), 1, full.size(), f) != full.size()) return 1;
	std::fclose(f);
	shadow_heights_host(p, n, full, zd);
	f = std::fopen(argv[8], "wb");
	if (!f || std::fwrite(zd.data(), sizeof(int), zd.size(), f) != zd.size()) return 1;
	std::fclose(f);
	return 0;
}
