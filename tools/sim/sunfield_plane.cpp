// sunfield_plane.cpp -- the sun plane of an occupancy grid on the CPU, built by brickmap_amd/csrc/sunfield_host.h with the functions of sunfield.h, slab by slab
// as sunfield.hip builds it (tools/sunfield_sim.py compiles and runs this).
// usage: sunfield_plane <cells xy> <cells z> <dx> <dy> <dz> <extent> <occupancy in: bytes [z][y][x]> <plane out: bytes [z][y][x]>
// prints the plan; exit status 2 when the sun gets no plane
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../brickmap_amd/csrc/sunfield_host.h"

int main(int argc, char** argv) {
	using namespace bm;
	if (argc < 9) return 1;
	const int n[3] = {std::atoi(argv[1]), std::atoi(argv[1]), std::atoi(argv[2])};
	const float dir[3] = {static_cast<float>(std::atof(argv[3])), static_cast<float>(std::atof(argv[4])), static_cast<float>(std::atof(argv[5]))};
	const SunPlan p = sun_plan(dir, static_cast<float>(std::atof(argv[6])));
	std::printf("valid %d octant %d dom %d bins_per_slab %d..%d %d..%d clear %d rise %d\n", p.valid, p.octant, p.dom, p.lo1, p.hi1, p.lo2, p.hi2, p.clear, p.rise);
	if (!p.valid) return 2;
	std::vector<uint8_t> occ(static_cast<size_t>(n[0]) * n[1] * n[2]), plane;
	FILE* f = std::fopen(argv[7], "rb");
	if (!f || std::fread(occ.data(), 1, occ.size(), f) != occ.size()) return 1;
	std::fclose(f);
	sun_plane_host(p, n, occ, plane);
	f = std::fopen(argv[8], "wb");
	if (!f || std::fwrite(plane.data(), 1, plane.size(), f) != plane.size()) return 1;
	std::fclose(f);
	return 0;
}
