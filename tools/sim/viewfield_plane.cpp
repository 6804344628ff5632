// viewfield_plane.cpp -- the view plane of an occupancy grid on the CPU, built by brickmap_amd/csrc/viewfield_host.h with the functions of viewfield.h
// (tools/viewfield_sim.py compiles and runs this).
// usage: viewfield_plane <cells xy> <cells z> <ox> <oy> <oz> <occupancy in: bytes [z][y][x]> <out>        (origin in voxels)
// out: the view plane, then the eight octant planes, bytes [z][y][x] each, then the eight escape thresholds of the camera's column as int32
// prints the plan; exit status 2 when the position gets no plane
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../brickmap_amd/csrc/viewfield_host.h"

int main(int argc, char** argv) {
	using namespace bm;
	if (argc < 8) return 1;
	const int n[3] = {std::atoi(argv[1]), std::atoi(argv[1]), std::atoi(argv[2])};
	const float origin[3] = {static_cast<float>(std::atof(argv[3])), static_cast<float>(std::atof(argv[4])), static_cast<float>(std::atof(argv[5]))};
	const ViewPlan v = view_plan(origin, 0.f, 8.f * n[0], 8.f * n[2], n[0], n[2]);
	std::printf("valid %d cell %d %d %d margin %g cap %d\n", v.valid, v.cell[0], v.cell[1], v.cell[2], v.margin, kViewCap);
	if (!v.valid) return 2;
	std::vector<uint8_t> occ(static_cast<size_t>(n[0]) * n[1] * n[2]), plane;
	FILE* f = std::fopen(argv[6], "rb");
	if (!f || std::fread(occ.data(), 1, occ.size(), f) != occ.size()) return 1;
	std::fclose(f);
	const ViewHostField field = view_host_field(n, occ);
	view_plane_host(v, field, plane);
	f = std::fopen(argv[7], "wb");
	if (!f || std::fwrite(plane.data(), 1, plane.size(), f) != plane.size()) return 1;
	for (int o = 0; o < 8; ++o) if (std::fwrite(field.cube[o].data(), 1, plane.size(), f) != plane.size()) return 1;
	int32_t e[8];
	for (int o = 0; o < 8; ++o) e[o] = field.threshold(o, v.cell[0], v.cell[1]);
	if (std::fwrite(e, 4, 8, f) != 8) return 1;
	std::fclose(f);
	return 0;
}
