// examples/headless_main.cpp -- the reference's main loop (src/main.cpp:100-147) without the window:
// State + Scene + generate(), then per frame launch_kernels -> process_load_queue, finally a PPM of the
// resolved frame.  Build: see `make -C examples` (g++ on this file, linked against libbrickmap_hip.so).
//   usage: headless_main [--denoise] [--temporal] [--voxels FILE] [--paste FILE:nx,ny,nz@x,y,z] [--mesh FILE@x,y,z] [--mesh-out x0,y0,z0:x1,y1,z1=FILE] [--dig x,y,z,r] [--grow x0,y0,z0:x1,y1,z1=r2] [--shrink x0,y0,z0:x1,y1,z1=r2] [--path x0,y0,z0:x1,y1,z1] [--walk x0,y0,z0:x1,y1,z1] [--pools x0,y0,z0:x1,y1,z1] [--drop-floating x0,y0,z0:x1,y1,z1] [--settle x0,y0,z0:x1,y1,z1] [--dig-at px,py,r] [--ground x,y] [grid_size grid_height width height frames out.ppm [wavefront | ring]]
// --voxels FILE: the world is FILE instead of the generated terrain -- raw bytes, one per voxel, [z][y][x] with x fastest,
// grid_size * grid_size * grid_height of them, non-zero = solid (Scene::load_voxels; the scene is resident afterwards).
// --paste FILE:nx,ny,nz@x,y,z writes the raw volume FILE (nx * ny * nz bytes, [z][y][x], non-zero = solid) into the world with its
// first voxel at (x, y, z) before the first frame, replacing what was there (Scene::write_region; clipped to the world).
// --mesh FILE@x,y,z adds a triangle mesh to the world after --paste: FILE is raw, 9 floats per triangle (xyz per vertex, in voxels), moved
// by (x, y, z); it is voxelized on the GPU over its own bounds -- every voxel a triangle touches and every voxel whose centre lies inside
// the closed mesh -- and written with "set" (Scene::write_mesh).  Prints the triangle counts and `open columns`, 0 for a closed mesh.
// --mesh-out x0,y0,z0:x1,y1,z1=FILE, applied after every edit above and below (--dig, --drop-floating, --dig-at): the surface of that box
// of the world, closed at the box's sides, is extracted on the GPU as quads merged inside the 8^3 cells (Scene::extract_mesh) and written
// to FILE as triangles in the raw format --mesh reads; prints the counts of quads, faces and triangles.
// --dig carves a sphere of radius r voxels around voxel (x, y, z) out of the world before the first frame (Scene::carve_sphere).
// --grow x0,y0,z0:x1,y1,z1=r2 and --shrink x0,y0,z0:x1,y1,z1=r2, applied after --dig (grow first): the world inside that box is dilated or
// eroded with a Euclidean ball of squared radius r2 -- the exact distance field of the box and a margin on the GPU, thresholded and written
// back (Scene::grow, Scene::shrink); prints how many voxels changed.
// --path x0,y0,z0:x1,y1,z1, applied after --dig, --grow and --shrink: a shortest face-step path through the empty voxels from the first
// voxel to the second, by the exact travel field of their surroundings on the GPU (Scene::find_path); prints "path of N voxels:" and the
// voxels, or "no path".
// --walk x0,y0,z0:x1,y1,z1, applied where --path is: a shortest walk on foot from the ground under the first voxel to the ground under the
// second, for an agent two voxels tall that climbs one voxel and drops three per move, by the exact walk field of their surroundings on
// the GPU (Scene::find_walk); prints "walk of N voxels:" and the voxels, or "no way on foot".
// --pools x0,y0,z0:x1,y1,z1, applied where --path is: where water stands in that box with its four sides open, by the exact spill levels of
// the box on the GPU (Scene::pools); prints "pools: W wet, C closed" and the deepest point with its depth, or "nothing is wet".
// --drop-floating x0,y0,z0:x1,y1,z1, applied after --dig and --shrink: the pieces of that box that hang on nothing -- connected components by faces,
// inside the box, without a voxel on the box's four sides or its bottom -- are removed (Scene::remove_floating); prints how many pieces
// and voxels went.
// --settle x0,y0,z0:x1,y1,z1, applied where --drop-floating is (after it, if both are given): the same pieces fall instead -- straight down, each as
// one rigid body, until they rest on the box's bottom, on something that did not move or on each other (Scene::settle_floating); prints
// how many pieces and voxels moved and the largest drop.  The floor is the bottom of the box: take z0 down to the ground.
// --dig-at picks the voxel under pixel (px, py) of the first frame's camera (Scene::pick) and carves a sphere of radius r there; the
// world streams, so while the pick lands on a brick that is not resident yet (level 3) the load queue is serviced and the pick repeated
// (at most 8 times).  Prints `picked voxel x,y,z level L`; after the carve, what the same pixel sees now.  A pick that stays
// unresolved (level 3) digs nothing.
// --ground x,y prints the height of the highest solid voxel of that column after the digging (one box query, Scene::query_volume): the
// world streams, so bricks that are not resident yet are reported as unresolved cells, not counted.
// --denoise filters the accumulated frame before the resolve (Scene::denoise: the a-trous filter guided by the first hits of the
// pixel-centre rays, Scene::pixel_rays + Scene::cast_rays with the frames' LoD rule around the camera) -- for runs of a few frames.
// --temporal moves the camera: it advances by a fixed small step (half a voxel sideways) per frame, every frame is 1 spp with samples of
// its own into a zeroed buffer and is reprojected into the history of the frames before (Scene::reproject: the samples of earlier
// frames carried to where the same surface point is now, tested by exact surface keys); the last history is what --denoise and the
// resolve get.  Not with `wavefront` or `ring`.
// With `wavefront` the frames are rendered with the reference's own queue schedule (one segment per call); with `ring` the
// world is made resident first and all frames are ONE launch of the persistent kernel (launch_frames, the frame ring).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../include/brickmap.hpp"

using namespace brickmap;

int main(int argc_in, char** argv_in) {
	std::vector<char*> args;
	int dig[4] = {0, 0, 0, -1};
	int dig_at[3] = {0, 0, -1};
	int drop_lo[3] = {0, 0, 0}, drop_hi[3] = {0, 0, 0};
	bool drop = false;
	int settle_lo[3] = {0, 0, 0}, settle_hi[3] = {0, 0, 0};
	bool settle = false;
	int ground[2] = {-1, -1};
	int morph_lo[2][3] = {{0, 0, 0}, {0, 0, 0}}, morph_hi[2][3] = {{0, 0, 0}, {0, 0, 0}}; // [0]: --grow, [1]: --shrink
	int morph_r2[2] = {0, 0};
	int path_ends[2][3] = {{0, 0, 0}, {0, 0, 0}};
	bool path = false;
	int walk_ends[2][3] = {{0, 0, 0}, {0, 0, 0}};
	bool walk = false;
	int pools_box[2][3] = {{0, 0, 0}, {0, 0, 0}};
	bool pools = false;
	const char* voxels_path = nullptr;
	bool denoise = false, temporal = false;
	std::string paste_path;
	int paste_size[3] = {0, 0, 0}, paste_at[3] = {0, 0, 0};
	std::string mesh_path;
	float mesh_at[3] = {0.f, 0.f, 0.f};
	std::string mesh_out_path;
	int mesh_out_lo[3] = {0, 0, 0}, mesh_out_hi[3] = {0, 0, 0};
	for (int i = 0; i < argc_in; ++i) {
		if (std::string(argv_in[i]) == "--denoise") {
			denoise = true;
			continue;
		}
		if (std::string(argv_in[i]) == "--temporal") {
			temporal = true;
			continue;
		}
		if (std::string(argv_in[i]) == "--voxels" && i + 1 < argc_in) {
			voxels_path = argv_in[++i];
			continue;
		}
		if (std::string(argv_in[i]) == "--paste" && i + 1 < argc_in) {
			const std::string spec = argv_in[++i];
			const size_t colon = spec.rfind(':');
			if (colon == std::string::npos || std::sscanf(spec.c_str() + colon + 1, "%d,%d,%d@%d,%d,%d", &paste_size[0], &paste_size[1], &paste_size[2], &paste_at[0],
														  &paste_at[1], &paste_at[2]) != 6 || paste_size[0] <= 0 || paste_size[1] <= 0 || paste_size[2] <= 0) {
				std::cerr << "--paste wants FILE:nx,ny,nz@x,y,z (sizes > 0)\n";
				return 2;
			}
			paste_path = spec.substr(0, colon);
			continue;
		}
		if (std::string(argv_in[i]) == "--mesh" && i + 1 < argc_in) {
			const std::string spec = argv_in[++i];
			const size_t at = spec.rfind('@');
			if (at == std::string::npos || at == 0 || std::sscanf(spec.c_str() + at + 1, "%f,%f,%f", &mesh_at[0], &mesh_at[1], &mesh_at[2]) != 3) {
				std::cerr << "--mesh wants FILE@x,y,z\n";
				return 2;
			}
			mesh_path = spec.substr(0, at);
			continue;
		}
		if (std::string(argv_in[i]) == "--mesh-out" && i + 1 < argc_in) {
			const std::string spec = argv_in[++i];
			const size_t eq = spec.find('=');
			int* lo = mesh_out_lo;
			int* hi = mesh_out_hi;
			if (eq == std::string::npos || eq + 1 == spec.size() ||
				std::sscanf(spec.substr(0, eq).c_str(), "%d,%d,%d:%d,%d,%d", &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2]) != 6 || hi[0] <= lo[0] || hi[1] <= lo[1] ||
				hi[2] <= lo[2]) {
				std::cerr << "--mesh-out wants x0,y0,z0:x1,y1,z1=FILE (a box that is not empty)\n";
				return 2;
			}
			mesh_out_path = spec.substr(eq + 1);
			continue;
		}
		if (std::string(argv_in[i]) == "--dig-at" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d,%d", &dig_at[0], &dig_at[1], &dig_at[2]) != 3 || dig_at[2] < 0) {
				std::cerr << "--dig-at wants px,py,r (r >= 0)\n";
				return 2;
			}
			continue;
		}
		if (std::string(argv_in[i]) == "--ground" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d", &ground[0], &ground[1]) != 2 || ground[0] < 0 || ground[1] < 0) {
				std::cerr << "--ground wants x,y (>= 0)\n";
				return 2;
			}
			continue;
		}
		if (std::string(argv_in[i]) == "--drop-floating" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d,%d:%d,%d,%d", &drop_lo[0], &drop_lo[1], &drop_lo[2], &drop_hi[0], &drop_hi[1], &drop_hi[2]) != 6) {
				std::cerr << "--drop-floating wants x0,y0,z0:x1,y1,z1\n";
				return 2;
			}
			drop = true;
			continue;
		}
		if (std::string(argv_in[i]) == "--settle" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d,%d:%d,%d,%d", &settle_lo[0], &settle_lo[1], &settle_lo[2], &settle_hi[0], &settle_hi[1], &settle_hi[2]) != 6) {
				std::cerr << "--settle wants x0,y0,z0:x1,y1,z1\n";
				return 2;
			}
			settle = true;
			continue;
		}
		if (std::string(argv_in[i]) == "--pools" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d,%d:%d,%d,%d", &pools_box[0][0], &pools_box[0][1], &pools_box[0][2], &pools_box[1][0], &pools_box[1][1], &pools_box[1][2]) != 6 ||
				pools_box[1][0] <= pools_box[0][0] || pools_box[1][1] <= pools_box[0][1] || pools_box[1][2] <= pools_box[0][2]) {
				std::cerr << "--pools wants x0,y0,z0:x1,y1,z1, a box that is not empty\n";
				return 2;
			}
			pools = true;
			continue;
		}
		if (std::string(argv_in[i]) == "--walk" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d,%d:%d,%d,%d", &walk_ends[0][0], &walk_ends[0][1], &walk_ends[0][2], &walk_ends[1][0], &walk_ends[1][1], &walk_ends[1][2]) != 6) {
				std::cerr << "--walk wants x0,y0,z0:x1,y1,z1\n";
				return 2;
			}
			walk = true;
			continue;
		}
		if (std::string(argv_in[i]) == "--path" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d,%d:%d,%d,%d", &path_ends[0][0], &path_ends[0][1], &path_ends[0][2], &path_ends[1][0], &path_ends[1][1], &path_ends[1][2]) != 6) {
				std::cerr << "--path wants x0,y0,z0:x1,y1,z1\n";
				return 2;
			}
			path = true;
			continue;
		}
		if ((std::string(argv_in[i]) == "--grow" || std::string(argv_in[i]) == "--shrink") && i + 1 < argc_in) {
			const int k = std::string(argv_in[i]) == "--shrink" ? 1 : 0;
			int* lo = morph_lo[k];
			int* hi = morph_hi[k];
			if (std::sscanf(argv_in[++i], "%d,%d,%d:%d,%d,%d=%d", &lo[0], &lo[1], &lo[2], &hi[0], &hi[1], &hi[2], &morph_r2[k]) != 7 || hi[0] <= lo[0] || hi[1] <= lo[1] ||
				hi[2] <= lo[2] || morph_r2[k] < 1) {
				std::cerr << (k ? "--shrink" : "--grow") << " wants x0,y0,z0:x1,y1,z1=r2 (a box that is not empty, r2 >= 1)\n";
				return 2;
			}
			continue;
		}
		if (std::string(argv_in[i]) == "--dig" && i + 1 < argc_in) {
			if (std::sscanf(argv_in[++i], "%d,%d,%d,%d", &dig[0], &dig[1], &dig[2], &dig[3]) != 4 || dig[3] < 0) {
				std::cerr << "--dig wants x,y,z,r (r >= 0)\n";
				return 2;
			}
			continue;
		}
		args.push_back(argv_in[i]);
	}
	const int argc = static_cast<int>(args.size());
	char** argv = args.data();
	const int grid_size = argc > 1 ? std::atoi(argv[1]) : 1024, grid_height = argc > 2 ? std::atoi(argv[2]) : 1024;
	const size_t width = argc > 3 ? std::atoi(argv[3]) : 1920, height = argc > 4 ? std::atoi(argv[4]) : 1080;
	const int frames = argc > 5 ? std::atoi(argv[5]) : 64;
	const char* out = argc > 6 ? argv[6] : "frame.ppm";
	const bool wavefront = argc > 7 && std::string(argv[7]) == "wavefront", ring = argc > 7 && std::string(argv[7]) == "ring";

	State state(width, height);                 // main.cpp:102
	Scene scene(grid_size, grid_height);        // main.cpp:104
	if (voxels_path) {
		std::ifstream in(voxels_path, std::ios::binary);
		std::vector<uint8_t> volume(static_cast<size_t>(grid_size) * grid_size * grid_height);
		if (!in || !in.read(reinterpret_cast<char*>(volume.data()), static_cast<std::streamsize>(volume.size())) || in.peek() != EOF) {
			std::cerr << "--voxels: " << voxels_path << " does not hold " << volume.size() << " bytes\n";
			return 2;
		}
		scene.load_voxels(volume.data(), volume.size());
	} else {
		scene.generate();                       // main.cpp:105 -- nothing resident yet: bricks stream in on demand
	}
	if (!paste_path.empty()) {
		std::ifstream in(paste_path, std::ios::binary);
		std::vector<uint8_t> volume(static_cast<size_t>(paste_size[0]) * paste_size[1] * paste_size[2]);
		if (!in || !in.read(reinterpret_cast<char*>(volume.data()), static_cast<std::streamsize>(volume.size())) || in.peek() != EOF) {
			std::cerr << "--paste: " << paste_path << " does not hold " << volume.size() << " bytes\n";
			return 2;
		}
		const int hi[3] = {paste_at[0] + paste_size[0], paste_at[1] + paste_size[1], paste_at[2] + paste_size[2]};
		scene.write_region(Scene::Region(paste_at, hi), volume.data());
	}
	if (!mesh_path.empty()) {
		std::ifstream in(mesh_path, std::ios::binary | std::ios::ate);
		const std::streamoff bytes = in ? static_cast<std::streamoff>(in.tellg()) : -1;
		if (bytes <= 0 || bytes % 36 != 0) {
			std::cerr << "--mesh: " << mesh_path << " does not hold triangles of 9 floats\n";
			return 2;
		}
		std::vector<float> triangles(static_cast<size_t>(bytes) / sizeof(float));
		in.seekg(0);
		if (!in.read(reinterpret_cast<char*>(triangles.data()), bytes)) {
			std::cerr << "--mesh: cannot read " << mesh_path << "\n";
			return 2;
		}
		for (size_t i = 0; i < triangles.size(); ++i) triangles[i] += mesh_at[i % 3];
		size_t box = 0;
		const bm_voxelize_result r = scene.write_mesh(triangles.data(), static_cast<int64_t>(triangles.size() / 9), BM_EDIT_SET, BM_VOXELIZE_SURFACE | BM_VOXELIZE_SOLID, &box);
		std::printf("mesh: %zu triangles (%u rejected, %u degenerate) into a box of %zu voxels, open columns %llu\n", triangles.size() / 9, r.rejected, r.degenerate, box,
					static_cast<unsigned long long>(r.open_columns));
	}
	if (dig[3] >= 0) scene.carve_sphere(dig, dig[3]);
	if (morph_r2[0] > 0) std::printf("grew %llu voxels\n", static_cast<unsigned long long>(scene.grow(morph_lo[0], morph_hi[0], static_cast<uint32_t>(morph_r2[0]))));
	if (morph_r2[1] > 0) std::printf("shrank %llu voxels\n", static_cast<unsigned long long>(scene.shrink(morph_lo[1], morph_hi[1], static_cast<uint32_t>(morph_r2[1]))));
	if (path) {
		const auto voxels = scene.find_path(path_ends[0], path_ends[1]);
		if (voxels.empty()) std::printf("no path\n");
		else {
			std::printf("path of %zu voxels:", voxels.size());
			for (const auto& v : voxels) std::printf(" %d,%d,%d", v[0], v[1], v[2]);
			std::printf("\n");
		}
	}
	if (pools) {
		const bm_water_result rec = scene.pools(pools_box[0], pools_box[1]);
		std::printf("pools: %llu wet, %llu closed\n", static_cast<unsigned long long>(rec.wet), static_cast<unsigned long long>(rec.closed));
		if (rec.deepest == 0) std::printf("nothing is wet\n");
		else {
			const unsigned long long nx = pools_box[1][0] - pools_box[0][0], ny = pools_box[1][1] - pools_box[0][1], at = rec.deepest_at;
			std::printf("deepest: %u at %d,%d,%d\n", rec.deepest, pools_box[0][0] + static_cast<int>(at % nx), pools_box[0][1] + static_cast<int>(at / nx % ny),
						pools_box[0][2] + static_cast<int>(at / (nx * ny)));
		}
	}
	if (walk) {
		const auto voxels = scene.find_walk(walk_ends[0], walk_ends[1]);
		if (voxels.empty()) std::printf("no way on foot\n");
		else {
			std::printf("walk of %zu voxels:", voxels.size());
			for (const auto& v : voxels) std::printf(" %d,%d,%d", v[0], v[1], v[2]);
			std::printf("\n");
		}
	}
	if (drop) {
		const Scene::Removed gone = scene.remove_floating(drop_lo, drop_hi);
		std::printf("dropped %llu floating pieces, %llu voxels\n", static_cast<unsigned long long>(gone.pieces), static_cast<unsigned long long>(gone.voxels));
	}
	if (settle) {
		const Scene::Settled fell = scene.settle_floating(settle_lo, settle_hi);
		std::printf("settled %llu floating pieces, %llu voxels, largest drop %u\n", static_cast<unsigned long long>(fell.pieces), static_cast<unsigned long long>(fell.voxels),
					fell.largest_drop);
	}
	camera.position = {grid_size / 2.f, grid_size / 8.f, 0.8f * grid_height};
	camera.horizontal_angle = 0.8;
	camera.vertical_angle = -0.5;
	camera.update();                            // main.cpp:140
	if (dig_at[2] >= 0) {
		if (dig_at[0] < 0 || dig_at[1] < 0 || dig_at[0] >= static_cast<int>(width) || dig_at[1] >= static_cast<int>(height)) {
			std::cerr << "--dig-at: pixel outside the frame\n";
			return 2;
		}
		auto pick = [&]() {
			bm_ray_hit hit = scene.pick(camera, static_cast<int>(width), static_cast<int>(height), dig_at[0], dig_at[1]);
			for (int k = 0; k < 8 && hit.level == 3; ++k) { // the brick was requested by the pick: make it resident, ask again
				scene.process_load_queue();
				hit = scene.pick(camera, static_cast<int>(width), static_cast<int>(height), dig_at[0], dig_at[1]);
			}
			return hit;
		};
		const bm_ray_hit hit = pick();
		std::printf("picked voxel %d,%d,%d level %d\n", hit.voxel[0], hit.voxel[1], hit.voxel[2], hit.level);
		if (hit.level >= 0 && hit.level <= 2) { // a resolved hit (level 3 after 8 rounds: the brick never arrived, nothing to dig at)
			scene.carve_sphere(hit.voxel, dig_at[2]);
			const bm_ray_hit now = pick();
			std::printf("carved radius %d at %d,%d,%d; the pixel now sees voxel %d,%d,%d level %d\n", dig_at[2], hit.voxel[0], hit.voxel[1],
						hit.voxel[2], now.voxel[0], now.voxel[1], now.voxel[2], now.level);
		}
	}
	if (!mesh_out_path.empty()) {
		std::vector<float> triangles;
		const Scene::Mesh mesh = scene.extract_mesh(Scene::Region(mesh_out_lo, mesh_out_hi), &triangles);
		std::ofstream file(mesh_out_path, std::ios::binary);
		file.write(reinterpret_cast<const char*>(triangles.data()), static_cast<std::streamsize>(triangles.size() * sizeof(float)));
		if (!file) {
			std::cerr << "--mesh-out: cannot write " << mesh_out_path << "\n";
			return 2;
		}
		std::printf("mesh-out: %llu quads, %llu faces, %zu triangles\n", static_cast<unsigned long long>(mesh.result.quads),
					static_cast<unsigned long long>(mesh.result.faces), triangles.size() / 9);
	}
	if (ground[0] >= 0) {
		const int lo[3] = {ground[0], ground[1], 0}, hi[3] = {ground[0] + 1, ground[1] + 1, grid_height};
		const bm_volume_result column = scene.query_volume(Scene::Volume::box(lo, hi));
		std::printf("ground at %d,%d: height %d (%llu solid voxels in the column, %u brick cells not resident)\n", ground[0], ground[1], column.hi[2],
					static_cast<unsigned long long>(column.solid), column.unresolved);
	}

	if (temporal && (wavefront || ring)) {
		std::cerr << "--temporal renders its frames one by one: not with wavefront or ring\n";
		return 2;
	}
	const int w = static_cast<int>(width), h = static_cast<int>(height);
	const size_t n_pixels = width * height;
	const float* to_resolve = reinterpret_cast<const float*>(state.blit_buffer);
	void* temporal_buffers = nullptr; // rays, then hits, then the two histories that take turns
	if (temporal) {
		const size_t hist_bytes = (Scene::history_bytes(w, h) + 15) / 16 * 16;
		BM_CHECKED(bm_buffer_alloc(0, n_pixels * (sizeof(bm_ray) + sizeof(bm_ray_hit)) + 2 * hist_bytes, &temporal_buffers));
		bm_ray* rays = static_cast<bm_ray*>(temporal_buffers);
		bm_ray_hit* hits = reinterpret_cast<bm_ray_hit*>(rays + n_pixels);
		char* histories[2] = {reinterpret_cast<char*>(hits + n_pixels), reinterpret_cast<char*>(hits + n_pixels) + hist_bytes};
		float* frame = reinterpret_cast<float*>(state.blit_buffer);
		// the step: half a voxel along cross(direction, up), the view's right axis
		const vec3 d = camera.direction;
		const float len = std::sqrt(d.x * d.x + d.y * d.y);
		const vec3 step = {0.5f * d.y / len, -0.5f * d.x / len, 0.f};
		Camera before;
		for (int f = 0; f < frames; ++f) {
			bm_frame_params fp = detail::frame_params(state, 3);
			fp.sample_base = f; // samples of its own: the noise of consecutive frames must not be the same
			const bm_camera cam = camera.to_c();
			const float lod_origin[3] = {camera.position.x, camera.position.y, camera.position.z};
			BM_CHECKED(bm_buffer_zero(0, frame, n_pixels * sizeof(vec4), nullptr));
			BM_CHECKED(bm_render_frame(scene.gpuScene.handle, &cam, &fp, frame, nullptr, nullptr));
			scene.pixel_rays(camera, w, h, rays);
			scene.cast_rays(static_cast<int64_t>(n_pixels), rays, hits, BM_QUERY_LOD | BM_QUERY_NO_REQUESTS, lod_origin);
			scene.reproject(w, h, camera, f ? &before : nullptr, frame, hits, f ? histories[(f + 1) & 1] : nullptr, histories[f & 1]);
			BM_CHECKED(bm_synchronize(scene.gpuScene.handle));
			scene.process_load_queue();
			to_resolve = reinterpret_cast<const float*>(histories[f & 1]);
			before = camera;
			if (f + 1 < frames) camera.position = {camera.position.x + step.x, camera.position.y + step.y, camera.position.z + step.z};
		}
		std::cout << "temporal: " << frames << " frames of 1 spp, the camera half a voxel sideways per frame, max_history 32\n";
	} else if (wavefront) {
		Wavefront queues(scene.gpuScene); // state.h:19-21: ray_buffer_work / ray_buffer_next / shadow_queue_buffer
		for (int frame = 0; frame < frames; ++frame) {
			launch_kernels(state, state.blit_buffer, scene.gpuScene, queues); // main.cpp:142
			scene.process_load_queue();                                         // main.cpp:144 (the swap of :146 is inside)
		}
	} else if (ring) {
		scene.preload_all();                                                // (bricks are serviced between launches: a ring wants them resident)
		launch_frames(state, state.blit_buffer, scene.gpuScene, frames);   // main.cpp:117-147, `frames` iterations in one launch
	} else {
		for (int frame = 0; frame < frames; ++frame) {
			launch_kernels(state, state.blit_buffer, scene.gpuScene); // main.cpp:142
			scene.process_load_queue();                                 // main.cpp:144
		}
	}

	// blit_onto_framebuffer (kernel.cu:348-364) into an offscreen buffer instead of the GL surface
	void* resolved = nullptr;
	BM_CHECKED(bm_buffer_alloc(0, width * height * sizeof(vec4), &resolved));
	void* guides = nullptr; // rays, then hits, then the filter's workspace; the filtered frame goes to `resolved`, which is then resolved in place
	if (denoise) {
		const size_t n = n_pixels, ws_bytes = Scene::denoise_workspace_bytes(w, h);
		BM_CHECKED(bm_buffer_alloc(0, n * (sizeof(bm_ray) + sizeof(bm_ray_hit)) + ws_bytes, &guides));
		bm_ray* rays = static_cast<bm_ray*>(guides);
		bm_ray_hit* hits = reinterpret_cast<bm_ray_hit*>(rays + n);
		const float lod_origin[3] = {camera.position.x, camera.position.y, camera.position.z};
		scene.pixel_rays(camera, w, h, rays);
		scene.cast_rays(static_cast<int64_t>(n), rays, hits, BM_QUERY_LOD | BM_QUERY_NO_REQUESTS, lod_origin);
		scene.denoise(w, h, to_resolve, hits, static_cast<float*>(resolved), hits + n, ws_bytes);
		to_resolve = static_cast<const float*>(resolved);
		std::cout << "denoised: 5 a-trous iterations, sigma_l 4\n";
	}
	BM_CHECKED(bm_resolve(scene.gpuScene.handle, to_resolve, static_cast<float*>(resolved), static_cast<int64_t>(width * height), nullptr));
	std::vector<vec4> host(width * height);
	BM_CHECKED(bm_buffer_read(0, host.data(), resolved, host.size() * sizeof(vec4)));
	std::ofstream f(out, std::ios::binary);
	f << "P6\n" << width << " " << height << "\n255\n";
	for (const vec4& c : host) {
		const unsigned char rgb[3] = {static_cast<unsigned char>(std::min(1.f, std::max(0.f, c.x)) * 255.f),
									  static_cast<unsigned char>(std::min(1.f, std::max(0.f, c.y)) * 255.f),
									  static_cast<unsigned char>(std::min(1.f, std::max(0.f, c.z)) * 255.f)};
		f.write(reinterpret_cast<const char*>(rgb), 3);
	}
	bm_scene_info info;
	BM_CHECKED(bm_scene_get_info(scene.gpuScene.handle, &info));
	std::cout << "wrote " << out << ": " << frames << " frames, " << info.resident_bricks << " of " << info.total_bricks << " bricks resident\n";
	bm_buffer_free(0, resolved);
	if (guides) bm_buffer_free(0, guides);
	if (temporal_buffers) bm_buffer_free(0, temporal_buffers);
	return 0;
}
