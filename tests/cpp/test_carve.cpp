// VoxelGrid::carveRays of the C++ mirror: a 9 x 9 x 9 lattice map (voxel 0.5, one point per cell), twelve rays; prints the
// size the carve leaves and the number of voxels it erased (tests/test_carve_gpu.py builds the same map and rays).
#include <cstdio>

#include "check.hpp"
#include "lidar_odometry_amd.hpp"

int main()
{
    try {
        lom::VoxelGrid grid(0.5f, 4);
        lom::PointCloud<lom::PointXYZ> cloud;
        for (int x = -4; x <= 4; x++)
            for (int y = -4; y <= 4; y++)
                for (int z = -4; z <= 4; z++) {
                    auto at = [](int c) { return (float)c * 0.5f + 0.125f * (float)((c > 0) - (c < 0)); };
                    cloud.points.emplace_back(at(x), at(y), at(z));
                }
        grid.addCloudWithoutNormals(cloud);
        lom::PointCloud<lom::PointXYZ> rays;
        for (int k = 0; k < 12; k++) rays.points.emplace_back(2.1f, (float)(0.3 * k - 2.0), (float)(0.2 * k - 1.0));
        lom_carve_params p;
        p.margin = 0.25f;
        p.min_range = 0.5f;
        p.max_range = 6.0f;
        p.min_crossings = 1;
        const lom_carve_stats st = grid.carveRays(lom::Vector3f(0.1f, 0.1f, 0.1f), rays, p);
        CHECK(st.rays_walked + st.rays_skipped == 12);
        if (check_done()) return 1;
        std::printf("%zu %u\n", grid.size(), st.voxels_erased);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
