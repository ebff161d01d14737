// The C ABI of the shift rule (include/lidar_odometry_amd.h, "grid shift"): the two functions that need no handle and no
// device.  The rule itself is plane_geometry.hpp's, where the handles' shifts take it from too.  Plain C++, no HIP.
#include "plane_geometry.hpp"

extern "C" {

int lom_grid_shift_geometry(const lom_occupancy_geometry *in, int32_t dx, int32_t dy, lom_occupancy_geometry *out)
{
    return lom::plane::shift_geometry(in, dx, dy, out);
}

int lom_grid_follow(const lom_occupancy_geometry *g, double x, double y, uint32_t margin_cells, uint32_t quantum_cells, int32_t *dx,
                    int32_t *dy)
{
    return lom::plane::follow(g, x, y, margin_cells, quantum_cells, dx, dy);
}

}  // extern "C"
