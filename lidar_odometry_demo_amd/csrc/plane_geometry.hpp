// The geometry rule of the four planning grids (clearance, navigation field, region grid, visibility grid), written once.
// Plain C++: nothing here needs a device or a HIP header.  The occupancy and the elevation grid have rules of their own
// (occupancy_host.hpp, elevation_host.hpp).
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/lidar_odometry_amd.h"

namespace lom {
namespace plane {

constexpr uint32_t kMaxSide = 8192;  // cells per axis: a linear index fits 26 bits
// what a create says behind "<family> geometry: " where the rule below does not hold
constexpr const char *kGeometryRule = "resolution > 0 and finite, a finite origin, 1 <= width, height <= 8192";

inline bool geometry_ok(const lom_occupancy_geometry *g)
{
    return g && std::isfinite(g->resolution) && g->resolution > 0.f && std::isfinite(g->origin_x) && std::isfinite(g->origin_y) &&
           g->width >= 1u && g->width <= kMaxSide && g->height >= 1u && g->height <= kMaxSide;
}

}  // namespace plane
}  // namespace lom
