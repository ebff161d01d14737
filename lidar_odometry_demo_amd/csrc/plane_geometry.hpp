// The geometry rule of the four planning grids (clearance, navigation field, region grid, visibility grid), written once,
// and the rule by which any grid shifts by whole cells and follows a robot.  Plain C++: nothing here needs a device or a
// HIP header.  The occupancy and the elevation grid have geometry rules of their own (occupancy_host.hpp,
// elevation_host.hpp).
#pragma once
#include <cfloat>
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

// ---- the shift of a grid by whole cells (include/lidar_odometry_amd.h, "grid shift") ---------------------
// Written once for all seven grid families.  The side limit is the occupancy grid's, the widest of them.
constexpr uint32_t kShiftMaxSide = 16384;

inline bool shift_geometry_ok(const lom_occupancy_geometry *g)
{
    return g && std::isfinite(g->resolution) && g->resolution > 0.f && std::isfinite(g->origin_x) && std::isfinite(g->origin_y) &&
           g->width >= 1u && g->width <= kShiftMaxSide && g->height >= 1u && g->height <= kShiftMaxSide;
}

// origin' = (float)((double)origin + (double)d * (double)resolution), from the CURRENT f32 origin alone: two handles of
// equal geometry shifted by the same d stay bit-equal.  The rounding to f32 is part of the definition: the result is exact
// for a dyadic resolution and a modest origin (no bit is lost); with r = 0.1f the origin moves by under one ulp of itself
// per shift, so a long sequence of shifts drifts against origin0 + sum(d) * r by at most that per call.
// The conversion is only made where C++ defines it.  Round-to-nearest-even takes a double to a finite float exactly when
// its magnitude lies below FLT_MAX plus half an ulp, (2 - 2^-24) 2^127: up to FLT_MAX the cast does it, between FLT_MAX
// and that bound the result is FLT_MAX, and from the bound on (the tie goes to the even neighbour, 2^128) it is not finite.
// false: origin' is not finite, *out untouched.
inline bool shifted_origin(float origin, float resolution, int32_t d, float *out)
{
    constexpr double kRoundsToInf = 0x1.ffffffp127;
    const double v = (double)origin + (double)d * (double)resolution;
    if (!(std::fabs(v) < kRoundsToInf)) return false;
    *out = std::fabs(v) <= (double)FLT_MAX ? (float)v : (v < 0.0 ? -FLT_MAX : FLT_MAX);
    return true;
}

// out = in moved by (dx, dy) cells.  LOM_ERR_ARG: a NULL or a geometry that fails the rule; LOM_ERR_RANGE: an origin' that
// is not finite (out untouched).  in and out may be the same object.
inline int shift_geometry(const lom_occupancy_geometry *in, int32_t dx, int32_t dy, lom_occupancy_geometry *out)
{
    if (!out || !shift_geometry_ok(in)) return LOM_ERR_ARG;
    float ox, oy;
    if (!shifted_origin(in->origin_x, in->resolution, dx, &ox) || !shifted_origin(in->origin_y, in->resolution, dy, &oy)) return LOM_ERR_RANGE;
    lom_occupancy_geometry g = *in;
    g.origin_x = ox, g.origin_y = oy;
    *out = g;
    return LOM_OK;
}

// One axis of follow: the cell q of the point by the grids' own index rule, and the shift d that brings it back towards
// the middle of a side of n cells.  LOM_ERR_RANGE: |q| > 2^40 (also a quotient that is no number) or |d| > INT32_MAX.
inline int follow_axis(double x, float origin, float resolution, uint32_t n, uint32_t margin, uint32_t quantum, int32_t *d)
{
    const double qf = std::floor((x - (double)origin) / (double)resolution);
    if (!(std::fabs(qf) <= 1099511627776.0)) return LOM_ERR_RANGE;
    const int64_t q = (int64_t)qf;
    if (q >= (int64_t)margin && q < (int64_t)n - (int64_t)margin) {
        *d = 0;
        return LOM_OK;
    }
    const int64_t v = (q - (int64_t)(n / 2u)) / (int64_t)quantum * (int64_t)quantum;  // C++ division truncates towards zero
    if (v > INT32_MAX || v < -(int64_t)INT32_MAX) return LOM_ERR_RANGE;
    *d = (int32_t)v;
    return LOM_OK;
}

// The shift that brings a robot at (x, y) metres back towards the middle.  margin + quantum <= n / 2 on both axes is what
// guarantees that after the shift the robot's cell lies in [margin, n - margin).  On an error *dx = *dy = 0.
inline int follow(const lom_occupancy_geometry *g, double x, double y, uint32_t margin, uint32_t quantum, int32_t *dx, int32_t *dy)
{
    if (dx) *dx = 0;
    if (dy) *dy = 0;
    if (!dx || !dy || !shift_geometry_ok(g) || !std::isfinite(x) || !std::isfinite(y) || quantum == 0u) return LOM_ERR_ARG;
    if ((uint64_t)margin + quantum > g->width / 2u || (uint64_t)margin + quantum > g->height / 2u) return LOM_ERR_ARG;
    int32_t sx = 0, sy = 0;
    if (const int rc = follow_axis(x, g->origin_x, g->resolution, g->width, margin, quantum, &sx); rc != LOM_OK) return rc;
    if (const int rc = follow_axis(y, g->origin_y, g->resolution, g->height, margin, quantum, &sy); rc != LOM_OK) return rc;
    *dx = sx, *dy = sy;
    return LOM_OK;
}

}  // namespace plane
}  // namespace lom
