// Host planning of lom_elevation_*: the value ranges, the origins' start cells and range verdict, the launches of a
// call.  Plain C++, no HIP: elevation.hip calls these, and tests/cpp/test_elevation.cpp compiles this file and
// assemble_host.cpp alone.
#include "elevation_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace elevation {

namespace {
const float kBig = 3.402823466e+38f;  // (a NaN fails every comparison below)
bool finite_f(float v) { return v >= -kBig && v <= kBig; }
bool positive_f(float v) { return v > 0.f && v <= kBig; }
}  // namespace

bool geometry_ok(const lom_elevation_geometry *g)
{
    return g && positive_f(g->resolution) && finite_f(g->origin_x) && finite_f(g->origin_y) && finite_f(g->z_ref) &&
           g->width >= 1u && g->width <= kMaxSide && g->height >= 1u && g->height <= kMaxSide;
}

bool point_params_ok(const lom_elevation_point_params *p, float resolution)
{
    return p && p->z_lo < 0.f && p->z_lo >= -kBig && positive_f(p->z_hi) && p->min_range > 0.f &&
           p->max_range > p->min_range && p->max_range <= kBig && (double)p->max_range / (double)resolution <= 1048576.0;
}

bool layer_params_ok(const lom_elevation_layer_params *p)
{
    return p && p->min_points >= 1u && p->window >= 1u && p->window <= kMaxWindow;
}

bool cost_params_ok(const lom_elevation_cost_params *p)
{
    return p && positive_f(p->max_slope) && positive_f(p->max_step) && positive_f(p->max_rough) && positive_f(p->max_span);
}

bool origin_cell(const assemble::AsmScan &d, const lom_elevation_geometry &g, int32_t c[2])
{
    const double G[2] = {(double)g.origin_x, (double)g.origin_y};
    const double r = (double)g.resolution;
    for (int a = 0; a < 2; a++) {
        const double O = (double)(float)d.t[a];
        const double q = std::floor((O - G[a]) / r);
        if (!(q > -(double)kCellLimit && q < (double)kCellLimit)) return false;  // also NaN and the infinities
        c[a] = (int32_t)q;
    }
    return true;
}

int plan(const assemble::ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
         const lom_elevation_geometry &g, const lom_elevation_point_params *p, uint32_t scans_per_launch, Plan &out,
         std::string &why)
{
    out.launches.clear();
    int rc = assemble::plan(table, n_scans, ids, poses, count, out.scans, why);
    if (rc == LOM_OK && !point_params_ok(p, g.resolution)) {
        why = "point parameters: z_lo < 0 < z_hi, 0 < min_range < max_range, all finite, max_range / resolution <= 2^20";
        rc = LOM_ERR_ARG;
    }
    for (size_t k = 0; k < count && rc == LOM_OK; k++) {
        int32_t c[2];
        if (!origin_cell(out.scans.scans[k], g, c)) {
            why = "origin of scan " + std::to_string(k) + " of the call: its cell is beyond 2^30 or not finite";
            rc = LOM_ERR_RANGE;
        }
    }
    if (rc != LOM_OK) {
        out.scans = assemble::Plan();
        return rc;
    }
    const size_t per = scans_per_launch ? std::min(scans_per_launch, kScansPerLaunch) : kScansPerLaunch;
    for (size_t first = 0; first < count; first += per) {
        Launch l;
        l.first = (uint32_t)first;
        l.count = (uint32_t)std::min<size_t>(per, count - first);
        l.max_n = 0;
        for (uint32_t k = 0; k < l.count; k++) l.max_n = std::max(l.max_n, out.scans.scans[first + k].n);
        l.grid_x = (l.max_n + assemble::kAsmThreads - 1) / assemble::kAsmThreads;
        if (l.max_n) out.launches.push_back(l);
    }
    return LOM_OK;
}

}  // namespace elevation
}  // namespace lom
