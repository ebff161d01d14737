// Host planning of lom_elevation_*: the value ranges and the launches of a call.  The value-range helpers, the origins'
// start cells and range verdict, the planner's first checks and the cut into launches are assemble_host.cpp's, shared
// with the occupancy grid.  Plain C++, no HIP: elevation.hip calls these, and tests/cpp/test_elevation.cpp compiles this
// file and assemble_host.cpp alone.
#include "elevation_host.hpp"

#include <algorithm>

namespace lom {
namespace elevation {

using assemble::finite_f;
using assemble::kBig;
using assemble::positive_f;

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

int plan(const assemble::ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
         const lom_elevation_geometry &g, const lom_elevation_point_params *p, uint32_t scans_per_launch, Plan &out,
         std::string &why)
{
    out.launches.clear();
    std::vector<int32_t> cells;  // (only their range verdict is used)
    const int rc = assemble::plan_on_grid(
        table, n_scans, ids, poses, count, {g.resolution, g.origin_x, g.origin_y}, point_params_ok(p, g.resolution),
        "point parameters: z_lo < 0 < z_hi, 0 < min_range < max_range, all finite, max_range / resolution <= 2^20", out.scans,
        cells, why);
    if (rc != LOM_OK) return rc;
    out.launches = assemble::cut_launches(out.scans, scans_per_launch ? std::min(scans_per_launch, kScansPerLaunch) : kScansPerLaunch);
    return LOM_OK;
}

}  // namespace elevation
}  // namespace lom
