// Host planning of lom_occupancy_*: parameter ranges, the step bound, the slice size under the scratch budget, the
// slices of a call and their bounding boxes.  The value-range helpers, the origins' start cells and range verdict, the
// planner's first checks and the cut into launches are assemble_host.cpp's, shared with the elevation grid.  Plain C++,
// no HIP: occupancy.hip calls these, and tests/cpp/test_occupancy.cpp compiles this file and assemble_host.cpp alone.
#include "occupancy_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace occupancy {

using assemble::finite_f;
using assemble::kBig;
using assemble::positive_f;

bool geometry_ok(const lom_occupancy_geometry *g)
{
    return g && positive_f(g->resolution) && finite_f(g->origin_x) && finite_f(g->origin_y) && g->width >= 1u &&
           g->width <= kMaxSide && g->height >= 1u && g->height <= kMaxSide;
}

bool params_ok(const lom_occupancy_ray_params *p, float resolution)
{
    return p && p->z_lo < 0.f && p->z_lo >= -kBig && positive_f(p->z_hi) && p->margin >= 0.f && p->margin <= kBig &&
           p->min_range > 0.f && p->max_range > p->min_range && p->max_range <= kBig &&
           (double)p->max_range / (double)resolution <= 1048576.0;
}

bool rule_ok(const lom_occupancy_rule *r) { return r && r->min_free_scans >= 1u && r->min_seen_scans >= 1u; }

uint32_t max_steps(float max_range, float resolution)
{
    const double cells = std::min(std::ceil((double)max_range / (double)resolution), 1048576.0);
    return 2u * ((uint32_t)cells + 2u);
}

uint32_t slice_scans(const lom_occupancy_geometry &g, uint32_t test_slice_max)
{
    const size_t per_scan = map_words(g) * 2 * sizeof(uint32_t);
    size_t s = std::min<size_t>(kSliceScans, kScratchBudget / per_scan);
    if (s < 1) s = 1;
    if (test_slice_max && test_slice_max < s) s = test_slice_max;
    return (uint32_t)s;
}

Box box_of(const int32_t c[2], float max_range, const lom_occupancy_geometry &g)
{
    const int64_t reach = (int64_t)std::min(std::ceil((double)max_range / (double)g.resolution), 1048576.0) + 2;
    const int64_t side[2] = {(int64_t)g.width, (int64_t)g.height};
    int64_t lo[2], hi[2];
    for (int a = 0; a < 2; a++) {
        lo[a] = std::min(std::max<int64_t>((int64_t)c[a] - reach, 0), side[a]);
        hi[a] = std::min(std::max<int64_t>((int64_t)c[a] + reach + 1, 0), side[a]);
    }
    return Box{(uint32_t)lo[0], (uint32_t)lo[1], (uint32_t)hi[0], (uint32_t)hi[1]};
}

Box box_union(const Box &a, const Box &b)
{
    if (a.empty()) return b;
    if (b.empty()) return a;
    return Box{std::min(a.x0, b.x0), std::min(a.y0, b.y0), std::max(a.x1, b.x1), std::max(a.y1, b.y1)};
}

int plan(const assemble::ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
         const lom_occupancy_geometry &g, const lom_occupancy_ray_params *p, uint32_t test_slice_max, Plan &out,
         std::string &why)
{
    out.slices.clear();
    const int rc = assemble::plan_on_grid(
        table, n_scans, ids, poses, count, {g.resolution, g.origin_x, g.origin_y}, params_ok(p, g.resolution),
        "ray parameters: z_lo < 0 < z_hi, margin >= 0, 0 < min_range < max_range, all finite, max_range / resolution <= 2^20",
        out.scans, out.cells, why);
    if (rc != LOM_OK) return rc;
    for (const assemble::Launch &l : assemble::cut_launches(out.scans, slice_scans(g, test_slice_max))) {
        Slice s{l, Box{0, 0, 0, 0}};
        for (uint32_t k = l.first; k < l.first + l.count; k++)
            if (out.scans.scans[k].n) s.box = box_union(s.box, box_of(&out.cells[(size_t)k * 2], p->max_range, g));
        out.slices.push_back(s);
    }
    return LOM_OK;
}

}  // namespace occupancy
}  // namespace lom
