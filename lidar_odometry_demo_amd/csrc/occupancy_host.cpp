// Host planning of lom_occupancy_*: parameter ranges, the origins' start cells and range verdict, the step bound, the
// slice size under the scratch budget, the slices of a call and their bounding boxes.  Plain C++, no HIP: occupancy.hip
// calls these, and tests/cpp/test_occupancy.cpp compiles this file and assemble_host.cpp alone.
#include "occupancy_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace occupancy {

namespace {
const float kBig = 3.402823466e+38f;  // (a NaN fails every comparison below)
bool finite_f(float v) { return v >= -kBig && v <= kBig; }
}  // namespace

bool geometry_ok(const lom_occupancy_geometry *g)
{
    return g && g->resolution > 0.f && g->resolution <= kBig && finite_f(g->origin_x) && finite_f(g->origin_y) &&
           g->width >= 1u && g->width <= kMaxSide && g->height >= 1u && g->height <= kMaxSide;
}

bool params_ok(const lom_occupancy_ray_params *p, float resolution)
{
    return p && p->z_lo < 0.f && p->z_lo >= -kBig && p->z_hi > 0.f && p->z_hi <= kBig && p->margin >= 0.f &&
           p->margin <= kBig && p->min_range > 0.f && p->max_range > p->min_range && p->max_range <= kBig &&
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

bool origin_cell(const assemble::AsmScan &d, const lom_occupancy_geometry &g, int32_t c[2])
{
    const double G[2] = {(double)g.origin_x, (double)g.origin_y};
    const double r = (double)g.resolution;
    for (int a = 0; a < 2; a++) {
        const double O = (double)(float)d.t[a];
        const double O2 = O - G[a];
        const double q = std::floor(O2 / r);
        if (!(q > -(double)kCellLimit && q < (double)kCellLimit)) return false;  // also NaN and the infinities
        c[a] = (int32_t)q;
    }
    return true;
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
    out.cells.clear();
    int rc = assemble::plan(table, n_scans, ids, poses, count, out.scans, why);
    if (rc == LOM_OK && !params_ok(p, g.resolution)) {
        why = "ray parameters: z_lo < 0 < z_hi, margin >= 0, 0 < min_range < max_range, all finite, max_range / resolution <= 2^20";
        rc = LOM_ERR_ARG;
    }
    if (rc == LOM_OK) {
        out.cells.resize(count * 2);
        for (size_t k = 0; k < count && rc == LOM_OK; k++)
            if (!origin_cell(out.scans.scans[k], g, &out.cells[k * 2])) {
                why = "origin of scan " + std::to_string(k) + " of the call: its cell is beyond 2^30 or not finite";
                rc = LOM_ERR_RANGE;
            }
    }
    if (rc != LOM_OK) {
        out.scans = assemble::Plan();
        out.cells.clear();
        return rc;
    }
    const uint32_t per = slice_scans(g, test_slice_max);
    for (size_t first = 0; first < count; first += per) {
        Slice s;
        s.first = (uint32_t)first;
        s.count = (uint32_t)std::min<size_t>(per, count - first);
        s.max_n = 0;
        s.box = Box{0, 0, 0, 0};
        for (uint32_t k = 0; k < s.count; k++) {
            const uint32_t n = out.scans.scans[first + k].n;
            s.max_n = std::max(s.max_n, n);
            if (n) s.box = box_union(s.box, box_of(&out.cells[(first + k) * 2], p->max_range, g));
        }
        s.grid_x = (s.max_n + assemble::kAsmThreads - 1) / assemble::kAsmThreads;
        if (s.max_n) out.slices.push_back(s);
    }
    return LOM_OK;
}

}  // namespace occupancy
}  // namespace lom
