// Host planning of lom_navset_*: the offsets rule, the field index per goal, storage sizes, launch shapes, the refusals of
// gather and paths, a field's summary from its words.  Plain C++, no HIP: navset.hip calls these, and
// tests/cpp/test_navset.cpp compiles this file with navfield_host.cpp alone.
#include "navset_host.hpp"

#include <algorithm>

namespace lom {
namespace navset {

bool max_fields_ok(uint64_t max_fields) { return max_fields >= 1u && max_fields <= kMaxFields; }

const char *offsets_refusal(const uint32_t *goal_offsets, size_t n_fields, uint32_t max_fields, const void *goals, size_t *n_goals)
{
    *n_goals = 0;
    if (n_fields > max_fields) return "navigation field set solve: n_fields is 0 .. max_fields";
    if (!n_fields) return nullptr;
    if (!goal_offsets) return "navigation field set solve: goal_offsets, n_fields + 1 of them";
    if (goal_offsets[0] != 0u) return "navigation field set solve: goal_offsets start at 0";
    for (size_t i = 0; i < n_fields; i++)
        if (goal_offsets[i + 1] < goal_offsets[i]) return "navigation field set solve: goal_offsets never fall";
    const size_t n = goal_offsets[n_fields];
    if (n > navfield::kMaxPoints) return "navigation field set solve: at most 2^24 goals";
    if (n && !goals) return "navigation field set solve: goals";
    *n_goals = n;
    return nullptr;
}

void field_of_goals(const uint32_t *goal_offsets, size_t n_fields, uint32_t *out)
{
    for (size_t i = 0; i < n_fields; i++)
        for (uint32_t g = goal_offsets[i]; g < goal_offsets[i + 1]; g++) out[g] = (uint32_t)i;
}

Sizes sizes(uint32_t width, uint32_t height, uint32_t max_fields)
{
    const uint64_t cells = (uint64_t)width * height, tiles = navfield::tile_grid(width, height).n_tiles;
    Sizes s;
    s.fields = cells * 4u * max_fields;  // at most 2^26 * 4 * 2^16 = 2^44
    s.plane = cells;
    s.marks = 2u * tiles * 4u * max_fields;
    s.words = ((uint64_t)max_fields * kFieldWords + kPlaneWords) * 4u;
    return s;
}

RelaxGrid relax_grid(uint32_t width, uint32_t height, uint32_t n_fields)
{
    const navfield::TileGrid t = navfield::tile_grid(width, height);
    return RelaxGrid{t.tiles_x, t.tiles_y, n_fields};
}

uint32_t report_groups(uint64_t n_cells)
{
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_cells + navfield::kThreads - 1u) / navfield::kThreads, 1u), kReportGroups);
}

uint32_t nearest_groups(uint64_t n_cells)
{
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n_cells + navfield::kThreads - 1u) / navfield::kThreads, 1u), kNearestGroups);
}

const char *gather_refusal(int point_kind, const void *points, size_t n, size_t n_fields, const void *out)
{
    if (point_kind != LOM_NAV_CELLS && point_kind != LOM_NAV_METRES) return "navigation field set: points are LOM_NAV_CELLS or LOM_NAV_METRES";
    if ((n && !points) || n > navfield::kMaxPoints) return "navigation field set gather: points, at most 2^24 of them";
    if (n && n_fields > kMaxGatherOut / n) return "navigation field set gather: an output of n_fields * n values, at most 2^28";
    if (n && n_fields && !out) return "navigation field set gather: an output of n_fields * n values";
    return nullptr;
}

bool path_fields_ok(const int32_t *field_of_start, size_t n, size_t n_fields)
{
    if (n && !field_of_start) return false;
    for (size_t k = 0; k < n; k++)
        if (field_of_start[k] < 0 || (uint64_t)field_of_start[k] >= n_fields) return false;
    return true;
}

void summary_of(const uint32_t *w, const uint32_t *pw, uint64_t n_cells, lom_navfield_summary *out)
{
    out->cells_blocked = pw[0], out->cells_invalid = pw[1];
    out->cells_reached = w[0], out->max_potential = w[1], out->range_exceeded = w[2];
    out->goals_used = w[3], out->goals_rejected = w[4];
    out->cells_unreached = n_cells - pw[0] - w[0];
}

}  // namespace navset
}  // namespace lom
