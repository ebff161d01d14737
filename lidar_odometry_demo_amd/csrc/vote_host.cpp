// Host planning of lom_map_carve_scans / lom_map_scan_votes: parameter ranges, the slices of a call, the step bound.
// Plain C++, no HIP: vote.hip calls these, and tests/cpp/test_vote.cpp compiles this file and assemble_host.cpp alone.
#include "vote_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace vote {

bool params_ok(const lom_vote_params *p)
{
    using assemble::kBig;  // (a NaN fails every comparison below)
    return p && p->margin >= 0.f && p->margin <= kBig && p->min_range > 0.f && p->max_range > p->min_range &&
           p->max_range <= kBig && p->clearance >= 0.f && p->clearance <= kBig && p->min_free_scans >= 1u;
}

uint32_t max_steps(float max_range, float voxel_size)
{
    // (no ray is longer than the index range: 2^21 cells per axis)
    const double cells = std::min(std::ceil((double)max_range / (double)voxel_size), 2097152.0);
    return 3u * ((uint32_t)cells + 2u);
}

bool origin_ok(const assemble::AsmScan &d, float voxel_size)
{
    for (int a = 0; a < 3; a++) {
        const float f = (float)d.t[a] / voxel_size;
        if (!(f > -1048576.0f && f < 1048576.0f)) return false;  // also NaN and an infinity from the rounding
    }
    return true;
}

int plan(const assemble::ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
         const lom_vote_params *p, uint32_t slice_max, Plan &out, std::string &why)
{
    out.slices.clear();
    const int rc = assemble::plan(table, n_scans, ids, poses, count, out.scans, why);
    if (rc != LOM_OK) return rc;
    if (!params_ok(p)) {
        out.scans = assemble::Plan();
        why = "vote parameters: margin >= 0, 0 < min_range < max_range, clearance >= 0, all finite, min_free_scans >= 1";
        return LOM_ERR_ARG;
    }
    out.slices = assemble::cut_launches(out.scans, (slice_max == 0 || slice_max > kSliceScans) ? kSliceScans : slice_max);
    return LOM_OK;
}

}  // namespace vote
}  // namespace lom
