// Host planning of the scan votes (vote_host.cpp), shared with vote.hip.  Plain C++: nothing here needs a device.
// The scan descriptors and their checks are the assembly's (assemble_host.hpp); what is added is the value ranges of
// lom_vote_params, the origins' range verdict, the step bound of the walk and the slices a call is launched in.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "assemble_host.hpp"

namespace lom {
namespace vote {

constexpr uint32_t kSliceScans = 64;  // scans of one launch: a bit each in a voxel's 64-bit hit and cross masks

// scans [first, first + count) of the call: one launch of k_vote_walk over the descriptors desc + first, one k_vote_fold
using Slice = assemble::Launch;

struct Plan {
    assemble::Plan scans;       // descriptors in call order (out / blk are the assembly's and not read here)
    std::vector<Slice> slices;  // in call order; a slice of empty scans only is not listed
};

// margin >= 0, 0 < min_range < max_range, clearance >= 0, all finite, min_free_scans >= 1
bool params_ok(const lom_vote_params *p);
// 3 * (ceil(max_range / V) + 2), the carve's bound: a guard, the walk ends by itself before
uint32_t max_steps(float max_range, float voxel_size);
// the origin of scan d, each component rounded to f32, and whether its voxel index stays inside (-2^20, 2^20)
bool origin_ok(const assemble::AsmScan &d, float voxel_size);

// Ids and poses are checked as lom_map_assemble checks them (assemble::plan), then the parameters; the slices hold at
// most slice_max scans (0 or more than kSliceScans: kSliceScans).  LOM_OK, or LOM_ERR_ARG with `why`.
int plan(const assemble::ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
         const lom_vote_params *p, uint32_t slice_max, Plan &out, std::string &why);

}  // namespace vote
}  // namespace lom
