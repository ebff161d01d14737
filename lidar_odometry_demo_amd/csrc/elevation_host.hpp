// Host planning of the elevation grid (elevation_host.cpp), shared with elevation.hip.  Plain C++: nothing here needs a
// device.  The scan descriptors and their checks are the assembly's (assemble_host.hpp); what is added is the value
// ranges of the geometry and of the point, layer and cost parameters.  The origins' start cells and their range verdict
// (assemble::origin_cell) and the cut into launches are shared with the occupancy grid and live there too.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "assemble_host.hpp"

namespace lom {
namespace elevation {

constexpr uint32_t kMaxSide = 8192;      // cells per axis
constexpr uint32_t kMaxWindow = 4;       // R of the layer parameters
constexpr uint32_t kScansPerLaunch = assemble::kAsmScansPerLaunch;  // blockIdx.y of one launch

// scans [first, first + count) of the call: one launch of k_elev_accumulate over the descriptors desc + first
using Launch = assemble::Launch;

struct Plan {
    assemble::Plan scans;         // descriptors in call order (out / blk are the assembly's and not read here)
    std::vector<Launch> launches;  // in call order; a launch of empty scans only is not listed
};

// resolution > 0 and finite, a finite origin and z_ref, 1 <= width, height <= 8192
bool geometry_ok(const lom_elevation_geometry *g);
// z_lo < 0 < z_hi, 0 < min_range < max_range, all finite, max_range / resolution <= 2^20
bool point_params_ok(const lom_elevation_point_params *p, float resolution);
// min_points >= 1, 1 <= window <= 4
bool layer_params_ok(const lom_elevation_layer_params *p);
// all four finite and > 0
bool cost_params_ok(const lom_elevation_cost_params *p);

// Ids and poses are checked as lom_map_assemble checks them (assemble::plan), then the parameters (LOM_ERR_ARG), then
// every origin's range (LOM_ERR_RANGE); a launch holds at most scans_per_launch scans (0: kScansPerLaunch).
int plan(const assemble::ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
         const lom_elevation_geometry &g, const lom_elevation_point_params *p, uint32_t scans_per_launch, Plan &out,
         std::string &why);

}  // namespace elevation
}  // namespace lom
