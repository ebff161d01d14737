// Host planning of the map assembly (assemble_host.cpp), shared with archive.hip.  Plain C++: nothing here needs a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lidar_odometry_amd.h"

namespace lom {
namespace assemble {

constexpr uint32_t kAsmThreads = 256;               // workgroup of the k_asm_* kernels: one point per thread
constexpr uint64_t kAsmMaxPoints = 0x7FFFFFFEull;   // points of one call: what one insert takes
constexpr uint64_t kArchiveMaxPoints = 1ull << 32;  // the kernels index an archive's points with 32 bits
constexpr size_t kAsmMaxScans = size_t(1) << 24;    // scans of one call (the [scan][block] matrix stays inside 32 bits)
constexpr uint32_t kAsmScansPerLaunch = 32768;      // blockIdx.y of one launch

// a scan of the archive: its first point and its length
struct ScanEntry {
    uint64_t offset;
    uint32_t n;
};

// what a workgroup of k_asm_transform / k_asm_compact reads about its scan (constant address space, scalar loads)
struct AsmScan {
    uint32_t src;  // first point of the scan in the archive
    uint32_t n;
    uint32_t out;  // first point of the scan in the concatenated, un-culled cloud
    uint32_t blk;  // first entry of the scan's row in the [scan][block] matrix of kept counts
    double R[9];   // row-major, from the normalised quaternion (rotation_matrix below)
    double t[3];
};
static_assert(sizeof(AsmScan) == 112, "descriptor layout");

struct Plan {
    std::vector<AsmScan> scans;  // call order
    uint64_t points_in = 0;      // sum of n
    uint32_t max_n = 0;          // the largest scan: blockIdx.x runs over it
    uint32_t grid_x = 0;         // workgroups of the largest scan
    uint32_t blocks = 0;         // entries of the [scan][block] matrix (ragged: a scan has ceil(n / kAsmThreads))
};

bool pose_ok(const lom_graph_pose *p);              // finite, quaternion of non-zero length (as lom_graph_add_node)
void normalised_quaternion(const lom_graph_pose *p, double q[4]);  // q / |q|, |q|^2 summed w, x, y, z
void rotation_matrix(const double q[4], double R[9]);              // the header's formula, from a normalised quaternion

// Checks ids and poses against the archive's table and fills the descriptors.  LOM_OK, or LOM_ERR_ARG with `why`.
int plan(const ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count, Plan &out,
         std::string &why);
// params_or_null: NULL or radius <= 0 keeps everything (*cull = false); a non-finite value is LOM_ERR_ARG
int cull_of(const lom_assemble_params *params_or_null, bool *cull, std::string &why);

// ---- what the planners built on these descriptors share (vote_host, occupancy_host, elevation_host) ----------------
// scans [first, first + count) of a call: one launch over the descriptors desc + first, blockIdx.y over its scans
struct Launch {
    uint32_t first, count;
    uint32_t max_n;   // the largest scan of the launch
    uint32_t grid_x;  // its workgroups
};
// The scans of a plan cut into launches of at most `per` scans (>= 1), in call order; a launch of empty scans only is
// not listed.
std::vector<Launch> cut_launches(const Plan &plan, uint32_t per);

// value ranges (a NaN fails every comparison)
constexpr float kBig = 3.402823466e+38f;
inline bool finite_f(float v) { return v >= -kBig && v <= kBig; }
inline bool positive_f(float v) { return v > 0.f && v <= kBig; }

constexpr int32_t kCellLimit = 1 << 30;  // |start cell| of a scan on a 2-D grid stays below
// The start cell of scan d on a 2-D grid (the occupancy definition's step 2); false: |c_a| >= 2^30 or not finite.
// Geometry: anything with resolution, origin_x and origin_y -- a family's geometry, or the three alone.
struct GridFrame {
    float resolution, origin_x, origin_y;
};
template <class Geometry>
bool origin_cell(const AsmScan &d, const Geometry &g, int32_t c[2])
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
// What the planners of the 2-D grids begin with: ids and poses are checked as lom_map_assemble checks them (plan above),
// then the family's verdict on its parameters (false: LOM_ERR_ARG, params_why), then every origin's range (LOM_ERR_RANGE).
// cells: the start cells (x, y per scan, call order).  A refusal leaves `out` and `cells` empty.
int plan_on_grid(const ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                 const GridFrame &frame, bool params_ok, const char *params_why, Plan &out,
                 std::vector<int32_t> &cells, std::string &why);

}  // namespace assemble
}  // namespace lom
