// Host planning of the navigation field set (navset_host.cpp), shared with navset.hip and, for lom_navfield_adopt, with
// navfield.hip.  Plain C++: nothing here needs a device or a HIP header.  The offsets rule, the field index per goal, the
// sizes of a set's storage, the launch shapes, the refusals of gather and paths, and a field's summary from its words.
// Definitions: include/lidar_odometry_amd.h ("navigation field set").
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lidar_odometry_amd.h"
#include "navfield_host.hpp"

namespace lom {
namespace navset {

constexpr uint32_t kMaxFields = 65535;           // blockIdx.z of k_navset_relax; an owner is a u16 and 0xFFFF is "none"
constexpr uint32_t kReportGroups = 64;           // workgroups of k_navset_report per field, at most
constexpr uint32_t kNearestGroups = 2048;        // workgroups of k_navset_nearest, at most
constexpr uint32_t kFieldWords = 8;              // the report's words per field
constexpr uint32_t kPlaneWords = 2;              // ... and of the plane: cells_blocked, cells_invalid
constexpr size_t kMaxGatherOut = (size_t)1 << 28;  // n_fields * n of a gather call

bool max_fields_ok(uint64_t max_fields);  // 1 .. 65535

// The offsets rule of lom_navset_solve: n_fields <= max_fields; with fields, goal_offsets holds n_fields + 1 values that
// start at 0, never fall and end at n_goals <= 2^24, and goals is there where n_goals > 0.  The text of the refusal, or
// NULL; *n_goals is the last offset (0 for a set of no fields, whose offsets are not read).
const char *offsets_refusal(const uint32_t *goal_offsets, size_t n_fields, uint32_t max_fields, const void *goals, size_t *n_goals);
// the field of every goal: out[g] = i for g in [goal_offsets[i], goal_offsets[i + 1]); the offsets are valid
void field_of_goals(const uint32_t *goal_offsets, size_t n_fields, uint32_t *out);

// What a set of max_fields fields over width x height cells keeps in HBM, in bytes: 64-bit throughout, so 8192 x 8192 x
// 65535 does not wrap (the allocation then fails: LOM_ERR_OOM).
struct Sizes {
    uint64_t fields;  // 4 per cell and field
    uint64_t plane;   // 1 per cell
    uint64_t marks;   // [2][max_fields][n_tiles] u32
    uint64_t words;   // [max_fields][kFieldWords] u32 and the plane's
};
Sizes sizes(uint32_t width, uint32_t height, uint32_t max_fields);

// k_navset_relax: a workgroup per (tile, field), grid (tiles_x, tiles_y, n_fields)
struct RelaxGrid {
    uint32_t x, y, z;
    uint64_t groups() const { return (uint64_t)x * y * z; }
};
RelaxGrid relax_grid(uint32_t width, uint32_t height, uint32_t n_fields);
// workgroups per field of k_navset_report (and of k_navset_plane_count): one per 256 cells, at most kReportGroups
uint32_t report_groups(uint64_t n_cells);
uint32_t nearest_groups(uint64_t n_cells);  // one per 256 cells, at most kNearestGroups

// lom_navset_gather: points where n > 0, n <= 2^24, n_fields * n <= 2^28, an output where there is one to write
const char *gather_refusal(int point_kind, const void *points, size_t n, size_t n_fields, const void *out);
// lom_navset_paths: every field_of_start in 0 .. n_fields - 1
bool path_fields_ok(const int32_t *field_of_start, size_t n, size_t n_fields);

// A field's summary from its report words (reached, max potential, range, goals used, goals rejected) and the plane's
// (blocked, invalid): a reached cell is passable, so cells_unreached = cells - blocked - reached.
void summary_of(const uint32_t *field_words, const uint32_t *plane_words, uint64_t n_cells, lom_navfield_summary *out);

}  // namespace navset

// What lom_navfield_adopt (navfield.hip) reads of a set (navset.hip): LOM_ERR_STATE for a set with no solve since create,
// clear or shift, LOM_ERR_ARG for i outside its fields (each with the text in the set), else the view.  The pointers are
// the set's blocks in HBM, complete whenever no call on the set is running.
struct NavSetView {
    int device;
    lom_occupancy_geometry geo;
    const void *plane, *table, *field;  // int8 per cell; 256 u32; u32 per cell, field i
    lom_navfield_summary summary;       // of field i
    void *stream;                       // the set's
};
int navset_view(lom_navset *s, size_t i, NavSetView *out);

}  // namespace lom
