// Pose field: the least total cost to reach a goal state, per cell and heading, for a robot's footprint over an int8 cost
// plane; the floor over the headings, paths down the field and point queries.  Definitions: include/lidar_odometry_amd.h
// ("pose field"); kernels: k_posefield.hpp; the move rule: pose_rule.hpp; host planning (value ranges, stencils, tile
// counts, launch shapes): posefield_host.cpp; DESIGN.md 7u.  A handle family of its own on the PlaneHandle core
// (plane_handle.hpp), the three forms of the cost plane through its PlaneSource; the host loop to the fixed
// point is nav_fixed_point.hpp's.  The re-solve after a local cost change (k_posefield_resolve.hpp) keeps
// what a solve left and repairs it.  No default path launches any of this.
#include <algorithm>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "k_posefield_resolve.hpp"
#include "nav_fixed_point.hpp"
#include "navfield_host.hpp"
#include "plane_handle.hpp"
#include "posefield_host.hpp"

using namespace lom;

static_assert(posefield::kThreads == kPoseThreads && posefield::kTileX == kPoseTileX && posefield::kTileY == kPoseTileY &&
                  posefield::kMaxStencil == kPoseMaxStencil && posefield::kMaxWeight <= kPoseMaxWeight,
              "posefield_host.hpp and k_posefield.hpp disagree");
static_assert(LOM_NAV_UNREACHED == kPoseUnreached && LOM_NAV_MAX == kPoseMax, "the header and k_posefield.hpp disagree");
static_assert((kPoseHeadings * kPoseHaloCells * 2u + 4u) * 4u <= 64u * 1024u, "the LDS of k_pose_relax stays at or below 64 KB");
static_assert((size_t)QW_END * 4u <= 128u, "the words of a re-solve fit the block");

// The field owns its stream and every buffer below.
struct lom_posefield : lom::PlaneHandle {  // in_ev: the clearance grid's
    posefield::TileGrid tiles{};
    lom::DeviceBuf field;            // P: [8][height][width] u32
    lom::DeviceBuf layers;           // L: likewise
    lom::DeviceBuf floor;            // u32 per cell
    lom::DeviceBuf floor_heading;    // u8 per cell
    lom::DeviceBuf plane;            // the cost bytes of the last solve
    lom::DeviceBuf table;            // 256 u32: the cell costs of the last solve
    lom::DeviceBuf stencil_cells;    // 8 x 1024 (dx, dy) int16 pairs at most, heading after heading
    lom::DeviceBuf stencil_first;    // 9 u32: where a heading's cells start
    lom::DeviceBuf marks;            // 2 x n_tiles u32: the tiles active in an even and in an odd launch
    lom::DeviceBuf flags;            // kBatchMax u32: "launch j of the batch marked a tile"
    lom::DeviceBuf words;            // the summary words, and behind them a re-solve's
    lom::DeviceBuf seeds;            // n_tiles u32: the seeds of a re-solve's relaxation; empty until the first re-solve
    lom::DeviceBuf incoming;         // the window's rows of a re-solve's host plane, grow-only
    lom::DeviceBuf points;           // goals or starts as int32 triples, grow-only
    lom::DeviceBuf path_states, path_lengths;  // a paths call's results, grow-only
    lom::DeviceBuf q_xy, q_h, q_out; // a query's points, headings and results, grow-only
    lom::PinnedBuf h_table;          // the table, and behind it the stencils, on their way in
    lom::PinnedBuf h_flags;          // the batch's flags and the summary words on their way out
    uint32_t inner_cap = navfield::kInnerCapDefault;  // LOM_POSE_OPT_TEST_INNER_CAP
    uint32_t batch = navfield::kBatchDefault;         // LOM_POSE_OPT_TEST_BATCH
    uint32_t all_tiles = 0;                           // LOM_POSE_OPT_TEST_ALL_TILES
    uint32_t resolve_form = 0;                        // LOM_POSE_OPT_TEST_RESOLVE_FORM
    PoseCosts costs{};               // of the last solve: what paths walk under
    posefield::Stencils stencils{};  // of the last solve: what a re-solve dilates the changed box by
    lom_posefield_solve_stats stats{};
    lom_posefield_resolve_counters resolve_stats{};
    bool solved = false;             // a solve has completed since create, clear or shift: plane, layers and P are a fixed point
    uint32_t last_words[PW_COUNT] = {};  // ... and its summary words: what a re-solve that changes nothing reports

    PoseArgs args() const { return PoseArgs{geo.width, geo.height, tiles.tiles_x, tiles.tiles_y}; }
    size_t n_states() const { return n_cells() * kPoseHeadings; }
};

namespace {

thread_local std::string g_posefield_create_error;

constexpr const char *kName = "pose field";  // the head of the texts of the plane-handle core

constexpr const char *kParamsText =
    "pose field parameters: nav by the navigation field's rule, turn_cost, spin_cost, reverse_cost <= 2^24 - 1, spin_cost >= 1 "
    "under LOM_POSE_SPIN, known flags";

constexpr size_t kStencilWords = (size_t)kPoseHeadings * kPoseMaxStencil;  // u32 pairs of the stencils, at most
constexpr size_t kStagingBytes = (256 + kStencilWords + 16) * 4;           // the table, the stencil cells, first[9]

// every state unreached, no tile marked; with `all` every state impassable too: the layers, the floor, the plane, the table
int fill(lom_posefield *f, bool all)
{
    const size_t n = std::max(f->n_cells(), (size_t)2 * f->tiles.n_tiles);
    hipLaunchKernelGGL(k_pose_fill, dim3(posefield::blocks_for(n)), dim3(kPoseThreads), 0, f->stream, (uint32_t)f->n_cells(),
                       2u * f->tiles.n_tiles, all ? 1u : 0u, f->field.as<uint32_t>(), f->layers.as<uint32_t>(), f->floor.as<uint32_t>(),
                       f->floor_heading.as<uint8_t>(), f->marks.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    if (all) {
        LOM_HIP(f, hipMemsetAsync(f->plane.p, 0xFF, f->n_cells(), f->stream));
        LOM_HIP(f, hipMemsetAsync(f->table.p, 0, 256 * 4, f->stream));
    }
    return LOM_OK;
}

void summary_from(const uint32_t *t, lom_posefield_summary *s)
{
    s->states_blocked = t[PW_BLOCKED], s->states_reached = t[PW_REACHED], s->states_unreached = t[PW_UNREACHED];
    s->cells_reached = t[PW_CELLS_REACHED], s->cells_invalid = t[PW_INVALID], s->goals_used = t[PW_GOALS_USED];
    s->goals_rejected = t[PW_GOALS_REJECTED], s->range_exceeded = t[PW_RANGE], s->max_potential = t[PW_MAX_POTENTIAL];
}

// the refusals of every solve form that need no device: the text, or NULL
const char *solve_refusal(bool have_plane, const lom_posefield_params *p, const int32_t *footprint, size_t n_samples, const int32_t *goals,
                          size_t n_goals)
{
    if (!have_plane) return "pose field solve: a cost plane";
    if (!posefield::params_ok(p)) return kParamsText;
    if (!posefield::footprint_ok(footprint, n_samples)) return "pose field solve: a footprint of 1 .. 1024 samples with |fx|, |fy| <= 16384";
    if ((n_goals && !goals) || n_goals > posefield::kMaxPoints) return "pose field solve: goals, at most 2^24 of them";
    return nullptr;
}

// the relaxation from the marks of the first array to its fixed point
int relax(lom_posefield *f, uint64_t &launches, uint64_t &waits)
{
    const PoseArgs a = f->args();
    return to_fixed_point(f, f->tiles.n_tiles, launches, waits, "pose field: the relaxation did not settle",
                          [&](uint32_t *cur, uint32_t *nxt, uint32_t *flag) {
                              hipLaunchKernelGGL(k_pose_relax, dim3(f->tiles.tiles_x, f->tiles.tiles_y), dim3(kPoseThreads), 0, f->stream,
                                                 f->layers.as<const uint32_t>(), a, f->costs, f->inner_cap, f->all_tiles, f->field.as<uint32_t>(),
                                                 cur, nxt, flag);
                          });
}

// the summary of the field as it stands: the report, the way out of the first n_words words, done_ev, the wait.  The words
// are in h_flags.
int report(lom_posefield *f, uint32_t n_words)
{
    hipLaunchKernelGGL(k_pose_report, dim3(posefield::report_groups(f->n_cells())), dim3(kPoseThreads), 0, f->stream,
                       f->plane.as<const int8_t>(), f->layers.as<const uint32_t>(), f->field.as<const uint32_t>(), f->args(), f->costs,
                       f->floor.as<uint32_t>(), f->floor_heading.as<uint8_t>(), f->words.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    LOM_HIP(f, hipMemcpyAsync(f->h_flags.h, f->words.p, (size_t)n_words * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

// A solve over a plane in HBM that this stream may read now: the copy of the plane, the layers, the seed, the relaxation
// in batches of launches with one wait each, the report, then the wait.  The arguments are valid.
int solve_on_device(lom_posefield *f, const int8_t *d_plane, const lom_posefield_params &p, const int32_t *footprint, size_t n_samples,
                    const int32_t *goals, size_t n_goals, lom_posefield_summary *summary)
{
    // what needs no device and what can still fail for want of memory come first: a refused call changes nothing
    posefield::Stencils st = posefield::stencils(footprint, n_samples);
    if (const int rc = n_goals ? ensure(f, f->points, n_goals * 12) : LOM_OK; rc != LOM_OK) return rc;
    f->solved = false;
    // (every call waits for its work: nothing enqueued reads the staging block)
    uint32_t *const staging = f->h_table.as<uint32_t>();
    navfield::cell_costs(p.nav, staging);
    std::memcpy(staging + 256, st.cells.data(), st.cells.size() * sizeof(int16_t));
    std::memcpy(staging + 256 + kStencilWords, st.first, sizeof st.first);
    LOM_HIP(f, hipMemcpyAsync(f->table.p, staging, 256 * 4, hipMemcpyHostToDevice, f->stream));
    LOM_HIP(f, hipMemcpyAsync(f->stencil_cells.p, staging + 256, (size_t)st.first[kPoseHeadings] * 4, hipMemcpyHostToDevice, f->stream));
    LOM_HIP(f, hipMemcpyAsync(f->stencil_first.p, staging + 256 + kStencilWords, sizeof st.first, hipMemcpyHostToDevice, f->stream));
    if (n_goals) LOM_HIP(f, hipMemcpyAsync(f->points.p, goals, n_goals * 12, hipMemcpyHostToDevice, f->stream));
    if (d_plane != f->plane.as<const int8_t>())
        LOM_HIP(f, hipMemcpyAsync(f->plane.p, d_plane, f->n_cells(), hipMemcpyDeviceToDevice, f->stream));
    LOM_HIP(f, hipMemsetAsync(f->words.p, 0, (size_t)PW_COUNT * 4, f->stream));
    f->costs = posefield::costs_of(p);
    const PoseArgs a = f->args();
    const uint32_t *const layers = f->layers.as<const uint32_t>();
    hipLaunchKernelGGL(k_pose_layers, dim3(posefield::blocks_for(f->n_cells()), kPoseHeadings), dim3(kPoseThreads), 0, f->stream,
                       f->plane.as<const int8_t>(), f->table.as<const uint32_t>(), a, f->stencil_cells.as<const uint32_t>(),
                       f->stencil_first.as<const uint32_t>(), f->layers.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    if (const int rc = fill(f, false); rc != LOM_OK) return rc;
    if (n_goals) {
        hipLaunchKernelGGL(k_pose_seed, dim3(posefield::blocks_for(n_goals)), dim3(kPoseThreads), 0, f->stream, layers, a,
                           f->points.as<const int32_t>(), (uint32_t)n_goals, f->field.as<uint32_t>(), f->marks.as<uint32_t>(),
                           f->words.as<uint32_t>());
        LOM_HIP(f, hipGetLastError());
    }
    f->stats = lom_posefield_solve_stats{0, 0, f->tiles.n_tiles};
    if (const int rc = relax(f, f->stats.launches, f->stats.waits); rc != LOM_OK) return rc;
    if (const int rc = report(f, PW_COUNT); rc != LOM_OK) return rc;
    std::memcpy(f->last_words, f->h_flags.h, sizeof f->last_words);
    f->stencils = std::move(st);
    f->solved = true;
    if (summary) summary_from(f->h_flags.as<uint32_t>(), summary);
    return LOM_OK;
}

// the refusals of every re-solve form that need no device: the code and the text, or LOM_OK
int resolve_refusal(lom_posefield *f, bool have_plane)
{
    if (!have_plane) return fail(f, LOM_ERR_ARG, "pose field re-solve: a cost plane");
    if (!f->solved) return fail(f, LOM_ERR_STATE, "pose field re-solve: no solve has completed since create, clear or shift");
    return LOM_OK;
}

// A re-solve from a plane in HBM that this stream may read now, over a window that is not empty: the diff and a wait; then,
// where a cell changed, the layers over the dilated boxes, the raise phase to its fixed point (form 1: the layers over the
// whole plane and the reset), the relaxation from the seeds to its fixed point, the report and the wait.  done_ev stands
// behind the diff, the one reader of d_new.
int resolve_on_device(lom_posefield *f, const int8_t *d_new, const clearance::Rect &r, lom_posefield_summary *summary)
{
    const PoseArgs a = f->args();
    const uint32_t n_tiles = f->tiles.n_tiles, form = f->resolve_form;
    // what can still fail for want of memory comes first: a refused call changes nothing
    if (const int rc = ensure(f, f->seeds, (size_t)n_tiles * 4); rc != LOM_OK) return rc;
    const int8_t *const plane = f->plane.as<const int8_t>();
    const uint32_t *const table = f->table.as<const uint32_t>();
    uint32_t *const layers = f->layers.as<uint32_t>(), *const field = f->field.as<uint32_t>(), *const words = f->words.as<uint32_t>();
    uint32_t *const marks0 = f->marks.as<uint32_t>(), *const seeds = f->seeds.as<uint32_t>();
    uint32_t *const h = f->h_flags.as<uint32_t>();
    lom_posefield_resolve_counters &st = f->resolve_stats;
    st = lom_posefield_resolve_counters{};
    LOM_HIP(f, hipMemsetAsync(f->words.p, 0, (size_t)QW_END * 4, f->stream));
    hipLaunchKernelGGL(k_pose_diff, dim3((r.x1 - r.x0 + kPoseTileX - 1u) / kPoseTileX, (r.y1 - r.y0 + kPoseTileY - 1u) / kPoseTileY),
                       dim3(kPoseThreads), 0, f->stream, d_new, a, PoseBox{r.x0, r.y0, r.x1, r.y1}, f->plane.as<int8_t>(), words);
    LOM_HIP(f, hipGetLastError());
    f->solved = false;
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    LOM_HIP(f, hipMemcpyAsync(h, f->words.p, (size_t)QW_END * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    st.waits = 1;
    st.cells_changed = h[QW_CHANGED];
    uint32_t rejected = 0u;
    if (st.cells_changed != 0u) {
        const PoseBoxes boxes = posefield::relayer_boxes(f->stencils, PoseBox{~h[QW_X0_INV], ~h[QW_Y0_INV], h[QW_X1], h[QW_Y1]}, a.width, a.height);
        LOM_HIP(f, hipMemsetAsync(f->marks.p, 0, (size_t)2 * n_tiles * 4, f->stream));
        LOM_HIP(f, hipMemsetAsync(f->seeds.p, 0, (size_t)n_tiles * 4, f->stream));
        // form 0: the seeds gather from here on, and the raise phase starts from the same tiles; form 1: the goal states'
        // tiles are the seeds, and this launch only counts and takes the goal states that became impassable
        if (!boxes.all.empty()) {
            const size_t lanes = (size_t)(boxes.all.x1 - boxes.all.x0) * (boxes.all.y1 - boxes.all.y0);
            hipLaunchKernelGGL(k_pose_relayer, dim3(posefield::blocks_for(lanes), kPoseHeadings), dim3(kPoseThreads), 0, f->stream, plane, table, a,
                               f->stencil_cells.as<const uint32_t>(), f->stencil_first.as<const uint32_t>(), boxes, layers, field,
                               form == 0u ? marks0 : nullptr, form == 0u ? seeds : nullptr, words);
            LOM_HIP(f, hipGetLastError());
        }
        if (form == 0u) {
            const int rc = to_fixed_point(f, n_tiles, st.raise_launches, st.waits, "pose field: the raise phase did not settle",
                                          [&](uint32_t *cur, uint32_t *nxt, uint32_t *flag) {
                                              hipLaunchKernelGGL(k_pose_raise, dim3(f->tiles.tiles_x, f->tiles.tiles_y), dim3(kPoseThreads), 0,
                                                                 f->stream, layers, a, f->costs, f->inner_cap, f->all_tiles, field, cur, nxt, seeds,
                                                                 flag, words);
                                          });
            if (rc != LOM_OK) return rc;
            // (both arrays of the fixed point are clear: the seeds are the first launch's marks)
            LOM_HIP(f, hipMemcpyAsync(marks0, seeds, (size_t)n_tiles * 4, hipMemcpyDeviceToDevice, f->stream));
        } else {
            hipLaunchKernelGGL(k_pose_layers, dim3(posefield::blocks_for(f->n_cells()), kPoseHeadings), dim3(kPoseThreads), 0, f->stream, plane,
                               table, a, f->stencil_cells.as<const uint32_t>(), f->stencil_first.as<const uint32_t>(), layers);
            LOM_HIP(f, hipGetLastError());
            hipLaunchKernelGGL(k_pose_reseed, dim3(posefield::blocks_for(f->n_cells())), dim3(kPoseThreads), 0, f->stream, a, field, marks0, words);
            LOM_HIP(f, hipGetLastError());
        }
        if (const int rc = relax(f, st.relax_launches, st.waits); rc != LOM_OK) return rc;
        if (const int rc = report(f, QW_END); rc != LOM_OK) return rc;
        st.waits++;
        st.states_changed = h[QW_STATES], st.states_raised = h[QW_RAISED], st.tiles_marked = h[QW_TILES];
        rejected = h[PW_GOALS_REJECTED];
        h[PW_GOALS_USED] = f->last_words[PW_GOALS_USED] - rejected;  // (the report counts states: the goals are the host's to keep)
        std::memcpy(f->last_words, h, sizeof f->last_words);
    }
    f->last_words[PW_GOALS_REJECTED] = rejected;
    f->solved = true;
    if (summary) summary_from(f->last_words, summary);
    return LOM_OK;
}

// the summary of a re-solve over an empty window: the field as it stands, no goal rejected
int resolve_nothing(lom_posefield *f, lom_posefield_summary *summary)
{
    f->resolve_stats = lom_posefield_resolve_counters{};
    f->last_words[PW_GOALS_REJECTED] = 0u;
    if (summary) summary_from(f->last_words, summary);
    return LOM_OK;
}

// ---- one function per operation over the source of the plane (plane_handle.hpp) ---------------------------
// Each in one order: the refusals, the way out that needs no device, what can fail for want of memory, open, upload, body, close.
int solve_from(lom_posefield *f, const PlaneSource &src, const lom_posefield_params *params, const int32_t *footprint, size_t n_samples,
               const int32_t *goals, size_t n_goals, lom_posefield_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!f) return LOM_ERR_ARG;
    if (const char *why = solve_refusal(src.given(), params, footprint, n_samples, goals, n_goals)) return fail(f, LOM_ERR_ARG, why);
    if (const int rc = plane_source_check(f, kName, src, f->geo); rc != LOM_OK) return rc;
    LOM_HIP(f, hipSetDevice(f->device));
    // the goals first: their buffer is what can still be refused (no memory); then a host plane goes straight to the field's copy
    if (const int rc = n_goals ? ensure(f, f->points, n_goals * 12) : LOM_OK; rc != LOM_OK) return rc;
    const int8_t *d_plane = nullptr;
    if (const int rc = plane_source_open(f, kName, src, &d_plane); rc != LOM_OK) return rc;
    if (src.host) {
        LOM_HIP(f, hipMemcpyAsync(f->plane.p, src.host, f->n_cells(), hipMemcpyHostToDevice, f->stream));
        d_plane = f->plane.as<const int8_t>();
    }
    if (const int rc = solve_on_device(f, d_plane, *params, footprint, n_samples, goals, n_goals, summary); rc != LOM_OK) return rc;
    return plane_source_close(f, kName, src);
}

int resolve_from(lom_posefield *f, const PlaneSource &src, const lom_clearance_window *window_or_null, lom_posefield_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!f) return LOM_ERR_ARG;
    if (const int rc = resolve_refusal(f, src.given()); rc != LOM_OK) return rc;
    if (const int rc = plane_source_check(f, kName, src, f->geo); rc != LOM_OK) return rc;
    const clearance::Rect r = clearance::clip(window_or_null, f->geo);
    if (r.empty()) return resolve_nothing(f, summary);
    LOM_HIP(f, hipSetDevice(f->device));
    const int8_t *d_plane = nullptr;
    if (const int rc = plane_source_open(f, kName, src, &d_plane); rc != LOM_OK) return rc;
    if (src.host) {
        // the rows of the window, whole, at their place in a plane of the device: the cells outside the window are not read
        if (const int rc = ensure(f, f->incoming, f->n_cells()); rc != LOM_OK) return rc;
        const size_t first = (size_t)r.y0 * f->geo.width, bytes = (size_t)(r.y1 - r.y0) * f->geo.width;
        LOM_HIP(f, hipMemcpyAsync(f->incoming.as<int8_t>() + first, src.host + first, bytes, hipMemcpyHostToDevice, f->stream));
        d_plane = f->incoming.as<const int8_t>();
    }
    if (const int rc = resolve_on_device(f, d_plane, r, summary); rc != LOM_OK) return rc;
    return plane_source_close(f, kName, src);
}

}  // namespace

extern "C" {

int lom_posefield_create(const lom_occupancy_geometry *geometry, int device, lom_posefield **out)
{
    if (!out) return LOM_ERR_ARG;
    lom_posefield *f = nullptr;
    int rc = plane_new(geometry, device, g_posefield_create_error, kName, "pose field setup", 1, &f);
    if (rc != LOM_OK) return rc;
    f->tiles = posefield::tile_grid(geometry->width, geometry->height);
    hipError_t e = alloc(f->h_table, kStagingBytes, hipHostMallocDefault);
    if (e == hipSuccess) e = alloc(f->h_flags, (size_t)navfield::kBatchMax * 4, hipHostMallocDefault);
    if (e != hipSuccess) rc = create_fail(g_posefield_create_error, LOM_ERR_HIP, "pose field setup", e);
    const size_t n = f->n_cells();
    if (rc == LOM_OK &&
        (alloc(f->field, n * 32) != hipSuccess || alloc(f->layers, n * 32) != hipSuccess || alloc(f->floor, n * 4) != hipSuccess ||
         alloc(f->floor_heading, n) != hipSuccess || alloc(f->plane, n) != hipSuccess || alloc(f->table, 256 * 4) != hipSuccess ||
         alloc(f->stencil_cells, kStencilWords * 4) != hipSuccess || alloc(f->stencil_first, 16 * 4) != hipSuccess ||
         alloc(f->marks, (size_t)2 * f->tiles.n_tiles * 4) != hipSuccess || alloc(f->flags, (size_t)navfield::kBatchMax * 4) != hipSuccess ||
         alloc(f->words, 128) != hipSuccess))
        rc = create_fail(g_posefield_create_error, LOM_ERR_OOM, "hipMalloc (pose field)");
    if (rc == LOM_OK) {
        if (fill(f, true) != LOM_OK || (e = hipStreamSynchronize(f->stream)) != hipSuccess)
            rc = create_fail(g_posefield_create_error, LOM_ERR_HIP, f->error.empty() ? "pose field setup" : f->error.c_str(), e);
    }
    if (rc != LOM_OK) {
        lom_posefield_destroy(f);
        return rc;
    }
    *out = f;
    return LOM_OK;
}

void lom_posefield_destroy(lom_posefield *f) { plane_destroy(f); }
const char *lom_posefield_last_error(const lom_posefield *f) { return plane_last_error(f, g_posefield_create_error); }

int lom_posefield_clear(lom_posefield *f)
{
    if (!f) return LOM_ERR_ARG;
    LOM_HIP(f, hipSetDevice(f->device));
    f->costs = PoseCosts{};
    f->solved = false;
    if (const int rc = fill(f, true); rc != LOM_OK) return rc;
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

int lom_posefield_shift(lom_posefield *f, int32_t dx, int32_t dy) { return plane_shift(f, kName, dx, dy, &lom_posefield_clear); }
int lom_posefield_get_geometry(const lom_posefield *f, lom_occupancy_geometry *out) { return plane_get_geometry(f, out); }
void *lom_posefield_stream(lom_posefield *f) { return plane_stream(f); }
int lom_posefield_device(const lom_posefield *f) { return plane_device(f); }
int lom_posefield_wait_event(lom_posefield *f, void *hip_event) { return plane_wait_event(f, hip_event); }

int lom_posefield_set_option(lom_posefield *f, int option, int64_t value)
{
    if (!f) return LOM_ERR_ARG;
    switch (option) {
    case LOM_POSE_OPT_TEST_INNER_CAP:
        return set_test_option(f, f->inner_cap, value, navfield::kInnerCapMax, navfield::kInnerCapDefault,
                               "LOM_POSE_OPT_TEST_INNER_CAP: 1 .. 2^20, or <= 0 for the default");
    case LOM_POSE_OPT_TEST_BATCH:
        return set_test_option(f, f->batch, value, navfield::kBatchMax, navfield::kBatchDefault,
                               "LOM_POSE_OPT_TEST_BATCH: 1 .. 256, or <= 0 for the default");
    case LOM_POSE_OPT_TEST_ALL_TILES:
        return set_test_option(f, f->all_tiles, value, 1, 0, "LOM_POSE_OPT_TEST_ALL_TILES: 0, 1, or < 0 for the default");
    case LOM_POSE_OPT_TEST_RESOLVE_FORM:
        return set_test_option(f, f->resolve_form, value, 1, 0, "LOM_POSE_OPT_TEST_RESOLVE_FORM: 0, 1, or < 0 for the default");
    default:
        return fail(f, LOM_ERR_ARG, "unknown pose field option");
    }
}

int lom_posefield_solve(lom_posefield *f, const int8_t *plane, const lom_posefield_params *params, const int32_t *footprint,
                        size_t n_samples, const int32_t *goals, size_t n_goals, lom_posefield_summary *summary)
{
    return solve_from(f, plane_from_host(plane), params, footprint, n_samples, goals, n_goals, summary);
}

int lom_posefield_solve_device(lom_posefield *f, const int8_t *d_plane, void *hip_event_or_null, const lom_posefield_params *params,
                               const int32_t *footprint, size_t n_samples, const int32_t *goals, size_t n_goals,
                               lom_posefield_summary *summary)
{
    return solve_from(f, plane_from_device(d_plane, hip_event_or_null), params, footprint, n_samples, goals, n_goals, summary);
}

int lom_posefield_solve_from_clearance(lom_posefield *f, lom_clearance *clearance, const lom_posefield_params *params,
                                       const int32_t *footprint, size_t n_samples, const int32_t *goals, size_t n_goals,
                                       lom_posefield_summary *summary)
{
    return solve_from(f, plane_from_clearance(clearance), params, footprint, n_samples, goals, n_goals, summary);
}

int lom_posefield_resolve(lom_posefield *f, const int8_t *plane, const lom_clearance_window *window_or_null, lom_posefield_summary *summary)
{
    return resolve_from(f, plane_from_host(plane), window_or_null, summary);
}

int lom_posefield_resolve_device(lom_posefield *f, const int8_t *d_plane, void *hip_event_or_null, const lom_clearance_window *window_or_null,
                                 lom_posefield_summary *summary)
{
    return resolve_from(f, plane_from_device(d_plane, hip_event_or_null), window_or_null, summary);
}

int lom_posefield_resolve_from_clearance(lom_posefield *f, lom_clearance *clearance, const lom_clearance_window *window_or_null,
                                         lom_posefield_summary *summary)
{
    return resolve_from(f, plane_from_clearance(clearance), window_or_null, summary);
}

int lom_posefield_resolve_stats(const lom_posefield *f, lom_posefield_resolve_counters *out)
{
    if (!f || !out) return LOM_ERR_ARG;
    *out = f->resolve_stats;
    return LOM_OK;
}

int lom_posefield_potential(lom_posefield *f, uint32_t *out, size_t cap)
{
    if (!f || (cap && !out)) return LOM_ERR_ARG;
    return plane_copy_out(f, out, f->field, std::min(cap, f->n_states()) * 4);
}

int lom_posefield_potential_device(lom_posefield *f, const uint32_t **d_out)
{
    if (!f || !d_out) return LOM_ERR_ARG;
    *d_out = f->field.as<const uint32_t>();
    return LOM_OK;
}

int lom_posefield_layers(lom_posefield *f, uint32_t *out, size_t cap)
{
    if (!f || (cap && !out)) return LOM_ERR_ARG;
    return plane_copy_out(f, out, f->layers, std::min(cap, f->n_states()) * 4);
}

int lom_posefield_floor(lom_posefield *f, uint32_t *floor_out, uint8_t *heading_out, size_t cap)
{
    if (!f) return LOM_ERR_ARG;
    const size_t n = std::min(cap, f->n_cells());
    if (floor_out)
        if (const int rc = plane_copy_out(f, floor_out, f->floor, n * 4); rc != LOM_OK) return rc;
    if (heading_out)
        if (const int rc = plane_copy_out(f, heading_out, f->floor_heading, n); rc != LOM_OK) return rc;
    return LOM_OK;
}

int lom_posefield_floor_device(lom_posefield *f, const uint32_t **d_floor_out, const uint8_t **d_heading_out)
{
    if (!f) return LOM_ERR_ARG;
    if (d_floor_out) *d_floor_out = f->floor.as<const uint32_t>();
    if (d_heading_out) *d_heading_out = f->floor_heading.as<const uint8_t>();
    return LOM_OK;
}

int lom_posefield_paths(lom_posefield *f, const int32_t *starts, size_t n_starts, uint16_t *states_out, size_t cap, uint32_t *lengths_out)
{
    if (!f) return LOM_ERR_ARG;
    if (!posefield::paths_ok(starts, n_starts, states_out, cap))
        return fail(f, LOM_ERR_ARG, "pose field paths: at most 2^24 starts and an output of n_starts * cap states, at most 2^28");
    if (!n_starts) return LOM_OK;
    LOM_HIP(f, hipSetDevice(f->device));
    const size_t state_bytes = n_starts * cap * 6;
    int rc;
    if ((rc = ensure(f, f->path_states, std::max(state_bytes, (size_t)256))) != LOM_OK ||
        (rc = ensure(f, f->path_lengths, n_starts * 4)) != LOM_OK || (rc = ensure(f, f->points, n_starts * 12)) != LOM_OK)
        return rc;
    LOM_HIP(f, hipMemcpyAsync(f->points.p, starts, n_starts * 12, hipMemcpyHostToDevice, f->stream));
    if (state_bytes) LOM_HIP(f, hipMemsetAsync(f->path_states.p, 0, state_bytes, f->stream));
    hipLaunchKernelGGL(k_pose_trace, dim3(posefield::blocks_for(n_starts)), dim3(kPoseThreads), 0, f->stream, f->layers.as<const uint32_t>(),
                       f->field.as<const uint32_t>(), f->floor_heading.as<const uint8_t>(), f->args(), f->costs, f->points.as<const int32_t>(),
                       (uint32_t)n_starts, (uint32_t)cap, f->path_states.as<uint16_t>(), f->path_lengths.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    if (state_bytes) LOM_HIP(f, hipMemcpyAsync(states_out, f->path_states.p, state_bytes, hipMemcpyDeviceToHost, f->stream));
    if (lengths_out) LOM_HIP(f, hipMemcpyAsync(lengths_out, f->path_lengths.p, n_starts * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

int lom_posefield_query(lom_posefield *f, const float *xy, const int32_t *headings, size_t n, uint32_t *out)
{
    if (!f) return LOM_ERR_ARG;
    if ((n && (!xy || !headings)) || n > posefield::kMaxQueries)
        return fail(f, LOM_ERR_ARG, "pose field query: points and a heading for each, at most 2^30 of them");
    if (!n || !out) return LOM_OK;
    LOM_HIP(f, hipSetDevice(f->device));
    int rc;
    if ((rc = ensure(f, f->q_xy, n * 8)) != LOM_OK || (rc = ensure(f, f->q_h, n * 4)) != LOM_OK || (rc = ensure(f, f->q_out, n * 4)) != LOM_OK)
        return rc;
    LOM_HIP(f, hipMemcpyAsync(f->q_xy.p, xy, n * 8, hipMemcpyHostToDevice, f->stream));
    LOM_HIP(f, hipMemcpyAsync(f->q_h.p, headings, n * 4, hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(k_pose_query, dim3(posefield::blocks_for(n)), dim3(kPoseThreads), 0, f->stream, f->q_xy.as<const float>(),
                       f->q_h.as<const int32_t>(), (uint32_t)n, f->geo.resolution, f->geo.origin_x, f->geo.origin_y, f->args(),
                       f->field.as<const uint32_t>(), f->floor.as<const uint32_t>(), f->q_out.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    LOM_HIP(f, hipMemcpyAsync(out, f->q_out.p, n * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

int lom_posefield_stats(const lom_posefield *f, lom_posefield_solve_stats *out)
{
    if (!f || !out) return LOM_ERR_ARG;
    *out = f->stats;
    return LOM_OK;
}

}  // extern "C"
