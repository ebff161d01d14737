// Navigation field: the least total cost to reach a goal, per cell, over an int8 cost plane; paths down it and point
// queries.  Definitions: include/lidar_odometry_amd.h ("navigation field"); kernels: k_navfield.hpp; host planning (value
// ranges, the cell-cost table, goal quantisation, tile counts, launch shapes): navfield_host.cpp; DESIGN.md 7m.  The
// re-solve after a local cost change (k_navfield_resolve.hpp) keeps what a solve left and repairs it; the
// line of sight and the waypoints (k_navfield_waypoints.hpp) read what it left; the shift with a re-solve
// (k_navfield_shift.hpp) moves it into a second block and repairs it there.  A handle family of its own on
// the PlaneHandle core (plane_handle.hpp); the three forms in which a cost plane arrives -- host, device, clearance grid --
// are its PlaneSource, and every exported solve, re-solve and shift forwards to one function over it.  No
// default path launches any of this.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "clearance_host.hpp"
#include "k_navfield.hpp"
#include "k_navfield_resolve.hpp"
#include "k_navfield_shift.hpp"
#include "k_navfield_waypoints.hpp"
#include "nav_fixed_point.hpp"
#include "navfield_host.hpp"
#include "navset_host.hpp"
#include "plane_handle.hpp"

using namespace lom;

static_assert(navfield::kThreads == kNavThreads && navfield::kTile == kNavTile && navfield::kMaxCellCost == kNavMaxCellCost,
              "navfield_host.hpp and k_navfield.hpp disagree");
static_assert(navfield::kRoutesPerGroup == kNavRoutesPerGroup, "navfield_host.hpp and k_navfield_waypoints.hpp disagree");
static_assert(LOM_NAV_UNREACHED == kNavUnreached && LOM_NAV_MAX == kNavMax, "the header and k_navfield.hpp disagree");

// The field owns its stream and every buffer below.
struct lom_navfield : lom::PlaneHandle {  // in_ev: the clearance grid's
    navfield::TileGrid tiles{};
    lom::DeviceBuf field;            // u32 per cell
    lom::DeviceBuf plane;            // the cost bytes of the last solve
    lom::DeviceBuf table;            // 256 u32: the cell costs of the last solve
    lom::DeviceBuf marks;            // 3 x n_tiles u32: the tiles active in an even and in an odd launch; a re-solve's seeds
    lom::DeviceBuf flags;            // kBatchMax u32: "launch j of the batch marked a tile"
    lom::DeviceBuf words;            // the summary words, and behind them a re-solve's
    lom::DeviceBuf incoming;         // the window's rows of a re-solve's host plane, grow-only
    lom::DeviceBuf field2, plane2;   // the second block of a shift with a re-solve: empty until the first non-zero shift
    lom::DeviceBuf points;           // goals or starts as int32 pairs, grow-only
    lom::DeviceBuf path_cells, path_lengths;  // a paths call's results, grow-only
    lom::DeviceBuf q_xy, q_out;      // a query's points and results, grow-only
    lom::DeviceBuf wp_cells, wp_counts;  // a waypoints call's results, grow-only; its routes are in path_cells
    lom::PinnedBuf h_table;          // the table on its way in
    lom::PinnedBuf h_flags;          // the batch's flags and the summary words on their way out
    uint32_t inner_cap = navfield::kInnerCapDefault;  // LOM_NAV_OPT_TEST_INNER_CAP
    uint32_t batch = navfield::kBatchDefault;         // LOM_NAV_OPT_TEST_BATCH
    uint32_t all_tiles = 0;                           // LOM_NAV_OPT_TEST_ALL_TILES
    uint32_t resolve_form = 0;                        // LOM_NAV_OPT_TEST_RESOLVE_FORM
    uint32_t shortcut_serial = 0;                     // LOM_NAV_OPT_TEST_SHORTCUT_SERIAL
    lom_navfield_solve_stats stats{};
    lom_navfield_resolve_counters resolve_stats{};
    lom_navfield_shift_counters shift_stats{};
    bool solved = false;             // a solve has completed since create or clear: plane, table and P are a fixed point
    uint32_t last_words[NW_COUNT] = {};  // ... and its summary words: what a re-solve that changes nothing reports

    NavArgs args() const { return NavArgs{geo.width, geo.height, tiles.tiles_x, tiles.tiles_y}; }
};

namespace {

thread_local std::string g_navfield_create_error;

constexpr const char *kName = "navigation field";  // the head of the texts of the plane-handle core

constexpr const char *kParamsText =
    "navigation field parameters: neutral >= 1, 0 <= max_passable <= 98, neutral + 98 * factor <= 2^24 - 1, known flags, "
    "unknown_cost in 1 .. 2^24 - 1 under LOM_NAV_UNKNOWN_PASSABLE";

// every cell unreached and impassable, no tile marked
int fill(lom_navfield *f, bool plane_too)
{
    const size_t n = std::max(f->n_cells(), (size_t)2 * f->tiles.n_tiles);
    hipLaunchKernelGGL(k_nav_fill, dim3(navfield::blocks_for(n)), dim3(kNavThreads), 0, f->stream, (uint32_t)f->n_cells(),
                       2u * f->tiles.n_tiles, f->field.as<uint32_t>(), f->marks.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    if (plane_too) {
        LOM_HIP(f, hipMemsetAsync(f->plane.p, 0xFF, f->n_cells(), f->stream));
        LOM_HIP(f, hipMemsetAsync(f->table.p, 0, 256 * 4, f->stream));
    }
    return LOM_OK;
}

void summary_from(const uint32_t *t, lom_navfield_summary *s)
{
    s->cells_blocked = t[NW_BLOCKED], s->cells_reached = t[NW_REACHED], s->cells_unreached = t[NW_UNREACHED];
    s->cells_invalid = t[NW_INVALID], s->goals_used = t[NW_GOALS_USED], s->goals_rejected = t[NW_GOALS_REJECTED];
    s->range_exceeded = t[NW_RANGE], s->max_potential = t[NW_MAX_POTENTIAL];
}

// the refusals of every solve form that need no device: the text, or NULL
const char *solve_refusal(bool have_plane, const lom_navfield_params *p, int goal_kind, const void *goals, size_t n_goals)
{
    if (!have_plane) return "navigation field solve: a cost plane";
    if (!navfield::params_ok(p)) return kParamsText;
    if (goal_kind != LOM_NAV_CELLS && goal_kind != LOM_NAV_METRES) return "navigation field: goals are LOM_NAV_CELLS or LOM_NAV_METRES";
    if ((n_goals && !goals) || n_goals > navfield::kMaxPoints) return "navigation field solve: goals, at most 2^24 of them";
    return nullptr;
}

// n points of `kind` as int32 pairs in f->points, enqueued.  `cells` is the pageable staging block: the caller keeps it
// until it has waited for the stream.
int upload_points(lom_navfield *f, int kind, const void *pts, size_t n, std::vector<int32_t> &cells)
{
    if (!n) return LOM_OK;
    cells.resize(2 * n);
    navfield::quantise(f->geo, kind, pts, n, cells.data());
    if (const int rc = ensure(f, f->points, n * 8); rc != LOM_OK) return rc;
    LOM_HIP(f, hipMemcpyAsync(f->points.p, cells.data(), n * 8, hipMemcpyHostToDevice, f->stream));
    return LOM_OK;
}

// the relaxation from the marks of the first array to its fixed point
int relax(lom_navfield *f, uint64_t &launches, uint64_t &waits)
{
    const NavArgs a = f->args();
    return to_fixed_point(f, f->tiles.n_tiles, launches, waits, "navigation field: the relaxation did not settle", [&](uint32_t *cur, uint32_t *nxt, uint32_t *flag) {
        hipLaunchKernelGGL(k_nav_relax, dim3(f->tiles.tiles_x, f->tiles.tiles_y), dim3(kNavThreads), 0, f->stream, f->plane.as<const int8_t>(),
                           f->table.as<const uint32_t>(), a, f->inner_cap, f->all_tiles, f->field.as<uint32_t>(), cur, nxt, flag);
    });
}

// the summary of the field as it stands: the report, the way out of the first n_words words, done_ev, the wait.  The words
// are in h_flags.
int report(lom_navfield *f, uint32_t n_words)
{
    hipLaunchKernelGGL(k_nav_report, dim3(navfield::blocks_for(f->n_cells())), dim3(kNavThreads), 0, f->stream, f->plane.as<const int8_t>(),
                       f->table.as<const uint32_t>(), f->field.as<const uint32_t>(), f->args(), f->words.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    LOM_HIP(f, hipMemcpyAsync(f->h_flags.h, f->words.p, (size_t)n_words * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

// A solve over a plane in HBM that this stream may read now: the copy of the plane, the seed, the relaxation in batches of
// launches with one wait each, the report, then the wait.  The arguments are valid.
int solve_on_device(lom_navfield *f, const int8_t *d_plane, const lom_navfield_params &p, int goal_kind, const void *goals,
                    size_t n_goals, lom_navfield_summary *summary)
{
    // what can still fail for want of memory comes first: a refused call changes nothing
    std::vector<int32_t> goal_cells;
    if (const int rc = upload_points(f, goal_kind, goals, n_goals, goal_cells); rc != LOM_OK) return rc;
    f->solved = false;
    navfield::cell_costs(p, f->h_table.as<uint32_t>());  // (every call waits for its work: nothing enqueued reads the block)
    LOM_HIP(f, hipMemcpyAsync(f->table.p, f->h_table.h, 256 * 4, hipMemcpyHostToDevice, f->stream));
    if (d_plane != f->plane.as<const int8_t>())
        LOM_HIP(f, hipMemcpyAsync(f->plane.p, d_plane, f->n_cells(), hipMemcpyDeviceToDevice, f->stream));
    LOM_HIP(f, hipMemsetAsync(f->words.p, 0, (size_t)NW_COUNT * 4, f->stream));
    if (const int rc = fill(f, false); rc != LOM_OK) return rc;
    const NavArgs a = f->args();
    const int8_t *const plane = f->plane.as<const int8_t>();
    const uint32_t *const table = f->table.as<const uint32_t>();
    uint32_t *const marks = f->marks.as<uint32_t>();
    if (n_goals) {
        hipLaunchKernelGGL(k_nav_seed, dim3(navfield::blocks_for(n_goals)), dim3(kNavThreads), 0, f->stream, plane, table, a,
                           f->points.as<const int32_t>(), (uint32_t)n_goals, f->field.as<uint32_t>(), marks, f->words.as<uint32_t>());
        LOM_HIP(f, hipGetLastError());
    }
    f->stats = lom_navfield_solve_stats{0, 0, f->tiles.n_tiles};
    if (const int rc = relax(f, f->stats.launches, f->stats.waits); rc != LOM_OK) return rc;
    if (const int rc = report(f, NW_COUNT); rc != LOM_OK) return rc;
    std::memcpy(f->last_words, f->h_flags.h, sizeof f->last_words);
    f->solved = true;
    if (summary) summary_from(f->h_flags.as<uint32_t>(), summary);
    return LOM_OK;
}

// the refusals of every re-solve form that need no device: the code and the text, or LOM_OK
int resolve_refusal(lom_navfield *f, bool have_plane)
{
    if (!have_plane) return fail(f, LOM_ERR_ARG, "navigation field re-solve: a cost plane");
    if (!f->solved) return fail(f, LOM_ERR_STATE, "navigation field re-solve: no solve has completed since create or clear");
    return LOM_OK;
}

// The repair behind the first launch and wait of a re-solve or of a shift with one: the raise phase to its fixed point
// and its seeds as the first marks (form 0), or the reset of another form (1: the threshold, 2: the goals' tiles); the
// relaxation from the seeds to its fixed point; the report and the wait; the counters.  The report counts cells, the goals
// are the host's to keep: goals_used falls by `goals_gone`, those rejected and those that left the grid.
int repair(lom_navfield *f, uint32_t form, uint32_t goals_gone)
{
    const NavArgs a = f->args();
    const uint32_t n_tiles = f->tiles.n_tiles;
    const uint32_t *const table = f->table.as<const uint32_t>();
    uint32_t *const field = f->field.as<uint32_t>(), *const words = f->words.as<uint32_t>();
    uint32_t *const marks0 = f->marks.as<uint32_t>(), *const seeds = marks0 + (size_t)2 * n_tiles;
    uint32_t *const h = f->h_flags.as<uint32_t>();
    lom_navfield_resolve_counters &st = f->resolve_stats;
    if (form == 0u) {
        const int rc = to_fixed_point(f, f->tiles.n_tiles, st.raise_launches, st.waits, "navigation field: the raise phase did not settle",
                                      [&](uint32_t *cur, uint32_t *nxt, uint32_t *flag) {
                                          hipLaunchKernelGGL(k_nav_raise, dim3(f->tiles.tiles_x, f->tiles.tiles_y), dim3(kNavThreads), 0,
                                                             f->stream, f->plane.as<const int8_t>(), table, a, f->inner_cap, f->all_tiles,
                                                             field, cur, nxt, seeds, flag, words);
                                      });
        if (rc != LOM_OK) return rc;
        // (both arrays of the fixed point are clear: the seeds are the first launch's marks)
        LOM_HIP(f, hipMemcpyAsync(marks0, seeds, (size_t)n_tiles * 4, hipMemcpyDeviceToDevice, f->stream));
    } else if (form == 1u) {
        hipLaunchKernelGGL(k_nav_threshold, dim3(navfield::blocks_for(f->n_cells())), dim3(kNavThreads), 0, f->stream, a, field, marks0, words);
        LOM_HIP(f, hipGetLastError());
    } else {
        hipLaunchKernelGGL(k_nav_reseed, dim3(navfield::blocks_for(f->n_cells())), dim3(kNavThreads), 0, f->stream,
                           f->plane.as<const int8_t>(), table, a, field, marks0, words);
        LOM_HIP(f, hipGetLastError());
    }
    if (const int rc = relax(f, st.relax_launches, st.waits); rc != LOM_OK) return rc;
    if (const int rc = report(f, RW_END); rc != LOM_OK) return rc;
    st.waits++;
    st.cells_raised = h[RW_RAISED], st.tiles_marked = h[RW_TILES];
    h[NW_GOALS_USED] = f->last_words[NW_GOALS_USED] - goals_gone;
    std::memcpy(f->last_words, h, sizeof f->last_words);
    return LOM_OK;
}

// A re-solve from a plane in HBM that this stream may read now, over a window that is not empty: the diff and a wait;
// then, where a cell changed, the repair.  done_ev stands behind the diff, the one reader of d_new.
int resolve_on_device(lom_navfield *f, const int8_t *d_new, const clearance::Rect &r, lom_navfield_summary *summary)
{
    const NavArgs a = f->args();
    const navfield::TileRange tr = navfield::tile_range(r);
    const uint32_t n_tiles = f->tiles.n_tiles, form = f->resolve_form;
    const uint32_t *const table = f->table.as<const uint32_t>();
    uint32_t *const field = f->field.as<uint32_t>(), *const words = f->words.as<uint32_t>();
    uint32_t *const marks0 = f->marks.as<uint32_t>(), *const seeds = marks0 + (size_t)2 * n_tiles;
    uint32_t *const h = f->h_flags.as<uint32_t>();
    lom_navfield_resolve_counters &st = f->resolve_stats;
    st = lom_navfield_resolve_counters{};
    LOM_HIP(f, hipMemsetAsync(f->words.p, 0, (size_t)RW_END * 4, f->stream));
    LOM_HIP(f, hipMemsetAsync(f->marks.p, 0, (size_t)3 * n_tiles * 4, f->stream));
    // form 0: the seeds gather behind the raise phase, which starts from the diff's marks; form 1: the diff's marks are
    // seeds at once; form 2: the goals' tiles are the seeds
    hipLaunchKernelGGL(k_nav_diff, dim3(tr.n_tx, tr.n_ty), dim3(kNavThreads), 0, f->stream, d_new, table, a,
                       NavWindow{r.x0, r.y0, r.x1, r.y1, tr.tx0, tr.ty0}, form == 1u ? 1u : 0u, f->plane.as<int8_t>(), field,
                       form == 0u ? seeds : form == 1u ? marks0 : nullptr, form == 0u ? marks0 : nullptr, words);
    LOM_HIP(f, hipGetLastError());
    f->solved = false;
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    LOM_HIP(f, hipMemcpyAsync(h, f->words.p, (size_t)RW_END * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    st.waits = 1;
    st.cells_changed = h[RW_CHANGED];
    const uint32_t rejected = h[NW_GOALS_REJECTED];
    if (st.cells_changed != 0u)
        if (const int rc = repair(f, form, rejected); rc != LOM_OK) return rc;
    f->last_words[NW_GOALS_REJECTED] = rejected;
    f->solved = true;
    if (summary) summary_from(f->last_words, summary);
    return LOM_OK;
}

// the summary of a re-solve over an empty window: the field as it stands, no goal rejected
int resolve_nothing(lom_navfield *f, lom_navfield_summary *summary)
{
    f->resolve_stats = lom_navfield_resolve_counters{};
    f->last_words[NW_GOALS_REJECTED] = 0u;
    if (summary) summary_from(f->last_words, summary);
    return LOM_OK;
}

// ---- the shift with a re-solve ------------------------------------------------------------------------------------------
// the second block, at the first call that moves: 5 bytes per cell
int ensure_second_block(lom_navfield *f)
{
    if (f->field2.p && f->plane2.p) return LOM_OK;
    release(f->field2), release(f->plane2);
    if (alloc(f->field2, f->n_cells() * 4) != hipSuccess || alloc(f->plane2, f->n_cells()) != hipSuccess) {
        release(f->field2), release(f->plane2);
        return fail(f, LOM_ERR_OOM, "hipMalloc (navigation field, the second block of a shift)");
    }
    return LOM_OK;
}

// A shift that moves, from a plane in HBM that this stream may read now, in the new geometry's cells; r may be empty.  The
// mover and diff in one launch into the second block, the swap behind it, and a wait; then the repair, whatever changed
// (the threshold form runs the reset of form 2: its pmin would have to cover the trailing borders).  done_ev stands behind
// the first launch, the one reader of d_new.  Every allocation has been made.
int shift_resolve_on_device(lom_navfield *f, const navfield::ShiftPlan &plan, const lom_occupancy_geometry &g, const int8_t *d_new,
                            const clearance::Rect &r, lom_navfield_summary *summary)
{
    const NavArgs a = f->args();
    const uint32_t n_tiles = f->tiles.n_tiles;
    const bool raise = f->resolve_form == 0u;
    const uint32_t *const table = f->table.as<const uint32_t>();
    uint32_t *const words = f->words.as<uint32_t>();
    uint32_t *const marks0 = f->marks.as<uint32_t>(), *const seeds = marks0 + (size_t)2 * n_tiles;
    uint32_t *const h = f->h_flags.as<uint32_t>();
    lom_navfield_resolve_counters &st = f->resolve_stats;
    st = lom_navfield_resolve_counters{};
    LOM_HIP(f, hipMemsetAsync(f->words.p, 0, (size_t)SW_END * 4, f->stream));
    LOM_HIP(f, hipMemsetAsync(f->marks.p, 0, (size_t)3 * n_tiles * 4, f->stream));
    const clearance::Rect w = r.empty() ? clearance::Rect{0u, 0u, 0u, 0u} : r;
    const NavShift s{plan.dx, plan.dy, plan.kept.x0, plan.kept.y0, plan.kept.x1, plan.kept.y1, w.x0, w.y0, w.x1, w.y1};
    hipLaunchKernelGGL(k_nav_shift_diff, dim3(f->tiles.tiles_x, f->tiles.tiles_y), dim3(kNavThreads), 0, f->stream, d_new, table, a, s,
                       f->plane.as<const int8_t>(), f->field.as<const uint32_t>(), f->plane2.as<int8_t>(), f->field2.as<uint32_t>(),
                       raise ? seeds : nullptr, raise ? marks0 : nullptr, words);
    LOM_HIP(f, hipGetLastError());
    f->solved = false;
    swap(f->field, f->field2), swap(f->plane, f->plane2);
    f->geo = g;
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    LOM_HIP(f, hipMemcpyAsync(h, f->words.p, (size_t)SW_END * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    st.waits = 1;
    st.cells_changed = h[RW_CHANGED];
    const uint32_t rejected = h[NW_GOALS_REJECTED], left = h[SW_GOALS_LEFT];
    f->shift_stats = lom_navfield_shift_counters{plan.cells_kept, h[SW_ENTERED], left};
    if (const int rc = repair(f, raise ? 0u : 2u, rejected + left); rc != LOM_OK) return rc;
    f->last_words[NW_GOALS_REJECTED] = rejected;
    f->solved = true;
    if (summary) summary_from(f->last_words, summary);
    return LOM_OK;
}

// ---- one function per operation over the source of the plane (plane_handle.hpp) ---------------------------
// Each in one order: the refusals, the way out that needs no device, what can fail for want of memory, open, upload, body, close.
int solve_from(lom_navfield *f, const PlaneSource &src, const lom_navfield_params *params, int goal_kind, const void *goals, size_t n_goals,
               lom_navfield_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!f) return LOM_ERR_ARG;
    if (const char *why = solve_refusal(src.given(), params, goal_kind, goals, n_goals)) return fail(f, LOM_ERR_ARG, why);
    if (const int rc = plane_source_check(f, kName, src, f->geo); rc != LOM_OK) return rc;
    LOM_HIP(f, hipSetDevice(f->device));
    // the goals first: their buffer is what can still be refused (no memory); then a host plane goes straight to the field's copy
    if (const int rc = n_goals ? ensure(f, f->points, n_goals * 8) : LOM_OK; rc != LOM_OK) return rc;
    const int8_t *d_plane = nullptr;
    if (const int rc = plane_source_open(f, kName, src, &d_plane); rc != LOM_OK) return rc;
    if (src.host) {
        LOM_HIP(f, hipMemcpyAsync(f->plane.p, src.host, f->n_cells(), hipMemcpyHostToDevice, f->stream));
        d_plane = f->plane.as<const int8_t>();
    }
    if (const int rc = solve_on_device(f, d_plane, *params, goal_kind, goals, n_goals, summary); rc != LOM_OK) return rc;
    return plane_source_close(f, kName, src);
}

int resolve_from(lom_navfield *f, const PlaneSource &src, const lom_clearance_window *window_or_null, lom_navfield_summary *summary)
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

// The refusals of a re-solve, the geometry by the rule (LOM_ERR_RANGE) and the plan come before any device work.
int shift_resolve_from(lom_navfield *f, const PlaneSource &src, int32_t dx, int32_t dy, const lom_clearance_window *window_or_null,
                       lom_navfield_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!f) return LOM_ERR_ARG;
    if (const int rc = resolve_refusal(f, src.given()); rc != LOM_OK) return rc;
    lom_occupancy_geometry g;
    if (const int rc = plane_shifted_geometry(f, kName, dx, dy, &g); rc != LOM_OK) return rc;
    const navfield::ShiftPlan plan = navfield::shift_plan(f->geo.width, f->geo.height, dx, dy);
    if (!plan.moves()) {
        // A shift of (0, 0) is the re-solve with the same arguments, under the geometry the rule gives for it (an origin of
        // -0 becomes +0); a refusal puts the geometry back.
        const lom_occupancy_geometry before = f->geo;
        f->geo = g;
        if (const int rc = resolve_from(f, src, window_or_null, summary); rc != LOM_OK) {
            f->geo = before;
            return rc;
        }
        f->shift_stats = lom_navfield_shift_counters{f->n_cells(), 0u, 0u};
        return LOM_OK;
    }
    // a clearance grid has been shifted already: its geometry is the new one, bit for bit
    if (const int rc = plane_source_check(f, kName, src, g, " from the shifted geometry"); rc != LOM_OK) return rc;
    LOM_HIP(f, hipSetDevice(f->device));
    if (const int rc = ensure_second_block(f); rc != LOM_OK) return rc;
    const clearance::Rect r = clearance::clip(window_or_null, g);
    const int8_t *d_plane = nullptr;
    if (const int rc = plane_source_open(f, kName, src, &d_plane); rc != LOM_OK) return rc;
    if (src.host) {
        // the rows that hold an entered cell or a cell of the window, whole, at their place in a plane of the device
        if (const int rc = ensure(f, f->incoming, f->n_cells()); rc != LOM_OK) return rc;
        uint32_t y0, y1;
        navfield::shift_upload_rows(plan, r, g.height, &y0, &y1);
        const size_t first = (size_t)y0 * g.width, bytes = (size_t)(y1 - y0) * g.width;
        if (bytes) LOM_HIP(f, hipMemcpyAsync(f->incoming.as<int8_t>() + first, src.host + first, bytes, hipMemcpyHostToDevice, f->stream));
        d_plane = f->incoming.as<const int8_t>();
    }
    if (const int rc = shift_resolve_on_device(f, plan, g, d_plane, r, summary); rc != LOM_OK) return rc;
    return plane_source_close(f, kName, src);
}

}  // namespace

extern "C" {

int lom_navfield_create(const lom_occupancy_geometry *geometry, int device, lom_navfield **out)
{
    if (!out) return LOM_ERR_ARG;
    lom_navfield *f = nullptr;
    int rc = plane_new(geometry, device, g_navfield_create_error, kName, "navigation field setup", 1, &f);
    if (rc != LOM_OK) return rc;
    f->tiles = navfield::tile_grid(geometry->width, geometry->height);
    hipError_t e = alloc(f->h_table, 256 * 4, hipHostMallocDefault);
    if (e == hipSuccess) e = alloc(f->h_flags, (size_t)navfield::kBatchMax * 4, hipHostMallocDefault);
    if (e != hipSuccess) rc = create_fail(g_navfield_create_error, LOM_ERR_HIP, "navigation field setup", e);
    const size_t n = f->n_cells();
    if (rc == LOM_OK &&
        (alloc(f->field, n * 4) != hipSuccess || alloc(f->plane, n) != hipSuccess || alloc(f->table, 256 * 4) != hipSuccess ||
         alloc(f->marks, (size_t)3 * f->tiles.n_tiles * 4) != hipSuccess ||
         alloc(f->flags, (size_t)navfield::kBatchMax * 4) != hipSuccess || alloc(f->words, 64) != hipSuccess))
        rc = create_fail(g_navfield_create_error, LOM_ERR_OOM, "hipMalloc (navigation field)");
    if (rc == LOM_OK) {
        if (fill(f, true) != LOM_OK || (e = hipStreamSynchronize(f->stream)) != hipSuccess)
            rc = create_fail(g_navfield_create_error, LOM_ERR_HIP, f->error.empty() ? "navigation field setup" : f->error.c_str(), e);
    }
    if (rc != LOM_OK) {
        lom_navfield_destroy(f);
        return rc;
    }
    *out = f;
    return LOM_OK;
}

void lom_navfield_destroy(lom_navfield *f) { plane_destroy(f); }
const char *lom_navfield_last_error(const lom_navfield *f) { return plane_last_error(f, g_navfield_create_error); }

int lom_navfield_clear(lom_navfield *f)
{
    if (!f) return LOM_ERR_ARG;
    LOM_HIP(f, hipSetDevice(f->device));
    f->solved = false;
    if (const int rc = fill(f, true); rc != LOM_OK) return rc;
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

int lom_navfield_shift(lom_navfield *f, int32_t dx, int32_t dy) { return plane_shift(f, "navigation field", dx, dy, &lom_navfield_clear); }
int lom_navfield_get_geometry(const lom_navfield *f, lom_occupancy_geometry *out) { return plane_get_geometry(f, out); }
void *lom_navfield_stream(lom_navfield *f) { return plane_stream(f); }
int lom_navfield_device(const lom_navfield *f) { return plane_device(f); }
int lom_navfield_wait_event(lom_navfield *f, void *hip_event) { return plane_wait_event(f, hip_event); }

int lom_navfield_set_option(lom_navfield *f, int option, int64_t value)
{
    if (!f) return LOM_ERR_ARG;
    switch (option) {
    case LOM_NAV_OPT_TEST_INNER_CAP:
        return set_test_option(f, f->inner_cap, value, navfield::kInnerCapMax, navfield::kInnerCapDefault,
                               "LOM_NAV_OPT_TEST_INNER_CAP: 1 .. 2^20, or <= 0 for the default");
    case LOM_NAV_OPT_TEST_BATCH:
        return set_test_option(f, f->batch, value, navfield::kBatchMax, navfield::kBatchDefault,
                               "LOM_NAV_OPT_TEST_BATCH: 1 .. 256, or <= 0 for the default");
    case LOM_NAV_OPT_TEST_ALL_TILES: return set_test_option(f, f->all_tiles, value, 1, 0, "LOM_NAV_OPT_TEST_ALL_TILES: 0, 1, or < 0 for the default");
    case LOM_NAV_OPT_TEST_RESOLVE_FORM:
        return set_test_option(f, f->resolve_form, value, 2, 0, "LOM_NAV_OPT_TEST_RESOLVE_FORM: 0, 1, 2, or < 0 for the default");
    case LOM_NAV_OPT_TEST_SHORTCUT_SERIAL:
        return set_test_option(f, f->shortcut_serial, value, 1, 0, "LOM_NAV_OPT_TEST_SHORTCUT_SERIAL: 0, 1, or < 0 for the default");
    default:
        return fail(f, LOM_ERR_ARG, "unknown navigation field option");
    }
}

int lom_navfield_solve(lom_navfield *f, const int8_t *plane, const lom_navfield_params *params, int goal_kind, const void *goals,
                       size_t n_goals, lom_navfield_summary *summary)
{
    return solve_from(f, plane_from_host(plane), params, goal_kind, goals, n_goals, summary);
}

int lom_navfield_solve_device(lom_navfield *f, const int8_t *d_plane, void *hip_event_or_null, const lom_navfield_params *params,
                              int goal_kind, const void *goals, size_t n_goals, lom_navfield_summary *summary)
{
    return solve_from(f, plane_from_device(d_plane, hip_event_or_null), params, goal_kind, goals, n_goals, summary);
}

int lom_navfield_solve_from_clearance(lom_navfield *f, lom_clearance *clearance, const lom_navfield_params *params, int goal_kind,
                                      const void *goals, size_t n_goals, lom_navfield_summary *summary)
{
    return solve_from(f, plane_from_clearance(clearance), params, goal_kind, goals, n_goals, summary);
}

int lom_navfield_resolve(lom_navfield *f, const int8_t *plane, const lom_clearance_window *window_or_null, lom_navfield_summary *summary)
{
    return resolve_from(f, plane_from_host(plane), window_or_null, summary);
}

int lom_navfield_resolve_device(lom_navfield *f, const int8_t *d_plane, void *hip_event_or_null, const lom_clearance_window *window_or_null,
                                lom_navfield_summary *summary)
{
    return resolve_from(f, plane_from_device(d_plane, hip_event_or_null), window_or_null, summary);
}

int lom_navfield_resolve_from_clearance(lom_navfield *f, lom_clearance *clearance, const lom_clearance_window *window_or_null,
                                        lom_navfield_summary *summary)
{
    return resolve_from(f, plane_from_clearance(clearance), window_or_null, summary);
}

int lom_navfield_shift_resolve(lom_navfield *f, int32_t dx, int32_t dy, const int8_t *plane, const lom_clearance_window *window_or_null,
                               lom_navfield_summary *summary)
{
    return shift_resolve_from(f, plane_from_host(plane), dx, dy, window_or_null, summary);
}

int lom_navfield_shift_resolve_device(lom_navfield *f, int32_t dx, int32_t dy, const int8_t *d_plane, void *hip_event_or_null,
                                      const lom_clearance_window *window_or_null, lom_navfield_summary *summary)
{
    return shift_resolve_from(f, plane_from_device(d_plane, hip_event_or_null), dx, dy, window_or_null, summary);
}

int lom_navfield_shift_resolve_from_clearance(lom_navfield *f, int32_t dx, int32_t dy, lom_clearance *clearance,
                                              const lom_clearance_window *window_or_null, lom_navfield_summary *summary)
{
    return shift_resolve_from(f, plane_from_clearance(clearance), dx, dy, window_or_null, summary);
}

int lom_navfield_potential(lom_navfield *f, uint32_t *out, size_t cap)
{
    if (!f || (cap && !out)) return LOM_ERR_ARG;
    return plane_copy_out(f, out, f->field, std::min(cap, f->n_cells()) * 4);
}

int lom_navfield_potential_device(lom_navfield *f, const uint32_t **d_out)
{
    if (!f || !d_out) return LOM_ERR_ARG;
    *d_out = f->field.as<const uint32_t>();
    return LOM_OK;
}

int lom_navfield_paths(lom_navfield *f, int start_kind, const void *starts, size_t n_starts, uint16_t *cells_out, size_t cap,
                       uint32_t *lengths_out)
{
    if (!f) return LOM_ERR_ARG;
    if (start_kind != LOM_NAV_CELLS && start_kind != LOM_NAV_METRES) return fail(f, LOM_ERR_ARG, "navigation field: starts are LOM_NAV_CELLS or LOM_NAV_METRES");
    if ((n_starts && !starts) || n_starts > navfield::kMaxPoints) return fail(f, LOM_ERR_ARG, "navigation field paths: starts, at most 2^24 of them");
    if (cap > navfield::kMaxPathCells || (cap && n_starts > navfield::kMaxPathCells / cap) || (n_starts && cap && !cells_out))
        return fail(f, LOM_ERR_ARG, "navigation field paths: an output of n_starts * cap cells, at most 2^28");
    if (!n_starts) return LOM_OK;
    LOM_HIP(f, hipSetDevice(f->device));
    const size_t cell_bytes = n_starts * cap * 4;
    int rc;
    if ((rc = ensure(f, f->path_cells, std::max(cell_bytes, (size_t)256))) != LOM_OK || (rc = ensure(f, f->path_lengths, n_starts * 4)) != LOM_OK)
        return rc;
    std::vector<int32_t> start_cells;
    if ((rc = upload_points(f, start_kind, starts, n_starts, start_cells)) != LOM_OK) return rc;
    if (cell_bytes) LOM_HIP(f, hipMemsetAsync(f->path_cells.p, 0, cell_bytes, f->stream));
    hipLaunchKernelGGL(k_nav_trace, dim3(navfield::blocks_for(n_starts)), dim3(kNavThreads), 0, f->stream, f->plane.as<const int8_t>(),
                       f->table.as<const uint32_t>(), f->field.as<const uint32_t>(), f->args(), f->points.as<const int32_t>(),
                       (uint32_t)n_starts, (uint32_t)cap, f->path_cells.as<uint16_t>(), f->path_lengths.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    if (cell_bytes) LOM_HIP(f, hipMemcpyAsync(cells_out, f->path_cells.p, cell_bytes, hipMemcpyDeviceToHost, f->stream));
    if (lengths_out) LOM_HIP(f, hipMemcpyAsync(lengths_out, f->path_lengths.p, n_starts * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

int lom_navfield_query(lom_navfield *f, const float *xy, size_t n, uint32_t *out)
{
    if (!f) return LOM_ERR_ARG;
    if ((n && !xy) || n > (size_t)1 << 30) return fail(f, LOM_ERR_ARG, "navigation field query: points, at most 2^30 of them");
    if (!n || !out) return LOM_OK;
    LOM_HIP(f, hipSetDevice(f->device));
    int rc;
    if ((rc = ensure(f, f->q_xy, n * 8)) != LOM_OK || (rc = ensure(f, f->q_out, n * 4)) != LOM_OK) return rc;
    LOM_HIP(f, hipMemcpyAsync(f->q_xy.p, xy, n * 8, hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(k_nav_query, dim3(navfield::blocks_for(n)), dim3(kNavThreads), 0, f->stream, f->q_xy.as<const float>(), (uint32_t)n,
                       f->geo.resolution, f->geo.origin_x, f->geo.origin_y, f->args(), f->field.as<const uint32_t>(), f->q_out.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    LOM_HIP(f, hipMemcpyAsync(out, f->q_out.p, n * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

int lom_navfield_visible(lom_navfield *f, const int32_t *pairs, size_t n, uint32_t max_cell_cost, uint8_t *out)
{
    if (!f) return LOM_ERR_ARG;
    if ((n && (!pairs || !out)) || n > navfield::kMaxVisiblePairs)
        return fail(f, LOM_ERR_ARG, "navigation field visible: pairs and a byte for each, at most 2^24 of them");
    if (!n) return LOM_OK;
    LOM_HIP(f, hipSetDevice(f->device));
    int rc;
    if ((rc = ensure(f, f->q_xy, n * 16)) != LOM_OK || (rc = ensure(f, f->q_out, n)) != LOM_OK) return rc;
    LOM_HIP(f, hipMemcpyAsync(f->q_xy.p, pairs, n * 16, hipMemcpyHostToDevice, f->stream));
    hipLaunchKernelGGL(k_nav_visible, dim3(navfield::blocks_for(n)), dim3(kNavThreads), 0, f->stream, f->plane.as<const int8_t>(),
                       f->table.as<const uint32_t>(), f->args(), f->q_xy.as<const int32_t>(), (uint32_t)n, max_cell_cost, f->q_out.as<uint8_t>());
    LOM_HIP(f, hipGetLastError());
    LOM_HIP(f, hipMemcpyAsync(out, f->q_out.p, n, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

// (Aligned to a cache line, which makes the library's .text start on one: what is linked in front of navfield.o then keeps
// its place within cache lines when the tables in front of .text grow by an export; profiles/navfield_waypoints_ab.txt.)
__attribute__((aligned(64))) int lom_navfield_waypoints(lom_navfield *f, int start_kind, const void *starts, size_t n_starts,
                                                        const lom_navfield_waypoint_params *params, uint16_t *cells_out, size_t wp_cap,
                                                        uint32_t *counts_out, uint32_t *lengths_out)
{
    if (!f) return LOM_ERR_ARG;
    if (start_kind != LOM_NAV_CELLS && start_kind != LOM_NAV_METRES) return fail(f, LOM_ERR_ARG, "navigation field: starts are LOM_NAV_CELLS or LOM_NAV_METRES");
    if ((n_starts && !starts) || n_starts > navfield::kMaxPoints) return fail(f, LOM_ERR_ARG, "navigation field waypoints: starts, at most 2^24 of them");
    if (!navfield::waypoint_params_ok(params, n_starts))
        return fail(f, LOM_ERR_ARG, "navigation field waypoints: lookahead in 1 .. 65535, route_cap >= 1, n_starts * route_cap <= 2^28, flags 0");
    if (!navfield::waypoint_output_ok(n_starts, wp_cap, cells_out))
        return fail(f, LOM_ERR_ARG, "navigation field waypoints: an output of n_starts * wp_cap cells, at most 2^28");
    if (!n_starts) return LOM_OK;
    LOM_HIP(f, hipSetDevice(f->device));
    const uint32_t K = (uint32_t)n_starts, route_cap = params->route_cap;
    const size_t out_bytes = n_starts * wp_cap * 4;
    int rc;
    if ((rc = ensure(f, f->path_cells, std::max(n_starts * route_cap * 4, (size_t)256))) != LOM_OK ||
        (rc = ensure(f, f->path_lengths, n_starts * 4)) != LOM_OK || (rc = ensure(f, f->wp_cells, std::max(out_bytes, (size_t)256))) != LOM_OK ||
        (rc = ensure(f, f->wp_counts, n_starts * 4)) != LOM_OK)
        return rc;
    std::vector<int32_t> start_cells;
    if ((rc = upload_points(f, start_kind, starts, n_starts, start_cells)) != LOM_OK) return rc;
    if (out_bytes) LOM_HIP(f, hipMemsetAsync(f->wp_cells.p, 0, out_bytes, f->stream));
    // the routes stay in the handle's path buffer: only the first min(length, route_cap) cells of a row are read
    hipLaunchKernelGGL(k_nav_trace, dim3(navfield::blocks_for(n_starts)), dim3(kNavThreads), 0, f->stream, f->plane.as<const int8_t>(),
                       f->table.as<const uint32_t>(), f->field.as<const uint32_t>(), f->args(), f->points.as<const int32_t>(), K, route_cap,
                       f->path_cells.as<uint16_t>(), f->path_lengths.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    if (f->shortcut_serial)
        hipLaunchKernelGGL(k_nav_shortcut_serial, dim3(navfield::blocks_for(n_starts)), dim3(kNavThreads), 0, f->stream,
                           f->plane.as<const int8_t>(), f->table.as<const uint32_t>(), f->args(), f->path_cells.as<const uint16_t>(),
                           f->path_lengths.as<const uint32_t>(), K, route_cap, params->lookahead, params->max_cell_cost,
                           f->wp_cells.as<uint16_t>(), (uint32_t)wp_cap, f->wp_counts.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_nav_shortcut, dim3(navfield::shortcut_blocks_for(n_starts)), dim3(kNavThreads), 0, f->stream,
                           f->plane.as<const int8_t>(), f->table.as<const uint32_t>(), f->args(), f->path_cells.as<const uint32_t>(),
                           f->path_lengths.as<const uint32_t>(), K, route_cap, params->lookahead, params->max_cell_cost,
                           f->wp_cells.as<uint32_t>(), (uint32_t)wp_cap, f->wp_counts.as<uint32_t>());
    LOM_HIP(f, hipGetLastError());
    if (out_bytes) LOM_HIP(f, hipMemcpyAsync(cells_out, f->wp_cells.p, out_bytes, hipMemcpyDeviceToHost, f->stream));
    if (counts_out) LOM_HIP(f, hipMemcpyAsync(counts_out, f->wp_counts.p, n_starts * 4, hipMemcpyDeviceToHost, f->stream));
    if (lengths_out) LOM_HIP(f, hipMemcpyAsync(lengths_out, f->path_lengths.p, n_starts * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

int lom_navfield_cell_costs(const lom_navfield_params *params, uint32_t *out256)
{
    if (!navfield::params_ok(params) || !out256) return LOM_ERR_ARG;
    navfield::cell_costs(*params, out256);
    return LOM_OK;
}

int lom_navfield_stats(const lom_navfield *f, lom_navfield_solve_stats *out)
{
    if (!f || !out) return LOM_ERR_ARG;
    *out = f->stats;
    return LOM_OK;
}

int lom_navfield_resolve_stats(const lom_navfield *f, lom_navfield_resolve_counters *out)
{
    if (!f || !out) return LOM_ERR_ARG;
    *out = f->resolve_stats;
    return LOM_OK;
}

int lom_navfield_shift_stats(const lom_navfield *f, lom_navfield_shift_counters *out)
{
    if (!f || !out) return LOM_ERR_ARG;
    *out = f->shift_stats;
    return LOM_OK;
}

// Field i of a set becomes this field: what lom_navfield_solve of the set's plane, parameters and field i's goals leaves.
// Three copies within HBM behind the set's stream, released to it behind done_ev; the marks are clear after any solve.
int lom_navfield_adopt(lom_navfield *f, lom_navset *set, size_t i, lom_navfield_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!f) return LOM_ERR_ARG;
    if (!set) return fail(f, LOM_ERR_ARG, "navigation field adopt: a navigation field set");
    lom_occupancy_geometry g{};
    (void)lom_navset_get_geometry(set, &g);
    int rc = plane_check_producer(f, kName, "navigation field set", g, lom_navset_device(set));
    if (rc != LOM_OK) return rc;
    NavSetView v{};
    if ((rc = navset_view(set, i, &v)) != LOM_OK) return fail(f, rc, lom_navset_last_error(set));
    LOM_HIP(f, hipSetDevice(f->device));
    if ((rc = plane_read_behind(f, 0, v.stream)) != LOM_OK) return rc;
    f->solved = false;
    LOM_HIP(f, hipMemcpyAsync(f->field.p, v.field, f->n_cells() * 4, hipMemcpyDeviceToDevice, f->stream));
    LOM_HIP(f, hipMemcpyAsync(f->plane.p, v.plane, f->n_cells(), hipMemcpyDeviceToDevice, f->stream));
    LOM_HIP(f, hipMemcpyAsync(f->table.p, v.table, 256 * 4, hipMemcpyDeviceToDevice, f->stream));
    LOM_HIP(f, hipMemsetAsync(f->marks.p, 0, (size_t)2 * f->tiles.n_tiles * 4, f->stream));
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    const lom_navfield_summary &m = v.summary;
    const uint64_t words[NW_COUNT] = {m.cells_blocked, m.cells_reached, m.cells_unreached, m.cells_invalid, m.goals_used, m.goals_rejected,
                                      m.range_exceeded, m.max_potential};  // in the order of the NW_ words
    for (uint32_t k = 0; k < NW_COUNT; k++) f->last_words[k] = (uint32_t)words[k];
    f->stats = lom_navfield_solve_stats{0, 0, f->tiles.n_tiles};
    f->solved = true;
    if (summary) *summary = m;
    return plane_release(f, kName, set, lom_navset_wait_event, "lom_navset_wait_event");
}

}  // extern "C"
