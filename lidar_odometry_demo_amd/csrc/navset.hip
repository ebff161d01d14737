// Navigation field set: N navigation fields over one cost plane, solved side by side in one call; the travel-cost matrix,
// the nearest-goal partition and paths over them.  Definitions: include/lidar_odometry_amd.h ("navigation field set");
// kernels: k_navset.hpp (the tile body, the walk and the step rules are k_navfield.hpp's); host planning (the offsets
// rule, sizes, launch shapes): navset_host.cpp; DESIGN.md 7t.  A handle family of its own on the PlaneHandle core
// (plane_handle.hpp), the three forms of the cost plane through its PlaneSource; no default path launches
// any of this.  lom_navfield_adopt (navfield.hip) makes a field of the set a lom_navfield, so the set needs no copy of that
// family's consumers.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "k_navset.hpp"
#include "nav_fixed_point.hpp"
#include "navfield_host.hpp"
#include "navset_host.hpp"
#include "plane_handle.hpp"

using namespace lom;

static_assert(navset::kReportGroups == kNavSetReportGroups && navset::kNearestGroups == kNavSetNearestGroups &&
                  navset::kFieldWords == NSW_FIELD_COUNT && navset::kPlaneWords == NSP_COUNT,
              "navset_host.hpp and k_navset.hpp disagree");
static_assert(NSW_REACHED == 0 && NSW_MAX_POTENTIAL == 1 && NSW_RANGE == 2 && NSW_GOALS_USED == 3 && NSW_GOALS_REJECTED == 4 &&
                  NSP_BLOCKED == 0 && NSP_INVALID == 1,
              "navset::summary_of reads the words in this order");
static_assert(LOM_NAVSET_NO_OWNER == kNavSetNoOwner && LOM_NAVSET_MAX_FIELDS == navset::kMaxFields, "the header and k_navset.hpp disagree");

// The set owns its stream and every buffer below.
struct lom_navset : lom::PlaneHandle {  // in_ev: the clearance grid's
    navfield::TileGrid tiles{};
    uint32_t max_fields = 0;
    uint32_t n_fields = 0;           // of the last solve; 0 after create, clear or shift
    bool solved = false;             // a solve has completed since create, clear or shift
    lom::DeviceBuf fields;           // [max_fields][height][width] u32
    lom::DeviceBuf plane;            // the cost bytes of the last solve
    lom::DeviceBuf table;            // 256 u32: the cell costs of the last solve
    lom::DeviceBuf marks;            // [2][n_fields][n_tiles] u32 of a solve: the tiles active in an even and in an odd launch
    lom::DeviceBuf flags;            // kBatchMax u32: "launch j of the batch marked a tile of some field"
    lom::DeviceBuf words;            // [max_fields][NSW_FIELD_COUNT] u32 and the plane's NSP_COUNT behind them
    lom::DeviceBuf points, field_of; // goals, starts or points as int32 pairs and a field index each, grow-only
    lom::DeviceBuf out_a, out_b, out_c;  // the results of gather, nearest and paths on their way out, grow-only
    lom::PinnedBuf h_table;          // the table on its way in
    lom::PinnedBuf h_flags;          // the batch's flags on their way out
    lom::PinnedBuf h_words;          // the words on their way out
    std::vector<lom_navfield_summary> summaries;  // of the last solve, per field
    uint32_t inner_cap = navfield::kInnerCapDefault;  // LOM_NAVSET_OPT_TEST_INNER_CAP
    uint32_t batch = navfield::kBatchDefault;         // LOM_NAVSET_OPT_TEST_BATCH
    uint32_t all_tiles = 0;                           // LOM_NAVSET_OPT_TEST_ALL_TILES
    lom_navset_solve_stats stats{};

    NavArgs args() const { return NavArgs{geo.width, geo.height, tiles.tiles_x, tiles.tiles_y}; }
    uint32_t *plane_words() const { return words.as<uint32_t>() + (size_t)max_fields * NSW_FIELD_COUNT; }
};

namespace {

thread_local std::string g_navset_create_error;

constexpr const char *kName = "navigation field set";  // the head of the texts of the plane-handle core

constexpr const char *kParamsText =
    "navigation field set parameters: neutral >= 1, 0 <= max_passable <= 98, neutral + 98 * factor <= 2^24 - 1, known flags, "
    "unknown_cost in 1 .. 2^24 - 1 under LOM_NAV_UNKNOWN_PASSABLE";

void zero(lom_navfield_summary *summaries, size_t n)
{
    if (summaries && n) std::memset(summaries, 0, n * sizeof *summaries);
}

// the refusals of every solve form that need no device: the text, or NULL; *n_goals by the offsets
const char *solve_refusal(const lom_navset *s, bool have_plane, const lom_navfield_params *p, int goal_kind, const void *goals,
                          const uint32_t *goal_offsets, size_t n_fields, size_t *n_goals)
{
    *n_goals = 0;
    if (!have_plane) return "navigation field set solve: a cost plane";
    if (!navfield::params_ok(p)) return kParamsText;
    if (goal_kind != LOM_NAV_CELLS && goal_kind != LOM_NAV_METRES) return "navigation field set: goals are LOM_NAV_CELLS or LOM_NAV_METRES";
    return navset::offsets_refusal(goal_offsets, n_fields, s->max_fields, goals, n_goals);
}

// n points of `kind` as int32 pairs in s->points, enqueued.  `cells` is the pageable staging block: the caller keeps it
// until it has waited for the stream.
int upload_points(lom_navset *s, int kind, const void *pts, size_t n, std::vector<int32_t> &cells)
{
    if (!n) return LOM_OK;
    cells.resize(2 * n);
    navfield::quantise(s->geo, kind, pts, n, cells.data());
    if (const int rc = ensure(s, s->points, n * 8); rc != LOM_OK) return rc;
    LOM_HIP(s, hipMemcpyAsync(s->points.p, cells.data(), n * 8, hipMemcpyHostToDevice, s->stream));
    return LOM_OK;
}

// A solve over a plane in HBM that this stream may read now: the copy of the plane, one seed launch for all goals, the
// relaxation of every field in batches of launches with one wait each, the plane's counts and the report, then the wait.
// The arguments are valid and there is at least one field.
int solve_on_device(lom_navset *s, const int8_t *d_plane, const lom_navfield_params &p, int goal_kind, const void *goals,
                    const uint32_t *goal_offsets, size_t n_goals, uint32_t n_fields, lom_navfield_summary *summaries)
{
    // what can still fail for want of memory comes first: a refused call changes nothing
    std::vector<int32_t> goal_cells;
    std::vector<uint32_t> goal_fields(n_goals);
    if (const int rc = n_goals ? ensure(s, s->field_of, n_goals * 4) : LOM_OK; rc != LOM_OK) return rc;
    if (const int rc = upload_points(s, goal_kind, goals, n_goals, goal_cells); rc != LOM_OK) return rc;
    s->solved = false, s->n_fields = 0;
    const size_t n_cells = s->n_cells(), n_tiles = s->tiles.n_tiles;
    if (n_goals) {
        navset::field_of_goals(goal_offsets, n_fields, goal_fields.data());
        LOM_HIP(s, hipMemcpyAsync(s->field_of.p, goal_fields.data(), n_goals * 4, hipMemcpyHostToDevice, s->stream));
    }
    navfield::cell_costs(p, s->h_table.as<uint32_t>());  // (every call waits for its work: nothing enqueued reads the block)
    LOM_HIP(s, hipMemcpyAsync(s->table.p, s->h_table.h, 256 * 4, hipMemcpyHostToDevice, s->stream));
    if (d_plane != s->plane.as<const int8_t>()) LOM_HIP(s, hipMemcpyAsync(s->plane.p, d_plane, n_cells, hipMemcpyDeviceToDevice, s->stream));
    // every cell of every field unreached (0xFFFFFFFF), no tile marked, the words zero
    LOM_HIP(s, hipMemsetAsync(s->fields.p, 0xFF, (size_t)n_fields * n_cells * 4, s->stream));
    LOM_HIP(s, hipMemsetAsync(s->marks.p, 0, (size_t)2 * n_fields * n_tiles * 4, s->stream));
    LOM_HIP(s, hipMemsetAsync(s->words.p, 0, s->words.bytes, s->stream));
    const NavArgs a = s->args();
    const int8_t *const plane = s->plane.as<const int8_t>();
    const uint32_t *const table = s->table.as<const uint32_t>();
    uint32_t *const fields = s->fields.as<uint32_t>();
    if (n_goals) {
        hipLaunchKernelGGL(k_navset_seed, dim3(navfield::blocks_for(n_goals)), dim3(kNavThreads), 0, s->stream, plane, table, a,
                           s->points.as<const int32_t>(), s->field_of.as<const uint32_t>(), (uint32_t)n_goals, (uint32_t)n_tiles, fields,
                           s->marks.as<uint32_t>(), s->words.as<uint32_t>());
        LOM_HIP(s, hipGetLastError());
    }
    const navset::RelaxGrid g = navset::relax_grid(s->geo.width, s->geo.height, n_fields);
    s->stats = lom_navset_solve_stats{0, 0, g.groups(), n_fields};
    int rc = to_fixed_point(s, (size_t)n_fields * n_tiles, s->stats.launches, s->stats.waits, "navigation field set: the relaxation did not settle",
                            [&](uint32_t *cur, uint32_t *nxt, uint32_t *flag) {
                                hipLaunchKernelGGL(k_navset_relax, dim3(g.x, g.y, g.z), dim3(kNavThreads), 0, s->stream, plane, table, a,
                                                   s->inner_cap, s->all_tiles, (uint32_t)n_tiles, fields, cur, nxt, flag);
                            });
    if (rc != LOM_OK) return rc;
    const uint32_t groups = navset::report_groups(n_cells);
    hipLaunchKernelGGL(k_navset_plane_count, dim3(groups), dim3(kNavThreads), 0, s->stream, plane, table, (uint32_t)n_cells, s->plane_words());
    LOM_HIP(s, hipGetLastError());
    hipLaunchKernelGGL(k_navset_report, dim3(groups, n_fields), dim3(kNavThreads), 0, s->stream, plane, table, (const uint32_t *)fields, a,
                       s->words.as<uint32_t>());
    LOM_HIP(s, hipGetLastError());
    uint32_t *const h = s->h_words.as<uint32_t>(), *const h_plane = h + (size_t)n_fields * NSW_FIELD_COUNT;
    LOM_HIP(s, hipMemcpyAsync(h, s->words.p, (size_t)n_fields * NSW_FIELD_COUNT * 4, hipMemcpyDeviceToHost, s->stream));
    LOM_HIP(s, hipMemcpyAsync(h_plane, s->plane_words(), NSP_COUNT * 4, hipMemcpyDeviceToHost, s->stream));
    LOM_HIP(s, hipEventRecord(s->done_ev, s->stream));
    LOM_HIP(s, hipStreamSynchronize(s->stream));
    s->summaries.resize(n_fields);
    for (uint32_t i = 0; i < n_fields; i++) navset::summary_of(h + (size_t)i * NSW_FIELD_COUNT, h_plane, n_cells, &s->summaries[i]);
    if (summaries) std::memcpy(summaries, s->summaries.data(), n_fields * sizeof *summaries);
    s->n_fields = n_fields, s->solved = true;
    return LOM_OK;
}

// a solve of no fields: a set of no fields, nothing launched
int solve_nothing(lom_navset *s)
{
    s->n_fields = 0, s->solved = true;
    s->summaries.clear();
    s->stats = lom_navset_solve_stats{};
    return LOM_OK;
}

// The solve over the source of the plane (plane_handle.hpp), in one order: the refusals, the solve of no
// fields, what can fail for want of memory, open, upload, body, close.
int solve_from(lom_navset *s, const PlaneSource &src, const lom_navfield_params *params, int goal_kind, const void *goals,
               const uint32_t *goal_offsets, size_t n_fields, lom_navfield_summary *summaries)
{
    if (!s) return LOM_ERR_ARG;
    zero(summaries, std::min<size_t>(n_fields, s->max_fields));
    size_t n_goals;
    if (const char *why = solve_refusal(s, src.given(), params, goal_kind, goals, goal_offsets, n_fields, &n_goals)) return fail(s, LOM_ERR_ARG, why);
    if (const int rc = plane_source_check(s, kName, src, s->geo); rc != LOM_OK) return rc;
    if (!n_fields) return solve_nothing(s);
    LOM_HIP(s, hipSetDevice(s->device));
    // the goals first: their buffers are what can still be refused (no memory); then a host plane goes straight to the set's copy
    int rc;
    if (n_goals && ((rc = ensure(s, s->points, n_goals * 8)) != LOM_OK || (rc = ensure(s, s->field_of, n_goals * 4)) != LOM_OK)) return rc;
    const int8_t *d_plane = nullptr;
    if ((rc = plane_source_open(s, kName, src, &d_plane)) != LOM_OK) return rc;
    if (src.host) {
        s->solved = false, s->n_fields = 0;
        LOM_HIP(s, hipMemcpyAsync(s->plane.p, src.host, s->n_cells(), hipMemcpyHostToDevice, s->stream));
        d_plane = s->plane.as<const int8_t>();
    }
    if ((rc = solve_on_device(s, d_plane, *params, goal_kind, goals, goal_offsets, n_goals, (uint32_t)n_fields, summaries)) != LOM_OK) return rc;
    return plane_source_close(s, kName, src);
}

}  // namespace

namespace lom {

int navset_view(lom_navset *s, size_t i, NavSetView *out)
{
    if (!s->solved) return fail(s, LOM_ERR_STATE, "navigation field set: no solve has completed since create, clear or shift");
    if (i >= s->n_fields) return fail(s, LOM_ERR_ARG, "navigation field set: a field index in 0 .. field_count - 1");
    out->device = s->device, out->geo = s->geo;
    out->plane = s->plane.p, out->table = s->table.p, out->field = s->fields.as<uint32_t>() + i * s->n_cells();
    out->summary = s->summaries[i];
    out->stream = s->stream;
    return LOM_OK;
}

}  // namespace lom

extern "C" {

int lom_navset_create(const lom_occupancy_geometry *geometry, int device, size_t max_fields, lom_navset **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if (!navset::max_fields_ok(max_fields)) return create_fail(g_navset_create_error, LOM_ERR_ARG, "navigation field set: max_fields is 1 .. 65535");
    lom_navset *s = nullptr;
    int rc = plane_new(geometry, device, g_navset_create_error, kName, "navigation field set setup", 1, &s);
    if (rc != LOM_OK) return rc;
    s->tiles = navfield::tile_grid(geometry->width, geometry->height);
    s->max_fields = (uint32_t)max_fields;
    const navset::Sizes z = navset::sizes(geometry->width, geometry->height, s->max_fields);
    // the blocks in HBM first: the large one is what fails
    if (alloc(s->fields, (size_t)z.fields) != hipSuccess || alloc(s->plane, (size_t)z.plane) != hipSuccess ||
        alloc(s->table, 256 * 4) != hipSuccess || alloc(s->marks, (size_t)z.marks) != hipSuccess ||
        alloc(s->flags, (size_t)navfield::kBatchMax * 4) != hipSuccess || alloc(s->words, (size_t)z.words) != hipSuccess)
        rc = create_fail(g_navset_create_error, LOM_ERR_OOM, "hipMalloc (navigation field set)");
    if (rc == LOM_OK) {
        hipError_t e = alloc(s->h_table, 256 * 4, hipHostMallocDefault);
        if (e == hipSuccess) e = alloc(s->h_flags, (size_t)navfield::kBatchMax * 4, hipHostMallocDefault);
        if (e == hipSuccess) e = alloc(s->h_words, (size_t)z.words, hipHostMallocDefault);
        if (e != hipSuccess) rc = create_fail(g_navset_create_error, LOM_ERR_HIP, "navigation field set setup", e);
    }
    if (rc == LOM_OK && lom_navset_clear(s) != LOM_OK) rc = create_fail(g_navset_create_error, LOM_ERR_HIP, s->error.c_str());
    if (rc != LOM_OK) {
        lom_navset_destroy(s);
        return rc;
    }
    *out = s;
    return LOM_OK;
}

void lom_navset_destroy(lom_navset *s) { plane_destroy(s); }
const char *lom_navset_last_error(const lom_navset *s) { return plane_last_error(s, g_navset_create_error); }

// no field, every cell of the kept plane impassable (nothing reads either until the next solve)
int lom_navset_clear(lom_navset *s)
{
    if (!s) return LOM_ERR_ARG;
    LOM_HIP(s, hipSetDevice(s->device));
    s->solved = false, s->n_fields = 0;
    s->summaries.clear();
    s->stats = lom_navset_solve_stats{};
    LOM_HIP(s, hipMemsetAsync(s->plane.p, 0xFF, s->n_cells(), s->stream));
    LOM_HIP(s, hipMemsetAsync(s->table.p, 0, 256 * 4, s->stream));
    LOM_HIP(s, hipStreamSynchronize(s->stream));
    return LOM_OK;
}

int lom_navset_shift(lom_navset *s, int32_t dx, int32_t dy) { return plane_shift(s, "navigation field set", dx, dy, &lom_navset_clear); }
int lom_navset_get_geometry(const lom_navset *s, lom_occupancy_geometry *out) { return plane_get_geometry(s, out); }
void *lom_navset_stream(lom_navset *s) { return plane_stream(s); }
int lom_navset_device(const lom_navset *s) { return plane_device(s); }
int lom_navset_wait_event(lom_navset *s, void *hip_event) { return plane_wait_event(s, hip_event); }

int lom_navset_set_option(lom_navset *s, int option, int64_t value)
{
    if (!s) return LOM_ERR_ARG;
    switch (option) {
    case LOM_NAVSET_OPT_TEST_INNER_CAP:
        return set_test_option(s, s->inner_cap, value, navfield::kInnerCapMax, navfield::kInnerCapDefault,
                               "LOM_NAVSET_OPT_TEST_INNER_CAP: 1 .. 2^20, or <= 0 for the default");
    case LOM_NAVSET_OPT_TEST_BATCH:
        return set_test_option(s, s->batch, value, navfield::kBatchMax, navfield::kBatchDefault,
                               "LOM_NAVSET_OPT_TEST_BATCH: 1 .. 256, or <= 0 for the default");
    case LOM_NAVSET_OPT_TEST_ALL_TILES:
        return set_test_option(s, s->all_tiles, value, 1, 0, "LOM_NAVSET_OPT_TEST_ALL_TILES: 0, 1, or < 0 for the default");
    default:
        return fail(s, LOM_ERR_ARG, "unknown navigation field set option");
    }
}

size_t lom_navset_field_count(const lom_navset *s) { return s ? s->n_fields : 0; }

int lom_navset_solve(lom_navset *s, const int8_t *plane, const lom_navfield_params *params, int goal_kind, const void *goals,
                     const uint32_t *goal_offsets, size_t n_fields, lom_navfield_summary *summaries)
{
    return solve_from(s, plane_from_host(plane), params, goal_kind, goals, goal_offsets, n_fields, summaries);
}

int lom_navset_solve_device(lom_navset *s, const int8_t *d_plane, void *hip_event_or_null, const lom_navfield_params *params, int goal_kind,
                            const void *goals, const uint32_t *goal_offsets, size_t n_fields, lom_navfield_summary *summaries)
{
    return solve_from(s, plane_from_device(d_plane, hip_event_or_null), params, goal_kind, goals, goal_offsets, n_fields, summaries);
}

int lom_navset_solve_from_clearance(lom_navset *s, lom_clearance *clearance, const lom_navfield_params *params, int goal_kind, const void *goals,
                                    const uint32_t *goal_offsets, size_t n_fields, lom_navfield_summary *summaries)
{
    return solve_from(s, plane_from_clearance(clearance), params, goal_kind, goals, goal_offsets, n_fields, summaries);
}

int lom_navset_potential(lom_navset *s, size_t i, uint32_t *out, size_t cap)
{
    if (!s || (cap && !out)) return LOM_ERR_ARG;
    if (i >= s->n_fields) return fail(s, LOM_ERR_ARG, "navigation field set: a field index in 0 .. field_count - 1");
    const size_t n = std::min(cap, s->n_cells());
    if (!n) return LOM_OK;
    LOM_HIP(s, hipSetDevice(s->device));
    LOM_HIP(s, hipMemcpyAsync(out, s->fields.as<uint32_t>() + i * s->n_cells(), n * 4, hipMemcpyDeviceToHost, s->stream));
    LOM_HIP(s, hipStreamSynchronize(s->stream));
    return LOM_OK;
}

int lom_navset_potential_device(lom_navset *s, size_t i, const uint32_t **d_out)
{
    if (!s || !d_out) return LOM_ERR_ARG;
    *d_out = nullptr;
    if (i >= s->n_fields) return fail(s, LOM_ERR_ARG, "navigation field set: a field index in 0 .. field_count - 1");
    *d_out = s->fields.as<const uint32_t>() + i * s->n_cells();
    return LOM_OK;
}

int lom_navset_gather(lom_navset *s, int point_kind, const void *points, size_t n, uint32_t *out)
{
    if (!s) return LOM_ERR_ARG;
    if (const char *why = navset::gather_refusal(point_kind, points, n, s->n_fields, out)) return fail(s, LOM_ERR_ARG, why);
    if (!n || !s->n_fields) return LOM_OK;
    LOM_HIP(s, hipSetDevice(s->device));
    const size_t out_bytes = (size_t)s->n_fields * n * 4;
    int rc;
    if ((rc = ensure(s, s->out_a, out_bytes)) != LOM_OK) return rc;
    std::vector<int32_t> cells;
    if ((rc = upload_points(s, point_kind, points, n, cells)) != LOM_OK) return rc;
    hipLaunchKernelGGL(k_navset_gather, dim3(navfield::blocks_for(n), s->n_fields), dim3(kNavThreads), 0, s->stream, s->fields.as<const uint32_t>(),
                       s->args(), s->points.as<const int32_t>(), (uint32_t)n, s->out_a.as<uint32_t>());
    LOM_HIP(s, hipGetLastError());
    LOM_HIP(s, hipMemcpyAsync(out, s->out_a.p, out_bytes, hipMemcpyDeviceToHost, s->stream));
    LOM_HIP(s, hipStreamSynchronize(s->stream));
    return LOM_OK;
}

int lom_navset_nearest(lom_navset *s, uint16_t *owner_out, uint32_t *potential_out, uint64_t *cells_owned)
{
    if (!s) return LOM_ERR_ARG;
    if (!s->solved) return fail(s, LOM_ERR_STATE, "navigation field set: no solve has completed since create, clear or shift");
    if (!owner_out && !potential_out && !cells_owned) return LOM_OK;
    LOM_HIP(s, hipSetDevice(s->device));
    const size_t n_cells = s->n_cells(), owned_bytes = (size_t)s->n_fields * 8;
    int rc;
    if ((owner_out && (rc = ensure(s, s->out_a, n_cells * 2)) != LOM_OK) || (potential_out && (rc = ensure(s, s->out_b, n_cells * 4)) != LOM_OK) ||
        (cells_owned && owned_bytes && (rc = ensure(s, s->out_c, owned_bytes)) != LOM_OK))
        return rc;
    unsigned long long *const owned = cells_owned && owned_bytes ? s->out_c.as<unsigned long long>() : nullptr;
    if (owned) LOM_HIP(s, hipMemsetAsync(owned, 0, owned_bytes, s->stream));
    hipLaunchKernelGGL(k_navset_nearest, dim3(navset::nearest_groups(n_cells)), dim3(kNavThreads), 0, s->stream, s->fields.as<const uint32_t>(),
                       (uint32_t)n_cells, s->n_fields, owner_out ? s->out_a.as<uint16_t>() : nullptr,
                       potential_out ? s->out_b.as<uint32_t>() : nullptr, owned);
    LOM_HIP(s, hipGetLastError());
    if (owner_out) LOM_HIP(s, hipMemcpyAsync(owner_out, s->out_a.p, n_cells * 2, hipMemcpyDeviceToHost, s->stream));
    if (potential_out) LOM_HIP(s, hipMemcpyAsync(potential_out, s->out_b.p, n_cells * 4, hipMemcpyDeviceToHost, s->stream));
    if (owned) LOM_HIP(s, hipMemcpyAsync(cells_owned, owned, owned_bytes, hipMemcpyDeviceToHost, s->stream));
    LOM_HIP(s, hipStreamSynchronize(s->stream));
    return LOM_OK;
}

int lom_navset_paths(lom_navset *s, const int32_t *field_of_start, int start_kind, const void *starts, size_t n_starts, uint16_t *cells_out,
                     size_t cap, uint32_t *lengths_out)
{
    if (!s) return LOM_ERR_ARG;
    if (start_kind != LOM_NAV_CELLS && start_kind != LOM_NAV_METRES) return fail(s, LOM_ERR_ARG, "navigation field set: starts are LOM_NAV_CELLS or LOM_NAV_METRES");
    if ((n_starts && !starts) || n_starts > navfield::kMaxPoints) return fail(s, LOM_ERR_ARG, "navigation field set paths: starts, at most 2^24 of them");
    if (cap > navfield::kMaxPathCells || (cap && n_starts > navfield::kMaxPathCells / cap) || (n_starts && cap && !cells_out))
        return fail(s, LOM_ERR_ARG, "navigation field set paths: an output of n_starts * cap cells, at most 2^28");
    if (!navset::path_fields_ok(field_of_start, n_starts, s->n_fields))
        return fail(s, LOM_ERR_ARG, "navigation field set paths: a field index in 0 .. field_count - 1 per start");
    if (!n_starts) return LOM_OK;
    LOM_HIP(s, hipSetDevice(s->device));
    const size_t cell_bytes = n_starts * cap * 4;
    int rc;
    if ((rc = ensure(s, s->out_a, std::max(cell_bytes, (size_t)256))) != LOM_OK || (rc = ensure(s, s->out_b, n_starts * 4)) != LOM_OK ||
        (rc = ensure(s, s->field_of, n_starts * 4)) != LOM_OK)
        return rc;
    std::vector<int32_t> start_cells;
    if ((rc = upload_points(s, start_kind, starts, n_starts, start_cells)) != LOM_OK) return rc;
    LOM_HIP(s, hipMemcpyAsync(s->field_of.p, field_of_start, n_starts * 4, hipMemcpyHostToDevice, s->stream));
    if (cell_bytes) LOM_HIP(s, hipMemsetAsync(s->out_a.p, 0, cell_bytes, s->stream));
    hipLaunchKernelGGL(k_navset_trace, dim3(navfield::blocks_for(n_starts)), dim3(kNavThreads), 0, s->stream, s->plane.as<const int8_t>(),
                       s->table.as<const uint32_t>(), s->fields.as<const uint32_t>(), s->args(), s->points.as<const int32_t>(),
                       s->field_of.as<const int32_t>(), (uint32_t)n_starts, (uint32_t)cap, s->out_a.as<uint16_t>(), s->out_b.as<uint32_t>());
    LOM_HIP(s, hipGetLastError());
    if (cell_bytes) LOM_HIP(s, hipMemcpyAsync(cells_out, s->out_a.p, cell_bytes, hipMemcpyDeviceToHost, s->stream));
    if (lengths_out) LOM_HIP(s, hipMemcpyAsync(lengths_out, s->out_b.p, n_starts * 4, hipMemcpyDeviceToHost, s->stream));
    LOM_HIP(s, hipStreamSynchronize(s->stream));
    return LOM_OK;
}

int lom_navset_stats(const lom_navset *s, lom_navset_solve_stats *out)
{
    if (!s || !out) return LOM_ERR_ARG;
    *out = s->stats;
    return LOM_OK;
}

}  // extern "C"
