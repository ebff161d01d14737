// Clearance grid: the int8 planes of the occupancy and the elevation grid, merged, become an exact truncated Euclidean
// distance transform (squared cells, u16) and an inflated int8 cost.  Definitions: include/lidar_odometry_amd.h
// ("clearance grid"); kernels: k_clearance.hpp; host planning (value ranges, R, the cost table, rectangles, launch
// shapes): clearance_host.cpp; DESIGN.md 7l.  A handle family of its own: no scans are integrated here, so the handle is a
// PlaneHandle (plane_handle.hpp) and not a GridHandle, and no default path launches any of this.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "clearance_host.hpp"
#include "elevation_host.hpp"
#include "k_clearance.hpp"
#include "occupancy_host.hpp"
#include "plane_handle.hpp"

using namespace lom;

// The grid owns its stream and every buffer below.
struct lom_clearance : lom::PlaneHandle {  // in_ev: the occupancy grid's, the elevation grid's
    lom::DeviceBuf base, d2, cost;      // int8, u16, int8 per cell
    lom::DeviceBuf bitmap;              // height x ceil(width / 64) u64: the obstacles
    lom::DeviceBuf table;               // the cost table of the last update, 254^2 + 1 bytes
    lom::DeviceBuf words;               // the summary words (16 u32)
    lom::DeviceBuf in_occ, in_elev;     // host planes on their way in, from the first host update on
    lom::DeviceBuf q_xy, q_dist, q_cost;  // a query's points and results, grow-only
    lom::PinnedBuf h_words;             // the summary words on their way out
    std::vector<uint8_t> h_table;       // what `table` holds (empty: nothing yet)
    uint32_t tile_rows = clearance::kTileRowsMax;  // LOM_CLEAR_OPT_TEST_TILE_ROWS
    uint32_t no_prune = 0;                         // LOM_CLEAR_OPT_TEST_NO_PRUNE

    size_t n_words() const { return (size_t)geo.height * clearance::words_per_row(geo.width); }
};

namespace {

thread_local std::string g_clearance_create_error;

constexpr const char *kName = "clearance";  // the head of the texts of the plane-handle core

constexpr const char *kParamsText =
    "clearance parameters: 0 <= inscribed_radius <= inflation_radius, decay >= 0, all finite, known flags, "
    "floor(inflation_radius / resolution) <= 254";

int fill(lom_clearance *c)
{
    const uint32_t n = (uint32_t)c->n_cells();  // (n_words <= n_cells)
    hipLaunchKernelGGL(k_clear_fill, dim3((n + kClearThreads - 1) / kClearThreads), dim3(kClearThreads), 0, c->stream, n,
                       (uint32_t)c->n_words(), c->base.as<int8_t>(), c->d2.as<uint16_t>(), c->cost.as<int8_t>(),
                       c->bitmap.as<unsigned long long>());
    LOM_HIP(c, hipGetLastError());
    return LOM_OK;
}

void summary_from(const uint32_t *t, lom_clearance_summary *s)
{
    s->cells_lethal = t[CW_LETHAL], s->cells_inscribed = t[CW_INSCRIBED], s->cells_costed = t[CW_COSTED];
    s->cells_unknown = t[CW_UNKNOWN], s->cells_invalid = t[CW_INVALID], s->cells_cleared = t[CW_CLEARED];
}

// the refusals of every update form that need no device: the text, or NULL
const char *update_refusal(const lom_clearance *c, bool have_occ, bool have_elev, const lom_clearance_params *p)
{
    if (!have_occ && !have_elev) return "clearance update: an occupancy plane, an elevation plane or both";
    if (!clearance::params_ok(p, c->geo.resolution)) return kParamsText;
    return nullptr;
}

// The kernels of an update over planes in HBM that this stream may read now, then the wait.  The arguments are valid.
int update_on_device(lom_clearance *c, const int8_t *d_occ, const int8_t *d_elev, const lom_clearance_params &p,
                     const clearance::Rect &rect, lom_clearance_summary *summary)
{
    const uint32_t R = clearance::radius_cells(p.inflation_radius, c->geo.resolution);
    std::vector<uint8_t> t((size_t)R * R + 1);
    clearance::cost_table(p, c->geo.resolution, R, t.data());
    if (t != c->h_table) {  // (every call waits for its work, so no enqueued kernel reads the old table)
        c->h_table.clear();
        LOM_HIP(c, hipMemcpyAsync(c->table.p, t.data(), t.size(), hipMemcpyHostToDevice, c->stream));
        LOM_HIP(c, hipStreamSynchronize(c->stream));  // t is pageable and local
        c->h_table.swap(t);
    }
    const clearance::Rect grown = clearance::grow(rect, R, c->geo);
    const clearance::MergeGrid m = clearance::merge_grid(grown);
    const clearance::TileGrid tg = clearance::tile_grid(rect, R, c->tile_rows);
    ClearArgs a;
    a.width = c->geo.width, a.height = c->geo.height, a.wpr = clearance::words_per_row(c->geo.width);
    a.x0 = rect.x0, a.y0 = rect.y0, a.x1 = rect.x1, a.y1 = rect.y1;
    a.R = R, a.flags = p.flags, a.tile_rows = tg.tile_rows, a.no_prune = c->no_prune;
    LOM_HIP(c, hipMemsetAsync(c->words.p, 0, (size_t)CW_COUNT * 4, c->stream));
    hipLaunchKernelGGL(k_clear_merge, dim3(m.blocks), dim3(kClearThreads), 0, c->stream, d_occ, d_elev, a, m.wx0, m.n_wx, m.y0,
                       m.n_rows, c->base.as<int8_t>(), c->bitmap.as<unsigned long long>(), c->words.as<uint32_t>());
    LOM_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(k_clear_distance, dim3(tg.n_wx, tg.n_ty), dim3(kClearThreads), tg.lds_bytes, c->stream,
                       c->bitmap.as<const unsigned long long>(), c->base.as<const int8_t>(), c->table.as<const uint8_t>(), a,
                       tg.wx0, c->d2.as<uint16_t>(), c->cost.as<int8_t>(), c->words.as<uint32_t>());
    LOM_HIP(c, hipGetLastError());
    LOM_HIP(c, hipMemcpyAsync(c->h_words.h, c->words.p, (size_t)CW_COUNT * 4, hipMemcpyDeviceToHost, c->stream));
    LOM_HIP(c, hipEventRecord(c->done_ev, c->stream));
    LOM_HIP(c, hipStreamSynchronize(c->stream));
    if (summary) summary_from(c->h_words.as<uint32_t>(), summary);
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_clearance_create(const lom_occupancy_geometry *geometry, int device, lom_clearance **out)
{
    if (!out) return LOM_ERR_ARG;
    lom_clearance *c = nullptr;
    int rc = plane_new(geometry, device, g_clearance_create_error, kName, "clearance grid setup", 2, &c);
    if (rc != LOM_OK) return rc;
    hipError_t e = alloc(c->h_words, 64, hipHostMallocDefault);
    if (e != hipSuccess) rc = create_fail(g_clearance_create_error, LOM_ERR_HIP, "clearance grid setup", e);
    const size_t n = c->n_cells();
    if (rc == LOM_OK &&
        (alloc(c->base, n) != hipSuccess || alloc(c->d2, n * 2) != hipSuccess || alloc(c->cost, n) != hipSuccess ||
         alloc(c->bitmap, c->n_words() * 8) != hipSuccess ||
         alloc(c->table, (size_t)clearance::kMaxRadius * clearance::kMaxRadius + 1) != hipSuccess || alloc(c->words, 64) != hipSuccess))
        rc = create_fail(g_clearance_create_error, LOM_ERR_OOM, "hipMalloc (clearance grid)");
    if (rc == LOM_OK) {
        const uint32_t cells = (uint32_t)n;
        hipLaunchKernelGGL(k_clear_fill, dim3((cells + kClearThreads - 1) / kClearThreads), dim3(kClearThreads), 0, c->stream,
                           cells, (uint32_t)c->n_words(), c->base.as<int8_t>(), c->d2.as<uint16_t>(), c->cost.as<int8_t>(),
                           c->bitmap.as<unsigned long long>());
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = create_fail(g_clearance_create_error, LOM_ERR_HIP, "clearance grid setup", e);
    }
    if (rc != LOM_OK) {
        lom_clearance_destroy(c);
        return rc;
    }
    *out = c;
    return LOM_OK;
}

void lom_clearance_destroy(lom_clearance *c) { plane_destroy(c); }
const char *lom_clearance_last_error(const lom_clearance *c) { return plane_last_error(c, g_clearance_create_error); }

int lom_clearance_clear(lom_clearance *c)
{
    if (!c) return LOM_ERR_ARG;
    LOM_HIP(c, hipSetDevice(c->device));
    if (const int rc = fill(c); rc != LOM_OK) return rc;
    LOM_HIP(c, hipStreamSynchronize(c->stream));
    return LOM_OK;
}

int lom_clearance_shift(lom_clearance *c, int32_t dx, int32_t dy) { return plane_shift(c, "clearance", dx, dy, &lom_clearance_clear); }
int lom_clearance_get_geometry(const lom_clearance *c, lom_occupancy_geometry *out) { return plane_get_geometry(c, out); }
void *lom_clearance_stream(lom_clearance *c) { return plane_stream(c); }
int lom_clearance_device(const lom_clearance *c) { return plane_device(c); }
int lom_clearance_wait_event(lom_clearance *c, void *hip_event) { return plane_wait_event(c, hip_event); }

int lom_clearance_set_option(lom_clearance *c, int option, int64_t value)
{
    if (!c) return LOM_ERR_ARG;
    switch (option) {
    case LOM_CLEAR_OPT_TEST_TILE_ROWS:
        if (value > (int64_t)clearance::kTileRowsMax) return fail(c, LOM_ERR_ARG, "LOM_CLEAR_OPT_TEST_TILE_ROWS: 1 .. 32, or <= 0 for the default");
        c->tile_rows = value <= 0 ? clearance::kTileRowsMax : (uint32_t)value;
        return LOM_OK;
    case LOM_CLEAR_OPT_TEST_NO_PRUNE:
        if (value > 1) return fail(c, LOM_ERR_ARG, "LOM_CLEAR_OPT_TEST_NO_PRUNE: 0, 1, or < 0 for the default");
        c->no_prune = value == 1 ? 1u : 0u;
        return LOM_OK;
    default:
        return fail(c, LOM_ERR_ARG, "unknown clearance option");
    }
}

int lom_clearance_update_device(lom_clearance *c, const int8_t *d_occ, const int8_t *d_elev, void *hip_event_or_null,
                                const lom_clearance_params *params, const lom_clearance_window *window,
                                lom_clearance_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!c) return LOM_ERR_ARG;
    if (const char *why = update_refusal(c, d_occ != nullptr, d_elev != nullptr, params)) return fail(c, LOM_ERR_ARG, why);
    const clearance::Rect rect = clearance::clip(window, c->geo);
    if (rect.empty()) return LOM_OK;
    LOM_HIP(c, hipSetDevice(c->device));
    if (hip_event_or_null) LOM_HIP(c, hipStreamWaitEvent(c->stream, (hipEvent_t)hip_event_or_null, 0));
    return update_on_device(c, d_occ, d_elev, *params, rect, summary);
}

int lom_clearance_update(lom_clearance *c, const int8_t *occ, const int8_t *elev, const lom_clearance_params *params,
                         const lom_clearance_window *window, lom_clearance_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!c) return LOM_ERR_ARG;
    if (const char *why = update_refusal(c, occ != nullptr, elev != nullptr, params)) return fail(c, LOM_ERR_ARG, why);
    const clearance::Rect rect = clearance::clip(window, c->geo);
    if (rect.empty()) return LOM_OK;
    LOM_HIP(c, hipSetDevice(c->device));
    // only the rows the update reads go up: those of the rectangle grown by R
    const clearance::Rect grown = clearance::grow(rect, clearance::radius_cells(params->inflation_radius, c->geo.resolution), c->geo);
    const size_t first = (size_t)grown.y0 * c->geo.width, bytes = (size_t)(grown.y1 - grown.y0) * c->geo.width;
    const int8_t *host[2] = {occ, elev};
    DeviceBuf *dev[2] = {&c->in_occ, &c->in_elev};
    for (int k = 0; k < 2; k++) {
        if (!host[k]) continue;
        if (const int rc = ensure(c, *dev[k], c->n_cells()); rc != LOM_OK) return rc;
        LOM_HIP(c, hipMemcpyAsync(dev[k]->as<int8_t>() + first, host[k] + first, bytes, hipMemcpyHostToDevice, c->stream));
    }
    return update_on_device(c, occ ? c->in_occ.as<const int8_t>() : nullptr, elev ? c->in_elev.as<const int8_t>() : nullptr, *params,
                            rect, summary);
}

int lom_clearance_update_from_grids(lom_clearance *c, lom_occupancy *occupancy, const lom_occupancy_rule *rule,
                                    lom_elevation *elevation, const lom_elevation_layer_params *layer_params,
                                    const lom_elevation_cost_params *cost_params, const lom_clearance_params *params,
                                    const lom_clearance_window *window, lom_clearance_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!c) return LOM_ERR_ARG;
    if (const char *why = update_refusal(c, occupancy != nullptr, elevation != nullptr, params)) return fail(c, LOM_ERR_ARG, why);
    if (occupancy) {
        lom_occupancy_geometry g{};
        (void)lom_occupancy_get_geometry(occupancy, &g);
        if (const int rc = plane_check_producer(c, kName, "occupancy grid", g, lom_occupancy_device(occupancy)); rc != LOM_OK) return rc;
        if (!occupancy::rule_ok(rule)) return fail(c, LOM_ERR_ARG, "occupancy rule: min_free_scans >= 1, min_seen_scans >= 1");
    }
    if (elevation) {
        lom_elevation_geometry g{};
        (void)lom_elevation_get_geometry(elevation, &g);
        const lom_occupancy_geometry flat{g.resolution, g.origin_x, g.origin_y, g.width, g.height};
        if (const int rc = plane_check_producer(c, kName, "elevation grid", flat, lom_elevation_device(elevation)); rc != LOM_OK) return rc;
        if (!elevation::layer_params_ok(layer_params)) return fail(c, LOM_ERR_ARG, "elevation layers: min_points >= 1, window in 1 .. 4");
        if (!elevation::cost_params_ok(cost_params))
            return fail(c, LOM_ERR_ARG, "elevation cost: max_slope, max_step, max_rough, max_span finite and > 0");
    }
    const clearance::Rect rect = clearance::clip(window, c->geo);
    if (rect.empty()) return LOM_OK;
    LOM_HIP(c, hipSetDevice(c->device));
    // the hand-off of plane_handle.hpp, once per producer: read behind it, update, release to it
    const int8_t *d_occ = nullptr, *d_elev = nullptr;
    int rc;
    if (occupancy) {
        if (lom_occupancy_classify_device(occupancy, rule, &d_occ) != LOM_OK)
            return plane_fail_producer(c, kName, "lom_occupancy_classify_device", lom_occupancy_last_error(occupancy));
        if ((rc = plane_read_behind(c, 0, lom_occupancy_stream(occupancy))) != LOM_OK) return rc;
    }
    if (elevation) {
        if (lom_elevation_cost_device(elevation, layer_params, cost_params, &d_elev) != LOM_OK)
            return plane_fail_producer(c, kName, "lom_elevation_cost_device", lom_elevation_last_error(elevation));
        if ((rc = plane_read_behind(c, 1, lom_elevation_stream(elevation))) != LOM_OK) return rc;
    }
    if ((rc = update_on_device(c, d_occ, d_elev, *params, rect, summary)) != LOM_OK) return rc;
    if (occupancy && (rc = plane_release(c, kName, occupancy, lom_occupancy_wait_event, "lom_occupancy_wait_event")) != LOM_OK) return rc;
    return elevation ? plane_release(c, kName, elevation, lom_elevation_wait_event, "lom_elevation_wait_event") : LOM_OK;
}

int lom_clearance_cost(lom_clearance *c, int8_t *out, size_t cap, lom_clearance_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!c || (cap && !out)) return LOM_ERR_ARG;
    LOM_HIP(c, hipSetDevice(c->device));
    if (summary) {
        const uint32_t n = (uint32_t)c->n_cells();
        LOM_HIP(c, hipMemsetAsync(c->words.p, 0, (size_t)CW_COUNT * 4, c->stream));
        hipLaunchKernelGGL(k_clear_count, dim3((n + kClearThreads - 1) / kClearThreads), dim3(kClearThreads), 0, c->stream,
                           c->cost.as<const int8_t>(), n, c->words.as<uint32_t>());
        LOM_HIP(c, hipGetLastError());
        LOM_HIP(c, hipMemcpyAsync(c->h_words.h, c->words.p, (size_t)CW_COUNT * 4, hipMemcpyDeviceToHost, c->stream));
    }
    const size_t n = std::min(cap, c->n_cells());
    if (n) LOM_HIP(c, hipMemcpyAsync(out, c->cost.p, n, hipMemcpyDeviceToHost, c->stream));
    LOM_HIP(c, hipStreamSynchronize(c->stream));
    if (summary) summary_from(c->h_words.as<uint32_t>(), summary);
    return LOM_OK;
}

int lom_clearance_cost_device(lom_clearance *c, const int8_t **d_out)
{
    if (!c || !d_out) return LOM_ERR_ARG;
    *d_out = c->cost.as<const int8_t>();
    return LOM_OK;
}

int lom_clearance_distance_sq(lom_clearance *c, uint16_t *out, size_t cap)
{
    if (!c || (cap && !out)) return LOM_ERR_ARG;
    return plane_copy_out(c, out, c->d2, std::min(cap, c->n_cells()) * 2);
}

int lom_clearance_distance(lom_clearance *c, float *out, size_t cap)
{
    if (!c || (cap && !out)) return LOM_ERR_ARG;
    const size_t n = std::min(cap, c->n_cells());
    if (!n) return LOM_OK;
    std::vector<uint16_t> d2(n);
    if (const int rc = plane_copy_out(c, d2.data(), c->d2, n * 2); rc != LOM_OK) return rc;
    // step 5 per distinct value: d2 <= 254^2, or far
    std::vector<float> metres((size_t)clearance::kMaxRadius * clearance::kMaxRadius + 1);
    for (size_t k = 0; k < metres.size(); k++) metres[k] = (float)(std::sqrt((double)k) * (double)c->geo.resolution);
    for (size_t i = 0; i < n; i++) out[i] = d2[i] < metres.size() ? metres[d2[i]] : std::numeric_limits<float>::infinity();
    return LOM_OK;
}

int64_t lom_clearance_cost_table(const lom_clearance_params *params, const lom_occupancy_geometry *geometry, uint8_t *out, size_t cap)
{
    if (!clearance::geometry_ok(geometry) || !clearance::params_ok(params, geometry->resolution) || (cap && !out)) return LOM_ERR_ARG;
    const uint32_t R = clearance::radius_cells(params->inflation_radius, geometry->resolution);
    std::vector<uint8_t> t((size_t)R * R + 1);
    clearance::cost_table(*params, geometry->resolution, R, t.data());
    if (cap) std::memcpy(out, t.data(), std::min(cap, t.size()));
    return (int64_t)t.size();
}

int lom_clearance_query(lom_clearance *c, const float *xy, size_t n, float *dist_out, int8_t *cost_out)
{
    if (!c) return LOM_ERR_ARG;
    if ((n && !xy) || n > (size_t)1 << 30) return fail(c, LOM_ERR_ARG, "clearance query: points, at most 2^30 of them");
    if (!n || (!dist_out && !cost_out)) return LOM_OK;
    LOM_HIP(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, c->q_xy, n * 8)) != LOM_OK || (rc = ensure(c, c->q_dist, n * 4)) != LOM_OK || (rc = ensure(c, c->q_cost, n)) != LOM_OK)
        return rc;
    LOM_HIP(c, hipMemcpyAsync(c->q_xy.p, xy, n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_clear_query, dim3((uint32_t)((n + kClearThreads - 1) / kClearThreads)), dim3(kClearThreads), 0, c->stream,
                       c->q_xy.as<const float>(), (uint32_t)n, c->geo.resolution, c->geo.origin_x, c->geo.origin_y, c->geo.width,
                       c->geo.height, c->d2.as<const uint16_t>(), c->cost.as<const int8_t>(), c->q_dist.as<float>(),
                       c->q_cost.as<int8_t>());
    LOM_HIP(c, hipGetLastError());
    if (dist_out) LOM_HIP(c, hipMemcpyAsync(dist_out, c->q_dist.p, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (cost_out) LOM_HIP(c, hipMemcpyAsync(cost_out, c->q_cost.p, n, hipMemcpyDeviceToHost, c->stream));
    LOM_HIP(c, hipStreamSynchronize(c->stream));
    return LOM_OK;
}

}  // extern "C"
