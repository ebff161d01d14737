// Elevation grid: every point of a posed scan that is an occupancy hit adds its quantised height to its cell of a dense
// 2-D grid -- count, minimum, maximum, sum, all integers -- and a second pass derives ground height, slope, roughness,
// step and a traversability cost.  Definitions: include/lidar_odometry_amd.h ("elevation grid"); kernels:
// k_elevation.hpp; host planning (value ranges, launches): elevation_host.cpp; what a grid handle is and does around its
// kernels, the integrate entry points included: grid_handle.hpp; DESIGN.md 7k.  A handle family of its own beside the map
// path: the descriptors are the assembly's, the clouds an archive's or the caller's, and no default path launches any of
// this.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "elevation_host.hpp"
#include "grid_handle.hpp"
#include "grid_shift.hpp"
#include "k_elevation.hpp"

using namespace lom;

// Beside the core's (grid_handle.hpp):
struct lom_elevation : lom::GridHandle {
    lom_elevation_geometry geo{};
    lom::DeviceBuf cells;        // width * height records of 32 bytes
    lom::DeviceBuf cells_shadow; // where a shift moves them to, from the first shift on (grid_handle.hpp)
    lom::DeviceBuf cost;         // int8 per cell
    lom::DeviceBuf layers;       // six f32 planes, from the first lom_elevation_layers on
    lom::DeviceBuf unpacked;     // a chunk of the records as four arrays, on its way out (lom_elevation_cells)
    uint32_t merge = 1;          // LOM_ELEV_OPT_TEST_WAVE_MERGE

    size_t n_cells() const { return (size_t)geo.width * geo.height; }

    // the family's part of the integrate entry points
    using Plan = elevation::Plan;
    static constexpr const char *kName = "elevation";
    static constexpr auto kPlan = &elevation::plan;  // (no option sets plan_cap here)

    int run(const Plan &plan, const float *xyz, uint32_t stride_floats, const lom_elevation_point_params &p, lom_elevation_stats &st)
    {
        int rc;
        if ((rc = grid_stage(this, plan.scans.scans, EW_COUNT)) != LOM_OK) return rc;
        ElevArgs a;
        a.resolution = geo.resolution, a.origin_x = geo.origin_x, a.origin_y = geo.origin_y, a.z_ref = geo.z_ref;
        a.width = geo.width, a.height = geo.height;
        a.z_lo = p.z_lo, a.z_hi = p.z_hi, a.min_range = p.min_range, a.max_range = p.max_range;
        a.stride = stride_floats;
        a.merge = merge;
        for (const elevation::Launch &l : plan.launches) {
            hipLaunchKernelGGL(k_elev_accumulate, dim3(l.grid_x, l.count), dim3(kAsmThreads), 0, stream,
                               desc.as<const AsmScan>() + l.first, xyz, a, cells.as<ElevCell>(), words.as<uint32_t>());
            LOM_HIP(this, hipGetLastError());
        }
        if ((rc = grid_read_words(this, EW_COUNT, true)) != LOM_OK) return rc;
        const uint32_t *got = h_words.as<uint32_t>();
        st.points = plan.scans.points_in;
        st.points_marked = u64_of(got, EW_MARKED);
        st.points_out_of_height = u64_of(got, EW_HEIGHT);
        st.cells_new = u64_of(got, EW_NEW);
        return LOM_OK;
    }
};

namespace {

thread_local std::string g_elevation_create_error;

constexpr size_t kUnpackChunk = size_t(1) << 22;  // cells of one lom_elevation_cells round: 80 MB of staging at most

int clear_cells(lom_elevation *g)
{
    const uint32_t n = (uint32_t)g->n_cells();
    hipLaunchKernelGGL(k_elev_clear, dim3((n + kElevThreads - 1) / kElevThreads), dim3(kElevThreads), 0, g->stream,
                       g->cells.as<ElevCell>(), n);
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

// k_elev_derive over the whole grid: the layers named in `out` (six planes, each may be NULL) and, with cp, the cost
int derive_on_device(lom_elevation *g, const lom_elevation_layer_params *lp, const lom_elevation_cost_params *cp, float *const out[6])
{
    ElevDeriveArgs a;
    a.resolution = g->geo.resolution, a.z_ref = g->geo.z_ref;
    a.width = g->geo.width, a.height = g->geo.height, a.min_points = lp->min_points;
    a.R = (int)lp->window;
    a.min_out = out ? out[0] : nullptr, a.max_out = out ? out[1] : nullptr, a.mean_out = out ? out[2] : nullptr;
    a.slope_out = out ? out[3] : nullptr, a.rough_out = out ? out[4] : nullptr, a.step_out = out ? out[5] : nullptr;
    a.cost_out = cp ? g->cost.as<int8_t>() : nullptr;
    a.max_slope = cp ? cp->max_slope : 1.f, a.max_step = cp ? cp->max_step : 1.f;
    a.max_rough = cp ? cp->max_rough : 1.f, a.max_span = cp ? cp->max_span : 1.f;
    if (cp) LOM_HIP(g, hipMemsetAsync(g->words.p, 0, (size_t)EC_COUNT * 4, g->stream));
    hipLaunchKernelGGL(k_elev_derive, dim3((a.width + kElevTileX - 1) / kElevTileX, (a.height + kElevTileY - 1) / kElevTileY),
                       dim3(kElevTileX, kElevTileY), 0, g->stream, g->cells.as<const ElevCell>(), a, g->words.as<uint32_t>());
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

int cost_on_device(lom_elevation *g, const lom_elevation_layer_params *lp, const lom_elevation_cost_params *cp)
{
    if (!elevation::layer_params_ok(lp)) return fail(g, LOM_ERR_ARG, "elevation layers: min_points >= 1, window in 1 .. 4");
    if (!elevation::cost_params_ok(cp))
        return fail(g, LOM_ERR_ARG, "elevation cost: max_slope, max_step, max_rough, max_span finite and > 0");
    LOM_HIP(g, hipSetDevice(g->device));
    return derive_on_device(g, lp, cp, nullptr);
}

}  // namespace

extern "C" {

int lom_elevation_create(const lom_elevation_geometry *geometry, int device, lom_elevation **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if (!elevation::geometry_ok(geometry))
        return create_fail(g_elevation_create_error, LOM_ERR_ARG,
                           "elevation geometry: resolution > 0 and finite, a finite origin and z_ref, 1 <= width, height <= 8192");
    if (const int rc = check_device(device, g_elevation_create_error); rc != LOM_OK) return rc;
    lom_elevation *g = new (std::nothrow) lom_elevation();
    if (!g) return create_fail(g_elevation_create_error, LOM_ERR_OOM, "host allocation");
    g->device = device;
    g->geo = *geometry;
    int rc = grid_setup(g, g_elevation_create_error, "elevation grid setup", "hipMalloc (elevation grid)");
    if (rc == LOM_OK && (alloc(g->cells, g->n_cells() * sizeof(ElevCell)) != hipSuccess || alloc(g->cost, g->n_cells()) != hipSuccess))
        rc = create_fail(g_elevation_create_error, LOM_ERR_OOM, "hipMalloc (elevation grid)");
    if (rc == LOM_OK) {
        const uint32_t n = (uint32_t)g->n_cells();
        hipLaunchKernelGGL(k_elev_clear, dim3((n + kElevThreads - 1) / kElevThreads), dim3(kElevThreads), 0, g->stream,
                           g->cells.as<ElevCell>(), n);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = create_fail(g_elevation_create_error, LOM_ERR_HIP, "elevation grid setup", e);
    }
    if (rc != LOM_OK) {
        lom_elevation_destroy(g);
        return rc;
    }
    *out = g;
    return LOM_OK;
}

void lom_elevation_destroy(lom_elevation *g) { grid_destroy(g); }

const char *lom_elevation_last_error(const lom_elevation *g) { return g ? g->error.c_str() : g_elevation_create_error.c_str(); }

int lom_elevation_clear(lom_elevation *g)
{
    if (!g) return LOM_ERR_ARG;
    LOM_HIP(g, hipSetDevice(g->device));
    if (const int rc = clear_cells(g); rc != LOM_OK) return rc;
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

int lom_elevation_shift(lom_elevation *g, int32_t dx, int32_t dy)
{
    if (!g) return LOM_ERR_ARG;
    if (!dx && !dy) return LOM_OK;
    const lom_occupancy_geometry plane{g->geo.resolution, g->geo.origin_x, g->geo.origin_y, g->geo.width, g->geo.height};
    GridShift s;
    int rc = grid_shift_plan(g, "elevation", plane, dx, dy, s);
    if (rc != LOM_OK) return rc;
    if (!s.keeps) {
        if ((rc = lom_elevation_clear(g)) != LOM_OK) return rc;
    } else {
        LOM_HIP(g, hipSetDevice(g->device));
        if ((rc = grid_shift_shadow(g, g->cells_shadow, g->n_cells() * sizeof(ElevCell), "hipMalloc (elevation shift)")) != LOM_OK) return rc;
        LOM_HIP(g, launch_shift_rec32(g->stream, g->cells.p, g->cells_shadow.p, g->geo.width, g->geo.height, s.dx, s.dy));
        if ((rc = grid_shift_wait(g)) != LOM_OK) return rc;
        g->cells.swap(g->cells_shadow);
    }
    g->geo.origin_x = s.geo.origin_x, g->geo.origin_y = s.geo.origin_y;  // (z_ref stays)
    return LOM_OK;
}

int lom_elevation_get_geometry(const lom_elevation *g, lom_elevation_geometry *out)
{
    if (!g || !out) return LOM_ERR_ARG;
    *out = g->geo;
    return LOM_OK;
}

void *lom_elevation_stream(lom_elevation *g) { return g ? (void *)g->stream : nullptr; }
int lom_elevation_device(const lom_elevation *g) { return g ? g->device : LOM_ERR_ARG; }
int lom_elevation_wait_event(lom_elevation *g, void *hip_event) { return grid_wait_event(g, hip_event); }

int lom_elevation_set_option(lom_elevation *g, int option, int64_t value)
{
    if (!g) return LOM_ERR_ARG;
    switch (option) {
    case LOM_ELEV_OPT_TEST_WAVE_MERGE:
        if (value > 1) return fail(g, LOM_ERR_ARG, "LOM_ELEV_OPT_TEST_WAVE_MERGE: 0, 1, or < 0 for the default");
        g->merge = value == 0 ? 0u : 1u;
        return LOM_OK;
    default:
        return fail(g, LOM_ERR_ARG, "unknown elevation option");
    }
}

int lom_elevation_integrate(lom_elevation *g, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                            const lom_elevation_point_params *p, lom_elevation_stats *stats)
{
    return grid_integrate(g, a, ids, poses, count, p, stats);
}

int lom_elevation_integrate_cloud_device(lom_elevation *g, const float *d_xyz, size_t n, size_t stride_bytes,
                                         const lom_graph_pose *pose, const lom_elevation_point_params *p, void *hip_event_or_null,
                                         lom_elevation_stats *stats)
{
    return grid_integrate_cloud(g, d_xyz, false, n, stride_bytes, pose, p, hip_event_or_null, stats);
}

int lom_elevation_integrate_cloud(lom_elevation *g, const float *xyz, size_t n, size_t stride_bytes, const lom_graph_pose *pose,
                                  const lom_elevation_point_params *p, lom_elevation_stats *stats)
{
    return grid_integrate_cloud(g, xyz, true, n, stride_bytes, pose, p, nullptr, stats);
}

int64_t lom_elevation_cells(lom_elevation *g, uint32_t *count_out, int32_t *zmin_out, int32_t *zmax_out, int64_t *sum_out, size_t cap)
{
    if (!g) return LOM_ERR_ARG;
    const size_t n = std::min(cap, g->n_cells());
    if (n && (count_out || zmin_out || zmax_out || sum_out)) {
        LOM_HIP(g, hipSetDevice(g->device));
        const size_t chunk = std::min(n, kUnpackChunk);
        if (const int rc = ensure(g, g->unpacked, chunk * 20); rc != LOM_OK) return rc;
        // the chunk as [sum i64][count u32][zmin i32][zmax i32]: the 8-byte array first, so that all are aligned
        long long *const d_sum = g->unpacked.as<long long>();
        uint32_t *const d_count = reinterpret_cast<uint32_t *>(d_sum + chunk);
        int32_t *const d_zmin = reinterpret_cast<int32_t *>(d_count + chunk), *const d_zmax = d_zmin + chunk;
        for (size_t first = 0; first < n; first += chunk) {
            const uint32_t m = (uint32_t)std::min(chunk, n - first);
            hipLaunchKernelGGL(k_elev_unpack, dim3((m + kElevThreads - 1) / kElevThreads), dim3(kElevThreads), 0, g->stream,
                               g->cells.as<const ElevCell>(), (uint32_t)first, m, d_count, d_zmin, d_zmax, d_sum);
            LOM_HIP(g, hipGetLastError());
            if (count_out) LOM_HIP(g, hipMemcpyAsync(count_out + first, d_count, (size_t)m * 4, hipMemcpyDeviceToHost, g->stream));
            if (zmin_out) LOM_HIP(g, hipMemcpyAsync(zmin_out + first, d_zmin, (size_t)m * 4, hipMemcpyDeviceToHost, g->stream));
            if (zmax_out) LOM_HIP(g, hipMemcpyAsync(zmax_out + first, d_zmax, (size_t)m * 4, hipMemcpyDeviceToHost, g->stream));
            if (sum_out) LOM_HIP(g, hipMemcpyAsync(sum_out + first, d_sum, (size_t)m * 8, hipMemcpyDeviceToHost, g->stream));
            LOM_HIP(g, hipStreamSynchronize(g->stream));  // (the next round overwrites the staging block)
        }
    }
    return (int64_t)g->n_cells();
}

int lom_elevation_layers(lom_elevation *g, const lom_elevation_layer_params *lp, float *min_out, float *max_out, float *mean_out,
                         float *slope_out, float *rough_out, float *step_out, size_t cap)
{
    if (!g) return LOM_ERR_ARG;
    if (!elevation::layer_params_ok(lp)) return fail(g, LOM_ERR_ARG, "elevation layers: min_points >= 1, window in 1 .. 4");
    float *const host[6] = {min_out, max_out, mean_out, slope_out, rough_out, step_out};
    const size_t n = std::min(cap, g->n_cells());
    bool any = false;
    for (float *h : host) any = any || h != nullptr;
    if (!n || !any) return LOM_OK;
    LOM_HIP(g, hipSetDevice(g->device));
    if (const int rc = ensure(g, g->layers, g->n_cells() * 4 * 6); rc != LOM_OK) return rc;
    float *dev[6];
    for (int k = 0; k < 6; k++) dev[k] = host[k] ? g->layers.as<float>() + (size_t)k * g->n_cells() : nullptr;
    if (const int rc = derive_on_device(g, lp, nullptr, dev); rc != LOM_OK) return rc;
    for (int k = 0; k < 6; k++)
        if (host[k]) LOM_HIP(g, hipMemcpyAsync(host[k], dev[k], n * 4, hipMemcpyDeviceToHost, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

int lom_elevation_cost(lom_elevation *g, const lom_elevation_layer_params *lp, const lom_elevation_cost_params *cp, int8_t *out,
                       size_t cap, lom_elevation_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!g || (cap && !out)) return LOM_ERR_ARG;
    int rc = cost_on_device(g, lp, cp);
    if (rc != LOM_OK) return rc;
    if ((rc = grid_copy_out(g, out, g->cost, std::min(cap, g->n_cells()), EC_COUNT)) != LOM_OK) return rc;
    if (summary) {
        const uint32_t *t = g->h_words.as<uint32_t>();
        summary->cells_unknown = t[EC_UNKNOWN], summary->cells_lethal = t[EC_LETHAL], summary->cells_costed = t[EC_COSTED];
    }
    return LOM_OK;
}

int lom_elevation_cost_device(lom_elevation *g, const lom_elevation_layer_params *lp, const lom_elevation_cost_params *cp,
                              const int8_t **d_out)
{
    if (!g || !d_out) return LOM_ERR_ARG;
    *d_out = nullptr;
    const int rc = cost_on_device(g, lp, cp);
    if (rc != LOM_OK) return rc;
    *d_out = g->cost.as<const int8_t>();
    return LOM_OK;
}

}  // extern "C"
