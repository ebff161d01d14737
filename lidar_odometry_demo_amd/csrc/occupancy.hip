// Occupancy grid: every scan at its pose votes once per cell of a dense 2-D grid -- passed through, or hit -- and a rule on
// the two counts classifies free / occupied / unknown.  Definitions: include/lidar_odometry_amd.h ("occupancy grid");
// kernels: k_occupancy.hpp; host planning (parameter ranges, slices, boxes, step bound): occupancy_host.cpp; what a grid
// handle is and does around its kernels, the integrate entry points included: grid_handle.hpp; DESIGN.md 7j.  A handle
// family of its own beside the map path: the descriptors are the assembly's, the clouds an archive's or the caller's, and
// no default path launches any of this.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "grid_handle.hpp"
#include "grid_shift.hpp"
#include "k_occupancy.hpp"
#include "occupancy_host.hpp"

using namespace lom;

// Beside the core's (grid_handle.hpp): free / seen hold the counts; the bitmaps are scratch at rest (zero) between calls.
struct lom_occupancy : lom::GridHandle {
    lom_occupancy_geometry geo{};
    lom::DeviceBuf free_votes, seen_votes;  // width * height u32 each
    lom::DeviceBuf free_shadow, seen_shadow;  // where a shift moves them to, from the first shift on (grid_handle.hpp)
    lom::DeviceBuf bitmaps;                 // [scan of a slice][pass, hit][row][word], grow-only
    lom::DeviceBuf cells;                   // start cells of a call
    lom::DeviceBuf cls;                     // the classification, int8 per cell
    uint32_t window = occupancy::kWindowMax;  // LOM_OCC_OPT_TEST_WINDOW (LOM_OCC_OPT_TEST_SLICE_MAX: plan_cap)

    size_t n_cells() const { return (size_t)geo.width * geo.height; }

    // the family's part of the integrate entry points
    using Plan = occupancy::Plan;
    static constexpr const char *kName = "occupancy";
    static constexpr auto kPlan = &occupancy::plan;

    // every slice's walk and fold, then the one read-back: the status words
    int run(const Plan &plan, const float *xyz, uint32_t stride_floats, const lom_occupancy_ray_params &p, lom_occupancy_stats &st)
    {
        int rc;
        uint32_t s_max = 0;
        for (const occupancy::Slice &s : plan.slices) s_max = std::max(s_max, s.count);
        const size_t map_words = occupancy::map_words(geo);
        // grow-only and at rest: a fresh block is zeroed once, in stream order before its first use
        const size_t bm_bytes = (size_t)s_max * 2 * map_words * 4;
        if (bm_bytes > bitmaps.bytes) {
            if ((rc = ensure(this, bitmaps, bm_bytes)) != LOM_OK) return rc;
            LOM_HIP(this, hipMemsetAsync(bitmaps.p, 0, bitmaps.bytes, stream));
        }
        const size_t cell_bytes = plan.cells.size() * 4;
        if ((rc = ensure(this, cells, cell_bytes)) != LOM_OK) return rc;
        if ((rc = grid_stage(this, plan.scans.scans, OW_COUNT)) != LOM_OK) return rc;
        LOM_HIP(this, hipMemcpyAsync(cells.p, plan.cells.data(), cell_bytes, hipMemcpyHostToDevice, stream));
        OccArgs a;
        a.resolution = geo.resolution, a.origin_x = geo.origin_x, a.origin_y = geo.origin_y;
        a.width = geo.width, a.height = geo.height, a.wpr = occupancy::words_per_row(geo.width);
        a.z_lo = p.z_lo, a.z_hi = p.z_hi, a.margin = p.margin, a.min_range = p.min_range, a.max_range = p.max_range;
        a.max_steps = occupancy::max_steps(p.max_range, geo.resolution);
        a.window = window;
        a.stride = stride_floats;
        const size_t lds = (size_t)window * window / 8;
        for (const occupancy::Slice &s : plan.slices) {
            hipLaunchKernelGGL(k_occ_walk, dim3(s.grid_x, s.count), dim3(kAsmThreads), lds, stream,
                               desc.as<const AsmScan>() + s.first, cells.as<const int32_t>() + (size_t)s.first * 2, xyz, a,
                               bitmaps.as<uint32_t>(), words.as<uint32_t>());
            LOM_HIP(this, hipGetLastError());
            if (!s.box.empty()) {
                const uint32_t wx0 = s.box.x0 / 32u, wx1 = (s.box.x1 + 31u) / 32u;
                const size_t threads = (size_t)(wx1 - wx0) * 32u * (s.box.y1 - s.box.y0);
                hipLaunchKernelGGL(k_occ_fold, dim3((uint32_t)((threads + kOccThreads - 1) / kOccThreads)), dim3(kOccThreads), 0,
                                   stream, bitmaps.as<uint32_t>(), s.count, a.width, a.height, a.wpr, wx0, wx1, s.box.y0,
                                   s.box.y1, free_votes.as<uint32_t>(), seen_votes.as<uint32_t>());
                LOM_HIP(this, hipGetLastError());
            }
        }
        if ((rc = grid_read_words(this, OW_COUNT, true)) != LOM_OK) return rc;
        const uint32_t *got = h_words.as<uint32_t>();
        st.rays_walked = u64_of(got, OW_WALKED);
        st.rays_skipped = plan.scans.points_in - st.rays_walked;
        st.cells_visited = u64_of(got, OW_VISITED);
        st.endpoints_marked = u64_of(got, OW_MARKED);
        return LOM_OK;
    }
};

namespace {

thread_local std::string g_occupancy_create_error;

int classify_on_device(lom_occupancy *g, const lom_occupancy_rule *rule)
{
    if (!occupancy::rule_ok(rule)) return fail(g, LOM_ERR_ARG, "occupancy rule: min_free_scans >= 1, min_seen_scans >= 1");
    LOM_HIP(g, hipSetDevice(g->device));
    const uint32_t n = (uint32_t)g->n_cells();
    LOM_HIP(g, hipMemsetAsync(g->words.p, 0, (size_t)OC_COUNT * 4, g->stream));
    hipLaunchKernelGGL(k_occ_classify, dim3((n + kOccThreads - 1) / kOccThreads), dim3(kOccThreads), 0, g->stream,
                       g->free_votes.as<const uint32_t>(), g->seen_votes.as<const uint32_t>(), n, rule->min_free_scans,
                       rule->free_per_seen, rule->min_seen_scans, g->cls.as<int8_t>(), g->words.as<uint32_t>());
    LOM_HIP(g, hipGetLastError());
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_occupancy_create(const lom_occupancy_geometry *geometry, int device, lom_occupancy **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    if (!occupancy::geometry_ok(geometry))
        return create_fail(g_occupancy_create_error, LOM_ERR_ARG,
                           "occupancy geometry: resolution > 0 and finite, a finite origin, 1 <= width, height <= 16384");
    if (const int rc = check_device(device, g_occupancy_create_error); rc != LOM_OK) return rc;
    lom_occupancy *g = new (std::nothrow) lom_occupancy();
    if (!g) return create_fail(g_occupancy_create_error, LOM_ERR_OOM, "host allocation");
    g->device = device;
    g->geo = *geometry;
    const size_t count_bytes = g->n_cells() * 4;
    int rc = grid_setup(g, g_occupancy_create_error, "occupancy grid setup", "hipMalloc (occupancy grid)");
    if (rc == LOM_OK && (alloc(g->free_votes, count_bytes) != hipSuccess || alloc(g->seen_votes, count_bytes) != hipSuccess ||
                         alloc(g->cls, g->n_cells()) != hipSuccess))
        rc = create_fail(g_occupancy_create_error, LOM_ERR_OOM, "hipMalloc (occupancy grid)");
    if (rc == LOM_OK) {
        hipError_t e = hipMemsetAsync(g->free_votes.p, 0, count_bytes, g->stream);
        if (e == hipSuccess) e = hipMemsetAsync(g->seen_votes.p, 0, count_bytes, g->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = create_fail(g_occupancy_create_error, LOM_ERR_HIP, "occupancy grid setup", e);
    }
    if (rc != LOM_OK) {
        lom_occupancy_destroy(g);
        return rc;
    }
    *out = g;
    return LOM_OK;
}

void lom_occupancy_destroy(lom_occupancy *g) { grid_destroy(g); }

const char *lom_occupancy_last_error(const lom_occupancy *g) { return g ? g->error.c_str() : g_occupancy_create_error.c_str(); }

int lom_occupancy_clear(lom_occupancy *g)
{
    if (!g) return LOM_ERR_ARG;
    LOM_HIP(g, hipSetDevice(g->device));
    LOM_HIP(g, hipMemsetAsync(g->free_votes.p, 0, g->n_cells() * 4, g->stream));
    LOM_HIP(g, hipMemsetAsync(g->seen_votes.p, 0, g->n_cells() * 4, g->stream));
    LOM_HIP(g, hipStreamSynchronize(g->stream));
    return LOM_OK;
}

int lom_occupancy_shift(lom_occupancy *g, int32_t dx, int32_t dy)
{
    if (!g) return LOM_ERR_ARG;
    if (!dx && !dy) return LOM_OK;
    GridShift s;
    int rc = grid_shift_plan(g, "occupancy", g->geo, dx, dy, s);
    if (rc != LOM_OK) return rc;
    if (!s.keeps) {
        if ((rc = lom_occupancy_clear(g)) != LOM_OK) return rc;
        g->geo = s.geo;
        return LOM_OK;
    }
    LOM_HIP(g, hipSetDevice(g->device));
    const size_t count_bytes = g->n_cells() * 4;
    if ((rc = grid_shift_shadow(g, g->free_shadow, count_bytes, "hipMalloc (occupancy shift)")) != LOM_OK) return rc;
    if ((rc = grid_shift_shadow(g, g->seen_shadow, count_bytes, "hipMalloc (occupancy shift)")) != LOM_OK) return rc;
    LOM_HIP(g, launch_shift_u32x2(g->stream, g->free_votes.as<const uint32_t>(), g->seen_votes.as<const uint32_t>(),
                                  g->free_shadow.as<uint32_t>(), g->seen_shadow.as<uint32_t>(), g->geo.width, g->geo.height, s.dx, s.dy));
    if ((rc = grid_shift_wait(g)) != LOM_OK) return rc;
    g->free_votes.swap(g->free_shadow), g->seen_votes.swap(g->seen_shadow);
    g->geo = s.geo;
    return LOM_OK;
}

int lom_occupancy_get_geometry(const lom_occupancy *g, lom_occupancy_geometry *out)
{
    if (!g || !out) return LOM_ERR_ARG;
    *out = g->geo;
    return LOM_OK;
}

void *lom_occupancy_stream(lom_occupancy *g) { return g ? (void *)g->stream : nullptr; }
int lom_occupancy_device(const lom_occupancy *g) { return g ? g->device : LOM_ERR_ARG; }
int lom_occupancy_wait_event(lom_occupancy *g, void *hip_event) { return grid_wait_event(g, hip_event); }

int lom_occupancy_set_option(lom_occupancy *g, int option, int64_t value)
{
    if (!g) return LOM_ERR_ARG;
    switch (option) {
    case LOM_OCC_OPT_TEST_SLICE_MAX:
        if (value < 0 || value > (int64_t)occupancy::kSliceScans) return fail(g, LOM_ERR_ARG, "LOM_OCC_OPT_TEST_SLICE_MAX: 0 .. 64");
        g->plan_cap = (uint32_t)value;
        return LOM_OK;
    case LOM_OCC_OPT_TEST_WINDOW:
        if (value > (int64_t)occupancy::kWindowMax || (value > 0 && (value & 31)))
            return fail(g, LOM_ERR_ARG, "LOM_OCC_OPT_TEST_WINDOW: a multiple of 32 up to 512, 0, or < 0 for the default");
        g->window = value < 0 ? occupancy::kWindowMax : (uint32_t)value;
        return LOM_OK;
    default:
        return fail(g, LOM_ERR_ARG, "unknown occupancy option");
    }
}

int lom_occupancy_integrate(lom_occupancy *g, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                            const lom_occupancy_ray_params *p, lom_occupancy_stats *stats)
{
    return grid_integrate(g, a, ids, poses, count, p, stats);
}

int lom_occupancy_integrate_cloud_device(lom_occupancy *g, const float *d_xyz, size_t n, size_t stride_bytes,
                                         const lom_graph_pose *pose, const lom_occupancy_ray_params *p, void *hip_event_or_null,
                                         lom_occupancy_stats *stats)
{
    return grid_integrate_cloud(g, d_xyz, false, n, stride_bytes, pose, p, hip_event_or_null, stats);
}

int lom_occupancy_integrate_cloud(lom_occupancy *g, const float *xyz, size_t n, size_t stride_bytes, const lom_graph_pose *pose,
                                  const lom_occupancy_ray_params *p, lom_occupancy_stats *stats)
{
    return grid_integrate_cloud(g, xyz, true, n, stride_bytes, pose, p, nullptr, stats);
}

int64_t lom_occupancy_counts(lom_occupancy *g, uint32_t *free_out, uint32_t *seen_out, size_t cap)
{
    if (!g) return LOM_ERR_ARG;
    const size_t n = std::min(cap, g->n_cells());
    if (n && (free_out || seen_out)) {
        LOM_HIP(g, hipSetDevice(g->device));
        if (free_out) LOM_HIP(g, hipMemcpyAsync(free_out, g->free_votes.p, n * 4, hipMemcpyDeviceToHost, g->stream));
        if (seen_out) LOM_HIP(g, hipMemcpyAsync(seen_out, g->seen_votes.p, n * 4, hipMemcpyDeviceToHost, g->stream));
        LOM_HIP(g, hipStreamSynchronize(g->stream));
    }
    return (int64_t)g->n_cells();
}

int lom_occupancy_classify(lom_occupancy *g, const lom_occupancy_rule *rule, int8_t *out, size_t cap,
                           lom_occupancy_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!g || (cap && !out)) return LOM_ERR_ARG;
    int rc = classify_on_device(g, rule);
    if (rc != LOM_OK) return rc;
    if ((rc = grid_copy_out(g, out, g->cls, std::min(cap, g->n_cells()), OC_COUNT)) != LOM_OK) return rc;
    if (summary) {
        const uint32_t *t = g->h_words.as<uint32_t>();
        summary->cells_free = t[OC_FREE], summary->cells_occupied = t[OC_OCCUPIED], summary->cells_unknown = t[OC_UNKNOWN];
    }
    return LOM_OK;
}

int lom_occupancy_classify_device(lom_occupancy *g, const lom_occupancy_rule *rule, const int8_t **d_out)
{
    if (!g || !d_out) return LOM_ERR_ARG;
    *d_out = nullptr;
    const int rc = classify_on_device(g, rule);
    if (rc != LOM_OK) return rc;
    *d_out = g->cls.as<const int8_t>();
    return LOM_OK;
}

}  // extern "C"
