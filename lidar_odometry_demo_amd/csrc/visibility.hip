// Visibility grid: rays cast over a grid plane from many viewpoints at once, a record per viewpoint, a simulated scan and
// the window of unknown cells each sees on request, and a greedy next-best-view selection over those windows.
// Definitions: include/lidar_odometry_amd.h ("visibility grid"); kernels: k_visibility.hpp; host planning (value ranges,
// the table, window sizes, launch shapes, the key): visibility_host.cpp; DESIGN.md 7o.  A handle family of its own on the
// PlaneHandle core (plane_handle.hpp); no default path launches any of this.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "k_visibility.hpp"
#include "occupancy_host.hpp"
#include "plane_handle.hpp"
#include "visibility_host.hpp"

using namespace lom;

static_assert(visibility::kThreads == kVisThreads && visibility::kKeyIndexBits == kVisIndexBits, "visibility_host.hpp and k_visibility.hpp disagree");
static_assert(LOM_NAV_UNREACHED == kVisUnreached && LOM_VIS_END_INVALID == VIS_INVALID && LOM_VIS_END_EDGE == VIS_EDGE &&
                  LOM_VIS_END_RANGE == VIS_RANGE && LOM_VIS_END_HIT == VIS_HIT && LOM_VIS_END_UNKNOWN == VIS_UNKNOWN &&
                  LOM_VIS_END_CORNER == VIS_CORNER,
              "the header and k_visibility.hpp disagree");
static_assert(sizeof(VisRecord) == sizeof(lom_visibility_record) && sizeof(VisPick) == sizeof(lom_visibility_pick), "the records' layouts");

// The visibility grid owns its stream and every buffer below.
struct lom_visibility : lom::PlaneHandle {  // in_ev: the producer's of the call, the occupancy grid's or the navigation field's
    lom::DeviceBuf plane;                     // its own copy of the last cast's plane, i8 per cell
    lom::DeviceBuf table;                     // the direction table of table_beams beams, grow-only
    lom::DeviceBuf viewpoints, records;       // per viewpoint, grow-only
    lom::DeviceBuf beams, windows;            // per viewpoint and beam, per viewpoint and window word, grow-only
    lom::DeviceBuf covered;                   // the covered bitmap of a selection, u32 words, row-aligned
    lom::DeviceBuf picked, gain, cost;        // per viewpoint, of a selection, grow-only
    lom::DeviceBuf keys;                      // per round: the keys (u64), behind them the picks
    lom::DeviceBuf words;                     // the summary words
    lom::PinnedBuf h_words;                   // the summary words, or a selection's keys and picks, on their way out
    uint64_t max_window_bytes = visibility::kMaxWindowBytesDefault;  // LOM_VIS_OPT_MAX_WINDOW_BYTES
    uint32_t waves = visibility::kWavesDefault;                      // LOM_VIS_OPT_TEST_WAVES
    bool no_lds = false;                                             // LOM_VIS_OPT_TEST_NO_LDS
    uint32_t table_beams = 0;
    std::vector<int32_t> host_table;
    // what the last cast left
    size_t k = 0;
    lom_visibility_params params{};
    bool have_windows = false, have_beams = false;
    lom_visibility_summary summary{};
    lom_visibility_call_stats stats{};
};

namespace {

thread_local std::string g_visibility_create_error;

constexpr const char *kName = "visibility grid";  // the head of the texts of the plane-handle core

constexpr size_t kPinnedBytes = (size_t)visibility::kSelectMax * (8 + sizeof(lom_visibility_pick));

constexpr const char *kParamsText =
    "visibility parameters: 4 <= beams <= 8192, range_cells <= 254, 1 <= block_min <= 100, unknown_depth <= 65535, known flags";
constexpr const char *kSelectText = "visibility select: 1 <= n <= 1024, 1 <= gain_weight <= 4096, cost_shift <= 31, min_gain >= 1";

// the refusals of every cast form that need no device: the text, or NULL
const char *cast_refusal(const lom_visibility *v, bool have_plane, const int32_t *viewpoints, size_t k, const lom_visibility_params *p)
{
    if (!have_plane) return "visibility cast: a plane";
    if ((k && !viewpoints) || k > visibility::kMaxViewpoints) return "visibility cast: viewpoints, at most 2^20 of them";
    if (!visibility::params_ok(p)) return kParamsText;
    if (((p->flags & LOM_VIS_KEEP_WINDOWS) || v->no_lds) && visibility::windows_bytes(k, p->range_cells) > v->max_window_bytes)
        return "visibility cast: the windows would exceed LOM_VIS_OPT_MAX_WINDOW_BYTES";
    return nullptr;
}

// the blocks of a cast, before its first launch
int ensure_cast(lom_visibility *v, size_t k, const lom_visibility_params &p)
{
    const bool windows = (p.flags & LOM_VIS_KEEP_WINDOWS) || v->no_lds;
    int rc;
    if ((rc = ensure(v, v->viewpoints, std::max<size_t>(k, 1) * 8)) != LOM_OK || (rc = ensure(v, v->records, std::max<size_t>(k, 1) * sizeof(VisRecord))) != LOM_OK ||
        (rc = ensure(v, v->table, (size_t)p.beams * 8)) != LOM_OK)
        return rc;
    if ((p.flags & LOM_VIS_KEEP_BEAMS) && (rc = ensure(v, v->beams, std::max<size_t>(k * p.beams, 1) * 4)) != LOM_OK) return rc;
    if (windows && (rc = ensure(v, v->windows, std::max<size_t>((size_t)visibility::windows_bytes(k, p.range_cells), 4))) != LOM_OK) return rc;
    if (v->table_beams != p.beams) {
        v->host_table.resize((size_t)2 * p.beams);
        visibility::table(p.beams, v->host_table.data());
        v->table_beams = 0;  // (until the copy below is enqueued)
    }
    return LOM_OK;
}

VisArgs args_of(const lom_visibility *v, const lom_visibility_params &p, const visibility::Plan &pl)
{
    return VisArgs{v->geo.width, v->geo.height, p.beams, p.range_cells, p.unknown_depth, p.block_min, pl.win.words_per_row, pl.win.words,
                   (p.flags & LOM_VIS_KEEP_WINDOWS) ? 1u : 0u, (p.flags & LOM_VIS_KEEP_BEAMS) ? 1u : 0u, pl.covered_words_per_row};
}

// A cast over the handle's copy of the plane, which this stream has been told to fill: every launch, the summary's way
// out, one wait.  The arguments are valid and the blocks are there.
int cast_on_device(lom_visibility *v, const int32_t *viewpoints, size_t k, const lom_visibility_params &p, lom_visibility_summary *summary)
{
    const visibility::Plan pl = visibility::plan(v->geo.width, v->geo.height, p.range_cells, v->waves, v->no_lds, k);
    const VisArgs a = args_of(v, p, pl);
    const bool windows = (p.flags & LOM_VIS_KEEP_WINDOWS) || v->no_lds;
    unsigned long long *const words = v->words.as<unsigned long long>();
    uint64_t launches = 0;
    // the previous cast is gone from here on
    v->k = 0, v->have_windows = v->have_beams = false;
    v->summary = lom_visibility_summary{};
    if (v->table_beams != p.beams) {
        LOM_HIP(v, hipMemcpyAsync(v->table.p, v->host_table.data(), (size_t)p.beams * 8, hipMemcpyHostToDevice, v->stream));
        v->table_beams = p.beams;
    }
    LOM_HIP(v, hipMemsetAsync(words, 0, (size_t)VW_COUNT * 8, v->stream));
    if (k) {
        LOM_HIP(v, hipMemcpyAsync(v->viewpoints.p, viewpoints, k * 8, hipMemcpyHostToDevice, v->stream));
        if (v->no_lds) LOM_HIP(v, hipMemsetAsync(v->windows.p, 0, (size_t)visibility::windows_bytes(k, p.range_cells), v->stream));
        uint32_t *const d_beams = (p.flags & LOM_VIS_KEEP_BEAMS) ? v->beams.as<uint32_t>() : nullptr;
        uint32_t *const d_windows = windows ? v->windows.as<uint32_t>() : nullptr;
        if (v->no_lds)
            hipLaunchKernelGGL(k_vis_cast<false>, dim3((uint32_t)k), dim3(pl.cast_threads), pl.lds_bytes, v->stream, v->plane.as<const int8_t>(),
                               v->table.as<const int32_t>(), v->viewpoints.as<const int32_t>(), a, v->records.as<VisRecord>(), d_beams, d_windows);
        else
            hipLaunchKernelGGL(k_vis_cast<true>, dim3((uint32_t)k), dim3(pl.cast_threads), pl.lds_bytes, v->stream, v->plane.as<const int8_t>(),
                               v->table.as<const int32_t>(), v->viewpoints.as<const int32_t>(), a, v->records.as<VisRecord>(), d_beams, d_windows);
        LOM_HIP(v, hipGetLastError());
        hipLaunchKernelGGL(k_vis_summary, dim3(pl.summary_blocks), dim3(kVisThreads), 0, v->stream, v->records.as<const VisRecord>(), (uint32_t)k, words);
        LOM_HIP(v, hipGetLastError());
        launches += 2;
    }
    LOM_HIP(v, hipMemcpyAsync(v->h_words.h, words, (size_t)VW_COUNT * 8, hipMemcpyDeviceToHost, v->stream));
    LOM_HIP(v, hipStreamSynchronize(v->stream));
    const unsigned long long *const w = v->h_words.as<unsigned long long>();
    v->summary.viewpoints = k, v->summary.valid = w[VW_VALID], v->summary.unknown_total = w[VW_UNKNOWN];
    if (w[VW_KEY]) {
        v->summary.unknown_max = (w[VW_KEY] >> kVisIndexBits) - 1u;
        v->summary.unknown_argmax = kVisIndexMask - (w[VW_KEY] & kVisIndexMask);
    }
    v->k = k, v->params = p;
    v->have_windows = (p.flags & LOM_VIS_KEEP_WINDOWS) != 0u, v->have_beams = (p.flags & LOM_VIS_KEEP_BEAMS) != 0u;
    v->stats = lom_visibility_call_stats{launches, 1};
    if (summary) *summary = v->summary;
    return LOM_OK;
}

// the refusals of both select forms: the status and the text, or LOM_OK
int select_refusal(lom_visibility *v, const lom_visibility_select_params *s, const lom_visibility_pick *out, const size_t *picked)
{
    if (!visibility::select_ok(s)) return fail(v, LOM_ERR_ARG, kSelectText);
    if (!out || !picked) return fail(v, LOM_ERR_ARG, "visibility select: an output of n entries and a count");
    if (!v->have_windows) return fail(v, LOM_ERR_STATE, "visibility select: the last cast did not run under LOM_VIS_KEEP_WINDOWS");
    return LOM_OK;
}

int ensure_select(lom_visibility *v, const lom_visibility_select_params &s)
{
    const size_t k = std::max<size_t>(v->k, 1);
    int rc;
    if ((rc = ensure(v, v->picked, k * 4)) != LOM_OK || (rc = ensure(v, v->gain, k * 4)) != LOM_OK || (rc = ensure(v, v->cost, k * 4)) != LOM_OK ||
        (rc = ensure(v, v->keys, (size_t)s.n * (8 + sizeof(VisPick)))) != LOM_OK)
        return rc;
    return LOM_OK;
}

// A selection over the last cast's windows; d_cost: the handle's cost block, filled on this stream, or NULL.  All n
// rounds are enqueued ahead; a round behind an ended selection returns at once; one wait.
int select_on_device(lom_visibility *v, const lom_visibility_select_params &s, const uint32_t *d_cost, uint64_t launches_before,
                     lom_visibility_pick *out, size_t *picked)
{
    const size_t k = v->k;
    const visibility::Plan pl = visibility::plan(v->geo.width, v->geo.height, v->params.range_cells, v->waves, v->no_lds, k);
    const VisArgs a = args_of(v, v->params, pl);
    unsigned long long *const keys = v->keys.as<unsigned long long>();
    VisPick *const picks = reinterpret_cast<VisPick *>(keys + s.n);
    const size_t out_bytes = (size_t)s.n * (8 + sizeof(VisPick));
    uint64_t launches = launches_before;
    LOM_HIP(v, hipMemsetAsync(keys, 0, out_bytes, v->stream));
    hipLaunchKernelGGL(k_vis_fill, dim3(std::max(pl.fill_blocks, visibility::blocks_for(k))), dim3(kVisThreads), 0, v->stream, v->covered.as<uint32_t>(),
                       pl.covered_words, v->picked.as<uint32_t>(), (uint32_t)k);
    LOM_HIP(v, hipGetLastError());
    launches++;
    const VisRecord *const records = v->records.as<const VisRecord>();
    const uint32_t *const windows = v->windows.as<const uint32_t>();
    for (uint32_t round = 0; round < s.n; round++) {
        hipLaunchKernelGGL(k_vis_marginal, dim3((uint32_t)k), dim3(kVisThreads), 0, v->stream, round, keys, records, windows,
                           v->covered.as<const uint32_t>(), v->picked.as<const uint32_t>(), a, v->gain.as<uint32_t>());
        LOM_HIP(v, hipGetLastError());
        hipLaunchKernelGGL(k_vis_pick, dim3(visibility::blocks_for(k)), dim3(kVisThreads), 0, v->stream, round, keys, records, (uint32_t)k,
                           v->picked.as<const uint32_t>(), v->gain.as<const uint32_t>(), d_cost, s.gain_weight, s.cost_shift, s.min_gain);
        LOM_HIP(v, hipGetLastError());
        hipLaunchKernelGGL(k_vis_cover, dim3(pl.cover_blocks), dim3(kVisThreads), 0, v->stream, round, keys, records, windows, v->covered.as<uint32_t>(),
                           v->picked.as<uint32_t>(), v->gain.as<const uint32_t>(), a, picks);
        LOM_HIP(v, hipGetLastError());
        launches += 3;
    }
    LOM_HIP(v, hipMemcpyAsync(v->h_words.h, keys, out_bytes, hipMemcpyDeviceToHost, v->stream));
    LOM_HIP(v, hipStreamSynchronize(v->stream));
    const unsigned long long *const h_keys = v->h_words.as<unsigned long long>();
    const lom_visibility_pick *const h_picks = reinterpret_cast<const lom_visibility_pick *>(h_keys + s.n);
    size_t n = 0;
    while (n < s.n && h_keys[n]) n++;
    std::memcpy(out, h_picks, n * sizeof(lom_visibility_pick));
    *picked = n;
    v->stats = lom_visibility_call_stats{launches, 1};
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_visibility_create(const lom_occupancy_geometry *geometry, int device, lom_visibility **out)
{
    if (!out) return LOM_ERR_ARG;
    lom_visibility *v = nullptr;
    int rc = plane_new(geometry, device, g_visibility_create_error, kName, "visibility grid setup", 1, &v);
    if (rc != LOM_OK) return rc;
    const visibility::Plan pl = visibility::plan(geometry->width, geometry->height, 0, visibility::kWavesDefault, false, 0);
    const hipError_t e = alloc(v->h_words, kPinnedBytes, hipHostMallocDefault);
    if (e != hipSuccess) rc = create_fail(g_visibility_create_error, LOM_ERR_HIP, "visibility grid setup", e);
    if (rc == LOM_OK && (alloc(v->plane, v->n_cells()) != hipSuccess || alloc(v->covered, (size_t)pl.covered_words * 4) != hipSuccess ||
                         alloc(v->words, (size_t)VW_COUNT * 8) != hipSuccess))
        rc = create_fail(g_visibility_create_error, LOM_ERR_OOM, "hipMalloc (visibility grid)");
    if (rc != LOM_OK) {
        lom_visibility_destroy(v);
        return rc;
    }
    *out = v;
    return LOM_OK;
}

void lom_visibility_destroy(lom_visibility *v) { plane_destroy(v); }
const char *lom_visibility_last_error(const lom_visibility *v) { return plane_last_error(v, g_visibility_create_error); }

int lom_visibility_clear(lom_visibility *v)
{
    if (!v) return LOM_ERR_ARG;
    LOM_HIP(v, hipSetDevice(v->device));
    LOM_HIP(v, hipStreamSynchronize(v->stream));
    v->k = 0, v->have_windows = v->have_beams = false;
    v->summary = lom_visibility_summary{};
    return LOM_OK;
}

int lom_visibility_shift(lom_visibility *v, int32_t dx, int32_t dy) { return plane_shift(v, "visibility grid", dx, dy, &lom_visibility_clear); }
int lom_visibility_get_geometry(const lom_visibility *v, lom_occupancy_geometry *out) { return plane_get_geometry(v, out); }
void *lom_visibility_stream(lom_visibility *v) { return plane_stream(v); }
int lom_visibility_device(const lom_visibility *v) { return plane_device(v); }
int lom_visibility_wait_event(lom_visibility *v, void *hip_event) { return plane_wait_event(v, hip_event); }

int lom_visibility_set_option(lom_visibility *v, int option, int64_t value)
{
    if (!v) return LOM_ERR_ARG;
    switch (option) {
    case LOM_VIS_OPT_TEST_NO_LDS:
        if (value > 1) return fail(v, LOM_ERR_ARG, "LOM_VIS_OPT_TEST_NO_LDS: 0, 1, or < 0 for the default");
        v->no_lds = value == 1;
        return LOM_OK;
    case LOM_VIS_OPT_TEST_WAVES:
        if (value > 0 && !visibility::waves_ok(value)) return fail(v, LOM_ERR_ARG, "LOM_VIS_OPT_TEST_WAVES: 1, 4, or <= 0 for the default");
        v->waves = value <= 0 ? visibility::kWavesDefault : (uint32_t)value;
        return LOM_OK;
    case LOM_VIS_OPT_MAX_WINDOW_BYTES:
        v->max_window_bytes = value <= 0 ? visibility::kMaxWindowBytesDefault : (uint64_t)value;
        return LOM_OK;
    default:
        return fail(v, LOM_ERR_ARG, "unknown visibility grid option");
    }
}

int lom_visibility_table(uint32_t beams, int32_t *out) { return visibility::table(beams, out) ? LOM_OK : LOM_ERR_ARG; }

int lom_visibility_cast_device(lom_visibility *v, const int8_t *d_plane, void *hip_event_or_null, const int32_t *viewpoints, size_t k,
                               const lom_visibility_params *params, lom_visibility_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!v) return LOM_ERR_ARG;
    if (const char *why = cast_refusal(v, d_plane != nullptr, viewpoints, k, params)) return fail(v, LOM_ERR_ARG, why);
    LOM_HIP(v, hipSetDevice(v->device));
    if (const int rc = ensure_cast(v, k, *params); rc != LOM_OK) return rc;
    if (hip_event_or_null) LOM_HIP(v, hipStreamWaitEvent(v->stream, (hipEvent_t)hip_event_or_null, 0));
    LOM_HIP(v, hipMemcpyAsync(v->plane.p, d_plane, v->n_cells(), hipMemcpyDeviceToDevice, v->stream));
    return cast_on_device(v, viewpoints, k, *params, summary);
}

int lom_visibility_cast(lom_visibility *v, const int8_t *plane, const int32_t *viewpoints, size_t k, const lom_visibility_params *params,
                        lom_visibility_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!v) return LOM_ERR_ARG;
    if (const char *why = cast_refusal(v, plane != nullptr, viewpoints, k, params)) return fail(v, LOM_ERR_ARG, why);
    LOM_HIP(v, hipSetDevice(v->device));
    if (const int rc = ensure_cast(v, k, *params); rc != LOM_OK) return rc;
    LOM_HIP(v, hipMemcpyAsync(v->plane.p, plane, v->n_cells(), hipMemcpyHostToDevice, v->stream));
    return cast_on_device(v, viewpoints, k, *params, summary);
}

int lom_visibility_cast_from_occupancy(lom_visibility *v, lom_occupancy *occupancy, const lom_occupancy_rule *rule, const int32_t *viewpoints,
                                       size_t k, const lom_visibility_params *params, lom_visibility_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!v) return LOM_ERR_ARG;
    if (const char *why = cast_refusal(v, occupancy != nullptr, viewpoints, k, params)) return fail(v, LOM_ERR_ARG, why);
    if (!occupancy::rule_ok(rule)) return fail(v, LOM_ERR_ARG, "occupancy rule: min_free_scans >= 1, min_seen_scans >= 1");
    lom_occupancy_geometry g{};
    (void)lom_occupancy_get_geometry(occupancy, &g);
    int rc = plane_check_producer(v, kName, "occupancy grid", g, lom_occupancy_device(occupancy));
    if (rc != LOM_OK) return rc;
    LOM_HIP(v, hipSetDevice(v->device));
    if ((rc = ensure_cast(v, k, *params)) != LOM_OK) return rc;
    // the hand-off of plane_handle.hpp: read behind the occupancy grid -- a copy of its plane -- and release to it at once
    const int8_t *d_plane = nullptr;
    if (lom_occupancy_classify_device(occupancy, rule, &d_plane) != LOM_OK || !d_plane)
        return plane_fail_producer(v, kName, "lom_occupancy_classify_device", lom_occupancy_last_error(occupancy));
    if ((rc = plane_read_behind(v, 0, lom_occupancy_stream(occupancy))) != LOM_OK) return rc;
    LOM_HIP(v, hipMemcpyAsync(v->plane.p, d_plane, v->n_cells(), hipMemcpyDeviceToDevice, v->stream));
    LOM_HIP(v, hipEventRecord(v->done_ev, v->stream));
    if ((rc = plane_release(v, kName, occupancy, lom_occupancy_wait_event, "lom_occupancy_wait_event")) != LOM_OK) return rc;
    return cast_on_device(v, viewpoints, k, *params, summary);
}

int lom_visibility_records(lom_visibility *v, lom_visibility_record *out, size_t cap, size_t *count)
{
    if (count) *count = 0;
    if (!v || (cap && !out)) return LOM_ERR_ARG;
    if (const int rc = plane_copy_out(v, out, v->records, std::min(cap, v->k) * sizeof(lom_visibility_record)); rc != LOM_OK) return rc;
    if (count) *count = v->k;
    return LOM_OK;
}

int lom_visibility_beams(lom_visibility *v, uint32_t *out, size_t cap)
{
    if (!v || (cap && !out)) return LOM_ERR_ARG;
    if (!v->have_beams) return fail(v, LOM_ERR_STATE, "visibility beams: the last cast did not run under LOM_VIS_KEEP_BEAMS");
    return plane_copy_out(v, out, v->beams, std::min(cap, v->k * v->params.beams) * 4);
}

int lom_visibility_windows_device(lom_visibility *v, const uint32_t **d_out, size_t *words_per_window)
{
    if (!v || !d_out) return LOM_ERR_ARG;
    *d_out = nullptr;
    if (words_per_window) *words_per_window = 0;
    if (!v->have_windows) return fail(v, LOM_ERR_STATE, "visibility windows: the last cast did not run under LOM_VIS_KEEP_WINDOWS");
    *d_out = v->windows.as<const uint32_t>();
    if (words_per_window) *words_per_window = visibility::window(v->params.range_cells).words;
    return LOM_OK;
}

int lom_visibility_windows(lom_visibility *v, uint32_t *out, size_t cap, size_t *words_per_window)
{
    if (words_per_window) *words_per_window = 0;
    if (!v || (cap && !out)) return LOM_ERR_ARG;
    if (!v->have_windows) return fail(v, LOM_ERR_STATE, "visibility windows: the last cast did not run under LOM_VIS_KEEP_WINDOWS");
    const size_t words = visibility::window(v->params.range_cells).words, n = std::min(cap, v->k * words);
    if (words_per_window) *words_per_window = words;
    return plane_copy_out(v, out, v->windows, n * 4);
}

int lom_visibility_select(lom_visibility *v, const lom_visibility_select_params *select, const uint32_t *cost, lom_visibility_pick *out,
                          size_t *picked)
{
    if (picked) *picked = 0;
    if (!v) return LOM_ERR_ARG;
    if (const int rc = select_refusal(v, select, out, picked); rc != LOM_OK) return rc;
    if (!v->k) {
        v->stats = lom_visibility_call_stats{0, 0};
        return LOM_OK;
    }
    LOM_HIP(v, hipSetDevice(v->device));
    if (const int rc = ensure_select(v, *select); rc != LOM_OK) return rc;
    if (cost) {
        LOM_HIP(v, hipMemcpyAsync(v->cost.p, cost, v->k * 4, hipMemcpyHostToDevice, v->stream));
    }
    return select_on_device(v, *select, cost ? v->cost.as<const uint32_t>() : nullptr, 0, out, picked);
}

int lom_visibility_select_from_navfield(lom_visibility *v, lom_navfield *navfield, const lom_visibility_select_params *select,
                                        lom_visibility_pick *out, size_t *picked)
{
    if (picked) *picked = 0;
    if (!v) return LOM_ERR_ARG;
    if (!navfield) return fail(v, LOM_ERR_ARG, "visibility select: a navigation field");
    if (const int rc = select_refusal(v, select, out, picked); rc != LOM_OK) return rc;
    lom_occupancy_geometry g{};
    (void)lom_navfield_get_geometry(navfield, &g);
    if (const int rc = plane_check_producer(v, kName, "navigation field", g, lom_navfield_device(navfield)); rc != LOM_OK) return rc;
    if (!v->k) {
        v->stats = lom_visibility_call_stats{0, 0};
        return LOM_OK;
    }
    LOM_HIP(v, hipSetDevice(v->device));
    if (const int rc = ensure_select(v, *select); rc != LOM_OK) return rc;
    const uint32_t *d_pot = nullptr;
    if (lom_navfield_potential_device(navfield, &d_pot) != LOM_OK || !d_pot)
        return plane_fail_producer(v, kName, "lom_navfield_potential_device", lom_navfield_last_error(navfield));
    if (const int rc = plane_read_behind(v, 0, lom_navfield_stream(navfield)); rc != LOM_OK) return rc;
    hipLaunchKernelGGL(k_vis_costs, dim3(visibility::blocks_for(v->k)), dim3(kVisThreads), 0, v->stream, v->viewpoints.as<const int32_t>(), (uint32_t)v->k,
                       v->geo.width, v->geo.height, d_pot, v->cost.as<uint32_t>());
    LOM_HIP(v, hipGetLastError());
    // what the field does next to its potential comes behind that read
    LOM_HIP(v, hipEventRecord(v->done_ev, v->stream));
    if (const int rc = plane_release(v, kName, navfield, lom_navfield_wait_event, "lom_navfield_wait_event"); rc != LOM_OK) return rc;
    return select_on_device(v, *select, v->cost.as<const uint32_t>(), 1, out, picked);
}

int lom_visibility_stats(const lom_visibility *v, lom_visibility_call_stats *out)
{
    if (!v || !out) return LOM_ERR_ARG;
    *out = v->stats;
    return LOM_OK;
}

}  // extern "C"
