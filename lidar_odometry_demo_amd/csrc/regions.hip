// Region grid: the connected regions of a grid plane labelled on the device, a record per region, a ranked goal list.
// Definitions: include/lidar_odometry_amd.h ("frontier regions"); kernels: k_regions.hpp; host planning (value ranges,
// launch shapes, the list sort): regions_host.cpp; DESIGN.md 7n.  A handle family of its own on the PlaneHandle core
// (plane_handle.hpp); no default path launches any of this.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "k_regions.hpp"
#include "occupancy_host.hpp"
#include "plane_handle.hpp"
#include "regions_host.hpp"

using namespace lom;

static_assert(regions::kThreads == kRegThreads && regions::kTileCols == kRegTileCols && regions::kTileRowsMax == kRegTileRowsMax &&
                  regions::kScanWords == kRegScanWords && regions::kBandRows == kRegAccRows,
              "regions_host.hpp and k_regions.hpp disagree");
static_assert(LOM_REGIONS_NONE == kRegNone && LOM_NAV_UNREACHED == kRegUnreached && LOM_REGIONS_BYTES == 0 &&
                  LOM_REGIONS_NEIGHBOURS_8 == 1 && LOM_REGIONS_EDGE_UNKNOWN == 2,
              "the header and k_regions.hpp disagree");
static_assert(sizeof(RegRecord) == sizeof(lom_regions_record), "the record's layout");

// The region grid owns its stream and every buffer below.
struct lom_regions : lom::PlaneHandle {  // in_ev: the occupancy grid's, the clearance grid's, the navigation field's
    lom::DeviceBuf labels;                    // u32 per cell
    lom::DeviceBuf number;                    // u32 per cell: a root's dense number
    lom::DeviceBuf bitmap, rootbits;          // u64 words, row-aligned: the members, the roots
    lom::DeviceBuf prefix, block_sums;        // the scan of the root bitmap
    lom::DeviceBuf words;                     // the summary words
    lom::DeviceBuf acc, records;              // per recorded region, grow-only
    lom::DeviceBuf in_plane, in_cost, in_pot; // an extract's host planes on the device, grow-only
    lom::DeviceBuf q_xy, q_out;               // a query's points and results, grow-only
    lom::PinnedBuf h_words;                   // the summary words on their way out
    uint64_t max_regions = regions::kMaxRegionsDefault;  // LOM_REGIONS_OPT_MAX_REGIONS
    uint32_t tile_rows = regions::kTileRowsDefault;      // LOM_REGIONS_OPT_TEST_TILE_ROWS
    bool no_tiles = false, no_wave_merge = false;        // LOM_REGIONS_OPT_TEST_NO_TILES, _NO_WAVE_MERGE
    // what the last extract left
    lom_regions_summary summary{};
    lom_regions_extract_stats stats{};
    uint32_t list_min_cells = 1;
    int list_rank = LOM_REGIONS_RANK_LABEL;
    bool list_ready = true;                   // host_records and order hold the last extract's list
    std::vector<lom_regions_record> host_records;
    std::vector<uint32_t> order;

    RegArgs args() const { return RegArgs{geo.width, geo.height, (geo.width + 63u) / 64u}; }
};

namespace {

thread_local std::string g_regions_create_error;

constexpr const char *kName = "region grid";  // the head of the texts of the plane-handle core

constexpr const char *kParamsText =
    "region parameters: a known kind, lo <= hi under LOM_REGIONS_BYTES, 0 <= max_cost <= 99, min_cells >= 1, a known rank "
    "(LOM_REGIONS_RANK_POTENTIAL only with a potential), known flags";

// no member, no region, an empty list
int reset(lom_regions *r)
{
    LOM_HIP(r, hipMemsetAsync(r->labels.p, 0xFF, r->n_cells() * 4, r->stream));
    LOM_HIP(r, hipStreamSynchronize(r->stream));
    r->summary = lom_regions_summary{};
    r->host_records.clear(), r->order.clear();
    r->list_ready = true;
    return LOM_OK;
}

// the refusals of every extract form that need no device: the text, or NULL
const char *extract_refusal(bool have_plane, bool have_potential, const lom_regions_params *p)
{
    if (!have_plane) return "region extract: a plane";
    if (!regions::params_ok(p, have_potential)) return kParamsText;
    return nullptr;
}

// An extract over planes in HBM that this stream may read now: every launch, the summary's way out, one wait.  The
// arguments are valid.
int extract_on_device(lom_regions *r, const int8_t *d_plane, const int8_t *d_cost, const uint32_t *d_pot, const lom_regions_params &p,
                      lom_regions_summary *summary)
{
    const regions::Plan pl = regions::plan(r->geo.width, r->geo.height, r->tile_rows, r->no_tiles);
    const uint32_t cap = regions::record_cap(r->max_regions, r->geo.width, r->geo.height);
    // what can still fail for want of memory comes first: a refused call changes nothing
    int rc;
    if ((rc = ensure(r, r->acc, (size_t)cap * sizeof(RegAcc))) != LOM_OK || (rc = ensure(r, r->records, (size_t)cap * sizeof(RegRecord))) != LOM_OK)
        return rc;
    const RegArgs a = r->args();
    const dim3 rows(pl.row_blocks, r->geo.height), bands(pl.row_blocks, pl.bands), threads(kRegThreads);
    const uint32_t conn4 = (p.flags & LOM_REGIONS_CONNECT_4) ? 1u : 0u, wave_merge = r->no_wave_merge ? 0u : 1u;
    uint32_t *const L = r->labels.as<uint32_t>(), *const number = r->number.as<uint32_t>(), *const words = r->words.as<uint32_t>();
    unsigned long long *const bitmap = r->bitmap.as<unsigned long long>(), *const rootbits = r->rootbits.as<unsigned long long>();
    RegAcc *const acc = r->acc.as<RegAcc>();
    uint64_t launches = 0;
    // the previous list is gone from here on
    r->list_ready = false;
    r->summary = lom_regions_summary{};
    r->host_records.clear(), r->order.clear();
    LOM_HIP(r, hipMemsetAsync(words, 0, (size_t)RW_COUNT * 4, r->stream));
    hipLaunchKernelGGL(k_reg_mask, rows, threads, 0, r->stream, d_plane, d_cost, d_pot, a, (int)p.kind, (int)p.lo, (int)p.hi, (int)p.max_cost,
                       p.flags, bitmap, L);
    LOM_HIP(r, hipGetLastError());
    launches++;
    if (pl.n_tiles) {
        hipLaunchKernelGGL(k_reg_label_tile, dim3(pl.tiles_x, pl.tiles_y), threads, 0, r->stream, bitmap, a, pl.tile_rows, conn4, L);
        LOM_HIP(r, hipGetLastError());
        launches++;
    }
    if (pl.row_lanes + pl.col_lanes) {
        hipLaunchKernelGGL(k_reg_merge, dim3(regions::blocks_for(pl.row_lanes + pl.col_lanes)), threads, 0, r->stream, a, pl.tile_cols,
                           pl.tile_rows, (uint32_t)pl.row_lanes, (uint32_t)pl.col_lanes, conn4, L);
        LOM_HIP(r, hipGetLastError());
        launches++;
    }
    hipLaunchKernelGGL(k_reg_flatten, rows, threads, 0, r->stream, a, L, rootbits);
    LOM_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(k_reg_scan_partial, dim3(pl.scan_blocks), threads, 0, r->stream, rootbits, bitmap, pl.words, r->prefix.as<uint32_t>(),
                       r->block_sums.as<uint32_t>(), words);
    LOM_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(k_reg_scan_top, dim3(1), threads, 0, r->stream, pl.scan_blocks, r->block_sums.as<uint32_t>(), words);
    LOM_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(k_reg_number, rows, threads, 0, r->stream, a, rootbits, r->prefix.as<const uint32_t>(),
                       r->block_sums.as<const uint32_t>(), cap, number, acc);
    LOM_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(k_reg_accumulate, bands, threads, 0, r->stream, a, L, number, cap, wave_merge, acc);
    LOM_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(k_reg_centroid, dim3(regions::blocks_for(cap)), threads, 0, r->stream, words, cap, acc);
    LOM_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(k_reg_centre, bands, threads, 0, r->stream, a, L, number, d_pot, cap, wave_merge, acc);
    LOM_HIP(r, hipGetLastError());
    hipLaunchKernelGGL(k_reg_record, dim3(regions::blocks_for(cap)), threads, 0, r->stream, a, acc, cap, p.min_cells, d_pot ? 1u : 0u,
                       r->records.as<RegRecord>(), words);
    LOM_HIP(r, hipGetLastError());
    launches += 8;
    LOM_HIP(r, hipMemcpyAsync(r->h_words.h, words, (size_t)RW_COUNT * 4, hipMemcpyDeviceToHost, r->stream));
    LOM_HIP(r, hipEventRecord(r->done_ev, r->stream));
    LOM_HIP(r, hipStreamSynchronize(r->stream));
    const uint32_t *const w = r->h_words.as<uint32_t>();
    r->summary.cells_member = w[RW_MEMBER], r->summary.regions = w[RW_REGIONS];
    r->summary.regions_recorded = std::min(w[RW_REGIONS], cap);
    r->summary.regions_listed = w[RW_LISTED], r->summary.largest_cells = w[RW_LARGEST];
    r->list_min_cells = p.min_cells, r->list_rank = p.rank;
    r->stats = lom_regions_extract_stats{launches, 1, pl.n_tiles};
    if (summary) *summary = r->summary;
    return LOM_OK;
}

// the last extract's records on the host and the list's order, fetched and sorted on first use
int ready_list(lom_regions *r)
{
    if (r->list_ready) return LOM_OK;
    const size_t n = (size_t)r->summary.regions_recorded;
    r->host_records.resize(n);
    if (const int rc = plane_copy_out(r, r->host_records.data(), r->records, n * sizeof(lom_regions_record)); rc != LOM_OK) return rc;
    regions::sort_list(r->host_records.data(), n, r->list_min_cells, r->list_rank, r->order);
    r->list_ready = true;
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_regions_create(const lom_occupancy_geometry *geometry, int device, lom_regions **out)
{
    if (!out) return LOM_ERR_ARG;
    lom_regions *r = nullptr;
    int rc = plane_new(geometry, device, g_regions_create_error, kName, "region grid setup", 3, &r);
    if (rc != LOM_OK) return rc;
    const regions::Plan pl = regions::plan(geometry->width, geometry->height, regions::kTileRowsDefault, false);
    const hipError_t e = alloc(r->h_words, 64, hipHostMallocDefault);
    if (e != hipSuccess) rc = create_fail(g_regions_create_error, LOM_ERR_HIP, "region grid setup", e);
    const size_t n = r->n_cells();
    if (rc == LOM_OK &&
        (alloc(r->labels, n * 4) != hipSuccess || alloc(r->number, n * 4) != hipSuccess || alloc(r->bitmap, (size_t)pl.words * 8) != hipSuccess ||
         alloc(r->rootbits, (size_t)pl.words * 8) != hipSuccess || alloc(r->prefix, (size_t)pl.words * 4) != hipSuccess ||
         alloc(r->block_sums, (size_t)kRegScanWords * 4) != hipSuccess || alloc(r->words, 64) != hipSuccess))
        rc = create_fail(g_regions_create_error, LOM_ERR_OOM, "hipMalloc (region grid)");
    if (rc == LOM_OK && reset(r) != LOM_OK) rc = create_fail(g_regions_create_error, LOM_ERR_HIP, r->error.c_str());
    if (rc != LOM_OK) {
        lom_regions_destroy(r);
        return rc;
    }
    *out = r;
    return LOM_OK;
}

void lom_regions_destroy(lom_regions *r) { plane_destroy(r); }
const char *lom_regions_last_error(const lom_regions *r) { return plane_last_error(r, g_regions_create_error); }

int lom_regions_clear(lom_regions *r)
{
    if (!r) return LOM_ERR_ARG;
    LOM_HIP(r, hipSetDevice(r->device));
    return reset(r);
}

int lom_regions_shift(lom_regions *r, int32_t dx, int32_t dy) { return plane_shift(r, "region grid", dx, dy, &lom_regions_clear); }
int lom_regions_get_geometry(const lom_regions *r, lom_occupancy_geometry *out) { return plane_get_geometry(r, out); }
void *lom_regions_stream(lom_regions *r) { return plane_stream(r); }
int lom_regions_device(const lom_regions *r) { return plane_device(r); }
int lom_regions_wait_event(lom_regions *r, void *hip_event) { return plane_wait_event(r, hip_event); }

int lom_regions_set_option(lom_regions *r, int option, int64_t value)
{
    if (!r) return LOM_ERR_ARG;
    switch (option) {
    case LOM_REGIONS_OPT_MAX_REGIONS:
        if (value > (int64_t)regions::kMaxRegionsMax) return fail(r, LOM_ERR_ARG, "LOM_REGIONS_OPT_MAX_REGIONS: 1 .. 2^26, or <= 0 for the default");
        r->max_regions = value <= 0 ? regions::kMaxRegionsDefault : (uint64_t)value;
        return LOM_OK;
    case LOM_REGIONS_OPT_TEST_TILE_ROWS:
        if (value > 0 && !regions::tile_rows_ok(value)) return fail(r, LOM_ERR_ARG, "LOM_REGIONS_OPT_TEST_TILE_ROWS: 1, 8, 32, or <= 0 for the default");
        r->tile_rows = value <= 0 ? regions::kTileRowsDefault : (uint32_t)value;
        return LOM_OK;
    case LOM_REGIONS_OPT_TEST_NO_TILES:
        if (value > 1) return fail(r, LOM_ERR_ARG, "LOM_REGIONS_OPT_TEST_NO_TILES: 0, 1, or < 0 for the default");
        r->no_tiles = value == 1;
        return LOM_OK;
    case LOM_REGIONS_OPT_TEST_NO_WAVE_MERGE:
        if (value > 1) return fail(r, LOM_ERR_ARG, "LOM_REGIONS_OPT_TEST_NO_WAVE_MERGE: 0, 1, or < 0 for the default");
        r->no_wave_merge = value == 1;
        return LOM_OK;
    default:
        return fail(r, LOM_ERR_ARG, "unknown region grid option");
    }
}

int lom_regions_extract_device(lom_regions *r, const int8_t *d_plane, const int8_t *d_cost, const uint32_t *d_potential,
                               void *hip_event_or_null, const lom_regions_params *params, lom_regions_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!r) return LOM_ERR_ARG;
    if (const char *why = extract_refusal(d_plane != nullptr, d_potential != nullptr, params)) return fail(r, LOM_ERR_ARG, why);
    LOM_HIP(r, hipSetDevice(r->device));
    if (hip_event_or_null) LOM_HIP(r, hipStreamWaitEvent(r->stream, (hipEvent_t)hip_event_or_null, 0));
    return extract_on_device(r, d_plane, d_cost, d_potential, *params, summary);
}

int lom_regions_extract(lom_regions *r, const int8_t *plane, const int8_t *cost, const uint32_t *potential,
                        const lom_regions_params *params, lom_regions_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!r) return LOM_ERR_ARG;
    if (const char *why = extract_refusal(plane != nullptr, potential != nullptr, params)) return fail(r, LOM_ERR_ARG, why);
    LOM_HIP(r, hipSetDevice(r->device));
    const size_t n = r->n_cells();
    int rc;
    if ((rc = ensure(r, r->in_plane, n)) != LOM_OK || (cost && (rc = ensure(r, r->in_cost, n)) != LOM_OK) ||
        (potential && (rc = ensure(r, r->in_pot, n * 4)) != LOM_OK))
        return rc;
    LOM_HIP(r, hipMemcpyAsync(r->in_plane.p, plane, n, hipMemcpyHostToDevice, r->stream));
    if (cost) LOM_HIP(r, hipMemcpyAsync(r->in_cost.p, cost, n, hipMemcpyHostToDevice, r->stream));
    if (potential) LOM_HIP(r, hipMemcpyAsync(r->in_pot.p, potential, n * 4, hipMemcpyHostToDevice, r->stream));
    return extract_on_device(r, r->in_plane.as<const int8_t>(), cost ? r->in_cost.as<const int8_t>() : nullptr,
                             potential ? r->in_pot.as<const uint32_t>() : nullptr, *params, summary);
}

int lom_regions_extract_from_grids(lom_regions *r, lom_occupancy *occupancy, const lom_occupancy_rule *rule, lom_clearance *clearance,
                                   lom_navfield *navfield, const lom_regions_params *params, lom_regions_summary *summary)
{
    if (summary) std::memset(summary, 0, sizeof *summary);
    if (!r) return LOM_ERR_ARG;
    if (const char *why = extract_refusal(occupancy != nullptr, navfield != nullptr, params)) return fail(r, LOM_ERR_ARG, why);
    if (!occupancy::rule_ok(rule))
        return fail(r, LOM_ERR_ARG, "occupancy rule: min_free_scans >= 1, min_seen_scans >= 1");
    // every producer's geometry first, then one text for the devices: the core's check is given this grid's own device
    lom_occupancy_geometry og{}, cg{}, ng{};  // (one that cannot be read stays zero, which differs)
    (void)lom_occupancy_get_geometry(occupancy, &og);
    if (clearance) (void)lom_clearance_get_geometry(clearance, &cg);
    if (navfield) (void)lom_navfield_get_geometry(navfield, &ng);
    int rc;
    if ((rc = plane_check_producer(r, kName, "occupancy grid", og, r->device)) != LOM_OK ||
        (clearance && (rc = plane_check_producer(r, kName, "clearance grid", cg, r->device)) != LOM_OK) ||
        (navfield && (rc = plane_check_producer(r, kName, "navigation field", ng, r->device)) != LOM_OK))
        return rc;
    if (lom_occupancy_device(occupancy) != r->device || (clearance && lom_clearance_device(clearance) != r->device) ||
        (navfield && lom_navfield_device(navfield) != r->device))
        return fail(r, LOM_ERR_ARG, "region grid: a grid lives on another device");
    LOM_HIP(r, hipSetDevice(r->device));
    // the hand-off of plane_handle.hpp, once per producer: read behind it, extract, release to it
    const int8_t *d_plane = nullptr, *d_cost = nullptr;
    const uint32_t *d_pot = nullptr;
    if (lom_occupancy_classify_device(occupancy, rule, &d_plane) != LOM_OK || !d_plane)
        return plane_fail_producer(r, kName, "lom_occupancy_classify_device", lom_occupancy_last_error(occupancy));
    if ((rc = plane_read_behind(r, 0, lom_occupancy_stream(occupancy))) != LOM_OK) return rc;
    if (clearance) {
        if (lom_clearance_cost_device(clearance, &d_cost) != LOM_OK || !d_cost)
            return plane_fail_producer(r, kName, "lom_clearance_cost_device", lom_clearance_last_error(clearance));
        if ((rc = plane_read_behind(r, 1, lom_clearance_stream(clearance))) != LOM_OK) return rc;
    }
    if (navfield) {
        if (lom_navfield_potential_device(navfield, &d_pot) != LOM_OK || !d_pot)
            return plane_fail_producer(r, kName, "lom_navfield_potential_device", lom_navfield_last_error(navfield));
        if ((rc = plane_read_behind(r, 2, lom_navfield_stream(navfield))) != LOM_OK) return rc;
    }
    if ((rc = extract_on_device(r, d_plane, d_cost, d_pot, *params, summary)) != LOM_OK) return rc;
    if ((rc = plane_release(r, kName, occupancy, lom_occupancy_wait_event, "lom_occupancy_wait_event")) != LOM_OK) return rc;
    if (clearance && (rc = plane_release(r, kName, clearance, lom_clearance_wait_event, "lom_clearance_wait_event")) != LOM_OK) return rc;
    return navfield ? plane_release(r, kName, navfield, lom_navfield_wait_event, "lom_navfield_wait_event") : LOM_OK;
}

int lom_regions_labels(lom_regions *r, uint32_t *out, size_t cap)
{
    if (!r || (cap && !out)) return LOM_ERR_ARG;
    return plane_copy_out(r, out, r->labels, std::min(cap, r->n_cells()) * 4);
}

int lom_regions_labels_device(lom_regions *r, const uint32_t **d_out)
{
    if (!r || !d_out) return LOM_ERR_ARG;
    *d_out = r->labels.as<const uint32_t>();
    return LOM_OK;
}

int lom_regions_list(lom_regions *r, lom_regions_record *out, size_t cap, size_t *listed)
{
    if (listed) *listed = 0;
    if (!r || (cap && !out)) return LOM_ERR_ARG;
    if (const int rc = ready_list(r); rc != LOM_OK) return rc;
    const size_t n = std::min(cap, r->order.size());
    for (size_t i = 0; i < n; i++) out[i] = r->host_records[r->order[i]];
    if (listed) *listed = r->order.size();
    return LOM_OK;
}

int lom_regions_goals(lom_regions *r, int which, int32_t *out, size_t cap, size_t *listed)
{
    if (listed) *listed = 0;
    if (!r || (cap && !out)) return LOM_ERR_ARG;
    if (which != LOM_REGIONS_GOAL_CENTRE && which != LOM_REGIONS_GOAL_ENTRY)
        return fail(r, LOM_ERR_ARG, "region goals: LOM_REGIONS_GOAL_CENTRE or LOM_REGIONS_GOAL_ENTRY");
    if (const int rc = ready_list(r); rc != LOM_OK) return rc;
    const size_t n = std::min(cap, r->order.size());
    for (size_t i = 0; i < n; i++) {
        const lom_regions_record &g = r->host_records[r->order[i]];
        out[2 * i] = which == LOM_REGIONS_GOAL_CENTRE ? g.centre_x : g.entry_x;
        out[2 * i + 1] = which == LOM_REGIONS_GOAL_CENTRE ? g.centre_y : g.entry_y;
    }
    if (listed) *listed = r->order.size();
    return LOM_OK;
}

int lom_regions_query(lom_regions *r, const float *xy, size_t n, uint32_t *out)
{
    if (!r) return LOM_ERR_ARG;
    if ((n && !xy) || n > regions::kMaxQueryPoints) return fail(r, LOM_ERR_ARG, "region query: points, at most 2^30 of them");
    if (!n || !out) return LOM_OK;
    LOM_HIP(r, hipSetDevice(r->device));
    int rc;
    if ((rc = ensure(r, r->q_xy, n * 8)) != LOM_OK || (rc = ensure(r, r->q_out, n * 4)) != LOM_OK) return rc;
    LOM_HIP(r, hipMemcpyAsync(r->q_xy.p, xy, n * 8, hipMemcpyHostToDevice, r->stream));
    hipLaunchKernelGGL(k_reg_query, dim3(regions::blocks_for(n)), dim3(kRegThreads), 0, r->stream, r->q_xy.as<const float>(), (uint32_t)n,
                       r->geo.resolution, r->geo.origin_x, r->geo.origin_y, r->args(), r->labels.as<const uint32_t>(), r->q_out.as<uint32_t>());
    LOM_HIP(r, hipGetLastError());
    LOM_HIP(r, hipMemcpyAsync(out, r->q_out.p, n * 4, hipMemcpyDeviceToHost, r->stream));
    LOM_HIP(r, hipStreamSynchronize(r->stream));
    return LOM_OK;
}

int lom_regions_stats(const lom_regions *r, lom_regions_extract_stats *out)
{
    if (!r || !out) return LOM_ERR_ARG;
    *out = r->stats;
    return LOM_OK;
}

}  // extern "C"
