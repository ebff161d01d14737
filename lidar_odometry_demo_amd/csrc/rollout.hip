// Trajectory rollouts: K candidate command sequences rolled out from each of M states, the footprint tested at every pose
// against a cost plane, a record per state and candidate on request, and the best candidate per state.
// Definitions: include/lidar_odometry_amd.h ("trajectory rollouts"); the rule of a step and a pose test: rollout_rule.hpp;
// kernels: k_rollout.hpp; host planning (value ranges, the footprint's reach, the staged window, launch shapes, the key)
// and the host-only helpers: rollout_host.cpp; DESIGN.md 7q.  A handle family of its own on the PlaneHandle core
// (plane_handle.hpp); no default path launches any of this.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "k_rollout.hpp"
#include "plane_handle.hpp"
#include "rollout_host.hpp"

using namespace lom;

static_assert(rollout::kThreads == kRolloutThreads && rollout::kKeyIndexBits == kRolloutIndexBits && rollout::kKeyBias == kRolloutKeyBias,
              "rollout_host.hpp and k_rollout.hpp disagree");
static_assert(LOM_NAV_UNREACHED == kRolloutUnreached, "the header and k_rollout.hpp disagree");
static_assert(sizeof(RolloutRecord) == sizeof(lom_rollout_record) && sizeof(RolloutPick) == sizeof(lom_rollout_pick), "the records' layouts");
static_assert(rollout::kWaveLanes * rollout::kWavesDefault <= kRolloutThreads, "the launch bounds of k_rollout_eval");

// The rollout grid owns its stream and every buffer below.
struct lom_rollout : lom::PlaneHandle {  // in_ev: the clearance grid's, the navigation field's
    lom::DeviceBuf plane, potential;      // the host planes of lom_rollout_evaluate, grow-only (planes in HBM are read in place)
    lom::DeviceBuf table;                 // the direction table, filled once
    lom::DeviceBuf states, commands, footprint;  // of the evaluation, grow-only
    lom::DeviceBuf records;               // per state and candidate, under LOM_ROLLOUT_KEEP_RECORDS, grow-only
    lom::DeviceBuf keys, counts;          // per state: the best key (u64), the admissible candidates (u32)
    lom::DeviceBuf out;                   // the summary words, behind them the picks
    lom::PinnedBuf h_out;                 // ... on their way out
    uint32_t waves = rollout::kWavesDefault;  // LOM_ROLLOUT_OPT_TEST_WAVES
    bool serial = false;                      // LOM_ROLLOUT_OPT_TEST_SERIAL
    bool no_lds_plane = true;                 // LOM_ROLLOUT_OPT_TEST_NO_LDS_PLANE: staging lost where it was measured (profiles/rollout_cost.json)
    bool table_there = false;
    std::vector<int32_t> host_table;
    // what the last evaluation left
    size_t m = 0, k = 0;
    bool have_records = false;
    lom_rollout_call_stats stats{};
};

namespace {

thread_local std::string g_rollout_create_error;

constexpr const char *kName = "rollout grid";  // the head of the texts of the plane-handle core

constexpr size_t kOutBytes = (size_t)RW_COUNT * 8 + rollout::kMaxStates * sizeof(lom_rollout_pick);

constexpr const char *kParamsText =
    "rollout parameters: 1 <= segments <= 8, 1 <= steps_per_segment <= 128, 1 <= lethal_min <= 100, -1 <= unknown_cost <= 98, min_steps <= S, "
    "progress_weight <= 256, cost_weight <= 4096, truncation_weight <= 2^20, known flags";

// what a call's inputs are, in every form
struct Inputs {
    const lom_rollout_state *states;
    size_t m;
    const int16_t *commands;
    size_t k;
    const int32_t *footprint;
    size_t f;
    const lom_rollout_params *params;
    lom_rollout_pick *picks;
    lom_rollout_summary *summary;
};

// a refused call zeroes what it would have written
void zero_outputs(const Inputs &in)
{
    if (in.summary) std::memset(in.summary, 0, sizeof *in.summary);
    if (in.picks) std::memset(in.picks, 0, std::min(in.m, rollout::kMaxStates) * sizeof(lom_rollout_pick));
}

// the refusals of every form that need no device: the text, or NULL
const char *evaluate_refusal(bool have_plane, const Inputs &in)
{
    if (!have_plane) return "rollout evaluate: a cost plane";
    if (!rollout::params_ok(in.params)) return kParamsText;
    if (!rollout::counts_ok(in.m, in.k, in.f)) return "rollout evaluate: at most 4096 states, 2^20 candidates, 2^22 of both, 1 to 1024 footprint samples";
    if (in.m && !in.picks) return "rollout evaluate: picks, one per state";
    if (!rollout::states_ok(in.states, in.m)) return "rollout evaluate: states with -2^29 <= x, y < 2^29 and a < 65536";
    if (in.k && !in.commands) return "rollout evaluate: commands";
    if (!rollout::footprint_ok(in.footprint, in.f)) return "rollout evaluate: footprint samples with |fx|, |fy| <= 16384";
    return nullptr;
}

// the blocks of an evaluation, before its first launch
int ensure_evaluate(lom_rollout *r, const Inputs &in, bool host_plane, bool host_potential)
{
    const lom_rollout_params &p = *in.params;
    int rc;
    if ((rc = ensure(r, r->states, std::max<size_t>(in.m, 1) * sizeof(lom_rollout_state))) != LOM_OK ||
        (rc = ensure(r, r->commands, std::max<size_t>(in.k * p.segments, 1) * 4)) != LOM_OK ||
        (rc = ensure(r, r->footprint, in.f * 8)) != LOM_OK || (rc = ensure(r, r->keys, std::max<size_t>(in.m, 1) * 8)) != LOM_OK ||
        (rc = ensure(r, r->counts, std::max<size_t>(in.m, 1) * 4)) != LOM_OK)
        return rc;
    if (host_plane && (rc = ensure(r, r->plane, r->n_cells())) != LOM_OK) return rc;
    if (host_potential && (rc = ensure(r, r->potential, r->n_cells() * 4)) != LOM_OK) return rc;
    if ((p.flags & LOM_ROLLOUT_KEEP_RECORDS) && (rc = ensure(r, r->records, std::max<size_t>(in.m * in.k, 1) * sizeof(RolloutRecord))) != LOM_OK)
        return rc;
    return LOM_OK;
}

template <bool kWindow>
void launch_eval(lom_rollout *r, const rollout::Plan &pl, uint32_t m, const int8_t *d_plane, const uint32_t *d_potential, const RolloutArgs &a)
{
    const dim3 grid(pl.blocks_x, m), block(pl.eval_threads);
    if (r->serial)
        hipLaunchKernelGGL(k_rollout_eval_serial<kWindow>, grid, block, pl.lds_bytes, r->stream, d_plane, d_potential, r->table.as<const int32_t>(),
                           r->states.as<const int32_t>(), r->commands.as<const int16_t>(), r->footprint.as<const int32_t>(), a,
                           r->records.as<RolloutRecord>(), r->keys.as<unsigned long long>(), r->counts.as<uint32_t>());
    else
        hipLaunchKernelGGL(k_rollout_eval<kWindow>, grid, block, pl.lds_bytes, r->stream, d_plane, d_potential, r->table.as<const int32_t>(),
                           r->states.as<const int32_t>(), r->commands.as<const int16_t>(), r->footprint.as<const int32_t>(), a,
                           r->records.as<RolloutRecord>(), r->keys.as<unsigned long long>(), r->counts.as<uint32_t>());
}

// An evaluation over planes in HBM that this stream has been told to wait for: every launch, done_ev behind the last read
// of the planes, the picks' and the summary's way out, one wait.  The arguments are valid and the blocks are there.
int evaluate_on_device(lom_rollout *r, const int8_t *d_plane, const uint32_t *d_potential, const Inputs &in)
{
    const lom_rollout_params &p = *in.params;
    const rollout::Plan pl =
        rollout::plan(p, rollout::reach(in.footprint, in.f), in.m, in.k, in.f, r->waves, r->serial, r->no_lds_plane);
    const RolloutArgs a{r->geo.width, r->geo.height, p.segments, p.steps_per_segment, pl.steps, p.lethal_min, p.unknown_cost, p.min_steps,
                        p.progress_weight, p.cost_weight, p.truncation_weight, (uint32_t)in.k, (uint32_t)in.f, pl.window_side, pl.steps + pl.reach,
                        pl.block_candidates, (p.flags & LOM_ROLLOUT_KEEP_RECORDS) ? 1u : 0u};
    unsigned long long *const words = r->out.as<unsigned long long>();
    RolloutPick *const d_picks = reinterpret_cast<RolloutPick *>(words + RW_COUNT);
    uint64_t launches = 0;
    // the previous evaluation is gone from here on
    r->m = r->k = 0, r->have_records = false;
    if (in.summary) *in.summary = lom_rollout_summary{};
    if (!in.m) {
        r->stats = lom_rollout_call_stats{0, 0};
        return LOM_OK;
    }
    if (!r->table_there) {
        LOM_HIP(r, hipMemcpyAsync(r->table.p, r->host_table.data(), rollout::kTableBytes, hipMemcpyHostToDevice, r->stream));
        r->table_there = true;
    }
    LOM_HIP(r, hipMemcpyAsync(r->states.p, in.states, in.m * sizeof(lom_rollout_state), hipMemcpyHostToDevice, r->stream));
    LOM_HIP(r, hipMemcpyAsync(r->footprint.p, in.footprint, in.f * 8, hipMemcpyHostToDevice, r->stream));
    if (in.k) LOM_HIP(r, hipMemcpyAsync(r->commands.p, in.commands, in.k * p.segments * 4, hipMemcpyHostToDevice, r->stream));
    hipLaunchKernelGGL(k_rollout_fill, dim3(pl.fill_blocks), dim3(kRolloutThreads), 0, r->stream, r->keys.as<unsigned long long>(),
                       r->counts.as<uint32_t>(), (uint32_t)in.m, words);
    LOM_HIP(r, hipGetLastError());
    launches++;
    if (pl.blocks_x) {
        if (pl.window_side)
            launch_eval<true>(r, pl, (uint32_t)in.m, d_plane, d_potential, a);
        else
            launch_eval<false>(r, pl, (uint32_t)in.m, d_plane, d_potential, a);
        LOM_HIP(r, hipGetLastError());
        launches++;
    }
    LOM_HIP(r, hipEventRecord(r->done_ev, r->stream));  // behind the last read of the planes
    hipLaunchKernelGGL(k_rollout_summary, dim3(pl.summary_blocks), dim3(kRolloutThreads), 0, r->stream, r->states.as<const int32_t>(), (uint32_t)in.m,
                       r->geo.width, r->geo.height, r->keys.as<const unsigned long long>(), r->counts.as<const uint32_t>(), d_picks, words);
    LOM_HIP(r, hipGetLastError());
    launches++;
    const size_t out_bytes = (size_t)RW_COUNT * 8 + in.m * sizeof(lom_rollout_pick);
    LOM_HIP(r, hipMemcpyAsync(r->h_out.h, words, out_bytes, hipMemcpyDeviceToHost, r->stream));
    LOM_HIP(r, hipStreamSynchronize(r->stream));
    const unsigned long long *const w = r->h_out.as<unsigned long long>();
    std::memcpy(in.picks, w + RW_COUNT, in.m * sizeof(lom_rollout_pick));
    if (in.summary)
        *in.summary = lom_rollout_summary{in.m, w[RW_VALID], (uint64_t)in.m * in.k, w[RW_ADMISSIBLE], w[RW_NO_PICK]};
    r->m = in.m, r->k = in.k, r->have_records = (p.flags & LOM_ROLLOUT_KEEP_RECORDS) != 0u;
    r->stats = lom_rollout_call_stats{launches, 1};
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_rollout_create(const lom_occupancy_geometry *geometry, int device, lom_rollout **out)
{
    if (!out) return LOM_ERR_ARG;
    lom_rollout *r = nullptr;
    int rc = plane_new(geometry, device, g_rollout_create_error, kName, "rollout grid setup", 2, &r);
    if (rc != LOM_OK) return rc;
    const hipError_t e = alloc(r->h_out, kOutBytes, hipHostMallocDefault);
    if (e != hipSuccess) rc = create_fail(g_rollout_create_error, LOM_ERR_HIP, "rollout grid setup", e);
    if (rc == LOM_OK && (alloc(r->table, rollout::kTableBytes) != hipSuccess || alloc(r->out, kOutBytes) != hipSuccess))
        rc = create_fail(g_rollout_create_error, LOM_ERR_OOM, "hipMalloc (rollout grid)");
    if (rc != LOM_OK) {
        lom_rollout_destroy(r);
        return rc;
    }
    r->host_table.resize((size_t)2 * LOM_ROLLOUT_TABLE);
    rollout::table(r->host_table.data());
    *out = r;
    return LOM_OK;
}

void lom_rollout_destroy(lom_rollout *r) { plane_destroy(r); }
const char *lom_rollout_last_error(const lom_rollout *r) { return plane_last_error(r, g_rollout_create_error); }

int lom_rollout_clear(lom_rollout *r)
{
    if (!r) return LOM_ERR_ARG;
    LOM_HIP(r, hipSetDevice(r->device));
    LOM_HIP(r, hipStreamSynchronize(r->stream));
    r->m = r->k = 0, r->have_records = false;
    return LOM_OK;
}

int lom_rollout_shift(lom_rollout *r, int32_t dx, int32_t dy) { return plane_shift(r, "rollout grid", dx, dy, &lom_rollout_clear); }
int lom_rollout_get_geometry(const lom_rollout *r, lom_occupancy_geometry *out) { return plane_get_geometry(r, out); }
void *lom_rollout_stream(lom_rollout *r) { return plane_stream(r); }
int lom_rollout_device(const lom_rollout *r) { return plane_device(r); }
int lom_rollout_wait_event(lom_rollout *r, void *hip_event) { return plane_wait_event(r, hip_event); }

int lom_rollout_set_option(lom_rollout *r, int option, int64_t value)
{
    if (!r) return LOM_ERR_ARG;
    switch (option) {
    case LOM_ROLLOUT_OPT_TEST_SERIAL:
        if (value > 1) return fail(r, LOM_ERR_ARG, "LOM_ROLLOUT_OPT_TEST_SERIAL: 0, 1, or < 0 for the default");
        r->serial = value == 1;
        return LOM_OK;
    case LOM_ROLLOUT_OPT_TEST_NO_LDS_PLANE:
        if (value > 1) return fail(r, LOM_ERR_ARG, "LOM_ROLLOUT_OPT_TEST_NO_LDS_PLANE: 0, 1, or < 0 for the default");
        r->no_lds_plane = value != 0;
        return LOM_OK;
    case LOM_ROLLOUT_OPT_TEST_WAVES:
        if (value > 0 && !rollout::waves_ok(value)) return fail(r, LOM_ERR_ARG, "LOM_ROLLOUT_OPT_TEST_WAVES: 1, 4, or <= 0 for the default");
        r->waves = value <= 0 ? rollout::kWavesDefault : (uint32_t)value;
        return LOM_OK;
    default:
        return fail(r, LOM_ERR_ARG, "unknown rollout grid option");
    }
}

int lom_rollout_evaluate(lom_rollout *r, const int8_t *cost_plane, const uint32_t *potential, const lom_rollout_state *states, size_t m,
                         const int16_t *commands, size_t k, const int32_t *footprint, size_t f, const lom_rollout_params *params,
                         lom_rollout_pick *picks, lom_rollout_summary *summary)
{
    const Inputs in{states, m, commands, k, footprint, f, params, picks, summary};
    zero_outputs(in);
    if (!r) return LOM_ERR_ARG;
    if (const char *why = evaluate_refusal(cost_plane != nullptr, in)) return fail(r, LOM_ERR_ARG, why);
    LOM_HIP(r, hipSetDevice(r->device));
    if (const int rc = ensure_evaluate(r, in, true, potential != nullptr); rc != LOM_OK) return rc;
    if (m) {
        LOM_HIP(r, hipMemcpyAsync(r->plane.p, cost_plane, r->n_cells(), hipMemcpyHostToDevice, r->stream));
        if (potential) LOM_HIP(r, hipMemcpyAsync(r->potential.p, potential, r->n_cells() * 4, hipMemcpyHostToDevice, r->stream));
    }
    return evaluate_on_device(r, r->plane.as<const int8_t>(), potential ? r->potential.as<const uint32_t>() : nullptr, in);
}

int lom_rollout_evaluate_device(lom_rollout *r, const int8_t *d_cost_plane, void *cost_event, const uint32_t *d_potential, void *potential_event,
                                const lom_rollout_state *states, size_t m, const int16_t *commands, size_t k, const int32_t *footprint, size_t f,
                                const lom_rollout_params *params, lom_rollout_pick *picks, lom_rollout_summary *summary)
{
    const Inputs in{states, m, commands, k, footprint, f, params, picks, summary};
    zero_outputs(in);
    if (!r) return LOM_ERR_ARG;
    if (const char *why = evaluate_refusal(d_cost_plane != nullptr, in)) return fail(r, LOM_ERR_ARG, why);
    LOM_HIP(r, hipSetDevice(r->device));
    if (const int rc = ensure_evaluate(r, in, false, false); rc != LOM_OK) return rc;
    if (cost_event) LOM_HIP(r, hipStreamWaitEvent(r->stream, (hipEvent_t)cost_event, 0));
    if (d_potential && potential_event) LOM_HIP(r, hipStreamWaitEvent(r->stream, (hipEvent_t)potential_event, 0));
    return evaluate_on_device(r, d_cost_plane, d_potential, in);
}

int lom_rollout_evaluate_from_grids(lom_rollout *r, lom_clearance *clearance, lom_navfield *navfield, const lom_rollout_state *states, size_t m,
                                    const int16_t *commands, size_t k, const int32_t *footprint, size_t f, const lom_rollout_params *params,
                                    lom_rollout_pick *picks, lom_rollout_summary *summary)
{
    const Inputs in{states, m, commands, k, footprint, f, params, picks, summary};
    zero_outputs(in);
    if (!r) return LOM_ERR_ARG;
    if (const char *why = evaluate_refusal(clearance != nullptr, in)) return fail(r, LOM_ERR_ARG, why);
    lom_occupancy_geometry cg{}, ng{};  // (one that cannot be read stays zero, which differs)
    (void)lom_clearance_get_geometry(clearance, &cg);
    if (navfield) (void)lom_navfield_get_geometry(navfield, &ng);
    int rc;
    if ((rc = plane_check_producer(r, kName, "clearance grid", cg, lom_clearance_device(clearance))) != LOM_OK ||
        (navfield && (rc = plane_check_producer(r, kName, "navigation field", ng, lom_navfield_device(navfield))) != LOM_OK))
        return rc;
    LOM_HIP(r, hipSetDevice(r->device));
    if ((rc = ensure_evaluate(r, in, false, false)) != LOM_OK) return rc;
    // the hand-off of plane_handle.hpp, once per producer: read behind it, evaluate in place, release to it
    const int8_t *d_cost = nullptr;
    const uint32_t *d_pot = nullptr;
    if (lom_clearance_cost_device(clearance, &d_cost) != LOM_OK || !d_cost)
        return plane_fail_producer(r, kName, "lom_clearance_cost_device", lom_clearance_last_error(clearance));
    if (navfield && (lom_navfield_potential_device(navfield, &d_pot) != LOM_OK || !d_pot))
        return plane_fail_producer(r, kName, "lom_navfield_potential_device", lom_navfield_last_error(navfield));
    if (!m) return evaluate_on_device(r, d_cost, d_pot, in);  // nothing is read: no event either way
    if ((rc = plane_read_behind(r, 0, lom_clearance_stream(clearance))) != LOM_OK) return rc;
    if (navfield && (rc = plane_read_behind(r, 1, lom_navfield_stream(navfield))) != LOM_OK) return rc;
    if ((rc = evaluate_on_device(r, d_cost, d_pot, in)) != LOM_OK) return rc;  // (records done_ev behind its last read)
    if ((rc = plane_release(r, kName, clearance, lom_clearance_wait_event, "lom_clearance_wait_event")) != LOM_OK) return rc;
    return navfield ? plane_release(r, kName, navfield, lom_navfield_wait_event, "lom_navfield_wait_event") : LOM_OK;
}

int lom_rollout_records(lom_rollout *r, lom_rollout_record *out, size_t cap, size_t *count)
{
    if (count) *count = 0;
    if (!r || (cap && !out)) return LOM_ERR_ARG;
    if (r->m && !r->have_records) return fail(r, LOM_ERR_STATE, "rollout records: the last evaluation did not run under LOM_ROLLOUT_KEEP_RECORDS");
    if (const int rc = plane_copy_out(r, out, r->records, std::min(cap, r->m * r->k) * sizeof(lom_rollout_record)); rc != LOM_OK) return rc;
    if (count) *count = r->m * r->k;
    return LOM_OK;
}

int lom_rollout_stats(const lom_rollout *r, lom_rollout_call_stats *out)
{
    if (!r || !out) return LOM_ERR_ARG;
    *out = r->stats;
    return LOM_OK;
}

int lom_rollout_footprint_rectangle(int32_t front, int32_t back, int32_t half_width, int32_t spacing, int perimeter_only, int32_t *out, size_t cap,
                                    size_t *count)
{
    return rollout::footprint_rectangle(front, back, half_width, spacing, perimeter_only != 0, out, cap, count) ? LOM_OK : LOM_ERR_ARG;
}

int lom_rollout_state_from_pose(const lom_occupancy_geometry *geometry, float x_m, float y_m, float yaw, lom_rollout_state *out)
{
    return rollout::state_from_pose(geometry, x_m, y_m, yaw, out) ? LOM_OK : LOM_ERR_ARG;
}

int lom_rollout_poses(const lom_rollout_params *params, const lom_rollout_state *state, const int16_t *commands, lom_rollout_state *out)
{
    return rollout::poses(params, state, commands, out) ? LOM_OK : LOM_ERR_ARG;
}

}  // extern "C"
