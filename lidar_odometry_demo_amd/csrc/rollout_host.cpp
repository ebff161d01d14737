// Host planning of lom_rollout_*: value ranges, the footprint's reach, the staged window, the shapes of the launches, the
// score and its key, and the host-only helpers.  Plain C++, no HIP: rollout.hip calls these, and tests/cpp/test_rollout.cpp
// compiles this file with visibility_host.cpp (the table's one home) alone.
#include "rollout_host.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#include "rollout_rule.hpp"
#include "visibility_host.hpp"

namespace lom {
namespace rollout {

static_assert(sizeof(lom_rollout_params) == 36 && sizeof(lom_rollout_state) == 12 && sizeof(lom_rollout_record) == 32 &&
                  sizeof(lom_rollout_pick) == 16 && sizeof(lom_rollout_summary) == 40 && sizeof(lom_rollout_call_stats) == 16,
              "the layouts the header documents");
static_assert(LOM_ROLLOUT_TABLE == kRolloutTable && (kAngles >> kRolloutAngleShift) == kRolloutTable, "an angle reads entry a >> 4 of 4096");
static_assert((int)LOM_ROLLOUT_OK == (int)ROLLOUT_OK && (int)LOM_ROLLOUT_UNKNOWN == (int)ROLLOUT_UNKNOWN &&
                  (int)LOM_ROLLOUT_COLLISION == (int)ROLLOUT_COLLISION && (int)LOM_ROLLOUT_EDGE == (int)ROLLOUT_EDGE &&
                  (int)LOM_ROLLOUT_INVALID == (int)ROLLOUT_INVALID,
              "the header and rollout_rule.hpp disagree");
// the key's bit budget (rollout_host.hpp, step 4)
static_assert((uint64_t)kProgressWeightMax << 32 <= 1ull << 40 && (uint64_t)kCostWeightMax * (kStepsMax + 1) * 99 < 1ull << 29 &&
                  (uint64_t)kTruncationWeightMax * (kStepsMax + 1) < 1ull << 31,
              "|s| < 2^41");
static_assert(kMaxCandidates <= (1ull << kKeyIndexBits), "a candidate's index fits the key");
static_assert(kSegmentsMax * kStepsPerSegmentMax == kStepsMax, "S <= 1024 is the product of the two ranges");

bool params_ok(const lom_rollout_params *p)
{
    if (!p || p->segments < 1u || p->segments > kSegmentsMax || p->steps_per_segment < 1u || p->steps_per_segment > kStepsPerSegmentMax) return false;
    const uint32_t S = p->segments * p->steps_per_segment;
    return S <= kStepsMax && p->lethal_min >= kLethalMinLo && p->lethal_min <= kLethalMinHi && p->unknown_cost >= kUnknownCostLo &&
           p->unknown_cost <= kUnknownCostHi && p->min_steps <= S && p->progress_weight <= kProgressWeightMax &&
           p->cost_weight <= kCostWeightMax && p->truncation_weight <= kTruncationWeightMax && (p->flags & ~kKnownFlags) == 0u;
}

bool waves_ok(int64_t waves) { return waves == 1 || waves == 4; }

bool counts_ok(size_t m, size_t k, size_t f)
{
    return m <= kMaxStates && k <= kMaxCandidates && (uint64_t)m * k <= kMaxRecords && f >= 1u && f <= kMaxSamples;
}

bool states_ok(const lom_rollout_state *states, size_t m)
{
    if (m && !states) return false;
    for (size_t i = 0; i < m; i++)
        if (states[i].x < kPositionLo || states[i].x > kPositionHi || states[i].y < kPositionLo || states[i].y > kPositionHi || states[i].a >= kAngles)
            return false;
    return true;
}

bool footprint_ok(const int32_t *footprint, size_t f)
{
    if (!footprint || f < 1u || f > kMaxSamples) return false;
    for (size_t i = 0; i < 2 * f; i++)
        if (footprint[i] < -kSampleMax || footprint[i] > kSampleMax) return false;
    return true;
}

uint32_t reach(const int32_t *footprint, size_t f)
{
    uint32_t r = 0;
    for (size_t i = 0; i < f; i++) {
        const uint32_t l1 = (uint32_t)std::abs(footprint[2 * i]) + (uint32_t)std::abs(footprint[2 * i + 1]);
        r = std::max(r, (l1 + 255u) / 256u + 1u);
    }
    return r;
}

void table(int32_t *out) { (void)visibility::table(kRolloutTable, out); }

uint32_t blocks_for(uint64_t n) { return n ? (uint32_t)((n + kThreads - 1u) / kThreads) : 1u; }

Plan plan(const lom_rollout_params &p, uint32_t reach_cells, size_t m, size_t k, size_t f, uint32_t waves, bool serial, bool no_lds_plane)
{
    Plan pl{};
    pl.steps = p.segments * p.steps_per_segment;
    pl.reach = reach_cells;
    const uint64_t side = 2ull * (pl.steps + reach_cells) + 1ull;
    pl.window_side = (!no_lds_plane && side * side <= kWindowBudgetBytes) ? (uint32_t)side : 0u;
    pl.eval_threads = serial ? kThreads : kWaveLanes * waves;
    pl.block_candidates = serial ? kThreads : waves * kCandidatesPerWave;
    pl.blocks_x = k && m ? (uint32_t)((k + pl.block_candidates - 1u) / pl.block_candidates) : 0u;
    // the reduction's words; the window; and, in the lane-per-pose form, the table and the footprint
    const uint32_t window_bytes = (pl.window_side * pl.window_side + 15u) & ~15u;
    pl.lds_bytes = 128u + window_bytes + (serial ? 0u : kTableBytes + (uint32_t)f * 8u);
    pl.fill_blocks = pl.summary_blocks = blocks_for(m);
    return pl;
}

bool admissible(const lom_rollout_params &p, bool have_potential, uint32_t p0, const lom_rollout_record &r)
{
    if (r.free_poses <= p.min_steps) return false;
    return !have_potential || (p0 != LOM_NAV_UNREACHED && r.end_potential != LOM_NAV_UNREACHED);
}

int64_t score(const lom_rollout_params &p, bool have_potential, uint32_t p0, const lom_rollout_record &r)
{
    const int64_t S = (int64_t)p.segments * p.steps_per_segment;
    const int64_t progress = have_potential ? (int64_t)p.progress_weight * ((int64_t)p0 - (int64_t)r.end_potential) : 0;
    return progress - (int64_t)p.cost_weight * (int64_t)r.cost_sum - (int64_t)p.truncation_weight * (S + 1 - (int64_t)r.free_poses);
}

uint64_t key_of(int64_t s, uint32_t k) { return ((uint64_t)(s + kKeyBias) << kKeyIndexBits) | (kKeyIndexMask - k); }
uint32_t key_index(uint64_t key) { return (uint32_t)(kKeyIndexMask - (key & kKeyIndexMask)); }
int64_t key_score(uint64_t key) { return (int64_t)(key >> kKeyIndexBits) - kKeyBias; }

namespace {

// -lo, -lo + spacing, ... while < hi, then hi
std::vector<int32_t> axis(int32_t lo, int32_t hi, int32_t spacing)
{
    std::vector<int32_t> v;
    for (int32_t a = -lo; a < hi; a += spacing) v.push_back(a);
    v.push_back(hi);
    return v;
}

}  // namespace

bool footprint_rectangle(int32_t front, int32_t back, int32_t half_width, int32_t spacing, bool perimeter_only, int32_t *out, size_t cap,
                         size_t *count)
{
    if (count) *count = 0;
    if (!count || (cap && !out) || front < 0 || front > kSampleMax || back < 0 || back > kSampleMax || half_width < 0 ||
        half_width > kSampleMax || spacing < 1)
        return false;
    // at most 2^15 / spacing + 2 per axis; a count beyond 1024 is refused before the lattice is made
    // (summed in 64 bits: spacing may be INT32_MAX)
    const uint64_t sp = (uint64_t)spacing, nx = ((uint64_t)front + (uint64_t)back + sp - 1u) / sp + 1u,
                   ny = (2u * (uint64_t)half_width + sp - 1u) / sp + 1u;
    const uint64_t n = perimeter_only && nx > 2u && ny > 2u ? 2u * nx + 2u * (ny - 2u) : nx * ny;
    if (n > kMaxSamples) return false;
    const std::vector<int32_t> xs = axis(back, front, spacing), ys = axis(half_width, half_width, spacing);
    size_t written = 0;
    for (size_t i = 0; i < xs.size(); i++)
        for (size_t j = 0; j < ys.size(); j++) {
            if (perimeter_only && i != 0 && i + 1 != xs.size() && j != 0 && j + 1 != ys.size()) continue;
            if (written < cap) out[2 * written] = xs[i], out[2 * written + 1] = ys[j];
            written++;
        }
    *count = written;
    return true;
}

bool state_from_pose(const lom_occupancy_geometry *g, float x_m, float y_m, float yaw, lom_rollout_state *out)
{
    if (!geometry_ok(g) || !out || !std::isfinite(x_m) || !std::isfinite(y_m) || !std::isfinite(yaw)) return false;
    const double x = std::floor(((double)x_m - (double)g->origin_x) / (double)g->resolution * 32768.0);
    const double y = std::floor(((double)y_m - (double)g->origin_y) / (double)g->resolution * 32768.0);
    if (!(x >= (double)kPositionLo && x <= (double)kPositionHi && y >= (double)kPositionLo && y <= (double)kPositionHi)) return false;
    const double turns = (double)yaw / 6.283185307179586476925286766559 * 65536.0;
    if (!(std::fabs(turns) < 9.0e18)) return false;  // llround's range
    out->x = (int32_t)x, out->y = (int32_t)y;
    out->a = (uint32_t)((unsigned long long)std::llround(turns) & 65535ull);
    return true;
}

bool poses(const lom_rollout_params *p, const lom_rollout_state *state, const int16_t *commands, lom_rollout_state *out)
{
    if (!params_ok(p) || !states_ok(state, 1) || !state || !commands || !out) return false;
    static const std::vector<int32_t> tab = [] {
        std::vector<int32_t> t(2 * kRolloutTable);
        table(t.data());
        return t;
    }();
    const uint32_t S = p->segments * p->steps_per_segment;
    int32_t x = state->x, y = state->y;
    uint32_t a = state->a;
    out[0] = *state;
    for (uint32_t t = 0; t < S; t++) {
        const uint32_t l = t / p->steps_per_segment, b = a >> kRolloutAngleShift;
        const int32_t v = commands[2 * l], w = commands[2 * l + 1];
        x += rollout_increment(v, tab[2 * b]), y += rollout_increment(v, tab[2 * b + 1]);
        a = (uint32_t)((int32_t)a + w) & kRolloutAngleMask;
        out[t + 1] = lom_rollout_state{x, y, a};
    }
    return true;
}

}  // namespace rollout
}  // namespace lom
