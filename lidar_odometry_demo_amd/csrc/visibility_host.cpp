// Host planning of lom_visibility_*: value ranges, the direction table, the words of a window, the shapes of the launches
// and the selection's key.  Plain C++, no HIP: visibility.hip calls these, and tests/cpp/test_visibility.cpp compiles this
// file alone.
#include "visibility_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace visibility {

static_assert(sizeof(lom_visibility_params) == 20 && sizeof(lom_visibility_record) == 32 && sizeof(lom_visibility_summary) == 40 &&
                  sizeof(lom_visibility_select_params) == 16 && sizeof(lom_visibility_pick) == 16 && sizeof(lom_visibility_call_stats) == 16,
              "the layouts the header documents");
// the key's bit budget: the greatest gain is a full window of unknown cells
static_assert((uint64_t)(2u * kRangeMax + 1u) * (2u * kRangeMax + 1u) * kGainWeightMax <= (1ull << 30), "g * gain_weight <= 2^30");
static_assert(kMaxViewpoints <= (1ull << kKeyIndexBits), "a viewpoint's index fits the key");

bool params_ok(const lom_visibility_params *p)
{
    return p && p->beams >= kBeamsMin && p->beams <= kBeamsMax && p->range_cells <= kRangeMax && p->block_min >= kBlockMinLo &&
           p->block_min <= kBlockMinHi && p->unknown_depth <= kDepthMax && (p->flags & ~kKnownFlags) == 0u;
}

bool select_ok(const lom_visibility_select_params *s)
{
    return s && s->n >= 1u && s->n <= kSelectMax && s->gain_weight >= 1u && s->gain_weight <= kGainWeightMax &&
           s->cost_shift <= kCostShiftMax && s->min_gain >= 1u;
}

bool waves_ok(int64_t waves) { return waves == 1 || waves == 4; }

bool table(uint32_t beams, int32_t *out)
{
    if (beams < kBeamsMin || beams > kBeamsMax || !out) return false;
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t b = 0; b < beams; b++) {
        const double a = two_pi * (double)b / (double)beams;
        out[2 * b] = (int32_t)std::lround(std::cos(a) * (double)kTableScale);
        out[2 * b + 1] = (int32_t)std::lround(std::sin(a) * (double)kTableScale);
    }
    return true;
}

Window window(uint32_t range_cells)
{
    Window w;
    w.side = 2u * range_cells + 1u;
    w.words_per_row = (w.side + 31u) / 32u;
    w.words = w.side * w.words_per_row;
    w.bytes = 4u * w.words;
    return w;
}

uint64_t windows_bytes(size_t k, uint32_t range_cells) { return (uint64_t)k * window(range_cells).bytes; }

uint32_t blocks_for(uint64_t n) { return n ? (uint32_t)((n + kThreads - 1u) / kThreads) : 1u; }

Plan plan(uint32_t width, uint32_t height, uint32_t range_cells, uint32_t waves, bool no_lds, size_t k)
{
    Plan p;
    p.win = window(range_cells);
    p.cast_threads = kWaveLanes * waves;
    p.lds_bytes = 128u + (no_lds ? 0u : (p.win.bytes + 15u) & ~15u);
    p.summary_blocks = blocks_for(k);
    p.cover_blocks = blocks_for(p.win.words);
    p.covered_words_per_row = (width + 31u) / 32u;
    p.covered_words = p.covered_words_per_row * height;  // at most 256 * 8192
    p.fill_blocks = blocks_for(p.covered_words);
    return p;
}

int64_t score(uint32_t gain, uint32_t gain_weight, uint32_t cost, uint32_t cost_shift)
{
    return (int64_t)gain * (int64_t)gain_weight - (int64_t)(cost >> cost_shift);
}

uint64_t key_of(int64_t s, uint32_t k) { return ((uint64_t)(s + kKeyBias) << kKeyIndexBits) | (kKeyIndexMask - k); }
uint32_t key_index(uint64_t key) { return (uint32_t)(kKeyIndexMask - (key & kKeyIndexMask)); }
int64_t key_score(uint64_t key) { return (int64_t)(key >> kKeyIndexBits) - kKeyBias; }

}  // namespace visibility
}  // namespace lom
