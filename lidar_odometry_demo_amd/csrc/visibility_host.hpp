// Host planning of the visibility grid (visibility_host.cpp), shared with visibility.hip.  Plain C++: nothing here needs a
// device or a HIP header.  The value ranges of the geometry, the parameters, the selection and the options, the direction
// table, the words and bytes of a window, the shapes of the launches and the bit budget of the selection's key.
// Definitions: include/lidar_odometry_amd.h ("visibility grid").
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/lidar_odometry_amd.h"
#include "plane_geometry.hpp"

namespace lom {
namespace visibility {

constexpr uint32_t kWaveLanes = 64;
constexpr uint32_t kWavesDefault = 4;          // waves of a workgroup of k_vis_cast: 1 or 4 (LOM_VIS_OPT_TEST_WAVES)
constexpr uint32_t kThreads = 256;             // every other kernel runs workgroups of four waves
constexpr uint32_t kBeamsMin = 4, kBeamsMax = 8192;
constexpr uint32_t kRangeMax = 254;            // R: a window row of 2R + 1 cells fits 16 words
constexpr int32_t kBlockMinLo = 1, kBlockMinHi = 100;
constexpr uint32_t kDepthMax = 65535;
constexpr uint32_t kKnownFlags = LOM_VIS_KEEP_WINDOWS | LOM_VIS_KEEP_BEAMS;
constexpr size_t kMaxViewpoints = (size_t)1 << 20;
constexpr int32_t kTableScale = 32768;         // |direction| in table units
constexpr uint32_t kSelectMax = 1024, kGainWeightMax = 4096, kCostShiftMax = 31;
constexpr uint64_t kMaxWindowBytesDefault = 256ull << 20;
// the key of a selection round: (s + 2^32) << 20 | (2^20 - 1 - k)
constexpr uint32_t kKeyIndexBits = 20;
constexpr uint64_t kKeyIndexMask = (1ull << kKeyIndexBits) - 1u;
constexpr int64_t kKeyBias = (int64_t)1 << 32;

// The window of a viewpoint: 2R + 1 rows of words_per_row u32 around the start cell; bit (ix - x0 + R) & 31 of word
// (ix - x0 + R) >> 5 of row iy - y0 + R.
struct Window {
    uint32_t side;           // 2R + 1
    uint32_t words_per_row;  // ceil(side / 32), 1 .. 16
    uint32_t words;          // side * words_per_row, at most 8144
    uint32_t bytes;          // 4 * words, at most 32576
};

// The shapes of a cast's and a select's launches.
struct Plan {
    Window win;
    uint32_t cast_threads;     // 64 * waves
    uint32_t lds_bytes;        // dynamic LDS of k_vis_cast: the window (0 without it) and the reduction's words, a multiple of 16
    uint32_t summary_blocks;   // workgroups of kThreads lanes over the viewpoints
    uint32_t cover_blocks;     // ... over a window's words
    uint32_t covered_words_per_row, covered_words;  // the covered bitmap: ceil(width / 32) u32 per row
    uint32_t fill_blocks;      // ... and the workgroups that zero it
};

using plane::geometry_ok;  // the rule of all four planning grids
// 4 <= beams <= 8192, range_cells <= 254, 1 <= block_min <= 100, unknown_depth <= 65535, known flags only
bool params_ok(const lom_visibility_params *p);
// 1 <= n <= 1024, 1 <= gain_weight <= 4096, cost_shift <= 31, min_gain >= 1
bool select_ok(const lom_visibility_select_params *s);
bool waves_ok(int64_t waves);  // 1, 4
// Step 1: beam b of `beams` is (lround(cos(2 pi b / beams) * 32768), lround(sin(2 pi b / beams) * 32768)), computed in
// f64; out: 2 * beams int32.  false: beams out of range.
bool table(uint32_t beams, int32_t *out);
Window window(uint32_t range_cells);
// the bytes of k windows (k <= 2^20: below 2^35)
uint64_t windows_bytes(size_t k, uint32_t range_cells);
Plan plan(uint32_t width, uint32_t height, uint32_t range_cells, uint32_t waves, bool no_lds, size_t k);
// workgroups of kThreads lanes for n lanes (at least one)
uint32_t blocks_for(uint64_t n);
// The greatest gain times the greatest weight, and the score's range: g <= 509^2 < 2^18, weight <= 2^12, so
// -(2^32 - 1) <= s <= 2^30 and 1 <= s + 2^32 < 2^33: the key stays below 2^53 and is never 0.
int64_t score(uint32_t gain, uint32_t gain_weight, uint32_t cost, uint32_t cost_shift);
uint64_t key_of(int64_t s, uint32_t k);
uint32_t key_index(uint64_t key);
int64_t key_score(uint64_t key);

}  // namespace visibility
}  // namespace lom
