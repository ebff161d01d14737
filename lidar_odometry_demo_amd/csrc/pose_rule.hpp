// The rule of a pose field, written once for the host and the device (include/lidar_odometry_amd.h, "pose field"): the eight
// headings, the heading of an angle, the cell offset of a footprint sample at a heading, and the six moves of a state with
// their conditions, targets and weights.  posefield_host.cpp and the kernels of k_posefield.hpp call these, as
// nav_los_rule.hpp and rollout_rule.hpp are shared by their two homes.  Integers throughout; no HIP header.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LOM_POSE_HD __host__ __device__ inline
#else
#define LOM_POSE_HD inline
#endif

namespace lom {

constexpr uint32_t kPoseHeadings = 8;  // H
constexpr uint32_t kPoseMoves = 6;     // F, FL, FR, SL, SR, B, in this order
constexpr uint32_t kPoseFlagSpin = 1u, kPoseFlagReverse = 2u;  // LOM_POSE_SPIN, LOM_POSE_REVERSE
enum { POSE_F = 0, POSE_FL = 1, POSE_FR = 2, POSE_SL = 3, POSE_SR = 4, POSE_B = 5 };

// heading h points along E, NE, N, NW, W, SW, S, SE (+x is E, +y is N; counter-clockwise): hx + 1 and hy + 1 as two bits each
LOM_POSE_HD int pose_hx(uint32_t h) { return (int)((0x901Au >> (2u * h)) & 3u) - 1; }
LOM_POSE_HD int pose_hy(uint32_t h) { return (int)((0x01A9u >> (2u * h)) & 3u) - 1; }
LOM_POSE_HD uint32_t pose_len(uint32_t h) { return (h & 1u) ? 7u : 5u; }
// the heading of an angle in 1/65536 turn: heading h is the angle 8192 h, and an angle belongs to the nearest
LOM_POSE_HD uint32_t pose_heading_of_angle(uint32_t a) { return ((a + 4096u) >> 13) & 7u; }

// The cell offset of a footprint sample (fx, fy in 1/256 cell, robot frame) at a heading whose table entry is (c, s): the
// rollouts' step 2 for a pose at a cell's centre, so a layer and a rollout's pose test read the same cells.
LOM_POSE_HD void pose_sample_cell(int32_t fx, int32_t fy, int32_t c, int32_t s, int32_t *dx, int32_t *dy)
{
    const int32_t ox = (fx * c - fy * s + 128) >> 8, oy = (fx * s + fy * c + 128) >> 8;
    *dx = (16384 + ox) >> 15, *dy = (16384 + oy) >> 15;  // arithmetic: floor
}

struct PoseCosts {
    uint32_t turn, spin, reverse, flags;
};

// the heading a move ends in
LOM_POSE_HD uint32_t pose_move_heading(uint32_t h, uint32_t m)
{
    return (m == POSE_FL || m == POSE_SL) ? ((h + 1u) & 7u) : (m == POSE_FR || m == POSE_SR) ? ((h + 7u) & 7u) : h;
}
// the cells a move goes along its heading: 1, 0 (a spin) or -1 (backwards)
LOM_POSE_HD int pose_move_sign(uint32_t m) { return m <= POSE_FR ? 1 : m == POSE_B ? -1 : 0; }

// the weight of move m from a state of heading h and layer value s
LOM_POSE_HD uint32_t pose_move_weight(const PoseCosts &pc, uint32_t h, uint32_t s, uint32_t m)
{
    const uint32_t along = pose_move_sign(m) != 0 ? pose_len(h) * s : 0u;
    return along + (m == POSE_FL || m == POSE_FR ? pc.turn : m == POSE_B ? pc.reverse : m == POSE_F ? 0u : pc.spin);
}

// Move m of state (x, y, h), whose layer value s = L(h, x, y) is not 0.  L(h, x, y): the layer, 0 outside the grid, by any
// means (HBM, a tile in LDS).  false: the move is not allowed (or not enabled); else its target (*tx, *ty, *th) and weight.
//  - a translation along +-(hx, hy) to b needs L(h, b) != 0 and, for an odd h, L(h, .) != 0 at the two cells that share an
//    edge with both: the source heading's layer throughout;
//  - a rotation at b from h to h' needs L(h, b) != 0 and L(h', b) != 0.
// Every weight is positive and below 2^28: len * s <= 7 * (2^24 - 1), each cost <= 2^24 - 1, spin >= 1.
template <class Layer>
LOM_POSE_HD bool pose_move(const Layer &L, const PoseCosts &pc, int x, int y, uint32_t h, uint32_t s, uint32_t m, int *tx, int *ty,
                           uint32_t *th, uint32_t *w)
{
    if ((m == POSE_SL || m == POSE_SR) && !(pc.flags & kPoseFlagSpin)) return false;
    if (m == POSE_B && !(pc.flags & kPoseFlagReverse)) return false;
    const int sign = pose_move_sign(m);
    const int bx = x + sign * pose_hx(h), by = y + sign * pose_hy(h);
    const uint32_t h2 = pose_move_heading(h, m);
    if (sign != 0) {
        if (!L(h, bx, by)) return false;
        if ((h & 1u) && (!L(h, bx, y) || !L(h, x, by))) return false;
    }
    if (h2 != h && !L(h2, bx, by)) return false;
    *tx = bx, *ty = by, *th = h2;
    *w = pose_move_weight(pc, h, s, m);
    return true;
}

// the layers in plain memory, [8][height][width] u32
struct PoseLayerCells {
    const uint32_t *layers;
    uint32_t width, height;
    LOM_POSE_HD uint32_t operator()(uint32_t h, int x, int y) const
    {
        if (x < 0 || y < 0 || x >= (int)width || y >= (int)height) return 0u;
        return layers[((size_t)h * height + (uint32_t)y) * width + (uint32_t)x];
    }
};

// a rectangle of cells [x0, x1) x [y0, y1); empty where x0 >= x1 or y0 >= y1
struct PoseBox {
    uint32_t x0, y0, x1, y1;
    bool empty() const { return x0 >= x1 || y0 >= y1; }
};

// the boxes of a re-solve's k_pose_relayer: per heading the states whose stencil can cover a changed cell, and the box that
// holds the eight (posefield_host.cpp builds them)
struct PoseBoxes {
    PoseBox of[kPoseHeadings];
    PoseBox all;
};

}  // namespace lom
