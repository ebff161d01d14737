// The rule of a trajectory rollout, written once for the host and the device (include/lidar_odometry_amd.h, "trajectory
// rollouts", steps 1 and 2): the motion of a pose under a command, the closed form of a pose's angle, the cell of a
// footprint sample at a pose and the class of what lies under it.  lom_rollout_poses (rollout_host.cpp) and the kernels
// of k_rollout.hpp call these, as lm_core.hpp is shared by the LM policy's two homes.  Integers throughout; no HIP header.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define LOM_ROLLOUT_HD __host__ __device__ inline
#else
#define LOM_ROLLOUT_HD inline
#endif

namespace lom {

constexpr uint32_t kRolloutTable = 4096;        // T: entries of the direction table, (C, S) int32 pairs
constexpr uint32_t kRolloutAngleShift = 4;      // an angle a reads entry a >> 4
constexpr uint32_t kRolloutAngleMask = 65535u;  // angles are held mod 65536
constexpr int kRolloutCellShift = 15;           // a position is Q15 cells
// the code of a sample and of a pose (LOM_ROLLOUT_*); INVALID is a record's only
enum { ROLLOUT_OK = 0, ROLLOUT_UNKNOWN = 1, ROLLOUT_COLLISION = 2, ROLLOUT_EDGE = 3, ROLLOUT_INVALID = 4 };

// step 1: what one step under speed v adds along an axis whose table entry is c; |v * c| <= 2^30
LOM_ROLLOUT_HD int32_t rollout_increment(int32_t v, int32_t c) { return (v * c + 16384) >> 15; }

// Step 1 in closed form: the angle of pose t, 0 <= t <= L * Tn, as an unreduced sum (mask it), and the command (v, w) of
// the step that LEADS to pose t (step t - 1; untouched for t == 0).  commands: L pairs (v, w).  Pose t has taken
// clamp(t - j * Tn, 0, Tn) steps of segment j; |w * Tn * L| <= 2^25.
LOM_ROLLOUT_HD int32_t rollout_angle_sum(uint32_t a0, const int16_t *commands, uint32_t L, uint32_t Tn, uint32_t t, int32_t *v_in, int32_t *w_in)
{
    int32_t acc = (int32_t)a0;
    for (uint32_t j = 0; j < L; j++) {
        const uint32_t from = j * Tn;
        if (t <= from) break;
        const uint32_t n = t - from < Tn ? t - from : Tn;
        const int32_t w = commands[2 * j + 1];
        acc += w * (int32_t)n;
        *v_in = commands[2 * j], *w_in = w;  // the last segment entered is the one of step t - 1
    }
    return acc;
}

// step 2: the position of a footprint sample (fx, fy in 1/256 cell, robot frame) at a pose whose table entry is (c, s)
LOM_ROLLOUT_HD void rollout_sample_at(int32_t x, int32_t y, int32_t fx, int32_t fy, int32_t c, int32_t s, int32_t *px, int32_t *py)
{
    *px = x + ((fx * c - fy * s + 128) >> 8);
    *py = y + ((fx * s + fy * c + 128) >> 8);
}

// step 2: the code of a cell value, and the cost of an OK one
LOM_ROLLOUT_HD uint32_t rollout_classify(int32_t v, int32_t lethal_min, int32_t unknown_cost, uint32_t *cost)
{
    *cost = 0u;
    if (v >= lethal_min) return ROLLOUT_COLLISION;
    if (v < 0) {
        if (unknown_cost < 0) return ROLLOUT_UNKNOWN;
        *cost = (uint32_t)unknown_cost;
        return ROLLOUT_OK;
    }
    *cost = (uint32_t)v;
    return ROLLOUT_OK;
}

// Step 2 for one pose: the greatest sample code and the greatest cost over the OK samples.  Cell: int8 at (cx, cy), both in
// the grid, by any means (HBM, a window in LDS).  footprint: F pairs (fx, fy).
template <class Cell>
LOM_ROLLOUT_HD uint32_t rollout_pose_test(int32_t x, int32_t y, int32_t c, int32_t s, const int32_t *footprint, uint32_t F, uint32_t width,
                                          uint32_t height, int32_t lethal_min, int32_t unknown_cost, const Cell &cell, uint32_t *pose_cost)
{
    uint32_t code = ROLLOUT_OK, cost = 0u;
    for (uint32_t i = 0; i < F; i++) {
        int32_t px, py;
        rollout_sample_at(x, y, footprint[2 * i], footprint[2 * i + 1], c, s, &px, &py);
        const int32_t cx = px >> kRolloutCellShift, cy = py >> kRolloutCellShift;  // arithmetic: floor
        uint32_t sc = ROLLOUT_EDGE, sample_cost = 0u;
        if ((uint32_t)cx < width && (uint32_t)cy < height) sc = rollout_classify((int32_t)cell(cx, cy), lethal_min, unknown_cost, &sample_cost);
        code = sc > code ? sc : code;
        cost = sample_cost > cost ? sample_cost : cost;  // (0 for a sample that is not OK)
    }
    *pose_cost = cost;
    return code;
}

// the plane in plain memory
struct RolloutPlaneCell {
    const int8_t *plane;
    uint32_t width;
    LOM_ROLLOUT_HD int8_t operator()(int32_t cx, int32_t cy) const { return plane[(size_t)cy * width + (uint32_t)cx]; }
};

}  // namespace lom
