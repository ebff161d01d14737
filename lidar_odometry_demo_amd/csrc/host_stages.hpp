// The stages processCloud runs before the align, on the host:
//   utils::pointTimeNormalize            reference src/utils/point_time_normalize.h:15-39
//   CloudTransformer::transformNonRigid  reference src/utils/cloud_transform.h:15-40
//   CloudClassifier::classify            reference src/utils/cloud_classifier.h:19-168
//   utils::rangeFilter                   reference src/utils/range_filter.h:13-28
// With a Pool the per-point loops run in contiguous parts; the results are those of pool = nullptr, byte for byte.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/lidar_odometry_amd.h"
#include "host_threads.hpp"

namespace lom {

struct ClassifyScratch {  // reused across frames: no allocation or zero-fill beyond what the algorithm needs
    std::vector<lom_point_xyzirt> cloud;
    std::vector<uint32_t> cell, hist;
    std::vector<float> tmp_xyz, tmp_nrm;
    std::vector<size_t> cnt_p, cnt_u, off_p;
};

}  // namespace lom

namespace lom __attribute__((visibility("hidden"))) {  // internal: the library exports its C ABI only

void time_normalize(const lom_point_xyzirt *in, size_t n, lom_point_xyzirt *out, Pool *pool = nullptr);
void transform_non_rigid(const lom_point_xyzirt *in, size_t n, const lom_pose &start, const lom_pose &end,
                         lom_point_xyzirt *out, Pool *pool = nullptr);
size_t range_filter(const float *xyz, const float *nrm, size_t n, float min_range, float max_range, float *xyz_out,
                    float *nrm_out, Pool *pool = nullptr);

// planar points + normals (the unclassified cloud is discarded by the only caller,
// lidar_odometry.cpp:33, so only its size is reported)
size_t classify(const lom_point_xyzirt *in, size_t n, float *xyz_out, float *nrm_out, size_t *unclassified,
                size_t grid[2], ClassifyScratch &sc, Pool *pool = nullptr);

// Eigen eulerAngles(0,1,2) of (qa * qb^-1).toRotationMatrix(), degrees (lidar_odometry.cpp:54-55)
void delta_euler_deg(const float qa[4], const float qb[4], float out[3]);

}  // namespace lom
