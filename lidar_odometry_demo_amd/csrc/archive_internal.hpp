// The scan archive's handle, shared by archive.hip (which owns it) and vote.hip (which reads its table and clouds under
// its lock).  Definitions: include/lidar_odometry_amd.h ("scan archive and map assembly").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <vector>

#include "assemble_host.hpp"
#include "device_handle.hpp"

// The archive owns its stream and every buffer below; calls on one archive are serialised by `lock`.
struct lom_archive : lom::DeviceHandle {
    std::mutex lock;
    // the table (host) and the clouds (device): scan k is points [offset, offset + n) of both arrays, 12 bytes each
    std::vector<lom::assemble::ScanEntry> table;
    uint64_t points = 0, cap_points = 0;
    lom::DeviceBuf xyz, nrm;
    // staging of the assembly, reused call after call and sized by the call: descriptors, the transformed cloud, the
    // [scan][block] matrix of kept counts and its prefix, the compacted cloud
    lom::DeviceBuf desc, stage_xyz, stage_nrm, counts, offsets, out_xyz, out_nrm;
    lom::PinnedBuf h_desc;  // the descriptors on their way in
    lom::PinnedBuf h_word;  // the kept total on its way out
    // recorded on the archive's stream behind the kernels, for the map's stream to wait on before the insert; recorded on
    // the map's stream behind the insert, for the archive's stream to wait on before it overwrites the staging
    hipEvent_t ready_ev = nullptr, done_ev = nullptr;
    bool done_recorded = false;

    float *d_xyz() const { return xyz.as<float>(); }
    float *d_nrm() const { return nrm.as<float>(); }
};
