// The words the device stages of a frame hand back to the host before its align, and what they say about the frame.
// Every status word holds a sequence number: it speaks of this frame only if it equals the number the frame's stage
// ran under (the front end's `fe_seq`, the down-sampler's `seq_ds`).  No handle, no HIP: a pure function of the words.
#pragma once
#include <cstdint>

namespace lom {

// Order of the read-back.  The down-sampler words are the matching cloud's when the frame aligns against a keyframe,
// the update cloud's when it initialises one; kWordFeRange is read only under the neighbourhood classifier.
enum StageWord {
    kWordPlanar,      // planar points
    kWordFiltered,    // points after the range filter (input of both down-samplers)
    kWordFeRedoHost,  // front end: the ring classifier hands the frame to the host stages
    kWordFeGrid,      // front end: an in-kernel scan gave up, nothing written
    kWordDsCount,     // down-sampler: points
    kWordDsRange,     // down-sampler: a coordinate out of range or not finite
    kWordDsGrid,      // down-sampler: an in-kernel scan gave up, nothing written
    kWordFeRange,     // front end (neighbourhood classifier): a point of the frame out of range
    kStageWords
};

constexpr const char *kVoxelRangeError = "coordinate / voxel_size out of range or not finite";
constexpr const char *kRadiusRangeError = "coordinate / radius out of range or not finite";

struct StageVerdict {
    enum Action {
        kProceed,     // counts are valid: on to the align (or the keyframe's initialisation)
        kRedoHost,    // the frame takes the host stages
        kRedoDevice,  // neighbourhood classifier: both down-samplers again from the front end's result
        kFailRange    // LOM_ERR_RANGE with `error`
    } action;
    bool wait_front_end;  // kRedoDevice: the front end's own scan gave up, it redoes its stage first (and counts it)
    bool count_redo;      // the odometry's grid_redos goes up by one
    const char *error;    // kFailRange
    uint32_t planar, filtered, matching, update;  // kProceed (the update cloud's count comes later when there is a keyframe)
};

inline StageVerdict decode_stage_words(const uint32_t w[kStageWords], bool has_keyframe, bool neighbourhood, uint32_t fe_seq,
                                       uint32_t seq_ds, bool test_force_host_redo)
{
    StageVerdict v{StageVerdict::kProceed, false, false, nullptr, 0, 0, 0, 0};
    // an in-kernel scan that gave up waiting has written nothing and left its tables at rest (grid_scan.hpp)
    const bool fe_gave_up = w[kWordFeGrid] == fe_seq, ds_gave_up = w[kWordDsGrid] == seq_ds;
    if (neighbourhood) {
        // No host stages behind this classifier, and no azimuth bin that could be ambiguous (kWordFeRedoHost means
        // nothing).  A point out of range fails the frame; after a scan that gave up the stages run again on the device.
        if (w[kWordFeRange] == fe_seq) {
            v.action = StageVerdict::kFailRange;
            v.error = kRadiusRangeError;
            return v;
        }
        if (fe_gave_up || ds_gave_up) {
            v.action = StageVerdict::kRedoDevice;
            v.wait_front_end = fe_gave_up;
            v.count_redo = !fe_gave_up;
            return v;
        }
    }
    // An azimuth on a bin boundary, an organised cloud beyond the buffers, or a scan that gave up: the frame simply
    // takes the host stages, whose kernels wait for nobody.  (LOM_OPT_TEST_FORCE_HOST_REDO: tests take this path on
    // every frame; that is no redo.)
    const bool fe_redo_host = !neighbourhood && w[kWordFeRedoHost] == fe_seq;
    if (fe_redo_host || fe_gave_up || ds_gave_up || test_force_host_redo) {
        v.action = StageVerdict::kRedoHost;
        v.count_redo = fe_gave_up || ds_gave_up;
        return v;
    }
    if (w[kWordDsRange] == seq_ds) {
        v.action = StageVerdict::kFailRange;
        v.error = kVoxelRangeError;
        return v;
    }
    v.planar = w[kWordPlanar];
    v.filtered = w[kWordFiltered];
    (has_keyframe ? v.matching : v.update) = w[kWordDsCount];
    return v;
}

}  // namespace lom
