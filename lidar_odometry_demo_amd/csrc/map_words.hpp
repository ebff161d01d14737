// The status words of a map: what the map's kernels and its host code agree on by name.  Device and host code both
// include this (through grid_scan.hpp); nothing else says where a word lives.
//
// The scratch slot S_MISC of a lom_map is one block: 64 u32 status / counter words (256 bytes, zeroed at lom_map_create, never reset
// afterwards -- a call's sequence number tells fresh from stale), then the block aggregates of the single-pass kernels
// (grid_scan.hpp: 256 workgroups x 2 granules).  A kernel takes the block as `words` and indexes it with MW_*; the host
// takes a word's address with d_word(m, MW_*) and reads words back with read_words (map_internal.hpp).
//
// The handle's 1 KiB pinned report block (h_report / d_report) is laid out beside them: [0, 256) the AlignReport,
// from kWordsOffset the {word, tag} pairs of gather_words(), from kSpecWordsOffset those of the read-back that follows
// a cleanup scan enqueued behind an align.
#pragma once
#include <cstddef>

namespace lom {

enum MapWord : int {
    MW_TOTAL64 = 0,     // words 0-1 as one u64: total of the multi-launch insert's packed scan (scan_u64's d_total)
    MW_NEW_VOX = 0,     // k_ins_assign2 -> k_ins_place2: new voxels of this call (the single-pass insert; same word)
    MW_COUNT = 4,       // u32 scan total: voxels kept (cleanup, carve, votes), voxels found (down-sampler), points (export)
    MW_RANGE = 5,       // sequence number of the last call with a point out of range: it inserted / returned nothing
    MW_NVOX = 6,        // the device's voxel counter
    MW_GRID = 7,        // sequence number of the last call whose in-kernel scan gave up (grid_prefix64's error word)
    MW_BULK_BACK = 8,   // ... of the last bulk insert sent back: a partition beyond k_bi_group's LDS, nothing written
    MW_BULK_NVOX0 = 9,  // bulk insert: the voxel counter before the call (k_bi_claim -> k_bi_place)
    MW_BULK_SCAN = 10,  // bulk insert: the flag scan's running word (k_bi_flagscan -> k_bi_place)
    MW_SPEC_SEQ = 12,   // cleanup scan behind an align: the sequence number it was made for, 0 = the align had not ended
    MW_SPEC_CX = 13,    // ... the bits of the centre it used, x y z
    MW_SPEC_CY = 14,
    MW_SPEC_CZ = 15,
};

constexpr size_t kMapWordsBytes = 256;  // byte offset of the block aggregates in S_MISC

constexpr size_t kWordsOffset = 512;      // of h_report / d_report: the words of gather_words()
constexpr size_t kSpecWordsOffset = 768;  // ... the words of a scan enqueued behind an align

}  // namespace lom
