// Internal declarations shared by the HIP translation units.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lidar_odometry_amd.h"
#include "device_handle.hpp"

namespace lom {

// ---- open-addressed voxel hash in HBM ---------------------------------------
// One 16-byte slot per voxel: a single dwordx4 load yields key, point count
// and payload slab (reference: robin_map<Indices, VoxelWithPlanes>,
// src/voxel_grid.h:256).  Payload lives in slabs [slab][K] of packed 12-byte
// points and, separately, 12-byte normals (normals are read once per query,
// for the winner only, so they stay out of the candidate stream).
struct __attribute__((aligned(16))) Slot {
    unsigned long long key;  // packed (ix,iy,iz), 21 bits each, biased; kEmptyKey = free
    uint32_t count;          // stored points (<= K)
    uint32_t slab;           // creation index of the voxel; kNoSlab until assigned
};
static_assert(sizeof(Slot) == 16, "slot must be one dwordx4");

constexpr unsigned long long kEmptyKey = ~0ull;
constexpr uint32_t kNoSlab = 0xFFFFFFFFu;
constexpr int kIdxBias = 1 << 20;          // indices in (-2^20, 2^20)
constexpr float kIdxLimit = 1048576.0f;    // |x / voxel_size| must stay below

__host__ __device__ inline unsigned long long pack_key(int ix, int iy, int iz)
{
    return ((unsigned long long)(uint32_t)(ix + kIdxBias) << 42) |
           ((unsigned long long)(uint32_t)(iy + kIdxBias) << 21) |
           (unsigned long long)(uint32_t)(iz + kIdxBias);
}

// Fibonacci hashing: top log2(cap) bits of key * 2^64/phi.  The hash never
// influences results (reference IndicesHash, voxel_grid.h:31-38, likewise).
// (Round 3 tried a brick-local hash -- the 2x2x2 block of voxels sharing (ix >> 1, iy >> 1, iz >> 1) in ONE 128-byte
// bucket, so that a query's 27 slots lie in eight lines: half the L2 requests, but the bricks of one surface collide
// in whole parity patterns (chains 2.4 slots against 1.4 at equal load), the three per-axis hash parts have to travel
// through LDS, and at equal table size the probe phase of C2 took 2.4 us against 1.5: DESIGN.md section 5.)
__host__ __device__ inline uint32_t hash_key(unsigned long long key, uint32_t shift)
{
    return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> shift);
}

// voxel_grid.h:70-72 / :166-168: static_cast<int64_t>(x / voxel_size_), f32
// division (correctly rounded), truncation toward zero.
__device__ inline bool voxel_index(float x, float voxel_size, int &out)
{
    const float f = __fdiv_rn(x, voxel_size);
    if (!(f > -kIdxLimit && f < kIdxLimit)) return false;  // also NaN
    out = (int)f;
    return true;
}

// Same value, cheaper when the voxel size is a power of two (the reference's 0.5 / 1.0 / 0.25):
// x * 2^-k IS the correctly rounded quotient x / 2^k (an exact scaling; where it would go
// subnormal both truncate to 0).  inv == 0 selects the IEEE division.
__device__ inline bool voxel_index_fast(float x, float voxel_size, float inv, int &out)
{
    const float f = (inv != 0.f) ? x * inv : __fdiv_rn(x, voxel_size);
    if (!(f > -kIdxLimit && f < kIdxLimit)) return false;  // also NaN
    out = (int)f;
    return true;
}

struct MapView {
    const Slot *table;
    uint32_t mask;   // capacity - 1
    uint32_t shift;  // 64 - log2(capacity)
    const float *pts;  // [slab][K][3]
    const float *nrm;  // [slab][K][3]
    uint32_t K;
    float voxel_size;
    float inv_voxel_size;  // 1 / voxel_size when that is exact (power of two), else 0
    float prune_slack;     // 1e-4f * voxel_size (f32 product): the absolute slack of k_match's face-distance bounds, as a
                           // kernel argument so that it lives in a scalar register
};

// pose as the kernels consume it
struct PoseArgs {
    double R[9];  // f32 rotationMatrix() widened (voxel_grid.h:212)
    double t[3];  // f32 translation widened (voxel_grid.h:213)
    float max_sq; // max_correspondence_distance^2 in f32 (voxel_grid.h:215)
};

struct EvalArgs {
    double q[4];  // w,x,y,z
    double t[3];
};

// Single-GPU align: the outer loop's state lives in HBM between the kernels of one align.  k_lm's
// workgroup 0 writes it at the end of an outer iteration; the next k_match takes its pose from P,
// the next k_lm continues from pose_t / pose_q -- the host enqueues the kernels of several outer
// iterations without waiting for any of them.
struct AlignState {
    PoseArgs P;        // pose of the next correspondence search
    float pose_t[3];   // f32 pose after the write-back (cloud_matcher.cpp:161-167)
    float pose_q[4];
    int32_t finished;  // converged (:169-172) or 35 iterations done: later kernels of the chain do nothing
    int32_t error;     // a workgroup gave up waiting for the others
    int32_t outer_done;
    int32_t lm_iterations, evaluations;
    int32_t replayed;  // of outer_done: iterations accounted for by the replay fold (k_lm's tail), not executed
    double valid_last, valid_total, cand_total, occ_total, queries_total;
    double final_cost, last_step_norm;
};

// what the host reads back (pinned host memory): a copy of the scalar part of AlignState, written
// by k_lm's workgroup 0 after every outer iteration, sequence word last
struct AlignReport {
    unsigned long long seq;
    int32_t finished, error, outer_done, lm_iterations, evaluations, replayed;
    float pose_t[3], pose_q[4];
    float pad2;
    double valid_last, valid_total, cand_total, occ_total, queries_total;
    double final_cost, last_step_norm;
};

// ---- host-side handle ---------------------------------------------------------
// Device, stream, error text, LOM_HIP, the owning DeviceBuf / PinnedBuf and their grow-only ensure / ensure_pinned are
// the same for every handle: device_handle.hpp.  Below is what the map handle (and a scan context, which is one) adds.

// Buffers of the batched align (lom_match_align_batch / _multi): per-problem solve states and descriptors, records,
// k_match counters, exchange sets per round slot, staged host scans -- and per-problem reports in pinned host memory;
// the single align's align_state / scan_on / xrec / report are never touched by it
struct BatchAlignBufs {
    DeviceBuf dev, rec, cnt, xrec, src;
    PinnedBuf stage;    // pinned staging of the states and descriptors (one copy per call)
    PinnedBuf reports;  // AlignReport slots, 256 bytes each (mapped)
    unsigned long long report_seq = 0, lm_seq = 0;
    uint32_t per_cu[4] = {0, 0, 0, 0};  // k_lm blocks per CU a batch round may count on, per variant (cached)
    int test_round_max = 0;  // LOM_OPT_TEST_BATCH_ROUND_MAX: problems per round at most (0: by residency)
};
// ... of the quality report (lom_match_quality*): staged host scan, winner indices and records of its search, k_match
// counters, per-workgroup records, per-point residuals -- and the reduced values in pinned host memory; neither the
// single align's buffers nor the map-maintenance scratch (lom_map::scr) are touched
struct QualityBufs {
    DeviceBuf src, idx, rec, cnt, part, res;
    PinnedBuf sums;  // LOM_NQSUMS doubles (mapped)
};
// ... of the batched quality report (lom_match_quality_batch*): uploaded host clouds, one round's records / k_match
// counters / workgroup records, the per-problem poses and descriptors, the per-problem totals -- and a pinned host block
// that stages the descriptors on the way in and the totals on the way out
struct QualityBatchBufs {
    DeviceBuf src, rec, cnt, part, dev, sums;
    PinnedBuf stage;
    int test_round_max = 0;  // LOM_OPT_TEST_QUALITY_ROUND_MAX: problems per round at most (0: by the byte budget)
};

// ... of the scan votes (lom_map_carve_scans / lom_map_scan_votes, vote.hip): two u64 masks and two u32 counts per slab,
// at rest (zero) between calls -- whoever dirties a word puts it back --, the status words (k_vote.hpp, VW_*) and the
// call's scan descriptors; the erase itself uses the map-maintenance scratch as the carve does (erase_begin below)
struct VoteBufs {
    DeviceBuf hitmask, crossmask, free_votes, seen_votes, words, desc;
    uint32_t test_slice_max = 0;  // LOM_OPT_TEST_VOTE_SLICE_MAX: scans per launch at most (0: 64)
};

// one set of slab arrays (creation order), allocated and freed together (voxel_map.hip)
struct Slabs {
    unsigned long long *key = nullptr;  // [cap]
    uint32_t *count = nullptr;          // [cap]
    float *pts = nullptr, *nrm = nullptr;  // [cap][K][3]
    uint32_t cap = 0;
};

// points per partition k_bi_group can hold in LDS (its larger shape); bounds LOM_OPT_TEST_BULK_PARTITION_MAX
constexpr uint32_t kBiPartMax = 1024;

// ---- lom_map::scr: the map-maintenance scratch --------------------------------------------------------------------
// Grow-only device buffers, indexed by the enum below; the five files of the voxel map are the only ones that touch
// them.  Who keeps what in which slot is tabulated in map_internal.hpp; the status words of S_MISC are map_words.hpp.
enum {
    S_IN_XYZ = 0,
    S_IN_NRM,
    S_PT_SLOT,
    S_PT_POS,
    S_FLAG,
    S_RANK,
    S_BKT_CNT,
    S_BKT_HEAD,
    S_BKT_OFF,
    S_BKT_OLD,
    S_PT_OFF,
    S_PT_M,
    S_ITEMS,
    S_SCAN,
    S_DS_HEAD,
    S_MISC,
    S_ENT_ROW,  // bulk insert: row of every survivor
    S_HIST,     // bulk insert: [partition][block] counts
    S_PART,     // bulk insert: partition sizes and starts
    S_CARVE_CROSS,  // ray carving: u32 per slab, rays of this call that crossed the voxel
    S_CARVE_HIT,    // ray carving: u32 per slab, an endpoint of this call fell into the voxel
    S_CARVE_WORDS,  // ray carving: its status words (k_carve.hpp, CW_*)
    S_COUNT
};

}  // namespace lom

struct lom_map : lom::DeviceHandle {
    // a scan context (lom_scan_create): no table or slabs of its own, its kernels read the parent's
    lom_map *parent = nullptr;
    // map side: calls that changed the map (their kernels run on THIS handle's stream); context side: the count its
    // stream has been ordered behind, and the event it uses for that
    // (atomic: a context's fast path reads the parent's count while another context, or the map's own caller, settles)
    std::atomic<uint64_t> mutations{0};
    uint64_t seen_mutations = ~0ull;
    hipEvent_t parent_ev = nullptr;
    // Settling the map -- redoing an insert nobody has looked at yet, reading its voxel count back -- uses the MAP's
    // stream, pinned words and scratch: whoever does it (the map's own caller, a context's first call after a change,
    // lom_scan_create) holds this lock, so that several threads arriving together settle once.
    std::mutex settle_mutex;
    hipStream_t own_stream = nullptr;  // `stream` is this one unless lom_map_set_stream gave another
    // compute units this handle's own stream runs on: 0 = all of the device; a scan context on a partition
    // (lom_scan_create_on_partition) owns a stream with a CU mask, and its grids are sized for that many CUs
    uint32_t partition_cus = 0;
    float voxel_size = 0.5f;
    uint32_t K = 10;          // row stride of the slabs: the largest max_points_ the stored voxels have seen
    uint32_t max_points = 10; // max_points_ (voxel_grid.h:253): what an insert fills a voxel up to; <= K

    // hash table
    lom::Slot *d_table = nullptr;
    uint32_t cap = 0;  // power of two
    uint32_t min_cap = 0;

    // slabs (creation order).  n_vox is the host's copy of the device-side voxel counter: an insert
    // whose worst case fits the allocated slabs does not wait for the GPU, it only raises the upper
    // bound n_vox_ub and marks n_vox stale; whoever needs the exact value calls refresh_nvox().
    uint32_t n_vox = 0;
    uint32_t n_vox_ub = 0;
    bool n_vox_stale = false;
    // pinned bounce buffer for host-resident inputs (truly asynchronous H2D) + "last copy done" event
    lom::PinnedBuf h_stage;
    hipEvent_t stage_ev = nullptr;
    lom::Slabs slabs;
    uint64_t n_points = 0;
    // second slab set: radiusCleanup compacts into it and swaps (no allocation per frame)
    lom::Slabs alt;

    // scratch (grown on demand, never shrunk)
    lom::DeviceBuf scr[lom::S_COUNT];
    // sequence number of the last map-maintenance call (tags block aggregates and error words: no resets),
    // the one up to which lom_map_status has looked, and whether the table is known to be all-empty
    uint32_t call_seq = 0, status_seq = 0;
    bool table_clean = true;
    // the handle's last single-pass insert, for lom_map_status() to redo should its in-kernel scan have given up
    const char *pending_xyz = nullptr, *pending_nrm = nullptr;
    std::atomic<size_t> pending_n{0};  // != 0: an unverified single-pass insert (read without the lock by the fast paths)
    size_t pending_stride = 0;
    uint32_t pending_seq = 0, grid_resolved_seq = 0;
    uint32_t grid_redos = 0;  // calls redone with the multi-launch scan after a give-up (lom_map_debug_counter)
    // per-scan buffers of align/find_pairs
    lom::DeviceBuf scan_src, scan_idx, scan_on, scan_stats, partials, results;

    // the pinned blocks of handle_setup (handle.hip) and the typed views of them that the align path uses
    lom::PinnedBuf pin_results, pin_flags, pin_mail, pin_cmd, pin_report;
    double *h_results = nullptr;  // 1024 doubles (rank-ordered gather of up to 32 ranks)
    uint32_t *h_flags = nullptr;  // 64 words
    // mailbox: every k_eval workgroup stores one 32-double record (sums, counters,
    // sequence word) directly into coherent (fine-grained) pinned host memory; the host
    // polls the sequence words instead of paying a copy kernel plus
    // hipStreamSynchronize per residual evaluation.
    double *h_mail = nullptr;             // host view: 64 records x 32 doubles
    double *d_mail = nullptr;             // device view of the same allocation
    unsigned long long mail_seq = 0;
    // command word of the resident evaluation server (pinned host memory, host writes, device polls)
    void *h_cmd = nullptr, *d_cmd = nullptr;
    bool server_alive = false;
    bool eval_attr_set = false;
    // device-resident outer loop (single GPU): state in HBM, exchange records of k_lm's workgroups,
    // report in pinned host memory
    lom::DeviceBuf align_state, xrec, dbg_trace, dbg_stamps;
    bool align_state_dirty = true;  // AlignState must be zeroed before the next chain (fresh, or left with its error flag set)
    void *h_report = nullptr, *d_report = nullptr;  // 1 KiB: AlignReport, and at 512 the words of gather_words()
    uint32_t words_tag = 0;
    int words_pending = 0;  // words of a lom_map_read_device_words_begin not yet collected
    uint32_t n_dead = 0;  // slabs below n_vox whose voxel a radius cleanup erased without moving the others (k_cleanup_mark)
    uint32_t dead_below = 0;  // ... all of them below this slab number (the slab count at the last such cleanup)
    bool opt_dense_cleanup = false;  // LOM_DENSE_CLEANUP=1 at create: every radius cleanup closes its holes at once (as until round 4)
    void (*idle_hook)(void *) = nullptr;  // lom_map_set_align_idle_hook: one shot
    void *idle_user = nullptr;
    // the scan of a radius cleanup enqueued behind an align (lom_map_radius_cleanup_after_align, map_erase.hip)
    float spec_radius = 0.f;     // > 0: the next device-resident align on this handle enqueues it
    bool spec_inflight = false;  // scan and read-back are on the stream; what they were made for:
    float spec_r = 0.f;
    uint32_t spec_seq = 0, spec_tag = 0, spec_nv = 0;
    uint64_t spec_mutations = 0;
    uint32_t spec_gave_up_seq = 0;  // the last such scan that gave up and was not taken: no call's number, map_status skips it
    uint32_t cleanups_taken = 0;  // radius cleanups that used such a scan (lom_map_debug_counter)
    unsigned long long report_seq = 0, lm_seq = 0, lm_launches = 0;
    int last_replayed = 0;  // outer iterations of the last align on this handle that the replay fold accounted for (lom_debug_replayed_iterations)
    // the batched align, the quality report and the batched quality report keep buffers of their own
    lom::BatchAlignBufs batch;
    lom::QualityBufs qual;
    lom::QualityBatchBufs qualb;
    lom::VoteBufs vote;
    // lom_match_align_multi: recorded on this handle's stream -- as a problem map, for the runner to wait on before the
    // chain; as the runner, after the chain, for the problem maps to wait on (created once, timing disabled)
    hipEvent_t multi_ev = nullptr;
    uint32_t lm_max_blocks[4] = {0, 0, 0, 0};  // co-resident k_lm workgroups this device admits, per variant (occupancy query, cached)
    double last_counters[4] = {0, 0, 0, 0};  // valid, cand, occ, queries of the last k_match

    bool profiling = false;       // this align carries event pairs
    int profile_period = 0;       // 0 off, N: every N-th align
    unsigned long long align_count = 0;
    std::vector<hipEvent_t> prof_events;  // pairs around each k_match launch of one align

    // device-to-device exchange (lom_comm_attach_p2p): this rank's buffer and the peers' IPC mappings
    bool p2p = false;
    void *p2p_local = nullptr;          // [4 sets][kP2pMaxRanks][32] exchange words in this GPU's HBM
    void *p2p_peer[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    unsigned long long p2p_epoch = 0;   // device-to-device aligns since the attach: the same number on every rank
    // RCCL
    void *comm = nullptr;       // RCCL communicator (device-side all-gather)
    void *host_comm = nullptr;  // host shared-memory exchange between the ranks of one node
    int rank = 0, nranks = 1;
    lom::DeviceBuf gather;

    // run-time switches: environment read ONCE at lom_map_create, afterwards lom_map_set_option only
    uint32_t table_slots_per_voxel = 16;  // after a bulk insert (LOM_TABLE_SLOTS_PER_VOXEL at create)
    bool opt_host_lm = false;       // LOM_OPT_HOST_LM / LOM_HOST_LM=1
    bool opt_debug_lm = false;      // LOM_OPT_DEBUG_LM_STAMPS / LOM_DEBUG_LM=1
    bool opt_debug_lm_twice = false;  // LOM_DEBUG_LM_TWICE=1 at create: k_lm<256, 64, 2> runs every policy step twice, stamps time the second
    bool opt_debug_timing = false;  // LOM_OPT_DEBUG_TIMING / LOM_DEBUG_TIMING=1
    bool opt_count = false;         // LOM_OPT_COUNT_CANDIDATES / LOM_COUNT_CANDIDATES=1: the searches also produce the reference-
                                    // algorithm counts (occupied voxels, stored points of all 27 neighbours): 27 slot loads per query
    bool opt_replay_fold = true;    // LOM_OPT_REPLAY_FOLD: the single align folds repeated outer iterations (k_lm's tail; 0 = run them)
    bool opt_no_temporal = false;   // LOM_OPT_NO_TEMPORAL_BOUND / LOM_NO_TEMPORAL=1: every search at the plain max_dist bound
    unsigned long long patience_ticks = 5000000ull;  // bounded in-kernel waits: 50 ms of s_memrealtime (100 MHz)
    bool opt_no_bulk = false;       // LOM_OPT_NO_BULK_INSERT / LOM_NO_BULK_INSERT=1: batches above 65,536 points take the four-kernel path
    uint32_t bulk_ppt = 0;          // LOM_BULK_PPT at create: points per thread of k_bi_claim / k_bi_scatter (0: by batch size)
    uint32_t test_bulk_part_max = 0;  // LOM_OPT_TEST_BULK_PARTITION_MAX: points a partition of the bulk insert may hold (0: the LDS limit)
    int test_grid_give_up = -1;     // LOM_OPT_TEST_GRID_GIVE_UP: first workgroup that gives up in the next in-kernel scan
    int test_give_up_outer = -1;    // LOM_OPT_TEST_GIVE_UP_AT_OUTER: k_lm of that outer iteration of the next align gives up
};

namespace lom {

std::string &map_create_error();  // handle.hip: the map family's create slot (lom_last_error(NULL)), for comm.cpp
// handle.hip: a host scan into `buf` (grown as needed), one asynchronous copy on the handle's stream
int upload_scan(lom_map *m, DeviceBuf &buf, const void *src, size_t n, size_t stride, const char **d_src);
// handle.hip: the host clouds of a problem list into `buf`, every distinct (pointer, n, stride) once, at 256-byte aligned
// offsets in order of first appearance; d_src[i] is problem i's device address (an empty problem takes no room)
struct HostCloud {
    const void *p;
    size_t n, stride;
};
int upload_distinct(lom_map *m, DeviceBuf &buf, const HostCloud *clouds, int count, const char **d_src);
MapView view_of(const lom_map *m);
int resolve_pending(lom_map *m);  // voxel_map.hip: redo the last single-pass insert if its in-kernel scan gave up
int map_init(lom_map *m, size_t capacity_hint);  // voxel_map.hip: status words and the first table of a new map (lom_map_create)
int settle_map(lom_map *map);  // voxel_map.hip: settle a pending insert and the voxel count, under the map's settle lock
void map_free(lom_map *m);     // voxel_map.hip: the table and both slab sets (lom_map_destroy)
void cleanup_scan_behind_align(lom_map *m);  // map_erase.hip: see lom_map_radius_cleanup_after_align
// map_erase.hip: the erase of the ray carve, for an erase whose decision is made elsewhere (vote.hip), in this order --
//   map_settle_nvox: a pending insert is settled, m->n_vox is exact;
//   erase_begin: room for keep / newid / the scan's temporaries of m->n_vox slabs; the call counts as a change of the map
//     (call_seq, mutations) and a cleanup scan armed behind an align is never taken now; *keep: one word per slab to fill;
//   erase_rank: newid[] from keep[]; *d_kept: the device word that will hold the number of kept slabs;
//   erase_finish: n_keep of the m->n_vox slabs stay -- in place, or compaction (erase_unkept).
int map_settle_nvox(lom_map *m);
int erase_begin(lom_map *m, uint32_t **keep);
int erase_rank(lom_map *m, const uint32_t **d_kept);
int erase_finish(lom_map *m, uint32_t n_keep);
// voxel_map.hip: n device words in one read-back on the handle's stream (waits for them)
int gather_words(lom_map *m, const uint32_t *const *ptrs, int n, uint32_t *out);

// RCCL (comm.cpp), loaded lazily with dlopen
int comm_allgather_sums(lom_map *m, const double *d_send, double *d_recv, int count);
// host shared-memory exchange: out = sum over ranks (rank order) of `mine`
int host_exchange_sums(lom_map *m, const double *mine, double *out);
int host_comm_rank(void *host_comm, int *rank, int *nranks, unsigned long long *seq = nullptr);
// lom_host_comm_allreduce with a deadline of the caller's choosing (the exchange that follows a device-to-device
// align must outlast the device-side patience of the slowest rank)
int host_comm_allreduce_deadline(void *host_comm, double *buf, int count, double timeout_s);
const char *host_comm_error(void *host_comm);
// device-to-device exchange (match.hip)
constexpr int kP2pMaxRanks = 8;
void p2p_detach(lom_map *m);

}  // namespace lom
