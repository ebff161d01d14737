// Erasing voxels from the map: radiusCleanup (voxel_grid.h:236-246), its scan enqueued behind an align, and the erase
// back end that the ray carve (map_carve.hip) and the scan votes (vote.hip) share with it.  This file is the one
// translation unit that instantiates and launches the kernels of k_cleanup.hpp; scans, table rebuild and the word
// read-backs are voxel_map.hip's (map_internal.hpp).
//
// Built with -ffp-contract=off (see voxel_map.hip).
#include <algorithm>
#include <cstring>

#include "grid_scan.hpp"
#include "k_cleanup.hpp"
#include "lom_internal.hpp"
#include "map_internal.hpp"

namespace lom {

// the single-pass scan of a radius cleanup: flags, new slab numbers, number of voxels kept (MW_COUNT); `from` as k_cleanup_scan's
static bool launch_cleanup_scan(lom_map *m, uint32_t nv, const float center[3], float r2, uint32_t seq, const AlignState *from)
{
    // consecutive voxels per thread: the smallest form whose grid stays within kOnePassMax threads
    static const struct {
        uint32_t items;
        decltype(&k_cleanup_scan<1>) kernel;
    } forms[] = {{1, k_cleanup_scan<1>}, {4, k_cleanup_scan<4>}, {16, k_cleanup_scan<16>}};
    uint32_t *keep = m->scr[S_FLAG].as<uint32_t>(), *newid = m->scr[S_RANK].as<uint32_t>();
    for (const auto &f : forms) {
        if (nv > f.items * kOnePassMax) continue;
        hipLaunchKernelGGL(f.kernel, dim3(blocks_for((nv + f.items - 1) / f.items)), dim3(kThreads), 0, m->stream,
                           m->slabs.pts, m->slabs.count, m->K, nv, center[0], center[1], center[2], r2, keep, newid, d_agg(m), seq,
                           d_words(m), take_test_fail_from(m), from);
        return true;
    }
    return false;
}

// the same through kernels that wait for nobody: flags, multi-launch scan; the number of voxels kept in MW_COUNT
static int cleanup_scan_multi_launch(lom_map *m, uint32_t nv, const float center[3], float r2)
{
    uint32_t *keep = m->scr[S_FLAG].as<uint32_t>(), *newid = m->scr[S_RANK].as<uint32_t>();
    hipLaunchKernelGGL(k_cleanup_flag, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, m->slabs.pts, m->slabs.count, m->K, nv,
                       center[0], center[1], center[2], r2, keep);
    LOM_HIP(m, hipGetLastError());
    return scan_u32(m, keep, newid, nv, d_word(m, MW_COUNT), m->scr[S_SCAN].as<uint32_t>());
}

// lidar_odometry.cpp:65-67 calls radiusCleanup with the translation the align has just produced: the scan of that cleanup
// only reads the map and writes scratch, so it can run right behind the align's last solve -- with the centre taken from
// the align's state in HBM -- instead of a host round trip, a thread hand-off and a launch later.  The caller arms it
// (lom_map_radius_cleanup_after_align), the next device-resident align on the handle enqueues scan and read-back behind
// its first five (k_match, k_lm) pairs (align.hip), and lom_map_radius_cleanup takes the result if, and only if, it was
// made for exactly its arguments on exactly this state of the map; everything else is the plain path below.
static const MapWord kSpecWords[] = {MW_COUNT, MW_GRID, MW_SPEC_SEQ, MW_SPEC_CX, MW_SPEC_CY, MW_SPEC_CZ};
constexpr int kSpecWordCount = 6;

void cleanup_scan_behind_align(lom_map *m)
{
    const float radius = m->spec_radius;
    m->spec_radius = 0.f;  // armed for one align
    // (a scan nobody has asked for since -- the caller did something else with the map -- is superseded: the read-back
    // of this one follows it on the stream and carries the next tag; its give-up word is looked at before that)
    drop_cleanup_behind_align(m);
    if (!(radius > 0.f) || m->parent || m->n_vox_stale || m->pending_n.load() || m->n_vox == 0 || !m->align_state.p) return;
    const uint32_t nv = m->n_vox;
    // (scratch that has to grow: the plain path does that; an allocation here would wait for the align)
    if (m->scr[S_FLAG].bytes < (size_t)nv * 4 || m->scr[S_RANK].bytes < (size_t)nv * 4 || nv > 16 * kOnePassMax) return;
    const float zero[3] = {0.f, 0.f, 0.f};
    const uint32_t seq = ++m->call_seq;
    if (!launch_cleanup_scan(m, nv, zero, radius * radius, seq, m->align_state.as<const AlignState>())) return;
    const uint32_t *ptrs[kSpecWordCount];
    for (int i = 0; i < kSpecWordCount; i++) ptrs[i] = d_word(m, kSpecWords[i]);
    if (++m->spec_tag == 0) m->spec_tag = 1;
    if (launch_gather_words(m, ptrs, kSpecWordCount, kSpecWordsOffset, m->spec_tag) != hipSuccess)
        return;  // (nothing in flight that anybody will wait for)
    m->spec_inflight = true;
    m->spec_seq = seq;
    m->spec_nv = nv;
    m->spec_r = radius;
    m->spec_mutations = m->mutations.load();
}

// A scan that gave up has left its sequence number in MW_GRID, where map_status looks for calls that gave up.  Taken, the
// cleanup redoes it and says so (status_seq).  Not taken, it is nobody's call and nobody's to repeat: whoever ends its
// life without taking it -- another centre or radius, the map touched, its scratch handed to a writer, the next armed
// align -- notes the number here, and map_status, which may come while the scan is still in flight, skips that number.
static void note_scan_gave_up(lom_map *m, const uint32_t *got)  // got: in kSpecWords' order
{
    if (got[1] == m->spec_seq) m->spec_gave_up_seq = m->spec_seq;
}

void peek_cleanup_behind_align(lom_map *m)
{
    if (!m->spec_inflight) return;
    uint32_t got[kSpecWordCount];
    hipError_t e = hipSuccess;
    // (the align has returned, so the read-back is through: no wait.  A stream that failed: whoever uses it next reports it)
    if (poll_words(m, kSpecWordsOffset, m->spec_tag, kSpecWordCount, got, &e) == WORDS_ARRIVED) note_scan_gave_up(m, got);
}

void drop_cleanup_behind_align(lom_map *m)
{
    peek_cleanup_behind_align(m);
    m->spec_inflight = false;
}

// the result of a scan enqueued behind an align, if it was made for this call: true = *seq_out is the scan's sequence
// number, *kept_out the number of voxels it keeps, *grid_out its give-up word; false = not usable
static bool take_cleanup_behind_align(lom_map *m, const float center[3], float radius, uint32_t *seq_out, uint32_t *kept_out,
                                      uint32_t *grid_out)
{
    if (!m->spec_inflight) return false;
    m->spec_inflight = false;
    uint32_t got[kSpecWordCount];  // in kSpecWords' order
    hipError_t e = hipSuccess;
    // (a stream that failed: the plain path meets the same stream and reports it)
    if (poll_words(m, kSpecWordsOffset, m->spec_tag, kSpecWordCount, got, &e) != WORDS_ARRIVED) return false;
    uint32_t cb[3];
    std::memcpy(cb, center, 12);
    const bool usable = got[2] == m->spec_seq && got[3] == cb[0] && got[4] == cb[1] && got[5] == cb[2] &&
                        std::memcmp(&radius, &m->spec_r, 4) == 0 && m->call_seq == m->spec_seq &&
                        m->mutations.load() == m->spec_mutations && m->n_vox == m->spec_nv && !m->n_vox_stale;
    if (!usable) {
        note_scan_gave_up(m, got);
        return false;
    }
    *kept_out = got[0];
    *grid_out = got[1];
    *seq_out = m->spec_seq;
    return true;
}

// The back half of an erase, shared by lom_map_radius_cleanup, the ray carve and the scan votes: keep[] / newid[] of the
// `nv` slabs are in S_FLAG / S_RANK and `n_keep` of them are kept.  Few holes: the erased voxels' slabs are emptied in place
// (k_cleanup_mark); holes from a quarter of the slabs on (or LOM_DENSE_CLEANUP): compaction and a rebuilt table.
static int erase_unkept(lom_map *m, uint32_t nv, uint32_t n_keep)
{
    int rc;
    uint32_t *keep = m->scr[S_FLAG].as<uint32_t>(), *newid = m->scr[S_RANK].as<uint32_t>();
    const uint32_t n_live = nv - m->n_dead;
    if (n_keep == n_live) return LOM_OK;
    if (!m->opt_dense_cleanup && (uint64_t)(nv - n_keep) * 4u <= (uint64_t)nv) {
        // few holes: the erased voxels' slabs stay where they are, empty (see k_cleanup_mark)
        const MapView v = view_of(m);
        hipLaunchKernelGGL(k_cleanup_mark, dim3(blocks_for(nv)), dim3(kThreads), 0, m->stream, m->d_table, v.mask, v.shift, keep, nv,
                           m->slabs.key, m->slabs.count);
        LOM_HIP(m, hipGetLastError());
        m->n_dead = nv - n_keep;
        m->dead_below = nv;
        return LOM_OK;
    }
    // stable compaction into the second (persistent) set of slab arrays, swap, rebuild the table
    if (m->alt.cap != m->slabs.cap) {
        LOM_HIP(m, hipStreamSynchronize(m->stream));
        slabs_free(m->alt);
        if ((rc = slabs_alloc(m, m->slabs.cap, m->alt)) != LOM_OK) return rc;
    }
    const size_t work = (size_t)nv * m->K;
    hipLaunchKernelGGL(k_compact, dim3(blocks_for(work)), dim3(kThreads), 0, m->stream, keep, newid, nv, m->K,
                       m->slabs.key, m->slabs.count, m->slabs.pts, m->slabs.nrm, m->alt.key, m->alt.count, m->alt.pts,
                       m->alt.nrm, d_word(m, MW_NVOX), n_keep);
    LOM_HIP(m, hipGetLastError());
    std::swap(m->slabs, m->alt);  // (of equal capacity)
    m->n_vox = n_keep;
    m->n_vox_ub = n_keep;
    m->n_dead = 0;  // (the holes are closed)
    return table_rebuild(m, n_keep);
}

// ---- the erase for a decision made elsewhere (lom_internal.hpp; map_carve.hip, vote.hip) -------------------------------
int map_settle_nvox(lom_map *m) { return refresh_nvox(m); }

int erase_begin(lom_map *m, uint32_t **keep)
{
    int rc;
    const uint32_t nv = m->n_vox;
    *keep = nullptr;
    if (nv) {
        uint32_t *newid = nullptr, *scan_tmp = nullptr;
        if ((rc = scan_temps(m, (size_t)nv * 2, nv, keep, &newid, &scan_tmp)) != LOM_OK) return rc;
    }
    // keep / newid go where a cleanup scan armed behind an align may have left its own: that scan is never taken now
    // (scan_temps has said so; an empty map has not asked it)
    drop_cleanup_behind_align(m);
    ++m->call_seq;
    m->mutations++;
    return LOM_OK;
}

int erase_rank(lom_map *m, const uint32_t **d_kept)
{
    *d_kept = d_word(m, MW_COUNT);
    return scan_u32(m, m->scr[S_FLAG].as<uint32_t>(), m->scr[S_RANK].as<uint32_t>(), m->n_vox, d_word(m, MW_COUNT),
                    m->scr[S_SCAN].as<uint32_t>());
}

int erase_finish(lom_map *m, uint32_t n_keep) { return erase_unkept(m, m->n_vox, n_keep); }

}  // namespace lom

using namespace lom;

extern "C" {

int lom_map_radius_cleanup_after_align(lom_map *m, float radius)
{
    if (!m) return LOM_ERR_ARG;
    m->spec_radius = (radius > 0.f && !m->parent) ? radius : 0.f;
    return LOM_OK;
}

int lom_map_radius_cleanup(lom_map *m, const float center[3], float radius)
{
    if (!m || !center) return LOM_ERR_ARG;
    LOM_HIP(m, hipSetDevice(m->device));
    int rc;
    if ((rc = refresh_nvox(m)) != LOM_OK) return rc;
    uint32_t seq = 0, n_keep = 0, grid = 0;
    const bool taken = take_cleanup_behind_align(m, center, radius, &seq, &n_keep, &grid);
    if (m->n_vox == 0) return LOM_OK;
    const uint32_t nv = m->n_vox;
    // (twice what this call needs: a scan enqueued behind an align does not allocate, a growing keyframe should not
    // outgrow the scratch every few frames)
    // (a scan that has been taken left its flags and new slab numbers in these two: they stay as they are)
    uint32_t *keep, *newid, *scan_tmp;
    if ((rc = scan_temps(m, taken ? 0 : (size_t)nv * 2, nv, &keep, &newid, &scan_tmp)) != LOM_OK) return rc;
    const float r2 = radius * radius;  // voxel_grid.h:238
    if (!taken) seq = ++m->call_seq;
    m->mutations++;
    bool one_pass = true;
    WordsRead r;
    if (!taken) {
        one_pass = launch_cleanup_scan(m, nv, center, r2, seq, nullptr);
        if (!one_pass && (rc = cleanup_scan_multi_launch(m, nv, center, r2)) != LOM_OK) return rc;
        LOM_HIP(m, hipGetLastError());
        if ((rc = read_words(m, MW_COUNT, MW_GRID, &r)) != LOM_OK) return rc;
        n_keep = r[MW_COUNT];
        grid = r[MW_GRID];
    } else {
        m->cleanups_taken++;
    }
    if (one_pass && grid == seq) {
        // the in-kernel scan gave up (it has written scratch only): flags + multi-launch scan instead
        m->grid_redos++;
        m->status_seq = std::max(m->status_seq, seq);
        if ((rc = cleanup_scan_multi_launch(m, nv, center, r2)) != LOM_OK) return rc;
        if ((rc = read_words(m, MW_COUNT, MW_COUNT, &r)) != LOM_OK) return rc;
        n_keep = r[MW_COUNT];
    }
    return erase_unkept(m, nv, n_keep);
}

}  // extern "C"
