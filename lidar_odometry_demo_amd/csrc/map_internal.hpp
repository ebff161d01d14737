// What the five files of the voxel map share and nobody else needs (the rest of the library sees lom_internal.hpp):
//
//   voxel_map.hip   table and slabs, status words and their read-back, settle / pending / redo, the scan service, host
//                   staging, the entries that are only state          (k_table.hpp, k_scan.hpp)
//   map_insert.hip  the three insert paths                            (k_insert.hpp, k_bulk_insert.hpp)
//   map_erase.hip   radius cleanup, its scan behind an align, the erase back end (k_cleanup.hpp)
//   map_carve.hip   ray carving                                       (k_carve.hpp)
//   map_cloud.hip   down-samplers, export, upload, transform          (k_downsample_export.hpp)
//
// A kernel header belongs to one file, and a kernel is named only there; a file that needs another's kernel calls the
// owner's host function below.  Host code only.
#pragma once
#include "grid_scan.hpp"
#include "lom_internal.hpp"

namespace lom {

// ---- lom_map::scr[]: the map-maintenance scratch ------------------------------------------------------------------
// Grow-only device buffers, indexed by the S_* enum (lom_internal.hpp); the five map files are the only ones that touch
// them.  Most slots have one user.  The shared ones, by operation (element type: meaning):
//
//   slot      | insert, 4 kernels       | bulk insert               | radius cleanup     | down-sampler            | export / upload / transform
//   ----------+-------------------------+---------------------------+--------------------+-------------------------+----------------------------
//   S_IN_XYZ  | staged host points      | staged host points        |                    | staged host points      | f32[3]: exported / uploaded / transformed xyz
//   S_IN_NRM  | staged host normals     | staged host normals       |                    | staged host normals     | f32[3]: ... normals
//   S_PT_SLOT | u32: slot per point     | uint2: slot, old count    |                    | u32: slot per point     |
//   S_PT_POS  | u32: arrival position   | uint4: partition records  |                    | f32[3]: kept normals    |
//   S_FLAG    | u64: head flags (multi- | u32: bitmap of first      | u32: keep          | u32: flags (multi-      | u32: counts per slab
//             |   launch form only)     |   appearances             |                    |   launch form only)     |
//   S_RANK    | u64: their scan (ditto) | u32: bitmap word prefixes | u32: newid         | u32: ranks (ditto)      | u32: offsets per slab
//   S_PT_OFF  | u32: bucket offset      | u32: ent_idx              |                    |                         |
//   S_PT_M    | u32: bucket size        | u32: ent_w                |                    |                         |
//   S_ITEMS   | u32: bucket lists       |                           |                    | f32[3]: kept xyz        |
//   S_SCAN    | u64: scan temporaries   |                           | u32: scan temp.    | u32: scan temporaries   | u32: scan temporaries
//
// So S_FLAG / S_RANK carry five meanings and S_PT_POS three.  Within a call, call order keeps them apart.  One user
// leaves them behind for a LATER call: the cleanup scan enqueued behind an align (cleanup_scan_behind_align) leaves keep /
// newid in S_FLAG / S_RANK for the next lom_map_radius_cleanup to take.  So whoever is handed S_FLAG / S_RANK to write --
// scan_temps with room > 0, and bulk_scratch (map_insert.hip), the one user that grows them itself -- drops that scan first
// (drop_cleanup_behind_align): the cleanup then runs its own.  Readers of the map, and users of other slots, leave it
// takeable (tests/test_map_call_order_gpu.py walks every public call through that gap).
// Ray carving (k_carve.hpp) keeps cross / hit / its status words in slots of its own (S_CARVE_*) and uses S_FLAG / S_RANK /
// S_SCAN exactly as the radius cleanup does (keep, newid, scan temporaries).
// S_BKT_* and S_DS_HEAD are per table slot and kept "at rest" between calls (ensure_rest); S_MISC holds the status
// words and, behind them, the block aggregates of the single-pass kernels: map_words.hpp.

inline uint32_t *d_words(lom_map *m) { return m->scr[S_MISC].as<uint32_t>(); }  // what a kernel takes as `words`
inline uint32_t *d_word(lom_map *m, MapWord w) { return d_words(m) + w; }
inline Granule *d_agg(lom_map *m) { return (Granule *)(m->scr[S_MISC].as<char>() + kMapWordsBytes); }

// scratch slot `slot` grown to `count` elements of T
template <class T>
int scratch(lom_map *m, int slot, size_t count, T **out)
{
    const int rc = ensure(m, m->scr[slot], count * sizeof(T));
    *out = m->scr[slot].as<T>();
    return rc;
}

// ---- voxel_map.hip ---------------------------------------------------------------------------------------------------
uint32_t next_pow2(uint64_t v);
int rehash(lom_map *m, uint32_t new_cap);
void slabs_free(Slabs &s);
int slabs_alloc(lom_map *m, uint32_t cap, Slabs &s);
int ensure_slabs(lom_map *m, uint64_t want);
// k_table_init, then k_rebuild over the first n_vox slabs (after a compaction)
int table_rebuild(lom_map *m, uint32_t n_vox);
// grow-only scratch that is kept at rest (every byte == fill) between calls
int ensure_rest(lom_map *m, DeviceBuf &b, size_t bytes, int fill);

// the status words first .. last (consecutive) in ONE read-back on the handle's stream; a word by its name afterwards
struct WordsRead {
    int first = 0;
    uint32_t v[8] = {};
    uint32_t operator[](MapWord w) const { return v[w - first]; }
};
int read_words(lom_map *m, MapWord first, MapWord last, WordsRead *out);
// k_gather_words alone: n device words as {word, tag} pairs to byte `offset` of the handle's report block
hipError_t launch_gather_words(lom_map *m, const uint32_t *const *ptrs, int n, size_t offset, uint32_t tag);
// ... and the host's side: wait for the n words tagged `tag` at `offset`.  Not arrived although the stream is idle, and
// a stream that failed (*err), are the caller's to word.
enum WordsPoll { WORDS_ARRIVED, WORDS_MISSING, WORDS_STREAM_FAILED };
WordsPoll poll_words(lom_map *m, size_t offset, uint32_t tag, int n, uint32_t *out, hipError_t *err);

int refresh_nvox(lom_map *m);  // exact voxel count on the host (waits for pending inserts of this handle)
int map_status(lom_map *m);    // deferred verdict of the calls enqueued since the last check; redoes an insert that gave up
void set_pending(lom_map *m, const char *d_xyz, const char *d_nrm, size_t n, size_t stride, uint32_t seq);
void note_insert_enqueued(lom_map *m, uint64_t worst);
uint32_t take_test_fail_from(lom_map *m);  // one-shot test hook (LOM_OPT_TEST_GRID_GIVE_UP)

// the scan service: out[i] = sum in[0..i), *d_total = sum of all; tmp holds scan_tmp_words(n) elements
size_t scan_tmp_words(uint32_t n);
int scan_u32(lom_map *m, const uint32_t *in, uint32_t *out, uint32_t n, uint32_t *d_total, uint32_t *tmp);
int scan_u64(lom_map *m, const unsigned long long *in, unsigned long long *out, uint32_t n, unsigned long long *d_total,
             unsigned long long *tmp);
// map_erase.hip: a cleanup scan enqueued behind an align that nobody has taken yet.  Its keep / newid are about to be
// overwritten, or the call it was made for cannot follow any more: it is never taken now.  Should it have given up, its
// sequence number in MW_GRID is nobody's call: noted for map_status (spec_gave_up_seq), which looks with `peek` while
// the scan is still in flight.
void drop_cleanup_behind_align(lom_map *m);
void peek_cleanup_behind_align(lom_map *m);

// flags / their ranks / the scan's temporaries for a scan over n elements of T, from S_FLAG / S_RANK / S_SCAN: the first
// two with room for `room` elements (0: as large as they are, their contents kept -- a taken cleanup scan's; otherwise
// the caller writes them, and a cleanup scan behind an align that left its own there is dropped), the third as
// scan_tmp_words(n) asks
template <class T>
int scan_temps(lom_map *m, size_t room, uint32_t n, T **flag, T **rank, T **tmp)
{
    int rc;
    if (room) drop_cleanup_behind_align(m);
    if ((rc = scratch(m, S_FLAG, room, flag)) != LOM_OK) return rc;
    if ((rc = scratch(m, S_RANK, room, rank)) != LOM_OK) return rc;
    return scratch(m, S_SCAN, scan_tmp_words(n), tmp);
}

int stage_host_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride, const char **d_xyz,
                      const char **d_nrm);

// ---- map_insert.hip --------------------------------------------------------------------------------------------------
// sync_status: wait for the insert's verdict (LOM_ERR_RANGE when a point's index is out of range; such a
// call inserts nothing).  Without it the call only enqueues; lom_map_status() reports later.
int add_points_device(lom_map *m, const char *d_xyz, const char *d_nrm, size_t n, size_t stride, bool validated_on_host,
                      bool sync_status, bool allow_shrink = true, bool multi_launch = false);

}  // namespace lom
