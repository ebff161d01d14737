/*
 * lidar_odometry_amd.h -- C ABI of the MI355X-native scan-matching core.
 *
 * Drop-in boundary for the hot path of vovo-4K/lidar_odometry_demo: the
 * reference's VoxelGrid (src/voxel_grid.h:17-257), VoxelWithPlanes
 * (src/voxel_with_planes.h:10-36), Pose3D (src/pose_3d.h:10-59) and
 * CloudMatcher::align (src/cloud_matcher.h:15-16, src/cloud_matcher.cpp:105-178)
 * are replaced by these entry points; the ROS2 node and LidarOdometry keep
 * their C++ shape and call through include/lidar_odometry_amd.hpp (a header-only
 * mirror of the reference classes over this ABI).  See INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; never throws.
 *   - every function returns 0 (LOM_OK) or a negative lom_status; functions
 *     that return a count return int64 (negative = lom_status).
 *   - points are 3 consecutive f32 (x,y,z) every `stride_bytes` bytes
 *     (12 = packed, 16 = pcl::PointXYZ, 48 = pcl::PointNormal with the normal
 *     at byte offset 16).  Normals use the same stride.
 *   - poses are f32 {t[3], q[4] = w,x,y,z} like the reference's Pose3D.
 *   - a handle owns all device memory, one HIP stream and one pinned result
 *     buffer; it is single-caller (not internally locked).  Independent
 *     handles may be used from different threads; further callers of ONE map
 *     take a scan context each (lom_scan_create).
 *   - there is NO CPU fallback: without a gfx950 device lom_map_create fails
 *     with LOM_ERR_NO_DEVICE.
 */
#ifndef LIDAR_ODOMETRY_AMD_H
#define LIDAR_ODOMETRY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOM_ABI_VERSION 2

typedef enum {
    LOM_OK = 0,
    LOM_ERR_ARG = -1,       /* null/invalid argument                               */
    LOM_ERR_OOM = -2,       /* host or device allocation failed                    */
    LOM_ERR_RANGE = -3,     /* |coordinate / voxel_size| >= 2^20 or non-finite      */
    LOM_ERR_HIP = -4,       /* HIP runtime error, text via lom_last_error()        */
    LOM_ERR_NO_DEVICE = -5, /* no usable gfx950 device                             */
    LOM_ERR_COMM = -6,      /* RCCL error                                          */
    LOM_ERR_STATE = -7,     /* call not valid in this state                        */
    LOM_ERR_HOOK = -8       /* a user hook returned non-zero                       */
} lom_status;

int lom_abi_version(void);
/* number of visible HIP devices (0 when none; never initialises a context) */
int lom_device_count(void);
/* CPU list (sysfs syntax, e.g. "64-127,192-255") of the NUMA node a device is attached to; callers
 * that care about the latency of the host<->device round trips run on those CPUs */
int lom_device_local_cpus(int device, char *out, size_t cap);

/* ---- Pose3D (src/pose_3d.h:10-59), f32 ---------------------------------- */
typedef struct {
    float t[3];
    float q[4]; /* w, x, y, z */
} lom_pose;

void lom_pose_identity(lom_pose *out);                                         /* pose_3d.h:15-18 */
void lom_pose_compose(const lom_pose *a, const lom_pose *b, lom_pose *out);    /* :29-32 */
void lom_pose_inverse(const lom_pose *a, lom_pose *out);                       /* :34-39 */
void lom_pose_relative_to(const lom_pose *a, const lom_pose *target, lom_pose *out); /* :23-27 */
void lom_pose_rotation_matrix(const lom_pose *a, float R_rowmajor[9]);         /* :41-43 */
/* CloudTransformer::transform / transformWithNormals (src/utils/cloud_transform.h:43-97),
 * host-side f32; nrm_in/nrm_out may be NULL. */
int lom_transform_points(const lom_pose *pose, const float *xyz_in, const float *nrm_in, size_t n,
                         size_t stride_bytes_in, float *xyz_out, float *nrm_out,
                         size_t stride_bytes_out);

/* ---- VoxelGrid (src/voxel_grid.h:17-257) -------------------------------- */
typedef struct lom_map lom_map;

/* VoxelGrid(float voxel_size, size_t max_points), voxel_grid.h:48-52.
 * capacity_hint = expected number of voxels (0 = default); device = HIP device index. */
int lom_map_create(float voxel_size, size_t max_points, size_t capacity_hint, int device,
                   lom_map **out);
void lom_map_destroy(lom_map *m);
const char *lom_last_error(const lom_map *m); /* NULL handle: error of the last failed create */

int lom_map_clear(lom_map *m, float voxel_size);            /* setVoxelSize, :61-66 (clears) */
int lom_map_set_max_points(lom_map *m, size_t max_points);  /* setMaxPoints, :56-59; at any time: stored voxels keep what they hold (:86-90) */
/* addCloud (:77-93) when nrm != NULL, addCloudWithoutNormals (:95-110) when nrm == NULL.
 * Deterministic: a voxel keeps the first max_points points in call/input order. */
int lom_map_add_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride_bytes);
/* same with device-resident input (pointers valid on the handle's device) */
int lom_map_add_points_device(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n,
                              size_t stride_bytes);
/* the same, enqueued only: the range verdict (a call with a point out of range inserts nothing) is not
 * waited for; lom_map_status() waits for everything enqueued on the handle and returns the first deferred
 * error since the last check (LOM_ERR_RANGE, LOM_ERR_HIP) -- for callers that keep a frame in HBM and look at
 * the host only once per frame */
int lom_map_add_points_device_nowait(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n,
                                     size_t stride_bytes);
int lom_map_status(lom_map *m);
int lom_map_radius_cleanup(lom_map *m, const float center[3], float radius); /* :236-246 */
/* src/lidar_odometry.cpp:65-67 calls radiusCleanup with the translation the align has just returned.  A caller that will
 * do the same arms this before lom_match_align_device: the device-resident align then enqueues the cleanup's scan (it
 * only reads the map and writes scratch) behind its last solve, with the centre taken from its own result in HBM, and
 * the lom_map_radius_cleanup that follows takes that scan's result if -- and only if -- its centre and radius are
 * bit for bit what the scan used and the map has not been touched in between; otherwise it runs as if this had never
 * been called.  "Touched" is any call that changes the map (insert, cleanup, carve, votes, clear, a raised
 * lom_map_set_max_points) and any call that writes the scratch the scan's result waits in: lom_map_export and
 * lom_map_point_count.  Searches, aligns, quality reports, carve counts, scan votes, lom_map_size, lom_map_status,
 * upload and transform leave it takeable.  A scan that is not taken is never reported: should it have given up,
 * lom_map_status does not say so, since no call of the caller's failed.  One shot (the next align only), map handles only
 * (not scan contexts); results never differ. */
int lom_map_radius_cleanup_after_align(lom_map *m, float radius);
int64_t lom_map_size(const lom_map *m);        /* number of voxels, :248-251 */
int64_t lom_map_point_count(const lom_map *m); /* number of stored points */

typedef enum {
    LOM_EXPORT_FULL = 0,            /* getCloud, :112-130                       */
    LOM_EXPORT_FULL_NO_NORMALS = 1, /* getCloudWithoutNormals, :133-147         */
    LOM_EXPORT_FIRST_PER_VOXEL = 2  /* getSparseCloudWithoutNormals, :150-162   */
} lom_export_mode;
/* Packed (12-byte) host output in voxel creation order, insertion order inside a
 * voxel.  Returns the number of points the export holds; writes at most `cap`.
 * xyz_out / nrm_out may be NULL (count only). */
int64_t lom_map_export(lom_map *m, int mode, float *xyz_out, float *nrm_out, size_t cap);

/* ---- ray carving (not in the reference; nothing runs it unless asked) ------------------------------------------
 * A scan proves the voxels its rays pass through empty: lom_map_carve_rays erases the voxels that enough rays of one
 * call crossed and no endpoint of that call fell into.  The definition, operation by operation (tests/carve_ref.py
 * restates it in numpy f64 and the results are compared bit for bit):
 *
 * Inputs: a map with voxel size v (f32), an origin o and n endpoints p_i, f32, in the map's frame, and the parameters
 * below.  There are no defaults (no measured basis for any); margin < 0, min_range <= 0, max_range <= min_range, a
 * non-finite value or min_crossings == 0 is LOM_ERR_ARG.
 *
 * Range errors: a non-finite origin or endpoint, or one whose voxel index (f32 x / v, the map's own rule) leaves
 * (-2^20, 2^20), fails the call with LOM_ERR_RANGE, and so does a walk that leaves that range; the map is unchanged.
 *
 * Hits: every endpoint, whatever its ray's length, protects the voxel that contains it by the insert's index rule
 * (the correctly rounded f32 quotient x / v, truncated toward zero): if that voxel is live, hit[voxel] = 1.
 *
 * Walk, per ray, all in f64 from the f32 inputs, every operation rounded on its own (no contraction):
 *   V = (double)v, O = o, D = P - O, L = sqrt(Dx*Dx + (Dy*Dy + Dz*Dz)).
 *   If !(L >= min_range) the ray is not walked (L == 0 too).
 *   t_end = (min(L, max_range) - margin) / L.  If !(t_end > 0) the ray is not walked.
 *   Start cell c_a = (int)trunc(O_a / V) per axis a.
 *   Per axis with D_a != 0: s_a = +1 or -1, the sign of D_a; the next plane's index
 *     b_a = s_a > 0 ? (c_a >= 0 ? c_a + 1 : c_a) : (c_a <= 0 ? c_a - 1 : c_a)
 *   and t_a = ((double)b_a * V - O_a) / D_a.  With D_a == 0: t_a = +inf.
 *   (The truncating index's geometry: cell 0 spans (-V, V), there is no plane at 0.)
 *   Loop: 1. the current cell counts as crossed by this ray;
 *         2. a = the axis with the smallest t_a, ties to x before y before z;
 *         3. if !(t_a <= t_end): stop;
 *         4. c_a += s_a; b_a and t_a again from the new c_a by the formulas above (t_a is never incremented);
 *         5. if |c_a| >= 2^20: range error.
 *   A negative t_a (O_a / V rounded onto a plane) simply sorts first.  A ray visits a cell at most once.  At most
 *   3 * (ceil(max_range / V) + 2) steps can occur; the kernel's loop is bounded by that.
 *
 * Decision: cross[voxel] = the number of rays of this call that visited the live voxel; a table slot without a voxel
 * (left by an earlier erase) counts for nothing.  A voxel is erased iff it is live, cross >= min_crossings and !hit.
 * Erasing is what lom_map_radius_cleanup's erase is: an empty slab in place, or compaction once the holes are a quarter
 * of the slabs (LOM_DENSE_CLEANUP=1: always); a later insert into the voxel creates it anew at the end of the
 * creation order.  A cleanup scan armed with lom_map_radius_cleanup_after_align is never taken across a carve. */
typedef struct {
    float margin;           /* m; the walk stops this far before the endpoint; >= 0 */
    float min_range;        /* m; shorter rays are not walked; > 0 */
    float max_range;        /* m; longer rays are walked to here; > min_range */
    uint32_t min_crossings; /* >= 1: rays that must cross a voxel in this call */
} lom_carve_params;

typedef struct {
    uint64_t rays_walked, rays_skipped; /* rays_walked + rays_skipped == n */
    uint64_t cells_visited;             /* step 1 of the loop, summed over all rays */
    uint32_t voxels_crossed;            /* live voxels with cross >= 1 */
    uint32_t voxels_protected;          /* live voxels with cross >= min_crossings that a hit kept */
    uint32_t voxels_erased;
} lom_carve_stats;

/* n == 0: nothing happens, LOM_OK.  An empty map is a map like any other: the range verdict and rays_walked / cells_visited
 * are those of the definition, nothing is crossed.  On an error the stats are all zero.  Map handles only (a scan
 * context: LOM_ERR_ARG).  xyz: host memory, records of
 * stride_bytes (>= 12, a multiple of 4) that begin with x, y, z. */
int lom_map_carve_rays(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride_bytes,
                       const lom_carve_params *p, lom_carve_stats *stats_or_null);
/* the same with the endpoints in device memory (the origin stays a host array); the handle's staging buffers -- what
 * lom_transform_points_device returned -- are not touched */
int lom_map_carve_rays_device(lom_map *m, const float origin[3], const float *d_xyz, size_t n, size_t stride_bytes,
                              const lom_carve_params *p, lom_carve_stats *stats_or_null);
/* erases nothing: per live voxel, in lom_map_export's order, this call's crossing count and hit flag (host xyz).
 * Returns the number of live voxels; writes at most `cap` entries; either output may be NULL. */
int64_t lom_map_carve_counts(lom_map *m, const float origin[3], const float *xyz, size_t n, size_t stride_bytes,
                             const lom_carve_params *p, uint32_t *cross_out, uint8_t *hit_out, size_t cap);

/* The reference's down-sampling idiom in one pass: VoxelGrid(voxel_size, 1).addCloud(cloud)
 * followed by getCloud() / getCloudWithoutNormals() (src/lidar_odometry.cpp:37-38,42,46-47,50):
 * the first point of every voxel in input order, returned in order of first appearance -- exactly
 * what lom_map_create(voxel,1) + lom_map_add_points + lom_map_export(LOM_EXPORT_FULL) return.
 * `workspace` is any map handle; it is cleared and left empty.  nrm / nrm_out may be NULL
 * (nrm == NULL with nrm_out set yields zero normals, like addCloudWithoutNormals).  Returns the
 * number of voxels; writes at most `cap` points. */
int64_t lom_voxel_downsample(lom_map *workspace, float voxel_size, const float *xyz, const float *nrm, size_t n,
                             size_t stride_bytes, float *xyz_out, float *nrm_out, size_t cap);

/* ---- device-resident variants: a caller that keeps a frame in HBM (processCloud does) ---- */
/* Copy host points (and normals) into the handle's device staging buffers; the device pointers
 * stay valid until the next lom_upload_points / host-input call on this handle.  Records keep the
 * caller's stride. */
int lom_upload_points(lom_map *m, const float *xyz, const float *nrm, size_t n, size_t stride_bytes,
                      const float **d_xyz_out, const float **d_nrm_out);
/* lom_voxel_downsample with input and output in device memory: returns the number of voxels and
 * device pointers to packed 12-byte points (and normals, if d_nrm_out != NULL; zero normals when
 * d_nrm == NULL) inside the workspace handle, valid until the next call on that workspace. */
int64_t lom_voxel_downsample_device(lom_map *workspace, float voxel_size, const float *d_xyz, const float *d_nrm,
                                    size_t n, size_t stride_bytes, const float **d_xyz_out,
                                    const float **d_nrm_out);
/* the same, enqueued only: the input size may live on the device (*d_n, with n_bound its upper bound known
 * to the host, <= 262144 then; d_n == NULL: n_bound points), and the number of voxels is left in a device word
 * (*d_count_out) for the kernels that consume the result; lom_map_status() reports a point out of range. */
int lom_voxel_downsample_device_nowait(lom_map *workspace, float voxel_size, const float *d_xyz, const float *d_nrm,
                                       size_t n_bound, const uint32_t *d_n, size_t stride_bytes,
                                       const float **d_xyz_out, const float **d_nrm_out, const uint32_t **d_count_out);
/* for callers that fold a handle's deferred verdict into a read-back of their own: device words that hold the
 * sequence number of the last call that failed (range / a grid time-out) and the sequence number of the
 * handle's last call -- a word equal to *seq means that call failed */
int lom_map_status_words(lom_map *m, const uint32_t **d_range, const uint32_t **d_grid, uint32_t *seq);
/* up to 32 device words of any handle, read behind everything enqueued so far on this handle's stream: one
 * single-wave kernel that stores them into the handle's pinned block, no copy engine.  _begin enqueues it,
 * _end waits for its words (one read in flight per handle; work enqueued between the two does not delay it);
 * lom_map_read_device_words is both. */
int lom_map_read_device_words(lom_map *m, const uint32_t *const *d_ptrs, int n, uint32_t *out);
int lom_map_read_device_words_begin(lom_map *m, const uint32_t *const *d_ptrs, int n);
int lom_map_read_device_words_end(lom_map *m, uint32_t *out);
/* lom_transform_points on the device (same f32 arithmetic): packed 12-byte output in the handle's
 * staging buffers, valid until the next upload / host-input call on this handle. */
int lom_transform_points_device(lom_map *m, const lom_pose *pose, const float *d_xyz, const float *d_nrm, size_t n,
                                size_t stride_bytes, const float **d_xyz_out, const float **d_nrm_out);

/* ---- getCorrespondence / findMatchingPairs (voxel_grid.h:164-234) -------- */
typedef struct {
    int64_t index;   /* voxel_creation_index * max_points + in_voxel_index, or -1 */
    float origin[3]; /* Correspondence::plane_origin  */
    float normal[3]; /* Correspondence::plane_normal  */
    float sq_dist;   /* f32 squared distance to the winner (0 if none) */
    uint32_t n_cand; /* stored points scanned for this query */
    uint32_t n_occ;  /* occupied voxels among the 27 neighbours */
} lom_correspondence;

/* Deterministic findMatchingPairs: one entry per source point, in source order
 * (the reference's push order under its mutex is nondeterministic).  Returns the
 * number of valid correspondences. */
int64_t lom_match_find_pairs(lom_map *m, const float *src_xyz, size_t n, size_t stride_bytes,
                             const float t[3], const float q_wxyz[4], float max_dist,
                             lom_correspondence *out);
/* The same search with the SQUARED threshold handed over as the reference's getCorrespondence takes it
 * (`double max_correspondence_distance_sq`, src/voxel_grid.h:164): a stored point is accepted iff
 * (double)(f32 squared distance) < max_dist_sq (:184-186).  lom_match_find_pairs squares its f32 argument in f32, as
 * findMatchingPairs does (:215); callers that hold a squared threshold use this entry instead of taking a root. */
int64_t lom_match_find_pairs_sq(lom_map *m, const float *src_xyz, size_t n, size_t stride_bytes,
                                const float t[3], const float q_wxyz[4], double max_dist_sq,
                                lom_correspondence *out);
/* Parity entry for the temporal pruning bound of the align's searches (csrc/match.hip, csrc/align.hip): a search at the pose
 * (t_prev, q_prev), then the search at (t, q) with the first one's winners as upper bounds -- what outer iterations
 * >= 2 of an align run.  The result must equal lom_match_find_pairs at (t, q) entry for entry, whatever the two poses
 * are (a winner that has left a query's 27 voxels is found out and that query searched again at the plain bound). */
int64_t lom_debug_find_pairs_after(lom_map *m, const float *src_xyz, size_t n, size_t stride_bytes,
                                   const float t_prev[3], const float q_prev_wxyz[4], const float t[3],
                                   const float q_wxyz[4], float max_dist, lom_correspondence *out);

/* ---- CloudMatcher::align (src/cloud_matcher.cpp:105-178) ---------------- */
/* Reduced normal equations produced per evaluation (f64):
 * [0..20] upper triangle (row-major, a<=b) of sum w J J^T, tangent order
 * rotation(3), translation(3); [21..26] sum w J r; [27] sum 0.5*rho(r^2);
 * [28] valid correspondences; [29] stored points scanned; [30] occupied
 * neighbour voxels; [31] source points searched.  The translation prior is NOT
 * included. */
#define LOM_NSUMS 32

typedef struct {
    int32_t outer_iterations;  /* executed outer iterations (<=35)                  */
    int32_t lm_iterations;     /* recorded LM iterations incl. iteration 0, total   */
    int32_t evaluations;       /* residual evaluations, total                       */
    int32_t match_launches;    /* correspondence-kernel launches (= outer its)      */
    int64_t queries;           /* source points x outer iterations (this rank)      */
    int64_t valid_last;        /* valid correspondences of the last outer iteration */
    int64_t cand_total;        /* stored points scanned, all outer iterations       */
    int64_t occ_total;         /* occupied neighbour voxels, all outer iterations   */
    double final_cost;
    double last_step_norm;
    double match_kernel_ms;    /* HIP-event time of the correspondence launches (profiling on) */
    double algorithmic_bytes;  /* sum over queries of 444 + 12*cand + 12*valid     */
    double host_launch_ms;     /* host time spent inside kernel-launch calls                   */
    double host_wait_ms;       /* host time spent waiting for evaluation results               */
    int64_t profiled_launches; /* correspondence launches that carried the HIP event pair      */
    int32_t host_fallback;     /* 1: the device-resident loop gave up (its workgroups were not all
                                  resident in time) and the align was redone by the host-driven loop */
    int32_t lm_workgroups;     /* workgroups of the device-resident solve kernel (k_lm), one per CU: the CUs a solve keeps busy */
    double lm_kernel_ms;          /* HIP-event time of the k_lm launches of the device-resident loop (profiling on) */
    int64_t lm_profiled_launches; /* k_lm launches that carried the events                                        */
} lom_align_stats;

/* Replaces CloudMatcher::align (cloud_matcher.h:15-16): up to 35 outer iterations of
 * {correspondence search, Levenberg-Marquardt solve with max 4 iterations}, f32 pose write-back and
 * the reference's stop rule.  On one GPU the whole loop runs on the device (a chain of kernels
 * enqueued ahead of time, pose handed from kernel to kernel in HBM); with an attached exchange
 * (below) or LOM_HOST_LM=1 in the environment the loop is driven from the host, one round trip per
 * LM iteration.  Same policy source either way (csrc/lm_core.hpp).  Zero correspondences is not an
 * error: the prior-only problem is solved and the pose stays at the guess. */
int lom_match_align(lom_map *m, const float *src_xyz, size_t n, size_t stride_bytes,
                    const float guess_t[3], const float guess_q_wxyz[4], float out_t[3],
                    float out_q_wxyz[4], lom_align_stats *stats_or_null);
/* same, source cloud already resident on the handle's device */
int lom_match_align_device(lom_map *m, const float *d_src_xyz, size_t n, size_t stride_bytes,
                           const float guess_t[3], const float guess_q_wxyz[4], float out_t[3],
                           float out_q_wxyz[4], lom_align_stats *stats_or_null);

/* `reps` independent aligns of the same device-resident scan from the same guess, back to back, as
 * a compiled caller would issue them; `total` accumulates the counters and times of all of them
 * (valid_last / final_cost / last_step_norm are the last align's).  Used by bench.py so that the
 * timed region holds the hot path and not an interpreter's per-call overhead. */
int lom_match_align_repeat(lom_map *m, const float *d_src_xyz, size_t n, size_t stride_bytes,
                           const float guess_t[3], const float guess_q_wxyz[4], int reps, float out_t[3],
                           float out_q_wxyz[4], lom_align_stats *total_or_null);

/* ---- batched align: K (scan, guess) problems against ONE keyframe in one call ------------------------- */
/* Multi-hypothesis alignment (one scan from K guesses: relocalisation, loop-closure checks), several scans of a rig, the
 * reference's MatchingTest: CloudMatcher::align takes `const VoxelGrid&` (cloud_matcher.h:15-16), so all are legal
 * against one map at once.  The K solves run side by side in one device-resident chain -- one correspondence launch and
 * one solve launch per outer iteration for all problems of a round (csrc/align_batch.hip "batched align").  Problems may share
 * a cloud pointer and may differ in n (0 and 1 included).  Every result is BIT FOR BIT what lom_match_align* returns for
 * that (scan, guess) on the same handle, its counters included. */
typedef struct {
    const float *xyz;          /* host pointer (lom_*_align_batch) or device pointer (lom_*_align_batch_device) */
    size_t n, stride_bytes;
    float guess_t[3], guess_q_wxyz[4];
} lom_align_problem;

typedef struct {
    float t[3], q_wxyz[4];     /* the pose lom_match_align would return for this problem */
    /* its stats: the counting fields (outer_iterations, lm_iterations, evaluations, match_launches, queries, valid_last,
     * cand_total, occ_total, algorithmic_bytes, final_cost, last_step_norm, lm_workgroups) equal the single align's;
     * host_fallback = 1 where this problem's solve gave up and it was redone alone through lom_match_align_device;
     * the profiling fields read 0; host_launch_ms / host_wait_ms hold the whole call's times */
    lom_align_stats stats;
    int32_t round;             /* the round of the device-resident batch this problem ran in (0, 1, ...; rounds of one
                                  call run one after another), -1 where the batch ran problem by problem */
    int32_t pad;
} lom_align_result;

/* out[i] for p[i]; best_or_null: lom_align_batch_best(out, count).  count == 0 is valid (best = -1).
 * With LOM_OPT_HOST_LM = 1 or an attached rank exchange the problems are aligned one after another through
 * lom_match_align* (the same results by definition).  The batch has buffers of its own: the single align's state, a
 * lom_map_radius_cleanup_after_align and an idle hook armed for the next single align are neither used nor consumed.
 * LOM_OPT_TEST_GIVE_UP_AT_OUTER applies to the first problem of the first round only. */
int lom_match_align_batch(lom_map *m, const lom_align_problem *p, int count, lom_align_result *out, int *best_or_null);
int lom_match_align_batch_device(lom_map *m, const lom_align_problem *p, int count, lom_align_result *out,
                                 int *best_or_null);
/* the best result (host code, no GPU): the most valid_last; ties go to the lower final_cost, then to the lower index;
 * -1 if count <= 0 or r == NULL */
int lom_align_batch_best(const lom_align_result *r, int count);

/* ---- multi-map align: K (scan, guess) problems, each against a keyframe of its own, in one call -------------------- */
/* Many independent streams on one GPU (a dataset of drives, several robots): each problem names its map, and the K solves
 * run side by side in one device-resident chain on `runner`'s stream, as lom_match_align_batch's do.
 * Same answers: out[i] is BIT FOR BIT what lom_match_align* (p[i].map, ...) returns for that scan and guess -- the pose
 *   bytes and the counting fields (see lom_align_result) -- the promise lom_match_align_batch makes.
 * Maps may repeat, and may differ in voxel size, max points per voxel, size and LOM_OPT_COUNT_CANDIDATES.  Problems are
 *   grouped by (solve variant, counted or not); each keeps the solve grid its single align would use, and a round holds
 *   as many as are resident together (LOM_OPT_TEST_BATCH_ROUND_MAX of the runner caps it).
 * Arguments: LOM_ERR_ARG before any work for a NULL runner, count < 0, NULL p or out with count > 0, a NULL map, or a map
 *   on another device than runner; count == 0 is valid (best = -1); *best_or_null is left alone on an error.
 * Settling: every map is settled (its pending insert verified) before anything is launched; a map whose pending insert
 *   fails fails the call first, its error in runner's lom_last_error with the problem's index.
 * Stream order: runner's stream waits for the work already enqueued on every problem map's stream (a _nowait insert, a
 *   cleanup); before the call returns every problem map's stream is ordered behind the chain's last launch, so that a
 *   later insert or cleanup on a map cannot overtake the search.
 * Problems whose map has LOM_OPT_HOST_LM or an attached exchange run through that map's own single align, one after
 *   another (round = -1); a problem whose solve gave up is redone alone on its own map (host_fallback = 1).
 *   LOM_OPT_TEST_GIVE_UP_AT_OUTER of a map applies to that map's first device-resident problem.
 * Isolation as lom_match_align_batch, for every handle involved: armed radius cleanups and idle hooks stay armed, the
 *   single align's state is not touched. */
typedef struct {
    lom_map *map;              /* the keyframe this problem aligns against */
    const float *xyz;          /* host (lom_match_align_multi) or device (..._device) pointer */
    size_t n, stride_bytes;
    float guess_t[3], guess_q_wxyz[4];
} lom_align_multi_problem;
/* `runner`: the handle whose stream and batch buffers carry the chain; it may or may not be one of the problems' maps */
int lom_match_align_multi(lom_map *runner, const lom_align_multi_problem *p, int count, lom_align_result *out,
                          int *best_or_null);
int lom_match_align_multi_device(lom_map *runner, const lom_align_multi_problem *p, int count, lom_align_result *out,
                                 int *best_or_null);

/* Diagnostic build of the correspondence kernel with shader-clock stamps after each phase of every
 * workgroup's first query (8 u64 per workgroup: entry, point transformed, slots probed, prefix in
 * LDS, candidates scanned, minimum known, record stored, exit).  Not a timing of the product kernel. */
int lom_debug_match_stamps(lom_map *m, const float *d_src_xyz, size_t n, size_t stride_bytes, const float t[3],
                           const float q_wxyz[4], float max_dist, unsigned long long *stamps_out,
                           size_t cap_blocks, uint32_t *n_blocks_out);

/* Parity entries for PointToPlaneErrorAnalytic::Evaluate (src/cloud_matcher.cpp:38-103) and the reduction
 * ceres::Solve performs inside the reference (the tests compare them with the oracle sum by sum).
 * lom_debug_eval_sums: one correspondence search at the f32 pose (pose_t, pose_q) with the align's 0.3 m
 * gate, then ONE evaluation of the LOM_NSUMS reduced sums at the f64 point (q, t) -- q need not be a unit
 * quaternion, exactly as inside an align -- through the kernels of the host-driven path. */
int lom_debug_eval_sums(lom_map *m, const float *src_xyz, size_t n, size_t stride_bytes, const float pose_t[3],
                        const float pose_q_wxyz[4], const double q[4], const double t[3], double out[LOM_NSUMS]);
/* lom_debug_lm_trace: lom_match_align on the device-resident path, also returning what the LM policy
 * inside k_lm saw during outer iteration `outer_index`: trace_out[e * 40 + 0..6] = the point [q, t] of
 * evaluation e, trace_out[e * 40 + 8 .. + 39] = its LOM_NSUMS totals (after the in-kernel reduction and
 * exchange); *n_evals_out = evaluations of that solve (<= 5; 0 when the align ended earlier).
 * trace_out holds 200 doubles. */
int lom_debug_lm_trace(lom_map *m, const float *src_xyz, size_t n, size_t stride_bytes, const float guess_t[3],
                       const float guess_q_wxyz[4], int outer_index, double *trace_out, int *n_evals_out,
                       float out_t[3], float out_q_wxyz[4], lom_align_stats *stats_or_null);
/* Outer iterations of the LAST device-resident lom_match_align* on this handle that the replay fold (LOM_OPT_REPLAY_FOLD)
 * accounted for without running them: lom_align_stats.outer_iterations minus this many (k_match, k_lm) pairs did work.
 * 0 after an align that took the host-driven loop. */
int lom_debug_replayed_iterations(lom_map *m);
/* The host driver's replay fold (lom_align_with_hooks: same rule, same function, csrc/lm_core.hpp), process-wide, default
 * on; it never folds when hooks->allreduce is set.  Returns the previous setting.  For the tests. */
int lom_debug_set_host_replay_fold(int on);
/* The fold rule itself (csrc/lm_core.hpp, replay_fold_count; host code, no GPU): `outer` iterations are done, the last of
 * them with `last_step_norm`; how many further iterations the reference's loop (cloud_matcher.cpp:117, :169-172) executes
 * if each repeats that one. */
int lom_debug_replay_fold_count(int outer, double last_step_norm);
/* lom_debug_lm_policy: one form of the Levenberg-Marquardt policy of a solve, run on GIVEN sums (the policy sees
 * nothing else of a scan or a map; no handle is needed).  form 0: csrc/lm_core.hpp on the host (no GPU needed);
 * 1: csrc/lm_wave.hpp's first wave form; 2 / 3: the forms k_lm runs in its 512- / 256-thread shapes.  Forms 1-3 replay
 * all n_solves solves on one 64-lane workgroup in one launch on the current device.
 * Per solve s: n_evals[s] (1..5) evaluations are available, x0[s*7..] = the start point [qw qx qy qz tx ty tz],
 * prior_b[s*3..], sums[(s*5 + e)*32 ..] = the LOM_NSUMS block of evaluation e (prior excluded).  Evaluation 0 is fed to
 * the policy's begin, the others to its feed, until the policy answers 0 (done) or the evaluations run out.
 * action_out[s*5 + e] = 1 (evaluate the point point_out[(s*5 + e)*7 ..] next) or 0 (done: point_out = the solution),
 * -1 for evaluations not replayed.  recorded_out / evaluations_out / last_step_norm_out / cost_out [s]: the solve's
 * results as lom_align_stats counts them. */
int lom_debug_lm_policy(int form, int n_solves, const int *n_evals, const double *x0, const double *prior_b,
                        const double *sums, int *action_out, double *point_out, int *recorded_out,
                        int *evaluations_out, double *last_step_norm_out, double *cost_out);

/* Record a HIP event pair around the correspondence launches of lom_match_align*
 * (stats->match_kernel_ms over stats->profiled_launches launches).  `period` = 0: off; 1: every
 * align; N: every N-th align of this handle (an event pair costs the stream ~5 us per launch --
 * sampling keeps a live in-loop measurement from distorting the loop it measures). */
int lom_map_set_profiling(lom_map *m, int period);
/* Roofline probe: `reps` back-to-back launches of the correspondence kernel on a device-resident
 * scan at pose (t,q), bracketed by ONE HIP event pair on the handle's stream, so the per-event
 * packet overhead is amortised.  Returns the average launch duration in microseconds and the
 * algorithmic bytes of one launch (SURVEY.md 8d formula, counted by the kernel), and optionally the
 * bytes the kernel itself requests (candidates of pruned voxels are not read; + 52 B of output per
 * query).  pair_avg_us_out (optional): the average of the same launches bracketed by one event pair EACH --
 * minus avg_us_out that is what an event pair adds to one short kernel, the correction for the sampled
 * in-loop measurement of lom_match_align*. */
int lom_profile_match(lom_map *m, const float *d_src_xyz, size_t n, size_t stride_bytes, const float t[3],
                      const float q_wxyz[4], float max_dist, int reps, double *avg_us_out,
                      double *algorithmic_bytes_out, double *requested_bytes_out, double *pair_avg_us_out);
/* Roofline probe for the insert chain: lom_map_add_points_device bracketed by one HIP event pair on the handle's
 * stream (all kernels of the insert, no host wait in between); microseconds from the first kernel to the last. */
int lom_profile_insert(lom_map *m, const float *d_xyz, const float *d_nrm, size_t n, size_t stride_bytes,
                       double *total_us_out);
/* Run-time switches of a handle.  The environment is read ONCE, by lom_map_create (LOM_HOST_LM, LOM_DEBUG_LM,
 * LOM_DEBUG_TIMING: the production-side switches); afterwards only this call changes them -- nothing on the
 * align path looks at the environment.  Options of the 100 range exist for the tests. */
typedef enum {
    LOM_OPT_HOST_LM = 1,               /* 1: outer loop and LM policy on the host (one round trip per LM iteration) */
    LOM_OPT_DEVICE_PATIENCE_TICKS = 2, /* bound of every in-kernel wait, ticks of 10 ns; default 5,000,000 = 50 ms.
                                          Waits for a peer RANK take ten times that; the host-side agreement after
                                          a device-to-device align outlasts both (see lom_comm_attach_p2p).  A patience
                                          below 40 ticks -- shorter than the head start k_lm's gather sleeps before its
                                          first poll -- counts as timed out whatever the poll would find: that is what
                                          makes "1 tick" a deterministic way for the tests to force the give-up path, and
                                          it means values below 0.4 us are not a usable patience for anything else. */
    LOM_OPT_DEBUG_LM_STAMPS = 3,       /* 1: print k_lm's phase stamps after every align (stderr) */
    LOM_OPT_DEBUG_TIMING = 4,          /* 1: print host launch / wait times per evaluation (stderr) */
    LOM_OPT_NO_TEMPORAL_BOUND = 5,     /* 1: every correspondence search prunes at max_dist only.  Default 0: the searches
                                          of outer iterations >= 2 of an align also prune with the previous iteration's
                                          winner (exact, verified per query: csrc/k_match.hpp "temporal bound"); results
                                          are the same either way, this switch exists for A/B timing (LOM_NO_TEMPORAL=1
                                          in the environment at create) */
    LOM_OPT_COUNT_CANDIDATES = 6,      /* 1: every search also produces the counts of the reference ALGORITHM -- occupied voxels
                                          among the 27 neighbours and their stored points, per query (lom_correspondence.n_cand
                                          / n_occ) and summed (lom_align_stats.cand_total / occ_total / algorithmic_bytes: SURVEY
                                          8d's cand(q)) -- which takes all 27 slot loads per query.  Default 0: a neighbour voxel
                                          that the distance bound prunes is not looked up at all (same winners, same poses: the
                                          result cannot depend on a voxel none of whose points could win) and those fields read
                                          0.  LOM_COUNT_CANDIDATES=1 in the environment at create.  bench.py times the default
                                          and takes the algorithmic bytes from a counted replay of the same align. */
    LOM_OPT_NO_BULK_INSERT = 7,        /* 1: inserts of more than 65,536 points take the four-kernel path of the smaller ones
                                          (three device-scope atomics per point) instead of the partitioned bulk insert
                                          (csrc/map_insert.hip, add_points_bulk).  Same map either way, bytewise; the switch exists
                                          for A/B timing (LOM_NO_BULK_INSERT=1 in the environment at create) */
    LOM_OPT_QUALITY_REPORT = 8,        /* lom_odometry_set_option only.  1: every frame that runs an align is followed by
                                          lom_match_quality_device on its matching cloud (still in HBM) at the pose the
                                          align returned -- before the unstable-rotation override -- with the align's 0.3 m
                                          gate; lom_odometry_get_quality hands out the last frame's report.  Default 0:
                                          no extra launches, the same pose bytes */
    LOM_OPT_REPLAY_FOLD = 9,           /* Default 1: the single device-resident align accounts for repeated outer iterations
                                          instead of running them.  An outer iteration is a pure function of the f32 pose
                                          it searches at; one that writes back that very pose is followed, in the reference,
                                          by exact repeats of itself until the stop rule (which cannot fire before the fifth
                                          iteration) ends the loop.  Pose bytes and every field of lom_align_stats are the
                                          same either way -- the statistics describe the reference algorithm's align, folded
                                          iterations included; lom_debug_replayed_iterations tells how many were folded.
                                          0: every iteration runs (A/B timing, tests).  Never folds: the batched / multi-map
                                          aligns, aligns whose ranks exchange sums (more than one rank), and an align that carries the profiling
                                          events (lom_map_set_profiling: every bracketed launch runs) */
    LOM_OPT_TEST_GIVE_UP_AT_OUTER = 100, /* k: the k_lm of outer iteration k of the NEXT align behaves as if its
                                          workgroups had timed out waiting (one shot; -1 = off) */
    LOM_OPT_TEST_GRID_GIVE_UP = 101,   /* b >= 0: in the NEXT map-maintenance call with an in-kernel scan, workgroups
                                          b, b+1, ... give up waiting for their predecessors (one shot; -1 = off;
                                          + 65536 per such call to let pass first).  lom_frontend_set_option /
                                          lom_odometry_set_option also take b + 0x40000000: workgroup b ALONE gives up, the
                                          ones behind it get their prefix (a hole in the middle of the front end's output) */
    /* lom_odometry_set_option only: */
    LOM_OPT_TEST_FORCE_HOST_REDO = 102,        /* 1: every frame is handed back to the host stages */
    LOM_OPT_TEST_GRID_GIVE_UP_MATCHING_DS = 103, /* LOM_OPT_TEST_GRID_GIVE_UP on the matching down-sampler ... */
    LOM_OPT_TEST_GRID_GIVE_UP_UPDATE_DS = 104,   /* ... the next frame's update down-sampler ... */
    LOM_OPT_TEST_GRID_GIVE_UP_KEYFRAME = 105,    /* ... the keyframe (its next insert or cleanup) */
    /* lom_map_set_option again: */
    LOM_OPT_TEST_BULK_PARTITION_MAX = 106,       /* p > 0: a partition of the bulk insert may hold p points (at most the
                                                    1,024 its workgroup has LDS for; 0 = that limit): a bulk insert with a
                                                    larger partition writes nothing and is redone by the four-kernel path
                                                    (counted by LOM_COUNTER_GRID_REDOS) */
    LOM_OPT_TEST_BATCH_ROUND_MAX = 107,          /* r > 0: a round of lom_match_align_batch holds at most r problems (0 = as
                                                    many as are resident together): lets the tests force several rounds */
    LOM_OPT_TEST_QUALITY_ROUND_MAX = 108,        /* r > 0: a round of lom_match_quality_batch* holds at most r problems
                                                    (0 = as many as its byte budget admits) */
    LOM_OPT_TEST_VOTE_SLICE_MAX = 109            /* s in 1 .. 64: a launch of the scan votes (lom_map_carve_scans,
                                                    lom_map_scan_votes) holds at most s scans (0 = 64, one bit each of
                                                    a voxel's mask) */
} lom_option;
int lom_map_set_option(lom_map *m, int option, int64_t value);
/* diagnostics: LOM_COUNTER_GRID_REDOS = calls of this handle redone with the multi-launch scan after an
 * in-kernel scan gave up (such a call changes nothing; see csrc/grid_scan.hpp) */
enum { LOM_COUNTER_GRID_REDOS = 0,
       LOM_COUNTER_CLEANUPS_BEHIND_ALIGN = 1, /* radius cleanups that took the scan enqueued behind an align */
       LOM_COUNTER_FRAMES_SENT_AHEAD = 2,     /* lom_odometry only: frames found in pinned memory already (staged during the previous frame's align) */
       LOM_COUNTER_EMPTY_SLABS = 3            /* slabs whose voxel a radius cleanup erased in place and that are not closed yet */ };
int64_t lom_map_debug_counter(const lom_map *m, int which);

/* make the handle's stream wait for a hipEvent_t recorded elsewhere */
int lom_map_wait_event(lom_map *m, void *hip_event);
/* The device-resident align keeps the calling thread waiting for ~0.1 ms with nothing to do.  A caller with host work
 * that does not depend on the align's result (staging the next frame) hands it over here: fn(user) is called ONCE, by the
 * next lom_match_align_device on this handle, on the calling thread, after the align's kernels are enqueued and before it
 * waits for their report.  One shot; fn must not use this handle.  (An align that takes the host-driven path does not
 * call it: the caller checks whether its work was done.) */
int lom_map_set_align_idle_hook(lom_map *m, void (*fn)(void *user), void *user);
/* run the handle's work on a caller-owned hipStream_t (NULL = handle's own stream) */
int lom_map_set_stream(lom_map *m, void *hip_stream);
/* the hipStream_t the handle currently works on (to put several handles on one stream) */
void *lom_map_get_stream(lom_map *m);

/* ---- scan contexts: several callers aligning against ONE keyframe ------------------------------------- */
/* VoxelGrid::getCorrespondence / findMatchingPairs are const (src/voxel_grid.h:164,206) and CloudMatcher::align takes
 * `const VoxelGrid&` (src/cloud_matcher.h:15-16): any number of threads may align against one keyframe at a time.
 * A map handle is single-caller; a lom_scan is what each further caller owns -- stream, per-scan buffers, solve state,
 * report block -- while its kernels read the map's table and slabs.  Contexts of one map may be used concurrently
 * from different threads (one caller per context), as long as nobody changes the map meanwhile (lom_map_add_points*,
 * lom_map_radius_cleanup, lom_map_clear: the reference's non-const members); destroy them before the map.
 * One solve keeps 53 of the 256 CUs busy on a VLP16-sized scan: concurrent contexts are how one GPU is filled. */
typedef struct lom_scan lom_scan;
int lom_scan_create(lom_map *map, lom_scan **out);
/* The same, on a slice of the GPU: the context's stream runs on partition `part` of `nparts` equal, disjoint slices of
 * the device's compute units (a CU mask on the stream: the same number of CUs on every XCD; 1 <= nparts <= 8), and its
 * grids are sized for that slice.  One align alone leaves most of the GPU idle between the launches of its dependent
 * chain, and unpartitioned contexts queue behind each other's full-GPU search grids; k callers on k slices run side by
 * side (bench.py concurrent_contexts: 4 callers against 1).  Results do not depend on the slice: bit for bit those of
 * lom_scan_create / of the map handle.  A stream handed over with lom_scan_set_stream overrides the partition. */
int lom_scan_create_on_partition(lom_map *map, int part, int nparts, lom_scan **out);
void lom_scan_destroy(lom_scan *s);
const char *lom_scan_last_error(const lom_scan *s);
int lom_scan_set_option(lom_scan *s, int option, int64_t value);   /* lom_map_set_option's switches, per context */
int lom_scan_set_stream(lom_scan *s, void *hip_stream_or_null);
void *lom_scan_get_stream(lom_scan *s);
/* lom_match_align / _align_device / _align_repeat / lom_match_find_pairs on the context */
int lom_scan_align(lom_scan *s, const float *src_xyz, size_t n, size_t stride_bytes, const float guess_t[3],
                   const float guess_q_wxyz[4], float out_t[3], float out_q_wxyz[4], lom_align_stats *stats_or_null);
int lom_scan_align_device(lom_scan *s, const float *d_src_xyz, size_t n, size_t stride_bytes, const float guess_t[3],
                          const float guess_q_wxyz[4], float out_t[3], float out_q_wxyz[4], lom_align_stats *stats_or_null);
int lom_scan_align_repeat(lom_scan *s, const float *d_src_xyz, size_t n, size_t stride_bytes, const float guess_t[3],
                          const float guess_q_wxyz[4], int reps, float out_t[3], float out_q_wxyz[4],
                          lom_align_stats *total_or_null);
/* lom_match_align_batch / _batch_device on the context */
int lom_scan_align_batch(lom_scan *s, const lom_align_problem *p, int count, lom_align_result *out, int *best_or_null);
int lom_scan_align_batch_device(lom_scan *s, const lom_align_problem *p, int count, lom_align_result *out,
                                int *best_or_null);
int64_t lom_scan_find_pairs(lom_scan *s, const float *src_xyz, size_t n, size_t stride_bytes, const float t[3],
                            const float q_wxyz[4], float max_dist, lom_correspondence *out);
int64_t lom_scan_find_pairs_sq(lom_scan *s, const float *src_xyz, size_t n, size_t stride_bytes, const float t[3],
                               const float q_wxyz[4], double max_dist_sq, lom_correspondence *out);

/* ---- align quality report: information, covariance, degeneracy, fit ------------------------------------ */
/* How good is a pose?  One correspondence search at the pose, then one evaluation of the align's own residual and
 * Jacobian (csrc/k_eval.hpp point_terms) over its winners, reduced on the device in a fixed order (two calls with the
 * same inputs return the same bytes, on a map handle and on a scan context alike), and a little host math
 * (csrc/quality.cpp).
 *
 * Tangent order and units of `information` and `gradient` are the solver's own: rotation (3), then translation (3);
 * the rotation tangent is the Ceres QuaternionManifold increment, i.e. HALF the rotation vector, applied on the left
 * (world frame).  The translation prior of the align (weight 100 on each translation diagonal) is NOT included.
 * `covariance` is in nav_msgs order -- x, y, z, then rotation about the fixed X, Y, Z axes in radians:
 *     covariance = sigma2 * (S P H P^T S)^-1,   P: translation first,   S = diag(1, 1, 1, 1/2, 1/2, 1/2)
 * by Cholesky.  No pseudo-inverse and no regularisation: where the factorisation meets a pivot <= 0 or a non-finite
 * value, or valid < 7, covariance_valid = 0 and the 36 values read 0 (degenerate geometry: see eig_t / eig_r).  A caller
 * who wants the prior in adds 100 to information[21], [28] and [35] and inverts that matrix themself. */
typedef struct {
    int64_t queries;           /* source points searched                                                     */
    int64_t valid;             /* correspondences found                                                      */
    int64_t inliers;           /* valid with r^2 <= 0.15^2: the branch in which the Huber weight is 1       */
    double overlap;            /* valid / queries (0 for queries == 0)                                       */
    double cost;               /* sum 0.5 rho(r^2): the align's cost at this pose, without the prior         */
    double rmse;               /* sqrt(sum r^2 / valid), point-to-plane, metres (0 for valid == 0)           */
    double rmse_inliers;       /* the same over the inliers                                                  */
    double max_abs_residual;   /* max |r|                                                                    */
    double mean_sq_dist;       /* sum |R p + t - o|^2 / valid: squared point-to-point distance to the winner
                                  (the analogue of PCL's fitness score)                                      */
    double sigma2;             /* sum w r^2 / max(1, valid - 6)                                              */
    double sum_w;              /* sum of the Huber weights                                                   */
    double information[36];    /* H = sum w J J^T, full symmetric, row-major                                 */
    double gradient[6];        /* g = sum w J r                                                              */
    double eig_t[3];           /* eigenvalues, ascending, of H_tt / sum_w: with unit normals the weighted mean of
                                  n n^T, trace 1 -- each the share of the constraint on that direction       */
    double eigvec_t[9];        /* row k: the unit eigenvector of eig_t[k]                                    */
    double eig_r[3];           /* the same of H_rr / (4 sum_w) (4: half-angles to radians); m^2 of lever arm  */
    double eigvec_r[9];
    double covariance[36];     /* see above; row-major                                                       */
    int32_t degenerate_t;      /* eig_t below min_eig_t (threshold <= 0: not counted, 0)                     */
    int32_t degenerate_r;      /* eig_r below min_eig_r                                                      */
    int32_t covariance_valid;
    int32_t pad;
} lom_quality_report;

/* The reduced values of one evaluation, as the device leaves them: [0..27] the align's sums (LOM_NSUMS above: H upper
 * triangle, g, cost); [28] sum w; [29] sum w r^2; [30] sum r^2 over valid; [31] sum r^2 over inliers;
 * [32] sum |R p + t - o|^2; [33] valid; [34] inliers; [35] max |r|. */
#define LOM_NQSUMS 36
/* The host math alone (no device needed): fills *out from the reduced values, the number of queries and the two
 * thresholds.  The thresholds are the caller's: the smallest share (eig_t) / lever arm in m^2 (eig_r) a direction must
 * have to count as constrained.  Non-finite sums give covariance_valid = 0 and, for a non-finite block, NaN
 * eigenvalues and no degeneracy count.  LOM_ERR_ARG for a NULL pointer or a negative count. */
int lom_quality_from_sums(const double sums[LOM_NQSUMS], int64_t queries, float min_eig_t, float min_eig_r,
                          lom_quality_report *out);
/* One search at the f32 pose exactly as given (the quaternion is not re-normalised; max_dist squared in f32, as
 * lom_match_find_pairs does), then the evaluation at that pose widened to f64; the host waits once.  n == 0 and zero
 * correspondences are valid (all-zero report; valid = 0, covariance_valid = 0).  residual_out_or_null: n floats, the
 * signed residual r of every source point, quiet NaN where it has no correspondence.
 * Isolation as lom_match_align_batch: buffers of its own; the single align's state, an armed
 * lom_map_radius_cleanup_after_align and an armed idle hook are neither used nor consumed. */
int lom_match_quality(lom_map *m, const float *src_xyz, size_t n, size_t stride_bytes, const float t[3],
                      const float q_wxyz[4], float max_dist, float min_eig_t, float min_eig_r, lom_quality_report *out,
                      float *residual_out_or_null);
/* same, source cloud and the optional residual array in device memory */
int lom_match_quality_device(lom_map *m, const float *d_src_xyz, size_t n, size_t stride_bytes, const float t[3],
                             const float q_wxyz[4], float max_dist, float min_eig_t, float min_eig_r,
                             lom_quality_report *out, float *d_residual_out_or_null);
int lom_scan_quality(lom_scan *s, const float *src_xyz, size_t n, size_t stride_bytes, const float t[3],
                     const float q_wxyz[4], float max_dist, float min_eig_t, float min_eig_r, lom_quality_report *out,
                     float *residual_out_or_null);
int lom_scan_quality_device(lom_scan *s, const float *d_src_xyz, size_t n, size_t stride_bytes, const float t[3],
                            const float q_wxyz[4], float max_dist, float min_eig_t, float min_eig_r,
                            lom_quality_report *out, float *d_residual_out_or_null);

/* ---- batched quality report: K (scan, pose) candidates against one keyframe in one call ------------------- */
/* Scoring many candidate poses -- a lattice around a relocalisation or loop-closure guess, before the few best go to
 * lom_match_align_batch -- in one call: one host wait whatever K is, device memory bounded whatever K is.
 * Same definition as the single report: problem i gets one search at its f32 pose as given (not re-normalised; max_dist
 *   squared in f32), then the evaluation at that pose widened to f64, over the LOM_NQSUMS values in their order.
 * Clouds: problems may share a cloud (equal pointer, n and stride: the pose-lattice case is one cloud and K poses; the
 *   host entries upload such a cloud once) and may differ in n, 0 and 1 included.  Every s-th point of a cloud is
 *   stride_bytes * s and n / s.
 * Rounds: the call runs as many rounds as a byte budget for a round's records and partial sums asks for (csrc/match_plan.hpp
 *   kQualBatchBudgetBytes); all rounds are enqueued before the host waits, once.  LOM_OPT_TEST_QUALITY_ROUND_MAX caps a
 *   round's problems for the tests.
 * Determinism: the bytes of problem i's sums depend only on (map, cloud, n, stride, pose, max_dist, counted or not) --
 *   not on K, on its place in the batch, on the round size, on what else is in the batch, on map handle versus scan
 *   context (partitioned or not), or on the call.  Against lom_match_quality the counts are equal and every other sum
 *   agrees to 1e-12 of its scale; byte equality with the single call is not promised.
 * Arguments: LOM_ERR_ARG before any work for a NULL handle, count < 0, NULL p or output with count > 0, a problem with
 *   n > 0 and NULL xyz, a stride that does not hold three aligned floats or n >= 2^31 - 1; count == 0 is valid (best = -1,
 *   nothing is launched); *best_or_null is left alone on an error.  n == 0 or zero correspondences give all-zero sums
 *   and an all-zero report, as the single call does.
 * Isolation as lom_match_align_batch and the single report: buffers of its own; the single align's state, the single
 *   report's buffers, an armed lom_map_radius_cleanup_after_align and an armed idle hook are neither used nor consumed.
 *   LOM_OPT_HOST_LM and an attached exchange do not matter here. */
typedef struct {
    const float *xyz;          /* host (.._batch) or device (.._batch_device) pointer */
    size_t n, stride_bytes;
    float t[3], q_wxyz[4];     /* taken as given, not re-normalised, as lom_match_quality */
} lom_quality_problem;
/* the reduced values only: sums_out[i * LOM_NQSUMS + k] for p[i] */
int lom_match_quality_batch_sums(lom_map *m, const lom_quality_problem *p, int count, float max_dist, double *sums_out);
int lom_match_quality_batch_sums_device(lom_map *m, const lom_quality_problem *p, int count, float max_dist,
                                        double *sums_out);
/* full reports: out[i] = lom_quality_from_sums of p[i]'s values; best_or_null: lom_quality_batch_best(out, count) */
int lom_match_quality_batch(lom_map *m, const lom_quality_problem *p, int count, float max_dist, float min_eig_t,
                            float min_eig_r, lom_quality_report *out, int *best_or_null);
int lom_match_quality_batch_device(lom_map *m, const lom_quality_problem *p, int count, float max_dist, float min_eig_t,
                                   float min_eig_r, lom_quality_report *out, int *best_or_null);
int lom_scan_quality_batch_sums(lom_scan *s, const lom_quality_problem *p, int count, float max_dist, double *sums_out);
int lom_scan_quality_batch_sums_device(lom_scan *s, const lom_quality_problem *p, int count, float max_dist,
                                       double *sums_out);
int lom_scan_quality_batch(lom_scan *s, const lom_quality_problem *p, int count, float max_dist, float min_eig_t,
                           float min_eig_r, lom_quality_report *out, int *best_or_null);
int lom_scan_quality_batch_device(lom_scan *s, const lom_quality_problem *p, int count, float max_dist, float min_eig_t,
                                  float min_eig_r, lom_quality_report *out, int *best_or_null);
/* the best report (host code, no GPU): the most valid; ties go to the lower cost, then to the lower index; a report
 * with queries == 0 ranks below any other; -1 if count <= 0 or r == NULL */
int lom_quality_batch_best(const lom_quality_report *r, int count);
/* The poses of a lattice around `centre` (host code, no GPU).  Along axis a: 2 * floor(half_extent[a] / step[a]) + 1
 * nodes (a step <= 0 or an extent < step: one node, the centre); translation offsets in the world frame, added in f64 and
 * rounded once to f32.  Yaw node j: q = yaw_z(j * step_yaw) * centre.q -- a left product about world Z, in f64,
 * normalised, then rounded to f32.  Order: yaw outermost, then x, y, and z innermost, each ascending from the negative
 * end.  Returns the number of nodes; with out == NULL or cap too small nothing is written and the number is still
 * returned.  LOM_ERR_ARG for a NULL centre, a non-finite input, an all-zero quaternion or more than 2^31 - 1 nodes. */
int lom_pose_lattice(const lom_pose *centre, const float half_extent_xyz[3], const float step_xyz[3],
                     float half_extent_yaw_rad, float step_yaw_rad, lom_pose *out, int cap);

/* ---- multi-GPU: source points range-sharded, map replicated ------------- */
/* One all-gather of LOM_NSUMS f64 per residual evaluation over RCCL, summed in
 * rank order on every rank (results independent of the collective's tree). */
#define LOM_COMM_ID_BYTES 128
int lom_comm_unique_id(char id_out[LOM_COMM_ID_BYTES]);   /* rank 0: ncclGetUniqueId */
int lom_comm_init(lom_map *m, int rank, int nranks, const char id[LOM_COMM_ID_BYTES]);
int lom_comm_finalize(lom_map *m);
/* Same contract between the ranks of ONE node without a device-side collective: each rank's host
 * receives its own sums from the resident evaluation server, the hosts exchange the 256 bytes
 * through POSIX shared memory and add them in rank order.  lom_comm_host_id() on rank 0, broadcast
 * the id, lom_host_comm_create() on every rank, lom_comm_attach_host() on the map.  The exchange
 * object is plain host code (usable without a GPU, e.g. as the allreduce hook of
 * lom_align_with_hooks); the caller owns it. */
typedef struct lom_host_comm lom_host_comm;
int lom_comm_host_id(char id_out[LOM_COMM_ID_BYTES]);
int lom_host_comm_create(int rank, int nranks, const char id[LOM_COMM_ID_BYTES], lom_host_comm **out);
/* in place, count <= LOM_NSUMS.  LOM_ERR_COMM: a rank did not arrive within the deadline (lom_host_comm_set_timeout) or had
 * abandoned an exchange; the object stays broken on every rank from then on.  On the exchange a rank gives up on, a peer
 * that had just completed it may still return LOM_OK -- it fails at its next exchange, at once (csrc/comm.cpp exchange()). */
int lom_host_comm_allreduce(lom_host_comm *c, double *buf, int count);
/* Deadline of one exchange (default 60 s).  A rank that reaches it ABANDONS the exchange object: it marks its
 * slots, so that every rank still waiting for it -- or arriving later -- fails with LOM_ERR_COMM as well instead
 * of pairing with slots their owner has walked away from; all later calls on the object fail at once.
 * lom_host_comm_abort does the same on purpose (a rank that cannot continue tells its peers).
 * lom_host_comm_last_error says which exchange was abandoned, and by whom. */
int lom_host_comm_set_timeout(lom_host_comm *c, double seconds);
int lom_host_comm_abort(lom_host_comm *c);
const char *lom_host_comm_last_error(const lom_host_comm *c);
/* every rank contributes `bytes` (<= 256) raw bytes; all_out receives nranks * bytes in rank order */
int lom_host_comm_allgather(lom_host_comm *c, const void *mine, size_t bytes, void *all_out);
void lom_host_comm_destroy(lom_host_comm *c);
int lom_comm_attach_host(lom_map *m, lom_host_comm *c_or_null);
/* Third transport (ranks of one node, <= 8): the device-resident solve of the single-GPU path on
 * every rank, with the ranks' reduced sums exchanged by the GPUs themselves -- every rank's k_lm
 * stores its 32 words into a small buffer in each peer's HBM (IPC-mapped, over xGMI) and adds the
 * ranks' words in rank order: no host round trip per evaluation.  `c` carries rank / nranks and the
 * exchange of the IPC handles.  The call runs a self-test of the device-to-device exchange on all
 * ranks and returns LOM_ERR_COMM on EVERY rank if it fails on any (fall back to
 * lom_comm_attach_host).  Ranks must issue the same sequence of aligns.
 * Failure handling: a rank whose kernel gives up waiting (LOM_OPT_DEVICE_PATIENCE_TICKS) tells its peers through
 * an abort word in their exchange buffers, so they leave their waits at once instead of after their own patience;
 * after EVERY align the ranks agree on its outcome through `c` (deadline: 30 s + 12 x the patience for a peer
 * rank): all ranks keep the device result, or all redo the align through the host exchange (equal poses), or --
 * when a rank failed for good, or the agreement itself timed out -- all return an error. */
int lom_comm_attach_p2p(lom_map *m, lom_host_comm *c);

/* ---- host-side align driver over user evaluators ------------------------ */
/* lom_match_align* = this driver over the HIP kernels.  Exposed so that the
 * driver (outer loop, LM policy, reduction order) can be exercised with other
 * evaluators and collectives, e.g. world_size-2 gloo tests on CPU. */
typedef struct {
    void *user;
    /* new correspondences at the f32 pose, then sums at (q,t) (f64, = widened pose) */
    int (*match_eval)(void *user, const float pose_t[3], const float pose_q[4], const double q[4],
                      const double t[3], double out[LOM_NSUMS]);
    /* sums at (q,t) for the correspondences of the last match_eval */
    int (*eval_fixed)(void *user, const double q[4], const double t[3], double out[LOM_NSUMS]);
    /* optional: in-place sum over ranks of buf[count]; NULL = single rank */
    int (*allreduce)(void *user, double *buf, int count);
} lom_align_hooks;

int lom_align_with_hooks(const lom_align_hooks *hooks, const float guess_t[3],
                         const float guess_q_wxyz[4], float out_t[3], float out_q_wxyz[4],
                         lom_align_stats *stats_or_null);

/* ---- callers of the path, ROS-free; host code over the ABI above -- */
/* lidar_point::PointXYZIRT (src/lidar_point_type.h:13-21): 32 bytes, same field offsets */
typedef struct {
    float x, y, z, pad0;
    float intensity;
    uint16_t ring;
    uint16_t pad1;
    float time;
    float pad2;
} lom_point_xyzirt;

/* utils::pointTimeNormalize, src/utils/point_time_normalize.h:15-39 */
void lom_point_time_normalize(const lom_point_xyzirt *in, size_t n, lom_point_xyzirt *out);
/* CloudTransformer::transformNonRigid (deskew), src/utils/cloud_transform.h:15-40 */
void lom_transform_non_rigid(const lom_point_xyzirt *in, size_t n, const lom_pose *start_pose,
                             const lom_pose *end_pose, lom_point_xyzirt *out);
/* utils::rangeFilter, src/utils/range_filter.h:13-28; packed xyz (+ optional normals); returns kept count */
size_t lom_range_filter(const float *xyz, const float *nrm, size_t n, float min_range, float max_range,
                        float *xyz_out, float *nrm_out);
/* CloudClassifier::classify, src/utils/cloud_classifier.h:19-168: planar points with normals
 * (outputs sized for n points); the unclassified cloud's size and the organised grid {height,
 * width} are optional outputs.  Returns the number of planar points. */
size_t lom_cloud_classify(const lom_point_xyzirt *in, size_t n, float *xyz_out, float *nrm_out,
                          size_t *unclassified_out, size_t grid_out[2]);

/* ---- the same four callers on the device: a frame stays in HBM from its upload to its pose ------------- */
/* Per-frame front end = pointTimeNormalize + transformNonRigid + CloudClassifier::classify + rangeFilter
 * (the references above) as four HIP kernels; results bit-equal to the host functions above.  Sizes the
 * host does not know (planar / filtered point counts, organised-cloud shape) stay on the device as words
 * the consumers read (lom_voxel_downsample_device_nowait takes such a count).  A frame the device cannot
 * decide bit-exactly (an azimuth within 2e-14 rad of a bin boundary, where the device's atan2 could pick
 * another cell than the host's; an organised cloud beyond the device buffers) is reported by
 * lom_frontend_wait() == 1 and is redone by the caller with the host functions. */
typedef struct lom_frontend lom_frontend;
int lom_frontend_create(int device, void *hip_stream_or_null, lom_frontend **out);
void lom_frontend_destroy(lom_frontend *f);
const char *lom_frontend_last_error(const lom_frontend *f);
int lom_frontend_set_option(lom_frontend *f, int option, int64_t value); /* LOM_OPT_TEST_GRID_GIVE_UP: the next frame's scan */
/* enqueue one frame: upload, time normalisation, deskew from start_pose to end_pose, classification, range filter */
int lom_frontend_process(lom_frontend *f, const lom_point_xyzirt *pts, size_t n, const lom_pose *start_pose,
                         const lom_pose *end_pose, float min_range, float max_range);
/* device pointers of the last frame's filtered planar cloud (packed xyz, normals), the host's upper bound of
 * its size, and the device words {planar points, filtered points, grid height, grid width, ...} */
int lom_frontend_results(lom_frontend *f, const float **d_xyz, const float **d_nrm, const uint32_t **d_counts,
                         uint32_t *bound);
/* device pointer and size of the last frame's deskewed cloud (what lom_frontend_fetch(what = 0) copies out), valid behind
 * lom_frontend_done_event until the next frame is enqueued */
int lom_frontend_deskewed(lom_frontend *f, const lom_point_xyzirt **d_out, uint32_t *n_out);
/* wait for the frame: 0 = done on the device, 1 = redo this frame on the host, < 0 = lom_status;
 * counts_out = {planar, filtered, height, width} */
int lom_frontend_wait(lom_frontend *f, uint32_t counts_out[4]);
/* host copies: what = 0 the deskewed cloud (lom_point_xyzirt records into out_a), what = 1 the filtered planar
 * cloud (packed xyz into out_a, normals into out_b); returns the number of points available */
int64_t lom_frontend_fetch(lom_frontend *f, int what, void *out_a, void *out_b, size_t cap);
/* pinned staging buffer for a frame of n points: a caller that writes the frame there itself (e.g. straight from
 * its message) passes the same pointer to lom_frontend_process and saves the copy */
int lom_frontend_stage(lom_frontend *f, size_t n, lom_point_xyzirt **out);
/* hipEvent_t recorded behind the last frame's kernels; lom_map_wait_event makes a handle's stream wait for it
 * (the front end runs on a stream of its own, beside the previous frame's keyframe update) */
void *lom_frontend_done_event(lom_frontend *f);
void *lom_frontend_stream(lom_frontend *f);
/* sequence number of the last lom_frontend_process (words [4] / [5] of lom_frontend_results' d_counts hold the
 * number of the last frame that has to be redone on the host / that hit a grid time-out) */
uint32_t lom_frontend_sequence(const lom_frontend *f);
/* test hook: the device's restatement of glibc's sinf (used by the per-point slerp) on n host values */
int lom_debug_sinf(lom_frontend *f, const float *x, size_t n, float *out);

/* ---- classifier for frames without rings (solid-state and non-repetitive scanners, PCD files, merged or down-sampled
 * clouds, any message for which lom_pointcloud2_unpack sets the `ring` bit of missing_mask) ------------------------
 * Planar / not planar and a normal per point from the point's neighbourhood in the frame itself; `ring` is not read.
 *  1. index: a voxel map with voxel size `radius` that keeps the first `index_cap` points of a voxel, built from the
 *     frame in input order (a workspace of the front end, reused frame after frame);
 *  2. neighbours of point i: the STORED points of the 27 voxels around i's voxel with d^2 <= radius^2 (d^2 in f64
 *     from the f32 coordinates); a point whose voxel was full is not stored, hence not its own neighbour; m = their number;
 *  3. population covariance of d = p_j - p_i over the neighbours (f64), eigenvalues l0 <= l1 <= l2;
 *  4. planar iff m >= min_neighbours, l0 + l1 + l2 > 0, l0 / (l0 + l1 + l2) <= max_variation and
 *     l1 / l2 >= min_spread (which rejects a line);
 *  5. normal = the unit eigenvector of l0, flipped so that n . p_i <= 0 (towards the sensor origin), rounded to f32;
 *  6. output: the planar points in INPUT order, packed xyz + normals, their count in a device word; the range filter
 *     follows.  A non-finite or out-of-range point fails the frame with LOM_ERR_RANGE, as it fails the down-samplers.
 * There are no defaults: the project has no measured basis for any.  radius > 0, 1 <= index_cap <= 64,
 * min_neighbours >= 3, 0 < max_variation <= 1/3, 0 <= min_spread < 1; anything else is LOM_ERR_ARG. */
typedef struct {
    float radius;
    uint32_t index_cap, min_neighbours;
    float max_variation, min_spread;
} lom_neighbourhood_params;
typedef struct { /* per INPUT point */
    uint32_t neighbours;
    int32_t planar;
    double eig[3]; /* ascending; zero where there is no neighbour */
} lom_neighbourhood_detail;
enum { LOM_CLASSIFIER_RINGS = 0, LOM_CLASSIFIER_NEIGHBOURHOOD = 1 };
/* The stage alone, host in / host out, on the front end's stream and workspace (it overwrites the deskewed cloud the
 * last frame left in HBM).  Returns the number of planar points (no range filter); xyz_out / nrm_out: room for n
 * points; detail_out_or_null: n records. */
int64_t lom_classify_neighbourhood(lom_frontend *f, const lom_point_xyzirt *pts, size_t n, const lom_neighbourhood_params *p,
                                   float *xyz_out, float *nrm_out, lom_neighbourhood_detail *detail_out_or_null);
/* The classifier of the following lom_frontend_process calls.  With LOM_CLASSIFIER_NEIGHBOURHOOD (p required) a frame
 * runs upload, time normalisation and deskew as they are, then the stage above, then the range filter;
 * lom_frontend_wait never returns 1 for such a frame (there is no host version: a scan that gave up is redone on the
 * device by kernels that wait for nobody) and counts_out = {planar, filtered, 0, 0}.  LOM_CLASSIFIER_RINGS (p ignored)
 * is the default, and going back to it restores it bit for bit. */
int lom_frontend_set_classifier(lom_frontend *f, int kind, const lom_neighbourhood_params *p_or_null);
/* LOM_COUNTER_GRID_REDOS: neighbourhood stages of this front end redone after an in-kernel scan gave up */
int64_t lom_frontend_debug_counter(const lom_frontend *f, int which);

/* ---- file input: pcl::io::loadPCDFile<pcl::PointXYZ> (test/test.cpp:194) ---------------------------- */
/* PCD v0.7 reader, host code without PCL: `DATA ascii` and `DATA binary`, fields located by name (x y z,
 * optionally normal_x normal_y normal_z), any SIZE / TYPE / COUNT layout -- e.g. the reference's shipped
 * test/test_data/intersection00056.pcd (FIELDS rgb _ x y z _, 32-byte records).  NaN points are kept,
 * like loadPCDFile does.  Returns the number of points in the file (negative: lom_status, text via
 * lom_pcd_last_error()); writes at most `cap` packed xyz triples (and normals, zero when the file has
 * none, if nrm_out != NULL). */
typedef struct {
    uint64_t points;
    uint32_t width, height;
    uint32_t point_step; /* bytes per record in the file */
    int32_t has_normals;
    int32_t data_kind;   /* 0 ascii, 1 binary */
} lom_pcd_info;
int64_t lom_pcd_read(const char *path, float *xyz_out, float *nrm_out, size_t cap, lom_pcd_info *info_or_null);
const char *lom_pcd_last_error(void);

/* ---- message payloads: pcl::fromROSMsg / pcl::toROSMsg of the node (src/lidar_odometry_node.cpp:47-48,61,71) ---- */
/* sensor_msgs/msg/PointField datatypes */
enum {
    LOM_PF_INT8 = 1, LOM_PF_UINT8 = 2, LOM_PF_INT16 = 3, LOM_PF_UINT16 = 4,
    LOM_PF_INT32 = 5, LOM_PF_UINT32 = 6, LOM_PF_FLOAT32 = 7, LOM_PF_FLOAT64 = 8
};
typedef struct {
    const char *name;
    uint32_t offset;
    uint8_t datatype;
    uint32_t count;
} lom_pc2_field;
/* the members of a sensor_msgs/msg/PointCloud2 the conversion reads; nothing is copied or kept */
typedef struct {
    uint32_t height, width;
    const lom_pc2_field *fields;
    uint32_t n_fields;
    uint8_t is_bigendian;
    uint32_t point_step, row_step;
    const uint8_t *data;
    size_t data_bytes;
} lom_pc2_view;
/* fromROSMsg into PointCloud<lidar_point::PointXYZIRT>: x y z intensity (FLOAT32), ring (UINT16), time (FLOAT32)
 * located by name, datatype and count as PCL's FieldMatches does; a field without a match stays zero and sets
 * bit k of *missing_mask (k in the order above).  Returns width * height (writes at most cap records; out may be
 * NULL with cap 0), negative = lom_status with lom_pointcloud2_last_error().  `out` may be the pinned buffer of
 * lom_frontend_stage(). */
int64_t lom_pointcloud2_unpack(const lom_pc2_view *msg, lom_point_xyzirt *out, size_t cap, uint32_t *missing_mask_or_null);
/* toROSMsg: field table and point_step of an outgoing cloud (height 1, width n, row_step n * point_step, little
 * endian); LOM_PC2_XYZ for the keyframe clouds, LOM_PC2_XYZIRT for the deskewed cloud, whose records are
 * lom_point_xyzirt as they are.  Returns the number of fields. */
enum { LOM_PC2_XYZ = 0, LOM_PC2_XYZIRT = 1 };
int lom_pointcloud2_layout(int kind, lom_pc2_field fields_out[6], uint32_t *point_step_out);
/* payload of a PointCloud<pcl::PointXYZ> message from xyz triples (stride 0 = packed): 16-byte records
 * {x, y, z, 1.0f}.  Returns the bytes needed / written. */
int64_t lom_pointcloud2_pack_xyz(const float *xyz, size_t n, size_t stride_bytes, uint8_t *data_out, size_t cap_bytes);
const char *lom_pointcloud2_last_error(void);

/* ---- normal estimation helper: pcl::NormalEstimation, setRadiusSearch(r), viewpoint (0,0,0) (test/test.cpp:196-205) */
/* For every point: covariance of all points within `radius` (itself included), eigenvector of the smallest
 * eigenvalue, flipped towards the origin; NaN where fewer than 3 neighbours exist (test.cpp:219-221 drops those
 * points).  The one plane / covariance accumulation in the reference's data flow; outside the align path, which
 * uses the normals it is given.  Host input and output (packed 12-byte normals; optionally the neighbour counts);
 * returns the number of points with a normal. */
int64_t lom_estimate_normals(const float *xyz, size_t n, size_t stride_bytes, float radius, int device, float *nrm_out,
                             uint32_t *neighbours_out_or_null);

/* ---- place recognition: scan descriptors and a device-resident database of them (not in the reference) ------------
 * Which earlier place a scan belongs to, and how it is turned against that place: the stage before lom_pose_lattice /
 * lom_match_quality_batch / lom_match_align.  A descriptor in the style of Scan Context (Kim and Kim,
 * IROS 2018: a polar height image); a database of them in HBM; one call returns, for each of Q query descriptors, the k
 * nearest entries with their column shift, searched exactly over all entries and all shifts.
 *
 * Definitions (R = rings, S = sectors):
 *  - Cell of a point (x, y, z), f32.  In f64 from the f32 values: rho = sqrt(x^2 + y^2), ring = floor(rho / (max_range / R));
 *    phi = atan2(y, x), moved into [0, 2 pi) (a phi that the addition of 2 pi rounds to 2 pi itself counts as 0),
 *    sector = floor(phi / (2 pi / S)).  A point with ring >= R is ignored.  v = z - z_floor as one f32 subtraction; a point
 *    with v <= 0 is ignored.
 *  - Descriptor: an R x S array of f32, ring-major.  A cell holds the maximum v of its points, or 0 if it has none.  Every
 *    stored value is >= 0, so its bit pattern orders like an unsigned integer.  The maximum does not depend on point order,
 *    so the descriptor is a pure function of the point set.
 *  - Bad and empty clouds: a non-finite coordinate fails the call with LOM_ERR_RANGE and nothing is stored; a cloud with
 *    n = 0 gives the all-zero descriptor.
 *  - Distance of query q to entry c at shift s: V = the columns j where both q's column j and c's column (j + s) mod S are
 *    non-zero; d(s) = 1 - (1/|V|) sum_{j in V} cos(q_j, c_{(j+s) mod S}); where V is empty, d(s) = 1.  (The device works in
 *    f32 on unit columns and reports max(d, 0).)  The pair's distance is the minimum over s; on equal distance bits the
 *    smallest s wins.
 *  - Result per query: the k entries of the searched id range with the smallest (distance, id); equal distance bits go to
 *    the smaller id.  Slots beyond the number of entries searched hold id -1, distance +inf, shift 0.
 *  - Shift to yaw: lom_place_shift_yaw(params, shift) = psi = ((S - shift) mod S) * 2 pi / S, the rotation about z that
 *    takes the ENTRY's cloud onto the QUERY's cloud, to half a sector.  So the query sensor's rotation in the entry's
 *    frame is Rz(-psi): a pose search for the query scan against the entry's keyframe starts at (0, 0, 0, Rz(-psi)).
 *  - Invariance: the bits of a pair's (distance, shift) depend on the two descriptors only -- not on the number of
 *    entries or queries, the id range, or the entry's position.
 * There are no defaults.  1 <= rings <= 64, 1 <= sectors <= 64, max_range > 0 and finite, z_floor finite; anything else
 * is LOM_ERR_ARG.  The database owns its stream; calls on one database are serialised by a lock inside it.  The _device
 * forms read a cloud in HBM and wait on nothing but the database's own stream: the caller orders its producer
 * (lom_place_db_wait_event, or a host wait), as with lom_map_add_points_device.  A NULL handle, a bad k, bad ids or a
 * non-finite / negative descriptor value are refused with LOM_ERR_ARG before any device work. */
typedef struct {
    uint32_t rings, sectors;
    float max_range, z_floor;
} lom_place_params;
typedef struct {
    int64_t id;
    float distance;
    uint32_t shift;
} lom_place_match;
typedef struct lom_place_db lom_place_db;
/* capacity_hint: entries to make room for at once; the database grows geometrically past it (ids and bytes stay) */
int lom_place_db_create(const lom_place_params *params, int device, size_t capacity_hint, lom_place_db **out);
void lom_place_db_destroy(lom_place_db *db);
const char *lom_place_db_last_error(const lom_place_db *db); /* db == NULL: why the last create on this thread failed */
int64_t lom_place_db_size(const lom_place_db *db);
int lom_place_db_clear(lom_place_db *db); /* ids start again at 0 */
int lom_place_db_params(const lom_place_db *db, lom_place_params *out);
void *lom_place_db_stream(lom_place_db *db); /* hipStream_t */
int lom_place_db_device(const lom_place_db *db);
/* the database's stream waits for a hipEvent_t (e.g. lom_frontend_done_event) before what is enqueued next */
int lom_place_db_wait_event(lom_place_db *db, void *hip_event);
/* the raw R * S descriptor of a cloud; the database is a workspace here and is not changed */
int lom_place_describe(lom_place_db *db, const float *xyz, size_t n, size_t stride_bytes, float *desc_out);
int lom_place_describe_device(lom_place_db *db, const float *d_xyz, size_t n, size_t stride_bytes, float *desc_out);
/* new entries; the return value is the id (0, 1, 2 ... in order of arrival) or a negative lom_status.  A raw descriptor
 * takes the same kernel to its stored form as a cloud's does; with the _cloud forms the descriptor never leaves HBM. */
int64_t lom_place_db_add(lom_place_db *db, const float *desc);
int64_t lom_place_db_add_cloud(lom_place_db *db, const float *xyz, size_t n, size_t stride_bytes);
int64_t lom_place_db_add_cloud_device(lom_place_db *db, const float *d_xyz, size_t n, size_t stride_bytes);
int lom_place_db_get(lom_place_db *db, int64_t id, float *desc_out); /* the raw descriptor of an entry */
/* q >= 1 descriptors (q * R * S values) against the entries [id_begin, id_end), 0 <= id_begin <= id_end <= size (a
 * loop-closure caller leaves out the most recent entries this way; an empty range gives k empty slots); 1 <= k <= 64;
 * out: q * k matches, the nearest first; all_dist_or_null: q * (id_end - id_begin) distances (minimum over the shifts) */
int lom_place_db_query(lom_place_db *db, const float *desc, int q, int64_t id_begin, int64_t id_end, int k,
                       lom_place_match *out, float *all_dist_or_null);
/* one query straight from a cloud in HBM: describe + query with the descriptor staying on the device */
int lom_place_db_query_cloud_device(lom_place_db *db, const float *d_xyz, size_t n, size_t stride_bytes, int64_t id_begin,
                                    int64_t id_end, int k, lom_place_match *out);
double lom_place_shift_yaw(const lom_place_params *params, uint32_t shift); /* NaN for invalid params */

/* ---- pose graph: keyframe poses optimised on the device after a loop closure (not in the reference) ---------------
 * The stage behind lom_place_db_query / lom_pose_lattice / lom_match_quality_batch / lom_match_align / the quality
 * report: relative poses between keyframes, each with its information, go in as edges; the optimised
 * keyframe poses come out.  The graph lives in HBM and its optimiser runs there.  Everything is f64: f32 cannot hold a
 * kilometre-long trajectory to a millimetre.  There are no defaults.
 *
 *  - Node.  Node k has pose X_k = (R_k, t_k), stored as lom_graph_pose {t[3], q_wxyz[4]}; the quaternion is normalised
 *    on entry.  A `fixed` flag is given when the node is added.  Ids are 0, 1, 2, ... in order of arrival.
 *  - Edge.  (i, j, Z = (R_z, t_z), Omega, delta) with i != j.  Z is the measured pose of j in i's frame: for the align of
 *    j's scan against i's keyframe, the align's result itself.  Omega is symmetric 6x6, row-major (its upper triangle is
 *    read); tangent order is rotation (3, radians), then translation (3).  Omega is refused with LOM_ERR_ARG if its
 *    Cholesky factorisation fails or a value is non-finite.  delta >= 0 is the Huber width on the Mahalanobis norm; 0
 *    means no robust loss.
 *  - Error of an edge.  e = [ Log(R_i^T R_j R_z^T) ; R_i^T (t_j - t_i) - t_z ], Log the rotation vector in (-pi, pi].
 *    This is the left-perturbation error of the measurement; the quality report defines H the same way, so
 *    lom_graph_information_from_quality is a scaling and nothing else.
 *  - Cost.  Per edge s = e^T Omega e; rho(s) = s for delta == 0 or s <= delta^2, else 2 delta sqrt(s) - delta^2; weight
 *    w = 1 resp. delta / sqrt(s); cost = sum 0.5 rho(s).  Linearisation: H = sum w A^T Omega A, g = sum w A^T Omega e
 *    (IRLS, no second-order correction).
 *  - Retraction.  R_k <- R_k Exp(a_k), t_k <- t_k + b_k; node tangent (a_k, b_k).  The quaternion is re-normalised
 *    after each accepted step.
 *  - Jacobians (exact).  With e_r the rotation part of e and t_ij = R_i^T (t_j - t_i):
 *        de/d(a_i, b_i) = [ -Jl^-1(e_r), 0 ; [t_ij]x, -R_i^T ]
 *        de/d(a_j, b_j) = [ Jl^-1(-e_r) R_z, 0 ; 0, R_i^T ]
 *        Jl^-1(p) = I - 0.5 [p]x + c [p]x^2,  c = 1/th^2 - (1 + cos th) / (2 th sin th),  th = |p|;
 *    below th = 1e-8 the series I - 0.5 [p]x + [p]x^2 / 12.
 *  - Outer loop: Levenberg-Marquardt; the host decides, with one host wait per outer iteration.  Solve
 *    (H_ff + lambda D) d = -g_f over the free nodes, D = diag(H_ff); x_new = x (+) d;
 *    rho_gain = (cost - cost_new) / (0.5 d^T (lambda D d - g_f)).  rho_gain > 0: accept,
 *    lambda *= max(1/3, 1 - (2 rho_gain - 1)^3), nu = 2 (lom_graph_lm_policy); otherwise lambda *= nu, nu *= 2.  Stop
 *    when the poses in hand have max|g_f| <= gtol (LOM_GRAPH_STOP_GRADIENT: at the start, or after an accepted step),
 *    or a step has max|d| <= xtol (LOM_GRAPH_STOP_STEP; the step is kept if it was accepted), or after max_outer
 *    iterations (LOM_GRAPH_STOP_MAX_OUTER).  Non-finite or non-positive parameters are refused.
 *  - Linear solve: preconditioned conjugate gradients on the device, from d = 0.  The preconditioner is block-Jacobi:
 *    the inverse of each free node's 6x6 diagonal block of H_ff + lambda D, by Cholesky in one lane.  Stop at
 *    r^T z <= pcg_rtol^2 * r0^T z0, or after max_pcg iterations.  A solve that hits max_pcg is not an error: the LM gain
 *    test judges the step, and stats.pcg_capped counts such solves.
 *  - Gauge: checked on the host before any device work, by union-find over the edges.  Every connected component must
 *    contain a fixed node; otherwise lom_graph_optimize returns LOM_ERR_ARG and names a free node of the offending
 *    component in lom_graph_last_error.  Nothing is regularised silently.
 *  - Determinism: a result is a pure function of the nodes, the edges and their order; two runs return the same bytes.
 *    Every sum over a node's incident edges runs in ascending edge id (a node's k-th incident edge goes to lane k mod 16
 *    of a 16-lane row; the lanes' sums are added in lane order); every dot product is a fixed tree; there are no
 *    floating-point atomics anywhere.
 *  - Result: poses are read back as f64; lom_graph_stats.
 * The handle owns its stream; calls on one graph are serialised by a lock inside it.  All ids, counts and values are
 * validated before any device work; a refused call leaves the graph as it was.  The graph grows geometrically past the
 * hints given at create. */
typedef struct {
    double t[3];
    double q_wxyz[4];
} lom_graph_pose;
typedef struct {
    double lambda0, gtol, xtol, pcg_rtol;
    int32_t max_outer, max_pcg;
} lom_graph_params;
enum { LOM_GRAPH_STOP_GRADIENT = 1, LOM_GRAPH_STOP_STEP = 2, LOM_GRAPH_STOP_MAX_OUTER = 3 };
typedef struct {
    int32_t outer;      /* LM steps solved and judged                                  */
    int32_t accepted;   /* ... of which accepted                                       */
    int32_t pcg_total;  /* PCG iterations of all solves                                */
    int32_t pcg_capped; /* solves that ran max_pcg iterations without meeting pcg_rtol */
    int32_t stop_reason;
    int32_t pad;
    double cost_initial, cost_final; /* at the poses on entry / on return              */
    double grad_max;                 /* max|g_f| at the poses on return                */
    double lambda_final;
} lom_graph_stats;
typedef struct lom_graph lom_graph;

int lom_graph_create(int device, size_t node_hint, size_t edge_hint, lom_graph **out);
void lom_graph_destroy(lom_graph *g);
const char *lom_graph_last_error(const lom_graph *g); /* g == NULL: why the last create on this thread failed */
int lom_graph_clear(lom_graph *g);                    /* no nodes, no edges; ids start again at 0 */
void *lom_graph_stream(lom_graph *g);                 /* hipStream_t */
int lom_graph_device(const lom_graph *g);
/* new nodes; the return value is the (first) id or a negative lom_status.  A pose with a non-finite value or a zero
 * quaternion is LOM_ERR_ARG; with lom_graph_add_nodes nothing is added unless every pose is good.  fixed: one int per
 * node, non-zero = the node keeps its pose. */
int64_t lom_graph_add_node(lom_graph *g, const lom_graph_pose *pose, int fixed);
int64_t lom_graph_add_nodes(lom_graph *g, const lom_graph_pose *poses, const int32_t *fixed, size_t n);
/* new edges; the return value is the (first) id.  ij: n pairs (i, j); z: n poses; omega36: n * 36 values; delta: n values.
 * LOM_ERR_ARG for i == j, a node that does not exist, a bad pose, a bad Omega or a negative / non-finite delta; with
 * lom_graph_add_edges nothing is added unless every edge is good. */
int64_t lom_graph_add_edge(lom_graph *g, int64_t i, int64_t j, const lom_graph_pose *z, const double omega36[36],
                           double delta);
int64_t lom_graph_add_edges(lom_graph *g, const int32_t *ij, const lom_graph_pose *z, const double *omega36,
                            const double *delta, size_t n);
int64_t lom_graph_node_count(const lom_graph *g);
int64_t lom_graph_edge_count(const lom_graph *g);
int lom_graph_get_poses(lom_graph *g, int64_t first, int64_t n, lom_graph_pose *out);
int lom_graph_set_pose(lom_graph *g, int64_t id, const lom_graph_pose *pose);
int lom_graph_set_fixed(lom_graph *g, int64_t id, int fixed);
/* Levenberg-Marquardt as defined above, from the poses the graph holds, which it replaces.  A graph without an edge
 * returns at once (cost 0, LOM_GRAPH_STOP_GRADIENT).  stats may be NULL. */
int lom_graph_optimize(lom_graph *g, const lom_graph_params *params, lom_graph_stats *stats_or_null);
/* One linearisation at the current poses, read back; any output may be NULL.  e_out: 6 per edge; w_out: 1 per edge;
 * cost_out: 1; g_out: 6 per node; hdiag_out: 36 per node, the node's diagonal block of H_ff + lambda D, row-major.  A
 * fixed node's g and block read 0.  lambda >= 0 and finite. */
int lom_graph_evaluate(lom_graph *g, double lambda, double *e_out, double *w_out, double *cost_out, double *g_out,
                       double *hdiag_out);
/* y = (H_ff + lambda D) p at the current poses; p, y_out: 6 per node.  A fixed node's p counts as 0 and its y reads 0. */
int lom_graph_debug_matvec(lom_graph *g, double lambda, const double *p, double *y_out);
/* s = e^T Omega e of the edges [first, first + n) at the current poses: after an optimisation, what a caller looks at
 * to drop a false closure (and then builds the graph again without it). */
int lom_graph_edge_chi2(lom_graph *g, int64_t first, int64_t n, double *out);

/* Host functions of the pose graph; none needs a device. */
/* The gauge check alone.  fixed: n_nodes ints; ij: n_edges pairs.  LOM_OK, or LOM_ERR_ARG with *bad_node_or_null a free
 * node of a component without a fixed node (-1 where an edge has i == j or names a node that does not exist). */
int lom_graph_check_gauge(int64_t n_nodes, const int32_t *fixed, int64_t n_edges, const int32_t *ij,
                          int64_t *bad_node_or_null);
/* One step of the LM policy above.  denom = d^T (lambda D d - g_f).  Returns 1 (accepted) or 0 and updates *lambda and
 * *nu; *rho_gain_out = (cost - cost_new) / (0.5 denom).  A rho_gain that is not a number rejects. */
int lom_graph_lm_policy(double cost, double cost_new, double denom, double *lambda, double *nu, double *rho_gain_out);
/* Omega of an edge from the quality report of the align that measured it: S (H + P) S with
 * S = diag(1/2, 1/2, 1/2, 1, 1, 1) (the report's rotation tangent is half the rotation vector) and, for
 * with_prior != 0, P = 100 on the three translation diagonals (the align's translation prior, which the report leaves
 * out).  LOM_ERR_ARG for a report with valid < 7. */
int lom_graph_information_from_quality(const lom_quality_report *report, int with_prior, double omega_out[36]);
/* f32 pose (w, x, y, z quaternion) to the graph's and back (rounded to nearest) */
int lom_graph_pose_from_f32(const lom_pose *in, lom_graph_pose *out);
int lom_graph_pose_to_f32(const lom_graph_pose *in, lom_pose *out);

/* ---- scan archive and map assembly: rebuild a map from stored scans (not in the reference) -------------------------
 * The stage behind lom_graph_optimize: the optimised keyframe poses come in, together with the scans
 * they belong to, and the corrected map comes out -- a global map, or the odometry's keyframe
 * (lom_odometry_rebuild_keyframe).  The scans live in HBM and never pass through the host.
 *
 *  - Archive.  An append-only store of clouds in their own sensor frame: f32 points and f32 normals, 12 + 12 bytes per
 *    point, ragged lengths; a table on the host holds {offset, n} per scan.  Ids are 0, 1, 2, ... in order of arrival.
 *    Normals are required: an archive scan is what addCloud takes.  n == 0 is a valid, empty scan.  A host cloud with a
 *    non-finite coordinate is LOM_ERR_ARG; a device cloud is not looked at, and a non-finite coordinate in it is found
 *    when it is assembled, as a range error.  An archive holds at most 2^32 points: the kernels index with 32 bits.
 *  - Assembly.  lom_map_assemble(m, a, ids, poses, count, params, stats) leaves the map exactly as
 *    lom_map_add_points(m, C, Cn, |C|, 12) would, where C is the concatenation of the kept, transformed points of scan
 *    ids[k] at poses[k], for k = 0 .. count-1 in call order, and Cn their rotated normals.  Results are bytes, not
 *    tolerances.
 *  - Order is the priority.  A voxel keeps the first max_points points in that order, so the caller's order decides which
 *    points survive: newest first, or oldest first, is the caller's choice.  An id may appear more than once, each time
 *    with its own pose.
 *  - Rotation.  The quaternion is normalised on entry as lom_graph_add_node does (q / sqrt(((w w + x x) + y y) + z z)).
 *    With tx = 2x, ty = 2y, tz = 2z; twx = tx w, twy = ty w, twz = tz w; txx = tx x, txy = ty x, txz = tz x; tyy = ty y,
 *    tyz = tz y, tzz = tz z, all f64 and every operation rounded on its own:
 *        R = [ 1 - (tyy + tzz),  txy - twz,        txz + twy       ;
 *              txy + twz,        1 - (txx + tzz),  tyz - twx       ;
 *              txz - twy,        tyz + twx,        1 - (txx + tyy) ]   (row-major R0 .. R8)
 *    computed on the host; lom_graph_pose_rotation_matrix returns the same nine values.  t is the pose's.
 *  - Point.  x' = (f32)((R0 p0 + (R1 p1 + R2 p2)) + t0) in f64 from the f32 point, and y', z' likewise with rows 1 and
 *    2: the association order of lom_transform_points, widened to f64, with one rounding to f32 at the end.
 *  - Normal.  The same without t.
 *  - Cull.  params NULL or radius <= 0 keeps everything.  Otherwise, on the f32 result, with d = p' - centre (f32): the
 *    point is dropped iff dx dx + (dy dy + dz dz) > radius radius, all in f32, strict -- the predicate of
 *    lom_map_radius_cleanup, so a point at exactly the radius stays.  (A NaN compares false and stays, for the insert to
 *    refuse.)
 *  - Atomicity.  The call is atomic like the insert: with a kept point out of range (|x' / voxel_size| >= 2^20) or
 *    non-finite it returns LOM_ERR_RANGE and the map is unchanged.
 *  - Validation.  Ids, poses (finite, non-zero quaternion), the cull's values (finite) and the devices (the map's and the
 *    archive's must be the same; a scan context is refused) are checked before any launch: LOM_ERR_ARG.  More than 2^24
 *    scans or 2^31 - 2 points in one call are refused the same way.  count == 0, or a cloud that is empty before or
 *    after the cull, is LOM_OK and changes nothing.
 *  - Stats.  scans = count; points_in = the sum of the scans' sizes; points_kept = |C|; voxels_before / voxels_after /
 *    points_stored_after = lom_map_size and lom_map_point_count around the insert.  All zero on an error.
 *  - Cost.  Without a cull: one kernel, the insert, and the insert's verdict as the only host wait.  With a cull: three
 *    kernels (transform and count, prefix, compact), one read-back of |C| (4 bytes, one wait), then the insert.
 * The archive owns its stream; calls on one archive are serialised by a lock inside it, and lom_map_assemble holds it.
 * The archive's stream and the map's are ordered by events in both directions.  All arguments are validated before any
 * device work; a refused call leaves the archive as it was.  The archive grows geometrically past the hints given at
 * create (its clouds are copied device to device, ids and bytes stay); the staging buffers of the assembly belong to the
 * archive and are reused call after call. */
typedef struct lom_archive lom_archive;
typedef struct {
    float centre[3];
    float radius; /* <= 0: keep everything */
} lom_assemble_params;
typedef struct {
    int64_t scans, points_in, points_kept, voxels_before, voxels_after, points_stored_after;
} lom_assemble_stats;

int lom_archive_create(int device, size_t point_hint, size_t scan_hint, lom_archive **out);
void lom_archive_destroy(lom_archive *a);
const char *lom_archive_last_error(const lom_archive *a); /* a == NULL: why the last create on this thread failed */
int lom_archive_clear(lom_archive *a);                    /* no scans; ids start again at 0 */
void *lom_archive_stream(lom_archive *a);                 /* hipStream_t */
int lom_archive_device(const lom_archive *a);
/* the archive's stream waits for a hipEvent_t before what is enqueued next */
int lom_archive_wait_event(lom_archive *a, void *hip_event);
/* a new scan; the return value is its id or a negative lom_status.  Records of stride_bytes (>= 12, a multiple of 4)
 * that begin with x, y, z resp. nx, ny, nz.  The caller's buffers are its own again when the call returns.  The _device
 * form reads a cloud in HBM behind hip_event_or_null (the caller's producer), or behind nothing but the archive's own
 * stream when that is NULL. */
int64_t lom_archive_add(lom_archive *a, const float *xyz, const float *nrm, size_t n, size_t stride_bytes);
int64_t lom_archive_add_device(lom_archive *a, const float *d_xyz, const float *d_nrm, size_t n, size_t stride_bytes,
                               void *hip_event_or_null);
int64_t lom_archive_scan_count(const lom_archive *a);
int64_t lom_archive_point_count(const lom_archive *a);
int64_t lom_archive_scan_size(const lom_archive *a, int64_t id);
/* packed (12-byte) host copies of a scan; returns its size and writes at most `cap` points; either output may be NULL */
int64_t lom_archive_get(lom_archive *a, int64_t id, float *xyz_out, float *nrm_out, size_t cap);
int lom_map_assemble(lom_map *m, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                     const lom_assemble_params *params_or_null, lom_assemble_stats *stats_or_null);
/* Host function; needs no device.  int lom_graph_pose_rotation_matrix(const lom_graph_pose *pose, double R[9]): the
 * row-major R of the formula above from a pose's quaternion, normalised first; LOM_ERR_ARG for NULL, a non-finite value
 * or a zero quaternion.  It belongs to this section and not to the pose graph's, and is declared through its type. */
typedef int(lom_pose64_rotation_fn)(const lom_graph_pose *pose, double R_rowmajor[9]);
lom_pose64_rotation_fn lom_graph_pose_rotation_matrix;

/* ---- scan votes: moving objects out of an assembled map, scan by scan (not in the reference) ---------------------------
 * A map assembled from K archived scans holds everything that ever moved through it, and lom_map_carve_rays cannot
 * remove it: in such a map every voxel was hit by the scan that put it there.  Here every scan votes once per voxel --
 * "I saw through it" or "I saw it" -- and a rule on the two counts decides.  The definition, operation by operation
 * (tests/vote_ref.py restates it in numpy f64 and the results are compared bit for bit):
 *
 * Inputs: a map with voxel size v (f32), an archive, and ids[k], poses[k] for k = 0 .. count-1 exactly as
 * lom_map_assemble takes them, and the parameters below.  There are no defaults; margin < 0, min_range <= 0,
 * max_range <= min_range, clearance < 0, a non-finite value or min_free_scans == 0 is LOM_ERR_ARG.
 *
 * Per scan k:
 *  1. Points and normals.  The endpoint p'_i and the normal n'_i of every point of the scan are the f32 results of the
 *     assembly's transform ("Rotation", "Point" and "Normal" of the section above, byte for byte).  There is no cull:
 *     every point of the scan is a ray.
 *  2. Origin.  o_k = the pose's translation, each component rounded to f32.
 *  3. Hits.  As the carve: every endpoint, whatever its ray's length, marks the live voxel that contains it by the
 *     insert's index rule: hit_k[voxel] = 1.
 *  4. Walk.  The walk of "ray carving" with O = o_k and P = p'_i -- the same start cell, plane rule, tie order,
 *     recomputed t_a, step bound and range error -- but for t_end.  With N = n'_i, all f64 from the f32 inputs, every
 *     operation rounded on its own:
 *       c     = |Nx Dx + (Ny Dy + Nz Dz)| / L
 *       reach = min(L, max_range) - margin
 *       plane = L - clearance / c   when clearance > 0, else plane = reach
 *       t_end = (plane < reach ? plane : reach) / L
 *     The ray is walked iff L >= min_range and t_end > 0.  plane is where the ray comes within `clearance` of the plane
 *     through its endpoint with its endpoint's normal: a ray that grazes a surface stops before it runs inside that
 *     surface's layer of voxels.  With clearance > 0, a zero normal or a ray parallel to its plane has c == 0, plane =
 *     -inf, and is not walked; a NaN normal leaves reach (the comparison is false).
 *     cross_k[voxel] = 1 iff some walked ray of scan k visited the live voxel.
 *  5. Votes.  seen[voxel] = sum over k of hit_k; free[voxel] = sum over k of (cross_k && !hit_k).  Both count scans, so
 *     the density of points does not enter.  An id that appears twice votes twice, each time with its own pose.
 *  6. Decision.  A live voxel is erased iff free >= min_free_scans and (u64)free >= (u64)free_per_seen * seen.  Erasing
 *     is the carve's erase: in place, or compaction from a quarter of the slabs on (LOM_DENSE_CLEANUP=1: always); a later
 *     insert creates the voxel anew at the end of the creation order.
 *  7. Errors.  A non-finite origin or endpoint, or one whose voxel index leaves (-2^20, 2^20), or a walk that leaves
 *     that range, in any scan: LOM_ERR_RANGE, and the map is unchanged.  Ids, poses, devices and a scan context are
 *     refused as lom_map_assemble refuses them, before any launch (LOM_ERR_ARG).  count == 0 or only empty scans:
 *     LOM_OK, nothing changes.
 * The result is a pure function of the inputs: integer sums only, no order, and no dependence on how the scans are
 * grouped into launches (64 at a time; LOM_OPT_TEST_VOTE_SLICE_MAX).  The call holds the archive's lock, counts as a
 * change of the map, and a cleanup scan armed with lom_map_radius_cleanup_after_align is never taken across it.  The
 * error text is the map's (lom_last_error). */
typedef struct {
    float margin, min_range, max_range; /* as lom_carve_params: >= 0, > 0, > min_range */
    float clearance;         /* m, >= 0: the walk also ends where the ray is this close to its endpoint's plane; 0 = no such stop */
    uint32_t min_free_scans; /* >= 1 */
    uint32_t free_per_seen;  /* >= 0: free votes needed per seen vote */
} lom_vote_params;
typedef struct {
    uint64_t scans;                     /* count */
    uint64_t rays_walked, rays_skipped; /* rays_walked + rays_skipped == the sum of the scans' sizes */
    uint64_t cells_visited;             /* step 1 of the walk's loop, summed over all rays */
    uint32_t voxels_free;               /* live voxels with free >= 1 */
    uint32_t voxels_protected;          /* live voxels with free >= min_free_scans that the ratio kept */
    uint32_t voxels_erased;
} lom_vote_stats;
/* On an error the stats are all zero. */
int lom_map_carve_scans(lom_map *m, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                        const lom_vote_params *p, lom_vote_stats *stats_or_null);
/* erases nothing: free / seen per live voxel in lom_map_export's order.  Returns the number of live voxels; writes at
 * most `cap` entries; either output may be NULL.  Neither the map's change count nor an armed cleanup scan is touched. */
int64_t lom_map_scan_votes(lom_map *m, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                           const lom_vote_params *p, uint32_t *free_out, uint32_t *seen_out, size_t cap);

/* Scans without normals, for consumers that read points only (the occupancy grid below): a new scan whose normals are
 * stored as zeros.
 *   int64_t lom_archive_add_points(lom_archive *a, const float *xyz, size_t n, size_t stride_bytes);
 *   int64_t lom_archive_add_points_device(lom_archive *a, const float *d_xyz, size_t n, size_t stride_bytes,
 *                                         void *hip_event_or_null);
 * Everything else is lom_archive_add / lom_archive_add_device (ids, strides, the finite check of a host cloud, the
 * event).  Such a scan assembles like any other (its voxels get zero normals); in the scan votes a zero normal with
 * clearance > 0 has c == 0, plane = -inf, and its ray is not walked (step 4 there) -- it still hits.  Like
 * lom_graph_pose_rotation_matrix above, the two are declared through their types. */
typedef int64_t(lom_archive_points_fn)(lom_archive *a, const float *xyz, size_t n, size_t stride_bytes);
typedef int64_t(lom_archive_points_device_fn)(lom_archive *a, const float *d_xyz, size_t n, size_t stride_bytes,
                                              void *hip_event_or_null);
lom_archive_points_fn lom_archive_add_points;
lom_archive_points_device_fn lom_archive_add_points_device;

/* ---- occupancy grid: free, occupied and unknown cells from posed scans (not in the reference) ------------------------
 * The map holds surfaces only: "measured empty" and "never looked at" are both a missing voxel.  A planner needs the
 * difference, per ground cell, in the form of nav_msgs/OccupancyGrid.  Here every scan at its pose votes once per cell
 * of a dense 2-D grid -- "a ray of mine passed through it" or "a point of mine fell into it" -- and a rule on the two
 * integer counts classifies.  A handle family of its own beside the map path: nothing is launched unless a caller
 * creates a grid.  The definition, operation by operation (tests/occupancy_ref.py restates it in numpy f64 and the
 * results are compared exactly: counts are integer sums of bits, there is no tolerance anywhere):
 *
 * Grid.  lom_occupancy_geometry: cell (ix, iy) covers [origin + i r, origin + (i + 1) r) per axis; storage is row-major
 * with y as the row, iy * width + ix.  The index rule is floor, NOT the map's truncation, in f64 from the f32 values:
 * floor(((double)X - (double)origin_x) / (double)r).  A value is "in the grid" iff the floored f64 quotient q satisfies
 * 0 <= q < width (resp. height), compared before any integer conversion.  r > 0 and finite, 1 <= width, height <= 16384,
 * a finite origin; anything else is LOM_ERR_ARG.
 *
 * Ray parameters.  lom_occupancy_ray_params, no defaults: z_lo < 0 < z_hi (the height band relative to the scan
 * origin's z, in the grid's frame), margin >= 0, min_range > 0, max_range > min_range, all finite, and
 * max_range / resolution <= 2^20; anything else is LOM_ERR_ARG.
 *
 * Per scan k (pose = a lom_graph_pose, cloud = n points in the sensor frame), all f64 from f32 inputs, every operation
 * rounded on its own, no contraction:
 *  1. Endpoint.  p' is the f32 result of the assembly's "Rotation" and "Point" rules, byte for byte; P is p' widened.
 *     Normals are never read.
 *  2. Origin.  O = the pose's translation, each component rounded to f32 and widened.  G = (origin_x, origin_y) widened.
 *     O2_a = O_a - G_a for a = x, y.  Start cell c_a = floor(O2_a / r).  If |c_a| >= 2^30 on either axis (or it is not
 *     finite) the whole call is LOM_ERR_RANGE, before any launch, and nothing changes.
 *  3. Ray.  D = P - O (three components);  L = sqrt(Dx Dx + (Dy Dy + Dz Dz));
 *       t_band = Dz > 0 ? z_hi / Dz : (Dz < 0 ? z_lo / Dz : +inf)
 *       reach  = (L < max_range ? L : max_range) - margin
 *       q      = reach / L
 *       t_end  = q < t_band ? q : t_band
 *     The ray is walked iff L >= min_range and t_end > 0.
 *  4. Hit.  The endpoint is a hit iff L >= min_range, L <= max_range, z_lo <= Dz <= z_hi and its cell
 *     floor((P_a - G_a) / r), a = x, y, is in the grid; then hit_k[cell] = 1.  A non-finite endpoint is neither walked
 *     nor a hit: the comparisons above already give that (a NaN fails them all; an infinite L exceeds max_range and
 *     makes q, and with it t_end, zero).
 *  5. Walk (2-D, parameter t along the 3-D ray).  Per axis a = x, y with D_a != 0: s_a = the sign of D_a, the next plane
 *     b_a = s_a > 0 ? c_a + 1 : c_a, t_a = ((double)b_a r - O2_a) / D_a; with D_a == 0, t_a = +inf.  Loop:
 *       1. the current cell counts as passed if it is in the grid;
 *       2. a = the axis with the smaller t_a, ties to x;
 *       3. if !(t_a <= t_end) stop;
 *       4. c_a += s_a, and t_a is recomputed from the new c_a -- never incremented.
 *     A t_a <= 0 (an origin on a plane) simply sorts first.  At most 2 (ceil(max_range / r) + 2) steps can occur, and
 *     the kernel's loop is bounded by that.  Cells outside the grid count for nothing; an origin outside the grid is
 *     legal.  pass_k[cell] = 1 iff some walked ray of scan k visited the cell.
 *  6. Votes.  seen[cell] += hit_k;  free[cell] += pass_k && !hit_k.  Both are u32 and count scans, not rays.  An id given
 *     twice votes twice.  Counts accumulate over calls until lom_occupancy_clear.
 *  7. Classification.  lom_occupancy_rule with min_free_scans >= 1 and min_seen_scans >= 1 (else LOM_ERR_ARG):
 *     LOM_OCC_FREE (0) iff free >= min_free_scans and (u64)free >= (u64)free_per_seen * seen -- the votes' erase rule;
 *     else LOM_OCC_OCCUPIED (100) iff seen >= min_seen_scans; else LOM_OCC_UNKNOWN (-1).  int8, row-major: the values of
 *     nav_msgs/OccupancyGrid.
 * The result is a pure function of the inputs: it does not depend on the order of scans, rays or calls, on how scans are
 * grouped into launches (LOM_OCC_OPT_TEST_SLICE_MAX), or on any kernel tuning (LOM_OCC_OPT_TEST_WINDOW).
 *
 * lom_occupancy_integrate takes K archived scans exactly as lom_map_assemble takes them; ids, poses and the device are
 * refused before any launch the same way (LOM_ERR_ARG).  The call holds the archive's lock, and the archive's stream and
 * the grid's are ordered by events in both directions.  The _cloud forms integrate one scan that is not in an archive:
 * records of stride_bytes (>= 12, a multiple of 4) that begin with x, y, z, in host memory, or in HBM behind
 * hip_event_or_null.  count == 0 or n == 0 is LOM_OK and changes nothing.  Stats: scans = count; rays_walked +
 * rays_skipped = the sum of the scans' sizes; endpoints_marked = the rays that are hits; cells_visited = step 1 of the
 * walk's loop summed over all rays, in the grid or not.  All zero on an error.  Every call returns with its work done.
 * Calls on one grid are the caller's to serialise.  The error text is the grid's (lom_occupancy_last_error). */
typedef struct lom_occupancy lom_occupancy;
typedef struct {
    float resolution;         /* m per cell */
    float origin_x, origin_y; /* the corner of cell (0, 0) */
    uint32_t width, height;   /* cells along x and along y */
} lom_occupancy_geometry;
typedef struct {
    float z_lo, z_hi; /* < 0 < : the band around the scan origin's z */
    float margin, min_range, max_range;
} lom_occupancy_ray_params;
typedef struct {
    uint32_t min_free_scans; /* >= 1 */
    uint32_t free_per_seen;  /* >= 0: free votes needed per seen vote */
    uint32_t min_seen_scans; /* >= 1 */
} lom_occupancy_rule;
typedef struct {
    uint64_t scans, rays_walked, rays_skipped, endpoints_marked, cells_visited;
} lom_occupancy_stats;
typedef struct {
    uint64_t cells_free, cells_occupied, cells_unknown;
} lom_occupancy_summary;
enum { LOM_OCC_FREE = 0, LOM_OCC_OCCUPIED = 100, LOM_OCC_UNKNOWN = -1 };
enum {
    LOM_OCC_OPT_TEST_SLICE_MAX = 1, /* s in 1 .. 64: a launch holds at most s scans (0: what the scratch budget admits, 64 at most) */
    LOM_OCC_OPT_TEST_WINDOW = 2     /* the side of the walk's LDS window in cells: a multiple of 32 up to 512; 0: no window, every
                                       bit goes to global memory; < 0: the default */
};
int lom_occupancy_create(const lom_occupancy_geometry *geometry, int device, lom_occupancy **out);
void lom_occupancy_destroy(lom_occupancy *g);
const char *lom_occupancy_last_error(const lom_occupancy *g); /* g == NULL: why the last create on this thread failed */
int lom_occupancy_clear(lom_occupancy *g);                    /* all counts to zero */
int lom_occupancy_get_geometry(const lom_occupancy *g, lom_occupancy_geometry *out);
void *lom_occupancy_stream(lom_occupancy *g); /* hipStream_t */
int lom_occupancy_device(const lom_occupancy *g);
int lom_occupancy_wait_event(lom_occupancy *g, void *hip_event);
int lom_occupancy_set_option(lom_occupancy *g, int option, int64_t value);
int lom_occupancy_integrate(lom_occupancy *g, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                            const lom_occupancy_ray_params *p, lom_occupancy_stats *stats_or_null);
int lom_occupancy_integrate_cloud(lom_occupancy *g, const float *xyz, size_t n, size_t stride_bytes,
                                  const lom_graph_pose *pose, const lom_occupancy_ray_params *p,
                                  lom_occupancy_stats *stats_or_null);
int lom_occupancy_integrate_cloud_device(lom_occupancy *g, const float *d_xyz, size_t n, size_t stride_bytes,
                                         const lom_graph_pose *pose, const lom_occupancy_ray_params *p,
                                         void *hip_event_or_null, lom_occupancy_stats *stats_or_null);
/* free / seen per cell, row-major; returns width * height and writes at most `cap` entries; either output may be NULL */
int64_t lom_occupancy_counts(lom_occupancy *g, uint32_t *free_out, uint32_t *seen_out, size_t cap);
/* step 7 over the whole grid: at most `cap` cells go to `out` (may be NULL with cap 0); the summary counts all cells */
int lom_occupancy_classify(lom_occupancy *g, const lom_occupancy_rule *rule, int8_t *out, size_t cap,
                           lom_occupancy_summary *summary_or_null);
/* the same, left in HBM: *d_out holds width * height cells, complete on the grid's stream, valid until the next call
 * on the handle */
int lom_occupancy_classify_device(lom_occupancy *g, const lom_occupancy_rule *rule, const int8_t **d_out);

/* ---- elevation grid: ground height, slope, step and cost from posed scans (not in the reference) ----------------------
 * The occupancy grid above is flat: a cell is hit when a point falls into a band around the sensor's z, and it carries no
 * height.  A ground robot's planner asks for the 2.5-D product beside it -- ground height per cell, slope, step height,
 * roughness and a traversability cost (the "elevation" and "traversability" layers of grid-map style stacks).  A handle
 * family of its own: nothing is launched unless a caller creates a grid.  The definition, operation by operation
 * (tests/elevation_ref.py restates it in numpy f64; every comparison is exact: the accumulators are integers, and every
 * f64 operation below is rounded on its own, no contraction).  There are no floating-point atomics anywhere.
 *
 * Grid.  lom_elevation_geometry = the fields of lom_occupancy_geometry and z_ref.  Cell (ix, iy) covers
 * [origin + i r, origin + (i + 1) r) per axis; storage is row-major with y as the row, iy * width + ix; the index rule is
 * floor in f64 from the f32 values, floor(((double)X - (double)origin_x) / (double)r), and a value is "in the grid" iff
 * the floored quotient q satisfies 0 <= q < width (resp. height), compared before any integer conversion.  r > 0 and
 * finite, a finite origin, a finite z_ref, 1 <= width, height <= 8192; anything else is LOM_ERR_ARG.  A cell costs
 * 33 bytes of HBM at rest (a record of 32 bytes: sum, count, zmin, zmax, 12 bytes of padding so that a record is one
 * aligned 32-byte sector; 1 byte of cost) and 24 more (six f32 layers) from the first lom_elevation_layers on.
 * Heights are kept in quanta of Q = 2^LOM_ELEV_QUANTUM_LOG2 m = 1/256 m, relative to z_ref.
 *
 * Which points count.  lom_elevation_point_params, no defaults: z_lo < 0 < z_hi, min_range > 0, max_range > min_range,
 * all finite, max_range / resolution <= 2^20; anything else is LOM_ERR_ARG.  For scan k at its pose, the endpoint p',
 * the origin O, D, L and the cell are exactly steps 1 to 4 of the occupancy definition (step 2's verdict included: a
 * start cell beyond 2^30 or not finite is LOM_ERR_RANGE for the whole call, before any launch).  A point contributes iff
 * it is a hit there: L >= min_range, L <= max_range, z_lo <= Dz <= z_hi, and its cell is in the grid; a non-finite
 * endpoint fails those comparisons by itself.  Then
 *     h = (double)p'_z - (double)z_ref;
 *     if !(|h| < 2048) the point does not contribute and counts in points_out_of_height;
 *     else zq = rint(h * 256.0), ties to even, so |zq| <= 2^19.
 *
 * Accumulators per cell, integers, accumulated over calls until lom_elevation_clear:
 *     count u32 += 1 (empty: 0);  zmin i32 min= zq (empty: INT32_MAX);  zmax i32 max= zq (empty: INT32_MIN);
 *     sum i64 += zq (empty: 0).
 * An id given twice counts twice.  More than 2^32 - 1 points in one cell wrap its count: the caller's to avoid.
 * Integer sums, minima and maxima do not depend on order, so the cells are a pure function of the inputs: independent of
 * the order of points, scans and calls, and of any kernel tuning (LOM_ELEV_OPT_TEST_WAVE_MERGE).
 *
 * Stats.  scans = count; points = the sum of the scans' sizes; points_marked = the points that contributed;
 * points_out_of_height as above (hits that did not); cells_new = the cells whose count left 0 in this call.  All zero
 * on an error.
 *
 * Derived layers.  lom_elevation_layer_params: min_points >= 1, window R in 1 .. 4 (else LOM_ERR_ARG).  A cell is valid
 * iff count >= min_points; its ground height is zmin.  For a valid cell c at (cx, cy) take the valid cells (cx + i, cy + j),
 * -R <= i, j <= R, that lie in the grid -- c itself, i = j = 0, included -- with d = zmin(cx + i, cy + j) - zmin(c):
 *  1. The int64 sums n = sum 1, Si = sum i, Sj = sum j, Sii = sum i i, Sij = sum i j, Sjj = sum j j, Sd = sum d,
 *     Sid = sum i d, Sjd = sum j d.  All exact: n <= 81, |Si|, |Sj| <= 4 * 81 = 324, Sii, |Sij|, Sjj <= 16 * 81 = 1296,
 *     |d| <= 2^20, so |Sd| <= 81 * 2^20 and |Sid|, |Sjd| <= 324 * 2^20.
 *  2. The plane d ~ A i + B j + C by Cramer's rule in int64, each 3 x 3 determinant expanded along its first row:
 *       det   = Sii * (Sjj * n   - Sj  * Sj) - Sij * (Sij * n   - Sj  * Si) + Si  * (Sij * Sj - Sjj * Si)
 *       a_num = Sid * (Sjj * n   - Sj  * Sj) - Sij * (Sjd * n   - Sj  * Sd) + Si  * (Sjd * Sj - Sjj * Sd)
 *       b_num = Sii * (Sjd * n   - Sj  * Sd) - Sid * (Sij * n   - Sj  * Si) + Si  * (Sij * Sd - Sjd * Si)
 *       c_num = Sii * (Sjj * Sd  - Sjd * Sj) - Sij * (Sij * Sd  - Sjd * Si) + Sid * (Sij * Sj - Sjj * Si)
 *     Every product of three sums is bounded by the largest one of its kind: in det, 1296 * 1296 * 81 < 2^28; in a_num
 *     and b_num, (324 * 2^20) * 1296 * 81 < 2^45.1; in c_num, 1296 * 1296 * (81 * 2^20) < 2^47.1.  A determinant is
 *     six such products, so |det| < 2^31, |a_num|, |b_num| < 2^47.7 and |c_num| < 2^49.7: all below 2^53, exact in
 *     int64 and exactly convertible to f64.  det >= 0 always (a Gram determinant).
 *  3. If det > 0:  A = (double)a_num / (double)det, B and C likewise;
 *       slope = (sqrt(A * A + B * B) * Q) / (double)resolution            -- the rise over run
 *       e = (double)d - ((A * (double)i + B * (double)j) + C),  S = sum e * e, added in row-major order (j ascending,
 *       then i ascending) over the valid cells, starting from 0.0;
 *       rough = sqrt(S / (double)n) * Q.
 *  4. If det == 0 (fewer than three valid cells, or collinear ones): slope and rough are NaN.
 *  5. step = Q * (double)(max |d| over the valid cells among the 8 neighbours |i|, |j| <= 1 in the grid), 0 if none.
 *  6. span = Q * (double)(zmax(c) - zmin(c)).
 * The f32 outputs min, max, mean, slope, rough, step: min = (float)((double)z_ref + (double)zmin * Q), max likewise,
 * mean = (float)((double)z_ref + ((double)sum * Q) / (double)count); slope, rough and step are the f64 values rounded.
 * All six are NaN where the cell is invalid.
 *
 * Cost.  lom_elevation_cost_params: max_slope, max_step, max_rough, max_span, all finite and > 0 (else LOM_ERR_ARG),
 * widened to f64 and compared with the f64 values above.  int8, row-major, the values of a nav_msgs costmap:
 *   LOM_ELEV_COST_UNKNOWN (-1) for an invalid cell;
 *   LOM_ELEV_COST_LETHAL (100) iff span > max_span, or step > max_step, or det > 0 && slope > max_slope;
 *   else floor(99 * min(m, 1)) with m = the largest of step / max_step, slope / max_slope and rough / max_rough, the
 *   latter two taken as 0 where det == 0.
 * Summary: cells_unknown + cells_lethal + cells_costed = width * height.
 *
 * lom_elevation_integrate takes K archived scans exactly as lom_occupancy_integrate takes them: ids, poses and the device
 * are refused before any launch the same way, the call holds the archive's lock, and the two streams are ordered by
 * events in both directions.  The _cloud forms integrate one scan that is not in an archive: records of stride_bytes
 * (>= 12, a multiple of 4) that begin with x, y, z, in host memory, or in HBM behind hip_event_or_null.  count == 0 or
 * n == 0 is LOM_OK and changes nothing.  All arguments are validated before any device work; a refused call changes
 * nothing.  Every call returns with its work done.  Calls on one grid are the caller's to serialise.  The error text is
 * the grid's (lom_elevation_last_error). */
#define LOM_ELEV_QUANTUM_LOG2 (-8)
typedef struct lom_elevation lom_elevation;
typedef struct {
    float resolution;         /* m per cell */
    float origin_x, origin_y; /* the corner of cell (0, 0) */
    uint32_t width, height;   /* cells along x and along y */
    float z_ref;              /* heights are stored relative to it */
} lom_elevation_geometry;
typedef struct {
    float z_lo, z_hi; /* < 0 < : the band around the scan origin's z */
    float min_range, max_range;
} lom_elevation_point_params;
typedef struct {
    uint64_t scans, points, points_marked, points_out_of_height, cells_new;
} lom_elevation_stats;
typedef struct {
    uint32_t min_points; /* >= 1 */
    uint32_t window;     /* R in 1 .. 4: the fit looks at (2R + 1)^2 cells */
} lom_elevation_layer_params;
typedef struct {
    float max_slope, max_step, max_rough, max_span; /* rise over run; m; m; m */
} lom_elevation_cost_params;
typedef struct {
    uint64_t cells_unknown, cells_lethal, cells_costed;
} lom_elevation_summary;
enum { LOM_ELEV_COST_UNKNOWN = -1, LOM_ELEV_COST_LETHAL = 100 };
enum {
    LOM_ELEV_OPT_TEST_WAVE_MERGE = 1 /* 0: every lane sends its own four atomics; 1 or < 0, the default: the lanes of a
                                        wave that share a cell are merged first.  A test switch: the cells are the same. */
};
int lom_elevation_create(const lom_elevation_geometry *geometry, int device, lom_elevation **out);
void lom_elevation_destroy(lom_elevation *g);
const char *lom_elevation_last_error(const lom_elevation *g); /* g == NULL: why the last create on this thread failed */
int lom_elevation_clear(lom_elevation *g);                    /* every cell to its empty values */
int lom_elevation_get_geometry(const lom_elevation *g, lom_elevation_geometry *out);
void *lom_elevation_stream(lom_elevation *g); /* hipStream_t */
int lom_elevation_device(const lom_elevation *g);
int lom_elevation_wait_event(lom_elevation *g, void *hip_event);
int lom_elevation_set_option(lom_elevation *g, int option, int64_t value);
int lom_elevation_integrate(lom_elevation *g, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                            const lom_elevation_point_params *p, lom_elevation_stats *stats_or_null);
int lom_elevation_integrate_cloud(lom_elevation *g, const float *xyz, size_t n, size_t stride_bytes,
                                  const lom_graph_pose *pose, const lom_elevation_point_params *p,
                                  lom_elevation_stats *stats_or_null);
int lom_elevation_integrate_cloud_device(lom_elevation *g, const float *d_xyz, size_t n, size_t stride_bytes,
                                         const lom_graph_pose *pose, const lom_elevation_point_params *p,
                                         void *hip_event_or_null, lom_elevation_stats *stats_or_null);
/* the accumulators per cell, row-major; returns width * height and writes at most `cap` entries; any output may be NULL */
int64_t lom_elevation_cells(lom_elevation *g, uint32_t *count_out, int32_t *zmin_out, int32_t *zmax_out, int64_t *sum_out,
                            size_t cap);
/* the six f32 layers over the whole grid; at most `cap` cells go to each output; any output may be NULL */
int lom_elevation_layers(lom_elevation *g, const lom_elevation_layer_params *lp, float *min_out, float *max_out,
                         float *mean_out, float *slope_out, float *rough_out, float *step_out, size_t cap);
/* the cost over the whole grid: at most `cap` cells go to `out` (may be NULL with cap 0); the summary counts all cells */
int lom_elevation_cost(lom_elevation *g, const lom_elevation_layer_params *lp, const lom_elevation_cost_params *cp,
                       int8_t *out, size_t cap, lom_elevation_summary *summary_or_null);
/* the same, left in HBM: *d_out holds width * height cells, complete on the grid's stream, valid until the next call
 * on the handle */
int lom_elevation_cost_device(lom_elevation *g, const lom_elevation_layer_params *lp, const lom_elevation_cost_params *cp,
                              const int8_t **d_out);

/* ---- clearance grid: obstacle distance and inflated cost from the two grids (not in the reference) --------------------
 * The occupancy and the elevation grid each leave an int8 plane in HBM.  A planner reads neither as it is: it reads, per
 * cell, the distance to the nearest obstacle and a cost that is lethal on the obstacle, "inscribed" within the robot's
 * radius and decays out to an inflation radius (the inflation layer of nav2-style stacks).  This handle family merges the
 * two planes, computes an exact truncated Euclidean distance transform on the device and the inflated cost from it.
 * Nothing is launched unless a caller creates a clearance grid.  The definition, operation by operation
 * (tests/clearance_ref.py restates it in numpy; the distance is an integer -- squared cells -- so every comparison is
 * exact; the one tolerance of the feature is the last ulp of exp() in the host-built cost table, see step 3):
 *
 * Grid.  lom_occupancy_geometry, reused: cell (ix, iy) covers [origin + i r, origin + (i + 1) r) per axis, storage is
 * row-major with y as the row, the index rule is the occupancy grid's floor rule.  r > 0 and finite, a finite origin,
 * 1 <= width, height <= 8192; anything else is LOM_ERR_ARG.  A cell costs 5 bytes and 1 bit of HBM at rest (base i8, d2 u16,
 * cost i8, a bitmap bit), 2 more from the first update with host planes on.
 *
 * Inputs of an update.  Two full-grid int8 planes, either of which may be NULL (it then reads as all -1), not both:
 * occ holds -1 / 0 / 100, elev holds -1 / 0 .. 99 / 100.  Any other value reads as -1, and a cell with such a value in
 * either plane counts once in cells_invalid.  lom_clearance_params: 0 <= inscribed_radius <= inflation_radius,
 * decay >= 0, all finite, no unknown bit in flags, R (step 2) <= 254; anything else is LOM_ERR_ARG.
 *  1. Merge.  With o and e the cell's two values:
 *       cleared  = e == 100 && (flags & LOM_CLEAR_FREE_CLEARS_ELEVATION) && o == 0: the cell counts in cells_cleared and
 *                  reads e = 0 -- a FREE vote of the occupancy grid drops the ghost height a mover left;
 *       base     = 100 if o == 100 || e == 100;  else e if 0 <= e <= 99;  else 0 if o == 0;  else -1.
 *     A cell is an obstacle iff base == 100, or base == -1 and flags & LOM_CLEAR_UNKNOWN_IS_OBSTACLE.  Cells outside the
 *     grid are never obstacles.
 *  2. Distance.  R = floor((double)inflation_radius / (double)r), 0 <= R <= 254.  d2[cell] = the minimum over all obstacle
 *     cells of dx^2 + dy^2, in cells, if that is <= R^2; else LOM_CLEAR_FAR (65535).  u16: 254^2 = 64516 fits.
 *  3. Cost table, R^2 + 1 bytes, built on the host in f64.  With dist = sqrt((double)k) * (double)r, in this order:
 *       table[0] = 100;  99 where dist <= inscribed_radius;  0 where dist > inflation_radius;
 *       else floor(98 * exp(-(double)decay * (dist - (double)inscribed_radius))).
 *     The device only indexes it: no transcendental runs on the device.  lom_clearance_cost_table gives the bytes.
 *  4. Cost.  c = table[d2], 0 where d2 is far.  An obstacle gives 100; a known base (0 .. 99) gives max(base, c); an
 *     unknown base gives c if c > 0, else -1.  int8, the value range of nav_msgs/OccupancyGrid.
 *  5. Metres.  lom_clearance_distance gives (float)(sqrt((double)d2) * (double)r), +inf where d2 is far.
 * Summary, counted over the updated rectangle: cells_lethal (cost 100), cells_inscribed (99), cells_costed (0 .. 98),
 * cells_unknown (-1) -- the four add up to the rectangle's cells -- and cells_invalid, cells_cleared as above.
 *
 * Window.  An update takes an optional rectangle {x0, y0, width, height} in cells, clipped to the grid; NULL is the whole
 * grid; an empty rectangle is LOM_OK and changes nothing.  Only the rectangle's d2 and cost are rewritten.  Obstacles up
 * to R cells outside the rectangle count: they are read from the planes given to this call, so a windowed update over any
 * rectangle gives, on that rectangle, the bytes of the full update of the same planes.  After create or
 * lom_clearance_clear: d2 = far, cost = -1 everywhere.
 *
 * The result is a pure function of the inputs: it does not depend on the tile shape (LOM_CLEAR_OPT_TEST_TILE_ROWS), on
 * the pruning of the column pass (LOM_CLEAR_OPT_TEST_NO_PRUNE) or on how the work is cut into launches.
 *
 * lom_clearance_update takes host planes of width * height bytes; _update_device takes planes in HBM that are complete
 * when hip_event_or_null is (NULL: now).  _update_from_grids calls lom_occupancy_classify_device and
 * lom_elevation_cost_device itself (either grid may be NULL, not both; the parameters of a NULL grid are not read) and
 * orders the three streams by events in both directions; grids whose resolution, origin, width or height differ bit for
 * bit from the clearance grid's, or that live on another device, are LOM_ERR_ARG before any launch, as are bad
 * parameters of any of the three.  Every argument is validated before any device work; a refused call changes nothing
 * and zeroes the summary.  Every call returns with its work done.  Calls on one grid are the caller's to serialise.  The
 * error text is the grid's (lom_clearance_last_error). */
typedef struct lom_clearance lom_clearance;
typedef struct {
    float inflation_radius; /* m: beyond it the distance is "far" and the table is 0 */
    float inscribed_radius; /* m: within it the cost is 99 */
    float decay;            /* 1 / m: the exponent of the decay between the two */
    uint32_t flags;         /* LOM_CLEAR_* */
} lom_clearance_params;
typedef struct {
    int32_t x0, y0;         /* may lie outside the grid: the rectangle is clipped */
    uint32_t width, height; /* cells */
} lom_clearance_window;
typedef struct {
    uint64_t cells_lethal, cells_inscribed, cells_costed, cells_unknown, cells_invalid, cells_cleared;
} lom_clearance_summary;
#define LOM_CLEAR_FAR 65535
enum {
    LOM_CLEAR_FREE_CLEARS_ELEVATION = 1, /* a lethal elevation cell that the occupancy grid calls free reads as 0 */
    LOM_CLEAR_UNKNOWN_IS_OBSTACLE = 2    /* a cell unknown to both planes is an obstacle */
};
enum {
    LOM_CLEAR_OPT_TEST_TILE_ROWS = 1, /* T in 1 .. 32: rows of a tile of the distance kernel; <= 0: the default, 32 */
    LOM_CLEAR_OPT_TEST_NO_PRUNE = 2   /* 1: the column pass looks at all 2R + 1 rows; 0 or < 0, the default: it stops once
                                         dy^2 reaches the best so far.  Test switches: the bytes are the same. */
};
int lom_clearance_create(const lom_occupancy_geometry *geometry, int device, lom_clearance **out);
void lom_clearance_destroy(lom_clearance *c);
const char *lom_clearance_last_error(const lom_clearance *c); /* c == NULL: why the last create on this thread failed */
int lom_clearance_clear(lom_clearance *c);                    /* d2 = far, cost = -1 */
int lom_clearance_get_geometry(const lom_clearance *c, lom_occupancy_geometry *out);
void *lom_clearance_stream(lom_clearance *c); /* hipStream_t */
int lom_clearance_device(const lom_clearance *c);
int lom_clearance_wait_event(lom_clearance *c, void *hip_event);
int lom_clearance_set_option(lom_clearance *c, int option, int64_t value);
int lom_clearance_update(lom_clearance *c, const int8_t *occ_or_null, const int8_t *elev_or_null,
                         const lom_clearance_params *params, const lom_clearance_window *window_or_null,
                         lom_clearance_summary *summary_or_null);
int lom_clearance_update_device(lom_clearance *c, const int8_t *d_occ_or_null, const int8_t *d_elev_or_null,
                                void *hip_event_or_null, const lom_clearance_params *params,
                                const lom_clearance_window *window_or_null, lom_clearance_summary *summary_or_null);
int lom_clearance_update_from_grids(lom_clearance *c, lom_occupancy *occupancy_or_null, const lom_occupancy_rule *rule,
                                    lom_elevation *elevation_or_null, const lom_elevation_layer_params *layer_params,
                                    const lom_elevation_cost_params *cost_params, const lom_clearance_params *params,
                                    const lom_clearance_window *window_or_null, lom_clearance_summary *summary_or_null);
/* the cost over the whole grid: at most `cap` cells go to `out` (may be NULL with cap 0); the summary counts all cells of
 * the plane as it stands (cells_invalid and cells_cleared are 0: they belong to an update) */
int lom_clearance_cost(lom_clearance *c, int8_t *out, size_t cap, lom_clearance_summary *summary_or_null);
/* the same plane, left in HBM: width * height cells, valid until the next update or clear on the handle */
int lom_clearance_cost_device(lom_clearance *c, const int8_t **d_out);
/* d2 per cell (step 2) and metres per cell (step 5), row-major; at most `cap` entries */
int lom_clearance_distance_sq(lom_clearance *c, uint16_t *out, size_t cap);
int lom_clearance_distance(lom_clearance *c, float *out, size_t cap);
/* step 3 for these parameters on a grid of this resolution: returns R^2 + 1 and writes at most `cap` bytes (out may be
 * NULL with cap 0); LOM_ERR_ARG for a bad geometry or bad parameters.  Needs no handle and no device. */
int64_t lom_clearance_cost_table(const lom_clearance_params *params, const lom_occupancy_geometry *geometry, uint8_t *out,
                                 size_t cap);
/* n points (x, y in the grid's frame, f32 pairs in host memory): the cell by the floor rule, its distance in metres (step
 * 5) and its cost; NaN and -1 for a point outside the grid or not a number.  Either output may be NULL. */
int lom_clearance_query(lom_clearance *c, const float *xy, size_t n, float *dist_out, int8_t *cost_out);

/* ---- navigation field: cost-to-go from goals over the clearance cost (not in the reference) ----------------------------
 * The clearance grid leaves an inflated int8 cost plane in HBM.  A planner reads, per cell, the least total cost to reach
 * a goal -- the navigation function of nav2-style stacks -- and a route from any start follows its descent.  This handle
 * family computes that field on the device, entirely on integers, traces paths down it and answers point queries.
 * Nothing is launched unless a caller creates a field.  The definition, operation by operation (tests/navfield_ref.py
 * restates it with a heap Dijkstra on Python integers; the field is the unique fixed point of a relaxation, so every
 * comparison is exact):
 *
 * Grid.  lom_occupancy_geometry, reused, with the clearance grid's rules: cell (ix, iy) covers [origin + i r, origin +
 * (i + 1) r) per axis, storage is row-major with y as the row, the index rule is the floor rule.  r > 0 and finite, a
 * finite origin, 1 <= width, height <= 8192; anything else is LOM_ERR_ARG.  A cell costs 5 bytes of HBM (P u32, the cost
 * byte of the last solve i8).
 *
 * Input of a solve.  One full-grid int8 cost plane in the value range lom_clearance_cost writes: -1, 0 .. 99, 100.
 * lom_navfield_params: neutral >= 1; 0 <= max_passable <= 98; neutral + 98 * factor <= 2^24 - 1; unknown_cost in
 * 1 .. 2^24 - 1 when LOM_NAV_UNKNOWN_PASSABLE is set (it is not read otherwise); no unknown bit in flags; anything else is
 * LOM_ERR_ARG.
 *  1. Cell cost.  A table of 256 u32, built on the host and indexed by the cost byte read as unsigned: a value v in
 *     0 .. max_passable gives neutral + factor * v; -1 gives unknown_cost under LOM_NAV_UNKNOWN_PASSABLE, else 0; every
 *     other byte gives 0 -- max_passable + 1 .. 100, and the bytes outside -1 .. 100, which also count in cells_invalid.
 *     0 means impassable.  Cells outside the grid are impassable.  lom_navfield_cell_costs gives the table.
 *  2. Steps.  8-connected.  An axial step has length 5, a diagonal step 7 (7 / 5 is within 1.01 % of sqrt 2).  A step
 *     from a to b is allowed iff both cells are passable and, for a diagonal step, so are the two cells that share an edge
 *     with both: no corner is cut.  Its weight is len(a, b) * c[a]: a step pays for the cell it leaves.
 *  3. Goals.  G cells, as int32 (ix, iy) pairs (LOM_NAV_CELLS) or as f32 (x, y) in metres by the floor rule
 *     (LOM_NAV_METRES).  A goal outside the grid, not a number or on an impassable cell is skipped and counts in
 *     goals_rejected; the others, duplicates once, count in goals_used.  G = 0 or goals_used == 0 is LOM_OK with every
 *     cell unreached.
 *  4. Field.  P[goal] = 0; else P[a] = the least total weight over all sequences of allowed steps from a to any goal;
 *     u32.  LOM_NAV_UNREACHED = 0xFFFFFFFF, LOM_NAV_MAX = 0xFFFFFFFE.  A candidate above LOM_NAV_MAX is dropped: weights
 *     are positive, so exactly the cells whose true value exceeds LOM_NAV_MAX read LOM_NAV_UNREACHED, and so does every
 *     cell behind them.  range_exceeded = 1 iff, at the fixed point, some reached cell b and some allowed step a -> b
 *     have P[b] + len * c[a] > LOM_NAV_MAX (computed in the summary pass, so it is deterministic).  Impassable cells read
 *     LOM_NAV_UNREACHED.
 *  5. Summary, counted over the grid: cells_blocked (impassable), cells_reached, cells_unreached (passable, not reached)
 *     -- the three add up to the grid's cells -- cells_invalid, goals_used, goals_rejected, range_exceeded and
 *     max_potential (0 if nothing is reached).
 *  6. Paths.  K starts, as cells or metres.  A start outside the grid or on an unreached cell is not walked: length 0.
 *     Otherwise, from cell a with P[a] > 0, the walk steps to the first b in the fixed order E, N, W, S, NE, NW, SW, SE
 *     (+x is E, +y is N) for which the step is allowed and P[b] + len(a, b) * c[a] == P[a] -- one exists at the fixed
 *     point -- and stops at P == 0.  Output: u16 (ix, iy) pairs in a [K, cap] buffer; the length counts start and goal and
 *     is the full length even when it exceeds cap, only the first cap cells are written; the rest of a row is 0.  P falls
 *     strictly along a path, so a walk is bounded by the number of cells.
 *  7. Query.  n points in metres: the cell's P; LOM_NAV_UNREACHED for a point outside the grid or not a number.
 *  8. Line of sight.  Cells A = (x0, y0) and B = (x1, y1), under c[] of step 1 with the parameters of the last solve, and
 *     a threshold max_cell_cost.  A cell is clear iff c != 0 and (max_cell_cost == 0 or c <= max_cell_cost).  With dx =
 *     x1 - x0, dy = y1 - y0, ax = |dx|, ay = |dy|, sx and sy their signs, and i, j the steps taken so far along x and y:
 *     while (i, j) != (ax, ay), compare (2 i + 1) * ay with (2 j + 1) * ax (both below 2^27).  Less: x steps.  Greater: y
 *     steps.  Equal: the segment passes through a lattice corner; both step at once, and B is not visible unless both side
 *     cells (x + sx, y) and (x, y + sy) are clear -- the no-corner-cut rule of step 2.  Every cell stepped to, B included,
 *     must be clear; the first one that is not ends the walk: not visible.  A itself is tested for nothing.  A == B is
 *     visible.  A pair with either cell outside the grid is not visible.  The walk reaches B after ax + ay - (corners)
 *     steps and reads the cells whose interior the open segment meets (tests/navfield_waypoints_ref.py restates that
 *     on exact fractions).  lom_navfield_visible answers it for n pairs; after create or clear every cell is impassable,
 *     so only A == B is visible.
 *  9. Waypoints.  K starts, as in step 6, and lom_navfield_waypoint_params: max_cell_cost (0: any passable cell; neutral:
 *     cells of cost byte 0 only), lookahead W in 1 .. 65535, route_cap >= 1 with K * route_cap <= 2^28, flags == 0;
 *     anything else is LOM_ERR_ARG.  The route r[0 .. n - 1] of a start is the first n = min(length, route_cap) cells of
 *     its step-6 path.  The anchor is a = 0 and r[0] is emitted; while a < n - 1 the next anchor is the greatest j in
 *     (a, min(a + W, n - 1)] with r[j] visible from r[a] by step 8, a + 1 if none is, and r[next] is emitted.  Output: u16
 *     (ix, iy) pairs in a [K, wp_cap] buffer, the rest of a row 0; counts[k], the full number of waypoints even above
 *     wp_cap, 0 for a start that is not walked and 1 for a start on a goal; lengths[k], the full step-6 length, so a
 *     route cut at route_cap shows.  The waypoints are a subsequence of the route with its first and last cell; W = 1
 *     gives the route itself; every consecutive pair more than one route cell apart is visible.
 * After create or lom_navfield_clear every cell is unreached, every cell impassable.
 *
 * The result is a pure function of plane, parameters and goals: it does not depend on the tile shape, on the number of
 * launches, on the order in which workgroups run or on the test switches below.  The waypoints of step 9 are a pure
 * function of those, the starts and their three parameters.
 *
 * Re-solve.  A field that has completed a solve keeps its plane, its table and P.  lom_navfield_resolve* takes a new
 * full-grid int8 plane and an optional lom_clearance_window, with that struct's rules: the rectangle is clipped to the
 * grid, NULL is the whole grid, an empty rectangle is LOM_OK and changes nothing.
 *  a. Merged plane.  The kept plane with the cells of the clipped window replaced by the new plane's.  Cells outside the
 *     window are not read: the caller need not keep them equal, they do not count.
 *  b. Goals.  The cells with P == 0 before the call: the used goals of the last solve or re-solve.  No list is passed.  A
 *     goal whose cell is impassable in the merged plane counts in goals_rejected and is gone for later re-solves;
 *     goals_used + goals_rejected equals the previous goals_used.
 *  c. Result.  P and the summary are, byte for byte, what lom_navfield_solve gives on the merged plane with the last
 *     solve's parameters and those goals.  The kept plane becomes the merged plane; paths and queries read the new state;
 *     lom_navfield_potential_device's pointer stays valid across the call.
 *  d. Refusals.  Before the first successful solve since create or clear: LOM_ERR_STATE.  A NULL plane, or a clearance
 *     grid of other geometry or on another device: LOM_ERR_ARG.  A refused call changes nothing and zeroes the summary.
 * The work is incremental and still exact, because the field is the unique fixed point of a relaxation on positive
 * weights.  A diff over the window finds the changed cells (cells_changed: the bytes that differ from the kept ones) and
 * sets those that are now impassable to unreached; none changed ends the call there.  The raise phase then sets every
 * reached cell unreached that no chain of supporters carries down to a goal under the merged plane -- a supporter of a
 * is a cell b with an allowed step a -> b and P[b] + len * c[a] <= P[a]; cells_raised counts them, the least such set,
 * which does not depend on the schedule -- and the relaxation of a solve lowers what is left, every value an upper bound,
 * to the field.  LOM_NAV_OPT_TEST_RESOLVE_FORM chooses another way to the same bytes: 1, the threshold form, sets every
 * reached cell with P > 0 and P >= pmin unreached instead, pmin the least positive P among the changed cells and their
 * eight neighbours; 2 keeps only the goals and relaxes from them, the full solve on the same handle.  cells_raised is what
 * the chosen form set unreached behind the diff.
 *
 * Shift and re-solve.  lom_navfield_shift (grid shift, below) moves the geometry and clears the field.
 * lom_navfield_shift_resolve* moves the geometry, keeps what still overlaps and re-solves the rest in one call, for a
 * field that follows a robot.  It takes (dx, dy), a new full-grid int8 plane and an optional window, as a re-solve does.
 *  1. Geometry.  The new geometry is lom_grid_shift_geometry(geometry, dx, dy), that rule and nothing else.  The window and
 *     every plane are in the new geometry's cells.
 *  2. Moved state.  Cell (ix, iy) takes the kept plane's byte and P of cell (ix + dx, iy + dy) where that lies in the
 *     grid: the kept box, cells_kept cells.  Every other cell has entered: no kept byte, P unreached; cells_entered.
 *  3. Merged plane.  Entered cells take the new plane's byte, window or not.  Kept cells inside the clipped window take
 *     the new plane's byte.  Every other kept cell keeps its own byte and is not read from the new plane.  NULL window:
 *     the whole grid.  An empty window is allowed: the entered cells still take their bytes.  The host form reads the
 *     entered cells and the window; where the shift is not zero it uploads every row from the first to the last that
 *     holds such a cell, whole.
 *  4. Goals.  The cells with P == 0 in the moved state.  A goal whose source left the grid counts in goals_left; one that
 *     is impassable in the merged plane counts in goals_rejected.  The previous goals_used equals goals_used +
 *     goals_rejected + goals_left.
 *  5. Result.  P and the summary are, byte for byte, what lom_navfield_solve gives on the merged plane in the new
 *     geometry with the last solve's parameters and those goals.  Paths, waypoints, visibility and queries read the new
 *     state.  A shift that keeps nothing (|dx| >= width or |dy| >= height) leaves the full solve of the new plane with no
 *     goals, every cell unreached, and is LOM_OK.
 *  6. (0, 0).  The call is lom_navfield_resolve* with the same arguments: same bytes, same summary, same
 *     lom_navfield_resolve_stats; cells_kept is width * height.
 *  7. Counters of the last call, through lom_navfield_resolve_stats.  cells_changed: the kept cells of the clipped window
 *     whose byte differs from the kept one; entered cells are not in it.  cells_raised, under the default form: the size
 *     of the least raised set of the moved state under the merged plane, behind the diff's drop of impassable cells.
 *     lom_navfield_shift_stats gives cells_kept, cells_entered and goals_left of the last call.
 *  8. Refusals.  A refused call changes nothing -- not P, plane, geometry, the solved state or the counters -- and zeroes
 *     the summary.  A NULL plane: LOM_ERR_ARG.  No solve has completed since create or clear (lom_navfield_shift is a
 *     clear): LOM_ERR_STATE.  The rule refuses the origin: LOM_ERR_RANGE.  A clearance grid whose geometry is not bit for
 *     bit the SHIFTED geometry (shift it first), or one on another device: LOM_ERR_ARG.  A failed allocation:
 *     LOM_ERR_OOM.  Every refusal comes before any device work.
 *  9. Storage.  The moved state goes into a second block, the u32 field and the int8 plane, 5 bytes per cell, allocated
 *     at the first call with a shift that is not zero and swapped with the first behind the launch: a field that never
 *     shifts pays nothing.  lom_navfield_potential_device's pointer is therefore valid until the next solve, clear or
 *     shift-resolve on the handle.
 * 10. LOM_NAV_OPT_TEST_RESOLVE_FORM.  0, the default: raise, then relax.  2: the moved goals reseeded and the full
 *     relaxation, the baseline on the same handle.  1, the threshold form: a shift that is not zero runs form 2 (its pmin
 *     would have to cover the trailing borders as well); (0, 0) is the threshold form of a re-solve.  The bytes are the
 *     same under all three.  INNER_CAP, BATCH and ALL_TILES act as in a re-solve.
 * The device work is one pass over the destination (k_nav_shift_diff: the mover and the diff, every byte of the second
 * block written once) and then what a re-solve runs.  The raise phase needs no new rule: a cell on a trailing border --
 * column 0 for dx > 0, column width - 1 for dx < 0, rows likewise -- whose supporter left the grid has no supporter and
 * rises, and what hung on it rises behind it; a goal that left is simply not there any more.
 *
 * lom_navfield_solve takes a host plane of width * height bytes; _solve_device a plane in HBM that is complete when
 * hip_event_or_null is (NULL: now); _solve_from_clearance takes lom_clearance_cost_device's plane and orders the two
 * streams by events in both directions -- a clearance grid whose resolution, origin, width or height differ bit for bit,
 * or that lives on another device, is LOM_ERR_ARG before any launch.  The field keeps a copy of the plane, so paths and
 * queries do not depend on what becomes of the caller's.  Every argument is validated before any device work; a refused
 * call changes nothing and zeroes the summary.  Every call returns with its work done.  Calls on one field are the
 * caller's to serialise.  The error text is the field's (lom_navfield_last_error). */
typedef struct lom_navfield lom_navfield;
typedef struct {
    uint32_t neutral;      /* the cost of a cell whose byte is 0, >= 1 */
    uint32_t factor;       /* ... and what a unit of the byte adds */
    uint32_t unknown_cost; /* the cost of a -1 cell under LOM_NAV_UNKNOWN_PASSABLE */
    int8_t max_passable;   /* the largest passable byte, 0 .. 98 */
    uint32_t flags;        /* LOM_NAV_* */
} lom_navfield_params;
typedef struct {
    uint64_t cells_blocked, cells_reached, cells_unreached, cells_invalid, goals_used, goals_rejected, range_exceeded,
        max_potential;
} lom_navfield_summary;
typedef struct {
    uint64_t launches, waits; /* of k_nav_relax in the last solve, and the host's waits for them */
    uint64_t tiles;           /* workgroups per launch */
} lom_navfield_solve_stats;
typedef struct {
    uint64_t cells_changed;  /* cells of the clipped window whose byte differs from the kept one */
    uint64_t cells_raised;   /* reached cells that the raise phase (or the reset of another form) set unreached */
    uint64_t raise_launches, relax_launches; /* of k_nav_raise and k_nav_relax */
    uint64_t waits;          /* the host's waits of the call, the diff's and the summary's included */
    uint64_t tiles_marked;   /* tiles active in the first launch of the relaxation */
} lom_navfield_resolve_counters; /* what lom_navfield_resolve_stats gives */
typedef struct {
    uint64_t cells_kept;    /* destination cells whose source lies in the grid */
    uint64_t cells_entered; /* the others: width * height - cells_kept */
    uint64_t goals_left;    /* goals whose cell left the grid */
} lom_navfield_shift_counters; /* what lom_navfield_shift_stats gives */
typedef struct {
    uint32_t max_cell_cost; /* a cell is clear up to this cell cost; 0: any passable cell */
    uint32_t lookahead;     /* W: route cells a shortcut may skip to, 1 .. 65535 */
    uint32_t route_cap;     /* cells of a route that are read, >= 1; n_starts * route_cap <= 2^28 */
    uint32_t flags;         /* 0 */
} lom_navfield_waypoint_params;
#define LOM_NAV_UNREACHED 0xFFFFFFFFu
#define LOM_NAV_MAX 0xFFFFFFFEu
enum { LOM_NAV_UNKNOWN_PASSABLE = 1 }; /* a -1 cell is passable at unknown_cost */
enum { LOM_NAV_CELLS = 0, LOM_NAV_METRES = 1 }; /* what goals and starts are: int32 (ix, iy) pairs, f32 (x, y) pairs */
enum {
    LOM_NAV_OPT_TEST_INNER_CAP = 1, /* sweeps of a tile per launch, 1 .. 2^20; 1: a launch is one sweep per active tile; <= 0: the default */
    LOM_NAV_OPT_TEST_BATCH = 2,     /* launches per wait, 1 .. 256; <= 0: the default */
    LOM_NAV_OPT_TEST_ALL_TILES = 3, /* 1: every tile is active in every launch; 0 or < 0, the default: only marked tiles */
    LOM_NAV_OPT_TEST_RESOLVE_FORM = 4, /* of a re-solve: 0 or < 0, the default: raise, then relax; 1: the threshold form; 2: the
                                          full solve from the kept goals.  Test switches: the bytes are the same.  The first
                                          three act on both phases of a re-solve. */
    LOM_NAV_OPT_TEST_SHORTCUT_SERIAL = 5 /* of step 9: 0 or < 0, the default: a wave per route, 64 candidates at a time; 1: a
                                            lane per route, one candidate after another.  The bytes are the same. */
};
int lom_navfield_create(const lom_occupancy_geometry *geometry, int device, lom_navfield **out);
void lom_navfield_destroy(lom_navfield *f);
const char *lom_navfield_last_error(const lom_navfield *f); /* f == NULL: why the last create on this thread failed */
int lom_navfield_clear(lom_navfield *f);                    /* every cell unreached and impassable */
int lom_navfield_get_geometry(const lom_navfield *f, lom_occupancy_geometry *out);
void *lom_navfield_stream(lom_navfield *f); /* hipStream_t */
int lom_navfield_device(const lom_navfield *f);
int lom_navfield_wait_event(lom_navfield *f, void *hip_event);
int lom_navfield_set_option(lom_navfield *f, int option, int64_t value);
/* goals: n_goals pairs of goal_kind in host memory (may be NULL with n_goals 0), at most 2^24 */
int lom_navfield_solve(lom_navfield *f, const int8_t *plane, const lom_navfield_params *params, int goal_kind, const void *goals,
                       size_t n_goals, lom_navfield_summary *summary_or_null);
int lom_navfield_solve_device(lom_navfield *f, const int8_t *d_plane, void *hip_event_or_null, const lom_navfield_params *params,
                              int goal_kind, const void *goals, size_t n_goals, lom_navfield_summary *summary_or_null);
int lom_navfield_solve_from_clearance(lom_navfield *f, lom_clearance *clearance, const lom_navfield_params *params, int goal_kind,
                                      const void *goals, size_t n_goals, lom_navfield_summary *summary_or_null);
/* the re-solve: a host plane of width * height bytes, of which the window's rows are read; a plane in HBM that is complete
 * when hip_event_or_null is; lom_clearance_cost_device's plane behind a (windowed) lom_clearance_update*, with the hand-off
 * of _solve_from_clearance */
int lom_navfield_resolve(lom_navfield *f, const int8_t *plane, const lom_clearance_window *window_or_null,
                         lom_navfield_summary *summary_or_null);
int lom_navfield_resolve_device(lom_navfield *f, const int8_t *d_plane, void *hip_event_or_null,
                                const lom_clearance_window *window_or_null, lom_navfield_summary *summary_or_null);
int lom_navfield_resolve_from_clearance(lom_navfield *f, lom_clearance *clearance, const lom_clearance_window *window_or_null,
                                        lom_navfield_summary *summary_or_null);
/* the shift with a re-solve, in the three forms of a re-solve; the planes and the window are in the cells of the geometry
 * moved by (dx, dy), and a clearance grid has been shifted by the same (dx, dy) before */
int lom_navfield_shift_resolve(lom_navfield *f, int32_t dx, int32_t dy, const int8_t *plane, const lom_clearance_window *window_or_null,
                               lom_navfield_summary *summary_or_null);
int lom_navfield_shift_resolve_device(lom_navfield *f, int32_t dx, int32_t dy, const int8_t *d_plane, void *hip_event_or_null,
                                      const lom_clearance_window *window_or_null, lom_navfield_summary *summary_or_null);
int lom_navfield_shift_resolve_from_clearance(lom_navfield *f, int32_t dx, int32_t dy, lom_clearance *clearance,
                                              const lom_clearance_window *window_or_null, lom_navfield_summary *summary_or_null);
/* P over the whole grid, row-major: at most `cap` cells go to `out` (may be NULL with cap 0) */
int lom_navfield_potential(lom_navfield *f, uint32_t *out, size_t cap);
/* the same, left in HBM: width * height cells, valid until the next solve, clear or shift-resolve on the handle */
int lom_navfield_potential_device(lom_navfield *f, const uint32_t **d_out);
/* step 6: n_starts pairs of start_kind in host memory (at most 2^24, n_starts * cap at most 2^28); cells_out: [n_starts,
 * cap] u16 pairs (may be NULL with cap 0), lengths_out: n_starts u32 (may be NULL) */
int lom_navfield_paths(lom_navfield *f, int start_kind, const void *starts, size_t n_starts, uint16_t *cells_out, size_t cap,
                       uint32_t *lengths_out);
/* step 7: n points (x, y in the grid's frame, f32 pairs in host memory, at most 2^30) */
int lom_navfield_query(lom_navfield *f, const float *xy, size_t n, uint32_t *out);
/* step 8: n int32 quadruples (x0, y0, x1, y1) in host memory, at most 2^24; out: a byte per pair, 1 = visible */
int lom_navfield_visible(lom_navfield *f, const int32_t *pairs, size_t n, uint32_t max_cell_cost, uint8_t *out);
/* step 9: starts as for lom_navfield_paths; cells_out: [n_starts, wp_cap] u16 pairs (may be NULL with wp_cap 0; n_starts *
 * wp_cap at most 2^28), counts_out and lengths_out: n_starts u32 each (either may be NULL).  The routes stay in HBM: one
 * trace, one shortcut pass, one wait.  A refused call writes nothing. */
int lom_navfield_waypoints(lom_navfield *f, int start_kind, const void *starts, size_t n_starts,
                           const lom_navfield_waypoint_params *params, uint16_t *cells_out, size_t wp_cap, uint32_t *counts_out,
                           uint32_t *lengths_out);
/* step 1 for these parameters; LOM_ERR_ARG for bad parameters.  Needs no handle and no device. */
int lom_navfield_cell_costs(const lom_navfield_params *params, uint32_t *out256);
/* the launches and waits of the last solve (zeros before the first) */
int lom_navfield_stats(const lom_navfield *f, lom_navfield_solve_stats *out);
/* the counts of the last re-solve (zeros before the first, and for an empty window) */
int lom_navfield_resolve_stats(const lom_navfield *f, lom_navfield_resolve_counters *out);
/* the counts of the last shift with a re-solve (zeros before the first) */
int lom_navfield_shift_stats(const lom_navfield *f, lom_navfield_shift_counters *out);

/* ---- navigation field set: N fields over one cost plane in one call (not in the reference) -----------------------------
 * A navigation field holds one field, and its solve is a chain of dependent launches along the wavefront.  Ordering a tour
 * over frontier goals needs goal-to-goal travel costs, sharing goals among robots needs a field per robot, and cutting the
 * free space into "nearest goal" cells needs all the fields at once.  This handle family solves N fields over the same
 * plane and parameters side by side: every launch of the relaxation covers every field, so the launches and waits of a
 * call are near those of its slowest field, not their sum.  Nothing is launched unless a caller creates a set.
 *
 * Grid.  lom_occupancy_geometry with the planning grids' rule, as a navigation field.  lom_navset_create takes max_fields
 * in 1 .. LOM_NAVSET_MAX_FIELDS (65535); anything else is LOM_ERR_ARG.  Storage: 4 bytes per cell and field for max_fields
 * fields, one copy of the plane (a byte per cell), and the marks (8 bytes per 32 x 32 tile and field).  A failed allocation
 * is LOM_ERR_OOM and leaves no handle.
 *
 * Solve.  lom_navset_solve* takes one plane, one lom_navfield_params, one goal array of LOM_NAV_CELLS or LOM_NAV_METRES
 * pairs and n_fields + 1 offsets into it: field i takes the goals [goal_offsets[i], goal_offsets[i + 1]).
 *  1. Result.  Field i and summaries[i] are, byte for byte, what lom_navfield_solve gives for the same plane, parameters
 *     and those goals: P, cells_blocked, cells_reached, cells_unreached, cells_invalid, goals_used (duplicates within a
 *     field once), goals_rejected, range_exceeded and max_potential.  A field may have no goals (every cell unreached);
 *     two fields may share goals, or have the same goals.  Each field is the unique fixed point of the navigation field's
 *     relaxation and the fields share nothing but the read-only plane and table, so the bytes do not depend on the
 *     schedule, on the number of fields solved beside it or on the test switches below.
 *  2. Offsets.  n_fields is 0 .. max_fields.  The offsets start at 0, never fall, and end at n_goals <= 2^24; goals may be
 *     NULL only where n_goals is 0.  Otherwise LOM_ERR_ARG.  n_fields == 0 is LOM_OK, reads neither offsets nor goals,
 *     launches nothing and leaves a set of no fields.
 *  3. Refusals.  A NULL plane, bad parameters, an unknown goal kind, bad offsets, or (from a clearance grid) a geometry
 *     that is not bit for bit the set's or another device: LOM_ERR_ARG.  Every refusal comes before any device work,
 *     changes nothing -- the fields, lom_navset_field_count and the counters of the last solve stay -- and zeroes the
 *     first min(n_fields, max_fields) summaries.
 *  4. Forms.  lom_navset_solve takes a host plane of width * height bytes; _solve_device a plane in HBM that is complete
 *     when hip_event_or_null is (NULL: now); _solve_from_clearance takes lom_clearance_cost_device's plane and orders the
 *     two streams by events in both directions.  The set keeps a copy of the plane.
 * lom_navset_field_count gives the fields of the last solve, and 0 after create, lom_navset_clear or lom_navset_shift.  A
 * solve with fewer fields than the one before leaves the fewer.  lom_navset_shift is the planning grids' shift: the geometry
 * moves by the rule and the set becomes what a fresh, cleared set of the shifted geometry is.
 *
 * Fields.  Planar, [n_fields][height][width] u32 in lom_navfield_potential's form.  lom_navset_potential copies field i
 * out; lom_navset_potential_device gives its place in HBM, valid until the next solve, clear or shift on the set.  An
 * index outside 0 .. field_count - 1 is LOM_ERR_ARG.
 *
 * Gather.  n points, as cells or metres: out[i * n + j] is P of field i at point j, LOM_NAV_UNREACHED for a point outside
 * the grid or not a number.  n <= 2^24 and field_count * n <= 2^28.  With the goals as the points this is the travel-cost
 * matrix: out[i * n + j] is what it costs to go from goal j to the nearest goal of field i.  A step pays for the cell it
 * leaves (navigation field, step 2), so the cost from a to b counts c[a] and not c[b], and the cost from b to a counts
 * c[b] and not c[a]: the matrix is NOT symmetric unless the two end cells cost the same.
 *
 * Nearest.  Per cell, the least P over the fields and the least field index that attains it: owner_out (u16 per cell,
 * LOM_NAVSET_NO_OWNER = 0xFFFF where no field reaches the cell), potential_out (u32 per cell, LOM_NAV_UNREACHED there)
 * and cells_owned (u64 per field: the cells it owns); each may be NULL.  Invariant: potential_out is, byte for byte, P of
 * the single lom_navfield_solve from the union of all fields' goals.  Before the first solve since create, clear or shift:
 * LOM_ERR_STATE.  A set of no fields owns nothing: every owner is LOM_NAVSET_NO_OWNER.
 *
 * Paths.  lom_navfield_paths' walk (step 6) for n starts, start k on field field_of_start[k].  An index outside
 * 0 .. field_count - 1 is LOM_ERR_ARG before any device work, and nothing is written.
 *
 * Adopt.  lom_navfield_adopt(f, s, i, summary_or_null), of the navigation field's own family, makes the navigation field f
 * exactly what lom_navfield_solve of the set's plane, parameters and field i's goals would have left: P, the kept plane,
 * the table, the solved state and the summary words.  Afterwards paths, waypoints, visible, query, resolve* and
 * shift_resolve* on f give the bytes they give after the direct solve, and so do the consumers that take a lom_navfield
 * (regions, visibility select, rollouts): the set needs no copy of them.  The copies stay in HBM and are ordered by the two
 * handles' events.  A geometry that is not bit for bit the set's, another device or i outside 0 .. field_count - 1:
 * LOM_ERR_ARG.  A set with no solve since create, clear or shift: LOM_ERR_STATE.  A refused call leaves f untouched and
 * zeroes the summary.  lom_navfield_stats reads 0 launches and 0 waits after an adopt.
 *
 * Not part of this: a re-solve or a shift-resolve of a whole set (adopt a field and use the field's), waypoints on the set.
 *
 * Every argument is validated before any device work.  Every call returns with its work done.  Calls on one set are the
 * caller's to serialise.  The error text is the set's (lom_navset_last_error). */
typedef struct lom_navset lom_navset;
typedef struct {
    uint64_t launches, waits; /* of k_navset_relax in the last solve, and the host's waits for them */
    uint64_t tiles;           /* workgroups per launch: tiles * fields */
    uint64_t fields;          /* fields of the last solve */
} lom_navset_solve_stats;
#define LOM_NAVSET_NO_OWNER 0xFFFFu
#define LOM_NAVSET_MAX_FIELDS 65535u
enum {
    LOM_NAVSET_OPT_TEST_INNER_CAP = 1, /* as LOM_NAV_OPT_TEST_INNER_CAP */
    LOM_NAVSET_OPT_TEST_BATCH = 2,     /* launches per wait, as LOM_NAV_OPT_TEST_BATCH */
    LOM_NAVSET_OPT_TEST_ALL_TILES = 3  /* every tile of every field in every launch.  Test switches: the bytes are the same. */
};
int lom_navset_create(const lom_occupancy_geometry *geometry, int device, size_t max_fields, lom_navset **out);
void lom_navset_destroy(lom_navset *s);
const char *lom_navset_last_error(const lom_navset *s); /* s == NULL: why the last create on this thread failed */
int lom_navset_clear(lom_navset *s);                    /* no fields */
/* the planning families' shift ("grid shift", below): the geometry moves by that rule, the state is lom_navset_clear's;
 * LOM_ERR_RANGE from the rule leaves the set untouched */
int lom_navset_shift(lom_navset *s, int32_t dx, int32_t dy);
int lom_navset_get_geometry(const lom_navset *s, lom_occupancy_geometry *out);
void *lom_navset_stream(lom_navset *s); /* hipStream_t */
int lom_navset_device(const lom_navset *s);
int lom_navset_wait_event(lom_navset *s, void *hip_event);
int lom_navset_set_option(lom_navset *s, int option, int64_t value);
size_t lom_navset_field_count(const lom_navset *s); /* s == NULL: 0 */
/* goals: goal_offsets[n_fields] pairs of goal_kind in host memory; goal_offsets: n_fields + 1 u32 in host memory;
 * summaries_or_null: n_fields of them */
int lom_navset_solve(lom_navset *s, const int8_t *plane, const lom_navfield_params *params, int goal_kind, const void *goals,
                     const uint32_t *goal_offsets, size_t n_fields, lom_navfield_summary *summaries_or_null);
int lom_navset_solve_device(lom_navset *s, const int8_t *d_plane, void *hip_event_or_null, const lom_navfield_params *params,
                            int goal_kind, const void *goals, const uint32_t *goal_offsets, size_t n_fields,
                            lom_navfield_summary *summaries_or_null);
int lom_navset_solve_from_clearance(lom_navset *s, lom_clearance *clearance, const lom_navfield_params *params, int goal_kind,
                                    const void *goals, const uint32_t *goal_offsets, size_t n_fields,
                                    lom_navfield_summary *summaries_or_null);
/* P of field i over the whole grid, row-major: at most `cap` cells go to `out` (may be NULL with cap 0) */
int lom_navset_potential(lom_navset *s, size_t i, uint32_t *out, size_t cap);
/* the same, left in HBM: width * height cells, valid until the next solve, clear or shift on the set */
int lom_navset_potential_device(lom_navset *s, size_t i, const uint32_t **d_out);
/* points: n pairs of point_kind in host memory; out: [field_count, n] u32 */
int lom_navset_gather(lom_navset *s, int point_kind, const void *points, size_t n, uint32_t *out);
/* owner_out: width * height u16; potential_out: width * height u32; cells_owned: field_count u64; each may be NULL */
int lom_navset_nearest(lom_navset *s, uint16_t *owner_out_or_null, uint32_t *potential_out_or_null, uint64_t *cells_owned_or_null);
/* field_of_start: n_starts int32 in host memory; the rest as lom_navfield_paths */
int lom_navset_paths(lom_navset *s, const int32_t *field_of_start, int start_kind, const void *starts, size_t n_starts,
                     uint16_t *cells_out, size_t cap, uint32_t *lengths_out);
/* the launches, waits, workgroups per launch and fields of the last solve (zeros before the first, and for no fields) */
int lom_navset_stats(const lom_navset *s, lom_navset_solve_stats *out);
/* field i of the set becomes the navigation field f ("Adopt", above) */
int lom_navfield_adopt(lom_navfield *f, lom_navset *s, size_t i, lom_navfield_summary *summary_or_null);

/* ---- frontier regions: connected cells labelled on the device, ranked goals (not in the reference) ----------------------
 * The navigation field answers what it costs to get somewhere.  This handle family answers where to go: it labels the
 * connected regions of a grid plane -- the frontier cells of an occupancy plane (FREE next to UNKNOWN, as an explorer
 * reads nav_msgs/OccupancyGrid), or any byte range: obstacle blobs, connected free space, unreached pockets -- gives
 * each region a record (size, box, centre, cheapest cell to reach) and leaves a ranked goal list in the form
 * lom_navfield_solve takes under LOM_NAV_CELLS.  Nothing is launched unless a caller creates a region grid.  The
 * definition, operation by operation (tests/regions_ref.py restates it with a flood fill on Python integers; everything
 * is an integer, so every comparison is exact):
 *
 * Grid.  lom_occupancy_geometry, reused, with the navigation field's rules: row-major with y as the row, the linear
 * index of cell (ix, iy) is iy * width + ix (below 2^26), the index rule is the floor rule.  r > 0 and finite, a finite
 * origin, 1 <= width, height <= 8192; anything else is LOM_ERR_ARG.
 *
 * Inputs of an extract.  `plane`: a full-grid int8 plane, what lom_occupancy_classify writes; any byte is accepted.
 * `cost`, optional: a full-grid int8 plane in lom_clearance_cost's range.  `potential`, optional: a full-grid u32 plane
 * in lom_navfield_potential's form.  lom_regions_params: kind LOM_REGIONS_BYTES or LOM_REGIONS_FRONTIER; lo <= hi under
 * LOM_REGIONS_BYTES (neither is read otherwise); 0 <= max_cost <= 99; min_cells >= 1; a known rank, and
 * LOM_REGIONS_RANK_POTENTIAL only with a potential; no unknown bit in flags; anything else is LOM_ERR_ARG.
 *  1. Membership.  LOM_REGIONS_BYTES: a cell is a member iff lo <= plane <= hi.  LOM_REGIONS_FRONTIER: iff plane == 0 and
 *     at least one neighbour has plane == -1; the neighbours are the four edge neighbours, all eight under
 *     LOM_REGIONS_NEIGHBOURS_8; a neighbour outside the grid is not unknown unless LOM_REGIONS_EDGE_UNKNOWN is set.  In
 *     both kinds a member also needs 0 <= cost <= max_cost where a cost plane is given, and P != LOM_NAV_UNREACHED where
 *     a potential is given.
 *  2. Regions.  The 8-connected components of the members; the 4-connected ones under LOM_REGIONS_CONNECT_4.  The label
 *     of a member is the least linear index in its component; every other cell reads LOM_REGIONS_NONE.  Labels are a u32
 *     plane.
 *  3. Dense order.  Regions are numbered 0, 1, ... by ascending label.  Only the first max_regions of them
 *     (LOM_REGIONS_OPT_MAX_REGIONS, default 2^20) get a record; the summary counts all of them and the recorded ones.
 *  4. Record.  lom_regions_record, 48 bytes, per recorded region: label; cells; sum_x, sum_y (the sums of ix and of iy);
 *     the box min_x, min_y, max_x, max_y; the centroid cell cx = floor((2 sum_x + cells) / (2 cells)), cy likewise; the
 *     centre cell, the member that minimises (ix - cx)^2 + (iy - cy)^2, ties to the least linear index; the entry cell,
 *     the member with the least P, ties to the least linear index, and entry_potential, that P.  Without a potential the
 *     entry cell is the centre cell and entry_potential is LOM_NAV_UNREACHED.  Both minima are one unsigned 64-bit
 *     minimum of (key << 26) | linear index: d^2 is below 2^27, P below 2^32.
 *  5. List.  The recorded regions with cells >= min_cells, sorted by rank, ties by ascending label:
 *     LOM_REGIONS_RANK_LABEL; LOM_REGIONS_RANK_CELLS, largest first; LOM_REGIONS_RANK_POTENTIAL, least entry_potential
 *     first.  The list holds at most max_regions records and is sorted on the host.
 *  6. Goals.  The centre cells (LOM_REGIONS_GOAL_CENTRE) or the entry cells (LOM_REGIONS_GOAL_ENTRY) of the list, in list
 *     order, as int32 (ix, iy) pairs.
 *  7. Query.  n points in metres: the label of the cell; LOM_REGIONS_NONE for a point outside the grid or not a number.
 *  8. Summary.  cells_member, regions, regions_recorded, regions_listed, largest_cells (the largest count among recorded
 *     regions, 0 if none).
 * After create or lom_regions_clear there is no member, no region and an empty list.
 *
 * The result is a pure function of the planes and the parameters: it does not depend on the tile shape, on the number of
 * launches, on the order in which workgroups run or on the test switches below.
 *
 * lom_regions_extract takes host planes; _extract_device planes in HBM that are complete when hip_event_or_null is
 * (NULL: now); _extract_from_grids reads lom_occupancy_classify_device, lom_clearance_cost_device (or no cost plane) and
 * lom_navfield_potential_device (or no potential) and orders the streams by events in both directions -- a grid whose
 * resolution, origin, width or height differ bit for bit, or that lives on another device, is LOM_ERR_ARG before any
 * launch.  Every argument is validated before any device work; a refused call changes nothing and zeroes the summary.
 * Every call returns with its work done.  Calls on one handle are the caller's to serialise.  The error text is the
 * handle's (lom_regions_last_error). */
typedef struct lom_regions lom_regions;
typedef struct {
    int32_t kind;       /* LOM_REGIONS_BYTES, LOM_REGIONS_FRONTIER */
    int8_t lo, hi;      /* the byte range of LOM_REGIONS_BYTES */
    int8_t max_cost;    /* the largest cost byte of a member where a cost plane is given, 0 .. 99 */
    uint32_t min_cells; /* the smallest listed region, >= 1 */
    int32_t rank;       /* LOM_REGIONS_RANK_* */
    uint32_t flags;     /* LOM_REGIONS_NEIGHBOURS_8 | LOM_REGIONS_EDGE_UNKNOWN | LOM_REGIONS_CONNECT_4 */
} lom_regions_params;
typedef struct {
    uint32_t label;                       /* offset 0: the least linear index of the region */
    uint32_t cells;                       /* 4 */
    uint64_t sum_x, sum_y;                /* 8, 16 */
    uint16_t min_x, min_y, max_x, max_y;  /* 24 .. 31 */
    uint16_t centroid_x, centroid_y;      /* 32, 34 */
    uint16_t centre_x, centre_y;          /* 36, 38 */
    uint16_t entry_x, entry_y;            /* 40, 42 */
    uint32_t entry_potential;             /* 44 */
} lom_regions_record;
typedef struct {
    uint64_t cells_member, regions, regions_recorded, regions_listed, largest_cells;
} lom_regions_summary;
typedef struct {
    uint64_t launches, waits; /* kernel launches of the last extract, and the host's waits for them */
    uint64_t tiles;           /* workgroups of k_reg_label_tile (0 under LOM_REGIONS_OPT_TEST_NO_TILES) */
} lom_regions_extract_stats;
#define LOM_REGIONS_NONE 0xFFFFFFFFu
enum { LOM_REGIONS_BYTES = 0, LOM_REGIONS_FRONTIER = 1 };
enum { LOM_REGIONS_NEIGHBOURS_8 = 1, LOM_REGIONS_EDGE_UNKNOWN = 2, LOM_REGIONS_CONNECT_4 = 4 };
enum { LOM_REGIONS_RANK_LABEL = 0, LOM_REGIONS_RANK_CELLS = 1, LOM_REGIONS_RANK_POTENTIAL = 2 };
enum { LOM_REGIONS_GOAL_CENTRE = 0, LOM_REGIONS_GOAL_ENTRY = 1 };
enum {
    LOM_REGIONS_OPT_MAX_REGIONS = 1,        /* records kept, 1 .. 2^26; <= 0: the default, 2^20 */
    LOM_REGIONS_OPT_TEST_TILE_ROWS = 2,     /* rows of a tile of k_reg_label_tile: 1, 8 or 32; <= 0: the default */
    LOM_REGIONS_OPT_TEST_NO_TILES = 3,      /* 1: no tile pass, every adjacency goes through k_reg_merge; 0 or < 0: the default */
    LOM_REGIONS_OPT_TEST_NO_WAVE_MERGE = 4  /* 1: every member lane issues its own atomics; 0 or < 0: the default.
                                               Test switches: the bytes are the same. */
};
int lom_regions_create(const lom_occupancy_geometry *geometry, int device, lom_regions **out);
void lom_regions_destroy(lom_regions *r);
const char *lom_regions_last_error(const lom_regions *r); /* r == NULL: why the last create on this thread failed */
int lom_regions_clear(lom_regions *r);                    /* no member, no region, an empty list */
int lom_regions_get_geometry(const lom_regions *r, lom_occupancy_geometry *out);
void *lom_regions_stream(lom_regions *r); /* hipStream_t */
int lom_regions_device(const lom_regions *r);
int lom_regions_wait_event(lom_regions *r, void *hip_event);
int lom_regions_set_option(lom_regions *r, int option, int64_t value);
/* plane: width * height int8; cost_or_null: the same; potential_or_null: width * height u32 */
int lom_regions_extract(lom_regions *r, const int8_t *plane, const int8_t *cost_or_null, const uint32_t *potential_or_null,
                        const lom_regions_params *params, lom_regions_summary *summary_or_null);
int lom_regions_extract_device(lom_regions *r, const int8_t *d_plane, const int8_t *d_cost_or_null,
                               const uint32_t *d_potential_or_null, void *hip_event_or_null, const lom_regions_params *params,
                               lom_regions_summary *summary_or_null);
int lom_regions_extract_from_grids(lom_regions *r, lom_occupancy *occupancy, const lom_occupancy_rule *rule,
                                   lom_clearance *clearance_or_null, lom_navfield *navfield_or_null,
                                   const lom_regions_params *params, lom_regions_summary *summary_or_null);
/* the labels over the whole grid, row-major: at most `cap` cells go to `out` (may be NULL with cap 0) */
int lom_regions_labels(lom_regions *r, uint32_t *out, size_t cap);
/* the same, left in HBM: width * height cells, valid until the next extract or clear on the handle */
int lom_regions_labels_device(lom_regions *r, const uint32_t **d_out);
/* step 5: at most `cap` records go to `out` (may be NULL with cap 0); *listed_or_null: the length of the list */
int lom_regions_list(lom_regions *r, lom_regions_record *out, size_t cap, size_t *listed_or_null);
/* step 6: at most `cap` int32 (ix, iy) pairs go to `out`; which: LOM_REGIONS_GOAL_CENTRE or LOM_REGIONS_GOAL_ENTRY */
int lom_regions_goals(lom_regions *r, int which, int32_t *out, size_t cap, size_t *listed_or_null);
/* step 7: n points (x, y in the grid's frame, f32 pairs in host memory, at most 2^30) */
int lom_regions_query(lom_regions *r, const float *xy, size_t n, uint32_t *out);
/* the launches and waits of the last extract (zeros before the first) */
int lom_regions_stats(const lom_regions *r, lom_regions_extract_stats *out);

/* ---- visibility grid: rays cast from candidate viewpoints, goals picked by what they would see (not in the reference) ----
 * The region grid ranks frontiers by label, size or travel cost; none of these says what a robot would see from a goal.
 * This handle family casts B beams over a grid plane from each of K viewpoints at once and counts, per viewpoint, the
 * distinct cells the beams see, by class -- the unknown ones are the expected gain of driving there -- keeps, on request,
 * a simulated planar scan per viewpoint (end distance and end reason per beam) and the set of unknown cells each viewpoint
 * sees, and selects next-best views from those sets greedily, gain against travel cost.  Nothing is launched unless a
 * caller creates a visibility grid.  The definition, operation by operation (tests/visibility_ref.py restates it on
 * Python integers; everything is an integer, so every comparison is exact):
 *
 * Grid.  lom_occupancy_geometry, reused, with the region grid's rules: row-major with y as the row.  r > 0 and finite, a
 * finite origin, 1 <= width, height <= 8192; anything else is LOM_ERR_ARG.
 *
 * Plane.  A full-grid int8 plane; a cell with v < 0 is unknown, with 0 <= v < block_min free, with v >= block_min
 * blocking.  lom_occupancy_classify's plane works with block_min = 100, lom_clearance_cost's with block_min = 99.
 * lom_visibility_params: 4 <= beams <= 8192 (B); range_cells <= 254 (R); 1 <= block_min <= 100; unknown_depth <= 65535
 * (D; 0: no limit); flags of LOM_VIS_KEEP_WINDOWS | LOM_VIS_KEEP_BEAMS only; anything else is LOM_ERR_ARG.
 *  1. Direction table.  Beam b has the direction (dx, dy) = (lround(cos(2 pi b / B) * 32768), lround(sin(2 pi b / B) *
 *     32768)), computed on the host in f64; lom_visibility_table gives the int32 pairs.
 *  2. Walk.  From the centre of the start cell (x0, y0).  ax = |dx|, ay = |dy|, sx, sy the signs (a zero component never
 *     steps), i, j the steps taken so far along x and y.  The next crossing: (2 i + 1) * ay against (2 j + 1) * ax, both
 *     below 2^24.  Less: x steps.  Greater: y steps.  Equal: the ray passes exactly through a corner and both step at
 *     once; the ray then ends at the current cell with reason LOM_VIS_END_CORNER when both side cells (x + sx, y) and
 *     (x, y + sy) are blocking (a side cell outside the grid does not block); side cells are never marked seen.
 *  3. At the cell stepped to, with step counts (ni, nj), in this order: outside the grid: end LOM_VIS_END_EDGE at the
 *     previous cell; ni^2 + nj^2 > R^2: end LOM_VIS_END_RANGE at the previous cell; the cell is marked seen; v >=
 *     block_min: end LOM_VIS_END_HIT at this cell; v < 0: it counts for this ray, and when D > 0 and the count reaches D
 *     the ray ends LOM_VIS_END_UNKNOWN at this cell.  The start cell is marked seen once, is tested for nothing and counts
 *     for no ray's D.
 *  4. Viewpoints.  K int32 (ix, iy) pairs, in the form lom_regions_goals returns, 0 <= K <= 2^20.  A viewpoint outside
 *     the grid or on a blocking cell is invalid: valid = 0, every count 0, every beam 0 (d2 = 0, LOM_VIS_END_INVALID), an
 *     empty window.  Duplicates are cast independently.
 *  5. Record.  lom_visibility_record, 32 bytes, per viewpoint: ix, iy; valid; seen, the distinct cells marked; unknown,
 *     free, blocked, those cells by class (they sum to seen); hits, the beams that ended LOM_VIS_END_HIT.
 *  6. Beams (LOM_VIS_KEEP_BEAMS).  One u32 per viewpoint and beam: d2 = i^2 + j^2 of the end cell in the low 24 bits, the
 *     reason in the high 8.
 *  7. Summary.  viewpoints; valid; unknown_total, the sum of unknown over the valid ones; unknown_max, the greatest
 *     unknown among them, and unknown_argmax, the least index that has it (both 0 when none is valid).
 *  8. Windows (LOM_VIS_KEEP_WINDOWS).  W_k, the unknown cells viewpoint k sees, as a bitmap of 2R + 1 rows of
 *     ceil((2R + 1) / 32) u32 around the start cell: cell (ix, iy) is bit (ix - x0 + R) & 31 of word (ix - x0 + R) >> 5
 *     of row iy - y0 + R.  The window holds the whole disc; what lies outside the grid reads 0.
 *  9. Selection.  Needs the last cast to have kept its windows (LOM_ERR_STATE otherwise).  lom_visibility_select_params:
 *     1 <= n <= 1024; 1 <= gain_weight <= 4096; cost_shift <= 31; min_gain >= 1.  cost: K u32, optional (none: every cost
 *     is 0); a cost of LOM_NAV_UNREACHED excludes the viewpoint.  C, the covered set, is empty at the start of every
 *     select.  Each round: g_k = |W_k \ C| for every valid, not yet picked, not excluded k; s_k = g_k * gain_weight -
 *     (cost_k >> cost_shift) as int64; the winner is the greatest s_k among those with g_k >= min_gain, ties to the least
 *     k; without one the selection ends; else C |= W_winner.  Output: up to n lom_visibility_pick (k, gain, score) in the
 *     order picked, and their count.  -(2^32 - 1) <= s <= 2^30, so (s + 2^32) << 20 | (2^20 - 1 - k) orders the candidates
 *     as one unsigned 64-bit maximum.
 * After create or lom_visibility_clear there is no viewpoint: an empty summary, no records, no windows.
 *
 * The result is a pure function of the plane, the parameters and the viewpoints (and the costs): it does not depend on
 * the order in which beams, waves or workgroups run or on the test switches below.
 *
 * lom_visibility_cast takes a host plane of width * height bytes; _cast_device a plane in HBM that is complete when
 * hip_event_or_null is (NULL: now); _cast_from_occupancy takes lom_occupancy_classify_device's plane and orders the two
 * streams by events in both directions -- a grid whose resolution, origin, width or height differ bit for bit, or that
 * lives on another device, is LOM_ERR_ARG before any launch.  The handle keeps a copy of the plane.  The viewpoints are
 * host memory in every form.  _select takes host costs; _select_from_navfield reads them on the device from
 * lom_navfield_potential_device at the viewpoints' cells.  Every argument is validated and every allocation made before
 * the first launch; a refused call changes nothing and zeroes the summary (the count of a select).  A cast is one host
 * wait and a select is one host wait, whatever n.  Every call returns with its work done.  Calls on one handle are the
 * caller's to serialise.  The error text is the handle's (lom_visibility_last_error). */
typedef struct lom_visibility lom_visibility;
typedef struct {
    uint32_t beams;         /* B, 4 .. 8192 */
    uint32_t range_cells;   /* R, 0 .. 254 */
    int32_t block_min;      /* the least blocking value, 1 .. 100 */
    uint32_t unknown_depth; /* D, 0 .. 65535; 0: no limit */
    uint32_t flags;         /* LOM_VIS_KEEP_WINDOWS | LOM_VIS_KEEP_BEAMS */
} lom_visibility_params;
typedef struct {
    int32_t ix, iy;                       /* offset 0, 4 */
    uint32_t valid;                       /* 8 */
    uint32_t seen;                        /* 12 */
    uint32_t unknown, free, blocked;      /* 16, 20, 24 */
    uint32_t hits;                        /* 28 */
} lom_visibility_record;
typedef struct {
    uint64_t viewpoints, valid, unknown_total, unknown_max, unknown_argmax;
} lom_visibility_summary;
typedef struct {
    uint32_t n;           /* the most entries picked, 1 .. 1024 */
    uint32_t gain_weight; /* 1 .. 4096 */
    uint32_t cost_shift;  /* 0 .. 31 */
    uint32_t min_gain;    /* >= 1 */
} lom_visibility_select_params;
typedef struct {
    uint32_t k;    /* the viewpoint's index */
    uint32_t gain; /* g at the round it was picked */
    int64_t score; /* s at that round */
} lom_visibility_pick;
typedef struct {
    uint64_t launches, waits; /* kernel launches of the last cast or select, and the host's waits for them */
} lom_visibility_call_stats;
enum { LOM_VIS_KEEP_WINDOWS = 1, LOM_VIS_KEEP_BEAMS = 2 };
enum {
    LOM_VIS_END_INVALID = 0,
    LOM_VIS_END_EDGE = 1,
    LOM_VIS_END_RANGE = 2,
    LOM_VIS_END_HIT = 3,
    LOM_VIS_END_UNKNOWN = 4,
    LOM_VIS_END_CORNER = 5
};
enum {
    LOM_VIS_OPT_TEST_NO_LDS = 1,         /* 1: the seen bits go straight to the window in HBM; 0 or < 0: the default, LDS */
    LOM_VIS_OPT_TEST_WAVES = 2,          /* waves of a workgroup of k_vis_cast: 1 or 4; <= 0: the default.  Test switches:
                                            the bytes are the same. */
    LOM_VIS_OPT_MAX_WINDOW_BYTES = 3     /* a cast whose windows in HBM (under LOM_VIS_KEEP_WINDOWS, or under
                                            LOM_VIS_OPT_TEST_NO_LDS) would exceed this is LOM_ERR_ARG before any launch; <= 0:
                                            the default, 256 MiB */
};
int lom_visibility_create(const lom_occupancy_geometry *geometry, int device, lom_visibility **out);
void lom_visibility_destroy(lom_visibility *v);
const char *lom_visibility_last_error(const lom_visibility *v); /* v == NULL: why the last create on this thread failed */
int lom_visibility_clear(lom_visibility *v);                    /* no viewpoint, an empty summary */
int lom_visibility_get_geometry(const lom_visibility *v, lom_occupancy_geometry *out);
void *lom_visibility_stream(lom_visibility *v); /* hipStream_t */
int lom_visibility_device(const lom_visibility *v);
int lom_visibility_wait_event(lom_visibility *v, void *hip_event);
int lom_visibility_set_option(lom_visibility *v, int option, int64_t value);
/* step 1: 2 * beams int32 go to `out`; LOM_ERR_ARG for beams outside 4 .. 8192.  Needs no handle and no device. */
int lom_visibility_table(uint32_t beams, int32_t *out);
/* plane: width * height int8; viewpoints: k int32 (ix, iy) pairs in host memory (may be NULL with k 0) */
int lom_visibility_cast(lom_visibility *v, const int8_t *plane, const int32_t *viewpoints, size_t k,
                        const lom_visibility_params *params, lom_visibility_summary *summary_or_null);
int lom_visibility_cast_device(lom_visibility *v, const int8_t *d_plane, void *hip_event_or_null, const int32_t *viewpoints,
                               size_t k, const lom_visibility_params *params, lom_visibility_summary *summary_or_null);
int lom_visibility_cast_from_occupancy(lom_visibility *v, lom_occupancy *occupancy, const lom_occupancy_rule *rule,
                                       const int32_t *viewpoints, size_t k, const lom_visibility_params *params,
                                       lom_visibility_summary *summary_or_null);
/* step 5: at most `cap` records of the last cast go to `out` (may be NULL with cap 0); *count_or_null: K */
int lom_visibility_records(lom_visibility *v, lom_visibility_record *out, size_t cap, size_t *count_or_null);
/* step 6: at most `cap` u32 of the K * B of the last cast go to `out`, viewpoint by viewpoint; LOM_ERR_STATE when the last
 * cast did not keep them */
int lom_visibility_beams(lom_visibility *v, uint32_t *out, size_t cap);
/* step 8, left in HBM: K windows of *words_per_window_or_null u32 each, valid until the next cast or clear on the handle;
 * LOM_ERR_STATE when the last cast did not keep them */
int lom_visibility_windows_device(lom_visibility *v, const uint32_t **d_out, size_t *words_per_window_or_null);
/* the same, read back: at most `cap` u32 of the K windows go to `out` (may be NULL with cap 0), window by window */
int lom_visibility_windows(lom_visibility *v, uint32_t *out, size_t cap, size_t *words_per_window_or_null);
/* step 9: cost_or_null: K u32 in host memory; out: select->n entries; *picked: the entries written */
int lom_visibility_select(lom_visibility *v, const lom_visibility_select_params *select, const uint32_t *cost_or_null,
                          lom_visibility_pick *out, size_t *picked);
int lom_visibility_select_from_navfield(lom_visibility *v, lom_navfield *navfield, const lom_visibility_select_params *select,
                                        lom_visibility_pick *out, size_t *picked);
/* the launches and waits of the last cast or select (zeros before the first) */
int lom_visibility_stats(const lom_visibility *v, lom_visibility_call_stats *out);

/* ---- trajectory rollouts: velocity candidates scored on the cost plane (not in the reference) ------------------------
 * lom_navfield_paths walks cells as a point robot; nothing above tests a robot's footprint at a heading or compares many
 * candidate motions at once.  This handle family rolls K candidate command sequences out from each of M start states, tests
 * the footprint at every pose against a cost plane, and picks, per state, the candidate with the best score: progress on
 * a navigation potential against the cost gathered and the poses lost to a block.  One command per candidate is a dynamic
 * window, several are sampled control sequences.  Nothing is launched unless a caller creates a rollout grid.  The
 * definition, operation by operation (tests/rollout_ref.py restates it on Python integers; everything is an integer, so
 * every comparison is exact):
 *
 * Units.  A position is Q15 cells, int32: 1 unit = 1/32768 cell, and the cell of a coordinate p is p >> 15 (arithmetic, so
 * floor: -1 unit lies in cell -1).  An angle is 1/65536 turn, held mod 65536.  The direction table has T =
 * LOM_ROLLOUT_TABLE = 4096 entries (C[b], S[b]), exactly lom_visibility_table(4096); an angle a reads entry a >> 4.
 *
 * Grid.  lom_occupancy_geometry, reused, with the planning grids' rules: row-major with y as the row.  r > 0 and finite, a
 * finite origin, 1 <= width, height <= 8192; anything else is LOM_ERR_ARG.
 *
 * Planes.  The cost plane is a full-grid int8 plane: v >= lethal_min is lethal; v < 0 is unknown -- lethal when
 * unknown_cost < 0, else it costs unknown_cost; any other cell costs v.  lom_clearance_cost's plane works with lethal_min
 * 99 or 100.  The potential plane, optional, is u32 in lom_navfield_potential's form.
 * lom_rollout_params: 1 <= segments <= 8 (L); 1 <= steps_per_segment <= 128 (Tn); S = L * Tn <= 1024; 1 <= lethal_min <=
 * 100; -1 <= unknown_cost <= 98; min_steps <= S; progress_weight <= 256; cost_weight <= 4096; truncation_weight <= 2^20;
 * flags of LOM_ROLLOUT_KEEP_RECORDS only; anything else is LOM_ERR_ARG.
 * Inputs.  M states (x, y, a), 0 <= M <= 4096, with -2^29 <= x, y < 2^29 and a < 65536; K candidates of L commands (int16
 * v, int16 w) each, candidate by candidate, 0 <= K <= 2^20 and M * K <= 2^22: v is Q15 cells per step, w angle units per
 * step; F footprint samples (int32 fx, fy) in 1/256 cell in the robot's frame, 1 <= F <= 1024, |fx|, |fy| <= 16384;
 * anything else is LOM_ERR_ARG.
 *  1. Motion.  p_0 is the state.  For t = 0 .. S - 1 with l = t / Tn and b = a_t >> 4:  x_{t+1} = x_t + ((v_l * C[b] +
 *     16384) >> 15), y_{t+1} = y_t + ((v_l * S[b] + 16384) >> 15), a_{t+1} = (a_t + w_l) & 65535.  Every product fits
 *     int32.  The angle has a closed form per segment and the position is a prefix sum of integers, so no order of
 *     summation changes it.
 *  2. Pose test at p_t.  For each footprint sample, with b = a_t >> 4:  px = x_t + ((fx * C[b] - fy * S[b] + 128) >> 8),
 *     py = y_t + ((fx * S[b] + fy * C[b] + 128) >> 8), cell (px >> 15, py >> 15).  The sample's code, in this order:
 *     outside the grid LOM_ROLLOUT_EDGE (3); a lethal value LOM_ROLLOUT_COLLISION (2); unknown and lethal
 *     LOM_ROLLOUT_UNKNOWN (1); else LOM_ROLLOUT_OK (0) with the cell's cost.  The pose's code is the greatest sample code,
 *     its cost c_t the greatest cost over its OK samples.  A pose is free when its code is 0.
 *  3. Record.  lom_rollout_record, 32 bytes, per state and candidate (state-major): free_poses = t*, the least blocked t
 *     in 0 .. S, or S + 1 when there is none; reason, the code of pose t*, or 0; cost_sum and cost_max over the poses 0 ..
 *     t* - 1; end_x, end_y, end_angle, pose t* - 1, or the state itself when t* = 0; end_potential, P at the end pose's
 *     centre cell, LOM_NAV_UNREACHED outside the grid or without a potential plane.  A state whose own cell lies outside
 *     the grid is invalid: all of its records have free_poses = 0, the reason LOM_ROLLOUT_INVALID (4), and the rest as
 *     for t* = 0.
 *  4. Score and pick.  P0 is P at the state's cell.  A candidate is admissible when free_poses > min_steps and, with a
 *     potential plane, P0 and end_potential both differ from LOM_NAV_UNREACHED.  Its score, as int64:  s =
 *     progress_weight * (P0 - end_potential) - cost_weight * cost_sum - truncation_weight * (S + 1 - free_poses); the first
 *     term is 0 without a potential plane.  Per state, lom_rollout_pick: k, the greatest s among the admissible, ties to
 *     the least k -- 0xFFFFFFFF, with score 0, when there is none; admissible, their count; score.  |s| < 2^41, so (s +
 *     2^41) << 20 | (2^20 - 1 - k) orders the candidates as one unsigned 64-bit maximum.
 *  5. Summary.  states (M); valid_states; candidates (M * K); admissible, over all states; states_without_pick.
 * After create or lom_rollout_clear there is no state: no records.
 *
 * The result is a pure function of the planes, the parameters, the states, the commands and the footprint: it does not
 * depend on the order in which lanes, waves or workgroups run, on the test switches below, or on early exits.
 *
 * lom_rollout_evaluate takes host planes of width * height cells; _evaluate_device planes in HBM, each complete when its
 * event is (NULL: now), and reads them in place; _evaluate_from_grids reads lom_clearance_cost_device and, with a field,
 * lom_navfield_potential_device in place and orders the streams by events in both directions -- a grid whose resolution,
 * origin, width or height differ bit for bit, or that lives on another device, is LOM_ERR_ARG before any launch.  States,
 * commands and footprint are host memory in every form; picks: M entries.  Every argument is validated and every
 * allocation made before the first launch; a refused call changes nothing -- the records of the previous evaluation stay
 * -- and zeroes the picks (the first min(M, 4096) of them) and the summary.  An evaluation is one host wait, whatever M,
 * K and S.  Every call returns with its work done.  Calls on one handle are the caller's to serialise.  The error text is
 * the handle's (lom_rollout_last_error). */
#define LOM_ROLLOUT_TABLE 4096
typedef struct lom_rollout lom_rollout;
typedef struct {
    uint32_t segments;          /* L, 1 .. 8 */
    uint32_t steps_per_segment; /* Tn, 1 .. 128; S = L * Tn <= 1024 */
    int32_t lethal_min;         /* the least lethal value, 1 .. 100 */
    int32_t unknown_cost;       /* -1 .. 98; -1: unknown is lethal */
    uint32_t min_steps;         /* 0 .. S */
    uint32_t progress_weight;   /* 0 .. 256 */
    uint32_t cost_weight;       /* 0 .. 4096 */
    uint32_t truncation_weight; /* 0 .. 2^20 */
    uint32_t flags;             /* LOM_ROLLOUT_KEEP_RECORDS */
} lom_rollout_params;
typedef struct {
    int32_t x, y; /* Q15 cells */
    uint32_t a;   /* 1/65536 turn, < 65536 */
} lom_rollout_state;
typedef struct {
    uint32_t free_poses, reason;   /* offset 0, 4 */
    uint32_t cost_sum, cost_max;   /* 8, 12 */
    int32_t end_x, end_y;          /* 16, 20 */
    uint32_t end_angle;            /* 24 */
    uint32_t end_potential;        /* 28 */
} lom_rollout_record;
typedef struct {
    uint32_t k;          /* the candidate's index, 0xFFFFFFFF: none */
    uint32_t admissible; /* the state's admissible candidates */
    int64_t score;
} lom_rollout_pick;
typedef struct {
    uint64_t states, valid_states, candidates, admissible, states_without_pick;
} lom_rollout_summary;
typedef struct {
    uint64_t launches, waits; /* kernel launches of the last evaluation, and the host's waits for them */
} lom_rollout_call_stats;
enum { LOM_ROLLOUT_KEEP_RECORDS = 1 };
enum { LOM_ROLLOUT_OK = 0, LOM_ROLLOUT_UNKNOWN = 1, LOM_ROLLOUT_COLLISION = 2, LOM_ROLLOUT_EDGE = 3, LOM_ROLLOUT_INVALID = 4 };
enum {
    LOM_ROLLOUT_OPT_TEST_SERIAL = 1,       /* 1: the plain form, a lane per candidate stepping pose by pose; 0 or < 0: the
                                              default, a lane per pose */
    LOM_ROLLOUT_OPT_TEST_NO_LDS_PLANE = 2, /* 0: a window of the cost plane around the state is staged in LDS where that
                                              window fits; 1 or < 0: the default, the plane is read in HBM */
    LOM_ROLLOUT_OPT_TEST_WAVES = 3         /* waves of a workgroup of the lane-per-pose form: 1 or 4; <= 0: the default.  Test
                                              switches: the bytes are the same. */
};
int lom_rollout_create(const lom_occupancy_geometry *geometry, int device, lom_rollout **out);
void lom_rollout_destroy(lom_rollout *r);
const char *lom_rollout_last_error(const lom_rollout *r); /* r == NULL: why the last create on this thread failed */
int lom_rollout_clear(lom_rollout *r);                    /* no state, no records */
int lom_rollout_get_geometry(const lom_rollout *r, lom_occupancy_geometry *out);
void *lom_rollout_stream(lom_rollout *r); /* hipStream_t */
int lom_rollout_device(const lom_rollout *r);
int lom_rollout_wait_event(lom_rollout *r, void *hip_event);
int lom_rollout_set_option(lom_rollout *r, int option, int64_t value);
/* cost_plane: width * height int8; potential_or_null: width * height u32; states: m; commands: k * segments (v, w) int16
 * pairs; footprint: f (fx, fy) int32 pairs; picks: m entries */
int lom_rollout_evaluate(lom_rollout *r, const int8_t *cost_plane, const uint32_t *potential_or_null, const lom_rollout_state *states,
                         size_t m, const int16_t *commands, size_t k, const int32_t *footprint, size_t f,
                         const lom_rollout_params *params, lom_rollout_pick *picks, lom_rollout_summary *summary_or_null);
int lom_rollout_evaluate_device(lom_rollout *r, const int8_t *d_cost_plane, void *cost_event_or_null, const uint32_t *d_potential_or_null,
                                void *potential_event_or_null, const lom_rollout_state *states, size_t m, const int16_t *commands,
                                size_t k, const int32_t *footprint, size_t f, const lom_rollout_params *params,
                                lom_rollout_pick *picks, lom_rollout_summary *summary_or_null);
int lom_rollout_evaluate_from_grids(lom_rollout *r, lom_clearance *clearance, lom_navfield *navfield_or_null,
                                    const lom_rollout_state *states, size_t m, const int16_t *commands, size_t k,
                                    const int32_t *footprint, size_t f, const lom_rollout_params *params, lom_rollout_pick *picks,
                                    lom_rollout_summary *summary_or_null);
/* step 3: at most `cap` records of the last evaluation go to `out` (may be NULL with cap 0), state-major; *count_or_null:
 * M * K; LOM_ERR_STATE when the last evaluation did not run under LOM_ROLLOUT_KEEP_RECORDS */
int lom_rollout_records(lom_rollout *r, lom_rollout_record *out, size_t cap, size_t *count_or_null);
/* the launches and waits of the last evaluation (zeros before the first) */
int lom_rollout_stats(const lom_rollout *r, lom_rollout_call_stats *out);
/* Host-only helpers; none needs a handle or a device.
 * A rectangular footprint, all in 1/256 cell: xs = -back, -back + spacing, ... while < front, then front; ys likewise over
 * -half_width .. half_width; the lattice xs x ys (x-major), or with perimeter_only its border rows and columns.  At most
 * `cap` pairs go to `out` (may be NULL with cap 0); *count: the samples.  0 <= front, back, half_width <= 16384, spacing
 * >= 1, a count of at most 1024; anything else is LOM_ERR_ARG. */
int lom_rollout_footprint_rectangle(int32_t front, int32_t back, int32_t half_width, int32_t spacing, int perimeter_only, int32_t *out,
                                    size_t cap, size_t *count);
/* x = floor(((double)x_m - origin_x) / resolution * 32768), y likewise, a = llround(yaw / (2 pi) * 65536) & 65535; a
 * non-finite input or a position outside -2^29 .. 2^29 - 1 is LOM_ERR_ARG */
int lom_rollout_state_from_pose(const lom_occupancy_geometry *geometry, float x_m, float y_m, float yaw, lom_rollout_state *out);
/* step 1 alone: the S + 1 poses of one candidate (commands: segments pairs) go to `out` */
int lom_rollout_poses(const lom_rollout_params *params, const lom_rollout_state *state, const int16_t *commands, lom_rollout_state *out);

/* ---- grid shift: a grid follows the robot by whole cells (not in the reference) -----------------------------------------
 * Every grid family above fixes its geometry at create.  A shift moves the window by (dx, dy) whole cells: the content stays
 * where it is in the world, what still overlaps is kept, what enters is cleared, and the seven families follow by ONE rule,
 * so that handles of equal geometry shifted by the same (dx, dy) still agree bit for bit (what a consumer asks of its
 * producers).  A new capability: no default path launches any of it.  DESIGN.md 7r.
 *
 * The rule.  out = in moved by (dx, dy) cells: width, height and resolution unchanged,
 *   origin_x' = (float)((double)origin_x + (double)dx * (double)resolution), y likewise,
 * from the CURRENT f32 origin alone.  The rounding to f32 is part of the definition: the result is exact for a dyadic
 * resolution and a modest origin; with a resolution such as 0.1f the origin moves by under one ulp of itself per shift, so
 * shifting out and back need not return the first origin's bits.  The geometry rule is the occupancy grid's (sides up to
 * 16384), the widest of the families'.
 * LOM_ERR_ARG: `in` fails the geometry rule or a pointer is NULL.  LOM_ERR_RANGE: an origin' that is not finite (out
 * untouched).  in and out may be the same object.  Host code: no handle, no device. */
int lom_grid_shift_geometry(const lom_occupancy_geometry *in, int32_t dx, int32_t dy, lom_occupancy_geometry *out);
/* The shift that brings a robot at (x, y) metres back towards the middle.  Per axis, side n, shift d:
 *   q = floor(((double)x - (double)origin) / (double)resolution)            (the grids' own index rule)
 *   d = 0                                        if margin <= q < n - margin
 *   d = trunc((q - n / 2) / quantum) * quantum   otherwise                  (n / 2: integer division; trunc: towards zero)
 * margin + quantum <= n / 2 guarantees that after the shift the robot's cell lies in [margin, n - margin); d is a multiple
 * of the quantum.  The caller takes the pose from lom_odometry_get_pose, asks this, and shifts its handles.
 * LOM_ERR_ARG: a bad geometry or a NULL, x or y not finite, quantum == 0, or margin + quantum > n / 2 on either axis.
 * LOM_ERR_RANGE: |q| > 2^40 or |d| > INT32_MAX.  On an error *dx = *dy = 0.  Host code: no handle, no device. */
int lom_grid_follow(const lom_occupancy_geometry *g, double x, double y, uint32_t margin_cells, uint32_t quantum_cells, int32_t *dx,
                    int32_t *dy);
/* The two grids that hold state.  The geometry becomes lom_grid_shift_geometry(geometry, dx, dy) (an elevation grid's z_ref
 * stays); cell (ix, iy) afterwards holds what cell (ix + dx, iy + dy) held before where that cell is in the grid, and
 * elsewhere its cleared value: both counts 0; the record of lom_elevation_clear (sum 0, count 0, zmin INT32_MAX, zmax
 * INT32_MIN).  dx == dy == 0 is LOM_OK with no launch; |dx| >= width or |dy| >= height equals a clear plus the new geometry.
 * One launch moves everything, each destination cell written once, into a second block that is allocated at the first such
 * call and swapped with the first behind the launch: a grid that shifts holds its state twice.  LOM_ERR_RANGE from the rule
 * and LOM_ERR_OOM from that allocation leave the grid and its geometry untouched.  The call runs on the grid's stream,
 * behind whatever consumers released to it (lom_*_wait_event), and returns with its work done.  A pointer from
 * lom_occupancy_classify_device / lom_elevation_cost_device is invalid afterwards, as after any call on the handle; later
 * integrate, classify, cost, layers, cells and counts use the new geometry with no further step.  (The seven shifts are
 * declared through function types, like lom_archive_add_points: each family's own section lists what came with the family.) */
typedef int(lom_occupancy_shift_fn)(lom_occupancy *g, int32_t dx, int32_t dy);
typedef int(lom_elevation_shift_fn)(lom_elevation *g, int32_t dx, int32_t dy);
lom_occupancy_shift_fn lom_occupancy_shift;
lom_elevation_shift_fn lom_elevation_shift;
/* The five planning families follow: the geometry moves by the same rule and the handle's state afterwards is exactly what
 * its own lom_*_clear leaves (also for dx == dy == 0), so the next update / solve / extract / cast / evaluate is a full one:
 * these handles are recomputed from their producers anyway.  Carrying the clearance distances across a shift is not part of
 * this; a navigation field is carried by lom_navfield_shift_resolve* (navigation field, "Shift and re-solve").  LOM_ERR_RANGE from the rule leaves the handle untouched.  A consumer that was not shifted meets a
 * shifted producer with the usual refusal, "... resolution, origin, width or height differs". */
typedef int(lom_clearance_shift_fn)(lom_clearance *c, int32_t dx, int32_t dy);
typedef int(lom_navfield_shift_fn)(lom_navfield *f, int32_t dx, int32_t dy);
typedef int(lom_regions_shift_fn)(lom_regions *r, int32_t dx, int32_t dy);
typedef int(lom_visibility_shift_fn)(lom_visibility *v, int32_t dx, int32_t dy);
typedef int(lom_rollout_shift_fn)(lom_rollout *r, int32_t dx, int32_t dy);
lom_clearance_shift_fn lom_clearance_shift;
lom_navfield_shift_fn lom_navfield_shift;
lom_regions_shift_fn lom_regions_shift;
lom_visibility_shift_fn lom_visibility_shift;
lom_rollout_shift_fn lom_rollout_shift;

/* ---- pose field: cost-to-go over cell and heading under a footprint (not in the reference) ---------------------------
 * The navigation field is solved for a point: a robot that is longer than wide is routed round bends it cannot turn in, and
 * the rollouts, which do test a footprint at a heading, then find every candidate blocked.  This handle family solves the
 * field over states (cell, heading) for the robot's own footprint, with eight headings and unit primitives: the smallest
 * exact form of kinodynamic planning.  Nothing is launched unless a caller creates a pose field.  The definition, operation
 * by operation (tests/posefield_ref.py restates it with a heap Dijkstra on Python integers; everything is an integer and
 * the field is the unique fixed point of a relaxation with positive weights, so every comparison is exact):
 *
 * Grid.  lom_occupancy_geometry with the navigation field's rules and limits.  A cell costs 70 bytes of HBM: P and L at 32
 * bytes each (u32 per heading), the floor at 5 (u32 and the heading byte), the kept cost byte at 1.
 *
 * Input of a solve.  One full-grid int8 cost plane; lom_posefield_params: nav, a lom_navfield_params under its own rule;
 * turn_cost, spin_cost, reverse_cost, each at most 2^24 - 1, spin_cost >= 1 under LOM_POSE_SPIN; flags of LOM_POSE_SPIN |
 * LOM_POSE_REVERSE only; anything else is LOM_ERR_ARG.  c[] is exactly the table of lom_navfield_cell_costs(nav): 0 means
 * impassable, and cells outside the grid are impassable.
 *  1. Headings.  H = 8.  Heading h points along (hx, hy) = E, NE, N, NW, W, SW, S, SE for h = 0 .. 7: counter-clockwise,
 *     +x is E and +y is N.  len(h) = 5 for an even h, 7 for an odd h.  In the rollouts' angle units heading h is the angle
 *     8192 h, and the heading of an angle a is ((a + 4096) >> 13) & 7 (lom_posefield_heading_of_angle).
 *  2. Footprint and stencils.  F samples (int32 fx, fy) in 1/256 cell in the robot's frame, with the rollouts' limits: 1 <=
 *     F <= 1024, |fx|, |fy| <= 16384; anything else is LOM_ERR_ARG.  Per heading, with b = 512 h and (C, S) of
 *     lom_visibility_table(4096), the rollouts' step 2 at angle 8192 h:  ox = (fx * C[b] - fy * S[b] + 128) >> 8,  oy =
 *     (fx * S[b] + fy * C[b] + 128) >> 8, and the sample's cell offset is ((16384 + ox) >> 15, (16384 + oy) >> 15)
 *     (arithmetic shifts): the cell a rollout reads for that sample at a pose on a cell's centre.  The distinct cell
 *     offsets of a heading, sorted by (dy, dx), are its stencil; the host builds it.  lom_posefield_stencils gives the
 *     eight without a handle or a device.  An offset reaches up to 91 cells.
 *  3. Layers.  L[h][cell], u32: 0 if any stencil cell of h around the cell lies outside the grid or has c == 0, else the
 *     greatest c over the stencil.  A state (cell, h) is passable iff L[h][cell] != 0.  lom_posefield_layers reads them.
 *  4. Moves, from state (a, h) with s = L[h][a] != 0 and d(h) = (hx, hy).  A translation along +-d(h) to b is allowed iff
 *     L[h][b] != 0 and, for an odd h, L[h] != 0 at the two cells that share an edge with both a and b (the side cells are
 *     tested in the source heading's layer).  A rotation at cell b from h to h' = h +- 1 (mod 8) is allowed iff L[h][b] != 0
 *     and L[h'][b] != 0.  In this fixed order:
 *       0  F   (a + d(h), h)      translation                                     len(h) * s
 *       1  FL  (a + d(h), h + 1)  translation, then rotation at the target cell   len(h) * s + turn_cost
 *       2  FR  (a + d(h), h - 1)  the same                                        the same
 *       3  SL  (a, h + 1)         rotation at a; only under LOM_POSE_SPIN         spin_cost
 *       4  SR  (a, h - 1)         the same                                        the same
 *       5  B   (a - d(h), h)      translation backwards; only under LOM_POSE_REVERSE   len(h) * s + reverse_cost
 *     Every weight is positive and below 2^28: a move pays for the state it leaves.
 *  5. Goals.  G int32 triples (ix, iy, h), at most 2^24.  h in 0 .. 7 names one state; h = -1 names every heading of the
 *     cell whose layer is non-zero there.  A goal whose cell is outside the grid, whose h is outside -1 .. 7, or that names
 *     no passable state counts in goals_rejected; goals_used counts the distinct goal states.  G = 0 or nothing used is
 *     LOM_OK with everything unreached.
 *  6. Field.  P[h][cell], u32, planar [8][height][width]: 0 on goal states; elsewhere the least total weight over all move
 *     sequences to a goal state.  LOM_NAV_UNREACHED and LOM_NAV_MAX apply as in the navigation field: a candidate above
 *     LOM_NAV_MAX is dropped, so exactly the states whose true value exceeds it read LOM_NAV_UNREACHED, and every state
 *     behind them.  range_exceeded = 1 iff, at the fixed point, some reached state b and some allowed move a -> b have P[b]
 *     + weight > LOM_NAV_MAX (computed in the summary pass).  Impassable states read LOM_NAV_UNREACHED.
 *  7. Floor.  floor[cell] = the least P over h, u32 in lom_navfield_potential's form; floor_heading[cell], u8: the least h
 *     that attains it, 8 where no heading is reached.  Both come from the summary pass; with lom_posefield_floor_device,
 *     lom_rollout_evaluate_device and the other _device consumers take the floor as their potential plane as they are.
 *  8. Summary.  states_blocked (L == 0), states_reached, states_unreached (passable, not reached) -- the three add up to
 *     8 * width * height -- cells_reached (floor reached), cells_invalid (cost bytes outside -1 .. 100), goals_used,
 *     goals_rejected, range_exceeded, max_potential (0 if nothing is reached).
 *  9. Paths.  K int32 triples, at most 2^24; h = -1 starts at the floor_heading of the cell.  A start outside the grid,
 *     with h outside -1 .. 7, or on an unreached state has length 0.  From a state with P > 0 the walk takes the first move
 *     in the order of step 4 that is allowed and has P[target] + weight == P[state] -- one exists at the fixed point -- and
 *     stops at P == 0.  Output: u16 triples (ix, iy, h) in a [K, cap] buffer, K * cap <= 2^28, the rest of a row 0; the
 *     length counts start and goal and is the full length even above cap.  P falls strictly, so a walk is bounded by
 *     8 * cells.
 * 10. Query.  n points in metres by the floor rule, with one int32 heading each: P of that state, the floor for -1;
 *     LOM_NAV_UNREACHED for a point outside the grid, a coordinate that is not a number or a heading outside -1 .. 7.
 *
 * The result is a pure function of plane, parameters, footprint and goals: it does not depend on the order in which lanes,
 * waves or workgroups run, nor on the test switches below (k_posefield.hpp says why).
 *
 * lom_posefield_solve takes a host plane of width * height bytes; _solve_device a plane in HBM that is complete when
 * hip_event_or_null is; _solve_from_clearance reads lom_clearance_cost_device in place with the event ordering and the bit
 * for bit geometry check of lom_navfield_solve_from_clearance.  Footprint and goals are host memory in every form.  Every
 * argument is validated and every allocation made before the first launch; a refused call changes nothing and zeroes the
 * summary.  After create or clear every state is unreached and impassable, the floor unreached with heading 8.
 * lom_posefield_shift is the planning grids' shift: the geometry moves by that rule, the state is lom_posefield_clear's.
 * The relaxation runs to its fixed point through the navigation field's host loop with its bound of 2 * cells + 64
 * launches; a solve that would need more ends with LOM_ERR_HIP.  Every call returns with its work done.  Calls on one
 * handle are the caller's to serialise.  The error text is the handle's (lom_posefield_last_error).
 * Measured on one MI355X (python tools/posefield_cost.py -> profiles/posefield_cost.json; HIP events, five alternating blocks,
 * medians; lom_posefield_solve_device, one goal): 4096 x 4096 at 2 % obstacles 173.2 ms for a point and 187.5 ms for a 9 x 3-
 * cell rectangle with both flags (352 launches, 22 waits), 80.9 and 99.5 ms at 0.01 %; 1174 x 160 2.7 to 7.1 ms (32 to 64
 * launches).  The same call under LOM_POSE_OPT_TEST_ALL_TILES, the plain global sweep, takes 1.8 to 3.2 times as long at
 * 4096 x 4096 and 1 to 2 % more at 1174 x 160, with the same bytes.  lom_navfield_solve_device on the same plane and goal
 * cell, as context only: 46.6 / 20.2 ms and 2.87 / 1.42 ms.  What bounds k_pose_relax: NOT MEASURED.  DESIGN.md 7u.
 *
 * Re-solve.  A pose field that has completed a solve keeps its plane, its table, its stencils, its lom_posefield_params,
 * the layers and P.  lom_posefield_resolve* takes a new full-grid int8 plane and an optional lom_clearance_window, with that
 * struct's rules: the rectangle is clipped to the grid, NULL is the whole grid, an empty rectangle is LOM_OK and changes
 * nothing.  No footprint, parameters or goals are passed: they are the last solve's.
 *  a. Merged plane.  The kept plane with the cells of the clipped window replaced by the new plane's.  Cells outside the
 *     window are not read; the host form uploads only the rows of the window.
 *  b. Layers.  L of the merged plane is exactly what lom_posefield_solve computes for it (step 3) with the last solve's
 *     footprint and parameters.
 *  c. Goals.  The states with P == 0 before the call: the goal states the last solve or re-solve used.  A goal state whose
 *     layer is 0 under the merged plane counts in goals_rejected and is gone for later re-solves; goals_used +
 *     goals_rejected equals the previous goals_used.  The goals are states, not cells: a heading of a goal cell that the
 *     last solve skipped because it was impassable there does not become a goal when the change makes it passable, whether
 *     the goal was named with h = -1 or not.
 *  d. Result.  L, P, the floor, its heading and the summary are, byte for byte, what lom_posefield_solve leaves on the
 *     merged plane with the last solve's footprint and parameters and those goal states passed as explicit (ix, iy, h)
 *     triples.  The kept plane becomes the merged plane; paths and queries read the new state; the pointers of
 *     lom_posefield_potential_device and lom_posefield_floor_device stay valid across the call.
 *  e. Refusals.  No completed solve since create, clear or shift: LOM_ERR_STATE.  A NULL plane, or a clearance grid of
 *     other geometry or on another device: LOM_ERR_ARG.  Every refusal comes before any device work, changes nothing (the
 *     counters of lom_posefield_resolve_stats included) and zeroes the summary.
 *  f. Counters of the last re-solve, through lom_posefield_resolve_stats.  cells_changed: the bytes of the clipped window
 *     that differ from the kept ones.  states_changed: the (cell, heading) whose layer differs.  states_raised: the states
 *     that were reached and passable under the merged plane and that the raise phase set unreached -- the least such set,
 *     below; under form 1 every reached state but the goal states.  raise_launches, relax_launches, waits, tiles_marked as
 *     lom_navfield_resolve_counters'.  cells_changed == 0 ends the call behind the diff: nothing else is launched, the state
 *     is untouched and the summary is the last one with goals_rejected 0.
 * The work is incremental and still exact.  A diff over the window (k_pose_diff) merges the plane and finds the changed
 * cells and their bounding box; from there the work is sized by what changed, not by the window.  One launch
 * (k_pose_relayer) recomputes the layers per heading over the changed box dilated by that heading's stencil, sets the
 * states that are now impassable to unreached and marks the tiles that hold a changed state or read one as halo.  The
 * raise phase (k_pose_raise) then sets every reached state unreached that no chain of supporters carries down to a goal
 * state under the new layers -- a supporter of state a is a state b with an allowed move a -> b of step 4 and P[b] + weight
 * <= P[a]; every weight is positive (a translation at least 5, a spin spin_cost >= 1), so the set is well defined and does
 * not depend on the schedule -- and the relaxation of a solve lowers what is left, every value an upper bound, to the
 * field; the summary pass of a solve runs once.  LOM_POSE_OPT_TEST_RESOLVE_FORM 1 is the baseline on the same handle: the
 * layers over the whole merged plane, every state but the goal states unreached, the full relaxation; same bytes, same
 * summary.  LOM_POSE_OPT_TEST_INNER_CAP, _BATCH and _ALL_TILES act on the raise phase and the relaxation alike.  A seed
 * array of one u32 per tile is allocated at the first re-solve.
 * Measured on one MI355X (python tools/posefield_resolve_cost.py -> profiles/posefield_resolve_cost.json; HIP events, five
 * alternating blocks, medians; a wall of 64 cells put into / taken out of a 64 x 64 window, both planes in HBM, one goal in a
 * corner; the default form against form 1 on the same handle, same bytes in all 48 cases): with the window in the far
 * corner from the goal 5.2 to 6.3 ms against 155 to 447 ms at 4096 x 4096 (26x to 86x) and 0.50 to 1.57 ms against 4.8 to
 * 14.1 ms at 1174 x 160 (5.2x to 19x); half way ahead in all 32 cases (1.2x to 71x); next to the goal with the wall going
 * in it LOSES in 10 of 16 cases (0.35x to 0.79x; 416 to 550 ms against 157 to 204 at 4096 x 4096 and 0.01 % obstacles),
 * since nearly every state rises and is solved again, and is ahead when the wall comes out (1.1x to 5.3x).  What bounds
 * k_pose_raise: NOT MEASURED.  DESIGN.md 7v. */
#define LOM_POSE_HEADINGS 8
typedef struct lom_posefield lom_posefield;
typedef struct {
    lom_navfield_params nav; /* the cell costs */
    uint32_t turn_cost;      /* what FL and FR add, 0 .. 2^24 - 1 */
    uint32_t spin_cost;      /* the weight of SL and SR, 1 .. 2^24 - 1 under LOM_POSE_SPIN (0 .. 2^24 - 1 otherwise) */
    uint32_t reverse_cost;   /* what B adds, 0 .. 2^24 - 1 */
    uint32_t flags;          /* LOM_POSE_* */
} lom_posefield_params;
typedef struct {
    uint64_t states_blocked, states_reached, states_unreached, cells_reached, cells_invalid, goals_used, goals_rejected,
        range_exceeded, max_potential;
} lom_posefield_summary;
typedef struct {
    uint64_t launches, waits; /* of k_pose_relax in the last solve, and the host's waits for them */
    uint64_t tiles;           /* workgroups per launch */
} lom_posefield_solve_stats;
typedef struct {
    uint64_t cells_changed;  /* bytes of the clipped window that differ from the kept ones */
    uint64_t states_changed; /* (cell, heading) whose layer differs */
    uint64_t states_raised;  /* reached states the raise phase (form 1: the reset) set unreached */
    uint64_t raise_launches, relax_launches; /* of k_pose_raise and k_pose_relax */
    uint64_t waits;          /* the host's waits, the diff's included */
    uint64_t tiles_marked;   /* seeds of the relaxation */
} lom_posefield_resolve_counters; /* what lom_posefield_resolve_stats gives */
enum { LOM_POSE_SPIN = 1, LOM_POSE_REVERSE = 2 };
enum {
    LOM_POSE_OPT_TEST_INNER_CAP = 1, /* as LOM_NAV_OPT_TEST_INNER_CAP */
    LOM_POSE_OPT_TEST_BATCH = 2,     /* launches per wait, as LOM_NAV_OPT_TEST_BATCH */
    LOM_POSE_OPT_TEST_ALL_TILES = 3, /* as LOM_NAV_OPT_TEST_ALL_TILES */
    LOM_POSE_OPT_TEST_RESOLVE_FORM = 4 /* 0 or < 0, the default: raise, then relax; 1: the baseline, the full solve on the
                                          same handle.  Test switches: the bytes are the same. */
};
int lom_posefield_create(const lom_occupancy_geometry *geometry, int device, lom_posefield **out);
void lom_posefield_destroy(lom_posefield *f);
const char *lom_posefield_last_error(const lom_posefield *f); /* f == NULL: why the last create on this thread failed */
int lom_posefield_clear(lom_posefield *f);                    /* every state unreached and impassable */
int lom_posefield_shift(lom_posefield *f, int32_t dx, int32_t dy);
int lom_posefield_get_geometry(const lom_posefield *f, lom_occupancy_geometry *out);
void *lom_posefield_stream(lom_posefield *f); /* hipStream_t */
int lom_posefield_device(const lom_posefield *f);
int lom_posefield_wait_event(lom_posefield *f, void *hip_event);
int lom_posefield_set_option(lom_posefield *f, int option, int64_t value);
/* footprint: n_samples (fx, fy) int32 pairs; goals: n_goals (ix, iy, h) int32 triples (may be NULL with n_goals 0) */
int lom_posefield_solve(lom_posefield *f, const int8_t *plane, const lom_posefield_params *params, const int32_t *footprint,
                        size_t n_samples, const int32_t *goals, size_t n_goals, lom_posefield_summary *summary_or_null);
int lom_posefield_solve_device(lom_posefield *f, const int8_t *d_plane, void *hip_event_or_null, const lom_posefield_params *params,
                               const int32_t *footprint, size_t n_samples, const int32_t *goals, size_t n_goals,
                               lom_posefield_summary *summary_or_null);
int lom_posefield_solve_from_clearance(lom_posefield *f, lom_clearance *clearance, const lom_posefield_params *params,
                                       const int32_t *footprint, size_t n_samples, const int32_t *goals, size_t n_goals,
                                       lom_posefield_summary *summary_or_null);
/* Re-solve (above): plane as lom_posefield_solve's, d_plane as _solve_device's, clearance as _solve_from_clearance's */
int lom_posefield_resolve(lom_posefield *f, const int8_t *plane, const lom_clearance_window *window_or_null,
                          lom_posefield_summary *summary_or_null);
int lom_posefield_resolve_device(lom_posefield *f, const int8_t *d_plane, void *hip_event_or_null,
                                 const lom_clearance_window *window_or_null, lom_posefield_summary *summary_or_null);
int lom_posefield_resolve_from_clearance(lom_posefield *f, lom_clearance *clearance, const lom_clearance_window *window_or_null,
                                         lom_posefield_summary *summary_or_null);
/* the counters of the last re-solve (zeros before the first) */
int lom_posefield_resolve_stats(const lom_posefield *f, lom_posefield_resolve_counters *out);
/* P, [8][height][width]: at most `cap` states go to `out` (may be NULL with cap 0) */
int lom_posefield_potential(lom_posefield *f, uint32_t *out, size_t cap);
/* the same, left in HBM: 8 * width * height states, valid until the next solve, clear or shift on the handle */
int lom_posefield_potential_device(lom_posefield *f, const uint32_t **d_out);
/* L, [8][height][width], likewise */
int lom_posefield_layers(lom_posefield *f, uint32_t *out, size_t cap);
/* step 7: at most `cap` cells go to each of floor_out and heading_out (either may be NULL) */
int lom_posefield_floor(lom_posefield *f, uint32_t *floor_out, uint8_t *heading_out, size_t cap);
/* the same, left in HBM (either pointer may be NULL), valid as lom_posefield_potential_device's */
int lom_posefield_floor_device(lom_posefield *f, const uint32_t **d_floor_out, const uint8_t **d_heading_out);
/* step 9: n_starts triples in host memory; states_out: [n_starts, cap] u16 triples (may be NULL with cap 0), lengths_out:
 * n_starts u32 (may be NULL) */
int lom_posefield_paths(lom_posefield *f, const int32_t *starts, size_t n_starts, uint16_t *states_out, size_t cap,
                        uint32_t *lengths_out);
/* step 10: n points (x, y in the grid's frame, f32 pairs) and n int32 headings in host memory, at most 2^30 */
int lom_posefield_query(lom_posefield *f, const float *xy, const int32_t *headings, size_t n, uint32_t *out);
/* the launches and waits of the last solve (zeros before the first) */
int lom_posefield_stats(const lom_posefield *f, lom_posefield_solve_stats *out);
/* Host-only helpers; neither needs a handle or a device.
 * Step 2: counts_out[h], the cells of the stencil of heading h; at most `cap` (dx, dy) int32 pairs go to `cells_out` (may be
 * NULL with cap 0), heading after heading.  LOM_ERR_ARG for a bad footprint or a NULL counts_out. */
int lom_posefield_stencils(const int32_t *footprint, size_t n_samples, int32_t *cells_out, size_t cap, uint32_t *counts_out);
/* step 1: the heading of an angle in 1/65536 turn (any value: it is taken mod 65536) */
uint32_t lom_posefield_heading_of_angle(uint32_t angle);

/* LidarOdometry::Params, src/lidar_odometry.h:23-48 */
typedef struct {
    float lidar_min_range, lidar_max_range;
    float keyframe_voxel_size;
    uint32_t keyframe_max_points_cnt;
    float keyframe_matching_voxel_size, keyframe_update_voxel_size;
    float keyframe_cleanup_range, angular_divergence_threshold;
} lom_odometry_params;

typedef struct {
    int64_t planar_points, filtered_points, update_points, matching_points, keyframe_voxels, queries;
    int32_t outer_iterations, initialised_keyframe, unstable_rotation;
    int32_t host_stages; /* 1: the stages before the align ran on the host (LOM_HOST_FRONTEND=1, or a frame the device front end handed back) */
    int64_t queries_total; /* source points x outer iterations of all frames since creation */
} lom_odometry_frame_stats;

typedef struct lom_odometry lom_odometry;
void lom_odometry_default_params(lom_odometry_params *p);          /* lidar_odometry.h:36-48 defaults */
int lom_odometry_create(const lom_odometry_params *p, int device, lom_odometry **out); /* lidar_odometry.cpp:14-20 */
void lom_odometry_destroy(lom_odometry *o);
int lom_odometry_process_cloud(lom_odometry *o, const lom_point_xyzirt *pts, size_t n); /* :22-77 */
/* a caller's frame loop in compiled code (the reference's caller is the C++ node, lidar_odometry_node.cpp:45-76): exactly
 * `count` calls of lom_odometry_process_cloud, frames[i] with n[i] points, nothing else; stops at the first frame that
 * fails and returns its status; *done = frames processed */
int lom_odometry_process_sequence(lom_odometry *o, const lom_point_xyzirt *const *frames, const size_t *n, size_t count,
                                  size_t *done);
/* one frame for each of `count` distinct odometries on one device; for every i exactly what
 * lom_odometry_process_cloud(o[i], frames[i], n[i]) would do -- poses, stats, keyframe, temp cloud -- with the
 * aligns of all streams that have one run as one lom_match_align_multi.  status_out[i]: that stream's status;
 * returns LOM_OK or the first failing stream's status.  A stream that fails is left as process_cloud leaves it.
 * The stages of all streams are enqueued before any is waited for.  The batch neither runs the keyframe cleanup's scan
 * behind the align nor sends hinted frames ahead (as with LOM_NO_CLEANUP_BEHIND_ALIGN / LOM_NO_SEND_AHEAD: the results
 * are the same); a hint left on a handle is dropped.  LOM_ERR_ARG before any stream is touched for count < 0, a NULL
 * array with count > 0, a NULL handle or frame, the same handle twice, or handles on different devices. */
int lom_odometry_process_batch(lom_odometry *const *o, const lom_point_xyzirt *const *frames, const size_t *n, int count,
                               int *status_out_or_null);
/* A caller that already holds the frame that comes after the next lom_odometry_process_cloud (a recorded sequence; a
 * driver that buffers) says so here: while that call's align runs -- its thread would only watch the report -- the hinted
 * frame is copied into the front end's pinned staging buffer, and the process_cloud that then comes with exactly this
 * pointer and size skips that copy (8 us of a C5 frame).  The buffer must stay unchanged until that call has returned.
 * Host work only; poses and counts never differ; a hint that is not followed by its frame costs one copy.
 * lom_odometry_process_sequence hints frame i + 1 before frame i by itself. */
int lom_odometry_hint_next(lom_odometry *o, const lom_point_xyzirt *pts, size_t n);
int lom_odometry_get_pose(const lom_odometry *o, lom_pose *out);   /* getCurrentPose, :87-89 */
/* getTempCloud(), lidar_odometry.h:73-75 (the node publishes it as /deskewed_cloud,
 * lidar_odometry_node.cpp:66-75): the time-normalised, deskewed input cloud of the last processCloud
 * (lidar_odometry.cpp:30-31), all fields kept.  Returns the number of points it holds (0 before the
 * first frame, where the reference returns a null pointer); writes at most `cap` records; out may be
 * NULL with cap 0 (count only). */
int64_t lom_odometry_get_temp_cloud(const lom_odometry *o, lom_point_xyzirt *out, size_t cap);
/* The place descriptor (lom_place_describe) of that cloud -- the last frame's deskewed cloud -- through `db`, which
 * must live on the odometry's device: read from the front end's copy in HBM where the frame's stages ran on the device
 * (ordered behind the front end's done event), uploaded from the host copy for a host-stage frame; the result is the same
 * either way.  add != 0: the descriptor also becomes a new entry of db, whose id goes to id_out_or_null.
 * LOM_ERR_STATE before the first frame.  Reads only: no pose, counter or map of the odometry is touched. */
int lom_odometry_place_descriptor(lom_odometry *o, lom_place_db *db, int add, float *desc_out_or_null,
                                  int64_t *id_out_or_null);
/* The last frame's update cloud -- what the keyframe update of that frame transforms and inserts: the planar, range-
 * filtered cloud down-sampled at keyframe_update_voxel_size, with normals, in the sensor frame -- becomes a new scan of
 * `a`, which must live on the odometry's device (LOM_ERR_ARG otherwise); its id goes to *id_out.  The cloud is in HBM
 * whichever way the frame's stages ran, and is copied device to device; the result is the same either way.  The call
 * waits for the pending keyframe update and for its own copy, so the next frame cannot overwrite what it reads.
 * LOM_ERR_STATE before the first frame.  Reads only: no pose, counter or map of the odometry is touched. */
int lom_odometry_archive_scan(lom_odometry *o, lom_archive *a, int64_t *id_out);
/* The last frame's deskewed cloud -- every point of it, not the planar, down-sampled update cloud -- becomes a new scan of
 * `a` without normals (lom_archive_add_points): what an occupancy grid rebuilt after a loop closure needs, since the
 * update clouds miss every obstacle that is not planar.  Read as lom_odometry_place_descriptor reads it (the front end's
 * copy in HBM behind its done event, or the host copy of a host-stage frame; the same lifetime rule), records of 32
 * bytes.  `a` must live on the odometry's device.  LOM_ERR_STATE before the first frame.  Reads only. */
int lom_odometry_archive_deskewed(lom_odometry *o, lom_archive *a, int64_t *id_out);
/* That cloud at the current pose (lom_odometry_get_pose through lom_graph_pose_from_f32) into an occupancy grid on the
 * odometry's device: lom_occupancy_integrate_cloud_device behind the front end's done event, or
 * lom_occupancy_integrate_cloud of the host copy of a host-stage frame; the result is the same either way.
 * LOM_ERR_STATE before the first frame.  Reads only: no pose, counter or map of the odometry is touched. */
int lom_odometry_occupancy_scan(lom_odometry *o, lom_occupancy *g, const lom_occupancy_ray_params *p,
                                lom_occupancy_stats *stats_or_null);
/* Its twin for an elevation grid on the odometry's device: lom_elevation_integrate_cloud_device behind the front end's
 * done event, or lom_elevation_integrate_cloud of the host copy of a host-stage frame; the result is the same either way.
 * LOM_ERR_STATE before the first frame.  Reads only: no pose, counter or map of the odometry is touched. */
int lom_odometry_elevation_scan(lom_odometry *o, lom_elevation *g, const lom_elevation_point_params *p,
                                lom_elevation_stats *stats_or_null);
/* Go on after a loop closure: the keyframe is built again from archived scans at corrected poses.  In this order:
 *  1. the pending keyframe update is waited for (its failure is this call's, and nothing else happens);
 *  2. an armed cleanup behind the align and a pending lom_odometry_hint_next are dropped;
 *  3. the keyframe is cleared; it keeps its voxel size and keyframe_max_points_cnt;
 *  4. lom_map_assemble(keyframe, a, ids, poses, count, {centre = new_current->t, radius = keyframe_cleanup_range}, stats);
 *  5. with C = lom_pose_compose(new_current, lom_pose_inverse(current)):  previous = lom_pose_compose(C, previous), then
 *     current = *new_current.
 * LOM_ERR_STATE before the keyframe is initialised; LOM_ERR_ARG for NULL arguments or an archive on another device
 * (both before anything is touched).  If the assembly fails -- a bad id or pose, a point out of range -- its status is
 * returned, the poses stay as they were, and the keyframe is left cleared: the next frame initialises it anew, as the
 * first frame does. */
int lom_odometry_rebuild_keyframe(lom_odometry *o, lom_archive *a, const int64_t *ids, const lom_graph_pose *poses,
                                  size_t count, const lom_pose *new_current, lom_assemble_stats *stats_or_null);
int lom_odometry_get_stats(const lom_odometry *o, lom_odometry_frame_stats *out);
/* LOM_OPT_QUALITY_REPORT: the degeneracy thresholds of the per-frame report (lom_match_quality's min_eig_t / min_eig_r;
 * both 0 = not counted until the caller sets them: the project has no measured basis for a default), and the report of
 * the last frame that aligned -- LOM_ERR_STATE before the first such frame or with the option off.  With
 * lom_odometry_process_batch every stream gets its own, one stream after another. */
int lom_odometry_set_quality_thresholds(lom_odometry *o, float min_eig_t, float min_eig_r);
int lom_odometry_get_quality(const lom_odometry *o, lom_quality_report *out);
/* switches of the pipeline (LOM_OPT_TEST_FORCE_HOST_REDO, the LOM_OPT_TEST_GRID_GIVE_UP family) and, for every other
 * option, of its keyframe handle (the align's).  The environment is read once, by lom_odometry_create
 * (LOM_HOST_THREADS, LOM_SYNC_KEYFRAME_UPDATE, LOM_HOST_FRONTEND, LOM_DEBUG_TIMING, and the A/B switches
 * LOM_NO_CLEANUP_BEHIND_ALIGN, LOM_NO_SEND_AHEAD; lom_map_create reads LOM_DENSE_CLEANUP). */
int lom_odometry_set_option(lom_odometry *o, int option, int64_t value);
/* The classifier of the following frames (lom_frontend_set_classifier); process_cloud, process_sequence, process_batch,
 * hint_next and LOM_OPT_QUALITY_REPORT work with either.  The neighbourhood classifier has no host version: choosing it on
 * an object created with LOM_HOST_FRONTEND=1, or while LOM_OPT_TEST_FORCE_HOST_REDO is set (and setting that option while
 * it is chosen), is LOM_ERR_STATE, and a frame beyond the device front end's size limit fails with LOM_ERR_ARG. */
int lom_odometry_set_classifier(lom_odometry *o, int kind, const lom_neighbourhood_params *p_or_null);
/* Ray carving in the keyframe update (see "ray carving" above).  NULL, the default, launches nothing.  With parameters
 * set, the update of every frame that aligned runs lom_map_carve_rays_device between the radius cleanup and the insert
 * (lidar_odometry.cpp:67 / :70): the origin is the frame's pose translation, the rays are its update cloud in the map
 * frame.  The frame that initialises the keyframe carves nothing.  lom_odometry_get_carve_stats: the last carve's stats,
 * LOM_ERR_STATE while none has run. */
int lom_odometry_set_carve(lom_odometry *o, const lom_carve_params *p_or_null);
int lom_odometry_get_carve_stats(const lom_odometry *o, lom_carve_stats *out);
/* Scan votes in lom_odometry_rebuild_keyframe (see "scan votes" above).  NULL, the default: not one launch or byte of a
 * rebuild changes.  With parameters set, the rebuild runs lom_map_carve_scans(keyframe, a, ids, poses, count, p) right
 * after its step 4, so the movers that the archived update clouds still hold do not come back; a failure is handled as
 * the assembly's failure is (its status is returned, the poses stay, the keyframe is left cleared).  voxels_after and
 * points_stored_after of the rebuild's stats then describe the keyframe behind the votes.
 * lom_odometry_get_rebuild_vote_stats: the stats of the last rebuild's votes, LOM_ERR_STATE before one ran. */
int lom_odometry_set_rebuild_votes(lom_odometry *o, const lom_vote_params *p_or_null);
int lom_odometry_get_rebuild_vote_stats(const lom_odometry *o, lom_vote_stats *out);
int64_t lom_odometry_debug_counter(const lom_odometry *o, int which); /* LOM_COUNTER_GRID_REDOS: all its handles + frames redone */
/* test hook (teacher-forced parity tests): overwrite previous_transform_ / current_transform_
 * (lidar_odometry.h:84-85); the keyframe itself can be replaced through lom_odometry_keyframe() */
int lom_odometry_debug_set_state(lom_odometry *o, const lom_pose *previous, const lom_pose *current);
lom_map *lom_odometry_keyframe(lom_odometry *o); /* keyframe_ (getKeyFrameCloud / getFullKeyFrameCloud via lom_map_export) */
const char *lom_odometry_last_error(const lom_odometry *o);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR_ODOMETRY_AMD_H */
