// Per-frame front end of LidarOdometry::processCloud on the device -- the callers of the scan-matching
// path, so that a frame stays in HBM from its upload to its pose:
//
//   utils::pointTimeNormalize            reference src/utils/point_time_normalize.h:15-39
//   CloudTransformer::transformNonRigid  reference src/utils/cloud_transform.h:15-40   (deskew)
//   CloudClassifier::classify            reference src/utils/cloud_classifier.h:19-168
//   utils::rangeFilter                   reference src/utils/range_filter.h:13-28
//
// Kernels: k_frontend.hpp (and k_neighbourhood.hpp for the ringless classifier).
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "grid_scan.hpp"
#include "k_neighbourhood.hpp"
#include "lom_internal.hpp"
#include "pose_math.hpp"
#include "k_frontend.hpp"

using namespace lom;

// ---- host side ------------------------------------------------------------------------------------
struct lom_frontend : DeviceHandle {
    bool own_stream = false;
    PinnedBuf stage;  // pinned bounce buffer for the raw frame
    void *d_stage_view = nullptr;  // ... as the device sees it (looked up once per allocation, not per frame)
    hipEvent_t stage_ev = nullptr, done_ev = nullptr;
    // per-frame arrays, sized together by fe_reserve: the frame, deskewed; cell winners; organised cloud; results
    DeviceBuf in, desk, win, org, xyz, nrm;
    size_t cap_pts = 0, cap_cells = 0;
    DeviceBuf stats;    // FeStats [2]
    DeviceBuf words;    // u32: kFeWords + aggregates
    PinnedBuf h_words;  // pinned copy
    uint32_t seq = 0;
    uint32_t n_last = 0;
    int test_grid_give_up = -1;  // LOM_OPT_TEST_GRID_GIVE_UP (one shot)
    bool dma_upload = false;     // LOM_FE_DMA_UPLOAD=1 at create
    uint32_t stats_set = 0;      // which of the two FeStats sets the next frame uses
    // neighbourhood classifier (lom_frontend_set_classifier, k_neighbourhood.hpp): the frame's voxel index is a map
    // handle on this stream, created when the classifier is chosen and reused frame after frame
    int kind = LOM_CLASSIFIER_RINGS, last_kind = LOM_CLASSIFIER_RINGS;  // chosen / of the last frame
    lom_neighbourhood_params nb{};
    lom_map *nb_index = nullptr;
    DeviceBuf nb_blk;     // u64: workgroup totals of the multi-launch compaction
    DeviceBuf nb_detail;  // lom_neighbourhood_detail: lom_classify_neighbourhood with details only
    struct {  // the last run of the stage, for its redo
        lom_neighbourhood_params p{};
        float min_sq = 0.f, max_sq = 0.f;
        int apply_range = 0;
        bool detail = false;
    } nb_last;
    int64_t grid_redos = 0;  // neighbourhood stages redone by the multi-launch form (lom_frontend_debug_counter)

    lom_point_xyzirt *d_in() const { return in.as<lom_point_xyzirt>(); }
    lom_point_xyzirt *d_desk() const { return desk.as<lom_point_xyzirt>(); }
    uint32_t *d_win() const { return win.as<uint32_t>(); }
    float4 *d_org() const { return org.as<float4>(); }
    float *d_xyz() const { return xyz.as<float>(); }
    float *d_nrm() const { return nrm.as<float>(); }
    FeStats *d_stats() const { return stats.as<FeStats>(); }
    uint32_t *d_words() const { return words.as<uint32_t>(); }
    uint32_t *hw() const { return h_words.as<uint32_t>(); }
    unsigned long long *d_nb_blk() const { return nb_blk.as<unsigned long long>(); }
    lom_neighbourhood_detail *d_nb_detail() const { return nb_detail.as<lom_neighbourhood_detail>(); }
};

namespace {

Granule *fe_agg(lom_frontend *f) { return reinterpret_cast<Granule *>(f->d_words() + 64); }

// room for a frame of n points: all six arrays anew, nothing carried over
int fe_reserve(lom_frontend *f, size_t n)
{
    if (n <= f->cap_pts) return LOM_OK;
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    f->cap_pts = 0;
    const size_t cap = n + n / 2 + 4096;
    const size_t cells = 3 * cap + 4096;  // rings of unequal size make H * W exceed n; beyond this the host stages take the frame
    const std::pair<DeviceBuf *, size_t> want[] = {{&f->in, cap * sizeof(lom_point_xyzirt)}, {&f->desk, cap * sizeof(lom_point_xyzirt)},
                                                   {&f->win, cells * 4}, {&f->org, cells * sizeof(float4)},
                                                   {&f->xyz, cells * 12}, {&f->nrm, cells * 12}};
    for (const auto &w : want) release(*w.first);
    for (const auto &w : want)
        if (const int rc = ensure(f, *w.first, w.second); rc != LOM_OK) return rc;
    LOM_HIP(f, hipMemsetAsync(f->win.p, 0, cells * 4, f->stream));  // at rest: k_fe_planar clears what a frame set
    f->cap_pts = cap;
    f->cap_cells = cells;
    return LOM_OK;
}

// the frame-level part of Eigen's slerp (cloud_transform.h:27) with the host's libm
void frame_const(const lom_pose &start, const lom_pose &end, float min_range, float max_range, FrameConst &F)
{
    for (int k = 0; k < 4; k++) F.sq[k] = start.q[k], F.eq[k] = end.q[k];
    for (int k = 0; k < 3; k++) F.st[k] = start.t[k], F.et[k] = end.t[k];
    const float *a = start.q, *b = end.q;
    const float one = 1.0f - 1.1920928955078125e-07f;
    const float d = (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]);
    const float ad = std::fabs(d);
    F.linear = ad >= one ? 1 : 0;
    F.negate = d < 0.0f ? 1 : 0;
    F.theta = 0.f;
    F.sin_theta = 1.f;
    if (!F.linear) {
        F.theta = std::acos(ad);
        F.sin_theta = std::sin(F.theta);
    }
    F.min_sq = min_range * min_range;
    F.max_sq = max_range * max_range;
}

int nb_fail_map(lom_frontend *f, int rc)
{
    f->error = lom_last_error(f->nb_index);
    return rc;
}

// the index workspace for these parameters: created once, its slab stride follows index_cap, its voxel size is set by
// the clear in front of every insert
int nb_workspace(lom_frontend *f, const lom_neighbourhood_params &p)
{
    int rc;
    if (!f->nb_index) {
        // capacity hint 2^15: the table never reaches 16 times its smallest size for a frame the front end takes, so
        // the insert never settles the table size (a read-back) afterwards
        if ((rc = lom_map_create(p.radius, p.index_cap, (size_t)1 << 15, f->device, &f->nb_index)) != LOM_OK)
            return fail(f, rc, lom_last_error(nullptr));
        if ((rc = lom_map_set_stream(f->nb_index, f->stream)) != LOM_OK) return nb_fail_map(f, rc);
    }
    if ((rc = ensure(f, f->nb_blk, kNbMaxBlocks * sizeof(unsigned long long))) != LOM_OK) return rc;
    if (f->nb_index->max_points != p.index_cap) {
        if ((rc = lom_map_clear(f->nb_index, p.radius)) != LOM_OK) return nb_fail_map(f, rc);
        if ((rc = lom_map_set_max_points(f->nb_index, p.index_cap)) != LOM_OK) return nb_fail_map(f, rc);
    }
    return LOM_OK;
}

void nb_launch_compact(lom_frontend *f, uint32_t N, float min_sq, float max_sq, int apply_range, uint32_t seq, bool multi)
{
    const float4 *rec = f->d_org();  // the organised cloud's buffer is free under this classifier: one record per input point
    if (!multi) {
        const uint32_t fail_from = f->test_grid_give_up < 0 ? 0xFFFFFFFFu : (uint32_t)f->test_grid_give_up;
        f->test_grid_give_up = -1;
        if (N <= kOnePassMax)
            hipLaunchKernelGGL((k_nb_compact<1, 0>), dim3(std::max(1u, blocks_for(N))), dim3(kThreads), 0, f->stream, f->d_desk(), rec, N,
                               min_sq, max_sq, apply_range, f->d_xyz(), f->d_nrm(), fe_agg(f), f->d_nb_blk(), seq, f->d_words(), fail_from);
        else
            hipLaunchKernelGGL((k_nb_compact<kFeItems, 0>), dim3(blocks_for((N + kFeItems - 1) / kFeItems)), dim3(kThreads), 0,
                               f->stream, f->d_desk(), rec, N, min_sq, max_sq, apply_range, f->d_xyz(), f->d_nrm(), fe_agg(f),
                               f->d_nb_blk(), seq, f->d_words(), fail_from);
        return;
    }
    // the multi-launch form: totals, their scan, the write -- no workgroup waits for another
    const uint32_t nb = std::max(1u, blocks_for(N));  // <= kNbMaxBlocks: N <= kFeItems * kOnePassMax
    hipLaunchKernelGGL((k_nb_compact<1, 1>), dim3(nb), dim3(kThreads), 0, f->stream, f->d_desk(), rec, N, min_sq, max_sq, apply_range,
                       f->d_xyz(), f->d_nrm(), fe_agg(f), f->d_nb_blk(), seq, f->d_words(), 0xFFFFFFFFu);
    hipLaunchKernelGGL(k_nb_offsets, dim3(1), dim3(kThreads), 0, f->stream, f->d_nb_blk(), nb);
    hipLaunchKernelGGL((k_nb_compact<1, 2>), dim3(nb), dim3(kThreads), 0, f->stream, f->d_desk(), rec, N, min_sq, max_sq, apply_range,
                       f->d_xyz(), f->d_nrm(), fe_agg(f), f->d_nb_blk(), seq, f->d_words(), 0xFFFFFFFFu);
}

// the stage on the N deskewed points in f->d_desk(): index insert, evaluation, compaction -- enqueued, nothing waits.
// redo: the insert waits for its own verdict (and redoes itself should its scan give up), the compaction takes the
// multi-launch form.
int nb_enqueue(lom_frontend *f, uint32_t N, const lom_neighbourhood_params &p, float min_sq, float max_sq, int apply_range,
               bool detail, uint32_t seq, bool redo)
{
    int rc;
    if ((rc = nb_workspace(f, p)) != LOM_OK) return rc;
    lom_map *ix = f->nb_index;
    f->nb_last.p = p;
    f->nb_last.min_sq = min_sq, f->nb_last.max_sq = max_sq;
    f->nb_last.apply_range = apply_range;
    f->nb_last.detail = detail;
    if ((rc = lom_map_clear(ix, p.radius)) != LOM_OK) return nb_fail_map(f, rc);
    const uint32_t *d_range = nullptr, *d_grid = nullptr;
    uint32_t idx_seq = 0;
    if (N) {
        rc = redo ? lom_map_add_points_device(ix, reinterpret_cast<const float *>(f->d_desk()), nullptr, N, sizeof(lom_point_xyzirt))
                  : lom_map_add_points_device_nowait(ix, reinterpret_cast<const float *>(f->d_desk()), nullptr, N,
                                                     sizeof(lom_point_xyzirt));
        if (rc != LOM_OK) return nb_fail_map(f, rc);
        if (!redo) lom_map_status_words(ix, &d_range, &d_grid, &idx_seq);
    }
    NbArgs A;
    A.r2 = (double)p.radius * (double)p.radius;
    A.max_variation = (double)p.max_variation;
    A.min_spread = (double)p.min_spread;
    A.min_neighbours = p.min_neighbours;
    if (N) {
        const uint32_t blocks = std::min(blocks_for(N, kNbBatch), 256u * 8u);
        hipLaunchKernelGGL(k_nb_eval, dim3(blocks), dim3(kThreads), 0, f->stream, view_of(ix), f->d_desk(), N, A, f->d_org(),
                           detail ? f->d_nb_detail() : nullptr, d_range, d_grid, idx_seq, seq, f->d_words());
    }
    nb_launch_compact(f, N, min_sq, max_sq, apply_range, seq, redo);
    LOM_HIP(f, hipGetLastError());
    return LOM_OK;
}

// after a wait: the words of the last neighbourhood stage are in h_words.  A point out of range fails the frame as it
// fails the down-samplers; a scan that gave up -- the index insert's or the compaction's -- has written nothing, and the
// stage is redone here by the forms that wait for nobody.
int nb_settle(lom_frontend *f)
{
    if (f->hw()[6] == f->seq) return fail(f, LOM_ERR_RANGE, "coordinate / radius out of range or not finite");
    if (f->hw()[5] != f->seq) return LOM_OK;
    f->grid_redos++;
    int rc = nb_enqueue(f, f->n_last, f->nb_last.p, f->nb_last.min_sq, f->nb_last.max_sq, f->nb_last.apply_range,
                        f->nb_last.detail, f->seq, true);
    if (rc != LOM_OK) return rc;
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    LOM_HIP(f, hipMemcpyAsync(f->hw(), f->d_words(), kFeWords * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return LOM_OK;
}

}  // namespace

extern "C" {

int lom_frontend_create(int device, void *hip_stream, lom_frontend **out)
{
    if (!out) return LOM_ERR_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) {
        (void)hipGetLastError();
        return LOM_ERR_NO_DEVICE;
    }
    lom_frontend *f = new (std::nothrow) lom_frontend();
    if (!f) return LOM_ERR_OOM;
    f->device = device;
    f->dma_upload = getenv("LOM_FE_DMA_UPLOAD") != nullptr;
    const size_t wbytes = 64 * 4 + 256 * 2 * sizeof(Granule);
    if (hipSetDevice(device) != hipSuccess || (hip_stream == nullptr && hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking) != hipSuccess) ||
        alloc(f->stats, 2 * sizeof(FeStats)) != hipSuccess || alloc(f->words, wbytes) != hipSuccess ||
        alloc(f->h_words, 64 * 4, hipHostMallocDefault) != hipSuccess ||
        hipEventCreateWithFlags(&f->stage_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&f->done_ev, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        lom_frontend_destroy(f);
        return LOM_ERR_HIP;
    }
    if (hip_stream)
        f->stream = (hipStream_t)hip_stream;
    else
        f->own_stream = true;
    FeStats init[2];
    std::memset(init, 0, sizeof init);
    init[0].tmin = init[1].tmin = 0xFFFFFFFFu;
    if (hipMemcpy(f->d_stats(), init, sizeof init, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(f->d_words(), 0, wbytes) != hipSuccess) {
        (void)hipGetLastError();
        lom_frontend_destroy(f);
        return LOM_ERR_HIP;
    }
    *out = f;
    return LOM_OK;
}

void lom_frontend_destroy(lom_frontend *f)
{
    if (!f) return;
    (void)hipSetDevice(f->device);
    if (f->stream) (void)hipStreamSynchronize(f->stream);
    if (f->nb_index) lom_map_destroy(f->nb_index);  // it runs on this stream: it goes first
    if (f->stage_ev) (void)hipEventDestroy(f->stage_ev);
    if (f->done_ev) (void)hipEventDestroy(f->done_ev);
    if (f->own_stream && f->stream) (void)hipStreamDestroy(f->stream);
    delete f;  // the buffers go with it
}

const char *lom_frontend_last_error(const lom_frontend *f) { return f ? f->error.c_str() : ""; }

int lom_frontend_set_option(lom_frontend *f, int option, int64_t value)
{
    if (!f) return LOM_ERR_ARG;
    if (option == LOM_OPT_TEST_GRID_GIVE_UP && value >= -1 && (value & ~(int64_t)kGridFailOnlyOne) <= 65535) {
        f->test_grid_give_up = (int)value;
        return LOM_OK;
    }
    return LOM_ERR_ARG;
}

int lom_frontend_process(lom_frontend *f, const lom_point_xyzirt *pts, size_t n, const lom_pose *start, const lom_pose *end,
                         float min_range, float max_range)
{
    if (!f || (n && !pts) || !start || !end) return LOM_ERR_ARG;
    // the organised cloud is scanned by one grid of at most kFeItems * 65536 cells, sized n + n / 2 + 4096
    if (n + n / 2 + 4096 > (size_t)kFeItems * kOnePassMax) return fail(f, LOM_ERR_ARG, "frame too large for the device front end");
    LOM_HIP(f, hipSetDevice(f->device));
    f->error.clear();
    int rc = fe_reserve(f, std::max<size_t>(n, 1));
    if (rc != LOM_OK) return rc;
    const uint32_t N = (uint32_t)n;
    const uint32_t seq = ++f->seq;
    f->n_last = N;
    // raw frame -> pinned bounce buffer -> HBM (the caller's buffer is free when this returns); a caller that
    // has written the frame into lom_frontend_stage()'s buffer itself passes that pointer and skips the copy
    const size_t bytes = n * sizeof(lom_point_xyzirt);
    if (static_cast<const void *>(pts) != f->stage.h || bytes > f->stage.bytes) {
        lom_point_xyzirt *stage = nullptr;
        if ((rc = lom_frontend_stage(f, n, &stage)) != LOM_OK) return rc;
        if (bytes) std::memcpy(static_cast<void *>(stage), pts, bytes);
    }
    // the frame reaches HBM through k_fe_stats, which reads the pinned buffer itself (LOM_FE_DMA_UPLOAD=1 at create: through
    // a copy of its own in front of the kernels, as until round 3 -- on C5 that was ~10 us more per frame)
    const lom_point_xyzirt *stats_in = f->d_in();
    lom_point_xyzirt *stats_keep = nullptr;
    if (f->dma_upload || !bytes) {
        if (bytes) LOM_HIP(f, hipMemcpyAsync(f->d_in(), f->stage.h, bytes, hipMemcpyHostToDevice, f->stream));
        LOM_HIP(f, hipEventRecord(f->stage_ev, f->stream));
    } else {
        if (!f->d_stage_view) LOM_HIP(f, hipHostGetDevicePointer(&f->d_stage_view, f->stage.h, 0));
        stats_in = static_cast<const lom_point_xyzirt *>(f->d_stage_view);
        stats_keep = f->d_in();
    }
    FrameConst F;
    frame_const(*start, *end, min_range, max_range, F);
    FeStats *mine = f->d_stats() + f->stats_set, *next = f->d_stats() + (f->stats_set ^ 1u);
    f->stats_set ^= 1u;
    const uint32_t cell_cap = (uint32_t)std::min<size_t>(f->cap_cells, (size_t)kFeItems * kOnePassMax);
    const uint32_t pt_blocks = std::max(1u, std::min(blocks_for(N), 1024u));
    hipLaunchKernelGGL(k_fe_stats, dim3(pt_blocks), dim3(kThreads), 0, f->stream, stats_in, N, mine, next, stats_keep);
    if (stats_keep) LOM_HIP(f, hipEventRecord(f->stage_ev, f->stream));  // the staging buffer is free once this kernel has read it
    // the organised cloud has H * W cells, known on the device only: the grids cover what a frame of n points
    // normally needs (rings of equal size: H * W ~ n) with a margin; a larger cloud raises the fall-back flag
    const uint32_t cells_bound = (uint32_t)std::min<size_t>(cell_cap, (size_t)N + N / 2 + 4096);
    f->last_kind = f->kind;
    if (f->kind == LOM_CLASSIFIER_NEIGHBOURHOOD) {
        // time normalisation and deskew as they are; with no room for an organised cloud k_fe_deskew leaves the cell
        // table alone (its fall-back word [4] means nothing here: no azimuth bin is used)
        hipLaunchKernelGGL(k_fe_deskew, dim3(pt_blocks), dim3(kThreads), 0, f->stream, f->d_in(), N, F, mine, f->d_desk(), f->d_win(),
                           0u, seq, f->d_words());
        LOM_HIP(f, hipGetLastError());
        if ((rc = nb_enqueue(f, N, f->nb, F.min_sq, F.max_sq, 1, false, seq, false)) != LOM_OK) return rc;
        LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
        return LOM_OK;
    }
    hipLaunchKernelGGL(k_fe_deskew, dim3(pt_blocks), dim3(kThreads), 0, f->stream, f->d_in(), N, F, mine, f->d_desk(), f->d_win(),
                       cells_bound, seq, f->d_words());
    hipLaunchKernelGGL(k_fe_curv, dim3(blocks_for(cells_bound)), dim3(kThreads), 0, f->stream, f->d_desk(), f->d_win(),
                       f->d_words(), cells_bound, f->d_org());
    const uint32_t fail_from = f->test_grid_give_up < 0 ? 0xFFFFFFFFu : (uint32_t)f->test_grid_give_up;
    f->test_grid_give_up = -1;
    if (cells_bound <= kOnePassMax)
        hipLaunchKernelGGL(k_fe_planar<1>, dim3(blocks_for(cells_bound)), dim3(kThreads), 0, f->stream, f->d_org(), f->d_win(),
                           cells_bound, F, f->d_xyz(), f->d_nrm(), fe_agg(f), seq, f->d_words(), fail_from);
    else
        hipLaunchKernelGGL(k_fe_planar<kFeItems>, dim3(blocks_for((cells_bound + kFeItems - 1) / kFeItems)), dim3(kThreads), 0,
                           f->stream, f->d_org(), f->d_win(), cells_bound, F, f->d_xyz(), f->d_nrm(), fe_agg(f), seq, f->d_words(),
                           fail_from);
    LOM_HIP(f, hipGetLastError());
    LOM_HIP(f, hipEventRecord(f->done_ev, f->stream));
    return LOM_OK;
}

// pinned staging buffer for a frame of n points (valid until the next lom_frontend_stage / process of a larger
// frame); waits until the previous frame's upload has read it
int lom_frontend_stage(lom_frontend *f, size_t n, lom_point_xyzirt **out)
{
    if (!f || !out) return LOM_ERR_ARG;
    LOM_HIP(f, hipSetDevice(f->device));
    const size_t bytes = n * sizeof(lom_point_xyzirt);
    LOM_HIP(f, hipEventSynchronize(f->stage_ev));
    if (bytes > f->stage.bytes) {  // (its own rule: the upload that read the old block is over, nothing is synchronised)
        release(f->stage);
        f->d_stage_view = nullptr;
        const hipError_t e = alloc(f->stage, std::max(bytes + bytes / 2, (size_t)1 << 20), hipHostMallocDefault);
        if (e != hipSuccess) return fail(f, LOM_ERR_HIP, "hipHostMalloc(stage)", e);
    }
    *out = f->stage.as<lom_point_xyzirt>();
    return LOM_OK;
}

// hipEvent_t recorded behind the last frame's kernels: a consumer on another stream waits for it
void *lom_frontend_done_event(lom_frontend *f) { return f ? (void *)f->done_ev : nullptr; }

// device-side results of the last lom_frontend_process: the filtered planar cloud (packed xyz, normals),
// an upper bound of its size known to the host, and the words {planar, filtered, H, W, fall-back, error}
int lom_frontend_results(lom_frontend *f, const float **d_xyz, const float **d_nrm, const uint32_t **d_counts,
                         uint32_t *bound)
{
    if (!f) return LOM_ERR_ARG;
    if (d_xyz) *d_xyz = f->d_xyz();
    if (d_nrm) *d_nrm = f->d_nrm();
    if (d_counts) *d_counts = f->d_words();
    if (bound) *bound = f->n_last;
    return LOM_OK;
}

int lom_frontend_deskewed(lom_frontend *f, const lom_point_xyzirt **d_out, uint32_t *n_out)
{
    if (!f || !d_out || !n_out) return LOM_ERR_ARG;
    *d_out = f->d_desk();
    *n_out = f->n_last;
    return LOM_OK;
}

void *lom_frontend_stream(lom_frontend *f) { return f ? (void *)f->stream : nullptr; }
uint32_t lom_frontend_sequence(const lom_frontend *f) { return f ? f->seq : 0u; }

// test hook: the device's restatement of glibc's sinf on n host values
int lom_debug_sinf(lom_frontend *f, const float *x, size_t n, float *out)
{
    if (!f || (n && (!x || !out))) return LOM_ERR_ARG;
    LOM_HIP(f, hipSetDevice(f->device));
    DeviceBuf buf;
    LOM_HIP(f, alloc(buf, std::max<size_t>(n, 1) * 4));
    float *d = buf.as<float>();
    hipError_t e = hipMemcpyAsync(d, x, n * 4, hipMemcpyHostToDevice, f->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_debug_sinf, dim3(blocks_for(std::max<size_t>(n, 1))), dim3(kThreads), 0, f->stream, d, (uint32_t)n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, n * 4, hipMemcpyDeviceToHost, f->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(f->stream);
    if (e != hipSuccess) return fail(f, LOM_ERR_HIP, "lom_debug_sinf", e);
    return LOM_OK;
}

// waits for the frame and returns its verdict: LOM_OK, or 1 when the frame has to be redone by the host stages
// (an azimuth on a rounding boundary, an organised cloud larger than the device buffers), or a negative status
int lom_frontend_wait(lom_frontend *f, uint32_t counts_out[4])
{
    if (!f) return LOM_ERR_ARG;
    LOM_HIP(f, hipSetDevice(f->device));
    LOM_HIP(f, hipMemcpyAsync(f->hw(), f->d_words(), kFeWords * 4, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    if (f->last_kind == LOM_CLASSIFIER_NEIGHBOURHOOD) {  // never 1: there is no host version, the device redoes its own frame
        const int rc = nb_settle(f);
        if (rc != LOM_OK) return rc;
        if (counts_out)
            for (int k = 0; k < 4; k++) counts_out[k] = f->hw()[k];
        return LOM_OK;
    }
    if (counts_out)
        for (int k = 0; k < 4; k++) counts_out[k] = f->hw()[k];
    // a grid that gave up has written nothing and left the cell table at rest: the frame goes to the host stages
    return (f->hw()[4] == f->seq || f->hw()[5] == f->seq) ? 1 : LOM_OK;
}

int lom_frontend_set_classifier(lom_frontend *f, int kind, const lom_neighbourhood_params *p)
{
    if (kind == LOM_CLASSIFIER_NEIGHBOURHOOD && !neighbourhood_params_ok(p)) return LOM_ERR_ARG;
    if (!f || (kind != LOM_CLASSIFIER_RINGS && kind != LOM_CLASSIFIER_NEIGHBOURHOOD)) return LOM_ERR_ARG;
    if (kind == LOM_CLASSIFIER_NEIGHBOURHOOD) {
        LOM_HIP(f, hipSetDevice(f->device));
        const int rc = nb_workspace(f, *p);
        if (rc != LOM_OK) return rc;
        f->nb = *p;
    }
    f->kind = kind;
    return LOM_OK;
}

int64_t lom_frontend_debug_counter(const lom_frontend *f, int which)
{
    if (!f || which != LOM_COUNTER_GRID_REDOS) return LOM_ERR_ARG;
    return f->grid_redos + (f->nb_index ? lom_map_debug_counter(f->nb_index, which) : 0);
}

int64_t lom_classify_neighbourhood(lom_frontend *f, const lom_point_xyzirt *pts, size_t n, const lom_neighbourhood_params *p,
                                   float *xyz_out, float *nrm_out, lom_neighbourhood_detail *detail_out)
{
    if (!neighbourhood_params_ok(p)) return LOM_ERR_ARG;
    if (!f || (n && (!pts || !xyz_out || !nrm_out))) return LOM_ERR_ARG;
    if (n + n / 2 + 4096 > (size_t)kFeItems * kOnePassMax) return fail(f, LOM_ERR_ARG, "frame too large for the device front end");
    LOM_HIP(f, hipSetDevice(f->device));
    f->error.clear();
    int rc = fe_reserve(f, std::max<size_t>(n, 1));
    if (rc != LOM_OK) return rc;
    if (detail_out && (rc = ensure(f, f->nb_detail, n * sizeof(lom_neighbourhood_detail))) != LOM_OK) return rc;
    const uint32_t N = (uint32_t)n;
    const uint32_t seq = ++f->seq;
    f->n_last = N;
    f->last_kind = LOM_CLASSIFIER_NEIGHBOURHOOD;
    // the frame goes where the deskew would have left it
    if (n) LOM_HIP(f, hipMemcpyAsync(f->d_desk(), pts, n * sizeof(lom_point_xyzirt), hipMemcpyHostToDevice, f->stream));
    if ((rc = nb_enqueue(f, N, *p, 0.f, 0.f, 0, detail_out != nullptr, seq, false)) != LOM_OK) return rc;
    uint32_t counts[4];
    if ((rc = lom_frontend_wait(f, counts)) != LOM_OK) return rc;
    const size_t np = counts[0];
    if (np) {
        LOM_HIP(f, hipMemcpyAsync(xyz_out, f->d_xyz(), np * 12, hipMemcpyDeviceToHost, f->stream));
        LOM_HIP(f, hipMemcpyAsync(nrm_out, f->d_nrm(), np * 12, hipMemcpyDeviceToHost, f->stream));
    }
    if (detail_out && n)
        LOM_HIP(f, hipMemcpyAsync(detail_out, f->d_nb_detail(), n * sizeof(lom_neighbourhood_detail), hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return (int64_t)np;
}

// copies of the device results for callers on the host (getTempCloud, tests): what = 0 the deskewed cloud
// (n records), 1 the filtered planar cloud (xyz + normals)
int64_t lom_frontend_fetch(lom_frontend *f, int what, void *out_a, void *out_b, size_t cap)
{
    if (!f || what < 0 || what > 1) return LOM_ERR_ARG;
    LOM_HIP(f, hipSetDevice(f->device));
    if (what == 0) {
        const size_t n = f->n_last, take = std::min(n, cap);
        if (take && out_a)
            LOM_HIP(f, hipMemcpyAsync(out_a, f->d_desk(), take * sizeof(lom_point_xyzirt), hipMemcpyDeviceToHost, f->stream));
        LOM_HIP(f, hipStreamSynchronize(f->stream));
        return (int64_t)n;
    }
    uint32_t counts[4];
    const int rc = lom_frontend_wait(f, counts);
    if (rc < 0) return rc;
    const size_t n = counts[1], take = std::min(n, cap);
    if (take && out_a) LOM_HIP(f, hipMemcpyAsync(out_a, f->d_xyz(), take * 12, hipMemcpyDeviceToHost, f->stream));
    if (take && out_b) LOM_HIP(f, hipMemcpyAsync(out_b, f->d_nrm(), take * 12, hipMemcpyDeviceToHost, f->stream));
    LOM_HIP(f, hipStreamSynchronize(f->stream));
    return (int64_t)n;
}

}  // extern "C"
