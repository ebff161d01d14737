// The odometry's host side without a handle and without a GPU call, as a program of its own
// (tests/test_host_stages_cpp.py builds it twice, with csrc/host_stages.cpp and csrc/host_threads.cpp):
//   test_host_stages stages <frame.bin>   under -fsanitize=address,undefined: the four host stages run through worker
//                                         pools against the serial run (equal as bytes), and the table of
//                                         decode_stage_words (csrc/stage_words.hpp), one row per branch
//   test_host_stages threads              under -fsanitize=thread: Pool and Deferred (csrc/host_threads.hpp) on their
//                                         spinning and their parked paths; no report is the pass condition
// <frame.bin>: lom_point_xyzirt records (frame 0 of the synth sequence: 26579 points, 16 rings).
// copy_to_stage (csrc/odometry_frame.cpp) takes the odometry handle and is not reached from here.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "check.hpp"
#include "host_stages.hpp"
#include "stage_words.hpp"

using namespace lom;

// ---- the four stages, chained as the odometry chains them -----------------------------------------
struct StageOutputs {
    std::vector<lom_point_xyzirt> normalized, deskewed;
    std::vector<float> planar, planar_n, filtered, filtered_n;
    size_t np = 0, nu = 0, nf = 0, grid[2] = {0, 0};
};

static void run_stages(const lom_point_xyzirt *pts, size_t n, const lom_pose &start, const lom_pose &end,
                       ClassifyScratch &scratch, Pool *pool, StageOutputs &out)
{
    const size_t cap = n ? n : 1;
    out.normalized.assign(cap, lom_point_xyzirt{});
    out.deskewed.assign(cap, lom_point_xyzirt{});
    for (auto *v : {&out.planar, &out.planar_n, &out.filtered, &out.filtered_n}) v->assign(cap * 3, 0.f);
    time_normalize(pts, n, out.normalized.data(), pool);
    transform_non_rigid(out.normalized.data(), n, start, end, out.deskewed.data(), pool);
    out.np = classify(out.deskewed.data(), n, out.planar.data(), out.planar_n.data(), &out.nu, out.grid, scratch, pool);
    out.nf = range_filter(out.planar.data(), out.planar_n.data(), out.np, 4.0f, 80.0f, out.filtered.data(),
                          out.filtered_n.data(), pool);
}

template <typename T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b, size_t count)
{
    return count == 0 || std::memcmp(static_cast<const void *>(a.data()), static_cast<const void *>(b.data()), count * sizeof(T)) == 0;
}

static void compare(const StageOutputs &want, const StageOutputs &got, size_t n, const char *what, unsigned threads)
{
    CHECK(same_bytes(want.normalized, got.normalized, n), "%s: time_normalize, n=%zu threads=%u", what, n, threads);
    CHECK(same_bytes(want.deskewed, got.deskewed, n), "%s: transform_non_rigid, n=%zu threads=%u", what, n, threads);
    CHECK(want.np == got.np && want.nu == got.nu && want.grid[0] == got.grid[0] && want.grid[1] == got.grid[1],
          "%s: classify counts %zu/%zu/%zux%zu against %zu/%zu/%zux%zu, n=%zu threads=%u", what, got.np, got.nu, got.grid[0],
          got.grid[1], want.np, want.nu, want.grid[0], want.grid[1], n, threads);
    CHECK(same_bytes(want.planar, got.planar, 3 * want.np) && same_bytes(want.planar_n, got.planar_n, 3 * want.np),
          "%s: classify output, n=%zu threads=%u", what, n, threads);
    CHECK(want.nf == got.nf, "%s: range_filter count %zu against %zu, n=%zu threads=%u", what, got.nf, want.nf, n, threads);
    CHECK(same_bytes(want.filtered, got.filtered, 3 * want.nf) && same_bytes(want.filtered_n, got.filtered_n, 3 * want.nf),
          "%s: range_filter output, n=%zu threads=%u", what, n, threads);
}

static void test_pooled_against_serial(const std::vector<lom_point_xyzirt> &frame)
{
    // a start pose that is no identity (half a radian about (1, 2, 3)), and a small end translation
    const float s = std::sin(0.25f) / std::sqrt(14.0f);
    const lom_pose start = {{0.05f, -0.02f, 0.01f}, {std::cos(0.25f), s, 2.0f * s, 3.0f * s}};
    const lom_pose end = {{0.01f, 0.f, 0.f}, {1.f, 0.f, 0.f, 0.f}};
    const size_t whole = frame.size();
    const size_t lengths[] = {0, 1, 2047, 2048, 2049, whole};
    std::vector<StageOutputs> serial(6);
    for (int l = 0; l < 6; l++) {
        ClassifyScratch fresh;
        run_stages(frame.data(), lengths[l], start, end, fresh, nullptr, serial[l]);
    }
    CHECK(serial[5].np >= 1 && serial[5].nf >= 1 && serial[5].nf < serial[5].np, "whole frame: %zu planar, %zu filtered",
          serial[5].np, serial[5].nf);
    std::printf("whole frame: %zu points, grid %zux%zu, %zu planar, %zu unclassified, %zu filtered\n", whole,
                serial[5].grid[0], serial[5].grid[1], serial[5].np, serial[5].nu, serial[5].nf);
    for (unsigned threads : {2u, 3u, 16u}) {
        Pool pool(threads);
        CHECK(pool.size() == threads, "pool size");
        for (int l = 0; l < 6; l++) {
            ClassifyScratch fresh;
            StageOutputs got;
            run_stages(frame.data(), lengths[l], start, end, fresh, &pool, got);
            compare(serial[l], got, lengths[l], "fresh scratch", threads);
        }
        // one scratch over frames of different sizes, as the odometry keeps it: longer, shorter, longer
        ClassifyScratch kept;
        for (int l : {4, 5, 3, 5}) {
            StageOutputs got;
            run_stages(frame.data(), lengths[l], start, end, kept, &pool, got);
            compare(serial[l], got, lengths[l], "kept scratch", threads);
            if (l == 5) CHECK(got.np >= 1, "kept scratch: no planar point in the whole frame");
        }
    }
    {   // the serial run with a kept scratch as well
        ClassifyScratch kept;
        for (int l : {4, 5, 3, 5}) {
            StageOutputs got;
            run_stages(frame.data(), lengths[l], start, end, kept, nullptr, got);
            compare(serial[l], got, lengths[l], "kept scratch, serial", 1);
        }
    }
}

// ---- decode_stage_words: expectations written from the code this decoder replaced ------------------------
struct Row {
    const char *name;
    bool neighbourhood, force;
    uint32_t fe_redo_host, fe_grid, ds_range, ds_grid, fe_range;  // 1: the word holds this frame's number, 0: an older one
    StageVerdict::Action action;
    bool wait_front_end, count_redo;
    const char *error;
};

static void test_decoder()
{
    const uint32_t fe_seq = 7, seq_ds = 9;
    const char *voxel = "coordinate / voxel_size out of range or not finite";
    const char *radius = "coordinate / radius out of range or not finite";
    const StageVerdict::Action P = StageVerdict::kProceed, H = StageVerdict::kRedoHost, D = StageVerdict::kRedoDevice,
                               F = StageVerdict::kFailRange;
    const Row rows[] = {
        // ring classifier                                 nb     force  redo grid rng  dsg  fer
        {"rings: nothing",                                 false, false, 0, 0, 0, 0, 0, P, false, false, nullptr},
        {"rings: front end hands back",                    false, false, 1, 0, 0, 0, 0, H, false, false, nullptr},
        {"rings: front end's scan gave up",                false, false, 0, 1, 0, 0, 0, H, false, true, nullptr},
        {"rings: down-sampler's scan gave up",             false, false, 0, 0, 0, 1, 0, H, false, true, nullptr},
        {"rings: both scans gave up (one redo)",           false, false, 0, 1, 0, 1, 0, H, false, true, nullptr},
        {"rings: hands back and scan gave up",             false, false, 1, 1, 0, 0, 0, H, false, true, nullptr},
        {"rings: down-sampler out of range",               false, false, 0, 0, 1, 0, 0, F, false, false, voxel},
        {"rings: range word and give-up: give-up wins",    false, false, 0, 0, 1, 1, 0, H, false, true, nullptr},
        {"rings: range word and front-end give-up",        false, false, 0, 1, 1, 0, 0, H, false, true, nullptr},
        {"rings: range word and hand-back: host",          false, false, 1, 0, 1, 0, 0, H, false, false, nullptr},
        {"rings: forced host redo, nothing gave up",       false, true,  0, 0, 0, 0, 0, H, false, false, nullptr},
        {"rings: forced host redo and a give-up",          false, true,  0, 1, 0, 0, 0, H, false, true, nullptr},
        {"rings: forced host redo hides the range word",   false, true,  0, 0, 1, 0, 0, H, false, false, nullptr},
        {"rings: the front end's range word is not read",  false, false, 0, 0, 0, 0, 1, P, false, false, nullptr},
        // neighbourhood classifier
        {"nbhd: nothing",                                  true,  false, 0, 0, 0, 0, 0, P, false, false, nullptr},
        {"nbhd: fe_redo_host is the frame's: ignored",     true,  false, 1, 0, 0, 0, 0, P, false, false, nullptr},
        {"nbhd: a point out of range",                     true,  false, 0, 0, 0, 0, 1, F, false, false, radius},
        {"nbhd: point out of range and a give-up: fails",  true,  false, 0, 1, 0, 1, 1, F, false, false, radius},
        {"nbhd: front end's scan gave up (it counts)",     true,  false, 0, 1, 0, 0, 0, D, true,  false, nullptr},
        {"nbhd: down-sampler's scan gave up",              true,  false, 0, 0, 0, 1, 0, D, false, true, nullptr},
        {"nbhd: both scans gave up",                       true,  false, 0, 1, 0, 1, 0, D, true,  false, nullptr},
        {"nbhd: down-sampler out of range",                true,  false, 0, 0, 1, 0, 0, F, false, false, voxel},
        {"nbhd: range word and give-up: give-up wins",     true,  false, 0, 0, 1, 1, 0, D, false, true, nullptr},
        {"nbhd: ignored fe_redo_host, range word fails",   true,  false, 1, 0, 1, 0, 0, F, false, false, voxel},
        {"nbhd: ignored fe_redo_host, give-up on device",  true,  false, 1, 0, 0, 1, 0, D, false, true, nullptr},
        {"nbhd: forced host redo, nothing gave up",        true,  true,  0, 0, 0, 0, 0, H, false, false, nullptr},
    };
    for (const Row &r : rows)
        for (int kf = 0; kf < 2; kf++) {
            uint32_t w[kStageWords];
            w[kWordPlanar] = 100;
            w[kWordFiltered] = 80;
            w[kWordDsCount] = 50;
            w[kWordFeRedoHost] = r.fe_redo_host ? fe_seq : fe_seq - 1;
            w[kWordFeGrid] = r.fe_grid ? fe_seq : fe_seq - 1;
            w[kWordFeRange] = r.fe_range ? fe_seq : fe_seq - 1;
            w[kWordDsRange] = r.ds_range ? seq_ds : seq_ds - 1;
            w[kWordDsGrid] = r.ds_grid ? seq_ds : seq_ds - 1;
            const StageVerdict v = decode_stage_words(w, kf != 0, r.neighbourhood, fe_seq, seq_ds, r.force);
            CHECK(v.action == r.action, "%s (keyframe %d): action %d, expected %d", r.name, kf, (int)v.action, (int)r.action);
            CHECK(v.count_redo == r.count_redo, "%s (keyframe %d): count_redo %d", r.name, kf, (int)v.count_redo);
            if (r.action == D) CHECK(v.wait_front_end == r.wait_front_end, "%s (keyframe %d): wait_front_end %d", r.name, kf, (int)v.wait_front_end);
            if (r.action == F)
                CHECK(v.error && std::strcmp(v.error, r.error) == 0, "%s (keyframe %d): text '%s'", r.name, kf, v.error ? v.error : "(none)");
            if (r.action == P) {
                CHECK(v.planar == 100 && v.filtered == 80, "%s (keyframe %d): counts %u %u", r.name, kf, v.planar, v.filtered);
                CHECK(v.matching == (kf ? 50u : 0u) && v.update == (kf ? 0u : 50u), "%s (keyframe %d): down-sampler count %u / %u",
                      r.name, kf, v.matching, v.update);
            }
        }
    // the words of a fresh handle are zero, and so is no frame's number: sequence numbers start at one
    const uint32_t zero[kStageWords] = {0};
    CHECK(decode_stage_words(zero, true, false, 1, 1, false).action == P, "zero words");
}

// ---- Pool and Deferred under the thread sanitizer ------------------------------------------------------
static void sleep_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

static void pool_sum(Pool &pool, size_t n, size_t serial_below, bool expect_serial)
{
    size_t slot[16] = {0};
    unsigned calls[16] = {0};
    pool.parallel_for(n, [&](size_t b, size_t e, unsigned part) {
        for (size_t i = b; i < e; i++) slot[part] += i + 1;
        calls[part]++;
    }, serial_below);
    size_t sum = 0;
    unsigned parts = 0;
    for (int p = 0; p < 16; p++) sum += slot[p], parts += calls[p];
    CHECK(sum == n * (n + 1) / 2, "pool of %u, n=%zu: sum %zu", pool.size(), n, sum);
    CHECK(parts == (expect_serial ? 1u : pool.size()), "pool of %u, n=%zu: %u parts ran", pool.size(), n, parts);
}

static void test_pool()
{
    for (unsigned threads : {1u, 2u, 4u}) { Pool idle(threads); }  // no job at all
    for (unsigned threads : {2u, 4u}) {
        Pool pool(threads);
        for (int i = 0; i < 3000; i++) pool_sum(pool, 4096 + (size_t)(i % 7), 2048, false);  // back to back: workers spinning
        for (size_t n : {0, 1, 2047}) pool_sum(pool, n, 2048, true);                         // below serial_below
        pool_sum(pool, 2048, 2048, false);
        pool_sum(pool, 8191, 8192, true);
        pool_sum(pool, 8192, 8192, false);
        pool_sum(pool, 3, 2, false);  // (classify's per-ray loops)
        pool_sum(pool, 1, 2, true);
        for (int i = 0; i < 8; i++) {  // workers parked on the condition variable
            sleep_ms(20);
            pool_sum(pool, 5000, 2048, false);
            pool_sum(pool, 5001, 2048, false);
        }
        run_parts(&pool, 4096, [](size_t, size_t, unsigned) {});
        run_parts(static_cast<Pool *>(nullptr), 4096, [](size_t, size_t, unsigned) {});
    }
    Pool one(1);
    pool_sum(one, 100000, 2048, true);
}

static void test_deferred()
{
    { Deferred idle; }  // no job ever submitted
    {
        Deferred d;
        CHECK(d.join() == LOM_OK, "join with nothing submitted");
        CHECK(d.join() == LOM_OK, "join with nothing submitted, again");
    }
    Deferred d;
    int ran = 0;  // written by the jobs, read after the join: the join orders them
    for (int i = 0; i < 1000; i++) {
        const int code = (i & 1) ? LOM_ERR_HIP : LOM_OK;
        d.submit([&ran, code] { ran++; return code; });
        CHECK(d.join() == code, "pair %d: its code", i);
        CHECK(ran == i + 1, "pair %d: the job ran once", i);
        CHECK(d.join() == LOM_OK, "pair %d: the code is handed out once", i);
    }
    for (int i = 0; i < 8; i++) {  // the helper asleep on the condition variable
        sleep_ms(20);
        const int code = (i & 1) ? LOM_OK : LOM_ERR_RANGE;
        d.submit([&ran, code] { ran++; return code; });
        CHECK(d.join() == code, "pair %d after a sleep: its code", i);
        CHECK(d.join() == LOM_OK, "pair %d after a sleep: handed out once", i);
    }
    CHECK(ran == 1008, "%d jobs ran", ran);
    d.submit([] { return LOM_ERR_OOM; });
    CHECK(d.join() == LOM_ERR_OOM, "last job");
}   // destroyed directly after a join

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "stages" && argc > 2) {
        std::vector<lom_point_xyzirt> frame;
        FILE *f = std::fopen(argv[2], "rb");
        if (!f) {
            std::printf("cannot open %s\n", argv[2]);
            return 2;
        }
        lom_point_xyzirt rec;
        while (std::fread(&rec, sizeof rec, 1, f) == 1) frame.push_back(rec);
        std::fclose(f);
        CHECK(frame.size() > 20000, "frame of %zu points", frame.size());
        test_pooled_against_serial(frame);
        test_decoder();
    } else if (mode == "threads") {
        test_pool();
        test_deferred();
    } else {
        std::printf("usage: test_host_stages stages <frame.bin> | threads\n");
        return 2;
    }
    return check_done();
}
