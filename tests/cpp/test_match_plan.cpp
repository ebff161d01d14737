// The matcher's launch planning (csrc/match_plan.cpp) compiled into a program of its own under
// -fsanitize=address,undefined (tests/test_match_plan_cpp.py): the grids and k_lm shapes at their edges, the block layout,
// and the rounds of the batched align and of the batched quality report -- each planner against a restatement of its
// definition written here the slow and obvious way, and against the properties its callers rely on (a round of the
// align is resident at once, no two blocks of a quality round overlap), on fixed cases and on seeded random calls.
#include <algorithm>
#include <cstdio>
#include <random>
#include <tuple>
#include <vector>

#include "check.hpp"
#include "match_plan.hpp"

using namespace lom;

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

// ---- the batched align ------------------------------------------------------------------------------------------------
// the shape by its thresholds in points
static LmShape shape_of(uint32_t n) { return n <= 16384 ? kLmSmall : n <= 32768 ? kLmSmall2 : n <= 65536 ? kLmMid : kLmBig; }
using Key = std::tuple<int, bool, bool>;
static Key key_of(const AlignPlanProblem &p) { return Key{(int)shape_of(p.n), p.counted, p.temporal}; }

// the definition: the distinct keys in order of first appearance; a key's problems in call order; a round closes when it
// is full or the next problem carries a give-up test
static AlignPlan expected_align(const std::vector<AlignPlanProblem> &p, uint32_t cus, const uint32_t per_cu[4], int round_max)
{
    AlignPlan out;
    std::vector<Key> keys;
    for (const AlignPlanProblem &q : p)
        if (std::find(keys.begin(), keys.end(), key_of(q)) == keys.end()) keys.push_back(key_of(q));
    for (const Key &key : keys) {
        std::vector<int> members;
        uint32_t nb_max = 0;
        for (size_t i = 0; i < p.size(); i++)
            if (key_of(p[i]) == key) {
                members.push_back((int)i);
                nb_max = std::max(nb_max, p[i].nb);
            }
        size_t full = cus * per_cu[std::get<0>(key)] / nb_max;
        if (full < 1) full = 1;
        if (round_max > 0 && full > (size_t)round_max) full = (size_t)round_max;
        for (int i : members) {
            const bool opens = out.rounds.empty() || key_of(p[out.order[out.rounds.back().first]]) != key ||
                               (size_t)out.rounds.back().size == full || p[i].give_up_outer >= 0;
            if (opens)
                out.rounds.push_back(AlignRound{(int)out.order.size(), 0, (LmShape)std::get<0>(key), 0u, std::get<1>(key),
                                                std::get<2>(key), p[i].give_up_outer});
            AlignRound &R = out.rounds.back();
            R.size++;
            R.nb = std::max(R.nb, p[i].nb);
            out.order.push_back(i);
        }
    }
    return out;
}

static void check_align(const std::vector<AlignPlanProblem> &p, uint32_t cus, const uint32_t per_cu[4], int round_max)
{
    const int K = (int)p.size();
    AlignPlan got;
    got.order.assign(3, 7);  // (stale contents: the planner starts from nothing)
    plan_align_rounds(p.data(), K, cus, per_cu, round_max, got);
    const AlignPlan want = expected_align(p, cus, per_cu, round_max);
    CHECK(got.order == want.order);
    CHECK(got.rounds.size() == want.rounds.size());
    for (size_t r = 0; r < got.rounds.size() && r < want.rounds.size(); r++) {
        const AlignRound &a = got.rounds[r], &b = want.rounds[r];
        CHECK(a.first == b.first && a.size == b.size && a.shape == b.shape && a.nb == b.nb && a.counted == b.counted &&
              a.temporal == b.temporal && a.give_up_outer == b.give_up_outer);
    }
    // order is a permutation of 0..K-1, and the rounds tile it
    std::vector<int> sorted = got.order;
    std::sort(sorted.begin(), sorted.end());
    CHECK((int)sorted.size() == K);
    for (int i = 0; i < K && i < (int)sorted.size(); i++) CHECK(sorted[i] == i);
    if ((int)got.order.size() != K) return;
    int at = 0;
    std::vector<Key> seen;  // the groups so far, in the order their first round came
    int last_first_member = -1;
    for (const AlignRound &R : got.rounds) {
        CHECK(R.first == at && R.size >= 1 && R.first + R.size <= K);
        if (R.first != at || R.size < 1 || R.first + R.size > K) return;
        at += R.size;
        const Key key{(int)R.shape, R.counted, R.temporal};
        uint32_t nb = 0, group_nb = 0;
        for (int k = 0; k < R.size; k++) {
            const AlignPlanProblem &q = p[got.order[R.first + k]];
            CHECK(key_of(q) == key);  // homogeneous in (shape, counted, temporal)
            nb = std::max(nb, q.nb);
            // a give-up test is carried by member 0 alone, and the round carries its value
            if (k == 0) CHECK(R.give_up_outer == q.give_up_outer);
            else CHECK(q.give_up_outer < 0);
            if (k > 0) CHECK(got.order[R.first + k] > got.order[R.first + k - 1]);  // call order
        }
        CHECK(R.nb == nb);
        for (const AlignPlanProblem &q : p)
            if (key_of(q) == key) group_nb = std::max(group_nb, q.nb);
        // resident at once: counted with the group's largest grid
        CHECK(R.size == 1 || (uint64_t)R.size * group_nb <= (uint64_t)cus * per_cu[R.shape]);
        if (round_max > 0) CHECK(R.size <= round_max);
        // groups in order of first appearance, each in one run of rounds, its problems in call order
        if (seen.empty() || seen.back() != key) {
            CHECK(std::find(seen.begin(), seen.end(), key) == seen.end());
            seen.push_back(key);
            int first_member = 0;
            while (key_of(p[first_member]) != key) first_member++;
            CHECK(got.order[R.first] == first_member && first_member > last_first_member);
            last_first_member = first_member;
        } else {
            CHECK(got.order[R.first] > got.order[R.first - 1]);
        }
    }
    CHECK(at == K);
}

// ---- the batched quality report ---------------------------------------------------------------------------------------
struct QualSizes {
    uint32_t mb, nb;
    size_t rec, cnt, part;  // bytes in use, not rounded
};
static QualSizes sizes_of(uint32_t n, uint32_t partition_cus)
{
    QualSizes s;
    s.mb = std::max(1u, std::min((n + 15u) / 16u, partition_cus ? partition_cus * 7u : 1792u));
    s.nb = std::max(1u, std::min((n + 511u) / 512u, 64u));
    s.rec = (size_t)n * 48;
    s.cnt = (size_t)s.mb * 16;
    s.part = (size_t)s.nb * 36 * 8;
    return s;
}

static void check_quality(const std::vector<uint32_t> &n, uint32_t partition_cus, int round_max, QualPlan *keep = nullptr)
{
    const int K = (int)n.size();
    const size_t budget = (size_t)64 << 20;
    QualPlan got;
    got.rec_bytes = 99;  // (stale contents: the planner starts from nothing)
    got.rounds.push_back(QualRound{5, 5, 5u, 5u});
    plan_quality_rounds(n.data(), K, partition_cus, round_max, got);
    CHECK((int)got.problems.size() == K);
    if ((int)got.problems.size() != K) return;
    std::vector<QualSizes> s(K);
    for (int j = 0; j < K; j++) {
        s[j] = sizes_of(n[j], partition_cus);
        CHECK(got.problems[j].mb == s[j].mb && got.problems[j].nb == s[j].nb);
        CHECK(got.problems[j].mb == match_grid(n[j], partition_cus) && got.problems[j].nb == eval_grid(n[j]));
    }
    // the definition: a problem joins the open round if that stays within the cap and the budget; its offsets are the sums
    // of the rounded blocks of the members before it
    const int cap = round_max > 0 ? std::min(round_max, 32768) : 32768;
    std::vector<std::vector<int>> want(1);
    for (int j = 0; j < K; j++) {
        size_t total = up256(s[j].rec) + up256(s[j].cnt) + up256(s[j].part);
        for (int i : want.back()) total += up256(s[i].rec) + up256(s[i].cnt) + up256(s[i].part);
        if (!want.back().empty() && ((int)want.back().size() >= cap || total > budget)) want.push_back({});
        want.back().push_back(j);
    }
    if (K == 0) want.clear();
    CHECK(got.rounds.size() == want.size());
    if (got.rounds.size() != want.size()) return;
    size_t rec_max = 0, cnt_max = 0, part_max = 0;
    int at = 0;
    for (size_t r = 0; r < want.size(); r++) {
        const QualRound &R = got.rounds[r];
        // consecutive, every problem once, call order
        CHECK(R.first == at && R.size == (int)want[r].size() && R.first == want[r][0]);
        if (R.first != at || R.size != (int)want[r].size()) return;
        at += R.size;
        CHECK(R.size >= 1 && R.size <= cap);
        uint32_t mb = 0, nb = 0;
        size_t rec = 0, cnt = 0, part = 0;
        for (int j : want[r]) {
            const QualPlanProblem &q = got.problems[j];
            mb = std::max(mb, s[j].mb);
            nb = std::max(nb, s[j].nb);
            CHECK(q.off_rec == rec && q.off_cnt == cnt && q.off_part == part);
            CHECK(q.off_rec % 256 == 0 && q.off_cnt % 256 == 0 && q.off_part % 256 == 0);
            // no two blocks of a buffer overlap: against every member before it
            for (int i = R.first; i < j; i++) {
                const QualPlanProblem &o = got.problems[i];
                CHECK(o.off_rec + s[i].rec <= q.off_rec && o.off_cnt + s[i].cnt <= q.off_cnt && o.off_part + s[i].part <= q.off_part);
            }
            rec += up256(s[j].rec);
            cnt += up256(s[j].cnt);
            part += up256(s[j].part);
        }
        CHECK(R.mb == mb && R.nb == nb);
        CHECK(R.size == 1 || rec + cnt + part <= budget);
        rec_max = std::max(rec_max, rec);
        cnt_max = std::max(cnt_max, cnt);
        part_max = std::max(part_max, part);
    }
    CHECK(at == K);
    // each buffer is the largest round's extent
    CHECK(got.rec_bytes == rec_max && got.cnt_bytes == cnt_max && got.part_bytes == part_max);
    if (keep) *keep = got;
}

int main()
{
    // ---- shapes and grids at their edges
    CHECK(lm_shape(0) == kLmSmall && lm_shape(1) == kLmSmall && lm_shape(16384) == kLmSmall);
    CHECK(lm_shape(16385) == kLmSmall2 && lm_shape(32768) == kLmSmall2);
    CHECK(lm_shape(32769) == kLmMid && lm_shape(65536) == kLmMid);
    CHECK(lm_shape(65537) == kLmBig && lm_shape(0x7FFFFFFEu) == kLmBig);
    const uint32_t edges[] = {0, 1, 16384, 16385, 32768, 32769, 65536, 65537};
    for (uint32_t n : edges) CHECK(lm_shape(n) == shape_of(n));
    CHECK(lm_blocks(0, kLmSmall, 256) == 1 && lm_blocks(1, kLmSmall, 256) == 1);
    CHECK(lm_blocks(256, kLmSmall, 256) == 1 && lm_blocks(257, kLmSmall, 256) == 2);
    CHECK(lm_blocks(16384, kLmSmall, 256) == 64);
    CHECK(lm_blocks(32768, kLmSmall2, 256) == 64);  // 128 capped
    CHECK(lm_blocks(65536, kLmMid, 256) == 64);     // 128 capped
    CHECK(lm_blocks(65537, kLmBig, 256) == 128);    // 129 capped
    CHECK(lm_blocks(16384, kLmSmall, 32) == 32 && lm_blocks(65537, kLmBig, 100) == 100);  // what is resident wins
    for (uint32_t n : edges)
        for (uint32_t limit : {1u, 8u, 64u, 512u}) {
            const LmShape sh = lm_shape(n);
            const uint32_t points = (sh == kLmSmall || sh == kLmSmall2) ? 256u : 512u, top = sh == kLmBig ? 128u : 64u;
            const uint32_t nb = lm_blocks(n, sh, limit);
            CHECK(nb >= 1 && nb == std::min(std::min(std::max(1u, (n + points - 1) / points), top), limit));
        }
    CHECK(match_grid(0) == 1 && match_grid(16) == 1 && match_grid(17) == 2);
    CHECK(match_grid(16 * 1792) == 1792 && match_grid(16 * 1792 + 1) == 1792 && match_grid(0x7FFFFFFEu) == 1792);
    CHECK(match_grid(16 * 224, 32) == 224 && match_grid(16 * 224 + 1, 32) == 224 && match_grid(17, 32) == 2 && match_grid(0, 32) == 1);
    CHECK(eval_grid(0) == 1 && eval_grid(512) == 1 && eval_grid(513) == 2 && eval_grid(512 * 64) == 64 && eval_grid(512 * 64 + 1) == 64 &&
          eval_grid(0x7FFFFFFEu) == 64);
    CHECK(round_up256(0) == 0 && round_up256(1) == 256 && round_up256(256) == 256 && round_up256(257) == 512);
    CHECK(stride_ok(12) && stride_ok(16) && !stride_ok(8) && !stride_ok(13) && scan_args_ok(0x7FFFFFFEull, 12) && !scan_args_ok(0x7FFFFFFFull, 12));
    {
        BlockLayout b;
        CHECK(b.take(1) == 0 && b.end == 1 && b.next == 256);
        CHECK(b.take(256) == 256 && b.end == 512 && b.next == 512);
        CHECK(b.take(0) == 512 && b.end == 512 && b.next == 512);
        CHECK(b.take(300) == 512 && b.end == 812 && b.next == 1024);
    }

    // ---- the batched align: fixed cases
    const uint32_t two[4] = {2, 2, 2, 2}, one[4] = {1, 1, 1, 1};
    {
        // 8 equal problems, three per round at most: rounds 0,0,0,1,1,1,2,2
        const std::vector<AlignPlanProblem> p(8, AlignPlanProblem{26600, 64, false, true, -1});
        AlignPlan a;
        plan_align_rounds(p.data(), 8, 256, one, 3, a);
        CHECK(a.rounds.size() == 3 && a.order == (std::vector<int>{0, 1, 2, 3, 4, 5, 6, 7}));
        if (a.rounds.size() == 3)
            CHECK(a.rounds[0].first == 0 && a.rounds[0].size == 3 && a.rounds[1].first == 3 && a.rounds[1].size == 3 &&
                  a.rounds[2].first == 6 && a.rounds[2].size == 2 && a.rounds[0].shape == kLmSmall2 && a.rounds[2].nb == 64);
        check_align(p, 256, one, 3);
        // without the cap: 256 compute units x 1 / 64 = four per round
        plan_align_rounds(p.data(), 8, 256, one, 0, a);
        CHECK(a.rounds.size() == 2 && a.rounds[0].size == 4 && a.rounds[1].size == 4);
        // fewer workgroups resident than one solve has: one problem per round
        plan_align_rounds(p.data(), 8, 8, two, 0, a);
        CHECK(a.rounds.size() == 8);
        for (const AlignRound &R : a.rounds) CHECK(R.size == 1);
        check_align(p, 8, two, 0);
    }
    {
        // small and small-two alternate: two groups, not four
        std::vector<AlignPlanProblem> p;
        for (int i = 0; i < 4; i++) p.push_back(AlignPlanProblem{(i & 1) ? 20000u : 10000u, (i & 1) ? 64u : 40u, false, true, -1});
        AlignPlan a;
        plan_align_rounds(p.data(), 4, 256, one, 0, a);
        CHECK(a.rounds.size() == 2 && a.order == (std::vector<int>{0, 2, 1, 3}));
        if (a.rounds.size() == 2) CHECK(a.rounds[0].shape == kLmSmall && a.rounds[0].nb == 40 && a.rounds[1].shape == kLmSmall2);
        check_align(p, 256, one, 0);
        // the give-up test of problem 2 opens a round of its group
        p[2].give_up_outer = 3;
        plan_align_rounds(p.data(), 4, 256, one, 0, a);
        CHECK(a.rounds.size() == 3 && a.order == (std::vector<int>{0, 2, 1, 3}));
        if (a.rounds.size() == 3) CHECK(a.rounds[0].give_up_outer == -1 && a.rounds[1].first == 1 && a.rounds[1].give_up_outer == 3);
        check_align(p, 256, one, 0);
        // the group's largest grid counts for residency, the round's own for its launch: grids 10, 10, 60 on 64 resident
        // workgroups run one per round, and the first two rounds launch 10
        p = {{1000, 10, false, true, -1}, {1000, 10, false, true, -1}, {15000, 60, false, true, -1}};
        plan_align_rounds(p.data(), 3, 64, one, 0, a);
        CHECK(a.rounds.size() == 3 && a.rounds[0].nb == 10 && a.rounds[1].nb == 10 && a.rounds[2].nb == 60);
        check_align(p, 64, one, 0);
    }
    {
        AlignPlan a;
        a.order.assign(2, 1);
        a.rounds.resize(2);
        plan_align_rounds(nullptr, 0, 256, one, 0, a);
        CHECK(a.order.empty() && a.rounds.empty());
    }
    // ---- the batched align: seeded random calls
    std::mt19937 rng(20240607u);
    auto pick = [&](uint32_t k) { return (uint32_t)(rng() % k); };
    const uint32_t cus_of[] = {8, 32, 256};
    const int align_caps[] = {0, 1, 3}, qual_caps[] = {0, 1, 3, 7};
    for (int call = 0; call < 400; call++) {
        const int K = (int)pick(41);
        const uint32_t cus = cus_of[pick(3)];
        const uint32_t per_cu[4] = {1 + pick(2), 1 + pick(2), 1 + pick(2), 1 + pick(2)};
        const int round_max = align_caps[pick(3)];
        const uint32_t limit = pick(3) ? cus * pick(3) + cus : 1000u;  // resident workgroups of the single form of k_lm
        const bool flags = pick(2), give_ups = pick(2);
        std::vector<AlignPlanProblem> p(K);
        for (AlignPlanProblem &q : p) {
            q.n = edges[pick(8)];
            q.nb = lm_blocks(q.n, lm_shape(q.n), limit);
            q.counted = flags && pick(2);
            q.temporal = !flags || pick(2);
            q.give_up_outer = give_ups && pick(4) == 0 ? (int)pick(6) : -1;
        }
        check_align(p, cus, per_cu, round_max);
    }

    // ---- the batched quality report
    check_quality({}, 0, 0);
    {
        // 48 n just above the budget: alone, whatever stands beside it
        QualPlan q;
        check_quality({1, 1398102, 1}, 0, 0, &q);
        CHECK(q.rounds.size() == 3 && q.rec_bytes == up256((size_t)1398102 * 48) && q.rec_bytes > ((size_t)64 << 20));
        check_quality({1398102, 1398102}, 0, 0, &q);
        CHECK(q.rounds.size() == 2);
        // two problems of 698,065 points are 2 x (130,888 + 112 + 72) x 256 bytes, the budget to the byte: one round; five
        // points more in one of them are 256 bytes more: two rounds
        check_quality({698065, 698065}, 0, 0, &q);
        CHECK(q.rounds.size() == 1 && q.rec_bytes + q.cnt_bytes + q.part_bytes == ((size_t)64 << 20));
        check_quality({698065, 698070}, 0, 0, &q);
        CHECK(q.rounds.size() == 2);
        // the cap of the tests
        check_quality(std::vector<uint32_t>(8, 100), 0, 3, &q);
        CHECK(q.rounds.size() == 3 && q.rounds[2].first == 6 && q.rounds[2].size == 2);
        // one workgroup record of 288 bytes takes 512, two take 768
        check_quality({512, 513, 1}, 0, 0, &q);
        CHECK(q.rounds.size() == 1 && q.problems[1].off_part == 512 && q.problems[2].off_part == 512 + 768 && q.part_bytes == 512 + 768 + 512);
        CHECK(q.problems[1].off_rec == up256(512 * 48) && q.problems[1].off_cnt == 512 && q.problems[2].off_cnt == 512 + up256(33 * 16));
    }
    {
        // how many problems fill a round: what the comment at kQualBatchBudgetBytes says
        QualPlan q;
        check_quality(std::vector<uint32_t>(100, 28800), 0, 0, &q);
        const int big = q.rounds.empty() ? 0 : q.rounds[0].size;
        check_quality(std::vector<uint32_t>(1500, 1900), 0, 0, &q);
        const int small = q.rounds.empty() ? 0 : q.rounds[0].size;
        std::printf("a round of the batched quality report holds %d problems of 28,800 points or %d of 1,900\n", big, small);
        CHECK(big == 47 && small == 708);
    }
    const uint32_t qn[] = {1, 15, 16, 17, 512, 513, 1900, 28800, 1398102};
    for (int call = 0; call < 300; call++) {
        const int K = (int)pick(41);
        const int round_max = qual_caps[pick(4)];
        const uint32_t partition_cus = pick(2) ? 32u : 0u;
        const uint32_t kinds = 1 + pick(9);  // (calls of small problems only as well)
        std::vector<uint32_t> n(K);
        for (uint32_t &v : n) v = qn[pick(kinds)];
        check_quality(n, partition_cus, round_max);
    }
    return check_done();
}
