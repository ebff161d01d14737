// Launch planning of the matcher: the grids and k_lm shapes of a scan, the rounds of the batched align and of the batched
// quality report.  Plain C++, no HIP: match.hip, align.hip, align_batch.hip and quality_report.hip call these, and
// tests/cpp/test_match_plan.cpp compiles this file alone.
#include "match_plan.hpp"

#include <algorithm>

namespace lom {

uint32_t match_grid(uint32_t n, uint32_t partition_cus)
{
    const uint32_t per_block = (uint32_t)(kMatchThreads / kMatchG);
    const uint32_t need = (n + per_block - 1) / per_block;
    const uint32_t cap = partition_cus ? partition_cus * (uint32_t)kMatchMinWaves : kMaxMatchBlocks;
    return std::max(1u, std::min(need, cap));
}

uint32_t eval_grid(uint32_t n)
{
    const uint32_t need = (n + kEvalThreads - 1) / kEvalThreads;
    return std::max(1u, std::min(need, kMaxEvalBlocks));
}

// k_lm's workgroup size: 256 threads for clouds that 64 such workgroups cover with one point per lane (<= 16,384 points) or
// with TWO points per lane, both in registers for the whole solve (<= 32,768: the VLP16 scan of C2), else 512:
// the wave-level reduction is bound by the CU's f64 issue rate, and four waves -- one per SIMD -- are through it
// in half the time of eight; the final sum adds 8 partial sums instead of 16; two register points per lane are
// accumulated stage by stage so that their independent chains interleave (1.4k cycles for the two against 0.95k for
// one).  C2 (profiles/r03_*): k_lm 18.9 -> 17.8 us per launch against 512 threads with one point per lane; eight
// points per lane (C3 on 64 workgroups of 256) lose: 24.4-25.5 against 22.4 us.
// Clouds beyond what 64 workgroups of 512 cover with two points per lane (C3, C4 on one GPU) take up to 128 workgroups:
// the accumulation halves, the gather reads twice as many records (on C2-sized clouds that trade loses).
LmShape lm_shape(uint32_t n)
{
    if (n <= kMaxLmBlocks * kLmSmallThreads) return kLmSmall;
    if (n <= 2u * kMaxLmBlocks * kLmSmallThreads) return kLmSmall2;  // 256 threads, two points per lane in registers
    // (for C3's 124k points 128 workgroups of 256 threads with four points per lane in registers -- no point re-read
    // per evaluation -- measured the same as 512 threads with one: align 0.2315-0.2324 against 0.2314-0.2335 ms on one
    // box; eight per lane for C4's 248k points lose, 0.448 against 0.343 ms: AGPR spills, eight points in a row)
    return n <= 2u * kMaxLmBlocks * (uint32_t)kEvalThreads ? kLmMid : kLmBig;
}

uint32_t lm_blocks(uint32_t n, LmShape shape, uint32_t resident_limit)
{
    const LmGeometry &f = kLmGeometry[shape];
    return std::min(std::min(std::max(1u, (n + f.points - 1) / f.points), f.cap), resident_limit);
}

void plan_align_rounds(const AlignPlanProblem *p, int count, uint32_t cus, const uint32_t per_cu[4], int round_max,
                       AlignPlan &out)
{
    out.order.clear();
    out.rounds.clear();
    std::vector<char> taken(count > 0 ? count : 0, 0);
    for (int i = 0; i < count; i++) {
        if (taken[i]) continue;
        const LmShape shape = lm_shape(p[i].n);
        std::vector<int> members;
        uint32_t nb_max = 0;
        for (int k = i; k < count; k++)
            if (!taken[k] && lm_shape(p[k].n) == shape && p[k].counted == p[i].counted && p[k].temporal == p[i].temporal) {
                taken[k] = 1;
                members.push_back(k);
                nb_max = std::max(nb_max, p[k].nb);
            }
        // (a round's launch is sized for its largest grid: residency is counted with the group's largest)
        int per_round = (int)std::max(1u, cus * per_cu[shape] / nb_max);
        if (round_max > 0) per_round = std::min(per_round, round_max);
        // a problem that carries a give-up test opens a round (the kernel applies it to problem 0 of a launch)
        for (size_t a = 0; a < members.size();) {
            size_t size = 1;
            while (a + size < members.size() && size < (size_t)per_round && p[members[a + size]].give_up_outer < 0) size++;
            uint32_t grid = 0;
            for (size_t k = 0; k < size; k++) grid = std::max(grid, p[members[a + k]].nb);
            out.rounds.push_back(AlignRound{(int)out.order.size(), (int)size, shape, grid, p[i].counted, p[i].temporal,
                                            p[members[a]].give_up_outer});
            for (size_t k = 0; k < size; k++) out.order.push_back(members[a + k]);
            a += size;
        }
    }
}

void plan_quality_rounds(const uint32_t *n, int count, uint32_t partition_cus, int round_max, QualPlan &out)
{
    out = QualPlan();
    out.problems.resize(count > 0 ? count : 0);
    const int cap = round_max > 0 ? std::min(round_max, kQualBatchRoundCap) : kQualBatchRoundCap;
    BlockLayout rec, cnt, part;  // of the round that is open
    for (int j = 0; j < count; j++) {
        QualPlanProblem &q = out.problems[j];
        q.mb = match_grid(n[j], partition_cus);
        q.nb = eval_grid(n[j]);
        const size_t b_rec = (size_t)n[j] * kMatchRecBytes, b_cnt = (size_t)q.mb * kMatchCounterBytes,
                     b_part = (size_t)q.nb * kQualPartBytes;
        const bool open = !out.rounds.empty() && out.rounds.back().size < cap &&
                          rec.next + cnt.next + part.next + round_up256(b_rec) + round_up256(b_cnt) + round_up256(b_part) <=
                              kQualBatchBudgetBytes;
        if (!open) {
            out.rounds.push_back(QualRound{j, 0, 0u, 0u});
            rec = cnt = part = BlockLayout();
        }
        QualRound &R = out.rounds.back();
        R.size++;
        R.mb = std::max(R.mb, q.mb);
        R.nb = std::max(R.nb, q.nb);
        q.off_rec = rec.take(b_rec);
        q.off_cnt = cnt.take(b_cnt);
        q.off_part = part.take(b_part);
        out.rec_bytes = std::max(out.rec_bytes, rec.next);
        out.cnt_bytes = std::max(out.cnt_bytes, cnt.next);
        out.part_bytes = std::max(out.part_bytes, part.next);
    }
}

}  // namespace lom
