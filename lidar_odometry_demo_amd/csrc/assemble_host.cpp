// Host planning of lom_map_assemble: validation of ids and poses, quaternion to rotation matrix, the offsets of every scan
// in the concatenated cloud, grid sizes.  Plain C++, no HIP: archive.hip calls these, and lom_graph_pose_rotation_matrix is
// part of the C ABI.  The kernels index points with 32 bits: a plan whose archive offsets reach 2^32 or whose call holds
// more than an insert takes is refused here, before any device work.  Below them, what the planners built on these
// descriptors share: the cut of a call into launches (vote, occupancy, elevation) and the start cells and first checks
// of the two 2-D grids.
#include "assemble_host.hpp"

#include <algorithm>
#include <cmath>

namespace lom {
namespace assemble {

bool pose_ok(const lom_graph_pose *p)
{
    if (!p) return false;
    double n2 = 0.0;
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(p->t[a])) return false;
    for (int a = 0; a < 4; a++) {
        if (!std::isfinite(p->q_wxyz[a])) return false;
        n2 += p->q_wxyz[a] * p->q_wxyz[a];
    }
    return std::isfinite(n2) && n2 > 0.0;
}

void normalised_quaternion(const lom_graph_pose *p, double q[4])
{
    double n2 = 0.0;
    for (int a = 0; a < 4; a++) n2 += p->q_wxyz[a] * p->q_wxyz[a];
    const double n = std::sqrt(n2);
    for (int a = 0; a < 4; a++) q[a] = p->q_wxyz[a] / n;
}

void rotation_matrix(const double q[4], double R[9])
{
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1.0 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1.0 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1.0 - (txx + tyy);
}

int plan(const ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count, Plan &out,
         std::string &why)
{
    out = Plan();
    if (count == 0) return LOM_OK;
    if (!ids || !poses || (n_scans && !table)) {
        why = "ids and poses must not be NULL";
        return LOM_ERR_ARG;
    }
    if (count > kAsmMaxScans) {
        why = "more than 2^24 scans in one call";
        return LOM_ERR_ARG;
    }
    // everything is checked before anything is kept
    uint64_t total = 0, blocks = 0;
    for (size_t k = 0; k < count; k++) {
        if (ids[k] < 0 || (uint64_t)ids[k] >= (uint64_t)n_scans) {
            why = "scan " + std::to_string(k) + " of the call: no scan with this id";
            return LOM_ERR_ARG;
        }
        if (!pose_ok(poses + k)) {
            why = "scan " + std::to_string(k) + " of the call: a pose is not finite or its quaternion is zero";
            return LOM_ERR_ARG;
        }
        const ScanEntry &e = table[(size_t)ids[k]];
        if (e.n && e.offset + e.n > kArchiveMaxPoints) {
            why = "scan " + std::to_string(k) + " of the call lies beyond 2^32 points of the archive (32-bit indices)";
            return LOM_ERR_ARG;
        }
        total += e.n;
        blocks += (e.n + kAsmThreads - 1) / kAsmThreads;
        if (total > kAsmMaxPoints) {
            why = "more than 2^31 - 2 points in one call (32-bit indices)";
            return LOM_ERR_ARG;
        }
    }
    out.scans.resize(count);
    uint32_t at = 0, blk = 0;
    for (size_t k = 0; k < count; k++) {
        const ScanEntry &e = table[(size_t)ids[k]];
        AsmScan &d = out.scans[k];
        d.src = e.n ? (uint32_t)e.offset : 0u;
        d.n = e.n;
        d.out = at;
        d.blk = blk;
        double q[4];
        normalised_quaternion(poses + k, q);
        rotation_matrix(q, d.R);
        for (int a = 0; a < 3; a++) d.t[a] = poses[k].t[a];
        at += e.n;
        blk += (e.n + kAsmThreads - 1) / kAsmThreads;
        if (e.n > out.max_n) out.max_n = e.n;
    }
    out.points_in = total;
    out.blocks = (uint32_t)blocks;
    out.grid_x = (out.max_n + kAsmThreads - 1) / kAsmThreads;
    return LOM_OK;
}

int cull_of(const lom_assemble_params *p, bool *cull, std::string &why)
{
    *cull = false;
    if (!p) return LOM_OK;
    if (!std::isfinite(p->radius) || !std::isfinite(p->centre[0]) || !std::isfinite(p->centre[1]) ||
        !std::isfinite(p->centre[2])) {
        why = "centre and radius must be finite";
        return LOM_ERR_ARG;
    }
    *cull = p->radius > 0.0f;
    return LOM_OK;
}

std::vector<Launch> cut_launches(const Plan &plan, uint32_t per)
{
    std::vector<Launch> out;
    const size_t count = plan.scans.size();
    for (size_t first = 0; first < count; first += per) {
        Launch l;
        l.first = (uint32_t)first;
        l.count = (uint32_t)std::min<size_t>(per, count - first);
        l.max_n = 0;
        for (uint32_t k = 0; k < l.count; k++) l.max_n = std::max(l.max_n, plan.scans[first + k].n);
        l.grid_x = (l.max_n + kAsmThreads - 1) / kAsmThreads;
        if (l.max_n) out.push_back(l);
    }
    return out;
}

int plan_on_grid(const ScanEntry *table, size_t n_scans, const int64_t *ids, const lom_graph_pose *poses, size_t count,
                 const GridFrame &frame, bool params_ok, const char *params_why, Plan &out,
                 std::vector<int32_t> &cells, std::string &why)
{
    cells.clear();
    int rc = plan(table, n_scans, ids, poses, count, out, why);
    if (rc == LOM_OK && !params_ok) {
        why = params_why;
        rc = LOM_ERR_ARG;
    }
    if (rc == LOM_OK) cells.resize(count * 2);
    for (size_t k = 0; k < count && rc == LOM_OK; k++)
        if (!origin_cell(out.scans[k], frame, &cells[k * 2])) {
            why = "origin of scan " + std::to_string(k) + " of the call: its cell is beyond 2^30 or not finite";
            rc = LOM_ERR_RANGE;
        }
    if (rc != LOM_OK) {
        out = Plan();
        cells.clear();
    }
    return rc;
}

}  // namespace assemble
}  // namespace lom

extern "C" {

int lom_graph_pose_rotation_matrix(const lom_graph_pose *pose, double R[9])
{
    if (!pose || !R || !lom::assemble::pose_ok(pose)) return LOM_ERR_ARG;
    double q[4];
    lom::assemble::normalised_quaternion(pose, q);
    lom::assemble::rotation_matrix(q, R);
    return LOM_OK;
}

}  // extern "C"
