// Host side of the pose graph: argument checks, the 6x6 Cholesky of an edge's information, the union-find gauge check,
// the CSR of incident edges and the LM policy.  Plain C++, no HIP: graph.hip calls these, and the stateless ones are part
// of the C ABI (lom_graph_check_gauge, lom_graph_lm_policy, lom_graph_information_from_quality).
#include "graph_host.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

namespace lom {
namespace graph {

bool cholesky6_upper(const double omega[36], double U[21])
{
    for (int i = 0; i < 36; i++)
        if (!std::isfinite(omega[i])) return false;
    double L[6][6] = {};
    for (int j = 0; j < 6; j++) {
        double d = omega[j * 6 + j];
        for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        L[j][j] = std::sqrt(d);
        for (int i = j + 1; i < 6; i++) {
            double v = omega[j * 6 + i];  // upper triangle
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k];
            L[i][j] = v / L[j][j];
            if (!std::isfinite(L[i][j])) return false;
        }
    }
    int k = 0;
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) U[k++] = L[c][r];
    return true;
}

int check_gauge(int64_t n_nodes, const int32_t *fixed, int64_t n_edges, const int32_t *ij, int64_t *bad_node)
{
    if (bad_node) *bad_node = -1;
    if (n_nodes < 0 || n_edges < 0 || (n_nodes > 0 && !fixed) || (n_edges > 0 && !ij)) return LOM_ERR_ARG;
    for (int64_t e = 0; e < n_edges; e++) {
        const int64_t i = ij[2 * e], j = ij[2 * e + 1];
        if (i == j || i < 0 || j < 0 || i >= n_nodes || j >= n_nodes) return LOM_ERR_ARG;
    }
    std::vector<int64_t> parent((size_t)n_nodes);
    std::iota(parent.begin(), parent.end(), (int64_t)0);
    auto find = [&](int64_t a) {
        while (parent[(size_t)a] != a) {
            parent[(size_t)a] = parent[(size_t)parent[(size_t)a]];  // path halving
            a = parent[(size_t)a];
        }
        return a;
    };
    for (int64_t e = 0; e < n_edges; e++) {
        const int64_t a = find(ij[2 * e]), b = find(ij[2 * e + 1]);
        if (a != b) parent[(size_t)std::max(a, b)] = std::min(a, b);  // the root is the component's smallest id
    }
    std::vector<char> anchored((size_t)n_nodes, 0);
    for (int64_t k = 0; k < n_nodes; k++)
        if (fixed[k]) anchored[(size_t)find(k)] = 1;
    for (int64_t k = 0; k < n_nodes; k++)
        if (!fixed[k] && !anchored[(size_t)find(k)]) {
            if (bad_node) *bad_node = k;
            return LOM_ERR_ARG;
        }
    return LOM_OK;
}

void build_csr(int64_t n_nodes, int64_t n_edges, const int32_t *ij, std::vector<uint32_t> &row_ptr,
               std::vector<uint32_t> &entries)
{
    row_ptr.assign((size_t)n_nodes + 1, 0u);
    entries.assign((size_t)n_edges * 2, 0u);
    for (int64_t e = 0; e < n_edges; e++) {
        row_ptr[(size_t)ij[2 * e] + 1]++;
        row_ptr[(size_t)ij[2 * e + 1] + 1]++;
    }
    for (int64_t k = 0; k < n_nodes; k++) row_ptr[(size_t)k + 1] += row_ptr[(size_t)k];
    std::vector<uint32_t> at(row_ptr.begin(), row_ptr.end() - 1);
    for (int64_t e = 0; e < n_edges; e++)  // ascending edge id per node by construction
        for (int side = 0; side < 2; side++) entries[at[(size_t)ij[2 * e + side]]++] = (uint32_t)(e * 2 + side);
}

bool params_ok(const lom_graph_params *p)
{
    if (!p) return false;
    for (double v : {p->lambda0, p->gtol, p->xtol, p->pcg_rtol})
        if (!std::isfinite(v) || !(v > 0.0)) return false;
    return p->max_outer > 0 && p->max_pcg > 0;
}

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

void normalised(const lom_graph_pose *in, double out[7])
{
    double n2 = 0.0;
    for (int a = 0; a < 4; a++) n2 += in->q_wxyz[a] * in->q_wxyz[a];
    const double n = std::sqrt(n2);
    for (int a = 0; a < 3; a++) out[a] = in->t[a];
    for (int a = 0; a < 4; a++) out[3 + a] = in->q_wxyz[a] / n;
}

}  // namespace graph
}  // namespace lom

extern "C" {

int lom_graph_check_gauge(int64_t n_nodes, const int32_t *fixed, int64_t n_edges, const int32_t *ij, int64_t *bad_node)
{
    return lom::graph::check_gauge(n_nodes, fixed, n_edges, ij, bad_node);
}

int lom_graph_lm_policy(double cost, double cost_new, double denom, double *lambda, double *nu, double *rho_gain_out)
{
    if (!lambda || !nu) return LOM_ERR_ARG;
    const double rho_gain = (cost - cost_new) / (0.5 * denom);
    if (rho_gain_out) *rho_gain_out = rho_gain;
    if (rho_gain > 0.0) {  // false for NaN
        const double t = 2.0 * rho_gain - 1.0;
        *lambda *= std::max(1.0 / 3.0, 1.0 - t * t * t);
        *nu = 2.0;
        return 1;
    }
    *lambda *= *nu;
    *nu *= 2.0;
    return 0;
}

int lom_graph_information_from_quality(const lom_quality_report *report, int with_prior, double omega_out[36])
{
    if (!report || !omega_out || report->valid < 7) return LOM_ERR_ARG;
    static const double scale[6] = {0.5, 0.5, 0.5, 1.0, 1.0, 1.0};
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) {
            double h = report->information[a * 6 + b];
            if (with_prior && a == b && a >= 3) h += 100.0;
            omega_out[a * 6 + b] = scale[a] * h * scale[b];
        }
    return LOM_OK;
}

int lom_graph_pose_from_f32(const lom_pose *in, lom_graph_pose *out)
{
    if (!in || !out) return LOM_ERR_ARG;
    for (int a = 0; a < 3; a++) out->t[a] = (double)in->t[a];
    for (int a = 0; a < 4; a++) out->q_wxyz[a] = (double)in->q[a];
    return LOM_OK;
}

int lom_graph_pose_to_f32(const lom_graph_pose *in, lom_pose *out)
{
    if (!in || !out) return LOM_ERR_ARG;
    for (int a = 0; a < 3; a++) out->t[a] = (float)in->t[a];
    for (int a = 0; a < 4; a++) out->q[a] = (float)in->q_wxyz[a];
    return LOM_OK;
}

}  // extern "C"
