// Host side of the pose graph (graph_host.cpp), shared with graph.hip.  Plain C++: nothing here needs a device.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/lidar_odometry_amd.h"

namespace lom {
namespace graph {

// Omega = U^T U of a symmetric 6x6 (the upper triangle is read): U's upper triangle row-major, 21 values.  False where a
// value of omega is not finite or a pivot is not positive.
bool cholesky6_upper(const double omega[36], double U[21]);

// Union-find over the edges: every connected component must hold a fixed node.  Returns LOM_OK, or LOM_ERR_ARG with
// *bad_node the smallest free node of the first component without one (-1 where an edge itself is bad: i == j or an id
// outside [0, n_nodes)).
int check_gauge(int64_t n_nodes, const int32_t *fixed, int64_t n_edges, const int32_t *ij, int64_t *bad_node);

// Incident edges per node, ascending edge id: row_ptr[n_nodes + 1], entries[2 * n_edges] = edge * 2 + side (0: the node is
// the edge's i, 1: its j).
void build_csr(int64_t n_nodes, int64_t n_edges, const int32_t *ij, std::vector<uint32_t> &row_ptr,
               std::vector<uint32_t> &entries);

bool params_ok(const lom_graph_params *p);
bool pose_ok(const lom_graph_pose *p);             // finite, quaternion of non-zero length
void normalised(const lom_graph_pose *in, double out[7]);  // t, then q / |q|

}  // namespace graph
}  // namespace lom
