// Superpixel k-NN graphs of a batch of point sets, and the sort_eig column choice: what the reference's superpixel loader does per graph on the CPU.
//
// knn_kernel replaces sigma, compute_adjacency_matrix_images and compute_edges_list (data/superpixels.py:17-69) and the self-edge removal of
// SuperPixDGL._prepare (:139-145).  One workgroup of four waves per graph, all arithmetic in fp64, the operations in the reference's order
// (the library is built with -ffp-contract=off: no product is fused into a sum):
//
//   stage     the graph's coordinates and features go to LDS, features channel-major
//   phase 1   a wave per row i: d_c(i, j) = sqrt((x_i - x_j)^2 + (y_i - y_j)^2), d_f likewise over the channels in ascending order; lane l holds
//             the columns l, l + 64, l + 128, l + 192 in registers (indexed by unrolled constants: no scratch).  For n >= k + 1 the k + 1 smallest
//             entries of the row, its zero diagonal included, are taken by k + 1 rounds of a wave-wide arg-min and summed in that (ascending)
//             order: sigma(i) = sum / k + 1e-8.  Otherwise sigma(i) = 1 + 1e-8 (sigma()'s ValueError branch).  sigma_c, sigma_f -> LDS | barrier
//   phase 2   a wave per row i: the distances again, E(i, j) = exp(-(d_c / sigma_c(i))^2 - (d_f / sigma_f(i))^2), A(i, j) = (E(i, j) + E(j, i)) / 2,
//             then the neighbour rule:
//               n >= k + 2       the n - 1 other nodes ranked by A descending, equal values by lower column first, through rounds of a wave-wide
//                                arg-max; skip_nearest: ranks 1 .. k are emitted (rank 0, the most similar node, is left out -- what the
//                                reference's np.argpartition(A, n - 10)[:, n - 9:-1] keeps), else ranks 0 .. k - 1; k edges per node in rank order
//               2 <= n <= k + 1  every j != i in ascending j, n - 1 edges per node
//               n == 1           one self-loop of value 0
//             edge edge_off[g] + i * per_node + slot: src = n0 + i (the row is the sender, g.add_edges(src, dsts)), dst = n0 + j, value = (float) A(i, j)
//
// Every reduction has a shape fixed by n alone, so a graph's output bits do not depend on the batch.  Node and edge ranges are checked against
// the arrays before anything is read or written; a column index only ever selects a register or an LDS cell below n.  A value of A that is not
// a number >= 0 (non-finite input) ranks as 0, so every emitted dst is a node of the graph.
//
// LDS: 2 + 8 coordinate / feature columns and two sigma columns of 256 doubles: 24 576 bytes, static.
//
// sort_eig_kernel replaces sort_eig / get_scores (data/superpixels.py:371-420): a wave per graph, the four scores as integer counts through
// __ballot; hor1 or ver2 the maximum: the rows stay, otherwise column 1 is overwritten with column 2 in place -- what the reference's
// exchanging arms leave behind (see the kernel), pinned by fixture G15.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dgn_common.hpp"

namespace dgn {
namespace superpixels {

constexpr int kMaxNodes = 256;
constexpr int kMaxK = 32;
constexpr int kMaxFeat = 8;
constexpr int kGroups = kMaxNodes / kWave;   // 64-column groups a lane holds one column of each
constexpr int kWaves = 4;
constexpr int kThreads = kWaves * kWave;
constexpr int kNoCol = 0x7fffffff;

struct Args {
    const double* coord;
    const double* feat;
    int n_feat;
    int64_t n_nodes;
    const int64_t* graph_off;
    const int64_t* edge_off;
    int k, skip;
    int64_t n_edges;
    int64_t* src;
    int64_t* dst;
    float* value;
    int32_t* status;
};

// the wave's best (value, column) on every lane: smallest / largest value, equal values by lower column.  The order is total, so all lanes agree.
template <bool MAX>
__device__ __forceinline__ void wave_pick(double& v, int& col) {
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const double ov = shfl_xor_d(v, o);
        const int oc = __shfl_xor(col, o, kWave);
        const bool take = (MAX ? ov > v : ov < v) || (ov == v && oc < col);
        if (take) { v = ov; col = oc; }
    }
}

// sum of the k + 1 smallest of the row held in v (columns >= n: +inf), in ascending order; v is consumed
__device__ __forceinline__ double smallest_sum(double (&v)[kGroups], int n, int k) {
    const int lane = lane_id();
    double s = 0.0;
    for (int r = 0; r <= k; ++r) {
        double bv = __builtin_inf();
        int bc = kNoCol;
#pragma unroll
        for (int c = 0; c < kGroups; ++c)
            if (c * kWave < n && v[c] < bv) { bv = v[c]; bc = c * kWave + lane; }
        wave_pick<false>(bv, bc);
        s += bv;
#pragma unroll
        for (int c = 0; c < kGroups; ++c)
            if (bc == c * kWave + lane) v[c] = __builtin_inf();
    }
    return s;
}

__global__ __launch_bounds__(kThreads) void knn_kernel(Args a) {
    __shared__ double s_x[kMaxNodes], s_y[kMaxNodes], s_f[kMaxFeat * kMaxNodes], s_sc[kMaxNodes], s_sf[kMaxNodes];
    const int g = blockIdx.x, tid = threadIdx.x, lane = lane_id(), wave = tid / kWave;
    const int64_t n0 = a.graph_off[g], n1 = a.graph_off[g + 1];
    if (n0 < 0 || n1 < n0 || n1 > a.n_nodes) {
        if (tid == 0) a.status[g] = -2;
        return;
    }
    if (n1 - n0 > kMaxNodes) {
        if (tid == 0) a.status[g] = -1;
        return;
    }
    const int n = (int)(n1 - n0), k = a.k, C = a.feat ? a.n_feat : 0;
    const int per_node = n == 1 ? 1 : (n <= k + 1 ? n - 1 : k);
    const int64_t e0 = a.edge_off[g], e1 = a.edge_off[g + 1];
    if (e0 < 0 || e1 < e0 || e1 > a.n_edges || e1 - e0 != (int64_t)n * per_node) {
        if (tid == 0) a.status[g] = -2;
        return;
    }
    for (int i = tid; i < n; i += kThreads) {
        s_x[i] = a.coord[2 * (n0 + i)];
        s_y[i] = a.coord[2 * (n0 + i) + 1];
        for (int ch = 0; ch < C; ++ch) s_f[ch * kMaxNodes + i] = a.feat[(n0 + i) * C + ch];
    }
    __syncthreads();

    const bool ranked = n >= k + 1;           // sigma from the row's k + 1 smallest distances
    for (int i = wave; i < n; i += kWaves) {
        double sc = 1.0, sf = 1.0;
        if (ranked) {
            double dc[kGroups], df[kGroups];
#pragma unroll
            for (int c = 0; c < kGroups; ++c) {
                const int j = c * kWave + lane;
                dc[c] = df[c] = __builtin_inf();
                if (j < n) {
                    const double dx = s_x[i] - s_x[j], dy = s_y[i] - s_y[j];
                    dc[c] = sqrt(dx * dx + dy * dy);
                    double s = 0.0;
                    for (int ch = 0; ch < C; ++ch) {
                        const double d = s_f[ch * kMaxNodes + i] - s_f[ch * kMaxNodes + j];
                        s += d * d;
                    }
                    df[c] = sqrt(s);
                }
            }
            sc = smallest_sum(dc, n, k) / (double)k;
            if (C) sf = smallest_sum(df, n, k) / (double)k;
        }
        if (lane == 0) { s_sc[i] = sc + 1e-8; s_sf[i] = sf + 1e-8; }
    }
    __syncthreads();

    const bool select = n >= k + 2;
    const int skip = select ? a.skip : 0;
    for (int i = wave; i < n; i += kWaves) {
        double av[kGroups];
        const double sci = s_sc[i], sfi = s_sf[i];
#pragma unroll
        for (int c = 0; c < kGroups; ++c) {
            const int j = c * kWave + lane;
            av[c] = -1.0;
            if (j < n && j != i) {
                const double dx = s_x[i] - s_x[j], dy = s_y[i] - s_y[j];
                const double dc = sqrt(dx * dx + dy * dy);
                const double qi = dc / sci, qj = dc / s_sc[j];
                double ti = -(qi * qi), tj = -(qj * qj);
                if (C) {
                    double s = 0.0;
                    for (int ch = 0; ch < C; ++ch) {
                        const double d = s_f[ch * kMaxNodes + i] - s_f[ch * kMaxNodes + j];
                        s += d * d;
                    }
                    const double df = sqrt(s);
                    const double pi = df / sfi, pj = df / s_sf[j];
                    ti = ti - pi * pi;
                    tj = tj - pj * pj;
                }
                const double v = 0.5 * (exp(ti) + exp(tj));
                av[c] = v >= 0.0 ? v : 0.0;
            }
        }
        const int64_t base = e0 + (int64_t)i * per_node;
        if (n == 1) {
            if (lane == 0) { a.src[base] = n0; a.dst[base] = n0; a.value[base] = 0.0f; }
        } else if (!select) {
            // fully connected: lane = column (n <= k + 1 <= 33: the first group only)
            if (lane < n && lane != i) {
                const int64_t e = base + (lane < i ? lane : lane - 1);
                a.src[e] = n0 + i; a.dst[e] = n0 + lane; a.value[e] = (float)av[0];
            }
        } else {
            double keep_v = 0.0;
            int keep_c = i;
            for (int r = 0; r < k + skip; ++r) {
                double bv = -1.0;
                int bc = kNoCol;
#pragma unroll
                for (int c = 0; c < kGroups; ++c)
                    if (c * kWave < n && av[c] > bv) { bv = av[c]; bc = c * kWave + lane; }
                wave_pick<true>(bv, bc);
#pragma unroll
                for (int c = 0; c < kGroups; ++c)
                    if (bc == c * kWave + lane) av[c] = -1.0;
                if (lane == r - skip) { keep_v = bv; keep_c = bc; }
            }
            // (n - 1 >= k + skip candidates rank >= 0 > -1: every round finds a column below n)
            if (lane < k && keep_c < n) {
                const int64_t e = base + lane;
                a.src[e] = n0 + i; a.dst[e] = n0 + keep_c; a.value[e] = (float)keep_v;
            }
        }
    }
    if (tid == 0) a.status[g] = 0;
}

struct SortArgs {
    float* eig;
    int64_t ld;
    const float* x;
    const float* y;
    int64_t n_nodes;
    const int64_t* graph_off;
};

__device__ __forceinline__ int popc64(unsigned long long m) { return __popcll(m); }

__global__ __launch_bounds__(kWave) void sort_eig_kernel(SortArgs a) {
    const int g = blockIdx.x, lane = lane_id();
    const int64_t n0 = a.graph_off[g], n1 = a.graph_off[g + 1];
    if (n0 < 0 || n1 < n0 || n1 > a.n_nodes) return;
    int hor1 = 0, ver1 = 0, hor2 = 0, ver2 = 0;
    for (int64_t b = n0; b < n1; b += kWave) {
        const int64_t i = b + lane;
        const bool in = i < n1;
        const float e1 = in ? a.eig[i * a.ld + 1] : 0.0f, e2 = in ? a.eig[i * a.ld + 2] : 0.0f;
        const bool right = in && a.x[i] > 0.5f, up = in && a.y[i] > 0.5f;
        const bool p1 = in && e1 > 0.0f, p2 = in && e2 > 0.0f;
        hor1 += popc64(__ballot(p1 && right)) - popc64(__ballot(p1 && !right));
        ver1 += popc64(__ballot(p1 && up)) - popc64(__ballot(p1 && !up));
        hor2 += popc64(__ballot(p2 && right)) - popc64(__ballot(p2 && !right));
        ver2 += popc64(__ballot(p2 && up)) - popc64(__ballot(p2 && !up));
    }
    hor1 = abs(hor1); ver1 = abs(ver1); hor2 = abs(hor2); ver2 = abs(ver2);
    const int m = max(max(hor1, ver2), max(ver1, hor2));
    if (hor1 == m || ver2 == m) return;
    // the reference's "exchange" (eigs[:, 1] = eig2; eigs[:, 2] = eig1, eig1 being a view of column 1) leaves column 2 in both columns
    for (int64_t i = n0 + lane; i < n1; i += kWave) a.eig[i * a.ld + 1] = a.eig[i * a.ld + 2];
}

}  // namespace superpixels
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_knn_graph_max_nodes(void) { return superpixels::kMaxNodes; }

extern "C" int dgn_knn_graph(const double* coord, const double* feat, int n_feat, int64_t n_nodes, const int64_t* graph_off, const int64_t* edge_off,
                             int n_graphs, int k, int skip_nearest, int64_t n_edges, int64_t* src, int64_t* dst, float* value, int32_t* status,
                             void* stream) {
    if (n_graphs < 0 || n_nodes < 0 || n_edges < 0) {
        set_error("dgn_knn_graph: negative count (n_graphs %d, n_nodes %lld, n_edges %lld)", n_graphs, (long long)n_nodes, (long long)n_edges);
        return DGN_ERR_INVALID;
    }
    if (k < 1 || k > superpixels::kMaxK) { set_error("dgn_knn_graph: k = %d outside 1 .. %d", k, superpixels::kMaxK); return DGN_ERR_INVALID; }
    if (n_feat < 0 || n_feat > superpixels::kMaxFeat || (feat && n_feat < 1) || (!feat && n_feat != 0)) {
        set_error("dgn_knn_graph: n_feat = %d: 1 .. %d feature channels with feat, 0 without", n_feat, superpixels::kMaxFeat);
        return DGN_ERR_INVALID;
    }
    if (skip_nearest != 0 && skip_nearest != 1) { set_error("dgn_knn_graph: skip_nearest = %d is neither 0 nor 1", skip_nearest); return DGN_ERR_INVALID; }
    if (!coord || !graph_off || !edge_off || !src || !dst || !value || !status) {
        set_error("dgn_knn_graph: null coord / graph_off / edge_off / src / dst / value / status");
        return DGN_ERR_INVALID;
    }
    if (n_graphs == 0) return DGN_OK;
    superpixels::Args a{coord, feat, n_feat, n_nodes, graph_off, edge_off, k, skip_nearest, n_edges, src, dst, value, status};
    hipLaunchKernelGGL(superpixels::knn_kernel, dim3((unsigned)n_graphs), dim3(superpixels::kThreads), 0, static_cast<hipStream_t>(stream), a);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_superpixel_sort_eig(float* eig, int64_t ld_eig, int n_cols, const float* x, const float* y, int64_t n_nodes,
                                       const int64_t* graph_off, int n_graphs, void* stream) {
    if (n_graphs < 0 || n_nodes < 0) {
        set_error("dgn_superpixel_sort_eig: negative count (n_graphs %d, n_nodes %lld)", n_graphs, (long long)n_nodes);
        return DGN_ERR_INVALID;
    }
    if (n_cols < 3) { set_error("dgn_superpixel_sort_eig: n_cols = %d < 3 (columns 1 and 2 are compared)", n_cols); return DGN_ERR_INVALID; }
    if (ld_eig < n_cols) { set_error("dgn_superpixel_sort_eig: ld_eig = %lld < n_cols = %d", (long long)ld_eig, n_cols); return DGN_ERR_INVALID; }
    if (!eig || !x || !y || !graph_off) { set_error("dgn_superpixel_sort_eig: null eig / x / y / graph_off"); return DGN_ERR_INVALID; }
    if (n_graphs == 0) return DGN_OK;
    superpixels::SortArgs a{eig, ld_eig, x, y, n_nodes, graph_off};
    hipLaunchKernelGGL(superpixels::sort_eig_kernel, dim3((unsigned)n_graphs), dim3(kWave), 0, static_cast<hipStream_t>(stream), a);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}
