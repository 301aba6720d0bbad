// Laplacian eigenpairs of a batch of small graphs: one workgroup per graph, the whole solve in LDS, one launch per width class.
//
// Replaces, for graphs of at most 64 nodes, the per-graph ARPACK solve of the reference's data loaders (data/molecules.py:100-116 get_eig,
// :18-32 positional_encoding) and gives the eigenvalues its multiplicity check needs (data/multiplicity_eig.py:14-27).
//
//   build     L is accumulated in fp64 from the graph's rows of the destination-major CSR: in-degree d_i = max(indptr[i + 1] - indptr[i], 1),
//             every edge j -> i adds -w to L[i][j] and to L[j][i] (the symmetrised adjacency (A + A^T) / 2; multi-edges and self-loops add
//             up) with w = 1/2 ('none') or 1 / (2 sqrt(d_i d_j)) ('sym', 'walk'), then the diagonal gets d_i ('none') or 1.  The adds are LDS
//             fp64 atomics: multiples of 1/2, or two equal terms per cell on a simple graph, so their order does not show in the sum.
//             A source outside the graph's node range never becomes an LDS index: the graph gets status -2 and nothing else is written.
//   solve     two-sided cyclic Jacobi in round-robin order: a sweep is m - 1 steps (m = n rounded up to even) of m / 2 disjoint pairs
//             (an odd n leaves one slot idle).  Per step: every pair's rotation from the matrix as it stands (Rutishauser:
//             theta = (a_qq - a_pp) / 2 a_pq, t = sign(theta) / (|theta| + hypot(theta, 1)): no theta^2; a_pq == 0 skips the pair) | barrier |
//             the column rotations A <- A J | barrier | the row rotations A <- J^T A, with a_pq = 0 and a_pp - t a_pq, a_qq + t a_pq written
//             as such, and V <- V J | barrier.  Disjoint pairs commute, so a step is the sequential method in that order.
//   stop      after every sweep the off-diagonal squares are summed directly (sum a^2 - sum a_ii^2 cancels long before the threshold);
//             the solve ends when their root is <= 1e-14 ||L||_F or after max_sweeps sweeps.  status = sweeps done (>= 1).
//   epilogue  eigenvalues ranked ascending, ties by column index; the min(k, n) lowest eigenvectors go to vec[N, k] as fp32 ('walk': scaled
//             by d^-1/2 and brought back to unit length), their eigenvalues to val[G, k]; columns / slots beyond n: 0 / NaN.
//
// All sums run in an order fixed by n and the width class alone, and a graph's class depends on its n alone: a graph's rows and eigenvalues are
// the same bits in whatever batch it travels.  No size is known on the host: both classes are launched over all graphs and a workgroup whose
// graph belongs to the other class returns at once.
//
// LDS (doubles, row stride W + 1: a column walk of an fp64 matrix with an even stride stays on one bank pair): A and V [W][W + 1], per pair
// c, s and the two new diagonal entries, per node d^-1/2 (or d) and the eigenvalue, 8 reduction slots, 32 column scales; ints: the pairs, the
// order, the flag.  W = 32: 18 512 bytes, one wave-pair workgroup of 64 threads; W = 64: 69 456 bytes, 256 threads (dynamic LDS beyond 64 KB).
#include <hip/hip_runtime.h>

#include <cmath>

#include "dgn_common.hpp"

namespace dgn {
namespace eig_small {

constexpr int kMaxNodes = 64;
constexpr int kMaxK = 32;
constexpr double kTol2 = 1e-28;              // (1e-14)^2: the stop rule compares squares

struct Args {
    const int32_t* indptr;
    const int32_t* src;
    int64_t n_nodes, n_edges;
    const int64_t* graph_off;
    int k, norm, max_sweeps;
    float* vec;
    double* val;
    int32_t* status;
};

template <int W>
struct Lds {
    static constexpr int kStride = W + 1;
    static constexpr int kDoubles = 2 * W * kStride + 4 * (W / 2) + 2 * W + 8 + kMaxK;
    static constexpr int kInts = 2 * (W / 2) + W + 4;
    static constexpr int kBytes = kDoubles * 8 + kInts * 4;
};

template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    if constexpr (THREADS == kWave) return v;
    constexpr int kWaves = THREADS / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = red[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += red[w];
    __syncthreads();                         // (red is free again)
    return s;
}

// W = width class (graphs of (W / 2, W] nodes; the first class also takes everything below), THREADS = W * THREADS / W: lane i of a row group
// owns row / column i, THREADS / W groups work on different pairs.
template <int W, int THREADS>
__global__ __launch_bounds__(THREADS) void eig_small_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using L = Lds<W>;
    constexpr int S = L::kStride;
    constexpr int kGroups = THREADS / W;
    double* A = reinterpret_cast<double*>(smem);
    double* V = A + W * S;
    double* rc = V + W * S;                  // per pair: cos, sin, new a_pp, new a_qq
    double* rs = rc + W / 2;
    double* rpp = rs + W / 2;
    double* rqq = rpp + W / 2;
    double* dsc = rqq + W / 2;               // d^-1/2 ('sym', 'walk') or d ('none')
    double* lam = dsc + W;
    double* red = lam + W;
    double* cscale = red + 8;
    int* pp = reinterpret_cast<int*>(cscale + kMaxK);
    int* qq = pp + W / 2;
    int* order = qq + W / 2;
    int* flag = order + W;

    const int g = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t n0 = a.graph_off[g], n1 = a.graph_off[g + 1];
    const int64_t span = n1 - n0;
    const bool range_ok = n0 >= 0 && n1 >= n0 && n1 <= a.n_nodes;
    // which class owns the graph: a malformed range and everything up to 32 nodes the first, the rest (oversize included) the second
    const bool small = !range_ok || span <= 32;
    if (small != (W == 32)) return;
    if (!range_ok || span > kMaxNodes) {
        if (tid == 0) a.status[g] = range_ok ? -1 : -2;
        return;
    }
    const int n = (int)span;
    const bool normalised = a.norm != 0;

    for (int e = tid; e < W * S; e += THREADS) { A[e] = 0.0; V[e] = 0.0; }
    if (tid < W) order[tid] = tid;
    if (tid == 0) *flag = 0;
    if (tid < n) {
        const int d = a.indptr[n0 + tid + 1] - a.indptr[n0 + tid];
        const double dd = d > 1 ? (double)d : 1.0;
        dsc[tid] = normalised ? 1.0 / sqrt(dd) : dd;
    }
    __syncthreads();
    for (int i = tid; i < n; i += THREADS) {
        V[i * S + i] = 1.0;
        int64_t e0 = a.indptr[n0 + i], e1 = a.indptr[n0 + i + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > a.n_edges) e1 = a.n_edges;
        for (int64_t e = e0; e < e1; ++e) {
            const int64_t j = (int64_t)a.src[e] - n0;
            if (j < 0 || j >= n) { *flag = 1; continue; }                 // a foreign source: never an LDS index
            const double w = normalised ? (0.5 * dsc[i]) * dsc[j] : 0.5;
            lds_add_f64(&A[i * S + (int)j], -w);
            lds_add_f64(&A[(int)j * S + i], -w);
        }
    }
    __syncthreads();
    if (*flag) {
        if (tid == 0) a.status[g] = -2;
        return;
    }
    if (tid < n) A[tid * S + tid] += normalised ? 1.0 : dsc[tid];
    __syncthreads();

    const int col = tid % W, grp = tid / W;
    double part = 0.0;
    for (int i = grp; i < n; i += kGroups)
        if (col < n) { const double x = A[i * S + col]; part += x * x; }
    const double norm2 = block_sum<THREADS>(part, red);

    const int m = n + (n & 1), npairs = m / 2;
    int sweeps = 0;
    double off2;
    do {
        for (int r = 0; r < m - 1; ++r) {
            if (tid < npairs) {
                int x, y;
                if (tid == 0) { x = m - 1; y = r; }
                else { x = (r + tid) % (m - 1); y = (r - tid + (m - 1)) % (m - 1); }
                int p = x < y ? x : y, q = x < y ? y : x;
                double c = 1.0, s = 0.0, app = 0.0, aqq = 0.0;
                bool live = q < n;                                         // (q == n: the idle slot of an odd n)
                if (live) {
                    const double apq = A[p * S + q];
                    app = A[p * S + p];
                    aqq = A[q * S + q];
                    if (apq != 0.0) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + hypot(theta, 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        app -= t * apq;
                        aqq += t * apq;
                    } else {
                        live = false;
                    }
                }
                pp[tid] = live ? p : -1;
                qq[tid] = q;
                rc[tid] = c; rs[tid] = s; rpp[tid] = app; rqq[tid] = aqq;
            }
            __syncthreads();
            // column rotations: lane `col` is row i of A, the groups take pairs in turn
            for (int kp = grp; kp < npairs; kp += kGroups) {
                const int p = pp[kp], q = qq[kp];
                if (p < 0 || col >= n) continue;
                const double c = rc[kp], s = rs[kp];
                const double x = A[col * S + p], y = A[col * S + q];
                A[col * S + p] = c * x - s * y;
                A[col * S + q] = s * x + c * y;
            }
            __syncthreads();
            // row rotations: lane `col` is column j of A; then V's column rotations (lane `col` is row i of V)
            for (int kp = grp; kp < npairs; kp += kGroups) {
                const int p = pp[kp], q = qq[kp];
                if (p < 0 || col >= n) continue;
                const double c = rc[kp], s = rs[kp];
                const double x = A[p * S + col], y = A[q * S + col];
                double xn = c * x - s * y, yn = s * x + c * y;
                if (col == p) { xn = rpp[kp]; yn = 0.0; }
                if (col == q) { xn = 0.0; yn = rqq[kp]; }
                A[p * S + col] = xn;
                A[q * S + col] = yn;
                const double vx = V[col * S + p], vy = V[col * S + q];
                V[col * S + p] = c * vx - s * vy;
                V[col * S + q] = s * vx + c * vy;
            }
            __syncthreads();
        }
        ++sweeps;
        part = 0.0;
        for (int i = grp; i < n; i += kGroups)
            if (col < n && col != i) { const double x = A[i * S + col]; part += x * x; }
        off2 = block_sum<THREADS>(part, red);
    } while (off2 > kTol2 * norm2 && sweeps < a.max_sweeps);

    if (tid < n) lam[tid] = A[tid * S + tid];
    __syncthreads();
    if (tid < n) {
        const double mine = lam[tid];
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const double o = lam[i];
            rank += (o < mine || (o == mine && i < tid)) ? 1 : 0;
        }
        order[rank] = tid;                   // (rank < n: a NaN only leaves slots at their initial value, still a column of V)
    }
    __syncthreads();
    const int k = a.k, kk = k < n ? k : n;
    if (tid < kk) {
        double sc = 1.0;
        if (a.norm == 2) {                   // 'walk': D^-1/2 v, unit length
            const int c = order[tid];
            double s2 = 0.0;
            for (int i = 0; i < n; ++i) { const double x = V[i * S + c] * dsc[i]; s2 += x * x; }
            sc = 1.0 / sqrt(s2 > 1e-300 ? s2 : 1e-300);
        }
        cscale[tid] = sc;
    }
    __syncthreads();
    float* out = a.vec + n0 * (int64_t)k;
    for (int e = tid; e < n * k; e += THREADS) {
        const int i = e / k, c = e - i * k;
        double x = 0.0;
        if (c < kk) {
            x = V[i * S + order[c]];
            if (a.norm == 2) x = x * dsc[i] * cscale[c];
        }
        out[e] = (float)x;
    }
    if (a.val && tid < k) a.val[(int64_t)g * k + tid] = tid < kk ? lam[order[tid]] : __builtin_nan("");
    if (tid == 0) a.status[g] = sweeps;
}

}  // namespace eig_small
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_eig_small_max_nodes(void) { return eig_small::kMaxNodes; }

extern "C" int dgn_eig_small(const DgnGraph* graph, const int64_t* graph_off, int n_graphs, int k, int norm, int max_sweeps, float* vec, double* val,
                             int32_t* status, void* stream) {
    if (!graph || !graph->indptr || (graph->n_edges > 0 && !graph->src)) { set_error("dgn_eig_small: null CSR"); return DGN_ERR_INVALID; }
    if (graph->n_nodes < 0 || graph->n_edges < 0 || graph->n_nodes >= INT32_MAX || graph->n_edges >= INT32_MAX) {
        set_error("dgn_eig_small: graph outside the int32 CSR range");
        return DGN_ERR_INVALID;
    }
    if (n_graphs < 0) { set_error("dgn_eig_small: n_graphs = %d < 0", n_graphs); return DGN_ERR_INVALID; }
    if (k < 1 || k > eig_small::kMaxK) { set_error("dgn_eig_small: k = %d outside 1 .. %d", k, eig_small::kMaxK); return DGN_ERR_INVALID; }
    if (norm < DGN_EIG_NORM_NONE || norm > DGN_EIG_NORM_WALK) { set_error("dgn_eig_small: unknown norm %d", norm); return DGN_ERR_INVALID; }
    if (max_sweeps < 1) { set_error("dgn_eig_small: max_sweeps = %d < 1", max_sweeps); return DGN_ERR_INVALID; }
    if (!graph_off || !vec || !status) { set_error("dgn_eig_small: null graph_off / vec / status"); return DGN_ERR_INVALID; }
    if (n_graphs == 0) return DGN_OK;
    eig_small::Args a{graph->indptr, graph->src, graph->n_nodes, graph->n_edges, graph_off, k, norm, max_sweeps, vec, val, status};
    hipStream_t s = static_cast<hipStream_t>(stream);
    static LdsOptIn lds_ok{0};
    DGN_HIP_CHECK(allow_lds(lds_ok, eig_small::Lds<64>::kBytes, &eig_small::eig_small_kernel<64, 256>));
    hipLaunchKernelGGL((eig_small::eig_small_kernel<32, 64>), dim3((unsigned)n_graphs), dim3(64), eig_small::Lds<32>::kBytes, s, a);
    DGN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((eig_small::eig_small_kernel<64, 256>), dim3((unsigned)n_graphs), dim3(256), eig_small::Lds<64>::kBytes, s, a);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}
