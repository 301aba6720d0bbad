// Tail of the node-classification step (nets/SBMs_node_classification/dgn_net.py:67-81 and train/metrics.py:37-54): the cross-entropy
// whose class weights come from the batch's own label counts, its gradient, and the confusion matrix of the reference's accuracy_SBM --
// three launches, nothing read back, no floating-point atomics (fixed-order reductions: the same input gives the same bits).
//
//   node_ce_stats   one workgroup per contiguous row range: label counts (integer LDS atomics) and, per class column, an online
//                   (max, sum exp) pair over the range's valid rows -> slot g of the workspace
//   node_ce_rows    every workgroup folds the slots (counts -> weights, denominator; column log-sum-exps), then walks its rows with one
//                   lane per row: row log-sum-exp, loss term, gradient row, predicted class -> loss partial and C x C partial
//   node_ce_finish  one workgroup: loss partials, weights, the int64 confusion matrix
//
// A row is C <= 32 floats (8-128 bytes) and consecutive lanes own consecutive rows.  The kernels are instantiated for the class count
// rounded up to a power of two (CP = 2 .. 32) so that a row and the per-column state live in registers under compile-time indices (a
// runtime-indexed array would live in scratch memory); dense, aligned rows are read and written as 8- or 16-byte pieces.  At the sizes this
// runs at (15 k rows) each kernel is a chain of a few memory latencies, so the loads of a row are independent of one another and the
// slot folds are spread over the workgroup.  Cross-lane and cross-workgroup sums run in fp64 in an order that depends on N alone.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dgn_net_io.hpp"

namespace dgn {
namespace node_ce {

using namespace net_io;      // load_scores, row_max: the score-row helpers shared with the class cross-entropy

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxC = 32;
constexpr int kMaxGroups = 256;
constexpr int kMinRows = 512;        // rows per workgroup at least: few slots to fold for small batches
constexpr int kSub = kThreads / kMaxC;   // the slot folds run as kSub interleaved sub-sequences, combined in order

struct Layout {
    int groups;
    int64_t per;                     // rows per workgroup
    size_t cnt, colm, cols, lossp, cm, bytes;
};

inline Layout layout(int64_t n_rows, int32_t C) {
    Layout L{};
    const SlotSplit s = slot_split(n_rows, kMinRows, kMaxGroups);
    L.groups = s.groups;
    L.per = s.per;
    const size_t G = (size_t)s.bound;    // sized by the upper bound of `groups`
    L.cols = 0;                                              // double [G][32]
    L.lossp = L.cols + G * kMaxC * sizeof(double);           // double [G]
    L.cnt = L.lossp + G * sizeof(double);                    // int    [G][32]
    L.colm = L.cnt + G * kMaxC * sizeof(int);                // float  [G][32]
    L.cm = L.colm + G * kMaxC * sizeof(float);               // int    [G][C C]
    L.bytes = L.cm + G * (size_t)C * C * sizeof(int);
    return L;
}

// (m, s) := log-sum-exp pair of the union; s in units of exp(m)
__device__ __forceinline__ void lse_merge(float& m, double& s, float m2, double s2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) { m = M; s = 0.0; return; }
    s = s * (double)expf(m - M) + s2 * (double)expf(m2 - M);
    m = M;
}

// the reference's weight: (V - count).float() / V, zero for an absent class (dgn_net.py:74-75)
__device__ __forceinline__ float class_weight(int64_t V, int64_t count) {
    return count > 0 ? (float)(V - count) / (float)V : 0.f;
}

// row n's C scores into x[0 .. CP): net_io::load_scores, or as 8- / 16-byte pieces
template <int CP>
__device__ __forceinline__ void load_row(float (&x)[CP], const float* __restrict__ p, int C, bool vec) {
    if (vec) {                              // C == CP, dense rows, 16-byte (CP = 2: 8-byte) aligned
        if constexpr (CP == 2) {
            ldv<2>(x, p);
        } else {
#pragma unroll
            for (int c = 0; c < CP; c += 4) {
                float t[4];
                ldv<4>(t, p + c);
                x[c] = t[0]; x[c + 1] = t[1]; x[c + 2] = t[2]; x[c + 3] = t[3];
            }
        }
    } else {
        load_scores<CP>(x, p, C);
    }
}
template <int CP>
__device__ __forceinline__ void store_row(float* __restrict__ p, const float (&v)[CP], int C, bool vec) {
    if (vec) {
        if constexpr (CP == 2) {
            stv<2>(p, v);
        } else {
#pragma unroll
            for (int c = 0; c < CP; c += 4) {
                const float t[4] = {v[c], v[c + 1], v[c + 2], v[c + 3]};
                stv<4>(p + c, t);
            }
        }
    } else {
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) p[c] = v[c];
    }
}
template <int CP>
__device__ __forceinline__ bool rows_vectorisable(const float* p, int64_t ld, int C) {
    return C == CP && ld == CP && (reinterpret_cast<uintptr_t>(p) & (CP == 2 ? 7 : 15)) == 0;
}

template <int CP>
__global__ __launch_bounds__(kThreads) void node_ce_stats(int64_t N, int C, const float* __restrict__ scores, int64_t ld,
                                                           const int64_t* __restrict__ labels, int64_t per, int want_cols,
                                                           int* __restrict__ cnt, float* __restrict__ colm, double* __restrict__ cols) {
    __shared__ int s_cnt[kMaxC];
    __shared__ float s_m[kWaves][CP];
    __shared__ double s_s[kWaves][CP];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t r0 = (int64_t)b * per, r1 = (r0 + per < N) ? r0 + per : N;
    const bool vec = rows_vectorisable<CP>(scores, ld, C);
    if (tid < kMaxC) s_cnt[tid] = 0;
    __syncthreads();
    float m[CP], sf[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) { m[c] = -INFINITY; sf[c] = 0.f; }
    for (int64_t n = r0 + tid; n < r1; n += kThreads) {
        const int64_t y = labels[n];
        float x[CP];
        if (want_cols) load_row<CP>(x, scores + n * ld, C, vec);      // (issued with the label's load, not behind it)
        if (y < 0 || y >= C) continue;
        atomicAdd(&s_cnt[(int)y], 1);
        if (!want_cols) continue;
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            const float M = fmaxf(m[c], x[c]);
            if (M != -INFINITY) sf[c] = sf[c] * expf(m[c] - M) + expf(x[c] - M);
            m[c] = M;
        }
    }
    __syncthreads();
    if (tid < kMaxC) cnt[b * kMaxC + tid] = s_cnt[tid];
    if (!want_cols) return;
#pragma unroll
    for (int c = 0; c < CP; ++c) {
        if (c >= C) break;
        // the wave's maximum first (exact, order-free), every lane's sum rescaled to it once, then an fp64 butterfly whose operands are
        // ordered by lane (both partners form the same sum)
        const float mm = wave_max(m[c]);
        double ss = mm == -INFINITY ? 0.0 : (double)sf[c] * (double)expf(m[c] - mm);
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const double s2 = shfl_xor_d(ss, o);
            ss = (lane_id() & o) ? s2 + ss : ss + s2;
        }
        if (lane_id() == 0) { s_m[tid / kWave][c] = mm; s_s[tid / kWave][c] = ss; }
    }
    __syncthreads();
    if (tid < C) {
        float mm = s_m[0][tid];
        double ss = s_s[0][tid];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) lse_merge(mm, ss, s_m[w][tid], s_s[w][tid]);
        colm[b * kMaxC + tid] = mm;
        cols[b * kMaxC + tid] = ss;
    }
}

// Label counts of the batch from the G slots, by the whole workgroup: thread (sub, c) adds the slots sub, sub + kSub, ...; thread c < C
// adds the kSub partials.  With colm: the columns' (max, sum exp) pairs likewise, merged in that fixed order.  Ends with a barrier.
__device__ __forceinline__ void fold_slots(int C, int G, const int* __restrict__ cnt, const float* __restrict__ colm,
                                           const double* __restrict__ cols, int64_t* s_count, float* s_lse) {
    __shared__ int p_cnt[kSub][kMaxC];
    __shared__ float p_m[kSub][kMaxC];
    __shared__ double p_s[kSub][kMaxC];
    const int tid = threadIdx.x, c = tid & (kMaxC - 1), sub = tid / kMaxC;
    int count = 0;
    float m = -INFINITY;
    double s = 0.0;
    if (c < C) {
#pragma unroll 4
        for (int g = sub; g < G; g += kSub) count += cnt[g * kMaxC + c];
        if (colm)
#pragma unroll 2
            for (int g = sub; g < G; g += kSub) lse_merge(m, s, colm[g * kMaxC + c], cols[g * kMaxC + c]);
    }
    p_cnt[sub][c] = count; p_m[sub][c] = m; p_s[sub][c] = s;
    __syncthreads();
    if (tid < C) {
        int64_t total = 0;
        float mm = -INFINITY;
        double ss = 0.0;
#pragma unroll
        for (int q = 0; q < kSub; ++q) { total += p_cnt[q][tid]; lse_merge(mm, ss, p_m[q][tid], p_s[q][tid]); }
        s_count[tid] = total;
        if (colm) s_lse[tid] = (mm != -INFINITY) ? (float)((double)mm + log(ss)) : 0.f;
    }
    __syncthreads();
}

template <int CP>
__global__ __launch_bounds__(kThreads) void node_ce_rows(int64_t N, int C, const float* __restrict__ scores, int64_t ld,
                                                          const int64_t* __restrict__ labels, int64_t per, int G, const int* __restrict__ cnt,
                                                          const float* __restrict__ colm, const double* __restrict__ cols,
                                                          float* __restrict__ g, int64_t ld_g, double* __restrict__ lossp,
                                                          int* __restrict__ cmp) {
    __shared__ int64_t s_count[kMaxC];
    __shared__ float s_w[kMaxC];
    __shared__ float s_lse[kMaxC];
    __shared__ double s_den;
    __shared__ double s_red[kWaves];
    __shared__ int s_cm[kMaxC * kMaxC];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t r0 = (int64_t)b * per, r1 = (r0 + per < N) ? r0 + per : N;
    const bool vec = rows_vectorisable<CP>(scores, ld, C), vec_g = g && rows_vectorisable<CP>(g, ld_g, C);
    if (tid < kMaxC) s_lse[tid] = 0.f;
    if (cmp)
        for (int i = tid; i < C * C; i += kThreads) s_cm[i] = 0;
    __syncthreads();
    fold_slots(C, G, cnt, cmp ? colm : nullptr, cols, s_count, s_lse);
    if (tid == 0) {
        int64_t V = 0;
        for (int c = 0; c < C; ++c) V += s_count[c];
        double den = 0.0;
        for (int c = 0; c < C; ++c) {
            const float w = class_weight(V, s_count[c]);
            s_w[c] = w;
            den += (double)w * (double)s_count[c];
        }
        s_den = den;
    }
    __syncthreads();
    const float den = (float)s_den;
    double acc = 0.0;
    for (int64_t n = r0 + tid; n < r1; n += kThreads) {
        const int64_t y64 = labels[n];
        float x[CP], gr[CP];
        load_row<CP>(x, scores + n * ld, C, vec);                       // (issued with the label's load, not behind it)
        if (y64 < 0 || y64 >= C) {               // a row that does not exist: counts nowhere, exact zero gradient
            if (g) {
#pragma unroll
                for (int c = 0; c < CP; ++c) gr[c] = 0.f;
                store_row<CP>(g + n * ld_g, gr, C, vec_g);
            }
            continue;
        }
        const int y = (int)y64;
        const float m = row_max<CP>(x);
        float e[CP], s = 0.f, xy = 0.f;                                 // (sum exp as net_io::sum_exp adds it, the terms kept for the gradient)
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            e[c] = expf(x[c] - m);
            s += e[c];
            xy = c == y ? x[c] : xy;
        }
        const float wy = s_w[y];
        acc += (double)wy * ((double)m + log((double)s) - (double)xy);
        if (g) {
#pragma unroll
            for (int c = 0; c < CP; ++c) gr[c] = wy * (e[c] / s - (c == y ? 1.f : 0.f)) / den;
            store_row<CP>(g + n * ld_g, gr, C, vec_g);
        }
        if (cmp) {
            int best = 0;
            float bv = x[0] - s_lse[0];
#pragma unroll
            for (int c = 1; c < CP; ++c) {
                const float v = x[c] - s_lse[c];
                if (c < C && v > bv) { bv = v; best = c; }       // first maximum wins, as numpy.argmax
            }
            atomicAdd(&s_cm[y * C + best], 1);
        }
    }
    const double t = block_sum<kWaves>(acc, s_red);
    if (tid == 0) lossp[b] = t;
    if (cmp)
        for (int i = tid; i < C * C; i += kThreads) cmp[(int64_t)b * C * C + i] = s_cm[i];
}

__global__ __launch_bounds__(kThreads) void node_ce_finish(int C, int G, const int* __restrict__ cnt, const double* __restrict__ lossp,
                                                            const int* __restrict__ cmp, float* __restrict__ loss, float* __restrict__ weight,
                                                            int64_t* __restrict__ confusion) {
    __shared__ int64_t s_count[kMaxC];
    __shared__ double s_red[kWaves];
    const int tid = threadIdx.x;
    fold_slots(C, G, cnt, nullptr, nullptr, s_count, nullptr);
    const double total = block_sum<kWaves>(tid < G ? lossp[tid] : 0.0, s_red);           // G <= 256 = one slot per thread
    if (tid == 0) {
        int64_t V = 0;
        for (int c = 0; c < C; ++c) V += s_count[c];
        double den = 0.0;
        for (int c = 0; c < C; ++c) {
            const float w = class_weight(V, s_count[c]);
            if (weight) weight[c] = w;
            den += (double)w * (double)s_count[c];
        }
        // no valid row: 0 (the reference raises).  One class only: 0 / 0 = nan, as the reference returns.
        *loss = V > 0 ? (float)(total / den) : 0.f;
    }
    if (confusion)
        for (int i = tid; i < C * C; i += kThreads) {
            int64_t t = 0;
#pragma unroll 4
            for (int s = 0; s < G; ++s) t += cmp[(int64_t)s * C * C + i];
            confusion[i] = t;
        }
}

}  // namespace node_ce
}  // namespace dgn

using namespace dgn;

extern "C" size_t dgn_node_ce_workspace_bytes(int64_t n_rows, int32_t n_classes) {
    if (n_rows < 0 || n_rows > INT32_MAX || n_classes < 1 || n_classes > node_ce::kMaxC) return 0;
    return node_ce::layout(n_rows, n_classes).bytes;
}

extern "C" int dgn_node_ce_forward(int64_t n_rows, int32_t n_classes, const float* scores, int64_t ld, const int64_t* labels, float* loss,
                                   float* weight, float* g_scores, int64_t ld_g, int64_t* confusion, void* ws, size_t ws_bytes,
                                   void* stream) {
    const int C = n_classes;
    if (C < 1 || C > node_ce::kMaxC) { set_error("dgn_node_ce_forward: 1 <= n_classes <= 32 required (got %d)", C); return DGN_ERR_INVALID; }
    if (!net_io::rows_in_range("dgn_node_ce_forward", n_rows)) return DGN_ERR_INVALID;
    if (!loss) { set_error("dgn_node_ce_forward: null loss"); return DGN_ERR_INVALID; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_rows == 0) {
        hipLaunchKernelGGL(node_ce::node_ce_finish, dim3(1), dim3(node_ce::kThreads), 0, st, C, 0, (const int*)nullptr, (const double*)nullptr,
                           (const int*)nullptr, loss, weight, confusion);
        DGN_HIP_CHECK(hipGetLastError());
        return DGN_OK;
    }
    if (!scores || !labels) { set_error("dgn_node_ce_forward: null scores / labels"); return DGN_ERR_INVALID; }
    if (ld < C || (g_scores && ld_g < C)) { set_error("dgn_node_ce_forward: row stride below n_classes"); return DGN_ERR_INVALID; }
    const node_ce::Layout L = node_ce::layout(n_rows, C);
    if (!net_io::workspace_ok("dgn_node_ce_forward", ws, ws_bytes, L.bytes, 8)) return DGN_ERR_INVALID;
    char* base = static_cast<char*>(ws);
    double* cols = reinterpret_cast<double*>(base + L.cols);
    double* lossp = reinterpret_cast<double*>(base + L.lossp);
    int* cnt = reinterpret_cast<int*>(base + L.cnt);
    float* colm = reinterpret_cast<float*>(base + L.colm);
    int* cmp = confusion ? reinterpret_cast<int*>(base + L.cm) : nullptr;
    const dim3 grid((unsigned)L.groups), block(node_ce::kThreads);
#define DGN_NODE_CE_LAUNCH(CP)                                                                                                              \
    do {                                                                                                                                    \
        hipLaunchKernelGGL(node_ce::node_ce_stats<CP>, grid, block, 0, st, n_rows, C, scores, ld, labels, L.per, confusion ? 1 : 0, cnt,    \
                           colm, cols);                                                                                                     \
        hipLaunchKernelGGL(node_ce::node_ce_rows<CP>, grid, block, 0, st, n_rows, C, scores, ld, labels, L.per, L.groups, (const int*)cnt,  \
                           (const float*)colm, (const double*)cols, g_scores, ld_g, lossp, cmp);                                            \
    } while (0)
    DGN_CLASS_POW2_DISPATCH(C, DGN_NODE_CE_LAUNCH);
#undef DGN_NODE_CE_LAUNCH
    hipLaunchKernelGGL(node_ce::node_ce_finish, dim3(1), block, 0, st, C, L.groups, (const int*)cnt, (const double*)lossp, (const int*)cmp, loss,
                       weight, confusion);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_node_ce_backward(int64_t n_rows, int32_t n_classes, const float* g_saved, int64_t ld_g, const float* g_loss,
                                    float* g_scores, int64_t ld_out, void* stream) {
    const int C = n_classes;
    if (C < 1 || C > node_ce::kMaxC) { set_error("dgn_node_ce_backward: 1 <= n_classes <= 32 required (got %d)", C); return DGN_ERR_INVALID; }
    return net_io::loss_backward("dgn_node_ce_backward", "n_classes", n_rows, C, g_saved, ld_g, g_loss, g_scores, ld_out, stream);
}
