// The two pieces of the superpixel graph-classification net (nets/superpixels_graph_classification/dgn_net.py) that no other net has: the
// input embedding nn.Linear(in_dim <= 8, hidden) of dgn_net.py:31, :35, :53, :56 forward and backward, and the loss tail of its loop --
// nn.CrossEntropyLoss() (dgn_net.py:75-78) with the hit count of accuracy_MNIST_CIFAR (train/metrics.py:25-28).  Nothing read back, no
// floating-point atomics, fixed-order reductions (the same input gives the same bits), every launch parameter a function of the shapes.
//
//   embed_forward   one workgroup per kEmbRows rows: W (transposed), b and the rows' x in LDS, every output b + sum_k W[f, k] x[r, k] in
//                   increasing k; dense output rows leave as flat 16-byte chunks whatever the width (65, 75: net_io::write_rows)
//   embed_partial   one workgroup per contiguous row range: thread (sub, f) walks the rows sub, sub + n_sub, ... of column f of g and keeps
//                   dW[f, 0 .. K) and db[f]; the sub-sequences are joined in order, the [K + 1, F] block goes to the workgroup's slot
//   embed_fold      the slots added in a fixed order (wg::slot_sum16), dW in torch's [F, K] layout and db written
//   ce_stats        one workgroup per contiguous row range, one lane per row: loss term, valid and hit counts -> slot b
//   ce_rows         every workgroup folds the slots (net_io::fold_mean_slots; block 0 writes loss and hits), then writes the gradient rows
//                   of its range
//   (net_io::loss_backward: the autograd backward, g_saved * *g_loss)
//
// Both families are instantiated per width (K = 1 .. 8; the class count rounded up to a power of two, CP = 2 .. 64) so that a row lives
// in registers under compile-time indices (net_io::load_scores, row_max, sum_exp).
#include <hip/hip_runtime.h>

#include <cmath>

#include "dgn_net_io.hpp"
#include "dgn_wgrad.hpp"

namespace dgn {
namespace gcls {

using namespace net_io;

// ---- feature embedding ---------------------------------------------------------------------------------------------------------------

constexpr int kMaxK = DGN_FEAT_EMBED_MAX_K;
constexpr int kMaxF = DGN_FEAT_EMBED_MAX_F;
constexpr int kEmbThreads = 256;
constexpr int kEmbRows = 128;                   // rows per forward workgroup; a multiple of four: every workgroup's flat range begins on a chunk
constexpr int kEmbTile = 64;                    // rows of x staged per trip of the backward
constexpr int kEmbMinRows = 64;                 // rows per partial slot at least
constexpr int kEmbMaxGroups = 256;
constexpr int kFoldThreads = wg::kSumWaves * kWave;

static_assert(kEmbRows % 4 == 0 && kMaxF <= kEmbThreads, "embed_forward's chunks / embed_partial's column threads");

inline bool embed_args_ok(int32_t K, int32_t F) { return K >= 1 && K <= kMaxK && F >= 1 && F <= kMaxF; }

struct EmbLayout {
    int groups;
    int64_t per;                                // rows per workgroup
    int block;                                  // floats of one slot: [K + 1, F]
    size_t bytes;
};
inline EmbLayout emb_layout(int64_t n_rows, int32_t K, int32_t F) {
    EmbLayout L{};
    const SlotSplit s = slot_split(n_rows, kEmbMinRows, kEmbMaxGroups);
    L.groups = s.groups;
    L.per = s.per;
    L.block = (K + 1) * F;
    L.bytes = (size_t)s.bound * (size_t)L.block * sizeof(float);      // sized by the upper bound of `groups`
    return L;
}

template <int K>
__global__ __launch_bounds__(kEmbThreads) void embed_forward(int64_t R, int F, const float* __restrict__ x, int64_t ld,
                                                              const float* __restrict__ W, const float* __restrict__ b,
                                                              float* __restrict__ y, int64_t ld_y, int flat) {
    __shared__ float s_w[K][kMaxF];
    __shared__ float s_b[kMaxF];
    __shared__ float s_x[kEmbRows][K];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kEmbRows;
    const int n = (int)(R - r0 < kEmbRows ? R - r0 : kEmbRows);
    for (int i = tid; i < F * K; i += kEmbThreads) { const int f = i / K; s_w[i - f * K][f] = W[i]; }
    for (int i = tid; i < F; i += kEmbThreads) s_b[i] = b ? b[i] : 0.f;
    for (int i = tid; i < n * K; i += kEmbThreads) { const int r = i / K, k = i - r * K; s_x[r][k] = x[(r0 + r) * ld + k]; }
    __syncthreads();
    auto dot = [&](int r, int f) {
        float a = s_b[f];
#pragma unroll
        for (int k = 0; k < K; ++k) a = fmaf(s_w[k][f], s_x[r][k], a);
        return a;
    };
    write_rows<kEmbThreads>(y, ld_y, r0, n, F, flat, dot);
}

template <int K>
__global__ __launch_bounds__(kEmbThreads) void embed_partial(int64_t R, int F, const float* __restrict__ x, int64_t ld,
                                                              const float* __restrict__ g, int64_t ld_g, int64_t per,
                                                              float* __restrict__ part) {
    __shared__ float s_x[kEmbTile][K];
    __shared__ float s_p[K + 1][kEmbThreads];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int n_sub = kEmbThreads / F, sub = tid / F, f = tid - sub * F;
    const bool active = sub < n_sub;
    const int64_t r0 = (int64_t)b * per, r1 = (r0 + per < R) ? r0 + per : R;
    float acc[K + 1];
#pragma unroll
    for (int k = 0; k <= K; ++k) acc[k] = 0.f;
    for (int64_t t0 = r0; t0 < r1; t0 += kEmbTile) {
        const int nt = (int)(r1 - t0 < kEmbTile ? r1 - t0 : kEmbTile);
        __syncthreads();
        for (int i = tid; i < nt * K; i += kEmbThreads) { const int r = i / K, k = i - r * K; s_x[r][k] = x[(t0 + r) * ld + k]; }
        __syncthreads();
        if (active) {
            const float* gp = g + t0 * ld_g + f;
#pragma unroll 4
            for (int i = sub; i < nt; i += n_sub) {
                const float gv = gp[(int64_t)i * ld_g];
#pragma unroll
                for (int k = 0; k < K; ++k) acc[k] = fmaf(gv, s_x[i][k], acc[k]);
                acc[K] += gv;
            }
        }
    }
#pragma unroll
    for (int k = 0; k <= K; ++k) s_p[k][tid] = acc[k];
    __syncthreads();
    if (tid < F) {
        float* dst = part + (int64_t)b * (K + 1) * F + tid;
#pragma unroll
        for (int k = 0; k <= K; ++k) {
            float v = s_p[k][tid];
            for (int q = 1; q < n_sub; ++q) v += s_p[k][q * F + tid];
            dst[k * F] = v;
        }
    }
}

// element i = k F + f of the [K + 1, F] blocks: rows k < K are dW[:, k], row K is db
__global__ __launch_bounds__(kFoldThreads) void embed_fold(int K, int F, int slots, const float* __restrict__ part, float* __restrict__ dW,
                                                            float* __restrict__ db) {
    __shared__ float red[wg::kSumWaves][64];
    const int total = (K + 1) * F, i = blockIdx.x * 64 + (threadIdx.x & 63);
    const float v = wg::slot_sum16(part + i, total, slots, i < total, red);
    if (threadIdx.x < 64 && i < total) {
        const int k = i / F, f = i - k * F;
        if (k < K) dW[f * K + k] = v;
        else if (db) db[f] = v;
    }
}

// ---- class cross-entropy with hit count ----------------------------------------------------------------------------------------------

constexpr int kMaxC = DGN_CLASS_CE_MAX_CLASSES;
constexpr int kCeThreads = kMeanThreads;
constexpr int kCeWaves = kMeanWaves;
constexpr int kCeMinRows = 256;                 // rows per workgroup at least: one per lane

inline MeanLayout ce_layout(int64_t n_rows) { return mean_layout(n_rows, kCeMinRows, true); }

template <int CP>
__global__ __launch_bounds__(kCeThreads) void ce_stats(int64_t G, int C, const float* __restrict__ scores, int64_t ld,
                                                        const int64_t* __restrict__ labels, int64_t per, double* __restrict__ lossp,
                                                        int64_t* __restrict__ cnt, int64_t* __restrict__ hit) {
    __shared__ double s_red[kCeWaves];
    __shared__ unsigned long long s_cnt, s_hit;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t r0 = (int64_t)b * per, r1 = (r0 + per < G) ? r0 + per : G;
    if (tid == 0) { s_cnt = 0ull; s_hit = 0ull; }
    __syncthreads();
    double acc = 0.0;
    unsigned long long rows = 0ull, hits = 0ull;
    for (int64_t n = r0 + tid; n < r1; n += kCeThreads) {
        const int64_t y = labels[n];
        float x[CP];
        load_scores<CP>(x, scores + n * ld, C);                  // (issued with the label's load, not behind it)
        if (y < 0) continue;                                     // a row that does not exist
        const float m = row_max<CP>(x), s = sum_exp<CP>(x, m);
        float xy = NAN;                                          // a label >= C: the row's term is nan, nothing is read for it
        int best = 0;
        float bv = x[0];
#pragma unroll
        for (int c = 0; c < CP; ++c) {
            xy = (c == y && c < C) ? x[c] : xy;
            if (c > 0 && c < C && (x[c] > bv || (x[c] != x[c] && bv == bv))) { bv = x[c]; best = c; }      // first maximum, a NaN above all: torch.argmax
        }
        acc += ((double)m + log((double)s)) - (double)xy;
        ++rows;
        hits += best == y ? 1ull : 0ull;
    }
    if (rows) atomicAdd(&s_cnt, rows);                           // (integers: exact in any order)
    if (hits) atomicAdd(&s_hit, hits);
    const double t = block_sum<kCeWaves>(acc, s_red);            // (its barrier also orders the counts)
    if (tid == 0) { lossp[b] = t; cnt[b] = (int64_t)s_cnt; hit[b] = (int64_t)s_hit; }
}

template <int CP>
__global__ __launch_bounds__(kCeThreads) void ce_rows(int64_t G, int C, const float* __restrict__ scores, int64_t ld,
                                                       const int64_t* __restrict__ labels, int64_t per, int slots,
                                                       const double* __restrict__ lossp, const int64_t* __restrict__ cnt,
                                                       const int64_t* __restrict__ hit, float* __restrict__ loss, int64_t* __restrict__ hits,
                                                       float* __restrict__ g, int64_t ld_g) {
    const int tid = threadIdx.x, b = blockIdx.x;
    int64_t V, n_hit;
    const double total = fold_mean_slots<true>(slots, lossp, cnt, hit, V, n_hit);
    if (b == 0 && tid == 0) {
        *loss = (float)(total / (double)V);                      // no valid row: 0 / 0 = nan, the mean over nothing
        if (hits) *hits = n_hit;
    }
    if (!g) return;
    const float vf = (float)V;
    const int64_t r0 = (int64_t)b * per, r1 = (r0 + per < G) ? r0 + per : G;
    for (int64_t n = r0 + tid; n < r1; n += kCeThreads) {
        const int64_t y = labels[n];
        float x[CP];
        load_scores<CP>(x, scores + n * ld, C);
        float m = 0.f, s = 1.f;
        if (y >= 0) { m = row_max<CP>(x); s = sum_exp<CP>(x, m); }
        const float bad = y >= C ? NAN : 0.f;                    // a label >= C: a nan row, as its loss term
        float* gp = g + n * ld_g;
#pragma unroll
        for (int c = 0; c < CP; ++c)
            if (c < C) gp[c] = y < 0 ? 0.f : (expf(x[c] - m) / s - (c == y ? 1.f : 0.f)) / vf + bad;
    }
}

}  // namespace gcls
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_feat_embed_supported(int32_t k, int32_t f_out) { return gcls::embed_args_ok(k, f_out) ? 1 : 0; }

extern "C" size_t dgn_feat_embed_backward_workspace_bytes(int64_t n_rows, int32_t k, int32_t f_out) {
    if (n_rows < 0 || n_rows > INT32_MAX || !gcls::embed_args_ok(k, f_out)) return 0;
    return gcls::emb_layout(n_rows, k, f_out).bytes;
}

#define DGN_EMBED_DISPATCH(K, LAUNCH)                \
    switch (K) {                                     \
        case 1: LAUNCH(1); break;                    \
        case 2: LAUNCH(2); break;                    \
        case 3: LAUNCH(3); break;                    \
        case 4: LAUNCH(4); break;                    \
        case 5: LAUNCH(5); break;                    \
        case 6: LAUNCH(6); break;                    \
        case 7: LAUNCH(7); break;                    \
        default: LAUNCH(8); break;                   \
    }

extern "C" int dgn_feat_embed_forward(int64_t n_rows, int32_t k, int32_t f_out, const float* x, int64_t ld, const float* w, const float* b,
                                      float* y, int64_t ld_y, void* stream) {
    if (!gcls::embed_args_ok(k, f_out)) {
        set_error("dgn_feat_embed_forward: 1 <= k <= %d and 1 <= f_out <= %d required (got %d, %d)", gcls::kMaxK, gcls::kMaxF, k, f_out);
        return DGN_ERR_INVALID;
    }
    if (!net_io::rows_in_range("dgn_feat_embed_forward", n_rows)) return DGN_ERR_INVALID;
    if (n_rows == 0) return DGN_OK;
    if (!x || !w || !y) { set_error("dgn_feat_embed_forward: null pointer"); return DGN_ERR_INVALID; }
    if (ld < k || ld_y < f_out) { set_error("dgn_feat_embed_forward: row stride below the row's width"); return DGN_ERR_INVALID; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int flat = (ld_y == f_out && al16(y)) ? 1 : 0;
    const dim3 grid((unsigned)((n_rows + gcls::kEmbRows - 1) / gcls::kEmbRows)), block(gcls::kEmbThreads);
#define DGN_EMBED_FWD(K) hipLaunchKernelGGL(gcls::embed_forward<K>, grid, block, 0, st, n_rows, f_out, x, ld, w, b, y, ld_y, flat)
    DGN_EMBED_DISPATCH(k, DGN_EMBED_FWD)
#undef DGN_EMBED_FWD
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_feat_embed_backward(int64_t n_rows, int32_t k, int32_t f_out, const float* x, int64_t ld, const float* g, int64_t ld_g,
                                       float* g_w, float* g_b, void* ws, size_t ws_bytes, void* stream) {
    if (!gcls::embed_args_ok(k, f_out)) {
        set_error("dgn_feat_embed_backward: 1 <= k <= %d and 1 <= f_out <= %d required (got %d, %d)", gcls::kMaxK, gcls::kMaxF, k, f_out);
        return DGN_ERR_INVALID;
    }
    if (!net_io::rows_in_range("dgn_feat_embed_backward", n_rows)) return DGN_ERR_INVALID;
    if (n_rows == 0) return DGN_OK;
    if (!x || !g || !g_w) { set_error("dgn_feat_embed_backward: null pointer"); return DGN_ERR_INVALID; }
    if (ld < k || ld_g < f_out) { set_error("dgn_feat_embed_backward: row stride below the row's width"); return DGN_ERR_INVALID; }
    const gcls::EmbLayout L = gcls::emb_layout(n_rows, k, f_out);
    if (!net_io::workspace_ok("dgn_feat_embed_backward", ws, ws_bytes, L.bytes, 4)) return DGN_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* part = static_cast<float*>(ws);
    const dim3 grid((unsigned)L.groups), block(gcls::kEmbThreads);
#define DGN_EMBED_BWD(K) hipLaunchKernelGGL(gcls::embed_partial<K>, grid, block, 0, st, n_rows, f_out, x, ld, g, ld_g, L.per, part)
    DGN_EMBED_DISPATCH(k, DGN_EMBED_BWD)
#undef DGN_EMBED_BWD
    hipLaunchKernelGGL(gcls::embed_fold, dim3((unsigned)((L.block + 63) / 64)), dim3(gcls::kFoldThreads), 0, st, k, f_out, L.groups,
                       (const float*)part, g_w, g_b);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_class_ce_supported(int32_t n_classes) { return n_classes >= 2 && n_classes <= gcls::kMaxC ? 1 : 0; }

extern "C" size_t dgn_class_ce_workspace_bytes(int64_t n_rows, int32_t n_classes) {
    if (n_rows < 0 || n_rows > INT32_MAX || !dgn_class_ce_supported(n_classes)) return 0;
    return gcls::ce_layout(n_rows).bytes;
}

extern "C" int dgn_class_ce_forward(int64_t n_rows, int32_t n_classes, const float* scores, int64_t ld, const int64_t* labels, float* loss,
                                    int64_t* hits, float* g_scores, int64_t ld_g, void* ws, size_t ws_bytes, void* stream) {
    const int C = n_classes;
    if (!dgn_class_ce_supported(C)) {
        set_error("dgn_class_ce_forward: 2 <= n_classes <= %d required (got %d)", gcls::kMaxC, C);
        return DGN_ERR_INVALID;
    }
    if (!net_io::rows_in_range("dgn_class_ce_forward", n_rows)) return DGN_ERR_INVALID;
    if (!loss) { set_error("dgn_class_ce_forward: null loss"); return DGN_ERR_INVALID; }
    if (n_rows > 0 && (!scores || !labels)) { set_error("dgn_class_ce_forward: null scores / labels"); return DGN_ERR_INVALID; }
    if (ld < C || (g_scores && ld_g < C)) { set_error("dgn_class_ce_forward: row stride below n_classes"); return DGN_ERR_INVALID; }
    const net_io::MeanLayout L = gcls::ce_layout(n_rows);
    if (!net_io::workspace_ok("dgn_class_ce_forward", ws, ws_bytes, L.bytes, 8)) return DGN_ERR_INVALID;
    char* base = static_cast<char*>(ws);
    double* lossp = reinterpret_cast<double*>(base + L.lossp);
    int64_t* cnt = reinterpret_cast<int64_t*>(base + L.cnt);
    int64_t* hit = reinterpret_cast<int64_t*>(base + L.hit);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)L.groups), block(gcls::kCeThreads);
    // (no row: the one workgroup finds nothing valid and the loss is nan, as the mean over an empty selection)
#define DGN_CLASS_CE_LAUNCH(CP)                                                                                                           \
    do {                                                                                                                                  \
        hipLaunchKernelGGL(gcls::ce_stats<CP>, grid, block, 0, st, n_rows, C, scores, ld, labels, L.per, lossp, cnt, hit);                \
        hipLaunchKernelGGL(gcls::ce_rows<CP>, g_scores ? grid : dim3(1), block, 0, st, n_rows, C, scores, ld, labels, L.per, L.groups,   \
                           (const double*)lossp, (const int64_t*)cnt, (const int64_t*)hit, loss, hits, g_scores, ld_g);                   \
    } while (0)
    if (C <= 32) DGN_CLASS_POW2_DISPATCH(C, DGN_CLASS_CE_LAUNCH);
    else DGN_CLASS_CE_LAUNCH(64);
#undef DGN_CLASS_CE_LAUNCH
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_class_ce_backward(int64_t n_rows, int32_t n_classes, const float* g_saved, int64_t ld_g, const float* g_loss,
                                     float* g_scores, int64_t ld_out, void* stream) {
    const int C = n_classes;
    if (!dgn_class_ce_supported(C)) {
        set_error("dgn_class_ce_backward: 2 <= n_classes <= %d required (got %d)", gcls::kMaxC, C);
        return DGN_ERR_INVALID;
    }
    return net_io::loss_backward("dgn_class_ce_backward", "n_classes", n_rows, C, g_saved, ld_g, g_loss, g_scores, ld_out, stream);
}
