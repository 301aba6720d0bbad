// The pieces that the nets' input stages and loss tails share (dgn_mol_io.hip, dgn_node_input.hip, dgn_graph_cls.hip, dgn_node_ce.hip),
// each stated once: they fix the order of the adds, which indices are clamped and how the slots are folded, so a change here reaches every
// kernel that promises those bits.  Everything is inlined into the kernels and entry points of the four units; nothing is launched here.
#pragma once
#include <cmath>
#include <type_traits>

#include "dgn_common.hpp"

namespace dgn {
namespace net_io {

// ---- embedding tables: the separate nn.Embedding weights, their pointers by value in the kernel arguments -----------------------------

constexpr int kMaxCols = DGN_MULTI_EMBEDDING_MAX_COLS;

struct Tables {
    const float* t[kMaxCols];
    int dims[kMaxCols];
};
struct GradTables {
    float* t[kMaxCols];
    int dims[kMaxCols];
    int off[kMaxCols + 1];                      // first row of table c in the combined partial table; off[C] = all the tables' rows
};

inline int64_t table_rows(int32_t n_cols, const int32_t* dims) {
    int64_t rows = 0;
    for (int c = 0; c < n_cols; ++c) rows += dims[c];
    return rows;
}

inline bool tables_ok(int32_t n_cols, const int32_t* dims, int32_t F) {
    if (n_cols < 1 || n_cols > kMaxCols || !dims || F < 1) return false;
    for (int c = 0; c < n_cols; ++c)
        if (dims[c] < 1) return false;
    return true;
}

// dst (Tables or GradTables, zero-initialised) from the caller's arrays; a null table is an error in `who`'s name (`what`: "table")
template <class T, class P>
inline bool fill_tables(const char* who, const char* what, int32_t n_cols, const int32_t* dims, P* const* src, T& dst) {
    for (int c = 0; c < n_cols; ++c) {
        if (!src[c]) { set_error("%s: null %s %d", who, what, c); return false; }
        dst.t[c] = src[c];
        dst.dims[c] = dims[c];
        if constexpr (std::is_same<T, GradTables>::value) dst.off[c + 1] = dst.off[c] + dims[c];
    }
    return true;
}

// an index outside its table is clamped (memory-safe)
__device__ __forceinline__ int clamp_row(int64_t r, int dim) { return r < 0 ? 0 : (r >= dim ? dim - 1 : (int)r); }

// One column of one table's gradient in LDS (tab: the column's element of table row 0, F floats between rows): the rows [r0, r1) of the
// upstream gradient's column gp added at their clamped index, in row order -- the thread owns the column, so its adds are sequential.
__device__ __forceinline__ void scatter_column(float* tab, int dim, int F, const int64_t* ip, int64_t ld_idx, const float* gp, int64_t ld_g,
                                               int64_t r0, int64_t r1) {
    int64_t n = r0;
    for (; n + 4 <= r1; n += 4) {                // four rows' loads in flight, their adds in row order
        int64_t a[4];
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { a[k] = ip[(n + k) * ld_idx]; v[k] = gp[(n + k) * ld_g]; }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float* p = tab + clamp_row(a[k], dim) * F;
            *p = *p + v[k];
        }
    }
    for (; n < r1; ++n) {
        float* p = tab + clamp_row(ip[n * ld_idx], dim) * F;
        *p = *p + gp[n * ld_g];
    }
}

// the table that row `row` < off[C] of the combined partial table belongs to
__device__ __forceinline__ int table_of_row(const GradTables& m, int C, int row) {
    int c = 0;
    while (c + 1 < C && row >= m.off[c + 1]) ++c;
    return c;
}

// ---- a workgroup's n output rows of width F, out[r0 + r, f] = value(r, f) ----------------------------------------------------------------

// flat (ld_out == F, out 16-byte aligned, r0 a multiple of four): the rows leave as 16-byte chunks whatever F is -- a chunk may span two
// rows -- and (n F) mod 4 single floats, the last workgroup's only; otherwise one float per store
template <int THREADS, class Value>
__device__ __forceinline__ void write_rows(float* out, int64_t ld_out, int64_t r0, int n, int F, int flat, const Value& value) {
    const int tid = threadIdx.x, total = n * F;
    if (flat) {
        float* ob = out + r0 * F;
        const int chunks = total >> 2;
        for (int q = tid; q < chunks; q += THREADS) {
            int r = (4 * q) / F, f = 4 * q - r * F;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] = value(r, f);
                if (++f == F) { f = 0; ++r; }
            }
            stv<4>(ob + 4 * q, v);
        }
        for (int i = (chunks << 2) + tid; i < total; i += THREADS) {
            const int r = i / F;
            ob[i] = value(r, i - r * F);
        }
    } else {
        for (int i = tid; i < total; i += THREADS) {
            const int r = i / F, f = i - r * F;
            out[(r0 + r) * ld_out + f] = value(r, f);
        }
    }
}

// ---- a row of C class scores in registers, CP = C rounded up to a power of two -----------------------------------------------------------

// the row's C scores into x[0 .. CP), -inf behind the C-th (exp(-inf - m) = 0: the row loops need no guard)
template <int CP>
__device__ __forceinline__ void load_scores(float (&x)[CP], const float* __restrict__ p, int C) {
#pragma unroll
    for (int c = 0; c < CP; ++c) x[c] = c < C ? p[c] : -INFINITY;
}
// the row's maximum (fmaxf skips a NaN: it comes back through the sum)
template <int CP>
__device__ __forceinline__ float row_max(const float (&x)[CP]) {
    float m = x[0];
#pragma unroll
    for (int c = 1; c < CP; ++c) m = fmaxf(m, x[c]);
    return m;
}
// sum_c exp(x[c] - m) in increasing c
template <int CP>
__device__ __forceinline__ float sum_exp(const float (&x)[CP], float m) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < CP; ++c) s += expf(x[c] - m);
    return s;
}

// LAUNCH(CP) for the power of two CP = 2 .. 32 that holds C classes
#define DGN_CLASS_POW2_DISPATCH(C, LAUNCH) \
    do {                                   \
        if ((C) <= 2) LAUNCH(2);           \
        else if ((C) <= 4) LAUNCH(4);      \
        else if ((C) <= 8) LAUNCH(8);      \
        else if ((C) <= 16) LAUNCH(16);    \
        else LAUNCH(32);                   \
    } while (0)

// ---- masked mean: one (loss partial, count[, hit count]) slot per workgroup of the statistics kernel -------------------------------------

constexpr int kMeanThreads = 256;
constexpr int kMeanWaves = kMeanThreads / kWave;
constexpr int kMeanMaxGroups = 256;             // <= kMeanThreads: the fold takes one slot per thread

struct MeanLayout {
    int groups;
    int64_t per;                                // items per workgroup
    size_t lossp, cnt, hit, bytes;
};
inline MeanLayout mean_layout(int64_t n, int64_t min_per, bool hits) {
    MeanLayout L{};
    const SlotSplit s = slot_split(n, min_per, kMeanMaxGroups);
    L.groups = s.groups < 1 ? 1 : s.groups;     // (no item: one workgroup finds nothing and the loss is nan, the mean over nothing)
    L.per = s.per;
    L.lossp = 0;                                                // double [kMeanMaxGroups]
    L.cnt = L.lossp + kMeanMaxGroups * sizeof(double);          // int64  [kMeanMaxGroups]
    L.hit = L.cnt + kMeanMaxGroups * sizeof(int64_t);           // int64  [kMeanMaxGroups], with hits only
    L.bytes = L.hit + (hits ? kMeanMaxGroups * sizeof(int64_t) : 0);
    return L;
}

// Every workgroup of the rows kernel folds the slots for itself: the counts by integer atomics into zeroed LDS counters (exact in any
// order), the loss partials by block_sum, whose barrier also orders the counts.  Returns the loss sum; count (and n_hit with HITS).
template <bool HITS>
__device__ __forceinline__ double fold_mean_slots(int slots, const double* __restrict__ lossp, const int64_t* __restrict__ cnt,
                                                  const int64_t* __restrict__ hit, int64_t& count, int64_t& n_hit) {
    __shared__ double s_red[kMeanWaves];
    __shared__ unsigned long long s_n[HITS ? 2 : 1];
    const int tid = threadIdx.x;
    if (tid == 0) { s_n[0] = 0ull; if (HITS) s_n[1] = 0ull; }
    __syncthreads();
    if (tid < slots) {
        if (cnt[tid] > 0) atomicAdd(&s_n[0], (unsigned long long)cnt[tid]);
        if (HITS && hit[tid] > 0) atomicAdd(&s_n[1], (unsigned long long)hit[tid]);
    }
    const double total = block_sum<kMeanWaves>(tid < slots ? lossp[tid] : 0.0, s_red);
    count = (int64_t)s_n[0];
    n_hit = HITS ? (int64_t)s_n[1] : 0;
    return total;
}

// ---- host-side checks of the entry points; `who`: the entry point's name for the error text ----------------------------------------------

inline bool rows_in_range(const char* who, int64_t n_rows) {
    if (n_rows >= 0 && n_rows <= INT32_MAX) return true;
    set_error("%s: n_rows beyond the int32 range", who);
    return false;
}

using dgn::workspace_ok;      // (dgn_common.hpp, beside the workspace layout helpers)

// the autograd backward of a loss that saved its gradient: g_scores = g_saved * *g_loss over n_rows x width (`what`: the width's name)
inline int loss_backward(const char* who, const char* what, int64_t n_rows, int32_t width, const float* g_saved, int64_t ld_g,
                         const float* g_loss, float* g_scores, int64_t ld_out, void* stream) {
    if (!rows_in_range(who, n_rows)) return DGN_ERR_INVALID;
    if (n_rows == 0) return DGN_OK;
    if (!g_saved || !g_loss || !g_scores) { set_error("%s: null pointer", who); return DGN_ERR_INVALID; }
    if (ld_g < width || ld_out < width) { set_error("%s: row stride below %s", who, what); return DGN_ERR_INVALID; }
    if (n_rows * width > (int64_t)INT32_MAX * 64) { set_error("%s: n_rows x %s beyond the grid range", who, what); return DGN_ERR_INVALID; }
    return scale_rows_async(n_rows, width, g_saved, ld_g, g_loss, g_scores, ld_out, static_cast<hipStream_t>(stream));
}

}  // namespace net_io
}  // namespace dgn
