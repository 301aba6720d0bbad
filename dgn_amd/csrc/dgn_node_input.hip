// Input stage of the nets with positional encodings, h = embedding_h(h) + embedding_pos_enc(g.ndata['pos_enc'])
// (nets/molecules_graph_regression/dgn_net.py:60-62, nets/SBMs_node_classification/dgn_net.py:57-59, nets/HIV_graph_classification/
// dgn_net.py:64-66): the sum of C embedding lookups (one table, or OGB's nine) plus an nn.Linear(K <= 40, hidden) on the Laplacian
// eigenvector columns, forward in one launch and the gradients of all tables, the weight and the bias in one pass over the upstream
// gradient.  Nothing read back, no floating-point atomics, fixed-order reductions (the same input gives the same bits), every launch
// parameter a function of the shapes alone.
//
//   forward           one workgroup per kFwdRows rows: W (transposed), b, the rows' pe and their clamped table rows in LDS; an output is
//                     (((0 + T_0[i_0]) + T_1[i_1]) + ...) + fmaf(W[f, K-1], pe[K-1], ... fmaf(W[f, 0], pe[0], b[f])): the table terms in
//                     column order, the linear terms in increasing k from the bias on, the two partial results added last.  Dense output
//                     rows leave as flat 16-byte chunks whatever F is (net_io::write_rows).
//   backward_partial  one workgroup per contiguous row range, one combined [sum(dims) + K + 1, F] block in LDS: the table rows at
//                     GradTables::off, then K rows dW[:, k] and one row db.  Thread (q, f) owns column f of table q
//                     (net_io::scatter_column), of dW[:, k] or of db and walks the range's rows in order: a column's adds are sequential
//                     and no two threads share an address
//   backward_fold     the workgroups' blocks added in a fixed order (wg::slot_sum16), the table rows written to the separate tables, dW in
//                     torch's [F, K] layout, db
//
// The tables' pointers travel in the kernel arguments (net_io::Tables, a struct by value).  Indices outside a table are clamped.
// pe is read with 4-byte loads only: the nets pass eig[:, 1:K+1], a column slice whose base is 4-byte aligned and no more.
#include <hip/hip_runtime.h>

#include "dgn_net_io.hpp"
#include "dgn_wgrad.hpp"

namespace dgn {
namespace node_input {

using namespace net_io;

constexpr int kMaxK = DGN_NODE_INPUT_MAX_K;
constexpr int kLdsFloats = 160 * 1024 / 4;      // the combined partial block of one workgroup: the CU's whole LDS
constexpr int kFwdThreads = 256;
constexpr int kFwdRows = 64;                    // rows per forward workgroup; a multiple of four: every workgroup's flat range begins on a chunk
constexpr int kBwdThreads = 1024;               // (C + K + 1) F columns to own (ZINC at hidden 70, K = 8: 700)
constexpr int kMaxGroups = 256;
constexpr int kMinRows = 64;                    // rows per workgroup at least: few partial blocks to fold for small batches
constexpr int kFoldThreads = wg::kSumWaves * kWave;

static_assert(kFwdRows % 4 == 0, "forward's flat chunks");

struct Grads {
    GradTables tab;                             // tab.off[C] = first row of dW in the combined block
    float* dw;                                  // [F, K]
    float* db;                                  // [F] or NULL
};

struct Layout {
    int groups;
    int64_t per;                                // rows per workgroup
    int64_t total;                              // floats of the combined block
    size_t bytes;
};

inline bool args_ok(int32_t n_cols, const int32_t* dims, int32_t K, int32_t F) { return tables_ok(n_cols, dims, F) && K >= 1 && K <= kMaxK; }

inline int64_t block_floats(int32_t n_cols, const int32_t* dims, int32_t K, int32_t F) { return (table_rows(n_cols, dims) + K + 1) * (int64_t)F; }
// forward: W^T [K, F], b [F], pe [kFwdRows, K], clamped rows [kFwdRows, C]
inline int64_t forward_floats(int32_t n_cols, int32_t K, int32_t F) { return (int64_t)(K + 1) * F + (int64_t)kFwdRows * (K + n_cols); }

inline bool fits(int32_t n_cols, const int32_t* dims, int32_t K, int32_t F) {
    return block_floats(n_cols, dims, K, F) <= kLdsFloats && forward_floats(n_cols, K, F) <= kLdsFloats;
}

inline Layout layout(int64_t n_rows, int64_t total) {
    Layout L{};
    const SlotSplit s = slot_split(n_rows, kMinRows, kMaxGroups);
    L.groups = s.groups;
    L.per = s.per;
    L.total = total;
    L.bytes = (size_t)s.bound * (size_t)total * sizeof(float);       // sized by the upper bound of `groups`
    return L;
}

__global__ __launch_bounds__(kFwdThreads) void node_input_forward(int64_t N, int C, int K, int F, const int64_t* __restrict__ idx, int64_t ld_idx,
                                                                   Tables tb, const float* __restrict__ pe, int64_t ld_pe,
                                                                   const float* __restrict__ W, const float* __restrict__ b,
                                                                   float* __restrict__ out, int64_t ld_out, int flat) {
    extern __shared__ __attribute__((aligned(16))) float s_fwd[];
    float* s_w = s_fwd;                          // [K][F]
    float* s_b = s_w + K * F;                    // [F]
    float* s_pe = s_b + F;                       // [kFwdRows][K]
    int* s_row = reinterpret_cast<int*>(s_pe + kFwdRows * K);      // [kFwdRows][C]
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kFwdRows;
    const int n = (int)(N - r0 < kFwdRows ? N - r0 : kFwdRows);
    for (int i = tid; i < F * K; i += kFwdThreads) { const int f = i / K; s_w[(i - f * K) * F + f] = W[i]; }
    for (int i = tid; i < F; i += kFwdThreads) s_b[i] = b ? b[i] : 0.f;
    for (int i = tid; i < n * K; i += kFwdThreads) { const int r = i / K, k = i - r * K; s_pe[i] = pe[(r0 + r) * ld_pe + k]; }
    for (int i = tid; i < n * C; i += kFwdThreads) { const int r = i / C, c = i - r * C; s_row[i] = clamp_row(idx[(r0 + r) * ld_idx + c], tb.dims[c]); }
    __syncthreads();
    auto value = [&](int r, int f) {
        float t = 0.f;
        const int* rows = s_row + r * C;
        for (int c = 0; c < C; ++c) t = t + tb.t[c][(int64_t)rows[c] * F + f];
        float a = s_b[f];
        const float* x = s_pe + r * K;
        for (int k = 0; k < K; ++k) a = fmaf(s_w[k * F + f], x[k], a);
        return t + a;
    };
    write_rows<kFwdThreads>(out, ld_out, r0, n, F, flat, value);
}

__global__ __launch_bounds__(kBwdThreads) void node_input_backward_partial(int64_t N, int C, int K, int F, const int64_t* __restrict__ idx,
                                                                            int64_t ld_idx, Grads m, const float* __restrict__ pe, int64_t ld_pe,
                                                                            const float* __restrict__ g, int64_t ld_g, int64_t per,
                                                                            float* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float s_blk[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int lin0 = m.tab.off[C];               // first row of dW[:, 0]
    const int total = (lin0 + K + 1) * F;
    for (int i = tid; i < total; i += kBwdThreads) s_blk[i] = 0.f;
    __syncthreads();
    const int64_t r0 = (int64_t)b * per, r1 = (r0 + per < N) ? r0 + per : N;
    const int items = (C + K + 1) * F;
    for (int it = tid; it < items; it += kBwdThreads) {
        const int q = it / F, f = it - q * F;
        const float* gp = g + f;
        int64_t n = r0;
        if (q < C) {                             // column f of table q
            scatter_column(s_blk + m.tab.off[q] * F + f, m.tab.dims[q], F, idx + q, ld_idx, gp, ld_g, r0, r1);
        } else if (q < C + K) {                  // dW[f, k]
            const float* pp = pe + (q - C);
            float acc = 0.f;
            for (; n + 4 <= r1; n += 4) {
                float x[4], v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) { x[k] = pp[(n + k) * ld_pe]; v[k] = gp[(n + k) * ld_g]; }
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = fmaf(v[k], x[k], acc);
            }
            for (; n < r1; ++n) acc = fmaf(gp[n * ld_g], pp[n * ld_pe], acc);
            s_blk[(lin0 + q - C) * F + f] = acc;
        } else {                                 // db[f]
            float acc = 0.f;
            for (; n + 4 <= r1; n += 4) {
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = gp[(n + k) * ld_g];
#pragma unroll
                for (int k = 0; k < 4; ++k) acc += v[k];
            }
            for (; n < r1; ++n) acc += gp[n * ld_g];
            s_blk[(lin0 + K) * F + f] = acc;
        }
    }
    __syncthreads();
    float* dst = part + (int64_t)b * total;
    for (int i = tid; i < total; i += kBwdThreads) dst[i] = s_blk[i];
}

// element i = row F + f of the combined blocks: rows below off[C] belong to the tables, the next K are dW[:, k], the last is db
__global__ __launch_bounds__(kFoldThreads) void node_input_backward_fold(int C, int K, int F, int slots, Grads m, const float* __restrict__ part,
                                                                          int total) {
    __shared__ float red[wg::kSumWaves][64];
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const float v = wg::slot_sum16(part + i, total, slots, i < total, red);
    if (threadIdx.x < 64 && i < total) {
        const int row = i / F, f = i - row * F, lin0 = m.tab.off[C];
        if (row < lin0) {
            const int c = table_of_row(m.tab, C, row);
            m.tab.t[c][(int64_t)(row - m.tab.off[c]) * F + f] = v;
        } else if (row < lin0 + K) {
            m.dw[(int64_t)f * K + (row - lin0)] = v;
        } else if (m.db) {
            m.db[f] = v;
        }
    }
}

}  // namespace node_input
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_node_input_supported(int32_t n_cols, const int32_t* dims, int32_t k, int32_t F) {
    return node_input::args_ok(n_cols, dims, k, F) && node_input::fits(n_cols, dims, k, F) ? 1 : 0;
}

extern "C" size_t dgn_node_input_backward_workspace_bytes(int64_t n_rows, int32_t n_cols, const int32_t* dims, int32_t k, int32_t F) {
    if (n_rows < 0 || n_rows > INT32_MAX || !dgn_node_input_supported(n_cols, dims, k, F)) return 0;
    return node_input::layout(n_rows, node_input::block_floats(n_cols, dims, k, F)).bytes;
}

extern "C" int dgn_node_input_forward(int64_t n_rows, int32_t n_cols, int32_t k, int32_t F, const int64_t* idx, int64_t ld_idx,
                                      const float* const* tables, const int32_t* dims, const float* pe, int64_t ld_pe, const float* w,
                                      const float* b, float* out, int64_t ld_out, void* stream) {
    if (!node_input::args_ok(n_cols, dims, k, F)) {
        set_error("dgn_node_input_forward: 1 <= n_cols <= %d tables of at least one row, 1 <= k <= %d and F >= 1 required", net_io::kMaxCols,
                  node_input::kMaxK);
        return DGN_ERR_INVALID;
    }
    if (!node_input::fits(n_cols, dims, k, F)) {
        set_error("dgn_node_input_forward: the shape exceeds the LDS budget of %d floats (dgn_node_input_supported)", node_input::kLdsFloats);
        return DGN_ERR_INVALID;
    }
    if (!net_io::rows_in_range("dgn_node_input_forward", n_rows)) return DGN_ERR_INVALID;
    if (n_rows == 0) return DGN_OK;
    if (!idx || !tables || !pe || !w || !out) { set_error("dgn_node_input_forward: null pointer"); return DGN_ERR_INVALID; }
    if (ld_idx < n_cols || ld_pe < k || ld_out < F) { set_error("dgn_node_input_forward: row stride below the row's width"); return DGN_ERR_INVALID; }
    net_io::Tables tb{};
    if (!net_io::fill_tables("dgn_node_input_forward", "table", n_cols, dims, tables, tb)) return DGN_ERR_INVALID;
    const int lds = (int)(node_input::forward_floats(n_cols, k, F) * sizeof(float));
    static LdsOptIn lds_ok{0};
    DGN_HIP_CHECK(allow_lds(lds_ok, node_input::kLdsFloats * (int)sizeof(float), &node_input::node_input_forward));
    const int flat = (ld_out == F && al16(out)) ? 1 : 0;
    const int64_t blocks = (n_rows + node_input::kFwdRows - 1) / node_input::kFwdRows;
    hipLaunchKernelGGL(node_input::node_input_forward, dim3((unsigned)blocks), dim3(node_input::kFwdThreads), (size_t)lds,
                       static_cast<hipStream_t>(stream), n_rows, n_cols, k, F, idx, ld_idx, tb, pe, ld_pe, w, b, out, ld_out, flat);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_node_input_backward(int64_t n_rows, int32_t n_cols, int32_t k, int32_t F, const int64_t* idx, int64_t ld_idx,
                                       const int32_t* dims, const float* pe, int64_t ld_pe, const float* g, int64_t ld_g,
                                       float* const* g_tables, float* g_w, float* g_b, void* ws, size_t ws_bytes, void* stream) {
    if (!node_input::args_ok(n_cols, dims, k, F)) {
        set_error("dgn_node_input_backward: 1 <= n_cols <= %d tables of at least one row, 1 <= k <= %d and F >= 1 required", net_io::kMaxCols,
                  node_input::kMaxK);
        return DGN_ERR_INVALID;
    }
    if (!node_input::fits(n_cols, dims, k, F)) {
        set_error("dgn_node_input_backward: the shape exceeds the LDS budget of %d floats (dgn_node_input_supported)", node_input::kLdsFloats);
        return DGN_ERR_INVALID;
    }
    if (!net_io::rows_in_range("dgn_node_input_backward", n_rows)) return DGN_ERR_INVALID;
    if (n_rows == 0) return DGN_OK;
    if (!idx || !pe || !g || !g_tables || !g_w) { set_error("dgn_node_input_backward: null pointer"); return DGN_ERR_INVALID; }
    if (ld_idx < n_cols || ld_pe < k || ld_g < F) { set_error("dgn_node_input_backward: row stride below the row's width"); return DGN_ERR_INVALID; }
    node_input::Grads m{};
    if (!net_io::fill_tables("dgn_node_input_backward", "gradient table", n_cols, dims, g_tables, m.tab)) return DGN_ERR_INVALID;
    m.dw = g_w;
    m.db = g_b;
    const int64_t total = node_input::block_floats(n_cols, dims, k, F);
    const node_input::Layout L = node_input::layout(n_rows, total);
    if (!net_io::workspace_ok("dgn_node_input_backward", ws, ws_bytes, L.bytes, 4)) return DGN_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    static LdsOptIn lds_ok{0};
    DGN_HIP_CHECK(allow_lds(lds_ok, node_input::kLdsFloats * (int)sizeof(float), &node_input::node_input_backward_partial));
    float* part = static_cast<float*>(ws);
    hipLaunchKernelGGL(node_input::node_input_backward_partial, dim3((unsigned)L.groups), dim3(node_input::kBwdThreads),
                       (size_t)total * sizeof(float), st, n_rows, n_cols, k, F, idx, ld_idx, m, pe, ld_pe, g, ld_g, L.per, part);
    hipLaunchKernelGGL(node_input::node_input_backward_fold, dim3((unsigned)((total + 63) / 64)), dim3(node_input::kFoldThreads), 0, st, n_cols, k,
                       F, L.groups, m, (const float*)part, (int)total);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}
