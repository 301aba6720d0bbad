// Input encoders and loss of the OGB molecule nets (nets/HIV_graph_classification/dgn_net.py:41-44, :62, :68, :87-89 and
// nets/PCBA_graph_classification/dgn_net.py:36-39, :67, :70, :99-102; train/train_PCBA_graph_classification.py:32-33): the sum of C
// embedding lookups (OGB's AtomEncoder: nine tables, BondEncoder: three) forward and backward, and the binary cross-entropy with logits
// over the labelled entries of a [G, T] label matrix in which NaN means "not measured".  Nothing read back, no floating-point atomics,
// fixed-order reductions (the same input gives the same bits), every launch parameter a function of the shapes alone.
//
//   emb_forward           one thread per (row, 1 / 2 / 4 consecutive features): h = ((0 + T_0[i_0]) + T_1[i_1]) + ... in column order --
//                         the very adds of the torch composition, so the result is bit-equal to it
//   emb_backward_partial  one workgroup per contiguous row range, all C tables as one partial table in LDS; thread (c, f) owns column f of
//                         table c and walks the range's rows in order (net_io::scatter_column): a column's adds are sequential, no two
//                         threads share an address
//   emb_backward_fold     one thread per table element: the workgroups' partials added in workgroup order (fp64), written to table c
//   bce_stats             one workgroup per contiguous element range: labelled count (integer) and the fp64 sum of the loss terms
//   bce_rows              every workgroup folds the slots (net_io::fold_mean_slots), block 0 writes the loss; then the gradient of its range
//   (both instantiated twice: BceTerm, and L1Term for the masked L1 of the graph-regression net, nets/molecules_graph_regression/
//    dgn_net.py:90-92 -- dgn_masked_mae_*)
//   (net_io::loss_backward: the autograd backward, g_saved * *g_loss)
//
// The tables' pointers travel in the kernel arguments (net_io::Tables, a struct by value): the parameters stay the separate nn.Embedding
// weights of the state_dict and a captured graph holds their addresses like every other parameter's.  Indices outside a table are clamped.
// The table structs, the slot layout of the masked mean and the host-side checks are those of dgn_net_io.hpp.
#include <hip/hip_runtime.h>

#include <cmath>

#include "dgn_net_io.hpp"

namespace dgn {
namespace mol_io {

using namespace net_io;

constexpr int kLdsFloats = 160 * 1024 / 4;      // the partial tables of one workgroup: the CU's whole LDS (OGB atoms: 173 rows -> F <= 236)
constexpr int kFwdThreads = 256;
constexpr int kBwdThreads = 1024;               // C F columns to own (atoms at hidden 70: 630)
constexpr int kMaxGroups = 256;
constexpr int kMinRows = 64;                    // rows per workgroup at least: few partial tables to fold for small batches
constexpr int kFoldThreads = 256;

struct EmbLayout {
    int groups;
    int64_t per;                                // rows per workgroup
    int64_t total;                              // floats of the combined table
    size_t bytes;
};

inline EmbLayout emb_layout(int64_t n_rows, int64_t total) {
    EmbLayout L{};
    const SlotSplit s = slot_split(n_rows, kMinRows, kMaxGroups);
    L.groups = s.groups < 1 ? 1 : s.groups;
    L.per = s.per;
    L.total = total;
    L.bytes = (size_t)s.bound * (size_t)total * sizeof(float);       // sized by the upper bound of `groups`
    return L;
}

template <int VEC>
__global__ __launch_bounds__(kFwdThreads) void emb_forward(int64_t N, int C, int F, const int64_t* __restrict__ idx, int64_t ld_idx, Tables tb,
                                                           float* __restrict__ out, int64_t ld_out) {
    const int fv = F / VEC;
    const int64_t i = (int64_t)blockIdx.x * kFwdThreads + threadIdx.x;
    if (i >= N * fv) return;
    const int64_t n = i / fv;
    const int f = (int)(i - n * fv) * VEC;
    float acc[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
    const int64_t* ip = idx + n * ld_idx;
    for (int c = 0; c < C; ++c) {
        const int r = clamp_row(ip[c], tb.dims[c]);
        float v[VEC];
        ldv<VEC>(v, tb.t[c] + (int64_t)r * F + f);
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = acc[k] + v[k];
    }
    stv<VEC>(out + n * ld_out + f, acc);
}

__global__ __launch_bounds__(kBwdThreads) void emb_backward_partial(int64_t N, int C, int F, const int64_t* __restrict__ idx, int64_t ld_idx,
                                                                     GradTables m, const float* __restrict__ g, int64_t ld_g, int64_t per,
                                                                     float* __restrict__ part) {
    extern __shared__ float s_tab[];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int total = m.off[C] * F;
    for (int i = tid; i < total; i += kBwdThreads) s_tab[i] = 0.f;
    __syncthreads();
    const int64_t r0 = (int64_t)b * per, r1 = (r0 + per < N) ? r0 + per : N;
    const int items = C * F;
    for (int it = tid; it < items; it += kBwdThreads) {
        const int c = it / F, f = it - c * F;
        scatter_column(s_tab + m.off[c] * F + f, m.dims[c], F, idx + c, ld_idx, g + f, ld_g, r0, r1);
    }
    __syncthreads();
    float* dst = part + (int64_t)b * total;
    for (int i = tid; i < total; i += kBwdThreads) dst[i] = s_tab[i];
}

__global__ __launch_bounds__(kFoldThreads) void emb_backward_fold(int C, int F, int G, GradTables m, const float* __restrict__ part, int total) {
    const int i = blockIdx.x * kFoldThreads + threadIdx.x;
    if (i >= total) return;
    double s = 0.0;
#pragma unroll 8
    for (int gidx = 0; gidx < G; ++gidx) s += (double)part[(int64_t)gidx * total + i];
    const int row = i / F, f = i - row * F;
    const int c = table_of_row(m, C, row);
    m.t[c][(int64_t)(row - m.off[c]) * F + f] = (float)s;
}

// ---- masked binary cross-entropy with logits ----------------------------------------------------------------------------------------

constexpr int kBceThreads = kMeanThreads;
constexpr int kBceWaves = kMeanWaves;
constexpr int kBceMinElems = 2048;              // elements per workgroup at least

inline MeanLayout bce_layout(int64_t n) { return mean_layout(n, kBceMinElems, false); }

// The per-entry term of a masked mean loss and its gradient (x: score, y: target, not NaN).  nf = (float)count and inv = (float)(1 / count)
// are both at hand: each term keeps the arithmetic of the loss it replaces.
struct BceTerm {      // BCEWithLogitsLoss
    static __device__ __forceinline__ float loss(float xv, float yv) { return (fmaxf(xv, 0.f) - xv * yv) + log1pf(expf(-fabsf(xv))); }
    static __device__ __forceinline__ float grad(float xv, float yv, float nf, float) {
        const float e = expf(-fabsf(xv));                        // sigmoid without an overflow at either end
        const float s = xv >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
        return (s - yv) / nf;
    }
};
struct L1Term {       // L1Loss: |x - y|, gradient sign(x - y) / count with sign(0) = 0 (torch's l1_loss backward)
    static __device__ __forceinline__ float loss(float xv, float yv) { return fabsf(xv - yv); }
    static __device__ __forceinline__ float grad(float xv, float yv, float, float inv) {
        const float d = xv - yv;
        return d > 0.f ? inv : (d < 0.f ? -inv : 0.f);
    }
};

template <class Term>
__global__ __launch_bounds__(kBceThreads) void bce_stats(int64_t n, int T, const float* __restrict__ x, int64_t ld, const float* __restrict__ y,
                                                          int64_t ld_y, int64_t per, double* __restrict__ lossp, int64_t* __restrict__ cnt) {
    __shared__ double s_red[kBceWaves];
    __shared__ unsigned long long s_cnt;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t e0 = (int64_t)b * per, e1 = (e0 + per < n) ? e0 + per : n;
    if (tid == 0) s_cnt = 0ull;
    __syncthreads();
    double acc = 0.0;
    unsigned long long mine = 0ull;
    for (int64_t i = e0 + tid; i < e1; i += kBceThreads) {
        const int64_t r = i / T;
        const int c = (int)(i - r * T);
        const float xv = x[r * ld + c], yv = y[r * ld_y + c];
        if (yv == yv) {                                          // labelled
            const float term = Term::loss(xv, yv);
            acc += (double)term;
            ++mine;
        }
    }
    if (mine) atomicAdd(&s_cnt, mine);                           // (integer: exact in any order)
    const double t = block_sum<kBceWaves>(acc, s_red);                      // (its barrier also orders the count)
    if (tid == 0) { lossp[b] = t; cnt[b] = (int64_t)s_cnt; }
}

template <class Term>
__global__ __launch_bounds__(kBceThreads) void bce_rows(int64_t n, int T, const float* __restrict__ x, int64_t ld, const float* __restrict__ y,
                                                         int64_t ld_y, int64_t per, int G, const double* __restrict__ lossp,
                                                         const int64_t* __restrict__ cnt, float* __restrict__ loss, float* __restrict__ g,
                                                         int64_t ld_g) {
    const int tid = threadIdx.x, b = blockIdx.x;
    int64_t labelled, unused;
    const double total = fold_mean_slots<false>(G, lossp, cnt, nullptr, labelled, unused);
    // no labelled entry: 0 / 0 = nan, the mean over an empty selection (train_PCBA_graph_classification.py:32-33)
    if (b == 0 && tid == 0) *loss = (float)(total / (double)labelled);
    if (!g) return;
    const float nf = (float)labelled, inv = (float)(1.0 / (double)labelled);
    const int64_t e0 = (int64_t)b * per, e1 = (e0 + per < n) ? e0 + per : n;
    for (int64_t i = e0 + tid; i < e1; i += kBceThreads) {
        const int64_t r = i / T;
        const int c = (int)(i - r * T);
        const float xv = x[r * ld + c], yv = y[r * ld_y + c];
        float gv = 0.f;                                          // unlabelled: exactly zero
        if (yv == yv) gv = Term::grad(xv, yv, nf, inv);
        g[r * ld_g + c] = gv;
    }
}

}  // namespace mol_io
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_multi_embedding_supported(int32_t n_cols, const int32_t* dims, int32_t F) {
    if (!net_io::tables_ok(n_cols, dims, F)) return 0;
    return net_io::table_rows(n_cols, dims) * (int64_t)F <= mol_io::kLdsFloats ? 1 : 0;
}

extern "C" size_t dgn_multi_embedding_backward_workspace_bytes(int64_t n_rows, int32_t n_cols, const int32_t* dims, int32_t F) {
    if (n_rows < 0 || n_rows > INT32_MAX || !dgn_multi_embedding_supported(n_cols, dims, F)) return 0;
    return mol_io::emb_layout(n_rows, net_io::table_rows(n_cols, dims) * F).bytes;
}

extern "C" int dgn_multi_embedding_forward(int64_t n_rows, int32_t n_cols, int32_t F, const int64_t* idx, int64_t ld_idx, const float* const* tables,
                                           const int32_t* dims, float* out, int64_t ld_out, void* stream) {
    if (!net_io::tables_ok(n_cols, dims, F)) {
        set_error("dgn_multi_embedding_forward: 1 <= n_cols <= %d tables of at least one row and F >= 1 required", net_io::kMaxCols);
        return DGN_ERR_INVALID;
    }
    if (!net_io::rows_in_range("dgn_multi_embedding_forward", n_rows)) return DGN_ERR_INVALID;
    if (n_rows == 0) return DGN_OK;
    if (!idx || !tables || !out) { set_error("dgn_multi_embedding_forward: null pointer"); return DGN_ERR_INVALID; }
    if (ld_idx < n_cols || ld_out < F) { set_error("dgn_multi_embedding_forward: row stride below the row's width"); return DGN_ERR_INVALID; }
    net_io::Tables tb{};
    if (!net_io::fill_tables("dgn_multi_embedding_forward", "table", n_cols, dims, tables, tb)) return DGN_ERR_INVALID;
    uintptr_t align = reinterpret_cast<uintptr_t>(out) | (uintptr_t)(ld_out * sizeof(float)) | (uintptr_t)((int64_t)F * sizeof(float));
    for (int c = 0; c < n_cols; ++c) align |= reinterpret_cast<uintptr_t>(tables[c]);
    const int vec = (align & 15) == 0 ? 4 : ((align & 7) == 0 ? 2 : 1);     // 16-byte pieces where the rows allow them
    const int64_t blocks = (n_rows * (F / vec) + mol_io::kFwdThreads - 1) / mol_io::kFwdThreads;
    if (blocks > INT32_MAX) { set_error("dgn_multi_embedding_forward: n_rows x F beyond the grid range"); return DGN_ERR_INVALID; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks), block(mol_io::kFwdThreads);
    if (vec == 4) hipLaunchKernelGGL(mol_io::emb_forward<4>, grid, block, 0, st, n_rows, n_cols, F, idx, ld_idx, tb, out, ld_out);
    else if (vec == 2) hipLaunchKernelGGL(mol_io::emb_forward<2>, grid, block, 0, st, n_rows, n_cols, F, idx, ld_idx, tb, out, ld_out);
    else hipLaunchKernelGGL(mol_io::emb_forward<1>, grid, block, 0, st, n_rows, n_cols, F, idx, ld_idx, tb, out, ld_out);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_multi_embedding_backward(int64_t n_rows, int32_t n_cols, int32_t F, const int64_t* idx, int64_t ld_idx, const int32_t* dims,
                                            const float* g, int64_t ld_g, float* const* g_tables, void* ws, size_t ws_bytes, void* stream) {
    if (!net_io::tables_ok(n_cols, dims, F)) {
        set_error("dgn_multi_embedding_backward: 1 <= n_cols <= %d tables of at least one row and F >= 1 required", net_io::kMaxCols);
        return DGN_ERR_INVALID;
    }
    if (!net_io::rows_in_range("dgn_multi_embedding_backward", n_rows)) return DGN_ERR_INVALID;
    const int64_t total = net_io::table_rows(n_cols, dims) * F;
    if (total > mol_io::kLdsFloats) {
        set_error("dgn_multi_embedding_backward: %lld table floats exceed the LDS budget of %d (dgn_multi_embedding_supported)", (long long)total,
                  mol_io::kLdsFloats);
        return DGN_ERR_INVALID;
    }
    if (!g_tables) { set_error("dgn_multi_embedding_backward: null pointer"); return DGN_ERR_INVALID; }
    net_io::GradTables m{};
    if (!net_io::fill_tables("dgn_multi_embedding_backward", "gradient table", n_cols, dims, g_tables, m)) return DGN_ERR_INVALID;
    if (n_rows > 0 && (!idx || !g)) { set_error("dgn_multi_embedding_backward: null pointer"); return DGN_ERR_INVALID; }
    if (n_rows > 0 && (ld_idx < n_cols || ld_g < F)) { set_error("dgn_multi_embedding_backward: row stride below the row's width"); return DGN_ERR_INVALID; }
    const mol_io::EmbLayout L = mol_io::emb_layout(n_rows, total);
    if (!net_io::workspace_ok("dgn_multi_embedding_backward", ws, ws_bytes, L.bytes, 4)) return DGN_ERR_INVALID;
    hipStream_t st = static_cast<hipStream_t>(stream);
    static LdsOptIn lds_ok{0};
    DGN_HIP_CHECK(allow_lds(lds_ok, mol_io::kLdsFloats * (int)sizeof(float), &mol_io::emb_backward_partial));
    float* part = static_cast<float*>(ws);
    // (no row: one workgroup leaves a zero partial table, the fold writes the zero gradients)
    hipLaunchKernelGGL(mol_io::emb_backward_partial, dim3((unsigned)L.groups), dim3(mol_io::kBwdThreads), (size_t)total * sizeof(float), st, n_rows,
                       n_cols, F, idx, ld_idx, m, g, ld_g, L.per, part);
    hipLaunchKernelGGL(mol_io::emb_backward_fold, dim3((unsigned)((total + mol_io::kFoldThreads - 1) / mol_io::kFoldThreads)),
                       dim3(mol_io::kFoldThreads), 0, st, n_cols, F, L.groups, m, (const float*)part, (int)total);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" size_t dgn_masked_bce_workspace_bytes(int64_t n_rows, int32_t n_tasks) {
    if (n_rows < 0 || n_tasks < 1 || n_rows > INT32_MAX) return 0;
    return mol_io::bce_layout(n_rows * n_tasks).bytes;
}

// the two launches of a masked mean loss; `who`: the entry point's name for the error text
template <class Term>
static int masked_mean_forward(const char* who, int64_t n_rows, int32_t n_tasks, const float* scores, int64_t ld, const float* labels, int64_t ld_y,
                               float* loss, float* g_scores, int64_t ld_g, void* ws, size_t ws_bytes, void* stream) {
    const int T = n_tasks;
    if (T < 1) { set_error("%s: n_tasks >= 1 required (got %d)", who, T); return DGN_ERR_INVALID; }
    if (!net_io::rows_in_range(who, n_rows)) return DGN_ERR_INVALID;
    if (!loss) { set_error("%s: null loss", who); return DGN_ERR_INVALID; }
    if (n_rows > 0 && (!scores || !labels)) { set_error("%s: null scores / labels", who); return DGN_ERR_INVALID; }
    if (ld < T || ld_y < T || (g_scores && ld_g < T)) { set_error("%s: row stride below n_tasks", who); return DGN_ERR_INVALID; }
    const int64_t n = n_rows * T;
    if (n > (int64_t)INT32_MAX * 64) { set_error("%s: n_rows x n_tasks beyond the grid range", who); return DGN_ERR_INVALID; }
    const net_io::MeanLayout L = mol_io::bce_layout(n);
    if (!net_io::workspace_ok(who, ws, ws_bytes, L.bytes, 8)) return DGN_ERR_INVALID;
    char* base = static_cast<char*>(ws);
    double* lossp = reinterpret_cast<double*>(base + L.lossp);
    int64_t* cnt = reinterpret_cast<int64_t*>(base + L.cnt);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)L.groups), block(mol_io::kBceThreads);
    // (no row: the one workgroup finds nothing labelled and the loss is nan, as the mean over an empty selection)
    hipLaunchKernelGGL(mol_io::bce_stats<Term>, grid, block, 0, st, n, T, scores, ld, labels, ld_y, L.per, lossp, cnt);
    hipLaunchKernelGGL(mol_io::bce_rows<Term>, g_scores ? grid : dim3(1), block, 0, st, n, T, scores, ld, labels, ld_y, L.per, L.groups,
                       (const double*)lossp, (const int64_t*)cnt, loss, g_scores, ld_g);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" int dgn_masked_bce_forward(int64_t n_rows, int32_t n_tasks, const float* scores, int64_t ld, const float* labels, int64_t ld_y,
                                      float* loss, float* g_scores, int64_t ld_g, void* ws, size_t ws_bytes, void* stream) {
    return masked_mean_forward<mol_io::BceTerm>("dgn_masked_bce_forward", n_rows, n_tasks, scores, ld, labels, ld_y, loss, g_scores, ld_g, ws,
                                                ws_bytes, stream);
}

static int masked_mean_backward(const char* who, int64_t n_rows, int32_t n_tasks, const float* g_saved, int64_t ld_g, const float* g_loss,
                                float* g_scores, int64_t ld_out, void* stream) {
    const int T = n_tasks;
    if (T < 1) { set_error("%s: n_tasks >= 1 required (got %d)", who, T); return DGN_ERR_INVALID; }
    return net_io::loss_backward(who, "n_tasks", n_rows, T, g_saved, ld_g, g_loss, g_scores, ld_out, stream);
}

extern "C" int dgn_masked_bce_backward(int64_t n_rows, int32_t n_tasks, const float* g_saved, int64_t ld_g, const float* g_loss, float* g_scores,
                                       int64_t ld_out, void* stream) {
    return masked_mean_backward("dgn_masked_bce_backward", n_rows, n_tasks, g_saved, ld_g, g_loss, g_scores, ld_out, stream);
}

// ---- masked L1 (the graph-regression net's loss): the same two kernels on the L1 term ------------------------------------------------

extern "C" size_t dgn_masked_mae_workspace_bytes(int64_t n_rows, int32_t n_tasks) { return dgn_masked_bce_workspace_bytes(n_rows, n_tasks); }

extern "C" int dgn_masked_mae_forward(int64_t n_rows, int32_t n_tasks, const float* scores, int64_t ld, const float* targets, int64_t ld_y,
                                     float* loss, float* g_scores, int64_t ld_g, void* ws, size_t ws_bytes, void* stream) {
    return masked_mean_forward<mol_io::L1Term>("dgn_masked_mae_forward", n_rows, n_tasks, scores, ld, targets, ld_y, loss, g_scores, ld_g, ws,
                                               ws_bytes, stream);
}

extern "C" int dgn_masked_mae_backward(int64_t n_rows, int32_t n_tasks, const float* g_saved, int64_t ld_g, const float* g_loss, float* g_scores,
                                      int64_t ld_out, void* stream) {
    return masked_mean_backward("dgn_masked_mae_backward", n_rows, n_tasks, g_saved, ld_g, g_loss, g_scores, ld_out, stream);
}
