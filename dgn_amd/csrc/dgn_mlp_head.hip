// The nets' MLPReadout head (nets/mlp_readout_layer.py:24-30): L hidden Linear + ReLU layers and an output Linear, 1 to 4 Linears of any
// widths 1 .. 128 with at most 20 480 weight floats -- one launch forward, two backward, nothing kept for the backward but x, nothing read
// back, no floating-point atomics (fixed-order sums: the same input gives the same bits), every launch parameter a function of n_rows and
// the widths alone.
//
//   mlp_head_forward   a workgroup stages all weights (transposed, output columns padded to fours) and biases in LDS once, then walks its
//                      contiguous range of 32-row tiles: x tile -> LDS (transposed: feature k of row r at [k][r]), every Linear from LDS
//                      to LDS, the last one's tile -> y.  Thread (slot, r) of the 8 x 32 workgroup owns row r and the output columns
//                      4 (slot + 8 i) .. + 3: per k one activation word (consecutive lanes, consecutive words), one 16-byte weight piece
//                      (one address per half-wave: a broadcast), four fmaf.  Global traffic: one read of x, one write of y.
//   mlp_head_backward  per tile: the hidden activations again, by the forward's own function on the forward's own LDS image (the ReLU
//                      masks are bit for bit the forward's); g_y tile -> LDS; then per Linear, last to first: the weight / bias gradient of
//                      the tile (thread per weight, the 32 rows in row order, a row of ones under every activation tile makes the bias
//                      one more weight column) added by its owning thread to the workgroup's own workspace slot with plain loads and
//                      stores, and the input gradient written over the activation tile it masks (passes where the activation is > 0:
//                      an activation of exactly 0 passes nothing, torch's rule).  g_x leaves from the x tile's place.
//   mlp_head_finalize  thread per weight / bias element: the workgroups' slots added in slot order (fp64) -> g_W_l, g_b_l.
//
// Summation order.  A dot product starts at the bias and takes its terms in increasing k with explicit fmaf (the build has
// -ffp-contract=off: nothing else is contracted); a tile's weight gradient takes its rows in increasing row order on top of the slot's
// value; a workgroup takes its tiles in order; the finalize takes the slots in order.  The split into workgroups depends on n_rows alone.
//
// LDS budget (floats): a header of 32 + sum_l d_{l-1} pad4(d_l) weights + sum_l pad4(d_l) biases + (sum_{l=0..L} d_l + L + 1) rows of 32 + 4
// (the pad keeps the 16-byte reads of the weight-gradient pass, 16 lanes on 16 rows, off one another's banks).  Every shape of the domain fits
// the CU's 160 KB (largest found: 149.4 KB at 128 -> 62 -> 128 -> 18 -> 128); dgn_mlp_head_supported checks it all the same.  Both
// kernels use this one image, so the backward's recomputation reads what the forward read.  x, y, g_y, g_x move as single words, consecutive
// lanes on consecutive addresses of a row: any 4-byte-aligned base and any row stride, no alignment to prove.
#include <hip/hip_runtime.h>

#include "dgn_common.hpp"

namespace dgn {
namespace mlp_head {

constexpr int kThreads = 256;
constexpr int kTile = 32;                    // rows of a tile = lanes of a half-wave
constexpr int kStride = kTile + 4;           // floats between two features of a tile
constexpr int kSlots = kThreads / kTile;     // column groups in flight
constexpr int kMaxLin = 4;
constexpr int kMaxWidth = 128;
constexpr int kMaxWeights = 20480;
constexpr int kMaxGroups = 256;
constexpr int kLdsBytes = 160 * 1024;
constexpr int kHeader = 32;                  // floats at the front of the LDS image: the widths [0, 5) and the Layout [8, 32)

struct Params {                              // by value in the kernel arguments: the parameters stay the nn.Linear tensors of the state_dict
    const float* w[kMaxLin];
    const float* b[kMaxLin];
    int d[kMaxLin + 1];
    int n_lin;
};
struct Grads {
    float* w[kMaxLin];
    float* b[kMaxLin];
};

// Where everything lives: LDS offsets in floats (all multiples of 4), `item` = first element of Linear l in a workspace slot, whose
// layout is [d_l][d_{l-1} + 1] per Linear: the weight gradient's rows, each followed by its bias gradient.
struct Layout {
    int pad[kMaxLin];                        // pad4(d_l): row length of the transposed weight
    int wt[kMaxLin], bias[kMaxLin];
    int act[kMaxLin + 1];
    int item[kMaxLin + 1];
    int floats;
};
static_assert(sizeof(Layout) <= (kHeader - 8) * sizeof(int), "the Layout lives in the header of the LDS image");

__host__ __device__ inline void make_layout(const int* d, int n_lin, Layout& L) {
    int at = kHeader;
    for (int l = 0; l < n_lin; ++l) {
        L.pad[l] = (d[l + 1] + 3) & ~3;
        L.wt[l] = at;
        at += d[l] * L.pad[l];
    }
    for (int l = 0; l < n_lin; ++l) { L.bias[l] = at; at += L.pad[l]; }
    for (int l = 0; l <= n_lin; ++l) { L.act[l] = at; at += (d[l] + 1) * kStride; }
    L.floats = at;
    L.item[0] = 0;
    for (int l = 0; l < n_lin; ++l) L.item[l + 1] = L.item[l] + d[l + 1] * (d[l] + 1);
}

inline bool dims_ok(int32_t n_lin, const int32_t* dims) {
    if (n_lin < 1 || n_lin > kMaxLin || !dims) return false;
    int64_t weights = 0;
    for (int l = 0; l <= n_lin; ++l) {
        if (dims[l] < 1 || dims[l] > kMaxWidth) return false;
        if (l) weights += (int64_t)dims[l - 1] * dims[l];
    }
    if (weights > kMaxWeights) return false;
    Layout L;
    make_layout(dims, n_lin, L);
    return (size_t)L.floats * sizeof(float) <= (size_t)kLdsBytes;
}

struct Split {
    int groups;                              // workgroups = workspace slots written
    int64_t tiles, per;                      // tiles in all, tiles per workgroup
    int64_t bound;                           // upper bound of `groups`: the slots of the backward's workspace
};
inline Split split(int64_t n_rows) {
    const int64_t tiles = (n_rows + kTile - 1) / kTile;
    const SlotSplit s = slot_split(tiles, 1, kMaxGroups);
    return {s.groups, tiles, s.per, s.bound};
}

// the widths and the layout into LDS (no run-time index into the kernel arguments), then the parameters: W_l [d_l][d_{l-1}] as
// [d_{l-1}][pad4(d_l)], zeros in the padding; ends with a barrier
__device__ __forceinline__ void stage(const Params& p, float* lds) {
    const int tid = threadIdx.x;
    int* s_d = reinterpret_cast<int*>(lds);
    Layout& s_lay = *reinterpret_cast<Layout*>(lds + 8);
    if (tid == 0) {
#pragma unroll
        for (int l = 0; l <= kMaxLin; ++l) s_d[l] = p.d[l];
        make_layout(s_d, p.n_lin, s_lay);
    }
    __syncthreads();
#pragma unroll
    for (int l = 0; l < kMaxLin; ++l) {
        if (l >= p.n_lin) break;
        const int din = p.d[l], dout = p.d[l + 1], pad = s_lay.pad[l];
        const float* __restrict__ w = p.w[l];
        const float* __restrict__ b = p.b[l];
        float* wt = lds + s_lay.wt[l];
        for (int e = tid; e < din * pad; e += kThreads) {
            const int k = e / pad, j = e - k * pad;
            wt[e] = j < dout ? w[j * din + k] : 0.f;
        }
        if (tid < pad) lds[s_lay.bias[l] + tid] = tid < dout ? b[tid] : 0.f;
        // the row of ones under the activation tile of this Linear's input: its "weight gradient" column is the bias gradient
        if (tid < kStride) lds[s_lay.act[l] + din * kStride + tid] = 1.f;
    }
    __syncthreads();
}

// rows [row0, row0 + 32) of a [n_rows, width] matrix -> tile[c][r]; rows past the end: zeros
__device__ __forceinline__ void load_tile(float* tile, const float* __restrict__ src, int64_t ld, int width, int64_t row0, int64_t n_rows) {
    for (int e = threadIdx.x; e < kTile * width; e += kThreads) {
        const int r = e / width, c = e - r * width;
        tile[c * kStride + r] = row0 + r < n_rows ? src[(row0 + r) * ld + c] : 0.f;
    }
}
__device__ __forceinline__ void store_tile(float* __restrict__ dst, int64_t ld, const float* tile, int width, int64_t row0, int64_t n_rows) {
    for (int e = threadIdx.x; e < kTile * width; e += kThreads) {
        const int r = e / width, c = e - r * width;
        if (row0 + r < n_rows) dst[(row0 + r) * ld + c] = tile[c * kStride + r];
    }
}

// out[j][r] = act(bias[j] + sum_k in[k][r] W[j][k]), k increasing; the one function of the forward and of the backward's recomputation
__device__ __forceinline__ void linear_tile(const float* wt, const float* bias, int din, int dout, int pad, const float* in, float* out, bool relu) {
    const int r = threadIdx.x & (kTile - 1), slot = threadIdx.x / kTile;
    for (int j0 = 4 * slot; j0 < dout; j0 += 4 * kSlots) {
        float acc[4];
        ldv<4>(acc, bias + j0);
        const float* a = in + r;
        const float* w = wt + j0;
#pragma unroll 4
        for (int k = 0; k < din; ++k) {
            float wk[4];
            ldv<4>(wk, w + k * pad);
            const float ak = a[k * kStride];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(ak, wk[c], acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float v = relu && acc[c] < 0.f ? 0.f : acc[c];            // (a NaN stays a NaN, as torch's relu)
            if (j0 + c < dout) out[(j0 + c) * kStride + r] = v;
        }
    }
}

// in[k][r] := (mask ? in[k][r] > 0 : true) ? sum_j W[j][k] g[j][r] : 0, j increasing: the input gradient over the activation it masks
__device__ __forceinline__ void input_grad_tile(const float* wt, int din, int dout, int pad, const float* g, float* in, bool mask) {
    const int r = threadIdx.x & (kTile - 1), slot = threadIdx.x / kTile;
    for (int k0 = 4 * slot; k0 < din; k0 += 4 * kSlots) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        const float* w[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] = wt + (k0 + c < din ? k0 + c : din - 1) * pad;
#pragma unroll 4
        for (int j = 0; j < dout; ++j) {
            const float gj = g[j * kStride + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[c] = fmaf(w[c][j], gj, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (k0 + c >= din) break;
            float* cell = in + (k0 + c) * kStride + r;
            *cell = !mask || *cell > 0.f ? acc[c] : 0.f;
        }
    }
}

// slot[j][k] (+)= sum_r g[j][r] in[k][r] for k = 0 .. din, r increasing (in[din][.] = 1: the bias gradient); thread per element
__device__ __forceinline__ void weight_grad_tile(int din, int dout, const float* g, const float* in, float* __restrict__ slot, bool first) {
    const int items = dout * (din + 1);
    for (int it = threadIdx.x; it < items; it += kThreads) {
        const int j = it / (din + 1), k = it - j * (din + 1);
        float acc = first ? 0.f : slot[it];
        const float* gp = g + j * kStride;
        const float* ap = in + k * kStride;
#pragma unroll
        for (int r = 0; r < kTile; r += 4) {
            float gv[4], av[4];
            ldv<4>(gv, gp + r);
            ldv<4>(av, ap + r);
#pragma unroll
            for (int c = 0; c < 4; ++c) acc = fmaf(gv[c], av[c], acc);
        }
        slot[it] = acc;
    }
}

__global__ __launch_bounds__(kThreads) void mlp_head_forward(int64_t n_rows, Params p, const float* __restrict__ x, int64_t ld_x,
                                                             float* __restrict__ y, int64_t ld_y, int64_t per, int64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    stage(p, lds);
    const int* s_d = reinterpret_cast<const int*>(lds);          // (everything in the dynamic region: its base stays 16-byte aligned)
    const Layout& s_lay = *reinterpret_cast<const Layout*>(lds + 8);
    const int n_lin = p.n_lin;
    const int64_t t0 = (int64_t)blockIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t row0 = t * kTile;
        load_tile(lds + s_lay.act[0], x, ld_x, s_d[0], row0, n_rows);
        __syncthreads();
        for (int l = 0; l < n_lin; ++l) {
            linear_tile(lds + s_lay.wt[l], lds + s_lay.bias[l], s_d[l], s_d[l + 1], s_lay.pad[l], lds + s_lay.act[l], lds + s_lay.act[l + 1],
                        l + 1 < n_lin);
            __syncthreads();
        }
        store_tile(y, ld_y, lds + s_lay.act[n_lin], s_d[n_lin], row0, n_rows);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void mlp_head_backward(int64_t n_rows, Params p, const float* __restrict__ x, int64_t ld_x,
                                                              const float* __restrict__ g_y, int64_t ld_gy, float* __restrict__ g_x,
                                                              int64_t ld_gx, float* __restrict__ ws, int64_t per, int64_t tiles) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    stage(p, lds);
    const int* s_d = reinterpret_cast<const int*>(lds);          // (everything in the dynamic region: its base stays 16-byte aligned)
    const Layout& s_lay = *reinterpret_cast<const Layout*>(lds + 8);
    const int n_lin = p.n_lin;
    float* slot = ws + (int64_t)blockIdx.x * s_lay.item[n_lin];
    const int64_t t0 = (int64_t)blockIdx.x * per, t1 = t0 + per < tiles ? t0 + per : tiles;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t row0 = t * kTile;
        load_tile(lds + s_lay.act[0], x, ld_x, s_d[0], row0, n_rows);
        load_tile(lds + s_lay.act[n_lin], g_y, ld_gy, s_d[n_lin], row0, n_rows);       // (rows past the end: zero gradient, they add nothing)
        __syncthreads();
        for (int l = 0; l + 1 < n_lin; ++l) {
            linear_tile(lds + s_lay.wt[l], lds + s_lay.bias[l], s_d[l], s_d[l + 1], s_lay.pad[l], lds + s_lay.act[l], lds + s_lay.act[l + 1], true);
            __syncthreads();
        }
        for (int l = n_lin - 1; l >= 0; --l) {
            weight_grad_tile(s_d[l], s_d[l + 1], lds + s_lay.act[l + 1], lds + s_lay.act[l], slot + s_lay.item[l], t == t0);
            if (l == 0 && !g_x) break;
            __syncthreads();
            input_grad_tile(lds + s_lay.wt[l], s_d[l], s_d[l + 1], s_lay.pad[l], lds + s_lay.act[l + 1], lds + s_lay.act[l], l > 0);
            __syncthreads();
        }
        if (g_x) store_tile(g_x, ld_gx, lds + s_lay.act[0], s_d[0], row0, n_rows);
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void mlp_head_finalize(Params p, Grads g, int groups, const float* __restrict__ ws) {
    int item[kMaxLin + 1];
    item[0] = 0;
#pragma unroll
    for (int l = 0; l < kMaxLin; ++l) item[l + 1] = item[l] + (l < p.n_lin ? p.d[l + 1] * (p.d[l] + 1) : 0);
    const int total = item[kMaxLin];
    const int it = blockIdx.x * kThreads + threadIdx.x;
    if (it >= total) return;
    double acc = 0.0;
#pragma unroll 4
    for (int s = 0; s < groups; ++s) acc += (double)ws[(int64_t)s * total + it];
#pragma unroll
    for (int l = 0; l < kMaxLin; ++l) {
        if (it >= item[l] && it < item[l + 1]) {
            const int din = p.d[l], e = it - item[l];
            const int j = e / (din + 1), k = e - j * (din + 1);
            if (k < din) g.w[l][j * din + k] = (float)acc;
            else g.b[l][j] = (float)acc;
        }
    }
}

// the checks the two entry points share; fills p
inline int check_args(const char* who, int64_t n_rows, int32_t n_lin, const int32_t* dims, const float* const* w, const float* const* b, Params& p) {
    if (!dims_ok(n_lin, dims)) {
        set_error("%s: 1 to %d Linears of widths 1 .. %d with at most %d weight floats required (dgn_mlp_head_supported)", who, kMaxLin, kMaxWidth,
                  kMaxWeights);
        return DGN_ERR_INVALID;
    }
    if (n_rows < 0 || n_rows > INT32_MAX) { set_error("%s: n_rows beyond the int32 range", who); return DGN_ERR_INVALID; }
    if (!w || !b) { set_error("%s: null parameter table", who); return DGN_ERR_INVALID; }
    p = Params{};
    p.n_lin = n_lin;
    for (int l = 0; l <= n_lin; ++l) p.d[l] = dims[l];
    for (int l = 0; l < n_lin; ++l) {
        if (!w[l] || !b[l]) { set_error("%s: null weight / bias %d", who, l); return DGN_ERR_INVALID; }
        p.w[l] = w[l];
        p.b[l] = b[l];
    }
    return DGN_OK;
}

inline size_t lds_bytes(const Params& p) {
    Layout L;
    make_layout(p.d, p.n_lin, L);
    return (size_t)L.floats * sizeof(float);
}
inline int64_t slot_floats(int32_t n_lin, const int32_t* dims) {
    Layout L;
    make_layout(dims, n_lin, L);
    return L.item[n_lin];
}

}  // namespace mlp_head
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_mlp_head_supported(int32_t n_linears, const int32_t* dims) { return mlp_head::dims_ok(n_linears, dims) ? 1 : 0; }

extern "C" int dgn_mlp_head_forward(int64_t n_rows, int32_t n_linears, const int32_t* dims, const float* x, int64_t ld_x, const float* const* w,
                                    const float* const* b, float* y, int64_t ld_y, void* stream) {
    mlp_head::Params p;
    if (int rc = mlp_head::check_args("dgn_mlp_head_forward", n_rows, n_linears, dims, w, b, p)) return rc;
    if (n_rows == 0) return DGN_OK;
    if (!x || !y) { set_error("dgn_mlp_head_forward: null x / y"); return DGN_ERR_INVALID; }
    if (ld_x < dims[0] || ld_y < dims[n_linears]) { set_error("dgn_mlp_head_forward: row stride below the row's width"); return DGN_ERR_INVALID; }
    static LdsOptIn lds_ok{0};
    DGN_HIP_CHECK(allow_lds(lds_ok, mlp_head::kLdsBytes, &mlp_head::mlp_head_forward));
    const mlp_head::Split s = mlp_head::split(n_rows);
    hipLaunchKernelGGL(mlp_head::mlp_head_forward, dim3((unsigned)s.groups), dim3(mlp_head::kThreads), mlp_head::lds_bytes(p),
                       static_cast<hipStream_t>(stream), n_rows, p, x, ld_x, y, ld_y, s.per, s.tiles);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}

extern "C" size_t dgn_mlp_head_backward_workspace_bytes(int64_t n_rows, int32_t n_linears, const int32_t* dims) {
    if (n_rows < 0 || n_rows > INT32_MAX || !mlp_head::dims_ok(n_linears, dims)) return 0;
    return (size_t)mlp_head::split(n_rows).bound * (size_t)mlp_head::slot_floats(n_linears, dims) * sizeof(float);
}

extern "C" int dgn_mlp_head_backward(int64_t n_rows, int32_t n_linears, const int32_t* dims, const float* x, int64_t ld_x, const float* const* w,
                                     const float* const* b, const float* g_y, int64_t ld_gy, float* g_x, int64_t ld_gx, float* const* g_w,
                                     float* const* g_b, void* ws, size_t ws_bytes, void* stream) {
    mlp_head::Params p;
    if (int rc = mlp_head::check_args("dgn_mlp_head_backward", n_rows, n_linears, dims, w, b, p)) return rc;
    if (!g_w || !g_b) { set_error("dgn_mlp_head_backward: null gradient table"); return DGN_ERR_INVALID; }
    mlp_head::Grads g{};
    for (int l = 0; l < n_linears; ++l) {
        if (!g_w[l] || !g_b[l]) { set_error("dgn_mlp_head_backward: null weight / bias gradient %d", l); return DGN_ERR_INVALID; }
        g.w[l] = g_w[l];
        g.b[l] = g_b[l];
    }
    const int64_t total = mlp_head::slot_floats(n_linears, dims);
    const dim3 fin_grid((unsigned)((total + mlp_head::kThreads - 1) / mlp_head::kThreads)), block(mlp_head::kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_rows == 0) {                          // no row, no slot: the finalize writes the zero gradients
        hipLaunchKernelGGL(mlp_head::mlp_head_finalize, fin_grid, block, 0, st, p, g, 0, (const float*)nullptr);
        DGN_HIP_CHECK(hipGetLastError());
        return DGN_OK;
    }
    if (!x || !g_y) { set_error("dgn_mlp_head_backward: null x / g_y"); return DGN_ERR_INVALID; }
    if (ld_x < dims[0] || ld_gy < dims[n_linears] || (g_x && ld_gx < dims[0])) {
        set_error("dgn_mlp_head_backward: row stride below the row's width");
        return DGN_ERR_INVALID;
    }
    const size_t need = dgn_mlp_head_backward_workspace_bytes(n_rows, n_linears, dims);
    if (!ws || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 3)) {
        set_error("dgn_mlp_head_backward: workspace of %zu bytes (4-byte aligned) required, got %zu", need, ws_bytes);
        return DGN_ERR_INVALID;
    }
    static LdsOptIn lds_ok{0};
    DGN_HIP_CHECK(allow_lds(lds_ok, mlp_head::kLdsBytes, &mlp_head::mlp_head_backward));
    const mlp_head::Split s = mlp_head::split(n_rows);
    hipLaunchKernelGGL(mlp_head::mlp_head_backward, dim3((unsigned)s.groups), block, mlp_head::lds_bytes(p), st, n_rows, p, x, ld_x, g_y, ld_gy, g_x,
                       ld_gx, static_cast<float*>(ws), s.per, s.tiles);
    hipLaunchKernelGGL(mlp_head::mlp_head_finalize, fin_grid, block, 0, st, p, g, s.groups, (const float*)ws);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}
