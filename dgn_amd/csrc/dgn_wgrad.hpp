// The weight-gradient scheme of the MFMA product families (lin::ts_wgrad, lin::bd_wgrad / bd_backward_both, gemm::ts_gemm_wgrad /
// tile_wgrad, dc::dc_wgrad), one definition per piece: workgroups stream 16-row strips of G and X through LDS (strip_fetch /
// strip_commit), every workgroup leaves ONE partial block in its slot of a workspace (wave_fold where the waves of a workgroup each
// hold a partial of the same block), and a finalize kernel adds the slots in a fixed order (slot_sum16).  The order of summation in
// these pieces is the library's reproducibility contract: the same input gives the same bits.
#pragma once
#include "dgn_common.hpp"
#include "dgn_load4.hpp"

namespace dgn {
namespace wg {

using gemm::f4;
using gemm::Raw4;
using gemm::load4_raw;
using gemm::load4_window;

// ---- the slot sum of the finalize kernels ------------------------------------------------------------------------------------------
// A finalize block has kSumWaves waves and covers 64 consecutive output elements, one per lane.
constexpr int kSumWaves = 16;

// the waves' sums of one element joined in wave order (red[w][lane] written by wave w, a barrier since)
__device__ __forceinline__ float wave_join16(const float (&red)[kSumWaves][64], int lane) {
    float v = 0.f;
#pragma unroll
    for (int w = 0; w < kSumWaves; ++w) v += red[w][lane];
    return v;
}
// Sum over `slots` partial blocks of the element at src (slot 0) + q * stride: wave sg adds the slots sg, sg + 16, ... alternately into
// two running sums (all loads of a lane in flight together), red joins the sixteen waves in wave order.  live = false: nothing is
// read, the sum is zero.  Every thread of the block calls it; the result is on wave 0's lanes.
__device__ __forceinline__ float slot_sum16(const float* src, int64_t stride, int slots, bool live, float (&red)[kSumWaves][64]) {
    const int lane = threadIdx.x & 63, sg = threadIdx.x >> 6;
    float s0 = 0.f, s1 = 0.f;
    if (live) {
        int q = sg;
        for (; q + kSumWaves < slots; q += 2 * kSumWaves) {
            s0 += src[(int64_t)q * stride];
            s1 += src[(int64_t)(q + kSumWaves) * stride];
        }
        if (q < slots) s0 += src[(int64_t)q * stride];
    }
    red[sg][lane] = s0 + s1;
    __syncthreads();
    return sg == 0 ? wave_join16(red, lane) : 0.f;
}

// ---- the wave-order fold of a workgroup's accumulators -----------------------------------------------------------------------------
// Every wave holds N accumulator tiles of the same partial block: the waves add them up in LDS in wave order (wave 0 writes, wave w
// adds to what waves 0 .. w - 1 left), then the block of BLOCK floats goes to slot `slot` of part.  at(q, r): where entry r of this
// lane's tile q lives in the block.  red may reuse the strips: the fold begins with a barrier.
template <int BLOCK, int N, class At>
__device__ __forceinline__ void wave_fold(float* red, float* part, int64_t slot, const f4 (&acc)[N], At at) {
    const int tid = threadIdx.x, wave = tid >> 6, n_waves = blockDim.x >> 6;
    __syncthreads();
    for (int w = 0; w < n_waves; ++w) {
        if (wave == w) {
#pragma unroll
            for (int q = 0; q < N; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float* d = red + at(q, r);
                    *d = w == 0 ? acc[q][r] : *d + acc[q][r];
                }
        }
        __syncthreads();
    }
    float* out = part + slot * BLOCK;
    for (int i = tid; i < BLOCK / 4; i += blockDim.x) reinterpret_cast<f4*>(out)[i] = reinterpret_cast<const f4*>(red)[i];
}

// ---- strip staging -----------------------------------------------------------------------------------------------------------------
// A 16-row strip of G's and X's columns as 16-byte pieces, gq + xq pieces per row (G's first), dealt to the workgroup's THREADS
// threads ITEMS at a time: fetched into registers before the current strip's MFMAs, committed to the other LDS buffer after them
// (dgn_load4.hpp on why the two are apart).  Zero beyond the matrices.
// The strips' dynamic LDS: two (G strip, X strip) buffers of `rows` rows at the row strides gs, xs (floats); gemm::wgrad_bufs / tw_bufs, dc::wgrad_bufs
struct StripBufs {
    int rows, gs, xs;
    constexpr int half() const { return rows * (gs + xs); }      // floats of one buffer
    constexpr size_t bytes() const { return (size_t)2 * half() * sizeof(float); }
};
struct Strip {
    const float* G; int64_t ldg; int n, g0;      // G [rows, n], the strip's first column
    const float* X; int64_t ldx; int k, x0;
    int gq, per_row, total;                      // pieces of G per row, of G and X per row, of the whole strip
    bool ones;                                   // column k of X := 1 on the rows that exist (the bias gradient rides along)
};
// The row sources: virtual row i of the strips -> the row to read (always inside the matrix) and whether it exists
struct ClampRows {                               // the matrix's own rows; the strip past the last one is short
    int64_t M;
    __device__ __forceinline__ int64_t operator()(int64_t i, bool& live) const { live = i < M; return min(i, M - 1); }
};
struct PermRows {                                // rows gathered through a permutation, entries < 0 are holes
    const int32_t* vperm;
    __device__ __forceinline__ int64_t operator()(int64_t i, bool& live) const { const int nd = vperm[i]; live = nd >= 0; return max(nd, 0); }
};
// A row that does not exist is load4_raw's live = false (zeros).  With a ones column it is marked sh = 8 besides: sh = 4 .. 7 also
// occurs on rows that DO exist -- the window that starts at column k of X when k % 4 == 0, whose one live entry is the ones column.
constexpr int kDeadRow = 8;
template <int THREADS, bool ONES, int ITEMS, class Rows>
__device__ __forceinline__ void strip_fetch(Raw4 (&reg)[ITEMS], const Strip& s, const Rows& rows, int64_t strip) {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int it = min((int)threadIdx.x + j * THREADS, s.total - 1);      // (surplus threads repeat the last piece; commit skips them)
        const int r = it / s.per_row, c = it - r * s.per_row;
        bool live;
        const int64_t row = rows(strip * 16 + r, live);
        const bool is_g = c < s.gq;
        // (absolute columns against the whole row's width: always >= 4 columns to clamp into)
        reg[j] = load4_raw(is_g ? s.G + row * s.ldg : s.X + row * s.ldx, is_g ? s.g0 + 4 * c : s.x0 + 4 * (c - s.gq), is_g ? s.n : s.k, live);
        if (ONES && !live) reg[j].sh = kDeadRow;
    }
}
template <int THREADS, bool ONES, int ITEMS>
__device__ __forceinline__ void strip_commit(const Raw4 (&reg)[ITEMS], const Strip& s, float* Gb, int gs, float* Xb, int xs) {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
        const int it = (int)threadIdx.x + j * THREADS;
        if (it < s.total) {
            const int r = it / s.per_row, c = it - r * s.per_row;
            f4 v = load4_window(reg[j]);
            if (c < s.gq) *reinterpret_cast<f4*>(Gb + r * gs + 4 * c) = v;
            else {
                if (ONES && s.ones && reg[j].sh < kDeadRow) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = s.x0 + 4 * (c - s.gq) + e == s.k ? 1.f : v[e];
                }
                *reinterpret_cast<f4*>(Xb + r * xs + 4 * (c - s.gq)) = v;
            }
        }
    }
}

}  // namespace wg
}  // namespace dgn
