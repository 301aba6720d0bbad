// Eigenvector augmentations of the reference's training loops (include/dgn_hip.h: dgn_eig_augment) as ONE kernel whose random stream
// lives on the device: the random sign per entry of the molecule loop (train/train_molecules_graph_regression.py:29-33) and the
// per-node rotation of the (eig1, eig2) pair followed by the random sign on column 2 of the superpixel loop
// (train/train_superpixels_graph_classification.py:29-42).
//
//   rows         one thread per row: it reads its K <= 32 columns into registers, then writes them, so out may be eig.
//   stream       row i of call number c = state[1] draws Philox4x32-10(counter (i, c), key state[0]): r[0] is the angle's uniform,
//                the bits of r[1] are the signs of the columns.  Nothing depends on the grid.
//   the counter  the kernel advances it itself: thread 0 of every workgroup reads (key, c) first and takes a ticket from state[2] last;
//                the workgroup that draws the last ticket writes c + 1 and clears the tickets.  Every workgroup has read c before it
//                takes its ticket, so none sees the new value; a launch and a graph replay both move the stream by exactly one.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "dgn_common.hpp"
#include "dgn_philox.hpp"

namespace dgn {
namespace eig_augment {

constexpr int kThreads = 256;
constexpr int kMaxCols = 32;

__global__ __launch_bounds__(kThreads) void augment_rows(int64_t n_rows, int K, const float* eig /* may be out */, int64_t ld_in, float* out,
                                                         int64_t ld_out, float rotate_deg, uint32_t flip_mask, int64_t* state) {
    __shared__ uint64_t s_state[2];
    if (threadIdx.x == 0) {
        s_state[0] = (uint64_t)__hip_atomic_load(&state[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_state[1] = (uint64_t)__hip_atomic_load(&state[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    const uint64_t key = s_state[0], call = s_state[1];
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i < n_rows) {
        uint32_t r[4] = {(uint32_t)i, (uint32_t)((uint64_t)i >> 32), (uint32_t)call, (uint32_t)(call >> 32)};
        philox4x32_10(r, (uint32_t)key, (uint32_t)(key >> 32));
        const float* src = eig + i * ld_in;
        float v[kMaxCols];
#pragma unroll
        for (int j = 0; j < kMaxCols; ++j) v[j] = j < K ? src[j] : 0.f;
        if (rotate_deg != 0.f) {                                                  // (K >= 3: checked by the host)
            const float u = (float)(r[0] >> 8) * 0x1p-24f;
            const float angle = (u - 0.5f) * 2.f * rotate_deg;
            const float s = sinf(angle * 3.14159265358979323846f / 180.f);
            const float c = sqrtf(1.f - s * s);                                   // the reference's form: |cos|, not cos, beyond +-90 degrees
            const float x1 = v[1], x2 = v[2];
            v[1] = c * x1 + s * x2;
            v[2] = c * x2 - s * x1;
        }
        float* dst = out + i * ld_out;
#pragma unroll
        for (int j = 0; j < kMaxCols; ++j) {
            if (j < K) {
                if ((flip_mask >> j) & 1u) v[j] *= ((r[1] >> j) & 1u) ? 1.f : -1.f;   // a product, as torch.mul: 0 -> -0
                dst[j] = v[j];
            }
        }
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long* tickets = reinterpret_cast<unsigned long long*>(&state[2]);
        if (atomicAdd(tickets, 1ull) == (unsigned long long)gridDim.x - 1ull) {
            __hip_atomic_store(&state[1], (int64_t)(call + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&state[2], (int64_t)0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace eig_augment
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_eig_augment(int64_t n_rows, int32_t K, const float* eig, int64_t ld_in, float* out, int64_t ld_out, float rotate_deg,
                               int32_t flip_mask, int64_t* state, void* stream) {
    using namespace eig_augment;
    const char* fn = "dgn_eig_augment";
    if (n_rows < 0) { set_error("%s: n_rows >= 0 required", fn); return DGN_ERR_INVALID; }
    if (K < 1 || K > kMaxCols) { set_error("%s: 1 <= K <= %d required (K = %d)", fn, kMaxCols, K); return DGN_ERR_INVALID; }
    if (!std::isfinite(rotate_deg)) { set_error("%s: rotate_deg must be finite", fn); return DGN_ERR_INVALID; }
    if (rotate_deg != 0.f && K < 3) { set_error("%s: the rotation turns columns 1 and 2: K >= 3 required (K = %d)", fn, K); return DGN_ERR_INVALID; }
    if (ld_in < K || ld_out < K) { set_error("%s: row strides below K = %d", fn, K); return DGN_ERR_INVALID; }
    if (n_rows == 0) return DGN_OK;
    if (!eig || !out || !state) { set_error("%s: null buffer", fn); return DGN_ERR_INVALID; }
    if (eig == out && ld_in != ld_out) { set_error("%s: in place needs equal row strides", fn); return DGN_ERR_INVALID; }
    const int64_t blocks = (n_rows + kThreads - 1) / kThreads;
    if (blocks >= (int64_t)INT32_MAX) { set_error("%s: %lld rows exceed the grid", fn, (long long)n_rows); return DGN_ERR_INVALID; }
    hipLaunchKernelGGL(augment_rows, dim3((unsigned)blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), n_rows, (int)K, eig, ld_in, out,
                       ld_out, rotate_deg, (uint32_t)flip_mask, state);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}
