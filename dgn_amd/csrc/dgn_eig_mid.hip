// Laplacian eigenpairs of the graphs of 65 to 192 nodes of a batch: one workgroup per graph, the whole solve in LDS in fp64, one launch per
// width class.  The continuation of dgn_eig_small.hip (graphs of at most 64 nodes) with the same build, stop rule, epilogue and status codes.
//
// Two full fp64 squares (A and V) of 192 nodes are 2 x 295 KB against 160 KiB of LDS, so:
//   storage   A alone, packed symmetric: the lower triangle, cell (i, j), i >= j, at i (i + 1) / 2 + j.  192 nodes: 18 528 doubles.  An odd n is
//             padded with one zero row (m = n + 1 <= W), which the idle slot's identity rotation leaves zero.
//   build     as the small kernel: in-degree d_i = max(indptr[i + 1] - indptr[i], 1); every edge j -> i adds -w to cell {i, j}, w = 1/2 ('none')
//             or 1 / (2 sqrt(d_i d_j)); multi-edges add up.  Packed storage has ONE cell where the square has L[i][j] and L[j][i], so a
//             self-loop adds -2w to its diagonal cell (the square gets -w twice there; the oracle's (A + A^T) / 2 says the same).  One wave
//             per row, lanes over its edges, LDS fp64 atomics: all terms of a cell are equal (or multiples of 1/2), so their order does not
//             show.  A source outside the graph's node range never becomes an LDS index: status -2, nothing else written.
//   solve     two-sided cyclic Jacobi, the small kernel's round-robin schedule and Rutishauser rotation.  Per step: every pair's rotation
//             (t, c, s, the new a_pp / a_qq) from the matrix as it stands, t appended to the log | barrier | ONE tile pass | barrier.  With
//             one cell per {i, j} the column and the row pass merge: for pairs P = (p1, q1), Q = (p2, q2) of the step the 2 x 2 block
//             [a(p1,p2) a(p1,q2); a(q1,p2) a(q1,q2)] becomes J_P^T B J_Q, every cell read and written at (max, min); the tile P == Q writes
//             a_pp - t a_pq, a_qq + t a_pq and a_pq = 0 as such.  npairs (npairs + 1) / 2 tiles per step (4 656 at n = 192), all disjoint.
//             A skipped pair (a_pq == 0, the idle slot) has c = 1, s = 0: its tiles are exact identities and it logs t = 0.
//   log       no V.  t of (sweep, step r, pair slot) goes to the graph's log slot in global memory at ((sweep (W - 1) + r) (W / 2) + slot):
//             the schedule fixes p and q, c = 1 / sqrt(t^2 + 1) and s = t c are recomputed by the same expressions.  Coalesced 8-byte writes.
//   replay    after convergence the diagonal is ranked (ties by column index) and V e_c = J_1 J_2 ... J_m e_c of the min(k, n) lowest columns
//             is formed by applying the log BACKWARDS to an [m][kk] fp64 block that reuses A's space (A is dead once lam is saved):
//             x_p' = c x_p + s x_q, x_q' = -s x_p + c x_q.  The pairs of a step are disjoint: one barrier per step; c, s, p, q of 16 steps
//             at a time are staged in LDS behind the block, so no step waits for global memory.
//   stop      the off-diagonal squares summed directly after every sweep; <= 1e-14 ||L||_F or max_sweeps.  status = sweeps done (>= 1).
//   epilogue  fp32 vectors to vec[N, k] ('walk': scaled by d^-1/2, unit length), fp64 values to val[G, k], zeros / NaN beyond n.
//
// Classes by n alone: (64, 128] on 512 threads (71 568 bytes, two workgroups per CU), (128, 192] on 1024 threads (156 304 bytes of 163 840, one per
// CU).  Both are launched over the same grid; a workgroup whose graph belongs to the other class or has n <= 64 returns at once and writes
// nothing.  n > 192: status -1.  Every sum and every log position is fixed by n and the class: a graph's bits do not depend on the batch, on
// its place in it or on its log slot.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>

#include "dgn_common.hpp"

namespace dgn {
namespace eig_mid {

constexpr int kSmallNodes = 64;              // up to here: dgn_eig_small's graphs
constexpr int kMaxNodes = 192;
constexpr int kMaxK = 32;
constexpr int kChunk = 16;                   // steps of the replay staged at a time
constexpr double kTol2 = 1e-28;              // (1e-14)^2: the stop rule compares squares
constexpr size_t kSweepEntries = (size_t)(kMaxNodes - 1) * (kMaxNodes / 2);      // log entries of one sweep of the widest class

struct Args {
    const int32_t* indptr;
    const int32_t* src;
    int64_t n_nodes, n_edges;
    const int64_t* graph_off;
    const int32_t* graph_ids;
    int n_graphs, k, norm, max_sweeps;
    float* vec;
    double* val;
    int32_t* status;
    double* log;
};

template <int W>
struct Lds {
    static constexpr int kPacked = W * (W + 1) / 2;
    static constexpr int kDoubles = kPacked + 4 * (W / 2) + 2 * W + 16 + kMaxK;
    static constexpr int kInts = 2 * (W / 2) + W + 4;
    static constexpr int kBytes = kDoubles * 8 + kInts * 4;
    // the replay's view of A's space: X [W][kMaxK], then cos, sin [kChunk][W / 2] doubles and p, q [kChunk][W / 2] ints
    static constexpr int kReplayDoubles = W * kMaxK + 2 * kChunk * (W / 2) + kChunk * (W / 2);
    static_assert(kReplayDoubles <= kPacked, "the replay block and its staging area live in A's space");
};

__device__ __forceinline__ int pidx(int i, int j) {
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    return hi * (hi + 1) / 2 + lo;
}

// the pair (p < q) of slot t in step r of the round-robin over m players
__device__ __forceinline__ void pair_of(int m, int r, int t, int& p, int& q) {
    int x, y;
    if (t == 0) { x = m - 1; y = r; }
    else { x = (r + t) % (m - 1); y = (r - t + (m - 1)) % (m - 1); }
    p = x < y ? x : y;
    q = x < y ? y : x;
}

template <int W, int THREADS>
__global__ __launch_bounds__(THREADS) void eig_mid_kernel(Args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    using L = Lds<W>;
    constexpr int kWaves = THREADS / kWave;
    constexpr int H = W / 2;
    double* A = reinterpret_cast<double*>(smem);
    double* rc = A + L::kPacked;             // per pair: cos, sin, new a_pp, new a_qq
    double* rs = rc + H;
    double* rpp = rs + H;
    double* rqq = rpp + H;
    double* dsc = rqq + H;                   // d^-1/2 ('sym', 'walk') or d ('none')
    double* lam = dsc + W;
    double* red = lam + W;
    double* cscale = red + 16;
    int* pp = reinterpret_cast<int*>(cscale + kMaxK);
    int* qq = pp + H;
    int* order = qq + H;
    int* flag = order + W;

    const int slot = blockIdx.x;
    const int tid = threadIdx.x;
    int g = slot;
    if (a.graph_ids) g = a.graph_ids[slot];
    if (g < 0 || g >= a.n_graphs) return;                                  // never an index
    const int64_t n0 = a.graph_off[g], n1 = a.graph_off[g + 1];
    const int64_t span = n1 - n0;
    const bool range_ok = n0 >= 0 && n1 >= n0 && n1 <= a.n_nodes;
    if (range_ok && span <= kSmallNodes) return;                           // the small kernel's graph
    // which class owns the graph: (64, 128] the first, the rest (oversize and malformed ranges included) the second
    const bool lower = range_ok && span <= 128;
    if (lower != (W == 128)) return;
    if (!range_ok || span > kMaxNodes) {
        if (tid == 0) a.status[g] = range_ok ? -1 : -2;
        return;
    }
    const int n = (int)span;
    const bool normalised = a.norm != 0;
    const int lane = tid & (kWave - 1), wave = tid / kWave;

    for (int e = tid; e < L::kPacked; e += THREADS) A[e] = 0.0;
    if (tid < W) order[tid] = tid;
    if (tid == 0) *flag = 0;
    if (tid < n) {
        const int d = a.indptr[n0 + tid + 1] - a.indptr[n0 + tid];
        const double dd = d > 1 ? (double)d : 1.0;
        dsc[tid] = normalised ? 1.0 / sqrt(dd) : dd;
    }
    __syncthreads();
    for (int i = wave; i < n; i += kWaves) {                              // a wave per row, its lanes over the row's edges
        int64_t e0 = a.indptr[n0 + i], e1 = a.indptr[n0 + i + 1];
        if (e0 < 0) e0 = 0;
        if (e1 > a.n_edges) e1 = a.n_edges;
        for (int64_t e = e0 + lane; e < e1; e += kWave) {
            const int64_t j = (int64_t)a.src[e] - n0;
            if (j < 0 || j >= n) { *flag = 1; continue; }                 // a foreign source: never an LDS index
            const double w = normalised ? (0.5 * dsc[i]) * dsc[j] : 0.5;
            lds_add_f64(&A[pidx(i, (int)j)], (int)j == i ? -2.0 * w : -w);
        }
    }
    __syncthreads();
    if (*flag) {
        if (tid == 0) a.status[g] = -2;
        return;
    }
    if (tid < n) A[pidx(tid, tid)] += normalised ? 1.0 : dsc[tid];
    __syncthreads();

    // sum of the squares below the diagonal: a wave per row, lanes along it -- an order fixed by n and the class
    auto lower_squares = [&]() {
        double part = 0.0;
        for (int i = wave; i < n; i += kWaves) {
            const int base = i * (i + 1) / 2;
            for (int j = lane; j < i; j += kWave) { const double x = A[base + j]; part += x * x; }
        }
        const double s = block_sum<kWaves>(part, red);
        __syncthreads();                     // (red is free again)
        return s;
    };
    double norm2 = 2.0 * lower_squares();
    {
        double part = 0.0;
        if (tid < n) { const double x = A[pidx(tid, tid)]; part = x * x; }
        norm2 += block_sum<kWaves>(part, red);
        __syncthreads();
    }

    const int m = n + (n & 1), npairs = m / 2;
    // tiles of a step: row P, offset c in [0, npairs / 2], Q = (P + c) mod npairs -- every unordered {P, Q} once, except that an even npairs
    // meets the offset npairs / 2 from both ends (rows from npairs / 2 on skip it).  Thread -> (P, c) is the same in every step.
    const int hc = npairs / 2, tw = hc + 1, tiles = npairs * tw;
    const int tP0 = tid / tw, tc0 = tid - tP0 * tw, tdP = THREADS / tw, tdc = THREADS - tdP * tw;
    const bool even_pairs = (npairs & 1) == 0;
    double* logp = a.log + (size_t)slot * a.max_sweeps * kSweepEntries;

    int sweeps = 0;
    double off2;
    do {
        for (int r = 0; r < m - 1; ++r) {
            if (tid < npairs) {
                int p, q;
                pair_of(m, r, tid, p, q);
                const double apq = A[q * (q + 1) / 2 + p];
                double app = A[p * (p + 1) / 2 + p], aqq = A[q * (q + 1) / 2 + q];
                double t = 0.0, c = 1.0, s = 0.0;
                if (apq != 0.0) {
                    const double theta = (aqq - app) / (2.0 * apq);
                    t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + hypot(theta, 1.0));
                    c = 1.0 / sqrt(t * t + 1.0);
                    s = t * c;
                    app -= t * apq;
                    aqq += t * apq;
                }
                pp[tid] = p;
                qq[tid] = q;
                rc[tid] = c; rs[tid] = s; rpp[tid] = app; rqq[tid] = aqq;
                logp[((size_t)sweeps * (W - 1) + r) * H + tid] = t;
            }
            __syncthreads();
            int P = tP0, c = tc0;
            for (int e = tid; e < tiles; e += THREADS) {
                if (!(even_pairs && c == hc && P >= hc)) {
                    const int p1 = pp[P], q1 = qq[P];
                    if (c == 0) {
                        A[p1 * (p1 + 1) / 2 + p1] = rpp[P];
                        A[q1 * (q1 + 1) / 2 + q1] = rqq[P];
                        A[q1 * (q1 + 1) / 2 + p1] = 0.0;
                    } else {
                        int Q = P + c;
                        if (Q >= npairs) Q -= npairs;
                        const int p2 = pp[Q], q2 = qq[Q];
                        const double cP = rc[P], sP = rs[P], cQ = rc[Q], sQ = rs[Q];
                        const int i00 = pidx(p1, p2), i01 = pidx(p1, q2), i10 = pidx(q1, p2), i11 = pidx(q1, q2);
                        const double b00 = A[i00], b01 = A[i01], b10 = A[i10], b11 = A[i11];
                        const double x0 = cQ * b00 - sQ * b01, y0 = sQ * b00 + cQ * b01;        // B J_Q
                        const double x1 = cQ * b10 - sQ * b11, y1 = sQ * b10 + cQ * b11;
                        A[i00] = cP * x0 - sP * x1;                                          // J_P^T (B J_Q)
                        A[i10] = sP * x0 + cP * x1;
                        A[i01] = cP * y0 - sP * y1;
                        A[i11] = sP * y0 + cP * y1;
                    }
                }
                P += tdP;
                c += tdc;
                if (c >= tw) { c -= tw; ++P; }
            }
            __syncthreads();
        }
        ++sweeps;
        off2 = 2.0 * lower_squares();
    } while (off2 > kTol2 * norm2 && sweeps < a.max_sweeps);

    if (tid < n) lam[tid] = A[pidx(tid, tid)];
    __syncthreads();
    if (tid < n) {
        const double mine = lam[tid];
        int rank = 0;
        for (int i = 0; i < n; ++i) {
            const double o = lam[i];
            rank += (o < mine || (o == mine && i < tid)) ? 1 : 0;
        }
        order[rank] = tid;                   // (rank < n: a NaN only leaves slots at their initial value, still a column)
    }
    __syncthreads();

    // ---- replay: A's space becomes X [m][kk] and the staging area of kChunk steps ----
    const int k = a.k, kk = k < n ? k : n;
    double* X = A;
    double* cb = A + W * kMaxK;
    double* sb = cb + kChunk * H;
    int* pb = reinterpret_cast<int*>(sb + kChunk * H);
    int* qb = pb + kChunk * H;
    for (int e = tid; e < m * kk; e += THREADS) {
        const int i = e / kk, c = e - i * kk;
        X[e] = order[c] == i ? 1.0 : 0.0;
    }
    const int items = npairs * kk;
    const int xP0 = tid / kk, xc0 = tid - xP0 * kk, xdP = THREADS / kk, xdc = THREADS - xdP * kk;
    for (int sw = sweeps - 1; sw >= 0; --sw) {
        for (int rhi = m - 2; rhi >= 0; rhi -= kChunk) {
            const int rlo = rhi - kChunk + 1 > 0 ? rhi - kChunk + 1 : 0, cnt = rhi - rlo + 1;
            __syncthreads();                 // (X is initialised / the last chunk's steps are done with the staging area)
            for (int e = tid; e < cnt * npairs; e += THREADS) {
                const int j = e / npairs, ps = e - j * npairs;
                const double t = logp[((size_t)sw * (W - 1) + rlo + j) * H + ps];
                const double c = 1.0 / sqrt(t * t + 1.0);
                int p, q;
                pair_of(m, rlo + j, ps, p, q);
                cb[j * H + ps] = c;
                sb[j * H + ps] = t * c;
                pb[j * H + ps] = p;
                qb[j * H + ps] = q;
            }
            __syncthreads();
            for (int r = rhi; r >= rlo; --r) {
                const int j = (r - rlo) * H;
                int ps = xP0, col = xc0;
                for (int e = tid; e < items; e += THREADS) {
                    const double c = cb[j + ps], s = sb[j + ps];
                    const int ip = pb[j + ps] * kk + col, iq = qb[j + ps] * kk + col;
                    const double xp = X[ip], xq = X[iq];
                    X[ip] = c * xp + s * xq;
                    X[iq] = c * xq - s * xp;
                    ps += xdP;
                    col += xdc;
                    if (col >= kk) { col -= kk; ++ps; }
                }
                if (r > rlo) __syncthreads();
            }
        }
    }
    __syncthreads();

    if (tid < kk) {
        double sc = 1.0;
        if (a.norm == 2) {                   // 'walk': D^-1/2 v, unit length
            double s2 = 0.0;
            for (int i = 0; i < n; ++i) { const double x = X[i * kk + tid] * dsc[i]; s2 += x * x; }
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
            x = X[i * kk + c];
            if (a.norm == 2) x = x * dsc[i] * cscale[c];
        }
        out[e] = (float)x;
    }
    if (a.val && tid < k) a.val[(int64_t)g * k + tid] = tid < kk ? lam[order[tid]] : __builtin_nan("");
    if (tid == 0) a.status[g] = sweeps;
}

// the widest class's LDS against what the device grants a workgroup: asked once per device
static int lds_granted() {
    static std::atomic<unsigned long long> ok{0};
    int dev = 0;
    DGN_HIP_CHECK(hipGetDevice(&dev));
    const unsigned long long bit = dev >= 0 && dev < 64 ? 1ull << dev : 0;
    if (ok.load(std::memory_order_acquire) & bit) return DGN_OK;
    int limit = 0, optin = 0;
    DGN_HIP_CHECK(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    if (hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, dev) != hipSuccess) {
        (void)hipGetLastError();
        optin = 0;
    }
    if (optin > limit) limit = optin;
    if (limit < Lds<192>::kBytes) {
        set_error("dgn_eig_mid: the 192-node class needs %d bytes of LDS per workgroup, the device grants %d", Lds<192>::kBytes, limit);
        return DGN_ERR_INVALID;
    }
    ok.fetch_or(bit, std::memory_order_release);
    return DGN_OK;
}

}  // namespace eig_mid
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_eig_mid_max_nodes(void) { return eig_mid::kMaxNodes; }

extern "C" size_t dgn_eig_mid_workspace_bytes(int n_slots, int max_sweeps) {
    if (n_slots <= 0 || max_sweeps <= 0) return 0;
    return (size_t)n_slots * (size_t)max_sweeps * eig_mid::kSweepEntries * sizeof(double);
}

extern "C" int dgn_eig_mid(const DgnGraph* graph, const int64_t* graph_off, int n_graphs, const int32_t* graph_ids, int n_ids, int k, int norm,
                           int max_sweeps, float* vec, double* val, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    if (!graph || !graph->indptr || (graph->n_edges > 0 && !graph->src)) { set_error("dgn_eig_mid: null CSR"); return DGN_ERR_INVALID; }
    if (graph->n_nodes < 0 || graph->n_edges < 0 || graph->n_nodes >= INT32_MAX || graph->n_edges >= INT32_MAX) {
        set_error("dgn_eig_mid: graph outside the int32 CSR range");
        return DGN_ERR_INVALID;
    }
    if (n_graphs < 0) { set_error("dgn_eig_mid: n_graphs = %d < 0", n_graphs); return DGN_ERR_INVALID; }
    if (n_ids < 0) { set_error("dgn_eig_mid: n_ids = %d < 0", n_ids); return DGN_ERR_INVALID; }
    if (k < 1 || k > eig_mid::kMaxK) { set_error("dgn_eig_mid: k = %d outside 1 .. %d", k, eig_mid::kMaxK); return DGN_ERR_INVALID; }
    if (norm < DGN_EIG_NORM_NONE || norm > DGN_EIG_NORM_WALK) { set_error("dgn_eig_mid: unknown norm %d", norm); return DGN_ERR_INVALID; }
    if (max_sweeps < 1) { set_error("dgn_eig_mid: max_sweeps = %d < 1", max_sweeps); return DGN_ERR_INVALID; }
    if (!graph_off || !vec || !status) { set_error("dgn_eig_mid: null graph_off / vec / status"); return DGN_ERR_INVALID; }
    const int slots = graph_ids ? n_ids : n_graphs;
    if (n_graphs == 0 || slots == 0) return DGN_OK;
    const size_t need = dgn_eig_mid_workspace_bytes(slots, max_sweeps);
    if (!ws) { set_error("dgn_eig_mid: null workspace (%zu bytes for %d slots of %d sweeps)", need, slots, max_sweeps); return DGN_ERR_INVALID; }
    if (ws_bytes < need) {
        set_error("dgn_eig_mid: workspace of %zu bytes, %d slots of %d sweeps need %zu", ws_bytes, slots, max_sweeps, need);
        return DGN_ERR_WORKSPACE;
    }
    if (const int rc = eig_mid::lds_granted()) return rc;
    eig_mid::Args a{graph->indptr, graph->src, graph->n_nodes, graph->n_edges, graph_off, graph_ids, n_graphs, k, norm, max_sweeps, vec, val, status,
                    static_cast<double*>(ws)};
    hipStream_t s = static_cast<hipStream_t>(stream);
    static LdsOptIn lds_ok{0};
    DGN_HIP_CHECK(allow_lds(lds_ok, eig_mid::Lds<192>::kBytes, &eig_mid::eig_mid_kernel<128, 512>, &eig_mid::eig_mid_kernel<192, 1024>));
    hipLaunchKernelGGL((eig_mid::eig_mid_kernel<128, 512>), dim3((unsigned)slots), dim3(512), eig_mid::Lds<128>::kBytes, s, a);
    DGN_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL((eig_mid::eig_mid_kernel<192, 1024>), dim3((unsigned)slots), dim3(1024), eig_mid::Lds<192>::kBytes, s, a);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}
