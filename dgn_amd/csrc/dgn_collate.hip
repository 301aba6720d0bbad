// Collate of a device-resident dataset (include/dgn_hip.h: dgn_collate): what the reference's `collate` methods do on the host per
// step -- dgl.batch over 128 graph objects plus the graph-norm vectors, data/molecules.py:219-230 and its four siblings -- as ONE
// gather kernel.  The dataset's CSR was built once (dgn_graph_build over all its nodes); the graphs of a batch are disjoint and each
// graph's nodes, edges, CSR slots and CSC ranks are one contiguous range of the dataset, so every output is a run of per-graph copies
// with a per-graph shift: no sort, no scan, nothing read back.
//
//   segments     every wanted output is a "segment": (operation, domain, input, output, element count).  The grid is indexed over the
//                output elements of all segments, kBlockElems per workgroup; a workgroup finds its segment by its block index
//                (wave-uniform: the descriptors travel in the kernel arguments).
//   the graph    of a node row / edge slot: binary search over the batch's offsets (last j with off[j] <= x: graphs without edges
//                share an offset with their successor and are never found).  A workgroup first brackets its own row range by two
//                uniform searches; at most kChunk graphs in the bracket: their offsets go to LDS and every element searches there,
//                more (runs of tiny graphs, graphs without edges): every element searches the bracket in global memory.
//   columns      a thread owns four consecutive dwords.  Inside one graph's run the source dwords are consecutive too: one 16-byte
//                load and store when BOTH addresses are 16-byte aligned (12-, 24- and 72-byte rows shift the two sides against each
//                other from graph to graph), four dword accesses otherwise.  All other segments: elements strided by the block size.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dgn_common.hpp"

namespace dgn {
namespace collate {

constexpr int kThreads = 256;
constexpr int kPer = 4;                          // elements per thread
constexpr int kBlockElems = kThreads * kPer;
constexpr int kChunk = 512;                      // offsets of a workgroup's bracket held in LDS
constexpr int kMaxSegs = DGN_COLLATE_MAX_NODE_COLS + DGN_COLLATE_MAX_EDGE_COLS + DGN_COLLATE_MAX_GRAPH_COLS + 16;

enum Op : int32_t {
    OP_COL,          // out dword [row, c] = in dword [dataset row, c]; the pad pattern behind the batch
    OP_NORM,         // out [row] = in [dataset graph of the row]; 0 behind
    OP_GID,          // out [row] = batch graph of the row; -1 behind
    OP_PTR,          // out [row] = in [dataset row] shifted by the graph's EDGE offset; E from row N on (n_rows_out + 1 elements)
    OP_SHIFT32,      // out [slot] = in [dataset slot] + shift (of the nodes or of the edges); 0 behind
    OP_SHIFT64,      // the same on int64
    OP_CONST         // out dwords = (lo, hi, 0, 0, ...) of `pad`
};
enum Dom : int32_t { DOM_NODE = 0, DOM_EDGE = 1, DOM_GRAPH = 2 };
// rows of the table
enum { T_NODE_OFF = 0, T_EDGE_OFF = 1, T_NODE_BASE = 2, T_EDGE_BASE = 3, T_GID = 4 };

struct Seg {
    const void* in;
    void* out;
    int64_t n;           // output elements
    int64_t pad;
    uint32_t block0;     // first workgroup of the segment
    int32_t w;           // dwords per row (OP_COL), 1 otherwise
    int32_t op, dom;
    int32_t shift_dom;   // OP_SHIFT*: whose shift the values take
};

struct Args {
    Seg seg[kMaxSegs];
    const int32_t* table;
    int64_t N, E;
    int32_t G, n_seg;
};

// last j in [lo, hi] with off[j] <= x (off[lo] <= x given)
template <class P>
__device__ __forceinline__ int last_le(P off, int lo, int hi, int32_t x) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void collate_gather(const Args a) {
    __shared__ int32_t s_off[kChunk];
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x;
    int s = 0;
    for (int i = 1; i < a.n_seg; ++i)
        if (b >= a.seg[i].block0) s = i;
    const Seg& sg = a.seg[s];
    const int op = sg.op, dom = sg.dom, w = sg.w;
    const int64_t n = sg.n;
    const int64_t e0 = (int64_t)(b - sg.block0) * kBlockElems;
    const int64_t e1 = e0 + kBlockElems < n ? e0 + kBlockElems : n;
    uint32_t* out32 = static_cast<uint32_t*>(sg.out);
    const uint32_t* in32 = static_cast<const uint32_t*>(sg.in);
    const uint32_t pad_lo = (uint32_t)sg.pad, pad_hi = (uint32_t)((uint64_t)sg.pad >> 32);

    if (op == OP_CONST) {
        for (int64_t e = e0 + tid; e < e1; e += kThreads) out32[e] = e == 0 ? pad_lo : (e == 1 ? pad_hi : 0u);
        return;
    }
    const int G = a.G;
    const int64_t stride = (int64_t)G + 1;
    const int32_t* tab = a.table;
    const int32_t* off = tab + (dom == DOM_EDGE ? T_EDGE_OFF : T_NODE_OFF) * stride;
    const int32_t* base = tab + (dom == DOM_EDGE ? T_EDGE_BASE : T_NODE_BASE) * stride;
    const int32_t* gid = tab + T_GID * stride;
    // rows of the batch in this segment's domain (an empty batch: every row is padding and the table is never read)
    const int64_t count = G == 0 ? 0 : (dom == DOM_NODE ? a.N : (dom == DOM_EDGE ? a.E : (int64_t)G));
    // the block's row range, in 64-bit once per block; inside it 32-bit offsets
    const int64_t row_lo = e0 / w;
    const int c_lo = (int)(e0 - row_lo * w);
    const int64_t row_hi = (e1 - 1) / w;

    int j_lo = 0, j_hi = 0;
    bool in_lds = false;
    if (dom != DOM_GRAPH && row_lo < count) {
        const int64_t rh = row_hi < count - 1 ? row_hi : count - 1;
        j_lo = last_le(off, 0, G - 1, (int32_t)row_lo);
        j_hi = last_le(off, j_lo, G - 1, (int32_t)rh);
        in_lds = j_hi - j_lo < kChunk;
        if (in_lds)
            for (int i = tid; i <= j_hi - j_lo; i += kThreads) s_off[i] = off[j_lo + i];
    }
    __syncthreads();
    // batch graph of a row below `count` of the block's range
    auto graph_of = [&](int64_t row) -> int {
        if (dom == DOM_GRAPH) return (int)row;
        if (in_lds) return j_lo + last_le(s_off, 0, j_hi - j_lo, (int32_t)row);
        return last_le(off, j_lo, j_hi, (int32_t)row);
    };
    // dataset row of row `row` of batch graph j
    auto data_row = [&](int64_t row, int j) -> int64_t {
        return dom == DOM_GRAPH ? (int64_t)gid[j] : (int64_t)base[j] + (row - off[j]);
    };

    if (op == OP_COL) {
        const int64_t q0 = e0 + (int64_t)tid * kPer;
        if (q0 >= e1) return;
        const int t0 = c_lo + tid * kPer;                         // dword offset from the start of row_lo: below w + kBlockElems
        const int dr0 = t0 / w, c0 = t0 - dr0 * w;
        const int64_t row0 = row_lo + dr0;
        if (q0 + kPer <= e1) {
            const int dr3 = (t0 + kPer - 1) / w;
            const int64_t row3 = row_lo + dr3;
            if (row3 < count) {
                const int j0 = graph_of(row0);
                const bool one_run = dr3 == dr0 || (dom != DOM_GRAPH && graph_of(row3) == j0);
                if (one_run) {
                    const uint32_t* src = in32 + data_row(row0, j0) * w + c0;
                    uint32_t* dst = out32 + q0;
                    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0) {
                        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
                    } else {
#pragma unroll
                        for (int i = 0; i < kPer; ++i) dst[i] = src[i];
                    }
                    return;
                }
            }
        }
        // the general case: a thread's dwords cross a graph boundary, the end of the batch or the end of the segment
        for (int i = 0; i < kPer && q0 + i < e1; ++i) {
            const int t = t0 + i;
            const int dr = t / w, c = t - dr * w;
            const int64_t row = row_lo + dr;
            uint32_t v = (c & 1) ? pad_hi : pad_lo;
            if (row < count) {
                const int j = graph_of(row);
                v = in32[data_row(row, j) * w + c];
            }
            out32[q0 + i] = v;
        }
        return;
    }

    const int32_t* node_off = tab + T_NODE_OFF * stride;
    const int32_t* node_base = tab + T_NODE_BASE * stride;
    const int32_t* edge_off = tab + T_EDGE_OFF * stride;
    const int32_t* edge_base = tab + T_EDGE_BASE * stride;
    for (int64_t e = e0 + tid; e < e1; e += kThreads) {           // (w == 1: an element is a row)
        const bool real = e < count;
        const int j = real ? graph_of(e) : 0;
        const int64_t r = real ? data_row(e, j) : 0;
        switch (op) {
        case OP_NORM:
            out32[e] = real ? in32[gid[j]] : 0u;
            break;
        case OP_GID:
            out32[e] = real ? (uint32_t)j : 0xffffffffu;
            break;
        case OP_PTR:
            out32[e] = real ? (uint32_t)((int32_t)in32[r] - edge_base[j] + edge_off[j]) : (uint32_t)a.E;
            break;
        case OP_SHIFT32: {
            const int32_t sh = !real ? 0 : (sg.shift_dom == DOM_NODE ? node_off[j] - node_base[j] : edge_off[j] - edge_base[j]);
            out32[e] = real ? (uint32_t)((int32_t)in32[r] + sh) : 0u;
            break;
        }
        default: {                                                // OP_SHIFT64
            const int64_t sh = !real ? 0 : (sg.shift_dom == DOM_NODE ? (int64_t)node_off[j] - node_base[j] : (int64_t)edge_off[j] - edge_base[j]);
            static_cast<int64_t*>(sg.out)[e] = real ? static_cast<const int64_t*>(sg.in)[r] + sh : 0;
            break;
        }
        }
    }
}

struct Plan {
    Args a;
    uint64_t blocks;
};

inline void add(Plan& p, int op, int dom, const void* in, void* out, int64_t n, int w = 1, int64_t pad = 0, int shift_dom = DOM_NODE) {
    if (!out || n <= 0) return;
    Seg& s = p.a.seg[p.a.n_seg++];
    s.in = in; s.out = out; s.n = n; s.pad = pad; s.w = w; s.op = op; s.dom = dom; s.shift_dom = shift_dom;
    s.block0 = (uint32_t)p.blocks;
    p.blocks += (uint64_t)((n + kBlockElems - 1) / kBlockElems);
}

// the columns of one domain; false (error set) on a bad descriptor
inline bool add_cols(Plan& p, const char* what, int dom, int n_cols, int max_cols, const void* const* in, void* const* out, const int64_t* pad,
                     const int32_t* row_bytes, int64_t rows_out) {
    if (n_cols < 0 || n_cols > max_cols) { set_error("dgn_collate: %d %s columns (at most %d)", n_cols, what, max_cols); return false; }
    for (int c = 0; c < n_cols; ++c) {
        if (!out[c]) continue;
        if (!in[c]) { set_error("dgn_collate: %s column %d has an output and no input", what, c); return false; }
        if (row_bytes[c] <= 0 || row_bytes[c] % 4) { set_error("dgn_collate: %s column %d: %d bytes per row (a positive multiple of 4 required)", what, c, row_bytes[c]); return false; }
        if ((reinterpret_cast<uintptr_t>(in[c]) | reinterpret_cast<uintptr_t>(out[c])) & 3) { set_error("dgn_collate: %s column %d is not 4-byte aligned", what, c); return false; }
        const int w = row_bytes[c] / 4;
        if (rows_out > INT64_MAX / 4 / w) { set_error("dgn_collate: %s column %d is too large", what, c); return false; }
        add(p, OP_COL, dom, in[c], out[c], rows_out * w, w, pad[c]);
    }
    return true;
}

}  // namespace collate
}  // namespace dgn

using namespace dgn;

extern "C" int dgn_collate(const DgnCollate* c, void* stream) {
    using namespace collate;
    const char* fn = "dgn_collate";
    if (!c) { set_error("%s: null description", fn); return DGN_ERR_INVALID; }
    const int64_t G = c->n_graphs, N = c->n_nodes, E = c->n_edges;
    if (G < 0 || G > DGN_COLLATE_MAX_GRAPHS) { set_error("%s: 0 <= n_graphs <= %d required", fn, DGN_COLLATE_MAX_GRAPHS); return DGN_ERR_INVALID; }
    if (N < 0 || E < 0 || N >= INT32_MAX - 1 || E >= INT32_MAX - 1 || c->n_rows_out >= INT32_MAX - 1 || c->e_rows_out >= INT32_MAX - 1) {
        set_error("%s: sizes outside the int32 CSR range", fn);
        return DGN_ERR_INVALID;
    }
    if (c->n_rows_out < N || c->e_rows_out < E || c->g_rows_out < G) { set_error("%s: the batch (%lld nodes, %lld edges, %lld graphs) exceeds the outputs' rows", fn, (long long)N, (long long)E, (long long)G); return DGN_ERR_INVALID; }
    if (G == 0 && (N || E)) { set_error("%s: nodes or edges without a graph", fn); return DGN_ERR_INVALID; }
    if (G > 0 && !c->table) { set_error("%s: null table", fn); return DGN_ERR_INVALID; }
    Plan p{};
    p.a.table = c->table;
    p.a.G = (int32_t)(N ? G : 0);
    p.a.N = p.a.G ? N : 0; p.a.E = p.a.G ? E : 0;
    const int64_t n_out = c->n_rows_out, e_out = c->e_rows_out;
    if (!add_cols(p, "node", DOM_NODE, c->n_node_cols, DGN_COLLATE_MAX_NODE_COLS, c->node_in, c->node_out, c->node_pad, c->node_row_bytes, n_out) ||
        !add_cols(p, "edge", DOM_EDGE, c->n_edge_cols, DGN_COLLATE_MAX_EDGE_COLS, c->edge_in, c->edge_out, c->edge_pad, c->edge_row_bytes, e_out) ||
        !add_cols(p, "graph", DOM_GRAPH, c->n_graph_cols, DGN_COLLATE_MAX_GRAPH_COLS, c->graph_in, c->graph_out, c->graph_pad, c->graph_row_bytes, c->g_rows_out))
        return DGN_ERR_INVALID;
    // an output that is wanted needs the dataset array it is cut from (a dataset without edges has no per-edge arrays: never read)
    struct Want { const void* in; const void* out; const char* name; bool per_edge; };
    const Want wants[] = {{c->d_snorm_n, c->snorm_n, "snorm_n", false}, {c->d_snorm_e, c->snorm_e, "snorm_e", true}, {c->d_edge_src, c->src, "src", true},
                          {c->d_edge_dst, c->dst, "dst", true}, {c->d_indptr, c->indptr, "indptr", false}, {c->d_src, c->src_csr, "src_csr", true},
                          {c->d_dst_csr, c->dst_csr, "dst_csr", true}, {c->d_eid, c->eid, "eid", true}, {c->d_in_degree, c->in_degree, "in_degree", false},
                          {c->d_log_deg, c->log_deg, "log_deg", false}, {c->d_csc_ptr, c->csc_ptr, "csc_ptr", false}, {c->d_csc_pos, c->csc_pos, "csc_pos", true},
                          {c->d_csc_order, c->csc_order, "csc_order", true}};
    for (const Want& wn : wants)
        if (wn.out && !wn.in && (wn.per_edge ? p.a.E : p.a.N) > 0) {
            set_error("%s: output %s wanted without the dataset array it is cut from", fn, wn.name);
            return DGN_ERR_INVALID;
        }
    add(p, OP_NORM, DOM_NODE, c->d_snorm_n, c->snorm_n, n_out);
    add(p, OP_NORM, DOM_EDGE, c->d_snorm_e, c->snorm_e, e_out);
    add(p, OP_GID, DOM_NODE, nullptr, c->graph_id, n_out);
    add(p, OP_SHIFT64, DOM_EDGE, c->d_edge_src, c->src, e_out, 1, 0, DOM_NODE);
    add(p, OP_SHIFT64, DOM_EDGE, c->d_edge_dst, c->dst, e_out, 1, 0, DOM_NODE);
    add(p, OP_PTR, DOM_NODE, c->d_indptr, c->indptr, n_out + 1);
    add(p, OP_SHIFT32, DOM_EDGE, c->d_src, c->src_csr, e_out, 1, 0, DOM_NODE);
    add(p, OP_SHIFT32, DOM_EDGE, c->d_dst_csr, c->dst_csr, e_out, 1, 0, DOM_NODE);
    add(p, OP_SHIFT64, DOM_EDGE, c->d_eid, c->eid, e_out, 1, 0, DOM_EDGE);
    add(p, OP_COL, DOM_NODE, c->d_in_degree, c->in_degree, n_out * 2, 2, 0);
    add(p, OP_COL, DOM_NODE, c->d_log_deg, c->log_deg, n_out, 1, 0);
    add(p, OP_PTR, DOM_NODE, c->d_csc_ptr, c->csc_ptr, n_out + 1);
    add(p, OP_SHIFT32, DOM_EDGE, c->d_csc_pos, c->csc_pos, e_out, 1, 0, DOM_EDGE);
    add(p, OP_SHIFT32, DOM_EDGE, c->d_csc_order, c->csc_order, e_out, 1, 0, DOM_EDGE);
    add(p, OP_CONST, DOM_GRAPH, nullptr, c->stats, 4, 1, (int64_t)(uint32_t)(p.a.G ? c->max_in_degree : 0));
    add(p, OP_CONST, DOM_GRAPH, nullptr, c->n_valid, 2, 1, p.a.N);
    static_assert(kMaxSegs >= DGN_COLLATE_MAX_NODE_COLS + DGN_COLLATE_MAX_EDGE_COLS + DGN_COLLATE_MAX_GRAPH_COLS + 16, "one segment per output");
    if (p.a.n_seg == 0) return DGN_OK;
    if (p.blocks >= (uint64_t)INT32_MAX) { set_error("%s: the outputs exceed the grid (%llu workgroups)", fn, (unsigned long long)p.blocks); return DGN_ERR_INVALID; }
    hipLaunchKernelGGL(collate_gather, dim3((unsigned)p.blocks), dim3(kThreads), 0, static_cast<hipStream_t>(stream), p.a);
    DGN_HIP_CHECK(hipGetLastError());
    return DGN_OK;
}
