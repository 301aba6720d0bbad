/*
 * dgn_hip.h -- C ABI of libdgn_hip.so: the MI355X (gfx950) implementation of the DGN
 * directional-aggregation hot path.
 *
 * The reference (Saro00/DGN) is pure Python and has no FFI; what this library replaces is
 * the span between `g.apply_edges(...)` and the end of `reduce_func` inside every DGN layer
 * variant, i.e. (paths relative to the reference tree)
 *
 *   realworld_benchmark/nets/dgn_layer.py:183-186  (DGNLayerSimple:  apply_edges + update_all)
 *   realworld_benchmark/nets/dgn_layer.py:112-115  (DGNLayerComplex: apply_edges + update_all)
 *   realworld_benchmark/nets/dgn_layer.py:261-264  (DGNTower:        apply_edges + update_all)
 *   realworld_benchmark/nets/dgn_layer.py:161-173  (reduce_func: aggregator concat, scaler concat)
 *   realworld_benchmark/nets/aggregators.py:8-71   (the aggregators)
 *   realworld_benchmark/nets/scalers.py:7-18       (the degree scalers)
 *
 * plus the autograd backward of all of the above.  The reference-side binding a maintainer
 * would add (a ctypes stub called from a torch.autograd.Function) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C; every pointer is a DEVICE pointer owned by the caller unless stated otherwise;
 *   - sizes/strides are int64_t, strides ("ld") are in ELEMENTS (floats), not bytes;
 *   - every call enqueues on the caller's hipStream_t (passed as void*), never synchronises,
 *     keeps no global mutable state, and is re-entrant from several host threads;
 *   - return value: 0 = ok, < 0 = error (DGN_ERR_*); dgn_last_error() gives the thread-local text;
 *   - the graph is CSR by DESTINATION: slot range [indptr[i], indptr[i+1]) holds the in-edges of
 *     node i in ascending original edge id (the DGL mailbox order the oracle encodes).
 */
#ifndef DGN_HIP_H
#define DGN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGN_ABI_VERSION 38

#define DGN_MAX_AGG 16     /* aggregators per launch (the host splits longer lists)            */
#define DGN_MAX_CH 4       /* edge-weight channels per launch                                   */
#define DGN_MAX_SCALERS 4  /* applied scalers                                                   */

enum {
    DGN_OK = 0,
    DGN_ERR_INVALID = -1,   /* bad argument / unsupported shape                                 */
    DGN_ERR_WORKSPACE = -2, /* workspace too small                                              */
    DGN_ERR_HIP = -3        /* a HIP runtime call failed                                        */
};

/* aggregator op codes; `ch` = edge-weight channel the op reads (ignored by the first six)      */
enum {
    DGN_AGG_MEAN = 0,        /* aggregators.py:8   (1/d) sum_j m_j                              */
    DGN_AGG_SUM = 1,         /* aggregators.py:31  sum_j m_j                                    */
    DGN_AGG_MAX = 2,         /* aggregators.py:12                                               */
    DGN_AGG_MIN = 3,         /* aggregators.py:16                                               */
    DGN_AGG_STD = 4,         /* aggregators.py:20  sqrt(var + eps)                              */
    DGN_AGG_VAR = 5,         /* aggregators.py:24  relu(mean(m^2) - mean(m)^2)                  */
    DGN_AGG_DIR_AV = 6,      /* aggregators.py:35  sum_j |w_j| m_j            (ABSNORM channel) */
    DGN_AGG_DIR_WSUM = 7,    /* aggregators.py:42  sum_j w_j m_j              (SOFTMAX channel) */
    DGN_AGG_DIR_DX = 8,      /* aggregators.py:48/:62  |sum_j w_j m_j - (sum_j w_j) x_i|        */
    DGN_AGG_DIR_DX_NO_ABS = 9, /* aggregators.py:55  sum_j w_j m_j - (sum_j w_j) x_i            */
    DGN_AGG_X_IN = 10        /* not an aggregator: copies x_in (h_in) into the output row, so that
                                posttrans([h || agg]) of dgn_layer.py:116-119 is ONE GEMM on the sweep's output */
};

/* edge-weight channel kinds: how delta_j = eig[src_j,k] - eig[dst,k] becomes a per-edge weight */
enum {
    DGN_W_ABSNORM = 0,  /* delta_j / (sum_j |delta_j| + eps)                 aggregators.py:49  */
    DGN_W_BALANCED = 1, /* (relu(d)/(sum relu(d)+eps) + relu(-d)/(sum relu(-d)+eps)) / 2   :63-69 */
    DGN_W_SOFTMAX = 2   /* softmax_j(alpha * |delta_j|)                      aggregators.py:43  */
};

/* degree scalers, scalers.py:7-18; D = in-degree, avg = avg_d['log']                           */
enum {
    DGN_SCALE_IDENTITY = 0,
    DGN_SCALE_AMPLIFICATION = 1, /* x * (log(D+1) / avg)                                        */
    DGN_SCALE_ATTENUATION = 2    /* x * (avg / log(D+1))                                        */
};

typedef struct DgnGraph {
    int64_t n_nodes;
    int64_t n_edges;
    const int32_t* indptr;  /* [n_nodes+1]                                                       */
    const int32_t* src;     /* [n_edges] source node of each CSR slot                            */
    /* Rows with more than hub_threshold in-edges are "hub rows": the row kernels skip them and
     * they are processed in slices of hub_chunk edges (partials in the workspace, then a combine).
     * n_hub == 0 disables the mechanism.                                                        */
    int64_t n_hub;
    const int32_t* hub_rows;      /* [n_hub] node ids, ascending                                 */
    const int32_t* hub_chunk_ptr; /* [n_hub+1] first chunk of every hub row                      */
    int64_t n_chunks;
    const int32_t* chunk_hub;     /* [n_chunks] index into hub_rows                              */
    int32_t hub_threshold;
    int32_t hub_chunk;
    /* Optional transposed view (NULL = absent), used by dgn_agg_backward to avoid atomics: csc_pos[j] is the
     * rank of CSR slot j when the slots are ordered by (source node, slot) and csc_ptr[u] the first such rank
     * of source u.  With it (and a large enough workspace) the backward writes every per-edge gradient row
     * to its csc position and a second kernel sums each source's contiguous rows: deterministic, no atomics. */
    const int32_t* csc_ptr;  /* [n_src+1]   */
    const int32_t* csc_pos;  /* [n_edges]   */
    /* Hint: largest in-degree, 0 = unknown.  Lets launches that only concern long rows be skipped.       */
    int32_t max_in_degree;
    /* Number of SOURCE nodes when it differs from n_nodes (0 = same): a bipartite CSR whose rows are e.g. the
     * graphs of a batch and whose sources are its nodes -- the readouts (dgl.mean_nodes / sum_nodes / max_nodes,
     * nets/.../dgn_net.py:71-86) are this sweep over such a CSR.  x_src / g_src have n_src rows, csc_ptr
     * n_src + 1 entries; x_dst, x_in, log_deg, out are per destination row.                               */
    int64_t n_src;
    /* Destination-range shard of a larger graph (one giant graph split across GPUs, dgn_amd/dist.py): row i of
     * this CSR is node row_base + i of the source node set.  Only dgn_edge_weights uses it (the destination side of
     * eig is read at row row_base + i); the per-row arrays of the sweep (x_dst, x_in, log_deg, out) are the shard's. */
    int64_t row_base;
    /* Optional (NULL = absent): block description of a batch of small graphs, built by dgn_graph_build_cuts.  blk_cut[i], i in
     * [0, n_nodes], is the last CLOSED cut <= i -- a cut c is closed when no edge joins a node below c to a node at or above it (the
     * graph boundaries of a dgl.batch, data/molecules.py:229); blk_gap is the largest distance between consecutive closed cuts (the
     * largest graph).  With it dgn_agg_backward (define mode, hot aggregator lists, one feature tile, no hub rows, no edge term, at most
     * 3 edges per node) lets ONE WAVE own a run of whole graphs and accumulate d x_src in its LDS rows: one kernel, no [E, F] staging
     * buffer, the adds in ascending (source, slot) order as in the staged path (run-to-run reproducible).                       */
    const int32_t* blk_cut;  /* [n_nodes+1] */
    int32_t blk_gap;
    /* Optional (NULL = absent): batches of graphs too large for that (k-NN superpixel graphs, data/superpixels.py:139-145; SBM graphs).
     * gblk_desc [n_gblk][4] int32, 16-byte aligned: first row, end row, first CSR slot, end CSR slot of blocks of WHOLE graphs that
     * partition [0, n_nodes) in order, gblk_rows = the largest block; csc_order[k] = the CSR slot with (source, slot) rank k (the
     * inverse of csc_pos), dst_csr[j] = the row of CSR slot j.  With them (and csc_ptr) dgn_agg_backward (define mode, baked-in lists
     * without max / min / std / var, no edge term, the aux table where the list has a dx aggregator) runs ONE kernel, a workgroup per
     * block: the destination rows' coefficient vectors in LDS, every source row gathering its out-edges -- no [E, F] staging buffer.  */
    const int32_t* gblk_desc; int64_t n_gblk; int32_t gblk_rows;
    const int32_t* csc_order;  /* [n_edges] */
    const int32_t* dst_csr;    /* [n_edges] */
} DgnGraph;

typedef struct DgnChannel {
    int32_t kind;     /* DGN_W_*                                                                 */
    int32_t eig_col;  /* column k of eig                                                         */
    float alpha;      /* SOFTMAX only                                                            */
    float eps;        /* 1e-8 on the DGL path (aggregators.py:5)                                 */
} DgnChannel;

typedef struct DgnAggSpec {
    int32_t n_agg;
    int32_t agg_op[DGN_MAX_AGG];
    int32_t agg_ch[DGN_MAX_AGG];
    int32_t n_ch;                      /* channels referenced by agg_ch (0..DGN_MAX_CH)          */
    int32_t n_scalers;                 /* scalers APPLIED; a lone scaler of any name is the
                                          identity (dgn_layer.py:170)                            */
    int32_t scaler[DGN_MAX_SCALERS];
    float avg_log;                     /* avg_d['log']                                           */
    float eps;                         /* EPS of aggregators.py:5, used by STD                   */
    int32_t n_towers;                  /* T >= 1: output columns are laid out [T][S][A][F/T];
                                          T == 1 is the reference order [S][A][F]                */
    /* A launch may compute a slice of a longer aggregator list: the columns it writes are those of
     * aggregators [agg_offset, agg_offset + n_agg) out of agg_total (0 = n_agg, offset 0).       */
    int32_t agg_total;
    int32_t agg_offset;
    /* Distance (in elements) between the column blocks of consecutive towers; 0 = n_scalers*agg_total*(F/T),
     * i.e. the towers of a node are contiguous inside its row.  With tower_stride = n_nodes*ld_out and
     * ld_out = n_scalers*agg_total*(F/T) the output is tower-major [T][N][S*A*F/T]: the batched per-tower GEMMs
     * that follow then read (and their backward writes) contiguous matrices.  Applies to out and g_out.   */
    int64_t tower_stride;
} DgnAggSpec;

/* The message of CSR slot j into node i is  m_j = x_src[src_j] + x_dst[i] + m_edge[j];
 * any of the three terms may be NULL, but one of the two GATHERED terms, x_src or m_edge, must be given: x_dst alone (the
 * same message in every slot of a row) is refused with DGN_ERR_INVALID.
 *   simple layer:            x_src = h                                   (dgn_layer.py:154-155)
 *   complex/towers, 1-layer pretrans:  x_src = h W_s^T, x_dst = h W_d^T + b (+ m_edge = ef W_e^T)
 *   any other pretrans:      m_edge = materialised messages in CSR slot order
 * x_in is h_in of reduce_func (dgn_layer.py:162), needed by the dx aggregators.                 */
typedef struct DgnMsg {
    int64_t F;
    const float* x_src;  int64_t ld_src;   /* [n_nodes, ld_src]                                  */
    const float* x_dst;  int64_t ld_dst;   /* [n_nodes, ld_dst]                                  */
    const float* m_edge; int64_t ld_edge;  /* [n_edges, ld_edge], CSR slot order                 */
    const float* x_in;   int64_t ld_in;    /* [n_nodes, ld_in]                                   */
    /* Edge-TYPE table (optional; needs x_src): with edge_type != NULL, m_edge is a table [n_edge_types, ld_edge] and slot j
     * adds row edge_type[j] (values in 0 .. n_edge_types-1, CSR slot order) -- the edge-feature term of the pretrans Linear when
     * the edge features are an embedding lookup (nets/molecules_graph_regression/dgn_net.py:53,75: e = embedding_e(bond type);
     * dgn_layer.py:159-160: pretrans(cat[h_src, h_dst, e])): the caller passes table = embedding W_e^T instead of materialising
     * [n_edges, F].  n_edge_types * F <= DGN_MAX_EDGE_TABLE floats.  The backward then needs the two-phase scatter (g->csc_*
     * and a workspace that includes dgn_agg_edge_table_workspace_bytes()); DgnMsgGrad.g_edge is the TABLE's gradient.       */
    const int32_t* edge_type; int32_t n_edge_types;
    /* f_valid (0: every row holds F columns): the rows of x_src and x_in hold only f_valid = F - 1 columns (F even; dense rows of an ODD
     * width at their own strides, 4-byte aligned) and the sweep reads the last column pair as (x[F - 2], 0) -- what a zero-padded copy of
     * the rows would give, without the copy (the simple layer at hidden 75 / 65: configs ZINC simple, CIFAR10).  Only with x_src (and
     * x_in) alone -- no x_dst, no m_edge, one tower -- and only for the aggregator lists dgn_agg_f_valid_supported() accepts.          */
    int32_t f_valid;
} DgnMsg;
int dgn_agg_f_valid_supported(const DgnAggSpec* spec);      /* 1: this list has kernels for rows of an odd width (DgnMsg.f_valid) */
#define DGN_MAX_EDGE_TABLE 8192

/* Gradient sinks of dgn_agg_backward; NULL = not wanted.  g_edge is always overwritten.  g_src / g_dst / g_in:
 *   accumulate != 0: the call ADDS into caller-initialised buffers (a plan split into several launches, or a
 *                    caller summing several graphs' gradients);
 *   accumulate == 0: the call DEFINES them, the buffers may arrive uninitialised (with the two-phase scatter
 *                    every row is written exactly once: no zero-fill and no read-modify-write traffic; the
 *                    atomic scatter zero-fills them itself).
 * g_in may alias g_src (the simple layer's x_in IS x_src: both gradients land in one buffer).          */
typedef struct DgnMsgGrad {
    float* g_src;  int64_t ld_src;
    float* g_dst;  int64_t ld_dst;
    float* g_edge; int64_t ld_edge;
    float* g_in;   int64_t ld_in;
    int32_t accumulate;
} DgnMsgGrad;

int dgn_abi_version(void);
size_t dgn_sizeof(const char* struct_name);      /* sizeof of a struct of this header as the library was compiled ("DgnGraph", ...); 0: unknown */
/* Process-wide library options (experiments and tests; every default is what the benchmarks run).  Each option takes its initial value
 * from an environment variable ONCE, when the library first looks; afterwards only dgn_set_option changes it -- no entry point reads the
 * environment on a launch path.  Names: "blk_lds_kb" (DGN_BLK_LDS_KB, 13), "blk_min_nodes" (DGN_BLK_MIN_NODES, 131072),
 * "bwd_rows_per_wave" (DGN_BWD_ROWS_PER_WAVE, 4), "tile_gemm" / "tile_wgrad" (DGN_TILE_GEMM / DGN_TILE_WGRAD, -1 = by shape),
 * "no_zmask" (DGN_NO_ZMASK set, 0), "linear_small_min_waves" (8), "graph_bwd_tiles" (DGN_GRAPH_BWD_TILES, 0 = by batch size: feature tiles of
 * the graph backward of the sweep), "odd_direct" (DGN_ODD_DIRECT, 1: DgnMsg.f_valid in the simple whole-layer call instead of a padded copy).  dgn_set_option: DGN_ERR_INVALID for an unknown name;
 * dgn_get_option: INT64_MIN for an unknown name.                                                                            */
int dgn_set_option(const char* name, int64_t value);
int64_t dgn_get_option(const char* name);
const char* dgn_last_error(void);

/* Per-edge directional weights, once per (graph, eig): w[c*ld_w + j] for channel c, CSR slot j.
 * Either eig [n_nodes, ld_eig] (gathered through src / the row id), or -- for the reference's
 * mailbox-level function API (aggregators.py:74-93) -- eig_s_edge / eig_d_edge [n_edges, ld_eig]
 * given per slot.  Replaces the eig_s/eig_d materialisation of dgn_layer.py:155 and the
 * per-aggregator weight chains of aggregators.py:35-71.
 * ws: workspace of at least dgn_edge_weights_workspace_bytes() bytes (hub rows only).          */
size_t dgn_edge_weights_workspace_bytes(const DgnGraph* g, int32_t n_ch);
int dgn_edge_weights(const DgnGraph* g, const float* eig, const float* eig_s_edge, const float* eig_d_edge,
                     int64_t ld_eig, int32_t n_ch, const DgnChannel* ch, float* w, int64_t ld_w,
                     void* ws, size_t ws_bytes, void* stream);

/* Fused gather -> directional weighting -> multi-aggregator reduce -> degree scalers, one CSR
 * sweep.  out [n_nodes, ld_out], columns [T][S][A][F/T]; zero-in-degree rows are zeros.
 * log_deg [n_nodes] = (float)log((double)(in_degree + 1))  (scalers.py:13 evaluates np.log in
 * float64 and casts; the division by avg is done in fp32 like the reference).                  */
size_t dgn_agg_workspace_bytes(const DgnGraph* g, const DgnAggSpec* spec, int64_t F);
int dgn_agg_forward(const DgnGraph* g, const DgnAggSpec* spec, const DgnMsg* msg, const float* w, int64_t ld_w,
                    const float* log_deg, float* out, int64_t ld_out, void* ws, size_t ws_bytes, void* stream);

/* The forward / backward pair with an AUX table between them (training): one byte per (row, feature) in which the forward records
 * what the backward otherwise recomputes from the messages -- the slots of the row's first maximum / minimum and the sign of each
 * dx residual -- so that the backward gathers no source row, reads no x_dst / x_in row and still produces the same bits.
 * dgn_agg_aux_bytes() > 0 says the launch has such a table (molecule-like batches: at most three in-edges per row on average,
 * a baked-in list with max / min / dx but without std / var, at most two weight channels, even F); `aux` NULL = the plain calls.
 * Rows the 4-rows-per-wave kernels hand to the per-row routine (more than four in-edges, ...) are recomputed as before.          */
size_t dgn_agg_aux_bytes(const DgnGraph* g, const DgnAggSpec* spec, const DgnMsg* msg);
int dgn_agg_forward_aux(const DgnGraph* g, const DgnAggSpec* spec, const DgnMsg* msg, const float* w, int64_t ld_w,
                        const float* log_deg, float* out, int64_t ld_out, unsigned char* aux, void* ws, size_t ws_bytes, void* stream);
int dgn_agg_backward_aux(const DgnGraph* g, const DgnAggSpec* spec, const DgnMsg* msg, const float* w, int64_t ld_w,
                         const float* log_deg, const float* g_out, int64_t ld_gout, const unsigned char* aux, const DgnMsgGrad* grads,
                         void* ws, size_t ws_bytes, void* stream);

/* Backward of dgn_agg_forward for upstream gradient g_out [n_nodes, ld_gout].
 * Workspace: dgn_agg_backward_workspace_bytes(); with `deterministic` != 0 (needs g->csc_*) it includes the
 * [n_edges, F] staging buffer of the two-phase scatter; a smaller workspace silently selects the atomic path. */
size_t dgn_agg_backward_workspace_bytes(const DgnGraph* g, const DgnAggSpec* spec, int64_t F, int32_t deterministic);
/* extra workspace bytes of dgn_agg_backward when DgnMsg.edge_type is set (appended to the deterministic workspace) */
size_t dgn_agg_edge_table_workspace_bytes(int64_t F, int32_t n_edge_types);
int dgn_agg_backward(const DgnGraph* g, const DgnAggSpec* spec, const DgnMsg* msg, const float* w, int64_t ld_w,
                     const float* log_deg, const float* g_out, int64_t ld_gout, const DgnMsgGrad* grads,
                     void* ws, size_t ws_bytes, void* stream);

/* Degree scalers folded behind the post-aggregation Linear (they are per-row factors):
 *     y[n, t*f_out + o] = row_scale[n] * (bias[t*f_out + o] + sum_s scale[n, s] * z[t][n][s*f_out + o])
 * z is tower-major [T][N][S*f_out] (the batched GEMM output), y node-major [N, ld_y].  Replaces the scaler concat
 * of reduce_func (dgn_layer.py:170-171) + the Linear's bias + the graph-norm multiply `h * snorm_n`
 * (dgn_layer.py:121-122, :192-193, :270-271).  scale == NULL means S == 1 with factor 1; bias / row_scale may be NULL.
 * The backward writes g_z (same layout as z) from g_y and, if g_bias != NULL, ADDS the bias gradient
 * sum_n row_scale[n] * g_y[n, :] to g_bias [T*f_out] (caller zero-initialises).  The sum is formed from
 * per-workgroup partials in `ws` (dgn_scale_combine_backward_workspace_bytes(); needed only with g_bias) in a
 * fixed order -- no atomics, bitwise reproducible.  n_towers * f_out <= 4096.                               */
int dgn_scale_combine_forward(int64_t n_nodes, int32_t n_towers, int32_t n_scalers, int32_t f_out, const float* z,
                              const float* scale, const float* bias, const float* row_scale, float* y, int64_t ld_y,
                              void* stream);
size_t dgn_scale_combine_backward_workspace_bytes(int64_t n_nodes, int32_t n_towers, int32_t f_out);
/* Optional fusion with the BatchNorm tail that follows the combine (dgn_bn_tail_*): when `bn` is given, g_y is not
 * read; the upstream gradient of the combine is formed on the fly from the tail's inputs,
 *     g_y = gamma * invstd * (g' - sums[c]/N - xhat * sums[F+c]/N),   g' = g_out masked by the ReLU,  xhat = (y - mean) * invstd
 * with sums / g_gamma / g_beta from dgn_bn_tail_backward(..., g_x = NULL, sums): the [N, F] gradient between the two
 * steps is never written or re-read.                                                                        */
typedef struct DgnBnGrad {
    const float* g_out;    /* [N, ld] gradient of the tail's output                                          */
    const float* y;        /* [N, ld] the combine's output = the tail's input                                */
    int64_t ld;
    const float* gamma;    /* [F] or NULL                                                                    */
    const float* beta;     /* [F] or NULL                                                                    */
    const float* mean;     /* [F] save_mean of the forward                                                   */
    const float* invstd;   /* [F] save_invstd                                                                */
    const float* sums;     /* [2F] from dgn_bn_tail_backward                                                 */
    int32_t relu;
    const int64_t* n_valid; /* DEVICE scalar or NULL: only rows < *n_valid are the batch; the rest is padding of a batch held at a
                               fixed capacity (shape-bucketed HIP-graph replay): excluded from the statistics, zero gradient  */
} DgnBnGrad;
int dgn_scale_combine_backward(int64_t n_nodes, int32_t n_towers, int32_t n_scalers, int32_t f_out, const float* g_y,
                               int64_t ld_gy, const float* scale, const float* row_scale, float* g_z, float* g_bias,
                               void* ws, size_t ws_bytes, const DgnBnGrad* bn, void* stream);

/* Layer tail: BatchNorm1d over the node dimension, optionally followed by ReLU and the residual add
 *     y = [relu]( (x - mean) * invstd * gamma + beta ) [+ residual]          (dgn_layer.py:123-128, :194-199, :272-273)
 * training != 0: batch statistics (biased variance), running_mean / running_var updated in place with `momentum`
 * (running_var with the unbiased variance, like torch.nn.BatchNorm1d); save_mean / save_invstd [F] are written for
 * the backward.  training == 0: running statistics are used.  n_valid (DEVICE int64 scalar or NULL): rows >= *n_valid are
 * padding -- they take no part in the statistics (count = *n_valid) and get a zero input gradient in the backward -- so that a
 * batch can be held at a fixed row capacity (shape-bucketed HIP-graph replay).  1 <= F <= 1024.  All [N, F] tensors share the row
 * stride ld.  ws: dgn_bn_tail_workspace_bytes() of scratch (8-byte aligned; training / backward only) holding the
 * per-workgroup fp64 column partials, which are added in a fixed order (no atomics, bitwise reproducible).   */
size_t dgn_bn_tail_workspace_bytes(int64_t n_rows, int32_t F);
int dgn_bn_tail_forward(int64_t n_rows, int32_t F, const float* x, int64_t ld, const float* gamma, const float* beta,
                        float* running_mean, float* running_var, float momentum, float eps, int32_t training,
                        int32_t relu, const float* residual, float* y, float* save_mean, float* save_invstd, void* ws,
                        size_t ws_bytes, const int64_t* n_valid, void* stream);
/* Backward of the training-mode tail: g_x [N, F] (written), g_gamma / g_beta [F] (written; may be NULL).
 * The gradient of `residual` is g_y itself (left to the caller).  g_x == NULL skips the apply pass: only the column
 * sums are produced (`sums` [2F], may be NULL when g_x is given) for dgn_scale_combine_backward's fused form.  */
int dgn_bn_tail_backward(int64_t n_rows, int32_t F, const float* g_y, const float* x, int64_t ld, const float* gamma,
                         const float* beta, const float* save_mean, const float* save_invstd, int32_t relu, float* g_x,
                         float* g_gamma, float* g_beta, float* sums, void* ws, size_t ws_bytes, const int64_t* n_valid, void* stream);

/* Tail of an FCLayer (Linear -> activation, nets/layers.py:101-112) on the bias-free GEMM output x [N, F]:
 *     y = act(x + bias) [+ residual]        act: 0 none, 1 ReLU, 2 LeakyReLU(slope)
 * -- the towers' mixing network (LeakyReLU) with the layer's residual add (dgn_layer.py:319-324) in one pass.  Backward:
 * g_x = g_y * act'(x + bias) (written) and g_bias = sum_n g_x[n, :] (written; NULL = not wanted; fp64 per-workgroup
 * partials in `ws` of dgn_bn_tail_workspace_bytes(n_rows, F) bytes, fixed-order sum); the residual's gradient is g_y.
 * All [N, F] tensors share the row stride ld; F <= 1024 for the backward.                                           */
int dgn_bias_act_forward(int64_t n_rows, int32_t F, const float* x, int64_t ld, const float* bias, int32_t act, float slope,
                         const float* residual, float* y, void* stream);
int dgn_bias_act_backward(int64_t n_rows, int32_t F, const float* g_y, const float* x, int64_t ld, const float* bias,
                          int32_t act, float slope, float* g_x, float* g_bias, void* ws, size_t ws_bytes, void* stream);

/* ---- dropout (dgn_bn_tail.hip): F.dropout(h, p, training) at the end of DGNLayerSimple / DGNLayerComplex.forward and inside DGNTower
 * (nets/dgn_layer.py:130, :201, :275; configs HIV / PCBA / CIFAR10 ship dropout 0.3) -------------------------------------------------
 * y = keep ? x / (1 - p) : 0 over a CONTIGUOUS array; keep bits from Philox4x32-10 keyed by *seed (a DEVICE int64 scalar the caller
 * draws from its generator: capturable) and `offset`; mask: dgn_dropout_mask_bytes(n_elems) bytes, bit i of byte g = element 8 g + i,
 * what the backward re-applies: g_x = keep ? g_y / (1 - p) : 0.  The same (seed, offset) gives the same mask.  y may be x and g_x
 * may be g_y (in place).                                                                                                           */
size_t dgn_dropout_mask_bytes(int64_t n_elems);
int dgn_dropout_forward(int64_t n_elems, const float* x, float p, const int64_t* seed, uint64_t offset, float* y, unsigned char* mask,
                        void* stream);
int dgn_dropout_backward(int64_t n_elems, const float* g_y, const unsigned char* mask, float p, float* g_x, void* stream);

/* ---- tall-skinny fp32 Linear (dgn_linear.hip) ---------------------------------------------------------------------
 * The nn.Linear of the reference's pretrans / posttrans MLPs (layers.py:101-112, called from nets/dgn_layer.py:67-75
 * and :116-119) for matrices with ~1e5..1e6 rows (nodes) and k, n <= 160 columns, batched over towers:
 *   dgn_linear_forward   c[t] = a[t] . op(w[t]) (+ bias[t])    a: [n_rows, k], c: [n_rows, n], dense rows (lda == k, ldc == n)
 *                        w_is_kn == 0: w[t] is [n, k] (nn.Linear weight: c = a w^T, the forward)
 *                        w_is_kn == 1: w[t] is [k, n] (c = a w: the input gradient with a = g_out, w = weight)
 *   dgn_linear_wgrad     dw[t] = g[t]^T . x[t]                 g: [n_rows, n], x: [n_rows, k], both dense; dw: [n, k]
 *                        dbias[t] = column sums of g[t] (NULL = not wanted; needs k % 16 != 0: it is computed as the
 *                        product with an extra column of ones in x's tile padding, at no extra pass)
 * Exact fp32 (v_mfma_f32_16x16x4_f32 = an fmaf chain); the weight gradient is summed over per-wave partials in a fixed
 * order (bitwise reproducible).  dgn_linear_supported(k, n) says whether the pair is handled (even, <= 160, and for
 * the weight gradient at most 45 16x16 tiles); callers use a library GEMM otherwise.  stride_* are element offsets
 * between batch entries (towers).  `ws` of dgn_linear_wgrad_workspace_bytes(...) bytes holds the partials.           */
int dgn_linear_supported(int32_t k, int32_t n, int32_t wgrad);
int dgn_linear_forward(int64_t n_rows, int32_t k, int32_t n, int32_t batch, const float* a, int64_t lda, int64_t stride_a,
                       const float* w, int64_t ldw, int64_t stride_w, int32_t w_is_kn, const float* bias,
                       int64_t stride_bias, float* c, int64_t ldc, int64_t stride_c, void* stream);
/* The same two products with the operand a (resp. x) replaced by its BatchNorm -- ((v - mean[c]) * invstd[c]) * gamma[c] + beta[c], the
 * arithmetic of dgn_bn_tail_forward's apply pass in the same order, formed while the strips are staged: the normalised tensor is
 * never written (the towers layer: y1 = BatchNorm(y0) feeds the mixing Linear, nets/dgn_layer.py:272-273 -> :319).  batch = 1, dense
 * rows; gamma / beta may be NULL.  dgn_bn_tail_forward(..., y = NULL, ...) computes the statistics alone.                      */
int dgn_linear_forward_bn(int64_t n_rows, int32_t k, int32_t n, const float* a, const float* w, int64_t ldw, int32_t w_is_kn,
                          const float* bias, float* c, const float* bn_mean, const float* bn_invstd, const float* bn_gamma,
                          const float* bn_beta, void* stream);
int dgn_linear_wgrad_bn(int64_t n_rows, int32_t k, int32_t n, const float* g, const float* x, float* dw, int64_t lddw, float* dbias,
                        const float* bn_mean, const float* bn_invstd, const float* bn_gamma, const float* bn_beta, void* ws,
                        size_t ws_bytes, void* stream);
/* c = (g * act'(z + act_bias)) . op(w): the gradient through bias + activation (dgn_bias_act_backward's arithmetic) formed while the
 * strips of g and z ([n_rows, k] dense) are staged, then the Linear's input-gradient product; gz_out (may be NULL) receives the formed
 * operand (the Linear's weight gradient needs it: dgn_linear_wgrad / _bn, whose dbias output is then the bias gradient).
 * Replaces dgn_bias_act_backward + dgn_linear_forward(w_is_kn = 1) for LeakyReLU(Linear(.)) (mixing network, nets/dgn_layer.py:319). */
/* c = (add1 + a . op(w)) + add2: two more [n_rows, n] dense operands added in the product's epilogue (add2 may be NULL) -- the three-way
 * sum of the contributions to d h at the end of the towers layer's backward (residual, h_in of the sweep, the P|Q input gradient). */
int dgn_linear_add_supported(int32_t k, int32_t n);
int dgn_linear_forward_add(int64_t n_rows, int32_t k, int32_t n, const float* a, const float* w, int64_t ldw, int32_t w_is_kn,
                           const float* add1, const float* add2, float* c, void* stream);
/* BatchNorm -> Linear -> bias + activation (+ residual) in one pass: z_out = BatchNorm(a) w^T (the pre-activation the backward needs),
 * out = act(z_out + act_bias) + residual (dgn_bn_tail's apply, dgn_linear_forward and dgn_bias_act_forward in their arithmetic and order);
 * widths as dgn_linear_add_supported.  The tail of the towers layer: batchnorm_h -> mixing_network -> residual (nets/dgn_layer.py:272-273,
 * :318-324).                                                                                                                          */
int dgn_linear_forward_bn_act(int64_t n_rows, int32_t k, int32_t n, const float* a, const float* w, int64_t ldw, const float* bn_mean,
                              const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* act_bias, int32_t act,
                              float slope, const float* residual, float* z_out, float* out, void* stream);
/* The same two products with the pre-activation replaced by a byte mask (1/8 of its bytes): byte i of zmask describes elements 2 i and
 * 2 i + 1 of the dense [n_rows, n] pre-activation, bit 0 / bit 1 = (z + act_bias > 0).  dgn_linear_forward_bn_act_mask writes it (and
 * `out`) instead of z_out; dgn_linear_forward_act_mask takes the activation's derivative from it (1 where set, else slope for
 * LeakyReLU / 0 for ReLU): the values dgn_linear_forward_act computes from z.                                                    */
size_t dgn_linear_act_mask_bytes(int64_t n_rows, int32_t n);
int dgn_linear_forward_bn_act_mask(int64_t n_rows, int32_t k, int32_t n, const float* a, const float* w, int64_t ldw, const float* bn_mean,
                                   const float* bn_invstd, const float* bn_gamma, const float* bn_beta, const float* act_bias, int32_t act,
                                   float slope, const float* residual, unsigned char* zmask_out, float* out, void* stream);
int dgn_linear_forward_act_mask(int64_t n_rows, int32_t k, int32_t n, const float* g, const unsigned char* zmask, int32_t act, float slope,
                                const float* w, int64_t ldw, int32_t w_is_kn, float* c, float* gz_out, void* stream);
/* Round 6 -- the towers layer's mixing-network backward without the tensors between its steps (autograd through
 * nets/dgn_layer.py:272-273 BatchNorm -> :319 mixing Linear -> LeakyReLU):
 *   dgn_linear_wgrad_bn_act_mask     dw = (g * act'(mask))^T . BatchNorm(x), dbias = sum_m g * act'(mask): dgn_linear_wgrad_bn whose G
 *                                    operand is formed from the layer's output gradient g [n_rows, n] and the forward's byte mask while
 *                                    it is staged (the masked tensor g_z is never written or re-read);
 *   dgn_linear_forward_act_mask_bnb  the input-gradient product g_y1 = (g * act'(mask)) . op(w) of dgn_linear_forward_act_mask with
 *                                    BatchNorm's backward and the graph norm in its epilogue,
 *                                        gz[t][m][o] = row_scale[m] * gamma[c] invstd[c] (g_y1[m][c] - sums[c] / M - xhat[m][c] sums[n + c] / M),
 *                                        c = t f_out + o,  xhat = (y[m][c] - mean[c]) invstd[c]
 *                                    (dgn_scale_combine_backward's fused form, same arithmetic and order), written tower-major
 *                                    [n / f_out][n_rows][f_out] (stride_gz floats between towers): what dgn_linear_combine_backward_*
 *                                    read.  y [n_rows, n] is BatchNorm's input, sums [2 n] = (sum g_y1, sum g_y1 xhat) -- e.g. from the
 *                                    mixing weight gradient (csrc/dgn_towers.hip: mix_bn_finalize); g_y1 itself is never written.
 * Widths: dgn_linear_bnb_supported (k, n <= 80 and the limits of dgn_linear_act_supported / _add_supported); f_out even, n / f_out <= 15.  */
int dgn_linear_bnb_supported(int32_t k, int32_t n);
int dgn_linear_wgrad_bn_act_mask(int64_t n_rows, int32_t k, int32_t n, const float* g, const unsigned char* zmask, int32_t act, float slope,
                                 const float* x, float* dw, int64_t lddw, float* dbias, const float* bn_mean, const float* bn_invstd,
                                 const float* bn_gamma, const float* bn_beta, void* ws, size_t ws_bytes, void* stream);
int dgn_linear_forward_act_mask_bnb(int64_t n_rows, int32_t k, int32_t n, const float* g, const unsigned char* zmask, int32_t act, float slope,
                                    const float* w, int64_t ldw, int32_t w_is_kn, const float* y, const float* bn_mean, const float* bn_invstd,
                                    const float* bn_gamma, const float* sums, const float* row_scale, int32_t f_out, float* gz,
                                    int64_t stride_gz, void* stream);
int dgn_linear_act_supported(int32_t k, int32_t n);      /* (the widest tile shapes are not: two prefetched strips per wave) */
int dgn_linear_forward_act(int64_t n_rows, int32_t k, int32_t n, const float* g, const float* z, const float* act_bias, int32_t act,
                           float slope, const float* w, int64_t ldw, int32_t w_is_kn, float* c, float* gz_out, void* stream);
/* The towers' posttrans Linear with the scale-combine epilogue of dgn_scale_combine_forward in the same pass (the
 * [T, N, S*f_out] product never reaches memory):
 *   y[m, t*f_out + o] = row_scale[m] * (bias[t*f_out + o] + sum_s scale[m, s] * (a[t] w[t]^T)[m, s*f_out + o])
 * a: [T][n_rows][k] dense (stride_a between towers), w[t]: [S*f_out, k]; scale [n_rows, S] (NULL only if S == 1),
 * bias [T*f_out] / row_scale [n_rows] may be NULL.  Same width limits as dgn_linear_forward with n = S*f_out.        */
int dgn_linear_combine_forward(int64_t n_rows, int32_t k, int32_t n_towers, int32_t n_scalers, int32_t f_out, const float* a,
                               int64_t stride_a, const float* w, int64_t ldw, int64_t stride_w, const float* scale,
                               const float* bias, const float* row_scale, float* y, int64_t ld_y, void* stream);
/* Backward of dgn_linear_combine_forward without the [T, N, S*f_out] gradient in memory.  With
 *   G[t][m][s*f_out + o] = scale[m, s] * gy[t][m][o]
 * (gy [T][n_rows][f_out], stride_gy between towers = row_scale * the gradient of the combine's output in tower-major form,
 * i.e. what dgn_scale_combine_backward writes when called with ONE scaler and no scale table) the two products are formed
 * while the strips are staged:
 *   dgn_linear_combine_backward_input    g_a[t] = G[t] . w[t]        [n_rows, k]   (w[t]: [S*f_out, k])
 *   dgn_linear_combine_backward_weight   dw[t]  = G[t]^T . a[t]      [S*f_out, k]  (ws as for dgn_linear_wgrad with n = S*f_out)
 * f_out even, at most 3 scalers, widths as for dgn_linear_forward / dgn_linear_wgrad.                                */
int dgn_linear_combine_backward_input(int64_t n_rows, int32_t n_towers, int32_t n_scalers, int32_t f_out, int32_t k, const float* gy,
                                      int64_t stride_gy, const float* scale, const float* w, int64_t ldw, int64_t stride_w, float* g_a,
                                      int64_t stride_ga, void* stream);
int dgn_linear_combine_backward_weight(int64_t n_rows, int32_t n_towers, int32_t n_scalers, int32_t f_out, int32_t k, const float* gy,
                                       int64_t stride_gy, const float* scale, const float* a, int64_t stride_a, float* dw, int64_t lddw,
                                       int64_t stride_dw, void* ws, size_t ws_bytes, void* stream);
/* ... and with g_sum [T][S*f_out] (may be NULL; needs k % 16 != 0): g_sum[t][s*f_out + o] = sum_m G[t][m][s*f_out + o], the column sums of the
 * expanded gradient from a column of ones in a's padding -- for the identity scaler that is the gradient of posttrans' bias
 * (sum_m row_scale[m] g_y[m, t*f_out + o]), at no cost.                                                                          */
int dgn_linear_combine_backward_weight_bias(int64_t n_rows, int32_t n_towers, int32_t n_scalers, int32_t f_out, int32_t k, const float* gy,
                                            int64_t stride_gy, const float* scale, const float* a, int64_t stride_a, float* dw, int64_t lddw,
                                            int64_t stride_dw, float* g_sum, void* ws, size_t ws_bytes, void* stream);
size_t dgn_linear_wgrad_workspace_bytes(int64_t n_rows, int32_t k, int32_t n, int32_t batch);
int dgn_linear_wgrad(int64_t n_rows, int32_t k, int32_t n, int32_t batch, const float* g, int64_t ldg, int64_t stride_g,
                     const float* x, int64_t ldx, int64_t stride_x, float* dw, int64_t lddw, int64_t stride_dw, float* dbias,
                     int64_t stride_dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- block-diagonal pretrans Linear of the towers layer (dgn_linear_bd.hip) ---------------------------------------------
 * With divide_input every tower's pretrans MLP acts on its own f_in-column slice of h (nets/dgn_layer.py:226-231 via :309-316), so
 * the fused product pq = h [W_s | W_d]^T + [0 | b] has T diagonal blocks of [f_in, f_in] per half: 1/T of the dense
 * [2 T f_in, T f_in] matrix.  These entry points skip the structural zeros (ZINC towers: 40 instead of 180 MFMAs per 16 rows):
 *   dgn_linear_bd_forward          c [n_rows, 2 Fm] = a [n_rows, Fm] . blockdiag(w)^T (+ bias [2 Fm]),   Fm = n_towers * f_in
 *   dgn_linear_bd_backward_input   c [n_rows, Fm]   = (add1 + g [n_rows, 2 Fm] . blockdiag(w)) + add2    (add1 / add2 may be NULL)
 *   dgn_linear_bd_wgrad            dw [2 Fm, lddw]: diagonal blocks of g^T . x, ZERO elsewhere; dbias [2 Fm] = column sums of g (or NULL)
 * w is the dense [2 Fm, ldw] operand of dgn_linear_forward (row j Fm + t f_in + a, column t f_in + b; other entries are not read), so
 * the two routes are interchangeable.  Dense rows, 16-byte aligned operands.  dgn_linear_bd_supported(n_towers, f_in): the
 * instantiated shapes (five towers x even widths 10..30, + (4 | 2) x 14); callers use dgn_linear_forward / _wgrad otherwise.
 * Exact fp32 MFMA; the weight gradient is summed over per-workgroup partials in a fixed order (bitwise reproducible).        */
int dgn_linear_bd_supported(int32_t n_towers, int32_t f_in);
int dgn_linear_bd_forward(int64_t n_rows, int32_t n_towers, int32_t f_in, const float* a, const float* w, int64_t ldw,
                          const float* bias, float* c, void* stream);
int dgn_linear_bd_backward_input(int64_t n_rows, int32_t n_towers, int32_t f_in, const float* g, const float* w, int64_t ldw,
                                 const float* add1, const float* add2, float* c, void* stream);
size_t dgn_linear_bd_wgrad_workspace_bytes(int64_t n_rows, int32_t n_towers, int32_t f_in);
int dgn_linear_bd_wgrad(int64_t n_rows, int32_t n_towers, int32_t f_in, const float* g, const float* x, float* dw, int64_t lddw,
                        float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- wide tall-skinny fp32 GEMMs (dgn_gemm.hip) -----------------------------------------------------------------------
 * The same nn.Linear (layers.py:101-112) for the widths the simple / complex layers' posttrans has after scaler folding
 * (nets/dgn_layer.py:148,187-190 and :69,116-119): k = aggregators x features up to a few hundred, n = scalers x f_out, any
 * parity (hidden 75 / 65), any row stride >= the row.  Exact fp32 MFMA, shape independent (no library solution selection).
 *   dgn_gemm_forward   c = a . op(w) (+ bias)      a [n_rows, k], c [n_rows, n]; w_is_kn == 0: w [n, k] (forward),
 *                                                   w_is_kn == 1: w [k, n] (input gradient: a = g_out, w = weight)
 *   dgn_gemm_wgrad     dw [n, k] = g^T . x           g [n_rows, n], x [n_rows, k]; dbias [n] = column sums of g (NULL = not wanted:
 *                                                   it rides as a column of ones appended to x, no extra pass); per-workgroup partials
 *                                                   in ws (dgn_gemm_wgrad_workspace_bytes), fixed-order sum: bitwise reproducible.
 *                                                   From 4096 rows on (and always for n > 256 or with dbias): the tile kernel --
 *                                                   v_mfma_f32_32x32x2_f32, a block of up to 256 x 256 outputs held in one workgroup's
 *                                                   registers, every operand element read from memory once per k block */
int dgn_gemm_supported(int32_t k, int32_t n);
int dgn_gemm_forward(int64_t n_rows, int32_t k, int32_t n, const float* a, int64_t lda, const float* w, int64_t ldw, int32_t w_is_kn,
                     const float* bias, float* c, int64_t ldc, void* stream);
size_t dgn_gemm_wgrad_workspace_bytes(int64_t n_rows, int32_t k, int32_t n);
int dgn_gemm_wgrad(int64_t n_rows, int32_t k, int32_t n, const float* g, int64_t ldg, const float* x, int64_t ldx, float* dw,
                   int64_t lddw, float* dbias, void* ws, size_t ws_bytes, void* stream);

/* ---- the posttrans product inside the sweep (dgn_fused.hip) -----------------------------------------------------------
 * dgn_agg_forward + dgn_linear_combine_forward as ONE kernel: the aggregate rows ([T][A][F/T] per node: 1 680 bytes on the
 * ZINC towers config, 0.46 GB per pass) stay in LDS, are multiplied there by the posttrans weights (w[t]: [S*f_out, K],
 * K = agg_total * F/T, exact fp32 MFMA) and leave as
 *     y[i, t*f_out + o] = row_scale[i] * (bias[t*f_out + o] + sum_s scale[i, s] * (agg[t][i] w[t]^T)[s*f_out + o])
 * -- reduce_func's row feeding posttrans (nets/dgn_layer.py:237-249 -> :266-271) without the [N, A*F] tensor in between.
 * Domain (dgn_layer_fused_supported): spec with ONE identity scaler (scalers folded behind posttrans) and an aggregator list of
 * the reference's configs, even F <= 128 and F/T, K <= 96 (a multiple of 4), n_towers * ceil(S*f_out / 16) <= 16, graphs without
 * hub rows whose rows fit one slot batch (batched molecules / superpixel graphs), no bipartite CSR.                   */
int dgn_layer_fused_supported(const DgnGraph* g, const DgnAggSpec* spec, int64_t F, int32_t n_scalers, int32_t f_out);
int dgn_layer_fused_forward(const DgnGraph* g, const DgnAggSpec* spec, const DgnMsg* msg, const float* w, int64_t ld_w,
                            const float* log_deg, const float* weight, int64_t ldw, int64_t stride_w, int32_t n_scalers,
                            int32_t f_out, const float* scale, const float* bias, const float* row_scale, float* y, int64_t ld_y,
                            void* stream);
/* ---- graph batch preparation on the device (dgn_graph_build.hip) ------------------------------------------------------
 * The edge list of a (batched) graph in edge-id order -> the DgnGraph arrays, by a handful of kernels on `stream`, no host
 * synchronisation inside.  Replaces what DGL does per update_all call (degree bucketing, nets/dgn_layer.py:115,186,264) and
 * the ~40 torch ops of the Python build; `dgl.batch` (data/molecules.py:229) is where a caller invokes it ONCE per
 * dataset: dgn_amd/data.py builds the packed dataset's CSR with it, and dgn_collate (below) cuts every batch out of that.
 *   dgn_graph_build          indptr [N+1], src_csr / dst_csr [E] (source / destination of every CSR slot; slots of a row in
 *                            ascending edge id), eid [E] (slot -> edge id), log_deg [N], in_degree [N] (int64, may be NULL),
 *                            stats[0] = largest in-degree, stats[1] = rows with more than hub_threshold in-edges
 *   dgn_graph_build_csc      csc_ptr [N+1], csc_pos [E], csc_order [E] (rank -> slot) of DgnGraph's transposed view
 * src / dst are int64 (what torch / DGL hand over); all outputs are caller-allocated device arrays; stats is int32[4] on the
 * device (the caller reads it when it needs the numbers); ws: dgn_graph_build_workspace_bytes() bytes for every call.    */
size_t dgn_graph_build_workspace_bytes(int64_t n_nodes, int64_t n_edges);
int dgn_graph_build(int64_t n_nodes, int64_t n_edges, const int64_t* src, const int64_t* dst, int32_t* indptr, int32_t* src_csr,
                    int32_t* dst_csr, int64_t* eid, float* log_deg, int64_t* in_degree, int32_t* stats, int32_t hub_threshold,
                    void* ws, size_t ws_bytes, void* stream);
/* Closed cuts of a batch (DgnGraph.blk_cut / blk_gap above): blk_cut [n_nodes+1], gap_out a DEVICE int32 (the caller reads it back).
 * dst_csr [n_edges] = destination of every CSR slot (dgn_graph_build's output).  Workspace: dgn_graph_build_workspace_bytes().  */
int dgn_graph_build_cuts(int64_t n_nodes, int64_t n_edges, const int32_t* src_csr, const int32_t* dst_csr, int32_t* blk_cut,
                         int32_t* gap_out, void* ws, size_t ws_bytes, void* stream);
int dgn_graph_build_csc(int64_t n_nodes, int64_t n_edges, const int32_t* src_csr, int32_t* csc_ptr, int32_t* csc_pos,
                        int32_t* csc_order, void* ws, size_t ws_bytes, void* stream);


/* ---- whole towers layer in one call (dgn_towers.hip) ------------------------------------------------------------------
 * DGNLayerTower.forward of the reference (nets/dgn_layer.py:309-325 over DGNTower.forward :254-276) for the fused form the
 * host side already uses (dgn_amd/dgn_layer.py::_fused_towers): single-affine pretrans / posttrans, divide_input, scalers
 * folded behind posttrans, training-mode BatchNorm, mixing network + residual, no edge features, no dropout:
 *     pq   = h [W_s | W_d]^T + [0 | b]                    dgn_linear_forward
 *     aggx = sweep(pq, h)  tower-major [T][N][K]           dgn_agg_forward        (spec: the towers, ONE identity scaler,
 *                                                                                  aggregators incl. the h_in block)
 *     y0   = snorm * (b_post + sum_s scale_s * (aggx W_s^T))   dgn_linear_combine_forward
 *     y1   = BatchNorm(y0)                                  dgn_bn_tail_forward (training; running stats updated in place)
 *     z    = y1 W_mix^T ;  out = LeakyReLU(z + b_mix) [+ h]  dgn_linear_forward, dgn_bias_act_forward
 * One call enqueues all of it on `stream`; dgn_towers_layer_backward enqueues the whole backward.  pq, aggx, y0, y1, z,
 * save_mean, save_invstd are written by the forward and read by the backward (caller-owned: the autograd-saved tensors).
 * Shapes: h [N, T*f_in]; w_sd [2 T f_in, T f_in]; w_post [T][S*f_out][K], K = agg_total * f_in; w_mix [T f_out, T f_out].
 * dgn_towers_layer_supported() says whether the widths fit the streaming Linear kernels.                            */
typedef struct DgnTowersLayer {
    const DgnGraph* graph;
    const DgnAggSpec* spec;
    const float* w;            /* edge weights [n_ch][ld_w] (dgn_edge_weights), or NULL                     */
    int64_t ld_w;
    const float* log_deg;
    int32_t n_towers, f_in, f_out, n_scalers;
    int32_t residual;          /* add h to the output (in_dim == out_dim and the layer's residual flag)     */
    float momentum, eps, slope;
    const float* h;            /* [N, T*f_in]                                                               */
    const float* snorm;        /* [N] graph-norm factor or NULL                                             */
    const float* scale;        /* [N, S] degree-scaler table (NULL iff S == 1)                              */
    const float* w_sd;  const float* bias_sd;
    const float* w_post; const float* b_post;
    const float* bn_gamma; const float* bn_beta;
    float* running_mean; float* running_var;
    const float* w_mix; const float* b_mix;
    float* pq; float* aggx; float* y0; float* save_mean; float* save_invstd; float* y1; float* z;
    float* out;                /* [N, T*f_out]  (forward only)                                              */
    void* ws; size_t ws_bytes; /* scratch: dgn_towers_layer_{forward,backward}_workspace_bytes()            */
    const int64_t* n_valid;    /* DEVICE scalar or NULL: rows >= *n_valid are padding (see dgn_bn_tail_forward)         */
    /* Optional (dgn_towers_layer_zmask_supported): dgn_linear_act_mask_bytes(N, T*f_out) bytes.  When set, the mixing network's
     * pre-activation is never written: the forward leaves the sign mask of (z + b_mix) here, the backward reads the activation's
     * derivative from it (same values bit for bit), and `z` may be NULL.                                                      */
    unsigned char* zmask;
    /* Optional: dgn_agg_aux_bytes(graph, spec, the sweep's message) bytes -- the forward sweep leaves its aux table here, the
     * backward sweep works from it (dgn_agg_forward_aux / dgn_agg_backward_aux).  NULL: the backward recomputes.                */
    unsigned char* agg_aux;
    /* Optional: the towers' F.dropout(h, p, training) between BatchNorm and the mixing network (nets/dgn_layer.py:275).  drop_p > 0
     * needs y1 (the normalised rows are then materialised: the mask is applied to them in place, the mixing Linear and its weight
     * gradient read the dropped rows), drop_seed / drop_offset as dgn_dropout_forward takes them (forward only), and drop_mask of
     * dgn_dropout_mask_bytes(N * T * f_out) bytes (written by the forward, read by the backward); zmask must be NULL.                */
    float drop_p;
    const int64_t* drop_seed;
    uint64_t drop_offset;
    unsigned char* drop_mask;
    /* Round 6 (ABI 26): 1 + the index of the IDENTITY scaler among the n_scalers (its block of w_post carries the h columns,
     * dgn_amd/dgn_layer.py::_assemble); 0 (a zero-initialised struct): unknown -- the separate passes run.  With it the backward takes
     * posttrans' bias gradient from the weight-gradient pass (dgn_linear_combine_backward_weight_bias) and BatchNorm's backward rides in
     * the mixing network's input-gradient product (dgn_linear_forward_act_mask_bnb).                                                */
    int32_t id_slot1;
    /* Round 6 (ABI 28): the BatchNorm modules' num_batches_tracked counters (n_nbt of them, DEVICE memory; torch's
     * `num_batches_tracked += 1` of a training-mode forward, torch/nn/modules/batchnorm.py) -- each is incremented by the forward's
     * statistics kernel instead of by a launch of the caller's.  NULL / 0: not touched.                                            */
    int64_t* num_batches_tracked;
    int32_t n_nbt;
} DgnTowersLayer;
typedef struct DgnTowersGrads {
    const float* g_out;        /* [N, T*f_out]                                                              */
    float* g_h;                /* [N, T*f_in]   written                                                     */
    float* g_w_sd; float* g_bias_sd; float* g_w_post; float* g_b_post; float* g_gamma; float* g_beta; float* g_w_mix; float* g_b_mix;
} DgnTowersGrads;
/* The fused operand buffer from the per-tower parameters (the reference's state_dict layout, nets/dgn_layer.py:205-276 x towers) in ONE
 * launch: out[i] = ((const float*)param_ptrs[map_param[i]])[map_off[i]], or 0 where map_param[i] < 0.  param_ptrs is a DEVICE array of
 * device addresses (int64), the maps are device int32 arrays built once per layer (dgn_amd/dgn_layer.py::_operands).          */
int dgn_assemble_params(int64_t n_out, const int64_t* param_ptrs, const int32_t* map_param, const int32_t* map_off, float* out, void* stream);

/* ---- the simple / complex layers as ONE call per direction (dgn_layers.hip) --------------------------------------------------
 * DGNLayerSimple.forward (nets/dgn_layer.py:178-202) and DGNLayerComplex.forward (:103-132) in the fused form of
 * dgn_amd/dgn_layer.py: single-affine pretrans / posttrans, the degree scalers folded behind the posttrans Linear, training-mode
 * BatchNorm -> ReLU -> residual, no edge features, no dropout:
 *     hp   = h with a zero column appended when f_in is odd (hidden 75 / 65 / 45 / 47: 8-byte lanes + two-phase scatter in the sweep)
 *     pq   = hp [W_s | W_d]^T + [0 | b]                     complex only (pretrans on [h_src || h_dst], decomposed)
 *     agg  = sweep(hp | pq)  [N, K],  K = (n_agg (+ 1: the h_in block, complex)) * f_pad
 *     y    = snorm * (b_post + sum_s scale_s * (agg W_f^T)_s)   W_f = the posttrans weight folded scaler-major, zero columns at the padding
 *     out  = relu(BatchNorm(y)) [+ h]
 * Parameters keep the REFERENCE's layout (w_post [f_out, (complex: f_in +) S * n_agg * f_in], w_pre [f_in, 2 f_in]); the folds, the
 * padding and their adjoints are kernels of the call.  hp, pq, agg, y, wf, wsd, save_mean, save_invstd are written by the forward and
 * read by the backward (caller-owned: the autograd-saved tensors): hp [N, f_pad] (used only when f_in is odd), pq [N, 2 f_pad],
 * agg [N, K], y [N, f_out], wf [2 * S f_out * K] (W_f and its transpose), wsd [4 f_pad^2 + 2 f_pad] (complex: W_sd, its transpose,
 * bias_sd).  spec: the sweep's list (aggregators, + DGN_AGG_X_IN last for the complex layer) with ONE identity scaler, one tower.   */
/* ---- degree classes: the posttrans product with its degree scalers at 1 / S of the folded product's flops -------------------------
 * Every scaler of nets/scalers.py:7-18 multiplies a node's whole aggregate row by a function of its IN-DEGREE, so all nodes of one
 * in-degree d share y = agg (sum_s scale_s(d) W_f[s])^T: one product with f_out columns instead of S f_out (dgn_dc_kernels.hpp).
 * The kernels walk a virtual row space: nodes stably sorted by class = in-degree (0 .. DGN_DC_CLASSES - 1; graphs with larger
 * in-degrees keep the folded route), each class padded to a multiple of DGN_DC_UNIT rows.                                          */
#define DGN_DC_CLASSES 32
#define DGN_DC_UNIT 64
typedef struct DgnDegreeClasses {
    int64_t n_units;              /* units (DGN_DC_UNIT rows) of the virtual row space                                  */
    const int32_t* vperm;         /* [DGN_DC_UNIT * n_units] node of a virtual row, -1: padding                          */
    const int32_t* unit_class;    /* [n_units] class of a unit, -1: empty.  INVARIANT (not checked on the device): every class
                                   * lies in [0, DGN_DC_CLASSES) and the classes ASCEND along the units -- dgn_dc_wgrad keys its partial
                                   * blocks on (workgroup + class) and a 32-bit class mask, which alias otherwise.  DGNGraph.degree_classes()
                                   * (dgn_amd/graph.py) builds it from a stable sort by in-degree and refuses in-degrees >= DGN_DC_CLASSES. */
    const int32_t* present;       /* [DGN_DC_CLASSES] rows per class                                                     */
    const float* scale;           /* [DGN_DC_CLASSES, S] the layer's scaler factors per class (set per layer)            */
} DgnDegreeClasses;
/* Optional: the posttrans weight (and its gradient) in the reference's OWN layout, nn.Linear [f_out, (h_off +) S n_agg f_in], instead of
 * the scaler-major folded matrix wf [S f_out, k]: column kk = a f_pad + f of the product reads W[o][h_off + (s n_agg + a) f_in + f]; the
 * complex layer's h block (a == n_agg; h_off = f_in) reads W[o][f] through the identity scaler's slot; padded columns f >= f_in are 0.   */
typedef struct DgnDcLayout {
    int32_t n_agg, f_pad, f_in, h_off, id_slot;
    int64_t ld;
} DgnDcLayout;
int dgn_dc_supported(int32_t k, int32_t n);
int dgn_dc_wgrad_supported(int32_t k, int32_t n);
/* wc[c][t][o][kk] = sum_s scale[c][s] wf[t][s n + o][kk] and wct[c][t][kk][o] (its transpose), classes present only;
 * wf [towers][S n, k], wc / wct [DGN_DC_CLASSES][towers][n k]                                                                       */
int dgn_dc_fold(const DgnDegreeClasses* d, int32_t S, int32_t n, int32_t k, int32_t towers, const float* wf, const DgnDcLayout* layout /* NULL: wf as above */,
                float* wc, float* wct, void* stream);
/* c[node] = row_scale[node] * (bias + a[node] w_class(node)^T) for every tower t (element offsets t * a_tower / w_tower / c_tower, bias
 * t * n); w: class c at w + c * class_stride, [n, k] rows of stride ldw                                                             */
int dgn_dc_gemm(const DgnDegreeClasses* d, int32_t k, int32_t n, int32_t towers, const float* a, int64_t lda, int64_t a_tower, const float* w,
                int64_t ldw, int64_t class_stride, int64_t w_tower, const float* bias, const float* row_scale, float* c, int64_t ldc,
                int64_t c_tower, int32_t stream_out, void* stream);
/* g_wf[s n + o][kk] = sum_nodes scale[class(node)][s] g[node][o] x[node][kk]  (per-class products, fixed-order finalize)             */
size_t dgn_dc_wgrad_workspace_bytes(int64_t n_units, int32_t k, int32_t n);
int dgn_dc_wgrad(const DgnDegreeClasses* d, int32_t S, int32_t k, int32_t n, const float* g, int64_t ldg, const float* x, int64_t ldx,
                 float* g_wf, int64_t ldw, const DgnDcLayout* layout /* NULL, or: g_wf is the reference-layout gradient [n, layout->ld] */, void* ws,
                 size_t ws_bytes, void* stream);

typedef struct DgnDenseLayer {
    const DgnGraph* graph;
    const DgnAggSpec* spec;
    const float* w;            /* edge weights [n_ch][ld_w] (dgn_edge_weights), or NULL                      */
    int64_t ld_w;
    const float* log_deg;
    int32_t type;              /* 0 = simple, 1 = complex                                                    */
    int32_t f_in, f_out, n_scalers, n_agg;
    int32_t id_slot;           /* complex: position of the identity scaler among the applied ones           */
    int32_t residual;
    float momentum, eps;
    const float* h;            /* [N, f_in]                                                                  */
    const float* snorm;        /* [N] graph-norm factor or NULL                                              */
    const float* scale;        /* [N, S] degree-scaler table (NULL iff S == 1)                               */
    const float* w_pre;  const float* b_pre;     /* complex: pretrans Linear (bias may be NULL)              */
    const float* w_post; const float* b_post;    /* posttrans Linear (bias may be NULL)                      */
    const float* bn_gamma; const float* bn_beta;
    float* running_mean; float* running_var;
    float* hp; float* pq; float* agg; float* y; float* wf; float* wsd; float* save_mean; float* save_invstd;
    float* out;                /* [N, f_out]  (forward only)                                                 */
    void* ws; size_t ws_bytes;
    const int64_t* n_valid;    /* DEVICE scalar or NULL (padded batches, see dgn_bn_tail_forward)            */
    unsigned char* agg_aux;    /* optional: dgn_dense_layer_agg_aux_bytes() bytes, the sweep's aux table (dgn_agg_forward_aux) */
    const DgnDegreeClasses* dc; /* optional (S > 1, f_out <= 128): degree-class posttrans; wf then holds (2 S + 2 DGN_DC_CLASSES) f_out K floats */
    int64_t* num_batches_tracked; /* ABI 28: the BatchNorm module's counter (DEVICE; see DgnTowersLayer), incremented by the forward; NULL: not touched */
} DgnDenseLayer;
typedef struct DgnDenseGrads {
    const float* g_out;        /* [N, f_out]                                                                 */
    float* g_h;                /* [N, f_in]  (written; includes the residual's share)                        */
    float* g_w_pre; float* g_b_pre; float* g_w_post; float* g_b_post; float* g_gamma; float* g_beta;   /* written */
} DgnDenseGrads;
int dgn_dense_layer_supported(int32_t type, int32_t f_in, int32_t f_out, int32_t n_scalers, int32_t n_agg);
size_t dgn_dense_layer_agg_aux_bytes(const DgnDenseLayer* L);      /* graph, spec, type and widths set; 0: no aux table */
size_t dgn_dense_layer_forward_workspace_bytes(const DgnDenseLayer* layer);
int dgn_dense_layer_forward(const DgnDenseLayer* layer, void* stream);
size_t dgn_dense_layer_backward_workspace_bytes(const DgnDenseLayer* layer);
int dgn_dense_layer_backward(const DgnDenseLayer* layer, const DgnDenseGrads* grads, void* stream);

int dgn_towers_layer_supported(int32_t n_towers, int32_t f_in, int32_t f_out, int32_t n_scalers, int32_t n_agg_total);
/* 1 when dgn_towers_layer_forward / _backward can work from DgnTowersLayer.zmask alone (the fused mixing-network kernels exist for
 * T * f_out columns and are not switched off): the caller then need not allocate `z`.                                            */
int dgn_towers_layer_zmask_supported(int32_t n_towers, int32_t f_out);
/* bytes of DgnTowersLayer.agg_aux for this layer (graph, spec and widths set; 0: the sweep has no aux table)                    */
size_t dgn_towers_layer_agg_aux_bytes(const DgnTowersLayer* L);
size_t dgn_towers_layer_forward_workspace_bytes(const DgnTowersLayer* layer);
int dgn_towers_layer_forward(const DgnTowersLayer* layer, void* stream);
size_t dgn_towers_layer_backward_workspace_bytes(const DgnTowersLayer* layer);
int dgn_towers_layer_backward(const DgnTowersLayer* layer, const DgnTowersGrads* grads, void* stream);

/* ---- the layer of a batch at the reference's own batch size as FIVE launches per step (dgn_blk_layer.hip) ---------------------------
 * Every shipped config trains at batch 128 (configs/molecules_graph_regression_DGN_ZINC.json:12, superpixels_graph_classification_DGN_
 * CIFAR10.json:12; the hot loop of main_molecules.py / train/train_molecules_graph_regression.py:13-45): 3 000 - 15 000 rows, where a
 * layer through the streaming kernels above is ~28 launches of a few microseconds each.  A dgl.batch (data/molecules.py:229) is block
 * diagonal: a workgroup that owns whole graphs runs the layer for them out of LDS.  Replaces, for one DGNLayer{Simple,Complex,Tower}
 * .forward + autograd backward (nets/dgn_layer.py:178-202, :103-132, :254-276 + :309-325) in training mode:
 *     forward   blk_forward  (a workgroup per block): edge weights from eig (nets/aggregators.py:35-71) -> pretrans as P[src] + Q[dst]
 *               -> aggregators -> scalers -> posttrans -> graph norm = y0, BatchNorm partial sums
 *               blk_tail_fwd (16 rows per wave): BatchNorm (training statistics, running statistics and num_batches_tracked updated)
 *               -> ReLU -> + h (simple / complex)   or   -> mixing Linear -> LeakyReLU -> + h (towers)
 *     backward  blk_tail_bwd, blk_backward (recomputes the block's forward in LDS: only y0, mean, invstd were saved), blk_reduce
 * Parameters and their gradients keep the REFERENCE's state_dict layout, one tensor per tower (no fold / assembly launches):
 *     w_pre[t] [f_in, 2 f_in], b_pre[t] [f_in]  (complex / towers; no edge features on this route)
 *     w_post[t] [f_out, (complex / towers: f_in +) S * n_agg * f_in], b_post[t] [f_out];  gamma[t], beta[t] [f_out]
 *     w_mix [T f_out, T f_out], b_mix [T f_out]  (towers)
 * simple / complex: n_towers = 1, f_in = the hidden size.  No dropout, no padded batches, at most 3 edge-weight channels.           */
#define DGN_BLK_MAX_TOWERS 8
typedef struct DgnBlockTable {
    int32_t n_blocks;
    int32_t max_rows;        /* largest block: rows ...                                                                       */
    int32_t max_edges;       /* ... and CSR slots                                                                             */
    /* DEVICE [n_blocks][4] int32 (16-byte aligned): first row, end row, first CSR slot, end CSR slot.  The blocks partition [0, N) in
     * order and are CLOSED: every edge of a block's rows starts inside the block (whole graphs of the batch).                      */
    const int32_t* desc;
} DgnBlockTable;
typedef struct DgnBlockLayer {
    const DgnGraph* graph;       /* indptr, src; the backward also csc_ptr / csc_pos                                          */
    const DgnBlockTable* blocks;
    const DgnAggSpec* spec;      /* aggregators (no DGN_AGG_X_IN), n_ch, the APPLIED scalers (dgn_layer.py:170), avg_log, eps       */
    const DgnChannel* channels;  /* HOST array [spec->n_ch]: how eig becomes each weight channel                              */
    const float* eig; int64_t ld_eig; int32_t n_eig_cols;      /* [N, ld_eig] node eigenvectors (g.ndata['eig'])               */
    const float* log_deg;        /* [N] log(in-degree + 1) as the scalers use it (nets/scalers.py:11,16)                       */
    int32_t type;                /* 0 simple, 1 complex, 2 towers (n_towers >= 2, divide_input)                               */
    int32_t n_towers, f_in, f_out;      /* per tower                                                                          */
    int32_t residual;
    float momentum, eps, slope;  /* BatchNorm momentum / eps; LeakyReLU slope of the mixing network                           */
    const float* h;              /* [N, T f_in]                                                                               */
    const float* snorm;          /* [N] graph-norm factors, NULL: graph_norm off                                              */
    const float* const* w_pre; const float* const* b_pre; const float* const* w_post; const float* const* b_post;      /* HOST arrays of T device pointers */
    const float* const* gamma; const float* const* beta;
    const float* w_mix; const float* b_mix;
    float* running_mean; float* running_var;      /* [T f_out] (the towers' statistics behind each other), updated in place     */
    int64_t* num_batches_tracked; int32_t n_nbt;  /* n_nbt counters (one per BatchNorm module), each incremented; may be NULL   */
    float* y0; float* save_mean; float* save_invstd;      /* [N, T f_out], [T f_out] x 2: written by the forward, read by the backward */
    float* out;                  /* [N, T f_out] (forward)                                                                    */
    void* ws; size_t ws_bytes;   /* dgn_block_layer_{forward,backward}_workspace_bytes()                                      */
    /* Padded batches (a captured step replayed over batches of different sizes: the buffers hold N = graph->n_nodes rows of which the
     * first *n_valid are the batch): n_valid = DEVICE int64 scalar, NULL = every row is real.  BatchNorm counts *n_valid rows; out and
     * g_h rows from *n_valid on are written as zeros.  The block table then changes per batch inside static buffers: entries with
     * first row == end row are unused, negative slot fields are read from graph->indptr, and blocks->max_rows / max_edges are the
     * CAPACITY the LDS plan is made for -- a block beyond it is skipped and *overflow (DEVICE int32, may be NULL) set to 1.          */
    const int64_t* n_valid; int32_t* overflow;
    /* eval_mode = 1 (dgn_block_layer_forward only): the layer in evaluation mode -- BatchNorm with the RUNNING statistics, which are
     * read and not updated; num_batches_tracked, save_mean / save_invstd are not touched (may be NULL); y0 is still the hand-over
     * buffer between the two launches.  nn.Module.eval() + torch.no_grad() of the reference's evaluation loops
     * (train/train_molecules_graph_regression.py:47-66).                                                                         */
    int32_t eval_mode;
    float* dbg_agg; float* dbg_gagg;      /* tests only: [N, T n_agg f_in] aggregate rows (forward) / their gradients (backward); NULL */
    int64_t* dbg_time;           /* profiling only: [n_blocks][16] wall-clock stamps (100 MHz) of the block kernel's phases; NULL      */
    /* Round 6 (ABI 27): F.dropout(h, p, training) inside the tail kernels -- towers (type 2): between the towers' BatchNorm and the mixing
     * network (nets/dgn_layer.py:275); simple / complex (types 0 / 1; ABI 28's library, same fields): the layer's LAST op, on the finished
     * output rows (:130, :201; the backward masks the output gradient, the residual's share of d h included).  drop_p in (0, 1): drop_seed (DEVICE int64 key; forward only) / drop_offset as dgn_dropout_forward takes
     * them, drop_mask = dgn_dropout_mask_bytes(N * T * f_out) bytes, written by the forward (the very bits dgn_dropout_forward would
     * draw for the dense [N, T f_out] tensor) and read by the backward.  drop_p = 0: none.  Ignored in eval_mode.                   */
    float drop_p; const int64_t* drop_seed; uint64_t drop_offset; unsigned char* drop_mask;
} DgnBlockLayer;
typedef struct DgnBlockGrads {
    const float* g_out;          /* [N, T f_out]                                                                              */
    float* g_h;                  /* [N, T f_in] written (includes the residual's share)                                       */
    /* dgn_block_layer_param_grad_floats() floats, written: per tower [w_pre | b_pre] (complex / towers) [w_post | b_post], then
     * (towers) [w_mix | b_mix] -- each in the parameter's own layout                                                          */
    float* g_params;
    float* g_gamma; float* g_beta;      /* [T f_out] each                                                                     */
} DgnBlockGrads;
int dgn_block_layer_supported(const DgnBlockLayer* layer);      /* graph, blocks, spec, type and widths set: 1 if every block fits */
int64_t dgn_block_layer_param_grad_floats(const DgnBlockLayer* layer);
size_t dgn_block_layer_forward_workspace_bytes(const DgnBlockLayer* layer);
int dgn_block_layer_forward(const DgnBlockLayer* layer, void* stream);
size_t dgn_block_layer_backward_workspace_bytes(const DgnBlockLayer* layer);
int dgn_block_layer_backward(const DgnBlockLayer* layer, const DgnBlockGrads* grads, void* stream);

/* ---- node classification: balanced cross-entropy + the SBM confusion matrix (dgn_node_ce.hip) ------------------------------------
 * Replaces DGNNet.loss of nets/SBMs_node_classification/dgn_net.py:67-81 (bincount -> nonzero -> unique -> indexed assignment ->
 * CrossEntropyLoss(weight): ~20 launches and two device-to-host read-backs) and the prediction + confusion_matrix of accuracy_SBM
 * (train/metrics.py:37-40, a host-side scikit-learn call per batch) by three launches on the caller's stream with nothing read back.
 * scores [N, C] fp32 (row stride ld), labels [N] int64, 1 <= C <= 32, N < 2^31.  A label < 0 marks a row that does not exist
 * (padding of a captured batch): it counts nowhere and its gradient row is zero; a label >= C is treated the same way (no access
 * outside the tables).  V = number of valid rows, count[c] = valid rows labelled c:
 *     weight[c]   = count[c] > 0 ? float(V - count[c]) / float(V) : 0                                   (dgn_net.py:74-75)
 *     loss        = sum_n weight[y_n] (logsumexp_c scores[n, :] - scores[n, y_n]) / sum_c weight[c] count[c]   (:78-79, mean reduction)
 *     g_scores    = d loss / d scores  [N, C] (row stride ld_g), written in the pass that forms the loss terms; NULL: not wanted
 *     confusion   = [C, C] int64, rows = label, columns = argmax_c (scores[n, c] - logsumexp_{n' valid} scores[n', c]) -- the log form
 *                   of metrics.py:39's Softmax(dim=0) (over the NODES) then argmax(axis=1), first maximum on ties; NULL: not wanted
 * loss: DEVICE float, weight: DEVICE [C] or NULL.  With one class among the valid labels every weight is 0 and loss and the valid rows'
 * gradients are nan (0 / 0), as the reference's; V == 0 (the reference raises): loss 0, gradients 0; n_rows == 0: loss 0.
 * Reductions run in a fixed order without floating-point atomics: the same input gives the same bits.  ws: 8-byte aligned,
 * dgn_node_ce_workspace_bytes(n_rows, n_classes) bytes (0 for arguments out of range).
 * dgn_node_ce_backward: the autograd backward, ONE launch: g_scores[n, c] = g_saved[n, c] * *g_loss (g_loss: DEVICE float, the
 * incoming gradient of the scalar loss; g_saved: what the forward wrote).                                                          */
size_t dgn_node_ce_workspace_bytes(int64_t n_rows, int32_t n_classes);
int dgn_node_ce_forward(int64_t n_rows, int32_t n_classes, const float* scores, int64_t ld, const int64_t* labels, float* loss,
                        float* weight, float* g_scores, int64_t ld_g, int64_t* confusion, void* ws, size_t ws_bytes, void* stream);
int dgn_node_ce_backward(int64_t n_rows, int32_t n_classes, const float* g_saved, int64_t ld_g, const float* g_loss, float* g_scores,
                         int64_t ld_out, void* stream);

/* ---- OGB molecule nets: multi-column embedding sum + masked BCE with logits (dgn_mol_io.hip) ----------------------------------------
 * Multi-column embedding sum.  Replaces ogb's AtomEncoder / BondEncoder as the nets call them (nets/HIV_graph_classification/
 * dgn_net.py:41-44, :62, :68; nets/PCBA_graph_classification/dgn_net.py:36-39, :67, :70): C nn.Embedding lookups and C - 1 adds forward,
 * C sort-based embedding_dense_backward passes backward.  idx [N, C] int64 (row stride ld_idx, unit column stride), 1 <= C <=
 * DGN_MULTI_EMBEDDING_MAX_COLS; tables / g_tables: HOST arrays of C DEVICE pointers to fp32 [dims[c], F] dense tables (read at the call:
 * they travel in the kernel arguments), dims: HOST array.  N < 2^31.  An index outside [0, dims[c]) is CLAMPED into the table.
 *     forward   out[n, :] = ((0 + T_0[idx[n, 0]]) + T_1[idx[n, 1]]) + ...   plain fp32 adds in column order: bit-equal to the torch loop;
 *               one launch; 8- / 16-byte accesses where F, the row stride and the pointers allow them; any C <= 16 and F
 *     backward  g_tables[c][r, :] = sum_{n: idx[n, c] = r} g[n, :]  for all C tables in one pass over g, every element written (rows
 *               without a hit: 0); two launches: per-workgroup partial tables in LDS over contiguous row ranges (a column's adds in row
 *               order), then the partials added in workgroup order in fp64.  No floating-point atomics: the same input gives the same bits.
 *               Needs sum(dims) * F floats of LDS: dgn_multi_embedding_supported says whether the shape fits (callers take another route
 *               otherwise); ws: dgn_multi_embedding_backward_workspace_bytes bytes (0 for unsupported arguments).
 * Masked BCE with logits.  Replaces the boolean-index selection in front of the loss and the loss itself (train/
 * train_PCBA_graph_classification.py:32-33 + nets/PCBA_graph_classification/dgn_net.py:99-102; nets/HIV_graph_classification/
 * dgn_net.py:87-89): the index is a device-to-host read-back per step and cannot be captured.  scores [G, T] fp32 (row stride ld),
 * labels [G, T] fp32 (row stride ld_y), NaN = not labelled; G < 2^31.
 *     loss      = mean over the labelled entries of max(x, 0) - x y + log1p(exp(-|x|))        DEVICE float; no labelled entry: nan
 *     g_scores  = (sigmoid(x) - y) / n_labelled on labelled entries, exactly 0 elsewhere   [G, T] (row stride ld_g); NULL: not wanted
 * The labelled count is taken on the device; cross-lane and cross-workgroup sums run in fp64 in an order that depends on (G, T) alone.
 * Two launches; ws: 8-byte aligned, dgn_masked_bce_workspace_bytes bytes.  dgn_masked_bce_backward: the autograd backward, ONE launch:
 * g_scores[r, t] = g_saved[r, t] * *g_loss (g_loss: DEVICE float).                                                                    */
#define DGN_MULTI_EMBEDDING_MAX_COLS 16
int dgn_multi_embedding_supported(int32_t n_cols, const int32_t* dims, int32_t F);
size_t dgn_multi_embedding_backward_workspace_bytes(int64_t n_rows, int32_t n_cols, const int32_t* dims, int32_t F);
int dgn_multi_embedding_forward(int64_t n_rows, int32_t n_cols, int32_t F, const int64_t* idx, int64_t ld_idx, const float* const* tables,
                                const int32_t* dims, float* out, int64_t ld_out, void* stream);
int dgn_multi_embedding_backward(int64_t n_rows, int32_t n_cols, int32_t F, const int64_t* idx, int64_t ld_idx, const int32_t* dims,
                                 const float* g, int64_t ld_g, float* const* g_tables, void* ws, size_t ws_bytes, void* stream);
size_t dgn_masked_bce_workspace_bytes(int64_t n_rows, int32_t n_tasks);
int dgn_masked_bce_forward(int64_t n_rows, int32_t n_tasks, const float* scores, int64_t ld, const float* labels, int64_t ld_y, float* loss,
                           float* g_scores, int64_t ld_g, void* ws, size_t ws_bytes, void* stream);
int dgn_masked_bce_backward(int64_t n_rows, int32_t n_tasks, const float* g_saved, int64_t ld_g, const float* g_loss, float* g_scores,
                            int64_t ld_out, void* stream);
/* Masked L1.  Replaces nn.L1Loss() of nets/molecules_graph_regression/dgn_net.py:90-92 (= MAE of train/metrics.py:14-16) with the masking
 * convention above: targets [G, T] fp32 (row stride ld_y), NaN = the entry does not count (a padding graph row of a captured batch).  The
 * same two kernels on another term, the same workspace and launch counts:
 *     loss      = (float)(sum over the counted entries of |x - t| (fp32 terms, fp64 sum) / count)     DEVICE float; no counted entry: nan
 *     g_scores  = sign(x - t) * (float)(1.0 / (double)count) on counted entries (sign(0) = 0, as torch's l1_loss backward), exactly 0
 *                 elsewhere; NULL: not wanted
 * dgn_masked_mae_backward: the autograd backward, ONE launch: g_scores[r, t] = g_saved[r, t] * *g_loss.  (The entry points are named after
 * the metric, mean absolute error: the binding's symbol check reads names of letters and underscores.)                                */
size_t dgn_masked_mae_workspace_bytes(int64_t n_rows, int32_t n_tasks);
int dgn_masked_mae_forward(int64_t n_rows, int32_t n_tasks, const float* scores, int64_t ld, const float* targets, int64_t ld_y, float* loss,
                          float* g_scores, int64_t ld_g, void* ws, size_t ws_bytes, void* stream);      /* dgn_net.py:90-92 */
int dgn_masked_mae_backward(int64_t n_rows, int32_t n_tasks, const float* g_saved, int64_t ld_g, const float* g_loss, float* g_scores,
                           int64_t ld_out, void* stream);      /* autograd of dgn_net.py:90-92 */

/* ---- the nets' MLP head in one launch per direction (dgn_mlp_head.hip) ---------------------------------------------------------------
 * Replaces MLPReadout.forward of nets/mlp_readout_layer.py:24-30 (L hidden Linear + ReLU, then an output Linear: three addmm and two ReLU
 * launches forward, about a dozen backward) by one launch forward and two backward.  n_linears = L + 1 in 1 .. 4; dims: HOST array of the
 * n_linears + 1 widths, each in 1 .. 128, sum_l dims[l] dims[l + 1] <= 20 480 (dgn_mlp_head_supported: 1 inside this domain; callers
 * take torch's route outside it).  w / b / g_w / g_b: HOST arrays of n_linears DEVICE pointers to dense fp32 [dims[l + 1], dims[l]] /
 * [dims[l + 1]] tensors (torch's layout; read at the call: they travel in the kernel arguments).  x [n_rows, dims[0]], y and g_y
 * [n_rows, dims[n_linears]], g_x as x: fp32, unit column stride, row strides ld_* >= the width, any 4-byte-aligned base.  n_rows < 2^31.
 *     forward   y = W_L relu(... relu(W_1 x + b_1) ...) + b_L, a tile's activations in LDS between the Linears; every dot product starts
 *               at its bias and takes its terms in increasing k with fmaf.  n_rows == 0: nothing to do.
 *     backward  the hidden activations are computed again from x as the forward computed them (nothing else is kept); a ReLU passes the
 *               gradient where its activation is > 0.  g_x: NULL = not wanted.  g_w / g_b are WRITTEN (n_rows == 0: zeros): per-workgroup
 *               partials in ws, added in workgroup order in fp64 by the second launch.  No floating-point atomics: the same input gives
 *               the same bits.  ws: 4-byte aligned, dgn_mlp_head_backward_workspace_bytes bytes (0 for arguments out of range). */
int dgn_mlp_head_supported(int32_t n_linears, const int32_t* dims);      /* nets/mlp_readout_layer.py:24-30 */
int dgn_mlp_head_forward(int64_t n_rows, int32_t n_linears, const int32_t* dims, const float* x, int64_t ld_x, const float* const* w,
                         const float* const* b, float* y, int64_t ld_y, void* stream);      /* nets/mlp_readout_layer.py:24-30 */
size_t dgn_mlp_head_backward_workspace_bytes(int64_t n_rows, int32_t n_linears, const int32_t* dims);
int dgn_mlp_head_backward(int64_t n_rows, int32_t n_linears, const int32_t* dims, const float* x, int64_t ld_x, const float* const* w,
                          const float* const* b, const float* g_y, int64_t ld_gy, float* g_x, int64_t ld_gx, float* const* g_w,
                          float* const* g_b, void* ws, size_t ws_bytes, void* stream);      /* autograd of nets/mlp_readout_layer.py:24-30 */

/* ---- Laplacian eigenpairs of a batch of small graphs in one Jacobi kernel (dgn_eig_small.hip) ------------------------------------------
 * Replaces, for graphs of at most 64 nodes, the per-graph CPU solves of the reference's loaders: get_eig (data/molecules.py:100-116),
 * positional_encoding (data/molecules.py:18-32) and get_eig_val of the multiplicity check (data/multiplicity_eig.py:14-27).
 * graph: the batch's destination-major CSR (indptr, src; graphs occupy consecutive node ranges); graph_off: DEVICE [n_graphs + 1] node
 * offsets.  Per graph the kernel forms L in fp64 -- in-degrees from indptr clipped to 1, adjacency symmetrised to (A + A^T) / 2, multi-edges
 * and self-loops adding up; DGN_EIG_NORM_NONE: D - A, _SYM: I - D^-1/2 A D^-1/2, _WALK: the _SYM solve with the kept eigenvectors scaled by
 * D^-1/2 and brought back to unit length -- and diagonalises it by cyclic Jacobi rotations until the off-diagonal Frobenius norm is
 * <= 1e-14 ||L||_F or max_sweeps sweeps are done.
 *     vec     [n_nodes, k] fp32, dense rows: the min(k, n) eigenvectors of lowest eigenvalue (ascending, ties by column index; signs as the
 *             rotations leave them, the same bits for the same graph in any batch), further columns of the graph's rows 0
 *     val     [n_graphs, k] fp64 or NULL: their eigenvalues, further slots NaN
 *     status  [n_graphs]: sweeps done (>= 1; == max_sweeps: the stop rule was not met), -1: more than 64 nodes (the second function's
 *             value), -2: an edge source outside the graph's node range, or a node range outside the CSR.  A graph with a negative status
 *             has nothing else written: its rows of vec and val are as they were.
 * 1 <= k <= 32.  Two launches over all graphs (<= 32 nodes: 64 threads, <= 64: 256), nothing read back, capturable.  n_graphs == 0: no-op. */
enum { DGN_EIG_NORM_NONE = 0, DGN_EIG_NORM_SYM = 1, DGN_EIG_NORM_WALK = 2 };
int dgn_eig_small(const DgnGraph* graph, const int64_t* graph_off, int n_graphs, int k, int norm, int max_sweeps, float* vec, double* val,
                  int32_t* status, void* stream);
int dgn_eig_small_max_nodes(void);

/* ---- ... of the graphs of 65 to 192 nodes (dgn_eig_mid.hip) -----------------------------------------------------------------------------
 * The same build, solve, stop rule, epilogue and outputs as dgn_eig_small for the graphs it answers with -1, up to 192 nodes (CLUSTER's
 * largest graph has 190, PATTERN's 188, CIFAR10's 150).  One workgroup per graph, the matrix packed symmetric in LDS in fp64, no eigenvector
 * matrix: every rotation's tangent goes to the graph's log slot in `ws` and the k kept vectors are formed by replaying the log backwards.
 *     graph_ids  DEVICE [n_ids] graph indices or NULL.  Workgroup (= log slot) s solves graph graph_ids[s]; NULL: every graph, slot = graph
 *                index, n_ids ignored.  An entry outside [0, n_graphs) is skipped; no graph may be listed twice.
 *     ws         dgn_eig_mid_workspace_bytes(slots, max_sweeps) bytes, slots = n_ids (n_graphs for NULL graph_ids):
 *                slots * max_sweeps * 191 * 96 * 8.  Too small for the sweep cap: DGN_ERR_WORKSPACE, nothing launched.
 *     status     sweeps done (>= 1), -1: more than 192 nodes, -2 as dgn_eig_small; a graph of at most 64 nodes is NOT touched (status, vec and
 *                val keep what they held): launched after dgn_eig_small on the same buffers the two cover every graph up to 192 nodes.
 * Two launches over the slots ((64, 128] nodes: 512 threads, (128, 192]: 1024 threads and 156 304 bytes of LDS; a device that grants a
 * workgroup less: DGN_ERR_INVALID on the first call), nothing read back, capturable.  A graph's output bits depend on the graph alone. */
int dgn_eig_mid_max_nodes(void);
size_t dgn_eig_mid_workspace_bytes(int n_slots, int max_sweeps);
int dgn_eig_mid(const DgnGraph* graph, const int64_t* graph_off, int n_graphs, const int32_t* graph_ids, int n_ids, int k, int norm,
                int max_sweeps, float* vec, double* val, int32_t* status, void* ws, size_t ws_bytes, void* stream);

/* ---- superpixel k-NN graphs and the sort_eig column choice (dgn_superpixels.hip) --------------------------------------------------------
 * dgn_knn_graph replaces the per-graph host work of the reference's superpixel loader: sigma, compute_adjacency_matrix_images and
 * compute_edges_list (data/superpixels.py:17-69: cdist, two np.partition calls and an exp per graph) with the self-edge removal of
 * SuperPixDGL._prepare (:139-145).  coord: [n_nodes, 2] fp64 (already divided by the image size); feat: [n_nodes, n_feat] fp64, 1 <= n_feat <= 8,
 * or NULL with n_feat = 0 (coordinates only: use_feat=False); graph_off / edge_off: DEVICE [n_graphs + 1] node / edge offsets.  Per graph of
 * n nodes, in fp64 and in the reference's order of operations: d_c, d_f the Euclidean distances of coordinates / features,
 * sigma(i) = (sum of the k + 1 smallest entries of row i, the zero diagonal included) / k + 1e-8 for n >= k + 1, else 1 + 1e-8,
 * E(i, j) = exp(-(d_c / sigma_c(i))^2 - (d_f / sigma_f(i))^2), A = (E + E^T) / 2 with a zero diagonal.  Edges:
 *     n >= k + 2       the n - 1 other nodes of row i ranked by A descending, equal values by lower column; skip_nearest = 1 emits ranks 1 .. k
 *                      -- the reference's np.argpartition(A, n - 10)[:, n - 9:-1] at k = 8: it LEAVES OUT the most similar node --,
 *                      skip_nearest = 0 ranks 0 .. k - 1; k edges per node in rank order
 *     2 <= n <= k + 1  every j != i in ascending j: n - 1 edges per node
 *     n == 1           one self-loop of value 0
 *     src, dst   [n_edges] int64: edge edge_off[g] + i * per_node + slot has src = n0 + i (row i is the sender: g.add_edges(src, dsts)), dst = n0 + j
 *     value      [n_edges] fp32: (float) A(i, j), the reference's edge feature
 *     status     [n_graphs]: 0 ok, -1: more than dgn_knn_graph_max_nodes() = 256 nodes, -2: a node or edge range outside the arrays or an
 *                edge_off span that is not the count of the rule above.  A graph with a negative status has nothing else written.
 * 1 <= k <= 32.  One launch, one workgroup of 256 threads per graph, nothing read back, capturable; a graph's output bits depend on the graph
 * alone.  n_graphs == 0: no-op.
 *
 * dgn_superpixel_sort_eig replaces sort_eig / get_scores (data/superpixels.py:371-420) on eig [n_nodes, n_cols] fp32 (row stride ld_eig,
 * n_cols >= 3) with the nodes' coordinates x, y [n_nodes] fp32: for column c in {1, 2}, hor_c = |sum over eig[i, c] > 0 of (x_i > 0.5 ? 1 : -1)|,
 * ver_c likewise with y, m the largest of the four.  hor_1 == m or ver_2 == m: the graph's rows stay.  Otherwise column 1 of its rows is
 * overwritten with column 2, in place: what the reference's two exchanging arms leave (eigs[:, 1] = eig2; eigs[:, 2] = eig1 with eig1 a VIEW of
 * column 1 -- column 2 ends up in both columns; fixture G15 holds the reference's output).  One launch, a wave per graph, no status: a graph
 * whose node range lies outside [0, n_nodes] is skipped.  Nothing read back, capturable.  n_graphs == 0: no-op. */
int dgn_knn_graph_max_nodes(void);
int dgn_knn_graph(const double* coord, const double* feat, int n_feat, int64_t n_nodes, const int64_t* graph_off,
                  const int64_t* edge_off, int n_graphs, int k, int skip_nearest, int64_t n_edges,
                  int64_t* src, int64_t* dst, float* value, int32_t* status, void* stream);
int dgn_superpixel_sort_eig(float* eig, int64_t ld_eig, int n_cols, const float* x, const float* y,
                            int64_t n_nodes, const int64_t* graph_off, int n_graphs, void* stream);

/* ---- superpixel graph classification: feature embedding + class cross-entropy with hit count (dgn_graph_cls.hip) ------------------------
 * Feature embedding.  Replaces embedding_h / embedding_e of nets/superpixels_graph_classification/dgn_net.py:31, :35 as :53, :56 call them:
 * nn.Linear(in_dim, hidden) on the pixel value(s) + two coordinates (in_dim 3: MNIST, 5: CIFAR10) and nn.Linear(1, edge_dim) on the edge
 * value -- shapes dgn_linear_supported refuses (odd or tiny k).  x [n_rows, k] fp32 (row stride ld >= k), 1 <= k <= DGN_FEAT_EMBED_MAX_K;
 * w [f_out, k] dense (torch's layout), 1 <= f_out <= DGN_FEAT_EMBED_MAX_F, odd widths included; b [f_out] or NULL; n_rows < 2^31
 * (dgn_feat_embed_supported: 1 inside this domain of (k, f_out)).
 *     forward   y[r, f] = fmaf(w[f, k - 1], x[r, k - 1], ... fmaf(w[f, 0], x[r, 0], b[f])): the terms in increasing k, starting at the bias
 *               (0 without one).  y [n_rows, f_out] (row stride ld_y >= f_out); dense rows (ld_y == f_out) at a 16-byte aligned base are
 *               written as flat 16-byte chunks whatever f_out is.  One launch; w and b resident in LDS.
 *     backward  g_w[f, k] = sum_r g[r, f] x[r, k], g_b[f] = sum_r g[r, f] (g_b: NULL = not wanted); g [n_rows, f_out] (row stride ld_g).
 *               Two launches: per-workgroup partial [k + 1, f_out] blocks over contiguous row ranges in ws, then the blocks added in a
 *               fixed order.  No floating-point atomics: the same input gives the same bits.  There is no input gradient: x is data.
 *               ws: 4-byte aligned, dgn_feat_embed_backward_workspace_bytes bytes (0 for arguments out of range).
 * n_rows == 0: DGN_OK with nothing launched in either direction; the backward then leaves g_w / g_b as they were (the sum over no row
 * is the caller's zero fill).
 *
 * Class cross-entropy with hit count.  Replaces DGNNet.loss of nets/superpixels_graph_classification/dgn_net.py:75-78
 * (nn.CrossEntropyLoss(): log_softmax + nll_loss, five small launches forward and two backward) and accuracy_MNIST_CIFAR of
 * train/metrics.py:25-28 (argmax, eq, sum and the .item() read-back the loop train/train_superpixels_graph_classification.py makes per
 * step).  scores [n_rows, C] fp32 (row stride ld >= C), 2 <= C <= DGN_CLASS_CE_MAX_CLASSES (dgn_class_ce_supported), labels [n_rows]
 * int64, n_rows < 2^31.  A label < 0 marks a row that does not exist (padding of a captured batch, as for dgn_node_ce_forward): it counts
 * nowhere and its gradient row is exactly zero.  V = number of rows with a label >= 0:
 *     loss      = sum over those rows of (m + log sum_c exp(scores[n, c] - m)) - scores[n, y_n], m = max_c scores[n, c], divided by V
 *                 DEVICE float; per row in fp32 (exp, log), across rows in fp64 in an order that depends on n_rows alone
 *     hits      = number of those rows whose FIRST maximal score sits at column y_n (torch.argmax's tie rule; a NaN score counts as
 *                 the largest, as there).  DEVICE int64; NULL: not wanted
 *     g_scores  = (softmax(scores[n, :]) - onehot(y_n)) / V   [n_rows, C] (row stride ld_g), every row written; NULL: not wanted
 * V == 0 (n_rows == 0 included): loss nan (0 / 0, the mean over nothing), hits 0, every gradient row 0.  A label >= C is NOT padding: the
 * row counts in V, its loss term is nan (so the loss is), it is never a hit, its gradient row is nan, and nothing is read or written
 * outside the row's C columns.  A NaN score makes the loss nan.  Two launches; ws: 8-byte aligned, dgn_class_ce_workspace_bytes bytes
 * (0 for arguments out of range).  dgn_class_ce_backward: the autograd backward, ONE launch: g_scores[n, c] = g_saved[n, c] * *g_loss
 * (g_loss: DEVICE float; g_saved: what the forward wrote). */
#define DGN_FEAT_EMBED_MAX_K 8
#define DGN_FEAT_EMBED_MAX_F 160
#define DGN_CLASS_CE_MAX_CLASSES 64
int dgn_feat_embed_supported(int32_t k, int32_t f_out);      /* nets/superpixels_graph_classification/dgn_net.py:31, :35 */
int dgn_feat_embed_forward(int64_t n_rows, int32_t k, int32_t f_out, const float* x, int64_t ld, const float* w, const float* b, float* y,
                           int64_t ld_y, void* stream);      /* dgn_net.py:53, :56 */
size_t dgn_feat_embed_backward_workspace_bytes(int64_t n_rows, int32_t k, int32_t f_out);
int dgn_feat_embed_backward(int64_t n_rows, int32_t k, int32_t f_out, const float* x, int64_t ld, const float* g, int64_t ld_g, float* g_w,
                            float* g_b, void* ws, size_t ws_bytes, void* stream);      /* autograd of dgn_net.py:53, :56 */
int dgn_class_ce_supported(int32_t n_classes);
size_t dgn_class_ce_workspace_bytes(int64_t n_rows, int32_t n_classes);
int dgn_class_ce_forward(int64_t n_rows, int32_t n_classes, const float* scores, int64_t ld, const int64_t* labels, float* loss,
                         int64_t* hits, float* g_scores, int64_t ld_g, void* ws, size_t ws_bytes,
                         void* stream);      /* dgn_net.py:75-78 + train/metrics.py:25-28 */
int dgn_class_ce_backward(int64_t n_rows, int32_t n_classes, const float* g_saved, int64_t ld_g, const float* g_loss, float* g_scores,
                          int64_t ld_out, void* stream);      /* autograd of dgn_net.py:75-78 */

/* ---- input stage of the nets with positional encodings: embedding sum + Linear on pos_enc in one pass (dgn_node_input.hip) ---------------
 * Replaces h = embedding_h(h) + embedding_pos_enc(g.ndata['pos_enc']) of nets/molecules_graph_regression/dgn_net.py:60-62,
 * nets/SBMs_node_classification/dgn_net.py:57-59 and nets/HIV_graph_classification/dgn_net.py:64-66 (with in_feat_dropout inactive
 * between the two terms): the lookup(s), an nn.Linear(K, hidden) with K of 2 to 20 -- a library GEMM on a shape dgn_linear_supported
 * refuses -- and an add forward; the embedding backward(s), two GEMM gradients and a bias reduction backward.  idx [N, C] int64 (row
 * stride ld_idx >= C, unit column stride), 1 <= C <= DGN_MULTI_EMBEDDING_MAX_COLS; tables / g_tables: HOST arrays of C DEVICE pointers to
 * dense fp32 [dims[c], F] tables (they travel in the kernel arguments), dims: HOST array; pe [N, K] fp32 (row stride ld_pe >= K, unit
 * column stride, base 4-byte aligned: a column slice of eig), 1 <= K <= DGN_NODE_INPUT_MAX_K; w [F, K] dense (torch's layout), b [F] or
 * NULL.  N < 2^31.  (sum(dims) + K + 1) * F floats -- the backward's partial block -- and (K + 1) * F + 64 * (K + C) floats -- the forward's
 * residents -- must each fit the CU's 160 KB of LDS: dgn_node_input_supported says whether they do (callers take the composition
 * otherwise).  An index outside [0, dims[c]) is CLAMPED into the table.
 *     forward   out[n, f] = (((0 + T_0[i_0][f]) + T_1[i_1][f]) + ...) + fmaf(w[f, K-1], pe[n, K-1], ... fmaf(w[f, 0], pe[n, 0], b[f])):
 *               the table terms in column order, the linear terms in increasing k from the bias on (0 without one), the two partial
 *               results added last.  out [N, F] (row stride ld_out >= F); dense rows (ld_out == F) at a 16-byte aligned base are
 *               written as flat 16-byte chunks whatever F is.  One launch; w (transposed) and b resident in LDS.
 *     backward  g_tables[c][r, :] = sum_{n: idx[n, c] = r} g[n, :] (rows without a hit: 0), g_w[f, k] = sum_n g[n, f] pe[n, k],
 *               g_b[f] = sum_n g[n, f] (g_b: NULL = not wanted) in ONE pass over g [N, F] (row stride ld_g); two launches: per-workgroup
 *               partial blocks [sum(dims) + K + 1, F] in LDS over contiguous row ranges (every column's adds in row order), then the
 *               blocks added in a fixed order.  No floating-point atomics: the same input gives the same bits.  There is no gradient
 *               for pe: it is data.  ws: 4-byte aligned, dgn_node_input_backward_workspace_bytes bytes (0 for unsupported arguments).
 * N == 0: DGN_OK with nothing launched in either direction; the backward then leaves the gradients as they were (the sum over no row is
 * the caller's zero fill). */
#define DGN_NODE_INPUT_MAX_K 40      /* data/SBMs.py:135 prepares "40 PEs" */
int dgn_node_input_supported(int32_t n_cols, const int32_t* dims, int32_t k, int32_t F);      /* dgn_net.py:60-62 */
int dgn_node_input_forward(int64_t n_rows, int32_t n_cols, int32_t k, int32_t F, const int64_t* idx, int64_t ld_idx, const float* const* tables,
                           const int32_t* dims, const float* pe, int64_t ld_pe, const float* w, const float* b, float* out, int64_t ld_out,
                           void* stream);      /* molecules dgn_net.py:60-62, SBMs dgn_net.py:57-59, HIV dgn_net.py:64-66 */
size_t dgn_node_input_backward_workspace_bytes(int64_t n_rows, int32_t n_cols, const int32_t* dims, int32_t k, int32_t F);
int dgn_node_input_backward(int64_t n_rows, int32_t n_cols, int32_t k, int32_t F, const int64_t* idx, int64_t ld_idx, const int32_t* dims,
                            const float* pe, int64_t ld_pe, const float* g, int64_t ld_g, float* const* g_tables, float* g_w, float* g_b, void* ws,
                            size_t ws_bytes, void* stream);      /* autograd of the same lines */

/* ---- collate: a batch of a device-resident dataset as ONE gather (dgn_collate.hip) -------------------------------------------
 * The reference forms every batch on the host (`collate`: data/molecules.py:219-230, data/SBMs.py:167-179, data/HIV.py:113-125,
 * data/PCBA.py:266-278, data/superpixels.py:316-330: dgl.batch over the samples plus the graph-norm vectors).  Here the dataset
 * is packed once -- concatenated columns and ONE DgnGraph over all its nodes (dgn_graph_build + dgn_graph_build_csc) -- and, since
 * the graphs of a batch are disjoint and every graph's nodes, edges, CSR slots and CSC ranks are one contiguous range of the
 * dataset, a batch's arrays are shifted copies of those ranges.  One kernel launch on `stream`: no host synchronisation, no
 * workspace, no library call, every launch parameter a function of the sizes.
 *   table        DEVICE int32 [5][G + 1] (rows: batch node offset, batch edge offset, dataset node base, dataset edge base, dataset
 *                graph id; the offsets' entry G is N resp. E, the other rows' entry G is not read).  The host computes it (the batch's
 *                graph ids are host-known) and uploads it with one copy.
 *   d_*          the dataset: its DgnGraph arrays, its edge list in edge-id order (int64, dataset node ids), the per-GRAPH graph-norm
 *                values (the kernel only broadcasts them, so they carry the reference's own host arithmetic bit for bit)
 *   columns      *_in [c] a dataset column of *_row_bytes [c] bytes per row (a multiple of 4), *_out [c] its batch rows (NULL: not
 *                wanted), *_pad [c] the 8-byte pattern of the rows behind the batch (even dwords of a row take its low half, odd ones
 *                its high half: 0, -1 and two copies of a float's bits all fit).  Host arrays, they travel in the kernel arguments.
 *   outputs      each optional (NULL = not wanted) and written for the FULL capacity n_rows_out >= N, e_rows_out >= E, g_rows_out >= G:
 *                column rows; snorm_n / snorm_e (0 behind the batch); graph_id (int32, -1 behind); src / dst (int64, edge-id order,
 *                batch node ids; 0 behind); and the batch's DgnGraph arrays exactly as dgn_graph_build + dgn_graph_build_csc on that
 *                edge list with n_nodes = n_rows_out leave them: indptr / csc_ptr [n_rows_out + 1] (= E from row N on), src_csr /
 *                dst_csr / eid / csc_pos / csc_order [e_rows_out] (0 behind), in_degree / log_deg [n_rows_out] (0 behind), stats
 *                int32 [4] = (max_in_degree, 0, 0, 0), n_valid int64 [1] = N.
 * 1 <= G <= 65 535 graphs of any size within the int32 totals; G == 0 or N == 0: DGN_OK, the pad values everywhere.  More columns
 * than the limits below, a row width that is no multiple of 4, capacities below the batch: DGN_ERR_INVALID, nothing launched. */
#define DGN_COLLATE_MAX_NODE_COLS 8
#define DGN_COLLATE_MAX_EDGE_COLS 4
#define DGN_COLLATE_MAX_GRAPH_COLS 2
#define DGN_COLLATE_MAX_GRAPHS 65535
typedef struct DgnCollate {
    int64_t n_graphs, n_nodes, n_edges;              /* the batch: G, N, E                                            */
    int64_t n_rows_out, e_rows_out, g_rows_out;      /* rows of every per-node / per-edge / per-graph output           */
    const int32_t* table;
    const int32_t* d_indptr;
    const int32_t* d_src;
    const int32_t* d_dst_csr;
    const int64_t* d_eid;
    const int64_t* d_in_degree;
    const float* d_log_deg;
    const int32_t* d_csc_ptr;
    const int32_t* d_csc_pos;
    const int32_t* d_csc_order;
    const int64_t* d_edge_src;
    const int64_t* d_edge_dst;
    const float* d_snorm_n;
    const float* d_snorm_e;
    int32_t n_node_cols, n_edge_cols, n_graph_cols;
    int32_t max_in_degree;                           /* of the batch (host-known: the largest of its graphs')          */
    const void* node_in[DGN_COLLATE_MAX_NODE_COLS];
    void* node_out[DGN_COLLATE_MAX_NODE_COLS];
    int64_t node_pad[DGN_COLLATE_MAX_NODE_COLS];
    int32_t node_row_bytes[DGN_COLLATE_MAX_NODE_COLS];
    const void* edge_in[DGN_COLLATE_MAX_EDGE_COLS];
    void* edge_out[DGN_COLLATE_MAX_EDGE_COLS];
    int64_t edge_pad[DGN_COLLATE_MAX_EDGE_COLS];
    int32_t edge_row_bytes[DGN_COLLATE_MAX_EDGE_COLS];
    const void* graph_in[DGN_COLLATE_MAX_GRAPH_COLS];
    void* graph_out[DGN_COLLATE_MAX_GRAPH_COLS];
    int64_t graph_pad[DGN_COLLATE_MAX_GRAPH_COLS];
    int32_t graph_row_bytes[DGN_COLLATE_MAX_GRAPH_COLS];
    float* snorm_n;
    float* snorm_e;
    int32_t* graph_id;
    int64_t* src;
    int64_t* dst;
    int32_t* indptr;
    int32_t* src_csr;
    int32_t* dst_csr;
    int64_t* eid;
    int64_t* in_degree;
    float* log_deg;
    int32_t* csc_ptr;
    int32_t* csc_pos;
    int32_t* csc_order;
    int32_t* stats;
    int64_t* n_valid;
} DgnCollate;
int dgn_collate(const DgnCollate* c, void* stream);

/* ---- eigenvector augmentations of the training loops (dgn_eig_augment.hip) ------------------------------------------------------
 * The reference augments the Laplacian eigenvectors of every batch before the forward pass: a random sign per entry of `eig` in the
 * molecule loop (train/train_molecules_graph_regression.py:29-33, --flip), and in the superpixel loop a random per-node rotation of
 * the (eig1, eig2) pair by up to --augmentation degrees, then a random sign per node on column 2
 * (train/train_superpixels_graph_classification.py:29-42).  Here both are ONE kernel, one thread per row, whose random stream is kept
 * and advanced on the device by the kernel itself: nothing else is launched, so a captured graph draws new values on every replay.
 *   eig / out    fp32 [n_rows, K] with row strides ld_in / ld_out >= K, 1 <= K <= 32; out == eig with equal strides is allowed (a
 *                thread reads its whole row before it writes)
 *   state        DEVICE int64 [4] = {key, calls, ticket, 0}, ticket = 0 between calls.  Row i of call number c = calls draws
 *                r[0..3] = Philox4x32-10(counter = (lo32 i, hi32 i, lo32 c, hi32 c), key = (lo32 key, hi32 key)); the call that
 *                finishes leaves calls = c + 1: the same (key, calls) gives the same output for any grid
 *   rotate_deg   != 0 (needs K >= 3): u = (r[0] >> 8) 2^-24, angle = (u - 0.5) 2 rotate_deg, s = sin(angle pi / 180),
 *                c = sqrt(1 - s^2) -- the reference's form, |cos| beyond +-90 degrees --, out1 = c x1 + s x2, out2 = c x2 - s x1
 *   flip_mask    after the rotation, as in the superpixel loop: column j < K with bit j set is multiplied (0 -> -0, as torch.mul) by
 *                +1 where bit j of r[1] is set, by -1 where not.  Molecule loop: flip_mask = (1 << K) - 1, rotate_deg = 0;
 *                superpixel loop: flip_mask = 1 << 2 plus its angle.  Columns not named are copied.
 * n_rows == 0: DGN_OK, nothing launched, state untouched.  K outside 1..32, a rotation with K < 3, strides below K, a non-finite
 * angle: DGN_ERR_INVALID, nothing launched. */
int dgn_eig_augment(int64_t n_rows, int32_t K, const float* eig, int64_t ld_in, float* out, int64_t ld_out, float rotate_deg,
                    int32_t flip_mask, int64_t* state, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DGN_HIP_H */
