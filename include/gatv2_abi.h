/* gatv2_abi.h — C ABI of the MI355X-native GATv2 edge-centric hot path (libgatv2_hip.so).
 *
 * The reference (GATv2_edge_based.cu, cited E:<line>) has no FFI/plugin seam: `main` launches
 * its kernels inline (E:1370-1642).  This header defines the seam at exactly those launch
 * sites; every entry point names the reference launch(es) it replaces.  Plain C: pointers and
 * sizes only, no C++/torch types.  All functions return 0 on success, otherwise a non-zero
 * status (a hipError_t value, or one of GAT_E_*); gat_last_error() gives the message.
 *
 * Layouts at the boundary are the REFERENCE layouts:
 *   W   flat [l][H_l][D_l][2*F_l]  (cols 0..F-1 multiply x_src, F..2F-1 x_dst; E:294-316)
 *   a   flat [l][H_l][D_l]                                                    (E:296)
 *   Wo  [C][D_last]                                                           (E:464)
 *   edge tensors [H][E] head-major (E:297), node tensors [N][H][D] (E:410)
 * Inside the context tensors live in MI355X-friendly layouts (edge tensors [E][H], projected
 * features PL/PR [N][H*D]); gat_tap() converts back.
 *
 * Threading: a context is not thread-safe; one context per GPU / per rank.
 * Ownership: the caller owns host arrays and the gat_ctx*; the context owns its device memory
 * except buffers handed in through gat_bind_table() (borrowed, never freed).
 */
#ifndef GATV2_ABI_H
#define GATV2_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GAT_ABI_VERSION 6

enum {
    GAT_OK = 0,
    GAT_E_INVALID = 10001,   /* bad argument / shape */
    GAT_E_STATE = 10002,     /* call order (e.g. forward before set_graph) */
    GAT_E_NOMEM = 10003,
    GAT_E_UNSUPPORTED = 10004,
    GAT_E_COMM = 10005       /* exchange transport (RCCL / host-staged) */
};

typedef struct gat_ctx gat_ctx;

/* Mirrors the reference's CLI model config (E:934-1010, 1115-1118, 1143). */
typedef struct gat_config {
    int32_t num_layers;        /* --num-layers */
    const int32_t* heads;      /* --heads,   [num_layers] */
    const int32_t* outdims;    /* --outdims, [num_layers] */
    int32_t in_dim;            /* input_feature_vector_dim (E:1079) */
    int32_t num_classes;       /* max(label)+1 (E:1107) */
    float negative_slope;      /* 0.01f (E:1143) */
    int32_t device;            /* HIP device ordinal */
    void* stream;              /* hipStream_t to run on; NULL = context creates its own */
    int32_t flat_lrelu_index;  /* 0 = exact per-head LReLU' in the output gradient (default);
                                  1 = the reference's flat index n*D+d (E:598) */
    int32_t collect_timing;    /* 1 = bracket every kernel with hipEvents (gat_kernel_stats) */
    int32_t keep_taps;         /* 1 = also keep tensors only parity tests read (ge, max, sum) */
    int32_t storage_dtype;     /* GAT_DTYPE_F32 (default) | GAT_DTYPE_BF16: the projected source table PL (gathered
                                  per edge, exchanged between shards) and the per-edge message rows are STORED as
                                  bf16; every sum, the softmax and all other tensors stay fp32.  BASELINE config 5
                                  ("bf16"); parity bar vs the fp32 oracle: alpha, loss 1e-2. */
} gat_config;
enum { GAT_DTYPE_F32 = 0, GAT_DTYPE_BF16 = 1 };

const char* gat_last_error(void);
int gat_abi_version(void);
int gat_device_count(int* count);
/* The environment switches this process has read and found set, as "NAME=VALUE NAME=VALUE" (empty string: none).  They select among
 * kernels / launch shapes that compute the same results (A/B measurements and the test matrices use them) — never a
 * different result: the timing-only experiment variants (GAT_DBG) exist only in the experiment library (`make experiments`,
 * libgatv2_hip_exp.so, whose text starts with "[experiment library]").  buf: at least a few hundred bytes. */
int gat_switches(char* buf, int64_t cap);

/* ---- lifecycle (replaces the inline cudaMalloc plan, E:1151-1357) ------------------------- */
int gat_create(const gat_config* cfg, gat_ctx** out);
int gat_destroy(gat_ctx* ctx);
int gat_sync(gat_ctx* ctx);                       /* wait for the context's stream */
int gat_mem_info(size_t* free_bytes, size_t* total_bytes);   /* cudaMemGetInfo, E:930, 1362 */

/* ---- data (H2D copies E:1151-1172; CSR->COO E:1186) --------------------------------------
 * Rows are destinations, columns are sources (E:74-82).  Single GPU: n_table == n_rows,
 * table_row0 == 0.  Destination-range shard: the context owns rows
 * [table_row0, table_row0+n_rows) of an n_table-row source table and col_idx holds table row
 * ids (see INTEGRATION.md "sharding"); host arrays are copied. */
/* Limits: n_edges, n_rows and n_table must each fit int32 (the reference's CSR is int32 too, E:1045-1046; the
 * one-time source-major index is built with a 32-bit-count radix sort) — larger graphs are refused with
 * GAT_E_UNSUPPORTED, never truncated.  Offsets INTO tensors are 64-bit everywhere.  The wave-per-row kernels
 * address the gathered PL table as base + 32-bit byte offset: a table of 4 GiB or more (n_table * H*D * 4 bytes, i.e.
 * > 16.7 M rows at H*D = 64) runs on the generic kernels instead — same results, float atomics, several times slower
 * (no BASELINE config is that large per GPU; bf16 storage is refused there). */
int gat_set_graph(gat_ctx* ctx, const int32_t* row_ptr, const int32_t* col_idx, int64_t n_rows,
                  int64_t n_edges, int64_t n_table, int64_t table_row0);
/* Which edge kernels layer `layer` runs on (known once the graph is set).  The size cliff above is never silent: the
 * gat_set_* call that completes the context (graph + features + labels) still returns 0, but leaves a text starting with
 * "warning:" in gat_last_error() when a layer is GAT_PATH_GENERIC_SIZE (one text naming every affected layer; any later
 * failing call replaces it).  gat_last_error() is a per-thread last-message slot, so the durable way to find out is this query:
 * call it for every layer after the context is complete (train_edge does, and prints the warning once to stderr). */
enum {
    GAT_PATH_GENERIC_SHAPE = 0,   /* (H, D) outside the wave-per-row templates (H*D not in {8,16,32,64} or D not a power of two) */
    GAT_PATH_FAST = 1,            /* wave-per-row / group-per-row kernels, no atomics */
    GAT_PATH_GENERIC_SIZE = 2     /* the shape has fast kernels, but the gathered table is >= 4 GiB */
};
int gat_layer_path(gat_ctx* ctx, int32_t layer, int32_t* path);
/* Non-finite inputs: the reference's plain fp32 loops (E:303-316) turn a +-inf feature into +-inf or NaN sums; every row
 * that aggregates the node within the model's layers ends with NaN class probabilities, and the loss stays finite because
 * E:527 clamps with fmaxf(prob, 1e-12f), which drops a NaN.  Here the dense products cut every fp32 operand into three bf16
 * pieces (x - bf16(x) is inf - inf for an infinite x), so a non-finite — or within half a bf16 ulp of FLT_MAX — feature or
 * weight yields NaN at once where the reference may still hold +-inf: a row the reference rescues (an edge whose score is
 * -inf gets attention 0 there) can be NaN here.  The poisoned rows are a superset of the reference's and a subset of the
 * node's L-hop neighbourhood; all other rows are unaffected; nothing hangs or faults (tests/test_nonfinite.py). */
int gat_set_features(gat_ctx* ctx, const float* x, int64_t n_rows, int32_t in_dim);   /* [n_rows][F0] */
int gat_set_labels(gat_ctx* ctx, const int32_t* labels, int64_t n_rows);
/* Train / validation / test splits — beyond the reference, which trains and evaluates on ALL nodes (E:514-537,
 * README R:134 "later").  mask[n_rows]: 1 = the node belongs to the split.  With a training mask, loss, #correct and
 * the output gradient dz = y - onehot (E:571-573) are taken over the masked nodes only (every node still takes part in
 * the message passing); NULL restores the reference's behaviour.  gat_eval_mask: loss sum / #correct / #nodes of the
 * LAST forward over another split (call after gat_forward or gat_step). */
int gat_set_train_mask(gat_ctx* ctx, const uint8_t* mask, int64_t n_rows);
int gat_eval_mask(gat_ctx* ctx, const uint8_t* mask, int64_t n_rows, double* loss_sum, int32_t* n_correct, int32_t* n_nodes);
/* Device-resident variants (pointers on ctx's device; copied D2D). */
int gat_set_graph_device(gat_ctx* ctx, const int32_t* d_row_ptr, const int32_t* d_col_idx,
                         int64_t n_rows, int64_t n_edges, int64_t n_table, int64_t table_row0);
int gat_set_features_device(gat_ctx* ctx, const float* d_x, int64_t n_rows, int32_t in_dim);
int gat_set_labels_device(gat_ctx* ctx, const int32_t* d_labels, int64_t n_rows);
/* Replicated layer-0 input for a shard (call INSTEAD of gat_set_features, after gat_set_graph):
 * the features of every row of the source table, [n_table][F0] (padding rows: zeros).  The input
 * features are static (read-only in the reference too, E:1151), so each shard can project the
 * whole layer-0 table itself and accumulate gradW_left of layer 0 from its partial gPL table;
 * layer 0 then needs no PL all-gather and no gPL reduce-scatter (gat_layer_exchange reports 0) —
 * the packed parameter-gradient all-reduce completes the sum over shards. */
int gat_set_source_features(gat_ctx* ctx, const float* x_table, int64_t n_table, int32_t in_dim);
int gat_set_source_features_device(gat_ctx* ctx, const float* d_x_table, int64_t n_table, int32_t in_dim);

/* ---- graph construction (beyond the reference, which reads a finished CSR only: README "Graph Data Handling") ----------
 * The training graph built ON the device from an edge list (COO / `edge_index`): n_in edges (src[i], dst[i]), a message
 * flows src -> dst.  dst is a row of the context, 0 <= dst < n_rows; src is a row of the source table, 0 <= src < n_table
 * (single GPU: n_table == n_rows, table_row0 == 0; a destination-range shard as in gat_set_graph).
 *   GAT_GRAPH_SELF_LOOPS  every row r ends with EXACTLY one edge from table row table_row0 + r: self-loops already present
 *                         (any multiplicity) are dropped, one is added
 *   GAT_GRAPH_SYMMETRIZE  for every input edge with src != dst the edge (dst, src) is added as well; needs n_table == n_rows
 *                         and table_row0 == 0, else GAT_E_UNSUPPORTED (shards: symmetrize the whole graph, then shard)
 *   GAT_GRAPH_COALESCE    edges with equal (src, dst) are reduced to one
 * Applied in this order: symmetrize, self-loops, coalesce.  Without COALESCE multiplicities are kept.  flags == 0 is the
 * plain COO -> CSR conversion; any other bit: GAT_E_INVALID.  Result: CSR with rows = destinations and, inside every row,
 * the sources ascending — fully determined by the input multiset and the flags.
 * Errors: a src or dst out of range gives GAT_E_INVALID and a text naming the lowest offending edge index and its value;
 * more than 2^31-1 intermediate edges (n_in, doubled by SYMMETRIZE, plus n_rows with SELF_LOOPS: the count the 32-bit
 * radix sort takes) gives GAT_E_UNSUPPORTED, never a truncated graph.  n_in == 0 is legal.
 * Temporary device memory: 16 B x the intermediate edge count (two buffers of 64-bit keys) plus a few MB of sort scratch
 * — 0.99 GB for 61.9 M edges, 2.0 GB with SYMMETRIZE — freed before return.  Inputs are never modified. */
enum { GAT_GRAPH_SELF_LOOPS = 1, GAT_GRAPH_SYMMETRIZE = 2, GAT_GRAPH_COALESCE = 4 };
/* Stateless, device pointers (current device).  Count-then-fill: with d_col_idx == NULL only *n_edges_out is written; with
 * col_capacity < *n_edges_out the call returns GAT_E_INVALID and still sets *n_edges_out.  d_row_ptr: n_rows + 1 entries.
 * Both phases run the whole sort (the count of a COALESCE build is not known earlier).  Synchronises `stream` (may be NULL). */
int gat_graph_from_coo_device(const int32_t* d_src, const int32_t* d_dst, int64_t n_in, int64_t n_rows, int64_t n_table,
                              int64_t table_row0, int32_t flags, int32_t* d_row_ptr, int32_t* d_col_idx, int64_t col_capacity,
                              int64_t* n_edges_out, void* stream);
/* The same with HOST arrays in and out, staged by the library on `device` (callers without a device allocator). */
int gat_graph_from_coo(const int32_t* src, const int32_t* dst, int64_t n_in, int64_t n_rows, int64_t n_table, int64_t table_row0,
                       int32_t flags, int32_t* row_ptr_out, int32_t* col_idx_out, int64_t col_capacity, int64_t* n_edges_out,
                       int32_t device);
/* Build on the context's device, then continue exactly as gat_set_graph_device (work list, source-major index).  State
 * rules of gat_set_graph (graph already set: GAT_E_STATE).  Host arrays / device pointers. */
int gat_set_graph_coo(gat_ctx* ctx, const int32_t* src, const int32_t* dst, int64_t n_in, int64_t n_rows, int64_t n_table,
                      int64_t table_row0, int32_t flags);
int gat_set_graph_coo_device(gat_ctx* ctx, const int32_t* d_src, const int32_t* d_dst, int64_t n_in, int64_t n_rows,
                             int64_t n_table, int64_t table_row0, int32_t flags);
/* The CSR the context trains on (after a build the caller does not know the edge count).  Any pointer of gat_graph_size may
 * be NULL; gat_graph_get copies n_rows + 1 and n_edges int32 to the host. */
int gat_graph_size(gat_ctx* ctx, int64_t* n_rows, int64_t* n_edges, int64_t* n_table);
int gat_graph_get(gat_ctx* ctx, int32_t* row_ptr_host, int32_t* col_idx_host);
/* One pass over a DEVICE CSR (reads 4(n_rows+1) + 4 n_edges bytes).  *problem = 0 when the CSR is fine, else the first rule
 * broken in the order gat_set_graph checks them; *where (may be NULL) = the lowest offending index (0, n_rows, the row i with
 * row_ptr[i+1] < row_ptr[i], the edge e with col_idx[e] outside [0, n_table)), -1 when fine.  The call returns 0 when it could
 * check: a bad graph is a result, not a failure.  gat_set_graph_device runs this check on its arguments before anything
 * consumes them and fails with gat_set_graph's codes and texts, leaving the context without a graph. */
enum { GAT_CSR_OK = 0, GAT_CSR_BAD_START = 1, GAT_CSR_BAD_END = 2, GAT_CSR_NOT_MONOTONE = 3, GAT_CSR_COL_RANGE = 4 };
int gat_graph_check_device(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, int64_t n_edges, int64_t n_table,
                           int32_t* problem, int64_t* where, void* stream);

/* ---- parameters (Xavier init E:186-248; flat layouts E:1242-1258) ---------------------------
 * GAT_PARAM_WRES flat [l][H_l*D_l][F_l] and GAT_PARAM_B flat [l][H_l*D_l] exist on a context with gat_set_residual (see
 * "residual" below); with their flag off the group's count is 0 and a set / get of 0 floats is a no-op that succeeds.
 * GAT_PARAM_LN_G / GAT_PARAM_LN_B, each flat [l][H_l*D_l] over all L layers, exist on a context with gat_set_norm (see "layer
 * normalisation" below) and sit behind the other five; off, their counts are 0 as well.
 * GAT_PARAM_WE flat [l][H_l*D_l][Fe] exists on a context with gat_set_edge_dim(Fe > 0) (see "edge features" below) and sits behind
 * the other six; with edge_dim == 0 its count is 0. */
enum { GAT_PARAM_W = 0, GAT_PARAM_A = 1, GAT_PARAM_WO = 2, GAT_PARAM_WRES = 3, GAT_PARAM_B = 4, GAT_PARAM_LN_G = 5, GAT_PARAM_LN_B = 6, GAT_PARAM_WE = 7 };
/* the two norm groups under the name a batch-norm context reads them by (gat_set_batch_norm: the same groups, not new ones) */
enum { GAT_PARAM_NORM_G = GAT_PARAM_LN_G, GAT_PARAM_NORM_B = GAT_PARAM_LN_B };
int gat_param_count(gat_ctx* ctx, int group, int64_t* count);
/* U(-lim,lim], lim as E:208, 236.  With GAT_RES_LINEAR: Wres_l Xavier-uniform with lim = sqrt(6 / (F_l + H_l*D_l)), drawn from the same
 * counter stream AFTER all existing draws (layer by layer), so W, a and Wo of a seed are those of a context without it; b = 0.
 * With gat_set_norm: gamma = 1, beta = 0, no draws.  With gat_set_edge_dim: We_l Xavier-uniform with lim = sqrt(6 / (Fe + H_l*D_l)), drawn
 * after every other draw (after Wres), so all other groups of a seed are unchanged.
 * With gat_set_head_hidden(width > 0): Wo is drawn at its own place with its new shape [C][Dh], so the draws BEHIND it (Wres, We) shift on
 * such a context — W and a of a seed stay what they are; W1 is drawn after every other draw, b1 = 0 (see "hidden layer" below). */
int gat_params_init(gat_ctx* ctx, uint64_t seed);
int gat_params_set(gat_ctx* ctx, int group, const float* host, int64_t count);
int gat_params_get(gat_ctx* ctx, int group, float* host, int64_t count);
int gat_grads_get(gat_ctx* ctx, int group, float* host, int64_t count);
int gat_grads_set(gat_ctx* ctx, int group, const float* host, int64_t count);
/* Device address of the packed gradient buffer [gradW | grada | gradWo | gradWres | gradb | gradgamma | gradbeta | gradWe] (for the all-reduce;
 * groups 3 and 4 only with gat_set_residual, 5 and 6 only with gat_set_norm, 7 only with gat_set_edge_dim).  count = n_params, the sum of the eight group counts (ten with gat_set_head_hidden: gradW1 | gradb1 behind gradWe); the three-float result tail of
 * gat_result_export sits behind it, and the host transport's bytes_per_rank rule stays (n_params + 3) * 4. */
int gat_grads_device(gat_ctx* ctx, void** d_ptr, int64_t* count);
/* Async D2D copies of the packed gradients on the context's stream, to / from a caller-owned
 * device buffer of `count` floats (the buffer the host all-reduces). */
int gat_grads_export(gat_ctx* ctx, void* d_dst, int64_t count);
int gat_grads_import(gat_ctx* ctx, const void* d_src, int64_t count);
/* Async: the last gat_head_forward's results as three floats at d_dst3 — [loss_sum (E:542),
 * n_correct & 4095, n_correct >> 12] — so the host can append them to the packed gradients and
 * sum everything over shards in ONE float all-reduce, with no mid-step device sync
 * (n_correct = lo + 4096*hi after the sum; exact). */
int gat_result_export(gat_ctx* ctx, void* d_dst3);

/* ---- the step (world == 1): epoch body E:1374-1557 ------------------------------------------- */
/* forward over all layers + output head + loss; returns sum loss (E:542) and #correct (E:543). */
int gat_forward(gat_ctx* ctx, float* loss_sum, int32_t* n_correct);
int gat_backward(gat_ctx* ctx);                   /* E:1463-1557; adds into the grad buffers */
int gat_zero_grad(gat_ctx* ctx);                  /* E:1631-1637 */
int gat_clip(gat_ctx* ctx, float threshold);      /* clip_grad_norm x3, E:1561-1567 */
int gat_step_sgd(gat_ctx* ctx, float lr);         /* E:1601-1624 */
int gat_step_adam(gat_ctx* ctx, float lr, float beta1, float beta2, float eps, int32_t t);  /* E:1571-1596 */

/* ---- the step in phases (any world size; the host runs the exchange between phases) ---------
 * forward, layer l:  project -> [all-gather PL table] -> forward_edges
 * backward, layer l: backward_edges -> [reduce-scatter gPL table] -> backward_dense
 * after the last backward phase: [all-reduce packed grads, loss scalars]. */
int gat_layer_project(gat_ctx* ctx, int32_t layer);         /* W_l·x / W_r·x parts of E:1386, 1416 */
int gat_layer_forward_edges(gat_ctx* ctx, int32_t layer);   /* E:1386, 1398, 1407, 1416, 1428 */
int gat_head_forward(gat_ctx* ctx, float* loss_sum, int32_t* n_correct);   /* E:1446, 1457, 1460 */
int gat_head_backward(gat_ctx* ctx);                        /* E:1468 */
int gat_layer_backward_edges(gat_ctx* ctx, int32_t layer);  /* E:1489, 1503 + edge parts of 1517, 1533 */
int gat_layer_backward_dense(gat_ctx* ctx, int32_t layer);  /* dense parts of E:1517, 1533; E:1546 */
/* *needed = 1 if the host must run the PL all-gather / gPL reduce-scatter for this layer
 * (0 for a single shard, and for layer 0 of a shard with replicated input). */
int gat_layer_exchange(gat_ctx* ctx, int32_t layer, int32_t* needed);

/* ---- exchanges inside the library (optional; the alternative to driving the phases yourself) ----
 * With a transport attached, gat_forward / gat_backward / gat_step accept a sharded context and run
 * the exchanges on the context's stream: all-gather of PL / reduce-scatter of gPL for every layer
 * with gat_layer_exchange() == 1, and one all-reduce of the packed gradients at the end of the
 * backward.  gat_forward then returns the GLOBAL loss sum and #correct (a 3-float all-reduce), so
 * every rank prints the same numbers and takes the same optimizer step.
 *   rccl : RCCL over xGMI; librccl is dlopen'ed here, not at library load.  Rank 0 obtains the id
 *          (gat_comm_unique_id) and the HOST ships its GAT_COMM_ID_BYTES to the other ranks.
 *   host : staged through POSIX shared memory `shm_name` (rank 0 creates it); bytes_per_rank >=
 *          n_table*max(H*D)*4 and >= (n_params+3)*4.  For tests (ranks sharing one GPU) and boxes
 *          without peer links; sums in ascending rank order. */
#define GAT_COMM_ID_BYTES 128
int gat_comm_unique_id(void* id_out);
int gat_comm_init_rccl(gat_ctx* ctx, int32_t world, int32_t rank, const void* id);
int gat_comm_init_host(gat_ctx* ctx, int32_t world, int32_t rank, const char* shm_name, int64_t bytes_per_rank);
/* Options of the exchanges run by the library (any transport).
 *   GAT_COMM_GPL_BF16 = 1: in the gPL reduce-scatter the REMOTE partial sums travel as bf16 (half the xGMI volume of the
 *   backward exchange); each rank keeps its own partial in fp32 and adds the arrivals in fp32, in ascending rank order.
 *   Default 0 (fp32 on the wire).  Gradients then differ from the fp32 exchange by ~2^-9 relative per remote term: the
 *   parity bar of this mode is 1e-2 (like bf16 storage).
 *   GAT_COMM_PIPELINE = K (1..64, default 1): the forward exchange of a layer runs in K row chunks on a second stream,
 *   chunk k travelling while chunk k+1 is projected; results are bitwise those of K = 1.
 *   GAT_COMM_HALO = 0 | 1 | 2 (default 0): the table exchanges move only the rows the receiving shard's edges reference
 *   (the rows the reference reads per edge, E:287-290 / E:407-409, and adds into, E:868-869) instead of whole slices: per
 *   peer one packed send / receive pair forward, its mirror backward, the own slice summed in ascending rank order.  1 = on,
 *   2 = on if fewer than half of the rows of a full exchange would travel (a halo costs a pack and an unpack pass on each side).
 *   COLLECTIVE: every rank of the transport makes the call (the request lists are exchanged once, here).  Results equal those of
 *   the full exchange value for value on the host transport; excludes GAT_COMM_GPL_BF16; GAT_COMM_PIPELINE is ignored while on. */
enum { GAT_COMM_GPL_BF16 = 1, GAT_COMM_PIPELINE = 2, GAT_COMM_HALO = 3 };
int gat_comm_option(gat_ctx* ctx, int32_t option, int32_t value);
/* What GAT_COMM_HALO set up: active (0/1), rows this rank receives / sends per forward table exchange (the backward is the mirror),
 * and rows on the wire / rows of the full exchange over all ranks (1.0 before the option was ever set).  Any pointer may be NULL. */
int gat_comm_halo_info(gat_ctx* ctx, int32_t* active, int64_t* rows_received, int64_t* rows_sent, double* referenced_fraction);
/* forward + backward without a host round-trip in between; with a transport the loss and #correct
 * ride in the tail of the gradient all-reduce.  Returns the global loss sum / #correct. */
int gat_step(gat_ctx* ctx, float* loss_sum, int32_t* n_correct);
/* enable = 1: gat_step captures its kernel sequence into a hipGraph (after one eager step) and replays it —
 * one launch per step instead of ~25; for graphs small enough to be launch-bound.  Single shard, no
 * transport, collect_timing = 0.  Results are those of the eager step, bit for bit. */
int gat_step_graph(gat_ctx* ctx, int32_t enable);
/* *state = 0 off, 1 armed (the next gat_step runs eagerly or captures), 2 captured (the next gat_step is a replay).  A call that re-arms a
 * captured step (gat_bind_table, a changed mask, replaced pairs, ...) takes 2 back to 1; gat_eval_mask, gat_eval_rank and gat_tap do not. */
int gat_step_graph_state(gat_ctx* ctx, int32_t* state);

/* Exchange buffers.  GAT_TABLE_PL: projected source features, [n_table][H_l*D_l] f32, the
 * context writes rows [table_row0, +n_rows) in gat_layer_project and reads all rows in the edge
 * phases.  GAT_TABLE_GPL: gradient wrt PL, same shape, the edge backward adds into ALL rows; after
 * the host's reduce-scatter rows [table_row0, +n_rows) must hold the summed values.
 * gat_table() returns the context's own buffer; gat_bind_table() substitutes a caller-owned one
 * (e.g. memory registered with the collective library). */
enum { GAT_TABLE_PL = 0, GAT_TABLE_GPL = 1 };
int gat_table(gat_ctx* ctx, int which, int32_t layer, void** d_ptr, int64_t* n_rows, int64_t* row_floats);
int gat_bind_table(gat_ctx* ctx, int which, int32_t layer, void* d_ptr, int64_t bytes);

/* ---- taps: intermediates converted to the reference layout, for parity tests -----------------
 * host_dst receives `count` floats (int32 for SRC/DST). */
enum {
    GAT_TAP_SRC = 0,        /* int32 [E]             d_src  (E:1186) */
    GAT_TAP_DST = 1,        /* int32 [E]             d_dst */
    GAT_TAP_ALPHA = 2,      /* [H][E]                attn_coeff[l] (E:381) */
    GAT_TAP_HPRE = 3,       /* [N][H][D]             d_h[l] (E:422) */
    GAT_TAP_HOUT = 4,       /* [N][H*D] | [N][D]     d_layer_outputs[l] (E:449, 456) */
    GAT_TAP_Y = 5,          /* [N][C]                d_y (E:508) */
    GAT_TAP_G = 6,          /* [N][H][D]             input_gradients[l] (E:601, 891).  The device keeps the factors of
                                                      E:598-603 / E:888-892 unapplied (the edge backward applies them on
                                                      load); the tap returns the reference's tensor */
    GAT_TAP_GE = 7,         /* [H][E]                grad_attn_score (E:693) */
    GAT_TAP_MAX = 8,        /* [H][N]                d_max_attn_score (E:356) */
    GAT_TAP_SUM = 9,        /* [H][N]                d_sum_score_exp (E:357) */
    GAT_TAP_PL = 10,        /* [n_table][H*D]        W_left·x  (the product's own intermediate) */
    GAT_TAP_PR = 11,        /* [N][H*D]              W_right·x */
    GAT_TAP_SCORE = 12,     /* [H][E]                attn_score[l] (E:323), keep_taps */
    GAT_TAP_GALPHA = 13,    /* [H][E]                grad_attn_coeff (E:646), keep_taps */
    GAT_TAP_GX = 14,        /* [N][F_l], l >= 1      input_gradients[l-1] as compute_features_input_gradients leaves
                                                      it (E:868-869), BEFORE the LReLU'(h_pre_{l-1}) factor of E:888-892
                                                      (with feature dropout: wrt the undropped x_l, i.e. incl. kappa*s_f) */
    GAT_TAP_ATTN_KEEP = 15, /* [H][E]                attention-dropout factor kappa*s_a (0 or s_a) of layer l for the step the
                                                      counter holds (after a training forward: the masks that forward used) */
    GAT_TAP_FEAT_KEEP = 16, /* [N][F_l]              feature-dropout factor kappa*s_f (0 or s_f) of layer l's input, likewise */
    GAT_TAP_EDGE_KEEP = 17, /* [E]                   DropEdge: 1 = CSR edge kept, 0 = dropped, for layer l and the step the counter
                                                      holds, likewise (all 1 at edge_p = 0; needs gat_set_dropedge or gat_set_dropout).  Like the two
                                                      taps above it reports the mask of the SETTING, whatever the mode: in eval mode the passes drop
                                                      nothing, the tap still shows what a training forward at that counter value draws */
    GAT_TAP_POOLED = 18,    /* [n_graphs][D_last]    the pooled rows the head reads (last layer only; needs gat_set_readout, see
                                                      "graph-level readout", where GAT_TAP_Y becomes [n_graphs][C]) */
    GAT_TAP_PAIRED = 19     /* [n_pairs][D_last]     the rows the head reads (last layer only; needs gat_set_pairs, see "pair head",
                                                      where GAT_TAP_Y becomes [n_pairs][C]) */
};
int gat_tap(gat_ctx* ctx, int tensor, int32_t layer, void* host_dst, int64_t count);

/* ---- dropout (beyond the reference, which has none; the GAT / GATv2 papers' regulariser) ----------------------------
 * Inverted dropout: a kept value is multiplied by s = 1/(1-p), a dropped one by 0.  Training mode only.
 *   Attention, p_a, every layer.  With kappa[e,h] in {0,1}:
 *       h_pre[n,h,:] = sum_{e->n} kappa[e,h] * s_a * alpha[h,e] * PL[src_e]
 *     The softmax statistics (max, sum) and alpha are unchanged.  Backward: ge = alpha * (galpha - sum alpha*galpha) with
 *     galpha[e,h] = kappa * s_a * <g, PL[src_e]>, and sum_e alpha*galpha is still <g, h_pre>; the source-side message is
 *     g * (kappa*s_a*alpha) + ge * a * LReLU'(s).  The per-edge records / message rows carry kappa*s_a*alpha in place of alpha,
 *     so the source-major pass is unchanged.
 *   Features, p_f, the input of every layer (layer 0 included): x'_l = x_l (.) kappa*s_f.  Both projections read x'_l and
 *     grad_W is formed from x'_l; the gradient passed to x_l is gx' (.) kappa*s_f, before the LReLU' factor of the layer below.
 *   The output head (W_o) has no dropout.  DropEdge (dropping edges before the softmax) is a different regulariser, not this:
 *   see "DropEdge" below.
 * Masks are stateless and counter-based (no mask is stored; the backward recomputes the forward's).  uint32 arithmetic, wrapping:
 *   fmix32(h): h ^= h>>16; h *= 0x85EBCA6B; h ^= h>>13; h *= 0xC2B2AE35; h ^= h>>16
 *   mix(k, v)  = fmix32(k ^ (v * 0x9E3779B9 + 0x7F4A7C15))
 *   K(kind, l) = mix(mix(mix(mix(lo32(seed), hi32(seed)), lo32(step)), hi32(step)), 2*l + kind)    kind 0 = feature, 1 = attention
 *   attention: r = mix(mix(mix(K(1,l), node(dst)), k), h)   k = j - row_ptr[dst], the edge's position in its CSR row (the same
 *              when a hub row is processed as 256-edge segments)
 *   feature:   r = mix(mix(K(0,l), node(row)), column)
 *   keep <=> (r >> 8) >= T,  T = min(2^24, floor(p * 2^24 + 0.5));  s = (float)(1.0 / (1.0 - (double)p))
 * node(.) is the row's id in the UNSHARDED graph: the row index on one GPU; on a destination-range shard table row t maps to
 * bounds[t / max_rows] + t % max_rows with the bounds given to gat_set_shard_bounds (without them: t).  Every rank then draws
 * the masks of a single GPU (padding rows take some id; their features are zero).
 * step is a 64-bit counter on the device.  A TRAINING forward advances it by one at its start, inside the layer-0 projection (a
 * one-lane kernel): gat_forward, gat_step, a gat_step_graph replay (the advance is part of the captured graph) and the phase API
 * (gat_layer_project(0)) alike.  The backward reads it without advancing, so it uses the masks of the forward before it.
 * Eval mode (gat_set_training(ctx, 0)): the model is the identity with respect to dropout and nothing advances.
 * p_a = p_f = 0 (the default, also when set explicitly) runs exactly the kernels of a context without dropout.  With dropout on,
 * each edge pass runs the attention-dropout instantiation of the kernel the default settings select, so the A/B switches of the
 * default path (GAT_ROWGROUP, GAT_PACKED, GAT_CPL, GAT_FWD_WAVES, GAT_GROUP_MSG, GAT_FUSE_LAST) do not apply; GAT_BWD_ATOMICS=1
 * (no store path) is refused with GAT_E_UNSUPPORTED at the backward, and so is dropout in the experiment library with GAT_DBG set.
 * keep_taps = 1: GAT_TAP_ALPHA stays the softmax alpha, GAT_TAP_GALPHA is dL/dalpha (incl. kappa*s_a).  bf16 storage: the
 * masks and their factors are the same; PL rows are bf16 as without dropout.  Transports (host, RCCL, halo) are unaffected:
 * masks are drawn where the rows live, never exchanged. */
/* feat_p, attn_p in [0, 1) (else GAT_E_INVALID, NaN included); seed keys every mask; the counter is set to first_step (a run that
 * starts from step 5 repeats steps 5, 6, ... of a run that started from 0).  Allowed before the graph is set. */
int gat_set_dropout(gat_ctx* ctx, float feat_p, float attn_p, uint64_t seed, uint64_t first_step);
int gat_set_training(gat_ctx* ctx, int32_t training);           /* 1 = training (default), 0 = eval */
int gat_dropout_step(gat_ctx* ctx, uint64_t* step);             /* the counter's value (synchronises; 0 before gat_set_dropout) */
/* Shard bounds [world+1] (global row boundaries, bounds[0] = 0): node ids of the table rows for the masks.  Checked against
 * n_table (= world slices of max_rows), table_row0 and n_rows; call after the graph is set. */
int gat_set_shard_bounds(gat_ctx* ctx, int32_t world, const int64_t* bounds);

/* ---- DropEdge (Rong et al., ICLR 2020; beyond the reference): whole edges leave the neighbourhood, per step ------------------
 * Training mode only.  For layer l every CSR edge j of destination row dst is kept or dropped AS A WHOLE (all heads at once).
 * A dropped edge takes no part in the row's max, in Z, in alpha, in the aggregation or in any gradient: its alpha is exactly 0,
 * and it sends nothing to PL[src], to PR[dst] or to a.  The surviving edges renormalise among themselves (attention dropout
 * zeroes a term AFTER the softmax and leaves alpha alone; an attention mask cannot emulate this, because Z would keep the
 * dropped terms).  No rescaling: the softmax over the survivors normalises itself.  A row whose edges are all dropped is, for
 * that step, a zero in-degree row: max = -1e9f, sum = 0, h_pre = 0 (E:336).  In other words the layer computes exactly what it
 * computes on the CSR with the dropped edges removed.
 * Composes with feature dropout (unchanged) and with attention dropout, which still keys its draw by the edge's position k in
 * the FULL CSR row (its masks do not depend on edge_p).
 * Mask: the hash of the dropout section, bit for bit.  With base = mix(mix(mix(lo32(seed), hi32(seed)), lo32(step)), hi32(step))
 * (the chain K(kind, l) starts with):
 *   K_e(l) = mix(base, 0x40000000 + l')     l' = l, or 0 for every layer with GAT_DROPEDGE_SHARED_LAYERS
 *   r      = mix(mix(K_e(l), node(dst)), k)  k = j - row_ptr[dst] (position in the whole row, also when a hub row is processed as
 *                                            256-edge segments); node(.) as for dropout (shard bounds respected)
 *   keep <=> (r >> 8) >= T(edge_p)           T(p) = min(2^24, floor(p * 2^24 + 0.5)), as for dropout
 * 2*l + kind never reaches 0x40000000 (l < 2^29), so K_e cannot collide with a feature or attention key.  One draw per edge,
 * not per head.  Destination-range shards own whole rows, so every rank draws the masks of a single GPU.
 *   GAT_DROPEDGE_KEEP_SELF      an edge whose col_idx equals table_row0 + row (a self-loop) is never dropped: with a self-looped
 *                               graph no row can go empty.  (The draw is still made; only its outcome is overridden.)
 *   GAT_DROPEDGE_SHARED_LAYERS  one mask per step for all layers (the DropEdge paper's default); without it the layers draw
 *                               independently.
 * edge_p in [0, 1), else GAT_E_INVALID (NaN included); unknown flag bits: GAT_E_INVALID.  Allowed before the graph is set.  Seed
 * and step counter are those of gat_set_dropout (call it with both p = 0 to seed only; without it the seed is 0 and the counter
 * starts at 0); gat_set_dropedge does not touch the counter.  With edge_p > 0 a training forward advances the counter exactly as
 * dropout does (same one-lane kernel, same place, part of a captured graph) — ONCE per forward, whichever of the three
 * regularisers are on.  Eval mode (gat_set_training(ctx, 0)) drops nothing and advances nothing.
 * edge_p = 0 (the default, also when set explicitly) runs exactly the kernels a context without DropEdge runs.  Otherwise the
 * edge passes run their DROP instantiations (the same ones attention dropout selects), with their rules: the A/B switches of the
 * default path do not apply, GAT_BWD_ATOMICS=1 gives GAT_E_UNSUPPORTED at the backward, and so does the experiment library with
 * GAT_DBG set.  In the backward a dropped edge leaves an all-zero record / message row in its source-major slot, so the
 * source-major passes (list, slot-parallel, halo) are unchanged.
 * Taps (keep_taps = 1): GAT_TAP_ALPHA, GAT_TAP_GE and GAT_TAP_GALPHA are exactly 0 at dropped edges; GAT_TAP_SCORE may hold
 * anything there.  GAT_TAP_MAX / GAT_TAP_SUM are those of the surviving edges.
 * gat_algorithmic_bytes* keep pricing the FULL graph (every edge's index is read, every slot is written; the gathers a dropped
 * edge would not need are not subtracted). */
enum { GAT_DROPEDGE_KEEP_SELF = 1, GAT_DROPEDGE_SHARED_LAYERS = 2 };
int gat_set_dropedge(gat_ctx* ctx, float edge_p, int32_t flags);

/* ---- residual connections and per-layer bias (beyond the reference; GATv2 of the paper / PyG's GATv2Conv has both) ------------
 * With flags != 0 every layer l computes
 *     h_pre[n,h,d] = sum_{e->n} kappa*s_a*alpha[h,e] * PL[src_e][h,d]        (as without the feature, all regularisers included)
 *                  + sum_f Wres_l[h*D+d][f] * x'_l[n][f]                      GAT_RES_LINEAR
 *                  + b_l[h*D+d]                                               GAT_RES_BIAS
 * x'_l is the layer's input after feature dropout: the tensor both projections read.  Everything downstream of h_pre is unchanged
 * (LeakyReLU, the hidden concatenation, the mean over heads of the last layer, the output head).  The score s = PL[src] + PR[dst]
 * does not see the residual, and the softmax statistics are untouched: a row without in-edges — also one DropEdge emptied, and a
 * padding row of a shard — keeps max = -1e9f, sum = 0 and has h_pre = Wres x' + b instead of 0.
 * Backward, with G = dL/dh_pre including the LReLU'(h_pre) factor:
 *     gradWres_l = G^T x'_l      gradb_l = sum_n G[n]      dL/dx'_l += G Wres_l
 * the last added to the two existing terms BEFORE the feature-dropout factor and before the LReLU' factor of the layer below;
 * layer 0 forms no input gradient, as always.
 * Where it runs.  Forward: R = x' Wres^T is a third projection over the shard's own rows (the three-bf16-piece product of the other
 *   two, K walked in chunks of 128), and R + b joins the row's sum in the row epilogue of the edge forward while the accumulator is
 *   on chip, before h_pre and hout are written once: whole rows in the wave-per-row / group-per-row kernels, split hub rows once in
 *   the fix-up kernel's combine, the generic kernel alike.  A residual context runs the DROP instantiations of the forward (the ones
 *   dropout selects) with nothing dropped and the two pointers in their argument struct, so the default-path A/B switches
 *   (GAT_ROWGROUP, GAT_PACKED, GAT_CPL, GAT_FWD_WAVES) do not apply to its forward.
 *   Backward: one N-sized kernel per layer forms G in fp32 into a buffer of its own, the aggregate agg = h_pre - (R + b), and
 *   fixed-order per-block column sums of G (finished by the deferred slab reduction: grad_b is bitwise reproducible, no float
 *   atomics).  The edge backward kernels and the source-major passes are unchanged: they take G and agg where they took g and h_pre
 *   (their <g, h_pre> stands for sum_e alpha*galpha, which holds for the aggregate alone), so the last layer's decision-byte pull
 *   form is not used.  gradWres and the G Wres term of grad_x run on the three-piece GEMM kernels (the second as an adding launch
 *   after the existing grad_x).  Extra device memory: R per layer and two [n_rows][max H*D] buffers.
 * gat_set_residual is allowed only BEFORE the first gat_params_*, gat_grads_*, gat_set_graph* call on the context (the packed
 *   parameter and gradient buffers change size): later it gives GAT_E_STATE.  Unknown flag bits: GAT_E_INVALID.  flags == 0 is the
 *   default and leaves the context exactly as it is: same buffers, same kernels, same launch counts, bitwise the same results.
 * Optimizer: gat_zero_grad, gat_step_sgd and gat_step_adam cover the new groups (Adam moments included); gat_clip clips every
 *   group on its own, as the reference clips its three (five norms with both flags).
 * Works with every (H, D) family incl. the generic path, bf16 storage (R, G and agg stay fp32), keep_taps, the phase API
 *   (gat_layer_project forms R, gat_layer_backward_edges runs the N-sized kernel first, gat_layer_backward_dense adds the two dense
 *   terms), gat_step, gat_step_graph replay, training masks, all three regularisers, and shards on any transport: the residual
 *   rows are the shard's own (with replicated layer-0 input: its own rows of the table), nothing more is exchanged, and the
 *   parameter-gradient all-reduce sums the new groups with the others.
 * Not with: the GAT_FUSE_LAST=1 experiment (a residual context runs the separate passes instead); GAT_DBG in the experiment
 *   library (gat_set_residual gives GAT_E_UNSUPPORTED); the gat_op_* seams stay residual-free.  GAT_TAP_G keeps returning
 *   g (.) LReLU'(h_pre), which IS G.
 * gat_algorithmic_bytes*: unchanged with flags == 0.  gat_algorithmic_bytes (the context form) adds per layer, at 4 bytes:
 *   project += N*HD (R written) + HD*F (Wres read), x' counted as read once more (N*F) with GAT_RES_LINEAR;
 *   edge_forward += N*HD (R read); misc += N*HD * (h_pre + g read, G + agg written, + R read with GAT_RES_LINEAR);
 *   grad_w += N*HD + N*F + HD*F (G, x', gradWres) and, l >= 1, grad_x += N*HD + 2*N*F + HD*F (G, gX read and written, Wres) with
 *   GAT_RES_LINEAR.  gat_algorithmic_bytes_shape has no context and prices the model without the feature. */
enum { GAT_RES_LINEAR = 1, GAT_RES_BIAS = 2 };
int gat_set_residual(gat_ctx* ctx, int32_t flags);

/* ---- layer normalisation between the aggregation and the activation (beyond the reference; PyG's GAT takes norm="layer") ------
 * With GAT_NORM_LAYER every layer l — with GAT_NORM_SKIP_LAST every layer but the last — computes, with u[n,c] = h_pre exactly as
 * without the feature (attention dropout, DropEdge, Wres x' and b included) and c = h*D + d over the HD = H_l*D_l channels of the row,
 *     mu[n]   = (1/HD) sum_c u[n,c]
 *     var[n]  = (1/HD) sum_c (u[n,c] - mu[n])^2          (biased; two passes over the on-chip row, not E[u^2] - mu^2)
 *     rstd[n] = 1 / sqrt(var[n] + eps)
 *     v[n,c]  = gamma_l[c] * (u[n,c] - mu[n]) * rstd[n] + beta_l[c]
 *     hout    = LReLU(v)      hidden layers: concatenated; last layer: mean over heads of LReLU(v), as E:440-457 does with h_pre
 * Everything upstream of u is unchanged: the score, the softmax statistics, alpha, and GAT_TAP_HPRE, which keeps returning u.
 * A row without in-edges (also one DropEdge emptied, and a padding row of a shard) has u = 0 without residual flags, hence v = beta and
 * hout = LReLU(beta); with residual flags u = Wres x' + b is normalised like any row.  H*D = 1 gives var = 0 and v = beta; nothing
 * becomes NaN or Inf for a finite u.
 * Backward, with xhat = (u - mu) * rstd and dv = dL/dhout (.) LReLU'(v) — dL/dhout being the hidden g written by grad_x, or gH / H of
 * the head; the factor is LReLU'(v), never LReLU'(h_pre), for every consumer of a normalised layer:
 *     grad_gamma_l[c] = sum_n dv[n,c] * xhat[n,c]        grad_beta_l[c] = sum_n dv[n,c]
 *     G[n,c] = rstd[n] * (dxh[n,c] - mean_c dxh[n,.] - xhat[n,c] * mean_c (dxh (.) xhat)[n,.]),   dxh = dv (.) gamma_l
 * and G = dL/dh_pre plays the role it plays in a residual context: the edge backward takes G and agg = u - (R + b),
 * gradWres = G^T x', grad_b = sum_n G, grad_x += G Wres.
 * Parameters: GAT_PARAM_LN_G and GAT_PARAM_LN_B, flat [l][H_l*D_l] over ALL L layers, behind the five other groups in the packed
 *   parameter, gradient and Adam buffers (gat_grads_device reports the new n_params; the result tail stays behind it).  With
 *   GAT_NORM_SKIP_LAST the last layer's entries exist, are never read, and their gradients are exactly 0.  gat_params_init sets
 *   gamma = 1, beta = 0 and makes no draws.  gat_zero_grad, gat_step_sgd and gat_step_adam cover the groups; gat_clip clips each by
 *   its own norm.
 * Where it runs.  Forward: in the row epilogue of the edge forward, after the residual term, before h_pre (still u) and hout are
 *   written once — whole rows in the wave-per-row / group-per-row kernels, split hub rows once in the fix-up kernel's combine, the
 *   generic kernel alike.  The two sums over the row's lanes are butterfly sums in a fixed order.  A norm context runs the DROP
 *   instantiations of the forward, like a residual context; gamma, beta and eps travel in their argument struct.  No N-sized forward
 *   kernel, no N-sized forward traffic; the default-path instantiations are untouched.
 *   Backward: one N-sized kernel per normalised layer in the residual kernel's place.  It reads u, the output gradient, R, b, gamma
 *   and beta, recomputes mu, rstd and v (the forward stores nothing extra), writes G and agg, and per-block fixed-order column sums for
 *   grad_gamma, grad_beta and (GAT_RES_BIAS) grad_b, finished by the slab reduction: no float atomics, bitwise reproducible on the
 *   fast families.  A norm context without residual flags takes the same route (agg = u).  Every H*D the generic path allows.
 *   Downstream is the code of a residual context; GAT_FUSE_LAST and the last layer's decision-byte pull form are not used.
 * Taps: GAT_TAP_HOUT returns LReLU(v); GAT_TAP_G returns G = dL/dh_pre of any layer, recomputed on the device from the layer's stored
 *   output gradient and h_pre by the backward kernel's row function.
 * gat_set_norm follows gat_set_residual's state rules: only BEFORE the first gat_params_*, gat_grads_*, gat_set_graph* call (later:
 *   GAT_E_STATE), before or after gat_set_residual.  Unknown flag bits, GAT_NORM_SKIP_LAST without GAT_NORM_LAYER, and — with
 *   flags != 0 — an eps that is not finite and > 0 (NaN included): GAT_E_INVALID.  flags == 0 ignores eps and leaves the context
 *   exactly as it is.  A context created with flat_lrelu_index = 1: GAT_E_UNSUPPORTED (the reference's flat index has no meaning on
 *   v); the experiment library with GAT_DBG set: GAT_E_UNSUPPORTED.
 * Works with every (H, D) family incl. both generic ones, bf16 storage (the norm arithmetic, G and agg stay fp32), keep_taps, the
 *   phase API (gat_layer_forward_edges normalises, gat_layer_backward_edges runs the N-sized kernel first), gat_step, gat_step_graph
 *   replay, training masks, eval mode, all three regularisers, and shards on any transport: statistics are row-local, nothing more
 *   is exchanged, and the parameter-gradient all-reduce sums the new groups.
 * gat_algorithmic_bytes (context form): unchanged with the feature off.  On, every layer is priced on the residual route (misc +=
 *   N*HD * 4 at 4 bytes without GAT_RES_LINEAR: u + g read, G + agg written — already counted in a residual context), and each
 *   normalised layer adds 2*HD floats of parameters per pass to misc.  gat_algorithmic_bytes_shape prices the model without it. */
enum { GAT_NORM_LAYER = 1, GAT_NORM_SKIP_LAST = 2 };
int gat_set_norm(gat_ctx* ctx, int32_t flags, float eps);

/* ---- batch normalisation between the aggregation and the activation (beyond the reference; DGL's OGB GAT baselines put
 *      BatchNorm1d(H*D) behind every hidden GATConv, the usual graph-classification stack normalises over all nodes of the batch) ----
 * With GAT_BN_ON every layer l — with GAT_BN_SKIP_LAST every layer but the last — computes, with u[n,c] = h_pre exactly as without
 * the feature (attention dropout, DropEdge, Wres x' and b included), c = h*D + d, and N = ALL n_rows rows of the context (whatever the
 * training mask says; the nodes of all graphs of a readout context; rows without in-edges included), in TRAINING mode
 *     mu[c]   = (1/N) sum_n u[n,c]
 *     var[c]  = (1/N) sum_n (u[n,c] - mu[c])^2        biased; formed by Welford / Chan merges, never as E[u^2] - mu^2
 *     rstd[c] = 1 / sqrt(var[c] + eps)
 *     xhat    = (u - mu) * rstd
 *     v       = gamma_l[c] * xhat + beta_l[c]
 *     hout    = LReLU(v)      hidden layers: concatenated; last layer: mean over heads (h ascending) of LReLU(v)
 *     running_mean_l = (1 - m) * running_mean_l + m * mu
 *     running_var_l  = (1 - m) * running_var_l  + m * var * N/(N-1)        (N == 1: var itself)
 * The running statistics start at 0 and 1 and advance once per training forward: gat_forward, gat_step, a replay of a captured step
 * graph (the update is one of its kernels), or gat_layer_forward_edges of the phase API.  They never advance in eval mode.
 * EVAL mode (gat_set_training(ctx, 0)): mu and rstd are replaced by running_mean and 1 / sqrt(running_var + eps); no statistics pass
 * runs and nothing advances.
 * Backward, with dv = dL/dhout (.) LReLU'(v) and dL/dhout what the layer-norm backward takes (g of a hidden layer, gH / H of the last):
 *     grad_beta_l[c]  += s1[c],  s1 = sum_n dv[n,c]
 *     grad_gamma_l[c] += s2[c],  s2 = sum_n dv[n,c] * xhat[n,c]
 *     G[n,c] = gamma_l[c] * rstd[c] * (dv[n,c] - s1[c]/N - xhat[n,c] * s2[c]/N)        training mode
 *     G[n,c] = gamma_l[c] * rstd[c] * dv[n,c]                                          eval mode (the statistics are constants)
 * G and agg = u - (R + b) then play the role they play on the residual route (edge backward, gradWres = G^T x', grad_b = sum_n G,
 * grad_x += G Wres).  Upstream of u nothing changes: score, softmax statistics, alpha, and GAT_TAP_HPRE, which keeps returning u.
 * Parameters: gamma and beta live in the two existing norm groups, GAT_PARAM_NORM_G / GAT_PARAM_NORM_B (= GAT_PARAM_LN_G / _LN_B), flat
 *   [l][H_l*D_l] over ALL layers, gamma = 1, beta = 0, no draws; with GAT_BN_SKIP_LAST the last layer's entries exist, are never read
 *   and their gradients are exactly 0.  The running statistics are NOT parameters: two device buffers [l][H_l*D_l] outside the packed
 *   buffers, which SGD, Adam, clip and zero_grad never touch.
 * Kernels: forward = statistics (one read of u: per-lane Welford, the block's row lanes and then the blocks merged in ascending order
 *   with Chan's formula) + a one-block finish (mu, rstd, the running update) + apply (hout; it overwrites the LReLU(u) the edge forward
 *   wrote); eval mode is the apply launch alone.  Backward = column sums of dv and dv * xhat + a one-block finish + apply (G, agg, the
 *   block partials of grad_b).  No float atomics; every sum runs in an order fixed by (N, H*D, grid): bitwise reproducible.  Plain
 *   launches on the context's stream, capturable, timed under GAT_K_MISC.
 * Taps: GAT_TAP_HOUT returns the normalised output; GAT_TAP_G returns G of any layer, recomputed through the two backward launches.
 * gat_set_batch_norm follows gat_set_norm's state rules: only BEFORE the first gat_params_*, gat_grads_*, gat_set_graph* call (later:
 *   GAT_E_STATE).  flags == 0 is the default: it ignores eps and momentum and leaves the context exactly as it is.  Unknown bits,
 *   GAT_BN_SKIP_LAST without GAT_BN_ON, an eps that is not finite and > 0, a momentum outside [0, 1] or not finite: GAT_E_INVALID.
 *   GAT_E_UNSUPPORTED: together with gat_set_norm(flags != 0) on the same context, in either order (the second call is refused);
 *   flat_lrelu_index = 1; the experiment library with GAT_DBG set; a destination-range shard (n_table != n_rows or table_row0 != 0:
 *   refused by the call that sets the graph) and gat_comm_init_* — the column statistics of a shard would need an exchange that is
 *   not built.
 * Works with every (H, D) family incl. both generic ones, bf16 storage (the arithmetic, G and agg stay fp32), keep_taps, the residual
 *   flags, the three regularisers, edge features, readout, pair head, hidden head, all three loss modes, training masks, the phase
 *   API, gat_step and its graph replay.
 * gat_algorithmic_bytes (context form): unchanged with the feature off.  On, every layer is priced on the residual route and each
 *   normalised layer adds to misc 3 * N*HD floats forward (u read twice, hout written) and 6 * N*HD backward (u and g read twice, G and
 *   agg written; R once more with GAT_RES_LINEAR) in place of the residual route's 4.  gat_algorithmic_bytes_shape prices the model
 *   without it. */
enum { GAT_BN_ON = 1, GAT_BN_SKIP_LAST = 2 };
int gat_set_batch_norm(gat_ctx* ctx, int32_t flags, float eps, float momentum);
int gat_batch_norm_info(gat_ctx* ctx, int32_t* flags, float* eps, float* momentum);
/* The statistics, flat [l][H_l*D_l] over all layers, count = sum_l H_l*D_l (a layer GAT_BN_SKIP_LAST leaves out keeps 0 / 1 / 0 / 0).
 * BATCH_MEAN / BATCH_RSTD: of the last training forward.  set: the two running vectors only (others: GAT_E_INVALID); it writes into
 * the same buffers, so a captured step graph stays valid.  Both on a context without batch norm: GAT_E_STATE. */
enum { GAT_BN_RUNNING_MEAN = 0, GAT_BN_RUNNING_VAR = 1, GAT_BN_BATCH_MEAN = 2, GAT_BN_BATCH_RSTD = 3 };
int gat_batch_norm_stats_get(gat_ctx* ctx, int32_t which, float* host, int64_t count);
int gat_batch_norm_stats_set(gat_ctx* ctx, int32_t which, const float* host, int64_t count);
/* The kernels on caller-owned device pointers (stateless; synchronises `stream` before it returns).
 * forward: u [n_rows][H*D].  training != 0: the statistics of u go to d_mean_rstd [2][H*D] = {mu, rstd} and, unless both are null,
 *   d_running_mean / d_running_var advance.  training == 0: d_running_mean / d_running_var are what is normalised with (null:
 *   GAT_E_INVALID), d_mean_rstd is not touched.  d_hout [n_rows][H*D], with is_last [n_rows][D].
 * backward: d_g [n_rows][H*D] or d_gh [n_rows][gh_stride] (first D floats of a row: the gradient of the mean over heads) is dL/dhout;
 *   training != 0 reads d_mean_rstd, training == 0 the running pair.  d_res / d_bias: R and b (null: none).  d_G, d_agg [n_rows][H*D]
 *   (d_agg null: not written); d_grad_gamma / d_grad_beta / d_grad_b [H*D] are ADDED into (null: not formed). */
int gat_op_batch_norm_forward(const float* d_u, int64_t n_rows, int32_t H, int32_t D, int32_t is_last, const float* d_gamma,
                              const float* d_beta, float eps, float slope, float momentum, float* d_running_mean, float* d_running_var,
                              int32_t training, float* d_mean_rstd, float* d_hout, void* stream);
int gat_op_batch_norm_backward(const float* d_u, const float* d_g, const float* d_gh, int64_t gh_stride, int64_t n_rows, int32_t H, int32_t D,
                               const float* d_gamma, const float* d_beta, const float* d_mean_rstd, const float* d_running_mean,
                               const float* d_running_var, float eps, float slope, int32_t training, const float* d_res, const float* d_bias,
                               float* d_G, float* d_agg, float* d_grad_gamma, float* d_grad_beta, float* d_grad_b, void* stream);

/* ---- edge features in the attention score (beyond the reference; the `edge_dim` argument of PyG's GATv2Conv) ----------------------
 * With edge_dim = Fe > 0 every layer l has a parameter We_l, flat [H_l*D_l][Fe], and every CSR edge j of the context's graph an
 * attribute row EA[j] ([E][Fe], fp32, in the order of the context's CSR: the order gat_graph_get returns).  With dst the row of edge j:
 *     PE_l[j][c]  = sum_f We_l[c][f] * EA[j][f]
 *     s[j][c]     = PL[src_j][c] + PR[dst][c] + PE_l[j][c]
 *     score[j][h] = sum_d a[h,d] * LReLU(s[j][h,d])
 * The softmax, alpha, the aggregation, the residual, the norm and the head are as without it: the MESSAGE STAYS PL[src] (as in PyG),
 * the edge term is in the score only.  The same EA serves every layer.  Rows without in-edges are unaffected.
 * Backward, with ge = dL/dscore as without the feature:
 *     gs[j][c] = ge[j][h] * a[c] * LReLU'(s[j][c])      gPL[src] += gs + g * kappa*s_a*alpha      gPR[dst] += gs      ga += ge * LReLU(s)
 *     gPE_l[j] = gs[j]                                   gradWe_l += gPE_l^T EA
 * LReLU and LReLU' take the new s wherever they appear.  EA is an input: it gets no gradient.  A DropEdge-dropped edge has gPE[j] = 0;
 * attention dropout leaves gPE as the formula gives it (ge already contains kappa).
 * gat_set_edge_dim follows gat_set_residual's state rules: only BEFORE the first gat_params_*, gat_grads_*, gat_set_graph* call (later:
 *   GAT_E_STATE), in any order with gat_set_residual / gat_set_norm.  edge_dim < 0 or > GAT_EDGE_DIM_MAX: GAT_E_INVALID.  0 is the
 *   default and leaves the context exactly as it is: same buffers, same kernels, same launch counts, bitwise the same results.  The
 *   experiment library with GAT_DBG set: GAT_E_UNSUPPORTED.
 * gat_set_edge_features[_device] is called AFTER the graph is set (before: GAT_E_STATE); n_edges and edge_dim must be the context's
 *   (GAT_E_INVALID otherwise; with edge_dim == 0 on both sides the call does nothing).  The array is copied (rows padded to a multiple of 4 floats with
 *   zeros) and may be replaced by a later call.  A step / phase call on a context with edge_dim > 0 and no edge features set gives
 *   GAT_E_STATE and says so.  After gat_set_graph_coo* the rows are still "in the order of gat_graph_get": carrying attributes through
 *   GAT_GRAPH_SYMMETRIZE / SELF_LOOPS / COALESCE (PyG's fill_value) is the caller's business and out of scope.
 * Parameters: GAT_PARAM_WE, flat [l][H_l*D_l][Fe], behind the seven other groups in the packed parameter, gradient and Adam buffers
 *   (gat_grads_device reports the new n_params; the three-float result tail stays behind it; the host transport's
 *   (n_params + 3) * 4 rule holds with the new n_params).  gat_zero_grad, gat_step_sgd and gat_step_adam cover it; gat_clip clips it by
 *   its own norm.
 * Where it runs.  PE_l = EA We_l^T is a fourth dense product of gat_layer_project (the three-bf16-piece kernels of the residual term,
 *   rows = E, K = Fe), kept per layer in fp32 also under bf16 storage (it is streamed, never gathered).  Both edge passes run the PE
 *   instantiations of their extended kernels (EXT forward, DROP backward; without an active mask at T = Te = 0, scale = 1): per edge
 *   one more row load PE[j] at a CSR-contiguous address next to the PL[src] gather, and in the backward one streamed row store
 *   gPE[j] = gs into a single [E][max H*D] fp32 buffer shared by the layers.  gat_layer_backward_dense adds gradWe_l = gPE^T EA (the
 *   grad_W kernels on one half).  The fix-up kernels and the source-major passes are unchanged: the per-edge records / message rows
 *   already carry the LReLU'(s) decisions.  Destination-range shards: an edge's attributes belong to the destination shard's own CSR,
 *   nothing more is exchanged, and the packed all-reduce sums the new group.  Computing PE inside the edge kernels is out of scope.
 *   Extra device memory: (L + 1) * E * HD * 4 bytes at equal HD (PE per layer + gPE), plus E * ld * 4 for EA (ld = Fe rounded up to 4).
 * Works with every (H, D) family incl. both generic ones, bf16 storage, keep_taps (GAT_TAP_SCORE includes the edge term), the phase
 *   API (project forms PE_l, backward_edges writes gPE, backward_dense adds gradWe_l), gat_step, gat_step_graph replay, training
 *   masks, eval mode, all three regularisers, residual, bias, norm, and shards on any transport.
 * Not with: GAT_FUSE_LAST=1 and the last layer's decision-byte pull form (such a context runs the separate passes and gathers g rows,
 *   as a residual context does); GAT_BWD_ATOMICS=1 (GAT_E_UNSUPPORTED at the backward, as with dropout).  The gat_op_* seams stay
 *   edge-feature-free.
 * gat_algorithmic_bytes (context form): unchanged with the feature off.  On, per layer at 4 bytes:
 *   project += E*Fe + HD*Fe + E*HD; edge_forward += E*HD; edge_backward += 2*E*HD; grad_w += E*HD + E*Fe + HD*Fe.
 *   gat_algorithmic_bytes_shape prices the model without it.  At the Products shape and HD = 64 the step's bytes roughly double: the
 *   price of a dense per-edge term. */
#define GAT_EDGE_DIM_MAX 64
int gat_set_edge_dim(gat_ctx* ctx, int32_t edge_dim);
int gat_set_edge_features(gat_ctx* ctx, const float* ea, int64_t n_edges, int32_t edge_dim);              /* [n_edges][edge_dim], host */
int gat_set_edge_features_device(gat_ctx* ctx, const float* d_ea, int64_t n_edges, int32_t edge_dim);    /* the same, device pointer */

/* ---- graph-level readout (beyond the reference, which has one label per node; PyG's global_add_pool / global_mean_pool / global_max_pool) ----
 * Many small graphs packed block-diagonally into one CSR, ONE label per graph.  Graph g owns the contiguous rows
 * [graph_ptr[g], graph_ptr[g+1]) — the `ptr` of a PyG Batch; a sorted `batch` vector is the same information.  With X = the last layer's
 * output ([n_rows][D_last], after the mean over heads) and cnt_g the row count of graph g:
 *     GAT_READOUT_SUM   P[g][d] = sum_n X[n][d]                      dL/dX[n][d] = gP[g][d]
 *     GAT_READOUT_MEAN  P[g][d] = (sum_n X[n][d]) / (float)cnt_g     dL/dX[n][d] = gP[g][d] / (float)cnt_g
 *     GAT_READOUT_MAX   P[g][d] = max_n X[n][d]                      dL/dX[n][d] = gP[g][d] if n == argmax[g][d], else 0
 * argmax is the LOWEST row attaining the maximum.  An empty graph (cnt_g == 0) has P[g] = 0 in every mode, argmax -1, and sends no
 * gradient.  The output head runs unchanged on P with n_graphs rows where it had n_rows: z = P Wo^T, the reference's softmax and loss
 * (E:132-141, E:514-537), dz = y - onehot, gradWo += dz^T P, gP = dz Wo.  Wo keeps its shape [C][D_last]: no parameter group changes
 * size.  Labels, the training mask, gat_eval_mask, GAT_TAP_Y, loss_sum and n_correct are all PER GRAPH.  Everything from dL/dX downward
 * is the code of a context without readout (the / H and LReLU' expansion in the last layer's edge backward, the residual and norm kernels).
 * gat_set_readout[_device] is called AFTER the graph is set and BEFORE the labels (else GAT_E_STATE: the label, mask and head buffers are
 *   sized by it), at most once with a non-zero mode (a second one: GAT_E_STATE).  mode == 0 (GAT_READOUT_NONE) is the default and leaves the
 *   context exactly as it is: same buffers, same kernels, same launch counts, bitwise the same results (the other arguments are not read).
 *   mode outside 0..3: GAT_E_INVALID.  n_graphs >= 1 and must fit int32.  graph_ptr [n_graphs + 1] must start at 0, end at n_rows and never
 *   decrease, else GAT_E_INVALID with a text naming the lowest offending index (0; n_graphs; the i with graph_ptr[i+1] < graph_ptr[i]).
 *   The device form checks its argument in one pass on the device before anything walks it (as gat_graph_check_device does).  The array
 *   is copied.
 * With readout on, gat_set_labels[_device], gat_set_train_mask and gat_eval_mask take n_graphs where they took n_rows (another length:
 *   GAT_E_INVALID); gat_eval_mask's n_nodes counts graphs.
 * Where it runs.  Forward: a work list built once (a graph of at most 256 rows is one item, a longer one is cut into 256-row segments); one
 *   wave per item streams the item's contiguous rows — float4 loads with D_last / 4 lanes per row and the other lanes on the next rows when
 *   D_last is a multiple of 4, scalar loads otherwise, any D_last >= 1 — and combines its row slots by a fixed-order butterfly; the
 *   segments of a long graph leave partial rows that a second small kernel combines in ascending order.  Backward: one N-sized elementwise
 *   kernel that writes the first D_last floats of every row of the head's gradient buffer (all rows, zeros included).  No float atomics:
 *   bitwise reproducible.  The two launches are part of gat_head_forward (which pools first) and gat_head_backward (which ends with the
 *   un-pool), of gat_forward / gat_backward, gat_step and a gat_step_graph replay (no host synchronisation), and are timed under
 *   GAT_K_HEAD_FWD / GAT_K_HEAD_BWD.
 * Works with every (H, D) family incl. both generic ones, bf16 storage (pooling and the head stay fp32), keep_taps, eval mode, all three
 *   regularisers, residual, bias, norm and edge features.
 * Refused with GAT_E_UNSUPPORTED: a destination-range shard (n_table != n_rows) or a context with a transport (a graph may straddle shards;
 *   gat_comm_init_* on a readout context is refused alike); flat_lrelu_index = 1 (the head would write the last layer's g itself); the
 *   experiment library with GAT_DBG set.  GAT_FUSE_LAST=1 is not used by a readout context: it runs the separate passes.
 * gat_set_graph_coo* keeps the row order, so a caller's graph_ptr stays valid after a build; it is not carried through by the library.
 * gat_algorithmic_bytes (context form): unchanged with readout off.  On, the head classes are priced with n_graphs rows, and misc gains
 *   4 * (N*D_last + G*D_last) for the pool and 4 * (G*D_last + N*D_last) for the un-pool.  gat_algorithmic_bytes_shape has no context and
 *   prices the model without the feature. */
enum { GAT_READOUT_NONE = 0, GAT_READOUT_MEAN = 1, GAT_READOUT_SUM = 2, GAT_READOUT_MAX = 3 };
int gat_set_readout(gat_ctx* ctx, int32_t mode, const int32_t* graph_ptr, int64_t n_graphs);            /* host graph_ptr[n_graphs+1] */
int gat_set_readout_device(gat_ctx* ctx, int32_t mode, const int32_t* d_graph_ptr, int64_t n_graphs);   /* checked on the device */
int gat_readout_info(gat_ctx* ctx, int32_t* mode, int64_t* n_graphs);                                   /* (0, 0) while off; pointers may be NULL */
/* The two kernels as stateless seams on caller-owned DEVICE pointers (current device), like the gat_op_* below: d_x rows of x_stride >=
 * width floats, d_pooled [n_graphs][width], d_argmax [n_graphs][width] int32 (GAT_READOUT_MAX only, else may be NULL); the backward writes
 * floats 0..width-1 of every d_gh row (gh_stride >= width floats apart) and nothing behind them.  Each call checks d_graph_ptr with
 * gat_set_readout's rules (same codes and texts) before any kernel reads through it, builds its work list, allocates and frees its scratch,
 * and synchronises `stream` (may be NULL): parity seams, not the fast path. */
int gat_op_readout_forward(const float* d_x, int64_t x_stride, const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows,
                           int32_t width, int32_t mode, float* d_pooled, int32_t* d_argmax, void* stream);
int gat_op_readout_backward(const float* d_gpooled, const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t width,
                            int32_t mode, const int32_t* d_argmax, float* d_gh, int64_t gh_stride, void* stream);

/* ---- pair head (beyond the reference, which has one label per node: link prediction, edge classification, edge regression) ----
 * ONE label per pair of nodes.  A list of pairs (u_p, v_p), p = 0 .. P-1, both rows of the context; they need not be edges of the graph
 * (negatives are not).  With X = the last layer's output ([n_rows][D_last], after the mean over heads) the head's input rows are
 *     GAT_PAIR_MUL   Q[p][d] = X[u_p][d] * X[v_p][d]      dL/dX[n][d] = sum over incidences (p, role) of n:  gQ[p][d] * X[other(p, role)][d]
 *     GAT_PAIR_ADD   Q[p][d] = X[u_p][d] + X[v_p][d]      dL/dX[n][d] = sum over incidences (p, role) of n:  gQ[p][d]
 * An incidence of node n is a pair with u_p == n (role 0, other = v_p) or v_p == n (role 1, other = u_p).  A pair with u_p == v_p is two
 * incidences of the same node (the gradient of x*x is 2 x gQ, no special case); duplicate pairs are legal and count separately.
 * The output head runs unchanged on Q with P rows where it had n_rows: z = Q Wo^T, the context's loss mode, gradWo += dz^T Q, gQ = dz Wo.
 * Wo keeps its shape [C][D_last]: no parameter group changes size.  With C = 1, BCE and Wo fixed at ones this is GAE's dot-product
 * decoder; with C > 1 a DistMult-style relation scorer or an edge classifier; MSE gives edge regression.  Labels, targets, the training
 * mask, gat_eval_mask, gat_target_count, GAT_TAP_Y, loss_sum and n_correct are all PER PAIR; the train / validation / test pair sets of a
 * link-prediction run are one pair list with masks over it.  Everything from dL/dX downward is the code of a context without the feature.
 * gat_set_pairs[_device]: the first call comes AFTER the graph is set and BEFORE the labels or targets (else GAT_E_STATE: the head buffers
 *   are sized by P).  mode == 0 (GAT_PAIR_NONE) is the default and leaves the context exactly as it is: same buffers, same kernels, same
 *   launch counts, bitwise the same results (the other arguments are not read).  mode outside 0..2: GAT_E_INVALID.
 *   A later call with the same non-zero mode and the same n_pairs REPLACES the pairs (negatives resampled per epoch): the values go into
 *   the same device buffers, the incidence index and the work list are rebuilt, and a captured gat_step_graph is re-armed as by
 *   gat_bind_table (the work list changes: the next step runs eagerly, the one after captures again).  Another mode or n_pairs: GAT_E_STATE.
 *   1 <= n_pairs < 2^30 (the incidence keys 2p + role go through the 32-bit graph builder), more: GAT_E_UNSUPPORTED; n_pairs < 1:
 *   GAT_E_INVALID.  A u or v outside [0, n_rows): GAT_E_INVALID, "pair <p> has u|v <value> outside [0, n_rows)" for the lowest offending
 *   pair (u before v).  The device form finds this in one pass on the device before any kernel reads through the arrays (as
 *   gat_graph_check_device does); on failure the context keeps the pairs it had.  The arrays are copied.
 * With a pair head, gat_set_labels[_device], gat_set_targets[_device], gat_set_train_mask, gat_eval_mask and gat_target_count take
 *   n_pairs where they took n_rows (another length: GAT_E_INVALID, the text says "one per pair"); gat_eval_mask's n_nodes counts pairs.
 * Where it runs.  Forward: a pair takes LPR lanes (float4 loads when D_last is a multiple of 4, scalar loads otherwise, any D_last >= 1),
 *   a wave's other lane groups take the next pairs; two gathered rows in, one contiguous row of Q out, one fp32 operation per entry.
 *   Backward: a node-major PULL over an incidence index — a CSR over the nodes with every node's entries {p, other} in ascending
 *   2p + role, built on the device at gat_set_pairs* by the graph builder's sort — so that every row of the head's gradient buffer is
 *   written exactly once by one wave (zeros included), with no float atomics: bitwise reproducible, a function of the pair list alone.  A
 *   node of at most 256 incidences is one work item, a longer one is cut into 256-entry segments whose partial rows a second small kernel
 *   adds in ascending order.  The launches are part of gat_head_forward (which gathers first) and gat_head_backward (which ends with the
 *   scatter), of gat_forward / gat_backward, gat_step and a gat_step_graph replay (no host synchronisation), timed under GAT_K_HEAD_FWD /
 *   GAT_K_HEAD_BWD.  GAT_TAP_PAIRED returns Q.
 * Works with every (H, D) family incl. both generic ones, bf16 storage (X, Q, gQ and the head's gradient stay fp32), keep_taps, eval
 *   mode, all three regularisers, residual, bias, norm, edge features and all three loss modes.
 * Refused with GAT_E_UNSUPPORTED: a destination-range shard (n_table != n_rows) or a context with a transport (an endpoint may live on
 *   another shard; gat_comm_init_* on a pair context is refused alike); flat_lrelu_index = 1; the experiment library with GAT_DBG set; a
 *   pair head with a readout (whichever of the two is set second).  GAT_FUSE_LAST=1 is not used by a pair context.
 * gat_algorithmic_bytes (context form): unchanged with the feature off.  On, the head classes are priced with P rows, and misc gains, at
 *   4 bytes: forward 2P (indices) + 2 P D_last (gathered rows) + P D_last (Q); backward 4P (incidence entries) + 2 P D_last (gQ rows, once
 *   per incidence) + 2 P D_last (X rows, MUL only) + N D_last (the head's gradient rows). */
enum { GAT_PAIR_NONE = 0, GAT_PAIR_MUL = 1, GAT_PAIR_ADD = 2 };
int gat_set_pairs(gat_ctx* ctx, int32_t mode, const int32_t* u, const int32_t* v, int64_t n_pairs);            /* host arrays [n_pairs] */
int gat_set_pairs_device(gat_ctx* ctx, int32_t mode, const int32_t* d_u, const int32_t* d_v, int64_t n_pairs); /* checked on the device */
int gat_pairs_info(gat_ctx* ctx, int32_t* mode, int64_t* n_pairs);                                             /* (0, 0) while off; pointers may be NULL */
/* The two kernels as stateless seams on caller-owned DEVICE pointers (current device): d_x rows of x_stride >= width floats (may be NULL
 * in the backward of GAT_PAIR_ADD), d_q / d_gq [n_pairs][width]; the backward writes floats 0..width-1 of every d_gh row (n_rows rows,
 * gh_stride >= width floats apart) and nothing behind them.  Each call checks d_u / d_v with gat_set_pairs' rules (same codes and texts),
 * the backward builds the incidence index and the work list, allocates and frees its scratch, and both synchronise `stream` (may be
 * NULL): parity seams, not the fast path. */
int gat_op_pair_forward(const float* d_x, int64_t x_stride, const int32_t* d_u, const int32_t* d_v, int64_t n_pairs, int64_t n_rows,
                        int32_t width, int32_t mode, float* d_q, void* stream);
int gat_op_pair_backward(const float* d_gq, const float* d_x, int64_t x_stride, const int32_t* d_u, const int32_t* d_v, int64_t n_pairs,
                         int64_t n_rows, int32_t width, int32_t mode, float* d_gh, int64_t gh_stride, void* stream);

/* ---- negative sampling (for the pair head: link prediction draws fresh non-edges every epoch, PyG's negative_sampling /
 * structured_negative_sampling; here one full-batch step is one epoch) ----
 * A deterministic, edge-filtered sampler on the device and a call that rewrites the negative part of the context's pair list in place.
 * THE SAMPLING LAW — one function of (graph, mode, flags, seed, round, count[, source pairs]); synth.negative_pairs states it in numpy and
 * the kernel agrees with it to the bit.  H(seed, stream, idx) is the generators' counter hash (synth._hash).  For negative j in
 * [0, count) and attempt a in [0, GAT_NEG_TRIES) the counter is k = (round * count + j) * 16 + a, in wrapping uint64 arithmetic.
 *     GAT_NEG_UNIFORM   u = H(seed, 37, k) % N,  v = H(seed, 41, k) % N
 *     GAT_NEG_CORRUPT   structured: one endpoint of a real pair is kept.  Source pair p = j % n_src; role = H(seed, 43, round * count + j) & 1,
 *                       drawn once per negative, not per attempt; w = H(seed, 37, k) % N; role 0: (u, v) = (w, v_p), role 1: (u, v) = (u_p, w)
 *   A candidate is accepted when u != v (unless GAT_NEG_ALLOW_SELF), (u, v) is not an edge and, with GAT_NEG_BOTH_DIRECTIONS, (v, u) is not
 *   one either.  "(u, v) is an edge": u occurs in col_idx[row_ptr[v] .. row_ptr[v+1]) — rows are destinations, columns sources; rows whose
 *   sources are not ascending and rows with duplicate edges are tested correctly (a binary search when every row of the graph is
 *   ascending, checked in one pass at set-up; a linear scan of the row otherwise — the result does not depend on which).  The first
 *   accepted attempt wins.  When none of the 16 is accepted the negative keeps attempt 15's candidate and counts as one UNFILTERED
 *   negative (the list length is fixed); the count is reported.
 * gat_set_negative_sampling declares pairs [first, first + count) of the context's pair list as the negative slots.  Labels, targets and
 *   masks over those slots are the caller's and are never touched.  Needs a pair head (else GAT_E_STATE); count >= 1, 0 <= first,
 *   first + count <= n_pairs, a mode and flags inside the enums, else GAT_E_INVALID; GAT_NEG_CORRUPT takes pairs [0, first) as its sources
 *   and needs first >= 1 (GAT_E_INVALID).  mode == 0 (GAT_NEG_NONE) switches the feature off and leaves the context exactly as it was (the
 *   pairs stay what they are; the other arguments are not read).  It draws nothing itself.
 * gat_resample_negatives waits for the context's stream, draws round `round` from the context's own graph into u / v [first, first + count),
 *   rebuilds the incidence index and — on the device, without an n_rows-sized round trip — the scatter's work list (word for word the
 *   lists gat_set_pairs builds for the same pairs, so results are bitwise those of gat_set_pairs with the same lists), invalidates y and
 *   re-arms a captured gat_step_graph exactly as a replacing gat_set_pairs does.  Before gat_set_negative_sampling: GAT_E_STATE.  Not part
 *   of a step: not captured, and gat_algorithmic_bytes is unchanged.
 *   Only the graph's edges are rejected: a candidate equal to a held-out positive of the pair list is NOT (PyG's behaviour when it is
 *   given the training edges).
 * gat_negatives_info: (mode, first, count, the last round drawn, its unfiltered count); all 0 while off; pointers may be NULL.
 * gat_pairs_get copies the current pair lists to the host ([n_pairs] each; a wrong n_pairs: GAT_E_INVALID; no pair head: GAT_E_STATE).
 * gat_op_negative_sample is the sampler as a stateless seam on caller-owned DEVICE pointers (current device): a CSR of n_rows rows and
 *   n_edges edges over n_rows sources (checked on the device with gat_graph_check_device's rules before anything walks it), d_src_u /
 *   d_src_v [n_src] for GAT_NEG_CORRUPT (checked like gat_set_pairs' arrays; may be NULL for GAT_NEG_UNIFORM), d_u / d_v [count] out,
 *   *unfiltered (host) the count.  Same codes as the context form; mode 0 is GAT_E_INVALID here.  Synchronises `stream` (may be NULL). */
enum { GAT_NEG_NONE = 0, GAT_NEG_UNIFORM = 1, GAT_NEG_CORRUPT = 2 };
enum { GAT_NEG_BOTH_DIRECTIONS = 1, GAT_NEG_ALLOW_SELF = 2 };
#define GAT_NEG_TRIES 16
int gat_set_negative_sampling(gat_ctx* ctx, int32_t mode, int64_t first, int64_t count, int32_t flags, uint64_t seed);
int gat_resample_negatives(gat_ctx* ctx, uint64_t round);
int gat_negatives_info(gat_ctx* ctx, int32_t* mode, int64_t* first, int64_t* count, uint64_t* last_round, int64_t* unfiltered);
int gat_pairs_get(gat_ctx* ctx, int32_t* u_host, int32_t* v_host, int64_t n_pairs);
int gat_op_negative_sample(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, int64_t n_edges,
                           int32_t mode, int32_t flags, uint64_t seed, uint64_t round,
                           const int32_t* d_src_u, const int32_t* d_src_v, int64_t n_src,
                           int32_t* d_u, int32_t* d_v, int64_t count, int64_t* unfiltered, void* stream);

/* The dense launchers (the W_l / W_r projections, their two backward products and the residual's three) as stateless seams on caller-owned
 * DEVICE pointers (current device).  Each call runs exactly ONE launcher with exactly the caller's arguments and synchronises `stream`
 * (may be NULL): parity seams, not the fast path.  W is the reference layout [HD][2F], Wres [HD][F]; part: 0 both halves, 1 the left
 * (PL / gPL) half alone, 2 the right one — pointers of a half that is not asked for may be NULL and its cells are not written; ldx: floats
 * between rows of X (0 = F; a multiple of 4 with ZEROS behind column F selects 16-byte loads); d_pl holds fp32 rows, or bf16 rows with
 * pl_bf16 = 1; d_hpre_prev == NULL stores the plain sum; grad_w, grad_wres and grad_x_res ADD into their output.  Scratch sizes come from
 * gat_op_dense_scratch_floats (kind 0: the projection's split-K slabs for (n_rows, F, HD, part), 0 when that launch never splits; kind 1:
 * the slabs of grad_w / grad_wres, part is ignored).  The projection takes its split-K path only when scratch_floats covers it and the
 * streaming kernel otherwise; grad_w / grad_wres refuse a scratch_floats below the stated size.  Every argument is checked before any
 * launch: a NULL pointer the part needs, n_rows < 0, F < 1, HD < 1, ldx != 0 && ldx < F, a part or pl_bf16 outside its values give
 * GAT_E_INVALID and a text, and nothing is written.  picked (may be NULL) receives, NUL-terminated and cut to picked_cap bytes, the template
 * name of the row / tile kernel the launcher launched last, e.g. "rowgemm_x3_kernel<2, 8, true>" ("" when n_rows == 0 launched nothing):
 * it is how tests/test_dense_seams.py proves that a case reached the dispatch branch it names. */
int gat_op_dense_scratch_floats(int32_t kind, int64_t n_rows, int32_t F, int32_t HD, int32_t part, int64_t* floats_out);
int gat_op_dense_project(const float* d_x, int32_t ldx, const float* d_w, int64_t n_rows, int32_t F, int32_t HD, int32_t part, int32_t pl_bf16,
                         void* d_pl, float* d_pr, float* d_scratch, int64_t scratch_floats, void* stream, char* picked, int32_t picked_cap);
int gat_op_dense_grad_x(const float* d_gpl, const float* d_gpr, const float* d_w, const float* d_hpre_prev, float* d_gprev, int64_t n_rows,
                        int32_t F, int32_t HD, float slope, void* stream, char* picked, int32_t picked_cap);
int gat_op_dense_grad_w(const float* d_gpl, const float* d_gpr, const float* d_x, int32_t ldx, float* d_grad_w, float* d_scratch,
                        int64_t scratch_floats, int64_t n_rows, int32_t F, int32_t HD, int32_t part, void* stream, char* picked, int32_t picked_cap);
int gat_op_dense_project_res(const float* d_x, int32_t ldx, const float* d_wres, float* d_r, int64_t n_rows, int32_t F, int32_t HD, void* stream,
                             char* picked, int32_t picked_cap);
int gat_op_dense_grad_wres(const float* d_g, const float* d_x, int32_t ldx, float* d_grad_wres, float* d_scratch, int64_t scratch_floats,
                           int64_t n_rows, int32_t F, int32_t HD, void* stream, char* picked, int32_t picked_cap);
int gat_op_dense_grad_x_res(const float* d_g, const float* d_wres, float* d_gx, int64_t n_rows, int32_t F, int32_t HD, void* stream,
                            char* picked, int32_t picked_cap);

/* ---- loss modes of the output head (beyond the reference, whose head is one softmax + cross-entropy on an int32 label per row) ----------
 * Multi-label classification (PPI, ogbn-proteins), regression (ZINC, QM9) and multi-task targets with missing entries (ogbg-molpcba)
 * need a FLOAT target matrix T [rows][C], a per-entry loss, and entries that may be absent.  C = num_classes is the number of output
 * columns; Wo keeps its shape [C][D_last]; a row r is a node — a graph on a readout context, exactly where labels were per graph.
 *     z[r][c] = sum_j Wo[c][j] X[r][j]      fp32, ascending j, as in the softmax head (X = the head's input rows)
 *     present(r,c) = !isnan(T[r][c])  (NaN marks a missing entry, the OGB convention);  trains(r) = no training mask, or mask[r]
 *   Only entries that are present and in a training row contribute; every other entry has loss 0, count 0 and dz = 0.
 *     GAT_LOSS_BCE  T in [0,1] (soft labels allowed) or NaN;  e = exp(-|z|);  y = z >= 0 ? 1/(1+e) : e/(1+e)  (= sigmoid(z), stable for
 *                   both signs);  l = max(z,0) - t z + log1p(e);  dz = y - t;  the prediction is z > 0 and an entry is correct when
 *                   (z > 0) == (t > 0.5);  GAT_TAP_Y returns y
 *     GAT_LOSS_MSE  T finite or NaN;  y = z;  l = (z - t)^2;  dz = 2 (z - t)  (loss and gradient of torch.nn.MSELoss(reduction="sum"));
 *                   n_correct is 0;  GAT_TAP_Y returns the predictions
 *   loss_sum = sum of l over the contributing entries (fp32 terms, a double accumulator per thread, block and grid reductions in a fixed
 *   order), n_correct = the correct contributing entries, gH = dz Wo, gradWo += dz^T X.  The loss is a SUM, like the reference's: callers
 *   divide by gat_target_count.  Everything below the head is unchanged: the new head writes the gH the softmax head writes, and the
 *   last layer's edge backward, the residual / norm kernels and the un-pool consume it as they do now.  No new parameter group (no bias
 *   on the output head: a constant offset is reachable through the last layer's b / beta).
 * gat_set_loss is allowed until the first gat_set_labels* / gat_set_targets* call (later: GAT_E_STATE); a mode outside 0..2:
 *   GAT_E_INVALID.  Mode 0 (GAT_LOSS_SOFTMAX_CE) is the default and leaves the context exactly as it is: same buffers, same kernels,
 *   same launch counts, bitwise the same results.  With mode != 0, gat_set_labels* returns GAT_E_STATE (its text names gat_set_targets);
 *   with mode 0, gat_set_targets* returns GAT_E_STATE.
 * gat_set_targets[_device] is called where labels are set today: after the graph (before: GAT_E_STATE), and after gat_set_readout on a
 *   readout context.  n_cols must be C and n_rows the head's row count, else GAT_E_INVALID; n_rows * C >= 2^31: GAT_E_UNSUPPORTED
 *   (n_correct is int32).  A BCE entry outside [0,1], or a +-inf entry in either mode: GAT_E_INVALID with a text naming the lowest
 *   offending flat index; the device form finds it in one pass on the device before anything reads the array (as
 *   gat_graph_check_device does).  The array is copied.  A later call with the same shape replaces the values IN THE SAME DEVICE
 *   BUFFER: a captured gat_step_graph replay then reads the new targets without re-capture.  A step or phase call in mode != 0 without
 *   targets returns GAT_E_STATE and says so.
 * gat_set_train_mask is unchanged at the boundary; the new kernels read the mask byte of a row themselves (NULL = all rows) and
 *   changing the mask re-arms a captured step, as it does now.  gat_eval_mask keeps its signature: in the new modes it returns the sum
 *   of l and the correct count over the present entries of the mask's rows (it runs the head's forward kernel on the last forward's
 *   input rows with that mask); n_nodes still counts rows, gat_target_count gives the entry denominator.
 * Where it runs.  Two kernels in place of the softmax head's, both persistent over 128-row tiles (fewer rows per tile when C is large):
 *   Wo, the tile's targets — one contiguous block, loaded coalesced, NaN test and mask byte applied there — and the tile's input rows in
 *   LDS with odd row strides; the tile's entries are dealt to the 256 threads by flat index, so no thread owns a row and every C >= 1 and
 *   D_last >= 1 takes the same path.  D_last in {4, 8, 16} with C <= 128 runs the register-blocked form of the same tile (a thread keeps
 *   its input row in registers and walks half of the columns; then two waves own a row each for gH while the other two own (column, row
 *   part) for gradWo); every z is the same fmaf chain in both forms, and a shape always takes the same form in both kernels.
 *   exp / log / reciprocal are the hardware's (1 ulp; log1p(e) below 2^-10 by its series): absolute error of a loss term below 1e-6.
 *   The forward kernel writes y and the loss / count partials (gat_head_forward, gat_forward, gat_step with
 *   keep_taps); the gradient kernel recomputes z with the same expression in the same order, overwrites the targets in LDS with dz, and
 *   writes gH rows and per-block gradWo partials (gat_head_backward; gat_step without keep_taps, where it forms the loss / count partials
 *   too and y never reaches HBM).  Both run on the same grid: gat_step, gat_forward + gat_backward, the phase API and a graph replay
 *   give bitwise the same loss and gradients.  No float atomics.  Timed under GAT_K_HEAD_FWD / GAT_K_HEAD_BWD.
 * Shape limits: the gradient kernel needs C * D_last <= 2048, the forward kernel that one row of the tile fits in LDS beside Wo; beyond,
 *   the call that would launch the kernel returns GAT_E_UNSUPPORTED with a text naming the output head.
 * Works with every (H, D) family incl. both generic ones, bf16 storage (the head stays fp32), keep_taps, eval mode, all three
 *   regularisers, residual, bias, norm, edge features and readout (targets and mask per graph), the phase API, gat_step, gat_step_graph,
 *   and destination-range shards on any transport (the head is row-local, targets are the shard's own rows, nothing new is exchanged;
 *   loss and count ride in the existing three-float tail, whose 12-bit split of the count stays exact because n_rows * C < 2^31).
 * Refused with GAT_E_UNSUPPORTED (by gat_set_loss with mode != 0): flat_lrelu_index = 1 (the new head writes gH only, never a g); the
 *   experiment library with GAT_DBG set.  GAT_FUSE_LAST=1 is not used by such a context: it runs the separate passes.
 * gat_algorithmic_bytes (context form): unchanged in mode 0.  In the new modes GAT_K_HEAD_FWD and GAT_K_HEAD_BWD each price
 *   4 * rows * C bytes of targets in place of 4 * rows of labels: + 4 * rows * (C - 1) per class, rows = n_graphs with readout on. */
enum { GAT_LOSS_SOFTMAX_CE = 0, GAT_LOSS_BCE = 1, GAT_LOSS_MSE = 2 };
int gat_set_loss(gat_ctx* ctx, int32_t mode);
int gat_set_targets(gat_ctx* ctx, const float* t, int64_t n_rows, int32_t n_cols);            /* host  [n_rows][n_cols] */
int gat_set_targets_device(gat_ctx* ctx, const float* d_t, int64_t n_rows, int32_t n_cols);   /* device, checked on the device */
int gat_loss_info(gat_ctx* ctx, int32_t* mode, int32_t* n_cols);                              /* (0, num_classes) by default; pointers may be NULL */
int gat_target_count(gat_ctx* ctx, const uint8_t* mask, int64_t n_rows, int64_t* n_entries);
        /* present entries in the rows of `mask` (host, [n_rows]); mask NULL = the current training set */

/* ---- ranking metrics (beyond the reference, which reports a loss and an accuracy: ROC-AUC of ogbn-proteins / ogbg-molhiv, average
 * precision of ogbg-molpcba, MRR of ogbl-citation2, Hits@K of ogbl-collab / -ppa / -ddi) ----
 * The integer rank statistics behind those metrics, per output column, formed on the device from ONE sort of the scores it already holds.
 * THE LAW — tests/rank_ref.py states it in numpy.  Inputs: the head's rows r of the LAST forward (nodes; the graphs of a readout context; the
 * pairs of a pair head) and a host mask over those rows, as gat_eval_mask takes it.  The score of entry (r, c) is the value GAT_TAP_Y
 * returns for it: the softmax probability of class c in the default loss mode (one-vs-rest), sigmoid(z) under GAT_LOSS_BCE.
 *   Saturation: fp32 sigmoid(z) is exactly 1.0 above z ~ 17 (and the softmax probability of a dominant class likewise), so very confident
 *   entries TIE.  Ties are handled exactly (below); ranking on the logits z is out of scope.
 * An entry TAKES PART when its row is in the mask, its target is present (BCE: !isnan(t); softmax mode: always) and its score is not NaN.
 *   An entry with a NaN score that passes the first two tests is counted in n_nan and otherwise ignored.
 * An entry is POSITIVE when label[r] == c (softmax mode) or t > 0.5 (BCE: the rule n_correct uses), else NEGATIVE.
 * Two scores TIE when they compare equal as floats: -0.0 and +0.0 tie, +-inf are ordinary values.
 * Per column c, over its participating entries, with P positives and N negatives:
 *   n_pos, n_neg, n_nan   the counts
 *   auc_num  = sum over the positives of  2 * #{negatives strictly lower} + #{negatives equal}      (twice the Mann-Whitney U, ties at 1/2)
 *              AUC = auc_num / (2 P N) is the caller's division: sklearn.metrics.roc_auc_score; undefined when P * N == 0
 *   ap       = (1/P) sum over the positives of  TP(>= s) / (TP(>= s) + FP(>= s)),  s the positive's score, the counts over all participating
 *              entries of the column: sklearn.metrics.average_precision_score (one threshold per distinct score); 0 when P == 0
 *   mrr      = (1/P) sum over the positives of  1 / (1 + #{negatives higher} + 0.5 * #{negatives equal}): every positive ranked against ALL the
 *              column's negatives, OGB's tie rule (mean of the optimistic and the pessimistic rank); 0 when P == 0
 *   hits[k]  = for each of the n_ks <= GAT_RANK_MAX_KS caller-given K >= 1: the positives with a score STRICTLY above the K-th highest negative
 *              score (duplicates count, as torch.topk does): OGB's Hits@K numerator; with N < K it is P (OGB returns 1.0 there).  hits[n_ks ..] = 0
 *   All integers are exact.  Each fp64 term is one division of exact integers (mrr: of 1 by an exact half-integer); the two sums are formed
 *   in an order fixed by the shape — per-thread, per-block and per-column in ascending order, no float atomics — so they are bitwise
 *   reproducible from run to run and lie within (P + 2) * 2^-52 relative of the exact sum.  Integer atomics are used.
 * Grouped ranking (each positive against its OWN negatives, ogbl-citation2's evaluator), micro-averages and F1 are out of scope.
 * Where it runs (csrc/gat_rank.hip).  One pass writes a 64-bit key per (row, column) slot — column in the high bits, then the order-preserving
 *   unsigned image of the score (sign-flipped float bits, -0.0 folded onto +0.0), the positive bit lowest; the all-ones key for a slot that does
 *   not take part — and counts the NaN scores.  One radix sort over the 33 + bit_width(C) bits in use.  An inclusive prefix count of negatives
 *   over the sorted keys.  The C column segments by binary search.  The rank kernel: one lane per sorted slot; a positive finds its tie group
 *   by a galloping and a binary search on key >> 1 inside its column's segment (never a walk: a saturated column is one group of millions),
 *   reads negatives below / equal / above and TP, FP from the prefix counts, and leaves its terms to fixed-order block partials that a last
 *   kernel adds per column.  Hits@K: per (column, K) one search on the prefix counts and one for the end of the tie group, no pass over the data.
 *   Temporary device memory: 20 bytes per slot (two key buffers and the prefix counts; slots = rows * C) plus the sort's scratch (a few
 *   MB) and O(C) words — 80 MB for 4 M pairs at C = 1, 2.3 GB for 2.45 M rows at C = 47.  The context allocates it at the first
 *   gat_eval_rank and keeps it; the seam allocates and frees per call.  rows * C >= 2^31 slots: GAT_E_UNSUPPORTED, never truncated.
 * gat_eval_rank(ctx, mask, n_rows, ks, n_ks, out): out is a HOST array of num_classes entries.  The mask follows gat_eval_mask's rules (non-NULL,
 *   length = the head's rows, else GAT_E_INVALID), and so does y: after a fused head step (gat_step) the head's forward kernel is re-run
 *   on the last forward's rows, as gat_eval_mask and gat_tap(GAT_TAP_Y) do.  The call changes nothing a later step reads: it does not re-arm
 *   a captured gat_step_graph (gat_step_graph_state stays 2) and advances no counter; the steps after it are bitwise those of a run
 *   without it.  Between replayed steps it ranks the last replay's forward: a replay leaves y stale when its head is the fused one.
 *   It synchronises.
 *   n_ks outside 0..GAT_RANK_MAX_KS, or a K < 1: GAT_E_INVALID.  GAT_LOSS_MSE: GAT_E_UNSUPPORTED (no binary relevance).  A destination-range
 *   shard (n_table != n_rows) or a context with a transport: GAT_E_UNSUPPORTED (a ranking is global and cannot be summed over shards).  Before
 *   labels / targets, or before any forward: GAT_E_STATE.  Timed under GAT_K_MISC; gat_algorithmic_bytes is unchanged (not part of a step).
 * gat_op_rank_stats is the same computation as a stateless seam on caller-owned DEVICE pointers (current device): d_scores rows of
 *   score_stride >= n_cols floats; exactly one of d_labels [n_rows] / d_targets [n_rows][n_cols] non-NULL (else GAT_E_INVALID); d_mask
 *   [n_rows] may be NULL (every row); ks and out are HOST arrays.  Every argument is checked before any launch (n_rows < 0, n_cols < 1,
 *   score_stride < n_cols: GAT_E_INVALID; the K and slot rules above); it allocates and frees its scratch and synchronises `stream` (may
 *   be NULL).  Nothing is written to device memory the caller owns. */
#define GAT_RANK_MAX_KS 8
typedef struct gat_rank_stats {
    int64_t n_pos, n_neg, n_nan;
    uint64_t auc_num;
    double ap, mrr;
    int64_t hits[GAT_RANK_MAX_KS];
} gat_rank_stats;
int gat_eval_rank(gat_ctx* ctx, const uint8_t* mask, int64_t n_rows, const int32_t* ks, int32_t n_ks, gat_rank_stats* out /* [num_classes] */);
int gat_op_rank_stats(const float* d_scores, int64_t score_stride, const int32_t* d_labels, const float* d_targets, const uint8_t* d_mask,
                      int64_t n_rows, int32_t n_cols, const int32_t* ks, int32_t n_ks, gat_rank_stats* out /* host, [n_cols] */, void* stream);

/* ---- hidden layer in front of the output head (beyond the reference, whose head is one linear map: the MLP predictor of the OGB link
 * baselines and of PyG's MLP after global_*_pool) ----
 * An optional hidden stage for every head kind.  With R the head's rows (n_rows, n_graphs or n_pairs) and Xin [R][D_last] the rows the head
 * reads without it (the last layer's output, the pooled rows P, the pair rows Q):
 *     A  = Xin W1^T              W1 [Dh][D_last], the three-bf16-piece product of the other dense terms (fp32-accurate)
 *     Z1 = act(A + b1)           b1 [Dh];  act = ReLU, or with GAT_HEAD_ACT_LRELU LeakyReLU with the context's negative_slope
 *     z  = Z1 Wo^T               the existing head, unchanged, with Dh where it had D_last: Wo becomes [C][Dh]
 * Backward: gZ1 = the head's input gradient ([R][Dh]);  gA = gZ1 (.) (Z1 > 0 ? 1 : slope), slope = 0 for ReLU, Z1 == 0 takes the slope
 * branch (torch's convention);  gradb1 += column sums of gA,  gradW1 += gA^T Xin,  gXin = gA W1.  gXin goes where the head's gradient
 * went: the [n_rows][D_last] output gradient of a node head (the head then writes no g of its own, as with a readout), gP with a readout,
 * gQ with a pair head; everything from there downward is the code of a context without the feature.  The sign of A is that of Z1 for both
 * activations, so A is not kept.
 * gat_set_head_hidden(ctx, width, flags): width == 0 is the default and leaves the context exactly as it is: same buffers, same kernels,
 *   same launch counts, bitwise the same results (the flags are still checked).  width > 0 follows gat_set_residual's state rule: only
 *   before the first gat_params_*, gat_grads_* or gat_set_graph* call, else GAT_E_STATE (the packed buffers and Wo change size).
 *   width < 0 or unknown flag bits: GAT_E_INVALID.
 * Parameters: GAT_PARAM_HEAD_W flat [Dh][D_last] and GAT_PARAM_HEAD_B flat [Dh], behind GAT_PARAM_WE in the packed parameter, gradient and
 *   Adam buffers; their counts are 0 while the feature is off.  gat_zero_grad, gat_clip (one more norm per group), gat_step_sgd,
 *   gat_step_adam and gat_grads_device / export / import cover them; count of gat_grads_device = the sum of the ten group counts.
 *   gat_params_init: W and a of a seed are those of a context without the feature; Wo is drawn at its own place in the stream with its new
 *   shape [C][Dh] and lim = sqrt(6 / (C + Dh)), so the draws behind it (Wres, We) SHIFT on a context with the feature; W1 is Xavier-uniform
 *   with lim = sqrt(6 / (D_last + Dh)), drawn after every other draw; b1 = 0.
 * Shape limits: the head's, with Dh in D_last's place — C * Dh <= 2048 and the LDS tile of the head's kernels.  A width outside them is
 *   refused with GAT_E_UNSUPPORTED and a text naming the width and the limit, by gat_set_head_hidden itself where the limit does not depend
 *   on the loss mode, else by the call that completes the context.  Dh in {4, 8, 16} selects the head's register-blocked / fused forms as
 *   D_last does; every other width the any-shape forms.
 * Where it runs.  The three products run on the dense launchers of the residual term with rows = R, F = D_last, HD = Dh; gXin's launcher adds
 *   into its output, which is zeroed first (a memset node in a captured step).  Around them two row-streaming kernels: the forward writes
 *   Z1 = act(A + b1) in place (float4 accesses when Dh is a multiple of 4, scalar otherwise, b1 in registers, a persistent grid); the
 *   backward turns gZ1 into gA in place and leaves per-block column sums of gA in a fixed order, which the slab reduction adds into gradb1.
 *   No float atomics: the result is a function of (R, Dh) and the data alone, bitwise the same in gat_step, gat_forward + gat_backward,
 *   the phase API and a gat_step_graph replay.  The launches are part of gat_head_forward (after the pool or gather, before the head) and
 *   gat_head_backward (after the head, before the un-pool or scatter): no host synchronisation, fixed addresses; timed under
 *   GAT_K_HEAD_FWD / GAT_K_HEAD_BWD.  A replacing gat_set_pairs / gat_resample_negatives keeps every buffer.
 * gat_eval_mask, gat_eval_rank and gat_tap(GAT_TAP_Y) run the head on Z1 of the last forward; GAT_TAP_HEAD_HIDDEN returns Z1 ([R][Dh], last
 *   layer only, GAT_E_STATE without the feature).
 * Works with every head kind, all three loss modes, every (H, D) family, bf16 storage (the stage stays fp32), keep_taps, the regularisers,
 *   residual, bias, norm and edge features.
 * Refused with GAT_E_UNSUPPORTED, as the readout and the pair head refuse them: a destination-range shard (n_table != n_rows) or a context
 *   with a transport (at the call that sets such a graph; gat_comm_init_* on a hidden-head context alike); flat_lrelu_index = 1; the
 *   experiment library with GAT_DBG set.  GAT_FUSE_LAST=1 is not used by such a context.
 * Not there: more than one hidden layer, dropout on Z1, a bias on the output layer (a hidden unit with a zero W1 row and a positive b1
 *   supplies the offset), shards.
 * gat_algorithmic_bytes (context form): unchanged with the feature off.  On, the head classes are priced with Dh for D_last, and at 4 bytes
 *   GAT_K_HEAD_FWD gains R D_last + Dh D_last + 3 R Dh (Xin, W1, A written, A read and Z1 written) and GAT_K_HEAD_BWD gains 3 R Dh (the
 *   activation backward) + R Dh + R D_last + Dh D_last (gradW1) + R Dh + Dh D_last + R D_last (gXin). */
enum { GAT_HEAD_ACT_LRELU = 1 };                       /* flags; 0 = ReLU */
enum { GAT_PARAM_HEAD_W = 8, GAT_PARAM_HEAD_B = 9 };   /* [Dh][D_last], [Dh]: behind GAT_PARAM_WE; count 0 while off */
enum { GAT_TAP_HEAD_HIDDEN = 20 };                     /* [R][Dh]  Z1 of the last forward */
int gat_set_head_hidden(gat_ctx* ctx, int32_t width, int32_t flags);
int gat_head_hidden_info(gat_ctx* ctx, int32_t* width, int32_t* flags);   /* (0, 0) while off; pointers may be NULL */
/* The two row-streaming kernels as stateless seams on caller-owned DEVICE pointers (current device).  Forward: d_a [rows][width] becomes
 * Z1 = act(d_a + d_b1) in place, slope = 0 for ReLU.  Backward: d_gz [rows][width] becomes gA = d_gz (.) (d_z1 > 0 ? 1 : slope) in place
 * and the column sums of gA are ADDED into d_grad_b1 [width] (may be NULL: not formed).  rows == 0 launches nothing and succeeds.  rows < 0,
 * width < 1, a slope outside [0, 1] or not finite, or a null pointer with rows > 0: GAT_E_INVALID, nothing is written.  The backward
 * allocates and frees its block partials; both synchronise `stream` (may be NULL). */
int gat_op_head_hidden_forward(float* d_a, const float* d_b1, int64_t rows, int32_t width, float slope, void* stream);
int gat_op_head_hidden_backward(float* d_gz, const float* d_z1, int64_t rows, int32_t width, float slope, float* d_grad_b1, void* stream);

/* ---- optimizer step on the device (beyond the reference, whose three kernels stay behind gat_clip / gat_step_sgd / gat_step_adam): weight
 *      decay, SGD with momentum, Adam with L2, AdamW, per-group and global-norm clipping, one captured launch per epoch -------------------
 * The law.  p, g and the state are entries of the packed buffers, k is the parameter group (GAT_PARAM_*) of an entry, fp32 throughout.
 *   Clip factor, with s_k the sum of squares of group k's gradient:
 *     GAT_CLIP_NONE       c_k = 1
 *     GAT_CLIP_PER_GROUP  n_k = sqrt(s_k);  c_k = thr / (n_k + 1e-9f) if n_k > thr, else 1                       (gat_clip's law)
 *     GAT_CLIP_GLOBAL     n = sqrt(sum_k s_k), groups added in ascending order;  c = min(1, thr / (n + 1e-6f))   (clip_grad_norm_'s law)
 *   g^ = c_k * g.  The gradient buffer is only read: after the call it still holds the unclipped g.  A non-finite norm propagates as the
 *   formulas give it (a NaN norm gives c = NaN, as torch's clamp does; no special case).
 *   Update, with lambda = weight_decay where bit k of decay_groups is set and 0 elsewhere:
 *     GAT_OPT_SGD    d = g^ + lambda p;  buf = mu buf + d (buf starts at 0: the first step gives buf = d, torch's dampening = 0);
 *                    d = d + mu buf with GAT_OPT_NESTEROV, else d = buf;  p -= lr d.  With mu = 0 no buf exists and d is used as it is.
 *     GAT_OPT_ADAM   d = g^ + lambda p (L2, torch.optim.Adam(weight_decay=));  m = b1 m + (1 - b1) d;  v = b2 v + (1 - b2) d d;
 *                    m^ = m / (1 - b1^t);  v^ = v / (1 - b2^t);  p -= lr m^ / (sqrt(v^) + eps)   — the operations of gat_step_adam's kernel
 *     GAT_OPT_ADAMW  p *= 1 - lr lambda first, then the Adam update with d = g^ (torch.optim.AdamW)
 *   The two bias corrections 1 - b^t are formed once per block (powf on (float)t).  An entry with g = 0, lambda = 0 and zero state comes
 *   back bit for bit.
 * t and lr live on the device.  t is a 64-bit counter that starts at 0 and is advanced by one BEFORE use (the first step uses t = 1), by
 * one lane of the first launch; the second launch reads it.  gat_set_lr writes the device scalar on the context's stream (a one-lane
 * launch, no synchronisation): it does not re-arm a captured graph, so a learning-rate schedule costs nothing.
 * Kernels (csrc/gat_optimizer.hip): an optimizer step is TWO launches whatever the number of groups.  Both run over a block table built on
 * the host at gat_set_optimizer — rows {group, first, count} of at most 1024 entries, never straddling two groups.  opt_prepare writes each
 * block's sum of squares (lane-strided, wave butterfly, waves ascending) and advances t (GAT_CLIP_NONE: one block that only advances t);
 * opt_apply adds the partials it needs in ascending block order (its group's, or all of them with the groups ascending), forms c_k, reads t
 * and lr and updates its entries; block 0 leaves the norms for gat_optimizer_info.  No float atomics, no fences, no cooperative launch: the
 * result is a function of the packed sizes alone, bitwise reproducible, the same in a replay.  Timed under GAT_K_MISC;
 * gat_algorithmic_bytes* are unchanged (the optimizer never was priced).
 * State rules.  gat_set_optimizer counts as a first gat_params_* call: the packed sizes are final after it (a later gat_set_residual or
 * any other size-changing setter gives GAT_E_STATE).  It allocates and zeroes the state of the kind: m and v for the Adam kinds, buf for SGD
 * with momentum > 0.  A second call with the same kind keeps state and t and replaces the hyper-parameters (lr included); another kind
 * frees the old state, zeroes the new one and sets t = 0.  Either way a captured step graph is dropped (the hyper-parameters other than lr
 * are kernel arguments).  The state is the optimizer's own: gat_step_adam keeps its own moments, and gat_clip / gat_step_sgd /
 * gat_step_adam / gat_zero_grad neither read nor write anything of this section.
 * GAT_E_INVALID, with a text: a null config; a kind, flag or clip mode outside the enums; GAT_OPT_NESTEROV without momentum > 0 or on an
 * Adam kind; a beta outside (0, 1) (Adam kinds); eps, lr, weight_decay or momentum negative or not finite; momentum >= 1; a clip mode other
 * than NONE with a threshold that is not finite and > 0; a bit of decay_groups at or above group 10 unless the mask is exactly 0xFFFFFFFF.
 * Works with every context gat_step works on (all features, bf16 storage, shards with a transport: the update then reads the gradients the
 * all-reduce has summed, every rank takes the same step).  Refused: gat_optimizer_step, gat_train_step and the state calls before
 * gat_set_optimizer (GAT_E_STATE); capturing gat_train_step with a transport (gat_step_graph's own refusal). */
enum { GAT_OPT_SGD = 1, GAT_OPT_ADAM = 2, GAT_OPT_ADAMW = 3 };
enum { GAT_OPT_NESTEROV = 1 };
enum { GAT_CLIP_NONE = 0, GAT_CLIP_PER_GROUP = 1, GAT_CLIP_GLOBAL = 2 };
typedef struct gat_optimizer_config {
    int32_t kind, flags; float lr, momentum, beta1, beta2, eps, weight_decay;
    uint32_t decay_groups;          /* bit k = GAT_PARAM_* group k; 0xFFFFFFFF = all (torch's behaviour) */
    int32_t clip_mode; float clip_threshold;
} gat_optimizer_config;
int gat_set_optimizer(gat_ctx* ctx, const gat_optimizer_config* cfg);
int gat_optimizer_step(gat_ctx* ctx);                       /* prepare + apply; GAT_E_STATE before gat_set_optimizer */
int gat_set_lr(gat_ctx* ctx, float lr);                     /* negative or not finite: GAT_E_INVALID */
/* Synchronises.  Any pointer may be NULL.  *t: steps taken; *lr: the device scalar; group_norms [10]: n_k of the last step (0 for an empty
 * group), *global_norm: n of the last step under GAT_CLIP_GLOBAL, else 0.  With GAT_CLIP_NONE no norm is formed: all stay what they were (0
 * at first). */
int gat_optimizer_info(gat_ctx* ctx, gat_optimizer_config* cfg, int64_t* t, float* lr, float* global_norm, float* group_norms /* [10] or NULL */);
/* One group of one state buffer, to / from the host (checkpoints).  `which` must be a state the current configuration has (M, V: the Adam
 * kinds; MOMENTUM: SGD with momentum > 0), else GAT_E_INVALID; the size rules are gat_params_get's (a group that is off has count 0 and the
 * call is a no-op).  set writes into the same buffers, so a captured graph stays valid; gat_optimizer_step_count_set (t >= 0) likewise. */
enum { GAT_OPT_STATE_M = 0, GAT_OPT_STATE_V = 1, GAT_OPT_STATE_MOMENTUM = 2 };
int gat_optimizer_state_get(gat_ctx* ctx, int which, int group, float* host, int64_t count);
int gat_optimizer_state_set(gat_ctx* ctx, int which, int group, const float* host, int64_t count);
int gat_optimizer_step_count_set(gat_ctx* ctx, int64_t t);
/* One epoch body: zero the packed gradients (gat_zero_grad's memset), the body of gat_step, gat_optimizer_step — on the context's stream,
 * in that order.  Returns the loss sum and #correct of the forward BEFORE the update, as gat_step does.  With gat_step_graph(ctx, 1) the
 * whole sequence is captured into the one replay slot after one eager call, like gat_step; the slot remembers which of the two entry
 * points it holds, and calling the other one on a captured (or warmed) slot drops it: that call runs eagerly, the next one captures.
 * Everything that re-arms gat_step re-arms it too, and gat_step_graph_state keeps its meaning.  The batch-norm running update and the
 * dropout counter advance once per call, replay included.  With a transport it runs eagerly. */
int gat_train_step(gat_ctx* ctx, float* loss_sum, int32_t* n_correct);

/* ---- op-level entry points, whole layers: caller-provided DEVICE pointers in the reference layouts
 *      (unit parity).  `stream` may be NULL (default stream).  One entry point per reference KERNEL: below. ---- */
/* a1  csr_to_coo_kernel E:67-84 */
int gat_op_csr_to_coo(const int32_t* d_row_ptr, const int32_t* d_col_idx, int32_t* d_src,
                      int32_t* d_dst, int64_t n_rows, int64_t n_edges, void* stream);
/* a2-a6 forward of one layer (E:279-459) from reference-layout W,a: writes attn_coeff [H][E],
 * h_pre [N][H][D], H_out. */
int gat_op_layer_forward(const int32_t* d_row_ptr, const int32_t* d_col_idx, const float* d_x,
                         const float* d_w, const float* d_a, float* d_attn_coeff, float* d_hpre,
                         float* d_hout, int64_t n, int64_t e, int32_t f, int32_t h, int32_t d,
                         int32_t is_last, float slope, void* stream);
/* a7-a11 backward of one layer (E:612-893): adds into d_grad_w/d_grad_a; writes g_prev
 * (= gx ⊙ LReLU'(hpre_prev)) when d_hpre_prev != NULL. */
int gat_op_layer_backward(const int32_t* d_row_ptr, const int32_t* d_col_idx, const float* d_x,
                          const float* d_w, const float* d_a, const float* d_attn_coeff,
                          const float* d_hpre, const float* d_g, float* d_grad_w, float* d_grad_a,
                          const float* d_hpre_prev, float* d_g_prev, int64_t n, int64_t e,
                          int32_t f, int32_t h, int32_t d, float slope, void* stream);

/* ---- per-kernel entry points: ONE per reference kernel of the hot path, each with the argument list of the launch it
 *      replaces (node / edge counts widened to 64 bit, a stream appended; `n` added where the reference kernel reads the
 *      node count only through its indices).  Caller-owned DEVICE pointers in the reference layouts: edge tensors [H][E]
 *      head-major, node tensors [N][H][D], W [H][D][2F], a [H][D].  Accumulate-or-overwrite behaviour is the reference's.
 *      A maintainer can swap a single launch of the reference's main() for the matching call and keep everything else
 *      (INTEGRATION.md §2b).  Scratch (projected features, message tables) is allocated per call; calls synchronise their
 *      stream.  Scatters use float atomics like the reference's own kernels (sums over edges order-dependent at fp32
 *      round-off).  csrc/gat_ops.hip.
 *      THESE ARE PARITY SEAMS, NOT THE FAST PATH: every call hipMalloc's and frees its scratch, re-projects X.W on the matrix cores,
 *      synchronises the stream, and scatters with global float atomics (~1.3 TB/s on this chip).  A maintainer who wants the speed
 *      swaps the epoch loop for gat_step / the phase API on a context (which owns its buffers and runs without atomics or
 *      per-call allocation), not kernel by kernel. ---------------------------------------------------------------------- */
/* a2  gatv2_edge_score_kernel E:279-324, launch E:1386: attn_score[h][e] (overwritten) */
int gat_op_edge_score(const float* d_input_features, const int32_t* d_col_idx, const int32_t* d_dst, const float* d_w,
                      const float* d_a, float* d_attn_score, int64_t n, int32_t in_dim, int32_t out_dim, int32_t h,
                      int64_t e, float negative_slope, void* stream);
/* a3  compute_max_sum_attn_score E:326-359, launch E:1394-1398: max_score / score_sum at index n*h + dst (overwritten);
 *     zero in-degree rows give max = -1e9f, sum = 0 (E:336) */
int gat_op_max_sum(const int32_t* d_row_ptr, const float* d_attn_score, int64_t n, int32_t h, int64_t e,
                   float* d_max_score, float* d_score_sum, void* stream);
/* a4  compute_attn_coeff E:362-384, launch E:1407 (d_col_idx is carried by the reference's signature and unused there too) */
int gat_op_attn_coeff(const int32_t* d_col_idx, const int32_t* d_dst, const float* d_attn_score, const float* d_max_attn_score,
                      const float* d_sum_score_exp, float* d_attn_coeff, int64_t e, int32_t h, int64_t n, void* stream);
/* a5  aggregate_kernel E:386-424, launch E:1416: ADDS into d_out_feat [N][H][D] (the caller zeroes it) */
int gat_op_aggregate(const int32_t* d_src, const int32_t* d_dst, const float* d_attn_coeff, const float* d_in_feat,
                     const float* d_w, float* d_out_feat, int64_t n, int32_t h, int64_t e, int32_t in_dim, int32_t out_dim,
                     void* stream);
/* a6  postActivationLayerOutput E:426-459, launch E:1428: d_H [N][H*D], or [N][D] (mean over heads) when is_last_layer */
int gat_op_post_activation(const float* d_out_feat, float* d_H, int64_t n, int32_t h, int32_t out_dim, int32_t is_last_layer,
                           float negative_slope, void* stream);
/* C12 gatv2_output_kernel E:463-512 (+ softmax E:132-141), launch E:1446: d_z and d_y [N][C] both receive the
 *     probabilities, as in the reference */
int gat_op_output_head(const float* d_wo, const float* d_last_layer_output, float* d_z, float* d_y, int64_t num_nodes, int32_t c,
                       int32_t out_dim_last_layer, void* stream);
/* C13 compute_loss_accuracy_kernel E:514-537, launch E:1457: per-node loss / correct arrays (summed by the caller, E:542) */
int gat_op_loss_accuracy(const float* d_y, const int32_t* d_labels, float* d_losses, int32_t* d_corrects, int64_t n, int32_t c,
                         void* stream);
/* C14 compute_output_gradients E:553-608, launch E:1468: ADDS into grad_d_wo [C][D_L]; writes grad_d_hL [N][H][D_L].
 *     flat_lrelu_index: 0 = the exact per-head LReLU' index, 1 = the reference's n*D_L + d (E:598) */
int gat_op_output_gradients(const float* d_y, const int32_t* d_labels, const float* d_hL, const float* d_HL, const float* d_wo,
                            float* grad_d_wo, float* grad_d_hL, int64_t n, int32_t c, int32_t out_dim_l, int32_t num_heads,
                            float negative_slope, int32_t flat_lrelu_index, void* stream);
/* a7  kernel_grad_atten_coeff E:612-651, launch E:1489: grad_attn_coeff[h][e] (overwritten) */
int gat_op_grad_attn_coeff(int64_t num_edges, int32_t num_heads, int32_t in_dim, int32_t out_dim, const int32_t* d_src,
                           const int32_t* d_dst, const float* d_features, const float* d_w, const float* d_grad_input,
                           float* d_grad_attn_coeff, int64_t n, void* stream);
/* a8  compute_grad_attn_score_kernel E:654-696, launch E:1499-1506: grad_attn_score[h][e] (overwritten); one pass per row
 *     instead of the reference's O(deg) loop per edge (same sums up to fp32 order) */
int gat_op_grad_attn_score(const int32_t* d_row_ptr, const int32_t* d_dst, const float* d_alpha, const float* d_grad_alpha,
                           float* d_grad_e, int64_t n, int32_t h, int64_t e, void* stream);
/* a9  compute_grad_parameters_kernel E:698-798, launch E:1517: ADDS into grad_w [H][D][2F] and grad_a [H][D] */
int gat_op_grad_parameters(int64_t e, int32_t h, const int32_t* d_src, const int32_t* d_dst, const float* d_features,
                           const float* d_input_gradients, const float* d_grad_attn_score, const float* d_attn_coeff,
                           const float* d_w, const float* d_a, float* grad_w, float* grad_a, int32_t in_dim, int32_t out_dim,
                           float negative_slope, int64_t n, void* stream);
/* a10 compute_features_input_gradients E:801-874, launch E:1533: ADDS into grad_x_features [N][F] (zeroed per epoch, E:1636) */
int gat_op_features_input_gradients(int64_t n, int32_t h, int64_t e, int32_t in_dim, int32_t out_dim, float negative_slope,
                                    const int32_t* d_src, const int32_t* d_dst, const float* d_attn_coeff,
                                    const float* d_input_features, const float* d_w, const float* d_input_gradients,
                                    const float* d_grad_attn_score, const float* d_attn_vector, float* d_grad_x_features,
                                    void* stream);
/* a11 compute_preActivation_inputFeatures_gradient E:879-893, launch E:1546: in place on input_features_gradients [N][F] */
int gat_op_preact_gradient(int64_t n, float negative_slope, int32_t in_dim, const float* d_pre_activation_input_features,
                           float* d_input_features_gradients, void* stream);

/* ---- synthetic workloads on the device --------------------------------------------
 * The reference's datasets are a download link (README R:21); every BASELINE workload here is a deterministic
 * synthetic graph of the stated shape (SURVEY 8d law; host implementation: synth.py).  These three calls do the
 * parts proportional to E and N*F on the GPU, bit-for-bit equal to the host generator.  Outputs are DEVICE
 * pointers (feed them to gat_set_*_device).  `stream` may be NULL.
 *   sources : per edge e, u = hash(seed, 3, e) -> rank = first r with h_cdf[r] > u -> h_node_of_rank[rank]; the
 *             sources of every row then sorted ascending (one radix sort of dst*n + src).  h_cdf / h_node_of_rank /
 *             h_row_ptr are the host's N-sized tables (synth.graph_tables).
 *   features: kind 0 = U[-1,1) fp32, kind 1 = sparse binary rows normalised by their count (Cora-like); rows
 *             [row0, row0+rows) of the [n][f] matrix.
 *   labels  : hash % num_classes, node 0 forced to num_classes-1.
 *   argsort : the three N-sized stable sorts of the host tables (two node permutations, the largest-remainder order). */
int gat_synth_sources_device(const double* h_cdf, const int32_t* h_node_of_rank, const int32_t* h_row_ptr, int64_t n,
                             int64_t n_edges, uint64_t seed, int32_t* d_col_idx, void* stream);
/* host keys -> host order, sorted on the device: order[i] = index of the i-th smallest key, ties in index order */
int gat_synth_argsort_u64(const uint64_t* h_keys, int64_t n, int32_t* h_order, void* stream);
int gat_synth_features_device(uint64_t seed, int64_t row0, int64_t rows, int32_t f, int32_t kind, float* d_x, void* stream);
int gat_synth_labels_device(uint64_t seed, int64_t row0, int64_t rows, int32_t num_classes, int32_t* d_labels, void* stream);

/* ---- measurement ------------------------------------------------------------------------------ */
enum {
    GAT_K_PROJECT = 0, GAT_K_EDGE_FWD = 1, GAT_K_HEAD_FWD = 2, GAT_K_HEAD_BWD = 3,
    GAT_K_EDGE_BWD = 4, GAT_K_GPL_SUM = 5, GAT_K_GRAD_W = 6, GAT_K_GRAD_X = 7, GAT_K_MISC = 8,
    GAT_K_EXCHANGE = 9,     /* transport calls of gat_forward / gat_backward / gat_step (event-timed like kernels) */
    GAT_K_EDGE_FUSED = 10,  /* experiment, off unless GAT_FUSE_LAST=1 (measured not ahead: DESIGN §4): gat_step with the last layer's
                               forward edge pass, the gH part of the head and its backward edge pass fused per destination row
                               (E:1386-1428 + 1468 + 1489-1533 of that layer in one launch; gat_algorithmic_bytes then moves
                               that layer's edge bytes to this class) */
    GAT_K_COUNT = 11
};
/* Accumulated HIP-event time of kernel class `k` since the last gat_kernel_stats_reset (needs
 * collect_timing=1).  Synchronises the stream. */
int gat_kernel_stats(gat_ctx* ctx, int k, int64_t* launches, double* total_ms);
int gat_kernel_stats_reset(gat_ctx* ctx);
const char* gat_kernel_name(int k);
/* Algorithmic HBM bytes of one forward+backward step on this context's shard. */
int gat_algorithmic_bytes(gat_ctx* ctx, double* bytes_step, double* bytes_per_kernel /* [GAT_K_COUNT] or NULL */);
/* The same figure from the shape alone (host arithmetic, no device, no context): SURVEY §8d's formula with
 * b = 4 (GAT_DTYPE_F32) or 2 (GAT_DTYPE_BF16) bytes on every float term.  n_table / replicated_input describe a
 * destination-range shard (single GPU: n_table = n_rows, replicated_input = 0).  Only cfg->num_layers, heads,
 * outdims, in_dim, num_classes and storage_dtype are read. */
int gat_algorithmic_bytes_shape(const gat_config* cfg, int64_t n_rows, int64_t n_edges, int64_t n_table,
                                int32_t replicated_input, double* bytes_step, double* bytes_per_kernel);
/* The same model at the granularity the memory fabric serves: every per-edge gathered / scattered row (PL[src] in both edge
 * passes, the gPL scatter) rounded up to whole 128-byte requests.  Equal to the figure above when a row is a multiple of 128 B
 * (fp32, H*D = 64); larger for bf16 rows at H*D < 64 (BASELINE config 5: 64-byte rows cost a line each) — the roofline such a
 * shape can actually be served at.  bench.py reports it as `frac_request_granular`. */
int gat_request_bytes_shape(const gat_config* cfg, int64_t n_rows, int64_t n_edges, int64_t n_table,
                            int32_t replicated_input, double* bytes_step, double* bytes_per_kernel);

#ifdef __cplusplus
}
#endif
#endif /* GATV2_ABI_H */
