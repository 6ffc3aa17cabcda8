// gat_abi_data.hip — what a context is given: the graph (CSR or edge list, host or device) and its work list, the layer-0 features,
// labels, train / eval masks, the loss mode and its targets, the shard bounds.
#include "gat_ctx.h"

namespace gat {

void build_worklist(const int32_t* rp, int64_t n_rows, WorkList& w) {
    static const int seg_env = [] { const char* e = choice_env("GAT_SEG_EDGES"); const int v = e ? atoi(e) : 0; return v >= 16 ? v : 0; }();
    // GAT_SEG_EDGES=<n>: sweep of the hub-row segment length.  Default 256 (swept on the Products shape); graphs with
    // few edges get shorter segments: the persistent backward's critical path is its longest item (a 256-edge segment
    // is 64 dependent gather steps), which at Arxiv size (1.17 M edges) was longer than everything else together
    // (Products shape 256; 64 below 16 M edges; Arxiv shape 32: 1.35 -> 1.29 ms; Pubmed shape 16: 0.34 -> 0.31 ms)
    const int64_t ne = rp[n_rows];
    const int kSegEdges = seg_env ? seg_env : (ne < (512 << 10) ? 16 : ne < (4 << 20) ? 32 : ne < (16 << 20) ? 64 : gat::kSegEdges);
    w.items.clear(); w.slot_info.clear(); w.n_slots = 0; w.n_split = 0;
    std::vector<int32_t> firsts;
    // pass 1: segments of split rows first (the longest items start earliest)
    for (int64_t r = 0; r < n_rows; ++r) {
        const int32_t b = rp[r], e = rp[r + 1];
        if (e - b <= kSegEdges) continue;
        const int32_t nseg = (e - b + kSegEdges - 1) / kSegEdges, first = w.n_slots;
        firsts.push_back(first);
        for (int32_t sgm = 0; sgm < nseg; ++sgm) {
            const int32_t sb = b + sgm * kSegEdges, se = std::min(e, sb + kSegEdges);
            const int32_t item = (int32_t)(w.items.size() / 4);
            w.items.insert(w.items.end(), {(int32_t)r, sb, se, w.n_slots});
            w.slot_info.insert(w.slot_info.end(), {(int32_t)r, first, nseg, item});
            ++w.n_slots;
        }
    }
    // pass 2: every other row is one item.  The group-per-row kernels put 64/(H*D/N) consecutive items side by side in
    // one wave, each lane group walking its own row, so neighbours should be of (nearly) equal length: rows are sorted
    // by in-degree, longest first (counting sort, row order kept inside a degree) — inside WINDOWS of consecutive
    // rows, so that the list still walks the graph roughly in row order (the per-row reads and writes of PR / h_pre / g
    // stay near each other).  GAT_SORT_WINDOW rows per window, 0 = one window over all rows; swept on the Products
    // shape: 4096 and one window are within noise for the backward, 4096 is ~3 % better for the forward.
    {
        static const int64_t win_env = [] { const char* e = choice_env("GAT_SORT_WINDOW"); return e ? atoll(e) : (int64_t)-1; }();
        const int64_t win = win_env < 0 ? 4096 : (win_env == 0 ? n_rows : win_env);
        std::vector<int64_t> cnt((size_t)kSegEdges + 2);
        for (int64_t r0 = 0; r0 < n_rows; r0 += win) {
            const int64_t r1 = std::min(n_rows, r0 + win);
            std::fill(cnt.begin(), cnt.end(), 0);
            for (int64_t r = r0; r < r1; ++r) { const int32_t d = rp[r + 1] - rp[r]; if (d <= kSegEdges) ++cnt[(size_t)(kSegEdges - d) + 1]; }
            for (size_t i = 1; i < cnt.size(); ++i) cnt[i] += cnt[i - 1];
            const size_t base = w.items.size();
            w.items.resize(base + 4 * (size_t)cnt.back());
            for (int64_t r = r0; r < r1; ++r) {
                const int32_t b = rp[r], e = rp[r + 1];
                if (e - b > kSegEdges) continue;
                int32_t* it = &w.items[base + 4 * (size_t)cnt[(size_t)(kSegEdges - (e - b))]++];
                it[0] = (int32_t)r; it[1] = b; it[2] = e; it[3] = -1;
            }
        }
    }
    w.n_items = (int64_t)(w.items.size() / 4);
    w.n_split = (int32_t)firsts.size();                 // appended after the per-slot entries: one int4 per split row
    for (int32_t f : firsts) w.slot_info.insert(w.slot_info.end(), {f, 0, 0, 0});
}

}  // namespace gat

using namespace gat;
extern "C" {

// rows of in_dim floats -> rows of ld0 floats with zeros behind column in_dim
static int upload_rows_padded(gat_ctx* c, float* dst, const float* src, int64_t n_rows, int32_t in_dim, hipMemcpyKind kind) {
    if (c->in.ld0 == in_dim) {
        GAT_HIP(hipMemcpyAsync(dst, src, (size_t)n_rows * in_dim * sizeof(float), kind, c->stream));
        return 0;
    }
    GAT_HIP(hipMemsetAsync(dst, 0, (size_t)n_rows * c->in.ld0 * sizeof(float), c->stream));
    GAT_HIP(hipMemcpy2DAsync(dst, (size_t)c->in.ld0 * sizeof(float), src, (size_t)in_dim * sizeof(float), (size_t)in_dim * sizeof(float), (size_t)n_rows, kind, c->stream));
    return 0;
}
// c->graph.row_ptr / c->graph.col_idx are in place: the work list (from the host's row_ptr, or a copy fetched here), then the buffers
static int finish_graph(gat_ctx* c, const int32_t* host_row_ptr) {
    if (host_row_ptr) {
        build_worklist(host_row_ptr, c->graph.n_rows, c->graph.work);
    } else {
        std::vector<int32_t> h(c->graph.n_rows + 1);
        GAT_HIP(hipMemcpy(h.data(), c->graph.row_ptr, (c->graph.n_rows + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
        build_worklist(h.data(), c->graph.n_rows, c->graph.work);
    }
    c->graph.have = true;
    return ensure_buffers(c);
}
static int set_graph_common(gat_ctx* c, const int32_t* row_ptr, const int32_t* col_idx, int64_t n_rows,
                            int64_t n_edges, int64_t n_table, int64_t table_row0, hipMemcpyKind kind) {
    if (!c || !row_ptr || (!col_idx && n_edges > 0)) return fail(GAT_E_INVALID, "gat_set_graph: null argument");
    if (c->graph.have) return fail(GAT_E_STATE, "gat_set_graph: graph already set (create a new context)");
    c->packed.touched = true;                        // from here on gat_set_residual is refused
    if (n_rows <= 0 || n_edges < 0) return fail(GAT_E_INVALID, "gat_set_graph: bad sizes");
    if (n_edges > 0x7fffffffLL || n_rows >= 0x7fffffffLL || n_table > 0x7fffffffLL)
        return fail(GAT_E_UNSUPPORTED, "gat_set_graph: int32 CSR limits (E:1045-1046) exceeded");
    if (table_row0 < 0 || table_row0 + n_rows > n_table) return fail(GAT_E_INVALID, "gat_set_graph: shard rows outside the table");
    GAT_TRY(hidden_refuse_shard(c, n_rows, n_table));
    GAT_TRY(bn_refuse_shard(c, n_rows, n_table, table_row0));
    if (kind == hipMemcpyHostToDevice) {
        if (row_ptr[0] != 0 || (int64_t)row_ptr[n_rows] != n_edges)
            return fail(GAT_E_INVALID, "Invalid row_ptr: must start at 0 and end at the edge count");
        for (int64_t i = 0; i < n_rows; ++i)
            if (row_ptr[i + 1] < row_ptr[i]) return fail(GAT_E_INVALID, "Invalid row_ptr: not monotone");
        for (int64_t e = 0; e < n_edges; ++e)
            if (col_idx[e] < 0 || (int64_t)col_idx[e] >= n_table) return fail(GAT_E_INVALID, "col_idx entry outside the node table");
    } else {    // the same rules on the caller's device arrays, before anything walks them (one pass, gat_graph.hip)
        int32_t problem = 0; int64_t where = -1;
        GAT_TRY(csr_check_device(row_ptr, col_idx, n_rows, n_edges, n_table, &problem, &where, c->stream));
        if (problem) return fail(GAT_E_INVALID, csr_problem_text(problem));
    }
    c->graph.n_rows = n_rows; c->graph.n_edges = n_edges; c->graph.n_table = n_table; c->graph.table_row0 = table_row0;
    GAT_TRY(dalloc(c, &c->graph.row_ptr, n_rows + 1));
    GAT_TRY(dalloc(c, &c->graph.col_idx, n_edges));
    GAT_HIP(hipMemcpyAsync(c->graph.row_ptr, row_ptr, (n_rows + 1) * sizeof(int32_t), kind, c->stream));
    if (n_edges > 0) GAT_HIP(hipMemcpyAsync(c->graph.col_idx, col_idx, n_edges * sizeof(int32_t), kind, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return finish_graph(c, kind == hipMemcpyHostToDevice ? row_ptr : nullptr);
}
int gat_set_graph(gat_ctx* c, const int32_t* row_ptr, const int32_t* col_idx, int64_t n_rows, int64_t n_edges,
                  int64_t n_table, int64_t table_row0) {
    return set_graph_common(c, row_ptr, col_idx, n_rows, n_edges, n_table, table_row0, hipMemcpyHostToDevice);
}
int gat_set_graph_device(gat_ctx* c, const int32_t* row_ptr, const int32_t* col_idx, int64_t n_rows,
                         int64_t n_edges, int64_t n_table, int64_t table_row0) {
    return set_graph_common(c, row_ptr, col_idx, n_rows, n_edges, n_table, table_row0, hipMemcpyDeviceToDevice);
}

// Build the CSR from an edge list on the device (gat_graph.hip) straight into the context's arrays, then as above.
static int set_graph_coo_common(gat_ctx* c, const int32_t* src, const int32_t* dst, int64_t n_in, int64_t n_rows, int64_t n_table,
                                int64_t table_row0, int32_t flags, bool on_host) {
    if (!c || ((!src || !dst) && n_in > 0)) return fail(GAT_E_INVALID, "gat_set_graph_coo: null argument");
    if (c->graph.have) return fail(GAT_E_STATE, "gat_set_graph: graph already set (create a new context)");
    c->packed.touched = true;                        // from here on gat_set_residual is refused
    if (n_in < 0 || n_in > 0x7fffffffLL) return fail(n_in < 0 ? GAT_E_INVALID : GAT_E_UNSUPPORTED, "gat_set_graph_coo: edge count outside the 32-bit count of the sort");
    GAT_TRY(hidden_refuse_shard(c, n_rows, n_table));
    GAT_TRY(bn_refuse_shard(c, n_rows, n_table, table_row0));
    int32_t *d_src = nullptr, *d_dst = nullptr;
    if (on_host && n_in > 0) {
        GAT_TRY(dalloc(c, &d_src, n_in));
        if (int rc = dalloc(c, &d_dst, n_in)) { dfree(c, d_src); return rc; }
        hipError_t e = hipMemcpyAsync(d_src, src, n_in * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_dst, dst, n_in * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { dfree(c, d_src); dfree(c, d_dst); return fail((int)e, std::string("gat_set_graph_coo: upload: ") + hipGetErrorString(e)); }
        src = d_src; dst = d_dst;
    }
    CooBuild b;
    int rc = coo_sort(src, dst, n_in, n_rows, n_table, table_row0, flags, c->stream, &b);
    dfree(c, d_src); dfree(c, d_dst);
    if (rc) return rc;
    int32_t *rp = nullptr, *ci = nullptr;
    const int64_t m = b.m;
    rc = dalloc(c, &rp, n_rows + 1);
    if (!rc) rc = dalloc(c, &ci, m);
    if (!rc) rc = coo_fill(&b, n_rows, rp, ci, c->stream);
    coo_free(&b);
    if (rc) { dfree(c, rp); dfree(c, ci); return rc; }
    c->graph.n_rows = n_rows; c->graph.n_edges = m; c->graph.n_table = n_table; c->graph.table_row0 = table_row0;
    c->graph.row_ptr = rp; c->graph.col_idx = ci;
    return finish_graph(c, nullptr);
}
int gat_set_graph_coo(gat_ctx* c, const int32_t* src, const int32_t* dst, int64_t n_in, int64_t n_rows, int64_t n_table,
                      int64_t table_row0, int32_t flags) {
    return set_graph_coo_common(c, src, dst, n_in, n_rows, n_table, table_row0, flags, true);
}
int gat_set_graph_coo_device(gat_ctx* c, const int32_t* d_src, const int32_t* d_dst, int64_t n_in, int64_t n_rows, int64_t n_table,
                             int64_t table_row0, int32_t flags) {
    return set_graph_coo_common(c, d_src, d_dst, n_in, n_rows, n_table, table_row0, flags, false);
}
int gat_graph_size(gat_ctx* c, int64_t* n_rows, int64_t* n_edges, int64_t* n_table) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_graph_size: no graph set");
    if (n_rows) *n_rows = c->graph.n_rows;
    if (n_edges) *n_edges = c->graph.n_edges;
    if (n_table) *n_table = c->graph.n_table;
    return 0;
}
int gat_graph_get(gat_ctx* c, int32_t* row_ptr_host, int32_t* col_idx_host) {
    if (!c || !row_ptr_host || (!col_idx_host && c->graph.have && c->graph.n_edges > 0)) return fail(GAT_E_INVALID, "gat_graph_get: null argument");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_graph_get: no graph set");
    GAT_HIP(hipStreamSynchronize(c->stream));
    GAT_HIP(hipMemcpy(row_ptr_host, c->graph.row_ptr, (c->graph.n_rows + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (c->graph.n_edges > 0) GAT_HIP(hipMemcpy(col_idx_host, c->graph.col_idx, c->graph.n_edges * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

static int set_features_common(gat_ctx* c, const float* x, int64_t n_rows, int32_t in_dim, hipMemcpyKind kind) {
    if (!c || !x) return fail(GAT_E_INVALID, "gat_set_features: null argument");
    if (in_dim != c->cfg.in_dim) return fail(GAT_E_INVALID, "gat_set_features: in_dim differs from the config");
    if (c->graph.have && n_rows != c->graph.n_rows) return fail(GAT_E_INVALID, "gat_set_features: row count differs from the graph");
    c->in.ld0 = (in_dim + 3) / 4 * 4;
    if (!c->in.X0) GAT_TRY(dalloc(c, &c->in.X0, n_rows * c->in.ld0));
    GAT_TRY(upload_rows_padded(c, c->in.X0, x, n_rows, in_dim, kind));
    GAT_HIP(hipStreamSynchronize(c->stream));
    c->in.have = true;
    return ensure_buffers(c);
}
int gat_set_features(gat_ctx* c, const float* x, int64_t n_rows, int32_t in_dim) {
    return set_features_common(c, x, n_rows, in_dim, hipMemcpyHostToDevice);
}
int gat_set_features_device(gat_ctx* c, const float* x, int64_t n_rows, int32_t in_dim) {
    return set_features_common(c, x, n_rows, in_dim, hipMemcpyDeviceToDevice);
}
// The layer-0 input is static, so a shard may hold it for EVERY row of the source table instead of
// exchanging layer-0 projections: PL_0 is then computed locally for the whole table and
// gradW_left_0 is accumulated from the shard's partial gPL_0 table (the parameter-gradient
// all-reduce completes the sum) — layer 0 needs neither the all-gather nor the reduce-scatter.
static int set_source_features_common(gat_ctx* c, const float* x, int64_t n_table, int32_t in_dim, hipMemcpyKind kind) {
    if (!c || !x) return fail(GAT_E_INVALID, "gat_set_source_features: null argument");
    if (in_dim != c->cfg.in_dim) return fail(GAT_E_INVALID, "gat_set_source_features: in_dim differs from the config");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_set_source_features: set the graph first");
    if (n_table != c->graph.n_table) return fail(GAT_E_INVALID, "gat_set_source_features: row count differs from the source table");
    if (c->buffers_ready) return fail(GAT_E_STATE, "gat_set_source_features: call before the features/labels complete the context");
    if (c->in.X0) return fail(GAT_E_STATE, "gat_set_source_features: features already set (the table replaces gat_set_features)");
    c->in.ld0 = (in_dim + 3) / 4 * 4;
    GAT_TRY(dalloc(c, &c->in.Xtab, n_table * c->in.ld0));
    GAT_TRY(upload_rows_padded(c, c->in.Xtab, x, n_table, in_dim, kind));
    GAT_HIP(hipStreamSynchronize(c->stream));
    c->in.X0 = c->in.Xtab + c->graph.table_row0 * c->in.ld0;      // the shard's own rows are rows table_row0.. of the table
    c->in.have = true;
    return ensure_buffers(c);
}
int gat_set_source_features(gat_ctx* c, const float* x, int64_t n_table, int32_t in_dim) {
    return set_source_features_common(c, x, n_table, in_dim, hipMemcpyHostToDevice);
}
int gat_set_source_features_device(gat_ctx* c, const float* x, int64_t n_table, int32_t in_dim) {
    return set_source_features_common(c, x, n_table, in_dim, hipMemcpyDeviceToDevice);
}
int gat_layer_path(gat_ctx* c, int32_t l, int32_t* path) {
    if (!c || !path) return fail(GAT_E_INVALID, "null argument");
    if (l < 0 || l >= c->cfg.num_layers) return fail(GAT_E_INVALID, "layer index out of range");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_layer_path: set the graph first");
    const Layer& y = c->layers[l];
    *path = edge_fast_path(y.H, y.D, c->graph.n_table) ? GAT_PATH_FAST : (edge_fast_path(y.H, y.D, 1) ? GAT_PATH_GENERIC_SIZE : GAT_PATH_GENERIC_SHAPE);
    return 0;
}
int gat_layer_exchange(gat_ctx* c, int32_t l, int32_t* needed) {
    if (!c || !needed) return fail(GAT_E_INVALID, "null argument");
    if (l < 0 || l >= c->cfg.num_layers) return fail(GAT_E_INVALID, "layer index out of range");
    *needed = (c->graph.n_table != c->graph.n_rows) && !(l == 0 && c->in.Xtab);
    return 0;
}
static int set_labels_common(gat_ctx* c, const int32_t* labels, int64_t n_rows, hipMemcpyKind kind) {
    if (!c || !labels) return fail(GAT_E_INVALID, "gat_set_labels: null argument");
    if (c->sup.loss_mode != 0) return fail(GAT_E_STATE, "gat_set_labels: the context's loss mode takes float targets: call gat_set_targets");
    if (c->graph.have && n_rows != head_rows(c)) return fail(GAT_E_INVALID, pairs_on(c) ? "Invalid labels length (with a pair head: one per pair)" : readout_on(c) ? "Invalid labels length (with readout: one label per graph)" : "Invalid labels length");
    if (kind == hipMemcpyHostToDevice)
        for (int64_t i = 0; i < n_rows; ++i)
            if (labels[i] < 0 || labels[i] >= c->cfg.num_classes) return fail(GAT_E_INVALID, "label outside [0, num_classes)");
    if (c->sup.labels && n_rows != c->sup.n_labels) return fail(GAT_E_INVALID, "gat_set_labels: length differs from the labels set before");
    if (!c->sup.labels) GAT_TRY(dalloc(c, &c->sup.labels, n_rows));
    c->sup.n_labels = n_rows;
    GAT_HIP(hipMemcpyAsync(c->sup.labels, labels, n_rows * sizeof(int32_t), kind, c->stream));
    // an active training mask applies to the NEW labels too: labels_eff holds masked copies, not a view
    if (c->sup.labels_eff != nullptr) GAT_TRY(launch_apply_mask(c->sup.labels, c->sup.train_mask, c->sup.labels_eff_buf, n_rows, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    c->sup.have = true;
    c->sup.loss_locked = true;
    return ensure_buffers(c);
}
// ---- train / validation masks (the reference trains and evaluates on ALL nodes, README R:134: "later") ----------
static int upload_mask(gat_ctx* c, const uint8_t* mask, int64_t n_rows, uint8_t** dst) {
    if (!c->sup.have) return fail(GAT_E_STATE, "set the labels first");
    if (n_rows != c->sup.n_labels || (c->graph.have && n_rows != head_rows(c)))
        return fail(GAT_E_INVALID, std::string("mask length differs from the ") + head_row_name(c) + " count" + (pairs_on(c) ? " (with a pair head: one per pair)" : ""));
    if (!*dst) GAT_TRY(dalloc(c, dst, n_rows));
    GAT_HIP(hipMemcpyAsync(*dst, mask, (size_t)n_rows, hipMemcpyHostToDevice, c->stream));
    return 0;
}
int gat_set_train_mask(gat_ctx* c, const uint8_t* mask, int64_t n_rows) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (c->sup.loss_mode != 0) {                        // the BCE / MSE head reads the mask byte of a row itself: no labels_eff
        if (mask) {
            GAT_TRY(upload_mask(c, mask, n_rows, &c->sup.train_mask));
            GAT_HIP(hipStreamSynchronize(c->stream));
        }
        c->sup.mask_on = mask != nullptr;
        graph_drop(c);                          // a captured step holds the old mask pointer (or none)
        return 0;
    }
    if (!mask) {                                    // back to the reference's behaviour: every node trains
        c->sup.labels_eff = nullptr;                    // (the buffer stays owned by the context)
        graph_drop(c);
        return 0;
    }
    GAT_TRY(upload_mask(c, mask, n_rows, &c->sup.train_mask));
    if (!c->sup.labels_eff_buf) GAT_TRY(dalloc(c, &c->sup.labels_eff_buf, n_rows));      // one buffer, reused by later calls
    GAT_TRY(launch_apply_mask(c->sup.labels, c->sup.train_mask, c->sup.labels_eff_buf, n_rows, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    c->sup.labels_eff = c->sup.labels_eff_buf;
    graph_drop(c);                              // a captured step holds the old label pointer
    return 0;
}
// gat_eval_mask in the BCE / MSE modes: the forward kernel with the given mask in place of the training mask — the sum of the loss
// terms and the correct count over the present entries of the mask's rows, from the head's input rows of the last forward
static int eval_mask_targets(gat_ctx* c, const uint8_t* mask, int64_t n_rows, double* loss_sum, int32_t* n_correct, int32_t* n_nodes) {
    GAT_TRY(upload_mask(c, mask, n_rows, &c->sup.mask_tmp));
    HeadArgs a = head_args(c);
    const int blocks = loss_head_blocks(a.n_rows, a.C, a.DL, a.mode);
    if (blocks < 0) return fail(GAT_E_UNSUPPORTED, "output head: num_classes*D_last too large for the LDS tile");
    if (!c->sup.eval_loss) { GAT_TRY(dalloc(c, &c->sup.eval_loss, head_blocks(a.n_rows))); GAT_TRY(dalloc(c, &c->sup.eval_cnt, head_blocks(a.n_rows))); }
    a.mask = c->sup.mask_tmp; a.loss_partial = c->sup.eval_loss; a.correct_partial = c->sup.eval_cnt; a.loss_out = nullptr; a.correct_out = nullptr;
    {
        Scope t(c, GAT_K_HEAD_FWD);
        GAT_TRY(launch_head_forward(a, c->stream));
    }
    c->head.y_valid = true;                              // (y does not depend on the mask)
    std::vector<double> hl((size_t)blocks); std::vector<int32_t> hc((size_t)blocks);
    GAT_HIP(hipMemcpyAsync(hl.data(), c->sup.eval_loss, (size_t)blocks * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipMemcpyAsync(hc.data(), c->sup.eval_cnt, (size_t)blocks * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    double l = 0.0; int64_t cr = 0, nn = 0;
    for (int b = 0; b < blocks; ++b) { l += hl[(size_t)b]; cr += hc[(size_t)b]; }
    for (int64_t i = 0; i < n_rows; ++i) nn += mask[i] != 0;
    if (loss_sum) *loss_sum = l;
    if (n_correct) *n_correct = (int32_t)cr;
    if (n_nodes) *n_nodes = (int32_t)nn;
    return 0;
}
int gat_eval_mask(gat_ctx* c, const uint8_t* mask, int64_t n_rows, double* loss_sum, int32_t* n_correct, int32_t* n_nodes) {
    GAT_TRY(check_layer(c, 0));
    if (!mask) return fail(GAT_E_INVALID, "gat_eval_mask: null mask");
    if (c->sup.loss_mode != 0) return eval_mask_targets(c, mask, n_rows, loss_sum, n_correct, n_nodes);
    if (!c->head.y_valid) GAT_TRY(gat_head_forward(c, nullptr, nullptr));     // after a fused head step: y = f(H_L, Wo), both still there
    GAT_TRY(upload_mask(c, mask, n_rows, &c->sup.mask_tmp));
    const int blocks = 256;
    if (!c->sup.eval_loss) { GAT_TRY(dalloc(c, &c->sup.eval_loss, blocks)); GAT_TRY(dalloc(c, &c->sup.eval_cnt, 2 * blocks)); }
    GAT_TRY(launch_eval_mask(c->head.y, c->sup.labels, c->sup.mask_tmp, n_rows, c->cfg.num_classes, c->sup.eval_loss, c->sup.eval_cnt, blocks, c->stream));
    std::vector<double> hl(blocks); std::vector<int32_t> hc(2 * blocks);
    GAT_HIP(hipMemcpyAsync(hl.data(), c->sup.eval_loss, blocks * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipMemcpyAsync(hc.data(), c->sup.eval_cnt, 2 * blocks * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    double l = 0.0; int64_t cr = 0, nn = 0;
    for (int b = 0; b < blocks; ++b) { l += hl[b]; cr += hc[2 * b]; nn += hc[2 * b + 1]; }
    if (loss_sum) *loss_sum = l;
    if (n_correct) *n_correct = (int32_t)cr;
    if (n_nodes) *n_nodes = (int32_t)nn;
    return 0;
}
// Ranking metrics of the last forward over a split (gatv2_abi.h "ranking metrics"): y as gat_eval_mask takes it, the mask in mask_tmp, the
// call's buffers allocated once.  Reads y, the labels / targets and the mask; writes only its own buffers: a later step sees nothing of it.
int gat_eval_rank(gat_ctx* c, const uint8_t* mask, int64_t n_rows, const int32_t* ks, int32_t n_ks, gat_rank_stats* out) {
    GAT_TRY(check_layer(c, 0));
    if (c->sup.loss_mode == GAT_LOSS_MSE) return fail(GAT_E_UNSUPPORTED, "gat_eval_rank: not with GAT_LOSS_MSE (a regression target has no binary relevance)");
    if (c->graph.n_table != c->graph.n_rows || c->graph.table_row0 != 0 || c->xch.comm)
        return fail(GAT_E_UNSUPPORTED, "gat_eval_rank: not on a destination-range shard or a context with a transport (a ranking is global: it cannot be summed over shards)");
    const int32_t C = c->cfg.num_classes;
    GAT_TRY(rank_check("gat_eval_rank", head_rows(c), C, ks, n_ks));
    if (!mask || !out) return fail(GAT_E_INVALID, "gat_eval_rank: null argument");
    if (!c->head.ran) return fail(GAT_E_STATE, "gat_eval_rank: no forward yet (call it after gat_forward or gat_step)");
    GAT_TRY(upload_mask(c, mask, n_rows, &c->sup.mask_tmp));
    if (!c->head.y_valid) GAT_TRY(gat_head_forward(c, nullptr, nullptr));     // after a fused head step: y = f(H_L, Wo), both still there
    RankSizes z;
    GAT_TRY(rank_sizes(n_rows, C, &z));
    if (!c->rank.have || z.slots != c->rank.sizes.slots || z.temp_bytes != c->rank.sizes.temp_bytes || z.partial_doubles != c->rank.sizes.partial_doubles) {
        RankBuffers& b = c->rank.buf;                   // first use (the head's rows and C are fixed for the context's life; a change: again)
        for (void* p : {(void*)b.keys0, (void*)b.keys1, (void*)b.incl, b.temp, (void*)b.seg, (void*)b.stats, (void*)b.partial, (void*)b.ks}) dfree(c, p);
        b = RankBuffers{};
        c->rank.have = false;
        GAT_TRY(rank_buffers_get(&b, z, C, [c](void** p, size_t bytes) { return dmalloc(c, p, bytes); }));
        c->rank.sizes = z; c->rank.have = true;
    }
    RankArgs a{};
    a.scores = c->head.y; a.score_stride = C;
    a.labels = c->sup.loss_mode == 0 ? c->sup.labels : nullptr; a.targets = c->sup.loss_mode == 0 ? nullptr : c->sup.targets;
    a.mask = c->sup.mask_tmp; a.n_rows = n_rows; a.n_cols = C; a.ks = ks; a.n_ks = n_ks;
    {
        Scope t(c, GAT_K_MISC);
        GAT_TRY(launch_rank_stats(a, c->rank.buf, c->stream));
    }
    GAT_HIP(hipMemcpyAsync(out, c->rank.buf.stats, (size_t)C * sizeof(gat_rank_stats), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
int gat_set_labels(gat_ctx* c, const int32_t* labels, int64_t n_rows) {
    return set_labels_common(c, labels, n_rows, hipMemcpyHostToDevice);
}
int gat_set_labels_device(gat_ctx* c, const int32_t* labels, int64_t n_rows) {
    return set_labels_common(c, labels, n_rows, hipMemcpyDeviceToDevice);
}

// ---- loss modes of the output head (gatv2_abi.h) -------------------------------------------------------------------
int gat_set_loss(gat_ctx* c, int32_t mode) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode < GAT_LOSS_SOFTMAX_CE || mode > GAT_LOSS_MSE) return fail(GAT_E_INVALID, "gat_set_loss: mode must be 0 (softmax cross-entropy), 1 (BCE) or 2 (MSE)");
    if (c->sup.loss_locked) return fail(GAT_E_STATE, "gat_set_loss: call it before the first gat_set_labels / gat_set_targets call");
    if (mode == GAT_LOSS_SOFTMAX_CE) { c->sup.loss_mode = 0; return 0; }      // the default: nothing is touched
    if (c->cfg.flat_lrelu_index)
        return fail(GAT_E_UNSUPPORTED, "gat_set_loss: not with flat_lrelu_index = 1 (the BCE / MSE head writes gH only, never the last layer's g)");
    GAT_REFUSE_DBG(c, true, "gat_set_loss", "");
    c->sup.loss_mode = mode;
    return 0;
}
int gat_loss_info(gat_ctx* c, int32_t* mode, int32_t* n_cols) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode) *mode = c->sup.loss_mode;
    if (n_cols) *n_cols = c->cfg.num_classes;
    return 0;
}
static int set_targets_common(gat_ctx* c, const float* t, int64_t n_rows, int32_t n_cols, bool on_host) {
    if (!c || !t) return fail(GAT_E_INVALID, "gat_set_targets: null argument");
    if (c->sup.loss_mode == 0) return fail(GAT_E_STATE, "gat_set_targets: the context's loss is softmax cross-entropy (gat_set_loss comes first); it takes gat_set_labels");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_set_targets: set the graph first (and gat_set_readout, on a readout context)");
    const int32_t C = c->cfg.num_classes;
    if (n_cols != C) return fail(GAT_E_INVALID, "gat_set_targets: n_cols differs from num_classes");
    if (n_rows < 0) return fail(GAT_E_INVALID, "gat_set_targets: negative n_rows");
    if (n_rows * (int64_t)C >= (1ll << 31)) return fail(GAT_E_UNSUPPORTED, "gat_set_targets: n_rows * n_cols >= 2^31 (n_correct is int32)");
    if (n_rows != head_rows(c)) return fail(GAT_E_INVALID, pairs_on(c) ? "gat_set_targets: n_rows differs from the pair count (with a pair head: one per pair)" : readout_on(c) ? "gat_set_targets: n_rows differs from the graph count (with readout: one target row per graph)" : "gat_set_targets: n_rows differs from the node count");
    const int64_t n = n_rows * C;
    if (!c->sup.tgt_scratch) GAT_TRY(dalloc(c, &c->sup.tgt_scratch, 256));
    int64_t bad = -1;
    if (on_host) bad = targets_check_host(t, n, c->sup.loss_mode);
    else GAT_TRY(targets_check_device(t, n, c->sup.loss_mode, c->sup.tgt_scratch, &bad, c->stream));      // before anything reads the array
    if (bad >= 0)
        return fail(GAT_E_INVALID, "gat_set_targets: entry " + std::to_string(bad) + " (row " + std::to_string(bad / C) + ", column " + std::to_string(bad % C) +
                                   (c->sup.loss_mode == GAT_LOSS_BCE ? ") is outside [0, 1] or infinite (BCE targets are probabilities or NaN)" : ") is infinite (MSE targets are finite or NaN)"));
    if (!c->sup.targets) GAT_TRY(dalloc(c, &c->sup.targets, n));                 // later calls have the same shape: the same buffer
    GAT_HIP(hipMemcpyAsync(c->sup.targets, t, (size_t)n * sizeof(float), on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    c->sup.n_labels = n_rows;
    c->sup.have = true;                          // the head's rows have their supervision: the buffers can be sized
    c->sup.loss_locked = true;
    return ensure_buffers(c);
}
int gat_set_targets(gat_ctx* c, const float* t, int64_t n_rows, int32_t n_cols) { return set_targets_common(c, t, n_rows, n_cols, true); }
int gat_set_targets_device(gat_ctx* c, const float* d_t, int64_t n_rows, int32_t n_cols) { return set_targets_common(c, d_t, n_rows, n_cols, false); }
int gat_target_count(gat_ctx* c, const uint8_t* mask, int64_t n_rows, int64_t* n_entries) {
    if (!c || !n_entries) return fail(GAT_E_INVALID, "gat_target_count: null argument");
    if (c->sup.loss_mode == 0 || !c->sup.targets) return fail(GAT_E_STATE, "gat_target_count: targets not set (gat_set_loss with BCE / MSE, then gat_set_targets)");
    const uint8_t* d_mask = c->sup.mask_on ? c->sup.train_mask : nullptr;       // null argument: the current training set
    if (mask) {
        GAT_TRY(upload_mask(c, mask, n_rows, &c->sup.mask_tmp));
        d_mask = c->sup.mask_tmp;
    }
    GAT_TRY(launch_target_count(c->sup.targets, d_mask, c->sup.n_labels, c->cfg.num_classes, c->sup.tgt_scratch, c->stream));
    unsigned long long part[256];
    GAT_HIP(hipMemcpyAsync(part, c->sup.tgt_scratch, sizeof(part), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    unsigned long long tot = 0;
    for (int b = 0; b < 256; ++b) tot += part[b];
    *n_entries = (int64_t)tot;
    return 0;
}
int gat_set_shard_bounds(gat_ctx* c, int32_t world, const int64_t* bounds) {
    if (!c || !bounds) return fail(GAT_E_INVALID, "null argument");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_set_shard_bounds: set the graph first");
    if (world < 1 || c->graph.n_table % world != 0) return fail(GAT_E_INVALID, "gat_set_shard_bounds: n_table is not world slices of equal size");
    const int64_t max_rows = c->graph.n_table / world;
    if (bounds[0] != 0) return fail(GAT_E_INVALID, "gat_set_shard_bounds: bounds[0] must be 0");
    for (int32_t r = 0; r < world; ++r)
        if (bounds[r + 1] < bounds[r] || bounds[r + 1] - bounds[r] > max_rows)
            return fail(GAT_E_INVALID, "gat_set_shard_bounds: every rank's row range must be ascending and fit its table slice");
    const int64_t rank = c->graph.table_row0 / max_rows;
    if (c->graph.table_row0 % max_rows != 0 || rank >= world || bounds[rank + 1] - bounds[rank] != c->graph.n_rows)
        return fail(GAT_E_INVALID, "gat_set_shard_bounds: bounds do not match this shard's table_row0 / n_rows");
    if (!c->drop.bounds) GAT_TRY(dalloc(c, &c->drop.bounds, (int64_t)world + 1));
    else if (c->drop.max_rows != max_rows) {
        dfree(c, c->drop.bounds);
        GAT_TRY(dalloc(c, &c->drop.bounds, (int64_t)world + 1));
    }
    GAT_HIP(hipMemcpyAsync(c->drop.bounds, bounds, ((size_t)world + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    graph_drop(c);
    c->drop.max_rows = max_rows;
    return 0;
}

}  // extern "C"
