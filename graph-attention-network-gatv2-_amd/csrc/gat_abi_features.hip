// gat_abi_features.hip — the optional features of a context, switched on before it is complete: residual / bias, layer
// normalisation, edge features, graph-level readout, pair head, dropout / DropEdge / training mode.
#include "gat_ctx.h"

using namespace gat;
extern "C" {

// ---- residual / bias --------------------------------------------------------------------------------------------
int gat_set_residual(gat_ctx* c, int32_t flags) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (flags & ~(GAT_RES_LINEAR | GAT_RES_BIAS)) return fail(GAT_E_INVALID, "gat_set_residual: unknown flag bits");
    GAT_LAYOUT_OPEN(c, "gat_set_residual");
    if (flags == c->res.flags) return 0;                 // (0 on a fresh context: nothing is touched)
    GAT_REFUSE_DBG(c, flags != 0, "gat_set_residual", " (those kernels have no residual form)");
    c->res.flags = flags;
    return relayout(c);
}
// ---- layer normalisation ----------------------------------------------------------------------------------------
int gat_set_norm(gat_ctx* c, int32_t flags, float eps) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (flags & ~(GAT_NORM_LAYER | GAT_NORM_SKIP_LAST)) return fail(GAT_E_INVALID, "gat_set_norm: unknown flag bits");
    if ((flags & GAT_NORM_SKIP_LAST) && !(flags & GAT_NORM_LAYER)) return fail(GAT_E_INVALID, "gat_set_norm: GAT_NORM_SKIP_LAST needs GAT_NORM_LAYER");
    if (flags != 0 && !(std::isfinite(eps) && eps > 0.f)) return fail(GAT_E_INVALID, "gat_set_norm: eps must be finite and > 0");
    GAT_LAYOUT_OPEN(c, "gat_set_norm");
    if (flags == 0 && c->res.norm_flags == 0) return 0;      // the default: nothing is touched
    if (flags != 0 && c->cfg.flat_lrelu_index)
        return fail(GAT_E_UNSUPPORTED, "gat_set_norm: not with flat_lrelu_index (the reference's flat index has no meaning on the normalised row)");
    if (flags != 0 && bn_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_set_norm: not on a context with batch normalisation (gat_set_batch_norm): one normaliser per context");
    GAT_REFUSE_DBG(c, flags != 0, "gat_set_norm", " (those kernels have no normalised form)");
    c->res.norm_flags = flags; c->res.norm_eps = flags != 0 ? eps : 0.f;
    return relayout(c);
}
// ---- batch normalisation ----------------------------------------------------------------------------------------
int gat_set_batch_norm(gat_ctx* c, int32_t flags, float eps, float momentum) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (flags & ~(GAT_BN_ON | GAT_BN_SKIP_LAST)) return fail(GAT_E_INVALID, "gat_set_batch_norm: unknown flag bits");
    if ((flags & GAT_BN_SKIP_LAST) && !(flags & GAT_BN_ON)) return fail(GAT_E_INVALID, "gat_set_batch_norm: GAT_BN_SKIP_LAST needs GAT_BN_ON");
    if (flags != 0 && !(std::isfinite(eps) && eps > 0.f)) return fail(GAT_E_INVALID, "gat_set_batch_norm: eps must be finite and > 0");
    if (flags != 0 && !(std::isfinite(momentum) && momentum >= 0.f && momentum <= 1.f)) return fail(GAT_E_INVALID, "gat_set_batch_norm: momentum must be in [0, 1]");
    GAT_LAYOUT_OPEN(c, "gat_set_batch_norm");
    if (flags == 0 && c->res.bn_flags == 0) return 0;        // the default: nothing is touched
    if (flags != 0 && norm_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_set_batch_norm: not on a context with layer normalisation (gat_set_norm): one normaliser per context");
    if (flags != 0 && c->cfg.flat_lrelu_index)
        return fail(GAT_E_UNSUPPORTED, "gat_set_batch_norm: not with flat_lrelu_index (the reference's flat index has no meaning on the normalised row)");
    GAT_REFUSE_DBG(c, flags != 0, "gat_set_batch_norm", " (those kernels have no normalised form)");
    c->res.bn_flags = flags; c->res.bn_eps = flags != 0 ? eps : 0.f; c->res.bn_momentum = flags != 0 ? momentum : 0.f;
    GAT_TRY(relayout(c));
    if (flags != 0 && !c->res.bn_stats) {                    // the statistics: allocated once and never moved (a captured step keeps its pointers)
        int64_t total = 0;
        for (const Layer& y : c->layers) total += y.HD;
        c->res.bn_total = total;
        GAT_TRY(dalloc(c, &c->res.bn_stats, 4 * total));
        std::vector<float> init((size_t)(4 * total), 0.f);
        std::fill(init.begin() + total, init.begin() + 2 * total, 1.0f);      // running mean 0, running var 1
        GAT_HIP(hipMemcpy(c->res.bn_stats, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return 0;
}
int gat_batch_norm_info(gat_ctx* c, int32_t* flags, float* eps, float* momentum) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (flags) *flags = c->res.bn_flags;
    if (eps) *eps = c->res.bn_eps;
    if (momentum) *momentum = c->res.bn_momentum;
    return 0;
}
static int bn_stats_access(gat_ctx* c, const char* who, int32_t which, const void* host, int64_t count, int32_t max_which) {
    if (!c || !host) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (!bn_on(c) || !c->res.bn_stats) return fail(GAT_E_STATE, std::string(who) + ": the context has no batch normalisation (gat_set_batch_norm)");
    if (which < 0 || which > max_which)
        return fail(GAT_E_INVALID, std::string(who) + (max_which == GAT_BN_RUNNING_VAR ? ": only GAT_BN_RUNNING_MEAN and GAT_BN_RUNNING_VAR can be set" : ": unknown statistic"));
    if (count != c->res.bn_total) return fail(GAT_E_INVALID, std::string(who) + ": count mismatch (sum over the layers of H*D)");
    return 0;
}
int gat_batch_norm_stats_get(gat_ctx* c, int32_t which, float* host, int64_t count) {
    GAT_TRY(bn_stats_access(c, "gat_batch_norm_stats_get", which, host, count, GAT_BN_BATCH_RSTD));
    GAT_HIP(hipMemcpyAsync(host, c->res.bn_stats + (int64_t)which * c->res.bn_total, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
int gat_batch_norm_stats_set(gat_ctx* c, int32_t which, const float* host, int64_t count) {
    GAT_TRY(bn_stats_access(c, "gat_batch_norm_stats_set", which, host, count, GAT_BN_RUNNING_VAR));
    GAT_HIP(hipMemcpyAsync(c->res.bn_stats + (int64_t)which * c->res.bn_total, host, (size_t)count * sizeof(float), hipMemcpyHostToDevice, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));               // (the same buffer: a captured step graph reads the new values)
    return 0;
}
// ---- edge features ------------------------------------------------------------------------------------------------
int gat_set_edge_dim(gat_ctx* c, int32_t edge_dim) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (edge_dim < 0 || edge_dim > GAT_EDGE_DIM_MAX) return fail(GAT_E_INVALID, "gat_set_edge_dim: edge_dim must be in [0, " + std::to_string(GAT_EDGE_DIM_MAX) + "]");
    GAT_LAYOUT_OPEN(c, "gat_set_edge_dim");
    if (edge_dim == c->ef.dim) return 0;               // (0 on a fresh context: nothing is touched)
    GAT_REFUSE_DBG(c, edge_dim != 0, "gat_set_edge_dim", " (those kernels have no edge-feature form)");
    c->ef.dim = edge_dim; c->ef.ld = (edge_dim + 3) / 4 * 4;
    return relayout(c);
}
static int set_edge_features_common(gat_ctx* c, const float* ea, int64_t n_edges, int32_t edge_dim, hipMemcpyKind kind) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_set_edge_features: set the graph first (the rows are in the order of its CSR)");
    if (edge_dim != c->ef.dim) return fail(GAT_E_INVALID, "gat_set_edge_features: edge_dim differs from the context's (gat_set_edge_dim)");
    if (n_edges != c->graph.n_edges) return fail(GAT_E_INVALID, "gat_set_edge_features: row count differs from the graph's edge count");
    if (edge_dim == 0) return 0;                         // a context without the feature: nothing to copy
    if (!ea && n_edges > 0) return fail(GAT_E_INVALID, "gat_set_edge_features: null argument");
    const int64_t Ea = std::max<int64_t>(n_edges, 1);
    if (!c->ef.EA) {                                        // allocated once: a later call refills the same buffer (a captured step stays valid)
        GAT_TRY(dalloc(c, &c->ef.EA, Ea * c->ef.ld));
        GAT_HIP(hipMemsetAsync(c->ef.EA, 0, (size_t)(Ea * c->ef.ld) * sizeof(float), c->stream));
    }
    if (n_edges > 0)
        GAT_HIP(hipMemcpy2DAsync(c->ef.EA, (size_t)c->ef.ld * sizeof(float), ea, (size_t)edge_dim * sizeof(float), (size_t)edge_dim * sizeof(float),
                                 (size_t)n_edges, kind, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    c->ef.have = true;
    return 0;
}
int gat_set_edge_features(gat_ctx* c, const float* ea, int64_t n_edges, int32_t edge_dim) {
    return set_edge_features_common(c, ea, n_edges, edge_dim, hipMemcpyHostToDevice);
}
int gat_set_edge_features_device(gat_ctx* c, const float* d_ea, int64_t n_edges, int32_t edge_dim) {
    return set_edge_features_common(c, d_ea, n_edges, edge_dim, hipMemcpyDeviceToDevice);
}
// ---- hidden layer in front of the output head -----------------------------------------------------------------------
}  // extern "C"
namespace gat {
// The head's own limits with Dh in D_last's place.  mode_known: the loss mode is fixed (the context is being completed); before that
// only what holds for every mode is refused: C * Dh <= 2048.
static int hidden_width_check(gat_ctx* c, int32_t width, bool mode_known) {
    const int32_t C = c->cfg.num_classes;
    std::string limit;
    int rc = (int64_t)C * width > 2048 ? GAT_E_UNSUPPORTED : 0;
    if (rc) limit = "num_classes * width <= 2048";
    else if (mode_known) rc = head_shape_check(C, width, c->sup.loss_mode, &limit);
    if (rc) return fail(rc, "gat_set_head_hidden: width " + std::to_string(width) + " with num_classes " + std::to_string(C) + " is outside the output head's limit: " + limit);
    return 0;
}
int head_hidden_check(gat_ctx* c) {
    if (!hidden_on(c)) return 0;
    GAT_TRY(hidden_refuse_shard(c, c->graph.n_rows, c->graph.n_table));
    return hidden_width_check(c, c->hid.width, true);
}
}  // namespace gat
extern "C" {
int gat_set_head_hidden(gat_ctx* c, int32_t width, int32_t flags) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (width < 0) return fail(GAT_E_INVALID, "gat_set_head_hidden: width must be >= 0 (0 = no hidden layer)");
    if (flags & ~GAT_HEAD_ACT_LRELU) return fail(GAT_E_INVALID, "gat_set_head_hidden: unknown flag bits");
    if (width == 0 && c->hid.width == 0) return 0;       // the default: nothing is touched
    GAT_LAYOUT_OPEN(c, "gat_set_head_hidden");
    if (width > 0 && c->cfg.flat_lrelu_index)
        return fail(GAT_E_UNSUPPORTED, "gat_set_head_hidden: not with flat_lrelu_index = 1 (the head would write the last layer's g itself)");
    GAT_REFUSE_DBG(c, width > 0, "gat_set_head_hidden", "");
    if (width > 0) GAT_TRY(hidden_width_check(c, width, false));
    c->hid.width = width; c->hid.flags = width > 0 ? flags : 0;
    return relayout(c);
}
int gat_head_hidden_info(gat_ctx* c, int32_t* width, int32_t* flags) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (width) *width = c->hid.width;
    if (flags) *flags = c->hid.flags;
    return 0;
}
// ---- graph-level readout ------------------------------------------------------------------------------------------
static int set_readout_common(gat_ctx* c, int32_t mode, const int32_t* graph_ptr, int64_t n_graphs, bool on_host) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode < GAT_READOUT_NONE || mode > GAT_READOUT_MAX) return fail(GAT_E_INVALID, "gat_set_readout: mode must be 0 (none), 1 (mean), 2 (sum) or 3 (max)");
    if (mode == GAT_READOUT_NONE) return 0;              // the default: nothing is touched
    if (readout_on(c)) return fail(GAT_E_STATE, "gat_set_readout: readout already set (create a new context)");
    if (pairs_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_set_readout: not on a context with a pair head (gat_set_pairs)");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_set_readout: set the graph first");
    if (c->sup.have) return fail(GAT_E_STATE, "gat_set_readout: call it before gat_set_labels (the label, mask and head buffers are sized by it)");
    if (c->graph.n_table != c->graph.n_rows || c->xch.comm)
        return fail(GAT_E_UNSUPPORTED, "gat_set_readout: not on a destination-range shard or with a transport (a graph may straddle shards)");
    if (c->cfg.flat_lrelu_index)
        return fail(GAT_E_UNSUPPORTED, "gat_set_readout: not with flat_lrelu_index = 1 (the head would write the last layer's g itself)");
    GAT_REFUSE_DBG(c, true, "gat_set_readout", "");
    if (!graph_ptr) return fail(GAT_E_INVALID, "gat_set_readout: null graph_ptr");
    if (n_graphs < 1 || n_graphs >= 0x7fffffffLL) return fail(GAT_E_INVALID, "gat_set_readout: n_graphs must be >= 1 and fit int32");
    const int64_t N = c->graph.n_rows, G = n_graphs;
    int32_t problem = 0; int64_t where = -1;
    std::vector<int32_t> fetched;
    if (on_host) {
        GAT_TRY(graph_ptr_check_host(graph_ptr, G, N, &problem, &where));
    } else {                                             // the same rules on the caller's device array, before anything walks it
        GAT_TRY(graph_ptr_check_device(graph_ptr, G, N, &problem, &where, c->stream));
    }
    if (problem) return fail(GAT_E_INVALID, "gat_set_readout: " + graph_ptr_problem_text(problem, where, N));
    if (!on_host) {                                      // the work list is built on the host (as the edge passes' is)
        fetched.resize((size_t)G + 1);
        GAT_HIP(hipMemcpy(fetched.data(), graph_ptr, (size_t)(G + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    const int32_t* gp = on_host ? graph_ptr : fetched.data();
    ReadoutPlan plan;
    build_readout_plan(gp, G, plan);
    const int32_t DL = c->layers.back().D;
    GAT_TRY(dalloc(c, &c->readout.graph_ptr, G + 1));
    GAT_TRY(dalloc(c, &c->readout.node_graph, N));
    GAT_HIP(hipMemcpyAsync(c->readout.graph_ptr, gp, (size_t)(G + 1) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    GAT_TRY(upload_list(c, &c->readout.items, plan.items, 4));
    GAT_TRY(upload_list(c, &c->readout.split, plan.split, 4));
    GAT_TRY(dalloc(c, &c->readout.part, (int64_t)std::max<int32_t>(plan.n_parts, 1) * DL));
    if (mode == GAT_READOUT_MAX) {
        GAT_TRY(dalloc(c, &c->readout.part_arg, (int64_t)std::max<int32_t>(plan.n_parts, 1) * DL));
        GAT_TRY(dalloc(c, &c->readout.argmax, G * DL));
    }
    GAT_TRY(dalloc(c, &c->readout.P, G * DL));
    GAT_TRY(dalloc(c, &c->readout.gP, G * DL));
    GAT_TRY(launch_node_graph(c->readout.graph_ptr, G, N, c->readout.node_graph, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));            // (the host lists go out of scope)
    c->readout.n_items = plan.n_items; c->readout.n_split = plan.n_split;
    c->readout.mode = mode; c->readout.n_graphs = G;
    c->head.y_valid = false;                                  // the head's outputs change shape: nothing of an earlier forward stays
    graph_drop(c);
    return 0;
}
int gat_set_readout(gat_ctx* c, int32_t mode, const int32_t* graph_ptr, int64_t n_graphs) {
    return set_readout_common(c, mode, graph_ptr, n_graphs, true);
}
int gat_set_readout_device(gat_ctx* c, int32_t mode, const int32_t* d_graph_ptr, int64_t n_graphs) {
    return set_readout_common(c, mode, d_graph_ptr, n_graphs, false);
}
int gat_readout_info(gat_ctx* c, int32_t* mode, int64_t* n_graphs) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode) *mode = c->readout.mode;
    if (n_graphs) *n_graphs = c->readout.n_graphs;
    return 0;
}
// ---- pair head ----------------------------------------------------------------------------------------------------
// The scatter's work list from the incidence row_ptr (fetched to the host, cut as the readout's graphs are), into the context's buffers
static int pairs_plan(gat_ctx* c) {
    const int64_t N = c->graph.n_rows;
    std::vector<int32_t> ip((size_t)N + 1);
    GAT_HIP(hipMemcpy(ip.data(), c->pairs.inc_ptr, ip.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    ReadoutPlan plan;
    build_readout_plan(ip.data(), N, plan);
    GAT_HIP(hipMemcpyAsync(c->pairs.items, plan.items.data(), plan.items.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if (plan.n_split > 0) GAT_HIP(hipMemcpyAsync(c->pairs.split, plan.split.data(), plan.split.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));            // (the host lists go out of scope)
    c->pairs.n_items = plan.n_items; c->pairs.n_split = plan.n_split;
    return 0;
}
static int set_pairs_common(gat_ctx* c, int32_t mode, const int32_t* u, const int32_t* v, int64_t n_pairs, bool on_host) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode < GAT_PAIR_NONE || mode > GAT_PAIR_ADD) return fail(GAT_E_INVALID, "gat_set_pairs: mode must be 0 (none), 1 (mul) or 2 (add)");
    if (mode == GAT_PAIR_NONE) return 0;                 // the default: nothing is touched
    const bool first = !pairs_on(c);
    if (!first && (mode != c->pairs.mode || n_pairs != c->pairs.n_pairs))
        return fail(GAT_E_STATE, "gat_set_pairs: a later call replaces the pairs and keeps the mode and n_pairs (create a new context for others)");
    if (first) {
        if (readout_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_set_pairs: not on a readout context (gat_set_readout)");
        if (!c->graph.have) return fail(GAT_E_STATE, "gat_set_pairs: set the graph first");
        if (c->sup.have) return fail(GAT_E_STATE, "gat_set_pairs: call it before gat_set_labels / gat_set_targets (the label, target, mask and head buffers are sized by it)");
        if (c->graph.n_table != c->graph.n_rows || c->xch.comm)
            return fail(GAT_E_UNSUPPORTED, "gat_set_pairs: not on a destination-range shard or with a transport (an endpoint may live on another shard)");
        if (c->cfg.flat_lrelu_index)
            return fail(GAT_E_UNSUPPORTED, "gat_set_pairs: not with flat_lrelu_index = 1 (the head would write the last layer's g itself)");
        GAT_REFUSE_DBG(c, true, "gat_set_pairs", "");
    }
    if (!u || !v) return fail(GAT_E_INVALID, "gat_set_pairs: null argument");
    if (n_pairs < 1) return fail(GAT_E_INVALID, "gat_set_pairs: n_pairs must be >= 1");
    if (n_pairs >= (1ll << 30)) return fail(GAT_E_UNSUPPORTED, "gat_set_pairs: n_pairs must be below 2^30 (the incidence keys 2p + role go through the 32-bit graph builder)");
    const int64_t N = c->graph.n_rows, P = n_pairs;
    int64_t where = -1; int32_t value = 0;
    if (on_host) {
        where = pair_check_host(u, v, P, N);
        if (where >= 0) value = (where & 1) ? v[where >> 1] : u[where >> 1];
    } else {                                             // the same rule on the caller's device arrays, before anything reads through them
        GAT_TRY(pair_check_device(u, v, P, N, &where, &value, c->stream));
    }
    if (where >= 0) return fail(GAT_E_INVALID, "gat_set_pairs: " + pair_problem_text(where, value, N));
    if (first) {
        const int32_t DL = c->layers.back().D;
        // upper bounds of the work list over every pair list of this length: an item per node plus one per started segment of a long
        // node; a long node has more than kPairSegEntries of the 2P incidences
        const int64_t seg = 2 * P / kPairSegEntries + 1;
        GAT_TRY(dalloc(c, &c->pairs.u, P)); GAT_TRY(dalloc(c, &c->pairs.v, P));
        GAT_TRY(dalloc(c, &c->pairs.inc_ptr, N + 1)); GAT_TRY(dalloc(c, &c->pairs.inc, 2 * P));
        GAT_TRY(dalloc(c, &c->pairs.items, N + 2 * seg)); GAT_TRY(dalloc(c, &c->pairs.split, seg));
        GAT_TRY(dalloc(c, &c->pairs.part, 2 * seg * DL));
        GAT_TRY(dalloc(c, &c->pairs.Q, P * DL)); GAT_TRY(dalloc(c, &c->pairs.gQ, P * DL));
    }
    const hipMemcpyKind kind = on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    GAT_HIP(hipStreamSynchronize(c->stream));            // a step in flight still reads the old pairs
    GAT_HIP(hipMemcpyAsync(c->pairs.u, u, (size_t)P * sizeof(int32_t), kind, c->stream));
    GAT_HIP(hipMemcpyAsync(c->pairs.v, v, (size_t)P * sizeof(int32_t), kind, c->stream));
    GAT_TRY(pair_index_build(c->pairs.u, c->pairs.v, P, N, c->pairs.inc_ptr, c->pairs.inc, c->stream));
    GAT_TRY(pairs_plan(c));
    c->pairs.mode = mode; c->pairs.n_pairs = P;
    c->head.y_valid = false;                                  // nothing of an earlier forward stays
    graph_drop(c);                                            // the work list changed: no replay may survive
    return 0;
}
int gat_set_pairs(gat_ctx* c, int32_t mode, const int32_t* u, const int32_t* v, int64_t n_pairs) {
    return set_pairs_common(c, mode, u, v, n_pairs, true);
}
int gat_set_pairs_device(gat_ctx* c, int32_t mode, const int32_t* d_u, const int32_t* d_v, int64_t n_pairs) {
    return set_pairs_common(c, mode, d_u, d_v, n_pairs, false);
}
int gat_pairs_info(gat_ctx* c, int32_t* mode, int64_t* n_pairs) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode) *mode = c->pairs.mode;
    if (n_pairs) *n_pairs = c->pairs.n_pairs;
    return 0;
}
int gat_pairs_get(gat_ctx* c, int32_t* u_host, int32_t* v_host, int64_t n_pairs) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (!pairs_on(c)) return fail(GAT_E_STATE, "gat_pairs_get: no pair head (gat_set_pairs)");
    if (n_pairs != c->pairs.n_pairs) return fail(GAT_E_INVALID, "gat_pairs_get: n_pairs differs from the context's pair count");
    if (!u_host || !v_host) return fail(GAT_E_INVALID, "gat_pairs_get: null argument");
    GAT_HIP(hipStreamSynchronize(c->stream));
    GAT_HIP(hipMemcpy(u_host, c->pairs.u, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
    GAT_HIP(hipMemcpy(v_host, c->pairs.v, (size_t)n_pairs * sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}
// ---- negative sampling ------------------------------------------------------------------------------------------
int gat_set_negative_sampling(gat_ctx* c, int32_t mode, int64_t first, int64_t count, int32_t flags, uint64_t seed) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode < GAT_NEG_NONE || mode > GAT_NEG_CORRUPT) return fail(GAT_E_INVALID, "gat_set_negative_sampling: mode must be 0 (none), 1 (uniform) or 2 (corrupt)");
    if (mode == GAT_NEG_NONE) {                          // off: the pairs, the index and every buffer stay what they are
        auto& g = c->neg;
        g.mode = 0; g.flags = 0; g.first = g.count = 0; g.seed = 0; g.last_round = 0; g.unfiltered = 0;
        return 0;
    }
    if (!pairs_on(c)) return fail(GAT_E_STATE, "gat_set_negative_sampling: needs a pair head (gat_set_pairs comes first)");
    if (flags & ~(GAT_NEG_BOTH_DIRECTIONS | GAT_NEG_ALLOW_SELF)) return fail(GAT_E_INVALID, "gat_set_negative_sampling: unknown flag bits");
    if (count < 1 || first < 0 || first > c->pairs.n_pairs || count > c->pairs.n_pairs - first)
        return fail(GAT_E_INVALID, "gat_set_negative_sampling: the slots [first, first + count) must be at least one pair inside the pair list");
    if (mode == GAT_NEG_CORRUPT && first < 1) return fail(GAT_E_INVALID, "gat_set_negative_sampling: GAT_NEG_CORRUPT takes pairs [0, first) as its sources: first must be >= 1");
    const int64_t N = c->graph.n_rows;
    if (!c->neg.ascending_known) {
        GAT_TRY(csr_rows_ascending(c->graph.row_ptr, c->graph.col_idx, N, &c->neg.ascending, c->stream));
        c->neg.ascending_known = true;
    }
    if (!c->neg.counter) {
        GAT_TRY(dalloc(c, &c->neg.counter, 1));
        GAT_TRY(dalloc(c, &c->neg.plan_key, N + 1)); GAT_TRY(dalloc(c, &c->neg.plan_off, N + 1));
        GAT_TRY(pair_plan_temp_bytes(N, &c->neg.plan_temp_bytes));
        GAT_TRY(dmalloc(c, &c->neg.plan_temp, c->neg.plan_temp_bytes));
    }
    c->neg.mode = mode; c->neg.flags = flags; c->neg.first = first; c->neg.count = count; c->neg.seed = seed;
    c->neg.last_round = 0; c->neg.unfiltered = 0;
    return 0;
}
int gat_resample_negatives(gat_ctx* c, uint64_t round) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (c->neg.mode == GAT_NEG_NONE) return fail(GAT_E_STATE, "gat_resample_negatives: gat_set_negative_sampling comes first");
    auto& g = c->neg; auto& p = c->pairs;
    const int64_t N = c->graph.n_rows;
    GAT_HIP(hipStreamSynchronize(c->stream));            // a step in flight still reads the old pairs
    GAT_HIP(hipMemsetAsync(g.counter, 0, sizeof(unsigned long long), c->stream));
    NegSampleArgs a{};
    a.row_ptr = c->graph.row_ptr; a.col_idx = c->graph.col_idx; a.n_rows = N; a.ascending = g.ascending;
    a.mode = g.mode; a.flags = g.flags; a.seed = g.seed; a.round = round;
    a.src_u = p.u; a.src_v = p.v; a.n_src = g.first;     // (disjoint from the slots written below)
    a.u = p.u + g.first; a.v = p.v + g.first; a.count = g.count; a.unfiltered = g.counter;
    GAT_TRY(launch_negative_sample(a, c->stream));
    GAT_TRY(pair_index_build(p.u, p.v, p.n_pairs, N, p.inc_ptr, p.inc, c->stream));       // synchronises
    unsigned long long unfiltered = 0;
    GAT_HIP(hipMemcpy(&unfiltered, g.counter, sizeof(unfiltered), hipMemcpyDeviceToHost));
    int32_t n_parts = 0;
    GAT_TRY(pair_plan_device(p.inc_ptr, N, g.plan_key, g.plan_off, g.plan_temp, g.plan_temp_bytes, p.items, p.split, &p.n_items, &p.n_split, &n_parts, c->stream));
    g.last_round = round; g.unfiltered = (int64_t)unfiltered;
    c->head.y_valid = false;                                  // nothing of an earlier forward stays
    graph_drop(c);                                            // the work list changed: no replay may survive
    return 0;
}
int gat_negatives_info(gat_ctx* c, int32_t* mode, int64_t* first, int64_t* count, uint64_t* last_round, int64_t* unfiltered) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (mode) *mode = c->neg.mode;
    if (first) *first = c->neg.first;
    if (count) *count = c->neg.count;
    if (last_round) *last_round = c->neg.last_round;
    if (unfiltered) *unfiltered = c->neg.unfiltered;
    return 0;
}
// ---- dropout ---------------------------------------------------------------------------------------------------
int gat_set_dropout(gat_ctx* c, float feat_p, float attn_p, uint64_t seed, uint64_t first_step) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (!(feat_p >= 0.f && feat_p < 1.f)) return fail(GAT_E_INVALID, "gat_set_dropout: feat_p must be in [0, 1)");
    if (!(attn_p >= 0.f && attn_p < 1.f)) return fail(GAT_E_INVALID, "gat_set_dropout: attn_p must be in [0, 1)");
    GAT_REFUSE_DBG(c, feat_p > 0.f || attn_p > 0.f, "gat_set_dropout", " (those kernels have no dropout form)");
    GAT_TRY(ensure_drop_step(c));
    GAT_HIP(hipMemcpyAsync(c->drop.step, &first_step, sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    graph_drop(c);                                       // a captured step holds the other kernel sequence
    c->drop.pf = feat_p; c->drop.pa = attn_p; c->drop.seed = seed;
    return ensure_drop_buffers(c);
}
int gat_set_dropedge(gat_ctx* c, float edge_p, int32_t flags) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (!(edge_p >= 0.f && edge_p < 1.f)) return fail(GAT_E_INVALID, "gat_set_dropedge: edge_p must be in [0, 1)");
    if (flags & ~(GAT_DROPEDGE_KEEP_SELF | GAT_DROPEDGE_SHARED_LAYERS)) return fail(GAT_E_INVALID, "gat_set_dropedge: unknown flag bits");
    GAT_REFUSE_DBG(c, edge_p > 0.f, "gat_set_dropedge", " (those kernels have no dropout form)");
    GAT_TRY(ensure_drop_step(c));
    graph_drop(c);                                       // a captured step holds the other kernel sequence
    c->drop.edge_p = edge_p; c->drop.edge_flags = flags;
    return 0;
}
int gat_set_training(gat_ctx* c, int32_t training) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (training != 0 && training != 1) return fail(GAT_E_INVALID, "gat_set_training: 0 (eval) or 1 (training)");
    if (c->drop.training != (training == 1)) graph_drop(c);
    c->drop.training = training == 1;
    return 0;
}
int gat_dropout_step(gat_ctx* c, uint64_t* step) {
    if (!c || !step) return fail(GAT_E_INVALID, "null argument");
    *step = 0;
    if (!c->drop.step) return 0;
    GAT_HIP(hipMemcpyAsync(step, c->drop.step, sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // extern "C"
