// gat_abi_step.hip — the training step: the phase API (gat_layer_*, gat_head_*), the sequences behind gat_forward / gat_backward /
// gat_step (fused head, fused last layer, overlapped grad_w, the replayed step graph), the transports and the exchange tables.
#include "gat_ctx.h"

namespace gat {

// The whole step as ONE graph launch: small graphs (Cora / Pubmed / Arxiv shapes) are launch-bound — ~25
// kernels of a few microseconds each — so the sequence is captured once from the context's stream and
// replayed.  First call after arming runs eagerly (fills the occupancy caches, which may not be queried
// during capture), the second captures, later ones replay.  Everything the step touches has a fixed
// address once the context is complete; gat_bind_table re-arms.
void graph_drop(gat_ctx* c) {
    if (c->replay.exec) { (void)hipGraphExecDestroy(c->replay.exec); c->replay.exec = nullptr; }
    if (c->replay.graph) { (void)hipGraphDestroy(c->replay.graph); c->replay.graph = nullptr; }
    if (c->replay.state == 2) c->replay.state = 1;
    c->replay.warm = 0;
}
HeadArgs head_args(gat_ctx* c) {
    const Layer& y = c->layers.back();
    HeadArgs a{};
    a.mode = c->sup.loss_mode; a.Wo = Wo_of(c); a.X = y.hout; a.y = c->head.y;
    a.labels = c->sup.labels_eff ? c->sup.labels_eff : c->sup.labels;
    a.T = c->sup.targets; a.mask = c->sup.mask_on ? c->sup.train_mask : nullptr;
    a.hpre = y.hpre; a.g = y.g; a.gh_out = c->bwd.gH; a.gh_stride = c->bwd.gh_stride; a.gradWo = gWo_of(c); a.partial = c->head.hb_partial;
    a.loss_partial = c->head.loss_partial; a.correct_partial = c->head.correct_partial;
    a.loss_out = c->head.loss_out; a.correct_out = c->head.correct_out;
    a.n_rows = c->graph.n_rows; a.C = c->cfg.num_classes; a.DL = y.D; a.H = y.H;
    a.slope = c->cfg.negative_slope; a.flat_index = c->cfg.flat_lrelu_index;
    if (readout_on(c)) {
        // the head on the pooled rows: one row per graph, its gradient into gP (rows of D_last floats); the un-pool fills c->bwd.gH
        // afterwards and the last layer's edge backward expands that as always, so the head never writes a g of its own
        a.X = c->readout.P; a.n_rows = c->readout.n_graphs;
        a.g = nullptr; a.hpre = nullptr; a.gh_out = c->readout.gP; a.gh_stride = y.D;
    }
    if (pairs_on(c)) {
        // the head on the pair rows Q: one row per pair, its gradient into gQ; the scatter fills c->bwd.gH afterwards, as the un-pool does
        a.X = c->pairs.Q; a.n_rows = c->pairs.n_pairs;
        a.g = nullptr; a.hpre = nullptr; a.gh_out = c->pairs.gQ; a.gh_stride = y.D;
    }
    if (hidden_on(c)) {
        // the head on Z1 = act(Xin W1^T + b1), rows of Dh floats (Wo is [C][Dh]), its gradient into gZ1; the hidden stage's backward
        // fills the buffer the head's gradient went to before (gH, gP or gQ), so the head never writes a g of its own here either
        a.X = c->hid.Z1; a.DL = c->hid.width;
        a.g = nullptr; a.hpre = nullptr; a.gh_out = c->hid.gZ1; a.gh_stride = c->hid.width;
    }
    return a;
}
// gat_step: the head's forward and backward as ONE kernel when nothing needs the class probabilities in HBM
static bool fused_head(gat_ctx* c) { return !c->cfg.keep_taps && head_step_supported(head_args(c)); }
// gat_step: the last layer's forward edge pass, the output head and its backward edge pass fused per destination row
// (edge_last_fused_kernel) — single shard, fp32, H*D = 64 / D = 8 record path.  The idea: the separate backward finds nothing
// of the forward's rows left in the caches when a pass's gathers exceed the Infinity Cache; fused per row, the second walk of
// a row's sources comes a few microseconds after the first.
bool fused_last(gat_ctx* c) {
    if (c->sup.loss_mode != 0) return false;            // the BCE / MSE head runs the separate passes
    if (!fused_head(c) || bf16(c) || c->xch.comm || c->graph.n_table != c->graph.n_rows || c->cfg.flat_lrelu_index || res_route(c) || edge_feat_on(c) || readout_on(c) || pairs_on(c) || hidden_on(c)) return false;   // no residual / norm / edge-feature / readout / pair / hidden-head form
    const Layer& y = c->layers.back();
    if (!edge_fast_path(y.H, y.D, c->graph.n_table) || !y.stash || c->bwd.stash == nullptr || c->bwd.gH == nullptr) return false;
    if (!edge_last_fused_supported(y.H, y.D, c->cfg.num_classes) || c->dbg != 0 || drop_on(c)) return false;   // no dropout form
    // MEASURED, NOT THE DEFAULT (DESIGN §4 "Round 3"): on the Products shape the fused launch takes 5.0 ms for the 76 % of the edges
    // that sit in unsplit rows — what the separate forward + backward take for them — and the split rows' segments, launched on
    // their own, lose what they used to hide behind the bulk: 20.95 vs 20.78 ms per step.  GAT_FUSE_LAST=1 enables.
    static const int env = [] { const char* e = choice_env("GAT_FUSE_LAST"); return e ? (e[0] == '0' ? 0 : 1) : 0; }();
    return env == 1;
}

}  // namespace gat

using namespace gat;
extern "C" {

// ---- phases --------------------------------------------------------------------------------------------------
// What a layer's projection phase runs in front of PL / PR, whole (gat_layer_project) or in chunks (forward_exchange_pipelined).
// Training forward with dropout: layer 0 advances the step counter first (one lane, captured like any other kernel), then every
// layer with p_f > 0 writes its masked input x' = x (.) kappa s_f, which the projection and grad_W read instead of x.
static int project_side_terms(gat_ctx* c, int32_t l) {
    const Layer& y = c->layers[l];
    if (drop_on(c) && l == 0) GAT_TRY(launch_drop_advance(c->drop.step, c->stream));
    if (feat_drop_on(c)) {
        if (c->drop.x.empty() || (c->in.Xtab && !c->drop.x_tab)) GAT_TRY(ensure_drop_buffers(c));
        DropArgs d = drop_args(c, l, kDropFeat);
        GAT_TRY(launch_feat_drop_fwd(Xin_raw(c, l), c->drop.x[(size_t)l], c->graph.n_rows, y.F, ldX_of(c, l), d, c->stream));
        if (l == 0 && c->in.Xtab) {      // the replicated table: its rows are table rows, the same node ids
            d.row0 = 0;
            GAT_TRY(launch_feat_drop_fwd(c->in.Xtab, c->drop.x_tab, c->graph.n_table, y.F, c->in.ld0, d, c->stream));
        }
    }
    // edge features: PE = EA We^T over the E edges of the shard's own CSR — the residual term's product with rows = E, K = Fe
    if (y.PE != nullptr && c->graph.n_edges > 0) GAT_TRY(launch_project_res(c->ef.EA, We_of(c, l), y.PE, c->graph.n_edges, c->ef.dim, y.HD, c->stream, c->ef.ld));
    // residual: R = x' Wres^T over the shard's own rows (with replicated input: its own rows of the table) — the third projection
    if (y.R != nullptr) GAT_TRY(launch_project_res(Xin_of(c, l), Wres_of(c, l), y.R, c->graph.n_rows, y.F, y.HD, c->stream, ldX_of(c, l)));
    return 0;
}
int gat_layer_project(gat_ctx* c, int32_t l) {
    GAT_TRY(check_layer(c, l));
    GAT_TRY(check_edge_features(c));
    Layer& y = c->layers[l];
    Scope t(c, GAT_K_PROJECT);
    GAT_TRY(project_side_terms(c, l));
    if (l == 0 && c->in.Xtab) {      // replicated input: whole PL table from the table rows, PR from the shard's rows
        GAT_TRY(launch_project(Xtab_of(c), W_of(c, l), y.PL, nullptr, c->graph.n_table, y.F, y.HD, kPartLeft, bf16(c), c->bwd.gw_scratch, c->bwd.gw_scratch_floats, c->stream, c->in.ld0));
        return launch_project(Xin_of(c, 0), W_of(c, l), nullptr, y.PR, c->graph.n_rows, y.F, y.HD, kPartRight, bf16(c), c->bwd.gw_scratch, c->bwd.gw_scratch_floats, c->stream, c->in.ld0);
    }
    float* own_rows = reinterpret_cast<float*>(reinterpret_cast<char*>(y.PL) + c->graph.table_row0 * y.HD * st_bytes(c));
    return launch_project(Xin_of(c, l), W_of(c, l), own_rows, y.PR, c->graph.n_rows, y.F, y.HD, kPartBoth, bf16(c), c->bwd.gw_scratch, c->bwd.gw_scratch_floats, c->stream, ldX_of(c, l));
}

static EdgeFwdArgs plan_forward_edges(gat_ctx* c, int32_t l) {
    Layer& y = c->layers[l];
    EdgeFwdArgs a{};
    a.row_ptr = c->graph.row_ptr; a.col_idx = c->graph.col_idx; a.PL = y.PL; a.PR = y.PR; a.a = a_of(c, l);
    a.alpha = y.alpha; a.score = y.score; a.hpre = y.hpre; a.hout = y.hout; a.mstat = y.mstat; a.zstat = y.zstat;
    a.n_rows = c->graph.n_rows; a.n_table = c->graph.n_table; a.bf16 = bf16(c); a.H = y.H; a.D = y.D; a.is_last = (l == c->cfg.num_layers - 1);
    a.slope = c->cfg.negative_slope;
    set_work_list(a, c->graph.work, c->graph.items, c->graph.slot_info, c->graph.part_acc, c->graph.part_mz);
    return a;
}
// Batch-normalised layer, behind its edge forward (gatv2_abi.h "batch normalisation"): in training mode the column statistics of u = h_pre
// and their finish (mu, rstd, the running update), then hout = LReLU(v) over the LReLU(u) the edge forward left; eval mode: the apply
// launch alone, on the running statistics.  Plain launches on the context's stream: capturable, no host synchronisation.
static int bn_forward_layer(gat_ctx* c, int32_t l) {
    if (!bn_layer(c, l)) return 0;
    const Layer& y = c->layers[l];
    Scope t(c, GAT_K_MISC);
    if (c->drop.training)
        GAT_TRY(launch_batch_norm_stats(y.hpre, c->graph.n_rows, y.HD, c->res.bn_partial, c->res.bn_partial + (int64_t)kResPartialRows * c->HDmax,
                                        c->res.bn_eps, c->res.bn_momentum, bn_stat_of(c, GAT_BN_BATCH_MEAN, l), bn_stat_of(c, GAT_BN_BATCH_RSTD, l),
                                        bn_stat_of(c, GAT_BN_RUNNING_MEAN, l), bn_stat_of(c, GAT_BN_RUNNING_VAR, l), c->stream));
    return launch_batch_norm_apply(y.hpre, bn_stats_now(c, l), lng_of(c, l), lnb_of(c, l), c->cfg.negative_slope, y.hout, c->graph.n_rows, y.H, y.D,
                                   l == c->cfg.num_layers - 1, c->stream);
}
int gat_layer_forward_edges(gat_ctx* c, int32_t l) {
    GAT_TRY(check_layer(c, l));
    GAT_TRY(check_edge_features(c));
    const EdgeFwdArgs a = plan_forward_edges(c, l);
    EdgeFwdExtras x;                                 // masks, residual, bias, norm, edge term: whatever of them is on (launch_edge_forward: none = the plain kernels)
    x.drop = drop_args(c, l); x.res = c->layers[l].R; x.bias = b_of(c, l); x.ln = ln_args(c, l); x.pe = c->layers[l].PE;
    {
        Scope t(c, GAT_K_EDGE_FWD);
        GAT_TRY(launch_edge_forward(a, c->stream, &x));
    }
    return bn_forward_layer(c, l);
}

// Readout: P = pool(hout of the last layer) in front of the head, gH = un-pool(gP) behind it (both no-ops with readout off).  Plain
// launches on the context's stream: capturable, no host synchronisation.
static int readout_pool(gat_ctx* c) {
    if (!readout_on(c)) return 0;
    const Layer& y = c->layers.back();
    ReadoutFwdArgs a{};
    a.x = y.hout; a.x_stride = y.D; a.graph_ptr = c->readout.graph_ptr;
    a.items = c->readout.items; a.n_items = c->readout.n_items; a.split = c->readout.split; a.n_split = c->readout.n_split;
    a.pooled = c->readout.P; a.argmax = c->readout.argmax; a.part = c->readout.part; a.part_arg = c->readout.part_arg;
    a.width = y.D; a.mode = c->readout.mode;
    Scope t(c, GAT_K_HEAD_FWD);
    return launch_readout_forward(a, c->stream);
}
static int readout_unpool(gat_ctx* c) {
    if (!readout_on(c)) return 0;
    ReadoutBwdArgs a{};
    a.gpooled = c->readout.gP; a.argmax = c->readout.argmax; a.graph_ptr = c->readout.graph_ptr; a.node_graph = c->readout.node_graph;
    a.gh = c->bwd.gH; a.gh_stride = c->bwd.gh_stride; a.n_rows = c->graph.n_rows;
    a.width = c->layers.back().D; a.mode = c->readout.mode;
    Scope t(c, GAT_K_HEAD_BWD);
    return launch_readout_backward(a, c->stream);
}
// Pair head: Q = gather(hout of the last layer) in front of the head, gH = scatter(gQ) behind it (both no-ops with the feature off).
// Plain launches on the context's stream, like the readout's.
static int pair_gather(gat_ctx* c) {
    if (!pairs_on(c)) return 0;
    const Layer& y = c->layers.back();
    PairFwdArgs a{};
    a.x = y.hout; a.x_stride = y.D; a.u = c->pairs.u; a.v = c->pairs.v; a.n_pairs = c->pairs.n_pairs;
    a.q = c->pairs.Q; a.width = y.D; a.mode = c->pairs.mode;
    Scope t(c, GAT_K_HEAD_FWD);
    return launch_pair_forward(a, c->stream);
}
static int pair_scatter(gat_ctx* c) {
    if (!pairs_on(c)) return 0;
    const Layer& y = c->layers.back();
    PairBwdArgs a{};
    a.gq = c->pairs.gQ; a.x = y.hout; a.x_stride = y.D; a.inc = c->pairs.inc;
    a.items = c->pairs.items; a.n_items = c->pairs.n_items; a.split = c->pairs.split; a.n_split = c->pairs.n_split; a.part = c->pairs.part;
    a.gh = c->bwd.gH; a.gh_stride = c->bwd.gh_stride; a.width = y.D; a.mode = c->pairs.mode;
    Scope t(c, GAT_K_HEAD_BWD);
    return launch_pair_backward(a, c->stream);
}
// Hidden layer (gatv2_abi.h "hidden layer"): Z1 = act(Xin W1^T + b1) in front of the head, and behind it gA from gZ1 in place, gradb1,
// gradW1 and gXin = gA W1 into the buffer the head's gradient goes to without the feature (both no-ops with it off).  Xin: the rows the
// head reads without it.  Plain launches on the context's stream: capturable, no host synchronisation.
static const float* hidden_input(gat_ctx* c) { return pairs_on(c) ? c->pairs.Q : readout_on(c) ? c->readout.P : c->layers.back().hout; }
static int hidden_forward(gat_ctx* c) {
    if (!hidden_on(c)) return 0;
    const int32_t DL = c->layers.back().D, Dh = c->hid.width;
    Scope t(c, GAT_K_HEAD_FWD);
    GAT_TRY(launch_project_res(hidden_input(c), W1_of(c), c->hid.Z1, head_rows(c), DL, Dh, c->stream, DL));
    return launch_head_hidden_forward(c->hid.Z1, b1_of(c), head_rows(c), Dh, hidden_slope(c), c->stream);
}
static int hidden_backward(gat_ctx* c) {
    if (!hidden_on(c)) return 0;
    const int32_t DL = c->layers.back().D, Dh = c->hid.width;
    const int64_t R = head_rows(c);
    float* gxin = pairs_on(c) ? c->pairs.gQ : readout_on(c) ? c->readout.gP : c->bwd.gH;      // (a node head's gH: rows of D_last floats here)
    Scope t(c, GAT_K_HEAD_BWD);
    GAT_TRY(launch_head_hidden_backward(c->hid.gZ1, c->hid.Z1, c->hid.partial, R, Dh, hidden_slope(c), c->stream));
    GAT_TRY(launch_reduce_partials_add(c->hid.partial, head_hidden_blocks(R, Dh), Dh, gb1_of(c), c->stream));
    GAT_TRY(launch_grad_wres(c->hid.gZ1, hidden_input(c), gW1_of(c), c->hid.gw_scratch, R, DL, Dh, c->stream, DL));
    GAT_HIP(hipMemsetAsync(gxin, 0, (size_t)R * DL * sizeof(float), c->stream));          // the launcher below adds into its output
    return launch_grad_x_res(c->hid.gZ1, W1_of(c), gxin, R, DL, Dh, c->stream);
}
int gat_head_forward(gat_ctx* c, float* loss_sum, int32_t* n_correct) {
    GAT_TRY(check_layer(c, 0));
    GAT_TRY(readout_pool(c));
    GAT_TRY(pair_gather(c));
    GAT_TRY(hidden_forward(c));
    {
        Scope t(c, GAT_K_HEAD_FWD);
        GAT_TRY(launch_head_forward(head_args(c), c->stream));
    }
    c->head.y_valid = true; c->head.ran = true;
    if (loss_sum || n_correct) {
        float hl = 0.f; int32_t hc = 0;
        GAT_HIP(hipMemcpyAsync(&hl, c->head.loss_out, sizeof(float), hipMemcpyDeviceToHost, c->stream));
        GAT_HIP(hipMemcpyAsync(&hc, c->head.correct_out, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        GAT_HIP(hipStreamSynchronize(c->stream));
        if (loss_sum) *loss_sum = hl;
        if (n_correct) *n_correct = hc;
    }
    return 0;
}

int gat_head_backward(gat_ctx* c) {
    GAT_TRY(check_layer(c, 0));
    {
        Scope t(c, GAT_K_HEAD_BWD);
        GAT_TRY(launch_head_backward(head_args(c), c->stream));
    }
    GAT_TRY(hidden_backward(c));
    GAT_TRY(readout_unpool(c));
    return pair_scatter(c);
}

// Arguments of layer l's edge backward (shared by gat_layer_backward_edges and the fused last layer of gat_step), and x: what it takes
// beyond them (the forward's masks, the edge term) — filled here and nowhere else, handed as it is to the grid sizing and the launch.
// edge_order: the layer's records lie in CSR edge order (records_take_edge_order), for the backward (a.edge_order) and the pull alike
struct BwdPlan { EdgeBwdArgs a; bool store, stash, last_g, edge_order; EdgeBwdExtras x; };
static int plan_backward_edges(gat_ctx* c, int32_t l, BwdPlan* P) {
    Layer& y = c->layers[l];
    const bool store = c->bwd.msg != nullptr && edge_fast_path(y.H, y.D, c->graph.n_table);
    const bool stash = store && y.stash && c->bwd.stash != nullptr;
    EdgeBwdArgs a{};
    a.row_ptr = c->graph.row_ptr; a.col_idx = c->graph.col_idx; a.PL = y.PL; a.PR = y.PR; a.a = a_of(c, l);
    a.alpha = y.alpha; a.mstat = y.mstat; a.zstat = y.zstat;
    a.hpre = y.hpre; a.g = y.g; a.gPL = gPL_of(c, l); a.gPR = gPR_of(c, l); a.ge = y.ge; a.galpha = y.galpha;
    a.g_raw = l < c->cfg.num_layers - 1;           // hidden layers: written by launch_grad_x without the LReLU' factor
    a.gh = (l == c->cfg.num_layers - 1) ? c->bwd.gH : nullptr; a.gh_stride = c->bwd.gh_stride; a.hb_stride = 64;
    if (res_route(c)) {                             // residual / norm: G (complete) and the aggregate h_pre - (R + b), from res_backward_layer
        a.g = c->res.G; a.g_raw = 0; a.gh = nullptr; a.hpre = c->res.agg;
    }
    a.pos = store ? c->bwd.csc_pos : nullptr; a.msg = store ? c->bwd.msg : nullptr;
    a.stash = stash ? c->bwd.stash : nullptr; a.gfull = stash ? c->bwd.gfull : nullptr; a.stash_spare = (uint32_t)c->graph.n_edges;
    // last layer: the pull pass rebuilds g from gH and the decision bytes (GAT_PULL_LAST=0: gathers gfull like a hidden layer, A/B)
    // Worth it only when the g rows the pull pass would gather do not stay in the caches (Products shape 627 MB: 2.73 -> 2.29 ms;
    // Arxiv shape 43 MB: the extra loads per slot cost more than the smaller rows save, 1.31 -> 1.25 ms per step without)
    static const int pull_last = [] { const char* e = choice_env("GAT_PULL_LAST"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    // With the slot-parallel pull pass (short lists: shards) the records pay from 64 MB of g rows on: one cache line per slot instead
    // of two, and that pass is bound by lines per second (Products P = 8 shard, 78 MB: 0.84 -> 0.78 ms per step; Arxiv 43 MB: equal)
    const bool runs_form = c->bwd.src_index.csrc != nullptr && short_lists_take_runs(c->graph.n_edges, c->graph.n_table);
    const bool big_rows = (int64_t)c->graph.n_rows * y.H * y.D * 4 > ((int64_t)(runs_form ? 64 : 128) << 20);
    const bool last_g = stash && a.gh != nullptr && c->bwd.hbits != nullptr && !bf16(c) && !edge_feat_on(c) && (pull_last >= 0 ? pull_last == 1 : big_rows) &&
                        c->graph.n_rows < ((int64_t)1 << 26);             // the pull pass addresses the 64-byte node records with 32-bit offsets
    a.hbits = last_g ? c->bwd.hbits : nullptr;
    // the layout of the records: one answer for this layer's backward and pull.  The fused last layer writes its records itself, by slot
    const bool fused = l == c->cfg.num_layers - 1 && fused_last(c);
    const bool edge_order = stash && !y.ge && c->dbg == 0 && !fused &&
                            records_take_edge_order(c->bwd.src_index, y.H, y.D, !bf16(c), last_g, !last_g || c->bwd.gh_stride == 16);
    a.edge_order = edge_order ? 1 : 0;
    set_work_list(a, c->graph.work, c->graph.items, c->graph.slot_info, c->graph.part_acc);
    a.ga_partial = c->bwd.ga_partial + (int64_t)l * kGaPartialRows * c->HDmax; a.n_rows = c->graph.n_rows; a.n_table = c->graph.n_table; a.bf16 = bf16(c); a.H = y.H; a.D = y.D;
    a.slope = c->cfg.negative_slope;
    a.dbg = c->dbg;
    P->x.drop = drop_args(c, l);
    // edge features: the PE instantiations; gs of every edge goes to the shared gPE buffer (rows of this layer's HD floats)
    P->x.pe = y.PE;
    P->x.gpe = y.PE != nullptr ? c->ef.gPE : nullptr;
    a.ga_blocks = edge_backward_blocks(a, &P->x);
    P->a = a; P->store = store; P->stash = stash; P->last_g = last_g; P->edge_order = edge_order;
    return 0;
}
// The source-major pass of layer l (records -> gPL, or message rows -> gPL)
static int sum_backward_edges(gat_ctx* c, int32_t l, const BwdPlan& P) {
    Layer& y = c->layers[l];
    if (!P.stash && !P.store) return 0;
    Scope t(c, GAT_K_GPL_SUM);
    if (P.stash) {
        PullArgs p{};
        p.stash = c->bwd.stash; p.edge_order = P.edge_order;                  // the records and their layout
        p.gfull = c->bwd.gfull; p.g_bf16 = bf16(c);                           // g rows, gathered ...
        if (P.last_g) { p.gh = c->bwd.gH; p.hbits = c->bwd.hbits; }           // ... or rebuilt from the node records (last layer)
        p.gh_stride = c->bwd.gh_stride; p.hb_stride = 64;
        p.a = a_of(c, l); p.slope = c->cfg.negative_slope;
        p.gPL = gPL_of(c, l); p.H = y.H; p.D = y.D;
        return launch_gpl_pull(c->bwd.src_index, p, c->stream);
    }
    return launch_gpl_sum(c->bwd.src_index, c->bwd.msg, bf16(c), gPL_of(c, l), y.HD, c->stream);
}
// Residual layer, before its edge backward: G = dL/dh_pre and agg = h_pre - (R + b) into the context's two N-sized buffers, the
// block column sums of G into the layer's region, and their fixed-order reduction into grad_b (queued in a ReduceBatch)
static int res_backward_layer(gat_ctx* c, int32_t l) {
    Layer& y = c->layers[l];
    const bool last = l == c->cfg.num_layers - 1;
    ResBwdArgs r{};
    r.hpre = y.hpre; r.g = y.g; r.gh = (last && c->bwd.gH != nullptr) ? c->bwd.gH : nullptr; r.res = y.R; r.bias = b_of(c, l);
    r.G = c->res.G; r.agg = c->res.agg;
    r.partial = b_of(c, l) ? c->res.partial + (int64_t)l * kResPartialRows * c->HDmax : nullptr;
    r.n_rows = c->graph.n_rows; r.H = y.H; r.D = y.D; r.gh_stride = c->bwd.gh_stride; r.g_raw = last ? 0 : 1;
    r.slope = c->cfg.negative_slope;
    Scope t(c, GAT_K_MISC);
    if (norm_layer(c, l)) {                          // normalised layer: the norm's own kernel stands in (G through the normalisation)
        NormBwdArgs n{};
        n.gamma = lng_of(c, l); n.beta = lnb_of(c, l); n.eps = c->res.norm_eps;
        n.part_gamma = c->res.norm_partial + (int64_t)l * 2 * kResPartialRows * c->HDmax;
        n.part_beta = n.part_gamma + (int64_t)kResPartialRows * c->HDmax;
        r.blocks = norm_backward_blocks(c->graph.n_rows, y.HD);
        n.r = r;
        GAT_TRY(launch_norm_backward(n, c->stream));
        GAT_TRY(launch_reduce_partials_add(n.part_gamma, r.blocks, y.HD, glng_of(c, l), c->stream));
        GAT_TRY(launch_reduce_partials_add(n.part_beta, r.blocks, y.HD, glnb_of(c, l), c->stream));
    } else if (bn_layer(c, l)) {                     // batch-normalised layer: column sums of dv and dv * xhat, then G through the normalisation
        BnBwdArgs n{};
        n.u = y.hpre; n.g = r.g; n.gh = r.gh; n.res = r.res; n.bias = r.bias; n.gamma = lng_of(c, l); n.beta = lnb_of(c, l);
        n.stats = bn_stats_now(c, l);
        n.G = r.G; n.agg = r.agg; n.part_G = r.partial;
        n.part_s1 = c->res.bn_partial; n.part_s2 = c->res.bn_partial + (int64_t)kResPartialRows * c->HDmax; n.sums = c->res.bn_sums;
        n.n_rows = r.n_rows; n.gh_stride = r.gh_stride; n.H = y.H; n.D = y.D; n.training = c->drop.training ? 1 : 0; n.slope = r.slope;
        n.blocks = r.blocks = batch_norm_blocks(c->graph.n_rows, y.HD);
        GAT_TRY(launch_batch_norm_backward(n, glng_of(c, l), glnb_of(c, l), c->stream));
    } else {
        r.blocks = res_backward_blocks(c->graph.n_rows, y.HD);
        GAT_TRY(launch_res_backward(r, c->stream));
    }
    if (r.partial != nullptr) return launch_reduce_partials_add(r.partial, r.blocks, y.HD, gb_of(c, l), c->stream);
    return 0;
}
int gat_layer_backward_edges(gat_ctx* c, int32_t l) {
    GAT_TRY(check_layer(c, l));
    GAT_TRY(check_edge_features(c));
    Layer& y = c->layers[l];
    BwdPlan P;
    GAT_TRY(plan_backward_edges(c, l, &P));
    if (res_route(c)) GAT_TRY(res_backward_layer(c, l));
    if (!P.store) {
        Scope t(c, GAT_K_MISC);
        GAT_HIP(hipMemsetAsync(gPL_of(c, l), 0, (size_t)c->graph.n_table * y.HD * sizeof(float), c->stream));
    }
    {
        Scope t(c, GAT_K_EDGE_BWD);
        GAT_TRY(launch_edge_backward(P.a, c->stream, &P.x));
    }
    GAT_TRY(sum_backward_edges(c, l, P));
    Scope t(c, GAT_K_MISC);
    return launch_reduce_partials_add(P.a.ga_partial, P.a.ga_blocks, y.HD, ga_of(c, l), c->stream);
}

// grad_w of layer l on stream st (the context's, or the side stream of the overlapped backward)
static int backward_grad_w(gat_ctx* c, int32_t l, hipStream_t st) {
    Layer& y = c->layers[l];
    const float* gPL_rows = gPL_of(c, l) + c->graph.table_row0 * y.HD;
    Scope t(c, GAT_K_GRAD_W, st);
    // residual: gradWres += G^T x' over the shard's own rows (G: this layer's, still in place — the next res_backward_layer runs later
    // on the same stream; the side stream of GAT_OVERLAP is not used with a residual context)
    if (y.R != nullptr)
        GAT_TRY(launch_grad_wres(c->res.G, Xin_of(c, l), gWres_of(c, l), c->res.gw_scratch + c->res.gw_off[(size_t)l], c->graph.n_rows, y.F, y.HD, st, ldX_of(c, l)));
    // edge features: gradWe += gPE^T EA over the E edges (gPE: this layer's, still in place — the next layer's edge backward runs later on
    // the same stream; the side stream of GAT_OVERLAP is not used with edge features)
    if (y.PE != nullptr)
        GAT_TRY(launch_grad_wres(c->ef.gPE, c->ef.EA, gWe_of(c, l), c->ef.gw_scratch + c->ef.gw_off[(size_t)l], c->graph.n_edges, c->ef.dim, y.HD, st, c->ef.ld));
    if (l == 0 && c->in.Xtab) {  // partial gPL over the whole table x replicated input; the gradient all-reduce sums shards
        GAT_TRY(launch_grad_w(gPL_of(c, l), nullptr, Xtab_of(c), gW_of(c, l), c->bwd.gw_scratch, c->graph.n_table, y.F, y.HD, kPartLeft, st, c->in.ld0));
        return launch_grad_w(nullptr, gPR_of(c, l), Xin_of(c, 0), gW_of(c, l), c->bwd.gw_scratch, c->graph.n_rows, y.F, y.HD, kPartRight, st, c->in.ld0);
    }
    return launch_grad_w(gPL_rows, gPR_of(c, l), Xin_of(c, l), gW_of(c, l), c->bwd.gw_scratch + c->bwd.gw_off[(size_t)l], c->graph.n_rows, y.F, y.HD, kPartBoth, st, ldX_of(c, l));
}
static int backward_grad_x(gat_ctx* c, int32_t l) {
    if (l == 0) return 0;                                             // E:1528
    Layer& y = c->layers[l];
    const float* gPL_rows = gPL_of(c, l) + c->graph.table_row0 * y.HD;
    Scope t(c, GAT_K_GRAD_X);
    // plain dL/d(input) of this layer: the LReLU'(h_pre) factor of E:888-892 is applied by the edge backward
    // of layer l-1, which reads h_pre anyway (the epilogue's extra read of h_pre cost 0.45 of 1.03 ms)
    GAT_TRY(launch_grad_x(gPL_rows, gPR_of(c, l), W_of(c, l), nullptr, c->layers[l - 1].g, c->graph.n_rows, y.F, y.HD,
                          c->cfg.negative_slope, c->stream));
    // residual: + G Wres, before the feature-dropout factor and before the LReLU' factor of the layer below
    if (y.R != nullptr) GAT_TRY(launch_grad_x_res(c->res.G, Wres_of(c, l), c->layers[l - 1].g, c->graph.n_rows, y.F, y.HD, c->stream));
    // feature dropout: dL/dx_l = dL/dx'_l (.) kappa s_f, before the LReLU' factor of layer l-1 (applied by its edge backward)
    if (feat_drop_on(c)) return launch_feat_drop_bwd(c->layers[l - 1].g, c->graph.n_rows, y.F, drop_args(c, l, kDropFeat), c->stream);
    return 0;
}
int gat_layer_backward_dense(gat_ctx* c, int32_t l) {
    GAT_TRY(check_layer(c, l));
    GAT_TRY(check_edge_features(c));
    GAT_TRY(backward_grad_w(c, l, c->stream));
    return backward_grad_x(c, l);
}

// ---- whole step (single shard, or a shard with a transport attached) ------------------------------------------
static int64_t table_slice(gat_ctx* c, const Layer& y) { return (c->graph.n_table / c->xch.comm->world) * y.HD; }      // fp32 rows
static int64_t pl_slice(gat_ctx* c, const Layer& y) { return table_slice(c, y) * st_bytes(c) / 4; }        // PL rows, as floats
static bool needs_exchange(gat_ctx* c, int l) { return c->graph.n_table != c->graph.n_rows && !(l == 0 && c->in.Xtab); }
static int check_step(gat_ctx* c, const char* who) {
    GAT_TRY(check_layer(c, 0));
    GAT_TRY(check_edge_features(c));
    if (c->graph.n_table != c->graph.n_rows && !c->xch.comm)
        return fail(GAT_E_STATE, std::string(who) + ": sharded context — attach a transport (gat_comm_init_*) or drive "
                                                   "the phase API with the exchange steps");
    return 0;
}
// Chunk-pipelined forward exchange of one layer (gat_comm_option GAT_COMM_PIPELINE = K > 1): the shard's rows are
// projected in K row chunks on the compute stream; as soon as chunk k exists, its part of every rank's table slice is
// exchanged on a second stream, while chunk k+1 is being projected.  The edge pass waits for the last part.  Chunk
// boundaries are the same slice coordinates on every rank (multiples of 128 rows of max_rows), so the parts have fixed
// counts.  Every PL / PR row is produced by the same sequence of matrix instructions as in one launch: results are bitwise those of the
// unchunked exchange (tests/test_shard.py).  What can hide behind the exchange this way is the projection itself; the
// edge pass needs the whole table.
static int forward_exchange_pipelined(gat_ctx* c, int l) {
    Layer& y = c->layers[l];
    const int K = c->xch.chunks;
    const int64_t max_rows = c->graph.n_table / c->xch.comm->world;
    const int64_t rpc = ((max_rows + K - 1) / K + 127) / 128 * 128;       // rows per chunk, a multiple of the GEMM's row tile
    if (!c->xch.stream) GAT_HIP(hipStreamCreateWithFlags(&c->xch.stream, hipStreamNonBlocking));
    while ((int)c->xch.events.size() < K + 1) {
        hipEvent_t e;
        GAT_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->xch.events.push_back(e);
    }
    const int64_t rowf = y.HD * st_bytes(c) / 4;                           // floats per PL row (bf16 rows: half)
    char* own_rows = reinterpret_cast<char*>(y.PL) + c->graph.table_row0 * y.HD * st_bytes(c);
    Scope t(c, GAT_K_EXCHANGE);                                            // timed as a whole: projection chunks + their exchanges
    GAT_TRY(project_side_terms(c, l));
    for (int k = 0; k < K; ++k) {
        const int64_t r0 = (int64_t)k * rpc, r1s = std::min<int64_t>(r0 + rpc, max_rows), r1 = std::min<int64_t>(r1s, c->graph.n_rows);
        if (r0 >= max_rows) break;
        if (r1 > r0)
            GAT_TRY(launch_project(Xin_of(c, l) + r0 * ldX_of(c, l), W_of(c, l), reinterpret_cast<float*>(own_rows + r0 * y.HD * st_bytes(c)),
                                   y.PR + r0 * y.HD, r1 - r0, y.F, y.HD, kPartBoth, bf16(c), nullptr, 0, c->stream, ldX_of(c, l)));
        GAT_HIP(hipEventRecord(c->xch.events[k], c->stream));
        GAT_HIP(hipStreamWaitEvent(c->xch.stream, c->xch.events[k], 0));
        GAT_TRY(c->xch.comm->all_gather_part(y.PL, pl_slice(c, y), r0 * rowf, (r1s - r0) * rowf, c->xch.stream));
    }
    GAT_HIP(hipEventRecord(c->xch.events[K], c->xch.stream));
    GAT_HIP(hipStreamWaitEvent(c->stream, c->xch.events[K], 0));
    return 0;
}
static int forward_phases(gat_ctx* c, int l_end = -1, bool last_edges = true) {
    // layers [0, l_end) completely; last_edges = false: the last of them stops after its projection (+ exchange)
    if (l_end < 0) l_end = c->cfg.num_layers;
    for (int l = 0; l < l_end; ++l) {
        const bool edges = last_edges || l < l_end - 1;
        // the chunked projection runs the streaming kernel; a layer whose one-launch projection takes the split-K kernel
        // (few rows, F > 128: another summation order) keeps the plain exchange, so that K chunks stay bitwise K = 1
        if (c->xch.comm && needs_exchange(c, l) && c->xch.chunks > 1 && !c->xch.halo_on &&
            project_scratch_floats(c->graph.n_rows, c->layers[l].F, c->layers[l].HD, kPartBoth) == 0) {
            GAT_TRY(check_layer(c, l));
            GAT_TRY(check_edge_features(c));
            GAT_TRY(forward_exchange_pipelined(c, l));
            if (edges) GAT_TRY(gat_layer_forward_edges(c, l));
            continue;
        }
        GAT_TRY(gat_layer_project(c, l));
        if (c->xch.comm && needs_exchange(c, l)) {
            Scope t(c, GAT_K_EXCHANGE);
            if (c->xch.halo_on) GAT_TRY(halo_forward(c->xch.comm.get(), c->xch.halo, c->layers[l].PL, c->layers[l].HD * st_bytes(c) / 4, c->stream));
            else GAT_TRY(c->xch.comm->all_gather(c->layers[l].PL, pl_slice(c, c->layers[l]), c->stream));
        }
        if (edges) GAT_TRY(gat_layer_forward_edges(c, l));
    }
    return 0;
}
static int head_step(gat_ctx* c, bool with_gh = true) {
    HeadArgs a = head_args(c);
    if (!with_gh) a.gh_out = nullptr;               // loss, #correct and grad_Wo only (the fused last layer formed gH itself)
    GAT_TRY(readout_pool(c));
    GAT_TRY(pair_gather(c));
    GAT_TRY(hidden_forward(c));
    {
        Scope t(c, GAT_K_HEAD_BWD);
        c->head.y_valid = false; c->head.ran = true;
        GAT_TRY(launch_head_step(a, c->stream));
    }
    GAT_TRY(hidden_backward(c));
    GAT_TRY(readout_unpool(c));
    return pair_scatter(c);
}
static int last_layer_fused(gat_ctx* c) {
    const int l = c->cfg.num_layers - 1;
    Layer& y = c->layers[l];
    BwdPlan P;
    GAT_TRY(plan_backward_edges(c, l, &P));
    const EdgeFwdArgs f = plan_forward_edges(c, l);
    const int32_t n_seg = c->graph.work.n_slots;          // the segments of split rows come first in the work list
    float* ga_a = P.a.ga_partial;                   // this layer's region (kGaPartialRows rows): the segments' launch, then the fused one,
    int blocks_a = 0;                               // back to back — ONE reduction job (two jobs into one output would race)
    if (n_seg > 0) {                                // split rows: forward segments + fix-up, their gH, backward segments + fix-up
        EdgeFwdArgs fs = f;
        fs.n_items = n_seg;
        {
            Scope t(c, GAT_K_EDGE_FWD);
            GAT_TRY(launch_edge_forward(fs, c->stream));
        }
        {
            Scope t(c, GAT_K_HEAD_BWD);
            GAT_TRY(launch_head_rows(c->graph.slot_info, c->graph.work.n_slots, c->graph.work.n_split, Wo_of(c), y.hout, c->sup.labels_eff ? c->sup.labels_eff : c->sup.labels,
                                     c->bwd.gH, c->bwd.gh_stride, c->cfg.num_classes, y.D, c->stream));
        }
        EdgeBwdArgs bs = P.a;
        bs.n_items = n_seg;
        bs.ga_partial = ga_a;
        // without P.x on purpose, grid and launch alike: fused_last() excludes dropout and edge features, so the plan's extras are inert here
        bs.ga_blocks = blocks_a = std::min(kGaPartialRows / 2, edge_backward_blocks(bs));
        Scope t(c, GAT_K_EDGE_BWD);
        GAT_TRY(launch_edge_backward(bs, c->stream));
    }
    EdgeLastArgs a{};
    a.f = f; a.f.items = c->graph.items + n_seg; a.f.n_items = c->graph.work.n_items - n_seg;
    float* ga_b = ga_a + (int64_t)blocks_a * y.HD;
    a.b = P.a; a.b.ga_partial = ga_b; a.b.ga_blocks = a.f.n_items > 0 ? std::min(edge_last_fused_blocks(a.f.n_items), kGaPartialRows - blocks_a) : 0;    // what is left of the layer's region
    a.Wo = Wo_of(c); a.labels = c->sup.labels_eff ? c->sup.labels_eff : c->sup.labels; a.gh_out = c->bwd.gH; a.C = c->cfg.num_classes;
    {
        Scope t(c, GAT_K_EDGE_FUSED);
        GAT_TRY(launch_edge_last_fused(a, c->stream));
    }
    GAT_TRY(head_step(c, false));                   // loss, #correct, grad_Wo from the stored H (all rows)
    GAT_TRY(sum_backward_edges(c, l, P));
    Scope t(c, GAT_K_MISC);
    return launch_reduce_partials_add(ga_a, blocks_a + a.b.ga_blocks, y.HD, ga_of(c, l), c->stream);
}
// grad_w of a layer feeds nothing but the parameter gradients, yet on one stream it sits between the layer's source-major pass
// and grad_x -> the next layer's edge passes (E:1517 vs 1533).  With GAT_OVERLAP=1 it runs on a side stream: forked after the
// layer's gPL is complete, joined before that layer's buffer pair is written again (two layers later) or at the end of the
// backward.  MEASURED, NOT THE DEFAULT (DESIGN §4 "Round 4", profiles/r04/experiments/overlap_*): Products shape, same box,
// A/B/A/B 20.98 / 21.18 / 21.21 / 21.42 ms per step and 21.15 / 21.29 / 21.17 / 22.36 with a lowest-priority side stream — the
// 0.31 ms of layer 1's grad_w leave the critical path, and the backward edge pass it runs beside (a persistent grid sized to
// the chip, items dealt statically: any CU that shares its wave slots and fabric requests becomes the tail) slows by
// 0.33-0.36 ms, grad_x by 0.06, grad_w itself from 0.79 to 1.29; under hipGraph replay the fork / join costs more than it hides
// (Arxiv shape 1.12 -> 1.16 ms, Pubmed 0.245 -> 0.263, Cora 0.188 -> 0.202).  The edge passes are bound by fabric requests
// per second, which the dense kernels (4-6 TB/s of row streaming) consume too: there is no idle unit to fill.  Needs the second gPL / gPR pair (odd layers), hence not with a caller-bound gPL table
// or a replicated layer-0 input (its two grad_w launches share one slab region).  Same kernels, same operands: bitwise the
// serial order's gradients.  Captured by gat_step_graph as a fork / join in the graph.
static int overlap_prepare(gat_ctx* c) {
    static const int env = [] { const char* e = choice_env("GAT_OVERLAP"); return e ? (e[0] == '0' ? 0 : 1) : -1; }();
    const int L = c->cfg.num_layers;
    const bool want = env == 1;
    if (!want || L < 2 || c->bwd.gPL_bound || c->in.Xtab || res_route(c) || edge_feat_on(c)) return 0;      // (residual: one G buffer, read by grad_w; edge features: one gPE)
    if (!c->ov.gPL) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        (void)hipStreamIsCapturing(c->stream, &cs);
        if (cs != hipStreamCaptureStatusNone) return 0;               // first use inside a capture: allocate on the next eager step
        GAT_TRY(dalloc(c, &c->ov.gPL, c->graph.n_table * c->HDmax));
        GAT_TRY(dalloc(c, &c->ov.gPR, c->graph.n_rows * c->HDmax));
        {   // lowest priority: grad_w should fill what the edge passes leave free (their tails), not take their wave slots
            int least = 0, greatest = 0;
            (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
            static const bool prio = [] { const char* e = choice_env("GAT_OVERLAP_PRIO"); return !(e && e[0] == '0'); }();
            if (prio) GAT_HIP(hipStreamCreateWithPriority(&c->ov.stream, hipStreamNonBlocking, least));
            else GAT_HIP(hipStreamCreateWithFlags(&c->ov.stream, hipStreamNonBlocking));
        }
        for (int l = 0; l < L; ++l) {
            hipEvent_t a, b;
            GAT_HIP(hipEventCreateWithFlags(&a, hipEventDisableTiming));
            GAT_HIP(hipEventCreateWithFlags(&b, hipEventDisableTiming));
            c->ov.fork.push_back(a); c->ov.join.push_back(b);
        }
    }
    return 1;
}
struct OverlapScope {       // ov_active only while backward_phases runs (the phase API keeps the single pair)
    gat_ctx* c;
    explicit OverlapScope(gat_ctx* c_, bool on) : c(c_) { c->ov.active = on; }
    ~OverlapScope() { c->ov.active = false; }
};
static int backward_phases(gat_ctx* c, bool head_done = false, bool last_edges_done = false) {
    // last_edges_done: the last layer's edge passes (incl. its source-major pass) have run already (fused last layer)
    const int L = c->cfg.num_layers;
    const int ov = last_edges_done ? 0 : overlap_prepare(c);          // (the fused last layer wrote the first pair before this call)
    if (ov < 0) return ov;
    OverlapScope scope(c, ov == 1);
    std::vector<char> forked((size_t)L, 0);
    if (!head_done) GAT_TRY(gat_head_backward(c));
    for (int l = L - 1; l >= 0; --l) {
        if (ov && l + 2 < L && forked[(size_t)l + 2]) {               // this layer rewrites the pair layer l+2's grad_w reads
            GAT_HIP(hipStreamWaitEvent(c->stream, c->ov.join[(size_t)l + 2], 0));
            forked[(size_t)l + 2] = 0;
        }
        if (!(last_edges_done && l == L - 1)) GAT_TRY(gat_layer_backward_edges(c, l));
        if (c->xch.comm && needs_exchange(c, l)) {
            Scope t(c, GAT_K_EXCHANGE);
            if (c->xch.halo_on) GAT_TRY(halo_backward(c->xch.comm.get(), c->xch.halo, gPL_of(c, l), c->layers[l].HD, c->stream));
            else if (c->xch.gpl_bf16) GAT_TRY(c->xch.comm->reduce_scatter_bf16(gPL_of(c, l), table_slice(c, c->layers[l]), c->stream));
            else GAT_TRY(c->xch.comm->reduce_scatter(gPL_of(c, l), table_slice(c, c->layers[l]), c->stream));
        }
        if (ov && l > 0) {                                            // layer 0's grad_w is the last kernel: nothing to hide behind
            GAT_HIP(hipEventRecord(c->ov.fork[(size_t)l], c->stream));
            GAT_HIP(hipStreamWaitEvent(c->ov.stream, c->ov.fork[(size_t)l], 0));
            GAT_TRY(backward_grad_w(c, l, c->ov.stream));
            GAT_HIP(hipEventRecord(c->ov.join[(size_t)l], c->ov.stream));
            forked[(size_t)l] = 1;
            GAT_TRY(backward_grad_x(c, l));
        } else {
            GAT_TRY(backward_grad_w(c, l, c->stream));
            GAT_TRY(backward_grad_x(c, l));
        }
    }
    for (int l = 0; l < L; ++l)
        if (forked[(size_t)l]) GAT_HIP(hipStreamWaitEvent(c->stream, c->ov.join[(size_t)l], 0));        // join: the slab reductions follow
    return 0;
}
// tail of the packed gradient buffer -> host values (after an all-reduce the sums over shards)
static int read_result_tail(gat_ctx* c, float* loss_sum, int32_t* n_correct) {
    float t[3] = {0.f, 0.f, 0.f};
    GAT_HIP(hipMemcpyAsync(t, c->packed.grads + n_params(c), sizeof(t), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    if (loss_sum) *loss_sum = t[0];
    if (n_correct) *n_correct = (int32_t)(t[1] + 4096.0f * t[2] + 0.5f);
    return 0;
}
int gat_forward(gat_ctx* c, float* loss_sum, int32_t* n_correct) {
    GAT_TRY(check_step(c, "gat_forward"));
    GAT_TRY(forward_phases(c));
    if (!c->xch.comm) return gat_head_forward(c, loss_sum, n_correct);
    GAT_TRY(gat_head_forward(c, nullptr, nullptr));
    if (!loss_sum && !n_correct) return 0;
    float* tail = c->packed.grads + n_params(c);
    GAT_TRY(launch_pack_result(c->head.loss_out, c->head.correct_out, tail, c->stream));
    {
        Scope t(c, GAT_K_EXCHANGE);
        GAT_TRY(c->xch.comm->all_reduce(tail, 3, c->stream));
    }
    return read_result_tail(c, loss_sum, n_correct);
}
// The gradient buffer ACCUMULATES until gat_zero_grad (E:1262-1266, 1631-1633).  With a transport the step's
// contribution must be summed over shards exactly once: the accumulated (already reduced) values are set
// aside, the step runs into a zeroed buffer, that is all-reduced, and the old values are added back —
// without this, a second step before gat_zero_grad would reduce the earlier sums again (x world).
static int reduce_begin(gat_ctx* c) {
    if (!c->xch.comm) return 0;
    const int64_t np = n_params(c);
    if (!c->xch.grads_prev) GAT_TRY(dalloc(c, &c->xch.grads_prev, np));
    Scope t(c, GAT_K_MISC);
    GAT_HIP(hipMemcpyAsync(c->xch.grads_prev, c->packed.grads, (size_t)np * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    GAT_HIP(hipMemsetAsync(c->packed.grads, 0, (size_t)np * sizeof(float), c->stream));
    return 0;
}
static int reduce_end(gat_ctx* c, int64_t count) {          // count: n_params, or n_params + 3 with the result tail
    if (!c->xch.comm) return 0;
    {
        Scope t(c, GAT_K_EXCHANGE);
        GAT_TRY(c->xch.comm->all_reduce(c->packed.grads, count, c->stream));
    }
    Scope t(c, GAT_K_MISC);
    return launch_reduce_partials_add(c->xch.grads_prev, 1, n_params(c), c->packed.grads, c->stream);
}
// Slab reductions of the backward (grad_Wo, grad_a and grad_W of every layer) and the result pack as one launch at the
// end (ReduceBatch).  Not with replicated layer-0 input: its two grad_w launches share one slab region.  GAT_REDUCE_BATCH=0: A/B.
struct BatchScope {
    bool on;
    explicit BatchScope(gat_ctx* c) {
        static const bool env_on = [] { const char* e = choice_env("GAT_REDUCE_BATCH"); return !(e && e[0] == '0'); }();
        on = env_on && !c->in.Xtab;
        if (on) reduce_batch_begin();
    }
    // host_tail: pinned copy of the packed result written by the same kernel (*host_done = it was: no copy node needed)
    int finish(gat_ctx* c, bool pack, float* host_tail = nullptr, bool* host_done = nullptr) {
        float* tail = c->packed.grads + n_params(c);
        if (host_done) *host_done = on && pack && host_tail != nullptr;
        if (!on) return pack ? launch_pack_result(c->head.loss_out, c->head.correct_out, tail, c->stream) : 0;
        on = false;
        if (pack) reduce_batch_pack(c->head.loss_out, c->head.correct_out, tail, host_tail);
        Scope t(c, GAT_K_MISC);
        return reduce_batch_flush(c->stream);
    }
    ~BatchScope() { if (on) reduce_batch_abort(); }       // error return in between: nothing stays queued
};
int gat_backward(gat_ctx* c) {
    GAT_TRY(check_step(c, "gat_backward"));
    GAT_TRY(reduce_begin(c));
    {
        BatchScope batch(c);
        GAT_TRY(backward_phases(c));
        GAT_TRY(batch.finish(c, false));
    }
    return reduce_end(c, n_params(c));
}
static int step_body(gat_ctx* c, float* host_tail = nullptr, bool* host_done = nullptr) {
    if (host_done) *host_done = false;
    if (fused_last(c)) {
        GAT_TRY(forward_phases(c, c->cfg.num_layers, false));      // every layer; the last one stops after its projection
        BatchScope batch(c);
        GAT_TRY(last_layer_fused(c));
        GAT_TRY(backward_phases(c, true, true));
        return batch.finish(c, true, host_tail, host_done);
    }
    GAT_TRY(forward_phases(c));
    BatchScope batch(c);
    if (fused_head(c)) {
        GAT_TRY(head_step(c));
        GAT_TRY(backward_phases(c, true));
    } else {
        GAT_TRY(gat_head_forward(c, nullptr, nullptr));
        GAT_TRY(backward_phases(c));
    }
    return batch.finish(c, true, host_tail, host_done);
}
// What the replay slot holds: the body of gat_step (entry 0), or of gat_train_step (entry 1) — the packed gradients zeroed in front of
// it, the optimizer's two launches behind it (the result tail sits behind the gradients and is packed by the body: the update does not
// touch it).
static int entry_body(gat_ctx* c, int entry, float* host_tail = nullptr, bool* host_done = nullptr) {
    if (entry == 0) return step_body(c, host_tail, host_done);
    {
        Scope t(c, GAT_K_MISC);
        GAT_HIP(hipMemsetAsync(c->packed.grads, 0, (size_t)n_params(c) * sizeof(float), c->stream));
    }
    GAT_TRY(step_body(c, host_tail, host_done));
    return optimizer_launch(c);
}
static int step_graph(gat_ctx* c, int entry, float* loss_sum, int32_t* n_correct) {
    const int64_t np = n_params(c);
    if (c->replay.entry != entry) {                               // the slot holds (or was warmed by) the other entry point: start over
        graph_drop(c);
        c->replay.entry = entry;
    }
    if (c->replay.state == 1 && c->replay.warm == 0) {            // eager warm-up
        GAT_TRY(entry_body(c, entry));
        c->replay.warm = 1;
        return (loss_sum || n_correct) ? read_result_tail(c, loss_sum, n_correct) : 0;
    }
    if (c->replay.state == 1) {                                  // capture
        if (!c->replay.pinned_tail) GAT_HIP(hipHostMalloc((void**)&c->replay.pinned_tail, 4 * sizeof(float)));
        GAT_HIP(hipStreamSynchronize(c->stream));
        GAT_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        bool host_done = false;                             // the batch kernel's pack block wrote the pinned copy itself
        int rc = entry_body(c, entry, c->replay.pinned_tail, &host_done);
        if (rc == 0 && !host_done && hipMemcpyAsync(c->replay.pinned_tail, c->packed.grads + np, 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            rc = fail(GAT_E_STATE, "gat_step_graph: capture of the result copy failed");
        hipGraph_t g = nullptr;
        const hipError_t e = hipStreamEndCapture(c->stream, &g);
        if (rc != 0 || e != hipSuccess || !g) {
            if (g) (void)hipGraphDestroy(g);
            (void)hipGetLastError();
            c->replay.state = 0;                                     // fall back to eager for good
            return rc != 0 ? rc : fail((int)e, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
        }
        c->replay.graph = g;
        GAT_HIP(hipGraphInstantiate(&c->replay.exec, c->replay.graph, nullptr, nullptr, 0));
        c->replay.state = 2;
        c->replay.y_after = c->head.y_valid;
    }
    GAT_HIP(hipGraphLaunch(c->replay.exec, c->stream));
    c->head.y_valid = c->replay.y_after;              // y of an earlier forward (gat_eval_mask, gat_eval_rank, gat_tap between replays) is stale now
    if (!loss_sum && !n_correct) return 0;
    GAT_HIP(hipStreamSynchronize(c->stream));
    if (loss_sum) *loss_sum = c->replay.pinned_tail[0];
    if (n_correct) *n_correct = (int32_t)(c->replay.pinned_tail[1] + 4096.0f * c->replay.pinned_tail[2] + 0.5f);
    return 0;
}
int gat_step_graph(gat_ctx* c, int32_t enable) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (enable && c->xch.comm) return fail(GAT_E_UNSUPPORTED, "gat_step_graph: not with a transport attached (the exchanges are issued eagerly)");
    if (enable && c->cfg.collect_timing) return fail(GAT_E_UNSUPPORTED, "gat_step_graph: not with collect_timing (event pairs cannot be read back from a replay)");
    graph_drop(c);
    c->replay.state = enable ? 1 : 0;
    return 0;
}
int gat_step_graph_state(gat_ctx* c, int32_t* state) {
    if (!c || !state) return fail(GAT_E_INVALID, "gat_step_graph_state: null argument");
    *state = c->replay.state;
    return 0;
}

int gat_step(gat_ctx* c, float* loss_sum, int32_t* n_correct) {
    GAT_TRY(check_step(c, "gat_step"));
    if (c->replay.state != 0) return step_graph(c, 0, loss_sum, n_correct);
    GAT_TRY(reduce_begin(c));
    GAT_TRY(step_body(c));                              // ends with the packed {loss, correct} behind the gradients
    GAT_TRY(reduce_end(c, n_params(c) + 3));
    if (!loss_sum && !n_correct) return 0;
    return read_result_tail(c, loss_sum, n_correct);
}
// gatv2_abi.h "optimizer": zero the gradients, the step, the update — eagerly here (with a transport: the update reads the gradients the
// all-reduce has summed), or as the replay slot's entry 1
int gat_train_step(gat_ctx* c, float* loss_sum, int32_t* n_correct) {
    GAT_TRY(check_step(c, "gat_train_step"));
    if (!c->opt.have) return fail(GAT_E_STATE, "gat_train_step: call gat_set_optimizer first");
    if (c->replay.state != 0) return step_graph(c, 1, loss_sum, n_correct);
    GAT_TRY(gat_zero_grad(c));
    GAT_TRY(reduce_begin(c));
    GAT_TRY(step_body(c));
    GAT_TRY(reduce_end(c, n_params(c) + 3));
    GAT_TRY(optimizer_launch(c));
    if (!loss_sum && !n_correct) return 0;
    return read_result_tail(c, loss_sum, n_correct);
}

// ---- transports ----------------------------------------------------------------------------------------------
static int check_comm_target(gat_ctx* c, int32_t world, int32_t rank) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (c->xch.comm) return fail(GAT_E_STATE, "a transport is already attached");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_comm_init: set the graph first");
    if (readout_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_comm_init: not on a readout context (a graph may straddle shards)");
    if (pairs_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_comm_init: not on a context with a pair head (an endpoint may live on another shard)");
    if (hidden_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_comm_init: not on a context with a hidden head layer (gat_set_head_hidden has no sharded form)");
    if (bn_on(c)) return fail(GAT_E_UNSUPPORTED, "gat_comm_init: not on a context with batch normalisation (the column statistics of a shard would need an exchange)");
    if (world < 1 || rank < 0 || rank >= world) return fail(GAT_E_INVALID, "gat_comm_init: bad world / rank");
    if (c->graph.n_table % world != 0 || c->graph.table_row0 != (int64_t)rank * (c->graph.n_table / world) || c->graph.n_rows > c->graph.n_table / world)
        return fail(GAT_E_INVALID, "gat_comm_init: the source table must be [world][max_rows] with this shard's rows at rank*max_rows");
    return 0;
}
int gat_comm_unique_id(void* id_out) { return comm_unique_id(id_out); }
int gat_comm_init_rccl(gat_ctx* c, int32_t world, int32_t rank, const void* id) {
    GAT_TRY(check_comm_target(c, world, rank));
    Comm* cm = nullptr;
    GAT_TRY(comm_create_rccl(world, rank, id, &cm));
    c->xch.comm.reset(cm);
    return 0;
}
int gat_comm_init_host(gat_ctx* c, int32_t world, int32_t rank, const char* shm_name, int64_t bytes_per_rank) {
    GAT_TRY(check_comm_target(c, world, rank));
    Comm* cm = nullptr;
    GAT_TRY(comm_create_host(world, rank, shm_name, bytes_per_rank, &cm));
    c->xch.comm.reset(cm);
    return 0;
}
int gat_comm_option(gat_ctx* c, int32_t option, int32_t value) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (option == GAT_COMM_GPL_BF16) {
        if (value != 0 && c->xch.halo_on) return fail(GAT_E_UNSUPPORTED, "gat_comm_option: GAT_COMM_GPL_BF16 and GAT_COMM_HALO exclude each other (the halo backward travels as fp32)");
        c->xch.gpl_bf16 = value != 0;
        return 0;
    }
    if (option == GAT_COMM_HALO) {                       // collective: every rank of the transport makes the same call
        if (value < 0 || value > 2) return fail(GAT_E_INVALID, "gat_comm_option: GAT_COMM_HALO takes 0 (off), 1 (on) or 2 (on where it pays)");
        c->xch.halo_on = false;
        if (value == 0) { halo_free(&c->xch.halo); return 0; }
        if (!c->xch.comm) return fail(GAT_E_STATE, "gat_comm_option: GAT_COMM_HALO needs a transport (gat_comm_init_*) first");
        if (c->xch.gpl_bf16) return fail(GAT_E_UNSUPPORTED, "gat_comm_option: GAT_COMM_GPL_BF16 and GAT_COMM_HALO exclude each other");
        if (c->HDmax % 2 != 0 && bf16(c)) return fail(GAT_E_UNSUPPORTED, "gat_comm_option: GAT_COMM_HALO with bf16 rows needs an even H*D");
        GAT_TRY(halo_build(c->xch.comm.get(), c->graph.col_idx, c->graph.n_edges, c->graph.n_table, c->HDmax, &c->xch.halo, c->stream));
        // value 2: only where fewer than half of the rows would travel — a halo costs a pack and an unpack pass over the rows it moves
        // on each side (4 row transfers through HBM at ~5 TB/s against one over ~1 TB/s of xGMI links: break-even near 0.5)
        c->xch.halo_on = value == 1 || c->xch.halo.referenced_fraction < 0.5;
        return 0;
    }
    if (option == GAT_COMM_PIPELINE) {
        if (value < 1 || value > 64) return fail(GAT_E_INVALID, "gat_comm_option: GAT_COMM_PIPELINE takes 1..64 chunks");
        c->xch.chunks = value;
        return 0;
    }
    return fail(GAT_E_INVALID, "gat_comm_option: unknown option");
}
int gat_comm_halo_info(gat_ctx* c, int32_t* active, int64_t* rows_received, int64_t* rows_sent, double* referenced_fraction) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (active) *active = c->xch.halo_on ? 1 : 0;
    if (rows_received) *rows_received = c->xch.halo.n_need;
    if (rows_sent) *rows_sent = c->xch.halo.n_send;
    if (referenced_fraction) *referenced_fraction = c->xch.halo.world > 0 ? c->xch.halo.referenced_fraction : 1.0;
    return 0;
}

// ---- exchange tables ----------------------------------------------------------------------------------------------
int gat_table(gat_ctx* c, int which, int32_t l, void** d_ptr, int64_t* n_rows, int64_t* row_floats) {
    GAT_TRY(check_layer(c, l));
    if (!d_ptr) return fail(GAT_E_INVALID, "null argument");
    if (which == GAT_TABLE_PL) *d_ptr = c->layers[l].PL;
    else if (which == GAT_TABLE_GPL) *d_ptr = c->bwd.gPL;                 // (the phase API always uses the first pair)
    else return fail(GAT_E_INVALID, "unknown table");
    if (n_rows) *n_rows = c->graph.n_table;
    if (row_floats) *row_floats = which == GAT_TABLE_PL ? c->layers[l].HD * st_bytes(c) / 4 : c->layers[l].HD;
    return 0;
}
int gat_bind_table(gat_ctx* c, int which, int32_t l, void* d_ptr, int64_t bytes) {
    if (!c || !d_ptr) return fail(GAT_E_INVALID, "null argument");
    if (l < 0 || l >= c->cfg.num_layers) return fail(GAT_E_INVALID, "layer index out of range");
    if (!c->graph.have) return fail(GAT_E_STATE, "gat_bind_table: set the graph first");
    graph_drop(c);                                       // captured addresses would be stale
    if (which == GAT_TABLE_PL) {
        Layer& y = c->layers[l];
        if (bytes < (int64_t)c->graph.n_table * y.HD * st_bytes(c)) return fail(GAT_E_INVALID, "bound PL table too small");
        if (!y.PL_bound) dfree(c, y.PL);
        y.PL = (float*)d_ptr; y.PL_bound = true;
        return 0;
    }
    if (which == GAT_TABLE_GPL) {
        if (bytes < (int64_t)c->graph.n_table * c->HDmax * (int64_t)sizeof(float)) return fail(GAT_E_INVALID, "bound gPL table too small (needs n_table*max(H*D) floats)");
        if (!c->bwd.gPL_bound) dfree(c, c->bwd.gPL);
        c->bwd.gPL = (float*)d_ptr; c->bwd.gPL_bound = true;
        return 0;
    }
    return fail(GAT_E_INVALID, "unknown table");
}

}  // extern "C"
