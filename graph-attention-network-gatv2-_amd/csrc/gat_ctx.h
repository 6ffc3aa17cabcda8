// gat_ctx.h — the context behind include/gatv2_abi.h and the small helpers every ABI translation unit (gat_abi*.hip) needs.
// Private to those files: gat_internal.h stays the kernel-facing header and does not include this one, the kernel files never see
// the context.  The state of one feature is one named sub-struct of gat_ctx; functions shared between the ABI files are declared at the end.
#pragma once
#include "gat_internal.h"

#include <algorithm>
#include <cmath>
#include <memory>

namespace gat {

struct Layer {
    int32_t H = 0, D = 0, F = 0, HD = 0;
    int64_t w_off = 0, a_off = 0;
    int64_t wres_off = 0, b_off = 0;                // inside the Wres / b groups (gat_set_residual)
    int64_t ln_off = 0;                             // inside the gamma and the beta group (gat_set_norm)
    int64_t we_off = 0;                             // inside the We group (gat_set_edge_dim)
    float* PE = nullptr;      // [n_edges][HD]  EA We^T, fp32 also under bf16 storage (streamed by the edge passes, never gathered)
    float* R = nullptr;       // [n_rows][HD]  x' Wres^T of the shard's own rows (GAT_RES_LINEAR)
    float* PL = nullptr;      // [n_table][HD]  (table; may be caller-owned)
    bool PL_bound = false;
    float* PR = nullptr;      // [n_rows][HD]
    float* alpha = nullptr;   // [E][H]
    float* hpre = nullptr;    // [n_rows][HD]
    float* hout = nullptr;    // [n_rows][HD] / last: [n_rows][D]
    float* g = nullptr;       // [n_rows][HD]   dL/dh_pre (input_gradients[l], E:1339)
    float* ge = nullptr;      // [E][H]  (keep_taps)
    float* score = nullptr;   // [E][H]  (keep_taps) raw attention scores, E:323
    float* galpha = nullptr;  // [E][H]  (keep_taps) grad wrt attn_coeff, E:646
    float* mstat = nullptr;   // [n_rows][H] (keep_taps)
    bool stash = false;       // backward scatter through per-edge records + pull pass (edge_stash_words) instead of message rows
    float* zstat = nullptr;
};
struct Pending { int k; hipEvent_t e0, e1; };

}  // namespace gat

constexpr int kParamGroups = GAT_PARAM_HEAD_B + 1;   // GAT_PARAM_* are 0 .. 9, in packed order
struct gat_ctx {
    gat_config cfg{};
    std::vector<int32_t> heads, outdims;
    std::vector<gat::Layer> layers;
    int32_t HDmax = 0, Hmax = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool buffers_ready = false;                     // graph, features and labels / targets are set: everything sized by them exists
    int32_t dbg = 0;                                // GAT_DBG timing experiments (0 = product behaviour)
    std::vector<void*> owned;                       // every hipMalloc of this context

    // The graph: n_rows own rows (a destination range of a shard) over a source table of n_table rows that starts table_row0 rows before
    // them; the work list of the wave-per-item kernels (host copy, device items, per-segment partials of the split rows).
    struct Graph {
        int64_t n_rows = 0, n_edges = 0, n_table = 0, table_row0 = 0;
        bool have = false;
        int32_t* row_ptr = nullptr; int32_t* col_idx = nullptr;
        gat::WorkList work;
        int4* items = nullptr; int4* slot_info = nullptr; float* part_acc = nullptr; float* part_mz = nullptr;
    } graph;
    // Layer-0 input.  ld0: floats between rows of X0 / Xtab, in_dim rounded up to a multiple of 4 (zeros behind column in_dim), so that an
    // odd in_dim — Cora's 1,433 — still gets 16-byte loads.  Xtab: [n_table][ld0] replicated input (gat_set_source_features).
    struct Input {
        bool have = false;
        float* X0 = nullptr; float* Xtab = nullptr; int32_t ld0 = 0;
    } in;
    // Supervision of the head's rows.  labels_eff: with a training mask the label, or ~label outside the mask (null while no mask is set;
    // labels_eff_buf is its storage); train_mask: device copy of the active mask (re-applied when the labels change); mask_tmp: of the
    // last gat_eval_mask.  Loss modes (gatv2_abi.h): the mode (fixed once labels or targets were given), the targets [head rows][C] (one
    // buffer for the context's life: a captured step reads later values through the same pointer), mask_on: train_mask is active (mode 0
    // carries the mask in labels_eff), tgt_scratch [256]: the check's result word and the count's block partials.
    struct Supervision {
        bool have = false;
        int32_t* labels = nullptr; int32_t* labels_eff = nullptr; int32_t* labels_eff_buf = nullptr;
        uint8_t* mask_tmp = nullptr; uint8_t* train_mask = nullptr;
        int64_t n_labels = 0;                       // length the labels were set with
        int32_t loss_mode = 0; bool loss_locked = false, mask_on = false;
        float* targets = nullptr; unsigned long long* tgt_scratch = nullptr;
        double* eval_loss = nullptr; int32_t* eval_cnt = nullptr;      // block partials of gat_eval_mask
    } sup;
    // The packed parameters [W | a | Wo | Wres | b | gamma | beta | We | W1 | b1] and their gradients (+ 4 floats of tail: [loss, correct lo,
    // correct hi, -]).  group_cnt / group_off by GAT_PARAM_* (layout_params): floats in each group — Wres / b are empty unless
    // gat_set_residual, gamma / beta unless gat_set_norm, We unless gat_set_edge_dim, W1 / b1 unless gat_set_head_hidden switched them on — and the group's first float.
    // touched: a gat_params_* / gat_grads_* / gat_set_graph* call was made, the buffers keep their size.
    struct Packed {
        int64_t group_cnt[kParamGroups] = {0}, group_off[kParamGroups] = {0};
        float* params = nullptr; float* grads = nullptr; bool touched = false;
        float* adam_m = nullptr; float* adam_v = nullptr; float* clip_scratch = nullptr;
    } packed;
    // The optimizer on the device (gatv2_abi.h "optimizer"; gat_abi_optimizer.hip): the configuration, the state of its kind over the packed
    // layout (m, v: the Adam kinds; buf: SGD with momentum > 0; all apart from adam_m / adam_v above, which stay gat_step_adam's), the
    // device scalars t and lr, the record of norms [kOptGroups + 1], the block table with its partials.  have: gat_set_optimizer was called.
    struct Optimizer {
        bool have = false; gat_optimizer_config cfg{};
        float* m = nullptr; float* v = nullptr; float* buf = nullptr;
        unsigned long long* t = nullptr; float* lr = nullptr; float* norms = nullptr;
        gat::OptBlock* table = nullptr; float* partial = nullptr; int32_t n_blocks = 0;
        int32_t group_block0[gat::kOptGroups + 1] = {0};
    } opt;
    // Residual / bias (GAT_RES_* flags) and layer normalisation (GAT_NORM_* flags): G and agg [n_rows][HDmax] are dL/dh_pre and
    // h_pre - (R + b) of the layer whose backward runs; partial [L][kResPartialRows][HDmax] block column sums of G (grad_b) and
    // norm_partial [L][2][kResPartialRows][HDmax] (grad_gamma / grad_beta), one region per layer; the slabs of gradWres likewise.
    // Batch normalisation (GAT_BN_* flags, gatv2_abi.h "batch normalisation"): bn_stats [4][bn_total] = running mean | running var |
    // batch mean | batch rstd, each flat [l][H_l*D_l] at the layers' ln_off (not parameters: outside the packed buffers, allocated by
    // the setter and never moved); bn_partial [2][kResPartialRows][HDmax] the block partials of whichever launch runs (consumed by its
    // finish launch at once, so the layers share it) and bn_sums [2][HDmax] this step's s1 / s2.
    struct Residual {
        int32_t flags = 0, norm_flags = 0; float norm_eps = 0.f;
        int32_t bn_flags = 0; float bn_eps = 0.f, bn_momentum = 0.f;
        float* bn_stats = nullptr; int64_t bn_total = 0; float* bn_partial = nullptr; float* bn_sums = nullptr;
        float* G = nullptr; float* agg = nullptr; float* partial = nullptr; float* norm_partial = nullptr;
        float* gw_scratch = nullptr; std::vector<int64_t> gw_off;
    } res;
    // Edge features (gatv2_abi.h "edge features"): dim = Fe, the attribute rows EA [n_edges][ld] (ld = Fe rounded up to 4, zeros behind
    // column Fe), the one dL/dPE buffer gPE [n_edges][HDmax] the layers share, the slabs of gradWe (one region per layer).
    struct EdgeFeatures {
        int32_t dim = 0, ld = 0;
        float* EA = nullptr; bool have = false; float* gPE = nullptr;
        float* gw_scratch = nullptr; std::vector<int64_t> gw_off;
    } ef;
    // Dropout and DropEdge (gatv2_abi.h "dropout"): probabilities, seed, mode, the device step counter (advanced by the layer-0 projection
    // of a training forward), the unsharded node ids of a shard (gat_set_shard_bounds; null: node id = table row), the layer inputs after
    // feature dropout (x [L], rows as Xin_of; x_tab the replicated layer-0 input), allocated with p_f > 0.
    struct Dropout {
        float pf = 0.f, pa = 0.f;
        float edge_p = 0.f; int32_t edge_flags = 0;     // DropEdge (gat_set_dropedge); seed and counter are the dropout ones
        uint64_t seed = 0; bool training = true; uint64_t* step = nullptr;
        int64_t* bounds = nullptr; int64_t max_rows = 0;
        std::vector<float*> x; float* x_tab = nullptr;
    } drop;
    // Graph-level readout (gatv2_abi.h "graph-level readout"): mode, the graphs' row ranges, the graph of every row, the pooling's work
    // list and partial rows [n_parts][D_last], the pooled rows P the head reads, its gradient gP, the argmax rows of GAT_READOUT_MAX.
    struct Readout {
        int32_t mode = 0; int64_t n_graphs = 0;
        int32_t* graph_ptr = nullptr; int32_t* node_graph = nullptr;       // [n_graphs + 1], [n_rows]
        int4* items = nullptr; int64_t n_items = 0;
        int4* split = nullptr; int32_t n_split = 0;
        float* part = nullptr; int32_t* part_arg = nullptr;
        float* P = nullptr; float* gP = nullptr; int32_t* argmax = nullptr;       // [n_graphs][D_last]
    } readout;
    // Pair head (gatv2_abi.h "pair head"): mode, the pairs, the incidence index over the nodes (inc_ptr [n_rows + 1], inc [2 n_pairs]
    // entries {p, other}), the scatter's work list and partial rows (allocated once at their upper bounds: a replacement of the pairs
    // refills them), the rows Q the head reads and its gradient gQ [n_pairs][D_last].
    struct Pairs {
        int32_t mode = 0; int64_t n_pairs = 0;
        int32_t* u = nullptr; int32_t* v = nullptr;
        int32_t* inc_ptr = nullptr; int2* inc = nullptr;
        int4* items = nullptr; int64_t n_items = 0;
        int4* split = nullptr; int32_t n_split = 0;
        float* part = nullptr;
        float* Q = nullptr; float* gQ = nullptr;
    } pairs;
    // Negative sampling (gatv2_abi.h "negative sampling"): pairs [first, first + count) are the slots gat_resample_negatives redraws;
    // ascending: every row of the graph is (checked once, when the feature is first switched on: the sampler then searches a row
    // instead of scanning it); counter [1]: the kernel's unfiltered count; plan_key / plan_off [n_rows + 1] and plan_temp: the device
    // plan's scratch (pair_plan_device), allocated once; last_round / unfiltered: of the last resample.
    struct Negatives {
        int32_t mode = 0, flags = 0; int64_t first = 0, count = 0; uint64_t seed = 0;
        bool ascending_known = false, ascending = false;
        unsigned long long* counter = nullptr;
        unsigned long long* plan_key = nullptr; unsigned long long* plan_off = nullptr; void* plan_temp = nullptr; size_t plan_temp_bytes = 0;
        uint64_t last_round = 0; int64_t unfiltered = 0;
    } neg;
    // The output head: block partials, results, the class probabilities y (valid: y holds the last forward's, not after a fused head step;
    // ran: the head has run at least once, so its input rows are those of a forward).
    struct Head {
        float* hb_partial = nullptr; double* loss_partial = nullptr; int32_t* correct_partial = nullptr;
        float* loss_out = nullptr; int32_t* correct_out = nullptr;
        float* y = nullptr; bool y_valid = false, ran = false;
    } head;
    // Hidden layer in front of the head (gatv2_abi.h "hidden layer"): width Dh (0: off) and the activation flags; Z1 [R][Dh] = act(Xin W1^T
    // + b1), what the head reads; gZ1 [R][Dh] the head's input gradient, turned into gA in place; partial [head_hidden_blocks][Dh] block
    // column sums of gA (gradb1); gw_scratch the slabs of gradW1.  Allocated by ensure_buffers for R = head_rows.
    struct HeadHidden {
        int32_t width = 0, flags = 0;
        float* Z1 = nullptr; float* gZ1 = nullptr; float* partial = nullptr; float* gw_scratch = nullptr;
    } hid;
    // Ranking metrics (gatv2_abi.h "ranking metrics"): the buffers of gat_eval_rank, allocated at its first call for head rows x C slots
    // and kept (sizes: what they were allocated for).
    struct Rank {
        gat::RankBuffers buf; gat::RankSizes sizes; bool have = false;
    } rank;
    // Backward scratch.  gPL [n_table][HDmax] (may be caller-bound), gPR [n_rows][HDmax]; gH [n_rows][gh_stride] the head-independent output
    // gradient (gh_stride: D_last, or 16 = 64-B records {gH row | the row's LReLU'(h_pre) decision bytes at +32}, hbits); the per-edge
    // scatter: csc_pos [E] slot of each CSR edge in source-major order, src_index everything else the source-major pass walks (src_ptr null
    // = not built), msg [E][msg_hd] message rows or stash [E][stash_words] records (Layer::stash) in one buffer, gfull [n_rows][HDmax]
    // dL/dh_pre incl. LReLU' (gathered by the pull pass); ga_partial / gw_scratch: block partials of grad_a and the slabs of grad_w, one
    // region per layer (gw_off) — gw_scratch also serves the split-K projection.
    struct Backward {
        float* gPL = nullptr; bool gPL_bound = false; float* gPR = nullptr;
        float* gH = nullptr; int32_t gh_stride = 0; uint8_t* hbits = nullptr;
        int32_t* csc_pos = nullptr; gat::SourceIndex src_index;
        float* msg = nullptr; int32_t msg_hd = 0; uint32_t* stash = nullptr; int32_t stash_words = 0; float* gfull = nullptr;
        float* ga_partial = nullptr;
        float* gw_scratch = nullptr; int64_t gw_scratch_floats = 0; std::vector<int64_t> gw_off;
    } bwd;
    // Transport of a shard (gat_comm_init_*) and its options: chunks of the pipelined forward exchange with their second stream and
    // events, bf16 gPL partials, the halo plan (rows each peer's edges reference, built collectively; halo_on: the table exchanges use
    // it), grads_prev [n_params]: what the gradient buffer held before this step (reduce_begin).
    struct Exchange {
        std::unique_ptr<gat::Comm> comm;
        int32_t chunks = 1; hipStream_t stream = nullptr; std::vector<hipEvent_t> events;
        bool gpl_bf16 = false;
        gat::HaloPlan halo; bool halo_on = false;
        float* grads_prev = nullptr;
    } xch;
    // grad_w off the edge passes' stream (GAT_OVERLAP): a second gPL / gPR pair for the odd layers, so that layer l's grad_w may still read
    // its operands while layer l-1's edge passes write theirs; side stream + fork / join events per layer.  active: inside
    // backward_phases with the overlap on.
    struct Overlap {
        float* gPL = nullptr; float* gPR = nullptr; bool active = false;
        hipStream_t stream = nullptr;
        std::vector<hipEvent_t> fork, join;
    } ov;
    // gat_step as a replayed hipGraph (gat_step_graph).  state: 0 off, 1 armed (next step runs eagerly, then captures), 2 ready;
    // pinned_tail [4]: host-pinned landing zone of {loss, correct lo, correct hi}; y_after: what head.y_valid is after the captured body
    // (a replay runs none of the host code that keeps the flag: false when the body's head is the fused one, which writes no y).
    // entry: which entry point the slot holds or is warming up for (0 gat_step, 1 gat_train_step).
    struct Replay {
        int state = 0, warm = 0, entry = 0; bool y_after = false;
        hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        float* pinned_tail = nullptr;
    } replay;
    // Event timing per kernel class (cfg.collect_timing).
    struct Timing {
        std::vector<std::pair<hipEvent_t, hipEvent_t>> free;
        std::vector<gat::Pending> pending;
        int64_t launches[GAT_K_COUNT] = {0}; double ms[GAT_K_COUNT] = {0};
    } timing;
};

namespace gat {
// Device memory owned by the context (freed by gat_destroy, or earlier by dfree).  quiet: a failure leaves the error text alone — for
// the one caller that has a fall-back (the backward's scatter scratch).
inline int dmalloc(gat_ctx* c, void** p, size_t bytes, bool quiet = false) {
    if (bytes == 0) bytes = 4;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) {
        *p = nullptr;
        return quiet ? GAT_E_NOMEM : fail(GAT_E_NOMEM, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    }
    c->owned.push_back(*p);
    return 0;
}
template <class T> inline int dalloc(gat_ctx* c, T** p, int64_t count) { return dmalloc(c, (void**)p, (size_t)count * sizeof(T)); }
inline void dfree(gat_ctx* c, void* p) {
    if (!p) return;
    auto it = std::find(c->owned.begin(), c->owned.end(), p);
    if (it != c->owned.end()) { c->owned.erase(it); (void)hipFree(p); }
}
// device copy of a host list of int32 (`per` of them to an entry of *d: 4 for an int4 list), at least one entry allocated
template <class T> inline int upload_list(gat_ctx* c, T** d, const std::vector<int32_t>& h, int per) {
    GAT_TRY(dalloc(c, d, std::max<int64_t>((int64_t)(h.size() / per), 1)));
    if (!h.empty()) GAT_HIP(hipMemcpyAsync(*d, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    return 0;
}
inline int flush_events(gat_ctx* c) {
    if (c->timing.pending.empty()) return 0;
    GAT_HIP(hipStreamSynchronize(c->stream));
    for (auto& p : c->timing.pending) {
        float ms = 0.f;
        GAT_HIP(hipEventElapsedTime(&ms, p.e0, p.e1));
        c->timing.ms[p.k] += ms;
        c->timing.launches[p.k] += 1;
        c->timing.free.emplace_back(p.e0, p.e1);
    }
    c->timing.pending.clear();
    return 0;
}
struct Scope {      // brackets the launches of one kernel class with a HIP event pair (on the stream they are launched on)
    gat_ctx* c; int k; hipEvent_t e0 = nullptr, e1 = nullptr; bool on; hipStream_t st;
    Scope(gat_ctx* c_, int k_, hipStream_t st_ = nullptr) : c(c_), k(k_), on(c_->cfg.collect_timing != 0), st(st_ ? st_ : c_->stream) {
        if (!on) return;
        if (c->timing.pending.size() >= 2048) (void)flush_events(c);
        if (c->timing.free.empty()) {
            if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { on = false; return; }
        } else { e0 = c->timing.free.back().first; e1 = c->timing.free.back().second; c->timing.free.pop_back(); }
        (void)hipEventRecord(e0, st);
    }
    ~Scope() {
        if (!on) return;
        (void)hipEventRecord(e1, st);
        c->timing.pending.push_back({k, e0, e1});
    }
};
inline bool bf16(const gat_ctx* c) { return c->cfg.storage_dtype == GAT_DTYPE_BF16; }
inline int64_t st_bytes(const gat_ctx* c) { return bf16(c) ? 2 : 4; }       // element size of PL / message rows
inline int check_layer(gat_ctx* c, int32_t l) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (l < 0 || l >= c->cfg.num_layers) return fail(GAT_E_INVALID, "layer index out of range");
    if (!c->buffers_ready && c->sup.loss_mode != 0 && !c->sup.targets)
        return fail(GAT_E_STATE, "targets not set: the context's loss mode needs gat_set_targets (after set_graph / set_features)");
    if (!c->buffers_ready) return fail(GAT_E_STATE, "set_graph / set_features / set_labels must come first");
    return 0;
}
// layer l's part of a parameter group (layer_off: the layer's offset inside the group) and of its gradient
inline float* param_of(gat_ctx* c, int group, int64_t layer_off = 0) { return c->packed.params + c->packed.group_off[group] + layer_off; }
inline float* grad_of(gat_ctx* c, int group, int64_t layer_off = 0) { return c->packed.grads + c->packed.group_off[group] + layer_off; }
inline float* W_of(gat_ctx* c, int l) { return param_of(c, GAT_PARAM_W, c->layers[l].w_off); }
inline float* a_of(gat_ctx* c, int l) { return param_of(c, GAT_PARAM_A, c->layers[l].a_off); }
inline float* Wo_of(gat_ctx* c) { return param_of(c, GAT_PARAM_WO); }
inline float* gW_of(gat_ctx* c, int l) { return grad_of(c, GAT_PARAM_W, c->layers[l].w_off); }
inline float* ga_of(gat_ctx* c, int l) { return grad_of(c, GAT_PARAM_A, c->layers[l].a_off); }
inline float* gWo_of(gat_ctx* c) { return grad_of(c, GAT_PARAM_WO); }
inline float* We_of(gat_ctx* c, int l) { return param_of(c, GAT_PARAM_WE, c->layers[l].we_off); }
inline float* gWe_of(gat_ctx* c, int l) { return grad_of(c, GAT_PARAM_WE, c->layers[l].we_off); }
inline float* lng_of(gat_ctx* c, int l) { return param_of(c, GAT_PARAM_LN_G, c->layers[l].ln_off); }
inline float* lnb_of(gat_ctx* c, int l) { return param_of(c, GAT_PARAM_LN_B, c->layers[l].ln_off); }
inline float* glng_of(gat_ctx* c, int l) { return grad_of(c, GAT_PARAM_LN_G, c->layers[l].ln_off); }
inline float* glnb_of(gat_ctx* c, int l) { return grad_of(c, GAT_PARAM_LN_B, c->layers[l].ln_off); }
// null while the group is off
inline float* Wres_of(gat_ctx* c, int l) { return c->packed.group_cnt[GAT_PARAM_WRES] ? param_of(c, GAT_PARAM_WRES, c->layers[l].wres_off) : nullptr; }
inline float* b_of(gat_ctx* c, int l) { return c->packed.group_cnt[GAT_PARAM_B] ? param_of(c, GAT_PARAM_B, c->layers[l].b_off) : nullptr; }
inline float* gWres_of(gat_ctx* c, int l) { return grad_of(c, GAT_PARAM_WRES, c->layers[l].wres_off); }
inline float* gb_of(gat_ctx* c, int l) { return grad_of(c, GAT_PARAM_B, c->layers[l].b_off); }
inline int64_t n_params(const gat_ctx* c) { return c->packed.group_off[kParamGroups - 1] + c->packed.group_cnt[kParamGroups - 1]; }
inline bool res_on(const gat_ctx* c) { return c->res.flags != 0; }
inline bool norm_on(const gat_ctx* c) { return c->res.norm_flags != 0; }
// layer l is normalised (gatv2_abi.h "layer normalisation")
inline bool norm_layer(const gat_ctx* c, int l) {
    return norm_on(c) && !((c->res.norm_flags & GAT_NORM_SKIP_LAST) && l == c->cfg.num_layers - 1);
}
inline bool bn_on(const gat_ctx* c) { return c->res.bn_flags != 0; }
// layer l is batch-normalised (gatv2_abi.h "batch normalisation")
inline bool bn_layer(const gat_ctx* c, int l) {
    return bn_on(c) && !((c->res.bn_flags & GAT_BN_SKIP_LAST) && l == c->cfg.num_layers - 1);
}
// one of the four statistics vectors (GAT_BN_*) of layer l
inline float* bn_stat_of(gat_ctx* c, int which, int l) { return c->res.bn_stats + (int64_t)which * c->res.bn_total + c->layers[l].ln_off; }
// what layer l normalises with now: the batch's statistics in training mode, the running ones in eval mode (training: of the dropout block,
// the one mode switch of the context)
inline BnStats bn_stats_now(gat_ctx* c, int l);
// a batch-norm context takes no destination-range shard (asked by the calls that set the graph: the feature is switched on before them)
inline int bn_refuse_shard(const gat_ctx* c, int64_t n_rows, int64_t n_table, int64_t table_row0) {
    if (bn_on(c) && (n_table != n_rows || table_row0 != 0))
        return fail(GAT_E_UNSUPPORTED, "gat_set_batch_norm: not on a destination-range shard (n_table != n_rows or table_row0 != 0): the column statistics of a shard would need an exchange");
    return 0;
}
// the context runs the residual route: the forward takes EdgeFwdExtras, the backward the N-sized kernel, G and agg in the edge backward
inline bool res_route(const gat_ctx* c) { return res_on(c) || norm_on(c) || bn_on(c); }
inline bool edge_feat_on(const gat_ctx* c) { return c->ef.dim > 0; }
inline bool readout_on(const gat_ctx* c) { return c->readout.mode != GAT_READOUT_NONE; }
inline bool pairs_on(const gat_ctx* c) { return c->pairs.mode != GAT_PAIR_NONE; }
inline bool hidden_on(const gat_ctx* c) { return c->hid.width > 0; }
// width of the rows the output head reads (columns of Wo): Dh with a hidden layer in front of it, else D_last
inline int32_t head_width(const gat_ctx* c) { return hidden_on(c) ? c->hid.width : c->layers.back().D; }
// the hidden stage's activation as a slope: 0 = ReLU
inline float hidden_slope(const gat_ctx* c) { return (c->hid.flags & GAT_HEAD_ACT_LRELU) ? c->cfg.negative_slope : 0.f; }
// a hidden-head context takes no destination-range shard (asked by the calls that set the graph: the feature is switched on before them)
inline int hidden_refuse_shard(const gat_ctx* c, int64_t n_rows, int64_t n_table) {
    if (hidden_on(c) && n_table != n_rows)
        return fail(GAT_E_UNSUPPORTED, "gat_set_head_hidden: not on a destination-range shard (n_table != n_rows) or with a transport (the head's rows may straddle shards)");
    return 0;
}
inline float* W1_of(gat_ctx* c) { return c->packed.params + c->packed.group_off[GAT_PARAM_HEAD_W]; }
inline float* b1_of(gat_ctx* c) { return c->packed.params + c->packed.group_off[GAT_PARAM_HEAD_B]; }
inline float* gW1_of(gat_ctx* c) { return c->packed.grads + c->packed.group_off[GAT_PARAM_HEAD_W]; }
inline float* gb1_of(gat_ctx* c) { return c->packed.grads + c->packed.group_off[GAT_PARAM_HEAD_B]; }
// rows of the output head, hence of the labels, the targets, the masks and y: the pairs of a pair head, the graphs with readout on, else
// the nodes (the two features exclude each other)
inline int64_t head_rows(const gat_ctx* c) { return pairs_on(c) ? c->pairs.n_pairs : readout_on(c) ? c->readout.n_graphs : c->graph.n_rows; }
// what one of them is called in the length checks' texts
inline const char* head_row_name(const gat_ctx* c) { return pairs_on(c) ? "pair" : readout_on(c) ? "graph" : "node"; }
// a step / phase on a context with edge_dim > 0 needs the attribute rows
inline int check_edge_features(gat_ctx* c) {
    if (edge_feat_on(c) && !c->ef.have)
        return fail(GAT_E_STATE, "edge features not set: the context has edge_dim > 0 (gat_set_edge_dim) but gat_set_edge_features was never called");
    return 0;
}
inline LnArgs ln_args(gat_ctx* c, int l) {
    LnArgs a;
    if (norm_layer(c, l)) { a.gamma = lng_of(c, l); a.beta = lnb_of(c, l); a.eps = c->res.norm_eps; }
    return a;
}
inline BnStats bn_stats_now(gat_ctx* c, int l) {
    BnStats s{};
    s.eps = c->res.bn_eps; s.from_var = c->drop.training ? 0 : 1;
    s.mean = bn_stat_of(c, c->drop.training ? GAT_BN_BATCH_MEAN : GAT_BN_RUNNING_MEAN, l);
    s.scale = bn_stat_of(c, c->drop.training ? GAT_BN_BATCH_RSTD : GAT_BN_RUNNING_VAR, l);
    return s;
}
inline bool feat_drop_on(const gat_ctx* c) { return c->drop.training && c->drop.pf > 0.f; }
inline bool attn_drop_on(const gat_ctx* c) { return c->drop.training && c->drop.pa > 0.f; }
inline bool edge_drop_on(const gat_ctx* c) { return c->drop.training && c->drop.edge_p > 0.f; }
inline bool drop_on(const gat_ctx* c) { return feat_drop_on(c) || attn_drop_on(c) || edge_drop_on(c); }
// what layer l reads as its input: x_l, or x_l with the feature-dropout mask applied (projection and grad_W alike)
inline const float* Xin_raw(gat_ctx* c, int l) { return l == 0 ? c->in.X0 : c->layers[l - 1].hout; }
inline const float* Xin_of(gat_ctx* c, int l) { return feat_drop_on(c) && (size_t)l < c->drop.x.size() && c->drop.x[(size_t)l] ? c->drop.x[(size_t)l] : Xin_raw(c, l); }
inline const float* Xtab_of(gat_ctx* c) { return feat_drop_on(c) && c->drop.x_tab ? c->drop.x_tab : c->in.Xtab; }
inline uint32_t drop_threshold(double p) { return (uint32_t)std::min<double>(16777216.0, std::floor(p * 16777216.0 + 0.5)); }
// The mask parameters of layer l, fully identified (step, seed, bounds, row0, layer).  kind = kDropAttn: what the edge passes take —
// attention dropout and DropEdge; kDropFeat: the feature mask of the layer's input.  The thresholds are those of the masks that are
// active now (training mode, p > 0) — with `setting`, those of the settings whatever the mode (the taps) — and 0 / scale 1 otherwise;
// on: a mask is active (under `setting` it says the same of the settings; the tap kernels do not read it, and the attention-keep tap
// ignores the DropEdge fields it is handed along).
inline DropArgs drop_args(gat_ctx* c, int32_t l, int32_t kind = kDropAttn, bool setting = false) {
    const bool live = c->drop.training || setting;
    const double p = !live ? 0.0 : kind == kDropAttn ? c->drop.pa : c->drop.pf;
    const bool edges = live && kind == kDropAttn && c->drop.edge_p > 0.f;
    DropArgs d{};
    d.step = c->drop.step; d.bounds = c->drop.bounds; d.max_rows = c->drop.max_rows; d.row0 = c->graph.table_row0;
    d.seed_lo = (uint32_t)c->drop.seed; d.seed_hi = (uint32_t)(c->drop.seed >> 32);
    d.T = drop_threshold(p);
    d.scale = (float)(1.0 / (1.0 - p));
    if (edges) { d.Te = drop_threshold(c->drop.edge_p); d.eflags = c->drop.edge_flags; }
    d.layer = l;
    d.on = p > 0.0 || edges;
    return d;
}
inline int32_t ldX_of(gat_ctx* c, int l) { return l == 0 ? c->in.ld0 : c->layers[l].F; }
inline float* gPL_of(gat_ctx* c, int l) { return (c->ov.active && (l & 1)) ? c->ov.gPL : c->bwd.gPL; }
inline float* gPR_of(gat_ctx* c, int l) { return (c->ov.active && (l & 1)) ? c->ov.gPR : c->bwd.gPR; }

// A feature without a form in the GAT_DBG timing experiments refuses them: "<who>: not with a GAT_DBG timing experiment<tail>".  Nothing
// in the release library, which does not know the switch's name.
#ifdef GAT_EXPERIMENTS
#define GAT_REFUSE_DBG(c, applies, who, tail) \
    do { if ((c)->dbg != 0 && (applies)) return ::gat::fail(GAT_E_UNSUPPORTED, who ": not with a GAT_DBG timing experiment" tail); } while (0)
#else
#define GAT_REFUSE_DBG(c, applies, who, tail) do {} while (0)
#endif
// The setters that change the packed layout (gat_set_residual / gat_set_norm / gat_set_batch_norm / gat_set_edge_dim / gat_set_head_hidden) open with this refusal, make their own
// checks, set their fields and end with relayout().
#define GAT_LAYOUT_OPEN(c, who)                                                                                                  \
    do { if ((c)->packed.touched) return ::gat::fail(GAT_E_STATE, who ": call it before the first gat_params_*, gat_grads_* or " \
                                                                      "gat_set_graph* call (the packed buffers change size)"); } while (0)

// ---- defined in one ABI file, used in others ----------------------------------------------------------------------------------------
int relayout(gat_ctx* c);                 // gat_abi.hip: the packed layout for the groups that are on now, the packed buffers at their new size
int ensure_drop_step(gat_ctx* c);         // gat_abi.hip: the dropout step counter, zeroed when first needed (before gat_set_dropout: seed 0, counter 0)
int ensure_drop_buffers(gat_ctx* c);      // gat_abi.hip: feature-dropout copies of the layer inputs (only once p_f > 0 was set on a complete context)
int ensure_buffers(gat_ctx* c);           // gat_abi.hip: everything sized by the graph, once graph, features and labels / targets are all set
void graph_drop(gat_ctx* c);              // gat_abi_step.hip: forgets a captured step (it holds pointers and a kernel sequence); the next one runs eagerly
HeadArgs head_args(gat_ctx* c);           // gat_abi_step.hip: the output head's arguments in the context's loss mode: the rows it reads (readout / pair / hidden overrides), outputs, partial buffers
int head_hidden_check(gat_ctx* c);        // gat_abi_features.hip: the head's shape limits at the hidden width and the shard refusal, once the graph (and the loss mode) are known
int optimizer_launch(gat_ctx* c);         // gat_abi_optimizer.hip: the two launches of an optimizer step on the context's stream (gat_set_optimizer was called)
bool fused_last(gat_ctx* c);              // gat_abi_step.hip: gat_step runs the last layer's edge passes and the head's gradient as one kernel (GAT_FUSE_LAST=1)

}  // namespace gat
