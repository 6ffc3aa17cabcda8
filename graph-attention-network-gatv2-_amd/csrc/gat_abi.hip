// gat_abi.hip — implementation of include/gatv2_abi.h, first part: error state and choice switches, the context's life (create / destroy /
// sync), the packed parameter layout, the memory plan of a complete context (ensure_buffers), parameters and gradients, the optimizer
// steps, the kernel statistics.  The rest is in gat_abi_*.hip (by concern) and gat_ops.hip (op level); gat_ctx.h holds the context.
// Replaces the inline allocation + launch code of the reference's main() (GATv2_edge_based.cu E:1151-1357 memory plan, E:1370-1642 epoch loop).
#include "gat_ctx.h"
#include <cstdlib>
#include <cstring>
#include <mutex>

namespace gat {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int fail(int code, const std::string& msg) {
    g_err = msg;
    return code ? code : GAT_E_INVALID;
}
// Choice switches: environment variables that select among kernels / launch shapes computing the SAME results (the test
// matrices force every one).  Each is read once per process through here, and what was set is reported by gat_switches().
static std::mutex g_choice_mu;
static std::vector<std::pair<std::string, std::string>> g_choices;
const char* choice_env(const char* name) {
    const char* e = getenv(name);
    if (e) {
        std::lock_guard<std::mutex> lock(g_choice_mu);
        bool seen = false;
        for (auto& kv : g_choices) if (kv.first == name) { kv.second = e; seen = true; }
        if (!seen) g_choices.emplace_back(name, e);
    }
    return e;
}
static std::string choices_text() {
    std::lock_guard<std::mutex> lock(g_choice_mu);
    std::string t;
    for (auto& kv : g_choices) { if (!t.empty()) t += ' '; t += kv.first + "=" + kv.second; }
    return t;
}

// The packed layout [W | a | Wo | Wres | b | gamma | beta | We | W1 | b1]: every layer's offset inside the groups, the groups' sizes and where they
// start.  Called whenever the set of groups changes: by relayout (gat_create, gat_set_residual, gat_set_norm, gat_set_edge_dim, gat_set_head_hidden).
static void layout_params(gat_ctx* c) {
    int64_t* n = c->packed.group_cnt;
    std::fill(n, n + kParamGroups, (int64_t)0);
    for (Layer& y : c->layers) {
        y.w_off = n[GAT_PARAM_W]; y.a_off = n[GAT_PARAM_A]; y.wres_off = n[GAT_PARAM_WRES]; y.b_off = n[GAT_PARAM_B]; y.ln_off = n[GAT_PARAM_LN_G]; y.we_off = n[GAT_PARAM_WE];
        n[GAT_PARAM_W] += (int64_t)y.HD * 2 * y.F;                       // E:1248-1254
        n[GAT_PARAM_A] += y.HD;
        if (c->res.flags & GAT_RES_LINEAR) n[GAT_PARAM_WRES] += (int64_t)y.HD * y.F;
        if (c->res.flags & GAT_RES_BIAS) n[GAT_PARAM_B] += y.HD;
        if (c->res.norm_flags != 0 || c->res.bn_flags != 0) n[GAT_PARAM_LN_G] += y.HD;   // all L layers; with GAT_NORM_SKIP_LAST / GAT_BN_SKIP_LAST the last one's entries are never read
        n[GAT_PARAM_WE] += (int64_t)y.HD * c->ef.dim;
    }
    n[GAT_PARAM_WO] = (int64_t)c->cfg.num_classes * head_width(c);      // [C][Dh] behind a hidden layer
    if (hidden_on(c)) { n[GAT_PARAM_HEAD_W] = (int64_t)c->hid.width * c->layers.back().D; n[GAT_PARAM_HEAD_B] = c->hid.width; }
    n[GAT_PARAM_LN_B] = n[GAT_PARAM_LN_G];
    for (int k = 0; k < kParamGroups; ++k) c->packed.group_off[k] = k ? c->packed.group_off[k - 1] + n[k - 1] : 0;
}
int relayout(gat_ctx* c) {
    layout_params(c);
    const int64_t np = n_params(c);
    GAT_HIP(hipStreamSynchronize(c->stream));
    dfree(c, c->packed.params); dfree(c, c->packed.grads);
    c->packed.params = nullptr; c->packed.grads = nullptr;
    GAT_TRY(dalloc(c, &c->packed.params, np));
    GAT_TRY(dalloc(c, &c->packed.grads, np + 4));
    GAT_HIP(hipMemsetAsync(c->packed.params, 0, np * sizeof(float), c->stream));
    GAT_HIP(hipMemsetAsync(c->packed.grads, 0, np * sizeof(float), c->stream));
    return 0;
}
int ensure_drop_step(gat_ctx* c) {
    if (c->drop.step) return 0;
    GAT_TRY(dalloc(c, &c->drop.step, 1));
    GAT_HIP(hipMemsetAsync(c->drop.step, 0, sizeof(uint64_t), c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
int ensure_drop_buffers(gat_ctx* c) {
    if (!c->buffers_ready || c->drop.pf <= 0.f) return 0;
    const int L = c->cfg.num_layers;
    if (c->drop.x.empty()) {
        c->drop.x.assign((size_t)L, nullptr);
        for (int l = 0; l < L; ++l) GAT_TRY(dalloc(c, &c->drop.x[(size_t)l], c->graph.n_rows * (l == 0 ? c->in.ld0 : c->layers[l].F)));
    }
    if (c->in.Xtab && !c->drop.x_tab) GAT_TRY(dalloc(c, &c->drop.x_tab, c->graph.n_table * c->in.ld0));
    return 0;
}
int ensure_buffers(gat_ctx* c) {
    if (c->buffers_ready) return 0;
    if (!(c->graph.have && c->in.have && c->sup.have)) return 0;
    GAT_TRY(head_hidden_check(c));                   // the head's limits at the hidden width, now that the loss mode is fixed
    const int L = c->cfg.num_layers;
    const int64_t N = c->graph.n_rows, E = c->graph.n_edges, T = c->graph.n_table;
    for (int l = 0; l < L; ++l) {
        Layer& y = c->layers[l];
        if (bf16(c) && !edge_fast_path(y.H, y.D, T))
            return fail(GAT_E_UNSUPPORTED, "bf16 storage needs every layer on the wave-per-row path (H*D in {8,16,32,64}, D a power of two)");
        if (!y.PL_bound) GAT_TRY(dmalloc(c, (void**)&y.PL, (size_t)(T * y.HD * st_bytes(c))));
        GAT_TRY(dalloc(c, &y.PR, N * y.HD));
        // attn_coeff [E][H] is only materialised for parity taps and for layers on the generic
        // path; the fast path's backward recomputes it from the per-(row, head) softmax stats.
        if (c->cfg.keep_taps || !edge_fast_path(y.H, y.D, c->graph.n_table)) GAT_TRY(dalloc(c, &y.alpha, E * y.H));
        GAT_TRY(dalloc(c, &y.hpre, N * y.HD));
        GAT_TRY(dalloc(c, &y.hout, N * (l == L - 1 ? y.D : y.HD)));
        // the last layer's g is formed inside its edge backward from gH (except in the flat-index mode, E:598)
        if (l < L - 1 || c->cfg.flat_lrelu_index) GAT_TRY(dalloc(c, &y.g, N * y.HD));
        GAT_TRY(dalloc(c, &y.mstat, N * y.H));
        GAT_TRY(dalloc(c, &y.zstat, N * y.H));
        if (c->cfg.keep_taps) {
            GAT_TRY(dalloc(c, &y.ge, E * y.H));
            GAT_TRY(dalloc(c, &y.score, E * y.H));
            GAT_TRY(dalloc(c, &y.galpha, E * y.H));
        }
    }
    if (!c->bwd.gPL_bound) GAT_TRY(dalloc(c, &c->bwd.gPL, T * c->HDmax));
    GAT_TRY(dalloc(c, &c->bwd.gPR, N * c->HDmax));
    if (!c->cfg.flat_lrelu_index) {
        // the last layer's pull pass rebuilds g from gH and one decision byte per lane: both in ONE 64-byte record per
        // node, so that an edge costs one cache line there instead of two (the edge passes are bound by the number of
        // L1 misses in flight, not by bytes: DESIGN §4)
        const Layer& yl = c->layers[L - 1];
        const int w = edge_stash_words(yl.H, yl.D);
        // (a hidden layer's gXin = gA W1 is written by a dense launcher: plain rows of D_last floats)
        c->bwd.gh_stride = (w > 0 && w <= 32 && yl.D <= 8 && !bf16(c) && !c->cfg.keep_taps && !hidden_on(c)) ? 16 : yl.D;
        GAT_TRY(dalloc(c, &c->bwd.gH, N * c->bwd.gh_stride));
    }
    // work items (rows / hub-row segments) of the wave-per-item kernels
    GAT_TRY(dalloc(c, &c->graph.items, std::max<int64_t>(c->graph.work.n_items, 1)));
    GAT_TRY(dalloc(c, &c->graph.slot_info, std::max<int32_t>(c->graph.work.n_slots + c->graph.work.n_split, 1)));
    GAT_TRY(dalloc(c, &c->graph.part_acc, (int64_t)std::max<int32_t>(c->graph.work.n_slots, 1) * c->HDmax));
    GAT_TRY(dalloc(c, &c->graph.part_mz, (int64_t)std::max<int32_t>(c->graph.work.n_slots, 1) * 2 * c->Hmax));
    if (c->graph.work.n_items > 0)
        GAT_HIP(hipMemcpyAsync(c->graph.items, c->graph.work.items.data(), c->graph.work.items.size() * sizeof(int32_t),
                               hipMemcpyHostToDevice, c->stream));
    if (c->graph.work.n_slots > 0)
        GAT_HIP(hipMemcpyAsync(c->graph.slot_info, c->graph.work.slot_info.data(), c->graph.work.slot_info.size() * sizeof(int32_t),
                               hipMemcpyHostToDevice, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    // Store-then-sum backward for the layers on the wave-per-row fast path: needs the source-major
    // slot index and an [E][H*D] scratch.  GAT_BWD_ATOMICS=1 forces the float-atomic variant (A/B).
    // Which form the per-edge scatter takes, per layer: the stash path (64-B records + one gathered row of g[dst] in
    // the source-major pass) where the shape has one, else H*D-float message rows.  GAT_BWD_STASH=0 forces message
    // rows everywhere (the A/B of DESIGN §4); the taps variant of the backward always uses message rows.
    int32_t msg_hd = 0, stash_words = 0;
    const char* no_stash = choice_env("GAT_BWD_STASH");
    for (int l = 0; l < L; ++l) {
        Layer& y = c->layers[l];
        if (!edge_fast_path(y.H, y.D, c->graph.n_table)) continue;
        const int w = edge_stash_words(y.H, y.D);
        // bf16 storage: only where the message row (H*D*2 bytes) is larger than a record — at H*D = 32 the record path
        // trades a 64-B streamed row for a 32-B record plus a 64-B random gather and loses (10 M / 250 M shape: the
        // source-major pass 8.4 -> 13.4 ms per step, the destination-major pass unchanged)
        y.stash = w > 0 && !c->cfg.keep_taps && !(no_stash && no_stash[0] == '0') && !(bf16(c) && y.HD < 64);
        if (y.stash) stash_words = std::max(stash_words, w); else msg_hd = std::max(msg_hd, y.HD);
    }
    const char* force = choice_env("GAT_BWD_ATOMICS");
    if ((msg_hd > 0 || stash_words > 0) && E > 0 && !(force && force[0] == '1')) {
        float* m = nullptr;
        int32_t *src_ptr = nullptr, *cdst = nullptr, *cedge = nullptr, *csrc = nullptr;      // the SourceIndex's arrays while they are written
        // E + 1 rows / records: the last one takes the stores of the group-per-row kernels' padded lanes; kPullPad records of
        // padding behind the records and the destination list: the pull pass reads whole 16-slot chunks without clamping
        if (dmalloc(c, (void**)&m, std::max<size_t>((size_t)(E + kPullPad) * msg_hd * (size_t)st_bytes(c), (size_t)(E + kPullPad) * stash_words * sizeof(uint32_t)), true) == 0) {
            if (msg_hd > 0) { c->bwd.msg = m; c->bwd.msg_hd = msg_hd; }
            if (stash_words > 0) {                  // records and message rows are never live at the same time: one buffer
                c->bwd.stash = reinterpret_cast<uint32_t*>(m); c->bwd.stash_words = stash_words;
                if (msg_hd == 0) { c->bwd.msg = m; c->bwd.msg_hd = 0; }
                GAT_TRY(dalloc(c, &c->bwd.gfull, N * c->HDmax));
                if (c->layers[L - 1].stash && c->bwd.gH != nullptr && c->bwd.gh_stride == 16) c->bwd.hbits = reinterpret_cast<uint8_t*>(c->bwd.gH) + 32;
                GAT_TRY(dalloc(c, &cdst, E + kPullPad));
                GAT_HIP(hipMemsetAsync(cdst + E, 0, (size_t)kPullPad * sizeof(int32_t), c->stream));      // padding: row 0 (any valid row)
                // the CSR edge of every slot (4 B per slot): fp32 records may lie in edge order (records_take_edge_order)
                if (!bf16(c)) GAT_TRY(dalloc(c, &cedge, E + kPullPad));
                GAT_HIP(hipMemsetAsync(reinterpret_cast<uint32_t*>(m) + (size_t)E * stash_words, 0, (size_t)kPullPad * stash_words * sizeof(uint32_t), c->stream));
            }
            GAT_TRY(dalloc(c, &c->bwd.csc_pos, E));
            GAT_TRY(dalloc(c, &src_ptr, T + 1));
            // slot-parallel source-major pass (gat_csc.hip "runs"): the source of every slot + the lists crossing a run boundary.
            // GAT_PULL_RUN=<slots per run> (a multiple of 32; 0 = do not build)
            static const int run_env = [] { const char* e = choice_env("GAT_PULL_RUN"); return e ? atoi(e) : -1; }();
            const int32_t run = run_env >= 0 ? (run_env / 32) * 32 : 64;
            if (run > 0) GAT_TRY(dalloc(c, &csrc, E + kPullPad));
            GAT_TRY(build_csc(c->graph.col_idx, E, T, c->bwd.csc_pos, src_ptr, csrc, c->stream));
            if (cdst) GAT_TRY(build_csc_dst(c->graph.row_ptr, c->bwd.csc_pos, cdst, N, E, c->stream, cedge));
            SourceIndex& ix = c->bwd.src_index;
            ix.src_ptr = src_ptr; ix.cdst = cdst; ix.cedge = cedge; ix.n_table = T; ix.n_slots = E; ix.slot_capacity = E + kPullPad;
            HeavyList hl;
            GAT_TRY(build_heavy_list(src_ptr, T, E, &hl, c->stream, run));
            if (hl.run > 0 && csrc != nullptr) {
                ix.run = hl.run; ix.n_runs = hl.n_runs; ix.n_open = (int32_t)(hl.open.size() / 4); ix.n_empty = (int64_t)hl.empty.size();
                int4* d_open = nullptr; int32_t* d_empty = nullptr;
                GAT_TRY(upload_list(c, &d_open, hl.open, 4));
                GAT_TRY(upload_list(c, &d_empty, hl.empty, 1));
                GAT_TRY(dalloc(c, &ix.run_part, std::max<int64_t>(2 * ix.n_runs, 1) * c->HDmax));
                GAT_HIP(hipStreamSynchronize(c->stream));
                ix.open = d_open; ix.empty = d_empty; ix.csrc = csrc;
            }
            ix.n_chunks = (int32_t)(hl.chunks.size() / 4); ix.n_heavy = (int32_t)(hl.heavy.size() / 4);
            if (c->bwd.stash != nullptr && !hl.items.empty()) {
                int4* d_items = nullptr;
                GAT_TRY(upload_list(c, &d_items, hl.items, 4));
                GAT_HIP(hipStreamSynchronize(c->stream));
                ix.items = d_items; ix.n_items = (int64_t)(hl.items.size() / 4);
            }
            if (ix.n_heavy > 0) {
                int4* d_chunks = nullptr; int4* d_heavy = nullptr;
                GAT_TRY(upload_list(c, &d_chunks, hl.chunks, 4));
                GAT_TRY(upload_list(c, &d_heavy, hl.heavy, 4));
                GAT_TRY(dalloc(c, &ix.part, (int64_t)ix.n_chunks * c->HDmax));
                GAT_HIP(hipStreamSynchronize(c->stream));
                ix.chunks = d_chunks; ix.heavy = d_heavy;
            }
        } else (void)hipGetLastError();       // not enough HBM for the scratch
    }
    if (!c->bwd.msg) for (int l = 0; l < L; ++l) c->layers[l].stash = false;      // no scatter scratch: the atomics variant
    // one region per layer (grad_a block partials, grad_w slabs): their reductions are queued until the end of the
    // backward and run as one launch (reduce_batch_flush), so a later layer must not overwrite an earlier layer's slabs
    GAT_TRY(dalloc(c, &c->bwd.ga_partial, (int64_t)L * kGaPartialRows * c->HDmax));  // per layer >= any edge_backward_blocks()
    int64_t gw = 0;
    c->bwd.gw_off.assign((size_t)L, 0);
    for (int l = 0; l < L; ++l) { c->bwd.gw_off[(size_t)l] = gw; gw += grad_w_scratch_floats(N, c->layers[l].F, c->layers[l].HD); }
    gw = std::max<int64_t>(gw, 1);
    if (c->in.Xtab) gw = std::max(gw, grad_w_scratch_floats(T, c->layers[0].F, c->layers[0].HD));
    // split-K projection (few rows, long K): sized from the exact (rows, part) pairs gat_layer_project launches
    for (int l = 0; l < L; ++l) {
        const Layer& y = c->layers[l];
        if (l == 0 && c->in.Xtab) gw = std::max({gw, project_scratch_floats(T, y.F, y.HD, kPartLeft), project_scratch_floats(N, y.F, y.HD, kPartRight)});
        else gw = std::max(gw, project_scratch_floats(N, y.F, y.HD, kPartBoth));
    }
    GAT_TRY(dalloc(c, &c->bwd.gw_scratch, gw));
    c->bwd.gw_scratch_floats = gw;
    const int C = c->cfg.num_classes, DL = head_width(c);      // the rows the head reads: Dh floats behind a hidden layer
    const int64_t NH = head_rows(c);                 // graphs with readout on
    if (hidden_on(c)) {                              // gatv2_abi.h "hidden layer": Z1 and gZ1 [R][Dh], the column-sum partials, the slabs of gradW1
        const int32_t Dh = c->hid.width;
        GAT_TRY(dalloc(c, &c->hid.Z1, NH * Dh));
        GAT_TRY(dalloc(c, &c->hid.gZ1, NH * Dh));
        GAT_TRY(dalloc(c, &c->hid.partial, (int64_t)kHiddenPartialRows * Dh));
        GAT_TRY(dalloc(c, &c->hid.gw_scratch, std::max<int64_t>(grad_w_scratch_floats(NH, c->layers[L - 1].D, Dh), 1)));
    }
    GAT_TRY(dalloc(c, &c->head.hb_partial, (int64_t)head_bwd_blocks(NH) * C * DL));
    GAT_TRY(dalloc(c, &c->head.loss_partial, head_blocks(NH)));
    GAT_TRY(dalloc(c, &c->head.correct_partial, head_blocks(NH)));
    GAT_TRY(dalloc(c, &c->head.loss_out, 1));
    GAT_TRY(dalloc(c, &c->head.correct_out, 1));
    GAT_TRY(dalloc(c, &c->head.y, NH * C));
    if (res_route(c)) {                              // gatv2_abi.h "residual" / "layer normalisation"
        if (norm_on(c)) GAT_TRY(dalloc(c, &c->res.norm_partial, (int64_t)L * 2 * kResPartialRows * c->HDmax));
        if (bn_on(c)) {                              // gatv2_abi.h "batch normalisation" (the statistics themselves: gat_set_batch_norm)
            GAT_TRY(dalloc(c, &c->res.bn_partial, (int64_t)2 * kResPartialRows * c->HDmax));
            GAT_TRY(dalloc(c, &c->res.bn_sums, (int64_t)2 * c->HDmax));
        }
        GAT_TRY(dalloc(c, &c->res.G, N * c->HDmax));
        GAT_TRY(dalloc(c, &c->res.agg, N * c->HDmax));
        GAT_TRY(dalloc(c, &c->res.partial, (int64_t)L * kResPartialRows * c->HDmax));
        if (c->packed.group_cnt[GAT_PARAM_WRES]) {
            int64_t rg = 0;
            c->res.gw_off.assign((size_t)L, 0);
            for (int l = 0; l < L; ++l) {
                GAT_TRY(dalloc(c, &c->layers[l].R, N * c->layers[l].HD));
                c->res.gw_off[(size_t)l] = rg;
                rg += grad_w_scratch_floats(N, c->layers[l].F, c->layers[l].HD);
            }
            GAT_TRY(dalloc(c, &c->res.gw_scratch, std::max<int64_t>(rg, 1)));
        }
        GAT_TRY(ensure_drop_step(c));                // the forward's extended kernels read the step counter (nothing is dropped)
    }
    if (edge_feat_on(c)) {                           // gatv2_abi.h "edge features": PE per layer, one gPE, the slabs of gradWe
        const int64_t Ea = std::max<int64_t>(E, 1);  // (the edge kernels clamp their index prefetch to edge 0: one row always exists)
        int64_t wg = 0;
        c->ef.gw_off.assign((size_t)L, 0);
        for (int l = 0; l < L; ++l) {
            GAT_TRY(dalloc(c, &c->layers[l].PE, Ea * c->layers[l].HD));
            c->ef.gw_off[(size_t)l] = wg;
            wg += grad_w_scratch_floats(E, c->ef.dim, c->layers[l].HD);
        }
        GAT_TRY(dalloc(c, &c->ef.gPE, Ea * c->HDmax));
        GAT_TRY(dalloc(c, &c->ef.gw_scratch, std::max<int64_t>(wg, 1)));
        GAT_TRY(ensure_drop_step(c));                // both passes run extended kernels, which read the step counter
    }
    c->buffers_ready = true;
    GAT_TRY(ensure_drop_buffers(c));
    // The cliff of gatv2_abi.h "Limits": a layer whose SHAPE has wave-per-row kernels but whose gathered table is 4 GiB or
    // more drops to the generic float-atomic kernels.  Not an error (same results) — but never silent: the call that
    // completed the context returns 0 with this text in gat_last_error(), and gat_layer_path() reports it per layer.
    std::string slow;
    for (int l = 0; l < L; ++l) {
        const Layer& y = c->layers[l];
        if (!edge_fast_path(y.H, y.D, T) && edge_fast_path(y.H, y.D, 1)) slow += (slow.empty() ? "" : ", ") + std::to_string(l) + " (H*D = " + std::to_string(y.HD) + ")";
    }
    if (!slow.empty())
        set_error("warning: layer(s) " + slow + ": source table of " + std::to_string(T) + " rows is >= 4 GiB — these layers run on the generic "
                  "float-atomic kernels (several times slower); shard the graph by destination range to stay on the wave-per-row path (gat_layer_path reports it per layer)");
    return 0;
}

}  // namespace gat

using namespace gat;
extern "C" {

const char* gat_last_error(void) { return g_err.c_str(); }
int gat_abi_version(void) { return GAT_ABI_VERSION; }
int gat_switches(char* buf, int64_t cap) {
    if (!buf || cap <= 0) return fail(GAT_E_INVALID, "gat_switches: null buffer");
    std::string t = choices_text();
#ifdef GAT_EXPERIMENTS
    t = t.empty() ? "[experiment library]" : "[experiment library] " + t;
#endif
    if ((int64_t)t.size() + 1 > cap) return fail(GAT_E_INVALID, "gat_switches: buffer too small");
    memcpy(buf, t.c_str(), t.size() + 1);
    return 0;
}
int gat_device_count(int* count) {
    if (!count) return fail(GAT_E_INVALID, "null count");
    GAT_HIP(hipGetDeviceCount(count));
    return 0;
}
int gat_mem_info(size_t* free_bytes, size_t* total_bytes) {
    GAT_HIP(hipMemGetInfo(free_bytes, total_bytes));
    return 0;
}

int gat_create(const gat_config* cfg, gat_ctx** out) {
    if (!cfg || !out) return fail(GAT_E_INVALID, "gat_create: null argument");
    if (cfg->num_layers <= 0) return fail(GAT_E_INVALID, "Number of layers must be > 0");
    if (!cfg->heads || !cfg->outdims) return fail(GAT_E_INVALID, "--heads and --outdims are required (no defaults, E:954-955)");
    if (cfg->in_dim <= 0 || cfg->num_classes <= 0) return fail(GAT_E_INVALID, "in_dim and num_classes must be > 0");
    GAT_HIP(hipSetDevice(cfg->device));
    std::unique_ptr<gat_ctx> c(new gat_ctx());
    c->cfg = *cfg;
    c->heads.assign(cfg->heads, cfg->heads + cfg->num_layers);
    c->outdims.assign(cfg->outdims, cfg->outdims + cfg->num_layers);
    c->cfg.heads = c->heads.data();
    c->cfg.outdims = c->outdims.data();
    if (c->cfg.negative_slope == 0.0f) c->cfg.negative_slope = 0.01f;
    if (!(c->cfg.negative_slope > 0.0f && c->cfg.negative_slope <= 1.0f))
        return fail(GAT_E_INVALID, "negative_slope must be in (0, 1] (the kernels use LReLU(x) = max(x, slope*x))");
    c->layers.resize(cfg->num_layers);
    for (int l = 0; l < cfg->num_layers; ++l) {
        Layer& y = c->layers[l];
        y.H = c->heads[l]; y.D = c->outdims[l];
        if (y.H <= 0 || y.D <= 0) return fail(GAT_E_INVALID, "heads/outdims must be positive");
        y.HD = y.H * y.D;
        y.F = (l == 0) ? cfg->in_dim : c->layers[l - 1].HD;            // E:1115-1118
        c->HDmax = std::max(c->HDmax, y.HD);
        c->Hmax = std::max(c->Hmax, y.H);
    }
    if (cfg->storage_dtype != GAT_DTYPE_F32 && cfg->storage_dtype != GAT_DTYPE_BF16)
        return fail(GAT_E_INVALID, "storage_dtype must be GAT_DTYPE_F32 or GAT_DTYPE_BF16");
#ifdef GAT_EXPERIMENTS                               // the release library does not know the name: a stray variable cannot change results
    if (const char* d = getenv("GAT_DBG")) c->dbg = atoi(d);
#endif
    if (cfg->stream) { c->stream = (hipStream_t)cfg->stream; c->own_stream = false; }
    else { GAT_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)); c->own_stream = true; }
    GAT_TRY(relayout(c.get()));
    GAT_TRY(dalloc(c.get(), &c->packed.clip_scratch, kParamGroups));
    *out = c.release();
    return 0;
}

int gat_destroy(gat_ctx* c) {
    if (!c) return 0;
    (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->timing.pending) { (void)hipEventDestroy(p.e0); (void)hipEventDestroy(p.e1); }
    for (auto& p : c->timing.free) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
    c->xch.comm.reset();
    halo_free(&c->xch.halo);
    for (hipEvent_t e : c->xch.events) (void)hipEventDestroy(e);
    if (c->xch.stream) (void)hipStreamDestroy(c->xch.stream);
    for (hipEvent_t e : c->ov.fork) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ov.join) (void)hipEventDestroy(e);
    if (c->ov.stream) { (void)hipStreamSynchronize(c->ov.stream); (void)hipStreamDestroy(c->ov.stream); }
    if (c->replay.exec) (void)hipGraphExecDestroy(c->replay.exec);
    if (c->replay.graph) (void)hipGraphDestroy(c->replay.graph);
    if (c->replay.pinned_tail) (void)hipHostFree(c->replay.pinned_tail);
    for (void* p : c->owned) (void)hipFree(p);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return 0;
}

int gat_sync(gat_ctx* c) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

// ---- parameters --------------------------------------------------------------------------------------------
static int group_span(gat_ctx* c, int group, int64_t* off, int64_t* cnt) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (group < 0 || group >= kParamGroups) return fail(GAT_E_INVALID, "unknown parameter group");
    *off = c->packed.group_off[group]; *cnt = c->packed.group_cnt[group];
    return 0;
}
int gat_param_count(gat_ctx* c, int group, int64_t* count) {
    int64_t off;
    return group_span(c, group, &off, count);
}
static int copy_group(gat_ctx* c, bool grads, int group, float* host, int64_t count, bool to_device) {
    int64_t off, cnt;
    GAT_TRY(group_span(c, group, &off, &cnt));
    float* base = grads ? c->packed.grads : c->packed.params;
    c->packed.touched = true;
    if (count != cnt || (!host && cnt > 0)) return fail(GAT_E_INVALID, "parameter group size mismatch");
    if (cnt == 0) return 0;                          // a residual group that is off
    if (to_device) GAT_HIP(hipMemcpyAsync(base + off, host, cnt * sizeof(float), hipMemcpyHostToDevice, c->stream));
    else GAT_HIP(hipMemcpyAsync(host, base + off, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
int gat_params_set(gat_ctx* c, int group, const float* host, int64_t count) {
    return copy_group(c, false, group, const_cast<float*>(host), count, true);
}
int gat_params_get(gat_ctx* c, int group, float* host, int64_t count) {
    return copy_group(c, false, group, host, count, false);
}
int gat_grads_get(gat_ctx* c, int group, float* host, int64_t count) {
    return copy_group(c, true, group, host, count, false);
}
int gat_grads_set(gat_ctx* c, int group, const float* host, int64_t count) {
    return copy_group(c, true, group, const_cast<float*>(host), count, true);
}
int gat_grads_device(gat_ctx* c, void** d_ptr, int64_t* count) {
    if (!c || !d_ptr || !count) return fail(GAT_E_INVALID, "null argument");
    c->packed.touched = true;
    *d_ptr = c->packed.grads; *count = n_params(c);
    return 0;
}

int gat_grads_export(gat_ctx* c, void* d_dst, int64_t count) {
    if (!c || !d_dst) return fail(GAT_E_INVALID, "null argument");
    c->packed.touched = true;
    if (count != n_params(c)) return fail(GAT_E_INVALID, "packed gradient size mismatch");
    GAT_HIP(hipMemcpyAsync(d_dst, c->packed.grads, count * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}
int gat_result_export(gat_ctx* c, void* d_dst3) {
    if (!c || !d_dst3) return fail(GAT_E_INVALID, "null argument");
    if (!c->buffers_ready) return fail(GAT_E_STATE, "gat_result_export: no forward pass yet");
    return launch_pack_result(c->head.loss_out, c->head.correct_out, (float*)d_dst3, c->stream);
}
int gat_grads_import(gat_ctx* c, const void* d_src, int64_t count) {
    if (!c || !d_src) return fail(GAT_E_INVALID, "null argument");
    c->packed.touched = true;
    if (count != n_params(c)) return fail(GAT_E_INVALID, "packed gradient size mismatch");
    GAT_HIP(hipMemcpyAsync(c->packed.grads, d_src, count * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int gat_params_init(gat_ctx* c, uint64_t seed) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    c->packed.touched = true;
    // Same distribution as xavier_init_kernel_curand (E:205-242): U(-lim, lim] with lim = sqrt(6/(2F+D)) for the W rows
    // and a of a layer, sqrt(6/(C+D_L)) for W_o; own counter-based stream ON THE DEVICE, since the reference's cuRAND
    // XORWOW stream is seeded with time(NULL) (E:1305) and unreproducible.  Draw order: per layer W then a, then W_o.
    const uint64_t s0 = seed * 0x9E3779B97F4A7C15ull + 0x67617432ull;
    uint64_t draw = 0;
    for (int l = 0; l < c->cfg.num_layers; ++l) {
        const Layer& y = c->layers[l];
        const float lim = sqrtf(6.0f / (float)(2 * y.F + y.D));
        const int64_t nw = (int64_t)y.HD * 2 * y.F;
        GAT_TRY(launch_xavier_init(W_of(c, l), nw, s0, draw, lim, c->stream));
        draw += (uint64_t)nw;
        GAT_TRY(launch_xavier_init(a_of(c, l), y.HD, s0, draw, lim, c->stream));
        draw += (uint64_t)y.HD;
    }
    const float limo = sqrtf(6.0f / (float)(c->cfg.num_classes + head_width(c)));        // Wo [C][Dh] behind a hidden layer: the draws behind it shift
    GAT_TRY(launch_xavier_init(Wo_of(c), c->packed.group_cnt[GAT_PARAM_WO], s0, draw, limo, c->stream));
    draw += (uint64_t)c->packed.group_cnt[GAT_PARAM_WO];
    if (c->packed.group_cnt[GAT_PARAM_WRES]) {                                  // after every existing draw: W, a and Wo of a seed do not depend on the flag
        for (int l = 0; l < c->cfg.num_layers; ++l) {
            const Layer& y = c->layers[l];
            const int64_t nr = (int64_t)y.HD * y.F;
            GAT_TRY(launch_xavier_init(Wres_of(c, l), nr, s0, draw, sqrtf(6.0f / (float)(y.F + y.HD)), c->stream));
            draw += (uint64_t)nr;
        }
    }
    if (edge_feat_on(c)) {                                               // after Wres: every other group of a seed is unchanged
        for (int l = 0; l < c->cfg.num_layers; ++l) {
            const Layer& y = c->layers[l];
            const int64_t ne = (int64_t)y.HD * c->ef.dim;
            GAT_TRY(launch_xavier_init(We_of(c, l), ne, s0, draw, sqrtf(6.0f / (float)(c->ef.dim + y.HD)), c->stream));
            draw += (uint64_t)ne;
        }
    }
    if (hidden_on(c)) {                                                  // after every other draw; b1 = 0
        const int64_t n1 = c->packed.group_cnt[GAT_PARAM_HEAD_W];
        GAT_TRY(launch_xavier_init(W1_of(c), n1, s0, draw, sqrtf(6.0f / (float)(c->layers.back().D + c->hid.width)), c->stream));
        draw += (uint64_t)n1;
        GAT_HIP(hipMemsetAsync(b1_of(c), 0, (size_t)c->hid.width * sizeof(float), c->stream));
    }
    if (b_of(c, 0)) GAT_HIP(hipMemsetAsync(b_of(c, 0), 0, (size_t)c->packed.group_cnt[GAT_PARAM_B] * sizeof(float), c->stream));
    const std::vector<float> ones((size_t)c->packed.group_cnt[GAT_PARAM_LN_G], 1.0f);      // layer normalisation: gamma = 1, beta = 0, no draws
    if (!ones.empty()) {
        GAT_HIP(hipMemcpyAsync(lng_of(c, 0), ones.data(), ones.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        GAT_HIP(hipMemsetAsync(lnb_of(c, 0), 0, ones.size() * sizeof(float), c->stream));
    }
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

int gat_zero_grad(gat_ctx* c) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    Scope t(c, GAT_K_MISC);
    GAT_HIP(hipMemsetAsync(c->packed.grads, 0, (size_t)n_params(c) * sizeof(float), c->stream));
    return 0;
}
int gat_clip(gat_ctx* c, float threshold) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    Scope t(c, GAT_K_MISC);
    for (int k = 0; k < kParamGroups; ++k)          // every group by its own norm, like the reference's three (E:250-278); scratch slot k
        if (c->packed.group_cnt[k]) GAT_TRY(launch_clip(grad_of(c, k), c->packed.group_cnt[k], threshold, c->packed.clip_scratch + k, c->stream));
    return 0;
}
int gat_step_sgd(gat_ctx* c, float lr) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    Scope t(c, GAT_K_MISC);
    return launch_sgd(c->packed.params, c->packed.grads, lr, n_params(c), c->stream);
}
int gat_step_adam(gat_ctx* c, float lr, float b1, float b2, float eps, int32_t t_) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    if (!(b1 > 0.f && b1 < 1.f && b2 > 0.f && b2 < 1.f))
        return fail(GAT_E_INVALID, "For Adam optimizer, beta1 and beta2 must be in (0,1).");
    const int64_t np = n_params(c);
    if (!c->packed.adam_m) {
        GAT_TRY(dalloc(c, &c->packed.adam_m, np));
        GAT_TRY(dalloc(c, &c->packed.adam_v, np));
        GAT_HIP(hipMemsetAsync(c->packed.adam_m, 0, np * sizeof(float), c->stream));
        GAT_HIP(hipMemsetAsync(c->packed.adam_v, 0, np * sizeof(float), c->stream));
    }
    Scope t(c, GAT_K_MISC);
    return launch_adam(c->packed.params, c->packed.grads, c->packed.adam_m, c->packed.adam_v, lr, np, b1, b2, eps, t_, c->stream);
}

// ---- measurement -------------------------------------------------------------------------------------------------------
static const char* kNames[GAT_K_COUNT] = {"project_gemm", "edge_forward", "head_forward", "head_backward",
                                          "edge_backward", "gpl_sum", "grad_w_gemm", "grad_x_gemm", "misc",
                                          "exchange", "edge_last_fused"};
const char* gat_kernel_name(int k) { return (k >= 0 && k < GAT_K_COUNT) ? kNames[k] : "?"; }
int gat_kernel_stats(gat_ctx* c, int k, int64_t* launches, double* total_ms) {
    if (!c || k < 0 || k >= GAT_K_COUNT) return fail(GAT_E_INVALID, "bad argument");
    GAT_TRY(flush_events(c));
    if (launches) *launches = c->timing.launches[k];
    if (total_ms) *total_ms = c->timing.ms[k];
    return 0;
}
int gat_kernel_stats_reset(gat_ctx* c) {
    if (!c) return fail(GAT_E_INVALID, "null context");
    GAT_TRY(flush_events(c));
    for (int k = 0; k < GAT_K_COUNT; ++k) { c->timing.launches[k] = 0; c->timing.ms[k] = 0.0; }
    return 0;
}

}  // extern "C"
