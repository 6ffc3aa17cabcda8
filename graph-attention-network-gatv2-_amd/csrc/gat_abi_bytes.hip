// gat_abi_bytes.hip — the byte models a step is measured against (pure host arithmetic).
#include "gat_ctx.h"

using namespace gat;
extern "C" {

// what every model ends with: the per-class figures and their sum, each where the caller asked for it
static int report_bytes(const double* k, double* bytes_step, double* per_kernel) {
    double tot = 0;
    for (int i = 0; i < GAT_K_COUNT; ++i) { tot += k[i]; if (per_kernel) per_kernel[i] = k[i]; }
    if (bytes_step) *bytes_step = tot;
    return 0;
}
// SURVEY §8(d), literally: every tensor the restructured algorithm must move once per step, with
// b = storage bytes (4 fp32 / 2 bf16) on every float term — the single figure `roofline.achieved` is quoted
// against.  It is a property of the WORKLOAD, not of this implementation: it counts the alpha write/read
// (E*H per direction) although the training path recomputes alpha from the softmax stats instead, it counts
// the gPL scatter once although the no-atomics scatter stores and re-reads a per-edge record, and in bf16 mode
// it prices PR / h_pre / g at 2 bytes although they are kept in fp32 here.  Pure host arithmetic (no device).
int gat_algorithmic_bytes_shape(const gat_config* cfg, int64_t n_rows, int64_t n_edges, int64_t n_table,
                                int32_t replicated_input, double* bytes_step, double* per_kernel) {
    if (!cfg || !cfg->heads || !cfg->outdims || cfg->num_layers <= 0) return fail(GAT_E_INVALID, "gat_algorithmic_bytes_shape: bad config");
    double k[GAT_K_COUNT] = {0};
    const double N = (double)n_rows, E = (double)n_edges;
    const double b = cfg->storage_dtype == GAT_DTYPE_BF16 ? 2.0 : 4.0;
    const int L = cfg->num_layers;
    for (int l = 0; l < L; ++l) {
        const double H = cfg->heads[l], D = cfg->outdims[l], HD = H * D;
        const double F = l == 0 ? (double)cfg->in_dim : (double)cfg->heads[l - 1] * cfg->outdims[l - 1];
        const double Dout = (l == L - 1) ? D : HD;
        const double NL = (l == 0 && replicated_input) ? (double)n_table : N;     // rows of the W_left half (shards)
        k[GAT_K_PROJECT] += b * (std::max(N, NL) * F + 2 * HD * F + (N + NL) * HD);          // X, W read; PL + PR written
        k[GAT_K_EDGE_FWD] += 4 * (N + 1) + 4 * E + b * (E * HD + N * HD + E * H + N * HD + N * Dout);   // PL[src], PR, alpha, h_pre, H
        // g, PL[src], PR, alpha, gPR in the destination-major pass; the gPL scatter (counted once, E*HD) belongs to the
        // source-major pass that performs it here (it gathers g[dst] per edge and sums per source)
        k[GAT_K_EDGE_BWD] += 4 * (N + 1) + 4 * E + b * (N * HD + E * HD + N * HD + E * H + N * HD);
        k[GAT_K_GPL_SUM] += b * E * HD;
        k[GAT_K_GRAD_W] += b * ((N + NL) * HD + std::max(N, NL) * F + 2 * HD * F);            // gPL + gPR re-read, X, grad_W
        if (l > 0) k[GAT_K_GRAD_X] += b * (2 * N * HD + 2 * N * F);                            // gPL + gPR, gX write, h_pre_{l-1}
    }
    const double head = 2.0 * 4.0 * N * ((double)cfg->outdims[L - 1] + 2.0 * cfg->num_classes + 2.0);
    k[GAT_K_HEAD_FWD] = head / 2; k[GAT_K_HEAD_BWD] = head / 2;
    return report_bytes(k, bytes_step, per_kernel);
}
// The same model with every RANDOM row access priced at what the memory system can serve: the fabric moves 128-byte requests
// (TCC_EA0_RDREQ_128B == TCC_EA0_RDREQ in every PMC pass of this build), so a gathered or scattered row of b*H*D bytes costs
// ceil(b*H*D / 128) * 128.  Identical to SURVEY 8d's figure wherever a row is a multiple of 128 B (fp32 at H*D = 64: 256 B);
// for bf16 rows at H*D = 32 (BASELINE config 5: 64-byte rows) the three per-edge row terms double.  Sequential streams
// (indices, attention coefficients, node-major rows) are unchanged.
int gat_request_bytes_shape(const gat_config* cfg, int64_t n_rows, int64_t n_edges, int64_t n_table,
                            int32_t replicated_input, double* bytes_step, double* per_kernel) {
    double k[GAT_K_COUNT] = {0};
    GAT_TRY(gat_algorithmic_bytes_shape(cfg, n_rows, n_edges, n_table, replicated_input, nullptr, k));
    const double E = (double)n_edges, b = cfg->storage_dtype == GAT_DTYPE_BF16 ? 2.0 : 4.0;
    for (int l = 0; l < cfg->num_layers; ++l) {
        const double row = b * (double)cfg->heads[l] * cfg->outdims[l];
        const double extra = E * (std::ceil(row / 128.0) * 128.0 - row);
        k[GAT_K_EDGE_FWD] += extra; k[GAT_K_EDGE_BWD] += extra; k[GAT_K_GPL_SUM] += extra;      // PL[src] twice, the gPL scatter once
    }
    return report_bytes(k, bytes_step, per_kernel);
}
// edge features (gatv2_abi.h "edge features"): what the dense per-edge term adds, fp32 throughout — EA and We read and PE written by the
// projection, PE read by the edge forward, PE read and gPE written by the edge backward, gPE, EA and gradWe in the dense term
static void edge_feature_bytes(const gat_ctx* c, double* k) {
    if (!edge_feat_on(c)) return;
    const double E = (double)c->graph.n_edges, Fe = c->ef.dim;
    for (int l = 0; l < c->cfg.num_layers; ++l) {
        const double HD = c->layers[l].HD;
        k[GAT_K_PROJECT] += 4.0 * (E * Fe + HD * Fe + E * HD);
        k[GAT_K_EDGE_FWD] += 4.0 * E * HD;
        k[GAT_K_EDGE_BWD] += 4.0 * 2 * E * HD;
        k[GAT_K_GRAD_W] += 4.0 * (E * HD + E * Fe + HD * Fe);
    }
}
// the figure of a context whose head has one row per node
static int algorithmic_bytes_nodes(gat_ctx* c, double* bytes_step, double* per_kernel) {
    if (edge_feat_on(c) && !res_route(c)) {
        double k[GAT_K_COUNT] = {0};
        GAT_TRY(gat_algorithmic_bytes_shape(&c->cfg, c->graph.n_rows, c->graph.n_edges, c->graph.n_table, c->in.Xtab != nullptr, nullptr, k));
        edge_feature_bytes(c, k);
        return report_bytes(k, bytes_step, per_kernel);
    }
    if (res_route(c)) {
        // residual (gatv2_abi.h "residual"): the N-sized traffic it adds, fp32 throughout — R written, read by the edge forward and by
        // the N-sized backward kernel; that kernel's h_pre and g read, G and agg written; G, x' and Wres in the two dense terms
        double k[GAT_K_COUNT] = {0};
        GAT_TRY(gat_algorithmic_bytes_shape(&c->cfg, c->graph.n_rows, c->graph.n_edges, c->graph.n_table, c->in.Xtab != nullptr, nullptr, k));
        const double N = (double)c->graph.n_rows;
        for (int l = 0; l < c->cfg.num_layers; ++l) {
            const double HD = c->layers[l].HD, F = c->layers[l].F;
            const bool lin = (c->res.flags & GAT_RES_LINEAR) != 0;
            // a norm context without residual flags runs the same N-sized kernel (h_pre + g read, G + agg written); a normalised layer
            // adds gamma and beta, read by the forward epilogue and by the backward kernel: 2*HD floats per pass
            k[GAT_K_MISC] += 4.0 * N * HD * (lin ? 5 : 4);
            if (norm_layer(c, l)) k[GAT_K_MISC] += 4.0 * 2 * HD * 2;       // (both passes priced under misc)
            // a batch-normalised layer (gatv2_abi.h "batch normalisation"): forward u read twice and hout written; backward u and g read
            // twice, G and agg written, in place of the route's four tensors (R, with GAT_RES_LINEAR, is read once as before)
            if (bn_layer(c, l)) k[GAT_K_MISC] += 4.0 * N * HD * (3 + 2);
            if (!lin) continue;
            k[GAT_K_PROJECT] += 4.0 * (N * HD + HD * F + N * F);
            k[GAT_K_EDGE_FWD] += 4.0 * N * HD;
            k[GAT_K_GRAD_W] += 4.0 * (N * HD + N * F + HD * F);
            if (l > 0) k[GAT_K_GRAD_X] += 4.0 * (N * HD + 2 * N * F + HD * F);
        }
        edge_feature_bytes(c, k);
        return report_bytes(k, bytes_step, per_kernel);
    }
    GAT_TRY(gat_algorithmic_bytes_shape(&c->cfg, c->graph.n_rows, c->graph.n_edges, c->graph.n_table, c->in.Xtab != nullptr, bytes_step, per_kernel));
    if (per_kernel && c->buffers_ready && fused_last(c)) {
        // gat_step runs the last layer's forward and backward edge passes (and forms gH) in ONE kernel class: its share of
        // the SAME byte model moves there (the step total is unchanged; the head class keeps its bytes: head_step still runs)
        const int L = c->cfg.num_layers;
        const double N = (double)c->graph.n_rows, E = (double)c->graph.n_edges, H = c->layers[L - 1].H, D = c->layers[L - 1].D, HD = H * D;
        const double fwd = 4 * (N + 1) + 4 * E + 4.0 * (E * HD + N * HD + E * H + N * HD + N * D);
        const double bwd = 4 * (N + 1) + 4 * E + 4.0 * (N * HD + E * HD + N * HD + E * H + N * HD);
        per_kernel[GAT_K_EDGE_FWD] -= fwd; per_kernel[GAT_K_EDGE_BWD] -= bwd; per_kernel[GAT_K_EDGE_FUSED] += fwd + bwd;
    }
    return 0;
}
static int algorithmic_bytes_softmax(gat_ctx* c, double* bytes_step, double* per_kernel) {
    if (pairs_on(c)) {
        // pair head (gatv2_abi.h "pair head"): the head classes priced with P rows; the gather reads the indices and two rows per pair and
        // writes Q, the scatter reads an 8-byte entry and a gQ row (MUL: and an X row) per incidence and writes every gH row (under misc, fp32)
        double k[GAT_K_COUNT] = {0};
        GAT_TRY(algorithmic_bytes_nodes(c, nullptr, k));
        const double N = (double)c->graph.n_rows, P = (double)c->pairs.n_pairs, DL = c->layers.back().D;
        const double head = 2.0 * 4.0 * P * (DL + 2.0 * c->cfg.num_classes + 2.0);
        k[GAT_K_HEAD_FWD] = head / 2; k[GAT_K_HEAD_BWD] = head / 2;
        k[GAT_K_MISC] += 4.0 * (2 * P + 2 * P * DL + P * DL) + 4.0 * (4 * P + 2 * P * DL + (c->pairs.mode == GAT_PAIR_MUL ? 2 * P * DL : 0.0) + N * DL);
        return report_bytes(k, bytes_step, per_kernel);
    }
    if (!readout_on(c)) return algorithmic_bytes_nodes(c, bytes_step, per_kernel);
    // readout (gatv2_abi.h "graph-level readout"): the head classes priced with G rows; the pool reads N*DL and writes G*DL, the un-pool
    // reads G*DL and writes N*DL (under misc, fp32)
    double k[GAT_K_COUNT] = {0};
    GAT_TRY(algorithmic_bytes_nodes(c, nullptr, k));
    const double N = (double)c->graph.n_rows, G = (double)c->readout.n_graphs, DL = c->layers.back().D;
    const double head = 2.0 * 4.0 * G * (DL + 2.0 * c->cfg.num_classes + 2.0);
    k[GAT_K_HEAD_FWD] = head / 2; k[GAT_K_HEAD_BWD] = head / 2;
    k[GAT_K_MISC] += 4.0 * (N * DL + G * DL) + 4.0 * (G * DL + N * DL);
    return report_bytes(k, bytes_step, per_kernel);
}
static int algorithmic_bytes_modes(gat_ctx* c, double* bytes_step, double* per_kernel);
int gat_algorithmic_bytes(gat_ctx* c, double* bytes_step, double* per_kernel) {
    if (!c || !c->graph.have) return fail(GAT_E_STATE, "graph not set");
    if (!hidden_on(c)) return algorithmic_bytes_modes(c, bytes_step, per_kernel);
    // hidden layer (gatv2_abi.h "hidden layer"): the head classes read rows of Dh floats where they read D_last; the stage adds, fp32:
    // forward Xin, W1, A written, A read and Z1 written; backward gZ1 and Z1 read and gA written, then gA, Xin and gradW1, then gA, W1 and gXin
    double k[GAT_K_COUNT] = {0};
    GAT_TRY(algorithmic_bytes_modes(c, nullptr, k));
    const double R = (double)head_rows(c), DL = c->layers.back().D, Dh = c->hid.width;
    k[GAT_K_HEAD_FWD] += 4.0 * R * (Dh - DL) + 4.0 * (R * DL + Dh * DL + 3 * R * Dh);
    k[GAT_K_HEAD_BWD] += 4.0 * R * (Dh - DL) + 4.0 * (3 * R * Dh + (R * Dh + R * DL + Dh * DL) + (R * Dh + Dh * DL + R * DL));
    return report_bytes(k, bytes_step, per_kernel);
}
static int algorithmic_bytes_modes(gat_ctx* c, double* bytes_step, double* per_kernel) {
    if (c->sup.loss_mode == 0) return algorithmic_bytes_softmax(c, bytes_step, per_kernel);
    // loss modes (gatv2_abi.h "loss modes of the output head"): each head class reads 4*rows*C bytes of targets where the softmax head
    // reads 4*rows of labels
    double k[GAT_K_COUNT] = {0};
    GAT_TRY(algorithmic_bytes_softmax(c, nullptr, k));
    const double extra = 4.0 * (double)head_rows(c) * (c->cfg.num_classes - 1.0);
    k[GAT_K_HEAD_FWD] += extra; k[GAT_K_HEAD_BWD] += extra;
    return report_bytes(k, bytes_step, per_kernel);
}

}  // extern "C"
