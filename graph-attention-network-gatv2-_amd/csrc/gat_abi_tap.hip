// gat_abi_tap.hip — gat_tap: intermediate tensors of the last pass in the reference's layouts, for the parity tests.
#include "gat_ctx.h"
#include <cstring>

using namespace gat;
extern "C" {

static int d2h(gat_ctx* c, void* host, const void* dev, size_t bytes) {
    GAT_HIP(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}
int gat_tap(gat_ctx* c, int tensor, int32_t l, void* host, int64_t count) {
    GAT_TRY(check_layer(c, l));
    if (!host) return fail(GAT_E_INVALID, "null destination");
    const Layer& y = c->layers[l];
    const int64_t N = c->graph.n_rows, E = c->graph.n_edges;
    const bool last = (l == c->cfg.num_layers - 1);
    Scratch tmps;                                    // every temporary of the call: freed on return, after d2h's synchronisation
    auto need = [&](int64_t n) { return n == count ? 0 : fail(GAT_E_INVALID, "gat_tap: count mismatch"); };
    auto transposed = [&](const float* src, int64_t A_, int32_t B_, bool eh) -> int {
        if (!src) return fail(GAT_E_STATE, "gat_tap: tensor not kept (create the context with keep_taps=1)");
        float* tmp = nullptr;
        GAT_TRY(tmps.get(&tmp, A_ * B_));
        GAT_TRY(eh ? launch_transpose_eh_to_he(src, tmp, A_, B_, c->stream) : launch_transpose_nh_to_hn(src, tmp, A_, B_, c->stream));
        return d2h(c, host, tmp, (size_t)A_ * B_ * sizeof(float));
    };
    switch (tensor) {
        case GAT_TAP_SRC: GAT_TRY(need(E)); return d2h(c, host, c->graph.col_idx, E * sizeof(int32_t));
        case GAT_TAP_DST: {
            GAT_TRY(need(E));
            int32_t *s = nullptr, *d = nullptr;
            GAT_TRY(tmps.get(&s, E)); GAT_TRY(tmps.get(&d, E));
            GAT_TRY(launch_csr_to_coo(c->graph.row_ptr, c->graph.col_idx, s, d, N, E, 0, c->stream));
            return d2h(c, host, d, E * sizeof(int32_t));
        }
        case GAT_TAP_ALPHA: GAT_TRY(need(E * y.H)); return transposed(y.alpha, E, y.H, true);
        case GAT_TAP_MAX: {
            GAT_TRY(need(N * y.H));
            GAT_TRY(transposed(y.mstat, N, y.H, false));
            if (edge_fast_path(y.H, y.D, c->graph.n_table)) {          // kept in the log2 domain on the device
                float* f = static_cast<float*>(host);
                for (int64_t i = 0; i < N * y.H; ++i) f[i] = std::max(f[i] * 0.6931471805599453f, -1e9f);
            }
            return 0;
        }
        case GAT_TAP_GE: GAT_TRY(need(E * y.H)); return transposed(y.ge, E, y.H, true);
        case GAT_TAP_SCORE: GAT_TRY(need(E * y.H)); return transposed(y.score, E, y.H, true);
        case GAT_TAP_GALPHA: GAT_TRY(need(E * y.H)); return transposed(y.galpha, E, y.H, true);
        case GAT_TAP_GX:                              // what launch_grad_x of layer l left in layer l-1's g buffer
            if (l < 1) return fail(GAT_E_INVALID, "gat_tap: GAT_TAP_GX exists for layers >= 1 (E:1528 skips layer 0)");
            GAT_TRY(need(N * y.F));
            return d2h(c, host, c->layers[l - 1].g, N * y.F * sizeof(float));
        case GAT_TAP_SUM: GAT_TRY(need(N * y.H)); return transposed(y.zstat, N, y.H, false);
        case GAT_TAP_HPRE: GAT_TRY(need(N * y.HD)); return d2h(c, host, y.hpre, N * y.HD * sizeof(float));
        case GAT_TAP_HOUT: { const int64_t n = N * (last ? y.D : y.HD); GAT_TRY(need(n)); return d2h(c, host, y.hout, n * sizeof(float)); }
        case GAT_TAP_Y:                               // one row per graph with readout on, per pair with a pair head
            GAT_TRY(need(head_rows(c) * c->cfg.num_classes));
            if (!c->head.y_valid) GAT_TRY(gat_head_forward(c, nullptr, nullptr));     // after a fused head step: y = f(H_L, Wo), both still there
            return d2h(c, host, c->head.y, head_rows(c) * c->cfg.num_classes * sizeof(float));
        case GAT_TAP_POOLED:                          // what the last head forward (or head step) pooled
            if (!readout_on(c)) return fail(GAT_E_STATE, "gat_tap: GAT_TAP_POOLED needs gat_set_readout");
            if (!last) return fail(GAT_E_INVALID, "gat_tap: GAT_TAP_POOLED exists for the last layer only");
            GAT_TRY(need(c->readout.n_graphs * y.D));
            return d2h(c, host, c->readout.P, c->readout.n_graphs * y.D * sizeof(float));
        case GAT_TAP_PAIRED:                          // what the last head forward (or head step) gathered
            if (!pairs_on(c)) return fail(GAT_E_STATE, "gat_tap: GAT_TAP_PAIRED needs gat_set_pairs");
            if (!last) return fail(GAT_E_INVALID, "gat_tap: GAT_TAP_PAIRED exists for the last layer only");
            GAT_TRY(need(c->pairs.n_pairs * y.D));
            return d2h(c, host, c->pairs.Q, c->pairs.n_pairs * y.D * sizeof(float));
        case GAT_TAP_HEAD_HIDDEN:                     // Z1 of the last head forward (or head step): what the head reads
            if (!hidden_on(c)) return fail(GAT_E_STATE, "gat_tap: GAT_TAP_HEAD_HIDDEN needs gat_set_head_hidden");
            if (!last) return fail(GAT_E_INVALID, "gat_tap: GAT_TAP_HEAD_HIDDEN exists for the last layer only");
            GAT_TRY(need(head_rows(c) * c->hid.width));
            return d2h(c, host, c->hid.Z1, head_rows(c) * c->hid.width * sizeof(float));
        case GAT_TAP_G: {
            GAT_TRY(need(N * y.HD));
            if (norm_layer(c, l)) {                     // dL/dh_pre through the normalisation: the backward kernel's row function again, on the
                NormBwdArgs n{};                        // layer's stored output gradient and h_pre (no column sums, no aggregate)
                n.r.hpre = y.hpre; n.r.g = y.g; n.r.gh = (last && c->bwd.gH != nullptr) ? c->bwd.gH : nullptr;
                n.r.n_rows = N; n.r.H = y.H; n.r.D = y.D; n.r.gh_stride = c->bwd.gh_stride; n.r.slope = c->cfg.negative_slope;
                n.r.blocks = norm_backward_blocks(N, y.HD);
                n.gamma = lng_of(c, l); n.beta = lnb_of(c, l); n.eps = c->res.norm_eps;
                float* tmp = nullptr;
                GAT_TRY(tmps.get(&tmp, N * y.HD));
                n.r.G = tmp;
                GAT_TRY(launch_norm_backward(n, c->stream));
                return d2h(c, host, tmp, (size_t)(N * y.HD) * sizeof(float));
            }
            if (bn_layer(c, l)) {                       // through the batch normalisation: the two backward launches again, into scratch (no
                BnBwdArgs n{};                          // gradient is added to, no aggregate, no column sums of G)
                n.u = y.hpre; n.g = y.g; n.gh = (last && c->bwd.gH != nullptr) ? c->bwd.gH : nullptr; n.gamma = lng_of(c, l); n.beta = lnb_of(c, l);
                n.stats = bn_stats_now(c, l);
                n.n_rows = N; n.gh_stride = c->bwd.gh_stride; n.H = y.H; n.D = y.D; n.training = c->drop.training ? 1 : 0; n.slope = c->cfg.negative_slope;
                n.blocks = batch_norm_blocks(N, y.HD);
                float* tmp = nullptr;
                GAT_TRY(tmps.get(&tmp, N * y.HD));
                GAT_TRY(tmps.get(&n.part_s1, (int64_t)n.blocks * y.HD)); GAT_TRY(tmps.get(&n.part_s2, (int64_t)n.blocks * y.HD)); GAT_TRY(tmps.get(&n.sums, 2 * y.HD));
                n.G = tmp;
                GAT_TRY(launch_batch_norm_backward(n, nullptr, nullptr, c->stream));
                return d2h(c, host, tmp, (size_t)(N * y.HD) * sizeof(float));
            }
            if (last && c->bwd.gH) {                        // formed on the fly by the kernels: same expression, same order
                std::vector<float> hp((size_t)(N * y.HD)), gh((size_t)(N * c->bwd.gh_stride));
                GAT_TRY(d2h(c, hp.data(), y.hpre, hp.size() * sizeof(float)));
                GAT_TRY(d2h(c, gh.data(), c->bwd.gH, gh.size() * sizeof(float)));
                float* out = static_cast<float*>(host);
                const float inv_heads = 1.0f / (float)y.H;
                for (int64_t i = 0; i < N * y.HD; ++i)
                    out[i] = gh[(size_t)((i / y.HD) * c->bwd.gh_stride + i % y.D)] * (hp[(size_t)i] > 0.f ? 1.0f : c->cfg.negative_slope) * inv_heads;
                return 0;
            }
            GAT_TRY(d2h(c, host, y.g, N * y.HD * sizeof(float)));
            if (l < c->cfg.num_layers - 1) {         // stored without the LReLU'(h_pre) factor (EdgeBwdArgs::g_raw)
                std::vector<float> hp((size_t)(N * y.HD));
                GAT_TRY(d2h(c, hp.data(), y.hpre, hp.size() * sizeof(float)));
                float* gh = static_cast<float*>(host);
                for (size_t i = 0; i < hp.size(); ++i) gh[i] *= hp[i] > 0.f ? 1.0f : c->cfg.negative_slope;
            }
            return 0;
        }
        case GAT_TAP_PL: {
            GAT_TRY(need(c->graph.n_table * y.HD));
            if (!bf16(c)) return d2h(c, host, y.PL, c->graph.n_table * y.HD * sizeof(float));
            std::vector<uint16_t> hb((size_t)(c->graph.n_table * y.HD));          // bf16 rows -> fp32 for the caller
            GAT_TRY(d2h(c, hb.data(), y.PL, hb.size() * sizeof(uint16_t)));
            for (size_t i = 0; i < hb.size(); ++i) {
                const uint32_t u = (uint32_t)hb[i] << 16;
                memcpy(static_cast<float*>(host) + i, &u, sizeof(float));
            }
            return 0;
        }
        case GAT_TAP_PR: GAT_TRY(need(N * y.HD)); return d2h(c, host, y.PR, N * y.HD * sizeof(float));
        case GAT_TAP_ATTN_KEEP:
        case GAT_TAP_FEAT_KEEP: {                      // the masks for the step the counter holds, from the kernels' own device functions
            const bool attn = tensor == GAT_TAP_ATTN_KEEP;
            const int64_t n = attn ? E * y.H : N * y.F;
            GAT_TRY(need(n));
            if (!c->drop.step) return fail(GAT_E_STATE, "gat_tap: dropout was never set (gat_set_dropout)");
            float* tmp = nullptr;
            GAT_TRY(tmps.get(&tmp, n));
            const DropArgs d = drop_args(c, l, attn ? kDropAttn : kDropFeat, true);
            GAT_TRY(attn ? launch_attn_keep_tap(c->graph.row_ptr, N, E, y.H, d, tmp, c->stream) : launch_feat_keep_tap(N, y.F, d, tmp, c->stream));
            return d2h(c, host, tmp, (size_t)n * sizeof(float));
        }
        case GAT_TAP_EDGE_KEEP: {                      // DropEdge's mask for the step the counter holds (0 / 1 per CSR edge)
            GAT_TRY(need(E));
            if (!c->drop.step) return fail(GAT_E_STATE, "gat_tap: DropEdge was never set (gat_set_dropedge)");
            float* tmp = nullptr;
            GAT_TRY(tmps.get(&tmp, E));
            const DropArgs d = drop_args(c, l, kDropAttn, true);
            GAT_TRY(launch_edge_keep_tap(c->graph.row_ptr, c->graph.col_idx, N, E, d, tmp, c->stream));
            return d2h(c, host, tmp, (size_t)E * sizeof(float));
        }
        default: return fail(GAT_E_INVALID, "gat_tap: unknown tensor id");
    }
}

}  // extern "C"
