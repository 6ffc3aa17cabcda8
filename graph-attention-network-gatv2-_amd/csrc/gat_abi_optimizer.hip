// gat_abi_optimizer.hip — the optimizer on the device (gatv2_abi.h "optimizer"): configuration and its refusals, the state of a kind over
// the packed layout, the device scalars t and lr, the checkpoint calls.  The kernels are in gat_optimizer.hip; gat_train_step, which runs
// the step in front of optimizer_launch, is in gat_abi_step.hip.
#include "gat_ctx.h"

static_assert(kParamGroups == gat::kOptGroups, "the optimizer's block table covers every GAT_PARAM_* group");

namespace gat {

static bool adam_kind(int32_t kind) { return kind == GAT_OPT_ADAM || kind == GAT_OPT_ADAMW; }
static bool nonneg_finite(float v) { return std::isfinite(v) && v >= 0.f; }

static int check_config(const gat_optimizer_config* q) {
    if (!q) return fail(GAT_E_INVALID, "gat_set_optimizer: null config");
    if (q->kind != GAT_OPT_SGD && q->kind != GAT_OPT_ADAM && q->kind != GAT_OPT_ADAMW)
        return fail(GAT_E_INVALID, "gat_set_optimizer: kind must be GAT_OPT_SGD, GAT_OPT_ADAM or GAT_OPT_ADAMW");
    if (q->flags & ~GAT_OPT_NESTEROV) return fail(GAT_E_INVALID, "gat_set_optimizer: unknown flag bits");
    if (q->clip_mode != GAT_CLIP_NONE && q->clip_mode != GAT_CLIP_PER_GROUP && q->clip_mode != GAT_CLIP_GLOBAL)
        return fail(GAT_E_INVALID, "gat_set_optimizer: clip_mode must be GAT_CLIP_NONE, GAT_CLIP_PER_GROUP or GAT_CLIP_GLOBAL");
    if (!nonneg_finite(q->lr)) return fail(GAT_E_INVALID, "gat_set_optimizer: lr must be finite and >= 0");
    if (!nonneg_finite(q->weight_decay)) return fail(GAT_E_INVALID, "gat_set_optimizer: weight_decay must be finite and >= 0");
    if (!nonneg_finite(q->eps)) return fail(GAT_E_INVALID, "gat_set_optimizer: eps must be finite and >= 0");
    if (!nonneg_finite(q->momentum) || q->momentum >= 1.f) return fail(GAT_E_INVALID, "gat_set_optimizer: momentum must be in [0, 1)");
    if ((q->flags & GAT_OPT_NESTEROV) && adam_kind(q->kind)) return fail(GAT_E_INVALID, "gat_set_optimizer: GAT_OPT_NESTEROV is an SGD flag");
    if ((q->flags & GAT_OPT_NESTEROV) && !(q->momentum > 0.f)) return fail(GAT_E_INVALID, "gat_set_optimizer: GAT_OPT_NESTEROV needs momentum > 0");
    if (adam_kind(q->kind) && !(q->beta1 > 0.f && q->beta1 < 1.f && q->beta2 > 0.f && q->beta2 < 1.f))
        return fail(GAT_E_INVALID, "gat_set_optimizer: beta1 and beta2 must be in (0, 1)");
    if (q->clip_mode != GAT_CLIP_NONE && !(std::isfinite(q->clip_threshold) && q->clip_threshold > 0.f))
        return fail(GAT_E_INVALID, "gat_set_optimizer: a clip mode other than GAT_CLIP_NONE needs a finite clip_threshold > 0");
    if (q->decay_groups != 0xFFFFFFFFu && (q->decay_groups >> kParamGroups) != 0)
        return fail(GAT_E_INVALID, "gat_set_optimizer: decay_groups names a group at or above 10 (0xFFFFFFFF = all groups)");
    return 0;
}
static int zeroed(gat_ctx* c, float** p, int64_t n) {
    GAT_TRY(dalloc(c, p, n));
    GAT_HIP(hipMemsetAsync(*p, 0, (size_t)n * sizeof(float), c->stream));
    return 0;
}
static void free_state(gat_ctx* c) {
    dfree(c, c->opt.m); dfree(c, c->opt.v); dfree(c, c->opt.buf);
    c->opt.m = c->opt.v = c->opt.buf = nullptr;
}
int optimizer_launch(gat_ctx* c) {
    const gat_optimizer_config& q = c->opt.cfg;
    OptArgs a;
    a.p = c->packed.params; a.g = c->packed.grads;
    if (adam_kind(q.kind)) { a.s0 = c->opt.m; a.s1 = c->opt.v; }
    else a.s0 = q.momentum > 0.f ? c->opt.buf : nullptr;
    a.table = c->opt.table; a.n_blocks = c->opt.n_blocks;
    std::copy(c->opt.group_block0, c->opt.group_block0 + kOptGroups + 1, a.group_block0);
    a.partial = c->opt.partial; a.t = c->opt.t; a.lr = c->opt.lr; a.norms = c->opt.norms;
    a.kind = q.kind; a.flags = q.flags; a.clip_mode = q.clip_mode;
    a.momentum = q.momentum; a.beta1 = q.beta1; a.beta2 = q.beta2; a.eps = q.eps; a.weight_decay = q.weight_decay;
    a.clip_threshold = q.clip_threshold; a.decay_groups = q.decay_groups;
    Scope t(c, GAT_K_MISC);
    return launch_opt_step(a, c->stream);
}
static int check_have(gat_ctx* c, const char* who) {
    if (!c) return fail(GAT_E_INVALID, std::string(who) + ": null context");
    if (!c->opt.have) return fail(GAT_E_STATE, std::string(who) + ": call gat_set_optimizer first");
    return 0;
}
// the state buffer `which` names under the current configuration, or null
static float* state_of(gat_ctx* c, int which) {
    if (which == GAT_OPT_STATE_M && adam_kind(c->opt.cfg.kind)) return c->opt.m;
    if (which == GAT_OPT_STATE_V && adam_kind(c->opt.cfg.kind)) return c->opt.v;
    if (which == GAT_OPT_STATE_MOMENTUM && c->opt.cfg.kind == GAT_OPT_SGD && c->opt.cfg.momentum > 0.f) return c->opt.buf;
    return nullptr;
}
static int copy_state(gat_ctx* c, const char* who, int which, int group, float* host, int64_t count, bool to_device) {
    GAT_TRY(check_have(c, who));
    float* base = state_of(c, which);
    if (!base) return fail(GAT_E_INVALID, std::string(who) + ": the optimizer's configuration has no such state (M, V: the Adam kinds; MOMENTUM: SGD with momentum > 0)");
    if (group < 0 || group >= kParamGroups) return fail(GAT_E_INVALID, "unknown parameter group");
    const int64_t off = c->packed.group_off[group], cnt = c->packed.group_cnt[group];
    if (count != cnt || (!host && cnt > 0)) return fail(GAT_E_INVALID, "parameter group size mismatch");
    if (cnt == 0) return 0;
    if (to_device) GAT_HIP(hipMemcpyAsync(base + off, host, cnt * sizeof(float), hipMemcpyHostToDevice, c->stream));
    else GAT_HIP(hipMemcpyAsync(host, base + off, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    return 0;
}

}  // namespace gat

using namespace gat;
extern "C" {

int gat_set_optimizer(gat_ctx* c, const gat_optimizer_config* q) {
    if (!c) return fail(GAT_E_INVALID, "gat_set_optimizer: null context");
    GAT_TRY(check_config(q));
    c->packed.touched = true;                        // the packed sizes are final: the state and the block table are laid over them
    graph_drop(c);                                   // the hyper-parameters other than lr are kernel arguments
    const int64_t np = n_params(c);
    if (!c->opt.t) {                                 // first call: the scalars, the record, the block table
        std::vector<OptBlock> table;
        opt_build_table(c->packed.group_off, c->packed.group_cnt, &table, c->opt.group_block0);
        c->opt.n_blocks = (int32_t)table.size();
        GAT_TRY(dalloc(c, &c->opt.t, 1));
        GAT_TRY(dalloc(c, &c->opt.lr, 1));
        GAT_TRY(zeroed(c, &c->opt.norms, kOptGroups + 1));
        GAT_TRY(zeroed(c, &c->opt.partial, std::max<int64_t>(c->opt.n_blocks, 1)));
        GAT_TRY(dalloc(c, &c->opt.table, std::max<int64_t>(c->opt.n_blocks, 1)));
        GAT_HIP(hipMemcpyAsync(c->opt.table, table.data(), table.size() * sizeof(OptBlock), hipMemcpyHostToDevice, c->stream));
        GAT_HIP(hipMemsetAsync(c->opt.t, 0, sizeof(unsigned long long), c->stream));
        GAT_HIP(hipStreamSynchronize(c->stream));     // `table` leaves scope
    }
    if (!c->opt.have || c->opt.cfg.kind != q->kind) {          // another kind: its own zeroed state, t = 0
        GAT_HIP(hipStreamSynchronize(c->stream));     // nothing in flight reads what is freed
        free_state(c);
        if (adam_kind(q->kind)) { GAT_TRY(zeroed(c, &c->opt.m, np)); GAT_TRY(zeroed(c, &c->opt.v, np)); }
        GAT_TRY(launch_opt_set_count(c->opt.t, 0, c->stream));
    }
    if (q->kind == GAT_OPT_SGD && q->momentum > 0.f && !c->opt.buf) GAT_TRY(zeroed(c, &c->opt.buf, np));
    c->opt.cfg = *q;
    c->opt.have = true;
    return launch_opt_set_lr(c->opt.lr, q->lr, c->stream);
}
int gat_optimizer_step(gat_ctx* c) {
    GAT_TRY(check_have(c, "gat_optimizer_step"));
    return optimizer_launch(c);
}
int gat_set_lr(gat_ctx* c, float lr) {
    GAT_TRY(check_have(c, "gat_set_lr"));
    if (!nonneg_finite(lr)) return fail(GAT_E_INVALID, "gat_set_lr: lr must be finite and >= 0");
    c->opt.cfg.lr = lr;
    return launch_opt_set_lr(c->opt.lr, lr, c->stream);
}
int gat_optimizer_info(gat_ctx* c, gat_optimizer_config* cfg, int64_t* t, float* lr, float* global_norm, float* group_norms) {
    GAT_TRY(check_have(c, "gat_optimizer_info"));
    unsigned long long ht = 0; float hlr = 0.f, hn[kOptGroups + 1] = {0.f};
    GAT_HIP(hipMemcpyAsync(&ht, c->opt.t, sizeof(ht), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipMemcpyAsync(&hlr, c->opt.lr, sizeof(hlr), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipMemcpyAsync(hn, c->opt.norms, sizeof(hn), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(hipStreamSynchronize(c->stream));
    if (cfg) { *cfg = c->opt.cfg; cfg->lr = hlr; }
    if (t) *t = (int64_t)ht;
    if (lr) *lr = hlr;
    if (global_norm) *global_norm = c->opt.cfg.clip_mode == GAT_CLIP_GLOBAL ? hn[kOptGroups] : 0.f;
    if (group_norms) std::copy(hn, hn + kOptGroups, group_norms);
    return 0;
}
int gat_optimizer_state_get(gat_ctx* c, int which, int group, float* host, int64_t count) {
    return copy_state(c, "gat_optimizer_state_get", which, group, host, count, false);
}
int gat_optimizer_state_set(gat_ctx* c, int which, int group, const float* host, int64_t count) {
    return copy_state(c, "gat_optimizer_state_set", which, group, const_cast<float*>(host), count, true);
}
int gat_optimizer_step_count_set(gat_ctx* c, int64_t t) {
    GAT_TRY(check_have(c, "gat_optimizer_step_count_set"));
    if (t < 0) return fail(GAT_E_INVALID, "gat_optimizer_step_count_set: t must be >= 0");
    return launch_opt_set_count(c->opt.t, (uint64_t)t, c->stream);
}

}  // extern "C"
