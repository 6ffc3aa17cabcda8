// pick_sweep.hip — are the folded ladders of gat_edge_kernels.hip the parent's?  A stand-alone program: it includes the library's
// source, next to it a verbatim copy of the parent's pick_fwd / pick_bwd (parent_picks.inc) and of the parent's host logic around
// them (below), and compares, for every input of the sweep, the whole EdgePick, the edge-order refusal decision of the launcher and the
// pick the grid is sized from.  It only compares kernel stub addresses: no device.
// Build and run: sweep.py in this directory.  One process per setting of the choice switches (they are read once per process).
//
// Output: one line "SWEEP inputs N differences D", then "FN <address>" for every distinct kernel the PARENT's ladders returned
// (fn and fix), which sweep.py turns into names through the program's symbol table.
#include "../../graph-attention-network-gatv2-_amd/csrc/gat_edge_kernels.hip"

#include <cstdio>
#include <cstdlib>
#include <set>

namespace gat {
// what the library's other translation units provide
static std::string g_msg;
void set_error(const std::string& m) { g_msg = m; }
int fail(int code, const std::string& m) { g_msg = m; return code; }
const char* choice_env(const char* name) { return getenv(name); }
int64_t resident_capped(int64_t blocks) { return blocks; }

namespace {
#include "parent_picks.inc"
static EdgePick parent_pick_forward(const EdgeFwdArgs& a, bool ext, bool res, bool pe) {
    GAT_DISPATCH_HD_D(a.H * a.D, a.D, parent_pick_fwd, a.bf16 != 0, a, ext, res, pe)
    return {};
}
static EdgePick parent_pick_backward(const EdgeBwdArgs& a, bool drop, int dbg, bool pe = false) {
    GAT_DISPATCH_HD_D(a.H * a.D, a.D, parent_pick_bwd, a.bf16 != 0, a, drop, dbg, pe)
    return {};
}
// the parent's edge_backward_blocks up to the occupancy query, verbatim: the pick the grid is sized from (and the experiments' divisor)
static EdgePick parent_grid_pick(const EdgeBwdArgs& a, const DropArgs* drop, bool pe, int* grid_div) {
    const bool on = (drop != nullptr && drop->on != 0) || pe;     // edge features: the DROP instantiations, masks or not
    // the experiment kernels (dbg) run on the grid of the product kernel of their selection
    EdgePick p = parent_pick_backward(a, on, 0, pe);
    if (p.fn == nullptr) p = parent_pick_backward(a, false, 0);  // no dropout form: launch_edge_backward reports it
    *grid_div = 1;
#ifdef GAT_EXPERIMENTS
    *grid_div = parent_pick_backward(a, on, a.dbg).grid_div;
#endif
    return p;
}
// the parent's condition of "edge_backward: records in edge order need the fp32 group-per-row record kernel", verbatim
static bool parent_refuses_edge_order(const EdgeBwdArgs& a) {
    return a.edge_order && !(a.stash != nullptr && a.ge == nullptr && !a.bf16 && a.dbg == 0 && edge_backward_groups(a.H, a.D));
}
static bool same(const EdgePick& p, const EdgePick& q) {
    return p.fn == q.fn && p.block == q.block && p.per_block == q.per_block && p.fix == q.fix && p.grid_div == q.grid_div;
}
}  // namespace
}  // namespace gat

using namespace gat;

int main() {
    // any non-null address serves: nothing here is dereferenced
    static float buf[4]; static int32_t ibuf[4]; static uint32_t ubuf[4]; static uint64_t step; static int4 items[1];
    std::set<const void*> reached;
    long inputs = 0, diffs = 0;
#ifdef GAT_EXPERIMENTS
    const int n_dbg = 19;
#else
    const int n_dbg = 1;
#endif
    for (const auto& sh : kEdgeShapes)
        for (int bf = 0; bf < 2; ++bf) {
            for (int alpha = 0; alpha < 2; ++alpha)
                for (int v : {0b000, 0b100, 0b110, 0b101, 0b111}) {                   // (ext, res, pe)
                    EdgeFwdArgs a{};
                    a.H = sh.HD / sh.D; a.D = sh.D; a.bf16 = bf; a.alpha = alpha ? buf : nullptr;
                    const bool ext = v & 4, res = v & 2, pe = v & 1;
                    const EdgePick p = parent_pick_forward(a, ext, res, pe), q = pick_forward(a, ext, res, pe);
                    ++inputs;
                    if (!same(p, q) || p.fn == nullptr || p.fix == nullptr) {
                        ++diffs;
                        printf("DIFF fwd hd%d d%d bf%d alpha%d ext%d res%d pe%d\n", sh.HD, sh.D, bf, alpha, ext, res, pe);
                    }
                    reached.insert(p.fn); reached.insert(p.fix);
                }
            for (int m = 0; m < 16; ++m)                                              // store, taps, records, edge_order
                for (int on = 0; on < 2; ++on)
                    for (int pe = 0; pe < 2; ++pe)                                    // plain, drop, edge term without and with masks
                        for (int dbg = 0; dbg < n_dbg; ++dbg) {
                            EdgeBwdArgs a{};
                            a.H = sh.HD / sh.D; a.D = sh.D; a.bf16 = bf; a.dbg = dbg; a.items = items; a.n_items = 1; a.n_table = 1;
                            if (m & 1) { a.pos = ibuf; a.msg = buf; }
                            if (m & 2) { a.ge = buf; a.galpha = buf; }
                            if (m & 4) { a.stash = ubuf; a.gfull = buf; }
                            a.edge_order = (m & 8) ? 1 : 0;
                            EdgeBwdExtras x;
                            x.drop.step = &step; x.drop.on = on;
                            if (pe) { x.pe = buf; x.gpe = buf; }
                            const char* what = nullptr;
                            // 1. the ladders themselves
                            const bool drop = on || pe;
                            const EdgePick p = parent_pick_backward(a, drop, dbg, pe != 0), q = pick_backward(a, drop, dbg, pe != 0);
                            if (!same(p, q)) what = "pick";
                            if (p.fn != nullptr) reached.insert(p.fn);
                            // 2. the edge-order refusal: the parent's restated condition against the flag of the branch's pick, for every input
                            // that reaches it (both launchers have refused records without pos one check earlier: "stash path needs gfull and pos")
                            const bool reaches = !(a.stash != nullptr && a.ge == nullptr && (a.gfull == nullptr || a.pos == nullptr));
                            if (reaches && parent_refuses_edge_order(a) != (a.edge_order && !pick_backward(a, &x, dbg).edge_order)) what = "refusal";
                            // 3. the pick the grid is sized from
                            int div_p = 1, div_q = 1;
                            const EdgePick gp = parent_grid_pick(a, &x.drop, pe != 0, &div_p), gq = grid_pick(a, &x);
#ifdef GAT_EXPERIMENTS
                            div_q = pick_backward(a, &x, a.dbg).grid_div;
#endif
                            if (!same(gp, gq) || div_p != div_q || gp.fn == nullptr) what = "grid";
                            ++inputs;
                            if (what != nullptr) {
                                ++diffs;
                                printf("DIFF bwd %s hd%d d%d bf%d store%d taps%d records%d eo%d on%d pe%d dbg%d\n", what, sh.HD, sh.D, bf, m & 1, (m >> 1) & 1,
                                       (m >> 2) & 1, (m >> 3) & 1, on, pe, dbg);
                            }
                        }
        }
    printf("SWEEP inputs %ld differences %ld\n", inputs, diffs);
    for (const void* fn : reached) printf("FN %p\n", fn);
    return diffs ? 1 : 0;
}
