// gat_internal.h — declarations shared by the HIP translation units behind include/gatv2_abi.h.
// gfx950 (MI355X) only: wave64, fp32 MFMA, no portability layer.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <vector>

#include "gatv2_abi.h"

namespace gat {

constexpr int kWave = 64;

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
// getenv for CHOICE switches (same results, other kernel / launch shape): records what was set for gat_switches().  Timing-only and
// wrong-result experiments (GAT_DBG) are not choice switches: they exist only in a -DGAT_EXPERIMENTS build (make experiments).
const char* choice_env(const char* name);

#define GAT_HIP(expr)                                                                     \
    do {                                                                                  \
        hipError_t e__ = (expr);                                                          \
        if (e__ != hipSuccess)                                                            \
            return ::gat::fail((int)e__, std::string(#expr) + ": " + hipGetErrorString(e__)); \
    } while (0)

#define GAT_TRY(expr)                 \
    do {                              \
        int rc__ = (expr);            \
        if (rc__ != 0) return rc__;   \
    } while (0)

// ---- the generators' counter hash (synth._hash): gat_synth.hip draws the datasets with it, gat_negsample.hip the negatives -----------
constexpr uint64_t kGold = 0x9E3779B97F4A7C15ull;
__host__ __device__ inline uint64_t mix64(uint64_t x) {          // synth._mix (splitmix64 finaliser)
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}
// H(seed, stream, idx) = hash_at(hash_base(seed, stream), idx): the base is formed once on the host
inline uint64_t hash_base(uint64_t seed, uint64_t stream) { return mix64(seed ^ (stream * 0xD1342543DE82EF95ull)); }
__device__ inline uint64_t hash_at(uint64_t base, uint64_t idx) { return mix64(idx * kGold + base); }

// ---- dropout masks (gat_dropout.hip; the contract is in gatv2_abi.h "dropout") -------------------------
// Stateless, counter-based: every keep decision is a hash of (seed, step, layer, kind, node, position), so a shard, a replay and
// the backward draw the same masks as the forward without storing them.  `step` lives on the device (advanced by the layer-0
// projection of a training forward), so a captured graph replays with fresh masks.
struct DropArgs {
    const uint64_t* step = nullptr;   // device counter
    const int64_t* bounds = nullptr;  // [world+1] device, or null: the node id of table row t is t
    int64_t max_rows = 0;             // rows per rank slice of the source table (with bounds)
    int64_t row0 = 0;                 // table row of local row 0
    uint32_t seed_lo = 0, seed_hi = 0;
    uint32_t T = 0;                   // drop threshold on the 24-bit draw: keep <=> (r >> 8) >= T
    float scale = 1.f;                // 1 / (1 - p)
    int32_t layer = 0;
    int32_t on = 0;                   // generic kernels: runtime switch (the wave-per-row kernels take a template flag)
    uint32_t Te = 0;                  // DropEdge threshold (gatv2_abi.h "DropEdge"): edge kept <=> (r >> 8) >= Te; 0 = every edge kept
    int32_t eflags = 0;               // GAT_DROPEDGE_* bits
};
enum : int32_t { kDropFeat = 0, kDropAttn = 1 };
constexpr uint32_t kDropEdgeKey = 0x40000000u;   // last word of K_e: never reached by 2*l + kind
__host__ __device__ __forceinline__ uint32_t drop_fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__host__ __device__ __forceinline__ uint32_t drop_mix(uint32_t k, uint32_t v) { return drop_fmix32(k ^ (v * 0x9E3779B9u + 0x7F4A7C15u)); }
// K(kind, l) for the step the counter holds
__device__ __forceinline__ uint32_t drop_key(const DropArgs& d, int32_t kind) {
    const uint64_t st = *d.step;
    uint32_t k = drop_mix(d.seed_lo, d.seed_hi);
    k = drop_mix(k, (uint32_t)st);
    k = drop_mix(k, (uint32_t)(st >> 32));
    return drop_mix(k, (uint32_t)(2 * d.layer + kind));
}
// K_e(l) for the step the counter holds: the same chain, last word 0x40000000 + l (l = 0 with GAT_DROPEDGE_SHARED_LAYERS)
__device__ __forceinline__ uint32_t drop_edge_key(const DropArgs& d) {
    const uint64_t st = *d.step;
    uint32_t k = drop_mix(d.seed_lo, d.seed_hi);
    k = drop_mix(k, (uint32_t)st);
    k = drop_mix(k, (uint32_t)(st >> 32));
    return drop_mix(k, kDropEdgeKey + (uint32_t)((d.eflags & GAT_DROPEDGE_SHARED_LAYERS) ? 0 : d.layer));
}
// id in the unsharded graph of local row r (padding rows of a shard get some id: their features are zero)
__device__ __forceinline__ uint32_t drop_node(const DropArgs& d, int64_t r) {
    const int64_t t = d.row0 + r;
    if (d.bounds == nullptr) return (uint32_t)t;
    return (uint32_t)(d.bounds[t / d.max_rows] + t % d.max_rows);
}
// 0 or 1/(1-p)
__device__ __forceinline__ float drop_factor(const DropArgs& d, uint32_t r) { return (r >> 8) >= d.T ? d.scale : 0.f; }
// DropEdge: is edge k (position in its full CSR row) of local row `row` kept?  ke = mix(K_e(l), node(row)); src = its col_idx entry.
// One draw per edge, shared by all heads.
__device__ __forceinline__ bool drop_edge_kept(const DropArgs& d, uint32_t ke, int k, int src, int64_t row) {
    return (drop_mix(ke, (uint32_t)k) >> 8) >= d.Te || ((d.eflags & GAT_DROPEDGE_KEEP_SELF) && (int64_t)src == d.row0 + row);
}

int launch_drop_advance(uint64_t* step, hipStream_t s);
// xo[r][f] = x[r][f] * kappa * s_f for f < F, 0 for F <= f < ld (rows of `ld` floats)
int launch_feat_drop_fwd(const float* x, float* xo, int64_t rows, int32_t F, int32_t ld, const DropArgs& d, hipStream_t s);
// g[r][f] *= kappa * s_f   (rows of F floats)
int launch_feat_drop_bwd(float* g, int64_t rows, int32_t F, const DropArgs& d, hipStream_t s);
// taps: out [H][E] = 0 or s_a per (head, CSR edge); out [rows][F] = 0 or s_f
int launch_attn_keep_tap(const int32_t* row_ptr, int64_t n_rows, int64_t n_edges, int32_t H, const DropArgs& d, float* out, hipStream_t s);
int launch_feat_keep_tap(int64_t rows, int32_t F, const DropArgs& d, float* out, hipStream_t s);
// out [E] = 0 or 1 per CSR edge (DropEdge)
int launch_edge_keep_tap(const int32_t* row_ptr, const int32_t* col_idx, int64_t n_rows, int64_t n_edges, const DropArgs& d, float* out, hipStream_t s);

// ---- edge-centric kernels (gat_edge_kernels.hip) ------------------------------------------------
struct EdgeFwdArgs {
    const int32_t* row_ptr;   // [n_rows+1]
    const int32_t* col_idx;   // [E] table row ids
    const float* PL;          // [n_table][HD]
    const float* PR;          // [n_rows][HD]
    const float* a;           // [HD]
    float* alpha;             // [E][H]; fast path: null = do not materialise (training path)
    float* score;             // [E][H] or null: raw attention scores (tap, E:323); only with alpha
    float* hpre;              // [n_rows][HD]
    float* hout;              // hidden [n_rows][HD]; last [n_rows][D]
    float* mstat;             // [n_rows][H] softmax max per (row, head); fast path: log2 domain
    float* zstat;             // [n_rows][H] softmax sum
    int64_t n_rows;
    int64_t n_table;          // rows of the gathered PL table (fast path: < 4 GiB, see edge_fast_path)
    int32_t bf16;             // PL (and msg) rows stored as bf16 (cfg.storage_dtype)
    int32_t H, D;
    int32_t is_last;
    float slope;
    // work items of the wave-per-item fast path (see WorkList); unused by the generic path
    const int4* items;        // [n_items] {row, beg, end, slot|-1}
    int64_t n_items;
    const int4* slot_info;    // [n_slots] {row, first_slot, nseg, item}
    int32_t n_slots;
    int32_t n_split;          // split rows: slot_info[n_slots + k].x = first slot of the k-th
    float* part_acc;          // [n_slots][HD]  per-segment partial sums of split rows
    float* part_mz;           // [n_slots][2H]  per-segment (max, sum)
};

// Work decomposition of a CSR graph for the wave-per-item kernels: every row with <= kSegEdges
// in-edges is one item, longer rows (power-law hubs) are cut into segments of kSegEdges edges
// (slot >= 0) that are listed first; slot_info describes the split rows for the fix-up kernels.
constexpr int kSegEdges = 256;      // swept 64..512 on the Products shape (GAT_SEG_EDGES): 256 best by ~0.5 %
struct WorkList {
    std::vector<int32_t> items;       // 4 per item
    std::vector<int32_t> slot_info;   // 4 per slot {row, first slot, segments, item}; then 4 per SPLIT ROW {first slot,-,-,-}
    int64_t n_items = 0;
    int32_t n_slots = 0;
    int32_t n_split = 0;              // rows cut into segments (entries n_slots .. n_slots+n_split-1 of slot_info)
};
void build_worklist(const int32_t* row_ptr, int64_t n_rows, WorkList& w);
struct LnArgs {
    const float* gamma = nullptr; // [HD], null: no normalisation
    const float* beta = nullptr;  // [HD]
    float eps = 0.f;
};
// What a forward may take beyond EdgeFwdArgs.  Any of it selects the extended instantiations of the kernels (and of the fix-up kernel),
// whose argument struct is EdgeFwdExtArgs below; without extras the kernels keep the plain struct and the machine code they have
// without these features.
// drop: attention dropout / DropEdge (drop.on: a mask is active).  drop.step must point at a device counter whenever extras are
//   passed: the extended instantiations hash every edge.  THE RULE (neutral_mask below, called by the two launchers): extras without
//   an active mask run the extended instantiation with T = Te = 0, scale = 1 — every draw keeps, nothing is scaled.  (The generic
//   kernels get the same struct and read drop.on at run time: off, they do not hash at all.  The template kernels never read it.)
// res / bias (either may be null, gatv2_abi.h "residual"): h_pre[row][c] += res[row][c] + bias[c] in the row epilogue, before h_pre
//   and hout are written (split rows: once, in the fix-up kernel's combine).
// ln (gatv2_abi.h "layer normalisation"): with ln.gamma set, the row u = h_pre (residual term included) is normalised over its H*D
//   channels in the same epilogue, v = gamma * (u - mu) * rstd + beta, and hout = LReLU(v); h_pre stays u.
// pe (gatv2_abi.h "edge features"): PE = EA We^T, one fp32 row per CSR edge, joins the score s = PL[src] + PR[dst] + PE[j]; the message
//   stays PL[src].  Non-null selects the PE instantiations of the extended kernels (their last template flag).
struct EdgeFwdExtras {
    DropArgs drop;
    const float* res = nullptr;   // [n_rows][HD] R = x' Wres^T of the shard's own rows, or null
    const float* bias = nullptr;  // [HD], or null
    LnArgs ln;
    const float* pe = nullptr;    // [n_edges][HD] fp32 in CSR order, or null
};
int launch_edge_forward(const EdgeFwdArgs& a, hipStream_t s, const EdgeFwdExtras* extras = nullptr);
struct EdgeFwdExtArgs : EdgeFwdArgs { EdgeFwdExtras x; };

struct EdgeBwdArgs {
    const int32_t* row_ptr;
    const int32_t* col_idx;
    const float* PL;          // [n_table][HD]
    const float* PR;          // [n_rows][HD]
    const float* a;           // [HD]
    const float* alpha;       // [E][H]  generic path only (the fast path recomputes it from mstat/zstat)
    const float* mstat;       // [n_rows][H] forward softmax max (fast path: log2 domain)
    const float* zstat;       // [n_rows][H] forward softmax sum
    const float* hpre;        // [n_rows][HD]
    const float* g;           // [n_rows][HD]  dL/dh_pre — or, with g_raw, dL/d(layer output): the edge kernels then
                              // apply LReLU'(h_pre) on load (E:888-892 folded into the consumer, which reads h_pre anyway)
    int32_t g_raw;
    const float* gh;          // last layer, or null: [n_rows][D] head-independent output gradient; the kernels form
                              // g[n,h,d] = gh[n,d] * LReLU'(h_pre[n,h,d]) / H themselves (E:598-603) and ignore `g`
    float* gPL;               // [n_table][HD]  atomics path only: zeroed by the caller, added into
    const int32_t* pos;       // [E] CSC slot of every edge, or null = atomics path
    float* msg;               // [E][HD] message rows by slot (store path; summed by launch_gpl_sum)
    uint32_t* stash;          // or: [E + 1][HD/N] per-edge records by slot (stash path, see edge_stash_words; launch_gpl_pull)
    uint32_t stash_spare;     // index of the spare record behind the last slot (= E): where padded lanes store
    float* gfull;             // [n_rows][HD] written with the stash path: dL/dh_pre incl. the LReLU' factor (gathered by launch_gpl_pull)
    int32_t gh_stride;        // floats between consecutive rows of gh (D, or 16 when gh rows and their decision bytes share 64-B records)
    int32_t hb_stride;        // bytes between consecutive rows of hbits
    uint8_t* hbits;           // last layer (gh != null), or null: [n_rows][HD/N] one byte per lane = the LReLU'(h_pre) decisions of its
                              // N channels; written INSTEAD of gfull — the pull pass rebuilds g = gh * LReLU'(h_pre) / H from gh
                              // (32 B per node at D = 8) and these 16 B instead of gathering a 256-B row of g
    float* gPR;               // [n_rows][HD]   written
    float* ge;                // [E][H] or null (tap)
    float* galpha;            // [E][H] or null (tap, E:646); only with ge
    float* ga_partial;        // [ga_blocks][HD] written
    int32_t ga_blocks;        // grid size the launcher must use (== rows of ga_partial)
    int64_t n_rows;
    int64_t n_table;          // rows of the gathered PL table (fast path: < 4 GiB, see edge_fast_path)
    int32_t bf16;             // PL (and msg) rows stored as bf16 (cfg.storage_dtype)
    int32_t H, D;
    float slope;
    const int4* items;        // as in EdgeFwdArgs
    int64_t n_items;
    const int4* slot_info;
    int32_t n_slots;
    int32_t n_split;          // split rows: slot_info[n_slots + k].x = first slot of the k-th
    float* part_acc;          // [n_slots][HD]  per-segment gPR partials of split rows
    int32_t dbg;
    int32_t edge_order;       // records in CSR edge order: record j = edge j (records_take_edge_order below), not stash[pos[j]]; fits the struct's tail padding
};
// What a backward may take beyond EdgeBwdArgs, the counterpart of EdgeFwdExtras.  An active mask or the edge term selects the DROP
// instantiations of the kernels, whose argument struct is EdgeBwdDropArgs below.  The grid and the launch are handed the SAME object:
// edge_backward_blocks(a, &x) sizes the grid — and the ga_partial rows — for the kernel launch_edge_backward(a, s, &x) runs.
// drop: the attention dropout / DropEdge of the forward this backward follows (same masks)
// pe / gpe (both or neither; gatv2_abi.h "edge features"): the forward's PE rows, and where gs = ge * a * LReLU'(s) of every CSR edge is
//   written ([n_edges][HD] fp32, zeros at dropped edges).  They select the PE instantiations of the DROP kernels, under the forward's
//   rule (neutral_mask): without an active mask those run with T = Te = 0, scale = 1 (drop.step must still point at the device counter).
struct EdgeBwdExtras {
    DropArgs drop;
    const float* pe = nullptr;    // [n_edges][HD] fp32 in CSR order, or null
    float* gpe = nullptr;         // [n_edges][HD] fp32, written
};
int launch_edge_backward(const EdgeBwdArgs& a, hipStream_t s, const EdgeBwdExtras* x = nullptr);
// the DROP kernels' argument: the plain struct, then drop, pe, gpe — the layout those kernels were compiled against
struct EdgeBwdDropArgs : EdgeBwdArgs, EdgeBwdExtras {};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(offsetof(EdgeBwdDropArgs, drop) == sizeof(EdgeBwdArgs) && offsetof(EdgeBwdDropArgs, pe) == sizeof(EdgeBwdArgs) + sizeof(DropArgs) &&
                  offsetof(EdgeBwdDropArgs, gpe) == offsetof(EdgeBwdDropArgs, pe) + sizeof(float*) &&
                  sizeof(EdgeBwdDropArgs) == sizeof(EdgeBwdArgs) + sizeof(EdgeBwdExtras) && sizeof(EdgeBwdArgs) % alignof(DropArgs) == 0,
              "EdgeBwdDropArgs: EdgeBwdArgs, then drop, pe, gpe");
#pragma clang diagnostic pop
// THE RULE of the extended instantiations, forward and backward (they hash every edge): without an active mask every draw keeps and
// nothing is scaled.  The launchers apply it to their copy of the extras; nothing else does.
inline void neutral_mask(DropArgs& d) {
    if (!d.on) { d.T = 0; d.Te = 0; d.scale = 1.f; d.eflags = 0; }
}
// The work-list fields of EdgeFwdArgs / EdgeBwdArgs from a WorkList and its device copies (part_mz: the forward's only)
template <class Args> void set_work_list(Args& a, const WorkList& w, const int4* items, const int4* slot_info, float* part_acc, float* part_mz = nullptr) {
    a.items = items; a.n_items = w.n_items; a.slot_info = slot_info; a.n_slots = w.n_slots; a.n_split = w.n_split; a.part_acc = part_acc;
    if constexpr (std::is_same<Args, EdgeFwdArgs>::value) a.part_mz = part_mz;
}
// Temporary device buffers of one call, freed at scope exit: declare it before the call's last synchronisation of its stream.
struct Scratch {
    std::vector<void*> bufs;
    ~Scratch() { for (void* p : bufs) (void)hipFree(p); }
    template <class T> int get(T** out, int64_t count) {
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, (size_t)(count > 0 ? count : 1) * sizeof(T));
        if (e != hipSuccess) return fail(GAT_E_NOMEM, std::string("op scratch: ") + hipGetErrorString(e));
        bufs.push_back(p); *out = (T*)p;
        return 0;
    }
};
// Device work list of a caller-provided CSR, its buffers in a Scratch (the op-level entry points have no context)
struct ScratchWorkList {
    WorkList w; int4* items = nullptr; int4* slot_info = nullptr; float* part_acc = nullptr; float* part_mz = nullptr;
    int build(Scratch& t, const int32_t* d_row_ptr, int64_t n, int32_t hd, int32_t h, hipStream_t s) {
        std::vector<int32_t> rp(n + 1);
        GAT_HIP(hipMemcpyAsync(rp.data(), d_row_ptr, (n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        GAT_HIP(hipStreamSynchronize(s));
        build_worklist(rp.data(), n, w);
        GAT_TRY(t.get(&items, w.n_items));
        GAT_TRY(t.get(&slot_info, w.n_slots + w.n_split));
        GAT_TRY(t.get(&part_acc, (int64_t)(w.n_slots > 0 ? w.n_slots : 1) * hd));
        GAT_TRY(t.get(&part_mz, (int64_t)(w.n_slots > 0 ? w.n_slots : 1) * 2 * h));
        if (w.n_items) GAT_HIP(hipMemcpyAsync(items, w.items.data(), w.items.size() * 4, hipMemcpyHostToDevice, s));
        if (w.n_slots) GAT_HIP(hipMemcpyAsync(slot_info, w.slot_info.data(), w.slot_info.size() * 4, hipMemcpyHostToDevice, s));
        GAT_HIP(hipStreamSynchronize(s));
        return 0;
    }
};
// Last layer, fused per row (gat_step): forward edge pass + output head + backward edge pass of every WHOLE row in one kernel
// (edge_last_fused_kernel); f / b as for the separate passes (f.items / f.n_items: the whole-row items only; b.ga_partial /
// b.ga_blocks from edge_last_fused_blocks), gh_out = the [n_rows][gh_stride] node records the pull pass reads.
struct EdgeLastArgs {
    EdgeFwdArgs f;
    EdgeBwdArgs b;
    const float* Wo;          // [C][D]
    const int32_t* labels;    // [n_rows]; negative = outside the training mask
    float* gh_out;            // [n_rows][b.gh_stride]
    int32_t C;
};
bool edge_last_fused_supported(int32_t H, int32_t D, int32_t C);
int edge_last_fused_blocks(int64_t n_items);
int launch_edge_last_fused(const EdgeLastArgs& a, hipStream_t s);
// gH = Wo^T dz of the split rows only (their forward runs as segments): slot_info as in EdgeFwdArgs
int launch_head_rows(const int4* slot_info, int32_t n_slots, int32_t n_split, const float* Wo, const float* HL, const int32_t* labels,
                     float* gh_out, int32_t gh_stride, int32_t C, int32_t DLAST, hipStream_t s);
// Words per edge record of the stash path for an (H, D) layer, 0 = that shape has no stash path (the message-row
// path is used): two lanes per head are needed (D = 8 with four channels per lane, D = 4 with two).
int edge_stash_words(int32_t H, int32_t D);
// Rows of ga_partial a layer's backward may write: the cap of every grid that writes one row per block
constexpr int kGaPartialRows = 2048;
// Grid size (== rows of ga_partial, <= kGaPartialRows) for the backward launch_edge_backward(a, s, x) will run: sized for the
// kernel those arguments select (a.ga_blocks is not read)
int edge_backward_blocks(const EdgeBwdArgs& a, const EdgeBwdExtras* x = nullptr);
// wave-per-row templates cover this (H, D), and the gathered table is < 4 GiB (they address it as
// uniform base + 32-bit byte offset); anything else runs the generic kernels
bool edge_fast_path(int32_t H, int32_t D, int64_t n_table);

// ---- source-major slot index + segmented sum (gat_csc.hip) ----------------------------------------
// csrc (optional): [n_edges + kPullPad] table row of every slot (the sorted keys), -1 in the padding
int build_csc(const int32_t* col_idx, int64_t n_edges, int64_t n_table, int32_t* pos, int32_t* src_ptr,
              int32_t* csrc, hipStream_t s);
// sources with long slot lists, cut into chunks (gat_csc.hip kHeavySlots): built once per graph from the CSC pointers
struct HeavyList {
    std::vector<int32_t> chunks;    // int4 {first slot, end slot, partial row, -}
    std::vector<int32_t> heavy;     // int4 {source, first partial, partial count, -}
    int32_t threshold = 0;          // slots above which a list is chunked (depends on the graph size)
    std::vector<int32_t> items;     // int4 {source, first slot, end slot, partial row | -1}: chunks first, then the other sources by length
    // slot-parallel form (SourceIndex::run ...): run length (0 = not built), number of runs, lists crossing a run boundary, rows without slots
    int32_t run = 0; int64_t n_runs = 0;
    std::vector<int32_t> open;      // int4 {source, first run, last run, -}
    std::vector<int32_t> empty;     // table rows without slots
};
int build_heavy_list(const int32_t* d_src_ptr, int64_t n_table, int64_t n_edges, HeavyList* out, hipStream_t s, int32_t run = 0);
// slots of padding behind the record buffer and the destination list: the pull pass reads whole 16-slot chunks (and one chunk
// of destinations ahead) without clamping its indices
// REQUIREMENT on callers of launch_gpl_pull: SourceIndex::slot_capacity is the allocated slot count; below n_slots + kPullPad the
// clamped first form is used.  The padding's CONTENT is not relied on (slots beyond a list are zeroed after their load), only its presence;
// the gathered tables are addressed with 32-bit byte offsets (n_table * H*D * 4 < 4 GiB: edge_fast_path; node records: n_rows < 2^26).
constexpr int64_t kPullPad = 32;
// The device-side source-major index of one graph, everything the second pass walks beside the records or rows themselves.  Built
// once per graph by ensure_buffers in gat_abi.hip (which owns the allocations) from build_csc / build_csc_dst / build_heavy_list.
struct SourceIndex {
    const int32_t* src_ptr = nullptr;   // [n_table + 1] first slot of every table row
    const int32_t* cdst = nullptr;      // [slot_capacity] destination row of every slot (record path), or null
    const int32_t* cedge = nullptr;     // [slot_capacity] CSR edge of every slot (the inverse of pos), the padding at the spare record n_slots; or null
    // slot-parallel ("runs") form (gat_csc.hip gpl_pull_runs_kernel): the flat slot stream cut into runs of `run` slots, one per
    // lane group, segmented by a streamed source id per slot
    const int32_t* csrc = nullptr;      // [n_slots + kPullPad] table row of every slot, -1 behind the last; null = runs not built
    int32_t run = 0;                    // slots per run (a multiple of 32)
    int64_t n_runs = 0;
    const int4* open = nullptr; int32_t n_open = 0;       // lists crossing a run boundary {source, first run, last run, -}
    const int32_t* empty = nullptr; int64_t n_empty = 0;  // table rows without slots
    float* run_part = nullptr;          // [2 n_runs][HDmax] partial rows of the runs' open segments
    // long source lists, cut into chunks (HeavyList)
    const int4* chunks = nullptr; int32_t n_chunks = 0;   // {first slot, end slot, partial row, -}
    const int4* heavy = nullptr; int32_t n_heavy = 0;     // {source, first partial, partial count, -}
    float* part = nullptr;              // [n_chunks][HDmax] partial rows of the chunks
    const int4* items = nullptr; int64_t n_items = 0;     // length-sorted source items of the pull pass (HeavyList::items), or null
    int64_t n_table = 0, n_slots = 0;
    int64_t slot_capacity = 0;          // slots allocated in the record buffer AND cdst: n_slots + kPullPad enables the unclamped forms
};
// below this many slots the runs cannot fill the chip (Pubmed shape: 44 k slots = 173 waves; 0.244 -> 0.268 ms per step with
// runs, Cora shape 0.190 -> 0.216) and the list-per-wave kernels stay; Arxiv shape (1.17 M slots): 0.256 -> 0.195 ms per step
constexpr int64_t kRunsMinSlots = 512 << 10;
// THE short-list rule: lists this short (a destination-range shard, a sparse graph), and enough of them, take the slot-parallel
// form.  Unforced: the callers apply their switches (GAT_PULL_RUNS, ...) and their own conditions around it.
inline bool short_lists_take_runs(int64_t n_slots, int64_t n_table) { return n_slots < 8 * n_table && n_slots >= kRunsMinSlots; }
// Which family of pull kernels a record pass over `ix` runs (gat_csc.hip pick_pull, switches GAT_PULL_RUNS / GAT_PULL_GROUPS included).
// lpe = lanes per record, records64: hidden layer, or the last layer's 64-byte node records.
enum PullForm : int32_t { kPullLists, kPullItems, kPullRuns };
PullForm pull_form(const SourceIndex& ix, int32_t lpe, bool records64);
// the fp32 record backward of this shape is the group-per-row kernel (gat_edge_kernels.hip; GAT_ROWGROUP=0: the chunked one)
bool edge_backward_groups(int32_t H, int32_t D);
// THE record-order rule.  A layer's records may lie in CSR edge order (record j = edge j: the backward streams them out instead of
// scattering half lines, the pull pass fetches record cedge[slot]) only where the group-per-row backward writes fp32 records and the
// wave-per-list pull (gpl_pull_kernel + gpl_pull_chunk_kernel) reads them: the only kernels with that form.  node_records: the pull
// rebuilds g from the last layer's node records (else it gathers gfull rows, as on a hidden layer) — the default is per kind, from
// the measurement in DESIGN §4 "Record order"; GAT_STASH_ORDER=0|1 forces it wherever the form exists.  plan_backward_edges asks
// once per layer and hands the answer to both passes (EdgeBwdArgs::edge_order, PullArgs::edge_order); pick_pull refuses a layout
// the rule does not give.
constexpr bool kEdgeOrderHidden = true, kEdgeOrderLast = false;     // the unforced answer per layer kind
bool records_take_edge_order(const SourceIndex& ix, int32_t H, int32_t D, bool fp32, bool node_records, bool records64);
// message rows: gPL[s][:] = sum over the slots of s of msg[slot][:]   (rows of HD floats, or HD bf16 with msg_bf16)
int launch_gpl_sum(const SourceIndex& ix, const float* msg, bool msg_bf16, float* gPL, int32_t HD, hipStream_t s);
// cdst[pos[e]] = destination row of CSR edge e (the source-major twin of a1's dst array; built once per graph)
// cedge (or null): [n_edges + kPullPad], cedge[pos[e]] = e, the padding = n_edges (the spare record)
int build_csc_dst(const int32_t* row_ptr, const int32_t* pos, int32_t* cdst, int64_t n_rows, int64_t n_edges, hipStream_t s, int32_t* cedge = nullptr);
// Stash path: gPL[s][:] = sum over the slots of s of  g[cdst][:] * alpha + ge * a (.) LReLU'  rebuilt from the records
// gh / hbits non-null (last layer): g rows are rebuilt from gh [n_rows][D] and the per-lane decision bytes instead of read from gfull
struct PullArgs {
    const uint32_t* stash; const float* gfull; bool g_bf16; const float* gh; const uint8_t* hbits;
    int32_t gh_stride, hb_stride; const float* a; float slope; float* gPL; int32_t H, D;
    bool edge_order = false;            // the records lie in CSR edge order (records_take_edge_order): read through SourceIndex::cedge
};
int launch_gpl_pull(const SourceIndex& ix, const PullArgs& p, hipStream_t s);

int launch_csr_to_coo(const int32_t* row_ptr, const int32_t* col_idx, int32_t* src, int32_t* dst,
                      int64_t n_rows, int64_t n_edges, int64_t table_row0, hipStream_t s);

// out[c] += sum_b partial[b][c]   (deterministic: one thread per c, ascending b)
// ---- exchange transports (gat_comm.hip) ---------------------------------------------------------------
struct Comm {
    int world = 1, rank = 0;
    virtual ~Comm();
    // table: [world][slice] floats; the rank's slice already written / afterwards holding the sum
    virtual int all_gather(float* table, int64_t slice, hipStream_t s) = 0;
    // the same for floats [off, off+cnt) of EVERY rank's slice only (chunk-pipelined forward exchange)
    virtual int all_gather_part(float* table, int64_t slice, int64_t off, int64_t cnt, hipStream_t s) = 0;
    virtual int reduce_scatter(float* table, int64_t slice, hipStream_t s) = 0;
    // The same exchange with the REMOTE partial sums travelling as bf16 (half the xGMI volume): every rank rounds the
    // slices it sends to bf16 (nearest even), keeps its own partial in fp32, and adds what arrives in fp32 in ascending
    // rank order.  Option GAT_COMM_GPL_BF16; relative error of the summed rows ~ 2^-9 per remote term.
    virtual int reduce_scatter_bf16(float* table, int64_t slice, hipStream_t s) = 0;
    virtual int all_reduce(float* buf, int64_t n, hipStream_t s) = 0;
    // Pairwise exchange of packed rows (halo form, gat_halo.hip): this rank sends cnt_send[q] rows of rf floats to every rank q
    // (sendbuf grouped by q, ascending) and receives cnt_recv[q] rows from it (recvbuf grouped the same way); the counts (host
    // arrays of `world` entries) are fixed at set-up and consistent between the two ends.  One send / receive pair per peer.
    virtual int exchange_rows(const float* sendbuf, const int64_t* cnt_send, float* recvbuf, const int64_t* cnt_recv, int64_t rf, hipStream_t s) = 0;
};
// Halo form of the table exchanges (gat_halo.hip): per peer, the rows of its slice this shard's edges reference.
struct HaloPlan {
    int world = 0, rank = 0;
    int64_t max_rows = 0;
    std::vector<int64_t> need_cnt, send_cnt;      // [world] rows received from / sent to each rank in the forward exchange
    int64_t n_need = 0, n_send = 0, buf_rows = 0;
    int32_t* need_rows = nullptr;                 // device [n_need] table rows, grouped by owner (ascending)
    int32_t* send_rows = nullptr;                 // device [n_send] rows of the own slice (local ids), grouped by requester (ascending)
    int32_t *arr_ptr = nullptr, *arr_split = nullptr, *arr_pos = nullptr;      // backward sum: arrivals per own row, lower ranks first
    float *sendbuf = nullptr, *recvbuf = nullptr; // [buf_rows][max H*D]
    double referenced_fraction = 1.0;             // rows on the wire / rows of the full exchange, over all ranks
};
int halo_build(Comm* comm, const int32_t* d_col_idx, int64_t n_edges, int64_t n_table, int32_t hd_max, HaloPlan* out, hipStream_t s);
int halo_forward(Comm* comm, const HaloPlan& h, float* table, int64_t rf, hipStream_t s);
int halo_backward(Comm* comm, const HaloPlan& h, float* gPL, int64_t rf, hipStream_t s);
void halo_free(HaloPlan* h);
int comm_unique_id(void* id_out);
int comm_create_rccl(int world, int rank, const void* id_bytes, Comm** out);
int comm_create_host(int world, int rank, const char* shm_name, int64_t bytes_per_rank, Comm** out);

// Deferred slab reductions.  Between reduce_batch_begin() and reduce_batch_flush() (same host thread) launch_reduce_gradw /
// launch_reduce_partials_add queue their job instead of launching it, and the flush runs all of them — plus the result
// pack, if asked for — as ONE kernel: on Cora / Pubmed-size graphs every launch is ~5 us of a ~250 us step.  The slabs
// of a queued job must stay untouched until the flush (per-layer scratch regions: ensure_buffers in gat_abi.hip).
struct ReduceJob { const float* slabs; float* out; int64_t width; int32_t nslabs, HD, F, c_base, block0; };   // HD == 0: out[idx]
struct ReduceBatch {
    ReduceJob jobs[8]; int32_t n, blocks;
    const float* loss; const int32_t* correct; float* dst3; float* dst3_host;      // result pack (dst3_host: optional pinned copy)
    const double* fin_loss; const int32_t* fin_corr; int32_t fin_n; float* fin_loss_out; int32_t* fin_corr_out;   // head finalize
};
void reduce_batch_begin();
void reduce_batch_abort();
void reduce_batch_pack(const float* loss, const int32_t* correct, float* dst3, float* dst3_host);
// the output head's block partials -> {loss, #correct} (head_finalize_kernel) inside the batch kernel's pack block; false = not queued
bool reduce_batch_finalize(const double* loss_partial, const int32_t* correct_partial, int32_t nblocks, float* loss_out, int32_t* correct_out);
int reduce_batch_flush(hipStream_t s);
int launch_reduce_partials_add(const float* partial, int32_t nblocks, int64_t width, float* out,
                               hipStream_t s);

// gradW[(c%HD)][(c/HD)*F + f] += sum_z slabs[z][c - c_base][f]   (c over c_base .. c_base+M-1, fixed order)
int launch_reduce_gradw(const float* slabs, int32_t ksplit, int32_t HD, int32_t F, int32_t c_base, int32_t M,
                        float* gradW, hipStream_t s);

// Blocks of a 256-thread kernel that are resident on the whole chip at once (occupancy API incl.
// dynamic LDS; cached).  Persistent kernels use exactly this grid: a larger one runs a second,
// partly filled round of blocks.
int64_t resident_blocks(const void* fn, size_t dyn_lds, int threads = 256);
// GAT_RESIDENT_CAP=<n> (tests) applied to a resident count: min(blocks, n), at least 1; unset: blocks.  Every persistent grid —
// resident_blocks() above and the edge kernels' own count (gat_edge_kernels.hip) — answers through it.
int64_t resident_capped(int64_t blocks);
// The template name of the row / tile kernel the dense launchers below launched last on this host thread, e.g.
// "rowgemm_x3_kernel<2, 8, true>" ("" after the clear: nothing launched) — the gat_op_dense_* seams report it.
const char* dense_last_kernel();
void dense_last_kernel_clear();

// layout converters for taps / op-level entry points
int launch_transpose_eh_to_he(const float* src_eh, float* dst_he, int64_t E, int32_t H, hipStream_t s);
int launch_transpose_he_to_eh(const float* src_he, float* dst_eh, int64_t E, int32_t H, hipStream_t s);
int launch_transpose_nh_to_hn(const float* src_nh, float* dst_hn, int64_t N, int32_t H, hipStream_t s);

// ---- dense kernels (gat_dense_kernels.hip) -------------------------------------------------------
// PL[table_row0 + i][j] = sum_f X[i][f] * W[j][f],  PR[i][j] = sum_f X[i][f] * W[j][F+f]
// W in reference layout [HD][2F].
// part: both halves in one pass over X, or only the W_left (PL) / W_right (PR) half — the two halves run over
// different row sets when the layer input is replicated on every shard (gat_set_source_features).
enum : int32_t { kPartBoth = 0, kPartLeft = 1, kPartRight = 2 };
// pl_bf16: PL_rows points at bf16 rows ([.][HD] of 2 bytes) — cfg.storage_dtype
// scratch / scratch_floats: a buffer of at least project_scratch_floats(n_rows, F, HD, part) floats (0 = this launch never
// needs one), or null; few rows with a long K (Cora / Pubmed shapes) take a split-K path through it.  A scratch smaller than
// this launch needs (or null) selects the streaming kernel — never an overrun.
int64_t project_scratch_floats(int64_t n_rows, int32_t F, int32_t HD, int32_t part);
// ldx: floats between consecutive rows of X (0 = F).  A pitch that is a multiple of 4 with ZEROS behind column F lets the kernels use
// 16-byte loads for an odd F (a float4 that starts below F may read up to three padding floats: they must be finite).
int launch_project(const float* X, const float* W, float* PL_rows, float* PR, int64_t n_rows,
                   int32_t F, int32_t HD, int32_t part, bool pl_bf16, float* scratch, int64_t scratch_floats, hipStream_t s, int32_t ldx = 0);
// gradW[j][0:F] += sum_n gPL[n][j] X[n][:],  gradW[j][F:2F] += sum_n gPR[n][j] X[n][:]
// scratch: at least grad_w_scratch_floats(n_rows, F, HD) floats.
int64_t grad_w_scratch_floats(int64_t n_rows, int32_t F, int32_t HD);
int launch_grad_w(const float* gPL_rows, const float* gPR, const float* X, float* gradW,
                  float* scratch, int64_t n_rows, int32_t F, int32_t HD, int32_t part, hipStream_t s, int32_t ldx = 0);
// gprev[n][f] = (sum_j gPL[n][j] W[j][f] + gPR[n][j] W[j][F+f]) * LReLU'(hpre_prev[n][f])
// hpre_prev == nullptr: the plain sum is stored (the consumer applies LReLU', see EdgeBwdArgs::g_raw)
int launch_grad_x(const float* gPL_rows, const float* gPR, const float* W, const float* hpre_prev,
                  float* gprev, int64_t n_rows, int32_t F, int32_t HD, float slope, hipStream_t s);

// ---- residual / bias (gatv2_abi.h "residual") ------------------------------------------------------------------
// R[i][j] = sum_f X[i][f] * Wres[j][f]   (Wres flat [HD][F]; the three-piece product of launch_project, K walked in chunks of 128)
int launch_project_res(const float* X, const float* Wres, float* R, int64_t n_rows, int32_t F, int32_t HD, hipStream_t s, int32_t ldx = 0);
// gradWres[j][f] += sum_n G[n][j] X[n][f]   (the grad_w kernels on one half; scratch: grad_w_scratch_floats(n_rows, F, HD) floats)
int launch_grad_wres(const float* G, const float* X, float* gradWres, float* scratch, int64_t n_rows, int32_t F, int32_t HD,
                     hipStream_t s, int32_t ldx = 0);
// gx[n][f] += sum_j G[n][j] Wres[j][f]   (the grad_x kernel with an accumulating epilogue; run after launch_grad_x)
int launch_grad_x_res(const float* G, const float* Wres, float* gx, int64_t n_rows, int32_t F, int32_t HD, hipStream_t s);
// One N-sized pass of a residual layer's backward.  G = dL/dh_pre in fp32:
//   g_raw != 0 : g[n][c] * LReLU'(hpre[n][c])                       (hidden layers)
//   gh != null : gh[n][c % D] * LReLU'(hpre[n][c]) / H              (last layer; rows of gh_stride floats)
//   otherwise  : g[n][c]                                            (last layer with flat_lrelu_index: the head applied the factor)
// agg[n][c] = hpre[n][c] - (res[n][c] + bias[c]): the aggregate alone, which the edge backward takes in place of h_pre (its
// <g, h_pre> stands for sum_e alpha * galpha, true of the aggregate only).  partial [blocks][HD]: per-block column sums of G in
// fixed order (null: not formed), blocks = res_backward_blocks(...) <= kResPartialRows; finished by launch_reduce_partials_add.
struct ResBwdArgs {
    const float* hpre; const float* g; const float* gh; const float* res; const float* bias;
    float* G; float* agg; float* partial;
    int64_t n_rows;
    int32_t H, D, gh_stride, g_raw, blocks;
    float slope;
};
constexpr int kResPartialRows = 1024;
int res_backward_blocks(int64_t n_rows, int32_t HD);
int launch_res_backward(const ResBwdArgs& a, hipStream_t s);

// ---- layer normalisation (gatv2_abi.h "layer normalisation") ---------------------------------------------------
// The N-sized pass of a NORMALISED layer's backward, in res_backward's place.  Per row it recomputes mu, rstd and
// v = gamma * xhat + beta from u = r.hpre (two passes, as the forward), takes dL/dhout from r.g (hidden) or r.gh / H (last layer),
// dv = dL/dhout * LReLU'(v), and writes
//   G[n][c]   = rstd * (dxh - mean_c dxh - xhat * mean_c (dxh * xhat)),  dxh = dv * gamma        (r.G)
//   agg[n][c] = u - (res + bias)                                                                (r.agg; null: not written)
// with per-block fixed-order column sums  part_gamma = sum dv * xhat,  part_beta = sum dv,  r.partial = sum G  (each [blocks][HD], null:
// not formed), blocks = norm_backward_blocks(...) <= kResPartialRows; finished by launch_reduce_partials_add.  r.g_raw is not read.
// Any H*D >= 1: rows wider than one pass of the row's lanes are walked in rounds.
struct NormBwdArgs {
    ResBwdArgs r;
    const float* gamma; const float* beta;
    float* part_gamma; float* part_beta;
    float eps;
};
int norm_backward_blocks(int64_t n_rows, int32_t HD);
int launch_norm_backward(const NormBwdArgs& a, hipStream_t s);

// ---- batch normalisation (gatv2_abi.h "batch normalisation"; gat_batchnorm.hip) ----------------------------------
// The statistics a kernel normalises with, per channel [HD]: the batch's (mean, rstd) of a training forward, or — from_var — the
// running (mean, var) of eval mode, turned into 1 / sqrt(var + eps) as they are read.
struct BnStats { const float* mean; const float* scale; float eps; int32_t from_var; };
// Blocks of the kernels that write per-block column partials (each region [blocks][HD], blocks <= kResPartialRows).
int batch_norm_blocks(int64_t n_rows, int32_t HD);
// Training forward, launches 1 and 2: Welford / Chan column statistics of u [n_rows][HD] through part_mean / part_m2 [blocks][HD]
// into mean / rstd [HD]; run_mean / run_var (both or neither) advance by `momentum` with the unbiased variance.
int launch_batch_norm_stats(const float* u, int64_t n_rows, int32_t HD, float* part_mean, float* part_m2, float eps, float momentum, float* mean,
                            float* rstd, float* run_mean, float* run_var, hipStream_t s);
// Launch 3 (eval mode: the only one): hout = LReLU(gamma * (u - mean) * rstd + beta), [n_rows][HD], or with is_last the mean over heads
// [n_rows][D] (h ascending).
int launch_batch_norm_apply(const float* u, const BnStats& st, const float* gamma, const float* beta, float slope, float* hout, int64_t n_rows,
                            int32_t H, int32_t D, bool is_last, hipStream_t s);
// Backward of a normalised layer, in res_backward's place: dv = dL/dhout * LReLU'(v) with dL/dhout = g (hidden) or gh / H (last layer),
//   sums [2][HD] = {s1 = sum_n dv, s2 = sum_n dv * xhat} of THIS call (through part_s1 / part_s2 [blocks][HD]), added to grad_beta / grad_gamma,
//   G   = gamma * rstd * (dv - s1 / N - xhat * s2 / N)   (training)      gamma * rstd * dv   (training == 0: the statistics are constants)
//   agg = u - (res + bias)   (null: not written),  part_G [blocks][HD]: block column sums of G (null: not formed; finished by
//   launch_reduce_partials_add).  blocks = batch_norm_blocks(n_rows, H * D).
struct BnBwdArgs {
    const float* u; const float* g; const float* gh; const float* res; const float* bias;
    const float* gamma; const float* beta;
    BnStats stats;
    float* G; float* agg; float* part_G; float* part_s1; float* part_s2; float* sums;
    int64_t n_rows, gh_stride;
    int32_t H, D, blocks, training;
    float slope;
};
int launch_batch_norm_backward(const BnBwdArgs& a, float* grad_gamma, float* grad_beta, hipStream_t s);

// ---- output head (gat_head.hip) --------------------------------------------------------------------------------------
// One argument struct for the three loss modes and the three entry points.  mode 0: softmax + cross-entropy on integer labels (a
// negative label: the row is outside the training mask).  GAT_LOSS_BCE / GAT_LOSS_MSE (gatv2_abi.h "loss modes of the output head"): a
// float target matrix; an entry contributes when its row trains (mask null, or mask[r] != 0) and its target is not NaN, every other
// entry has loss 0, count 0 and dz 0.  In each mode every kernel forms z with the same expression in the same order, and the forward
// and the fused step run on grids that pair up, so their loss and count are bitwise equal.
struct HeadArgs {             // (what every forward reads comes first, together: a kernel fetches its fields with scalar loads)
    const float* Wo;          // [C][DL]
    const float* X;           // [n_rows][DL] the head's input rows: H_L, the pooled rows, the pair rows or the hidden layer's Z1
    const int32_t* labels;    // mode 0: [n_rows]
    float* y;                 // [n_rows][C] softmax / sigmoid(z) (BCE) / z (MSE): the forward writes it, the mode-0 backward reads it
    double* loss_partial;     // [head_blocks]
    int32_t* correct_partial; // [head_blocks]
    float* loss_out;          // [1] device, or null (loss-mode forward): the block partials are left for the caller (gat_eval_mask)
    int32_t* correct_out;     // [1] device
    int64_t n_rows;
    int32_t C, DL;
    int32_t mode;             // 0, GAT_LOSS_BCE or GAT_LOSS_MSE
    const float* T;           // loss modes: [n_rows][C] targets, NaN = missing
    const uint8_t* mask;      // loss modes: [n_rows] or null: every row
    const float* hpre;        // mode 0 with g: last layer pre-activation [n_rows][H][DL]
    float* g;                 // mode 0: [n_rows][H][DL], or null: only gh_out is written and the edge backward of the last
                              // layer expands it (EdgeBwdArgs::gh) — saves writing 4*N*H*D and reading h_pre here
    float* gh_out;            // rows of Wo^T dz (the head-independent part of g); null: mode 0 with g, or a step without gH
    int32_t gh_stride;        // floats between consecutive rows of gh_out (0 = DL)
    float* gradWo;            // [C][DL] added into
    float* partial;           // [head_bwd_blocks][C*DL]
    int32_t H;
    float slope;
    int32_t flat_index;
};
// sizes of the partial buffers: upper bounds of every head grid, functions of the row count alone
int head_blocks(int64_t n_rows);
int head_bwd_blocks(int64_t n_rows);
// blocks every launch of a loss mode uses (<= head_bwd_blocks <= head_blocks); < 0: the shape does not fit the LDS tile
int loss_head_blocks(int64_t n_rows, int32_t C, int32_t DL, int32_t mode);
// forward: y, loss, count.  backward: gH (or g) and gradWo from y (mode 0) or from z formed again (loss modes).  step: forward and
// backward in one kernel, y is not stored (gat_step without keep_taps) — where head_step_supported(a); gh_out may be null in mode 0.
int launch_head_forward(const HeadArgs& a, hipStream_t s);
int launch_head_backward(const HeadArgs& a, hipStream_t s);
bool head_step_supported(const HeadArgs& a);
int launch_head_step(const HeadArgs& a, hipStream_t s);
// The head's own shape limits for rows of DL floats and C columns under loss mode `mode` (the checks its launchers make, without
// a launch): 0, or GAT_E_UNSUPPORTED with *limit naming the limit that is broken
int head_shape_check(int32_t C, int32_t DL, int32_t mode, std::string* limit);
int launch_pack_result(const float* loss, const int32_t* correct, float* dst3, hipStream_t s);
// lowest flat index of an entry that is +-inf, or (BCE) outside [0, 1]; -1: none.  Device form: one pass, synchronises s.
int64_t targets_check_host(const float* t, int64_t n, int32_t mode);
int targets_check_device(const float* d_t, int64_t n, int32_t mode, unsigned long long* d_scratch, int64_t* where, hipStream_t s);
// part[b] = present entries in the rows of mask (null: all rows) seen by block b, blocks = 256
int launch_target_count(const float* T, const uint8_t* mask, int64_t n_rows, int32_t C, unsigned long long* part, hipStream_t s);
// train / validation masks (README R:134 "later"): labels_eff = mask ? label : ~label — the head kernels skip negative
// labels (no loss, no count, dz = 0); eval_mask: fixed-order block partials of loss / #correct / #nodes over a mask
int launch_apply_mask(const int32_t* labels, const uint8_t* mask, int32_t* eff, int64_t n, hipStream_t s);
int launch_eval_mask(const float* y, const int32_t* labels, const uint8_t* mask, int64_t n, int32_t C, double* part_loss,
                     int32_t* part_cnt, int32_t blocks, hipStream_t s);

// ---- graph-level readout (gat_readout.hip; the contract is in gatv2_abi.h "graph-level readout") ----------------------
// Work decomposition of the pooling: a graph of at most kReadoutSegRows rows is one item (an empty graph too), a longer one is cut into
// segments of kReadoutSegRows rows whose partial rows the combine kernel adds in ascending order.  256 like the hub rows' kSegEdges.
constexpr int kReadoutSegRows = 256;
struct ReadoutPlan {
    std::vector<int32_t> items;       // 4 per item {graph, first row, end row, partial row | -1}
    std::vector<int32_t> split;       // 4 per split graph {graph, first partial row, partial rows, -}
    int64_t n_items = 0;
    int32_t n_split = 0, n_parts = 0;
};
void build_readout_plan(const int32_t* graph_ptr, int64_t n_graphs, ReadoutPlan& p);
// the rules of gat_set_readout on a graph_ptr: *problem = 0, or 1 (entry 0 is not 0) / 2 (the last entry is not n_rows) / 3 (decreasing),
// *where = the lowest offending index (-1: none).  The device form is one pass and synchronises s.
int graph_ptr_check_host(const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t* problem, int64_t* where);
int graph_ptr_check_device(const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t* problem, int64_t* where, hipStream_t s);
std::string graph_ptr_problem_text(int32_t problem, int64_t where, int64_t n_rows);
// node_graph[n] = graph of row n (a checked graph_ptr)
int launch_node_graph(const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t* d_node_graph, hipStream_t s);
struct ReadoutFwdArgs {
    const float* x; int64_t x_stride;       // [n_rows] rows of x_stride floats, the first `width` pooled
    const int32_t* graph_ptr;               // [n_graphs + 1]
    const int4* items; int64_t n_items;     // ReadoutPlan::items
    const int4* split; int32_t n_split;     // ReadoutPlan::split
    float* pooled; int32_t* argmax;         // [n_graphs][width]; argmax: GAT_READOUT_MAX only
    float* part; int32_t* part_arg;         // [n_parts][width] partial rows of the segments (part_arg: GAT_READOUT_MAX only)
    int32_t width, mode;
};
int launch_readout_forward(const ReadoutFwdArgs& a, hipStream_t s);
// gh[n][0:width] = gpooled[g] (SUM), gpooled[g] / cnt_g (MEAN), gpooled[g][d] where argmax[g][d] == n, else 0 (MAX); floats behind
// column `width` of a gh row are not touched
struct ReadoutBwdArgs {
    const float* gpooled; const int32_t* argmax; const int32_t* graph_ptr; const int32_t* node_graph;
    float* gh; int64_t gh_stride; int64_t n_rows;
    int32_t width, mode;
};
int launch_readout_backward(const ReadoutBwdArgs& a, hipStream_t s);

// ---- pair head (gat_pair.hip; the contract is in gatv2_abi.h "pair head") ------------------------------------------------
// The backward's work list is the readout's plan over the incidence counts of the nodes (build_readout_plan on the incidence
// row_ptr): the same 256 — a node of at most kPairSegEntries incidences is one item, a longer one is cut into segments of that many.
constexpr int kPairSegEntries = kReadoutSegRows;
// the rules of gat_set_pairs on u / v: -1, or 2p + (0: u, 1: v) of the lowest pair p with an endpoint outside [0, n_rows), u before v.
// The device form is one pass, synchronises s and fetches the offending value.
int64_t pair_check_host(const int32_t* u, const int32_t* v, int64_t n_pairs, int64_t n_rows);
int pair_check_device(const int32_t* d_u, const int32_t* d_v, int64_t n_pairs, int64_t n_rows, int64_t* where, int32_t* value, hipStream_t s);
std::string pair_problem_text(int64_t where, int32_t value, int64_t n_rows);
// The incidence index of checked device pairs: inc_ptr [n_rows + 1], inc [2 n_pairs] entries {p, other endpoint}, every node's in
// ascending 2p + role.  Through coo_sort / coo_fill; allocates and frees its temporaries, synchronises s.
int pair_index_build(const int32_t* d_u, const int32_t* d_v, int64_t n_pairs, int64_t n_rows, int32_t* d_inc_ptr, int2* d_inc, hipStream_t s);
struct PairFwdArgs {
    const float* x; int64_t x_stride;       // [n_rows] rows of x_stride floats, the first `width` used
    const int32_t* u; const int32_t* v;     // [n_pairs], checked
    int64_t n_pairs;
    float* q;                               // [n_pairs][width]
    int32_t width, mode;
};
int launch_pair_forward(const PairFwdArgs& a, hipStream_t s);
// gh[n][0:width] = sum over the incidences {p, other} of n of gq[p] (ADD) / gq[p] * x[other] (MUL); floats behind column `width` of a
// gh row are not touched
struct PairBwdArgs {
    const float* gq;                        // [n_pairs][width]
    const float* x; int64_t x_stride;       // MUL only (ADD: may be null)
    const int2* inc;                        // the incidence entries
    const int4* items; int64_t n_items;     // ReadoutPlan::items over the incidence row_ptr
    const int4* split; int32_t n_split;     // ReadoutPlan::split
    float* part;                            // [n_parts][width] partial rows of the segments
    float* gh; int64_t gh_stride;
    int32_t width, mode;
};
int launch_pair_backward(const PairBwdArgs& a, hipStream_t s);
// build_readout_plan over a DEVICE incidence row_ptr, without the n_rows-sized round trip: d_items / d_split receive word for word the
// host plan's lists (order, the -1 slot, partial-row numbering), only the three totals come back.  One packed count per node {split
// nodes << 32 | partial rows} in d_key [n_rows + 1], its exclusive sum in d_off [n_rows + 1] — a node's first item is
// n + partial rows before it - split nodes before it — then one fill kernel.  d_temp: pair_plan_temp_bytes(n_rows) bytes.  The lists
// must hold the upper bounds of gat_set_pairs (n_rows + 2 seg items, seg split entries).  Synchronises s.
int pair_plan_temp_bytes(int64_t n_rows, size_t* bytes);
int pair_plan_device(const int32_t* d_inc_ptr, int64_t n_rows, unsigned long long* d_key, unsigned long long* d_off, void* d_temp,
                     size_t temp_bytes, int4* d_items, int4* d_split, int64_t* n_items, int32_t* n_split, int32_t* n_parts, hipStream_t s);

// ---- hidden layer in front of the output head (gat_head_hidden.hip; the contract is in gatv2_abi.h "hidden layer") ------------------
// The two row-streaming kernels around the stage's three products (which run on launch_project_res / launch_grad_wres /
// launch_grad_x_res with rows = R, F = D_last, HD = Dh).  slope = 0: ReLU.
// a[r][j] = act(a[r][j] + b1[j]) in place, act(t) = t > 0 ? t : slope * t
int launch_head_hidden_forward(float* a, const float* b1, int64_t rows, int32_t width, float slope, hipStream_t s);
// gz[r][j] *= z1[r][j] > 0 ? 1 : slope in place; partial [blocks][width] (or null: not formed) receives the column sums of the rows each
// block walked, rows in ascending order — blocks = head_hidden_blocks(rows, width) <= kHiddenPartialRows, a function of the shape alone;
// finished by launch_reduce_partials_add
constexpr int kHiddenPartialRows = 1024;
int head_hidden_blocks(int64_t rows, int32_t width);
int launch_head_hidden_backward(float* gz, const float* z1, float* partial, int64_t rows, int32_t width, float slope, hipStream_t s);

// ---- negative sampling (gat_negsample.hip; the contract — the sampling law — is in gatv2_abi.h "negative sampling") ---------------
// *ascending = every row of the CSR has its sources in non-decreasing order (one pass, synchronises s): the sampler's membership test
// is then a binary search, else a linear scan of the row — the drawn pairs are the same either way.
int csr_rows_ascending(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, bool* ascending, hipStream_t s);
struct NegSampleArgs {
    const int32_t* row_ptr; const int32_t* col_idx; int64_t n_rows;     // rows = destinations, columns = sources (a checked CSR)
    bool ascending;                                                     // csr_rows_ascending
    int32_t mode, flags;                                                // GAT_NEG_UNIFORM | GAT_NEG_CORRUPT, GAT_NEG_* flag bits
    uint64_t seed, round;
    const int32_t* src_u; const int32_t* src_v; int64_t n_src;          // GAT_NEG_CORRUPT: the source pairs
    int32_t* u; int32_t* v; int64_t count;                              // out
    unsigned long long* unfiltered;                                     // [1] device word, ADDED to: negatives whose 16 attempts all failed
};
int launch_negative_sample(const NegSampleArgs& a, hipStream_t s);

// ---- ranking metrics (gat_rank.hip; the contract — the law — is in gatv2_abi.h "ranking metrics") -----------------------------------
// Per column of scores [n_rows][n_cols] (rows score_stride floats apart) the rank statistics of gat_rank_stats.  Exactly one of labels
// [n_rows] / targets [n_rows][n_cols] is set; mask [n_rows] may be null (every row); ks: host values, checked by rank_check.
struct RankArgs {
    const float* scores; int64_t score_stride;
    const int32_t* labels; const float* targets; const uint8_t* mask;
    int64_t n_rows; int32_t n_cols;
    const int32_t* ks; int32_t n_ks;
};
// What a call of that shape needs: slots = n_rows * n_cols keys per key buffer and prefix counts, temp_bytes for the sort and the scan,
// partial_doubles of block partials (blocks_per_col blocks of the rank kernel per column, a function of the shape alone).
struct RankSizes { int64_t slots = 0; size_t temp_bytes = 0; int32_t blocks_per_col = 0; int64_t partial_doubles = 0; };
// The call's device buffers (20 B per slot + temp + O(n_cols)): the context keeps one set for its life, the seam a Scratch.
// stats [n_cols] is where the kernels leave the result.
struct RankBuffers {
    unsigned long long* keys0 = nullptr; unsigned long long* keys1 = nullptr; uint32_t* incl = nullptr;
    void* temp = nullptr; size_t temp_bytes = 0;
    uint4* seg = nullptr; gat_rank_stats* stats = nullptr; double* partial = nullptr; int32_t* ks = nullptr;
};
// get(void** p, size_t bytes) -> int allocates one buffer
template <class Get> int rank_buffers_get(RankBuffers* b, const RankSizes& z, int32_t n_cols, Get&& get) {
    const size_t slots = (size_t)std::max<int64_t>(z.slots, 1);
    GAT_TRY(get((void**)&b->keys0, slots * sizeof(unsigned long long)));
    GAT_TRY(get((void**)&b->keys1, slots * sizeof(unsigned long long)));
    GAT_TRY(get((void**)&b->incl, slots * sizeof(uint32_t)));
    GAT_TRY(get(&b->temp, z.temp_bytes));
    b->temp_bytes = z.temp_bytes;
    GAT_TRY(get((void**)&b->seg, (size_t)n_cols * sizeof(uint4)));
    GAT_TRY(get((void**)&b->stats, (size_t)n_cols * sizeof(gat_rank_stats)));
    GAT_TRY(get((void**)&b->partial, (size_t)std::max<int64_t>(z.partial_doubles, 2) * sizeof(double)));
    GAT_TRY(get((void**)&b->ks, GAT_RANK_MAX_KS * sizeof(int32_t)));
    return 0;
}
// argument rules shared by gat_eval_rank and gat_op_rank_stats (codes of gatv2_abi.h); who: the caller's name for the text
int rank_check(const char* who, int64_t n_rows, int32_t n_cols, const int32_t* ks, int32_t n_ks);
int rank_sizes(int64_t n_rows, int32_t n_cols, RankSizes* out);
// all launches on s, no synchronisation; afterwards b.stats holds the result
int launch_rank_stats(const RankArgs& a, const RankBuffers& b, hipStream_t s);

// p[i] = the (draw0+i)-th draw of the seeded counter stream mapped to (-lim, lim]  (Xavier-uniform, E:186-248)
int launch_xavier_init(float* p, int64_t n, uint64_t s0, uint64_t draw0, float lim, hipStream_t s);
int launch_sgd(float* p, const float* g, float lr, int64_t n, hipStream_t s);
int launch_adam(float* p, const float* g, float* m, float* v, float lr, int64_t n, float b1, float b2,
                float eps, int32_t t, hipStream_t s);
// per-group clip (E:250-278) with the norm kept on the device; scratch >= 1 float
int launch_clip(float* g, int64_t n, float thresh, float* scratch, hipStream_t s);

// ---- optimizer step on the device (gat_optimizer.hip; the law is in gatv2_abi.h "optimizer") ---------------------------------------
// The block table: row b = the entries [first, first + count) of the packed buffers, all of parameter group `group`; count is at most
// kOptBlockEntries, a group of 0 entries has no row, a short group is one partial row.  group_block0 [kOptGroups + 1]: the rows of group
// k are [group_block0[k], group_block0[k + 1]) — the partials a clip norm adds, in that order.
constexpr int kOptGroups = 10;                       // GAT_PARAM_* 0 .. 9
constexpr int kOptThreads = 256;
constexpr int kOptBlockEntries = 1024;
struct OptBlock { int64_t first; int32_t count; int32_t group; };
struct OptArgs {
    float* p = nullptr; const float* g = nullptr;    // packed parameters (updated) and gradients (read only)
    float* s0 = nullptr; float* s1 = nullptr;        // state: Adam kinds m, v; SGD the momentum buffer (null: momentum = 0), -
    const OptBlock* table = nullptr; int32_t n_blocks = 0;
    int32_t group_block0[kOptGroups + 1] = {0};
    float* partial = nullptr;                        // [n_blocks] block sums of squares of g
    unsigned long long* t = nullptr;                 // step counter: opt_prepare advances it, opt_apply reads it
    const float* lr = nullptr;                       // the learning rate (gat_set_lr)
    float* norms = nullptr;                          // [kOptGroups + 1] the record of gat_optimizer_info: n_k, then the global n
    int32_t kind = 0, flags = 0, clip_mode = 0;
    float momentum = 0.f, beta1 = 0.f, beta2 = 0.f, eps = 0.f, weight_decay = 0.f, clip_threshold = 0.f;
    uint32_t decay_groups = 0;
};
void opt_build_table(const int64_t* group_off, const int64_t* group_cnt, std::vector<OptBlock>* table, int32_t* group_block0);
// opt_prepare + opt_apply on s: two launches, no synchronisation, capturable
int launch_opt_step(const OptArgs& a, hipStream_t s);
// one-lane stream-ordered writes of the device scalars
int launch_opt_set_lr(float* lr, float v, hipStream_t s);
int launch_opt_set_count(unsigned long long* t, uint64_t v, hipStream_t s);

// ---- graph construction (gat_graph.hip; the contract is in gatv2_abi.h "graph construction") ---------------------------
// coo_sort: range check + packing + sort (+ unique) of the edge keys; afterwards b->m is the edge count of the result and
// coo_fill writes row_ptr [n_rows+1] / col_idx [m].  coo_free releases the temporaries (also after a failure).
struct CooBuild {
    uint64_t* k0 = nullptr; uint64_t* k1 = nullptr; uint64_t* sorted = nullptr;   // sorted: k0 or k1
    void* temp = nullptr; size_t temp_bytes = 0;
    unsigned long long* status = nullptr;
    int64_t slots = 0, m = 0;
    int sbits = 0;
};
int coo_sort(const int32_t* d_src, const int32_t* d_dst, int64_t n_in, int64_t n_rows, int64_t n_table, int64_t table_row0,
             int32_t flags, hipStream_t s, CooBuild* b);
int coo_fill(CooBuild* b, int64_t n_rows, int32_t* d_row_ptr, int32_t* d_col_idx, hipStream_t s);
void coo_free(CooBuild* b);
// one pass over a device CSR: *problem = 0 or GAT_CSR_*, *where = lowest offending index (-1: none); synchronises s
int csr_check_device(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, int64_t n_edges, int64_t n_table,
                     int32_t* problem, int64_t* where, hipStream_t s);
const char* csr_problem_text(int32_t problem);     // the text gat_set_graph fails with for this rule

}  // namespace gat
