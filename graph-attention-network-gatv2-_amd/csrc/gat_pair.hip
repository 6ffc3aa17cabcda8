// gat_pair.hip — the pair head (gatv2_abi.h "pair head"): the head's input rows Q[p] = X[u_p] (*|+) X[v_p] of a list of node pairs, and
// the adjoint that sums the head's gradient gQ back over the nodes.
//
// Forward: a pair takes LPR lanes (float4 columns where width, strides and bases allow), the wave's other lane groups take the next
// pairs; two gathered rows in, one contiguous row out, ONE fp32 operation per entry.
// Backward: node-major pull, not a scatter.  The incidence index is a CSR over the nodes — entry {p, other} for every pair p that has
// the node as u (other = v_p) or as v (other = u_p), in ascending 2p + role — built by the COO builder of gat_graph.hip from
// dst = endpoint, src = 2p + role.  The work list is the readout's (build_readout_plan over the incidence counts): a node of at most
// kPairSegEntries incidences is one item — a node with none too, its wave writes the zero row — a longer one is cut into segments whose
// partial rows a second small kernel adds in ascending order.  ONE WAVE runs an item: LPR lanes per row, the other lane groups are entry
// slots that walk their entries in ascending order and are combined by a fixed-order xor butterfly.  No float atomics anywhere: the
// result is a function of the pair list alone, bitwise reproducible.
// pair_plan_device builds the same work list from a DEVICE incidence row_ptr (one packed count per node, one exclusive sum, one fill
// kernel; only the totals return to the host): what gat_resample_negatives uses in place of the host plan.
#include <algorithm>

#include "gat_internal.h"

#include <hipcub/hipcub.hpp>

namespace gat {

namespace {

constexpr unsigned long long kNone = ~0ull;

unsigned grid_for(int64_t work, int64_t cap = 8192) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, cap)); }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// One pass over u / v.  result = rule << 32 | index, atomicMin; one rule (1: endpoint outside [0, n_rows)), index = 2p + (0: u, 1: v),
// so the minimum is the lowest offending pair, u before v.
__global__ __launch_bounds__(256) void pair_check_kernel(const int32_t* __restrict__ u, const int32_t* __restrict__ v, int64_t n_pairs,
                                                         int64_t n_rows, unsigned long long* __restrict__ result) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned long long worst = kNone;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_pairs; p += stride) {
        const int64_t a = u[p], b = v[p];
        if (a < 0 || a >= n_rows) { worst = 1ull << 32 | (unsigned long long)(2 * p); break; }
        if (b < 0 || b >= n_rows) { worst = 1ull << 32 | (unsigned long long)(2 * p + 1); break; }
    }
    if (worst != kNone) atomicMin(result, worst);
}

// the COO builder's input: incidence i = 2p + role has dst = its endpoint, src = i
__global__ __launch_bounds__(256) void pair_keys_kernel(const int32_t* __restrict__ u, const int32_t* __restrict__ v, int64_t n_inc,
                                                        int32_t* __restrict__ src, int32_t* __restrict__ dst) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_inc; i += stride) {
        src[i] = (int32_t)i;
        dst[i] = (i & 1) ? v[i >> 1] : u[i >> 1];
    }
}
// sorted keys 2p + role -> packed entries {p, other endpoint}
__global__ __launch_bounds__(256) void pair_entries_kernel(const int32_t* __restrict__ keys, const int32_t* __restrict__ u,
                                                           const int32_t* __restrict__ v, int64_t n_inc, int2* __restrict__ inc) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_inc; i += stride) {
        const int32_t k = keys[i], p = k >> 1;
        inc[i] = make_int2(p, (k & 1) ? u[p] : v[p]);
    }
}

template <int V>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, float (&x)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
        x[0] = p[0];
    }
}
template <int V>
__device__ __forceinline__ void store_cols(float* __restrict__ p, const float (&x)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    } else {
        p[0] = x[0];
    }
}

// LPR lanes per pair (a power of two <= 64), 256 / LPR pairs per block and round; rows wider than LPR * V columns take further rounds
template <int V, bool MUL>
__global__ __launch_bounds__(256) void pair_fwd_kernel(PairFwdArgs A, int32_t LPR) {
    const int per_block = 256 / LPR, g = threadIdx.x / LPR, cl = threadIdx.x % LPR;
    const int span = LPR * V, W = A.width;
    const int64_t stride = (int64_t)gridDim.x * per_block;
    for (int64_t p = (int64_t)blockIdx.x * per_block + g; p < A.n_pairs; p += stride) {
        const int64_t a = A.u[p], b = A.v[p];
        for (int ob = 0; ob < W; ob += span) {
            const int c0 = ob + cl * V;
            if (c0 >= W) break;
            float xa[V], xb[V], q[V];
            load_cols<V>(A.x + a * A.x_stride + c0, xa);
            load_cols<V>(A.x + b * A.x_stride + c0, xb);
#pragma unroll
            for (int i = 0; i < V; ++i) q[i] = MUL ? xa[i] * xb[i] : xa[i] + xb[i];
            store_cols<V>(A.q + p * W + c0, q);
        }
    }
}

// One wave per item {node, first entry, end entry, partial row | -1}; LPR lanes of a row, 64 / LPR entry slots
template <int V, bool MUL>
__global__ __launch_bounds__(256) void pair_bwd_kernel(PairBwdArgs A, int32_t LPR) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= A.n_items) return;
    const int4 it = A.items[item];                       // uniform over the wave
    const int beg = it.y, end = it.z, slot = it.w;
    const int64_t n = it.x;
    const int slots = 64 / LPR, rs = lane / LPR, cl = lane % LPR;
    const int W = A.width, span = LPR * V;
    for (int ob = 0; ob < W; ob += span) {
        const int c0 = ob + cl * V;
        const bool own = c0 < W;
        float acc[V];
#pragma unroll
        for (int i = 0; i < V; ++i) acc[i] = 0.f;
        if (own) {
#pragma unroll 2
            for (int e = beg + rs; e < end; e += slots) {            // ascending entries per slot
                const int2 en = A.inc[e];
                float gq[V];
                load_cols<V>(A.gq + (int64_t)en.x * W + c0, gq);
                if constexpr (MUL) {
                    float xo[V];
                    load_cols<V>(A.x + (int64_t)en.y * A.x_stride + c0, xo);
#pragma unroll
                    for (int i = 0; i < V; ++i) acc[i] = fmaf(gq[i], xo[i], acc[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < V; ++i) acc[i] += gq[i];
                }
            }
        }
        for (int off = 32; off >= LPR; off >>= 1) {                  // the entry slots, fixed order (partners share cl, hence `own`)
#pragma unroll
            for (int i = 0; i < V; ++i) acc[i] += __shfl_xor(acc[i], off);
        }
        if (rs == 0 && own) {
            if (slot >= 0) store_cols<V>(A.part + (int64_t)slot * W + c0, acc);      // a segment of a long node: partial row
            else store_cols<V>(A.gh + n * A.gh_stride + c0, acc);
        }
    }
}

// split nodes {node, first partial row, partial rows, -}: one thread per (split node, column), partials in ascending order
__global__ __launch_bounds__(256) void pair_combine_kernel(PairBwdArgs A) {
    const int W = A.width;
    const int64_t total = (int64_t)A.n_split * W, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int4 sp = A.split[t / W];
        const int d = (int)(t % W);
        float acc = A.part[(int64_t)sp.y * W + d];
        for (int k = 1; k < sp.z; ++k) acc += A.part[(int64_t)(sp.y + k) * W + d];
        A.gh[(int64_t)sp.x * A.gh_stride + d] = acc;
    }
}

// ---- the work list on the device (pair_plan_device): build_readout_plan's lists from a device inc_ptr ----
// key[n] = split << 32 | partial rows of node n (0 for a node of at most kPairSegEntries incidences), key[n_rows] = 0: the exclusive sum's
// last entry then holds the totals
__global__ __launch_bounds__(256) void pair_plan_keys_kernel(const int32_t* __restrict__ inc_ptr, int64_t n_rows, unsigned long long* __restrict__ key) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n <= n_rows; n += stride) {
        unsigned long long k = 0;
        if (n < n_rows) {
            const int32_t cnt = inc_ptr[n + 1] - inc_ptr[n];
            if (cnt > kPairSegEntries) k = 1ull << 32 | (unsigned long long)((cnt + kPairSegEntries - 1) / kPairSegEntries);
        }
        key[n] = k;
    }
}
// off[n] = {split nodes, partial rows} before node n.  Items are in node order, one per short node and one per segment of a long one:
// node n's first item is n + (partial rows before) - (split nodes before).
__global__ __launch_bounds__(256) void pair_plan_fill_kernel(const int32_t* __restrict__ inc_ptr, int64_t n_rows, const unsigned long long* __restrict__ off,
                                                             int4* __restrict__ items, int4* __restrict__ split) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < n_rows; n += stride) {
        const int32_t beg = inc_ptr[n], end = inc_ptr[n + 1], cnt = end - beg;
        const unsigned long long o = off[n];
        const int32_t parts0 = (int32_t)(o & 0xffffffffull), split0 = (int32_t)(o >> 32);
        const int64_t item0 = n + parts0 - split0;
        if (cnt <= kPairSegEntries) {
            items[item0] = make_int4((int32_t)n, beg, end, -1);
            continue;
        }
        const int32_t nseg = (cnt + kPairSegEntries - 1) / kPairSegEntries;
        split[split0] = make_int4((int32_t)n, parts0, nseg, 0);
        for (int32_t k = 0; k < nseg; ++k)
            items[item0 + k] = make_int4((int32_t)n, beg + k * kPairSegEntries, min(end, beg + (k + 1) * kPairSegEntries), parts0 + k);
    }
}

bool pair_mode_ok(int32_t mode) { return mode == GAT_PAIR_MUL || mode == GAT_PAIR_ADD; }
int32_t lanes_per_row(int groups) {
    int32_t LPR = 1;
    while (LPR < groups && LPR < 64) LPR <<= 1;
    return LPR;
}

}  // namespace

int64_t pair_check_host(const int32_t* u, const int32_t* v, int64_t n_pairs, int64_t n_rows) {
    for (int64_t p = 0; p < n_pairs; ++p) {
        if (u[p] < 0 || u[p] >= n_rows) return 2 * p;
        if (v[p] < 0 || v[p] >= n_rows) return 2 * p + 1;
    }
    return -1;
}
int pair_check_device(const int32_t* d_u, const int32_t* d_v, int64_t n_pairs, int64_t n_rows, int64_t* where, int32_t* value, hipStream_t s) {
    unsigned long long* d_res = nullptr;
    unsigned long long res = kNone;
    GAT_HIP(hipMalloc((void**)&d_res, sizeof(res)));
    auto done = [&](hipError_t e, const char* what) { (void)hipFree(d_res); return e == hipSuccess ? 0 : fail((int)e, std::string(what) + ": " + hipGetErrorString(e)); };
    hipError_t e = hipMemcpyAsync(d_res, &res, sizeof(res), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return done(e, "hipMemcpyAsync");
    hipLaunchKernelGGL(pair_check_kernel, dim3(grid_for(n_pairs, 4096)), dim3(256), 0, s, d_u, d_v, n_pairs, n_rows, d_res);
    if ((e = hipGetLastError()) != hipSuccess) return done(e, "pair_check_kernel");
    if ((e = hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, s)) != hipSuccess) return done(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return done(e, "hipStreamSynchronize");
    *where = res == kNone ? -1 : (int64_t)(res & 0xffffffffull);
    if (*where >= 0 && value) {
        const int32_t* arr = (*where & 1) ? d_v : d_u;
        if ((e = hipMemcpy(value, arr + (*where >> 1), sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess) return done(e, "hipMemcpy");
    }
    return done(hipSuccess, "");
}
std::string pair_problem_text(int64_t where, int32_t value, int64_t n_rows) {
    return "pair " + std::to_string(where >> 1) + " has " + ((where & 1) ? "v " : "u ") + std::to_string(value) + " outside [0, " + std::to_string(n_rows) + ")";
}

int pair_index_build(const int32_t* d_u, const int32_t* d_v, int64_t n_pairs, int64_t n_rows, int32_t* d_inc_ptr, int2* d_inc, hipStream_t s) {
    const int64_t n_inc = 2 * n_pairs;
    Scratch tmp;
    int32_t *src = nullptr, *dst = nullptr, *keys = nullptr;
    GAT_TRY(tmp.get(&src, n_inc)); GAT_TRY(tmp.get(&dst, n_inc)); GAT_TRY(tmp.get(&keys, n_inc));
    hipLaunchKernelGGL(pair_keys_kernel, dim3(grid_for(n_inc)), dim3(256), 0, s, d_u, d_v, n_inc, src, dst);
    GAT_HIP(hipGetLastError());
    // the builder wants its rows inside its source table: a table of max(2P, n_rows) "sources" (only the key's bit width depends on it)
    CooBuild b;
    int rc = coo_sort(src, dst, n_inc, n_rows, std::max(n_inc, n_rows), 0, 0, s, &b);
    if (rc == 0 && b.m != n_inc) { coo_free(&b); rc = fail(GAT_E_STATE, "pair head: the incidence sort lost entries"); }
    if (rc == 0) rc = coo_fill(&b, n_rows, d_inc_ptr, keys, s);
    coo_free(&b);
    if (rc) { (void)hipStreamSynchronize(s); return rc; }
    hipLaunchKernelGGL(pair_entries_kernel, dim3(grid_for(n_inc)), dim3(256), 0, s, keys, d_u, d_v, n_inc, d_inc);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));                    // before the scratch is freed
    return 0;
}

int pair_plan_temp_bytes(int64_t n_rows, size_t* bytes) {
    *bytes = 0;
    GAT_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, *bytes, (unsigned long long*)nullptr, (unsigned long long*)nullptr, (int)(n_rows + 1)));
    return 0;
}
int pair_plan_device(const int32_t* d_inc_ptr, int64_t n_rows, unsigned long long* d_key, unsigned long long* d_off, void* d_temp,
                     size_t temp_bytes, int4* d_items, int4* d_split, int64_t* n_items, int32_t* n_split, int32_t* n_parts, hipStream_t s) {
    hipLaunchKernelGGL(pair_plan_keys_kernel, dim3(grid_for(n_rows + 1)), dim3(256), 0, s, d_inc_ptr, n_rows, d_key);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipcub::DeviceScan::ExclusiveSum(d_temp, temp_bytes, d_key, d_off, (int)(n_rows + 1), s));
    hipLaunchKernelGGL(pair_plan_fill_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s, d_inc_ptr, n_rows, d_off, d_items, d_split);
    GAT_HIP(hipGetLastError());
    unsigned long long total = 0;                        // off[n_rows]: the only words that return to the host
    GAT_HIP(hipMemcpyAsync(&total, d_off + n_rows, sizeof(total), hipMemcpyDeviceToHost, s));
    GAT_HIP(hipStreamSynchronize(s));
    *n_parts = (int32_t)(total & 0xffffffffull);
    *n_split = (int32_t)(total >> 32);
    *n_items = n_rows + *n_parts - *n_split;
    return 0;
}

int launch_pair_forward(const PairFwdArgs& a, hipStream_t s) {
    if (!pair_mode_ok(a.mode)) return fail(GAT_E_INVALID, "pair head: mode must be GAT_PAIR_MUL or GAT_PAIR_ADD");
    if (a.width < 1 || a.x_stride < a.width) return fail(GAT_E_INVALID, "pair head: width must be >= 1 and the row stride >= width");
    if (!a.x || !a.u || !a.v || !a.q) return fail(GAT_E_INVALID, "pair head: null argument");
    if (a.n_pairs <= 0) return 0;
    const bool v4 = a.width % 4 == 0 && a.x_stride % 4 == 0 && aligned16(a.x) && aligned16(a.q);
    const int32_t LPR = lanes_per_row(v4 ? a.width / 4 : a.width);
    const dim3 grid(grid_for(a.n_pairs * LPR, 16384)), block(256);
    const bool mul = a.mode == GAT_PAIR_MUL;
    if (v4) {
        if (mul) hipLaunchKernelGGL((pair_fwd_kernel<4, true>), grid, block, 0, s, a, LPR);
        else hipLaunchKernelGGL((pair_fwd_kernel<4, false>), grid, block, 0, s, a, LPR);
    } else {
        if (mul) hipLaunchKernelGGL((pair_fwd_kernel<1, true>), grid, block, 0, s, a, LPR);
        else hipLaunchKernelGGL((pair_fwd_kernel<1, false>), grid, block, 0, s, a, LPR);
    }
    GAT_HIP(hipGetLastError());
    return 0;
}

int launch_pair_backward(const PairBwdArgs& a, hipStream_t s) {
    if (!pair_mode_ok(a.mode)) return fail(GAT_E_INVALID, "pair head: mode must be GAT_PAIR_MUL or GAT_PAIR_ADD");
    if (a.width < 1 || a.gh_stride < a.width) return fail(GAT_E_INVALID, "pair head: width must be >= 1 and the row stride >= width");
    const bool mul = a.mode == GAT_PAIR_MUL;
    if (mul && a.x_stride < a.width) return fail(GAT_E_INVALID, "pair head: width must be >= 1 and the row stride >= width");
    if (!a.gq || !a.inc || !a.items || !a.gh || (mul && !a.x)) return fail(GAT_E_INVALID, "pair head: null argument");
    if (a.n_split > 0 && (!a.split || !a.part)) return fail(GAT_E_INVALID, "pair head: null partial buffer");
    if (a.n_items <= 0) return 0;
    const bool v4 = a.width % 4 == 0 && a.gh_stride % 4 == 0 && aligned16(a.gh) && aligned16(a.gq) && (!mul || (a.x_stride % 4 == 0 && aligned16(a.x))) &&
                    (a.n_split == 0 || aligned16(a.part));
    const int32_t LPR = lanes_per_row(v4 ? a.width / 4 : a.width);
    const dim3 grid((unsigned)((a.n_items + 3) / 4)), block(256);
    if (v4) {
        if (mul) hipLaunchKernelGGL((pair_bwd_kernel<4, true>), grid, block, 0, s, a, LPR);
        else hipLaunchKernelGGL((pair_bwd_kernel<4, false>), grid, block, 0, s, a, LPR);
    } else {
        if (mul) hipLaunchKernelGGL((pair_bwd_kernel<1, true>), grid, block, 0, s, a, LPR);
        else hipLaunchKernelGGL((pair_bwd_kernel<1, false>), grid, block, 0, s, a, LPR);
    }
    GAT_HIP(hipGetLastError());
    if (a.n_split > 0) {
        hipLaunchKernelGGL(pair_combine_kernel, dim3(grid_for((int64_t)a.n_split * a.width)), dim3(256), 0, s, a);
        GAT_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace gat
