// gat_readout.hip — graph-level readout (gatv2_abi.h "graph-level readout"): per-graph sum / mean / max pooling of the last layer's
// output rows in front of the output head, and the spread of the head's gradient back over the rows behind it.
//
// Forward: the rows of a graph are one contiguous block of X, so the pooling is a streamed column reduction.  The work list
// (build_readout_plan) holds one item per graph of at most kReadoutSegRows rows and one per kReadoutSegRows-row segment of a longer
// graph; ONE WAVE runs an item.  With a width that is a multiple of 4 a row takes width/4 lanes (float4 loads) and the wave's other
// lanes take the next rows of the item ("row slots"); each lane accumulates its slot's rows in ascending order, then the slots are
// combined by a fixed-order xor butterfly.  A whole graph writes P (and argmax) itself; segments write partial rows that a second small
// kernel combines in ascending segment order.  No float atomics anywhere: results are bitwise reproducible.
// MAX ties go to the LOWEST row: value and row travel as one ordered 64-bit key (max_key below) through every step.
// Backward: one N-sized elementwise kernel, row n -> its graph through node_graph [N].
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "gat_internal.h"

namespace gat {

namespace {

constexpr unsigned long long kNone = ~0ull;

// One pass over a device graph_ptr.  result = rule << 32 | index, atomicMin: the lowest rule in the order of the host path's checks
// (1 graph_ptr[0] != 0, 2 graph_ptr[n_graphs] != n_rows, 3 decreasing), then the lowest index.
__global__ __launch_bounds__(256) void graph_ptr_check_kernel(const int32_t* __restrict__ gp, int64_t n_graphs, int64_t n_rows,
                                                              unsigned long long* __restrict__ result) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long worst = kNone;
    if (t0 == 0) {
        if (gp[0] != 0) worst = 1ull << 32;
        else if ((int64_t)gp[n_graphs] != n_rows) worst = 2ull << 32 | (unsigned long long)n_graphs;
    }
    for (int64_t i = t0; i < n_graphs; i += stride)
        if (gp[i + 1] < gp[i]) { worst = min(worst, 3ull << 32 | (unsigned long long)i); break; }
    if (worst != kNone) atomicMin(result, worst);
}

// node_graph[n] = the graph g with graph_ptr[g] <= n < graph_ptr[g+1] (empty graphs own no row): the last g with graph_ptr[g] <= n
__global__ __launch_bounds__(256) void node_graph_kernel(const int32_t* __restrict__ gp, int64_t n_graphs, int64_t n_rows,
                                                         int32_t* __restrict__ node_graph) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < n_rows; n += stride) {
        int64_t lo = 0, hi = n_graphs;               // invariant: gp[lo] <= n < gp[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)gp[mid] <= n) lo = mid; else hi = mid;
        }
        node_graph[n] = (int32_t)lo;
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
template <int V, class T>
__device__ __forceinline__ void store_cols(T* __restrict__ p, const T (&x)[V]) {
    if constexpr (V == 4) {
        using T4 = typename std::conditional<std::is_same<T, float>::value, float4, int4>::type;
        T4 t; t.x = x[0]; t.y = x[1]; t.z = x[2]; t.w = x[3];
        *reinterpret_cast<T4*>(p) = t;
    } else {
        p[0] = x[0];
    }
}

// GAT_READOUT_MAX carries (value, row) as ONE 64-bit key whose unsigned order is "larger value first, then lower row": the float's
// bits made order-preserving in the high word, 0x7FFFFFFF - row in the low word.  Every step of the reduction — a lane's rows, the
// butterfly over the row slots, the segments of a long graph — is then a plain max of keys: associative and commutative, so the
// lowest-row rule holds whatever the order.  0 is "no row yet" (a row's low word is never 0: rows stay below 2^31 - 1).
__device__ __forceinline__ unsigned long long max_key(float v, int32_t row) {
    uint32_t u = __float_as_uint(v);
    u ^= (u >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return ((unsigned long long)u << 32) | (uint32_t)(0x7FFFFFFF - row);
}
__device__ __forceinline__ float key_value(unsigned long long k) {
    uint32_t u = (uint32_t)(k >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    return __uint_as_float(u);
}
__device__ __forceinline__ int32_t key_row(unsigned long long k) { return k ? 0x7FFFFFFF - (int32_t)(uint32_t)k : -1; }
__device__ __forceinline__ unsigned long long shfl_xor_key(unsigned long long k, int off) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), off);
    return ((unsigned long long)hi << 32) | lo;
}

// One wave per item {graph, first row, end row, partial row | -1}.  LPR: lanes of a row (a power of two <= 64); 64 / LPR row slots.
// Rows wider than LPR * V columns are walked in rounds (each round a pass over the item's rows).
template <int V, bool MAX>
__global__ __launch_bounds__(256) void readout_fwd_kernel(ReadoutFwdArgs A, int32_t LPR) {
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (item >= A.n_items) return;
    const int4 it = A.items[item];                       // uniform over the wave
    const int g = it.x, beg = it.y, end = it.z, slot = it.w;
    const int slots = 64 / LPR, rs = lane / LPR, cl = lane % LPR;
    const int DL = A.width;
    const int span = LPR * V;
    for (int ob = 0; ob < DL; ob += span) {
        const int c0 = ob + cl * V;
        const bool own = c0 < DL;
        float acc[V]; unsigned long long key[V];
#pragma unroll
        for (int i = 0; i < V; ++i) { acc[i] = 0.f; key[i] = 0; }
        if (own) {
#pragma unroll 4
            for (int r = beg + rs; r < end; r += slots) {            // ascending rows per lane
                float x[V];
                load_cols<V>(A.x + (int64_t)r * A.x_stride + c0, x);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if constexpr (MAX) key[i] = max(key[i], max_key(x[i], r));
                    else acc[i] += x[i];
                }
            }
        }
        for (int off = 32; off >= LPR; off >>= 1) {                  // the row slots, fixed order (partners share cl, hence `own`)
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if constexpr (MAX) key[i] = max(key[i], shfl_xor_key(key[i], off));
                else acc[i] += __shfl_xor(acc[i], off);
            }
        }
        if (rs == 0 && own) {
            int32_t arg[V];
            if constexpr (MAX) {
#pragma unroll
                for (int i = 0; i < V; ++i) { arg[i] = key_row(key[i]); acc[i] = key[i] ? key_value(key[i]) : 0.f; }
            }
            if (slot >= 0) {                                         // a segment of a long graph: partial row
                store_cols<V, float>(A.part + (int64_t)slot * DL + c0, acc);
                if constexpr (MAX) store_cols<V, int32_t>(A.part_arg + (int64_t)slot * DL + c0, arg);
            } else {
                const int cnt = end - beg;
                float out[V];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    if constexpr (MAX) out[i] = acc[i];                       // (0 for an empty graph, argmax -1)
                    else out[i] = cnt == 0 ? 0.f : (A.mode == GAT_READOUT_MEAN ? acc[i] / (float)cnt : acc[i]);
                }
                store_cols<V, float>(A.pooled + (int64_t)g * DL + c0, out);
                if constexpr (MAX) store_cols<V, int32_t>(A.argmax + (int64_t)g * DL + c0, arg);
            }
        }
    }
}

// split graphs {graph, first partial row, partial rows, -}: one thread per (split graph, column), partials in ascending order
__global__ __launch_bounds__(256) void readout_combine_kernel(ReadoutFwdArgs A) {
    const int DL = A.width;
    const int64_t total = (int64_t)A.n_split * DL, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int4 sp = A.split[t / DL];
        const int d = (int)(t % DL);
        const int64_t o = (int64_t)sp.x * DL + d;
        float acc = A.part[(int64_t)sp.y * DL + d];
        if (A.mode == GAT_READOUT_MAX) {
            unsigned long long key = 0;                  // (a segment always has rows)
            for (int k = 0; k < sp.z; ++k) key = max(key, max_key(A.part[(int64_t)(sp.y + k) * DL + d], A.part_arg[(int64_t)(sp.y + k) * DL + d]));
            A.pooled[o] = key_value(key); A.argmax[o] = key_row(key);
        } else {
            for (int k = 1; k < sp.z; ++k) acc += A.part[(int64_t)(sp.y + k) * DL + d];
            if (A.mode == GAT_READOUT_MEAN) acc = acc / (float)(A.graph_ptr[sp.x + 1] - A.graph_ptr[sp.x]);
            A.pooled[o] = acc;
        }
    }
}

// gH[n][c] of every row and every column c < width; V columns per thread
template <int V>
__global__ __launch_bounds__(256) void readout_bwd_kernel(ReadoutBwdArgs A) {
    const int DL = A.width, groups = DL / V;
    const int64_t total = A.n_rows * groups, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t n = t / groups;
        const int c0 = (int)(t % groups) * V;
        const int g = A.node_graph[n];
        float gp[V], out[V];
        load_cols<V>(A.gpooled + (int64_t)g * DL + c0, gp);
        if (A.mode == GAT_READOUT_MAX) {
#pragma unroll
            for (int i = 0; i < V; ++i) out[i] = (int64_t)A.argmax[(int64_t)g * DL + c0 + i] == n ? gp[i] : 0.f;
        } else if (A.mode == GAT_READOUT_MEAN) {
            const float cnt = (float)(A.graph_ptr[g + 1] - A.graph_ptr[g]);
#pragma unroll
            for (int i = 0; i < V; ++i) out[i] = gp[i] / cnt;
        } else {
#pragma unroll
            for (int i = 0; i < V; ++i) out[i] = gp[i];
        }
        store_cols<V, float>(A.gh + n * A.gh_stride + c0, out);
    }
}

unsigned grid_for(int64_t work, int64_t cap = 8192) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, cap)); }
bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int graph_ptr_check_device(const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t* problem, int64_t* where, hipStream_t s) {
    unsigned long long* d_res = nullptr;
    unsigned long long res = kNone;
    GAT_HIP(hipMalloc((void**)&d_res, sizeof(res)));
    auto done = [&](hipError_t e, const char* what) { (void)hipFree(d_res); return e == hipSuccess ? 0 : fail((int)e, std::string(what) + ": " + hipGetErrorString(e)); };
    hipError_t e = hipMemcpyAsync(d_res, &res, sizeof(res), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return done(e, "hipMemcpyAsync");
    hipLaunchKernelGGL(graph_ptr_check_kernel, dim3(grid_for(n_graphs, 4096)), dim3(256), 0, s, d_graph_ptr, n_graphs, n_rows, d_res);
    if ((e = hipGetLastError()) != hipSuccess) return done(e, "graph_ptr_check_kernel");
    if ((e = hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, s)) != hipSuccess) return done(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return done(e, "hipStreamSynchronize");
    *problem = res == kNone ? 0 : (int32_t)(res >> 32);
    *where = res == kNone ? -1 : (int64_t)(res & 0xffffffffull);
    return done(hipSuccess, "");
}
int graph_ptr_check_host(const int32_t* gp, int64_t n_graphs, int64_t n_rows, int32_t* problem, int64_t* where) {
    *problem = 0; *where = -1;
    if (gp[0] != 0) { *problem = 1; *where = 0; return 0; }
    if ((int64_t)gp[n_graphs] != n_rows) { *problem = 2; *where = n_graphs; return 0; }
    for (int64_t i = 0; i < n_graphs; ++i)
        if (gp[i + 1] < gp[i]) { *problem = 3; *where = i; return 0; }
    return 0;
}
std::string graph_ptr_problem_text(int32_t problem, int64_t where, int64_t n_rows) {
    switch (problem) {
        case 1: return "Invalid graph_ptr: entry 0 must be 0";
        case 2: return "Invalid graph_ptr: entry " + std::to_string(where) + " (the last) must be the row count " + std::to_string(n_rows);
        case 3: return "Invalid graph_ptr: decreases behind entry " + std::to_string(where);
        default: return "";
    }
}

void build_readout_plan(const int32_t* gp, int64_t n_graphs, ReadoutPlan& p) {
    p = ReadoutPlan{};
    for (int64_t g = 0; g < n_graphs; ++g) {
        const int32_t beg = gp[g], end = gp[g + 1], cnt = end - beg;
        if (cnt <= kReadoutSegRows) {                    // (an empty graph is an item too: its wave writes the zeros and argmax -1)
            p.items.insert(p.items.end(), {(int32_t)g, beg, end, -1});
            continue;
        }
        const int32_t nseg = (cnt + kReadoutSegRows - 1) / kReadoutSegRows;
        p.split.insert(p.split.end(), {(int32_t)g, p.n_parts, nseg, 0});
        for (int32_t k = 0; k < nseg; ++k)
            p.items.insert(p.items.end(), {(int32_t)g, beg + k * kReadoutSegRows, std::min(end, beg + (k + 1) * kReadoutSegRows), p.n_parts + k});
        p.n_parts += nseg;
    }
    p.n_items = (int64_t)(p.items.size() / 4);
    p.n_split = (int32_t)(p.split.size() / 4);
}

int launch_node_graph(const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t* d_node_graph, hipStream_t s) {
    if (n_rows <= 0) return 0;
    hipLaunchKernelGGL(node_graph_kernel, dim3(grid_for(n_rows)), dim3(256), 0, s, d_graph_ptr, n_graphs, n_rows, d_node_graph);
    GAT_HIP(hipGetLastError());
    return 0;
}

static bool readout_mode_ok(int32_t mode) { return mode == GAT_READOUT_MEAN || mode == GAT_READOUT_SUM || mode == GAT_READOUT_MAX; }

int launch_readout_forward(const ReadoutFwdArgs& a, hipStream_t s) {
    if (!readout_mode_ok(a.mode)) return fail(GAT_E_INVALID, "readout: mode must be GAT_READOUT_MEAN, _SUM or _MAX");
    if (a.width < 1 || a.x_stride < a.width) return fail(GAT_E_INVALID, "readout: width must be >= 1 and the row stride >= width");
    if (!a.x || !a.items || !a.pooled || !a.graph_ptr || (a.mode == GAT_READOUT_MAX && !a.argmax)) return fail(GAT_E_INVALID, "readout: null argument");
    if (a.n_split > 0 && (!a.split || !a.part || (a.mode == GAT_READOUT_MAX && !a.part_arg))) return fail(GAT_E_INVALID, "readout: null partial buffer");
    if (a.n_items <= 0) return 0;
    const bool max = a.mode == GAT_READOUT_MAX;
    // float4 columns: every address base + row * stride + 4k must be 16-byte aligned, on the input and on every output
    const bool v4 = a.width % 4 == 0 && a.x_stride % 4 == 0 && aligned16(a.x) && aligned16(a.pooled) && (!max || aligned16(a.argmax)) &&
                    (a.n_split == 0 || (aligned16(a.part) && (!max || aligned16(a.part_arg))));
    const int groups = v4 ? a.width / 4 : a.width;
    int32_t LPR = 1;
    while (LPR < groups && LPR < 64) LPR <<= 1;
    const dim3 grid((unsigned)((a.n_items + 3) / 4)), block(256);
    if (v4) {
        if (max) hipLaunchKernelGGL((readout_fwd_kernel<4, true>), grid, block, 0, s, a, LPR);
        else hipLaunchKernelGGL((readout_fwd_kernel<4, false>), grid, block, 0, s, a, LPR);
    } else {
        if (max) hipLaunchKernelGGL((readout_fwd_kernel<1, true>), grid, block, 0, s, a, LPR);
        else hipLaunchKernelGGL((readout_fwd_kernel<1, false>), grid, block, 0, s, a, LPR);
    }
    GAT_HIP(hipGetLastError());
    if (a.n_split > 0) {
        hipLaunchKernelGGL(readout_combine_kernel, dim3(grid_for((int64_t)a.n_split * a.width)), dim3(256), 0, s, a);
        GAT_HIP(hipGetLastError());
    }
    return 0;
}

int launch_readout_backward(const ReadoutBwdArgs& a, hipStream_t s) {
    if (!readout_mode_ok(a.mode)) return fail(GAT_E_INVALID, "readout: mode must be GAT_READOUT_MEAN, _SUM or _MAX");
    if (a.width < 1 || a.gh_stride < a.width) return fail(GAT_E_INVALID, "readout: width must be >= 1 and the row stride >= width");
    if (!a.gpooled || !a.node_graph || !a.graph_ptr || !a.gh || (a.mode == GAT_READOUT_MAX && !a.argmax)) return fail(GAT_E_INVALID, "readout: null argument");
    if (a.n_rows <= 0) return 0;
    const bool v4 = a.width % 4 == 0 && a.gh_stride % 4 == 0 && aligned16(a.gh) && aligned16(a.gpooled);
    const int64_t work = a.n_rows * (v4 ? a.width / 4 : a.width);
    if (v4) hipLaunchKernelGGL(readout_bwd_kernel<4>, dim3(grid_for(work)), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(readout_bwd_kernel<1>, dim3(grid_for(work)), dim3(256), 0, s, a);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
