// gat_graph.hip — the training graph built ON the device from an edge list, and the one-pass check of a device CSR
// (include/gatv2_abi.h "graph construction").  The reference reads a finished CSR only (README "Graph Data Handling");
// nothing here replaces a reference launch.
//
// Builder.  One 64-bit key per intermediate edge, key = dst << sbits | src (sbits = bits of n_table - 1), so that ONE
// radix sort over sbits + dbits bits yields rows = destinations with ascending sources inside a row:
//   1. pack_kernel      slot i            <- key(src[i], dst[i])            (dropped: an existing self-loop with SELF_LOOPS)
//                       slot n_in + i     <- key(dst[i], src[i])            (SYMMETRIZE; dropped for src == dst)
//                       slot base + r     <- key(table_row0 + r, r)         (SELF_LOOPS)
//                       a dropped slot takes the sentinel n_rows << sbits, which sorts behind every real key; the range
//                       check of the input rides in the same pass (atomicMin on the lowest offending edge index)
//   2. hipcub::DeviceRadixSort::SortKeys over the slots, ping-pong between the two key buffers
//   3. hipcub::DeviceSelect::Unique       (COALESCE) into the other key buffer
//   4. fill_kernel      col_idx[i] = key & mask; row_ptr[r] = first i whose dst >= r  (every thread writes the row
//                       pointers of the gap between its predecessor's row and its own; thread m closes the tail)
// Temporary memory: two key buffers of 8 B x slots plus hipcub's scratch (a few MB); freed before return.
#include "gat_internal.h"

#include <hipcub/hipcub.hpp>

namespace gat {
namespace {

constexpr unsigned long long kNone = ~0ull;

int grid_for(int64_t n, int64_t cap = 16384) { return (int)std::min<int64_t>(std::max<int64_t>((n + 255) / 256, 1), cap); }

// status[0]: lowest edge index with src or dst out of range (kNone: all fine); status[1]: slots that took the sentinel
__global__ __launch_bounds__(256) void pack_kernel(const int32_t* __restrict__ src, const int32_t* __restrict__ dst, int64_t n_in,
                                                   int64_t n_rows, int64_t n_table, int64_t table_row0, int32_t flags, int sbits,
                                                   uint64_t* __restrict__ keys, unsigned long long* __restrict__ status) {
    const bool loops = flags & GAT_GRAPH_SELF_LOOPS, sym = flags & GAT_GRAPH_SYMMETRIZE;
    const uint64_t sentinel = (uint64_t)n_rows << sbits;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long bad = kNone, dropped = 0;
    for (int64_t i = t0; i < n_in; i += stride) {
        const int64_t s = src[i], d = dst[i];
        const bool ok = s >= 0 && s < n_table && d >= 0 && d < n_rows;
        if (!ok && bad == kNone) bad = (unsigned long long)i;
        const bool loop = s == table_row0 + d;
        const bool keep = ok && !(loops && loop);
        keys[i] = keep ? ((uint64_t)d << sbits | (uint64_t)s) : sentinel;
        dropped += keep ? 0 : 1;
        if (sym) {                                       // n_table == n_rows, table_row0 == 0 (checked by the caller)
            const bool keep_r = ok && !loop;
            keys[n_in + i] = keep_r ? ((uint64_t)s << sbits | (uint64_t)d) : sentinel;
            dropped += keep_r ? 0 : 1;
        }
    }
    if (loops) {
        const int64_t base = sym ? 2 * n_in : n_in;
        for (int64_t r = t0; r < n_rows; r += stride) keys[base + r] = (uint64_t)r << sbits | (uint64_t)(table_row0 + r);
    }
    if (bad != kNone) atomicMin(&status[0], bad);
    for (int off = 32; off > 0; off >>= 1) dropped += __shfl_xor(dropped, off);
    if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&status[1], dropped);
}

// keys[0, m) sorted, real; i == m stands for the end (row n_rows)
__global__ __launch_bounds__(256) void fill_kernel(const uint64_t* __restrict__ keys, int64_t m, int64_t n_rows, int sbits,
                                                   int32_t* __restrict__ row_ptr, int32_t* __restrict__ col_idx) {
    const uint64_t mask = ((uint64_t)1 << sbits) - 1;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= m; i += stride) {
        int64_t d = n_rows;
        if (i < m) {
            const uint64_t k = keys[i];
            col_idx[i] = (int32_t)(k & mask);
            d = (int64_t)(k >> sbits);
        }
        const int64_t dprev = i > 0 ? (int64_t)(keys[i - 1] >> sbits) : -1;
        for (int64_t r = dprev + 1; r <= d; ++r) row_ptr[r] = (int32_t)i;
    }
}

// One pass over a device CSR.  result = rule << 32 | index, atomicMin: the lowest rule in the order of the host path's checks
// (1 row_ptr[0] != 0, 2 row_ptr[n_rows] != n_edges, 3 not monotone, 4 col_idx outside the table), then the lowest index.
__global__ __launch_bounds__(256) void csr_check_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx,
                                                        int64_t n_rows, int64_t n_edges, int64_t n_table,
                                                        unsigned long long* __restrict__ result) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long worst = kNone;
    if (t0 == 0) {
        if (row_ptr[0] != 0) worst = 1ull << 32;
        else if ((int64_t)row_ptr[n_rows] != n_edges) worst = 2ull << 32 | (unsigned long long)n_rows;
    }
    for (int64_t i = t0; i < n_rows; i += stride)
        if (row_ptr[i + 1] < row_ptr[i]) { worst = min(worst, 3ull << 32 | (unsigned long long)i); break; }
    for (int64_t e = t0; e < n_edges; e += stride) {
        const int64_t v = col_idx[e];
        if (v < 0 || v >= n_table) { worst = min(worst, 4ull << 32 | (unsigned long long)e); break; }
    }
    if (worst != kNone) atomicMin(result, worst);
}

int bits_for(int64_t max_value) {       // bits needed to hold values 0 .. max_value
    int b = 1;
    while (b < 63 && ((int64_t)1 << b) <= max_value) ++b;
    return b;
}

}  // namespace

void coo_free(CooBuild* b) {
    (void)hipFree(b->k0); (void)hipFree(b->k1); (void)hipFree(b->temp); (void)hipFree(b->status);
    *b = CooBuild{};
}

#define COO_HIP(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { coo_free(b); return fail((int)e__, std::string(#x) + ": " + hipGetErrorString(e__)); } } while (0)

int coo_sort(const int32_t* d_src, const int32_t* d_dst, int64_t n_in, int64_t n_rows, int64_t n_table, int64_t table_row0,
             int32_t flags, hipStream_t s, CooBuild* b) {
    *b = CooBuild{};
    if ((!d_src || !d_dst) && n_in > 0) return fail(GAT_E_INVALID, "gat_graph_from_coo: null argument");
    if (flags & ~(GAT_GRAPH_SELF_LOOPS | GAT_GRAPH_SYMMETRIZE | GAT_GRAPH_COALESCE)) return fail(GAT_E_INVALID, "gat_graph_from_coo: unknown flag bit");
    if (n_in < 0 || n_rows <= 0) return fail(GAT_E_INVALID, "gat_graph_from_coo: bad sizes");
    if (n_rows >= 0x7fffffffLL || n_table > 0x7fffffffLL) return fail(GAT_E_UNSUPPORTED, "gat_graph_from_coo: int32 CSR limits exceeded");
    if (table_row0 < 0 || table_row0 + n_rows > n_table) return fail(GAT_E_INVALID, "gat_graph_from_coo: shard rows outside the table");
    if ((flags & GAT_GRAPH_SYMMETRIZE) && (n_table != n_rows || table_row0 != 0))
        return fail(GAT_E_UNSUPPORTED, "gat_graph_from_coo: GAT_GRAPH_SYMMETRIZE needs the whole graph (n_table == n_rows, table_row0 == 0): symmetrize first, then shard");
    const int64_t slots = n_in * ((flags & GAT_GRAPH_SYMMETRIZE) ? 2 : 1) + ((flags & GAT_GRAPH_SELF_LOOPS) ? n_rows : 0);
    if (n_in > 0x7fffffffLL || slots > 0x7fffffffLL)
        return fail(GAT_E_UNSUPPORTED, "gat_graph_from_coo: " + std::to_string(slots) + " intermediate edges exceed the 32-bit count of the sort");
    b->sbits = bits_for(n_table - 1);
    b->slots = slots;
    if (slots == 0) return 0;
    const int end_bit = b->sbits + bits_for(n_rows);      // the sentinel's dst is n_rows
    COO_HIP(hipMalloc((void**)&b->k0, slots * sizeof(uint64_t)));
    COO_HIP(hipMalloc((void**)&b->k1, slots * sizeof(uint64_t)));
    COO_HIP(hipMalloc((void**)&b->status, 3 * sizeof(unsigned long long)));
    const unsigned long long init[3] = {kNone, 0, 0};
    COO_HIP(hipMemcpyAsync(b->status, init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for(std::max(n_in, n_rows))), dim3(256), 0, s, d_src, d_dst, n_in, n_rows, n_table,
                       table_row0, flags, b->sbits, b->k0, b->status);
    COO_HIP(hipGetLastError());
    unsigned long long st[3];
    COO_HIP(hipMemcpyAsync(st, b->status, sizeof(st), hipMemcpyDeviceToHost, s));
    COO_HIP(hipStreamSynchronize(s));
    if (st[0] != kNone) {
        int32_t bs = 0, bd = 0;
        COO_HIP(hipMemcpy(&bs, d_src + st[0], sizeof(int32_t), hipMemcpyDeviceToHost));
        COO_HIP(hipMemcpy(&bd, d_dst + st[0], sizeof(int32_t), hipMemcpyDeviceToHost));
        coo_free(b);
        const bool src_bad = bs < 0 || bs >= n_table;
        return fail(GAT_E_INVALID, "gat_graph_from_coo: edge " + std::to_string(st[0]) + " has " + (src_bad ? "src " + std::to_string(bs) +
                    " outside [0, " + std::to_string(n_table) + ")" : "dst " + std::to_string(bd) + " outside [0, " + std::to_string(n_rows) + ")"));
    }
    const int64_t real = slots - (int64_t)st[1];
    // in place over the two key buffers (DoubleBuffer): the sort then needs no third buffer of keys
    hipcub::DoubleBuffer<uint64_t> keys(b->k0, b->k1);
    size_t temp_bytes = 0, unique_bytes = 0;
    COO_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, temp_bytes, keys, (int)slots, 0, end_bit, s));
    if (flags & GAT_GRAPH_COALESCE)
        COO_HIP(hipcub::DeviceSelect::Unique(nullptr, unique_bytes, b->k1, b->k0, (int64_t*)nullptr, (int)slots, s));
    b->temp_bytes = std::max(temp_bytes, unique_bytes);
    COO_HIP(hipMalloc(&b->temp, std::max<size_t>(b->temp_bytes, 8)));
    COO_HIP(hipcub::DeviceRadixSort::SortKeys(b->temp, temp_bytes, keys, (int)slots, 0, end_bit, s));
    b->sorted = keys.Current();
    b->m = real;
    if (flags & GAT_GRAPH_COALESCE) {
        uint64_t* uniq = keys.Alternate();
        int64_t* d_sel = (int64_t*)(b->status + 2);
        COO_HIP(hipcub::DeviceSelect::Unique(b->temp, unique_bytes, b->sorted, uniq, d_sel, (int)slots, s));
        int64_t sel = 0;
        COO_HIP(hipMemcpyAsync(&sel, d_sel, sizeof(sel), hipMemcpyDeviceToHost, s));
        COO_HIP(hipStreamSynchronize(s));
        b->m = sel - (st[1] ? 1 : 0);                    // the sentinels collapse into one trailing entry
        b->sorted = uniq;
    }
    return 0;
}

int coo_fill(CooBuild* b, int64_t n_rows, int32_t* d_row_ptr, int32_t* d_col_idx, hipStream_t s) {
    hipLaunchKernelGGL(fill_kernel, dim3(grid_for(b->m + 1)), dim3(256), 0, s, b->sorted, b->m, n_rows, b->sbits, d_row_ptr, d_col_idx);
    COO_HIP(hipGetLastError());
    COO_HIP(hipStreamSynchronize(s));
    return 0;
}
#undef COO_HIP

int csr_check_device(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, int64_t n_edges, int64_t n_table,
                     int32_t* problem, int64_t* where, hipStream_t s) {
    unsigned long long* d_res = nullptr;
    unsigned long long res = kNone;
    GAT_HIP(hipMalloc((void**)&d_res, sizeof(res)));
    auto done = [&](hipError_t e, const char* what) { (void)hipFree(d_res); return e == hipSuccess ? 0 : fail((int)e, std::string(what) + ": " + hipGetErrorString(e)); };
    hipError_t e = hipMemcpyAsync(d_res, &res, sizeof(res), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return done(e, "hipMemcpyAsync");
    hipLaunchKernelGGL(csr_check_kernel, dim3(grid_for(std::max(n_rows, n_edges), 4096)), dim3(256), 0, s, d_row_ptr, d_col_idx, n_rows,
                       n_edges, n_table, d_res);
    if ((e = hipGetLastError()) != hipSuccess) return done(e, "csr_check_kernel");
    if ((e = hipMemcpyAsync(&res, d_res, sizeof(res), hipMemcpyDeviceToHost, s)) != hipSuccess) return done(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return done(e, "hipStreamSynchronize");
    *problem = res == kNone ? 0 : (int32_t)(res >> 32);
    *where = res == kNone ? -1 : (int64_t)(res & 0xffffffffull);
    return done(hipSuccess, "");
}

const char* csr_problem_text(int32_t problem) {
    switch (problem) {
        case GAT_CSR_BAD_START: case GAT_CSR_BAD_END: return "Invalid row_ptr: must start at 0 and end at the edge count";
        case GAT_CSR_NOT_MONOTONE: return "Invalid row_ptr: not monotone";
        case GAT_CSR_COL_RANGE: return "col_idx entry outside the node table";
        default: return "";
    }
}

}  // namespace gat

using namespace gat;

extern "C" {

int gat_graph_check_device(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, int64_t n_edges, int64_t n_table,
                           int32_t* problem, int64_t* where, void* stream) {
    if (!d_row_ptr || (!d_col_idx && n_edges > 0) || !problem) return fail(GAT_E_INVALID, "gat_graph_check_device: null argument");
    if (n_rows <= 0 || n_edges < 0 || n_table <= 0) return fail(GAT_E_INVALID, "gat_graph_check_device: bad sizes");
    if (n_edges > 0x7fffffffLL || n_rows >= 0x7fffffffLL || n_table > 0x7fffffffLL)
        return fail(GAT_E_UNSUPPORTED, "gat_graph_check_device: int32 CSR limits exceeded");
    int64_t w = -1;
    GAT_TRY(csr_check_device(d_row_ptr, d_col_idx, n_rows, n_edges, n_table, problem, &w, (hipStream_t)stream));
    if (where) *where = w;
    return 0;
}

int gat_graph_from_coo_device(const int32_t* d_src, const int32_t* d_dst, int64_t n_in, int64_t n_rows, int64_t n_table,
                              int64_t table_row0, int32_t flags, int32_t* d_row_ptr, int32_t* d_col_idx, int64_t col_capacity,
                              int64_t* n_edges_out, void* stream) {
    if (!n_edges_out) return fail(GAT_E_INVALID, "gat_graph_from_coo: null argument");
    if (d_col_idx && !d_row_ptr) return fail(GAT_E_INVALID, "gat_graph_from_coo: d_col_idx without d_row_ptr");
    CooBuild b;
    GAT_TRY(coo_sort(d_src, d_dst, n_in, n_rows, n_table, table_row0, flags, (hipStream_t)stream, &b));
    *n_edges_out = b.m;
    int rc = 0;
    if (d_row_ptr && (d_col_idx || b.m == 0)) {
        if (b.m > col_capacity && b.m > 0)
            rc = fail(GAT_E_INVALID, "gat_graph_from_coo: col_capacity " + std::to_string(col_capacity) + " < " + std::to_string(b.m) + " edges");
        else
            rc = coo_fill(&b, n_rows, d_row_ptr, d_col_idx, (hipStream_t)stream);
    }
    coo_free(&b);
    return rc;
}

int gat_graph_from_coo(const int32_t* src, const int32_t* dst, int64_t n_in, int64_t n_rows, int64_t n_table, int64_t table_row0,
                       int32_t flags, int32_t* row_ptr_out, int32_t* col_idx_out, int64_t col_capacity, int64_t* n_edges_out,
                       int32_t device) {
    if (!n_edges_out || ((!src || !dst) && n_in > 0)) return fail(GAT_E_INVALID, "gat_graph_from_coo: null argument");
    if (col_idx_out && !row_ptr_out) return fail(GAT_E_INVALID, "gat_graph_from_coo: col_idx_out without row_ptr_out");
    if (n_in < 0 || n_in > 0x7fffffffLL) return fail(n_in < 0 ? GAT_E_INVALID : GAT_E_UNSUPPORTED, "gat_graph_from_coo: edge count outside the 32-bit count of the sort");
    if (n_rows <= 0 || n_rows >= 0x7fffffffLL) return fail(GAT_E_INVALID, "gat_graph_from_coo: bad sizes");
    GAT_HIP(hipSetDevice(device));
    int32_t *d_src = nullptr, *d_dst = nullptr, *d_rp = nullptr, *d_ci = nullptr;
    auto cleanup = [&](int rc) { (void)hipFree(d_src); (void)hipFree(d_dst); (void)hipFree(d_rp); (void)hipFree(d_ci); return rc; };
#define G_HIP(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) return cleanup(fail((int)e__, std::string(#x) + ": " + hipGetErrorString(e__))); } while (0)
    if (n_in > 0) {
        G_HIP(hipMalloc((void**)&d_src, n_in * sizeof(int32_t)));
        G_HIP(hipMalloc((void**)&d_dst, n_in * sizeof(int32_t)));
        G_HIP(hipMemcpy(d_src, src, n_in * sizeof(int32_t), hipMemcpyHostToDevice));
        G_HIP(hipMemcpy(d_dst, dst, n_in * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    CooBuild b;
    int rc = coo_sort(d_src, d_dst, n_in, n_rows, n_table, table_row0, flags, nullptr, &b);
    if (rc) return cleanup(rc);
    (void)hipFree(d_src); (void)hipFree(d_dst); d_src = d_dst = nullptr;      // the keys hold everything from here on
    *n_edges_out = b.m;
    if (row_ptr_out && (col_idx_out || b.m == 0)) {
        if (b.m > col_capacity && b.m > 0) {
            rc = fail(GAT_E_INVALID, "gat_graph_from_coo: col_capacity " + std::to_string(col_capacity) + " < " + std::to_string(b.m) + " edges");
        } else {
            hipError_t e = hipMalloc((void**)&d_rp, (n_rows + 1) * sizeof(int32_t));
            if (e == hipSuccess) e = hipMalloc((void**)&d_ci, std::max<int64_t>(b.m, 1) * sizeof(int32_t));
            if (e != hipSuccess) rc = fail(GAT_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
            else rc = coo_fill(&b, n_rows, d_rp, d_ci, nullptr);
        }
    }
    coo_free(&b);
    if (rc) return cleanup(rc);
    if (d_rp) {
        G_HIP(hipMemcpy(row_ptr_out, d_rp, (n_rows + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (*n_edges_out > 0) G_HIP(hipMemcpy(col_idx_out, d_ci, *n_edges_out * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
#undef G_HIP
    return cleanup(0);
}

}  // extern "C"
