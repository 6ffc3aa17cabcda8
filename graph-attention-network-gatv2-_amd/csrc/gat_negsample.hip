// gat_negsample.hip — negative sampling on the device (gatv2_abi.h "negative sampling"): node pairs that are NOT edges of the graph,
// drawn with the generators' counter hash so that the list is a function of (graph, mode, flags, seed, round, count[, source pairs])
// alone — synth.negative_pairs states the same law in numpy and the two agree to the bit.
//
// One lane per negative, grid-stride.  A negative makes up to GAT_NEG_TRIES attempts; attempt a of negative j of round r draws from
// counter k = (r * count + j) * 16 + a (wrapping uint64), the first accepted candidate wins, and a negative whose attempts all fail
// keeps the last candidate and adds one to the caller's count of unfiltered negatives (an integer atomic on one word, once per wave).
// "(u, v) is an edge" = u occurs among the sources of row v: a binary search where every row of the CSR is ascending
// (csr_rows_ascending, one pass at set-up — Products' hub rows hold thousands of sources), a linear scan of the row otherwise; both
// answer the same question, on rows with duplicate edges too, so the pairs do not depend on which one runs.
#include <algorithm>

#include "gat_internal.h"

namespace gat {

namespace {

unsigned grid_for(int64_t work, int64_t cap) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, cap)); }

// one thread per row: flag = 0 once a row steps down
__global__ __launch_bounds__(256) void rows_ascending_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx,
                                                             int64_t n_rows, unsigned int* __restrict__ flag) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) {
        const int32_t beg = row_ptr[r], end = row_ptr[r + 1];
        bool down = false;
        for (int32_t e = beg + 1; e < end && !down; ++e) down = col_idx[e - 1] > col_idx[e];
        if (down) { atomicExch(flag, 0u); return; }
    }
}

template <bool ASC>
__device__ __forceinline__ bool is_edge(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx, int32_t u, int32_t v) {
    const int32_t beg = row_ptr[v], end = row_ptr[v + 1];
    if constexpr (ASC) {
        int32_t lo = beg, hi = end;                      // first entry >= u
        while (lo < hi) {
            const int32_t mid = lo + ((hi - lo) >> 1);
            if (col_idx[mid] < u) lo = mid + 1; else hi = mid;
        }
        return lo < end && col_idx[lo] == u;
    } else {
        for (int32_t e = beg; e < end; ++e)
            if (col_idx[e] == u) return true;
        return false;
    }
}

struct NegBases { uint64_t b37, b41, b43; };             // hash_base(seed, stream) of the law's three streams

template <bool ASC, bool CORRUPT>
__global__ __launch_bounds__(256) void negative_sample_kernel(NegSampleArgs A, NegBases B) {
    const uint64_t N = (uint64_t)A.n_rows;
    const bool both = (A.flags & GAT_NEG_BOTH_DIRECTIONS) != 0, allow_self = (A.flags & GAT_NEG_ALLOW_SELF) != 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int failed = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < A.count; j += stride) {
        const uint64_t c = A.round * (uint64_t)A.count + (uint64_t)j;       // wrapping, as numpy's uint64
        int32_t keep_u = 0, keep_v = 0, role = 0;
        if constexpr (CORRUPT) {
            const int64_t p = j % A.n_src;
            keep_u = A.src_u[p]; keep_v = A.src_v[p];
            role = (int32_t)(hash_at(B.b43, c) & 1ull);                     // once per negative
        }
        int32_t u = 0, v = 0;
        bool ok = false;
        for (int a = 0; a < GAT_NEG_TRIES && !ok; ++a) {
            const uint64_t k = c * (uint64_t)GAT_NEG_TRIES + (uint64_t)a;
            if constexpr (CORRUPT) {
                const int32_t w = (int32_t)(hash_at(B.b37, k) % N);
                u = role == 0 ? w : keep_u;
                v = role == 0 ? keep_v : w;
            } else {
                u = (int32_t)(hash_at(B.b37, k) % N);
                v = (int32_t)(hash_at(B.b41, k) % N);
            }
            ok = (allow_self || u != v) && !is_edge<ASC>(A.row_ptr, A.col_idx, u, v) && !(both && is_edge<ASC>(A.row_ptr, A.col_idx, v, u));
        }
        A.u[j] = u; A.v[j] = v;                                              // the accepted candidate, or attempt 15's
        failed += ok ? 0u : 1u;
    }
    for (int off = 32; off > 0; off >>= 1) failed += __shfl_xor(failed, off);      // every lane is here: the loop has no early exit
    if ((threadIdx.x & 63) == 0 && failed) atomicAdd(A.unfiltered, (unsigned long long)failed);
}

}  // namespace

int csr_rows_ascending(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, bool* ascending, hipStream_t s) {
    Scratch tmp;
    unsigned int* d_flag = nullptr;
    unsigned int flag = 1;
    GAT_TRY(tmp.get(&d_flag, 1));
    GAT_HIP(hipMemcpyAsync(d_flag, &flag, sizeof(flag), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(rows_ascending_kernel, dim3(grid_for(n_rows, 16384)), dim3(256), 0, s, d_row_ptr, d_col_idx, n_rows, d_flag);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, s));
    GAT_HIP(hipStreamSynchronize(s));
    *ascending = flag != 0;
    return 0;
}

int launch_negative_sample(const NegSampleArgs& a, hipStream_t s) {
    if (a.mode != GAT_NEG_UNIFORM && a.mode != GAT_NEG_CORRUPT) return fail(GAT_E_INVALID, "negative sampling: mode must be GAT_NEG_UNIFORM or GAT_NEG_CORRUPT");
    if (a.flags & ~(GAT_NEG_BOTH_DIRECTIONS | GAT_NEG_ALLOW_SELF)) return fail(GAT_E_INVALID, "negative sampling: unknown flag bits");
    if (a.n_rows < 1 || a.n_rows >= 0x7fffffffLL || a.count < 1) return fail(GAT_E_INVALID, "negative sampling: bad sizes");
    if (!a.row_ptr || !a.col_idx || !a.u || !a.v || !a.unfiltered) return fail(GAT_E_INVALID, "negative sampling: null argument");
    const bool corrupt = a.mode == GAT_NEG_CORRUPT;
    if (corrupt && (a.n_src < 1 || !a.src_u || !a.src_v)) return fail(GAT_E_INVALID, "negative sampling: GAT_NEG_CORRUPT needs at least one source pair");
    const NegBases b{hash_base(a.seed, 37), hash_base(a.seed, 41), hash_base(a.seed, 43)};
    const dim3 grid(grid_for(a.count, 16384)), block(256);
    if (a.ascending) {
        if (corrupt) hipLaunchKernelGGL((negative_sample_kernel<true, true>), grid, block, 0, s, a, b);
        else hipLaunchKernelGGL((negative_sample_kernel<true, false>), grid, block, 0, s, a, b);
    } else {
        if (corrupt) hipLaunchKernelGGL((negative_sample_kernel<false, true>), grid, block, 0, s, a, b);
        else hipLaunchKernelGGL((negative_sample_kernel<false, false>), grid, block, 0, s, a, b);
    }
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
