// gat_dropout.hip — the dense side of dropout (include/gatv2_abi.h "dropout"): the step counter, the feature-dropout
// copy of a layer's input and its backward, and the mask taps (DropEdge's included).  Attention dropout lives inside the edge kernels
// (gat_edge_kernels.hip: the forward's EXT and the backward's DROP instantiations).  Every kernel evaluates the masks with the same device functions
// (gat_internal.h drop_*), so the taps show exactly what the passes used.
#include "gat_internal.h"

namespace gat {
namespace {

// one lane, an ordinary store: captured into a step graph like any other kernel
__global__ void drop_advance_kernel(uint64_t* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *step = *step + 1;
}

__global__ __launch_bounds__(256) void feat_drop_fwd_kernel(const float* __restrict__ x, float* __restrict__ xo, int64_t rows,
                                                            int32_t F, int32_t ld, DropArgs d) {
    const uint32_t K = drop_key(d, kDropFeat);
    const int64_t total = rows * ld, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / ld;
        const int32_t f = (int32_t)(i - r * ld);
        float v = 0.f;
        if (f < F) v = x[i] * drop_factor(d, drop_mix(drop_mix(K, drop_node(d, r)), (uint32_t)f));
        xo[i] = v;
    }
}

__global__ __launch_bounds__(256) void feat_drop_bwd_kernel(float* __restrict__ g, int64_t rows, int32_t F, DropArgs d) {
    const uint32_t K = drop_key(d, kDropFeat);
    const int64_t total = rows * F, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / F;
        const int32_t f = (int32_t)(i - r * F);
        g[i] *= drop_factor(d, drop_mix(drop_mix(K, drop_node(d, r)), (uint32_t)f));
    }
}

__global__ __launch_bounds__(256) void feat_keep_tap_kernel(int64_t rows, int32_t F, DropArgs d, float* __restrict__ out) {
    const uint32_t K = drop_key(d, kDropFeat);
    const int64_t total = rows * F, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int64_t r = i / F;
        const int32_t f = (int32_t)(i - r * F);
        out[i] = drop_factor(d, drop_mix(drop_mix(K, drop_node(d, r)), (uint32_t)f));
    }
}

// out[h][e]: the destination row of CSR edge e by binary search (as csr_to_coo_kernel), k = e - row_ptr[row]
__global__ __launch_bounds__(256) void attn_keep_tap_kernel(const int32_t* __restrict__ row_ptr, int64_t n_rows, int64_t n_edges,
                                                            int32_t H, DropArgs d, float* __restrict__ out) {
    const uint32_t K = drop_key(d, kDropAttn);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += stride) {
        int64_t lo = 0, hi = n_rows;                 // row_ptr[lo] <= e < row_ptr[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)row_ptr[mid] <= e) lo = mid; else hi = mid;
        }
        const uint32_t kn = drop_mix(drop_mix(K, drop_node(d, lo)), (uint32_t)(e - row_ptr[lo]));
        for (int32_t h = 0; h < H; ++h) out[(int64_t)h * n_edges + e] = drop_factor(d, drop_mix(kn, (uint32_t)h));
    }
}

// out[e] = 1 if CSR edge e is kept by DropEdge, else 0 (row by binary search, as above)
__global__ __launch_bounds__(256) void edge_keep_tap_kernel(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col_idx,
                                                            int64_t n_rows, int64_t n_edges, DropArgs d, float* __restrict__ out) {
    const uint32_t K = drop_edge_key(d);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += stride) {
        int64_t lo = 0, hi = n_rows;                 // row_ptr[lo] <= e < row_ptr[hi]
        while (hi - lo > 1) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)row_ptr[mid] <= e) lo = mid; else hi = mid;
        }
        out[e] = drop_edge_kept(d, drop_mix(K, drop_node(d, lo)), (int)(e - row_ptr[lo]), col_idx[e], lo) ? 1.f : 0.f;
    }
}

unsigned grid_for(int64_t n) {
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

int launch_drop_advance(uint64_t* step, hipStream_t s) {
    hipLaunchKernelGGL(drop_advance_kernel, dim3(1), dim3(64), 0, s, step);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_feat_drop_fwd(const float* x, float* xo, int64_t rows, int32_t F, int32_t ld, const DropArgs& d, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(feat_drop_fwd_kernel, dim3(grid_for(rows * ld)), dim3(256), 0, s, x, xo, rows, F, ld, d);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_feat_drop_bwd(float* g, int64_t rows, int32_t F, const DropArgs& d, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(feat_drop_bwd_kernel, dim3(grid_for(rows * F)), dim3(256), 0, s, g, rows, F, d);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_attn_keep_tap(const int32_t* row_ptr, int64_t n_rows, int64_t n_edges, int32_t H, const DropArgs& d, float* out, hipStream_t s) {
    if (n_edges <= 0 || n_rows <= 0) return 0;
    hipLaunchKernelGGL(attn_keep_tap_kernel, dim3(grid_for(n_edges)), dim3(256), 0, s, row_ptr, n_rows, n_edges, H, d, out);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_edge_keep_tap(const int32_t* row_ptr, const int32_t* col_idx, int64_t n_rows, int64_t n_edges, const DropArgs& d, float* out, hipStream_t s) {
    if (n_edges <= 0 || n_rows <= 0) return 0;
    hipLaunchKernelGGL(edge_keep_tap_kernel, dim3(grid_for(n_edges)), dim3(256), 0, s, row_ptr, col_idx, n_rows, n_edges, d, out);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_feat_keep_tap(int64_t rows, int32_t F, const DropArgs& d, float* out, hipStream_t s) {
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(feat_keep_tap_kernel, dim3(grid_for(rows * F)), dim3(256), 0, s, rows, F, d, out);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
