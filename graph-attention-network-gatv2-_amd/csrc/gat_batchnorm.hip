// gat_batchnorm.hip — batch normalisation between the aggregation and the activation (gatv2_abi.h "batch normalisation"): the N-sized
// kernels of both directions and their one-block finish kernels.
//
// Lane layout of res_backward_kernel (gat_dense_kernels.hip): a row is LPR lanes of V = 4 (H*D a multiple of 4) or 1 consecutive
// channels, a block is rpb = 256 / LPR rows, the grid is persistent: block b visits the row chunks b, b + grid, b + 2 grid, ... of rpb
// rows each.  A lane owns ITS channels of ITS row slot for every chunk it visits, so a lane's running sum (or Welford triple) is a
// fixed-order sum over rows; the block then folds its rpb row slots in ascending order; the finish kernel folds the blocks in ascending
// order.  Every order depends on (N, H*D, grid) alone: no atomics, bitwise reproducible.  Rows wider than one pass of the block's
// lanes (H*D > 256 V: generic shapes only) are walked in rounds of LPR * V channels.
#include "gat_internal.h"

#include <algorithm>

namespace gat {
namespace {

template <int V>
__device__ __forceinline__ void bn_load(const float* __restrict__ p, float (&x)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
        x[0] = p[0];
    }
}
template <int V>
__device__ __forceinline__ void bn_store(float* __restrict__ p, const float (&x)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else p[0] = x[0];
}
// mean and 1 / sqrt(var + eps) of channel c: the batch's (mean, rstd) as the finish kernel left them, or — from_var — the running
// (mean, var) of eval mode
__device__ __forceinline__ void bn_channel_stats(const BnStats& S, int c, float* mu, float* rstd) {
    *mu = S.mean[c];
    const float s = S.scale[c];
    *rstd = S.from_var ? 1.0f / sqrtf(s + S.eps) : s;
}
// rows of block b of `grid`: its chunks b, b + grid, ... of rpb rows each, the table's last chunk maybe short
__device__ __forceinline__ float bn_block_rows(int64_t N, int rpb, int grid, int b) {
    const int64_t nchunks = (N + rpb - 1) / rpb;
    if (b >= nchunks) return 0.f;
    int64_t rows = ((nchunks - 1 - b) / grid + 1) * rpb;
    if ((nchunks - 1) % grid == b) rows -= nchunks * rpb - N;
    return (float)rows;
}
// Chan's merge of (nb, mb, Mb) into (n, m, M2); nb == 0 leaves the left side as it is
__device__ __forceinline__ void bn_chan(float& n, float& m, float& M2, float nb, float mb, float Mb) {
    if (nb == 0.f) return;
    if (n == 0.f) { n = nb; m = mb; M2 = Mb; return; }
    const float tot = n + nb, delta = mb - m;
    m += delta * (nb / tot);
    M2 += Mb + delta * delta * (n * (nb / tot));
    n = tot;
}

// ---- forward 1: column statistics of u, one (mean, M2) partial per block and column ------------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ u, int64_t N, int32_t HD, float* __restrict__ part_mean,
                                                       float* __restrict__ part_m2, int32_t LPR, int32_t rpb) {
    __shared__ float red_m[256 * 4], red_q[256 * 4], red_n[256];
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    for (int base = 0; base < HD; base += LPR * V) {     // (the round count is the same for every lane: barriers below)
        float n = 0.f;                                   // rows this lane's slot visits: the same in every round
        const int c0 = base + cl * V;
        const bool active = r_in < rpb && c0 < HD;
        float m[V], q[V];
#pragma unroll
        for (int i = 0; i < V; ++i) { m[i] = 0.f; q[i] = 0.f; }
        if (active) {
            for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < N; row += (int64_t)gridDim.x * rpb) {
                float x[V];
                bn_load<V>(u + row * HD + c0, x);
                n += 1.0f;
                const float inv = 1.0f / n;
#pragma unroll
                for (int i = 0; i < V; ++i) {            // Welford
                    const float d = x[i] - m[i];
                    m[i] += d * inv;
                    q[i] += d * (x[i] - m[i]);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < V; ++i) { red_m[t * V + i] = m[i]; red_q[t * V + i] = q[i]; }
        if (cl == 0 && r_in < rpb) red_n[r_in] = n;
        __syncthreads();
        if (r_in == 0 && c0 < HD) {
#pragma unroll
            for (int i = 0; i < V; ++i) {
                float nn = 0.f, mm = 0.f, qq = 0.f;
                for (int r = 0; r < rpb; ++r) bn_chan(nn, mm, qq, red_n[r], red_m[(r * LPR + cl) * V + i], red_q[(r * LPR + cl) * V + i]);
                part_mean[(int64_t)blockIdx.x * HD + c0 + i] = mm;
                part_m2[(int64_t)blockIdx.x * HD + c0 + i] = qq;
            }
        }
        __syncthreads();
    }
}
// ---- forward 2: one block folds the block partials in ascending order, writes mu and rstd, advances the running statistics ------------------
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const float* __restrict__ part_mean, const float* __restrict__ part_m2, int32_t grid,
                                                              int32_t rpb, int64_t N, int32_t HD, float eps, float momentum, float* __restrict__ mean,
                                                              float* __restrict__ rstd, float* __restrict__ run_mean, float* __restrict__ run_var) {
    for (int c = threadIdx.x; c < HD; c += 256) {
        float n = 0.f, m = 0.f, q = 0.f;
        for (int b = 0; b < grid; ++b) bn_chan(n, m, q, bn_block_rows(N, rpb, grid, b), part_mean[(int64_t)b * HD + c], part_m2[(int64_t)b * HD + c]);
        const float var = q / (float)N;
        mean[c] = m;
        rstd[c] = 1.0f / sqrtf(var + eps);
        if (run_mean != nullptr) {
            const float unbiased = N > 1 ? var * ((float)N / (float)(N - 1)) : var;
            run_mean[c] = (1.0f - momentum) * run_mean[c] + momentum * m;
            run_var[c] = (1.0f - momentum) * run_var[c] + momentum * unbiased;
        }
    }
}
// ---- forward 3: hout = LReLU(gamma * xhat + beta); hidden layers [N][HD], row lanes as above ------------------------------------------------
template <int V>
__global__ __launch_bounds__(256) void bn_apply_kernel(const float* __restrict__ u, BnStats S, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, float slope, float* __restrict__ hout, int64_t N, int32_t HD,
                                                       int32_t LPR, int32_t rpb) {
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    if (r_in >= rpb) return;
    for (int c0 = cl * V; c0 < HD; c0 += LPR * V) {
        float mu[V], rs[V], gm[V], bt[V];
#pragma unroll
        for (int i = 0; i < V; ++i) { bn_channel_stats(S, c0 + i, &mu[i], &rs[i]); gm[i] = gamma[c0 + i]; bt[i] = beta[c0 + i]; }
        for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < N; row += (int64_t)gridDim.x * rpb) {
            float x[V], o[V];
            bn_load<V>(u + row * HD + c0, x);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                const float v = gm[i] * ((x[i] - mu[i]) * rs[i]) + bt[i];
                o[i] = v > 0.f ? v : v * slope;
            }
            bn_store<V>(hout + row * HD + c0, o);
        }
    }
}
// last layer: hout [N][D] = mean over heads, h ascending, of LReLU(v); one lane per (row, d), consecutive lanes consecutive d
__global__ __launch_bounds__(256) void bn_apply_last_kernel(const float* __restrict__ u, BnStats S, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float slope, float* __restrict__ hout, int64_t N, int32_t H,
                                                            int32_t D) {
    const int64_t total = N * D;
    const int HD = H * D;
    const float inv_heads = 1.0f / (float)H;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / D;
        const int d = (int)(i - row * D);
        float acc = 0.f;
        for (int h = 0; h < H; ++h) {
            const int c = h * D + d;
            float mu, rs;
            bn_channel_stats(S, c, &mu, &rs);
            const float v = gamma[c] * ((u[row * HD + c] - mu) * rs) + beta[c];
            acc += v > 0.f ? v : v * slope;
        }
        hout[i] = acc * inv_heads;
    }
}

// ---- backward: dv = dL/dhout * LReLU'(v) of channels c0 .. c0+V-1 of a row, with xhat ---------------------------------------------------------
template <int V>
__device__ __forceinline__ void bn_row_dv(const BnBwdArgs& A, int64_t row, int c0, int HD, float inv_heads, const float (&mu)[V], const float (&rs)[V],
                                          const float (&gm)[V], const float (&bt)[V], float (&x)[V], float (&xh)[V], float (&dv)[V]) {
    bn_load<V>(A.u + row * HD + c0, x);
    float go[V];
    if (A.gh == nullptr) bn_load<V>(A.g + row * HD + c0, go);
#pragma unroll
    for (int i = 0; i < V; ++i) {
        if (A.gh != nullptr) go[i] = A.gh[row * A.gh_stride + (c0 + i) % A.D] * inv_heads;     // the mean over heads, backwards
        xh[i] = (x[i] - mu[i]) * rs[i];
        const float v = gm[i] * xh[i] + bt[i];
        // rounded on its own (no contraction into the sums and differences that take it): both backward kernels see the same dv, and
        // dv - s1 / N is exactly 0 where it should be (N == 1)
        {
#pragma clang fp contract(off)
            dv[i] = go[i] * (v > 0.f ? 1.0f : A.slope);
        }
    }
}
// the block's column sums of V-wide lane sums, row slots in ascending order, into partial[block][c]
template <int V>
__device__ __forceinline__ void bn_flush(float* red, const float (&sum)[V], float* __restrict__ partial, int t, int r_in, int cl, int c0, int HD, int LPR,
                                         int rpb) {
#pragma unroll
    for (int i = 0; i < V; ++i) red[t * V + i] = sum[i];
    __syncthreads();
    if (r_in == 0 && c0 < HD) {
#pragma unroll
        for (int i = 0; i < V; ++i) {
            float tot = 0.f;
            for (int r = 0; r < rpb; ++r) tot += red[(r * LPR + cl) * V + i];
            partial[(int64_t)blockIdx.x * HD + c0 + i] = tot;
        }
    }
    __syncthreads();
}
// backward 1: per-block column partials of dv (part_s1) and dv * xhat (part_s2)
template <int V>
__global__ __launch_bounds__(256) void bn_colsum_kernel(BnBwdArgs A, int32_t LPR, int32_t rpb) {
    __shared__ float red[256 * 4];
    const int HD = A.H * A.D;
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    const float inv_heads = 1.0f / (float)A.H;
    for (int base = 0; base < HD; base += LPR * V) {
        const int c0 = base + cl * V;
        const bool active = r_in < rpb && c0 < HD;
        float s1[V], s2[V];
#pragma unroll
        for (int i = 0; i < V; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
        if (active) {
            float mu[V], rs[V], gm[V], bt[V];
#pragma unroll
            for (int i = 0; i < V; ++i) { bn_channel_stats(A.stats, c0 + i, &mu[i], &rs[i]); gm[i] = A.gamma[c0 + i]; bt[i] = A.beta[c0 + i]; }
            for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < A.n_rows; row += (int64_t)gridDim.x * rpb) {
                float x[V], xh[V], dv[V];
                bn_row_dv<V>(A, row, c0, HD, inv_heads, mu, rs, gm, bt, x, xh, dv);
#pragma unroll
                for (int i = 0; i < V; ++i) { s1[i] += dv[i]; s2[i] += dv[i] * xh[i]; }
            }
        }
        bn_flush<V>(red, s1, A.part_s1, t, r_in, cl, c0, HD, LPR, rpb);
        bn_flush<V>(red, s2, A.part_s2, t, r_in, cl, c0, HD, LPR, rpb);
    }
}
// one block: the block partials in ascending order into sums [2][HD] = {s1, s2} of THIS step, which are also added to grad_beta / grad_gamma
__global__ __launch_bounds__(256) void bn_colsum_finish_kernel(const float* __restrict__ part_s1, const float* __restrict__ part_s2, int32_t grid,
                                                               int32_t HD, float* __restrict__ sums, float* __restrict__ grad_gamma,
                                                               float* __restrict__ grad_beta) {
    for (int c = threadIdx.x; c < HD; c += 256) {
        float a = 0.f, b = 0.f;
        for (int k = 0; k < grid; ++k) { a += part_s1[(int64_t)k * HD + c]; b += part_s2[(int64_t)k * HD + c]; }
        sums[c] = a; sums[HD + c] = b;
        if (grad_beta != nullptr) grad_beta[c] += a;
        if (grad_gamma != nullptr) grad_gamma[c] += b;
    }
}
// backward 2: G = gamma rstd (dv - s1 / N - xhat s2 / N) (training) or gamma rstd dv (eval), agg = u - (R + b), block column partials of G
template <int V>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(BnBwdArgs A, int32_t LPR, int32_t rpb) {
    __shared__ float red[256 * 4];
    const int HD = A.H * A.D;
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    const float inv_heads = 1.0f / (float)A.H, inv_n = 1.0f / (float)A.n_rows;
    for (int base = 0; base < HD; base += LPR * V) {
        const int c0 = base + cl * V;
        const bool active = r_in < rpb && c0 < HD;
        float sG[V];
#pragma unroll
        for (int i = 0; i < V; ++i) sG[i] = 0.f;
        if (active) {
            float mu[V], rs[V], gm[V], bt[V], m1[V], m2[V], bv[V];
#pragma unroll
            for (int i = 0; i < V; ++i) {
                bn_channel_stats(A.stats, c0 + i, &mu[i], &rs[i]); gm[i] = A.gamma[c0 + i]; bt[i] = A.beta[c0 + i];
                m1[i] = A.training ? A.sums[c0 + i] * inv_n : 0.f;
                m2[i] = A.training ? A.sums[HD + c0 + i] * inv_n : 0.f;
                bv[i] = A.bias != nullptr ? A.bias[c0 + i] : 0.f;
            }
            for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < A.n_rows; row += (int64_t)gridDim.x * rpb) {
                float x[V], xh[V], dv[V], G[V];
                bn_row_dv<V>(A, row, c0, HD, inv_heads, mu, rs, gm, bt, x, xh, dv);
                const int64_t o = row * HD + c0;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    G[i] = gm[i] * rs[i] * (dv[i] - m1[i] - xh[i] * m2[i]);
                    sG[i] += G[i];
                }
                bn_store<V>(A.G + o, G);
                if (A.agg != nullptr) {
                    float rv[V], ag[V];
#pragma unroll
                    for (int i = 0; i < V; ++i) rv[i] = 0.f;
                    if (A.res != nullptr) bn_load<V>(A.res + o, rv);
#pragma unroll
                    for (int i = 0; i < V; ++i) ag[i] = x[i] - (rv[i] + bv[i]);
                    bn_store<V>(A.agg + o, ag);
                }
            }
        }
        if (A.part_G != nullptr) bn_flush<V>(red, sG, A.part_G, t, r_in, cl, c0, HD, LPR, rpb);      // (uniform per block)
    }
}

void bn_shape(int32_t HD, int* V, int* LPR, int* rpb) {
    *V = HD % 4 == 0 ? 4 : 1;
    const int groups = HD / *V;                          // column groups of a row
    *LPR = groups < 256 ? groups : 256;
    *rpb = 256 / *LPR;
}
enum { kBnStats = 0, kBnApply = 1, kBnColsum = 2, kBnBwdApply = 3 };
const void* bn_fn(int which, int V) {
    switch (which) {
        case kBnStats: return V == 4 ? (const void*)bn_stats_kernel<4> : (const void*)bn_stats_kernel<1>;
        case kBnApply: return V == 4 ? (const void*)bn_apply_kernel<4> : (const void*)bn_apply_kernel<1>;
        case kBnColsum: return V == 4 ? (const void*)bn_colsum_kernel<4> : (const void*)bn_colsum_kernel<1>;
        default: return V == 4 ? (const void*)bn_bwd_apply_kernel<4> : (const void*)bn_bwd_apply_kernel<1>;
    }
}
int bn_grid(int which, int64_t n_rows, int32_t HD) {
    int V, LPR, rpb;
    bn_shape(HD, &V, &LPR, &rpb);
    const int64_t want = std::max<int64_t>(1, (n_rows + rpb - 1) / rpb);
    return (int)std::min({want, resident_blocks(bn_fn(which, V), 0), (int64_t)kResPartialRows});
}
int bn_stats_check(const char* who, const BnStats& s) {
    if (s.mean == nullptr || s.scale == nullptr) return fail(GAT_E_INVALID, std::string(who) + ": null statistics");
    return 0;
}

}  // namespace

int batch_norm_blocks(int64_t n_rows, int32_t HD) {
    // one answer for the kernels that write block partials and the regions sized for them: the smallest of their grids
    return std::min({bn_grid(kBnStats, n_rows, HD), bn_grid(kBnColsum, n_rows, HD), bn_grid(kBnBwdApply, n_rows, HD)});
}

int launch_batch_norm_stats(const float* u, int64_t n_rows, int32_t HD, float* part_mean, float* part_m2, float eps, float momentum, float* mean,
                            float* rstd, float* run_mean, float* run_var, hipStream_t s) {
    if (n_rows <= 0) return 0;
    if (u == nullptr || part_mean == nullptr || part_m2 == nullptr || mean == nullptr || rstd == nullptr || HD < 1)
        return fail(GAT_E_INVALID, "batch_norm_stats: null argument");
    if ((run_mean == nullptr) != (run_var == nullptr)) return fail(GAT_E_INVALID, "batch_norm_stats: one running statistic without the other");
    int V, LPR, rpb;
    bn_shape(HD, &V, &LPR, &rpb);
    const int grid = batch_norm_blocks(n_rows, HD);
    if (V == 4) hipLaunchKernelGGL(bn_stats_kernel<4>, dim3((unsigned)grid), dim3(256), 0, s, u, n_rows, HD, part_mean, part_m2, LPR, rpb);
    else hipLaunchKernelGGL(bn_stats_kernel<1>, dim3((unsigned)grid), dim3(256), 0, s, u, n_rows, HD, part_mean, part_m2, LPR, rpb);
    GAT_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_stats_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)part_mean, (const float*)part_m2, grid, rpb, n_rows, HD, eps,
                       momentum, mean, rstd, run_mean, run_var);
    GAT_HIP(hipGetLastError());
    return 0;
}

int launch_batch_norm_apply(const float* u, const BnStats& st, const float* gamma, const float* beta, float slope, float* hout, int64_t n_rows,
                            int32_t H, int32_t D, bool is_last, hipStream_t s) {
    if (n_rows <= 0) return 0;
    GAT_TRY(bn_stats_check("batch_norm_apply", st));
    if (u == nullptr || gamma == nullptr || beta == nullptr || hout == nullptr || H < 1 || D < 1) return fail(GAT_E_INVALID, "batch_norm_apply: null argument");
    const int32_t HD = H * D;
    if (is_last) {
        const int64_t want = std::max<int64_t>(1, (n_rows * D + 255) / 256);
        const int grid = (int)std::min(want, resident_blocks((const void*)bn_apply_last_kernel, 0));
        hipLaunchKernelGGL(bn_apply_last_kernel, dim3((unsigned)grid), dim3(256), 0, s, u, st, gamma, beta, slope, hout, n_rows, H, D);
    } else {
        int V, LPR, rpb;
        bn_shape(HD, &V, &LPR, &rpb);
        const int grid = bn_grid(kBnApply, n_rows, HD);
        if (V == 4) hipLaunchKernelGGL(bn_apply_kernel<4>, dim3((unsigned)grid), dim3(256), 0, s, u, st, gamma, beta, slope, hout, n_rows, HD, LPR, rpb);
        else hipLaunchKernelGGL(bn_apply_kernel<1>, dim3((unsigned)grid), dim3(256), 0, s, u, st, gamma, beta, slope, hout, n_rows, HD, LPR, rpb);
    }
    GAT_HIP(hipGetLastError());
    return 0;
}

int launch_batch_norm_backward(const BnBwdArgs& a, float* grad_gamma, float* grad_beta, hipStream_t s) {
    if (a.n_rows <= 0) return 0;
    GAT_TRY(bn_stats_check("batch_norm_backward", a.stats));
    if (a.gh == nullptr && a.g == nullptr) return fail(GAT_E_INVALID, "batch_norm_backward: no output gradient");
    if (a.u == nullptr || a.gamma == nullptr || a.beta == nullptr || a.G == nullptr || a.part_s1 == nullptr || a.part_s2 == nullptr || a.sums == nullptr ||
        a.H < 1 || a.D < 1)
        return fail(GAT_E_INVALID, "batch_norm_backward: null argument");
    const int32_t HD = a.H * a.D;
    int V, LPR, rpb;
    bn_shape(HD, &V, &LPR, &rpb);
    if (a.blocks != batch_norm_blocks(a.n_rows, HD)) return fail(GAT_E_INVALID, "batch_norm_backward: blocks must come from batch_norm_blocks()");
    if (V == 4) hipLaunchKernelGGL(bn_colsum_kernel<4>, dim3((unsigned)a.blocks), dim3(256), 0, s, a, LPR, rpb);
    else hipLaunchKernelGGL(bn_colsum_kernel<1>, dim3((unsigned)a.blocks), dim3(256), 0, s, a, LPR, rpb);
    GAT_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_colsum_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)a.part_s1, (const float*)a.part_s2, a.blocks, HD, a.sums, grad_gamma,
                       grad_beta);
    GAT_HIP(hipGetLastError());
    if (V == 4) hipLaunchKernelGGL(bn_bwd_apply_kernel<4>, dim3((unsigned)a.blocks), dim3(256), 0, s, a, LPR, rpb);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<1>, dim3((unsigned)a.blocks), dim3(256), 0, s, a, LPR, rpb);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
