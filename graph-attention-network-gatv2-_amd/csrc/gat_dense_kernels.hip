// gat_dense_kernels.hip — node-level pieces of the GATv2 step on gfx950 that are not GEMMs:
// the fixed-order slab reductions, the optimizer and clip kernels, the residual / layer-norm backward and the Xavier
// init.  (Projection GEMMs: gat_gemm_kernels.hip; the output head: gat_head.hip.)
#include "gat_internal.h"

#include <algorithm>

namespace gat {
namespace {

// out[map(idx)] += sum_z slabs[z][idx].  Block = 64 columns x 16 z-slices, 4 independent partial
// sums per thread, combined in a fixed order: bitwise reproducible, and short dependent chains
// (nslabs/64 rounds) instead of one thread walking all slabs.
struct MapIdentity {
    __device__ __forceinline__ int64_t operator()(int64_t idx) const { return idx; }
};
struct MapGradW {             // idx = (c-c_base)*F + f over rows c of [2HD][F]  ->  reference layout [HD][2F]
    int32_t HD, F, c_base;
    __device__ __forceinline__ int64_t operator()(int64_t idx) const {
        const int32_t c = c_base + (int32_t)idx / F, f = (int32_t)idx % F;
        return (int64_t)(c % HD) * 2 * F + (c / HD) * F + f;
    }
};
template <class MAP>
__global__ __launch_bounds__(1024) void reduce_slabs_kernel(const float* __restrict__ slabs, int32_t nslabs,
                                                           int64_t width, float* __restrict__ out, MAP map) {
    __shared__ float part[16][64];
    const int q = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int64_t idx = (int64_t)blockIdx.x * 64 + q;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (idx < width) {
        int z = sl;
        for (; z + 48 < nslabs; z += 64) {
            s0 += slabs[(int64_t)z * width + idx];
            s1 += slabs[(int64_t)(z + 16) * width + idx];
            s2 += slabs[(int64_t)(z + 32) * width + idx];
            s3 += slabs[(int64_t)(z + 48) * width + idx];
        }
        for (; z < nslabs; z += 16) s0 += slabs[(int64_t)z * width + idx];
    }
    part[sl][q] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl == 0 && idx < width) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += part[w][q];
        out[map(idx)] += tot;
    }
}

// every queued reduction in one launch (ReduceBatch); block -> job by the jobs' first-block prefix; one extra block
// packs {loss, correct} like pack_result_kernel
__global__ __launch_bounds__(1024) void reduce_batch_kernel(ReduceBatch B) {
    __shared__ float part[16][64];
    if ((int)blockIdx.x >= B.blocks) {                   // the extra block: head finalize (as head_finalize_kernel), then the pack
        if (threadIdx.x >= 64) return;
        float lossv = 0.f; int32_t corrv = 0;
        if (B.fin_loss != nullptr) {
            double l = 0.0; int c = 0;
            for (int i = threadIdx.x; i < B.fin_n; i += 64) { l += B.fin_loss[i]; c += B.fin_corr[i]; }
            for (int off = 32; off > 0; off >>= 1) { l += __shfl_down(l, off); c += __shfl_down(c, off); }
            lossv = (float)l; corrv = c;
            if (threadIdx.x == 0) { *B.fin_loss_out = lossv; *B.fin_corr_out = corrv; }
        } else if (threadIdx.x == 0 && B.dst3 != nullptr) {
            lossv = *B.loss; corrv = *B.correct;
        }
        if (threadIdx.x == 0 && B.dst3 != nullptr) {
            const float v0 = lossv, v1 = (float)(corrv & 4095), v2 = (float)(corrv >> 12);
            B.dst3[0] = v0; B.dst3[1] = v1; B.dst3[2] = v2;
            if (B.dst3_host != nullptr) { B.dst3_host[0] = v0; B.dst3_host[1] = v1; B.dst3_host[2] = v2; }
        }
        return;
    }
    int j = 0;
#pragma unroll
    for (int i = 1; i < 8; ++i) if (i < B.n && (int)blockIdx.x >= B.jobs[i].block0) j = i;
    const ReduceJob J = B.jobs[j];
    const int q = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int64_t idx = (int64_t)((int)blockIdx.x - J.block0) * 64 + q;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (idx < J.width) {
        int z = sl;
        for (; z + 48 < J.nslabs; z += 64) {
            s0 += J.slabs[(int64_t)z * J.width + idx];
            s1 += J.slabs[(int64_t)(z + 16) * J.width + idx];
            s2 += J.slabs[(int64_t)(z + 32) * J.width + idx];
            s3 += J.slabs[(int64_t)(z + 48) * J.width + idx];
        }
        for (; z < J.nslabs; z += 16) s0 += J.slabs[(int64_t)z * J.width + idx];
    }
    part[sl][q] = (s0 + s1) + (s2 + s3);
    __syncthreads();
    if (sl == 0 && idx < J.width) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < 16; ++w) tot += part[w][q];
        const int64_t o = J.HD != 0 ? MapGradW{J.HD, J.F, J.c_base}(idx) : idx;
        J.out[o] += tot;
    }
}

// ---- optimizer / clip (E:146-177, 250-278, 896-923) ---------------------------------------------------------------
__global__ __launch_bounds__(256) void sgd_kernel(float* p, const float* g, float lr, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] -= lr * g[i];
}
__global__ __launch_bounds__(256) void adam_kernel(float* p, const float* g, float* m, float* v, float lr,
                                                  int64_t n, float b1, float b2, float eps, int32_t t) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float gi = g[i];
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * (gi * gi);
        m[i] = mi; v[i] = vi;
        const float mh = mi / (1.0f - powf(b1, (float)t));
        const float vh = vi / (1.0f - powf(b2, (float)t));
        p[i] -= lr * mh / (sqrtf(vh) + eps);
    }
}
// one block: sum of squares in a fixed order, result (the squared norm) to *out
__global__ __launch_bounds__(1024) void sumsq_kernel(const float* __restrict__ g, int64_t n, float* out) {
    __shared__ float part[16];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) s += g[i] * g[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < 16; ++w) t += part[w];
        *out = t;
    }
}
__global__ __launch_bounds__(256) void clip_scale_kernel(float* g, int64_t n, const float* sumsq, float thresh) {
    const float norm = sqrtf(*sumsq);
    float scale = 1.0f;
    if (norm > thresh) scale = thresh / (norm + 1e-9f);
    if (!(scale < 1.0f)) return;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) g[i] *= scale;
}

// ---- residual / bias backward (gatv2_abi.h "residual"): one pass over the N x HD tensors of a layer -----------------------------
// G = dL/dh_pre (fp32), agg = h_pre - (R + b), and the block's column sums of G for grad_b.  A block is rpb rows of LPR lanes, a
// lane owns V consecutive channels of ITS column group for every row it visits (rows blockIdx*rpb + r_in, stride gridDim*rpb), so
// its running sum is a fixed-order sum over rows; the block then adds its rpb row lanes in ascending order: partial[block][c] is
// bitwise reproducible, and the sum over blocks is finished by the fixed-order slab reduction.  V = 4: 16-byte loads and stores.
template <int V>
__global__ __launch_bounds__(256) void res_backward_kernel(ResBwdArgs A, int32_t LPR, int32_t rpb) {
    __shared__ float red[256 * 4];
    const int HD = A.H * A.D;
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    const float inv_heads = 1.0f / (float)A.H;
    for (int base = 0; base < HD; base += LPR * V) {     // one round unless H*D exceeds what 256 lanes cover (generic shapes only);
        const int c0 = base + cl * V;                    // the round count is the same for every lane (barriers below)
        const bool active = r_in < rpb && c0 < HD;
        float sum[V];
        float bv[V];
#pragma unroll
        for (int i = 0; i < V; ++i) { sum[i] = 0.f; bv[i] = (active && A.bias != nullptr) ? A.bias[c0 + i] : 0.f; }
        if (active) {
            for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < A.n_rows; row += (int64_t)gridDim.x * rpb) {
                const int64_t o = row * HD + c0;
                float hp[V], gv[V], rv[V];
                if constexpr (V == 4) {
                    const float4 h4 = *reinterpret_cast<const float4*>(A.hpre + o);
                    hp[0] = h4.x; hp[1] = h4.y; hp[2] = h4.z; hp[3] = h4.w;
                    float4 r4 = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (A.res != nullptr) r4 = *reinterpret_cast<const float4*>(A.res + o);
                    rv[0] = r4.x; rv[1] = r4.y; rv[2] = r4.z; rv[3] = r4.w;
                    if (A.gh == nullptr) {
                        const float4 g4 = *reinterpret_cast<const float4*>(A.g + o);
                        gv[0] = g4.x; gv[1] = g4.y; gv[2] = g4.z; gv[3] = g4.w;
                    }
                } else {
                    hp[0] = A.hpre[o];
                    rv[0] = A.res != nullptr ? A.res[o] : 0.f;
                    if (A.gh == nullptr) gv[0] = A.g[o];
                }
                float G[V], ag[V];
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float d = hp[i] > 0.f ? 1.0f : A.slope;
                    if (A.gh != nullptr) G[i] = A.gh[row * A.gh_stride + (c0 + i) % A.D] * d * inv_heads;     // E:598-603
                    else G[i] = A.g_raw ? gv[i] * d : gv[i];                                               // E:888-892
                    ag[i] = hp[i] - (rv[i] + bv[i]);
                    sum[i] += G[i];
                }
                if constexpr (V == 4) {
                    *reinterpret_cast<float4*>(A.G + o) = make_float4(G[0], G[1], G[2], G[3]);
                    *reinterpret_cast<float4*>(A.agg + o) = make_float4(ag[0], ag[1], ag[2], ag[3]);
                } else {
                    A.G[o] = G[0];
                    A.agg[o] = ag[0];
                }
            }
        }
        if (A.partial != nullptr) {                       // (uniform per block: every lane reaches the barriers)
#pragma unroll
            for (int i = 0; i < V; ++i) red[t * V + i] = sum[i];
            __syncthreads();
            if (r_in == 0 && c0 < HD) {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    float tot = 0.f;
                    for (int r = 0; r < rpb; ++r) tot += red[(r * LPR + cl) * V + i];
                    A.partial[(int64_t)blockIdx.x * HD + c0 + i] = tot;
                }
            }
            __syncthreads();
        }
    }
}

// ---- layer normalisation backward (gatv2_abi.h "layer normalisation"): one pass over the N x HD tensors of a normalised layer ------
// A row is LPR lanes (a power of two <= 64, inside one wave), a lane owns V consecutive channels per round of LPR * V channels; a block
// is rpb = 256 / LPR rows.  The row's four means (u; (u - mu)^2; dxh; dxh * xhat) are butterfly sums over the row's lanes: every lane
// ends with the same bits, in an order that depends on nothing but LPR.  ONE: the row fits one round, and the compiler keeps it in
// registers over the passes; else the outer loop writes one round of channels at a time and walks the row again for the means
// (generic shapes only).  Column sums as in res_backward_kernel: a lane's running sum over its rows, then the block's row lanes in
// ascending order.
__device__ __forceinline__ float row_lanes_sum(float x, int LPR) {
    for (int off = LPR >> 1; off > 0; off >>= 1) x += __shfl_xor(x, off);
    return x;
}
template <int V>
__device__ __forceinline__ void load_channels(const float* __restrict__ p, float (&x)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        x[0] = t.x; x[1] = t.y; x[2] = t.z; x[3] = t.w;
    } else {
        x[0] = p[0];
    }
}
template <int V, bool ONE>
__global__ __launch_bounds__(256) void norm_backward_kernel(NormBwdArgs A, int32_t LPR, int32_t rpb) {
    __shared__ float red[256 * 4];
    const ResBwdArgs& R = A.r;
    const int HD = R.H * R.D;
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    const int span = LPR * V;
    const int walk = ONE ? 1 : HD;                       // bound of the loops over the row's rounds
    const float inv_heads = 1.0f / (float)R.H, inv_hd = 1.0f / (float)HD;
    // channel c .. c+V-1 of a row: xhat, dv = dL/dhout * LReLU'(v), dxh = dv * gamma
    auto channels = [&](int64_t row, int c, float mu, float rstd, float (&u)[V], float (&xh)[V], float (&dv)[V], float (&dxh)[V]) {
        load_channels<V>(R.hpre + row * HD + c, u);
        float go[V];
        if (R.gh == nullptr) load_channels<V>(R.g + row * HD + c, go);
#pragma unroll
        for (int i = 0; i < V; ++i) {
            const float gm = A.gamma[c + i];
            xh[i] = (u[i] - mu) * rstd;
            const float v = gm * xh[i] + A.beta[c + i];
            if (R.gh != nullptr) go[i] = R.gh[row * R.gh_stride + (c + i) % R.D] * inv_heads;     // mean over heads (E:440-449)
            dv[i] = go[i] * (v > 0.f ? 1.0f : R.slope);
            dxh[i] = dv[i] * gm;
        }
    };
    for (int ob = 0; ob < HD; ob += span) {              // the round this pass writes; the same count for every lane (barriers below)
        const int c0 = ob + cl * V;
        const bool own = c0 < HD;
        float sG[V], sg[V], sb[V], bv[V];
#pragma unroll
        for (int i = 0; i < V; ++i) { sG[i] = 0.f; sg[i] = 0.f; sb[i] = 0.f; bv[i] = (own && R.bias != nullptr) ? R.bias[c0 + i] : 0.f; }
        // (rows are uniform over a row's lanes: they share r_in)
        for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < R.n_rows; row += (int64_t)gridDim.x * rpb) {
            float u[V], xh[V], dv[V], dxh[V];
            float s = 0.f;
            for (int rb = 0; rb < walk; rb += span) {
                const int c = rb + cl * V;
                if (c < HD) {
                    load_channels<V>(R.hpre + row * HD + c, u);
#pragma unroll
                    for (int i = 0; i < V; ++i) s += u[i];
                }
            }
            const float mu = row_lanes_sum(s, LPR) * inv_hd;
            float q = 0.f;
            for (int rb = 0; rb < walk; rb += span) {
                const int c = rb + cl * V;
                if (c < HD) {
                    load_channels<V>(R.hpre + row * HD + c, u);
#pragma unroll
                    for (int i = 0; i < V; ++i) q += (u[i] - mu) * (u[i] - mu);
                }
            }
            const float rstd = 1.0f / sqrtf(row_lanes_sum(q, LPR) * inv_hd + A.eps);
            float a1 = 0.f, a2 = 0.f;
            for (int rb = 0; rb < walk; rb += span) {
                const int c = rb + cl * V;
                if (c < HD) {
                    channels(row, c, mu, rstd, u, xh, dv, dxh);
#pragma unroll
                    for (int i = 0; i < V; ++i) { a1 += dxh[i]; a2 += dxh[i] * xh[i]; }
                }
            }
            const float m1 = row_lanes_sum(a1, LPR) * inv_hd, m2 = row_lanes_sum(a2, LPR) * inv_hd;
            if (own) {
                channels(row, c0, mu, rstd, u, xh, dv, dxh);
                const int64_t o = row * HD + c0;
                float rv[V], G[V], ag[V];
#pragma unroll
                for (int i = 0; i < V; ++i) rv[i] = 0.f;
                if (R.res != nullptr) load_channels<V>(R.res + o, rv);
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    G[i] = rstd * (dxh[i] - m1 - xh[i] * m2);
                    ag[i] = u[i] - (rv[i] + bv[i]);
                    sG[i] += G[i]; sg[i] += dv[i] * xh[i]; sb[i] += dv[i];
                }
                if constexpr (V == 4) {
                    *reinterpret_cast<float4*>(R.G + o) = make_float4(G[0], G[1], G[2], G[3]);
                    if (R.agg != nullptr) *reinterpret_cast<float4*>(R.agg + o) = make_float4(ag[0], ag[1], ag[2], ag[3]);
                } else {
                    R.G[o] = G[0];
                    if (R.agg != nullptr) R.agg[o] = ag[0];
                }
            }
        }
        auto flush = [&](const float (&sum)[V], float* __restrict__ partial) {     // (partial: uniform per block)
            if (partial == nullptr) return;
#pragma unroll
            for (int i = 0; i < V; ++i) red[t * V + i] = sum[i];
            __syncthreads();
            if (r_in == 0 && own) {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    float tot = 0.f;
                    for (int r = 0; r < rpb; ++r) tot += red[(r * LPR + cl) * V + i];
                    partial[(int64_t)blockIdx.x * HD + c0 + i] = tot;
                }
            }
            __syncthreads();
        };
        flush(sg, A.part_gamma);
        flush(sb, A.part_beta);
        flush(sG, R.partial);
    }
}

}  // namespace

// ---- launchers -----------------------------------------------------------------------------------------------------
static void res_backward_shape(int32_t HD, int* V, int* LPR, int* rpb) {
    *V = HD % 4 == 0 ? 4 : 1;
    const int groups = HD / *V;                          // column groups of a row
    *LPR = groups < 256 ? groups : 256;
    *rpb = 256 / *LPR;
}
int res_backward_blocks(int64_t n_rows, int32_t HD) {
    int V, LPR, rpb;
    res_backward_shape(HD, &V, &LPR, &rpb);
    const void* fn = V == 4 ? (const void*)res_backward_kernel<4> : (const void*)res_backward_kernel<1>;
    const int64_t want = std::max<int64_t>(1, (n_rows + rpb - 1) / rpb);
    return (int)std::min({want, resident_blocks(fn, 0), (int64_t)kResPartialRows});
}
int launch_res_backward(const ResBwdArgs& a, hipStream_t s) {
    if (a.n_rows <= 0) return 0;
    if (a.blocks < 1 || a.blocks > kResPartialRows) return fail(GAT_E_INVALID, "res_backward: blocks must come from res_backward_blocks()");
    if (a.gh == nullptr && a.g == nullptr) return fail(GAT_E_INVALID, "res_backward: no output gradient");
    int V, LPR, rpb;
    res_backward_shape(a.H * a.D, &V, &LPR, &rpb);
    if (V == 4) hipLaunchKernelGGL(res_backward_kernel<4>, dim3((unsigned)a.blocks), dim3(256), 0, s, a, LPR, rpb);
    else hipLaunchKernelGGL(res_backward_kernel<1>, dim3((unsigned)a.blocks), dim3(256), 0, s, a, LPR, rpb);
    GAT_HIP(hipGetLastError());
    return 0;
}
static void norm_backward_shape(int32_t HD, int* V, int* LPR, int* rpb, bool* one) {
    *V = HD % 4 == 0 ? 4 : 1;
    const int groups = HD / *V;                          // column groups of a row
    int l = 1;
    while (l < groups && l < 64) l <<= 1;                // the row's lanes: a power of two inside one wave
    *LPR = l;
    *rpb = 256 / l;
    *one = groups <= l;
}
static const void* norm_backward_fn(int V, bool one) {
    if (V == 4) return one ? (const void*)norm_backward_kernel<4, true> : (const void*)norm_backward_kernel<4, false>;
    return one ? (const void*)norm_backward_kernel<1, true> : (const void*)norm_backward_kernel<1, false>;
}
int norm_backward_blocks(int64_t n_rows, int32_t HD) {
    int V, LPR, rpb;
    bool one;
    norm_backward_shape(HD, &V, &LPR, &rpb, &one);
    const int64_t want = std::max<int64_t>(1, (n_rows + rpb - 1) / rpb);
    return (int)std::min({want, resident_blocks(norm_backward_fn(V, one), 0), (int64_t)kResPartialRows});
}
int launch_norm_backward(const NormBwdArgs& a, hipStream_t s) {
    if (a.r.n_rows <= 0) return 0;
    if (a.r.blocks < 1 || a.r.blocks > kResPartialRows) return fail(GAT_E_INVALID, "norm_backward: blocks must come from norm_backward_blocks()");
    if (a.r.gh == nullptr && a.r.g == nullptr) return fail(GAT_E_INVALID, "norm_backward: no output gradient");
    if (a.gamma == nullptr || a.beta == nullptr || a.r.G == nullptr || a.r.H < 1 || a.r.D < 1) return fail(GAT_E_INVALID, "norm_backward: null argument");
    int V, LPR, rpb;
    bool one;
    norm_backward_shape(a.r.H * a.r.D, &V, &LPR, &rpb, &one);
    NormBwdArgs arg = a;
    void* args[] = {&arg, &LPR, &rpb};
    GAT_HIP(hipLaunchKernel(norm_backward_fn(V, one), dim3((unsigned)a.r.blocks), dim3(256), args, 0, s));
    return 0;
}
static thread_local ReduceBatch t_batch;
static thread_local bool t_batch_on = false;
void reduce_batch_begin() { t_batch = ReduceBatch{}; t_batch_on = true; }
void reduce_batch_abort() { t_batch_on = false; }
void reduce_batch_pack(const float* loss, const int32_t* correct, float* dst3, float* dst3_host) {
    t_batch.loss = loss; t_batch.correct = correct; t_batch.dst3 = dst3; t_batch.dst3_host = dst3_host;
}
bool reduce_batch_finalize(const double* lp, const int32_t* cp, int32_t nb, float* loss_out, int32_t* correct_out) {
    if (!t_batch_on || t_batch.fin_loss != nullptr) return false;
    t_batch.fin_loss = lp; t_batch.fin_corr = cp; t_batch.fin_n = nb; t_batch.fin_loss_out = loss_out; t_batch.fin_corr_out = correct_out;
    return true;
}
static bool reduce_batch_push(const float* slabs, int32_t nslabs, int64_t width, float* out, int32_t HD, int32_t F, int32_t c_base) {
    if (!t_batch_on || t_batch.n >= 8 || width <= 0) return false;
    ReduceJob& j = t_batch.jobs[t_batch.n++];
    j = ReduceJob{slabs, out, width, nslabs, HD, F, c_base, t_batch.blocks};
    t_batch.blocks += (int32_t)((width + 63) / 64);
    return true;
}
int reduce_batch_flush(hipStream_t s) {
    if (!t_batch_on) return 0;
    t_batch_on = false;
    const int extra = (t_batch.dst3 != nullptr || t_batch.fin_loss != nullptr) ? 1 : 0;
    if (t_batch.blocks + extra == 0) return 0;
    hipLaunchKernelGGL(reduce_batch_kernel, dim3((unsigned)(t_batch.blocks + extra)), dim3(1024), 0, s, t_batch);
    GAT_HIP(hipGetLastError());
    return 0;
}

int launch_reduce_gradw(const float* slabs, int32_t ksplit, int32_t HD, int32_t F, int32_t c_base, int32_t M,
                        float* gradW, hipStream_t s) {
    const int64_t width = (int64_t)M * F;
    if (reduce_batch_push(slabs, ksplit, width, gradW, HD, F, c_base)) return 0;
    hipLaunchKernelGGL((reduce_slabs_kernel<MapGradW>), dim3((unsigned)((width + 63) / 64)), dim3(1024), 0, s, slabs,
                       ksplit, width, gradW, MapGradW{HD, F, c_base});
    GAT_HIP(hipGetLastError());
    return 0;
}

int launch_reduce_partials_add(const float* partial, int32_t nblocks, int64_t width, float* out, hipStream_t s) {
    if (width <= 0) return 0;
    if (reduce_batch_push(partial, nblocks, width, out, 0, 0, 0)) return 0;
    hipLaunchKernelGGL((reduce_slabs_kernel<MapIdentity>), dim3((unsigned)((width + 63) / 64)), dim3(1024), 0, s,
                       partial, nblocks, width, out, MapIdentity{});
    GAT_HIP(hipGetLastError());
    return 0;
}

// Xavier-uniform init on the device (E:186-248): element i of a segment = the (draw0 + i)-th draw of the
// counter-based stream  z_k = splitmix64_finalise(s0 + (k+1)*0x9E3779B97F4A7C15)  mapped to (0, 1] like
// curand_uniform (E:217) and then to (-lim, lim].
__global__ __launch_bounds__(256) void xavier_init_kernel(float* __restrict__ p, int64_t n, uint64_t s0, uint64_t draw0, float lim) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t z = s0 + (draw0 + (uint64_t)i + 1ull) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        const float u = ((float)(z >> 40) + 1.0f) * (1.0f / 16777216.0f);
        p[i] = u * 2.0f * lim - lim;
    }
}
int launch_xavier_init(float* p, int64_t n, uint64_t s0, uint64_t draw0, float lim, hipStream_t s) {
    if (n <= 0) return 0;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(xavier_init_kernel, dim3((unsigned)blocks), dim3(256), 0, s, p, n, s0, draw0, lim);
    GAT_HIP(hipGetLastError());
    return 0;
}

int launch_sgd(float* p, const float* g, float lr, int64_t n, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, g, lr, n);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_adam(float* p, const float* g, float* m, float* v, float lr, int64_t n, float b1, float b2, float eps,
                int32_t t, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, g, m, v, lr, n, b1, b2,
                       eps, t);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_clip(float* g, int64_t n, float thresh, float* scratch, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(sumsq_kernel, dim3(1), dim3(1024), 0, s, g, n, scratch);
    GAT_HIP(hipGetLastError());
    hipLaunchKernelGGL(clip_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, g, n, scratch, thresh);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
