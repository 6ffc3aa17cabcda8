// gat_ops.hip — op-level entry points, ONE PER REFERENCE KERNEL ("one per row a1-a11 (+ head/loss), taking
// device pointers in the reference layouts").  A maintainer can replace a single launch inside the reference's own main()
// — compute_max_sum_attn_score at E:1398, say — and leave the rest of that program as it is: every function takes exactly
// the argument list of the launch it replaces (sizes widened to 64 bit where they count nodes or edges) plus a stream,
// reads and writes caller-owned DEVICE memory in the reference layouts ([H][E] head-major edge tensors, [N][H][D] node
// tensors, W [H][D][2F]) and keeps the reference's accumulate-or-overwrite behaviour.
//
// Same restructuring as the fused path, one stage at a time: wherever the reference recomputes W·x per
// (head, edge) thread, the op projects PL = X·W_left^T / PR = X·W_right^T once per node on the matrix cores
// (launch_project) and the per-edge kernel reads rows of them.  Scratch (PL, PR, gPL, gPR) is allocated per call and freed
// before returning; calls synchronise their stream.  These are the unit-parity seams — the training path is the fused one
// behind gat_step (no [H][E] tensor is materialised there).  Scatters here use float atomics like the reference's own
// kernels (E:422, 783-786, 868-869), so sums over edges are order-dependent at fp32 round-off, as in the reference.
#include "gat_internal.h"

#include <algorithm>

namespace gat {
namespace {

__device__ __forceinline__ float lrelu_f(float v, float s) { return v > 0.f ? v : v * s; }

constexpr int kBlock = 256;
static unsigned grid_for(int64_t work) { return (unsigned)std::min<int64_t>((work + kBlock - 1) / kBlock, (int64_t)1 << 20); }

// a2 (E:303-323): score[h][e] = sum_k a[h][k] * LReLU(PL[src][h][k] + PR[dst][h][k]); one thread per (e, h), h fastest:
// the H threads of an edge read its two rows contiguously.
__global__ __launch_bounds__(kBlock) void op_edge_score_kernel(const float* __restrict__ PL, const float* __restrict__ PR,
                                                              const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                              const float* __restrict__ a, float* __restrict__ score,
                                                              int64_t E, int32_t H, int32_t D, float slope) {
    const int64_t total = E * H, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t e = t / H;
        const int h = (int)(t % H);
        const float* pl = PL + ((int64_t)src[e] * H + h) * D;
        const float* pr = PR + ((int64_t)dst[e] * H + h) * D;
        float acc = 0.f;
        for (int k = 0; k < D; ++k) acc += a[h * D + k] * lrelu_f(pl[k] + pr[k], slope);
        score[(int64_t)h * E + e] = acc;
    }
}

// a3 (E:326-359): one wave per destination row, heads one after the other, lanes striding the row's edges; max seeded with
// -1e9f (E:336), sum of __expf(score - max) (E:349).  max[N*h + dst], sum[N*h + dst].
__global__ __launch_bounds__(kBlock) void op_max_sum_kernel(const int32_t* __restrict__ row_ptr, const float* __restrict__ score,
                                                           int64_t N, int32_t H, int64_t E, float* __restrict__ mx,
                                                           float* __restrict__ sm) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); row < N; row += waves) {
        const int b = row_ptr[row], e = row_ptr[row + 1];
        for (int h = 0; h < H; ++h) {
            const float* sc = score + (int64_t)h * E;
            float m = -1e9f;
            for (int i = b + lane; i < e; i += 64) m = fmaxf(m, sc[i]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
            float z = 0.f;
            for (int i = b + lane; i < e; i += 64) z += __expf(sc[i] - m);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off);
            if (lane == 0) { mx[N * h + row] = m; sm[N * h + row] = z; }
        }
    }
}

// a4 (E:362-384): alpha = __expf(score - max[dst + N*h]) / (sum[dst + N*h] + 1e-8f), thread per tid = h*E + e
__global__ __launch_bounds__(kBlock) void op_attn_coeff_kernel(const int32_t* __restrict__ dst, const float* __restrict__ score,
                                                              const float* __restrict__ mx, const float* __restrict__ sm,
                                                              float* __restrict__ alpha, int64_t E, int32_t H, int64_t N) {
    const int64_t total = E * H, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t h = t / E, e = t % E;
        const int64_t off = dst[e] + N * h;
        alpha[t] = __expf(score[t] - mx[off]) / (sm[off] + 1e-8f);
    }
}

// a5 (E:386-424): out[dst][h][k] += alpha[h][e] * PL[src][h][k]  (atomicAdd like E:422: the caller zeroes);
// one thread per (e, channel), channel fastest: coalesced row reads and 4*HD-byte atomic bursts
__global__ __launch_bounds__(kBlock) void op_aggregate_kernel(const float* __restrict__ PL, const int32_t* __restrict__ src,
                                                             const int32_t* __restrict__ dst, const float* __restrict__ alpha,
                                                             float* __restrict__ out, int64_t E, int32_t H, int32_t D) {
    const int HD = H * D;
    const int64_t total = E * HD, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t e = t / HD;
        const int c = (int)(t % HD);
        atomicAdd(out + (int64_t)dst[e] * HD + c, alpha[(int64_t)(c / D) * E + e] * PL[(int64_t)src[e] * HD + c]);
    }
}

// a6 (E:426-459): LeakyReLU, then concat (hidden) or mean over heads (last); thread per output element
__global__ __launch_bounds__(kBlock) void op_post_activation_kernel(const float* __restrict__ hpre, float* __restrict__ out,
                                                                   int64_t N, int32_t H, int32_t D, int32_t is_last, float slope) {
    const int64_t total = N * (is_last ? D : H * D), stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        if (!is_last) { out[t] = lrelu_f(hpre[t], slope); continue; }
        const int64_t n = t / D;
        const int d = (int)(t % D);
        float s = 0.f;
        for (int h = 0; h < H; ++h) s += lrelu_f(hpre[(n * H + h) * D + d], slope);
        out[t] = s / (float)H;
    }
}

// C12 (E:463-512 with softmax E:132-141): z = W_o x, softmax with the DOUBLE-literal epsilon of E:140; both d_z and d_y end
// up holding the probabilities, as in the reference (softmax runs in place on node_z, then is copied).  Thread per node,
// same loop order as the reference (classes outer, features inner).
__global__ __launch_bounds__(kBlock) void op_output_head_kernel(const float* __restrict__ Wo, const float* __restrict__ HL,
                                                               float* __restrict__ z, float* __restrict__ y, int64_t N, int32_t C,
                                                               int32_t DL) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride) {
        const float* x = HL + n * DL;
        float* zn = z + n * C;
        float m = -INFINITY;
        for (int c = 0; c < C; ++c) {
            float acc = 0.f;
            for (int j = 0; j < DL; ++j) acc += Wo[c * DL + j] * x[j];
            zn[c] = acc;
            m = fmaxf(m, acc);
        }
        float s = 0.f;
        for (int c = 0; c < C; ++c) { const float v = expf(zn[c] - m); zn[c] = v; s += v; }
        for (int c = 0; c < C; ++c) {
            const float p = (float)((double)zn[c] / ((double)s + 1e-8));
            zn[c] = p;
            y[n * C + c] = p;
        }
    }
}

// C13 (E:514-537): per-node cross-entropy with the 1e-12f clamp and the strict-> arg-max
__global__ __launch_bounds__(kBlock) void op_loss_accuracy_kernel(const float* __restrict__ y, const int32_t* __restrict__ labels,
                                                                 float* __restrict__ loss, int32_t* __restrict__ correct, int64_t N,
                                                                 int32_t C) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride) {
        const int label = labels[n];
        loss[n] = -logf(fmaxf(y[n * C + label], 1e-12f));
        float mv = y[n * C];
        int pred = 0;
        for (int c = 1; c < C; ++c) { const float v = y[n * C + c]; if (v > mv) { mv = v; pred = c; } }
        correct[n] = pred == label;
    }
}

// C14 (E:553-608): dz = y - onehot; grad_Wo[c][d] += sum_n dz[c] H_L[n][d] (block partials in LDS, one atomicAdd per block
// and element); grad_hL[n][h][d] = (sum_c Wo[c][d] dz[c]) * LReLU'(.) / H with the exact per-head pre-activation, or the
// reference's flat index n*D + d (E:598) when flat_index is set
__global__ __launch_bounds__(kBlock) void op_output_gradients_kernel(const float* __restrict__ y, const int32_t* __restrict__ labels,
                                                                    const float* __restrict__ hL, const float* __restrict__ HL,
                                                                    const float* __restrict__ Wo, float* __restrict__ gradWo,
                                                                    float* __restrict__ gradhL, int64_t N, int32_t C, int32_t DL,
                                                                    int32_t H, float slope, int32_t flat_index) {
    extern __shared__ float sh[];                    // [C*DL] partial of grad_Wo
    for (int i = threadIdx.x; i < C * DL; i += blockDim.x) sh[i] = 0.f;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += stride) {
        const int label = labels[n];
        for (int d = 0; d < DL; ++d) {
            float s = 0.f;
            const float hv = HL[n * DL + d];
            for (int c = 0; c < C; ++c) {
                const float dz = y[n * C + c] - (c == label ? 1.0f : 0.0f);
                s += Wo[c * DL + d] * dz;
                atomicAdd(&sh[c * DL + d], dz * hv);
            }
            const float inv_heads = 1.0f / (float)H;
            for (int h = 0; h < H; ++h) {
                const float pre = flat_index ? hL[n * DL + d] : hL[(n * H + h) * DL + d];
                gradhL[(n * H + h) * DL + d] = s * (pre > 0.f ? 1.0f : slope) * inv_heads;
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * DL; i += blockDim.x) atomicAdd(&gradWo[i], sh[i]);
}

// a7 (E:612-651): galpha[h][e] = sum_k g[dst][h][k] * PL[src][h][k]; thread per (e, h), h fastest
__global__ __launch_bounds__(kBlock) void op_grad_attn_coeff_kernel(const float* __restrict__ PL, const float* __restrict__ g,
                                                                   const int32_t* __restrict__ src, const int32_t* __restrict__ dst,
                                                                   float* __restrict__ galpha, int64_t E, int32_t H, int32_t D) {
    const int64_t total = E * H, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t e = t / H;
        const int h = (int)(t % H);
        const float* pl = PL + ((int64_t)src[e] * H + h) * D;
        const float* gj = g + ((int64_t)dst[e] * H + h) * D;
        float acc = 0.f;
        for (int k = 0; k < D; ++k) acc += gj[k] * pl[k];
        galpha[(int64_t)h * E + e] = acc;
    }
}

// a8 (E:654-696): ge_ij = sum_k galpha_kj alpha_kj (delta_ik - alpha_ij) = alpha_ij (galpha_ij - sum_k galpha_kj alpha_kj):
// one pass per (row, head) for the row's dot product, one to write — O(E) instead of the reference's O(sum deg^2).
// One wave per destination row.
__global__ __launch_bounds__(kBlock) void op_grad_attn_score_kernel(const int32_t* __restrict__ row_ptr, const float* __restrict__ alpha,
                                                                   const float* __restrict__ galpha, float* __restrict__ ge,
                                                                   int64_t N, int32_t H, int64_t E) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); row < N; row += waves) {
        const int b = row_ptr[row], e = row_ptr[row + 1];
        for (int h = 0; h < H; ++h) {
            const float* al = alpha + (int64_t)h * E;
            const float* ga = galpha + (int64_t)h * E;
            float dot = 0.f;
            for (int i = b + lane; i < e; i += 64) dot += ga[i] * al[i];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off);
            for (int i = b + lane; i < e; i += 64) ge[(int64_t)h * E + i] = al[i] * (ga[i] - dot);
        }
    }
}

// a9 / a10 edge part (E:746-786, 840-869): per (e, channel c = h*D + k), s = PL[src][c] + PR[dst][c],
//   gs = ge[h][e] * a[c] * LReLU'(s);  gPL[src][c] += g[dst][c] * alpha[h][e] + gs;  gPR[dst][c] += gs   (float atomics),
//   and (WITH_GA) grad_a[c] += ge * LReLU(s) through a per-block LDS partial
template <bool WITH_GA>
__global__ __launch_bounds__(kBlock) void op_messages_kernel(const float* __restrict__ PL, const float* __restrict__ PR,
                                                            const float* __restrict__ g, const int32_t* __restrict__ src,
                                                            const int32_t* __restrict__ dst, const float* __restrict__ alpha,
                                                            const float* __restrict__ ge, const float* __restrict__ a,
                                                            float* __restrict__ gPL, float* __restrict__ gPR, float* __restrict__ grad_a,
                                                            int64_t E, int32_t H, int32_t D, float slope) {
    extern __shared__ float sh_ga[];                 // [HD]
    const int HD = H * D;
    if constexpr (WITH_GA) {
        for (int i = threadIdx.x; i < HD; i += blockDim.x) sh_ga[i] = 0.f;
        __syncthreads();
    }
    const int64_t total = E * HD, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const int64_t e = t / HD;
        const int c = (int)(t % HD);
        const int64_t s_ = src[e], d_ = dst[e];
        const int64_t he = (int64_t)(c / D) * E + e;
        const float s = PL[s_ * HD + c] + PR[d_ * HD + c];
        const float gev = ge[he];
        const float gs = gev * a[c] * (s > 0.f ? 1.0f : slope);
        atomicAdd(gPL + s_ * HD + c, g[d_ * HD + c] * alpha[he] + gs);
        atomicAdd(gPR + d_ * HD + c, gs);
        if constexpr (WITH_GA) atomicAdd(&sh_ga[c], gev * lrelu_f(s, slope));
    }
    if constexpr (WITH_GA) {
        __syncthreads();
        for (int i = threadIdx.x; i < HD; i += blockDim.x) atomicAdd(&grad_a[i], sh_ga[i]);
    }
}

__global__ __launch_bounds__(kBlock) void op_add_kernel(float* __restrict__ out, const float* __restrict__ add, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] += add[i];
}

// a11 (E:879-893): gx *= LReLU'(h_pre_prev), in place
__global__ __launch_bounds__(kBlock) void op_preact_gradient_kernel(const float* __restrict__ hpre, float* __restrict__ gx, int64_t n,
                                                                   float slope) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) gx[i] *= hpre[i] > 0.f ? 1.0f : slope;
}

static int check_shape(int64_t n, int64_t e, int32_t f, int32_t h, int32_t d) {
    if (n <= 0 || e < 0 || f <= 0 || h <= 0 || d <= 0) return fail(GAT_E_INVALID, "op: bad sizes");
    if (n > 0x7fffffffLL || e > 0x7fffffffLL) return fail(GAT_E_UNSUPPORTED, "op: int32 CSR limits (E:1045-1046) exceeded");
    return 0;
}
static int project(Scratch& t, const float* x, const float* w, int64_t n, int32_t f, int32_t hd, float** PL, float** PR, hipStream_t s) {
    GAT_TRY(t.get(PL, n * hd));
    GAT_TRY(t.get(PR, n * hd));
    return launch_project(x, w, *PL, *PR, n, f, hd, kPartBoth, false, nullptr, 0, s);
}
// gPL / gPR of one layer from reference-layout inputs (shared by a9 and a10)
static int messages(Scratch& t, int64_t n, int32_t h, int64_t e, int32_t f, int32_t d, float slope, const int32_t* src, const int32_t* dst,
                    const float* alpha, const float* x, const float* w, const float* g, const float* ge, const float* a, float* grad_a,
                    float** gPL, float** gPR, hipStream_t s) {
    const int hd = h * d;
    float *PL, *PR;
    GAT_TRY(project(t, x, w, n, f, hd, &PL, &PR, s));
    GAT_TRY(t.get(gPL, n * hd));
    GAT_TRY(t.get(gPR, n * hd));
    GAT_HIP(hipMemsetAsync(*gPL, 0, (size_t)n * hd * sizeof(float), s));
    GAT_HIP(hipMemsetAsync(*gPR, 0, (size_t)n * hd * sizeof(float), s));
    if (e > 0) {
        if (grad_a) hipLaunchKernelGGL(op_messages_kernel<true>, dim3(grid_for(e * hd)), dim3(kBlock), (size_t)hd * sizeof(float), s, PL, PR, g, src, dst,
                                       alpha, ge, a, *gPL, *gPR, grad_a, e, h, d, slope);
        else hipLaunchKernelGGL(op_messages_kernel<false>, dim3(grid_for(e * hd)), dim3(kBlock), 0, s, PL, PR, g, src, dst, alpha, ge, a, *gPL, *gPR,
                                (float*)nullptr, e, h, d, slope);
        GAT_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace
}  // namespace gat

using namespace gat;

extern "C" {

int gat_op_edge_score(const float* d_x, const int32_t* d_col_idx, const int32_t* d_dst, const float* d_w, const float* d_a,
                      float* d_attn_score, int64_t n, int32_t in_dim, int32_t out_dim, int32_t h, int64_t e, float slope, void* stream) {
    if (!d_x || !d_w || !d_a || (e > 0 && (!d_col_idx || !d_dst || !d_attn_score))) return fail(GAT_E_INVALID, "gat_op_edge_score: null argument");
    GAT_TRY(check_shape(n, e, in_dim, h, out_dim));
    if (e == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    Scratch t;
    float *PL, *PR;
    GAT_TRY(project(t, d_x, d_w, n, in_dim, h * out_dim, &PL, &PR, s));
    hipLaunchKernelGGL(op_edge_score_kernel, dim3(grid_for(e * h)), dim3(kBlock), 0, s, PL, PR, d_col_idx, d_dst, d_a, d_attn_score, e, h, out_dim, slope);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_max_sum(const int32_t* d_row_ptr, const float* d_attn_score, int64_t n, int32_t h, int64_t e, float* d_max, float* d_sum, void* stream) {
    if (!d_row_ptr || !d_max || !d_sum || (e > 0 && !d_attn_score)) return fail(GAT_E_INVALID, "gat_op_max_sum: null argument");
    GAT_TRY(check_shape(n, e, 1, h, 1));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_max_sum_kernel, dim3(grid_for(n * 64)), dim3(kBlock), 0, s, d_row_ptr, d_attn_score, n, h, e, d_max, d_sum);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_attn_coeff(const int32_t* d_col_idx, const int32_t* d_dst, const float* d_attn_score, const float* d_max, const float* d_sum,
                      float* d_attn_coeff, int64_t e, int32_t h, int64_t n, void* stream) {
    (void)d_col_idx;                                 // carried by the reference's signature (E:362), never read there either
    if (e > 0 && (!d_dst || !d_attn_score || !d_max || !d_sum || !d_attn_coeff)) return fail(GAT_E_INVALID, "gat_op_attn_coeff: null argument");
    GAT_TRY(check_shape(n, e, 1, h, 1));
    if (e == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_attn_coeff_kernel, dim3(grid_for(e * h)), dim3(kBlock), 0, s, d_dst, d_attn_score, d_max, d_sum, d_attn_coeff, e, h, n);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_aggregate(const int32_t* d_src, const int32_t* d_dst, const float* d_attn_coeff, const float* d_in_feat, const float* d_w,
                     float* d_out_feat, int64_t n, int32_t h, int64_t e, int32_t in_dim, int32_t out_dim, void* stream) {
    if (!d_in_feat || !d_w || !d_out_feat || (e > 0 && (!d_src || !d_dst || !d_attn_coeff))) return fail(GAT_E_INVALID, "gat_op_aggregate: null argument");
    GAT_TRY(check_shape(n, e, in_dim, h, out_dim));
    if (e == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    Scratch t;
    float* PL;
    GAT_TRY(t.get(&PL, n * h * out_dim));
    GAT_TRY(launch_project(d_in_feat, d_w, PL, nullptr, n, in_dim, h * out_dim, kPartLeft, false, nullptr, 0, s));
    hipLaunchKernelGGL(op_aggregate_kernel, dim3(grid_for(e * h * out_dim)), dim3(kBlock), 0, s, PL, d_src, d_dst, d_attn_coeff, d_out_feat, e, h, out_dim);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_post_activation(const float* d_out_feat, float* d_H, int64_t n, int32_t h, int32_t out_dim, int32_t is_last, float slope, void* stream) {
    if (!d_out_feat || !d_H) return fail(GAT_E_INVALID, "gat_op_post_activation: null argument");
    GAT_TRY(check_shape(n, 0, 1, h, out_dim));
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_post_activation_kernel, dim3(grid_for(n * h * out_dim)), dim3(kBlock), 0, s, d_out_feat, d_H, n, h, out_dim, is_last, slope);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_output_head(const float* d_wo, const float* d_last_layer_output, float* d_z, float* d_y, int64_t n, int32_t c, int32_t out_dim_last, void* stream) {
    if (!d_wo || !d_last_layer_output || !d_z || !d_y) return fail(GAT_E_INVALID, "gat_op_output_head: null argument");
    if (n <= 0 || c <= 0 || out_dim_last <= 0) return fail(GAT_E_INVALID, "gat_op_output_head: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_output_head_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, d_wo, d_last_layer_output, d_z, d_y, n, c, out_dim_last);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_loss_accuracy(const float* d_y, const int32_t* d_labels, float* d_losses, int32_t* d_corrects, int64_t n, int32_t c, void* stream) {
    if (!d_y || !d_labels || !d_losses || !d_corrects) return fail(GAT_E_INVALID, "gat_op_loss_accuracy: null argument");
    if (n <= 0 || c <= 0) return fail(GAT_E_INVALID, "gat_op_loss_accuracy: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_loss_accuracy_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, d_y, d_labels, d_losses, d_corrects, n, c);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_output_gradients(const float* d_y, const int32_t* d_labels, const float* d_hL, const float* d_HL, const float* d_wo, float* grad_d_wo,
                            float* grad_d_hL, int64_t n, int32_t c, int32_t out_dim_l, int32_t num_heads, float slope, int32_t flat_lrelu_index,
                            void* stream) {
    if (!d_y || !d_labels || !d_hL || !d_HL || !d_wo || !grad_d_wo || !grad_d_hL) return fail(GAT_E_INVALID, "gat_op_output_gradients: null argument");
    if (n <= 0 || c <= 0 || out_dim_l <= 0 || num_heads <= 0) return fail(GAT_E_INVALID, "gat_op_output_gradients: bad sizes");
    if ((size_t)c * out_dim_l * sizeof(float) > 60 * 1024) return fail(GAT_E_UNSUPPORTED, "gat_op_output_gradients: C * D_L beyond the LDS partial");
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + kBlock - 1) / kBlock, 1024);
    hipLaunchKernelGGL(op_output_gradients_kernel, dim3(blocks), dim3(kBlock), (size_t)c * out_dim_l * sizeof(float), s, d_y, d_labels, d_hL, d_HL, d_wo,
                       grad_d_wo, grad_d_hL, n, c, out_dim_l, num_heads, slope, flat_lrelu_index);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_grad_attn_coeff(int64_t e, int32_t h, int32_t in_dim, int32_t out_dim, const int32_t* d_src, const int32_t* d_dst, const float* d_features,
                           const float* d_w, const float* d_grad_input, float* d_grad_attn_coeff, int64_t n, void* stream) {
    if (!d_features || !d_w || !d_grad_input || (e > 0 && (!d_src || !d_dst || !d_grad_attn_coeff))) return fail(GAT_E_INVALID, "gat_op_grad_attn_coeff: null argument");
    GAT_TRY(check_shape(n, e, in_dim, h, out_dim));
    if (e == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    Scratch t;
    float* PL;
    GAT_TRY(t.get(&PL, n * h * out_dim));
    GAT_TRY(launch_project(d_features, d_w, PL, nullptr, n, in_dim, h * out_dim, kPartLeft, false, nullptr, 0, s));
    hipLaunchKernelGGL(op_grad_attn_coeff_kernel, dim3(grid_for(e * h)), dim3(kBlock), 0, s, PL, d_grad_input, d_src, d_dst, d_grad_attn_coeff, e, h, out_dim);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_grad_attn_score(const int32_t* d_row_ptr, const int32_t* d_dst, const float* d_alpha, const float* d_grad_alpha, float* d_grad_e, int64_t n,
                           int32_t h, int64_t e, void* stream) {
    (void)d_dst;                                     // the reference finds the row through d_dst (E:671); the rows are walked directly here
    if (!d_row_ptr || (e > 0 && (!d_alpha || !d_grad_alpha || !d_grad_e))) return fail(GAT_E_INVALID, "gat_op_grad_attn_score: null argument");
    GAT_TRY(check_shape(n, e, 1, h, 1));
    if (e == 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_grad_attn_score_kernel, dim3(grid_for(n * 64)), dim3(kBlock), 0, s, d_row_ptr, d_alpha, d_grad_alpha, d_grad_e, n, h, e);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_grad_parameters(int64_t e, int32_t h, const int32_t* d_src, const int32_t* d_dst, const float* d_features, const float* d_input_gradients,
                           const float* d_grad_attn_score, const float* d_attn_coeff, const float* d_w, const float* d_a, float* grad_w, float* grad_a,
                           int32_t in_dim, int32_t out_dim, float slope, int64_t n, void* stream) {
    if (!d_features || !d_input_gradients || !d_w || !d_a || !grad_w || !grad_a || (e > 0 && (!d_src || !d_dst || !d_grad_attn_score || !d_attn_coeff)))
        return fail(GAT_E_INVALID, "gat_op_grad_parameters: null argument");
    GAT_TRY(check_shape(n, e, in_dim, h, out_dim));
    hipStream_t s = (hipStream_t)stream;
    Scratch t;
    float *gPL, *gPR, *scr;
    GAT_TRY(messages(t, n, h, e, in_dim, out_dim, slope, d_src, d_dst, d_attn_coeff, d_features, d_w, d_input_gradients, d_grad_attn_score, d_a, grad_a, &gPL, &gPR, s));
    GAT_TRY(t.get(&scr, grad_w_scratch_floats(n, in_dim, h * out_dim)));
    GAT_TRY(launch_grad_w(gPL, gPR, d_features, grad_w, scr, n, in_dim, h * out_dim, kPartBoth, s));
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_features_input_gradients(int64_t n, int32_t h, int64_t e, int32_t in_dim, int32_t out_dim, float slope, const int32_t* d_src,
                                    const int32_t* d_dst, const float* d_attn_coeff, const float* d_input_features, const float* d_w,
                                    const float* d_input_gradients, const float* d_grad_attn_score, const float* d_a, float* d_grad_x_features,
                                    void* stream) {
    if (!d_input_features || !d_w || !d_input_gradients || !d_a || !d_grad_x_features || (e > 0 && (!d_src || !d_dst || !d_attn_coeff || !d_grad_attn_score)))
        return fail(GAT_E_INVALID, "gat_op_features_input_gradients: null argument");
    GAT_TRY(check_shape(n, e, in_dim, h, out_dim));
    hipStream_t s = (hipStream_t)stream;
    Scratch t;
    float *gPL, *gPR, *gx;
    GAT_TRY(messages(t, n, h, e, in_dim, out_dim, slope, d_src, d_dst, d_attn_coeff, d_input_features, d_w, d_input_gradients, d_grad_attn_score, d_a, nullptr, &gPL, &gPR, s));
    GAT_TRY(t.get(&gx, n * in_dim));
    GAT_TRY(launch_grad_x(gPL, gPR, d_w, nullptr, gx, n, in_dim, h * out_dim, slope, s));
    hipLaunchKernelGGL(op_add_kernel, dim3(grid_for(n * in_dim)), dim3(kBlock), 0, s, d_grad_x_features, gx, n * in_dim);     // accumulates like E:868-869
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_preact_gradient(int64_t n, float slope, int32_t in_dim, const float* d_pre_activation, float* d_gradients, void* stream) {
    if (!d_pre_activation || !d_gradients) return fail(GAT_E_INVALID, "gat_op_preact_gradient: null argument");
    if (n <= 0 || in_dim <= 0) return fail(GAT_E_INVALID, "gat_op_preact_gradient: bad sizes");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(op_preact_gradient_kernel, dim3(grid_for(n * in_dim)), dim3(kBlock), 0, s, d_pre_activation, d_gradients, n * in_dim, slope);
    GAT_HIP(hipGetLastError());
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_csr_to_coo(const int32_t* d_row_ptr, const int32_t* d_col_idx, int32_t* d_src, int32_t* d_dst,
                      int64_t n_rows, int64_t n_edges, void* stream) {
    if (!d_row_ptr || !d_src || !d_dst || (!d_col_idx && n_edges > 0)) return fail(GAT_E_INVALID, "null argument");
    return launch_csr_to_coo(d_row_ptr, d_col_idx, d_src, d_dst, n_rows, n_edges, 0, (hipStream_t)stream);
}

int gat_op_layer_forward(const int32_t* d_row_ptr, const int32_t* d_col_idx, const float* d_x, const float* d_w,
                         const float* d_a, float* d_attn_coeff, float* d_hpre, float* d_hout, int64_t n, int64_t e,
                         int32_t f, int32_t h, int32_t d, int32_t is_last, float slope, void* stream) {
    if (!d_row_ptr || !d_x || !d_w || !d_a || !d_attn_coeff || !d_hpre || !d_hout) return fail(GAT_E_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int HD = h * d;
    Scratch t; ScratchWorkList wl;
    float *PL, *PR, *alpha, *ms, *zs;
    GAT_TRY(t.get(&PL, n * HD)); GAT_TRY(t.get(&PR, n * HD)); GAT_TRY(t.get(&alpha, e * h));
    GAT_TRY(t.get(&ms, n * h)); GAT_TRY(t.get(&zs, n * h));
    GAT_TRY(launch_project(d_x, d_w, PL, PR, n, f, HD, kPartBoth, false, nullptr, 0, s));
    EdgeFwdArgs a{};
    a.row_ptr = d_row_ptr; a.col_idx = d_col_idx; a.PL = PL; a.PR = PR; a.a = d_a; a.alpha = alpha;
    a.mstat = ms; a.zstat = zs;
    a.hpre = d_hpre; a.hout = d_hout; a.n_rows = n; a.n_table = n; a.H = h; a.D = d; a.is_last = is_last; a.slope = slope;
    GAT_TRY(wl.build(t, d_row_ptr, n, HD, h, s));
    set_work_list(a, wl.w, wl.items, wl.slot_info, wl.part_acc, wl.part_mz);
    GAT_TRY(launch_edge_forward(a, s));
    GAT_TRY(launch_transpose_eh_to_he(alpha, d_attn_coeff, e, h, s));
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

int gat_op_layer_backward(const int32_t* d_row_ptr, const int32_t* d_col_idx, const float* d_x, const float* d_w,
                          const float* d_a, const float* d_attn_coeff, const float* d_hpre, const float* d_g,
                          float* d_grad_w, float* d_grad_a, const float* d_hpre_prev, float* d_g_prev, int64_t n,
                          int64_t e, int32_t f, int32_t h, int32_t d, float slope, void* stream) {
    if (!d_row_ptr || !d_x || !d_w || !d_a || !d_attn_coeff || !d_hpre || !d_g || !d_grad_w || !d_grad_a)
        return fail(GAT_E_INVALID, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int HD = h * d;
    Scratch t; ScratchWorkList wl;
    if (!d_col_idx) {                  // e == 0: the kernels still clamp their index prefetch to edge 0 — give them one to read
        int32_t* dummy = nullptr;
        GAT_TRY(t.get(&dummy, 1));
        GAT_HIP(hipMemsetAsync(dummy, 0, sizeof(int32_t), s));
        d_col_idx = dummy;
    }
    float *PL, *PR, *alpha, *gPL, *gPR, *gap, *scr;
    GAT_TRY(t.get(&PL, n * HD)); GAT_TRY(t.get(&PR, n * HD)); GAT_TRY(t.get(&alpha, e * h));
    GAT_TRY(t.get(&gPL, n * HD)); GAT_TRY(t.get(&gPR, n * HD)); GAT_TRY(t.get(&gap, (int64_t)kGaPartialRows * HD));    // capacity: >= any edge_backward_blocks()
    GAT_TRY(t.get(&scr, grad_w_scratch_floats(n, f, HD)));
    GAT_TRY(launch_project(d_x, d_w, PL, PR, n, f, HD, kPartBoth, false, nullptr, 0, s));
    GAT_TRY(launch_transpose_he_to_eh(d_attn_coeff, alpha, e, h, s));
    GAT_TRY(wl.build(t, d_row_ptr, n, HD, h, s));
    // softmax stats of this layer (the fast-path backward recomputes alpha from them): one
    // forward edge pass into scratch outputs
    float *ms, *zs, *hp_tmp, *ho_tmp;
    GAT_TRY(t.get(&ms, n * h)); GAT_TRY(t.get(&zs, n * h)); GAT_TRY(t.get(&hp_tmp, n * HD)); GAT_TRY(t.get(&ho_tmp, n * HD));
    {
        EdgeFwdArgs fa{};
        fa.row_ptr = d_row_ptr; fa.col_idx = d_col_idx; fa.PL = PL; fa.PR = PR; fa.a = d_a;
        fa.alpha = edge_fast_path(h, d, n) ? nullptr : alpha; fa.hpre = hp_tmp; fa.hout = ho_tmp; fa.mstat = ms; fa.zstat = zs;
        fa.n_rows = n; fa.n_table = n; fa.H = h; fa.D = d; fa.is_last = 0; fa.slope = slope;
        set_work_list(fa, wl.w, wl.items, wl.slot_info, wl.part_acc, wl.part_mz);
        GAT_TRY(launch_edge_forward(fa, s));
    }
    GAT_HIP(hipMemsetAsync(gPL, 0, (size_t)n * HD * sizeof(float), s));
    EdgeBwdArgs a{};
    a.mstat = ms; a.zstat = zs;
    a.row_ptr = d_row_ptr; a.col_idx = d_col_idx; a.PL = PL; a.PR = PR; a.a = d_a; a.alpha = alpha;
    a.hpre = d_hpre; a.g = d_g; a.gPL = gPL; a.gPR = gPR; a.ge = nullptr; a.ga_partial = gap;
    a.n_rows = n; a.n_table = n; a.H = h; a.D = d; a.slope = slope;
    set_work_list(a, wl.w, wl.items, wl.slot_info, wl.part_acc, wl.part_mz);
    a.ga_blocks = edge_backward_blocks(a);
    GAT_TRY(launch_edge_backward(a, s));
    GAT_TRY(launch_reduce_partials_add(gap, a.ga_blocks, HD, d_grad_a, s));
    GAT_TRY(launch_grad_w(gPL, gPR, d_x, d_grad_w, scr, n, f, HD, kPartBoth, s));
    if (d_hpre_prev && d_g_prev) GAT_TRY(launch_grad_x(gPL, gPR, d_w, d_hpre_prev, d_g_prev, n, f, HD, slope, s));
    GAT_HIP(hipStreamSynchronize(s));
    return 0;
}

// The two kernels on caller-owned device pointers.  The graph_ptr is checked on the device before anything reads through it.
static int op_readout_check(const char* who, const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t width, int32_t mode, hipStream_t s) {
    if (!d_graph_ptr) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (mode < GAT_READOUT_MEAN || mode > GAT_READOUT_MAX) return fail(GAT_E_INVALID, std::string(who) + ": mode must be 1 (mean), 2 (sum) or 3 (max)");
    if (n_graphs < 1 || n_graphs >= 0x7fffffffLL || n_rows < 0 || n_rows >= 0x7fffffffLL || width < 1) return fail(GAT_E_INVALID, std::string(who) + ": bad sizes");
    int32_t problem = 0; int64_t where = -1;
    GAT_TRY(graph_ptr_check_device(d_graph_ptr, n_graphs, n_rows, &problem, &where, s));
    if (problem) return fail(GAT_E_INVALID, std::string(who) + ": " + graph_ptr_problem_text(problem, where, n_rows));
    return 0;
}
int gat_op_readout_forward(const float* d_x, int64_t x_stride, const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows,
                           int32_t width, int32_t mode, float* d_pooled, int32_t* d_argmax, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GAT_TRY(op_readout_check("gat_op_readout_forward", d_graph_ptr, n_graphs, n_rows, width, mode, s));
    if ((!d_x && n_rows > 0) || !d_pooled || (mode == GAT_READOUT_MAX && !d_argmax)) return fail(GAT_E_INVALID, "gat_op_readout_forward: null argument");
    if (x_stride < width) return fail(GAT_E_INVALID, "gat_op_readout_forward: x_stride below width");
    std::vector<int32_t> gp((size_t)n_graphs + 1);
    GAT_HIP(hipMemcpy(gp.data(), d_graph_ptr, gp.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    ReadoutPlan plan;
    build_readout_plan(gp.data(), n_graphs, plan);
    Scratch tmp;
    int4 *items = nullptr, *split = nullptr; float* part = nullptr; int32_t* part_arg = nullptr;
    GAT_TRY(tmp.get(&items, plan.n_items)); GAT_TRY(tmp.get(&split, plan.n_split));
    GAT_TRY(tmp.get(&part, (int64_t)plan.n_parts * width)); GAT_TRY(tmp.get(&part_arg, (int64_t)plan.n_parts * width));
    GAT_HIP(hipMemcpyAsync(items, plan.items.data(), plan.items.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (plan.n_split > 0) GAT_HIP(hipMemcpyAsync(split, plan.split.data(), plan.split.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ReadoutFwdArgs a{};
    a.x = d_x ? d_x : d_pooled; a.x_stride = x_stride; a.graph_ptr = d_graph_ptr;      // (n_rows == 0: no item has a row to load)
    a.items = items; a.n_items = plan.n_items; a.split = split; a.n_split = plan.n_split;
    a.pooled = d_pooled; a.argmax = d_argmax; a.part = part; a.part_arg = part_arg; a.width = width; a.mode = mode;
    int rc = launch_readout_forward(a, s);
    const hipError_t e = hipStreamSynchronize(s);        // before the scratch is freed
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string("gat_op_readout_forward: ") + hipGetErrorString(e));
    return rc;
}
int gat_op_readout_backward(const float* d_gpooled, const int32_t* d_graph_ptr, int64_t n_graphs, int64_t n_rows, int32_t width,
                            int32_t mode, const int32_t* d_argmax, float* d_gh, int64_t gh_stride, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GAT_TRY(op_readout_check("gat_op_readout_backward", d_graph_ptr, n_graphs, n_rows, width, mode, s));
    if (!d_gpooled || (!d_gh && n_rows > 0) || (mode == GAT_READOUT_MAX && !d_argmax)) return fail(GAT_E_INVALID, "gat_op_readout_backward: null argument");
    if (gh_stride < width) return fail(GAT_E_INVALID, "gat_op_readout_backward: gh_stride below width");
    if (n_rows == 0) return 0;
    Scratch tmp;
    int32_t* node_graph = nullptr;
    GAT_TRY(tmp.get(&node_graph, n_rows));
    GAT_TRY(launch_node_graph(d_graph_ptr, n_graphs, n_rows, node_graph, s));
    ReadoutBwdArgs a{};
    a.gpooled = d_gpooled; a.argmax = d_argmax; a.graph_ptr = d_graph_ptr; a.node_graph = node_graph;
    a.gh = d_gh; a.gh_stride = gh_stride; a.n_rows = n_rows; a.width = width; a.mode = mode;
    int rc = launch_readout_backward(a, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string("gat_op_readout_backward: ") + hipGetErrorString(e));
    return rc;
}

// The pair head's two kernels on caller-owned device pointers.  u / v are checked on the device before anything reads through them.
static int op_pair_check(const char* who, const int32_t* d_u, const int32_t* d_v, int64_t n_pairs, int64_t n_rows, int32_t width, int32_t mode, hipStream_t s) {
    if (!d_u || !d_v) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (mode < GAT_PAIR_MUL || mode > GAT_PAIR_ADD) return fail(GAT_E_INVALID, std::string(who) + ": mode must be 1 (mul) or 2 (add)");
    if (n_pairs < 1 || n_rows < 1 || n_rows >= 0x7fffffffLL || width < 1) return fail(GAT_E_INVALID, std::string(who) + ": bad sizes");
    if (n_pairs >= (1ll << 30)) return fail(GAT_E_UNSUPPORTED, std::string(who) + ": n_pairs must be below 2^30 (the incidence keys 2p + role go through the 32-bit graph builder)");
    int64_t where = -1; int32_t value = 0;
    GAT_TRY(pair_check_device(d_u, d_v, n_pairs, n_rows, &where, &value, s));
    if (where >= 0) return fail(GAT_E_INVALID, std::string(who) + ": " + pair_problem_text(where, value, n_rows));
    return 0;
}
int gat_op_pair_forward(const float* d_x, int64_t x_stride, const int32_t* d_u, const int32_t* d_v, int64_t n_pairs, int64_t n_rows,
                        int32_t width, int32_t mode, float* d_q, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GAT_TRY(op_pair_check("gat_op_pair_forward", d_u, d_v, n_pairs, n_rows, width, mode, s));
    if (!d_x || !d_q) return fail(GAT_E_INVALID, "gat_op_pair_forward: null argument");
    if (x_stride < width) return fail(GAT_E_INVALID, "gat_op_pair_forward: x_stride below width");
    PairFwdArgs a{};
    a.x = d_x; a.x_stride = x_stride; a.u = d_u; a.v = d_v; a.n_pairs = n_pairs; a.q = d_q; a.width = width; a.mode = mode;
    int rc = launch_pair_forward(a, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string("gat_op_pair_forward: ") + hipGetErrorString(e));
    return rc;
}
int gat_op_pair_backward(const float* d_gq, const float* d_x, int64_t x_stride, const int32_t* d_u, const int32_t* d_v, int64_t n_pairs,
                         int64_t n_rows, int32_t width, int32_t mode, float* d_gh, int64_t gh_stride, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    GAT_TRY(op_pair_check("gat_op_pair_backward", d_u, d_v, n_pairs, n_rows, width, mode, s));
    if (!d_gq || !d_gh || (mode == GAT_PAIR_MUL && !d_x)) return fail(GAT_E_INVALID, "gat_op_pair_backward: null argument");
    if (gh_stride < width) return fail(GAT_E_INVALID, "gat_op_pair_backward: gh_stride below width");
    if (mode == GAT_PAIR_MUL && x_stride < width) return fail(GAT_E_INVALID, "gat_op_pair_backward: x_stride below width");
    Scratch tmp;
    int32_t* inc_ptr = nullptr; int2* inc = nullptr;
    GAT_TRY(tmp.get(&inc_ptr, n_rows + 1)); GAT_TRY(tmp.get(&inc, 2 * n_pairs));
    GAT_TRY(pair_index_build(d_u, d_v, n_pairs, n_rows, inc_ptr, inc, s));
    std::vector<int32_t> ip((size_t)n_rows + 1);
    GAT_HIP(hipMemcpy(ip.data(), inc_ptr, ip.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    ReadoutPlan plan;
    build_readout_plan(ip.data(), n_rows, plan);
    int4 *items = nullptr, *split = nullptr; float* part = nullptr;
    GAT_TRY(tmp.get(&items, plan.n_items)); GAT_TRY(tmp.get(&split, plan.n_split)); GAT_TRY(tmp.get(&part, (int64_t)plan.n_parts * width));
    GAT_HIP(hipMemcpyAsync(items, plan.items.data(), plan.items.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    if (plan.n_split > 0) GAT_HIP(hipMemcpyAsync(split, plan.split.data(), plan.split.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    PairBwdArgs a{};
    a.gq = d_gq; a.x = d_x; a.x_stride = x_stride; a.inc = inc; a.items = items; a.n_items = plan.n_items; a.split = split; a.n_split = plan.n_split;
    a.part = part; a.gh = d_gh; a.gh_stride = gh_stride; a.width = width; a.mode = mode;
    int rc = launch_pair_backward(a, s);
    const hipError_t e = hipStreamSynchronize(s);        // before the scratch is freed
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string("gat_op_pair_backward: ") + hipGetErrorString(e));
    return rc;
}

// The negative sampler on caller-owned device pointers.  The CSR and the source pairs are checked on the device before anything walks them.
int gat_op_negative_sample(const int32_t* d_row_ptr, const int32_t* d_col_idx, int64_t n_rows, int64_t n_edges, int32_t mode, int32_t flags,
                           uint64_t seed, uint64_t round, const int32_t* d_src_u, const int32_t* d_src_v, int64_t n_src, int32_t* d_u,
                           int32_t* d_v, int64_t count, int64_t* unfiltered, void* stream) {
    static const char* who = "gat_op_negative_sample";
    hipStream_t s = (hipStream_t)stream;
    if (mode != GAT_NEG_UNIFORM && mode != GAT_NEG_CORRUPT) return fail(GAT_E_INVALID, std::string(who) + ": mode must be 1 (uniform) or 2 (corrupt)");
    if (flags & ~(GAT_NEG_BOTH_DIRECTIONS | GAT_NEG_ALLOW_SELF)) return fail(GAT_E_INVALID, std::string(who) + ": unknown flag bits");
    if (n_rows < 1 || n_rows >= 0x7fffffffLL || n_edges < 0 || n_edges > 0x7fffffffLL || count < 1) return fail(GAT_E_INVALID, std::string(who) + ": bad sizes");
    if (!d_row_ptr || (!d_col_idx && n_edges > 0) || !d_u || !d_v || !unfiltered) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    const bool corrupt = mode == GAT_NEG_CORRUPT;
    if (corrupt && (n_src < 1 || !d_src_u || !d_src_v)) return fail(GAT_E_INVALID, std::string(who) + ": GAT_NEG_CORRUPT needs at least one source pair");
    int32_t problem = 0; int64_t where = -1;
    GAT_TRY(csr_check_device(d_row_ptr, d_col_idx, n_rows, n_edges, n_rows, &problem, &where, s));
    if (problem) return fail(GAT_E_INVALID, std::string(who) + ": " + csr_problem_text(problem));
    if (corrupt) {
        int32_t value = 0;
        GAT_TRY(pair_check_device(d_src_u, d_src_v, n_src, n_rows, &where, &value, s));
        if (where >= 0) return fail(GAT_E_INVALID, std::string(who) + ": source " + pair_problem_text(where, value, n_rows));
    }
    Scratch tmp;
    unsigned long long* d_cnt = nullptr;
    int32_t* d_none = nullptr;                           // a graph without edges: the rows are never dereferenced
    GAT_TRY(tmp.get(&d_cnt, 1)); GAT_TRY(tmp.get(&d_none, 1));
    GAT_HIP(hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), s));
    NegSampleArgs a{};
    a.row_ptr = d_row_ptr; a.col_idx = d_col_idx ? d_col_idx : d_none; a.n_rows = n_rows;
    GAT_TRY(csr_rows_ascending(a.row_ptr, a.col_idx, n_rows, &a.ascending, s));
    a.mode = mode; a.flags = flags; a.seed = seed; a.round = round;
    a.src_u = d_src_u; a.src_v = d_src_v; a.n_src = corrupt ? n_src : 0;
    a.u = d_u; a.v = d_v; a.count = count; a.unfiltered = d_cnt;
    int rc = launch_negative_sample(a, s);
    unsigned long long cnt = 0;
    hipError_t e = hipMemcpyAsync(&cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);    // before the scratch is freed
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string(who) + ": " + hipGetErrorString(e));
    if (rc == 0) *unfiltered = (int64_t)cnt;
    return rc;
}

// ---- the six dense launchers on caller-owned device pointers: one launcher per call, exactly the caller's arguments ----------------
static int op_dense_sizes(const char* who, int64_t n_rows, int32_t F, int32_t HD) {
    if (n_rows < 0 || n_rows >= 0x7fffffffLL || F < 1 || HD < 1) return fail(GAT_E_INVALID, std::string(who) + ": bad sizes (n_rows >= 0, F >= 1, HD >= 1)");
    if ((int64_t)2 * HD * F >= 0x7fffffffLL) return fail(GAT_E_INVALID, std::string(who) + ": 2 * HD * F does not fit 32 bits");
    return 0;
}
static int op_dense_part(const char* who, int32_t part) {
    if (part != kPartBoth && part != kPartLeft && part != kPartRight) return fail(GAT_E_INVALID, std::string(who) + ": part must be 0 (both), 1 (left) or 2 (right)");
    return 0;
}
static int op_dense_ldx(const char* who, int32_t ldx, int32_t F) {
    if (ldx != 0 && ldx < F) return fail(GAT_E_INVALID, std::string(who) + ": ldx must be 0 or at least F");
    return 0;
}
// synchronise, then hand the launcher's kernel name to the caller
static int op_dense_finish(const char* who, int rc, hipStream_t s, char* picked, int32_t picked_cap) {
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string(who) + ": " + hipGetErrorString(e));
    if (picked != nullptr && picked_cap > 0) snprintf(picked, (size_t)picked_cap, "%s", dense_last_kernel());
    return rc;
}
int gat_op_dense_scratch_floats(int32_t kind, int64_t n_rows, int32_t F, int32_t HD, int32_t part, int64_t* floats_out) {
    if (!floats_out) return fail(GAT_E_INVALID, "gat_op_dense_scratch_floats: null argument");
    if (kind != 0 && kind != 1) return fail(GAT_E_INVALID, "gat_op_dense_scratch_floats: kind must be 0 (project) or 1 (grad_w)");
    GAT_TRY(op_dense_sizes("gat_op_dense_scratch_floats", n_rows, F, HD));
    GAT_TRY(op_dense_part("gat_op_dense_scratch_floats", part));
    *floats_out = kind == 0 ? project_scratch_floats(n_rows, F, HD, part) : grad_w_scratch_floats(n_rows, F, HD);
    return 0;
}
int gat_op_dense_project(const float* d_x, int32_t ldx, const float* d_w, int64_t n_rows, int32_t F, int32_t HD, int32_t part, int32_t pl_bf16,
                         void* d_pl, float* d_pr, float* d_scratch, int64_t scratch_floats, void* stream, char* picked, int32_t picked_cap) {
    static const char* who = "gat_op_dense_project";
    GAT_TRY(op_dense_sizes(who, n_rows, F, HD));
    GAT_TRY(op_dense_part(who, part));
    GAT_TRY(op_dense_ldx(who, ldx, F));
    if (pl_bf16 != 0 && pl_bf16 != 1) return fail(GAT_E_INVALID, std::string(who) + ": pl_bf16 must be 0 or 1");
    if (!d_x || !d_w || (part != kPartRight && !d_pl) || (part != kPartLeft && !d_pr)) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (scratch_floats < 0 || (!d_scratch && scratch_floats != 0)) return fail(GAT_E_INVALID, std::string(who) + ": scratch_floats without a scratch");
    hipStream_t s = (hipStream_t)stream;
    dense_last_kernel_clear();
    const int rc = launch_project(d_x, d_w, (float*)d_pl, d_pr, n_rows, F, HD, part, pl_bf16 != 0, d_scratch, scratch_floats, s, ldx);
    return op_dense_finish(who, rc, s, picked, picked_cap);
}
int gat_op_dense_grad_x(const float* d_gpl, const float* d_gpr, const float* d_w, const float* d_hpre_prev, float* d_gprev, int64_t n_rows,
                        int32_t F, int32_t HD, float slope, void* stream, char* picked, int32_t picked_cap) {
    static const char* who = "gat_op_dense_grad_x";
    GAT_TRY(op_dense_sizes(who, n_rows, F, HD));
    if (!d_gpl || !d_gpr || !d_w || !d_gprev) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (!(slope == slope)) return fail(GAT_E_INVALID, std::string(who) + ": slope is NaN");
    hipStream_t s = (hipStream_t)stream;
    dense_last_kernel_clear();
    const int rc = launch_grad_x(d_gpl, d_gpr, d_w, d_hpre_prev, d_gprev, n_rows, F, HD, slope, s);
    return op_dense_finish(who, rc, s, picked, picked_cap);
}
int gat_op_dense_grad_w(const float* d_gpl, const float* d_gpr, const float* d_x, int32_t ldx, float* d_grad_w, float* d_scratch,
                        int64_t scratch_floats, int64_t n_rows, int32_t F, int32_t HD, int32_t part, void* stream, char* picked, int32_t picked_cap) {
    static const char* who = "gat_op_dense_grad_w";
    GAT_TRY(op_dense_sizes(who, n_rows, F, HD));
    GAT_TRY(op_dense_part(who, part));
    GAT_TRY(op_dense_ldx(who, ldx, F));
    if ((part != kPartRight && !d_gpl) || (part != kPartLeft && !d_gpr) || !d_x || !d_grad_w || !d_scratch) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (scratch_floats < grad_w_scratch_floats(n_rows, F, HD))
        return fail(GAT_E_INVALID, std::string(who) + ": scratch below gat_op_dense_scratch_floats(1, ...) = " + std::to_string(grad_w_scratch_floats(n_rows, F, HD)) + " floats");
    hipStream_t s = (hipStream_t)stream;
    dense_last_kernel_clear();
    const int rc = launch_grad_w(d_gpl, d_gpr, d_x, d_grad_w, d_scratch, n_rows, F, HD, part, s, ldx);
    return op_dense_finish(who, rc, s, picked, picked_cap);
}
int gat_op_dense_project_res(const float* d_x, int32_t ldx, const float* d_wres, float* d_r, int64_t n_rows, int32_t F, int32_t HD, void* stream,
                             char* picked, int32_t picked_cap) {
    static const char* who = "gat_op_dense_project_res";
    GAT_TRY(op_dense_sizes(who, n_rows, F, HD));
    GAT_TRY(op_dense_ldx(who, ldx, F));
    if (!d_x || !d_wres || !d_r) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    hipStream_t s = (hipStream_t)stream;
    dense_last_kernel_clear();
    const int rc = launch_project_res(d_x, d_wres, d_r, n_rows, F, HD, s, ldx);
    return op_dense_finish(who, rc, s, picked, picked_cap);
}
int gat_op_dense_grad_wres(const float* d_g, const float* d_x, int32_t ldx, float* d_grad_wres, float* d_scratch, int64_t scratch_floats,
                           int64_t n_rows, int32_t F, int32_t HD, void* stream, char* picked, int32_t picked_cap) {
    static const char* who = "gat_op_dense_grad_wres";
    GAT_TRY(op_dense_sizes(who, n_rows, F, HD));
    GAT_TRY(op_dense_ldx(who, ldx, F));
    if (!d_g || !d_x || !d_grad_wres || !d_scratch) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (scratch_floats < grad_w_scratch_floats(n_rows, F, HD))
        return fail(GAT_E_INVALID, std::string(who) + ": scratch below gat_op_dense_scratch_floats(1, ...) = " + std::to_string(grad_w_scratch_floats(n_rows, F, HD)) + " floats");
    hipStream_t s = (hipStream_t)stream;
    dense_last_kernel_clear();
    const int rc = launch_grad_wres(d_g, d_x, d_grad_wres, d_scratch, n_rows, F, HD, s, ldx);
    return op_dense_finish(who, rc, s, picked, picked_cap);
}
int gat_op_dense_grad_x_res(const float* d_g, const float* d_wres, float* d_gx, int64_t n_rows, int32_t F, int32_t HD, void* stream,
                            char* picked, int32_t picked_cap) {
    static const char* who = "gat_op_dense_grad_x_res";
    GAT_TRY(op_dense_sizes(who, n_rows, F, HD));
    if (!d_g || !d_wres || !d_gx) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    hipStream_t s = (hipStream_t)stream;
    dense_last_kernel_clear();
    const int rc = launch_grad_x_res(d_g, d_wres, d_gx, n_rows, F, HD, s);
    return op_dense_finish(who, rc, s, picked, picked_cap);
}

// ---- ranking metrics (gatv2_abi.h "ranking metrics"): the kernels of gat_eval_rank on caller-owned device pointers -------------------
int gat_op_rank_stats(const float* d_scores, int64_t score_stride, const int32_t* d_labels, const float* d_targets, const uint8_t* d_mask,
                      int64_t n_rows, int32_t n_cols, const int32_t* ks, int32_t n_ks, gat_rank_stats* out, void* stream) {
    static const char* who = "gat_op_rank_stats";
    GAT_TRY(rank_check(who, n_rows, n_cols, ks, n_ks));
    if (!d_scores || !out) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if ((d_labels != nullptr) == (d_targets != nullptr)) return fail(GAT_E_INVALID, std::string(who) + ": exactly one of d_labels / d_targets must be given");
    if (score_stride < n_cols) return fail(GAT_E_INVALID, std::string(who) + ": score_stride below n_cols");
    hipStream_t s = (hipStream_t)stream;
    Scratch tmp;
    RankSizes z; RankBuffers b;
    GAT_TRY(rank_sizes(n_rows, n_cols, &z));
    GAT_TRY(rank_buffers_get(&b, z, n_cols, [&tmp](void** p, size_t bytes) { return tmp.get((char**)p, (int64_t)bytes); }));
    RankArgs a{};
    a.scores = d_scores; a.score_stride = score_stride; a.labels = d_labels; a.targets = d_targets; a.mask = d_mask;
    a.n_rows = n_rows; a.n_cols = n_cols; a.ks = ks; a.n_ks = n_ks;
    int rc = launch_rank_stats(a, b, s);
    if (rc == 0 && hipMemcpyAsync(out, b.stats, (size_t)n_cols * sizeof(gat_rank_stats), hipMemcpyDeviceToHost, s) != hipSuccess)
        rc = fail(GAT_E_STATE, std::string(who) + ": copy of the result failed");
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string(who) + ": " + hipGetErrorString(e));
    return rc;
}

// ---- hidden layer in front of the head (gatv2_abi.h "hidden layer"): the two row-streaming kernels on caller-owned device pointers -----
static int op_hidden_check(const char* who, int64_t rows, int32_t width, float slope) {
    if (rows < 0 || width < 1) return fail(GAT_E_INVALID, std::string(who) + ": bad sizes (rows >= 0, width >= 1)");
    if (!(slope >= 0.f && slope <= 1.f)) return fail(GAT_E_INVALID, std::string(who) + ": slope must be in [0, 1] (0 = ReLU)");
    return 0;
}
int gat_op_head_hidden_forward(float* d_a, const float* d_b1, int64_t rows, int32_t width, float slope, void* stream) {
    static const char* who = "gat_op_head_hidden_forward";
    GAT_TRY(op_hidden_check(who, rows, width, slope));
    if (rows == 0) return 0;
    if (!d_a || !d_b1) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    hipStream_t s = (hipStream_t)stream;
    int rc = launch_head_hidden_forward(d_a, d_b1, rows, width, slope, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string(who) + ": " + hipGetErrorString(e));
    return rc;
}
int gat_op_head_hidden_backward(float* d_gz, const float* d_z1, int64_t rows, int32_t width, float slope, float* d_grad_b1, void* stream) {
    static const char* who = "gat_op_head_hidden_backward";
    GAT_TRY(op_hidden_check(who, rows, width, slope));
    if (rows == 0) return 0;
    if (!d_gz || !d_z1) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    hipStream_t s = (hipStream_t)stream;
    Scratch tmp;
    float* partial = nullptr;
    const int blocks = head_hidden_blocks(rows, width);
    if (d_grad_b1) GAT_TRY(tmp.get(&partial, (int64_t)blocks * width));
    int rc = launch_head_hidden_backward(d_gz, d_z1, partial, rows, width, slope, s);
    if (rc == 0 && d_grad_b1) rc = launch_reduce_partials_add(partial, blocks, width, d_grad_b1, s);
    const hipError_t e = hipStreamSynchronize(s);        // before the scratch is freed
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string(who) + ": " + hipGetErrorString(e));
    return rc;
}

// The batch-normalisation kernels on caller-owned device pointers (gatv2_abi.h "batch normalisation").
int gat_op_batch_norm_forward(const float* d_u, int64_t n_rows, int32_t H, int32_t D, int32_t is_last, const float* d_gamma, const float* d_beta,
                              float eps, float slope, float momentum, float* d_running_mean, float* d_running_var, int32_t training,
                              float* d_mean_rstd, float* d_hout, void* stream) {
    const char* who = "gat_op_batch_norm_forward";
    if (n_rows < 1 || n_rows >= 0x7fffffffLL || H < 1 || D < 1 || (int64_t)H * D >= (1 << 24)) return fail(GAT_E_INVALID, std::string(who) + ": bad sizes");
    if (!d_u || !d_gamma || !d_beta || !d_hout) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if (!(std::isfinite(eps) && eps > 0.f) || !(std::isfinite(momentum) && momentum >= 0.f && momentum <= 1.f)) return fail(GAT_E_INVALID, std::string(who) + ": bad eps or momentum");
    if ((d_running_mean == nullptr) != (d_running_var == nullptr)) return fail(GAT_E_INVALID, std::string(who) + ": one running statistic without the other");
    if (training == 0 && !d_running_mean) return fail(GAT_E_INVALID, std::string(who) + ": eval mode needs the running statistics");
    if (training != 0 && !d_mean_rstd) return fail(GAT_E_INVALID, std::string(who) + ": training mode needs d_mean_rstd");
    hipStream_t s = (hipStream_t)stream;
    const int32_t HD = H * D;
    Scratch tmp;
    int rc = 0;
    BnStats st{};
    st.eps = eps;
    if (training != 0) {
        float* part = nullptr;
        const int blocks = batch_norm_blocks(n_rows, HD);
        GAT_TRY(tmp.get(&part, (int64_t)2 * blocks * HD));
        rc = launch_batch_norm_stats(d_u, n_rows, HD, part, part + (int64_t)blocks * HD, eps, momentum, d_mean_rstd, d_mean_rstd + HD, d_running_mean,
                                     d_running_var, s);
        st.mean = d_mean_rstd; st.scale = d_mean_rstd + HD; st.from_var = 0;
    } else {
        st.mean = d_running_mean; st.scale = d_running_var; st.from_var = 1;
    }
    if (rc == 0) rc = launch_batch_norm_apply(d_u, st, d_gamma, d_beta, slope, d_hout, n_rows, H, D, is_last != 0, s);
    const hipError_t e = hipStreamSynchronize(s);        // before the scratch is freed
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string(who) + ": " + hipGetErrorString(e));
    return rc;
}
int gat_op_batch_norm_backward(const float* d_u, const float* d_g, const float* d_gh, int64_t gh_stride, int64_t n_rows, int32_t H, int32_t D,
                               const float* d_gamma, const float* d_beta, const float* d_mean_rstd, const float* d_running_mean,
                               const float* d_running_var, float eps, float slope, int32_t training, const float* d_res, const float* d_bias,
                               float* d_G, float* d_agg, float* d_grad_gamma, float* d_grad_beta, float* d_grad_b, void* stream) {
    const char* who = "gat_op_batch_norm_backward";
    if (n_rows < 1 || n_rows >= 0x7fffffffLL || H < 1 || D < 1 || (int64_t)H * D >= (1 << 24)) return fail(GAT_E_INVALID, std::string(who) + ": bad sizes");
    if (!d_u || !d_gamma || !d_beta || !d_G) return fail(GAT_E_INVALID, std::string(who) + ": null argument");
    if ((d_g == nullptr) == (d_gh == nullptr)) return fail(GAT_E_INVALID, std::string(who) + ": exactly one of d_g and d_gh");
    if (d_gh && gh_stride < D) return fail(GAT_E_INVALID, std::string(who) + ": gh_stride below D");
    if (training != 0 ? !d_mean_rstd : (!d_running_mean || !d_running_var)) return fail(GAT_E_INVALID, std::string(who) + ": the statistics of this mode are null");
    if (training == 0 && !(std::isfinite(eps) && eps > 0.f)) return fail(GAT_E_INVALID, std::string(who) + ": bad eps");
    hipStream_t s = (hipStream_t)stream;
    const int32_t HD = H * D;
    BnBwdArgs a{};
    a.u = d_u; a.g = d_g; a.gh = d_gh; a.res = d_res; a.bias = d_bias; a.gamma = d_gamma; a.beta = d_beta;
    a.stats.eps = eps; a.stats.from_var = training != 0 ? 0 : 1;
    a.stats.mean = training != 0 ? d_mean_rstd : d_running_mean; a.stats.scale = training != 0 ? d_mean_rstd + HD : d_running_var;
    a.G = d_G; a.agg = d_agg; a.n_rows = n_rows; a.gh_stride = gh_stride; a.H = H; a.D = D; a.training = training != 0 ? 1 : 0; a.slope = slope;
    a.blocks = batch_norm_blocks(n_rows, HD);
    Scratch tmp;
    float* part = nullptr;
    GAT_TRY(tmp.get(&part, ((int64_t)3 * a.blocks + 2) * HD));
    a.part_s1 = part; a.part_s2 = part + (int64_t)a.blocks * HD; a.sums = part + (int64_t)3 * a.blocks * HD;
    a.part_G = d_grad_b ? part + (int64_t)2 * a.blocks * HD : nullptr;
    int rc = launch_batch_norm_backward(a, d_grad_gamma, d_grad_beta, s);
    if (rc == 0 && d_grad_b) rc = launch_reduce_partials_add(a.part_G, a.blocks, HD, d_grad_b, s);
    const hipError_t e = hipStreamSynchronize(s);        // before the scratch is freed
    if (rc == 0 && e != hipSuccess) rc = fail((int)e, std::string(who) + ": " + hipGetErrorString(e));
    return rc;
}

}  // extern "C"
