// gat_optimizer.hip — the optimizer step on the device (include/gatv2_abi.h "optimizer"): weight decay, SGD with momentum, Adam,
// AdamW, per-group and global-norm clipping, with the step counter t and the learning rate in device memory.  Two launches per step,
// whatever the number of parameter groups: opt_prepare (block sums of squares of the gradient, t advanced) and opt_apply (clip factor,
// bias corrections, update).  Both walk the block table the host built once (opt_build_table): a block owns at most kOptBlockEntries
// consecutive entries of ONE group, so every partial, every norm and every update is a function of the packed sizes alone — no float
// atomics, no fences, no cooperative launch; a replay computes the bits of the eager step.
#include "gat_internal.h"

namespace gat {
namespace {

// sum of squares of the block's entries in a fixed order: lane-strided, then the wave butterfly, then the waves ascending
__device__ __forceinline__ float block_sumsq(const float* __restrict__ g, int32_t count, float* wave_part) {
    float s = 0.f;
    for (int32_t i = threadIdx.x; i < count; i += kOptThreads) { const float v = g[i]; s += v * v; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = s;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kOptThreads / 64; ++w) t += wave_part[w];
    return t;
}

// One block per table row (clip mode NONE: one block, which only advances t).  partial[block] = the block's sum of squares.  Block 0
// advances the step counter: one lane, an ordinary store — the launch that reads it (opt_apply) is the next one on the stream.
__global__ __launch_bounds__(kOptThreads) void opt_prepare_kernel(OptArgs A) {
    __shared__ float wave_part[kOptThreads / 64];
    if (blockIdx.x == 0 && threadIdx.x == 0) *A.t = *A.t + 1ull;
    if (A.clip_mode == GAT_CLIP_NONE) return;
    const OptBlock row = A.table[blockIdx.x];
    const float s = block_sumsq(A.g + row.first, row.count, wave_part);
    if (threadIdx.x == 0) A.partial[blockIdx.x] = s;
}

// squared norm of group k's gradient: its blocks' partials in ascending block order (0 for a group without entries)
__device__ __forceinline__ float group_sumsq(const OptArgs& A, int k) {
    float s = 0.f;
    for (int32_t b = A.group_block0[k]; b < A.group_block0[k + 1]; ++b) s += A.partial[b];
    return s;
}

// One block per table row.  Lane 0 forms what the whole block shares — the clip factor c of the block's group, lr, the decay of the group,
// the two bias corrections — and the block then updates its entries (the law: gatv2_abi.h "optimizer").  Block 0 leaves the norms in
// the device record gat_optimizer_info reads.
__global__ __launch_bounds__(kOptThreads) void opt_apply_kernel(OptArgs A) {
    __shared__ float sh[4];            // c, lr, 1 - b1^t, 1 - b2^t
    const OptBlock row = A.table[blockIdx.x];
    if (threadIdx.x == 0) {
        float c = 1.0f;
        if (A.clip_mode == GAT_CLIP_PER_GROUP) {
            if (blockIdx.x == 0)
                for (int k = 0; k < kOptGroups; ++k) A.norms[k] = sqrtf(group_sumsq(A, k));
            const float n = sqrtf(group_sumsq(A, row.group));
            if (n > A.clip_threshold) c = A.clip_threshold / (n + 1e-9f);
        } else if (A.clip_mode == GAT_CLIP_GLOBAL) {
            float tot = 0.f;
            for (int k = 0; k < kOptGroups; ++k) {
                const float sk = group_sumsq(A, k);
                if (blockIdx.x == 0) A.norms[k] = sqrtf(sk);
                tot += sk;
            }
            const float n = sqrtf(tot);
            if (blockIdx.x == 0) A.norms[kOptGroups] = n;
            const float q = A.clip_threshold / (n + 1e-6f);
            c = q > 1.0f ? 1.0f : q;                      // a NaN norm stays NaN
        }
        const float tf = (float)*A.t;
        sh[0] = c; sh[1] = *A.lr;
        sh[2] = 1.0f - powf(A.beta1, tf); sh[3] = 1.0f - powf(A.beta2, tf);
    }
    __syncthreads();
    const float c = sh[0], lr = sh[1], bc1 = sh[2], bc2 = sh[3];
    const float wd = ((A.decay_groups >> row.group) & 1u) ? A.weight_decay : 0.0f;
    float* __restrict__ p = A.p + row.first;
    const float* __restrict__ g = A.g + row.first;
    if (A.kind == GAT_OPT_SGD) {
        float* __restrict__ buf = A.s0 ? A.s0 + row.first : nullptr;         // null: momentum = 0
        for (int32_t i = threadIdx.x; i < row.count; i += kOptThreads) {
            const float pi = p[i];
            float d = c * g[i] + wd * pi;
            if (buf) {
                const float bi = A.momentum * buf[i] + d;
                buf[i] = bi;
                d = (A.flags & GAT_OPT_NESTEROV) ? d + A.momentum * bi : bi;
            }
            p[i] = pi - lr * d;
        }
        return;
    }
    float* __restrict__ m = A.s0 + row.first;
    float* __restrict__ v = A.s1 + row.first;
    const bool decoupled = A.kind == GAT_OPT_ADAMW;
    for (int32_t i = threadIdx.x; i < row.count; i += kOptThreads) {
        float pi = p[i];
        float d = c * g[i];
        if (decoupled) pi *= 1.0f - lr * wd;
        else d += wd * pi;
        const float mi = A.beta1 * m[i] + (1.0f - A.beta1) * d;
        const float vi = A.beta2 * v[i] + (1.0f - A.beta2) * (d * d);
        m[i] = mi; v[i] = vi;
        const float mh = mi / bc1;
        const float vh = vi / bc2;
        p[i] = pi - lr * mh / (sqrtf(vh) + A.eps);
    }
}

// stream-ordered writes of the two device scalars (the value travels as a kernel argument: no host buffer has to outlive the call)
__global__ void opt_set_lr_kernel(float* lr, float v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *lr = v;
}
__global__ void opt_set_count_kernel(unsigned long long* t, unsigned long long v) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *t = v;
}

}  // namespace

void opt_build_table(const int64_t* group_off, const int64_t* group_cnt, std::vector<OptBlock>* table, int32_t* group_block0) {
    table->clear();
    for (int k = 0; k < kOptGroups; ++k) {
        group_block0[k] = (int32_t)table->size();
        for (int64_t i = 0; i < group_cnt[k]; i += kOptBlockEntries) {
            OptBlock b;
            b.first = group_off[k] + i;
            b.count = (int32_t)std::min<int64_t>(kOptBlockEntries, group_cnt[k] - i);
            b.group = k;
            table->push_back(b);
        }
    }
    group_block0[kOptGroups] = (int32_t)table->size();
}

int launch_opt_step(const OptArgs& a, hipStream_t s) {
    if (a.n_blocks < 1) return fail(GAT_E_INVALID, "launch_opt_step: empty block table");      // (W, a and Wo are never empty)
    const unsigned prepare_blocks = a.clip_mode == GAT_CLIP_NONE ? 1u : (unsigned)a.n_blocks;
    hipLaunchKernelGGL(opt_prepare_kernel, dim3(prepare_blocks), dim3(kOptThreads), 0, s, a);
    GAT_HIP(hipGetLastError());
    hipLaunchKernelGGL(opt_apply_kernel, dim3((unsigned)a.n_blocks), dim3(kOptThreads), 0, s, a);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_opt_set_lr(float* lr, float v, hipStream_t s) {
    hipLaunchKernelGGL(opt_set_lr_kernel, dim3(1), dim3(64), 0, s, lr, v);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_opt_set_count(unsigned long long* t, uint64_t v, hipStream_t s) {
    hipLaunchKernelGGL(opt_set_count_kernel, dim3(1), dim3(64), 0, s, t, (unsigned long long)v);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
