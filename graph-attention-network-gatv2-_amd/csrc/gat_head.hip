// gat_head.hip — the output head of the GATv2 step on gfx950: logits z = Wo·x over the head's input rows, the loss, and the backward
// gH = Wo^T dz, gradWo += dz^T X.  Three loss modes (HeadArgs::mode), three entry points (launch_head_forward / _backward / _step),
// one set of tile pieces under every kernel; with it the mask, target-check and result kernels around the head.
//
// Softmax mode (C12-C14, E:463-608): y = exp(z-max)/(sum+1e-8) (double divide, E:140); loss_n = -log(max(y[label],1e-12)); correct_n =
// (argmax == label); dz = y - onehot; g[n,h,d] = (Wo^T dz)[d]·LReLU'(h_pre)/H.  A thread owns a row for the softmax (softmax_row).
//   head_forward_kernel<DLP>   y, loss, count.  The block's y tile lives in LDS ([NB][ldz], ldz odd) and is written back coalesced.  DLP =
//                              D_last padded to 8/16/32/64: the row is held in registers, Wo rows are padded with zeros in LDS; DLP = 0
//                              is the any-size form that re-reads the row from memory.
//   head_backward_kernel       any shape, from y: gradWo as a per-block register partial (thread = one (c,d) entry), gH rows and, where
//                              HeadArgs::g is set, the full g with a coalesced sweep.
//   head_backward2_kernel<DL>  the training path (only gH: g == nullptr), DL in {4, 8, 16}, C <= 64, 128-row tiles, register-blocked over
//                              the DL outputs so that an FMA costs 3/8 LDS reads instead of 2 (head_grads_blocked).
//   head_step_kernel<DL>       forward AND backward in one pass over the rows (gat_step): the class probabilities never reach HBM (0.46 GB
//                              written by head_forward_kernel and read back by head_backward2_kernel otherwise).  It is those two
//                              kernels' pieces on one tile: waves 0-1 own a row each for the softmax and gH, waves 2-3 own (class,
//                              half-tile) for gradWo.
// Loss modes, BCE / MSE on float targets (gatv2_abi.h "loss modes of the output head"): loss_head_forward_kernel<MODE, DLT> and
// loss_head_grad_kernel<MODE, FUSED, DLT>, persistent over tiles of NB <= 128 rows.  LDS: Wo [C][ws], the tile's targets — afterwards dz —
// [NB][ldz], the tile's input rows [NB][ldx]; ws, ldz, ldx odd.  DLT = 0: work inside a tile is dealt by flat entry index q = r*C + c
// (logits, loss, dz: the global y / T accesses are q itself, coalesced), by r*DL + d (gH) and by c*DL + d (gradWo, registers across the
// tiles of a block): no thread owns a row, so every C >= 1 and D_last >= 1 takes the same path.  DLT = D_last in {4, 8, 16} with C <= 128
// is the register-blocked form of the same tile, laid out like head_step_kernel: thread (row, column half) keeps its input row in
// registers and walks its columns with wave-uniform (broadcast) reads of Wo; then head_grads_blocked.  Every z is the same fmaf chain in
// both forms.
// All tile index arithmetic is 32-bit and incremental (no per-element division).  Every reduction has a fixed order: lanes by shuffle,
// waves and row parts in ascending order, blocks by head_finalize_kernel / the slab reduction.
#include "gat_internal.h"

#include <algorithm>
#include <type_traits>

#include <cstdlib>

namespace gat {
namespace {

// ---- tile pieces ---------------------------------------------------------------------------------------------------
// A tile in LDS: Wo [C][ws], what the entries leave behind (y or dz) [NB][ldz], the input rows [NB][ldx]
struct HeadTile { float* s_wo; float* s_dz; float* s_x; int NB, ldz, ldx, ws; };
__device__ __forceinline__ HeadTile head_tile_at(float* lds, int C, int NB, int ldz, int ldx, int ws) {
    return HeadTile{lds, lds + C * ws, lds + C * ws + NB * ldz, NB, ldz, ldx, ws};
}

// One row of the softmax head: logits from the row x (DLR > 0: DLR entries in registers against Wo rows DLR floats apart, unrolled;
// DLR = 0: DL entries read through x), softmax, argmax; the row's loss term and count into the thread's accumulators.  Leaves y
// (DZ false) or dz (DZ true; 0 outside the training mask) in zr[0..C).  The products are not written as fmaf: the sum of DLR terms is
// the reference's multiply-then-add chain where the compiler leaves it one.
template <int DLR, bool DZ>
__device__ __forceinline__ void softmax_row(const float* s_wo, const float* x, int DL, int C, const int32_t* label, float* zr,
                                            double& loss_acc, int& corr_acc) {
    float mv = -INFINITY;
    for (int c = 0; c < C; ++c) {
        float acc = 0.f;
        if constexpr (DLR > 0) {
#pragma unroll
            for (int j = 0; j < DLR; ++j) acc += s_wo[c * DLR + j] * x[j];      // ascending j (E:496-498)
        } else {
            for (int j = 0; j < DL; ++j) acc += s_wo[c * DL + j] * x[j];
        }
        zr[c] = acc;
        mv = fmaxf(mv, acc);
    }
    float sum = 0.f;
    // E:514 uses __expf (= ex2.approx(x * log2 e)): the hardware exp2 here, not the 10-instruction libm expf
    for (int c = 0; c < C; ++c) { const float ev = __builtin_amdgcn_exp2f((zr[c] - mv) * 1.4426950408889634f); zr[c] = ev; sum += ev; }
    const double rden = 1.0 / ((double)sum + 1e-8);
    const int lab = *label;
    float best = -1.f; int pred = 0; float plab = 0.f;
    for (int c = 0; c < C; ++c) {
        const float yv = (float)((double)zr[c] * rden);           // E:140 divides in double: one reciprocal + a product per class
                                                                  // (47 fp64 divisions per node made this kernel VALU-bound)
        if constexpr (!DZ) zr[c] = yv;
        if (c == 0 || yv > best) { best = yv; pred = c; }         // strict >, first max wins
        if (c == lab) plab = yv;
        if constexpr (DZ) zr[c] = lab >= 0 ? yv - (c == lab ? 1.0f : 0.0f) : 0.0f;
    }
    // lab < 0: the node is outside the training mask (gat_set_train_mask stores ~label): no loss, no count
    loss_acc += lab >= 0 ? (double)(-logf(fmaxf(plab, 1e-12f))) : 0.0;
    corr_acc += (lab >= 0 && pred == lab) ? 1 : 0;
}

// dz = y - onehot of the tile's rows from y in memory -> LDS (labels: the tile's; < 0: outside the training mask => dz = 0)
__device__ __forceinline__ void tile_load_dz(const float* yt, const int32_t* labels, float* s_dz, int ldz, int C, int rows_here) {
    const int dq = 256 / C, dr = 256 % C;                // advance of (row, col) per 256 linear elements
    int r = threadIdx.x / C, c = threadIdx.x % C;
    for (int q = threadIdx.x; q < rows_here * C; q += 256) {
        const int lab_r = labels[r];
        s_dz[r * ldz + c] = lab_r >= 0 ? yt[q] - (c == lab_r ? 1.0f : 0.0f) : 0.0f;
        r += dq; c += dr;
        if (c >= C) { c -= C; ++r; }
    }
}
// the tile's y: LDS -> one contiguous block of global memory, coalesced
__device__ __forceinline__ void tile_store_y(float* yt, const float* s_y, int ldz, int C, int rows_here) {
    const int dq = 256 / C, dr = 256 % C;                // advance of (row, col) per 256 linear elements
    int r = threadIdx.x / C, c = threadIdx.x % C;
    for (int q = threadIdx.x; q < rows_here * C; q += 256) {
        yt[q] = s_y[r * ldz + c];
        r += dq; c += dr;
        if (c >= C) { c -= C; ++r; }
    }
}

// The register-blocked second phase of a tile (D_last = DL in {4, 8, 16}, Wo rows DL floats apart), from dz in LDS: waves 0-1 own a row
// each for gH; waves 2-3 own (column, row part) for gradWo — nparts parts of ceil(NB / nparts) consecutive rows — and run beside them;
// per-thread partials live across all tiles of the block.  NPARTS = 2: the softmax kernels' two halves of a 128-row tile (C <= 64);
// NPARTS = 0: 128 / C parts (the loss modes, C <= 128).  The parts decide the order of a column's sum, so each family keeps its own.
template <int DL, int NPARTS>
struct GradWoParts {
    float wacc[DL]; int wc, part, nparts, rows_per;
    __device__ __forceinline__ void init(int C, int NB) {
        const int t2 = (int)threadIdx.x - 128;
        nparts = NPARTS > 0 ? NPARTS : 128 / C; rows_per = (NB + nparts - 1) / nparts;
        wc = t2 >= 0 ? t2 % C : 0; part = t2 >= 0 ? t2 / C : nparts;       // part >= nparts: no gradWo work
#pragma unroll
        for (int d = 0; d < DL; ++d) wacc[d] = 0.f;
    }
};
// GH_OPTIONAL: gh_out may be null — loss, count and gradWo only (head_step_kernel under the fused last layer: gH is formed there)
template <int DL, int NPARTS, bool GH_OPTIONAL>
__device__ __forceinline__ void head_grads_blocked(const HeadArgs& A, const HeadTile& L, int64_t n0, int rows_here, GradWoParts<DL, NPARTS>& W) {
    const int C = A.C, tid = threadIdx.x;
    if (tid < 128) {
        if (tid < rows_here) {                           // gH[r][:] = sum_c dz[r][c] Wo[c][:], ascending c: the reference's loop (E:585-590)
            float acc[DL];
#pragma unroll
            for (int d = 0; d < DL; ++d) acc[d] = 0.f;
            const float* dzr = L.s_dz + tid * L.ldz;
            for (int c = 0; c < C; ++c) {
                const float z = dzr[c];
#pragma unroll
                for (int d = 0; d < DL; ++d) acc[d] = fmaf(L.s_wo[c * DL + d], z, acc[d]);
            }
            if (!GH_OPTIONAL || A.gh_out != nullptr) {
                float* out = A.gh_out + (n0 + tid) * (A.gh_stride ? A.gh_stride : DL);
#pragma unroll
                for (int d = 0; d < DL; ++d) out[d] = acc[d];
            }
        }
    } else if (W.part < W.nparts) {                      // gradWo[c][:] += sum_r dz[r][c] X[r][:], ascending r inside the part
        const int r0 = W.part * W.rows_per, r1 = (r0 + W.rows_per < rows_here) ? r0 + W.rows_per : rows_here;
        for (int r = r0; r < r1; ++r) {
            const float z = L.s_dz[r * L.ldz + W.wc];
#pragma unroll
            for (int d = 0; d < DL; ++d) W.wacc[d] = fmaf(z, L.s_x[r * L.ldx + d], W.wacc[d]);
        }
    }
}
// the parts of a column added in ascending order; s_tmp [nparts][C][DL] lies in the tile region (its size: loss_head_tile)
template <int DL, int NPARTS>
__device__ __forceinline__ void head_partial_blocked(const HeadArgs& A, const HeadTile& L, const GradWoParts<DL, NPARTS>& W) {
    const int C = A.C, CD = C * DL;
    __syncthreads();
    float* s_tmp = L.s_dz;
    if (W.part < W.nparts) {
#pragma unroll
        for (int d = 0; d < DL; ++d) s_tmp[(W.part * C + W.wc) * DL + d] = W.wacc[d];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < CD; i += 256) {
        float tot = s_tmp[i];
        for (int p = 1; p < W.nparts; ++p) tot += s_tmp[p * CD + i];
        A.partial[(int64_t)blockIdx.x * CD + i] = tot;
    }
}

// the block's loss / count partial, fixed order: lanes by shuffle, then the first WAVES waves (the others hold no rows)
template <int WAVES>
__device__ __forceinline__ void head_block_partial(double loss_acc, int corr_acc, double* loss_partial, int32_t* correct_partial) {
    __shared__ double s_loss[WAVES];
    __shared__ int32_t s_corr[WAVES];
    for (int off = 32; off > 0; off >>= 1) {
        loss_acc += __shfl_down(loss_acc, off);
        corr_acc += __shfl_down(corr_acc, off);
    }
    if ((threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < WAVES) { s_loss[threadIdx.x >> 6] = loss_acc; s_corr[threadIdx.x >> 6] = corr_acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if constexpr (WAVES == 4) {
            loss_partial[blockIdx.x] = (s_loss[0] + s_loss[1]) + (s_loss[2] + s_loss[3]);
            correct_partial[blockIdx.x] = s_corr[0] + s_corr[1] + s_corr[2] + s_corr[3];
        } else {
            loss_partial[blockIdx.x] = s_loss[0] + s_loss[1];
            correct_partial[blockIdx.x] = s_corr[0] + s_corr[1];
        }
    }
}

// ---- softmax mode ------------------------------------------------------------------------------------------------------
template <int DLP>
__global__ __launch_bounds__(256) void head_forward_kernel(HeadArgs A, int32_t NB, int32_t ldz) {
    extern __shared__ float lds[];
    const int C = A.C, DL = A.DL;
    const int wstride = DLP > 0 ? DLP : DL;
    float* s_wo = lds;                               // [C][wstride]
    float* s_z = lds + C * wstride;                  // [NB][ldz]
    for (int i = threadIdx.x; i < C * wstride; i += blockDim.x) {
        const int c = i / wstride, j = i % wstride;
        s_wo[i] = j < DL ? A.Wo[c * DL + j] : 0.f;
    }
    __syncthreads();
    double loss_acc = 0.0;
    int corr_acc = 0;
    const int64_t ntiles = (A.n_rows + NB - 1) / NB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * NB;
        const int t = threadIdx.x;
        const int64_t n = n0 + t;
        if (t < NB && n < A.n_rows) {
            const float* x = A.X + n * DL;
            if constexpr (DLP > 0) {
                float xr[DLP];
#pragma unroll
                for (int j = 0; j < DLP; ++j) xr[j] = j < DL ? x[j] : 0.f;
                softmax_row<DLP, false>(s_wo, xr, DL, C, A.labels + n, s_z + t * ldz, loss_acc, corr_acc);
            } else {
                softmax_row<0, false>(s_wo, x, DL, C, A.labels + n, s_z + t * ldz, loss_acc, corr_acc);
            }
        }
        __syncthreads();
        const int rows_here = (int)((A.n_rows - n0 < NB) ? (A.n_rows - n0) : NB);
        tile_store_y(A.y + n0 * C, s_z, ldz, C, rows_here);
        __syncthreads();
    }
    head_block_partial<4>(loss_acc, corr_acc, A.loss_partial, A.correct_partial);
}

__global__ __launch_bounds__(256) void head_backward_kernel(HeadArgs A, int32_t NB, int32_t ldz, int32_t per_thread) {
    extern __shared__ float lds[];
    const int C = A.C, DL = A.DL, H = A.H;
    float* s_wo = lds;                                   // [C*DL]
    float* s_dz = s_wo + C * DL;                         // [NB][ldz]
    float* s_hl = s_dz + NB * ldz;                       // [NB][DL]
    float* s_gh = s_hl + NB * DL;                        // [NB][DL]
    for (int i = threadIdx.x; i < C * DL; i += blockDim.x) s_wo[i] = A.Wo[i];
    float wacc[8];
#pragma unroll
    for (int p = 0; p < 8; ++p) wacc[p] = 0.f;
    const float inv_heads = 1.0f / (float)H;
    const int64_t ntiles = (A.n_rows + NB - 1) / NB;
    const int hd = H * DL;
    const int dqD = 256 / DL, drD = 256 % DL, dqH = 256 / hd, drH = 256 % hd;
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * NB;
        const int rows_here = (int)((A.n_rows - n0 < NB) ? (A.n_rows - n0) : NB);
        tile_load_dz(A.y + n0 * C, A.labels + n0, s_dz, ldz, C, rows_here);
        for (int q = threadIdx.x; q < rows_here * DL; q += 256) s_hl[q] = A.X[n0 * DL + q];
        __syncthreads();
        {
            int r = threadIdx.x / DL, d = threadIdx.x % DL;
            for (int q = threadIdx.x; q < rows_here * DL; q += 256) {
                float sum = 0.f;
                for (int c = 0; c < C; ++c) sum += s_wo[c * DL + d] * s_dz[r * ldz + c];
                s_gh[q] = sum;
                r += dqD; d += drD;
                if (d >= DL) { d -= DL; ++r; }
            }
        }
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int t = threadIdx.x + p * 256;
            if (p < per_thread && t < C * DL) {
                const int c = t / DL, d = t % DL;
                float acc = wacc[p];
                for (int r = 0; r < rows_here; ++r) acc += s_dz[r * ldz + c] * s_hl[r * DL + d];
                wacc[p] = acc;
            }
        }
        __syncthreads();
        if (A.gh_out != nullptr)
            for (int q = threadIdx.x; q < rows_here * DL; q += 256) A.gh_out[(n0 + q / DL) * (A.gh_stride ? A.gh_stride : DL) + q % DL] = s_gh[q];
        if (A.g != nullptr) {
            const float* hp = A.hpre + n0 * hd;
            float* gt = A.g + n0 * hd;
            int r = threadIdx.x / hd, x = threadIdx.x % hd;     // x = h*DL + d
            for (int q = threadIdx.x; q < rows_here * hd; q += 256) {
                const int d = x % DL;
                const float hv = A.flat_index ? A.hpre[(n0 + r) * DL + d] : hp[q];
                gt[q] = s_gh[r * DL + d] * (hv > 0.f ? 1.0f : A.slope) * inv_heads;
                r += dqH; x += drH;
                if (x >= hd) { x -= hd; ++r; }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int t = threadIdx.x + p * 256;
        if (p < per_thread && t < C * DL) A.partial[(int64_t)blockIdx.x * C * DL + t] = wacc[p];
    }
}

template <int DL>
__global__ __launch_bounds__(256) void head_backward2_kernel(HeadArgs A, int32_t ldz) {
    constexpr int NB = 128;
    extern __shared__ float lds[];
    const int C = A.C;
    const HeadTile L = head_tile_at(lds, C, NB, ldz, DL, DL);
    for (int i = threadIdx.x; i < C * DL; i += 256) L.s_wo[i] = A.Wo[i];
    GradWoParts<DL, 2> W;
    W.init(C, NB);
    const int64_t ntiles = (A.n_rows + NB - 1) / NB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * NB;
        const int rows_here = (int)((A.n_rows - n0 < NB) ? (A.n_rows - n0) : NB);
        __syncthreads();                                 // previous tile fully consumed
        tile_load_dz(A.y + n0 * C, A.labels + n0, L.s_dz, ldz, C, rows_here);
        for (int q = threadIdx.x; q < rows_here * DL; q += 256) L.s_x[q] = A.X[n0 * DL + q];
        __syncthreads();
        head_grads_blocked<DL, 2, false>(A, L, n0, rows_here, W);
    }
    head_partial_blocked(A, L, W);
}

template <int DL>
__global__ __launch_bounds__(256) void head_step_kernel(HeadArgs A, int32_t ldz) {
    constexpr int NB = 128;
    extern __shared__ float lds[];
    const int C = A.C;
    const HeadTile L = head_tile_at(lds, C, NB, ldz, DL, DL);
    for (int i = threadIdx.x; i < C * DL; i += 256) L.s_wo[i] = A.Wo[i];
    const int tid = threadIdx.x;
    GradWoParts<DL, 2> W;
    W.init(C, NB);
    double loss_acc = 0.0;
    int corr_acc = 0;
    const int64_t ntiles = (A.n_rows + NB - 1) / NB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * NB;
        const int rows_here = (int)((A.n_rows - n0 < NB) ? (A.n_rows - n0) : NB);
        __syncthreads();                                 // previous tile fully consumed (and s_wo loaded)
        if (tid < rows_here) {
            const int64_t n = n0 + tid;
            float x[DL];
#pragma unroll
            for (int j = 0; j < DL; ++j) { x[j] = A.X[n * DL + j]; L.s_x[tid * DL + j] = x[j]; }
            softmax_row<DL, true>(L.s_wo, x, DL, C, A.labels + n, L.s_dz + tid * ldz, loss_acc, corr_acc);
        }
        __syncthreads();
        head_grads_blocked<DL, 2, true>(A, L, n0, rows_here, W);
    }
    head_partial_blocked(A, L, W);
    head_block_partial<2>(loss_acc, corr_acc, A.loss_partial, A.correct_partial);      // loss / #correct live in waves 0-1
}

__global__ __launch_bounds__(64) void head_finalize_kernel(const double* __restrict__ lp,
                                                          const int32_t* __restrict__ cp, int32_t nb,
                                                          float* loss_out, int32_t* correct_out) {
    double l = 0.0; int c = 0;
    for (int i = threadIdx.x; i < nb; i += 64) { l += lp[i]; c += cp[i]; }
    for (int off = 32; off > 0; off >>= 1) { l += __shfl_down(l, off); c += __shfl_down(c, off); }
    if (threadIdx.x == 0) { *loss_out = (float)l; *correct_out = c; }
}

// loss sum and #correct as three floats that survive a float all-reduce exactly: the count is split
// into 12-bit halves (each half's sum over ranks stays below 2^24 for any realistic world size)
__global__ void pack_result_kernel(const float* __restrict__ loss, const int32_t* __restrict__ correct,
                                   float* __restrict__ dst) {
    if (threadIdx.x == 0) {
        const int32_t c = *correct;
        dst[0] = *loss; dst[1] = (float)(c & 4095); dst[2] = (float)(c >> 12);
    }
}

// ---- loss modes: BCE / MSE ---------------------------------------------------------------------------------------------
// y, loss term, dz and "correct" of one entry from its logit and target (the expressions of the header, fp32; hardware exp2 / log2 /
// rcp as in the softmax head: 1 ulp each, against the 1e-4 bars)
template <int MODE>
__device__ __forceinline__ void loss_entry(float z, float t, float& y, float& l, float& dz, int& ok) {
    if constexpr (MODE == GAT_LOSS_BCE) {
        const float e = __builtin_amdgcn_exp2f(-fabsf(z) * 1.4426950408889634f);     // exp(-|z|) in (0, 1]: no overflow for either sign
        const float r = __builtin_amdgcn_rcpf(1.0f + e);
        y = z >= 0.f ? r : e * r;
        // log1p(e): below 2^-10 the series e - e^2/2 (error < e^3/3), where 1 + e would round e away; absolute error < 1e-7 throughout
        const float lp = e < 0.0009765625f ? e * fmaf(-0.5f, e, 1.0f) : __logf(1.0f + e);
        l = fmaf(-t, z, fmaxf(z, 0.f)) + lp;
        dz = y - t;
        ok = (z > 0.f) == (t > 0.5f);
    } else {
        const float d = z - t;
        y = z; l = d * d; dz = 2.0f * d; ok = 0;
    }
}

__device__ __forceinline__ HeadTile loss_tile_setup(const HeadArgs& A, float* lds, int NB, int ldz, int ldx, int ws) {
    const HeadTile L = head_tile_at(lds, A.C, NB, ldz, ldx, ws);
    const int DL = A.DL;
    int c = threadIdx.x / DL, j = threadIdx.x % DL;
    const int dq = 256 / DL, dr = 256 % DL;
    for (int i = threadIdx.x; i < A.C * DL; i += 256) {
        L.s_wo[c * ws + j] = A.Wo[i];
        c += dq; j += dr;
        if (j >= DL) { j -= DL; ++c; }
    }
    return L;
}

// the tile's targets (NaN where the entry does not contribute: missing, or a row outside the mask) and input rows -> LDS
__device__ __forceinline__ void loss_tile_load(const HeadArgs& A, const HeadTile& L, int64_t n0, int rows_here) {
    const int C = A.C, DL = A.DL;
    {
        const float* tt = A.T + n0 * C;
        const int tot = rows_here * C;
        int r = threadIdx.x / C, c = threadIdx.x % C;
        const int dq = 256 / C, dr = 256 % C;
        constexpr int U = 8;                             // loads in flight per thread: the tile is one latency per 2048 entries, not per 256
        for (int q0 = threadIdx.x; q0 < tot; q0 += 256 * U) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) { const int q = q0 + u * 256; v[u] = q < tot ? tt[q] : 0.f; }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (q0 + u * 256 < tot) {
                    const bool on = A.mask == nullptr || A.mask[n0 + r] != 0;
                    L.s_dz[r * L.ldz + c] = on ? v[u] : __builtin_nanf("");
                }
                r += dq; c += dr;
                if (c >= C) { c -= C; ++r; }
            }
        }
    }
    {
        const float* xt = A.X + n0 * DL;
        int r = threadIdx.x / DL, j = threadIdx.x % DL;
        const int dq = 256 / DL, dr = 256 % DL;
        for (int q = threadIdx.x; q < rows_here * DL; q += 256) {
            L.s_x[r * L.ldx + j] = xt[q];
            r += dq; j += dr;
            if (j >= DL) { j -= DL; ++r; }
        }
    }
}

// One entry: from its logit and target (NaN = does not contribute) the loss / count into the thread's accumulators (LOSS); -> what the
// entry leaves behind: y (WRITE_Y) or dz (GRAD)
template <int MODE, bool WRITE_Y, bool LOSS, bool GRAD>
__device__ __forceinline__ float loss_entry_apply(float z, float t, double& loss_acc, int& corr_acc) {
    float y, l, dz; int ok;
    loss_entry<MODE>(z, t, y, l, dz, ok);
    const bool on = !(t != t);
    if constexpr (LOSS) { loss_acc += on ? (double)l : 0.0; corr_acc += (on && ok) ? 1 : 0; }
    if constexpr (GRAD) return on ? dz : 0.0f;
    return y;
}

// ---- the any-shape form: the tile's work dealt by flat index ----
// logits of the tile's entries q = r*C + c: y straight to yt[q] (WRITE_Y), dz over the target in LDS (GRAD)
template <int MODE, bool WRITE_Y, bool LOSS, bool GRAD>
__device__ __forceinline__ void loss_entries_any(const HeadArgs& A, const HeadTile& L, int rows_here, float* __restrict__ yt,
                                                 double& loss_acc, int& corr_acc) {
    const int C = A.C, DL = A.DL;
    int r = threadIdx.x / C, c = threadIdx.x % C;
    const int dq = 256 / C, dr = 256 % C;
    for (int q = threadIdx.x; q < rows_here * C; q += 256) {
        const float t = L.s_dz[r * L.ldz + c];
        const float* w = L.s_wo + c * L.ws;
        const float* x = L.s_x + r * L.ldx;
        float z = 0.f;
        for (int j = 0; j < DL; ++j) z = fmaf(w[j], x[j], z);          // ascending j, as the softmax head
        const float out = loss_entry_apply<MODE, WRITE_Y, LOSS, GRAD>(z, t, loss_acc, corr_acc);
        if constexpr (WRITE_Y) yt[q] = out;
        if constexpr (GRAD) L.s_dz[r * L.ldz + c] = out;
        r += dq; c += dr;
        if (c >= C) { c -= C; ++r; }
    }
}
// the block's gradWo partial: entry (c, d) = threadIdx.x + p*256 in wacc[p], p < ceil(C*DL / 256) <= 8
struct GradWoAny {
    float wacc[8]; int wc[8], wd[8];
    __device__ __forceinline__ void init(int DL) {
#pragma unroll
        for (int p = 0; p < 8; ++p) { wacc[p] = 0.f; const int t = threadIdx.x + p * 256; wc[p] = t / DL; wd[p] = t % DL; }
    }
};
// gH rows of the tile (one thread per (r, d)) and the tile's term of gradWo, from dz in LDS.  (head_backward_kernel is the softmax
// mode's kernel of this kind; the two share no piece: its tile is head_tile's, dense and of another size, which decides the rows a
// block sums and so the bits of gradWo, and it writes the full g besides.)
__device__ __forceinline__ void loss_grads_any(const HeadArgs& A, const HeadTile& L, int64_t n0, int rows_here, GradWoAny& W) {
    const int C = A.C, DL = A.DL, CD = C * DL;
    const int gstride = A.gh_stride ? A.gh_stride : DL;
    int r = threadIdx.x / DL, d = threadIdx.x % DL;
    const int dq = 256 / DL, dr = 256 % DL;
    for (int q = threadIdx.x; q < rows_here * DL; q += 256) {          // gH[r][d] = sum_c dz[r][c] Wo[c][d], ascending c
        const float* dzr = L.s_dz + r * L.ldz;
        float acc = 0.f;
        for (int c = 0; c < C; ++c) acc = fmaf(L.s_wo[c * L.ws + d], dzr[c], acc);
        A.gh_out[(n0 + r) * gstride + d] = acc;
        r += dq; d += dr;
        if (d >= DL) { d -= DL; ++r; }
    }
#pragma unroll
    for (int p = 0; p < 8; ++p) {                                       // gradWo[c][d] += sum_r dz[r][c] X[r][d], ascending r
        if (threadIdx.x + p * 256 < CD) {
            float acc = W.wacc[p];
            const float* dzc = L.s_dz + W.wc[p];
            const float* xd = L.s_x + W.wd[p];
            for (int rr = 0; rr < rows_here; ++rr) acc = fmaf(dzc[rr * L.ldz], xd[rr * L.ldx], acc);
            W.wacc[p] = acc;
        }
    }
}
__device__ __forceinline__ void loss_partial_any(const HeadArgs& A, const GradWoAny& W) {
    const int CD = A.C * A.DL;
#pragma unroll
    for (int p = 0; p < 8; ++p) {
        const int t = threadIdx.x + p * 256;
        if (t < CD) A.partial[(int64_t)blockIdx.x * CD + t] = W.wacc[p];
    }
}

// ---- the register-blocked form: D_last = DLT in {4, 8, 16}, C <= 128, ws == DLT ----
// thread (row, column half): the row's X in registers, its columns in ascending order; half is wave-uniform, so is c, and the Wo reads
// broadcast.  What an entry leaves behind (y or dz) stays in the LDS tile.
template <int MODE, int DLT, bool WRITE_Y, bool LOSS, bool GRAD>
__device__ __forceinline__ void loss_entries_blocked(const HeadArgs& A, const HeadTile& L, int rows_here, double& loss_acc, int& corr_acc) {
    const int C = A.C;
    const int r = threadIdx.x & 127, half = threadIdx.x >> 7;
    const int ch = (C + 1) >> 1;
    const int c0 = half * ch, c1 = (c0 + ch < C) ? c0 + ch : C;
    if (r >= rows_here) return;
    float x[DLT];
#pragma unroll
    for (int j = 0; j < DLT; ++j) x[j] = L.s_x[r * L.ldx + j];
    float* tr = L.s_dz + r * L.ldz;
    for (int c = c0; c < c1; ++c) {
        const float* w = L.s_wo + c * DLT;
        float z = 0.f;
#pragma unroll
        for (int j = 0; j < DLT; ++j) z = fmaf(w[j], x[j], z);          // ascending j, as the softmax head
        tr[c] = loss_entry_apply<MODE, WRITE_Y, LOSS, GRAD>(z, tr[c], loss_acc, corr_acc);
    }
}

// DLT = 0: the any-shape form; DLT = D_last: the register-blocked form
template <int MODE, int DLT>
__global__ __launch_bounds__(256) void loss_head_forward_kernel(HeadArgs A, int32_t NB, int32_t ldz, int32_t ldx, int32_t ws) {
    extern __shared__ float lds[];
    const HeadTile L = loss_tile_setup(A, lds, NB, ldz, ldx, ws);
    double loss_acc = 0.0;
    int corr_acc = 0;
    const int64_t ntiles = (A.n_rows + NB - 1) / NB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * NB;
        const int rows_here = (int)((A.n_rows - n0 < NB) ? (A.n_rows - n0) : NB);
        __syncthreads();                                 // previous tile fully consumed (and Wo loaded)
        loss_tile_load(A, L, n0, rows_here);
        __syncthreads();
        if constexpr (DLT > 0) {
            loss_entries_blocked<MODE, DLT, true, true, false>(A, L, rows_here, loss_acc, corr_acc);
            __syncthreads();
            tile_store_y(A.y + n0 * A.C, L.s_dz, L.ldz, A.C, rows_here);
        } else {
            loss_entries_any<MODE, true, true, false>(A, L, rows_here, A.y + n0 * A.C, loss_acc, corr_acc);
        }
    }
    head_block_partial<4>(loss_acc, corr_acc, A.loss_partial, A.correct_partial);
}

// z recomputed as in the forward kernel; dz in LDS; gH rows and the block's gradWo partial.  FUSED: the loss / count partials too.
template <int MODE, bool FUSED, int DLT>
__global__ __launch_bounds__(256) void loss_head_grad_kernel(HeadArgs A, int32_t NB, int32_t ldz, int32_t ldx, int32_t ws) {
    extern __shared__ float lds[];
    const HeadTile L = loss_tile_setup(A, lds, NB, ldz, ldx, ws);
    double loss_acc = 0.0;
    int corr_acc = 0;
    typename std::conditional<(DLT > 0), GradWoParts<(DLT > 0 ? DLT : 1), 0>, GradWoAny>::type W;
    if constexpr (DLT > 0) W.init(A.C, NB); else W.init(A.DL);
    const int64_t ntiles = (A.n_rows + NB - 1) / NB;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t n0 = tile * NB;
        const int rows_here = (int)((A.n_rows - n0 < NB) ? (A.n_rows - n0) : NB);
        __syncthreads();                                 // previous tile fully consumed (and Wo loaded)
        loss_tile_load(A, L, n0, rows_here);
        __syncthreads();
        if constexpr (DLT > 0) loss_entries_blocked<MODE, DLT, false, FUSED, true>(A, L, rows_here, loss_acc, corr_acc);
        else loss_entries_any<MODE, false, FUSED, true>(A, L, rows_here, nullptr, loss_acc, corr_acc);
        __syncthreads();
        if constexpr (DLT > 0) head_grads_blocked<DLT, 0, false>(A, L, n0, rows_here, W);
        else loss_grads_any(A, L, n0, rows_here, W);
    }
    if constexpr (DLT > 0) head_partial_blocked(A, L, W);
    else loss_partial_any(A, W);
    if constexpr (FUSED) head_block_partial<4>(loss_acc, corr_acc, A.loss_partial, A.correct_partial);
}

constexpr unsigned long long kNoBadTarget = ~0ull;
__global__ __launch_bounds__(256) void targets_check_kernel(const float* __restrict__ t, int64_t n, int32_t bce,
                                                            unsigned long long* __restrict__ result) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float v = t[i];
        if (v != v) continue;                            // NaN: a missing entry
        if (fabsf(v) == INFINITY || (bce && (v < 0.f || v > 1.f))) { atomicMin(result, (unsigned long long)i); break; }   // ascending i: the thread's lowest
    }
}

__global__ __launch_bounds__(256) void target_count_kernel(const float* __restrict__ T, const uint8_t* __restrict__ mask, int64_t n_rows,
                                                           int32_t C, unsigned long long* __restrict__ part) {
    __shared__ unsigned long long s_n[256];
    unsigned long long cnt = 0;
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (int64_t)gridDim.x * 256) {
        if (mask != nullptr && !mask[r]) continue;
        const float* tr = T + r * C;
        for (int c = 0; c < C; ++c) cnt += tr[c] == tr[c] ? 1 : 0;
    }
    s_n[threadIdx.x] = cnt;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) s_n[threadIdx.x] += s_n[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = s_n[0];
}

}  // namespace

// labels_eff[i] = mask[i] ? labels[i] : ~labels[i]   (mask == nullptr: copy)
__global__ __launch_bounds__(256) void apply_mask_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ mask,
                                                         int32_t* __restrict__ eff, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        eff[i] = (mask == nullptr || mask[i]) ? labels[i] : ~labels[i];
}
// Loss / accuracy of the last forward over the nodes of `mask` (validation / test split): per block a fixed-order
// partial {sum of -log(max(y[label], 1e-12)), #correct, #nodes}; the host adds the block partials in order.
__global__ __launch_bounds__(256) void eval_mask_kernel(const float* __restrict__ y, const int32_t* __restrict__ labels,
                                                        const uint8_t* __restrict__ mask, int64_t n, int32_t C,
                                                        double* __restrict__ part_loss, int32_t* __restrict__ part_cnt) {
    __shared__ double s_l[256];
    __shared__ int32_t s_c[256], s_n[256];
    double l = 0.0; int32_t cr = 0, nn = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        if (!mask[i]) continue;
        const float* yr = y + i * C;
        const int lab = labels[i];
        float best = -1.f; int pred = 0;
        for (int c = 0; c < C; ++c) if (c == 0 || yr[c] > best) { best = yr[c]; pred = c; }      // strict >, first max wins (E:530-535)
        l += (double)(-logf(fmaxf(yr[lab], 1e-12f)));
        cr += pred == lab; ++nn;
    }
    s_l[threadIdx.x] = l; s_c[threadIdx.x] = cr; s_n[threadIdx.x] = nn;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) { s_l[threadIdx.x] += s_l[threadIdx.x + off]; s_c[threadIdx.x] += s_c[threadIdx.x + off]; s_n[threadIdx.x] += s_n[threadIdx.x + off]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part_loss[blockIdx.x] = s_l[0]; part_cnt[2 * blockIdx.x] = s_c[0]; part_cnt[2 * blockIdx.x + 1] = s_n[0]; }
}

// ---- host side: one sizing rule per family, three entry points -----------------------------------------------------------------
// A kernel with its tile: what a launch passes and what head_shape_check asks.  Every head kernel is persistent over row tiles:
// its grid is what the partial buffers hold, capped by what is resident at once.
struct HeadLaunch { const void* fn; int32_t NB, ldz, ldx, ws, per_thread; size_t lds; };
static int head_grid(int64_t cap, const HeadLaunch& p) {
    return (int)std::max<int64_t>(1, std::min(cap, resident_blocks(p.fn, p.lds)));
}
static int head_finalize(const HeadArgs& a, int blocks, bool batched, hipStream_t s) {
    if (batched && reduce_batch_finalize(a.loss_partial, a.correct_partial, blocks, a.loss_out, a.correct_out)) return 0;
    hipLaunchKernelGGL(head_finalize_kernel, dim3(1), dim3(64), 0, s, a.loss_partial, a.correct_partial, blocks, a.loss_out, a.correct_out);
    GAT_HIP(hipGetLastError());
    return 0;
}
static const char* const kTileLimit = "output head: num_classes*D_last too large for the LDS tile";

int head_blocks(int64_t n_rows) {
    // nodes per block: 128 = one tile of the fused head kernel per block (GAT_HEAD_NODES=256: two tiles in sequence per block, as before)
    static const int per = [] { const char* e = choice_env("GAT_HEAD_NODES"); const int v = e ? atoi(e) : 0; return v == 256 ? 256 : 128; }();
    const int64_t b = (n_rows + per - 1) / per;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
int head_bwd_blocks(int64_t n_rows) {
    const int64_t b = (n_rows + 127) / 128;          // head_backward2_kernel: 128-node tiles
    return (int)(b < 1 ? 1 : (b > 1024 ? 1024 : b));
}

// -- softmax mode --
// NB rows of ldz (odd: conflict-free rows) + extra_per_row floats beside Wo [C][ws] in 60 KiB
static bool head_tile(int32_t C, int32_t ws, int32_t extra_per_row, HeadLaunch* p) {
    p->ldz = C | 1;
    const int64_t budget = 60 * 1024 / 4 - (int64_t)C * ws;      // floats
    int nb = 256;
    while (nb >= 32 && (int64_t)nb * (p->ldz + extra_per_row) > budget) nb >>= 1;
    p->NB = nb;
    p->lds = ((size_t)C * ws + (size_t)nb * (p->ldz + extra_per_row)) * sizeof(float);
    return nb >= 32;
}
static bool head_forward_plan(int32_t C, int32_t DL, HeadLaunch* p) {
    const int dlp = DL <= 8 ? 8 : (DL <= 16 ? 16 : (DL <= 32 ? 32 : (DL <= 64 ? 64 : 0)));
    p->fn = dlp == 8 ? (const void*)head_forward_kernel<8> : dlp == 16 ? (const void*)head_forward_kernel<16>
          : dlp == 32 ? (const void*)head_forward_kernel<32> : dlp == 64 ? (const void*)head_forward_kernel<64>
                                                                         : (const void*)head_forward_kernel<0>;
    return head_tile(C, dlp ? dlp : DL, 0, p);
}
// head_backward_kernel: the tile also holds the H_L and gH rows; a thread owns up to 8 entries of gradWo (the caller holds C*DL <= 2048)
static bool head_backward_plan(int32_t C, int32_t DL, HeadLaunch* p) {
    p->fn = (const void*)head_backward_kernel;
    p->per_thread = (C * DL + 255) / 256;
    return head_tile(C, DL, 2 * DL, p);
}
// head_backward2_kernel / head_step_kernel: one 128-row tile of dz and H_L rows; fits at every shape they take
static bool head_blocked_shape(int32_t C, int32_t DL) { return C <= 64 && (DL == 4 || DL == 8 || DL == 16); }
static void head_blocked_plan(int32_t C, int32_t DL, bool step, HeadLaunch* p) {
    p->fn = step ? (DL == 4 ? (const void*)head_step_kernel<4> : DL == 8 ? (const void*)head_step_kernel<8> : (const void*)head_step_kernel<16>)
                 : (DL == 4 ? (const void*)head_backward2_kernel<4> : DL == 8 ? (const void*)head_backward2_kernel<8> : (const void*)head_backward2_kernel<16>);
    p->NB = 128; p->ldz = C | 1;
    p->lds = ((size_t)C * DL + (size_t)128 * (p->ldz + DL)) * sizeof(float);
}

// -- loss modes --
// NB rows per tile (<= 128), the strides (ldz, ldx odd; ws odd, or D_last in the register-blocked form) and the kernels' form: the
// register-blocked one when D_last is 4, 8 or 16, C <= 128 and the parts of the block's gradWo fit in the tile region at the end, else
// the any-shape one.  fn: forward, gradient, fused gradient.  false: not even one row fits beside Wo.  One function for every launch of a
// mode: the same form, hence (loss_head_blocks) the same grid and the same loss bits.
static bool loss_head_plan(int32_t C, int32_t DL, int32_t mode, HeadLaunch* p, const void* fn[3]) {
    p->ldz = C | 1; p->ldx = DL | 1;
    // GAT_LOSS_BLOCKED=0: the any-shape form at every shape (A/B: tools/loss_cost.py, tests/test_loss_modes.py)
    static const bool blocked_on = [] { const char* e = choice_env("GAT_LOSS_BLOCKED"); return !(e && e[0] == '0'); }();
    const bool blocked_shape = blocked_on && (DL == 4 || DL == 8 || DL == 16) && C <= 128;
    p->ws = blocked_shape ? DL : (DL | 1);
    const int64_t budget = 60 * 1024 / 4 - (int64_t)C * p->ws;       // floats
    const int64_t nb = budget / (p->ldz + p->ldx);
    p->NB = (int32_t)(nb > 128 ? 128 : nb);
    if (nb < 1) return false;
    int dlt = 0;
    if (blocked_shape && (int64_t)(128 / C) * C * DL <= (int64_t)p->NB * (p->ldz + p->ldx)) dlt = DL;
    else p->ws = DL | 1;
    p->lds = ((size_t)C * p->ws + (size_t)p->NB * (p->ldz + p->ldx)) * sizeof(float);
#define GAT_LOSS_FNS(M, D) { fn[0] = (const void*)loss_head_forward_kernel<M, D>; fn[1] = (const void*)loss_head_grad_kernel<M, false, D>; fn[2] = (const void*)loss_head_grad_kernel<M, true, D>; }
#define GAT_LOSS_FNS_D(M) switch (dlt) { case 4: GAT_LOSS_FNS(M, 4) break; case 8: GAT_LOSS_FNS(M, 8) break; case 16: GAT_LOSS_FNS(M, 16) break; default: GAT_LOSS_FNS(M, 0) break; }
    if (mode == GAT_LOSS_BCE) { GAT_LOSS_FNS_D(GAT_LOSS_BCE) } else { GAT_LOSS_FNS_D(GAT_LOSS_MSE) }
#undef GAT_LOSS_FNS_D
#undef GAT_LOSS_FNS
    return true;
}
// One grid for the three kernels of a mode (the loss partials of the forward and of the fused gradient kernel must pair up): the
// tiles, the two partial buffers, and what is resident at once of the kernel that fits the fewest blocks
int loss_head_blocks(int64_t n_rows, int32_t C, int32_t DL, int32_t mode) {
    HeadLaunch p{};
    const void* fn[3];
    if (!loss_head_plan(C, DL, mode, &p, fn)) return -1;
    int64_t blocks = std::min<int64_t>((n_rows + p.NB - 1) / p.NB, std::min(head_bwd_blocks(n_rows), head_blocks(n_rows)));
    for (int k = 0; k < 3; ++k) blocks = std::min(blocks, resident_blocks(fn[k], p.lds));
    return (int)std::max<int64_t>(1, blocks);
}
// which: 0 forward, 1 gradient, 2 fused gradient (with the loss / count partials and their finalize)
static int launch_loss_head(const HeadArgs& a, int which, hipStream_t s) {
    if (which != 0 && (int64_t)a.C * a.DL > 2048) return fail(GAT_E_UNSUPPORTED, "output head: num_classes*D_last > 2048");
    HeadLaunch p{};
    const void* fn[3];
    if (!loss_head_plan(a.C, a.DL, a.mode, &p, fn)) return fail(GAT_E_UNSUPPORTED, kTileLimit);
    const int blocks = loss_head_blocks(a.n_rows, a.C, a.DL, a.mode);
    HeadArgs arg = a;
    void* args[] = {&arg, &p.NB, &p.ldz, &p.ldx, &p.ws};
    GAT_HIP(hipLaunchKernel(fn[which], dim3((unsigned)blocks), dim3(256), args, p.lds, s));
    if (which == 0 ? a.loss_out != nullptr : which == 2) GAT_TRY(head_finalize(a, blocks, which == 2, s));
    if (which == 0) return 0;
    return launch_reduce_partials_add(a.partial, blocks, (int64_t)a.C * a.DL, a.gradWo, s);
}

// -- the entry points --
int launch_head_forward(const HeadArgs& a, hipStream_t s) {
    if (a.mode != 0) return launch_loss_head(a, 0, s);
    HeadLaunch p{};
    if (!head_forward_plan(a.C, a.DL, &p)) return fail(GAT_E_UNSUPPORTED, kTileLimit);
    const int blocks = head_grid(head_blocks(a.n_rows), p);
    HeadArgs arg = a;
    void* args[] = {&arg, &p.NB, &p.ldz};
    GAT_HIP(hipLaunchKernel(p.fn, dim3((unsigned)blocks), dim3(256), args, p.lds, s));
    return head_finalize(a, blocks, false, s);
}
// the fused step's kernel exists: every loss-mode shape; softmax without a full g, at the register-blocked shapes
bool head_step_supported(const HeadArgs& a) { return a.mode != 0 || (a.g == nullptr && head_blocked_shape(a.C, a.DL)); }
int launch_head_backward(const HeadArgs& a, hipStream_t s) {
    if (a.mode != 0) return launch_loss_head(a, 1, s);
    HeadLaunch p{};
    HeadArgs arg = a;
    if (head_step_supported(a) && a.gh_out != nullptr) {                // (head_backward2_kernel writes gH, always)
        head_blocked_plan(a.C, a.DL, false, &p);
        void* args[] = {&arg, &p.ldz};
        const int blocks = head_grid(head_bwd_blocks(a.n_rows), p);
        GAT_HIP(hipLaunchKernel(p.fn, dim3((unsigned)blocks), dim3(256), args, p.lds, s));
        return launch_reduce_partials_add(a.partial, blocks, (int64_t)a.C * a.DL, a.gradWo, s);
    }
    if (!head_backward_plan(a.C, a.DL, &p)) return fail(GAT_E_UNSUPPORTED, kTileLimit);
    if (p.per_thread > 8) return fail(GAT_E_UNSUPPORTED, "output head: num_classes*D_last > 2048");
    void* args[] = {&arg, &p.NB, &p.ldz, &p.per_thread};
    const int blocks = head_grid(head_bwd_blocks(a.n_rows), p);
    GAT_HIP(hipLaunchKernel(p.fn, dim3((unsigned)blocks), dim3(256), args, p.lds, s));
    return launch_reduce_partials_add(a.partial, blocks, (int64_t)a.C * a.DL, a.gradWo, s);
}
int launch_head_step(const HeadArgs& a, hipStream_t s) {
    if (a.mode != 0) return launch_loss_head(a, 2, s);
    if (!head_step_supported(a)) return fail(GAT_E_UNSUPPORTED, "head_step: shape outside the fused kernel");
    HeadLaunch p{};
    head_blocked_plan(a.C, a.DL, true, &p);
    const int blocks = head_grid(std::min(head_blocks(a.n_rows), head_bwd_blocks(a.n_rows)), p);      // both partial buffers
    HeadArgs arg = a;
    void* args[] = {&arg, &p.ldz};
    GAT_HIP(hipLaunchKernel(p.fn, dim3((unsigned)blocks), dim3(256), args, p.lds, s));
    GAT_TRY(head_finalize(a, blocks, true, s));
    return launch_reduce_partials_add(a.partial, blocks, (int64_t)a.C * a.DL, a.gradWo, s);
}
// The limits the entry points above apply to (C, DL), asked without a launch (the hidden layer's width is checked with it)
int head_shape_check(int32_t C, int32_t DL, int32_t mode, std::string* limit) {
    if ((int64_t)C * DL > 2048) { *limit = "num_classes * width <= 2048"; return GAT_E_UNSUPPORTED; }
    HeadLaunch p{};
    const void* fn[3];
    const bool fits = mode != 0 ? loss_head_plan(C, DL, mode, &p, fn)
                                : head_forward_plan(C, DL, &p) && (head_blocked_shape(C, DL) || head_backward_plan(C, DL, &p));
    if (!fits) { *limit = "the head's LDS tile (Wo and its row tile in 60 KiB)"; return GAT_E_UNSUPPORTED; }
    return 0;
}

int launch_pack_result(const float* loss, const int32_t* correct, float* dst3, hipStream_t s) {
    hipLaunchKernelGGL(pack_result_kernel, dim3(1), dim3(64), 0, s, loss, correct, dst3);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_apply_mask(const int32_t* labels, const uint8_t* mask, int32_t* eff, int64_t n, hipStream_t s) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(apply_mask_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 4096)), dim3(256), 0, s, labels, mask, eff, n);
    GAT_HIP(hipGetLastError());
    return 0;
}
int launch_eval_mask(const float* y, const int32_t* labels, const uint8_t* mask, int64_t n, int32_t C, double* part_loss,
                     int32_t* part_cnt, int32_t blocks, hipStream_t s) {
    hipLaunchKernelGGL(eval_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, labels, mask, n, C, part_loss, part_cnt);
    GAT_HIP(hipGetLastError());
    return 0;
}

int64_t targets_check_host(const float* t, int64_t n, int32_t mode) {
    for (int64_t i = 0; i < n; ++i) {
        const float v = t[i];
        if (v != v) continue;
        if (std::fabs(v) == INFINITY || (mode == GAT_LOSS_BCE && (v < 0.f || v > 1.f))) return i;
    }
    return -1;
}
int targets_check_device(const float* d_t, int64_t n, int32_t mode, unsigned long long* d_scratch, int64_t* where, hipStream_t s) {
    GAT_HIP(hipMemsetAsync(d_scratch, 0xFF, sizeof(unsigned long long), s));
    if (n > 0) {
        hipLaunchKernelGGL(targets_check_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 2048)), dim3(256), 0, s, d_t, n,
                           mode == GAT_LOSS_BCE ? 1 : 0, d_scratch);
        GAT_HIP(hipGetLastError());
    }
    unsigned long long h = kNoBadTarget;
    GAT_HIP(hipMemcpyAsync(&h, d_scratch, sizeof(h), hipMemcpyDeviceToHost, s));
    GAT_HIP(hipStreamSynchronize(s));
    *where = h == kNoBadTarget ? -1 : (int64_t)h;
    return 0;
}
int launch_target_count(const float* T, const uint8_t* mask, int64_t n_rows, int32_t C, unsigned long long* part, hipStream_t s) {
    hipLaunchKernelGGL(target_count_kernel, dim3(256), dim3(256), 0, s, T, mask, n_rows, C, part);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
