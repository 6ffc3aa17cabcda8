// gat_head_hidden.hip — the two row-streaming kernels of the hidden layer in front of the output head (gatv2_abi.h "hidden layer"):
// Z1 = act(A + b1) in place behind the product A = Xin W1^T, and gA = gZ1 (.) act'(Z1) in place with the block column sums of gA
// (gradb1) in front of the products gradW1 += gA^T Xin and gXin = gA W1.  The products themselves are the dense launchers of the
// residual term (gat_gemm_kernels.hip); the sequence is in gat_abi_step.hip.
//
// Both kernels share one layout, that of res_backward_kernel: a row is LPR lanes, a lane owns V consecutive columns of ITS column
// group in every row it visits (V = 4 when the width is a multiple of 4, else 1), a block is rpb = 256 / LPR rows, the grid is
// persistent (rows blockIdx * rpb + r_in, stride gridDim * rpb).  Consecutive lanes touch consecutive addresses at every width: a
// wave's access is one contiguous run of 64 * V floats.  The layout is a function of the width alone; VEC only says whether a lane's
// four floats travel as one 16-byte access (the row buffers are 16-byte aligned) or as four scalar ones.  A lane's column group never
// changes, so its b1 values (forward) and its running column sums (backward) live in registers.  U rows are loaded before the first
// is used: U independent 16-byte loads per operand and lane in flight.  A width beyond 256 * V columns is walked in rounds.
#include "gat_internal.h"

namespace gat {
namespace {

constexpr int kU = 4;       // rows in flight per lane

template <int V, bool VEC>
__device__ __forceinline__ void load_cols(const float* __restrict__ p, float (&v)[V]) {
    if constexpr (V == 4 && VEC) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) v[i] = p[i];
    }
}
template <int V, bool VEC>
__device__ __forceinline__ void store_cols(float* __restrict__ p, const float (&v)[V]) {
    if constexpr (V == 4 && VEC) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < V; ++i) p[i] = v[i];
    }
}

// a[r][c] = act(a[r][c] + b1[c]), act(t) = t > 0 ? t : slope * t.  The sum and the product are single fp32 operations (no fma: the
// seam's law is np.where(a + b1 > 0, a + b1, slope * (a + b1)) bit for bit).
template <int V, bool VEC>
__global__ __launch_bounds__(256) void head_hidden_forward_kernel(float* __restrict__ a, const float* __restrict__ b1, int64_t rows,
                                                                  int32_t width, float slope, int32_t LPR, int32_t rpb) {
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    if (r_in >= rpb) return;                             // (no barrier in this kernel)
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int base = 0; base < width; base += LPR * V) {
        const int c0 = base + cl * V;
        if (c0 >= width) continue;
        float bv[V];
#pragma unroll
        for (int i = 0; i < V; ++i) bv[i] = b1[c0 + i];
        for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < rows; row += kU * stride) {
            float x[kU][V];
#pragma unroll
            for (int k = 0; k < kU; ++k) {
                const int64_t r = row + k * stride;
                if (r < rows) load_cols<V, VEC>(a + r * width + c0, x[k]);
            }
#pragma unroll
            for (int k = 0; k < kU; ++k) {
                const int64_t r = row + k * stride;
                if (r >= rows) break;
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    const float s = __fadd_rn(x[k][i], bv[i]);
                    x[k][i] = s > 0.f ? s : __fmul_rn(slope, s);
                }
                store_cols<V, VEC>(a + r * width + c0, x[k]);
            }
        }
    }
}

// gz[r][c] *= z1[r][c] > 0 ? 1 : slope; partial[block][c] = the block's column sum of the result: a lane's running sum over its rows in
// ascending order, then the block's rpb row lanes in ascending order — a fixed order, bitwise reproducible.
template <int V, bool VEC>
__global__ __launch_bounds__(256) void head_hidden_backward_kernel(float* __restrict__ gz, const float* __restrict__ z1,
                                                                   float* __restrict__ partial, int64_t rows, int32_t width, float slope,
                                                                   int32_t LPR, int32_t rpb) {
    __shared__ float red[256 * 4];
    const int t = threadIdx.x;
    const int r_in = t / LPR, cl = t % LPR;
    const int64_t stride = (int64_t)gridDim.x * rpb;
    for (int base = 0; base < width; base += LPR * V) {  // the round count is the same for every lane (barriers below)
        const int c0 = base + cl * V;
        const bool active = r_in < rpb && c0 < width;
        float sum[V];
#pragma unroll
        for (int i = 0; i < V; ++i) sum[i] = 0.f;
        if (active) {
            for (int64_t row = (int64_t)blockIdx.x * rpb + r_in; row < rows; row += kU * stride) {
                float g[kU][V], z[kU][V];
#pragma unroll
                for (int k = 0; k < kU; ++k) {
                    const int64_t r = row + k * stride;
                    if (r < rows) {
                        load_cols<V, VEC>(gz + r * width + c0, g[k]);
                        load_cols<V, VEC>(z1 + r * width + c0, z[k]);
                    }
                }
#pragma unroll
                for (int k = 0; k < kU; ++k) {
                    const int64_t r = row + k * stride;
                    if (r >= rows) break;
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        g[k][i] = __fmul_rn(g[k][i], z[k][i] > 0.f ? 1.0f : slope);
                        sum[i] = __fadd_rn(sum[i], g[k][i]);
                    }
                    store_cols<V, VEC>(gz + r * width + c0, g[k]);
                }
            }
        }
        if (partial != nullptr) {                         // (uniform per block: every lane reaches the barriers)
#pragma unroll
            for (int i = 0; i < V; ++i) red[t * V + i] = sum[i];
            __syncthreads();
            if (r_in == 0 && c0 < width) {
#pragma unroll
                for (int i = 0; i < V; ++i) {
                    float tot = 0.f;
                    for (int r = 0; r < rpb; ++r) tot += red[(r * LPR + cl) * V + i];
                    partial[(int64_t)blockIdx.x * width + c0 + i] = tot;
                }
            }
            __syncthreads();
        }
    }
}

void hidden_shape(int32_t width, int* V, int* LPR, int* rpb) {
    *V = width % 4 == 0 ? 4 : 1;
    const int groups = width / *V;                       // column groups of a row
    *LPR = groups < 256 ? groups : 256;
    *rpb = 256 / *LPR;
}
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

int head_hidden_blocks(int64_t rows, int32_t width) {
    int V, LPR, rpb;
    hidden_shape(width, &V, &LPR, &rpb);
    // the scalar-access form of a layout has the form with 16-byte accesses' registers at most: one grid for both
    const void* fn = V == 4 ? (const void*)head_hidden_backward_kernel<4, false> : (const void*)head_hidden_backward_kernel<1, false>;
    const int64_t want = std::max<int64_t>(1, (rows + (int64_t)rpb * kU - 1) / ((int64_t)rpb * kU));
    return (int)std::min({want, resident_blocks(fn, 0), (int64_t)kHiddenPartialRows});
}

int launch_head_hidden_forward(float* a, const float* b1, int64_t rows, int32_t width, float slope, hipStream_t s) {
    if (rows <= 0) return 0;
    if (width < 1 || a == nullptr || b1 == nullptr) return fail(GAT_E_INVALID, "head_hidden_forward: bad argument");
    int V, LPR, rpb;
    hidden_shape(width, &V, &LPR, &rpb);
    const bool vec = V == 4 && aligned16(a);
    const void* fn = V == 4 ? (vec ? (const void*)head_hidden_forward_kernel<4, true> : (const void*)head_hidden_forward_kernel<4, false>)
                            : (const void*)head_hidden_forward_kernel<1, false>;
    const int64_t want = std::max<int64_t>(1, (rows + (int64_t)rpb * kU - 1) / ((int64_t)rpb * kU));
    const dim3 grid((unsigned)std::min(want, std::max<int64_t>(1, resident_blocks(fn, 0))));
    if (V == 4 && vec) hipLaunchKernelGGL((head_hidden_forward_kernel<4, true>), grid, dim3(256), 0, s, a, b1, rows, width, slope, LPR, rpb);
    else if (V == 4) hipLaunchKernelGGL((head_hidden_forward_kernel<4, false>), grid, dim3(256), 0, s, a, b1, rows, width, slope, LPR, rpb);
    else hipLaunchKernelGGL((head_hidden_forward_kernel<1, false>), grid, dim3(256), 0, s, a, b1, rows, width, slope, LPR, rpb);
    GAT_HIP(hipGetLastError());
    return 0;
}

int launch_head_hidden_backward(float* gz, const float* z1, float* partial, int64_t rows, int32_t width, float slope, hipStream_t s) {
    if (rows <= 0) return 0;
    if (width < 1 || gz == nullptr || z1 == nullptr) return fail(GAT_E_INVALID, "head_hidden_backward: bad argument");
    int V, LPR, rpb;
    hidden_shape(width, &V, &LPR, &rpb);
    const bool vec = V == 4 && aligned16(gz) && aligned16(z1);
    const dim3 grid((unsigned)std::max(1, head_hidden_blocks(rows, width)));      // == rows of partial
    if (V == 4 && vec) hipLaunchKernelGGL((head_hidden_backward_kernel<4, true>), grid, dim3(256), 0, s, gz, z1, partial, rows, width, slope, LPR, rpb);
    else if (V == 4) hipLaunchKernelGGL((head_hidden_backward_kernel<4, false>), grid, dim3(256), 0, s, gz, z1, partial, rows, width, slope, LPR, rpb);
    else hipLaunchKernelGGL((head_hidden_backward_kernel<1, false>), grid, dim3(256), 0, s, gz, z1, partial, rows, width, slope, LPR, rpb);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
