// gat_rank.hip — ranking metrics on the device (gatv2_abi.h "ranking metrics"): per column of a score matrix the integer rank
// statistics behind ROC-AUC, average precision, MRR and Hits@K, from ONE sort of 64-bit keys.
//   1. rank_keys_kernel    one lane per (row, column) slot: key = column << 33 | image(score) << 1 | positive, the all-ones key for a
//                          slot that does not take part (it sorts behind every column); NaN scores counted per column
//   2. hipcub::DeviceRadixSort::SortKeys over the 33 + bit_width(C) bits in use, ping-pong between the two key buffers
//   3. hipcub::DeviceScan::InclusiveSum of "is a negative" over the sorted keys (uint32: slots < 2^31)
//   4. rank_columns_kernel one lane per (column, job): job 0 finds the column's segment by two binary searches and its counts, job
//                          1 + k the Hits@K count by one search on the prefix counts and one for the end of the tie group
//   5. rank_terms_kernel   rank_blocks_per_col blocks per column, each a contiguous part of the column's segment; a lane that holds a
//                          positive finds its tie group by a galloping + binary search on key >> 1 (O(log group), a saturated column is
//                          one group of millions), reads negatives below / equal / above and TP, FP from the prefix counts, adds its
//                          integer term (block sum, one integer atomic per block) and its two fp64 terms (fixed-order block partial)
//   6. rank_finish_kernel  one wave per column adds the column's block partials in a fixed order and divides by n_pos
// The two doubles are sums in an order fixed by the shape alone: bitwise reproducible.  No float atomics.
// Temporary memory: 20 B per slot (two key buffers, the prefix counts) plus hipcub's scratch (a few MB) and O(C) words.
#include "gat_internal.h"

#include <hipcub/hipcub.hpp>

namespace gat {

namespace {
constexpr int kRankThreads = 256;
constexpr uint64_t kRankAbsent = ~0ull;
constexpr int kRankScoreShift = 1, kRankColShift = 33;
constexpr int kRankLdsCols = 256;          // columns whose NaN counts go through LDS counters (more: global atomics)

// blocks the rank kernel gives every column: enough to fill the chip, never less than 512 rows each; a function of the shape alone
inline int32_t rank_blocks_per_col(int64_t n_rows, int32_t n_cols) {
    const int64_t by_chip = (2048 + n_cols - 1) / n_cols, by_rows = (n_rows + 511) / 512;
    return (int32_t)std::max<int64_t>(1, std::min(by_chip, by_rows));
}
inline int rank_col_bits(int32_t n_cols) {       // the all-ones column field must not be a column: 2^bits - 1 >= C
    int b = 1;
    while (((1ll << b) - 1) < (int64_t)n_cols) ++b;
    return b;
}

// unsigned image of a non-NaN float that sorts like the float; -0.0 and +0.0 share one image
__device__ __forceinline__ uint32_t rank_image(float x) {
    uint32_t u = __float_as_uint(x);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ void __launch_bounds__(kRankThreads)
rank_keys_kernel(const float* __restrict__ scores, int64_t stride, const int32_t* __restrict__ labels, const float* __restrict__ targets,
                 const uint8_t* __restrict__ mask, uint32_t n_slots, uint32_t C, unsigned long long* __restrict__ keys, gat_rank_stats* __restrict__ stats) {
    __shared__ unsigned int nan_cnt[kRankLdsCols];
    const bool lds = C <= (uint32_t)kRankLdsCols;
    if (lds) {
        for (uint32_t i = threadIdx.x; i < C; i += kRankThreads) nan_cnt[i] = 0u;
        __syncthreads();
    }
    const uint32_t idx = blockIdx.x * (uint32_t)kRankThreads + threadIdx.x;
    if (idx < n_slots) {
        const uint32_t r = idx / C, c = idx - r * C;
        unsigned long long key = kRankAbsent;
        if (mask == nullptr || mask[r] != 0) {
            bool present, positive;
            if (targets != nullptr) {
                const float t = targets[idx];
                present = !(t != t);
                positive = t > 0.5f;
            } else {
                present = true;
                positive = labels[r] == (int32_t)c;
            }
            if (present) {
                const float y = scores[(int64_t)r * stride + c];
                if (y != y) {
                    if (lds) atomicAdd(&nan_cnt[c], 1u);
                    else atomicAdd((unsigned long long*)&stats[c].n_nan, 1ull);
                } else {
                    key = ((unsigned long long)c << kRankColShift) | ((unsigned long long)rank_image(y) << kRankScoreShift) | (positive ? 1ull : 0ull);
                }
            }
        }
        keys[idx] = key;
    }
    if (lds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < C; i += kRankThreads)
            if (nan_cnt[i] != 0u) atomicAdd((unsigned long long*)&stats[i].n_nan, (unsigned long long)nan_cnt[i]);
    }
}

struct RankIsNegative {
    __host__ __device__ __forceinline__ uint32_t operator()(const unsigned long long& k) const { return (uint32_t)((k & 1ull) == 0ull); }
};

// first index in [lo, hi) whose key is >= `key`, hi when there is none
__device__ __forceinline__ uint32_t rank_lower_bound(const unsigned long long* __restrict__ keys, uint32_t lo, uint32_t hi, unsigned long long key) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// negatives among the sorted slots [0, i)
__device__ __forceinline__ uint32_t rank_neg_before(const uint32_t* __restrict__ incl, uint32_t i) { return i ? incl[i - 1] : 0u; }

// seg[c] = {first slot, end slot, negatives before the first slot, negatives of the column}
__global__ void __launch_bounds__(kRankThreads)
rank_columns_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ incl, uint32_t n_slots, uint32_t C,
                    const int32_t* __restrict__ ks, int32_t n_ks, uint4* __restrict__ seg, gat_rank_stats* __restrict__ stats) {
    const uint64_t jobs = 1u + (uint32_t)n_ks;
    const uint64_t t = (uint64_t)blockIdx.x * kRankThreads + threadIdx.x;
    if (t >= C * jobs) return;
    const uint32_t c = (uint32_t)(t / jobs), job = (uint32_t)(t - c * jobs);
    const uint32_t lo = rank_lower_bound(keys, 0u, n_slots, (unsigned long long)c << kRankColShift);
    // behind the last column come the absent slots only (C << 33 would leave 64 bits at C = 2^31 - 1)
    const uint32_t hi = rank_lower_bound(keys, lo, n_slots, c + 1u == C ? kRankAbsent : (unsigned long long)(c + 1u) << kRankColShift);
    const uint32_t base = rank_neg_before(incl, lo), n_neg = rank_neg_before(incl, hi) - base, n_pos = (hi - lo) - n_neg;
    if (job == 0u) {
        seg[c] = make_uint4(lo, hi, base, n_neg);
        stats[c].n_pos = (int64_t)n_pos;
        stats[c].n_neg = (int64_t)n_neg;
        return;
    }
    const uint32_t K = (uint32_t)ks[job - 1u];
    uint32_t hits = n_pos;                              // fewer than K negatives: every positive counts
    if (n_neg >= K) {
        // the K-th highest negative is the column's (n_neg - K + 1)-th lowest: the first slot whose inclusive count reaches it
        const uint32_t want = base + (n_neg - K) + 1u;
        uint32_t a = lo, b = hi;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (incl[mid] < want) a = mid + 1; else b = mid;
        }
        // a < hi holds a negative; the positives strictly above it start behind its tie group
        const unsigned long long next_group = ((keys[a] >> 1) + 1ull) << 1;
        const uint32_t gh = rank_lower_bound(keys, a + 1u, hi, next_group);
        hits = (hi - gh) - (rank_neg_before(incl, hi) - rank_neg_before(incl, gh));
    }
    stats[c].hits[job - 1u] = (int64_t)hits;
}

// fixed-order sums over the block: lanes by a shuffle tree, the four waves in ascending order by thread 0
template <class T> __device__ __forceinline__ T rank_wave_sum(T v) {
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    return v;
}

__global__ void __launch_bounds__(kRankThreads)
rank_terms_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ incl, const uint4* __restrict__ seg, uint32_t blocks_per_col,
                  double* __restrict__ partial, gat_rank_stats* __restrict__ stats) {
    __shared__ double s_ap[kRankThreads / kWave], s_mrr[kRankThreads / kWave];
    __shared__ unsigned long long s_auc[kRankThreads / kWave];
    const uint32_t c = blockIdx.x / blocks_per_col, j = blockIdx.x - c * blocks_per_col;
    const uint4 sg = seg[c];
    const uint32_t lo = sg.x, hi = sg.y, base = sg.z, n_neg = sg.w;
    // this block's part of [lo, hi): ceil(len / blocks) slots rounded up to whole passes of the block (64-bit: the rounding may pass 2^32)
    const uint64_t len = hi - lo;
    uint64_t per = (len + blocks_per_col - 1) / blocks_per_col;
    per = (per + kRankThreads - 1) / kRankThreads * kRankThreads;
    const uint64_t beg64 = (uint64_t)lo + (uint64_t)j * per, end64 = beg64 + per < (uint64_t)hi ? beg64 + per : (uint64_t)hi;
    double ap = 0.0, mrr = 0.0;
    unsigned long long auc = 0ull;
    for (uint64_t i64 = beg64 + threadIdx.x; i64 < end64; i64 += kRankThreads) {
        const uint32_t i = (uint32_t)i64;
        const unsigned long long key = keys[i];
        if ((key & 1ull) == 0ull) continue;             // a negative: nothing to add
        const unsigned long long g = key >> 1;
        // the tie group [gl, gh) of g inside [lo, hi): gallop away from i, then bisect — never a walk
        int64_t good = (int64_t)i, bad = (int64_t)lo - 1;
        for (int64_t step = 1;; step <<= 1) {
            const int64_t p = good - step;
            if (p <= bad) break;
            if ((keys[p] >> 1) == g) good = p; else { bad = p; break; }
        }
        while (good - bad > 1) {
            const int64_t mid = bad + (good - bad) / 2;
            if ((keys[mid] >> 1) == g) good = mid; else bad = mid;
        }
        const uint32_t gl = (uint32_t)good;
        good = (int64_t)i; bad = (int64_t)hi;
        for (int64_t step = 1;; step <<= 1) {
            const int64_t p = good + step;
            if (p >= bad) break;
            if ((keys[p] >> 1) == g) good = p; else { bad = p; break; }
        }
        while (bad - good > 1) {
            const int64_t mid = good + (bad - good) / 2;
            if ((keys[mid] >> 1) == g) good = mid; else bad = mid;
        }
        const uint32_t gh = (uint32_t)good + 1u;
        const uint32_t before_gl = rank_neg_before(incl, gl);
        const uint32_t neg_below = before_gl - base, neg_eq = rank_neg_before(incl, gh) - before_gl, neg_above = n_neg - neg_below - neg_eq;
        auc += 2ull * neg_below + neg_eq;
        const uint32_t at_or_above = hi - gl, fp = n_neg - neg_below, tp = at_or_above - fp;      // entries, negatives, positives with score >= s
        ap += (double)tp / (double)at_or_above;
        mrr += 1.0 / (1.0 + (double)neg_above + 0.5 * (double)neg_eq);
    }
    ap = rank_wave_sum(ap); mrr = rank_wave_sum(mrr); auc = rank_wave_sum(auc);
    const int wave = threadIdx.x / kWave;
    if ((threadIdx.x & (kWave - 1)) == 0) { s_ap[wave] = ap; s_mrr[wave] = mrr; s_auc[wave] = auc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = s_ap[0], m = s_mrr[0];
        unsigned long long u = s_auc[0];
        for (int w = 1; w < kRankThreads / kWave; ++w) { a += s_ap[w]; m += s_mrr[w]; u += s_auc[w]; }
        partial[2 * (size_t)blockIdx.x] = a;
        partial[2 * (size_t)blockIdx.x + 1] = m;
        if (u != 0ull) atomicAdd((unsigned long long*)&stats[c].auc_num, u);
    }
}

__global__ void __launch_bounds__(kRankThreads)
rank_finish_kernel(const double* __restrict__ partial, uint32_t blocks_per_col, uint32_t C, gat_rank_stats* __restrict__ stats) {
    // one wave per column: lane l adds partials l, l + 64, ... in ascending order, the lanes combine by the shuffle tree — a fixed order
    const uint32_t c = blockIdx.x * (uint32_t)(kRankThreads / kWave) + threadIdx.x / kWave, lane = threadIdx.x & (kWave - 1);
    if (c >= C) return;
    double a = 0.0, m = 0.0;
    const double* p = partial + 2 * (size_t)c * blocks_per_col;
    for (uint32_t j = lane; j < blocks_per_col; j += kWave) { a += p[2 * j]; m += p[2 * j + 1]; }
    a = rank_wave_sum(a); m = rank_wave_sum(m);
    if (lane != 0) return;
    const int64_t n_pos = stats[c].n_pos;
    stats[c].ap = n_pos > 0 ? a / (double)n_pos : 0.0;
    stats[c].mrr = n_pos > 0 ? m / (double)n_pos : 0.0;
}
}  // namespace

int rank_check(const char* who, int64_t n_rows, int32_t n_cols, const int32_t* ks, int32_t n_ks) {
    if (n_rows < 0 || n_cols < 1) return fail(GAT_E_INVALID, std::string(who) + ": n_rows < 0 or n_cols < 1");
    if (n_ks < 0 || n_ks > GAT_RANK_MAX_KS) return fail(GAT_E_INVALID, std::string(who) + ": n_ks outside 0.." + std::to_string(GAT_RANK_MAX_KS));
    if (n_ks > 0 && !ks) return fail(GAT_E_INVALID, std::string(who) + ": null ks");
    for (int32_t i = 0; i < n_ks; ++i)
        if (ks[i] < 1) return fail(GAT_E_INVALID, std::string(who) + ": K must be >= 1");
    if (n_rows > ((1ll << 31) - 1) / n_cols)            // n_rows * n_cols >= 2^31, without forming a product that may leave 64 bits
        return fail(GAT_E_UNSUPPORTED, std::string(who) + ": n_rows * n_cols >= 2^31 slots (the sort and the prefix counts are 32-bit)");
    return 0;
}

int rank_sizes(int64_t n_rows, int32_t n_cols, RankSizes* out) {
    const int64_t slots = n_rows * (int64_t)n_cols;
    out->slots = slots;
    out->blocks_per_col = rank_blocks_per_col(n_rows, n_cols);
    out->partial_doubles = 2 * (int64_t)n_cols * out->blocks_per_col;
    size_t sort_bytes = 0, scan_bytes = 0;
    if (slots > 0) {
        hipcub::DoubleBuffer<unsigned long long> keys(nullptr, nullptr);
        GAT_HIP(hipcub::DeviceRadixSort::SortKeys(nullptr, sort_bytes, keys, (int)slots, 0, kRankColShift + rank_col_bits(n_cols)));
        hipcub::TransformInputIterator<uint32_t, RankIsNegative, const unsigned long long*> neg((const unsigned long long*)nullptr, RankIsNegative());
        GAT_HIP(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, neg, (uint32_t*)nullptr, (int)slots));
    }
    out->temp_bytes = std::max<size_t>(std::max(sort_bytes, scan_bytes), 16);
    return 0;
}

int launch_rank_stats(const RankArgs& a, const RankBuffers& b, hipStream_t s) {
    const int64_t slots = a.n_rows * (int64_t)a.n_cols;
    const uint32_t C = (uint32_t)a.n_cols;
    GAT_HIP(hipMemsetAsync(b.stats, 0, (size_t)C * sizeof(gat_rank_stats), s));
    if (slots == 0) return 0;                           // no rows: every count is 0
    if (a.n_ks > 0) GAT_HIP(hipMemcpyAsync(b.ks, a.ks, (size_t)a.n_ks * sizeof(int32_t), hipMemcpyHostToDevice, s));
    rank_keys_kernel<<<(unsigned)((slots + kRankThreads - 1) / kRankThreads), kRankThreads, 0, s>>>(
        a.scores, a.score_stride, a.labels, a.targets, a.mask, (uint32_t)slots, C, b.keys0, b.stats);
    GAT_HIP(hipGetLastError());
    hipcub::DoubleBuffer<unsigned long long> keys(b.keys0, b.keys1);
    size_t temp_bytes = b.temp_bytes;
    GAT_HIP(hipcub::DeviceRadixSort::SortKeys(b.temp, temp_bytes, keys, (int)slots, 0, kRankColShift + rank_col_bits(a.n_cols), s));
    const unsigned long long* sorted = keys.Current();
    hipcub::TransformInputIterator<uint32_t, RankIsNegative, const unsigned long long*> neg(sorted, RankIsNegative());
    temp_bytes = b.temp_bytes;
    GAT_HIP(hipcub::DeviceScan::InclusiveSum(b.temp, temp_bytes, neg, b.incl, (int)slots, s));
    const uint64_t col_jobs = (uint64_t)C * (1u + (uint32_t)a.n_ks);
    rank_columns_kernel<<<(unsigned)((col_jobs + kRankThreads - 1) / kRankThreads), kRankThreads, 0, s>>>(sorted, b.incl, (uint32_t)slots, C, b.ks, a.n_ks, b.seg, b.stats);
    GAT_HIP(hipGetLastError());
    const uint32_t bpc = (uint32_t)rank_blocks_per_col(a.n_rows, a.n_cols);
    rank_terms_kernel<<<C * bpc, kRankThreads, 0, s>>>(sorted, b.incl, b.seg, bpc, b.partial, b.stats);
    GAT_HIP(hipGetLastError());
    rank_finish_kernel<<<(C + kRankThreads / kWave - 1) / (kRankThreads / kWave), kRankThreads, 0, s>>>(b.partial, bpc, C, b.stats);
    GAT_HIP(hipGetLastError());
    return 0;
}

}  // namespace gat
