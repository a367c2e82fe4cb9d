// wf_accum.h -- the deterministic fp64 accumulation of per-walker values, written once for the units that use it: wf_kernels_observe.hip,
// wf_kernels_overlap.hip, wf_kernels_dmc.hip and wf_kernels_dmc_observe.hip.  With it: the LDS-privatised integer histograms of the one-body
// density and the pair distance (the observe and forward-walking units) and the launch status of these four units.
//
// THE ORDER OF SUMMATION.  It is part of the contract (the tests hold the sums to it bit for bit; waveflow_amd/_accum.py: ordered_sum restates
// it in numpy) and depends on the number of walkers B alone:
//   1. the grid: observe_blocks(B) = min(ceil(B / 256), 1024) workgroups of 256 lanes, a grid-stride loop: lane l of block j takes the walkers
//      b = j 256 + l, then + 256 observe_blocks(B), ... < B, and adds their terms to its lane sums in that (ascending) order, from 0.  A walker
//      that is skipped adds nothing, which is the same as adding 0.
//   2. the wave: v += shfl_down(v, off) for off = 32, 16, 8, 4, 2, 1 (wave_sum): lane 0 holds the wave's sum.
//   3. the block: t = wave 0; t += wave 1; t += wave 2; t += wave 3, through LDS (block_partial); one row of 8-byte words per block in the
//      workspace: the sums as their bit patterns, then the integer counts.
//   4. the blocks: a one-workgroup launch whose thread k owns column k: t = 0; t += row[b][k] for b = 0, 1, ... in block order
//      (reduce_columns; the rows pass through LDS 256 at a time, which changes no order), and then once: accumulator += t (the generation
//      record of DMC: record = t).
// No floating-point atomics anywhere.  Counts and histogram bins are integers: no order to depend on.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wf_internal.h"
#include "wf_layout.h"

namespace wf {

// ---- the grid rule
constexpr int kObsBlock = 256;            // one lane per walker
constexpr int64_t kObsMaxBlocks = 1024;   // the grid-stride loop takes the rest: the block partials of 14 words stay within 112 KB
constexpr int kAccumStageRows = 256;      // rows of partials per staging round of reduce_columns

// blocks of an accumulation launch: a function of B alone
inline int64_t observe_blocks(int64_t B) { return B < 1 ? 0 : (B + kObsBlock - 1) / kObsBlock < kObsMaxBlocks ? (B + kObsBlock - 1) / kObsBlock : kObsMaxBlocks; }
// bytes of `rows` block partials of `words` 8-byte words each
inline int64_t partial_bytes(int64_t rows, int words) { return align256(rows * words * 8); }

// ---- histogram geometry (host)
constexpr int kObsMaxDensityBins = 512, kObsMaxPairBins = 1024;

struct HistGeom {
    int nd, np;                 // bins (0: no such histogram)
    float lo, scale_d, scale_p;
};
inline HistGeom make_hist_geom(int n_density_bins, int n_pair_bins, float lo, float hi) {
    HistGeom g{};
    g.nd = n_density_bins;
    g.np = n_pair_bins;
    g.lo = lo;
    const float width = hi - lo;
    g.scale_d = (float)g.nd / width;
    g.scale_p = (float)g.np / width;
    return g;
}
inline bool hist_range_ok(float lo, float hi) { return std::isfinite(lo) && std::isfinite(hi) && lo < hi && std::isfinite(hi - lo); }
// WF_OK, or the refusal of these bins, arrays and range, in the order of wf_observe_accumulate
inline int hist_check(int n_density_bins, int n_pair_bins, float lo, float hi, const void* density, const void* pair) {
    if (n_density_bins < 0 || n_pair_bins < 0) return WF_ERR_INVALID;
    if (n_density_bins > kObsMaxDensityBins || n_pair_bins > kObsMaxPairBins) return WF_ERR_UNSUPPORTED;
    if ((n_density_bins > 0 && !density) || (n_pair_bins > 0 && !pair)) return WF_ERR_INVALID;
    return hist_range_ok(lo, hi) ? WF_OK : WF_ERR_INVALID;
}

// ---- launch status of the four units
inline int launch_status() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error((int)e);
        return WF_ERR_HIP;
    }
    return WF_OK;
}

// ---- device side

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // (lane 0)
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// Steps 2 and 3 of the order: the lane sums s[0 .. NS) and lane counts c[0 .. NC) (c may be null where NC == 0) of the 256 lanes of a block
// -> row[0 .. n_sums) (bit patterns of the sums) and row[n_sums .. n_sums + NC) (the counts).  n_sums <= NS.  Every lane of the block calls
// it; it holds one barrier, behind which every earlier LDS update of the block has landed too.
template <int NS, int NC>
__device__ __forceinline__ void block_partial(const double (&s)[NS], const unsigned long long* c, int n_sums, unsigned long long* __restrict__ row) {
    __shared__ double red[kObsBlock / 64][NS];
    __shared__ unsigned long long redc[kObsBlock / 64][NC > 0 ? NC : 1];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double w = wave_sum(s[k]);
        if (lane == 0) red[wave][k] = w;
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const unsigned long long w = wave_sum(c[k]);
        if (lane == 0) redc[wave][k] = w;
    }
    __syncthreads();
    if (tid < n_sums) {
        double t = red[0][tid];
        for (int w = 1; w < kObsBlock / 64; ++w) t += red[w][tid];
        row[tid] = (unsigned long long)__double_as_longlong(t);
    } else if (NC > 0 && tid < n_sums + NC) {
        unsigned long long t = 0;
        for (int w = 0; w < kObsBlock / 64; ++w) t += redc[w][tid - n_sums];
        row[tid] = t;
    }
}

// Step 4 of the order, for the one-workgroup reduce kernels (256 threads, all of them call it): thread k gets column k of n_blocks rows of
// `words` <= MAXW words, the first n_sums of them sums: .sum for k < n_sums, .count for n_sums <= k < words.  The caller adds it to its
// accumulator.
struct Column {
    double sum;
    unsigned long long count;
};
template <int MAXW>
__device__ __forceinline__ Column reduce_columns(const unsigned long long* __restrict__ partial, int n_blocks, int words, int n_sums) {
    __shared__ unsigned long long stage[kAccumStageRows * MAXW];
    const int k = threadIdx.x;
    Column col{0.0, 0ull};
    for (int b0 = 0; b0 < n_blocks; b0 += kAccumStageRows) {
        const int rows = n_blocks - b0 < kAccumStageRows ? n_blocks - b0 : kAccumStageRows;
        // fetched by all 256 threads as plain 8-byte words: one thread walking 1024 rows in global memory pays a memory latency per row
        // (0.34 ms measured for 1024 blocks), the staged form pays four
        for (int i = k; i < rows * words; i += kObsBlock) stage[i] = partial[(int64_t)b0 * words + i];
        __syncthreads();
        if (k < n_sums) {
#pragma unroll 8
            for (int b = 0; b < rows; ++b) col.sum += __longlong_as_double((long long)stage[b * words + k]);
        } else if (k < words) {
#pragma unroll 8
            for (int b = 0; b < rows; ++b) col.count += stage[b * words + k];
        }
        __syncthreads();
    }
    return col;
}

// The histograms of a block, privatised in LDS as uint32: hist[D][nd] density, then [np] pair (at most 8 * 512 + 1024 counters = 20 KB),
// updated with LDS integer atomics; hist_flush sends the non-zero bins to the caller's uint64 arrays, one 64-bit integer atomic add each.
__device__ __forceinline__ void hist_clear(unsigned int* hist, int n) {
    for (int i = threadIdx.x; i < n; i += kObsBlock) hist[i] = 0u;
    __syncthreads();
}
// one walker by the fp32 rule of include/waveflow_observe.h: every column into its density histogram, every pair j < i into the pair
// histogram; what falls outside [0, bins) is counted in out_d / out_p and enters no bin
template <int D>
__device__ __forceinline__ void hist_add(const float (&x)[D], const HistGeom& g, unsigned int* hist, unsigned long long& out_d, unsigned long long& out_p) {
    unsigned int* hpair = hist + D * g.nd;
    const float nd_f = (float)g.nd, np_f = (float)g.np;
    if (g.nd > 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float t = __fmul_rn(__fsub_rn(x[d], g.lo), g.scale_d);
            if (t >= 0.0f && t < nd_f)
                atomicAdd(&hist[d * g.nd + (int)t], 1u);
            else
                out_d += 1;
        }
    }
    if (g.np > 0) {
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < i; ++j) {
                const float t = __fmul_rn(fabsf(__fsub_rn(x[i], x[j])), g.scale_p);
                if (t >= 0.0f && t < np_f)
                    atomicAdd(&hpair[(int)t], 1u);
                else
                    out_p += 1;
            }
    }
}
// (behind a barrier that follows the block's last hist_add: the one of block_partial)
template <int D>
__device__ __forceinline__ void hist_flush(const unsigned int* hist, const HistGeom& g, unsigned long long* __restrict__ density,
                                           unsigned long long* __restrict__ pair) {
    const unsigned int* hpair = hist + D * g.nd;
    for (int i = threadIdx.x; i < D * g.nd; i += kObsBlock) {
        const unsigned int n = hist[i];
        if (n) atomicAdd(&density[i], (unsigned long long)n);
    }
    for (int i = threadIdx.x; i < g.np; i += kObsBlock) {
        const unsigned int n = hpair[i];
        if (n) atomicAdd(&pair[i], (unsigned long long)n);
    }
}

}  // namespace wf
