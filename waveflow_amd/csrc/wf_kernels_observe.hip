// wf_kernels_observe.hip -- observables of a trained psi (include/waveflow_observe.h): the five per-walker values (fp32, one rounding per
// operation, spelled with the _rn intrinsics where an expression could fuse), their fp64 moments and the integer histograms of the one-body
// density and the pair distance.
//
// k_observe: one lane per walker in 256-lane workgroups, a grid-stride loop over a grid that depends on B alone (observe_blocks).  Histograms
// are privatised in LDS as uint32 ((D n_density_bins + n_pair_bins) counters, at most 8 * 512 + 1024 = 20 KB) and updated with LDS integer
// atomics; at the end of the block only the non-zero bins go to the caller's uint64 arrays, one 64-bit integer atomic add each.  (A block
// sees at most ceil(B / 1024) walkers (rounded up to its 256 lanes) of at most 28 pairs each: with B <= kObsMaxWalkers = 2^36, which the
// entries enforce, a uint32 counter receives at most 2^26 * 28 < 2^31 increments.)  The fp64
// sums: each lane adds its walkers in index order, a fixed shuffle tree per wave, the four waves in order through LDS, one partial per block
// in the workspace.  k_observe_reduce (one workgroup, one thread per column) adds the partials in block order and then adds them to the accumulator.
// No floating-point atomics anywhere.  (tests/test_gpu_observables.py restates this order in numpy, `_ordered_sum`, and holds the device's sums
// to it bit for bit: a change of the order here is a change there.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wf_eloc.h"
#include "wf_observe.h"

namespace wf {

namespace {

struct ObsGeom {
    int nd, np;                 // bins (0: no such histogram)
    float lo, scale_d, scale_p;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;   // (lane 0)
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <int D>
__global__ __launch_bounds__(kObsBlock) void k_observe(const float* __restrict__ xg, const float* __restrict__ psi, const float* __restrict__ grad,
                                                       const float* __restrict__ hdiag, int64_t B, const Protons pr, const ObsGeom g, int has_acc,
                                                       float* __restrict__ values, unsigned long long* __restrict__ partial,
                                                       unsigned long long* __restrict__ density, unsigned long long* __restrict__ pair) {
    extern __shared__ unsigned int hist[];   // [D][nd] density, then [np] pair
    __shared__ double red[kObsBlock / 64][10];
    __shared__ unsigned long long redc[kObsBlock / 64][4];
    const int tid = threadIdx.x;
    const int n_hist = has_acc ? D * g.nd + g.np : 0;
    for (int i = tid; i < n_hist; i += kObsBlock) hist[i] = 0u;
    __syncthreads();
    unsigned int* hpair = hist + D * g.nd;
    double s[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) s[k] = 0.0;
    unsigned long long n_ok = 0, n_skip = 0, out_d = 0, out_p = 0;
    const float nd_f = (float)g.nd, np_f = (float)g.np;
    for (int64_t b = (int64_t)blockIdx.x * kObsBlock + tid; b < B; b += (int64_t)gridDim.x * kObsBlock) {
        float x[D];
        bool fin = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            x[d] = xg[b * D + d];
            fin = fin && isfinite(x[d]);
        }
        const float ps = psi[b];
        fin = fin && isfinite(ps);
        float gr[D], hd[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            gr[d] = grad[b * D + d];
            hd[d] = hdiag[b * D + d];
            fin = fin && isfinite(gr[d]) && isfinite(hd[d]);
        }
        float v[WF_OBSERVE_SCALARS];
        local_values<D>(x, ps, gr, hd, pr, v);   // the rule of the header (wf_eloc.h)
#pragma unroll
        for (int k = 0; k < WF_OBSERVE_SCALARS; ++k) {
            fin = fin && isfinite(v[k]);
            if (values) values[b * WF_OBSERVE_SCALARS + k] = v[k];
        }
        if (!has_acc) continue;
        if (!fin) {
            n_skip += 1;
            continue;
        }
        n_ok += 1;
#pragma unroll
        for (int k = 0; k < WF_OBSERVE_SCALARS; ++k) {
            const double vk = (double)v[k];
            s[2 * k] += vk;
            s[2 * k + 1] += vk * vk;
        }
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
    if (!has_acc) return;   // (uniform)
    // the block's partial: lanes -> wave (fixed tree) -> waves in order
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        const double w = wave_sum(s[k]);
        if (lane == 0) red[wave][k] = w;
    }
    unsigned long long c[4] = {n_ok, n_skip, out_d, out_p};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned long long w = wave_sum(c[k]);
        if (lane == 0) redc[wave][k] = w;
    }
    __syncthreads();   // (also: every LDS histogram update of the block has landed)
    if (tid < kObsPartial) {
        unsigned long long* row = partial + (int64_t)blockIdx.x * kObsPartial;   // 8-byte words: the sums as their bit patterns, then the counts
        if (tid < 10) {
            double t = red[0][tid];
            for (int w = 1; w < kObsBlock / 64; ++w) t += red[w][tid];
            row[tid] = (unsigned long long)__double_as_longlong(t);
        } else {
            unsigned long long t = 0;
            for (int w = 0; w < kObsBlock / 64; ++w) t += redc[w][tid - 10];
            row[tid] = t;
        }
    }
    // non-zero bins -> the caller's 64-bit histograms
    for (int i = tid; i < D * g.nd; i += kObsBlock) {
        const unsigned int n = hist[i];
        if (n) atomicAdd(&density[i], (unsigned long long)n);
    }
    for (int i = tid; i < g.np; i += kObsBlock) {
        const unsigned int n = hpair[i];
        if (n) atomicAdd(&pair[i], (unsigned long long)n);
    }
}

// One workgroup: thread k < 14 adds column k of the block partials in block order, then adds it to the accumulator; the step's counter + 1.
// The partials pass through LDS, 256 rows (28 KB) at a time, fetched by all 256 threads as plain 8-byte words: one thread walking 1024 rows
// in global memory pays a memory latency per row (0.34 ms measured for 1024 blocks), the staged form pays four.
constexpr int kObsReduceRows = 256;
__global__ __launch_bounds__(kObsBlock) void k_observe_reduce(const unsigned long long* __restrict__ partial, int n_blocks, double* __restrict__ sums,
                                                              unsigned long long* __restrict__ counts, unsigned long long* __restrict__ counter) {
    __shared__ unsigned long long stage[kObsReduceRows * kObsPartial];
    const int k = threadIdx.x;
    double t = 0.0;
    unsigned long long c = 0;
    for (int b0 = 0; b0 < n_blocks; b0 += kObsReduceRows) {
        const int rows = n_blocks - b0 < kObsReduceRows ? n_blocks - b0 : kObsReduceRows;
        for (int i = k; i < rows * kObsPartial; i += kObsBlock) stage[i] = partial[(int64_t)b0 * kObsPartial + i];
        __syncthreads();
        if (k < 10) {
#pragma unroll 8
            for (int b = 0; b < rows; ++b) t += __longlong_as_double((long long)stage[b * kObsPartial + k]);
        } else if (k < kObsPartial) {
#pragma unroll 8
            for (int b = 0; b < rows; ++b) c += stage[b * kObsPartial + k];
        }
        __syncthreads();
    }
    if (n_blocks > 0) {
        if (k < 10)
            sums[k] += t;
        else if (k < kObsPartial)
            counts[k - 10] += c;
    }
    if (counter && k == 0) counter[0] += 1ull;
}

template <int D>
void launch_k_observe(int64_t blocks, size_t lds, hipStream_t s, const float* x, const float* psi, const float* grad, const float* hdiag, int64_t B,
                      const Protons& pr, const ObsGeom& g, int has_acc, float* values, unsigned long long* partial, unsigned long long* density,
                      unsigned long long* pair) {
    hipLaunchKernelGGL(k_observe<D>, dim3((unsigned)blocks), dim3(kObsBlock), lds, s, x, psi, grad, hdiag, B, pr, g, has_acc, values, partial, density, pair);
}

int finish() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error((int)e);
        return WF_ERR_HIP;
    }
    return WF_OK;
}

}  // namespace

int observe_check_acc(const wf_observe_acc* acc) {
    if (!acc->sums_dev || !acc->counts_dev || acc->n_density_bins < 0 || acc->n_pair_bins < 0) return WF_ERR_INVALID;
    if (acc->n_density_bins > kObsMaxDensityBins || acc->n_pair_bins > kObsMaxPairBins) return WF_ERR_UNSUPPORTED;
    if ((acc->n_density_bins > 0 && !acc->density_dev) || (acc->n_pair_bins > 0 && !acc->pair_dev)) return WF_ERR_INVALID;
    if (!std::isfinite(acc->lo) || !std::isfinite(acc->hi) || !(acc->lo < acc->hi) || !std::isfinite(acc->hi - acc->lo)) return WF_ERR_INVALID;
    return WF_OK;
}

int launch_observe(const float* x, const float* psi, const float* grad, const float* hdiag, int64_t B, int D, const Protons& pr,
                   const wf_observe_acc* acc, float* values, void* ws, unsigned long long* counter, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ObsGeom g{};
    if (acc) {
        g.nd = acc->n_density_bins;
        g.np = acc->n_pair_bins;
        g.lo = acc->lo;
        const float width = acc->hi - acc->lo;
        g.scale_d = (float)g.nd / width;
        g.scale_p = (float)g.np / width;
    }
    const int64_t blocks = observe_blocks(B);
    const size_t lds = acc ? ((size_t)D * g.nd + g.np) * sizeof(unsigned int) : 0;
    unsigned long long* partial = (unsigned long long*)ws;
    unsigned long long* density = acc ? (unsigned long long*)acc->density_dev : nullptr;
    unsigned long long* pair = acc ? (unsigned long long*)acc->pair_dev : nullptr;
#define WF_OBS_CASE(DD)                                                                                                              \
    case DD:                                                                                                                         \
        launch_k_observe<DD>(blocks, lds, s, x, psi, grad, hdiag, B, pr, g, acc ? 1 : 0, values, partial, density, pair);             \
        break;
    switch (D) {
        WF_OBS_CASE(2)
        WF_OBS_CASE(3)
        WF_OBS_CASE(4)
        WF_OBS_CASE(5)
        WF_OBS_CASE(6)
        WF_OBS_CASE(7)
        WF_OBS_CASE(8)
        default:
            return WF_ERR_INVALID;
    }
#undef WF_OBS_CASE
    if (acc || counter)
        hipLaunchKernelGGL(k_observe_reduce, dim3(1), dim3(kObsBlock), 0, s, partial, acc ? (int)blocks : 0, acc ? acc->sums_dev : nullptr,
                           acc ? (unsigned long long*)acc->counts_dev : nullptr, counter);
    return finish();
}

}  // namespace wf

extern "C" {

int64_t wf_observe_workspace_bytes(int64_t B) {
    if (B < 0) return WF_ERR_INVALID;
    if (B > wf::kObsMaxWalkers) return WF_ERR_UNSUPPORTED;
    return wf::observe_ws_bytes(B);
}

int wf_observe_accumulate(const float* x_dev, const float* psi_dev, const float* grad_dev, const float* hdiag_dev, int64_t B, int32_t n_dim,
                          const float* protons_host, int32_t n_protons, const wf_observe_acc* acc, float* values_dev,
                          void* workspace_dev, int64_t workspace_bytes, void* stream) {
    using namespace wf;
    Protons pr{};
    if (B < 0 || n_dim < 2 || n_dim > 8 || n_protons < 0 || n_protons > 8 || (n_protons > 0 && !protons_host)) return WF_ERR_INVALID;
    if (acc) {
        const int rc = observe_check_acc(acc);
        if (rc) return rc;
    }
    if (B == 0) return WF_OK;
    if (B > kObsMaxWalkers) return WF_ERR_UNSUPPORTED;
    if (!x_dev || !psi_dev || !grad_dev || !hdiag_dev || (!acc && !values_dev)) return WF_ERR_INVALID;
    if (acc && (!workspace_dev || workspace_bytes < observe_ws_bytes(B))) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    pr.n = n_protons;
    for (int i = 0; i < n_protons; ++i) pr.pos[i] = protons_host[i];
    return launch_observe(x_dev, psi_dev, grad_dev, hdiag_dev, B, n_dim, pr, acc, values_dev, workspace_dev, nullptr, stream);
}

}  // extern "C"
