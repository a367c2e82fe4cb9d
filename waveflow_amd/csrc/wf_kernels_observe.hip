// wf_kernels_observe.hip -- observables of a trained psi (include/waveflow_observe.h): the five per-walker values (fp32, one rounding per
// operation, spelled with the _rn intrinsics where an expression could fuse), their fp64 moments and the integer histograms of the one-body
// density and the pair distance.
//
// k_observe: one lane per walker in 256-lane workgroups, a grid-stride loop over a grid that depends on B alone (observe_blocks).  The
// histograms are privatised in LDS and the fp64 sums are formed in the one order of the project, both as wf_accum.h states them: the block
// partials go to the workspace, k_observe_reduce (one workgroup, one thread per column) adds them in block order and then adds them to the
// accumulator.  (A block sees at most ceil(B / 1024) walkers (rounded up to its 256 lanes) of at most 28 pairs each: with B <= kObsMaxWalkers =
// 2^36, which the entries enforce, a uint32 LDS counter receives at most 2^26 * 28 < 2^31 increments.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wf_eloc.h"
#include "wf_observe.h"

namespace wf {

namespace {

template <int D>
__global__ __launch_bounds__(kObsBlock) void k_observe(const float* __restrict__ xg, const float* __restrict__ psi, const float* __restrict__ grad,
                                                       const float* __restrict__ hdiag, int64_t B, const Protons pr, const HistGeom g, int has_acc,
                                                       float* __restrict__ values, unsigned long long* __restrict__ partial,
                                                       unsigned long long* __restrict__ density, unsigned long long* __restrict__ pair) {
    extern __shared__ unsigned int hist[];   // [D][nd] density, then [np] pair
    const int tid = threadIdx.x;
    hist_clear(hist, has_acc ? D * g.nd + g.np : 0);
    double s[kObsSums];
#pragma unroll
    for (int k = 0; k < kObsSums; ++k) s[k] = 0.0;
    unsigned long long n_ok = 0, n_skip = 0, out_d = 0, out_p = 0;
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
        hist_add<D>(x, g, hist, out_d, out_p);
    }
    if (!has_acc) return;   // (uniform)
    const unsigned long long c[kObsCounts] = {n_ok, n_skip, out_d, out_p};
    block_partial<kObsSums, kObsCounts>(s, c, kObsSums, partial + (int64_t)blockIdx.x * kObsPartial);
    hist_flush<D>(hist, g, density, pair);
}

// One workgroup: thread k < 14 gets column k of the block partials (reduce_columns) and adds it to the accumulator; the step's counter + 1.
__global__ __launch_bounds__(kObsBlock) void k_observe_reduce(const unsigned long long* __restrict__ partial, int n_blocks, double* __restrict__ sums,
                                                              unsigned long long* __restrict__ counts, unsigned long long* __restrict__ counter) {
    const int k = threadIdx.x;
    const Column col = reduce_columns<kObsPartial>(partial, n_blocks, kObsPartial, kObsSums);
    if (n_blocks > 0) {
        if (k < kObsSums)
            sums[k] += col.sum;
        else if (k < kObsPartial)
            counts[k - kObsSums] += col.count;
    }
    if (counter && k == 0) counter[0] += 1ull;
}

template <int D>
void launch_k_observe(int64_t blocks, size_t lds, hipStream_t s, const float* x, const float* psi, const float* grad, const float* hdiag, int64_t B,
                      const Protons& pr, const HistGeom& g, int has_acc, float* values, unsigned long long* partial, unsigned long long* density,
                      unsigned long long* pair) {
    hipLaunchKernelGGL(k_observe<D>, dim3((unsigned)blocks), dim3(kObsBlock), lds, s, x, psi, grad, hdiag, B, pr, g, has_acc, values, partial, density, pair);
}

}  // namespace

int observe_check_acc(const wf_observe_acc* acc) {
    if (!acc->sums_dev || !acc->counts_dev) return WF_ERR_INVALID;
    return hist_check(acc->n_density_bins, acc->n_pair_bins, acc->lo, acc->hi, acc->density_dev, acc->pair_dev);
}

int launch_observe(const float* x, const float* psi, const float* grad, const float* hdiag, int64_t B, int D, const Protons& pr,
                   const wf_observe_acc* acc, float* values, void* ws, unsigned long long* counter, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const HistGeom g = acc ? make_hist_geom(acc->n_density_bins, acc->n_pair_bins, acc->lo, acc->hi) : HistGeom{};
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
    return launch_status();
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
    if (B < 0 || n_dim < 2 || n_dim > 8 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (acc) {
        const int rc = observe_check_acc(acc);
        if (rc) return rc;
    }
    if (B == 0) return WF_OK;
    if (B > kObsMaxWalkers) return WF_ERR_UNSUPPORTED;
    if (!x_dev || !psi_dev || !grad_dev || !hdiag_dev || (!acc && !values_dev)) return WF_ERR_INVALID;
    if (acc && (!workspace_dev || workspace_bytes < observe_ws_bytes(B))) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return launch_observe(x_dev, psi_dev, grad_dev, hdiag_dev, B, n_dim, pr, acc, values_dev, workspace_dev, nullptr, stream);
}

}  // extern "C"
