// wf_kernels_overlap.hip -- overlaps between wavefunctions (include/waveflow_overlap.h): the ratios r_k = psi_k / (psi + 1e-8) of up to 8
// reference rows on the walkers of psi (fp32, one rounding per operation, spelled with the _rn intrinsics), their fp64 moments, and the
// overlap-penalised local energies.
//
// k_overlap: one lane per walker in 256-lane workgroups, a grid-stride loop over observe_blocks(B) blocks.  Memory-streaming: psi is read
// once, the K reference rows coalesced (lane = walker), a runtime loop over K.  The fp64 sums are formed in the one order of the project
// (wf_accum.h): block partials in the workspace, k_overlap_reduce (one workgroup, one thread per column) adds them in block order and then
// adds them to the accumulator.  (tests/test_gpu_overlap.py holds the sums to overlap.reference_accumulate, which restates that order.)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wf_overlap.h"

namespace wf {

namespace {

constexpr int kMaxK = WF_OVERLAP_MAX_REFS;
constexpr int kMaxWords = 2 * kMaxK + 2;

struct Lambdas {
    double v[kMaxK];
};

__global__ __launch_bounds__(kObsBlock) void k_overlap(const float* __restrict__ psi, const float* __restrict__ ref, int64_t ld, int64_t B, int K,
                                                       int has_acc, float* __restrict__ ratios, unsigned long long* __restrict__ partial) {
    const int tid = threadIdx.x;
    double s[2 * kMaxK];
#pragma unroll
    for (int k = 0; k < 2 * kMaxK; ++k) s[k] = 0.0;
    unsigned long long n_ok = 0, n_skip = 0;
    for (int64_t b = (int64_t)blockIdx.x * kObsBlock + tid; b < B; b += (int64_t)gridDim.x * kObsBlock) {
        const float ps = psi[b];
        const float inv = __fdiv_rn(1.0f, __fadd_rn(ps, 1e-8f));
        bool fin = isfinite(ps);
        float r[kMaxK];
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            r[k] = 0.0f;
            if (k < K) {
                const float rf = ref[(int64_t)k * ld + b];
                r[k] = __fmul_rn(rf, inv);
                fin = fin && isfinite(rf) && isfinite(r[k]);
                if (ratios) ratios[(int64_t)k * ld + b] = r[k];
            }
        }
        if (!has_acc) continue;
        if (!fin) {
            n_skip += 1;
            continue;
        }
        n_ok += 1;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k < K) {
                const double rk = (double)r[k];
                s[2 * k] += rk;
                s[2 * k + 1] += rk * rk;
            }
        }
    }
    if (!has_acc) return;   // (uniform)
    const unsigned long long c[2] = {n_ok, n_skip};
    block_partial<2 * kMaxK, 2>(s, c, 2 * K, partial + (int64_t)blockIdx.x * overlap_partial_words(K));
}

// One workgroup: thread c < 2 K + 2 gets column c of the block partials (reduce_columns) and adds it to the accumulator; the step's counter + 1.
__global__ __launch_bounds__(kObsBlock) void k_overlap_reduce(const unsigned long long* __restrict__ partial, int n_blocks, int K, double* __restrict__ sums,
                                                              unsigned long long* __restrict__ counts, unsigned long long* __restrict__ counter) {
    const int c = threadIdx.x;
    const int words = overlap_partial_words(K);
    const Column col = reduce_columns<kMaxWords>(partial, n_blocks, words, 2 * K);
    if (n_blocks > 0) {
        if (c < 2 * K)
            sums[c] += col.sum;
        else if (c < words)
            counts[c - 2 * K] += col.count;
    }
    if (counter && c == 0) counter[0] += 1ull;
}

// e and out may be one array: each lane reads e[b] before it writes out[b], and no other lane touches that element
__global__ __launch_bounds__(kObsBlock) void k_overlap_penalise(const float* e, const float* __restrict__ ratios, int64_t ld, int64_t B, int K, const Lambdas lam,
                                                                const double* __restrict__ sums, const unsigned long long* __restrict__ counts, float* out) {
    const unsigned long long n = counts[0];
    double a[kMaxK], la[kMaxK];
#pragma unroll
    for (int k = 0; k < kMaxK; ++k) {
        a[k] = (k < K && n > 0) ? sums[2 * k] / (double)n : 0.0;
        la[k] = lam.v[k] * a[k];
    }
    for (int64_t b = (int64_t)blockIdx.x * kObsBlock + threadIdx.x; b < B; b += (int64_t)gridDim.x * kObsBlock) {
        const float eb = e[b];
        double sum = (double)eb;
        bool fin = n > 0;
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) {
            if (k < K) {
                const float r = ratios[(int64_t)k * ld + b];
                fin = fin && isfinite(r);
                sum = sum + la[k] * ((double)r - a[k]);
            }
        }
        out[b] = fin ? (float)sum : eb;
    }
}

}  // namespace

int launch_overlap(const float* psi, const float* ref, int64_t ld, int64_t B, int K, const wf_overlap_acc* acc, float* ratios, void* ws,
                   unsigned long long* counter, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = observe_blocks(B);
    unsigned long long* partial = (unsigned long long*)ws;
    hipLaunchKernelGGL(k_overlap, dim3((unsigned)blocks), dim3(kObsBlock), 0, s, psi, ref, ld, B, K, acc ? 1 : 0, ratios, partial);
    if (acc || counter)
        hipLaunchKernelGGL(k_overlap_reduce, dim3(1), dim3(kObsBlock), 0, s, partial, acc ? (int)blocks : 0, K, acc ? acc->sums_dev : nullptr,
                           acc ? (unsigned long long*)acc->counts_dev : nullptr, counter);
    return launch_status();
}

}  // namespace wf

extern "C" {

int64_t wf_overlap_workspace_bytes(int64_t B, int32_t K) {
    if (B < 0 || K < 1) return WF_ERR_INVALID;
    if (K > WF_OVERLAP_MAX_REFS) return WF_ERR_UNSUPPORTED;
    return wf::overlap_ws_bytes(B, K);
}

int wf_overlap_accumulate(const float* psi_dev, const float* ref_dev, int64_t ld, int64_t B, int32_t K, const wf_overlap_acc* acc,
                          float* ratios_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    using namespace wf;
    if (B < 0 || K < 1 || ld < B) return WF_ERR_INVALID;
    if (K > WF_OVERLAP_MAX_REFS) return WF_ERR_UNSUPPORTED;
    if (acc) {
        const int rc = overlap_check_acc(acc);
        if (rc) return rc;
    }
    if (B == 0) return WF_OK;
    if (!psi_dev || !ref_dev || (!acc && !ratios_dev)) return WF_ERR_INVALID;
    if (acc && (!workspace_dev || workspace_bytes < overlap_ws_bytes(B, K))) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return launch_overlap(psi_dev, ref_dev, ld, B, K, acc, ratios_dev, workspace_dev, nullptr, stream);
}

int wf_overlap_penalise(const float* e_dev, const float* ratios_dev, int64_t ld, int64_t B, int32_t K, const float* lambda_host,
                        const wf_overlap_acc* acc, float* out_dev, void* stream) {
    using namespace wf;
    if (B < 0 || K < 1 || ld < B) return WF_ERR_INVALID;
    if (K > WF_OVERLAP_MAX_REFS) return WF_ERR_UNSUPPORTED;
    if (!lambda_host || !acc || overlap_check_acc(acc) != WF_OK) return WF_ERR_INVALID;
    Lambdas lam{};
    for (int k = 0; k < K; ++k) {
        if (!std::isfinite(lambda_host[k]) || lambda_host[k] < 0.0f) return WF_ERR_INVALID;
        lam.v[k] = (double)lambda_host[k];
    }
    if (B == 0) return WF_OK;
    if (!e_dev || !ratios_dev || !out_dev) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    hipLaunchKernelGGL(k_overlap_penalise, dim3((unsigned)observe_blocks(B)), dim3(kObsBlock), 0, (hipStream_t)stream, e_dev, ratios_dev, ld, B, (int)K, lam,
                       acc->sums_dev, (const unsigned long long*)acc->counts_dev, out_dev);
    return launch_status();
}

}  // extern "C"
