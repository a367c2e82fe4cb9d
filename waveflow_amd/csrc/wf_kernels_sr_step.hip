// wf_kernels_sr_step.hip -- the glue kernels of the stochastic-reconfiguration step, plain and SPRING (wf_train_sr.cpp; include/waveflow_sr_step.h,
// include/waveflow_sr_spring.h), between the entries it is made of:
//     inv, e_loc                                       k_sr_eloc         elementwise, ahead of the rows where the right-hand side has to wait for q = O phi
//     rhs = H (clamp(e) - (mu / 2) q)                  k_sr_rhs          one workgroup: median by a bitonic sort in LDS, mean absolute deviation, clamp, centring
//     eff = min(lr, sqrt(C / |d|^2)), theta, phi       k_sr_verdict / k_sr_update
// With mu = 0, clip = 0, C = 0 and no phi these are the plain step: rhs = e - mean(e), eff = lr, theta alone is updated.
// No floating-point atomics; every sum has one order that depends on its length alone.  The fp32 arithmetic is spelled with the _rn intrinsics:
// one rounding per operation, the values an elementwise fp32 expression gives (1 / (psi + 1e-8), hpsi * inv, theta - lr * d), never a fused
// multiply-add.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/waveflow_sr_spring.h"
#include "wf_internal.h"
#include "wf_sr_common.h"

namespace wf {

namespace {

constexpr int kStepBlock = 256;
constexpr int kNormBlock = 1024;   // |d|^2 over tens of thousands of parameters in one block: the widest one
constexpr int kMaxSort = 4096;     // walkers of one step (wf_sr_solve): 16 KiB of LDS

}  // namespace

// inv = 1 / (psi + 1e-8), e_loc = hpsi inv: the values of k_sr_rhs, ahead of the rows (which need inv)
__global__ __launch_bounds__(kStepBlock) void k_sr_eloc(const float* __restrict__ hpsi, const float* __restrict__ psi, int64_t B, float* __restrict__ e_loc,
                                                        float* __restrict__ inv) {
    const int64_t i = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (i >= B) return;
    const float iv = __fdiv_rn(1.0f, __fadd_rn(psi[i], 1e-8f));
    inv[i] = iv;
    e_loc[i] = __fmul_rn(hpsi[i], iv);
}

// One block, B <= 4096: inv and e_loc, then rhs = r - mean(r) with r_b = clamp(e_b, c - k w, c + k w) - (mu / 2) q_b in fp64.
// c: median of the fp32 e_b (bitonic sort in LDS, padded to a power of two with +inf, non-finite values last; even B: the mean of the two
// middle values in fp64); w = (1 / B) sum |e_b - c|.  Every sum: thread t adds walkers t, t + 256, ... in that order, then the tree.
// clip == 0: no sort, r_b = e_b exactly; mu == 0: q is not read.  stats[4] = [c, w, c - k w, c + k w] (zeros when clip == 0).
__global__ __launch_bounds__(kStepBlock) void k_sr_rhs(const float* __restrict__ hpsi, const float* __restrict__ psi, int64_t B, const double* __restrict__ q,
                                                       double mu, double clip, float* __restrict__ e_loc, float* __restrict__ inv, double* __restrict__ rhs,
                                                       double* __restrict__ stats) {
    __shared__ double red[kStepBlock];
    __shared__ float key[kMaxSort];
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < B; i += kStepBlock) {
        const float iv = __fdiv_rn(1.0f, __fadd_rn(psi[i], 1e-8f));
        inv[i] = iv;
        e_loc[i] = __fmul_rn(hpsi[i], iv);
    }
    double lo = 0.0, hi = 0.0, c = 0.0, w = 0.0;
    if (clip > 0.0) {   // (uniform)
        int n = 1;
        while (n < (int)B) n <<= 1;
        for (int i = tid; i < n; i += kStepBlock) {
            const float e = i < (int)B ? e_loc[i] : INFINITY;   // (the thread's own stores)
            key[i] = isfinite(e) ? e : INFINITY;
        }
        __syncthreads();
        for (int k = 2; k <= n; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n; i += kStepBlock) {
                    const int l = i ^ j;
                    if (l > i) {
                        const float a = key[i], b = key[l];
                        const bool up = (i & k) == 0;
                        if (up ? a > b : a < b) {
                            key[i] = b;
                            key[l] = a;
                        }
                    }
                }
                __syncthreads();
            }
        }
        c = (B & 1) ? (double)key[B / 2] : 0.5 * ((double)key[B / 2 - 1] + (double)key[B / 2]);
        double s = 0.0;
        for (int64_t i = tid; i < B; i += kStepBlock) s += fabs((double)e_loc[i] - c);
        w = sr_block_sum<kStepBlock>(s, red) / (double)B;
        lo = c - clip * w;
        hi = c + clip * w;
    }
    if (tid == 0 && stats) {
        stats[0] = c;
        stats[1] = w;
        stats[2] = lo;
        stats[3] = hi;
    }
    double s = 0.0;
    for (int64_t i = tid; i < B; i += kStepBlock) {
        double r = (double)e_loc[i];
        if (clip > 0.0) r = r < lo ? lo : (r > hi ? hi : r);
        if (mu != 0.0) r = r - (0.5 * mu) * q[i];
        rhs[i] = r;
        s += r;
    }
    s = sr_block_sum<kStepBlock>(s, red);
    const double mean = s / (double)B;
    for (int64_t i = tid; i < B; i += kStepBlock) rhs[i] = rhs[i] - mean;   // (the thread's own stores)
}

// one block: |d|^2 in fp64 (thread t sums entries t, t + 1024, ... in that order, then the tree), what the step does with d -- update iff the
// solver's info is 0 and |d|^2 is finite -- and the step size: eff = fl32(lr) when cap == 0 or |d|^2 == 0, else fl32(min(lr, sqrt(cap / |d|^2)));
// eff_dev[0] = eff and eff_ring[slot] = eff for a step that updates, 0 for a skipped one
__global__ __launch_bounds__(kNormBlock) void k_sr_verdict(const float* __restrict__ d, int64_t P, const int32_t* __restrict__ info, int32_t* __restrict__ status,
                                                           int32_t* __restrict__ flag, double* __restrict__ norm_ring, double* __restrict__ eff_ring, int ring_len,
                                                           const unsigned long long* __restrict__ counter, const float* __restrict__ step_size, double cap,
                                                           float* __restrict__ eff_dev) {
    __shared__ double red[kNormBlock];
    double s = 0.0;
    for (int64_t p = threadIdx.x; p < P; p += kNormBlock) {
        const double v = (double)d[p];
        s += v * v;
    }
    s = sr_block_sum<kNormBlock>(s, red);
    if (threadIdx.x != 0) return;
    const int32_t pivot = info[0];
    const bool ok = pivot == 0 && isfinite(s);
    flag[0] = ok ? 1 : 0;
    status[0] = ok ? 0 : (pivot != 0 ? pivot : -1);
    if (!ok) status[1] += 1;
    const double lr = (double)step_size[0];
    double eff64 = lr;
    if (cap != 0.0 && s != 0.0) eff64 = fmin(lr, sqrt(cap / s));
    const float eff = ok ? (float)eff64 : 0.0f;
    eff_dev[0] = eff;
    const unsigned long long slot = counter[0] % (unsigned long long)ring_len;
    if (norm_ring) norm_ring[slot] = s;
    if (eff_ring) eff_ring[slot] = (double)eff;
}

// theta <- fl32(theta - fl32(eff d)) and, where there is a phi, phi <- d, where the verdict allows it; neither is touched otherwise
__global__ __launch_bounds__(kStepBlock) void k_sr_update(float* __restrict__ params, float* __restrict__ phi, const float* __restrict__ d, int64_t P,
                                                          const float* __restrict__ eff, const int32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (p >= P || flag[0] == 0) return;
    const float dp = d[p];
    params[p] = __fsub_rn(params[p], __fmul_rn(eff[0], dp));
    if (phi) phi[p] = dp;   // (uniform)
}

int launch_sr_eloc(const float* hpsi, const float* psi, int64_t B, float* e_loc, float* inv, void* stream) {
    hipLaunchKernelGGL(k_sr_eloc, dim3((unsigned)((B + kStepBlock - 1) / kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, hpsi, psi, B, e_loc, inv);
    return sr_finish();
}

int launch_sr_rhs(const float* hpsi, const float* psi, int64_t B, const double* q, double mu, double clip, float* e_loc, float* inv, double* rhs,
                  double* stats, void* stream) {
    if (B < 1 || B > kMaxSort) return WF_ERR_INVALID;
    hipLaunchKernelGGL(k_sr_rhs, dim3(1), dim3(kStepBlock), 0, (hipStream_t)stream, hpsi, psi, B, q, mu, clip, e_loc, inv, rhs, stats);
    return sr_finish();
}

int launch_sr_verdict(const float* d, int64_t P, const int32_t* info, int32_t* status, int32_t* flag, double* norm_ring, double* eff_ring, int ring_len,
                      const unsigned long long* counter, const float* step_size, double cap, float* eff, void* stream) {
    hipLaunchKernelGGL(k_sr_verdict, dim3(1), dim3(kNormBlock), 0, (hipStream_t)stream, d, P, info, status, flag, norm_ring, eff_ring, ring_len, counter, step_size,
                       cap, eff);
    return sr_finish();
}

int launch_sr_update(float* params, float* phi, const float* d, int64_t P, const float* eff, const int32_t* flag, void* stream) {
    hipLaunchKernelGGL(k_sr_update, dim3((unsigned)((P + kStepBlock - 1) / kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, params, phi, d, P, eff, flag);
    return sr_finish();
}

}  // namespace wf

using namespace wf;

extern "C" {

int wf_spring_rhs(const float* hpsi_dev, const float* psi_dev, int64_t B, const double* q_dev, double mu, double clip, float* e_loc_dev, float* inv_dev,
                  double* rhs_dev, double* stats_dev, void* stream) {
    if (B < 1 || !hpsi_dev || !psi_dev || !e_loc_dev || !inv_dev || !rhs_dev) return WF_ERR_INVALID;
    if (!(mu >= 0.0) || !(mu < 1.0) || !(clip >= 0.0) || (mu != 0.0 && !q_dev)) return WF_ERR_INVALID;
    if (B > kMaxSort) return WF_ERR_UNSUPPORTED;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return launch_sr_rhs(hpsi_dev, psi_dev, B, q_dev, mu, clip, e_loc_dev, inv_dev, rhs_dev, stats_dev, stream);
}

}  // extern "C"
