// wf_kernels_sr_step.hip -- the glue kernels of wf_vqmc_sr_step (include/waveflow_sr_step.h) between the entries it is made of: local energies
// and the centred right-hand side, |d|^2 with the step's verdict, the guarded parameter update.  No floating-point atomics; every sum has one
// order that depends on its length alone.  The fp32 arithmetic is spelled with the _rn intrinsics: one rounding per operation, the values an
// elementwise fp32 expression gives (1 / (psi + 1e-8), hpsi * inv, theta - lr * d), never a fused multiply-add.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wf_internal.h"
#include "wf_sr_common.h"

namespace wf {

namespace {

constexpr int kStepBlock = 256;
constexpr int kNormBlock = 1024;   // |d|^2 over tens of thousands of parameters in one block: the widest one

}  // namespace

// one block: inv, e_loc, then rhs = e_loc - mean(e_loc) in fp64 (thread t sums walkers t, t + 256, ... in that order, then the tree)
__global__ __launch_bounds__(kStepBlock) void k_sr_eloc_rhs(const float* __restrict__ hpsi, const float* __restrict__ psi, int64_t B, float* __restrict__ e_loc,
                                                            float* __restrict__ inv, double* __restrict__ rhs) {
    __shared__ double red[kStepBlock];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += kStepBlock) {
        const float iv = __fdiv_rn(1.0f, __fadd_rn(psi[i], 1e-8f));
        const float el = __fmul_rn(hpsi[i], iv);
        inv[i] = iv;
        e_loc[i] = el;
        s += (double)el;
    }
    s = sr_block_sum<kStepBlock>(s, red);
    const double mean = s / (double)B;
    for (int64_t i = threadIdx.x; i < B; i += kStepBlock) rhs[i] = (double)e_loc[i] - mean;   // (the thread's own stores)
}

// one block: |d|^2 in fp64 (thread t sums entries t, t + 1024, ... in that order, then the tree) and what the step does with d
__global__ __launch_bounds__(kNormBlock) void k_sr_verdict(const float* __restrict__ d, int64_t P, const int32_t* __restrict__ info, int32_t* __restrict__ status,
                                                           int32_t* __restrict__ flag, double* __restrict__ norm_ring, int ring_len,
                                                           const unsigned long long* __restrict__ counter) {
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
    if (norm_ring) norm_ring[counter[0] % (unsigned long long)ring_len] = s;
}

// theta <- fl32(theta - fl32(lr d)) where the verdict allows it; the parameters are not touched otherwise
__global__ __launch_bounds__(kStepBlock) void k_sr_update(float* __restrict__ params, const float* __restrict__ d, int64_t P, const float* __restrict__ step_size,
                                                          const int32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * kStepBlock + threadIdx.x;
    if (p >= P || flag[0] == 0) return;
    params[p] = __fsub_rn(params[p], __fmul_rn(step_size[0], d[p]));
}

int launch_sr_eloc_rhs(const float* hpsi, const float* psi, int64_t B, float* e_loc, float* inv, double* rhs, void* stream) {
    hipLaunchKernelGGL(k_sr_eloc_rhs, dim3(1), dim3(kStepBlock), 0, (hipStream_t)stream, hpsi, psi, B, e_loc, inv, rhs);
    return sr_finish();
}

int launch_sr_verdict(const float* d, int64_t P, const int32_t* info, int32_t* status, int32_t* flag, double* norm_ring, int ring_len,
                      const unsigned long long* counter, void* stream) {
    hipLaunchKernelGGL(k_sr_verdict, dim3(1), dim3(kNormBlock), 0, (hipStream_t)stream, d, P, info, status, flag, norm_ring, ring_len, counter);
    return sr_finish();
}

int launch_sr_update(float* params, const float* d, int64_t P, const float* step_size, const int32_t* flag, void* stream) {
    hipLaunchKernelGGL(k_sr_update, dim3((unsigned)((P + kStepBlock - 1) / kStepBlock)), dim3(kStepBlock), 0, (hipStream_t)stream, params, d, P, step_size,
                       flag);
    return sr_finish();
}

}  // namespace wf
