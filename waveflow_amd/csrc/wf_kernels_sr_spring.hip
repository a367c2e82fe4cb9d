// wf_kernels_sr_spring.hip -- what the SPRING optimiser (include/waveflow_sr_spring.h) adds to stochastic reconfiguration:
//     q = O phi                                        wf_sr_matvec      one pass over the rows, fp64, one workgroup per row
//     d = mu phi + scale O^T (H y)                     wf_sr_apply_add   the slab pass of wf_sr_apply, then a reduce that adds mu phi before its one rounding
//     rhs = H (clamp(e) - (mu / 2) q)                  k_spring_rhs      one workgroup: median by a bitonic sort in LDS, mean absolute deviation, clamp, centring
//     eff = min(lr, sqrt(C / |d|^2)), theta, phi       k_spring_verdict / k_spring_update
// No floating-point atomics; every sum has one order that depends on its length alone.  The fp32 arithmetic of the step is spelled with the _rn
// intrinsics, as in wf_kernels_sr_step.hip, and gives its bits where momentum, cap and clip are off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/waveflow_sr_spring.h"
#include "wf_internal.h"
#include "wf_sr_common.h"

namespace wf {

namespace {

constexpr int kSpringBlock = 256;
constexpr int kSpringNormBlock = 1024;   // |d|^2 as k_sr_verdict sums it
constexpr int kSpringMaxSort = 4096;     // walkers of one step (wf_sr_solve): 16 KiB of LDS

}  // namespace

// q[b] = sum_p rows[b][p] v[p]: one workgroup per row; thread t takes columns 4 t .. 4 t + 3, then + 1024, ... into four fp64 sums (one per
// column of its group, every product exact in fp64), ((s0 + s1) + (s2 + s3)), then the tree over the 256 threads
__global__ __launch_bounds__(kSpringBlock) void k_sr_matvec(const float* __restrict__ rows, int64_t ld, int64_t B, int64_t P, int vec, const float* __restrict__ v,
                                                            int vvec, double* __restrict__ q) {
    __shared__ double red[kSpringBlock];
    const int64_t b = blockIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
    for (int64_t c = (int64_t)threadIdx.x * 4; c < P; c += 4 * kSpringBlock) {
        const float4 r = sr_load4(rows, ld, b, B, c, P, vec != 0);
        const float4 w = sr_load4(v, 0, 0, 1, c, P, vvec != 0);
        s0 += (double)r.x * (double)w.x;
        s1 += (double)r.y * (double)w.y;
        s2 += (double)r.z * (double)w.z;
        s3 += (double)r.w * (double)w.w;
    }
    const double s = sr_block_sum<kSpringBlock>((s0 + s1) + (s2 + s3), red);
    if (threadIdx.x == 0) q[b] = s;
}

// out[p] = (float)(mu prev[p] + scale * sum of the slab partials, slab 0 first); prev == nullptr or mu == 0: k_sr_apply_reduce.  out may be prev.
__global__ __launch_bounds__(256) void k_sr_apply_add_reduce(const double* __restrict__ partial, int64_t nslab, int64_t P, double scale, const float* prev, double mu,
                                                             float* out) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int64_t i = 0; i < nslab; ++i) s += partial[i * P + p];
    double v = scale * s;
    if (prev != nullptr && mu != 0.0) v = mu * (double)prev[p] + v;
    out[p] = (float)v;
}

// inv = 1 / (psi + 1e-8), e_loc = hpsi inv: the values of k_sr_eloc_rhs, ahead of the rows (which need inv)
__global__ __launch_bounds__(kSpringBlock) void k_spring_eloc(const float* __restrict__ hpsi, const float* __restrict__ psi, int64_t B, float* __restrict__ e_loc,
                                                              float* __restrict__ inv) {
    const int64_t i = (int64_t)blockIdx.x * kSpringBlock + threadIdx.x;
    if (i >= B) return;
    const float iv = __fdiv_rn(1.0f, __fadd_rn(psi[i], 1e-8f));
    inv[i] = iv;
    e_loc[i] = __fmul_rn(hpsi[i], iv);
}

// One block, B <= 4096: inv and e_loc as k_sr_eloc_rhs, then rhs = r - mean(r) with r_b = clamp(e_b, c - k w, c + k w) - (mu / 2) q_b in fp64.
// c: median of the fp32 e_b (bitonic sort in LDS, padded to a power of two with +inf, non-finite values last; even B: the mean of the two
// middle values in fp64); w = (1 / B) sum |e_b - c|.  Every sum: thread t adds walkers t, t + 256, ... in that order, then the tree.
// clip == 0: no sort, r_b = e_b exactly; mu == 0: q is not read.  stats[4] = [c, w, c - k w, c + k w] (zeros when clip == 0).
__global__ __launch_bounds__(kSpringBlock) void k_spring_rhs(const float* __restrict__ hpsi, const float* __restrict__ psi, int64_t B, const double* __restrict__ q,
                                                             double mu, double clip, float* __restrict__ e_loc, float* __restrict__ inv, double* __restrict__ rhs,
                                                             double* __restrict__ stats) {
    __shared__ double red[kSpringBlock];
    __shared__ float key[kSpringMaxSort];
    const int tid = threadIdx.x;
    for (int64_t i = tid; i < B; i += kSpringBlock) {
        const float iv = __fdiv_rn(1.0f, __fadd_rn(psi[i], 1e-8f));
        inv[i] = iv;
        e_loc[i] = __fmul_rn(hpsi[i], iv);
    }
    double lo = 0.0, hi = 0.0, c = 0.0, w = 0.0;
    if (clip > 0.0) {   // (uniform)
        int n = 1;
        while (n < (int)B) n <<= 1;
        for (int i = tid; i < n; i += kSpringBlock) {
            const float e = i < (int)B ? e_loc[i] : INFINITY;   // (the thread's own stores)
            key[i] = isfinite(e) ? e : INFINITY;
        }
        __syncthreads();
        for (int k = 2; k <= n; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int i = tid; i < n; i += kSpringBlock) {
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
        for (int64_t i = tid; i < B; i += kSpringBlock) s += fabs((double)e_loc[i] - c);
        w = sr_block_sum<kSpringBlock>(s, red) / (double)B;
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
    for (int64_t i = tid; i < B; i += kSpringBlock) {
        double r = (double)e_loc[i];
        if (clip > 0.0) r = r < lo ? lo : (r > hi ? hi : r);
        if (mu != 0.0) r = r - (0.5 * mu) * q[i];
        rhs[i] = r;
        s += r;
    }
    s = sr_block_sum<kSpringBlock>(s, red);
    const double mean = s / (double)B;
    for (int64_t i = tid; i < B; i += kSpringBlock) rhs[i] = rhs[i] - mean;   // (the thread's own stores)
}

// one block: |d|^2 as k_sr_verdict, its verdict, and the step size: eff = fl32(lr) when cap == 0 or |d|^2 == 0, else fl32(min(lr, sqrt(cap / |d|^2)));
// eff_dev[0] = eff and eff_ring[slot] = eff for a step that updates, 0 for a skipped one
__global__ __launch_bounds__(kSpringNormBlock) void k_spring_verdict(const float* __restrict__ d, int64_t P, const int32_t* __restrict__ info, int32_t* __restrict__ status,
                                                                     int32_t* __restrict__ flag, double* __restrict__ norm_ring, double* __restrict__ eff_ring,
                                                                     int ring_len, const unsigned long long* __restrict__ counter,
                                                                     const float* __restrict__ step_size, double cap, float* __restrict__ eff_dev) {
    __shared__ double red[kSpringNormBlock];
    double s = 0.0;
    for (int64_t p = threadIdx.x; p < P; p += kSpringNormBlock) {
        const double v = (double)d[p];
        s += v * v;
    }
    s = sr_block_sum<kSpringNormBlock>(s, red);
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

// theta <- fl32(theta - fl32(eff d)), phi <- d where the verdict allows it; neither is touched otherwise
__global__ __launch_bounds__(kSpringBlock) void k_spring_update(float* __restrict__ params, float* __restrict__ phi, const float* __restrict__ d, int64_t P,
                                                                const float* __restrict__ eff, const int32_t* __restrict__ flag) {
    const int64_t p = (int64_t)blockIdx.x * kSpringBlock + threadIdx.x;
    if (p >= P || flag[0] == 0) return;
    const float dp = d[p];
    params[p] = __fsub_rn(params[p], __fmul_rn(eff[0], dp));
    phi[p] = dp;
}

int launch_spring_eloc(const float* hpsi, const float* psi, int64_t B, float* e_loc, float* inv, void* stream) {
    hipLaunchKernelGGL(k_spring_eloc, dim3((unsigned)((B + kSpringBlock - 1) / kSpringBlock)), dim3(kSpringBlock), 0, (hipStream_t)stream, hpsi, psi, B, e_loc, inv);
    return sr_finish();
}

int launch_spring_rhs(const float* hpsi, const float* psi, int64_t B, const double* q, double mu, double clip, float* e_loc, float* inv, double* rhs,
                      double* stats, void* stream) {
    if (B < 1 || B > kSpringMaxSort) return WF_ERR_INVALID;
    hipLaunchKernelGGL(k_spring_rhs, dim3(1), dim3(kSpringBlock), 0, (hipStream_t)stream, hpsi, psi, B, q, mu, clip, e_loc, inv, rhs, stats);
    return sr_finish();
}

int launch_spring_verdict(const float* d, int64_t P, const int32_t* info, int32_t* status, int32_t* flag, double* norm_ring, double* eff_ring, int ring_len,
                          const unsigned long long* counter, const float* step_size, double cap, float* eff, void* stream) {
    hipLaunchKernelGGL(k_spring_verdict, dim3(1), dim3(kSpringNormBlock), 0, (hipStream_t)stream, d, P, info, status, flag, norm_ring, eff_ring, ring_len, counter,
                       step_size, cap, eff);
    return sr_finish();
}

int launch_spring_update(float* params, float* phi, const float* d, int64_t P, const float* eff, const int32_t* flag, void* stream) {
    hipLaunchKernelGGL(k_spring_update, dim3((unsigned)((P + kSpringBlock - 1) / kSpringBlock)), dim3(kSpringBlock), 0, (hipStream_t)stream, params, phi, d, P, eff,
                       flag);
    return sr_finish();
}

}  // namespace wf

using namespace wf;

extern "C" {

int wf_sr_matvec(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const float* v_dev, double* q_dev, void* stream) {
    if (B < 1 || P < 1 || ld < P || !rows_dev || !v_dev || !q_dev) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    hipLaunchKernelGGL(k_sr_matvec, dim3((unsigned)B), dim3(kSpringBlock), 0, (hipStream_t)stream, rows_dev, ld, B, P, (int)sr_vec_ok(rows_dev, ld), v_dev,
                       (int)sr_vec_ok(v_dev, 0), q_dev);
    return sr_finish();
}

int wf_spring_rhs(const float* hpsi_dev, const float* psi_dev, int64_t B, const double* q_dev, double mu, double clip, float* e_loc_dev, float* inv_dev,
                  double* rhs_dev, double* stats_dev, void* stream) {
    if (B < 1 || !hpsi_dev || !psi_dev || !e_loc_dev || !inv_dev || !rhs_dev) return WF_ERR_INVALID;
    if (!(mu >= 0.0) || !(mu < 1.0) || !(clip >= 0.0) || (mu != 0.0 && !q_dev)) return WF_ERR_INVALID;
    if (B > kSpringMaxSort) return WF_ERR_UNSUPPORTED;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return launch_spring_rhs(hpsi_dev, psi_dev, B, q_dev, mu, clip, e_loc_dev, inv_dev, rhs_dev, stats_dev, stream);
}

int wf_sr_apply_add(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const double* y_dev, double scale, const float* prev_dev, double mu,
                    float* out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (B < 1 || P < 1 || ld < P || !rows_dev || !y_dev || !out_dev || !workspace_dev) return WF_ERR_INVALID;
    if (!(mu >= 0.0) || !(mu < 1.0)) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    if (workspace_bytes < apply_ws_bytes(B, P)) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    double* yc = (double*)workspace_dev;
    double* partial = (double*)((char*)workspace_dev + sr_align(B * 8));
    const int64_t nslab = (B + kSrSlab - 1) / kSrSlab;
    hipLaunchKernelGGL(k_sr_ycentre, dim3(1), dim3(256), 0, s, y_dev, B, yc);
    hipLaunchKernelGGL(k_sr_apply, dim3((unsigned)((P + 1023) / 1024), (unsigned)nslab), dim3(256), 0, s, rows_dev, ld, B, P, (int)sr_vec_ok(rows_dev, ld),
                       (const double*)yc, partial);
    hipLaunchKernelGGL(k_sr_apply_add_reduce, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const double*)partial, nslab, P, scale, prev_dev, mu, out_dev);
    return sr_finish();
}

}  // extern "C"
