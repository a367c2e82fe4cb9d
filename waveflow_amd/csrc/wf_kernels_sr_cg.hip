// wf_kernels_sr_cg.hip -- the matrix-free solve of include/waveflow_sr_cg.h: preconditioned conjugate gradients on (Tbar + lambda I) y = rhs with
// Tbar v = H O (O^T (H v)) / B applied as two passes over the rows.  Per iteration four launches:
//     k_cg_pass_a      partial[chunk][k] = sum over the chunk's 32 rows of (p[b] - mean p) O[b][k]          (the slab pass of wf_sr_apply)
//     k_cg_reduce_a    z[k] = sum of the chunk partials, chunk 0 first; zzpart[block] = sum of z[k]^2 over the block's 256 entries
//     k_cg_pass_b      q[b] = sum_k O[b][k] z[k], four rows per workgroup                                   (k_sr_matvec with an fp64 vector)
//     k_cg_update      one workgroup: pAp, alpha, y, r, the convergence test and the status word, rho, p, mean p
// and at a restart k_cg_begin, the column means (pass A with unit weights), the diagonal of Tbar (k_cg_pass_b in its second form) and k_cg_init.
// Every kernel of an iteration returns at once unless the status word says "running".  No floating-point atomics; every sum has one order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/waveflow_sr_cg.h"
#include "wf_internal.h"
#include "wf_sr_common.h"

namespace wf {

namespace {

constexpr int kCgBlock = 256;
constexpr int kCgVecBlock = 1024;   // the one workgroup of the vector kernels
constexpr int kCgRows = 4;          // rows per workgroup of pass B
constexpr int32_t kCgConverged = 0, kCgRunning = 1, kCgFailed = 2;

struct CgControl {
    int32_t status;
    int32_t iterations;
    double rho;      // r^T (r / M)
    double rhs2;     // rhs^T rhs
    double r2;       // r^T r of the recurrence
    double lambda;
    double pmean;    // mean p: pass A centres with it
};

struct CgLayout {
    CgControl* ctrl;
    double *r, *p, *q, *diag, *z, *obar, *zzpart, *partial;
    int64_t nchunk, nzz, bytes;
};

inline CgLayout cg_layout(void* ws, int64_t B, int64_t P) {
    CgLayout l;
    char* c = (char*)ws;
    int64_t off = 0;
    auto take = [&](int64_t n) {
        char* at = c + off;
        off += sr_align(n);
        return at;
    };
    l.nchunk = (B + kSrSlab - 1) / kSrSlab;
    l.nzz = (P + kCgBlock - 1) / kCgBlock;
    // (the chunk partials first: wf_sr_apply may use the same workspace after the solve, and its layout fits inside this one)
    l.partial = (double*)take(l.nchunk * P * 8 + sr_align(B * 8));
    l.ctrl = (CgControl*)take(sizeof(CgControl));
    l.r = (double*)take(B * 8);
    l.p = (double*)take(B * 8);
    l.q = (double*)take(B * 8);
    l.diag = (double*)take(B * 8);
    l.z = (double*)take(P * 8);
    l.obar = (double*)take(P * 8);
    l.zzpart = (double*)take(l.nzz * 8);
    l.bytes = off;
    return l;
}

// sums of a, b, c, d over the 256 threads of the block (red[4][256]); the tree of sr_block_sum for each
__device__ __forceinline__ void cg_block_sum4(double& a, double& b, double& c, double& d, double (*red)[kCgBlock]) {
    const int tid = threadIdx.x;
    red[0][tid] = a;
    red[1][tid] = b;
    red[2][tid] = c;
    red[3][tid] = d;
    __syncthreads();
    for (int s = kCgBlock / 2; s > 0; s >>= 1) {
        if (tid < s) {
            red[0][tid] += red[0][tid + s];
            red[1][tid] += red[1][tid + s];
            red[2][tid] += red[2][tid + s];
            red[3][tid] += red[3][tid + s];
        }
        __syncthreads();
    }
    a = red[0][0];
    b = red[1][0];
    c = red[2][0];
    d = red[3][0];
}

// z[c .. c + 3] (fp64, 32-byte aligned at every c that is a multiple of 4: the workspace is), zeros past P
__device__ __forceinline__ void cg_load_z4(const double* __restrict__ z, int64_t c, int64_t P, double (&w)[4]) {
    if (c + 4 <= P) {
        const double2 lo = *reinterpret_cast<const double2*>(z + c), hi = *reinterpret_cast<const double2*>(z + c + 2);
        w[0] = lo.x;
        w[1] = lo.y;
        w[2] = hi.x;
        w[3] = hi.y;
        return;
    }
    for (int i = 0; i < 4; ++i) w[i] = c + i < P ? z[c + i] : 0.0;
}

}  // namespace

__global__ void k_cg_begin(CgControl* __restrict__ ctrl) {
    ctrl->status = kCgRunning;
    ctrl->iterations = 0;
}

// partial[chunk][k] = sum over the 32 rows of the chunk, first row first, of w_b O[b][k]; w_b = v[b] - ctrl->pmean, or 1 where v == nullptr
// (the column sums); four columns per thread
__global__ __launch_bounds__(kCgBlock) void k_cg_pass_a(const float* __restrict__ rows, int64_t ld, int64_t B, int64_t P, int vec, const double* __restrict__ v,
                                                        const CgControl* __restrict__ ctrl, double* __restrict__ partial) {
    if (ctrl->status != kCgRunning) return;
    __shared__ double ys[kSrSlab];
    const int64_t b0 = (int64_t)blockIdx.y * kSrSlab;
    if (threadIdx.x < kSrSlab) {
        const int64_t b = b0 + threadIdx.x;
        ys[threadIdx.x] = b < B ? (v ? v[b] - ctrl->pmean : 1.0) : 0.0;
    }
    __syncthreads();
    const int64_t c = ((int64_t)blockIdx.x * kCgBlock + threadIdx.x) * 4;
    if (c >= P) return;
    const int nr = (int)std::min<int64_t>(kSrSlab, B - b0);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 8
    for (int r = 0; r < nr; ++r) {
        const float4 x = sr_load4(rows, ld, b0 + r, B, c, P, vec != 0);
        const double w = ys[r];
        a0 += w * (double)x.x;
        a1 += w * (double)x.y;
        a2 += w * (double)x.z;
        a3 += w * (double)x.w;
    }
    double* out = partial + (int64_t)blockIdx.y * P + c;
    out[0] = a0;
    if (c + 1 < P) out[1] = a1;
    if (c + 2 < P) out[2] = a2;
    if (c + 3 < P) out[3] = a3;
}

// z[k] = scale * (sum of the chunk partials, chunk 0 first); zzpart[block] = sum over the block's entries of z[k]^2 (zzpart may be nullptr)
__global__ __launch_bounds__(kCgBlock) void k_cg_reduce_a(const double* __restrict__ partial, int64_t nchunk, int64_t P, double scale, const CgControl* __restrict__ ctrl,
                                                          double* __restrict__ z, double* __restrict__ zzpart) {
    if (ctrl->status != kCgRunning) return;
    __shared__ double red[kCgBlock];
    const int64_t k = (int64_t)blockIdx.x * kCgBlock + threadIdx.x;
    double s = 0.0;
    if (k < P) {
        for (int64_t i = 0; i < nchunk; ++i) s += partial[i * P + k];
        s = scale * s;
        z[k] = s;
    }
    if (zzpart == nullptr) return;   // (uniform)
    const double t = sr_block_sum<kCgBlock>(s * s, red);
    if (threadIdx.x == 0) zzpart[blockIdx.x] = t;
}

// DIAG false: q[b] = sum_k O[b][k] z[k].  DIAG true: q[b] = (1 / B) sum_k (O[b][k] - z[k])^2 with z = obar.  Four rows per workgroup; thread t
// takes columns 4 t .. 4 t + 3, then + 1024, ... into four sums per row, ((s0 + s1) + (s2 + s3)), then the tree over the 256 threads.
template <bool DIAG>
__global__ __launch_bounds__(kCgBlock) void k_cg_pass_b(const float* __restrict__ rows, int64_t ld, int64_t B, int64_t P, int vec, const double* __restrict__ z,
                                                        const CgControl* __restrict__ ctrl, double* __restrict__ q) {
    if (ctrl->status != kCgRunning) return;
    __shared__ double red[kCgRows][kCgBlock];
    const int64_t b0 = (int64_t)blockIdx.x * kCgRows;
    double s[kCgRows][4];
#pragma unroll
    for (int r = 0; r < kCgRows; ++r)
        for (int i = 0; i < 4; ++i) s[r][i] = 0.0;
#pragma unroll 2
    for (int64_t c = (int64_t)threadIdx.x * 4; c < P; c += 4 * kCgBlock) {
        double w[4];
        cg_load_z4(z, c, P, w);
        float4 x[kCgRows];
#pragma unroll
        for (int r = 0; r < kCgRows; ++r) x[r] = sr_load4(rows, ld, b0 + r, B, c, P, vec != 0);
#pragma unroll
        for (int r = 0; r < kCgRows; ++r) {
            const double e[4] = {(double)x[r].x, (double)x[r].y, (double)x[r].z, (double)x[r].w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (DIAG) {
                    const double d = c + i < P ? e[i] - w[i] : 0.0;
                    s[r][i] += d * d;
                } else {
                    s[r][i] += e[i] * w[i];
                }
            }
        }
    }
    double t[kCgRows];
#pragma unroll
    for (int r = 0; r < kCgRows; ++r) t[r] = (s[r][0] + s[r][1]) + (s[r][2] + s[r][3]);
    cg_block_sum4(t[0], t[1], t[2], t[3], red);
    if (threadIdx.x < kCgRows && b0 + threadIdx.x < B) {
        const double out = t[threadIdx.x];
        q[b0 + threadIdx.x] = DIAG ? out / (double)B : out;
    }
}

// one workgroup: trace, lambda, rhs^T rhs and the start of the recurrences (diag holds Tbar's diagonal)
__global__ __launch_bounds__(kCgVecBlock) void k_cg_init(const double* __restrict__ rhs, int64_t B, double damping_abs, double damping_rel, int precondition,
                                                         const double* __restrict__ diag, double* __restrict__ y, double* __restrict__ r, double* __restrict__ p,
                                                         CgControl* __restrict__ ctrl) {
    __shared__ double red[kCgVecBlock];
    const int tid = threadIdx.x;
    double tr = 0.0, rhs2 = 0.0;
    for (int64_t i = tid; i < B; i += kCgVecBlock) {
        tr += diag[i];
        rhs2 += rhs[i] * rhs[i];
    }
    tr = sr_block_sum<kCgVecBlock>(tr, red);
    rhs2 = sr_block_sum<kCgVecBlock>(rhs2, red);
    const double lambda = damping_abs + damping_rel * tr / (double)B;
    const bool bad = !isfinite(tr) || !isfinite(rhs2) || !(lambda > 0.0) || !isfinite(lambda);
    const bool done = !bad && (rhs2 == 0.0 || B == 1);
    double rho = 0.0, ps = 0.0;
    for (int64_t i = tid; i < B; i += kCgVecBlock) {
        const double ri = rhs[i];
        const double pi = ri / (precondition ? diag[i] + lambda : 1.0);
        y[i] = bad ? __builtin_nan("") : (done ? ri / lambda : 0.0);   // (rhs == 0: zeros; B == 1: rhs / lambda)
        r[i] = done ? 0.0 : ri;
        p[i] = pi;
        rho += ri * pi;
        ps += pi;
    }
    rho = sr_block_sum<kCgVecBlock>(rho, red);
    ps = sr_block_sum<kCgVecBlock>(ps, red);
    if (tid != 0) return;
    ctrl->status = bad ? kCgFailed : (done ? kCgConverged : kCgRunning);
    ctrl->iterations = 0;
    ctrl->rho = rho;
    ctrl->rhs2 = rhs2;
    ctrl->r2 = done ? 0.0 : rhs2;
    ctrl->lambda = lambda;
    ctrl->pmean = ps / (double)B;
}

// one workgroup: the vector part of an iteration.  Thread t owns entries t, t + 1024, ... of every B-vector throughout.
__global__ __launch_bounds__(kCgVecBlock) void k_cg_update(int64_t B, int64_t nzz, double tol, int precondition, const double* __restrict__ zzpart,
                                                           const double* __restrict__ q, const double* __restrict__ diag, double* __restrict__ y,
                                                           double* __restrict__ r, double* __restrict__ p, CgControl* __restrict__ ctrl) {
    if (ctrl->status != kCgRunning) return;
    __shared__ double red[kCgVecBlock];
    const int tid = threadIdx.x;
    const double lambda = ctrl->lambda, rho = ctrl->rho, rhs2 = ctrl->rhs2;
    double zz = 0.0, pp = 0.0, qs = 0.0;
    for (int64_t i = tid; i < nzz; i += kCgVecBlock) zz += zzpart[i];
    for (int64_t i = tid; i < B; i += kCgVecBlock) {
        pp += p[i] * p[i];
        qs += q[i];
    }
    zz = sr_block_sum<kCgVecBlock>(zz, red);
    pp = sr_block_sum<kCgVecBlock>(pp, red);
    qs = sr_block_sum<kCgVecBlock>(qs, red);
    const double pAp = zz / (double)B + lambda * pp;
    if (!(pAp > 0.0) || !isfinite(pAp)) {   // (uniform)
        for (int64_t i = tid; i < B; i += kCgVecBlock) y[i] = __builtin_nan("");
        if (tid == 0) ctrl->status = kCgFailed;
        return;
    }
    const double alpha = rho / pAp, qmean = qs / (double)B;
    double r2 = 0.0, rz = 0.0;
    for (int64_t i = tid; i < B; i += kCgVecBlock) {
        const double pi = p[i];
        const double ap = (q[i] - qmean) / (double)B + lambda * pi;
        y[i] += alpha * pi;
        const double ri = r[i] - alpha * ap;
        r[i] = ri;
        r2 += ri * ri;
        rz += ri * (ri / (precondition ? diag[i] + lambda : 1.0));
    }
    r2 = sr_block_sum<kCgVecBlock>(r2, red);
    rz = sr_block_sum<kCgVecBlock>(rz, red);
    if (!isfinite(r2) || !isfinite(rz)) {
        for (int64_t i = tid; i < B; i += kCgVecBlock) y[i] = __builtin_nan("");
        if (tid == 0) {
            ctrl->status = kCgFailed;
            ctrl->iterations += 1;
            ctrl->r2 = r2;
        }
        return;
    }
    const bool converged = r2 <= tol * tol * rhs2;
    double ps = 0.0;
    if (!converged) {
        const double beta = rz / rho;
        for (int64_t i = tid; i < B; i += kCgVecBlock) {
            const double pi = r[i] / (precondition ? diag[i] + lambda : 1.0) + beta * p[i];
            p[i] = pi;
            ps += pi;
        }
    }
    ps = sr_block_sum<kCgVecBlock>(ps, red);
    if (tid != 0) return;
    ctrl->iterations += 1;
    ctrl->r2 = r2;
    if (converged) {
        ctrl->status = kCgConverged;
    } else {
        ctrl->rho = rz;
        ctrl->pmean = ps / (double)B;
    }
}

// info[4] = status, iterations, sqrt(r^T r / rhs^T rhs) (0 where rhs == 0), lambda
__global__ void k_cg_info(const CgControl* __restrict__ ctrl, double* __restrict__ info) {
    info[0] = (double)ctrl->status;
    info[1] = (double)ctrl->iterations;
    info[2] = ctrl->rhs2 > 0.0 ? sqrt(ctrl->r2 / ctrl->rhs2) : (ctrl->status == kCgFailed ? __builtin_nan("") : 0.0);
    info[3] = ctrl->lambda;
}

}  // namespace wf

using namespace wf;

extern "C" {

int64_t wf_sr_cg_workspace_bytes(int64_t B, int64_t P) {
    if (B < 1 || P < 1) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    return cg_layout(nullptr, B, P).bytes;
}

int wf_sr_cg_solve(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const double* rhs_dev, double damping_abs, double damping_rel, double tol,
                   int32_t n_iter, int32_t restart, int32_t precondition, double* y_dev, double* info_dev, void* workspace_dev, int64_t workspace_bytes,
                   void* stream) {
    if (B < 1 || P < 1 || ld < P || !rows_dev || !rhs_dev || !y_dev || !info_dev || !workspace_dev) return WF_ERR_INVALID;
    if (!(damping_abs >= 0.0) || !(damping_rel >= 0.0) || !(tol > 0.0) || !(tol < 1.0) || n_iter < 0) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    const CgLayout l = cg_layout(workspace_dev, B, P);
    if (workspace_bytes < l.bytes) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    const int vec = (int)sr_vec_ok(rows_dev, ld), pre = precondition != 0;
    const dim3 grid_a((unsigned)((P + 4 * kCgBlock - 1) / (4 * kCgBlock)), (unsigned)l.nchunk), grid_b((unsigned)((B + kCgRows - 1) / kCgRows));
    if (restart != 0) {
        hipLaunchKernelGGL(k_cg_begin, dim3(1), dim3(1), 0, s, l.ctrl);
        hipLaunchKernelGGL(k_cg_pass_a, grid_a, dim3(kCgBlock), 0, s, rows_dev, ld, B, P, vec, (const double*)nullptr, (const CgControl*)l.ctrl, l.partial);
        hipLaunchKernelGGL(k_cg_reduce_a, dim3((unsigned)l.nzz), dim3(kCgBlock), 0, s, (const double*)l.partial, l.nchunk, P, 1.0 / (double)B,
                           (const CgControl*)l.ctrl, l.obar, (double*)nullptr);
        hipLaunchKernelGGL(k_cg_pass_b<true>, grid_b, dim3(kCgBlock), 0, s, rows_dev, ld, B, P, vec, (const double*)l.obar, (const CgControl*)l.ctrl, l.diag);
        hipLaunchKernelGGL(k_cg_init, dim3(1), dim3(kCgVecBlock), 0, s, rhs_dev, B, damping_abs, damping_rel, pre, (const double*)l.diag, y_dev, l.r, l.p, l.ctrl);
    }
    for (int32_t it = 0; it < n_iter; ++it) {
        hipLaunchKernelGGL(k_cg_pass_a, grid_a, dim3(kCgBlock), 0, s, rows_dev, ld, B, P, vec, (const double*)l.p, (const CgControl*)l.ctrl, l.partial);
        hipLaunchKernelGGL(k_cg_reduce_a, dim3((unsigned)l.nzz), dim3(kCgBlock), 0, s, (const double*)l.partial, l.nchunk, P, 1.0, (const CgControl*)l.ctrl, l.z,
                           l.zzpart);
        hipLaunchKernelGGL(k_cg_pass_b<false>, grid_b, dim3(kCgBlock), 0, s, rows_dev, ld, B, P, vec, (const double*)l.z, (const CgControl*)l.ctrl, l.q);
        hipLaunchKernelGGL(k_cg_update, dim3(1), dim3(kCgVecBlock), 0, s, B, l.nzz, tol, pre, (const double*)l.zzpart, (const double*)l.q, (const double*)l.diag,
                           y_dev, l.r, l.p, l.ctrl);
    }
    hipLaunchKernelGGL(k_cg_info, dim3(1), dim3(1), 0, s, (const CgControl*)l.ctrl, info_dev);
    return sr_finish();
}

}  // extern "C"
