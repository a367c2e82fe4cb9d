// wf_kernels_dmc.hip -- fixed-node diffusion Monte Carlo with a fixed population (include/waveflow_dmc.h, which states every formula): the
// proposal, the acceptance with the branching weight and the generation record, and the comb.  Model-free: psi and its derivatives come from
// the caller (wf_psi_coord_derivs in the step, wf_train_dmc.cpp).  One lane per walker everywhere.
//
// k_dmc_propose   one launch, B / 256 blocks.
// k_dmc_accept    observe_blocks(B) blocks, grid-stride; the generation record in the one order of the project's fp64 sums (wf_accum.h): one
//                 partial per block, k_dmc_record adds the partials in block order.
// the comb        k_comb_wmax (block maxima of the valid weights) -> k_comb_scan (every block reduces the <= 1024 block maxima again, quantises
//                 its 1024 weights and scans them in uint64) -> k_comb_src (every block scans the <= 1024 block totals again, finds the source
//                 of its slots by two bounded binary searches and gathers into the workspace) -> k_comb_store (copies back, weights 1, largest
//                 multiplicity).  Integers only behind the quantisation: no order of summation to depend on.
// fp64 arithmetic is spelled operation by operation; the unit is built with -ffp-contract=off and says so again below.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wf_dmc.h"
#include "wf_eloc.h"
#include "wf_philox.h"

#pragma clang fp contract(off)

namespace wf {

namespace {

using u64 = unsigned long long;

__device__ __forceinline__ u64 dmc_stream(int purpose, u64 step, u64 b) {
    return (1ull << 63) | ((u64)purpose << 60) | ((step & ((1ull << 40) - 1ull)) << 20) | b;
}

// the drift of the header: v_d = grad_d / (psi + 1e-8) in fp32, vbar in fp64; fin &= every v_d is finite
template <int D>
__device__ __forceinline__ void drift(float ps, const float (&gr)[D], double tau, int limit, double (&vb)[D], bool& fin) {
    const float inv = __fdiv_rn(1.0f, __fadd_rn(ps, 1e-8f));
    float v[D];
    double v2 = 0.0;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        v[d] = __fmul_rn(gr[d], inv);
        fin = fin && isfinite(v[d]);
        const double vd = (double)v[d];
        v2 = v2 + vd * vd;
    }
    double f = 1.0;
    if (limit) {
        const double a = v2 * tau;
        if (a != 0.0) f = (-1.0 + sqrt(1.0 + 2.0 * a)) / a;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) vb[d] = limit ? (double)v[d] * f : (double)v[d];
}

template <int D>
__global__ __launch_bounds__(kDmcBlock) void k_dmc_propose(const float* __restrict__ xg, const float* __restrict__ psi, const float* __restrict__ grad,
                                                           int64_t B, const DmcParams p, float* __restrict__ xn, int32_t* __restrict__ flag,
                                                           float* __restrict__ chi) {
    const int64_t b = (int64_t)blockIdx.x * kDmcBlock + threadIdx.x;
    if (b >= B) return;
    const u64 step = p.counter ? p.counter[0] : p.step;
    float x[D], gr[D];
    bool fin = true;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        x[d] = xg[b * D + d];
        gr[d] = grad[b * D + d];
        fin = fin && isfinite(x[d]) && isfinite(gr[d]);
    }
    const float ps = psi[b];
    fin = fin && isfinite(ps);
    double vb[D];
    drift<D>(ps, gr, p.tau, p.limit_drift, vb, fin);
    Philox rng(p.seed, dmc_stream(0, step, (u64)b));
    float c[D];
#pragma unroll
    for (int k = 0; k < (D + 1) / 2; ++k) {
        const float u1 = rng.uniform(), u2 = rng.uniform();
        const float r = sqrtf(-2.0f * logf(1.0f - u1));
        const float th = 6.28318530717958647692f * u2;
        c[2 * k] = r * cosf(th);
        if (2 * k + 1 < D) c[2 * k + 1] = r * sinf(th);
    }
    float xp[D];
    bool ok = fin;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        xp[d] = (float)(((double)x[d] + p.tau * vb[d]) + p.sqrt_tau * (double)c[d]);
        ok = ok && isfinite(xp[d]) && fabsf(xp[d]) < p.box;
        if (d > 0) ok = ok && xp[d] > xp[d - 1];
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
        xn[b * D + d] = ok ? xp[d] : x[d];
        if (chi) chi[b * D + d] = c[d];
    }
    flag[b] = ok ? 0 : 1;
}

template <int D>
__global__ __launch_bounds__(kDmcBlock) void k_dmc_accept(float* __restrict__ xg, float* __restrict__ psi, float* __restrict__ grad,
                                                          float* __restrict__ eloc, const float* __restrict__ xn, const float* __restrict__ psn,
                                                          const float* __restrict__ grn, const float* __restrict__ hdn,
                                                          const int32_t* __restrict__ flag, int64_t B, const Protons pr, const DmcParams p,
                                                          const double* __restrict__ e_trial, double* __restrict__ wg, u64* __restrict__ partial,
                                                          double* __restrict__ logA_out, float* __restrict__ u_out, int32_t* __restrict__ acc_out) {
    const u64 step = p.counter ? p.counter[0] : p.step;
    const double et = e_trial[0];
    double s[WF_DMC_RECORD];
#pragma unroll
    for (int k = 0; k < WF_DMC_RECORD; ++k) s[k] = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kDmcBlock + threadIdx.x; b < B; b += (int64_t)gridDim.x * kDmcBlock) {
        float xo[D], gro[D], xq[D], grq[D], hdq[D];
        bool fin_old = true, fin_new = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            xo[d] = xg[b * D + d];
            gro[d] = grad[b * D + d];
            xq[d] = xn[b * D + d];
            grq[d] = grn[b * D + d];
            hdq[d] = hdn[b * D + d];
            fin_old = fin_old && isfinite(xo[d]) && isfinite(gro[d]);
            fin_new = fin_new && isfinite(xq[d]) && isfinite(grq[d]) && isfinite(hdq[d]);
        }
        const float pso = psi[b], psq = psn[b], eo = eloc[b];
        fin_old = fin_old && isfinite(pso) && isfinite(eo);
        fin_new = fin_new && isfinite(psq);
        float v[WF_OBSERVE_SCALARS];
        local_values<D>(xq, psq, grq, hdq, pr, v);   // the rule of waveflow_observe.h (wf_eloc.h)
        const float eq = v[0];
        fin_new = fin_new && isfinite(eq);
        double vbo[D], vbq[D];
        bool fin_v = true;
        drift<D>(pso, gro, p.tau, p.limit_drift, vbo, fin_v);
        drift<D>(psq, grq, p.tau, p.limit_drift, vbq, fin_v);
        double qf = 0.0, qr = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const double f = ((double)xq[d] - (double)xo[d]) - p.tau * vbo[d];
            const double r = ((double)xo[d] - (double)xq[d]) - p.tau * vbq[d];
            qf = qf + f * f;
            qr = qr + r * r;
        }
        const double logA = 2.0 * log(fabs((double)psq) / fabs((double)pso)) + (qf - qr) / (2.0 * p.tau);
        Philox rng(p.seed, dmc_stream(1, step, (u64)b));
        const float u = rng.uniform();
        const double A = logA >= 0.0 ? 1.0 : exp(logA);
        const double sign = (double)psq * (double)pso;
        const bool fl = flag[b] != 0;
        const bool accept = !fl && sign > 0.0 && fin_new && (double)u < A;
        if (accept) {
            s[3] += 1.0;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                xg[b * D + d] = xq[d];
                grad[b * D + d] = grq[d];
            }
            psi[b] = psq;
            eloc[b] = eq;
        } else if (fl || sign <= 0.0) {
            s[4] += 1.0;
        } else if (!fin_new) {
            s[5] += 1.0;
        }
        const float en = accept ? eq : eo;
        double wb = 0.0;
        if (fin_old) {
            double ebar = ((double)en + (double)eo) * 0.5;
            if (p.e_cut > 0.0) {
                const double win = p.e_cut / p.sqrt_tau;
                ebar = ebar < et - win ? et - win : ebar > et + win ? et + win : ebar;
            }
            wb = exp(-p.tau * (ebar - et));
        }
        wg[b] = wb;
        if (wb != 0.0) {
            const double e = (double)en;
            s[0] += wb;
            s[1] += wb * e;
            s[2] += (wb * e) * e;
        }
        if (logA_out) logA_out[b] = logA;
        if (u_out) u_out[b] = u;
        if (acc_out) acc_out[b] = accept ? 1 : 0;
    }
    block_partial<WF_DMC_RECORD, 0>(s, nullptr, WF_DMC_RECORD, partial + (int64_t)blockIdx.x * WF_DMC_RECORD);
}

// wf_vqmc_dmc_init: e_loc of the walkers themselves, weight 1 or (a value that is not finite) 0, the record's first three sums
template <int D>
__global__ __launch_bounds__(kDmcBlock) void k_dmc_init_weights(const float* __restrict__ xg, const float* __restrict__ psi, const float* __restrict__ grad,
                                                                const float* __restrict__ hdiag, int64_t B, const Protons pr,
                                                                float* __restrict__ eloc, double* __restrict__ wg, u64* __restrict__ partial) {
    double s[WF_DMC_RECORD];
#pragma unroll
    for (int k = 0; k < WF_DMC_RECORD; ++k) s[k] = 0.0;
    for (int64_t b = (int64_t)blockIdx.x * kDmcBlock + threadIdx.x; b < B; b += (int64_t)gridDim.x * kDmcBlock) {
        float x[D], gr[D], hd[D];
        bool fin = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            x[d] = xg[b * D + d];
            gr[d] = grad[b * D + d];
            hd[d] = hdiag[b * D + d];
            fin = fin && isfinite(x[d]) && isfinite(gr[d]) && isfinite(hd[d]);
        }
        const float ps = psi[b];
        float v[WF_OBSERVE_SCALARS];
        local_values<D>(x, ps, gr, hd, pr, v);
        fin = fin && isfinite(ps) && isfinite(v[0]);
        eloc[b] = v[0];
        wg[b] = fin ? 1.0 : 0.0;
        if (fin) {
            const double e = (double)v[0];
            s[0] += 1.0;
            s[1] += e;
            s[2] += e * e;
        } else {
            s[5] += 1.0;
        }
    }
    block_partial<WF_DMC_RECORD, 0>(s, nullptr, WF_DMC_RECORD, partial + (int64_t)blockIdx.x * WF_DMC_RECORD);
}

// One workgroup: thread k < 6 gets column k of the block partials (reduce_columns): the record of this generation.
__global__ __launch_bounds__(kDmcBlock) void k_dmc_record(const u64* __restrict__ partial, int n_blocks, double* __restrict__ record) {
    const Column col = reduce_columns<WF_DMC_RECORD>(partial, n_blocks, WF_DMC_RECORD, WF_DMC_RECORD);
    if (threadIdx.x < WF_DMC_RECORD) record[threadIdx.x] = col.sum;
}

// ---- the comb

__device__ __forceinline__ bool weight_valid(double w) { return isfinite(w) && w > 0.0; }

// max over the block (every thread gets it); order does not matter for a maximum
__device__ __forceinline__ double block_max(double m) {
    __shared__ double red[kDmcBlock / 64];
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
    __syncthreads();   // (red may still be read from an earlier call)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    double t = red[0];
    for (int w = 1; w < kDmcBlock / 64; ++w) t = fmax(t, red[w]);
    return t;
}

__global__ __launch_bounds__(kDmcBlock) void k_comb_wmax(const double* __restrict__ w, int64_t B, double* __restrict__ bmax) {
    const int64_t base = (int64_t)blockIdx.x * kDmcScanTile;
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < kDmcScanTile / kDmcBlock; ++j) {
        const int64_t i = base + j * kDmcBlock + threadIdx.x;
        if (i < B) {
            const double v = w[i];
            if (weight_valid(v)) m = fmax(m, v);
        }
    }
    m = block_max(m);
    if (threadIdx.x == 0) bmax[blockIdx.x] = m;
}

// inclusive scan of one value per thread over the block, in thread order (uint64: exact); *total = the block's sum
__device__ __forceinline__ u64 block_scan(u64 v, u64* total) {
    __shared__ u64 wsum[kDmcBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const u64 t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    __syncthreads();   // (wsum may still be read from an earlier call)
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    u64 before = 0, all = 0;
    for (int k = 0; k < kDmcBlock / 64; ++k) {
        if (k < wave) before += wsum[k];
        all += wsum[k];
    }
    *total = all;
    return v + before;
}

__global__ __launch_bounds__(kDmcBlock) void k_comb_scan(const double* __restrict__ w, int64_t B, int n_blocks, const double* __restrict__ bmax,
                                                         u64* __restrict__ prefix, u64* __restrict__ bsum, u64* __restrict__ stats) {
    double m = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += kDmcBlock) m = fmax(m, bmax[i]);
    const double wmax = block_max(m);
    if (stats && blockIdx.x == 0 && threadIdx.x == 0) stats[0] = (u64)__double_as_longlong(wmax);
    const double scale = 4294967296.0 / wmax;   // (unused where wmax == 0: then no weight is valid)
    constexpr int kPer = kDmcScanTile / kDmcBlock;
    const int64_t first = (int64_t)blockIdx.x * kDmcScanTile + (int64_t)threadIdx.x * kPer;
    u64 q[kPer], mine = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        q[j] = 0;
        if (first + j < B) {
            const double v = w[first + j];
            if (weight_valid(v)) {
                const double t = v * scale;
                q[j] = t < 8589934592.0 ? (u64)t : 8589934592ull;
            }
        }
        mine += q[j];
    }
    u64 total;
    u64 run = block_scan(mine, &total) - mine;   // exclusive over the threads before this one
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        run += q[j];
        if (first + j < B) prefix[first + j] = run;
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

template <int D>
__global__ __launch_bounds__(kDmcBlock) void k_comb_src(const float* __restrict__ xg, const float* __restrict__ psi, const float* __restrict__ grad,
                                                        const float* __restrict__ eloc, int64_t B, int n_blocks, const u64* __restrict__ prefix,
                                                        const u64* __restrict__ bsum, const DmcParams p, int purpose, int32_t* __restrict__ src,
                                                        float* __restrict__ xt, float* __restrict__ pst, float* __restrict__ grt,
                                                        float* __restrict__ et, u64* __restrict__ stats, u64* __restrict__ status) {
    __shared__ u64 incl[kDmcScanBlocksMax];   // inclusive sums of the block totals
    constexpr int kPer = kDmcScanBlocksMax / kDmcBlock;
    {
        u64 q[kPer], mine = 0;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            const int i = threadIdx.x * kPer + j;
            q[j] = i < n_blocks ? bsum[i] : 0ull;
            mine += q[j];
        }
        u64 total;
        u64 run = block_scan(mine, &total) - mine;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            run += q[j];
            incl[threadIdx.x * kPer + j] = run;
        }
    }
    __syncthreads();
    const u64 w_int = incl[n_blocks - 1];
    const u64 S = w_int / (u64)B;
    const u64 step = purpose == 3 ? 0ull : p.counter ? p.counter[0] : p.step;
    Philox rng(p.seed, dmc_stream(purpose, step, 0ull));
    rng.refill();
    const u64 rand64 = ((u64)rng.out[0] << 32) | (u64)rng.out[1];
    const u64 r = __umul64hi(rand64, S);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (stats) {
            stats[1] = w_int;
            stats[2] = S;
            stats[3] = w_int ? r : 0ull;
            stats[4] = 0ull;
        }
        if (status && w_int == 0) status[0] += 1ull;
    }
    const int64_t k = (int64_t)blockIdx.x * kDmcBlock + threadIdx.x;
    if (k >= B) return;
    int64_t j = k;
    if (w_int != 0) {
        const u64 tooth = (u64)k * S + r;
        // the first block whose inclusive total exceeds the tooth: at most 11 halvings of [0, n_blocks)
        int lo = 0, hi = n_blocks - 1;
        for (int it = 0; it < 11 && lo < hi; ++it) {
            const int mid = (lo + hi) >> 1;
            if (incl[mid] > tooth)
                hi = mid;
            else
                lo = mid + 1;
        }
        const u64 rest = tooth - (lo > 0 ? incl[lo - 1] : 0ull);
        const int64_t base = (int64_t)lo * kDmcScanTile;
        int64_t a = 0, z = (B - base < kDmcScanTile ? B - base : kDmcScanTile) - 1;
        for (int it = 0; it < 11 && a < z; ++it) {
            const int64_t mid = (a + z) >> 1;
            if (prefix[base + mid] > rest)
                z = mid;
            else
                a = mid + 1;
        }
        j = base + a;
        j = j < 0 ? 0 : j > B - 1 ? B - 1 : j;
    }
    src[k] = (int32_t)j;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        xt[k * D + d] = xg[j * D + d];
        grt[k * D + d] = grad[j * D + d];
    }
    pst[k] = psi[j];
    et[k] = eloc[j];
}

template <int D>
__global__ __launch_bounds__(kDmcBlock) void k_comb_store(float* __restrict__ xg, float* __restrict__ psi, float* __restrict__ grad,
                                                          float* __restrict__ eloc, double* __restrict__ w, int64_t B, const int32_t* __restrict__ src,
                                                          const float* __restrict__ xt, const float* __restrict__ pst, const float* __restrict__ grt,
                                                          const float* __restrict__ et, int32_t* __restrict__ src_out, u64* __restrict__ stats) {
    const int64_t k = (int64_t)blockIdx.x * kDmcBlock + threadIdx.x;
    if (k >= B) return;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        xg[k * D + d] = xt[k * D + d];
        grad[k * D + d] = grt[k * D + d];
    }
    psi[k] = pst[k];
    eloc[k] = et[k];
    w[k] = 1.0;
    const int32_t mine = src[k];
    if (src_out) src_out[k] = mine;
    // src ascends with k: a source's multiplicity is the length of its run, measured once, at the run's first slot
    if (stats && (k == 0 || src[k - 1] != mine)) {
        int64_t a = k, z = B;   // the first slot in (k, B] whose source differs (B: none)
        for (int it = 0; it < 21 && a + 1 < z; ++it) {
            const int64_t mid = (a + z) >> 1;
            if (src[mid] == mine)
                a = mid;
            else
                z = mid;
        }
        atomicMax(&stats[4], (u64)(z - k));   // (an integer maximum: no order to depend on)
    }
}

__global__ void k_dmc_reset(u64* counter, u64* status, double* ring, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) ring[i] = 0.0;
    if (i == 0) {
        counter[0] = 0ull;
        status[0] = 0ull;
    }
}

__global__ void k_dmc_trial(const double* __restrict__ record, double* __restrict__ e_trial) {
    const double e = record[1] / record[0];
    e_trial[0] = isfinite(e) ? e : 0.0;
}

__global__ void k_dmc_finish(const double* __restrict__ record, u64* __restrict__ counter, double* __restrict__ e_trial, double* __restrict__ ring,
                             int ring_len, double batch, double tau) {
    const u64 g = counter[0];
    double* row = ring + (size_t)(g % (u64)ring_len) * WF_DMC_RING_RECORD;
    const double et = e_trial[0];
#pragma unroll
    for (int k = 0; k < WF_DMC_RECORD; ++k) row[k] = record[k];
    row[6] = et - log(record[0] / batch) / tau;
    row[7] = et;
    const double e = record[1] / record[0];
    if (isfinite(e)) e_trial[0] = e;
    counter[0] = g + 1ull;
}

#define WF_DMC_CASES(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

}  // namespace

int launch_dmc_propose(const float* x, const float* psi, const float* grad, int64_t B, int D, const DmcParams& p, float* x_new, int32_t* flag,
                       float* chi, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((B + kDmcBlock - 1) / kDmcBlock));
#define WF_DMC_X(DD)                                                                                                     \
    case DD:                                                                                                             \
        hipLaunchKernelGGL(k_dmc_propose<DD>, grid, dim3(kDmcBlock), 0, s, x, psi, grad, B, p, x_new, flag, chi);         \
        break;
    switch (D) {
        WF_DMC_CASES(WF_DMC_X)
        default:
            return WF_ERR_INVALID;
    }
#undef WF_DMC_X
    return launch_status();
}

int launch_dmc_accept(float* x, float* psi, float* grad, float* e_loc, const float* x_new, const float* psi_new, const float* grad_new,
                      const float* hdiag_new, const int32_t* flag, int64_t B, int D, const Protons& pr, const DmcParams& p, const double* e_trial,
                      double* w, double* record, double* logA, float* u, int32_t* accepted, int init, void* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const int64_t blocks = observe_blocks(B);
    u64* partial = (u64*)ws;
#define WF_DMC_X(DD)                                                                                                                              \
    case DD:                                                                                                                                      \
        if (init)                                                                                                                                 \
            hipLaunchKernelGGL(k_dmc_init_weights<DD>, dim3((unsigned)blocks), dim3(kDmcBlock), 0, s, (const float*)x, (const float*)psi,           \
                               (const float*)grad, hdiag_new, B, pr, e_loc, w, partial);                                                          \
        else                                                                                                                                      \
            hipLaunchKernelGGL(k_dmc_accept<DD>, dim3((unsigned)blocks), dim3(kDmcBlock), 0, s, x, psi, grad, e_loc, x_new, psi_new, grad_new,      \
                               hdiag_new, flag, B, pr, p, e_trial, w, partial, logA, u, accepted);                                                \
        break;
    switch (D) {
        WF_DMC_CASES(WF_DMC_X)
        default:
            return WF_ERR_INVALID;
    }
#undef WF_DMC_X
    hipLaunchKernelGGL(k_dmc_record, dim3(1), dim3(kDmcBlock), 0, s, (const u64*)partial, (int)blocks, record);
    return launch_status();
}

int launch_dmc_reconfigure(float* x, float* psi, float* grad, float* e_loc, double* w, int64_t B, int D, const DmcParams& p, int purpose,
                           int32_t* src_out, unsigned long long* stats, unsigned long long* status, void* ws, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    const DmcCombLayout l = dmc_comb_layout(B, D);
    char* base = (char*)ws;
    double* bmax = (double*)(base + l.bmax);
    u64 *bsum = (u64*)(base + l.bsum), *prefix = (u64*)(base + l.prefix);
    int32_t* src = (int32_t*)(base + l.src);
    float *xt = (float*)(base + l.x), *pst = (float*)(base + l.psi), *grt = (float*)(base + l.grad), *et = (float*)(base + l.e_loc);
    const int n_blocks = (int)dmc_scan_blocks(B);
    const dim3 lanes((unsigned)((B + kDmcBlock - 1) / kDmcBlock));
    hipLaunchKernelGGL(k_comb_wmax, dim3(n_blocks), dim3(kDmcBlock), 0, s, (const double*)w, B, bmax);
    hipLaunchKernelGGL(k_comb_scan, dim3(n_blocks), dim3(kDmcBlock), 0, s, (const double*)w, B, n_blocks, (const double*)bmax, prefix, bsum, stats);
#define WF_DMC_X(DD)                                                                                                                              \
    case DD:                                                                                                                                      \
        hipLaunchKernelGGL(k_comb_src<DD>, lanes, dim3(kDmcBlock), 0, s, (const float*)x, (const float*)psi, (const float*)grad,                    \
                           (const float*)e_loc, B, n_blocks, (const u64*)prefix, (const u64*)bsum, p, purpose, src, xt, pst, grt, et, stats,       \
                           status);                                                                                                               \
        hipLaunchKernelGGL(k_comb_store<DD>, lanes, dim3(kDmcBlock), 0, s, x, psi, grad, e_loc, w, B, (const int32_t*)src, (const float*)xt,        \
                           (const float*)pst, (const float*)grt, (const float*)et, src_out, stats);                                               \
        break;
    switch (D) {
        WF_DMC_CASES(WF_DMC_X)
        default:
            return WF_ERR_INVALID;
    }
#undef WF_DMC_X
    return launch_status();
}

int launch_dmc_reset(const wf_dmc_state* st, void* stream) {
    const int n = st->ring_len * WF_DMC_RING_RECORD;
    hipLaunchKernelGGL(k_dmc_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (u64*)st->counter_dev, (u64*)st->status_dev,
                       st->ring_dev, n);
    return launch_status();
}

int launch_dmc_trial_from_record(const double* record, double* e_trial, void* stream) {
    hipLaunchKernelGGL(k_dmc_trial, dim3(1), dim3(1), 0, (hipStream_t)stream, record, e_trial);
    return launch_status();
}

int launch_dmc_finish(const wf_dmc_state* st, const double* record, int64_t B, double tau, void* stream) {
    hipLaunchKernelGGL(k_dmc_finish, dim3(1), dim3(1), 0, (hipStream_t)stream, record, (u64*)st->counter_dev, st->e_trial_dev, st->ring_dev,
                       st->ring_len, (double)B, tau);
    return launch_status();
}

}  // namespace wf

extern "C" {

using namespace wf;

static int dmc_check_common(int64_t B, int32_t n_dim, double tau) {
    if (B < 0 || n_dim < 2 || n_dim > 8 || !std::isfinite(tau) || !(tau > 0.0)) return WF_ERR_INVALID;
    if (B > kDmcMaxWalkers) return WF_ERR_UNSUPPORTED;
    return WF_OK;
}

int wf_dmc_propose(const float* x_dev, const float* psi_dev, const float* grad_dev, int64_t B, int32_t n_dim, float box, double tau,
                   int32_t limit_drift, uint64_t seed, uint64_t step, float* x_new_dev, int32_t* flag_dev, float* chi_dev, void* stream) {
    const int rc = dmc_check_common(B, n_dim, tau);
    if (rc) return rc;
    if (!std::isfinite(box) || !(box > 0.0f)) return WF_ERR_INVALID;
    if (B == 0) return WF_OK;
    if (!x_dev || !psi_dev || !grad_dev || !x_new_dev || !flag_dev) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    const DmcParams p{tau, std::sqrt(tau), 0.0, box, limit_drift != 0, (unsigned long long)seed, (unsigned long long)step, nullptr};
    return launch_dmc_propose(x_dev, psi_dev, grad_dev, B, n_dim, p, x_new_dev, flag_dev, chi_dev, stream);
}

int64_t wf_dmc_accept_workspace_bytes(int64_t B) {
    if (B < 0) return WF_ERR_INVALID;
    if (B > kDmcMaxWalkers) return WF_ERR_UNSUPPORTED;
    return dmc_accept_ws_bytes(B);
}

int wf_dmc_accept(float* x_dev, float* psi_dev, float* grad_dev, float* e_loc_dev, const float* x_new_dev, const float* psi_new_dev,
                  const float* grad_new_dev, const float* hdiag_new_dev, const int32_t* flag_dev, int64_t B, int32_t n_dim,
                  const float* protons_host, int32_t n_protons, double tau, int32_t limit_drift, double e_cut, const double* e_trial_dev,
                  uint64_t seed, uint64_t step, double* w_dev, double* record_dev, double* logA_dev, float* u_dev, int32_t* accepted_dev,
                  void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const int rc = dmc_check_common(B, n_dim, tau);
    if (rc) return rc;
    Protons pr{};
    if (!make_protons(protons_host, n_protons, &pr) || !std::isfinite(e_cut) || e_cut < 0.0) return WF_ERR_INVALID;
    if (B == 0) return WF_OK;
    if (!x_dev || !psi_dev || !grad_dev || !e_loc_dev || !x_new_dev || !psi_new_dev || !grad_new_dev || !hdiag_new_dev || !flag_dev || !e_trial_dev ||
        !w_dev || !record_dev)
        return WF_ERR_INVALID;
    if (!workspace_dev || workspace_bytes < dmc_accept_ws_bytes(B)) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    const DmcParams p{tau, std::sqrt(tau), e_cut, 0.0f, limit_drift != 0, (unsigned long long)seed, (unsigned long long)step, nullptr};
    return launch_dmc_accept(x_dev, psi_dev, grad_dev, e_loc_dev, x_new_dev, psi_new_dev, grad_new_dev, hdiag_new_dev, flag_dev, B, n_dim, pr, p,
                             e_trial_dev, w_dev, record_dev, logA_dev, u_dev, accepted_dev, 0, workspace_dev, stream);
}

int64_t wf_dmc_reconfigure_workspace_bytes(int64_t B, int32_t n_dim) {
    if (B < 0 || n_dim < 2 || n_dim > 8) return WF_ERR_INVALID;
    if (B > kDmcMaxWalkers) return WF_ERR_UNSUPPORTED;
    return B == 0 ? 0 : dmc_comb_layout(B, n_dim).total;
}

int wf_dmc_reconfigure(float* x_dev, float* psi_dev, float* grad_dev, float* e_loc_dev, double* w_dev, int64_t B, int32_t n_dim, uint64_t seed,
                       uint64_t step, int32_t* src_dev, uint64_t* stats_dev, uint64_t* status_dev, void* workspace_dev, int64_t workspace_bytes,
                       void* stream) {
    const int rc = dmc_check_common(B, n_dim, 1.0);
    if (rc) return rc;
    if (B == 0) return WF_OK;
    if (!x_dev || !psi_dev || !grad_dev || !e_loc_dev || !w_dev) return WF_ERR_INVALID;
    if (!workspace_dev || workspace_bytes < dmc_comb_layout(B, n_dim).total) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    const DmcParams p{1.0, 1.0, 0.0, 0.0f, 0, (unsigned long long)seed, (unsigned long long)step, nullptr};
    return launch_dmc_reconfigure(x_dev, psi_dev, grad_dev, e_loc_dev, w_dev, B, n_dim, p, 2, src_dev, (unsigned long long*)stats_dev,
                                  (unsigned long long*)status_dev, workspace_dev, stream);
}

}  // extern "C"
