// wf_kernels_dmc_observe.hip -- forward walking behind the comb (include/waveflow_dmc_observe.h states the rule): the genealogy of n_slots
// tagged generations, and per lag the integer histograms and the fp64 moments of V_en and V_ee over the ancestors' configurations.
//
// Four launches per call, every one of them in every call; each reads the generation g on the device and decides from it (a captured
// sequence serves stride > 1):
//   k_fw_compose  (walker blocks x slots)   tmp[s][k] = anc[s][clamp(src[k])] for the non-empty slots, into the workspace; the marks of the
//                                           distinct-ancestor count and its counters zeroed; when measuring, the series row zeroed and the
//                                           measurement number copied for the last launch
//   k_fw_measure  (walker blocks x lags)    the accumulation of wf_accum.h for one lag per workgroup: lag 0 reads x, the workgroups of slot s
//                                           read snap[s][tmp[s][k]] and mark tmp[s][k] as seen; LDS histograms as uint32 (a block sees at
//                                           most 2^20 / 1024 * 28 increments per bin), block partials in the workspace
//   k_fw_store    (walker blocks x slots)   anc <- tmp; when measuring: the marks counted (integers), and slot s* retagged: snap <- x, anc <- k
//   k_fw_reduce   (one workgroup per lag)   the partials in block order -> sums and counts, the series row, tag[s*] <- g, measurements + 1
// The fp64 sums are formed in the one order of the project (wf_accum.h), per lag over the walker index k.  The potentials are those of
// wf_eloc.h (local_values with psi = 1 and no derivatives: the terms that are not asked for fold away).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "wf_dmc_observe.h"
#include "wf_eloc.h"

namespace wf {

namespace {

using u64 = unsigned long long;
constexpr u64 kFwEmpty = WF_DMC_FW_EMPTY;
constexpr int kFwCopySlot = WF_DMC_FW_MAX_SLOTS;   // word of the `distinct` area that holds the measurement number of this call

struct FwGeom {
    HistGeom h;
    int n_slots, stride, series_len;
};

// the lag slot s serves in generation g, or -1 (empty, tagged in the future, or a lag outside 1 .. n_slots)
__device__ __forceinline__ int served_lag(u64 tag, u64 g, const FwGeom& q) {
    if (tag == kFwEmpty || g < tag) return -1;
    const u64 j = (g - tag) / (u64)q.stride;
    return j >= 1 && j <= (u64)q.n_slots ? (int)j : -1;
}

__global__ __launch_bounds__(kDmcBlock) void k_fw_compose(const int32_t* __restrict__ src, int64_t B, const int32_t* __restrict__ anc,
                                                          const u64* __restrict__ tag, int32_t* __restrict__ tmp, unsigned char* __restrict__ mark,
                                                          u64* __restrict__ distinct, const u64* __restrict__ gen, const u64* __restrict__ measurements,
                                                          double* __restrict__ series, const FwGeom q) {
    const int s = blockIdx.y, tid = threadIdx.x;
    if (blockIdx.x == 0 && s == 0) {
        if (tid < WF_DMC_FW_MAX_SLOTS) distinct[tid] = 0ull;
        if (gen[0] % (u64)q.stride == 0) {
            const u64 m = measurements[0];
            if (tid == 0) distinct[kFwCopySlot] = m;
            double* row = series + (size_t)(m % (u64)q.series_len) * (q.n_slots + 1) * WF_DMC_FW_SERIES;
            for (int i = tid; i < (q.n_slots + 1) * WF_DMC_FW_SERIES; i += kDmcBlock) row[i] = 0.0;
        }
    }
    const int64_t k = (int64_t)blockIdx.x * kDmcBlock + tid;
    if (k >= B) return;
    mark[(int64_t)s * B + k] = 0;
    if (tag[s] == kFwEmpty) return;
    int64_t j = src ? (int64_t)src[k] : k;
    j = j < 0 ? 0 : j > B - 1 ? B - 1 : j;
    tmp[(int64_t)s * B + k] = anc[(int64_t)s * B + j];
}

template <int D>
__global__ __launch_bounds__(kObsBlock) void k_fw_measure(const float* __restrict__ xg, const float* __restrict__ snap, int64_t B,
                                                          const int32_t* __restrict__ tmp, const u64* __restrict__ tag,
                                                          unsigned char* __restrict__ mark, const u64* __restrict__ gen, const Protons pr,
                                                          const FwGeom q, u64* __restrict__ partial, u64* __restrict__ density, u64* __restrict__ pair) {
    extern __shared__ unsigned int hist[];   // [D][nd] density, then [np] pair
    const u64 g = gen[0];
    if (g % (u64)q.stride != 0) return;   // (uniform over the grid)
    const int y = blockIdx.y, tid = threadIdx.x;
    int lag = 0;
    const float* cfg = xg;
    const int32_t* idx = nullptr;
    unsigned char* seen = nullptr;
    if (y > 0) {
        lag = served_lag(tag[y - 1], g, q);
        if (lag < 0) return;   // (uniform over the block)
        cfg = snap + (int64_t)(y - 1) * B * D;
        idx = tmp + (int64_t)(y - 1) * B;
        seen = mark + (int64_t)(y - 1) * B;
    }
    hist_clear(hist, D * q.h.nd + q.h.np);
    double s[kFwSums] = {0.0, 0.0, 0.0, 0.0};
    u64 n_ok = 0, n_skip = 0, out_d = 0, out_p = 0;
    const float zero[D] = {};
    for (int64_t k = (int64_t)blockIdx.x * kObsBlock + tid; k < B; k += (int64_t)gridDim.x * kObsBlock) {
        int64_t a = k;
        if (idx) {
            a = (int64_t)idx[k];
            a = a < 0 ? 0 : a > B - 1 ? B - 1 : a;   // (anc of a tagged slot is in range; the clamp keeps a caller's mistake inside the arrays)
            seen[a] = 1;                             // (every writer stores the same byte)
        }
        float x[D];
        bool fin = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            x[d] = cfg[a * D + d];
            fin = fin && isfinite(x[d]);
        }
        if (!fin) {
            n_skip += 1;
            continue;
        }
        float v[WF_OBSERVE_SCALARS];
        local_values<D>(x, 1.0f, zero, zero, pr, v);   // V_en = v[3], V_ee = v[4]: the rule of waveflow_observe.h (wf_eloc.h)
        n_ok += 1;
        const double en = (double)v[3], ee = (double)v[4];
        s[0] += en;
        s[1] += en * en;
        s[2] += ee;
        s[3] += ee * ee;
        hist_add<D>(x, q.h, hist, out_d, out_p);
    }
    const u64 c[kFwCounts] = {n_ok, n_skip, out_d, out_p};
    block_partial<kFwSums, kFwCounts>(s, c, kFwSums, partial + ((int64_t)y * gridDim.x + blockIdx.x) * kFwPartial);
    hist_flush<D>(hist, q.h, density + (int64_t)lag * D * q.h.nd, pair + (int64_t)lag * q.h.np);   // the lag's 64-bit histograms
}

template <int D>
__global__ __launch_bounds__(kDmcBlock) void k_fw_store(const float* __restrict__ xg, int64_t B, int32_t* __restrict__ anc, float* __restrict__ snap,
                                                        const u64* __restrict__ tag, const int32_t* __restrict__ tmp,
                                                        const unsigned char* __restrict__ mark, u64* __restrict__ distinct,
                                                        const u64* __restrict__ gen, const FwGeom q) {
    __shared__ u64 redc[kDmcBlock / 64];
    const u64 g = gen[0];
    const bool measuring = g % (u64)q.stride == 0;   // (uniform over the grid)
    const int s = blockIdx.y, tid = threadIdx.x;
    const int s_star = (int)((g / (u64)q.stride) % (u64)q.n_slots);
    const int64_t k = (int64_t)blockIdx.x * kDmcBlock + tid;
    u64 c = 0;
    if (k < B) {
        const int64_t at = (int64_t)s * B + k;
        if (measuring) c = mark[at];
        if (measuring && s == s_star) {
            anc[at] = (int32_t)k;
#pragma unroll
            for (int d = 0; d < D; ++d) snap[at * D + d] = xg[k * D + d];
        } else if (tag[s] != kFwEmpty) {
            anc[at] = tmp[at];
        }
    }
    if (!measuring) return;
    c = wave_sum(c);
    if ((tid & 63) == 0) redc[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
        u64 t = 0;
        for (int w = 0; w < kDmcBlock / 64; ++w) t += redc[w];
        if (t) atomicAdd(&distinct[s], t);   // (an integer sum: no order to depend on)
    }
}

// One workgroup per lag slot y (0: the current walkers; s + 1: slot s).  Thread k < 8 adds column k of the slot's block partials in block
// order (reduce_columns), then adds it to the accumulator of the lag the slot serves and writes the series row.
__global__ __launch_bounds__(kObsBlock) void k_fw_reduce(const u64* __restrict__ partial, int n_blocks, int64_t B, u64* __restrict__ tag,
                                                         const u64* __restrict__ distinct, double* __restrict__ sums, u64* __restrict__ counts,
                                                         double* __restrict__ series, u64* __restrict__ measurements, const u64* __restrict__ gen,
                                                         const FwGeom q) {
    const u64 g = gen[0];
    if (g % (u64)q.stride != 0) return;   // (uniform over the grid)
    const int y = blockIdx.x, k = threadIdx.x;
    const int lag = y == 0 ? 0 : served_lag(tag[y - 1], g, q);   // (uniform over the block)
    __syncthreads();                                             // every thread holds the old tag before thread 0 replaces it (below)
    if (lag >= 0) {
        const Column col = reduce_columns<kFwPartial>(partial + (int64_t)y * n_blocks * kFwPartial, n_blocks, kFwPartial, kFwSums);
        const double t = col.sum;
        const u64 c = col.count;
        double* row = series + ((size_t)(distinct[kFwCopySlot] % (u64)q.series_len) * (q.n_slots + 1) + lag) * WF_DMC_FW_SERIES;
        if (k < 4) {
            sums[lag * 4 + k] += t;
            if ((k & 1) == 0) row[k >> 1] = t;   // sum V_en, sum V_ee of this measurement
        } else if (k < kFwPartial) {
            counts[lag * WF_DMC_FW_COUNTS + (k - 4)] += c;
            if (k == 4) row[2] = (double)c;
        } else if (k == kFwPartial) {
            row[3] = y == 0 ? (double)B : (double)distinct[y - 1];
        }
    }
    if (k == 0) {
        if (y - 1 == (int)((g / (u64)q.stride) % (u64)q.n_slots)) tag[y - 1] = g;   // the retag (k_fw_store wrote snap and anc)
        if (y == 0) measurements[0] = distinct[kFwCopySlot] + 1ull;
    }
}

#define WF_FW_CASES(X) X(2) X(3) X(4) X(5) X(6) X(7) X(8)

}  // namespace

int dmc_fw_check(const wf_dmc_fw* fw) {
    if (!fw || fw->n_slots < 1 || fw->n_slots > WF_DMC_FW_MAX_SLOTS || fw->stride < 1 || fw->series_len < 1) return WF_ERR_INVALID;
    // (a range that is no range is refused in front of bins beyond the limits, unlike wf_observe_accumulate: the header's order)
    if (!hist_range_ok(fw->lo, fw->hi)) return WF_ERR_INVALID;
    if (!fw->snap_dev || !fw->anc_dev || !fw->tag_dev || !fw->counts_dev || !fw->sums_dev || !fw->measurements_dev || !fw->series_dev)
        return WF_ERR_INVALID;
    return hist_check(fw->n_density_bins, fw->n_pair_bins, fw->lo, fw->hi, fw->density_dev, fw->pair_dev);
}

int launch_dmc_fw_update(const float* x, const int32_t* src, int64_t B, int D, const Protons& pr, const wf_dmc_fw* fw, const u64* generation,
                         void* ws, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const FwGeom q{make_hist_geom(fw->n_density_bins, fw->n_pair_bins, fw->lo, fw->hi), fw->n_slots, fw->stride, fw->series_len};
    const DmcFwLayout l = dmc_fw_layout(B, q.n_slots);
    char* base = (char*)ws;
    int32_t* tmp = (int32_t*)(base + l.anc);
    unsigned char* mark = (unsigned char*)(base + l.mark);
    u64 *partial = (u64*)(base + l.partials), *distinct = (u64*)(base + l.distinct);
    u64 *tag = (u64*)fw->tag_dev, *counts = (u64*)fw->counts_dev, *density = (u64*)fw->density_dev, *pair = (u64*)fw->pair_dev;
    u64* measurements = (u64*)fw->measurements_dev;
    const int n_blocks = (int)observe_blocks(B);
    const dim3 lanes((unsigned)((B + kDmcBlock - 1) / kDmcBlock), (unsigned)q.n_slots);
    const dim3 lags((unsigned)n_blocks, (unsigned)(q.n_slots + 1));
    const size_t lds = ((size_t)D * q.h.nd + q.h.np) * sizeof(unsigned int);
    hipLaunchKernelGGL(k_fw_compose, lanes, dim3(kDmcBlock), 0, st, src, B, (const int32_t*)fw->anc_dev, (const u64*)tag, tmp, mark, distinct,
                       generation, (const u64*)measurements, fw->series_dev, q);
#define WF_FW_X(DD)                                                                                                                           \
    case DD:                                                                                                                                  \
        hipLaunchKernelGGL(k_fw_measure<DD>, lags, dim3(kObsBlock), lds, st, x, (const float*)fw->snap_dev, B, (const int32_t*)tmp,            \
                           (const u64*)tag, mark, generation, pr, q, partial, density, pair);                                                 \
        hipLaunchKernelGGL(k_fw_store<DD>, lanes, dim3(kDmcBlock), 0, st, x, B, fw->anc_dev, fw->snap_dev, (const u64*)tag, (const int32_t*)tmp, \
                           (const unsigned char*)mark, distinct, generation, q);                                                              \
        break;
    switch (D) {
        WF_FW_CASES(WF_FW_X)
        default:
            return WF_ERR_INVALID;
    }
#undef WF_FW_X
    hipLaunchKernelGGL(k_fw_reduce, dim3((unsigned)(q.n_slots + 1)), dim3(kObsBlock), 0, st, (const u64*)partial, n_blocks, B, tag,
                       (const u64*)distinct, fw->sums_dev, counts, fw->series_dev, measurements, generation, q);
    return launch_status();
}

}  // namespace wf

extern "C" {

using namespace wf;

int64_t wf_dmc_fw_workspace_bytes(int64_t B, int32_t n_dim, int32_t n_slots) {
    if (B < 0 || n_dim < 2 || n_dim > 8 || n_slots < 1 || n_slots > WF_DMC_FW_MAX_SLOTS) return WF_ERR_INVALID;
    if (B > kDmcMaxWalkers) return WF_ERR_UNSUPPORTED;
    return B == 0 ? 0 : dmc_fw_layout(B, n_slots).total;
}

int wf_dmc_fw_update(const float* x_dev, const int32_t* src_dev, int64_t B, int32_t n_dim, const float* protons_host, int32_t n_protons,
                     const wf_dmc_fw* fw, const uint64_t* generation_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    Protons pr{};
    if (B < 0 || n_dim < 2 || n_dim > 8 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    const int rc = dmc_fw_check(fw);
    if (rc) return rc;
    if (B == 0) return WF_OK;
    if (B > kDmcMaxWalkers) return WF_ERR_UNSUPPORTED;
    if (!x_dev || !generation_dev) return WF_ERR_INVALID;
    if (!workspace_dev || workspace_bytes < dmc_fw_layout(B, fw->n_slots).total) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return launch_dmc_fw_update(x_dev, src_dev, B, n_dim, pr, fw, (const unsigned long long*)generation_dev, workspace_dev, stream);
}

}  // extern "C"
