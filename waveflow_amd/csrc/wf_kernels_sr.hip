// wf_kernels_sr.hip -- stochastic reconfiguration in its B x B ("minSR") form from per-walker Jacobian rows (include/waveflow_sr.h):
//     Tbar = H (O O^T) H / B        wf_sr_gram    fp64 matrix cores, P split into chunks, fixed-order reduce, centring on the B x B matrix
//     (Tbar + lambda I) y = rhs     wf_sr_solve   blocked right-looking Cholesky (32-column panels), forward solve fused into the panels
//     out = scale O^T (H y)         wf_sr_apply   one pass over the rows, fp64 slab partials, fixed-order reduce
// and the two row passes SPRING (include/waveflow_sr_spring.h) adds:
//     q = O v                       wf_sr_matvec      one pass over the rows, fp64, one workgroup per row
//     out = mu prev + scale O^T (H y)   wf_sr_apply_add   the same apply: its reduce adds mu prev before its one rounding (wf_sr_apply: no prev)
// Model-free, like wf_adam_step: kernels and their host entry points live in this one unit.  Nothing here adds with atomics, and every
// sum has one order that depends on (B, P) alone: the three results are bitwise reproducible.
//
// v_mfma_f64_16x16x4_f64: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15] (one double each); of the four results of a lane,
// number r is D[(l >> 4) + 4 r][l & 15] -- not the layout of the other MFMA shapes.  A wave owns a 32 x 32 piece of a 64 x 64 block tile
// (2 x 2 products, 16 accumulator doubles per lane).  Rows and columns that do not exist are never read: the loads are predicated and
// the missing operands are zeros made in registers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/waveflow_sr_spring.h"
#include "wf_internal.h"
#include "wf_sr_common.h"

namespace wf {

using d4 = __attribute__((ext_vector_type(4))) double;

constexpr int kSrTile = 64;       // rows of O per block tile of the Gram matrix / of the trailing update
constexpr int kSrKs = 32;         // columns of O staged in LDS per step
constexpr int kSrLds = 36;        // LDS row stride in floats: 16-byte rows, and the 16 rows x 4 columns a wave reads per product hit 64 banks
constexpr int kSrNb = 32;         // Cholesky panel width
constexpr int64_t kSrMaxSolve = 4096;

// How wf_sr_gram cuts its work for (B, P): block tiles on or below the diagonal, and P chunks (a multiple of the K step) so that about
// a thousand blocks exist even at B = 128; one chunk where the tiles alone fill the device.
struct GramPlan {
    int nside, ntiles, nsplit;
    int64_t chunk;
};
static GramPlan gram_plan(int64_t B, int64_t P) {
    GramPlan g;
    g.nside = (int)((B + kSrTile - 1) / kSrTile);
    g.ntiles = g.nside * (g.nside + 1) / 2;
    const int64_t want = std::max<int64_t>(1, 1024 / g.ntiles);
    int64_t chunk = std::max<int64_t>((P + want - 1) / want, (P + 65534) / 65535);   // (grid.y <= 65535)
    chunk = std::max<int64_t>(256, (chunk + kSrKs - 1) / kSrKs * kSrKs);
    g.chunk = chunk;
    g.nsplit = (int)((P + chunk - 1) / chunk);
    return g;
}
static int64_t gram_ws_bytes(int64_t B, int64_t P) {
    const GramPlan g = gram_plan(B, P);
    return (int64_t)g.nsplit * g.ntiles * kSrTile * kSrTile * 8 + sr_align(B * 8) + 256;
}
static int64_t solve_ws_bytes(int64_t B) { return sr_align(B * 8); }

// tile number t = bi (bi + 1) / 2 + bj  ->  (bi, bj), bi >= bj
__device__ __forceinline__ void sr_tile_of(int t, int& bi, int& bj) {
    int i = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while ((i + 1) * (i + 2) / 2 <= t) ++i;
    while (i * (i + 1) / 2 > t) --i;
    bi = i;
    bj = t - i * (i + 1) / 2;
}

// Nothing of the matrix pipe in flight when the accumulators are read behind a branch (isa_guard's second rule).
__device__ __forceinline__ void sr_drain_mfma() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

// ---- Gram matrix

// partial[split][tile][64][64] = O[tile rows bi][chunk] . O[tile rows bj][chunk]^T on the fp64 matrix cores
__global__ __launch_bounds__(256) void k_mfma_sr_gram(const float* __restrict__ rows, int64_t ld, int64_t B, int64_t P, int64_t chunk, int ntiles,
                                                      int vec, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float As[kSrTile * kSrLds];
    __shared__ __attribute__((aligned(16))) float Bs[kSrTile * kSrLds];
    int bi, bj;
    sr_tile_of((int)blockIdx.x, bi, bj);
    const int64_t p0 = (int64_t)blockIdx.y * chunk, p1 = std::min<int64_t>(P, p0 + chunk);
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wi = w >> 1, wj = w & 1;
    const int lr = tid >> 3, lc = (tid & 7) * 4;   // staging: 8 threads per row, 4 floats each, rows lr and lr + 32
    const int64_t ra = (int64_t)bi * kSrTile + lr, rb = (int64_t)bj * kSrTile + lr;
    const bool live = !(bi == bj && wj > wi);      // (the piece above the diagonal of a diagonal tile is never used)
    d4 acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
    float4 va[2], vb[2];
    for (int h = 0; h < 2; ++h) {
        va[h] = sr_load4(rows, ld, ra + 32 * h, B, p0 + lc, p1, vec != 0);
        vb[h] = sr_load4(rows, ld, rb + 32 * h, B, p0 + lc, p1, vec != 0);
    }
    const float* ap = As + (wi * 32 + (lane & 15)) * kSrLds + (lane >> 4);
    const float* bp = Bs + (wj * 32 + (lane & 15)) * kSrLds + (lane >> 4);
    for (int64_t k0 = p0; k0 < p1; k0 += kSrKs) {
        __syncthreads();   // the products of the step before have read the tiles
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<float4*>(As + (lr + 32 * h) * kSrLds + lc) = va[h];
            *reinterpret_cast<float4*>(Bs + (lr + 32 * h) * kSrLds + lc) = vb[h];
        }
        __syncthreads();
        if (k0 + kSrKs < p1) {   // the next step's rows, in flight under this step's products
            for (int h = 0; h < 2; ++h) {
                va[h] = sr_load4(rows, ld, ra + 32 * h, B, k0 + kSrKs + lc, p1, vec != 0);
                vb[h] = sr_load4(rows, ld, rb + 32 * h, B, k0 + kSrKs + lc, p1, vec != 0);
            }
        }
        if (live) {
#pragma unroll
            for (int kk = 0; kk < kSrKs / 4; ++kk) {
                const double a0 = (double)ap[kk * 4], a1 = (double)ap[16 * kSrLds + kk * 4];
                const double b0 = (double)bp[kk * 4], b1 = (double)bp[16 * kSrLds + kk * 4];
                acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
    }
    sr_drain_mfma();
    if (!live) return;
    double* out = partial + ((int64_t)blockIdx.y * ntiles + blockIdx.x) * (kSrTile * kSrTile);
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int r = 0; r < 4; ++r)
                out[(wi * 32 + a * 16 + (lane >> 4) + 4 * r) * kSrTile + wj * 32 + b * 16 + (lane & 15)] = acc[a][b][r];
}

// Both copies of a tile's entries on or below the diagonal: G[gi][gj] straight (coalesced along gj), G[gj][gi] through an LDS transpose
// (coalesced along gi).  val(r, c, gi, gj) is called once per existing entry with gi >= gj; a thread covers column c = tid & 63 of
// rows (tid >> 6) + 4 i.
template <typename F>
__device__ __forceinline__ void sr_store_sym(double* __restrict__ G, int64_t B, int bi, int bj, F val) {
    __shared__ double tr[kSrTile][kSrTile + 1];
    const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    for (int i = 0; i < 16; ++i) {
        const int r = r0 + 4 * i;
        const int64_t gi = (int64_t)bi * kSrTile + r, gj = (int64_t)bj * kSrTile + c;
        double v = 0.0;
        if (gi < B && gj < B && gi >= gj) {
            v = val(r, c, gi, gj);
            G[gi * B + gj] = v;
        }
        tr[r][c] = v;
    }
    __syncthreads();
    for (int i = 0; i < 16; ++i) {
        const int rr = r0 + 4 * i;   // row inside tile bj, column c inside tile bi
        const int64_t gi = (int64_t)bi * kSrTile + c, gj = (int64_t)bj * kSrTile + rr;
        if (gi < B && gj < B && gi > gj) G[gj * B + gi] = tr[c][rr];
    }
}

// G = sum of the chunk partials, split 0 first
__global__ __launch_bounds__(256) void k_sr_gram_reduce(const double* __restrict__ partial, int nsplit, int ntiles, int64_t B, double* __restrict__ G) {
    int bi, bj;
    sr_tile_of((int)blockIdx.x, bi, bj);
    const double* src = partial + (int64_t)blockIdx.x * (kSrTile * kSrTile);
    const int64_t step = (int64_t)ntiles * (kSrTile * kSrTile);
    sr_store_sym(G, B, bi, bj, [&](int r, int c, int64_t, int64_t) {
        double s = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) s += src[sp * step + r * kSrTile + c];
        return s;
    });
}

// rowsum[i] = sum_j G[i][j]
__global__ __launch_bounds__(256) void k_sr_rowsum(const double* __restrict__ G, int64_t B, double* __restrict__ rowsum) {
    __shared__ double red[256];
    const int64_t i = blockIdx.x;
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < B; j += 256) s += G[i * B + j];
    s = sr_block_sum(s, red);
    if (threadIdx.x == 0) rowsum[i] = s;
}

// total[0] = sum_i rowsum[i]
__global__ __launch_bounds__(256) void k_sr_total(const double* __restrict__ rowsum, int64_t B, double* __restrict__ total) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t j = threadIdx.x; j < B; j += 256) s += rowsum[j];
    s = sr_block_sum(s, red);
    if (threadIdx.x == 0) total[0] = s;
}

// Tbar = (G[i][j] - (mean_i + mean_j) + mean) / B, in place, both copies from the entry on or below the diagonal
__global__ __launch_bounds__(256) void k_sr_gram_centre(double* __restrict__ G, int64_t B, const double* __restrict__ rowsum, const double* __restrict__ total) {
    int bi, bj;
    sr_tile_of((int)blockIdx.x, bi, bj);
    const double n = (double)B, mean = total[0] / (n * n);
    sr_store_sym(G, B, bi, bj, [&](int, int, int64_t gi, int64_t gj) { return ((G[gi * B + gj] - (rowsum[gi] / n + rowsum[gj] / n)) + mean) / n; });
}

// ---- Cholesky solve

// lambda = damping_abs + damping_rel trace / B onto the diagonal; z = rhs; info = 0
__global__ __launch_bounds__(256) void k_sr_shift(double* __restrict__ T, int64_t B, const double* __restrict__ rhs, double damping_abs, double damping_rel,
                                                  double* __restrict__ z, int32_t* __restrict__ info) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += 256) s += T[i * B + i];
    s = sr_block_sum(s, red);
    const double lambda = damping_abs + damping_rel * s / (double)B;
    for (int64_t i = threadIdx.x; i < B; i += 256) {
        T[i * B + i] += lambda;
        z[i] = rhs[i];
    }
    if (threadIdx.x == 0) info[0] = 0;
}

// The diagonal block of panel j0 in LDS, the right-hand side as its 33rd row: L11 in place, z[j0 ..] = L11^-1 z[j0 ..].  A pivot that is
// not positive (NaN included) ends the factorisation: info = its 1-based index, nothing is written back.
__global__ __launch_bounds__(64) void k_sr_potrf(double* __restrict__ T, int64_t B, int64_t j0, double* __restrict__ z, int32_t* __restrict__ info) {
    if (info[0] != 0) return;
    __shared__ double L[kSrNb + 1][kSrNb + 1];
    const int tid = threadIdx.x;
    const int nb = (int)std::min<int64_t>(kSrNb, B - j0);
    for (int idx = tid; idx < (kSrNb + 1) * kSrNb; idx += 64) {
        const int r = idx / kSrNb, c = idx % kSrNb;
        double v = r == c ? 1.0 : 0.0;   // (a short last panel is padded with the identity)
        if (r < kSrNb) {
            if (r < nb && c <= r) v = T[(j0 + r) * B + j0 + c];
        } else {
            v = c < nb ? z[j0 + c] : 0.0;
        }
        L[r][c] = v;
    }
    __syncthreads();
    int bad = 0;
    for (int k = 0; k < nb; ++k) {
        const double d = L[k][k];   // the same value in every thread: the branch is uniform
        if (!(d > 0.0)) {
            bad = k + 1;
            break;
        }
        const double s = sqrt(d);
        __syncthreads();
        double l = 0.0;
        if (tid == k) {
            L[k][k] = s;
        } else if (tid > k && tid <= kSrNb) {
            l = L[tid][k] / s;
            L[tid][k] = l;
        }
        __syncthreads();
        if (tid > k && tid <= kSrNb) {
            const int cmax = std::min(tid, kSrNb - 1);
            for (int c = k + 1; c <= cmax; ++c) L[tid][c] -= l * L[c][k];
        }
        __syncthreads();
    }
    if (bad) {
        if (tid == 0) info[0] = (int32_t)(j0 + bad);
        return;
    }
    for (int idx = tid; idx < kSrNb * kSrNb; idx += 64) {
        const int r = idx / kSrNb, c = idx % kSrNb;
        if (r < nb && c <= r) T[(j0 + r) * B + j0 + c] = L[r][c];
    }
    if (tid < nb) z[j0 + tid] = L[kSrNb][tid];
}

// Rows below the panel, one per thread: L21 = A21 L11^-T, then the row's right-hand side: z[i] -= L21[i] . z[panel]
__global__ __launch_bounds__(64) void k_sr_trsm(double* __restrict__ T, int64_t B, int64_t j0, double* __restrict__ z, const int32_t* __restrict__ info) {
    if (info[0] != 0) return;
    __shared__ double L[kSrNb][kSrNb + 1];
    __shared__ double zs[kSrNb];
    const int tid = threadIdx.x;
    for (int idx = tid; idx < kSrNb * kSrNb; idx += 64) {
        const int r = idx / kSrNb, c = idx % kSrNb;
        L[r][c] = c <= r ? T[(j0 + r) * B + j0 + c] : 0.0;   // (rows exist below this panel, so it is a full one)
    }
    if (tid < kSrNb) zs[tid] = z[j0 + tid];
    __syncthreads();
    const int64_t i = j0 + kSrNb + (int64_t)blockIdx.x * 64 + tid;
    if (i >= B) return;
    double* row = T + i * B + j0;
    double x[kSrNb];
#pragma unroll
    for (int c = 0; c < kSrNb; ++c) x[c] = row[c];
#pragma unroll
    for (int k = 0; k < kSrNb; ++k) {
        double s = x[k];
#pragma unroll
        for (int m = 0; m < k; ++m) s -= x[m] * L[k][m];
        x[k] = s / L[k][k];
    }
    double u = 0.0;
#pragma unroll
    for (int c = 0; c < kSrNb; ++c) {
        row[c] = x[c];
        u += x[c] * zs[c];
    }
    z[i] -= u;
}

// Trailing update on the fp64 matrix cores: A22 -= L21 L21^T, entries on or below the diagonal only
__global__ __launch_bounds__(256) void k_mfma_sr_syrk(double* __restrict__ T, int64_t B, int64_t j0, const int32_t* __restrict__ info) {
    if (info[0] != 0) return;
    int bi, bj;
    sr_tile_of((int)blockIdx.x, bi, bj);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wi = w >> 1, wj = w & 1;
    if (bi == bj && wj > wi) return;
    const int64_t q0 = j0 + kSrNb;
    const int64_t ri = q0 + (int64_t)bi * kSrTile + wi * 32 + (lane & 15), rj = q0 + (int64_t)bj * kSrTile + wj * 32 + (lane & 15);
    d4 acc[2][2];
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < kSrNb / 4; ++kk) {
        const int64_t col = j0 + kk * 4 + (lane >> 4);
        const double a0 = ri < B ? T[ri * B + col] : 0.0, a1 = ri + 16 < B ? T[(ri + 16) * B + col] : 0.0;
        const double b0 = rj < B ? T[rj * B + col] : 0.0, b1 = rj + 16 < B ? T[(rj + 16) * B + col] : 0.0;
        acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    sr_drain_mfma();
    for (int a = 0; a < 2; ++a)
        for (int b = 0; b < 2; ++b)
            for (int r = 0; r < 4; ++r) {
                const int64_t gi = q0 + (int64_t)bi * kSrTile + wi * 32 + a * 16 + (lane >> 4) + 4 * r;
                const int64_t gj = q0 + (int64_t)bj * kSrTile + wj * 32 + b * 16 + (lane & 15);
                if (gi < B && gj < B && gi >= gj) T[gi * B + gj] -= acc[a][b][r];
            }
}

// Back substitution, right-looking, last panel first: y[panel] = L11^-T z[panel] (every block, block 0 stores it), then the columns left of
// the panel: z[c] -= sum_k L[j0 + k][c] y[j0 + k].  After a bad pivot y is NaN.
__global__ __launch_bounds__(256) void k_sr_back(const double* __restrict__ T, int64_t B, int64_t j0, double* __restrict__ z, double* __restrict__ y,
                                                 const int32_t* __restrict__ info) {
    const int tid = threadIdx.x;
    const int nb = (int)std::min<int64_t>(kSrNb, B - j0);
    if (info[0] != 0) {
        if (blockIdx.x == 0 && tid < nb) y[j0 + tid] = __builtin_nan("");
        return;
    }
    __shared__ double L[kSrNb][kSrNb + 1];
    __shared__ double ys[kSrNb];
    for (int idx = tid; idx < kSrNb * kSrNb; idx += 256) {
        const int r = idx / kSrNb, c = idx % kSrNb;
        double v = r == c ? 1.0 : 0.0;
        if (r < nb && c <= r) v = T[(j0 + r) * B + j0 + c];
        L[r][c] = v;
    }
    double zt = tid < nb ? z[j0 + tid] : 0.0;
    __syncthreads();
    for (int k = kSrNb - 1; k >= 0; --k) {
        if (tid == k) ys[k] = zt / L[k][k];
        __syncthreads();
        if (tid < k) zt -= L[k][tid] * ys[k];
    }
    if (blockIdx.x == 0 && tid < nb) y[j0 + tid] = ys[tid];
    const int64_t c = (int64_t)blockIdx.x * 256 + tid;
    if (c < j0) {
        double u = 0.0;
        for (int k = 0; k < nb; ++k) u += T[(j0 + k) * B + c] * ys[k];
        z[c] -= u;
    }
}

// ---- apply

// yc = y - mean y
__global__ __launch_bounds__(256) void k_sr_ycentre(const double* __restrict__ y, int64_t B, double* __restrict__ yc) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < B; i += 256) s += y[i];
    s = sr_block_sum(s, red);
    const double mean = s / (double)B;
    for (int64_t i = threadIdx.x; i < B; i += 256) yc[i] = y[i] - mean;
}

// partial[slab][p] = sum over the 32 rows of the slab, first row first, of yc[b] rows[b][p]; four columns per thread
__global__ __launch_bounds__(256) void k_sr_apply(const float* __restrict__ rows, int64_t ld, int64_t B, int64_t P, int vec, const double* __restrict__ yc,
                                                  double* __restrict__ partial) {
    __shared__ double ys[kSrSlab];
    const int64_t b0 = (int64_t)blockIdx.y * kSrSlab;
    if (threadIdx.x < kSrSlab) ys[threadIdx.x] = b0 + threadIdx.x < B ? yc[b0 + threadIdx.x] : 0.0;
    __syncthreads();
    const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= P) return;
    const int nr = (int)std::min<int64_t>(kSrSlab, B - b0);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll 8
    for (int r = 0; r < nr; ++r) {
        const float4 v = sr_load4(rows, ld, b0 + r, B, c, P, vec != 0);
        const double w = ys[r];
        a0 += w * (double)v.x;
        a1 += w * (double)v.y;
        a2 += w * (double)v.z;
        a3 += w * (double)v.w;
    }
    double* out = partial + (int64_t)blockIdx.y * P + c;
    out[0] = a0;
    if (c + 1 < P) out[1] = a1;
    if (c + 2 < P) out[2] = a2;
    if (c + 3 < P) out[3] = a3;
}

// out[p] = (float)(mu prev[p] + scale * sum of the slab partials, slab 0 first); prev == nullptr or mu == 0: (float)(scale * sum).  out may be prev.
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

// the three launches of wf_sr_apply and wf_sr_apply_add (arguments checked by the entries)
static int sr_apply(const float* rows, int64_t B, int64_t P, int64_t ld, const double* y, double scale, const float* prev, double mu, float* out, void* ws,
                    void* stream) {
    hipStream_t s = (hipStream_t)stream;
    double* yc = (double*)ws;
    double* partial = (double*)((char*)ws + sr_align(B * 8));
    const int64_t nslab = (B + kSrSlab - 1) / kSrSlab;
    hipLaunchKernelGGL(k_sr_ycentre, dim3(1), dim3(256), 0, s, y, B, yc);
    hipLaunchKernelGGL(k_sr_apply, dim3((unsigned)((P + 1023) / 1024), (unsigned)nslab), dim3(256), 0, s, rows, ld, B, P, (int)sr_vec_ok(rows, ld),
                       (const double*)yc, partial);
    hipLaunchKernelGGL(k_sr_apply_add_reduce, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, (const double*)partial, nslab, P, scale, prev, mu, out);
    return sr_finish();
}

// ---- matvec

// q[b] = sum_p rows[b][p] v[p]: one workgroup per row; thread t takes columns 4 t .. 4 t + 3, then + 1024, ... into four fp64 sums (one per
// column of its group, every product exact in fp64), ((s0 + s1) + (s2 + s3)), then the tree over the 256 threads
__global__ __launch_bounds__(256) void k_sr_matvec(const float* __restrict__ rows, int64_t ld, int64_t B, int64_t P, int vec, const float* __restrict__ v, int vvec,
                                                   double* __restrict__ q) {
    __shared__ double red[256];
    const int64_t b = blockIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll 4
    for (int64_t c = (int64_t)threadIdx.x * 4; c < P; c += 4 * 256) {
        const float4 r = sr_load4(rows, ld, b, B, c, P, vec != 0);
        const float4 w = sr_load4(v, 0, 0, 1, c, P, vvec != 0);
        s0 += (double)r.x * (double)w.x;
        s1 += (double)r.y * (double)w.y;
        s2 += (double)r.z * (double)w.z;
        s3 += (double)r.w * (double)w.w;
    }
    const double s = sr_block_sum((s0 + s1) + (s2 + s3), red);
    if (threadIdx.x == 0) q[b] = s;
}

}  // namespace wf

using namespace wf;

extern "C" {

int64_t wf_sr_workspace_bytes(int64_t B, int64_t P) {
    if (B < 1 || P < 1) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    return std::max(gram_ws_bytes(B, P), std::max(solve_ws_bytes(B), apply_ws_bytes(B, P)));
}

int wf_sr_gram(const float* rows_dev, int64_t B, int64_t P, int64_t ld, double* t_dev, void* workspace_dev, int64_t workspace_bytes,
               void* stream) {
    if (B < 1 || P < 1 || ld < P || !rows_dev || !t_dev || !workspace_dev) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    if (workspace_bytes < gram_ws_bytes(B, P)) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    const GramPlan g = gram_plan(B, P);
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace_dev;
    double* rowsum = partial + (int64_t)g.nsplit * g.ntiles * kSrTile * kSrTile;
    double* total = (double*)((char*)rowsum + sr_align(B * 8));
    hipLaunchKernelGGL(k_mfma_sr_gram, dim3((unsigned)g.ntiles, (unsigned)g.nsplit), dim3(256), 0, s, rows_dev, ld, B, P, g.chunk, g.ntiles,
                       (int)sr_vec_ok(rows_dev, ld), partial);
    hipLaunchKernelGGL(k_sr_gram_reduce, dim3((unsigned)g.ntiles), dim3(256), 0, s, partial, g.nsplit, g.ntiles, B, t_dev);
    hipLaunchKernelGGL(k_sr_rowsum, dim3((unsigned)B), dim3(256), 0, s, t_dev, B, rowsum);
    hipLaunchKernelGGL(k_sr_total, dim3(1), dim3(256), 0, s, rowsum, B, total);
    hipLaunchKernelGGL(k_sr_gram_centre, dim3((unsigned)g.ntiles), dim3(256), 0, s, t_dev, B, rowsum, total);
    return sr_finish();
}

int wf_sr_solve(double* t_dev, int64_t B, const double* rhs_dev, double damping_abs, double damping_rel, double* y_dev, int32_t* info_dev,
                void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (B < 1 || !t_dev || !rhs_dev || !y_dev || !info_dev || !workspace_dev) return WF_ERR_INVALID;
    if (!(damping_abs >= 0.0) || !(damping_rel >= 0.0)) return WF_ERR_INVALID;
    if (B > kSrMaxSolve) return WF_ERR_UNSUPPORTED;
    if (workspace_bytes < solve_ws_bytes(B)) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    double* z = (double*)workspace_dev;
    hipLaunchKernelGGL(k_sr_shift, dim3(1), dim3(256), 0, s, t_dev, B, rhs_dev, damping_abs, damping_rel, z, info_dev);
    for (int64_t j0 = 0; j0 < B; j0 += kSrNb) {
        hipLaunchKernelGGL(k_sr_potrf, dim3(1), dim3(64), 0, s, t_dev, B, j0, z, info_dev);
        const int64_t below = B - j0 - kSrNb;
        if (below <= 0) break;
        hipLaunchKernelGGL(k_sr_trsm, dim3((unsigned)((below + 63) / 64)), dim3(64), 0, s, t_dev, B, j0, z, (const int32_t*)info_dev);
        const int64_t side = (below + kSrTile - 1) / kSrTile;
        hipLaunchKernelGGL(k_mfma_sr_syrk, dim3((unsigned)(side * (side + 1) / 2)), dim3(256), 0, s, t_dev, B, j0, (const int32_t*)info_dev);
    }
    for (int64_t j0 = (B - 1) / kSrNb * kSrNb; j0 >= 0; j0 -= kSrNb)
        hipLaunchKernelGGL(k_sr_back, dim3((unsigned)std::max<int64_t>(1, (j0 + 255) / 256)), dim3(256), 0, s, (const double*)t_dev, B, j0, z, y_dev,
                           (const int32_t*)info_dev);
    return sr_finish();
}

int wf_sr_apply(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const double* y_dev, double scale, float* out_dev,
                void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (B < 1 || P < 1 || ld < P || !rows_dev || !y_dev || !out_dev || !workspace_dev) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    if (workspace_bytes < apply_ws_bytes(B, P)) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return sr_apply(rows_dev, B, P, ld, y_dev, scale, nullptr, 0.0, out_dev, workspace_dev, stream);
}

int wf_sr_apply_add(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const double* y_dev, double scale, const float* prev_dev, double mu,
                    float* out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (B < 1 || P < 1 || ld < P || !rows_dev || !y_dev || !out_dev || !workspace_dev) return WF_ERR_INVALID;
    if (!(mu >= 0.0) || !(mu < 1.0)) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    if (workspace_bytes < apply_ws_bytes(B, P)) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return sr_apply(rows_dev, B, P, ld, y_dev, scale, prev_dev, mu, out_dev, workspace_dev, stream);
}

int wf_sr_matvec(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const float* v_dev, double* q_dev, void* stream) {
    if (B < 1 || P < 1 || ld < P || !rows_dev || !v_dev || !q_dev) return WF_ERR_INVALID;
    if (B > kSrMaxRows) return WF_ERR_UNSUPPORTED;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    hipLaunchKernelGGL(k_sr_matvec, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, rows_dev, ld, B, P, (int)sr_vec_ok(rows_dev, ld), v_dev,
                       (int)sr_vec_ok(v_dev, 0), q_dev);
    return sr_finish();
}

}  // extern "C"
