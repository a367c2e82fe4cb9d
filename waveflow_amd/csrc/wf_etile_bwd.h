// wf_etile_bwd.h -- parameter gradients of the two-particle matrix-core path: the reverse helpers and the reverse kernel k_ebwd<PRIOR, NBK>.
// Included by wf_kernels_etile_bwd.hip (k_ebwd<., 1>, the reductions, the host side) and by wf_etile_bwd_k2.hip (k_ebwd<., 2> under the max-ilp
// scheduling strategy).
// The adjoint header first: its head algebra is compiled WITHOUT the contraction pragma of wf_etile_common.h (included by wf_etile_cond.h) -- with
// it the reverse kernel came out 10 % slower, 189 instead of 138 spilled registers: profiles/r04_grad33_times.txt, "adjoint header under fp contract".
// Everything behind it is compiled with contraction.
#pragma once
#include <hip/hip_runtime.h>

#include "wf_etile_adjoint.h"
#include "wf_etile_cond.h"

namespace wf {
namespace {

// ============================================================================ parameter gradients on the matrix cores (vqmc.py:193-221)
// grad[p] = sum_b ( w_psi[b] d psi_b / d theta_p + w_lap[b] d laplacian_b / d theta_p ) for the two-particle family (<= 64 bases: NBK = 1 or 2 row blocks per dimension), batch by batch:
//   k_efused (st_out)   forward, leaves the (u_0, u_1, log det) jets at the input of every net
//   k_ebwd<PRIOR>       one launch per net, last net first: recomputes the net's forward from its input jets, pulls the adjoint of its output
//                       jets back through the head algebra (wf_etile_adjoint.h) to adjoint head triples, through the conditioner with TRANSPOSED
//                       operand images on the matrix cores (three channels, like the forward), writes the adjoint of the net's input jets for the
//                       next launch -- and, since round 4, forms the weight-gradient products dW[k][u] = sum_walkers sum_channels X_c[k][w] Y_c[u][w]
//                       itself.  The walker axis is the K of that product, while every tensor of the sweep has the walker on the LANE (accumulator
//                       layout): the operands are transposed ON THE MATRIX CORES -- an fp16 fragment times a 0/1 permutation operand is an exact
//                       transposition, one v_mfma per K step (tr_frag) -- and the six 32 x 32 blocks of (dW1, dW2) accumulate in LDS, one private set
//                       per wave (24 KB; the four sets + the operand images fill the 160 KB), summed over the workgroup's waves in wave order at the
//                       end: one 25.6 KB block of partial sums per workgroup.  Tiles are dealt to the waves statically, so the sums -- and whole
//                       training runs -- stay bitwise reproducible.  Rounds 2 - 3 dumped the operands per tile (66 KB: 270 MB per net and 2^17
//                       walkers) for a second kernel (k_ewgrad) that read them back: ~2 GB of HBM traffic per call against ~27 MB algorithmic.
//                       One wave per SIMD (512 registers).
//   k_egrad_reduce, k_egrad_scatter   reduction over the workgroups' blocks (fixed order); scales and folds back to the flat leaf order
__device__ __forceinline__ float wave_max(float v) {   // v >= 0
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)));
    const unsigned u = __float_as_uint(v);
    const auto sw = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return xhalf_max(fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1])));
}
__device__ __forceinline__ int exponent_of(float amax) { return amax > 0.0f ? __builtin_amdgcn_frexp_expf(amax) : 0; }
using JA = adj::Jt<float>;
using TA = adj::T2t<float>;
constexpr int kBwdWaves = 4;
// Gradient block of a net (floats, in the units of the MFMA image; NBK = 32-row blocks of the head per dimension):
//   GW0 [64] (d / d W0'[0][u]), Gb0 [64], GW1 [64][64] (k, u), Gb1 [64], GW2 [64][32 NBK] (k, row), Gb2 of dimension 1 [32 NBK], of dimension 0 [32 NBK]
template <int NBK>
struct GL {
    static constexpr int W0 = 0, b0 = 64, W1 = 128, b1 = 4224, W2 = 4288, b21 = W2 + 2048 * NBK, b20 = b21 + 32 * NBK, floats = b20 + 32 * NBK;
};
constexpr int g_floats(int nbk) { return 4288 + 2048 * nbk + 64 * nbk; }
static_assert(GL<1>::floats == g_floats(1) && GL<2>::floats == g_floats(2), "gradient block layout");
constexpr int kESplit = 256;        // partial blocks per net: one per workgroup of k_ebwd (grid <= 256), summed in block order by k_egrad_reduce
// LDS accumulators of a workgroup: blocks 0..3 = dW1 (k block mb = b >> 1, u block nb = b & 1), 4.. = dW2 (k block (b - 4) / NBK, row block (b - 4) % NBK),
// each [4 q][64 lanes][4] (register 4 q + e of the lane: one conflict-free ds_read_b128 per q)
constexpr int acc_blocks(int nbk) { return 4 + 2 * nbk; }
// sets of accumulator blocks per workgroup.  One row block: a private set per wave (4 x 24 KB beside 66 KB of images), summed in wave order at the end.
// Two row blocks: the four private sets (128 KB) do not fit beside 103 KB of images -- ONE shared set filled in tile order (acc_add).  Sharing
// the set for one row block too was measured: 1.040 ms per loss + gradient of 2^17 walkers against 0.985 ms (the waves move in step, one add apart:
// any jitter of one holds up the other three); profiles/r04_grad33_times.txt
constexpr int acc_sets(int nbk) { return nbk == 1 ? kBwdWaves : 1; }
__device__ __forceinline__ int acc_rho(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }   // row of register r in lane half h (accumulator layout)
__device__ __forceinline__ f32x16 acc_load(const float* aw, int b, int lane) {
    f32x16 a;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(aw + ((b * 4 + q) * 64 + lane) * 4);
        a[4 * q] = v[0]; a[4 * q + 1] = v[1]; a[4 * q + 2] = v[2]; a[4 * q + 3] = v[3];
    }
    return a;
}
__device__ __forceinline__ void acc_store(float* aw, int b, int lane, const f32x16& a) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x4*>(aw + ((b * 4 + q) * 64 + lane) * 4) = f32x4{a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
}
// B operand of the transposition product: P[K = (s, khalf, i)][n] = 1 where the K slot holds row n (K slot (s, h, i) of a fragment = register 8 s + i of half h)
__device__ __forceinline__ void make_perm(int lane, f16x8 (&pm)[2]) {
    const int n = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 8; ++i) pm[s][i] = acc_rho(8 * s + i, h) == n ? (_Float16)1.0f : (_Float16)0.0f;
}
__device__ __forceinline__ f16x8 cvt8(const f32x16& d, int s) {
    using f32x2 = __attribute__((ext_vector_type(2))) float;
    f16x8 o;
#pragma unroll
    for (int i = 0; i < 8; i += 2) {
        const f16x2 pr = __builtin_convertvector((f32x2){d[8 * s + i], d[8 * s + i + 1]}, f16x2);
        o[i] = pr[0]; o[i + 1] = pr[1];
    }
    return o;
}
// One 32-row block X (accumulator layout: lane = walker, registers = rows) given as fp16 fragments (hi, lo) -> X^T as fp16 fragments with the ROW on the
// lane and the walkers in the registers (walker acc_rho(r, half) in register r): D[walker][row] = sum_K frag[walker][K] P[K][row] has one non-zero term
// per entry, so hi and lo come through exactly.  rowsum (may be null): += the sum over the lane's 16 walkers of hi + lo (both halves: xhalf at the end).
__device__ __forceinline__ void tr_frag(const Frag& f, const f16x8 (&pm)[2], Frag& t, float* rowsum = nullptr) {
    f32x16 dh = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, dl = dh;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        dh = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.hi[s], pm[s], dh, 0, 0, 0);
        dl = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.lo[s], pm[s], dl, 0, 0, 0);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) { t.hi[s] = cvt8(dh, s); t.lo[s] = cvt8(dl, s); }
    if (rowsum) {
        float a = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) a += dh[r] + dl[r];
        *rowsum += a;
    }
}
__device__ __forceinline__ float half32_sum(float v) {   // sum over the 32 lanes of this lane's half, in every lane of it
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));    // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));    // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));   // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));   // row_mirror
    const unsigned u = __float_as_uint(v);
    const auto sw = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __uint_as_float(sw[0]) + __uint_as_float(sw[1]);
}
__device__ __forceinline__ JA ja_load(const float* __restrict__ st, int slot, int64_t B, int64_t w) {
    const float* p = st + (int64_t)slot * 4 * B + w;
    return JA{p[0], p[B], p[2 * B], p[3 * B]};
}
__device__ __forceinline__ void ja_store(float* __restrict__ st, int slot, int64_t B, int64_t w, JA x) {
    float* p = st + (int64_t)slot * 4 * B + w;
    p[0] = x.v; p[B] = x.a; p[2 * B] = x.b; p[3 * B] = x.h;
}
// Fragments of ADJOINT tensors.  UNI: one power of two per (TILE, channel) instead of per (walker, channel) -- the wave's largest.  The adjoint tensors
// of the reverse kernel take it: what they feed are sums over walkers (the weight gradients; the input adjoints, which the next net's reverse again only
// sums), so a walker far below the tile's largest loses bits that do not show in any sum, and the same fragments serve as operands of the products over
// the walker axis, which need one scale per tile.
// two blocks, every channel scaled (adjoints are unbounded in every channel)
template <bool UNI = false>
__device__ __forceinline__ void to_frags_all(const f32x16 (&blk0)[NCH], const f32x16 (&blk1)[NCH], Frag (&f)[NCH][2], int (&e)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        float amax = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fmaxf(fabsf(blk0[c][r]), fabsf(blk1[c][r])));
        e[c] = UNI ? exponent_of(wave_max(amax)) : col_exponent(amax);
        const float sc = __builtin_amdgcn_ldexpf(1.0f, -e[c]);
#pragma unroll
        for (int ob = 0; ob < 2; ++ob)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float r8[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) r8[jj] = (ob == 0 ? blk0[c][8 * s + jj] : blk1[c][8 * s + jj]) * sc;
                split8(r8, f[c][ob].hi[s], f[c][ob].lo[s]);
            }
    }
}
// the NBK row blocks of the adjoint head triples -> fragments [channel][row block] (the K steps of the product with W2'), one power of two per (tile, channel)
template <int NBK>
__device__ __forceinline__ void to_frags_kb(const f32x16 (&blk)[NBK][NCH], Frag (&f)[NCH][2], int (&e)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        float amax = 0.0f;
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb)
#pragma unroll
            for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(blk[kb][c][r]));
        e[c] = exponent_of(wave_max(amax));
        const float sc = __builtin_amdgcn_ldexpf(1.0f, -e[c]);
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float r8[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) r8[jj] = blk[kb][c][8 * s + jj] * sc;
                split8(r8, f[c][kb].hi[s], f[c][kb].lo[s]);
            }
    }
}
__device__ __forceinline__ void unscale_all(f32x16 (&acc)[NCH], const int (&e)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const float sc = __builtin_amdgcn_ldexpf(1.0f, e[c]);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[c][r] = acc[c][r] * sc;
    }
}
// (x, x', x'') and the adjoint of (r, r' x', r' x'' + r'' x'^2) -> adjoint of (x, x', x''), in place in g
__device__ __forceinline__ void act_block_bwd(const f32x16 (&x)[NCH], f32x16 (&g)[NCH]) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float a, b, c;
        adj::r_triple_bwd(r_of(x[0][r]), x[1][r], x[2][r], g[0][r], g[1][r], g[2][r], a, b, c);
        g[0][r] = a; g[1][r] = b; g[2][r] = c;
    }
}
// extended row sums of a flow head over the lane's 16 rows (dimension 1: triples from the conditioner; CONST: dimension 0, (bias, 0, 0))
template <bool CONST>
__device__ __forceinline__ void flow_rows_ext(adj::FlowSumsT<float>& a, const f32x16 (&o)[NCH], const f32x16& g16, const float* __restrict__ tabI, int mesh_stride,
                                              const int* bnd, const LerpN& L, int kb, int h) {
    // the records of chunk q + 1 are requested before the rows of chunk q are worked on (two sets of 4 + 4 records in flight: the compiler's own order
    // waited for every set right behind its request -- one exposed L2 round trip per chunk)
    float4_t tq[2][2][4];
    chunk_rows<4>(tabI, mesh_stride, bnd, L, 8 * kb + h, tq[0][0], tq[0][1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < 3) chunk_rows<4>(tabI, mesh_stride, bnd, L, 8 * kb + 2 * (q + 1) + h, tq[(q + 1) & 1][0], tq[(q + 1) & 1][1]);
        const float4_t (&ta)[4] = tq[q & 1][0], (&tb)[4] = tq[q & 1][1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * q + e;
            float v0, v1 = 0.0f, v2 = 0.0f;
            if (CONST) v0 = r_of(o[0][r]);
            else adj::r_triple(r_of(o[0][r]), o[1][r], o[2][r], v0, v1, v2);
            const float g = g16[r];
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = __builtin_fmaf(tb[k][e] - ta[k][e], L.t, ta[k][e]) * g;
            a.s[0] += v0; a.qv[0] = __builtin_fmaf(v0, g, a.qv[0]);
#pragma unroll
            for (int k = 0; k < 4; ++k) { a.v0[k] = __builtin_fmaf(v0, t[k], a.v0[k]); a.r[k] += t[k]; }
            if (!CONST) {
                a.s[1] += v1; a.s[2] += v2;
                a.qv[1] = __builtin_fmaf(v1, g, a.qv[1]); a.qv[2] = __builtin_fmaf(v2, g, a.qv[2]);
#pragma unroll
                for (int k = 0; k < 4; ++k) a.v1[k] = __builtin_fmaf(v1, t[k], a.v1[k]);
#pragma unroll
                for (int k = 0; k < 3; ++k) a.v2[k] = __builtin_fmaf(v2, t[k], a.v2[k]);
            }
        }
    }
}
__device__ __forceinline__ void flow_sums_xhalf(adj::FlowSumsT<float>& a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { a.s[k] = xhalf_sum(a.s[k]); a.qv[k] = xhalf_sum(a.qv[k]); a.v2[k] = xhalf_sum(a.v2[k]); }
#pragma unroll
    for (int k = 0; k < 4; ++k) { a.r[k] = xhalf_sum(a.r[k]); a.v0[k] = xhalf_sum(a.v0[k]); a.v1[k] = xhalf_sum(a.v1[k]); }
}
// adjoint head triples of the lane's rows from the adjoints of the row sums (ab: summed over the halves already, the same in both)
template <bool CONST>
__device__ __forceinline__ void flow_rows_bwd(const adj::FlowSumsT<float>& ab, const f32x16 (&o)[NCH], const f32x16& g16, const float* __restrict__ tabI,
                                              int mesh_stride, const int* bnd, const LerpN& L, int kb, int h, f32x16 (&ob)[NCH]) {
    // the records of chunk q + 1 are requested before the rows of chunk q are worked on (two sets of 4 + 4 records in flight: the compiler's own order
    // waited for every set right behind its request -- one exposed L2 round trip per chunk)
    float4_t tq[2][2][4];
    chunk_rows<4>(tabI, mesh_stride, bnd, L, 8 * kb + h, tq[0][0], tq[0][1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < 3) chunk_rows<4>(tabI, mesh_stride, bnd, L, 8 * kb + 2 * (q + 1) + h, tq[(q + 1) & 1][0], tq[(q + 1) & 1][1]);
        const float4_t (&ta)[4] = tq[q & 1][0], (&tb)[4] = tq[q & 1][1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * q + e;
            const float g = g16[r];
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = __builtin_fmaf(tb[k][e] - ta[k][e], L.t, ta[k][e]) * g;
            float vb0 = __builtin_fmaf(g, ab.qv[0], ab.s[0]);
#pragma unroll
            for (int k = 0; k < 4; ++k) vb0 = __builtin_fmaf(ab.v0[k], t[k], vb0);
            const float rr = r_of(o[0][r]);
            if (CONST) {
                ob[0][r] = vb0 * adj::r_derivs(rr).r1;
                ob[1][r] = 0.0f; ob[2][r] = 0.0f;
            } else {
                float vb1 = __builtin_fmaf(g, ab.qv[1], ab.s[1]), vb2 = __builtin_fmaf(g, ab.qv[2], ab.s[2]);
#pragma unroll
                for (int k = 0; k < 3; ++k) vb1 = __builtin_fmaf(ab.v1[k], t[k], vb1);
#pragma unroll
                for (int k = 0; k < 2; ++k) vb2 = __builtin_fmaf(ab.v2[k], t[k], vb2);
                float x0b, x1b, x2b;
                adj::r_triple_bwd(rr, o[1][r], o[2][r], vb0, vb1, vb2, x0b, x1b, x2b);
                ob[0][r] = x0b; ob[1][r] = x1b; ob[2][r] = x2b;
            }
        }
    }
}
// the prior's rows: extended sums from the triples of c (CONST: channel 0 only), and back
template <bool CONST>
__device__ __forceinline__ void prior_rows_ext(adj::PriorSumsT<float>& a, const f32x16 (&c)[NCH], const float* __restrict__ tabP, int mesh_stride, const int* bnd,
                                               const LerpN& L, int kb, int h) {
    // the records of chunk q + 1 are requested before the rows of chunk q are worked on (two sets of 4 + 4 records in flight: the compiler's own order
    // waited for every set right behind its request -- one exposed L2 round trip per chunk)
    float4_t tq[2][2][4];
    chunk_rows<4>(tabP, mesh_stride, bnd, L, 8 * kb + h, tq[0][0], tq[0][1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < 3) chunk_rows<4>(tabP, mesh_stride, bnd, L, 8 * kb + 2 * (q + 1) + h, tq[(q + 1) & 1][0], tq[(q + 1) & 1][1]);
        const float4_t (&ta)[4] = tq[q & 1][0], (&tb)[4] = tq[q & 1][1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * q + e;
            const float c0 = c[0][r];
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) t[k] = __builtin_fmaf(tb[k][e] - ta[k][e], L.t, ta[k][e]);
#pragma unroll
            for (int k = 0; k < 4; ++k) a.d0[k] = __builtin_fmaf(c0, t[k], a.d0[k]);
            a.cc = __builtin_fmaf(c0, c0, a.cc);
            if (!CONST) {
                const float c1 = c[1][r], c2 = c[2][r];
#pragma unroll
                for (int k = 0; k < 3; ++k) a.d1[k] = __builtin_fmaf(c1, t[k], a.d1[k]);
                a.d2[0] = __builtin_fmaf(c2, t[0], a.d2[0]); a.d2[1] = __builtin_fmaf(c2, t[1], a.d2[1]);
                a.cc1 = __builtin_fmaf(c0, c1, a.cc1); a.c1c1 = __builtin_fmaf(c1, c1, a.c1c1); a.cc2 = __builtin_fmaf(c0, c2, a.cc2);
            }
        }
    }
}
__device__ __forceinline__ void prior_sums_xhalf(adj::PriorSumsT<float>& a) {
#pragma unroll
    for (int k = 0; k < 4; ++k) a.d0[k] = xhalf_sum(a.d0[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) a.d1[k] = xhalf_sum(a.d1[k]);
    a.d2[0] = xhalf_sum(a.d2[0]); a.d2[1] = xhalf_sum(a.d2[1]);
    a.cc = xhalf_sum(a.cc); a.cc1 = xhalf_sum(a.cc1); a.c1c1 = xhalf_sum(a.c1c1); a.cc2 = xhalf_sum(a.cc2);
}
template <bool CONST>
__device__ __forceinline__ void prior_rows_bwd(const adj::PriorSumsT<float>& ab, const f32x16 (&c)[NCH], const float* __restrict__ tabP, int mesh_stride,
                                               const int* bnd, const LerpN& L, int kb, int h, f32x16 (&cb)[NCH]) {
    // the records of chunk q + 1 are requested before the rows of chunk q are worked on (two sets of 3 + 3 records in flight: the compiler's own order
    // waited for every set right behind its request -- one exposed L2 round trip per chunk)
    float4_t tq[2][2][3];
    chunk_rows<3>(tabP, mesh_stride, bnd, L, 8 * kb + h, tq[0][0], tq[0][1]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (q < 3) chunk_rows<3>(tabP, mesh_stride, bnd, L, 8 * kb + 2 * (q + 1) + h, tq[(q + 1) & 1][0], tq[(q + 1) & 1][1]);
        const float4_t (&ta)[3] = tq[q & 1][0], (&tb)[3] = tq[q & 1][1];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int r = 4 * q + e;
            float t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = __builtin_fmaf(tb[k][e] - ta[k][e], L.t, ta[k][e]);
            const float c0 = c[0][r];
            float b0 = 2.0f * ab.cc * c0;
#pragma unroll
            for (int k = 0; k < 3; ++k) b0 = __builtin_fmaf(ab.d0[k], t[k], b0);
            if (CONST) {
                cb[0][r] = b0; cb[1][r] = 0.0f; cb[2][r] = 0.0f;
            } else {
                const float c1 = c[1][r], c2 = c[2][r];
                cb[0][r] = b0 + ab.cc1 * c1 + ab.cc2 * c2;
                cb[1][r] = ab.d1[0] * t[0] + ab.d1[1] * t[1] + ab.cc1 * c0 + 2.0f * ab.c1c1 * c1;
                cb[2][r] = ab.d2[0] * t[0] + ab.cc2 * c0;
            }
        }
    }
}
// NB blocks of triples -> fragments [block][channel], one power of two per (walker, channel) over the NB blocks (the operand of a product over the ROWS)
template <int NB>
__device__ __forceinline__ void to_frags_n(const f32x16 (&blk)[NB][NCH], Frag (&f)[NB][NCH], int (&e)[NCH]) {
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        float amax = 0.0f;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(blk[b][c][r]));
        e[c] = col_exponent(amax);
        const float sc = __builtin_amdgcn_ldexpf(1.0f, -e[c]);
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                float r8[8];
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) r8[jj] = blk[b][c][8 * s + jj] * sc;
                split8(r8, f[b][c].hi[s], f[b][c].lo[s]);
            }
    }
}
// ... of one channel
template <int NB>
__device__ __forceinline__ void to_frags_n1(const f32x16 (&blk)[NB], Frag (&f)[NB], int& e) {
    float amax = 0.0f;
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(blk[b][r]));
    e = col_exponent(amax);
    const float sc = __builtin_amdgcn_ldexpf(1.0f, -e);
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float r8[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) r8[jj] = blk[b][8 * s + jj] * sc;
            split8(r8, f[b].hi[s], f[b].lo[s]);
        }
}
// block ko of w @ M for ONE channel (M's image as prior_c_block takes it: [ko][ki]{hi 1024, lo 1024})
template <int NBK>
__device__ __forceinline__ void c_block1(const _Float16* obh, const Frag (&wf)[NBK], int e, int ko, int lane, f32x16& out) {
    f32x16 acc = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ki = 0; ki < NBK; ++ki)
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const _Float16* blk = obh + (size_t)(ko * NBK + ki) * 2048;
            const f16x8 ah = *reinterpret_cast<const f16x8*>(blk + (s * 64 + lane) * 8);
            const f16x8 al = *reinterpret_cast<const f16x8*>(blk + 1024 + (s * 64 + lane) * 8);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, wf[ki].hi[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wf[ki].lo[s], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, wf[ki].hi[s], acc, 0, 0, 0);
        }
    const float sc = __builtin_amdgcn_ldexpf(1.0f, e);
#pragma unroll
    for (int r = 0; r < 16; ++r) out[r] = acc[r] * sc;
}

// forward of one conditioner from its input (u0, u1) to the second hidden layer's pre-activation triples z2 (two 32-unit blocks).  HEAD: on to the head
// triples o (NBK row blocks).
template <bool HEAD, int NBK>
__device__ __forceinline__ void cond_fwd(const float* net, float u0v, float u1v, int lane, f32x16 (&z2a)[NCH], f32x16 (&z2b)[NCH], f32x16 (&o)[NBK][NCH]) {
    Frag f2[NCH][2];
    int e2[NCH];
    using O = NetOff<2, NBK>;
    const int h = lane >> 5;
    const float in0[2] = {u0v, 1.0f}, in1[2] = {u1v, 0.0f};
    f32x16 a0[NCH], a1[NCH];
    init_acc(a0, net + O::b0 + (0 * 2 + h) * 16);
    init_acc(a1, net + O::b0 + (1 * 2 + h) * 16);
    const float w0 = net[O::W0 + 0 * 64 + lane], w1 = net[O::W0 + 1 * 64 + lane];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        a0[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, h ? in1[c] : in0[c], a0[c], 0, 0, 0);
        a1[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, h ? in1[c] : in0[c], a1[c], 0, 0, 0);
    }
    act_block(a0);
    act_block(a1);
    to_frags(a0, a1, f2, e2);
    const _Float16* W1h = reinterpret_cast<const _Float16*>(net + O::W1h);
    const _Float16* W1l = reinterpret_cast<const _Float16*>(net + O::W1l);
    init_acc(z2a, net + O::b1 + (0 + h) * 16);
    init_acc(z2b, net + O::b1 + (2 + h) * 16);
    dense64_block<NCH>(W1h, W1l, f2, z2a, lane);
    dense64_block<NCH>(W1h + 2048, W1l + 2048, f2, z2b, lane);
    unscale(z2a, e2);
    unscale(z2b, e2);
    if (HEAD) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) { a0[c] = z2a[c]; a1[c] = z2b[c]; }
        act_block(a0);
        act_block(a1);
        to_frags(a0, a1, f2, e2);
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb) cond_out<NBK>(net, f2, e2, kb, lane, o[kb]);
    }
}
// X operand of a product over the walker axis: one 32-unit block of ACTIVATION jets (channel 0 = r in (0, 1)) -> fragments scaled by 2^-ex[c], one power
// of two per (tile, channel).  ey[c]: the exponents of the other operand's channels.  All three channels' products are to land in ONE accumulator
// chain, so the channels share the product's exponent E = max_c (natural exponent of X_c + ey[c]) and X_c is scaled by 2^-(E - ey[c]) -- at most its
// natural scale; a channel whose product lies below the largest one's loses bits that the sum does not see.  Returns E.
__device__ __forceinline__ int block_frags_x(const f32x16 (&blk)[NCH], const int (&ey)[NCH], Frag (&f)[NCH]) {
    int en[NCH];
    en[0] = 0;
#pragma unroll
    for (int c = 1; c < NCH; ++c) {
        float amax = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) amax = fmaxf(amax, fabsf(blk[c][r]));
        en[c] = exponent_of(wave_max(amax));
    }
    const int E = max(en[0] + ey[0], max(en[1] + ey[1], en[2] + ey[2]));
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const float sc = __builtin_amdgcn_ldexpf(1.0f, ey[c] - E);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float r8[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) r8[jj] = blk[c][8 * s + jj] * sc;
            split8(r8, f[c].hi[s], f[c].lo[s]);
        }
    }
    return E;
}
__device__ __forceinline__ void mfma3(f32x16& p, const f16x8& xh, const f16x8& xl, const f16x8& yh, const f16x8& yl) {
    p = __builtin_amdgcn_mfma_f32_32x32x16_f16(xl, yh, p, 0, 0, 0);
    p = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, yl, p, 0, 0, 0);
    p = __builtin_amdgcn_mfma_f32_32x32x16_f16(xh, yh, p, 0, 0, 0);
}
// one channel's product block over the 32 walkers of the tile: p += A (x) B (both K steps, three split products each)
__device__ __forceinline__ void wgrad_block(f32x16& p, const Frag& xt, const Frag& yt) {
#pragma unroll
    for (int s = 0; s < 2; ++s) mfma3(p, xt.hi[s], xt.lo[s], yt.hi[s], yt.lo[s]);
}
// block b of the workgroup's accumulators += p * un, in TILE ORDER: the tiles of a workgroup are numbered k = 0, 1, .. (tile = block + k * grid, wave
// k % waves), ticket[b] counts the tiles whose product has been added to block b, and tile k's wave adds when the count stands at k.  The sum of every
// block is therefore formed in the same order whatever the timing (bitwise reproducible gradients) although the waves share ONE set of blocks.  Progress:
// tile k waits only for tile k - 1's wave to pass the same point, tile 0 for nobody; the waves of a workgroup are resident together and each works
// through its tiles in increasing k, so every wait ends (the waves fall into step one add apart: ~200 cycles in a tile of ~10^5).
template <bool SHARED>
__device__ __forceinline__ void acc_add(float* acc, int* ticket, int b, int k, int lane, const f32x16& p, float un) {
    if (SHARED) {
        // Nothing of the matrix pipe may be in flight across the branch of the wait below.  hipcc (ROCm 7.2) counts the wait states between an MFMA and a
        // vector read of its result correctly in straight-line code, but at the join behind this loop it let v_accvgpr_read follow the product's last
        // MFMA by four instructions where eleven are due (ISA of k_ebwd<true, 2>, seventh wait): when the ticket was already there the last rows of
        // the product (registers 12 .. 15) were read before the pipe had written them -- 128 entries of one gradient block changed from run to run
        // by 4e-5 relative (scratch/r04_repro_diag.py).  24 idle issue slots in front of the branch, fenced against the scheduler, retire every MFMA.
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        while (__hip_atomic_load(ticket + b, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != k) __builtin_amdgcn_s_sleep(1);
    }
    f32x16 a = acc_load(acc, b, lane);
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = __builtin_fmaf(p[r], un, a[r]);
    acc_store(acc, b, lane, a);
    if (SHARED) __hip_atomic_store(ticket + b, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

}  // namespace
// (k_ebwd has external linkage: its two-row-block instantiations are compiled in a translation unit of their own, wf_etile_bwd_k2.hip, under the
// max-ilp scheduling strategy, which is worth 6 % to them and costs the one-row-block form 1 %: DESIGN 4.9)
template <bool PRIOR, int NBK>
__global__ __launch_bounds__(kBwdWaves * 64) void k_ebwd(const MfmaDev mm, int net_index, const float* __restrict__ tabI, const float* __restrict__ tabP,
                                                          const float* __restrict__ st_in, float* __restrict__ adjb, const float* __restrict__ w_psi,
                                                          const float* __restrict__ w_lap, int64_t B, float* __restrict__ partial) {
    // partial: [gridDim.x][GL<NBK>::floats] -- this workgroup's block of the net's gradient (image units), written once at the end
    using O = NetOff<2, NBK>;
    using G = GL<NBK>;
    constexpr int kThreads = kBwdWaves * 64;
    constexpr int kMeshStride = 128 * NBK;   // floats per mesh point of the regrouped tables (k_efused)
    constexpr int kAcc = acc_blocks(NBK);
    constexpr int kSets = acc_sets(NBK);
    constexpr bool kShared = kSets == 1;
    constexpr int kKinds = 4 + 2 * NBK;      // per-lane sums: Gb1 (two unit blocks), Gb2 of dimension 1 (NBK), of dimension 0 (NBK), Gb0, GW0
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int bnd_s[32 * NBK];
    __shared__ int ticket[kAcc];
    __shared__ __attribute__((aligned(16))) float c0s[32 * NBK + 16];   // prior: c of dimension 0 ([NBK][2][16], the same for every walker), + the sum of its raw outputs
    if (threadIdx.x < 16 * NBK) bnd_s[threadIdx.x] = reinterpret_cast<const int*>(tabI + (size_t)mm.n_mesh * kMeshStride)[threadIdx.x];
    else if (threadIdx.x < 32 * NBK) bnd_s[threadIdx.x] = reinterpret_cast<const int*>(tabP + (size_t)mm.n_mesh * kMeshStride)[threadIdx.x - 16 * NBK];
    if (threadIdx.x >= 64 && threadIdx.x < 64 + kAcc) ticket[threadIdx.x - 64] = 0;
    float* net_l = lds + mm.const_floats;
    float* tnet_l = net_l + mm.net_floats;
    float* tcon_l = tnet_l + mm.tnet_floats;
    stage_floats<kThreads>(mm.image + mm.const_img_off, lds, mm.const_floats);
    stage_floats<kThreads>(mm.image + (size_t)net_index * mm.net_floats, net_l, mm.net_floats);
    stage_floats<kThreads>(mm.image + mm.timg_off + (size_t)net_index * mm.tnet_floats, tnet_l, mm.tnet_floats);
    stage_floats<kThreads>(mm.image + mm.tconst_off, tcon_l, NBK * NBK * 1024);
    // the workgroup's accumulators of (dW1, dW2) behind the images
    float* acc_all = tcon_l + NBK * NBK * 1024;
    for (int i = threadIdx.x; i < kSets * kAcc * 1024; i += kThreads) acc_all[i] = 0.0f;
    __syncthreads();
    float* acc = acc_all + (kShared ? 0 : (threadIdx.x >> 6) * kAcc * 1024);
    // bias / input-layer sums of this lane over its wave's tiles: Gb1 and Gb2 (dimension 1) of unit / row (lane & 31) of its block (transposed operands:
    // partial over the lane half's 16 walkers), Gb2 of dimension 0, Gb0, GW0 in the lane assignment of the DPP sums below
    float gb1[2] = {0.0f, 0.0f}, gb21[NBK], gb20[NBK], gb0s = 0.0f, gw0s = 0.0f;
#pragma unroll
    for (int kb = 0; kb < NBK; ++kb) { gb21[kb] = 0.0f; gb20[kb] = 0.0f; }
    f16x8 pm[2];
    make_perm(threadIdx.x & 63, pm);
    const float* net = net_l;
    const float* fkI = lds;
    const float* fkP = lds + 32 * NBK;
    const _Float16* obh = reinterpret_cast<const _Float16*>(lds + 64 * NBK);
    const float* cbP = lds + 64 * NBK + NBK * NBK * 1024 + 64 * NBK;   // [NBK][2][16] constant term of the B prior's boundary map times ob_to_b (mm.p_bias)
    const _Float16* TW1h = reinterpret_cast<const _Float16*>(tnet_l);
    const _Float16* TW1l = reinterpret_cast<const _Float16*>(tnet_l + 2048);
    const _Float16* TW2h = reinterpret_cast<const _Float16*>(tnet_l + 4096);
    const _Float16* TW2l = reinterpret_cast<const _Float16*>(tnet_l + 4096 + 1024 * NBK);
    const float* TW0 = tnet_l + 4096 + 2048 * NBK;
    const _Float16* obT = reinterpret_cast<const _Float16*>(tcon_l);
    const int lane = threadIdx.x & 63;
    const int j = lane & 31, h = lane >> 5;
    const int n_mesh = mm.n_mesh;
    const int64_t n_tiles = (B + 31) >> 5;
    if (PRIOR) {
        // dimension 0 of the prior sees the bias alone (empty mask): c = (b2 * keep) @ ob_to_b (+ the constant term) is the same for every walker
        if (threadIdx.x < 64) {
            f32x16 w0[NBK];
            float s0 = 0.0f;
#pragma unroll
            for (int kb = 0; kb < NBK; ++kb) {
                const f32x16 b20 = load16(net + O::b2 + ((0 * NBK + kb) * 2 + h) * 16), keep = load16(fkP + (kb * 2 + h) * 16);
#pragma unroll
                for (int r = 0; r < 16; ++r) { s0 += b20[r]; w0[kb][r] = b20[r] * keep[r]; }
            }
            s0 = xhalf_sum(s0);
            Frag wf[NBK];
            int e0;
            to_frags_n1<NBK>(w0, wf, e0);
#pragma unroll
            for (int ko = 0; ko < NBK; ++ko) {
                f32x16 c;
                c_block1<NBK>(obh, wf, e0, ko, lane, c);
                if (mm.p_bias) {
                    const f32x16 cbv = load16(cbP + (ko * 2 + h) * 16);
#pragma unroll
                    for (int r = 0; r < 16; ++r) c[r] = __builtin_fmaf(s0, cbv[r], c[r]);
                }
                if (j == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) c0s[(ko * 2 + h) * 16 + r] = c[r];
                }
            }
            if (lane == 0) c0s[32 * NBK] = s0;
        }
        __syncthreads();
    }
    // tiles are dealt statically (tile = block + k * grid, k = round * waves + wave): which wave sums which tiles does not depend on timing, and the
    // shared accumulator blocks take the tiles' products in the order of k (acc_add)
    int k = (int)(threadIdx.x >> 6);
    for (int64_t tile = (int64_t)blockIdx.x + (int64_t)(threadIdx.x >> 6) * gridDim.x; tile < n_tiles; tile += (int64_t)kBwdWaves * gridDim.x, k += kBwdWaves) {
        const int64_t w = tile * 32 + j;
        const bool valid = w < B;
        const int64_t wl = valid ? w : B - 1;
        // (padding lanes of the last tile repeat walker B - 1 with zero adjoints: their columns add nothing to the sums over walkers)
        const JA u0 = ja_load(st_in, 0, B, wl), u1 = ja_load(st_in, 1, B, wl);
        // ---- the net's forward to the head triples o.  The second hidden layer's pre-activations z2, which the reverse needs, are computed again
        // behind the head: 96 registers less across the head algebra
        f32x16 o[NBK][NCH];
        {
            f32x16 z2a[NCH], z2b[NCH];
            cond_fwd<true, NBK>(net, u0.v, u1.v, lane, z2a, z2b, o);
        }
        // ---- head: forward sums, pullback to adjoint head triples ob (dimension 1) and ob0 (dimension 0, channel 0)
        f32x16 ob[NBK][NCH], ob0[NBK];
        JA u0b = adj::jzero<float>(), u1b = adj::jzero<float>(), ldb = adj::jzero<float>();
        if (!PRIOR) {
            const JA y1b = valid ? ja_load(adjb, 0, B, wl) : adj::jzero<float>(), y0b = valid ? ja_load(adjb, 1, B, wl) : adj::jzero<float>();
            ldb = valid ? ja_load(adjb, 2, B, wl) : adj::jzero<float>();
            const LerpN L1 = nlerp(u1.v, n_mesh), L0 = nlerp(u0.v, n_mesh);
            // the row factors and the biases of dimension 0 (its head sees the bias alone: empty mask).  One row block: loaded once per tile and held (the
            // compiler then also hoists what depends on them alone); two row blocks: loaded where they are used -- holding 64 registers of them across the
            // head costs more than it saves there (1.550 against 1.575 ms per loss + gradient of 2^17 walkers; one block: 0.937 against 0.973 the other way)
            f32x16 g16h[NBK], o0h[NBK];
            if (NBK == 1) {
                g16h[0] = load16(fkI + h * 16);
                o0h[0] = load16(net + O::b2 + h * 16);
            }
            auto g16 = [&](int kb) { return NBK == 1 ? g16h[0] : load16(fkI + (kb * 2 + h) * 16); };
            auto bias0 = [&](int kb) { return NBK == 1 ? o0h[0] : load16(net + O::b2 + ((0 * NBK + kb) * 2 + h) * 16); };
            // dimension 0 first, then dimension 1: the two heads share nothing but the incoming adjoints, and their sums / intermediates need not be live together
            JA sb0 = adj::jzero<float>(), tb0 = adj::jzero<float>();
            float tv0 = 0.0f;
            {
                adj::FlowSumsT<float> s0 = adj::flow_sums_zero<float>();
#pragma unroll
                for (int kb = 0; kb < NBK; ++kb) {
                    f32x16 o0[NCH];
                    o0[0] = bias0(kb);
                    flow_rows_ext<true>(s0, o0, g16(kb), tabI, kMeshStride, bnd_s, L0, kb, h);
                }
                flow_sums_xhalf(s0);
                JA y0, dl0;
                const adj::FlowHeadFwd<float> f0 = adj::flow_head_fwd(s0, mm.F_I, mm.i_reg, u0, u0, y0, dl0);
                adj::FlowSumsT<float> ab0 = adj::flow_sums_zero<float>();
                adj::flow_head_bwd(s0, f0, mm.F_I, mm.i_reg, u0, u0, y0b, ldb, ab0, sb0, tb0, tv0);
#pragma unroll
                for (int kb = 0; kb < NBK; ++kb) {
                    f32x16 o0[NCH], t0[NCH];
                    o0[0] = bias0(kb);
                    flow_rows_bwd<true>(ab0, o0, g16(kb), tabI, kMeshStride, bnd_s, L0, kb, h, t0);
                    ob0[kb] = t0[0];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            JA sb = adj::jzero<float>(), tb = adj::jzero<float>();
            float tv1 = 0.0f;
            {
                adj::FlowSumsT<float> s1 = adj::flow_sums_zero<float>();
#pragma unroll
                for (int kb = 0; kb < NBK; ++kb) flow_rows_ext<false>(s1, o[kb], g16(kb), tabI, kMeshStride, bnd_s, L1, kb, h);
                flow_sums_xhalf(s1);
                JA y1, dl1;
                const adj::FlowHeadFwd<float> f1 = adj::flow_head_fwd(s1, mm.F_I, mm.i_reg, u0, u1, y1, dl1);
                adj::FlowSumsT<float> ab1 = adj::flow_sums_zero<float>();
                adj::flow_head_bwd(s1, f1, mm.F_I, mm.i_reg, u0, u1, y1b, ldb, ab1, sb, tb, tv1);
#pragma unroll
                for (int kb = 0; kb < NBK; ++kb) flow_rows_bwd<false>(ab1, o[kb], g16(kb), tabI, kMeshStride, bnd_s, L1, kb, h, ob[kb]);
            }
            u0b = JA{tv0, sb.a + sb0.a + tb0.a, sb.b + sb0.b + tb0.b, sb.h + sb0.h + tb0.h};
            u1b = JA{tv1, tb.a, tb.b, tb.h};
        } else {
            const float wp = valid ? w_psi[wl] : 0.0f, wlp = valid ? w_lap[wl] : 0.0f;
            const JA ld = ja_load(st_in, 2, B, wl);
            const JA psib = JA{wp, 0.0f, 0.0f, 2.0f * wlp};
            // dimension 1: c = (o keep) @ ob_to_b as triples (+ the constant term of a boundary constraint with a non-zero value, mm.p_bias: c += (sum o) *
            // (b @ ob_to_b), channel by channel, as k_efused<.., true>); dimension 0: c0s
            float s1 = 0.0f, sder[2] = {0.0f, 0.0f};
            f32x16 c1[NBK][NCH];
            {
                Frag of[NBK][NCH];
                int eo[NCH];
                prior_frags<NBK>(o, fkP, lane, of, eo, s1, sder);
#pragma unroll
                for (int ko = 0; ko < NBK; ++ko) {
                    prior_c_block<NBK>(obh, of, eo, ko, lane, c1[ko]);
                    if (mm.p_bias) {
                        const f32x16 cbv = load16(cbP + (ko * 2 + h) * 16);
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            c1[ko][0][r] = __builtin_fmaf(s1, cbv[r], c1[ko][0][r]);
                            c1[ko][1][r] = __builtin_fmaf(sder[0], cbv[r], c1[ko][1][r]);
                            c1[ko][2][r] = __builtin_fmaf(sder[1], cbv[r], c1[ko][2][r]);
                        }
                    }
                }
            }
            const float s0 = c0s[32 * NBK];
            const float sg1 = s1 < 0.0f ? -1.0f : 1.0f, sg0 = s0 < 0.0f ? -1.0f : 1.0f;
            const bool in0 = u0.v >= 0.0f && u0.v <= 1.0f, in1 = u1.v >= 0.0f && u1.v <= 1.0f;
            const JA uc0 = in0 ? u0 : JA{u0.v < 0.0f ? 0.0f : 1.0f, 0.0f, 0.0f, 0.0f}, uc1 = in1 ? u1 : JA{u1.v < 0.0f ? 0.0f : 1.0f, 0.0f, 0.0f, 0.0f};
            const LerpN L1 = nlerp(uc1.v, n_mesh), L0 = nlerp(uc0.v, n_mesh);
            adj::PriorSumsT<float> p1 = adj::prior_sums_zero<float>(), p0 = adj::prior_sums_zero<float>();
#pragma unroll
            for (int ko = 0; ko < NBK; ++ko) {
                prior_rows_ext<false>(p1, c1[ko], tabP, kMeshStride, bnd_s + 16 * NBK, L1, ko, h);
                f32x16 c0[NCH];
                c0[0] = load16(c0s + (ko * 2 + h) * 16);
                prior_rows_ext<true>(p0, c0, tabP, kMeshStride, bnd_s + 16 * NBK, L0, ko, h);
            }
            prior_sums_xhalf(p1);
            prior_sums_xhalf(p0);
            JA val1, val0;
            const adj::PriorHeadFwd<float> f1 = adj::prior_head_fwd(p1, sg1, u0, uc1, val1);
            const adj::PriorHeadFwd<float> f0 = adj::prior_head_fwd(p0, sg0, u0, uc0, val0);
            const float sc0 = (mm.constrained_mask & 1u) ? 0.70710678118654752f : 1.0f, sc1 = (mm.constrained_mask & 2u) ? 0.70710678118654752f : 1.0f;
            const float ev = __expf(0.5f * ld.v);
            const JA E = adj::japply(ld, ev, 0.5f * ev, 0.25f * ev);
            const JA A = val0 * sc0, Bv = val1 * sc1, P = adj::jmul(A, Bv);
            JA Pb = adj::jzero<float>(), Eb = adj::jzero<float>(), Ab = adj::jzero<float>(), Bb = adj::jzero<float>();
            adj::jmul_bwd(E, psib, Pb);
            adj::jmul_bwd(P, psib, Eb);
            adj::jfun_bwd(ld, 0.5f * ev, 0.25f * ev, 0.125f * ev, Eb, ldb);
            adj::jmul_bwd(Bv, Pb, Ab);
            adj::jmul_bwd(A, Pb, Bb);
            adj::PriorSumsT<float> ab1 = adj::prior_sums_zero<float>(), ab0 = adj::prior_sums_zero<float>();
            JA sb = adj::jzero<float>(), tb1 = adj::jzero<float>(), sb0 = adj::jzero<float>(), tb0 = adj::jzero<float>();
            float tv1 = 0.0f, tv0 = 0.0f;
            adj::prior_head_bwd(p1, f1, sg1, u0, uc1, Bb * sc1, ab1, sb, tb1, tv1);
            adj::prior_head_bwd(p0, f0, sg0, u0, uc0, Ab * sc0, ab0, sb0, tb0, tv0);
            u0b = JA{in0 ? tv0 : 0.0f, sb.a + sb0.a + (in0 ? tb0.a : 0.0f), sb.b + sb0.b + (in0 ? tb0.b : 0.0f), sb.h + sb0.h + (in0 ? tb0.h : 0.0f)};
            u1b = in1 ? JA{tv1, tb1.a, tb1.b, tb1.h} : adj::jzero<float>();
            // rows back: adjoint of c -> through ob_to_b transposed -> adjoint of the raw outputs (the constant term reaches every one of a channel's
            // raw outputs through their sum: sbar)
            {
                f32x16 cb[NBK][NCH];
                float sbar[NCH] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int ko = 0; ko < NBK; ++ko) {
                    prior_rows_bwd<false>(ab1, c1[ko], tabP, kMeshStride, bnd_s + 16 * NBK, L1, ko, h, cb[ko]);
                    if (mm.p_bias) {
                        const f32x16 cbv = load16(cbP + (ko * 2 + h) * 16);
#pragma unroll
                        for (int c = 0; c < NCH; ++c)
#pragma unroll
                            for (int r = 0; r < 16; ++r) sbar[c] = __builtin_fmaf(cb[ko][c][r], cbv[r], sbar[c]);
                    }
                }
                if (mm.p_bias) {
#pragma unroll
                    for (int c = 0; c < NCH; ++c) sbar[c] = xhalf_sum(sbar[c]);
                }
                Frag fcb[NBK][NCH];
                int ecb[NCH];
                to_frags_n<NBK>(cb, fcb, ecb);
#pragma unroll
                for (int ki = 0; ki < NBK; ++ki) {
                    f32x16 wb[NCH];
                    prior_c_block<NBK>(obT, fcb, ecb, ki, lane, wb);
                    const f32x16 keep = load16(fkP + (ki * 2 + h) * 16);
#pragma unroll
                    for (int c = 0; c < NCH; ++c)
#pragma unroll
                        for (int r = 0; r < 16; ++r) ob[ki][c][r] = __builtin_fmaf(wb[c][r], keep[r], sbar[c]);
                }
            }
            {
                f32x16 cb0[NBK];
                float sbar = 0.0f;
#pragma unroll
                for (int ko = 0; ko < NBK; ++ko) {
                    f32x16 c0[NCH], t[NCH];
                    c0[0] = load16(c0s + (ko * 2 + h) * 16);
                    prior_rows_bwd<true>(ab0, c0, tabP, kMeshStride, bnd_s + 16 * NBK, L0, ko, h, t);
                    cb0[ko] = t[0];
                    if (mm.p_bias) {
                        const f32x16 cbv = load16(cbP + (ko * 2 + h) * 16);
#pragma unroll
                        for (int r = 0; r < 16; ++r) sbar = __builtin_fmaf(cb0[ko][r], cbv[r], sbar);
                    }
                }
                if (mm.p_bias) sbar = xhalf_sum(sbar);
                Frag f0b[NBK];
                int e0b;
                to_frags_n1<NBK>(cb0, f0b, e0b);
#pragma unroll
                for (int ki = 0; ki < NBK; ++ki) {
                    f32x16 wb0;
                    c_block1<NBK>(obT, f0b, e0b, ki, lane, wb0);
                    const f32x16 keep = load16(fkP + (ki * 2 + h) * 16);
#pragma unroll
                    for (int r = 0; r < 16; ++r) ob0[ki][r] = __builtin_fmaf(wb0[r], keep[r], sbar);
                }
            }
        }
        // Gb2 of dimension 0: sum over the tile's walkers of obar0 (16 registers per half: DPP sums; lane (j, h) keeps register j & 15 where j < 16)
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb) {
            float sb = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a = half32_sum(ob0[kb][r]);
                sb = (j & 15) == r ? a : sb;
            }
            gb20[kb] += sb;
        }
        // ---- conditioner, reverse: hbar2 = W2' obar, zbar2 = act'(z2) hbar2, hbar1 = W1' zbar2, zbar1 = act'(z1) hbar1
        __builtin_amdgcn_sched_barrier(0);
        f32x16 z2a[NCH], z2b[NCH];
        Frag f[NCH][2];       // fragments of the tensor the next product contracts: obar ([channel][row block]), then zbar2 ([channel][unit block])
        int e[NCH];
        to_frags_kb<NBK>(ob, f, e);
        {
            f32x16 o2[NBK][NCH];
            cond_fwd<false, NBK>(net, u0.v, u1.v, lane, z2a, z2b, o2);
        }
        // dW2[k][row] = sum_c sum_w X2_c[k][w] obar_c[row][w]: X2 = act(z2), block by block (32 units: 48 registers of fragments at a time); both operands
        // transposed on the matrix cores; the 2 x NBK blocks of the product go to the accumulator blocks 4 + (k block) NBK + (row block).  Gb2 rides on
        // obar's transposes.
        {
            Frag yt[NBK][NCH];      // obar^T, once for both k blocks
#pragma unroll
            for (int kb = 0; kb < NBK; ++kb) {
                float rs = 0.0f;
#pragma unroll
                for (int c = 0; c < NCH; ++c) tr_frag(f[c][kb], pm, yt[kb][c], c == 0 ? &rs : nullptr);
                gb21[kb] = __builtin_fmaf(rs, __builtin_amdgcn_ldexpf(1.0f, e[0]), gb21[kb]);
            }
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) {
                f32x16 t[NCH];
#pragma unroll
                for (int c = 0; c < NCH; ++c) t[c] = mb ? z2b[c] : z2a[c];
                act_block(t);
                Frag fx[NCH];
                const int E = block_frags_x(t, e, fx);
                f32x16 p[NBK];
#pragma unroll
                for (int kb = 0; kb < NBK; ++kb) p[kb] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    Frag xt;
                    tr_frag(fx[c], pm, xt);
#pragma unroll
                    for (int kb = 0; kb < NBK; ++kb) wgrad_block(p[kb], xt, yt[kb][c]);
                }
#pragma unroll
                for (int kb = 0; kb < NBK; ++kb) acc_add<kShared>(acc, ticket, 4 + mb * NBK + kb, k, lane, p[kb], __builtin_amdgcn_ldexpf(1.0f, E));
            }
        }
        f32x16 g0[NCH], g1[NCH];
        {
#pragma unroll
            for (int c = 0; c < NCH; ++c) { g0[c] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; g1[c] = g0[c]; }
#pragma unroll
            for (int kt = 0; kt < NBK; ++kt)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    mfma_step<NCH>(TW2h, TW2l, kt, s, f, g0, lane);
                    mfma_step<NCH>(TW2h + NBK * 1024, TW2l + NBK * 1024, kt, s, f, g1, lane);
                }
            unscale_all(g0, e);
            unscale_all(g1, e);
            act_block_bwd(z2a, g0);
            act_block_bwd(z2b, g1);
            to_frags_all<true>(g0, g1, f, e);
            // dW1[k][u] = sum_c sum_w X1_c[k][w] zbar2_c[u][w] while the fragments of zbar2 (f, exponents e) are at hand and before the product that
            // consumes them: X1, the first hidden layer's activation triples, is recomputed block by block from (s, 1, 0) (two f32 MFMAs and 16
            // activations per lane and block).  Accumulator blocks 0 .. 3 = (k block mb, u block nb); Gb1 rides on the transposes of zbar2.
            {
                const float in0[2] = {u0.v, 1.0f}, in1[2] = {u1.v, 0.0f};
#pragma unroll
                for (int mb = 0; mb < 2; ++mb) {
                    f32x16 t[NCH];
                    init_acc(t, net + O::b0 + (mb * 2 + h) * 16);
                    const float w0 = net[O::W0 + mb * 64 + lane];
#pragma unroll
                    for (int c = 0; c < 2; ++c) t[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, h ? in1[c] : in0[c], t[c], 0, 0, 0);
                    act_block(t);
                    Frag fx[NCH];
                    const int E = block_frags_x(t, e, fx);
                    Frag xt[NCH];
#pragma unroll
                    for (int c = 0; c < NCH; ++c) tr_frag(fx[c], pm, xt[c]);
                    const float un = __builtin_amdgcn_ldexpf(1.0f, E);
#pragma unroll
                    for (int nb = 0; nb < 2; ++nb) {
                        f32x16 p = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
                        for (int c = 0; c < NCH; ++c) {
                            Frag yt;
                            float rs = 0.0f;
                            const bool bias = c == 0 && mb == 0;
                            tr_frag(f[c][nb], pm, yt, bias ? &rs : nullptr);
                            wgrad_block(p, xt[c], yt);
                            if (bias) gb1[nb] = __builtin_fmaf(rs, __builtin_amdgcn_ldexpf(1.0f, e[0]), gb1[nb]);
                        }
                        acc_add<kShared>(acc, ticket, 2 * mb + nb, k, lane, p, un);
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NCH; ++c) { g0[c] = f32x16{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; g1[c] = g0[c]; }
            dense64_block<NCH>(TW1h, TW1l, f, g0, lane);
            dense64_block<NCH>(TW1h + 2048, TW1l + 2048, f, g1, lane);
            unscale_all(g0, e);
            unscale_all(g1, e);
        }
        {
            const float in0[2] = {u0.v, 1.0f}, in1[2] = {u1.v, 0.0f};
            f32x16 a0[NCH], a1[NCH];
            init_acc(a0, net + O::b0 + (0 * 2 + h) * 16);
            init_acc(a1, net + O::b0 + (1 * 2 + h) * 16);
            const float w0 = net[O::W0 + 0 * 64 + lane], w1 = net[O::W0 + 1 * 64 + lane];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                a0[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, h ? in1[c] : in0[c], a0[c], 0, 0, 0);
                a1[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, h ? in1[c] : in0[c], a1[c], 0, 0, 0);
            }
            act_block_bwd(a0, g0);
            act_block_bwd(a1, g1);
        }
        // input layer: Gb0[u] = sum_w zbar1_0[u][w], GW0[u] = sum_w zbar1_0[u][w] s_w + zbar1_1[u][w] (seed of the conditioner's input: (s, 1, 0)), summed
        // over the tile's walkers here (the lanes of a half); lane (j, h) keeps the sums of register j & 15 of block j >> 4
        {
            float sb = 0.0f, sw = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float a0 = half32_sum(g0[0][r]), a1 = half32_sum(g1[0][r]);
                const float b0 = half32_sum(__builtin_fmaf(g0[0][r], u0.v, g0[1][r])), b1 = half32_sum(__builtin_fmaf(g1[0][r], u0.v, g1[1][r]));
                const bool mine = (j & 15) == r;
                sb = mine ? (j < 16 ? a0 : a1) : sb;
                sw = mine ? (j < 16 ? b0 : b1) : sw;
            }
            gb0s += sb;
            gw0s += sw;
        }
        {
            const f32x16 wa = load16(TW0 + (0 * 2 + h) * 16), wb2 = load16(TW0 + (1 * 2 + h) * 16);
            float sbar = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) sbar = __builtin_fmaf(wa[r], g0[0][r], __builtin_fmaf(wb2[r], g1[0][r], sbar));
            u0b.v += xhalf_sum(sbar);
        }
        if (valid && h == 0) {
            ja_store(adjb, 0, B, w, u0b);
            ja_store(adjb, 1, B, w, u1b);
            ja_store(adjb, 2, B, w, ldb);
        }
    }
    // ---- this workgroup's block of the net's gradient: the accumulator blocks as they stand, the per-lane sums added over the waves in wave order
    __syncthreads();                       // every wave is done with its tiles: the operand images are dead, the accumulators complete
    float* red = lds;                      // [wave][kKinds][64 lanes] over the image area
    {
        float* mine = red + (threadIdx.x >> 6) * kKinds * 64 + lane;
        mine[0] = gb1[0]; mine[64] = gb1[1];
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb) { mine[(2 + kb) * 64] = gb21[kb]; mine[(2 + NBK + kb) * 64] = gb20[kb]; }
        mine[(2 + 2 * NBK) * 64] = gb0s; mine[(3 + 2 * NBK) * 64] = gw0s;
    }
    __syncthreads();
    float* g = partial + (size_t)blockIdx.x * G::floats;
    auto wsum = [&](int kind, int ln) {    // sum over the waves of a lane's value
        float a = 0.0f;
#pragma unroll
        for (int wv = 0; wv < kBwdWaves; ++wv) a += red[(wv * kKinds + kind) * 64 + ln];
        return a;
    };
    for (int i = threadIdx.x; i < kAcc * 1024; i += kThreads) {
        const int b = i >> 10, q = (i >> 8) & 3, ln = (i >> 2) & 63, r = 4 * q + (i & 3);
        const int row = acc_rho(r, ln >> 5), n = ln & 31;
        float a = 0.0f;
#pragma unroll
        for (int st = 0; st < kSets; ++st) a += acc_all[st * kAcc * 1024 + i];
        if (b < 4) g[G::W1 + (32 * (b >> 1) + row) * 64 + 32 * (b & 1) + n] = a;
        else g[G::W2 + (32 * ((b - 4) / NBK) + row) * (32 * NBK) + 32 * ((b - 4) % NBK) + n] = a;
    }
    for (int i = threadIdx.x; i < 128 + 64 * NBK; i += kThreads) {
        if (i < 64) {                      // Gb1[u]: u block = i >> 5; the two lane halves hold the two halves of the tile's walkers
            const int nb = i >> 5, n = i & 31;
            g[G::b1 + i] = wsum(nb, n) + wsum(nb, n + 32);
        } else if (i < 64 + 32 * NBK) {    // Gb2 of dimension 1
            const int t = i - 64, kb = t >> 5, n = t & 31;
            g[G::b21 + t] = wsum(2 + kb, n) + wsum(2 + kb, n + 32);
        } else if (i < 64 + 64 * NBK) {    // Gb2 of dimension 0: lane (j < 16, h) keeps register j of half h
            const int t = i - 64 - 32 * NBK, kb = t >> 5, jj = t & 15, hh = (t >> 4) & 1;
            g[G::b20 + 32 * kb + acc_rho(jj, hh)] = wsum(2 + NBK + kb, jj + 32 * hh);
        } else {                           // Gb0 / GW0: lane (j, h) keeps register j & 15 of block j >> 4
            const int ln = i - 64 - 64 * NBK, jj = ln & 31, hh = ln >> 5;
            const int u = 32 * (jj >> 4) + acc_rho(jj & 15, hh);
            g[G::b0 + u] = wsum(2 + 2 * NBK, ln);
            g[G::W0 + u] = wsum(3 + 2 * NBK, ln);
        }
    }
}

extern template __global__ void k_ebwd<true, 2>(const MfmaDev, int, const float*, const float*, const float*, float*, const float*, const float*, int64_t, float*);
extern template __global__ void k_ebwd<false, 2>(const MfmaDev, int, const float*, const float*, const float*, float*, const float*, const float*, int64_t, float*);
}  // namespace wf
