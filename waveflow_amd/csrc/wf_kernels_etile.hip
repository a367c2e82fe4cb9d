// wf_kernels_etile.hip -- local energy of large batches on the matrix cores (gfx950).
//
// H psi = -1/2 laplacian(psi) + V psi (physics.py:50-52, 79-93) needs psi with its gradient and Laplacian with respect to the walker's
// coordinates.  The wave kernels (wf_kernels_wave.hip) carry that (value, gradient, Laplacian / 2) jet through the model with one wave per
// walker; their conditioner products are LDS-fed GEMVs.  For large batches of the two-particle family this file splits the work by what
// the hardware is good at, one launch pair per conditioner net:
//
//   k_etile_cond   32 walkers per wave tile, the conditioner of ONE net on the matrix cores.  With two particles the MADE masks leave the
//                  conditioner ONE input (hidden degrees arange(64) % (D - 1) = 0: model_factory.py:15): every hidden and output unit is a
//                  function of the scalar u_0, so what travels is its Taylor triple (f, f', f'') in u_0 -- three channels = three extra
//                  column groups of the same split-fp16 MFMA products k_mfma issues (the weight operand is shared: mfma_step<3>); the
//                  activations r(x) = 1 / (2^x + 1) propagate the triple on the VALU.  Derivative channels are unbounded, fp16 is not: every
//                  (walker, channel) column is scaled by a power of two around each product (exact).  Output: the head's pre-activation
//                  triples, [row][channel][walker] in HBM (for the prior: already multiplied by ob_to_b); the head kernels turn them into
//                  jets in (x0, x1) with the chain rule through the jet of u_0.
//   k_etile_flow / k_etile_prior   one LANE per walker: sigmoid head, normalisations, table lerps of derivative orders 0..3 and the
//                  log-determinant as jet arithmetic in registers; row sums are sequential loops (no cross-lane traffic), the walker
//                  index is the fastest-moving one of every array (coalesced).
//
// State between launches (SoA, walker fastest): u_0, u_1, log det as jets; 12 floats per walker.  Head triples through HBM: 2 x 384 B per
// walker and net.  Same function as k_wave_fwd<2, RF<2>> + k_energy_out (same derivative rule of the table lerp: order nd -> table nd + 1),
// checked against it and against the torch oracle (tests/test_gpu_energy.py).  Coverage: D = 2, <= 64 bases (launch-per-net form: <= 32), mean-type box, IMADE layers,
// Waveflow prior, ungated heads (every homogeneous boundary dictionary: the tables carry the map); everything else stays on the wave kernel.
// (the gradient path: wf_etile_bwd.h, wf_kernels_etile_bwd.hip; the staged inverse / sampler: wf_kernels_etile_sample.hip)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "wf_etile_cond.h"

// The jet / Taylor algebra of this file is checked against oracles by tolerance, not by operation order: multiply-add pairs may fuse (the build's
// default is -ffp-contract=off).  The pragma is lexical: the index arithmetic of the table lerp (make_lerp, div_by_n in wf_mfma_impl.h, included
// above) keeps the reference's separate roundings, so the bin indices stay bit-exact.
#pragma clang fp contract(fast)

namespace wf {

namespace {
// ---------------------------------------------------------------------------- lane-per-walker stages
// BoxTransformLayer, mean type, two particles (made.py:156-183) as jets of (x0, x1)
// (JT = J: H psi; J5: the coordinate derivatives with the Hessian diagonal -- here and in the two head kernels below)
template <class JT = J>
__global__ void k_etile_box(const float* __restrict__ xg, int64_t B, float L, float* __restrict__ st) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const float tol = 1e-7f;
    const JT x0 = jvar<JT>(xg[b * 2], 0), x1 = jvar<JT>(xg[b * 2 + 1], 1);
    const JT mean = (x0 + x1) * 0.5f;
    const JT l = mean - x0, wd = x1 - x0;
    JT ld = jcst<JT>(0.0f);
    const JT space = jcst<JT>(2 * L);
    const JT diff = x1 - x0;
    const JT u0 = diff * jrcp(space + tol);
    ld = ld - jlog(space + tol);
    const JT den = (jcst<JT>(2 * L) - wd) + tol;
    const JT u1 = ((mean + L) - l) * jrcp(den);
    ld = ld - jlog(den);
    st_store(st, 0, B, b, u0);
    st_store(st, 1, B, b, u1);
    st_store(st, 2, B, b, ld);
}

// One IMADE layer behind its conditioner (made.py:66-81) + Reverse: dimension 0 from the composite table, dimension 1 from the head jets
template <class JT = J>
__global__ __launch_bounds__(256) void k_etile_flow(const float4_t* __restrict__ comp /* this net: [n_mesh] {Y, Y', Y'', Y'''} */,
                                                    const float* __restrict__ tabI /* [n_mesh][8 row chunks][4 orders][4 rows] */, const float* __restrict__ gI, int nb,
                                                    int n_mesh, float reg, const float* __restrict__ oj, int64_t B, float* __restrict__ st) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const JT u0 = st_get<JT>(st, 0, B, b), u1 = st_get<JT>(st, 1, B, b);
    JT ld = st_get<JT>(st, 2, B, b);
    // ---- dimension 0
    JT y0;
    {
        const LerpN L = nlerp(u0.v, n_mesh);
        const float4_t ca = comp[L.il], cb = comp[L.ir];
        const float t0 = __builtin_fmaf(cb.x - ca.x, L.t, ca.x), t1 = __builtin_fmaf(cb.y - ca.y, L.t, ca.y);
        const float t2 = __builtin_fmaf(cb.z - ca.z, L.t, ca.z), t3 = __builtin_fmaf(cb.w - ca.w, L.t, ca.w);
        y0 = jlift(t0, t1, t2, u0);
        ld = ld + jlog(jlift(t1, t2, t3, u0) + 1e-7f);
    }
    // ---- dimension 1: c_j = g_j (v_j / S0 + reg) / Q (calculate_bijection_params, + reg, remove_bias, boundary map: wf_model_build.cpp).
    // One pass over the rows: with V_k = sum_j v_j g_j B^(k)_j, R_k = sum_j g_j B^(k)_j, Qv = sum_j v_j g_j, G = sum_j g_j, S0 = sum_j v_j the
    // numerators are N_k = V_k / S0 + reg R_k and the normaliser Q = Qv / S0 + reg G.  Four rows per step: the lane's table rows come as
    // 16-byte loads (8 per step: 4 orders x the two mesh rows; rows >= nb are zero padding).
    const LerpN L = nlerp(u1.v, n_mesh);
    const int* bnd = reinterpret_cast<const int*>(tabI + (size_t)n_mesh * 128);   // [8 chunks][lo, hi] behind the table (wf_model_build.cpp: upload_chunked)
    // sums over the rows (see T2): S^(a) = sum v_j^(a), Qv^(a) = sum g_j v_j^(a), V[a][k] = sum v_j^(a) g_j T_j^(k) for a + k <= 3 (k <= 3 - a ... the
    // nine pairs the two numerators need), R[k] = sum g_j T_j^(k), G = sum g_j
    float S[3] = {0.0f, 0.0f, 0.0f}, Qv[3] = {0.0f, 0.0f, 0.0f}, R[4] = {0.0f, 0.0f, 0.0f, 0.0f}, G = 0.0f;
    float V0[4] = {0.0f, 0.0f, 0.0f, 0.0f}, V1[3] = {0.0f, 0.0f, 0.0f}, V2[2] = {0.0f, 0.0f};   // V[a][k]: a = 0: k 0..3, a = 1: k 0..2, a = 2: k 0..1
    for (int j0 = 0; j0 < nb; j0 += 4) {
        // the chunk at the mesh index clamped to its support: the same bits, and the walkers outside the support read two shared lines
        const int lo = bnd[j0 >> 1], hi = bnd[(j0 >> 1) + 1];
        const float4_t* rl = reinterpret_cast<const float4_t*>(tabI + (size_t)min(max(L.il, lo), hi) * 128);   // [8 chunks][4 orders] float4
        const float4_t* rr = reinterpret_cast<const float4_t*>(tabI + (size_t)min(max(L.ir, lo), hi) * 128);
        float4_t ta[4], tb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ta[k] = rl[j0 + k];     // (chunk j0 / 4) * 4 + k
            tb[k] = rr[j0 + k];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int jr_ = j0 + q;
            if (jr_ >= nb) break;
            const float* p = oj + ((b >> 5) * (32 * NCH) + jr_ * NCH) * 32 + (b & 31);     // [tile][row][channel][32 walkers]
            float v0, v1, v2;
            r_triple(p[0], p[32], p[64], v0, v1, v2);       // the head's weight and its first two derivatives in u_0
            const float g = gI[jr_];
            float t[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float a = q == 0 ? ta[k].x : (q == 1 ? ta[k].y : (q == 2 ? ta[k].z : ta[k].w));
                const float bb = q == 0 ? tb[k].x : (q == 1 ? tb[k].y : (q == 2 ? tb[k].z : tb[k].w));
                t[k] = __builtin_fmaf(bb - a, L.t, a) * g;   // g_j folded into the row
            }
            S[0] += v0; S[1] += v1; S[2] += v2;
            Qv[0] = __builtin_fmaf(v0, g, Qv[0]); Qv[1] = __builtin_fmaf(v1, g, Qv[1]); Qv[2] = __builtin_fmaf(v2, g, Qv[2]);
#pragma unroll
            for (int k = 0; k < 4; ++k) { V0[k] = __builtin_fmaf(v0, t[k], V0[k]); R[k] += t[k]; }
#pragma unroll
            for (int k = 0; k < 3; ++k) V1[k] = __builtin_fmaf(v1, t[k], V1[k]);
#pragma unroll
            for (int k = 0; k < 2; ++k) V2[k] = __builtin_fmaf(v2, t[k], V2[k]);
            G += g;
        }
    }
    JT y1;
    flow_head_finish(S, Qv, R, G, V0, V1, V2, reg, u0, u1, y1, ld);
    st_store(st, 0, B, b, y1);   // Reverse (bijections.py:337-340)
    st_store(st, 1, B, b, y0);
    st_store(st, 2, B, b, ld);
}

// Waveflow prior (wavefunctions.py:54-71) + H psi (physics.py:60-93); DERIV (wf_psi_coord_derivs): psi (may be null), its gradient and -- JT = J5 -- the
// diagonal of its Hessian instead
template <class JT = J, bool DERIV = false>
__global__ __launch_bounds__(256) void k_etile_prior(const float4_t* __restrict__ comp /* prior: {P, P', P''} with sign and norm */,
                                                     const float* __restrict__ tabP /* orthogonal B, [n_mesh][8][4][4] like tabI */, int nb, int n_mesh,
                                                     unsigned constrained_mask, const float* __restrict__ oj, const float* __restrict__ s1buf,
                                                     const float* __restrict__ st, const float* __restrict__ xg, int64_t B, const Protons pr,
                                                     float* __restrict__ hpsi, float* __restrict__ psi_out, float* __restrict__ lap_out,
                                                     float* __restrict__ grad_out = nullptr, float* __restrict__ hdiag_out = nullptr) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const JT u0 = st_get<JT>(st, 0, B, b), u1 = st_get<JT>(st, 1, B, b), ld = st_get<JT>(st, 2, B, b);
    // the spline sees the clipped coordinate (:45): outside [0, 1] it is a constant
    const JT uc0 = (u0.v < 0.0f) ? jcst<JT>(0.0f) : (u0.v > 1.0f ? jcst<JT>(1.0f) : u0);
    const JT uc1 = (u1.v < 0.0f) ? jcst<JT>(0.0f) : (u1.v > 1.0f ? jcst<JT>(1.0f) : u1);
    JT val0;
    {
        const LerpN L = nlerp(uc0.v, n_mesh);
        const float4_t ca = comp[L.il], cb = comp[L.ir];
        val0 = jlift(__builtin_fmaf(cb.x - ca.x, L.t, ca.x), __builtin_fmaf(cb.y - ca.y, L.t, ca.y), __builtin_fmaf(cb.z - ca.z, L.t, ca.z), uc0);
    }
    const LerpN L = nlerp(uc1.v, n_mesh);
    const int* bnd = reinterpret_cast<const int*>(tabP + (size_t)n_mesh * 128);
    // sums over the rows (see T2): D[a][k] = sum c_i^(a)(s) B_i^(k)(t), a + k <= 2; |c|^2 and its first two derivatives in s from cc, cc', c'c', cc''
    float D0[3] = {0.0f, 0.0f, 0.0f}, D1[2] = {0.0f, 0.0f}, D2 = 0.0f, cc = 0.0f, cc1 = 0.0f, c1c1 = 0.0f, cc2 = 0.0f;
    for (int i0 = 0; i0 < nb; i0 += 4) {
        const int lo = bnd[i0 >> 1], hi = bnd[(i0 >> 1) + 1];
        const float4_t* rl = reinterpret_cast<const float4_t*>(tabP + (size_t)min(max(L.il, lo), hi) * 128);
        const float4_t* rr = reinterpret_cast<const float4_t*>(tabP + (size_t)min(max(L.ir, lo), hi) * 128);
        float4_t ta[3], tb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ta[k] = rl[i0 + k];
            tb[k] = rr[i0 + k];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = i0 + q;
            if (i >= nb) break;
            const float* p = oj + ((b >> 5) * (32 * NCH) + i * NCH) * 32 + (b & 31);
            const float c0 = p[0], c1 = p[32], c2 = p[64];        // c_i and its derivatives in the unclipped u_0 (wavefunctions.py:40)
            float t[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float a = q == 0 ? ta[k].x : (q == 1 ? ta[k].y : (q == 2 ? ta[k].z : ta[k].w));
                const float bb = q == 0 ? tb[k].x : (q == 1 ? tb[k].y : (q == 2 ? tb[k].z : tb[k].w));
                t[k] = __builtin_fmaf(bb - a, L.t, a);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) D0[k] = __builtin_fmaf(c0, t[k], D0[k]);
            D1[0] = __builtin_fmaf(c1, t[0], D1[0]); D1[1] = __builtin_fmaf(c1, t[1], D1[1]);
            D2 = __builtin_fmaf(c2, t[0], D2);
            cc = __builtin_fmaf(c0, c0, cc); cc1 = __builtin_fmaf(c0, c1, cc1); c1c1 = __builtin_fmaf(c1, c1, c1c1); cc2 = __builtin_fmaf(c0, c2, cc2);
        }
    }
    const float sgn = s1buf[b] < 0.0f ? -1.0f : 1.0f;
    const T2 N2 = T2{cc, 2.0f * cc1, 0.0f, 2.0f * (c1c1 + cc2), 0.0f, 0.0f};
    const T2 dotp = T2{D0[0], D1[0], D0[1], D2, D1[1], D0[2]};
    const JT val1 = t2jet(dotp * t2rsqrt(N2), u0, uc1) * sgn;
    const float sc0 = (constrained_mask & 1u) ? 0.70710678118654752f : 1.0f, sc1 = (constrained_mask & 2u) ? 0.70710678118654752f : 1.0f;
    const JT psi = ((val0 * sc0) * (val1 * sc1)) * jexp_half(ld);
    if constexpr (DERIV) {
        if (psi_out) psi_out[b] = psi.v;
        grad_out[b * 2] = psi.a;
        grad_out[b * 2 + 1] = psi.b;
        if constexpr (std::is_same<JT, J5>::value) {
            hdiag_out[b * 2] = 2.0f * psi.h;
            hdiag_out[b * 2 + 1] = 2.0f * psi.k;
        }
    } else {
        const float lap = 2.0f * psi.h;
        float V = 0.0f;   // physics.py:60-76
        for (int p = 0; p < pr.n; ++p)
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const float r = pr.pos[p] - xg[b * 2 + d];
                V -= 1.0f / sqrtf(1.0f + r * r);
            }
        {
            const float r = xg[b * 2 + 1] - xg[b * 2];
            V += 1.0f / sqrtf(1.0f + r * r);
        }
        hpsi[b] = -0.5f * lap + V * psi.v;
        if (psi_out) psi_out[b] = psi.v;
        if (lap_out) lap_out[b] = lap;
    }
}

// ---------------------------------------------------------------------------- H psi in ONE kernel (every net resident in LDS)
// The conditioner's head triples stay in the accumulator registers: lane (walker j, half h) holds registers 4q .. 4q + 3 = rows 8q + 4h .. + 3 =
// row CHUNK 2q + h of the regrouped tables ([mesh][8 chunks][4 orders][4 rows]: one 64-byte segment per chunk and lerp end).  The head runs on
// those 16 rows per lane with the separable row sums of T2 (scalars, no jet per row); the two lane halves are combined with one
// v_permlane32_swap per sum; quotients, logarithms and the change to (x0, x1) jets once per walker.  No exchange buffer, no state in HBM:
// 8 B per walker in, 4 .. 12 B out.  One persistent workgroup of 8 waves per CU (two per SIMD, 256 registers), tiles from an LDS counter.
// (round 4, 2^20 walkers, one / two row blocks: 8 waves 0.81 / 1.16 ms, 6 waves 0.88 / 1.36, 4 waves -- no spills -- 0.98 / 1.31, 12 waves -- 133 / 330 spilled -- 0.96 / 2.21, 16 waves 2.31 / 3.98)
constexpr int kFusedWaves = 8;

template <class JT>
__device__ __forceinline__ void box_mean2(float x0v, float x1v, float L, JT& u0, JT& u1, JT& ld) {   // (k_etile_box)
    const float tol = 1e-7f;
    const JT x0 = jvar<JT>(x0v, 0), x1 = jvar<JT>(x1v, 1);
    const JT mean = (x0 + x1) * 0.5f;
    const JT l = mean - x0, wd = x1 - x0;
    const JT space = jcst<JT>(2 * L);
    const JT diff = x1 - x0;
    u0 = diff * jrcp(space + tol);
    ld = jcst<JT>(0.0f) - jlog(space + tol);
    const JT den = (jcst<JT>(2 * L) - wd) + tol;
    u1 = ((mean + L) - l) * jrcp(den);
    ld = ld - jlog(den);
}
// PBIAS: the B prior's boundary map has a constant term (a constraint with a non-zero value): its own instantiation, so that the derivative channels'
// sums do not lengthen live ranges in the common one
// OUT (wf_psi_coord_derivs): 0: H psi;  1: psi (may be null) and its gradient, J's a and b;  2: ... and the diagonal of its Hessian -- the per-walker jet
// is J5 (the conditioner's three MFMA channels and the separable row sums are those of OUT = 0: only the per-walker algebra behind them grows)
template <int NBK, bool PBIAS = false, int OUT = 0>
__global__ __launch_bounds__(kFusedWaves * 64) void k_efused(const MfmaDev mm, const float* __restrict__ tabI, const float* __restrict__ tabP,
                                                             const float* __restrict__ xg, int64_t B, const Protons pr, float* __restrict__ hpsi,
                                                             float* __restrict__ psi_out, float* __restrict__ lap_out, float* __restrict__ st_out,
                                                             float* __restrict__ grad_out = nullptr /* OUT >= 1: [B][2] */, float* __restrict__ hdiag_out = nullptr /* OUT = 2: [B][2] */) {
    using JT = typename std::conditional<OUT == 2, J5, J>::type;
    // st_out (may be null): the (u_0, u_1, log det) jets at the input of every net, [net][slot][channel][B] -- what the gradient path's
    // per-net reverse kernels (k_ebwd) restart from
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int next_tile;
    __shared__ int bnd_s[32 * NBK];   // support bounds of the table chunks: [I: 8 NBK][lo, hi], [prior: 8 NBK][lo, hi]
    constexpr int kThreads = kFusedWaves * 64;
    constexpr int kMeshStride = 128 * NBK;   // floats per mesh point of the regrouped tables: [8 NBK chunks][4 orders][4 rows]
    if (threadIdx.x == 0) next_tile = 0;
    if (threadIdx.x < 16 * NBK) bnd_s[threadIdx.x] = reinterpret_cast<const int*>(tabI + (size_t)mm.n_mesh * kMeshStride)[threadIdx.x];
    else if (threadIdx.x < 32 * NBK) bnd_s[threadIdx.x] = reinterpret_cast<const int*>(tabP + (size_t)mm.n_mesh * kMeshStride)[threadIdx.x - 16 * NBK];
    stage_floats<kThreads>(mm.image + mm.const_img_off, lds, mm.const_floats);
    stage_floats<kThreads>(mm.image, lds + mm.const_floats, mm.net_floats * mm.n_nets);
    __syncthreads();
    const float* fkI = lds;
    const float* fkP = lds + 32 * NBK;
    const _Float16* obh = reinterpret_cast<const _Float16*>(lds + 64 * NBK);
    const float* cbP = lds + 64 * NBK + NBK * NBK * 1024 + 64 * NBK;   // [NBK][2][16] constant term of the B prior's boundary map times ob_to_b (mm.p_bias; wf_model_images.cpp: mfma_prepare)
    const int lane = threadIdx.x & 63;
    const int j = lane & 31, h = lane >> 5;
    const int n_mesh = mm.n_mesh;
    const int64_t n_tiles = (B + 31) >> 5;
    const int64_t my_tiles = n_tiles > (int64_t)blockIdx.x ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    int f16_bad = 0;
    if (mm.f16_ovf)
        for (int n = 0; n < mm.n_nets; ++n) f16_bad |= mm.f16_ovf[n];
    for (;;) {
        int q_ = 0;
        if (lane == 0) q_ = __hip_atomic_fetch_add(&next_tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        q_ = __builtin_amdgcn_readfirstlane(q_);
        if (q_ >= my_tiles) break;
        const int64_t tile = (int64_t)blockIdx.x + (int64_t)q_ * gridDim.x;
        const int64_t w = tile * 32 + j;
        const bool valid = w < B;
        const int64_t wl = valid ? w : B - 1;
        const float x0v = xg[wl * 2], x1v = xg[wl * 2 + 1];
        JT u0, u1, ld;
        box_mean2(x0v, x1v, mm.box_L, u0, u1, ld);
        // ---- flow layers (made.py:66-81 + Reverse)
        for (int l = 0; l < mm.n_layers; ++l) {
            const float* net = lds + mm.const_floats + (size_t)l * mm.net_floats;
            if (OUT == 0 && st_out && valid && h == 0) {
                st_store(st_out + (size_t)l * 12 * B, 0, B, w, u0);
                st_store(st_out + (size_t)l * 12 * B, 1, B, w, u1);
                st_store(st_out + (size_t)l * 12 * B, 2, B, w, ld);
            }
            Frag f[NCH][2];
            int e[NCH];
            cond_hidden<NBK>(net, u0.v, u1.v, lane, f, e);
            // dimension 0: composite table of the net, all four orders
            JT y0;
            {
                const LerpN L0 = nlerp(u0.v, n_mesh);
                const float4_t* comp = mm.comp + (size_t)l * n_mesh;
                const float4_t ca = comp[L0.il], cb = comp[L0.ir];
                const float t0 = __builtin_fmaf(cb.x - ca.x, L0.t, ca.x), t1 = __builtin_fmaf(cb.y - ca.y, L0.t, ca.y);
                const float t2 = __builtin_fmaf(cb.z - ca.z, L0.t, ca.z), t3 = __builtin_fmaf(cb.w - ca.w, L0.t, ca.w);
                y0 = jlift(t0, t1, t2, u0);
                ld = ld + jlog(jlift(t1, t2, t3, u0) + 1e-7f);
            }
            // dimension 1: the lane's 16 rows of every 32-row block
            const LerpN L = nlerp(u1.v, n_mesh);
            FlowSums a = {};
#pragma unroll
            for (int kb = 0; kb < NBK; ++kb) {
                f32x16 o[NCH];
                cond_out<NBK>(net, f, e, kb, lane, o);
                flow_rows(a, o, load16(fkI + (kb * 2 + h) * 16), tabI, kMeshStride, bnd_s, L, kb, h);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) { a.S[k] = xhalf_sum(a.S[k]); a.Qv[k] = xhalf_sum(a.Qv[k]); a.V1[k] = xhalf_sum(a.V1[k]); }
#pragma unroll
            for (int k = 0; k < 4; ++k) { a.R[k] = xhalf_sum(a.R[k]); a.V0[k] = xhalf_sum(a.V0[k]); }
#pragma unroll
            for (int k = 0; k < 2; ++k) a.V2[k] = xhalf_sum(a.V2[k]);
            JT y1;
            flow_head_finish(a.S, a.Qv, a.R, mm.F_I, a.V0, a.V1, a.V2, mm.i_reg, u0, u1, y1, ld);
            u0 = y1;   // Reverse (bijections.py:337-340)
            u1 = y0;
        }
        // ---- Waveflow prior (wavefunctions.py:54-71)
        JT psi;
        {
            const float* net = lds + mm.const_floats + (size_t)mm.n_layers * mm.net_floats;
            if (OUT == 0 && st_out && valid && h == 0) {
                st_store(st_out + (size_t)mm.n_layers * 12 * B, 0, B, w, u0);
                st_store(st_out + (size_t)mm.n_layers * 12 * B, 1, B, w, u1);
                st_store(st_out + (size_t)mm.n_layers * 12 * B, 2, B, w, ld);
            }
            float s1 = 0.0f, sder[2] = {0.0f, 0.0f};
            Frag of[NBK][NCH];
            int eo[NCH];
            {
                Frag f[NCH][2];
                int e[NCH];
                cond_hidden<NBK>(net, u0.v, u1.v, lane, f, e);   // (the conditioner sees the unclipped u_0, wavefunctions.py:40)
                f32x16 o[NBK][NCH];
#pragma unroll
                for (int kb = 0; kb < NBK; ++kb) cond_out<NBK>(net, f, e, kb, lane, o[kb]);
                prior_frags<NBK>(o, fkP, lane, of, eo, s1, PBIAS ? sder : nullptr);
            }
            const JT uc0 = (u0.v < 0.0f) ? jcst<JT>(0.0f) : (u0.v > 1.0f ? jcst<JT>(1.0f) : u0);   // the spline sees the clipped coordinate (:45)
            const JT uc1 = (u1.v < 0.0f) ? jcst<JT>(0.0f) : (u1.v > 1.0f ? jcst<JT>(1.0f) : u1);
            JT val0;
            {
                const LerpN L0 = nlerp(uc0.v, n_mesh);
                const float4_t* comp = mm.comp + (size_t)mm.n_layers * n_mesh;
                const float4_t ca = comp[L0.il], cb = comp[L0.ir];
                val0 = jlift(__builtin_fmaf(cb.x - ca.x, L0.t, ca.x), __builtin_fmaf(cb.y - ca.y, L0.t, ca.y), __builtin_fmaf(cb.z - ca.z, L0.t, ca.z), uc0);
            }
            const LerpN L = nlerp(uc1.v, n_mesh);
            PriorSums a = {};
#pragma unroll
            for (int ko = 0; ko < NBK; ++ko) {
                f32x16 cblk[NCH];
                prior_c_block<NBK>(obh, of, eo, ko, lane, cblk);
                if (PBIAS) {   // a boundary constraint with a non-zero value (bsplines_jax.py:173-199): c += (sum o) * (b @ ob_to_b), channel by channel
                    const f32x16 cb = load16(cbP + (ko * 2 + h) * 16);
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        cblk[0][r] = __builtin_fmaf(s1, cb[r], cblk[0][r]);
                        cblk[1][r] = __builtin_fmaf(sder[0], cb[r], cblk[1][r]);
                        cblk[2][r] = __builtin_fmaf(sder[1], cb[r], cblk[2][r]);
                    }
                }
                prior_rows(a, cblk, tabP, kMeshStride, bnd_s + 16 * NBK, L, ko, h);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) a.D0[k] = xhalf_sum(a.D0[k]);
            a.D1[0] = xhalf_sum(a.D1[0]); a.D1[1] = xhalf_sum(a.D1[1]); a.D2 = xhalf_sum(a.D2);
            a.cc = xhalf_sum(a.cc); a.cc1 = xhalf_sum(a.cc1); a.c1c1 = xhalf_sum(a.c1c1); a.cc2 = xhalf_sum(a.cc2);
            const float sgn = s1 < 0.0f ? -1.0f : 1.0f;
            const T2 N2 = T2{a.cc, 2.0f * a.cc1, 0.0f, 2.0f * (a.c1c1 + a.cc2), 0.0f, 0.0f};
            const T2 dotp = T2{a.D0[0], a.D1[0], a.D0[1], a.D2, a.D1[1], a.D0[2]};
            const JT val1 = t2jet(dotp * t2rsqrt(N2), u0, uc1) * sgn;
            const float sc0 = (mm.constrained_mask & 1u) ? 0.70710678118654752f : 1.0f, sc1 = (mm.constrained_mask & 2u) ? 0.70710678118654752f : 1.0f;
            psi = ((val0 * sc0) * (val1 * sc1)) * jexp_half(ld);
        }
        if constexpr (OUT != 0) {
            if (valid && h == 0) {   // (a packed weight outside the fp16 range: NaN, as below)
                const float nan = __builtin_nanf("");
                if (psi_out) psi_out[w] = f16_bad ? nan : psi.v;
                grad_out[w * 2] = f16_bad ? nan : psi.a;
                grad_out[w * 2 + 1] = f16_bad ? nan : psi.b;
                if constexpr (OUT == 2) {
                    hdiag_out[w * 2] = f16_bad ? nan : 2.0f * psi.h;
                    hdiag_out[w * 2 + 1] = f16_bad ? nan : 2.0f * psi.k;
                }
            }
        } else if (valid && h == 0) {
            const float lap = 2.0f * psi.h;
            float V = 0.0f;   // physics.py:60-76
            for (int p = 0; p < pr.n; ++p) {
                const float r0 = pr.pos[p] - x0v, r1 = pr.pos[p] - x1v;
                V -= 1.0f / sqrtf(1.0f + r0 * r0);
                V -= 1.0f / sqrtf(1.0f + r1 * r1);
            }
            {
                const float r = x1v - x0v;
                V += 1.0f / sqrtf(1.0f + r * r);
            }
            // a packed weight outside the fp16 range (k_fold_bias): NaN instead of whatever inf operands made of the walker
            hpsi[w] = f16_bad ? __builtin_nanf("") : -0.5f * lap + V * psi.v;
            if (psi_out) psi_out[w] = f16_bad ? __builtin_nanf("") : psi.v;
            if (lap_out) lap_out[w] = f16_bad ? __builtin_nanf("") : lap;
        }
    }
}

}  // namespace

bool energy_tile_fused(const MfmaDev* mdev) {
    // (two row blocks per dimension: the static LDS of k_efused<2> -- 256 B of chunk bounds -- has to fit beside the resident nets too)
    const bool fits = (mdev->const_floats + mdev->net_floats * mdev->n_nets) * 4 + 512 <= 160 * 1024;
    return !mdev->staged && fits && env_energy_fused();
}

// workspace: state (12 floats), head triples (96 floats), the sign sum (1 float) per walker
int64_t energy_tile_floats(int64_t B) { return B * (12 + 1) + ((B + 31) / 32) * 32 * (32 * NCH); }   // state, s1, head triples of whole tiles
int64_t derivs_tile_floats(int64_t B) { return energy_tile_floats(B) + 3 * B; }                        // ... and the fifth component of the three state jets

// mdev: the model's MFMA description (resident or not: one net is staged per launch); md: ModelDev on the host (spline sizes, masks)
// grad == null: H psi (hpsi, psi, lap; st_out);  else the coordinate derivatives of psi (psi, grad, hdiag: either may be null but grad)
static int launch_tile(const MfmaDev* mdev, const ModelDev& md, const float* tabI4, const float* tabP4, const float* fk_nat, const float* x, int64_t B,
                       const Protons& pr, float* hpsi, float* psi, float* lap, float* ws, void* stream, float* st_out, float* grad, float* hdiag) {
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return WF_OK;
    const int out = !grad ? 0 : (hdiag ? 2 : 1);
    // every net resident in LDS (the shipped shapes): the whole of H psi in one launch, nothing through HBM but the walkers and the results.
    // WF_ENERGY_FUSED=0 (read per call) keeps the launch-per-net path below (A/B tests; models whose nets do not fit together take it anyway).
    {
        if (energy_tile_fused(mdev)) {
            const int lds_all = (mdev->const_floats + mdev->net_floats * mdev->n_nets) * (int)sizeof(float);
            const int64_t n_tiles = (B + 31) / 32;
            const unsigned blocks = (unsigned)std::min<int64_t>((n_tiles + kFusedWaves - 1) / kFusedWaves, 256);
#define WF_EFUSED_OUT(NBK_, PB_, OUT_)                                                                                                         \
    {                                                                                                                                          \
        static DynLdsSlots cfg{};                                                                                                              \
        if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(k_efused<NBK_, PB_, OUT_>), lds_all, &cfg)) return rc;                    \
        hipLaunchKernelGGL((k_efused<NBK_, PB_, OUT_>), dim3(blocks), dim3(kFusedWaves * 64), lds_all, s, *mdev, tabI4, tabP4, x, B, pr, hpsi, psi, lap, st_out, \
                           grad, hdiag);                                                                                                       \
    }
#define WF_EFUSED(NBK_, PB_)                                                                                                                   \
    {                                                                                                                                          \
        if (out == 0) WF_EFUSED_OUT(NBK_, PB_, 0) else if (out == 1) WF_EFUSED_OUT(NBK_, PB_, 1) else WF_EFUSED_OUT(NBK_, PB_, 2)                \
    }
            if (mdev->nbk == 1) {
                if (mdev->p_bias) WF_EFUSED(1, true) else WF_EFUSED(1, false)
            } else {
                if (mdev->p_bias) WF_EFUSED(2, true) else WF_EFUSED(2, false)
            }
#undef WF_EFUSED
#undef WF_EFUSED_OUT
            return check();
        }
    }
    float* st = ws;   // [12 B] state jets, J5: + [3 B] their fifth components
    float* s1 = st + (out == 2 ? 15 : 12) * B;
    float* oj = s1 + B;
    const unsigned lane_blocks = (unsigned)((B + 255) / 256);
    const int lds_bytes = (mdev->const_floats + mdev->net_floats) * (int)sizeof(float);
    static DynLdsSlots cfg_flow{}, cfg_prior{};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(k_etile_cond<false>), lds_bytes, &cfg_flow)) return rc;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(k_etile_cond<true>), lds_bytes, &cfg_prior)) return rc;
    const int64_t n_tiles = (B + 31) / 32;
    const unsigned cond_blocks = (unsigned)std::min<int64_t>((n_tiles + kCondWaves - 1) / kCondWaves, 256 * 4);
    if (out == 2) hipLaunchKernelGGL(k_etile_box<J5>, dim3(lane_blocks), dim3(256), 0, s, x, B, md.box_L, st);
    else hipLaunchKernelGGL(k_etile_box<J>, dim3(lane_blocks), dim3(256), 0, s, x, B, md.box_L, st);
    for (int l = 0; l < md.n_layers; ++l) {
        hipLaunchKernelGGL(k_etile_cond<false>, dim3(cond_blocks), dim3(kCondWaves * 64), lds_bytes, s, *mdev, l, (const float*)st, B, oj, s1);
        if (out == 2)
            hipLaunchKernelGGL(k_etile_flow<J5>, dim3(lane_blocks), dim3(256), 0, s, mdev->comp + (size_t)l * mdev->n_mesh, tabI4, fk_nat, md.isp.nb,
                               md.isp.n_mesh, md.i_reg, (const float*)oj, B, st);
        else
            hipLaunchKernelGGL(k_etile_flow<J>, dim3(lane_blocks), dim3(256), 0, s, mdev->comp + (size_t)l * mdev->n_mesh, tabI4, fk_nat, md.isp.nb,
                               md.isp.n_mesh, md.i_reg, (const float*)oj, B, st);
    }
    hipLaunchKernelGGL(k_etile_cond<true>, dim3(cond_blocks), dim3(kCondWaves * 64), lds_bytes, s, *mdev, md.n_layers, (const float*)st, B, oj, s1);
#define WF_EPRIOR(JT_, DERIV_)                                                                                                                        \
    hipLaunchKernelGGL((k_etile_prior<JT_, DERIV_>), dim3(lane_blocks), dim3(256), 0, s, mdev->comp + (size_t)md.n_layers * mdev->n_mesh, tabP4, md.psp.nb, \
                       md.psp.n_mesh, md.constrained_mask, (const float*)oj, (const float*)s1, (const float*)st, x, B, pr, hpsi, psi, lap, grad, hdiag)
    if (out == 2) WF_EPRIOR(J5, true);
    else if (out == 1) WF_EPRIOR(J, true);
    else WF_EPRIOR(J, false);
#undef WF_EPRIOR
    return check();
}
int launch_energy_tile(const MfmaDev* mdev, const ModelDev& md, const float* tabI4, const float* tabP4, const float* fk_nat, const float* x, int64_t B,
                       const Protons& pr, float* hpsi, float* psi, float* lap, float* ws, void* stream, float* st_out) {
    return launch_tile(mdev, md, tabI4, tabP4, fk_nat, x, B, pr, hpsi, psi, lap, ws, stream, st_out, nullptr, nullptr);
}
int launch_derivs_tile(const MfmaDev* mdev, const ModelDev& md, const float* tabI4, const float* tabP4, const float* fk_nat, const float* x, int64_t B,
                       float* psi, float* grad, float* hdiag, float* ws, void* stream) {
    if (!grad) return WF_ERR_INVALID;
    return launch_tile(mdev, md, tabI4, tabP4, fk_nat, x, B, Protons{}, nullptr, psi, nullptr, ws, stream, nullptr, grad, hdiag);
}

}  // namespace wf
