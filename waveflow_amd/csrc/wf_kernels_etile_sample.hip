// wf_kernels_etile_sample.hip -- inverse / sampler of large batches on the matrix cores (two-particle family).
// Serial.inverse_fun / the Waveflow prior's sample_fun (made.py:85-100, bsplines_jax.py:144-171) for batches the one-walker-per-wave kernel
// (wf_kernels_wave.hip: 6.8e7 walkers/s, a chain of dependent reads per walker) is too slow for.  Staged: the conditioner of a net runs on the
// matrix cores for the whole batch (k_etile_cond: head outputs to HBM, 384 B per walker), everything else is one lane per walker (k_tsample):
//   dimension 0 of a net does not depend on the walker: its spline is the composite table comp[net] (k_prepare_dim0), inverted by a binary
//     search over the mesh; the prior's first column is drawn by rejection under the table's own maximum (tight: the lerp of P is piecewise
//     linear, so P^2 peaks at a mesh point)
//   dimension 1: coefficients c_j = g_j (v_j / S0 + reg) / Q from the head outputs (as k_etile_flow), the spline sum_j c_j I_j inverted by the
//     same search with 32-term row sums; the prior's second column by rejection from a piecewise-constant envelope over the knot intervals
//     (the largest of the k + 1 B-spline coefficients alive on an interval: k_tsample, phase 1) -- the reference proposes uniformly under the
//     global bound max_i ((e @ b_to_ob)_i)^2: the same law at 2.5 x the acceptance rate
//   the root of a search is rounded to the reference's halving grid exactly as wf_kernels_wave.hip: ispline_inverse does (largest grid point
//     whose table-lerp value does not exceed y)
// Streams: Philox4x32-10 keyed by (seed, walker), proposal n of column col uses counter (n, col + 1) -- as the wave sampler; the draws differ
// from that kernel's (other proposal sequences), their law does not.
#include <hip/hip_runtime.h>

#include "wf_etile_cond.h"
#include "wf_philox.h"   // (behind the contraction pragma of wf_etile_common.h, like the rest of this unit)

namespace wf {
namespace {
struct TsArgs {
    const float4_t* comp;      // [n_nets][n_mesh] composite tables of dimension 0 (flow nets: Y; prior: P with sign and norm)
    const float* tabI0;        // order-0 rows of the I-spline table [n_mesh][32]
    const float* tabP0;        // order-0 rows of the prior's table [n_mesh][32]
    const float* gI;           // [32] row factors of the flow heads (boundary map; 0 beyond the bases)
    const float* b_to_ob;      // [32][32]
    const float* tabB0;        // plain B-splines of the prior, order 0 [n_mesh][NB] (with ow: the band-limited evaluation of a proposal), or null
    const float* ow;           // the prior's o * keep of the conditioner launch ([tile][row][32 walkers]) where they are the plain B-spline coefficients of c, or null
    int n_mesh, nbI, nbP, n_layers, degP;
    int i_band_int;            // > 0: knot intervals of the I-splines, and their rows are plain (exactly 1 left of a band of k + 1 <= 8 rows, 0 right of it): the band form of phase 2
    float i_reg, tol, box_L;
    unsigned long long seed;
    const unsigned long long* seed_offset_dev;
    int exact;
    int64_t b0;                // index of the chunk's first walker in the batch (the key of a walker's stream is its index in the batch)
};
// largest mesh point m with F(m) <= y (0 if there is none), F monotone on the mesh; yl = F(m), yr = F(m + 1) (yr = yl at the last point)
template <class F>
__device__ __forceinline__ void mesh_search(F f, int last, float y, int& m, float& yl, float& yr) {
    int lo = 0, hi = last;
    float flo = f(0), fhi = f(last);
    const bool beyond = fhi <= y;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        const float fm = f(mid);
        if (fm <= y) { lo = mid; flo = fm; } else { hi = mid; fhi = fm; }
    }
    m = beyond ? last : lo;
    yl = beyond ? fhi : flo;
    yr = fhi;
}
// the root on the line through the two mesh values, rounded down to the halving grid 2^-K of helpers.binary_search; the table lerp itself decides
// between the neighbouring grid points (wf_kernels_wave.hip: ispline_inverse)
template <class FL>
__device__ __forceinline__ float grid_root(FL flerp, int m, float yl, float yr, float y, int last, float tol) {
    const float n = (float)last;
    float xs = (float)m / n;
    if (yr > yl) xs = xs + (y - yl) / ((yr - yl) * n);
    int K = 0;
    float w = 1.0f;
    while (K < 64 && w * 0.5f > tol * 0.5f) { w *= 0.5f; ++K; }
    const float scale = ldexpf(1.0f, K);
    float q = floorf(xs * scale);
    q = fminf(fmaxf(q, 0.0f), scale - 1.0f);
    const float f_lo = flerp(q / scale) - y, f_hi = flerp(fminf(q + 1.0f, scale - 1.0f) / scale) - y;
    if (f_hi <= 0.0f && q + 1.0f <= scale - 1.0f) q = q + 1.0f;
    else if (f_lo > 0.0f && q >= 1.0f) q = q - 1.0f;
    return q / scale;
}
__device__ __forceinline__ float comp_lerp_x(const float4_t* __restrict__ comp, float x, int n_mesh) {
    const LerpN L = nlerp(x, n_mesh);
    const float a = comp[L.il].x, b = comp[L.ir].x;
    return __builtin_fmaf(b - a, L.t, a);
}
__device__ __forceinline__ float inv_comp(const float4_t* __restrict__ comp, int n_mesh, float y, float tol) {
    int m;
    float yl, yr;
    mesh_search([&](int i) { return comp[i].x; }, n_mesh - 1, y, m, yl, yr);
    return grid_root([&](float x) { return comp_lerp_x(comp, x, n_mesh); }, m, yl, yr, y, n_mesh - 1, tol);
}
template <int NB>
__device__ __forceinline__ float rows_dot(const float* __restrict__ row, const float (&c)[NB]) {   // sum_j c_j row[j], j ascending
    const float4_t* r4 = reinterpret_cast<const float4_t*>(row);
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < NB / 4; ++q) {
        const float4_t t = r4[q];
        acc = __builtin_fmaf(c[4 * q], t.x, acc);
        acc = __builtin_fmaf(c[4 * q + 1], t.y, acc);
        acc = __builtin_fmaf(c[4 * q + 2], t.z, acc);
        acc = __builtin_fmaf(c[4 * q + 3], t.w, acc);
    }
    return acc;
}
template <int NB>
__device__ __forceinline__ float rows_lerp(const float* __restrict__ tab0, const float (&c)[NB], float x, int n_mesh) {
    const LerpN L = nlerp(x, n_mesh);
    const float4_t* ra = reinterpret_cast<const float4_t*>(tab0 + (size_t)L.il * NB);
    const float4_t* rb = reinterpret_cast<const float4_t*>(tab0 + (size_t)L.ir * NB);
    float acc = 0.0f;
    constexpr int kQ = NB / 4;
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
        const float4_t a = ra[q], b = rb[q];
        acc = __builtin_fmaf(c[4 * q], __builtin_fmaf(b.x - a.x, L.t, a.x), acc);
        acc = __builtin_fmaf(c[4 * q + 1], __builtin_fmaf(b.y - a.y, L.t, a.y), acc);
        acc = __builtin_fmaf(c[4 * q + 2], __builtin_fmaf(b.z - a.z, L.t, a.z), acc);
        acc = __builtin_fmaf(c[4 * q + 3], __builtin_fmaf(b.w - a.w, L.t, a.w), acc);
    }
    return acc;
}
template <int NB>
__device__ __forceinline__ float inv_rows(const float* __restrict__ tab0, const float (&c)[NB], int n_mesh, float y, float tol) {
    int m;
    float yl, yr;
    mesh_search([&](int i) { return rows_dot<NB>(tab0 + (size_t)i * NB, c); }, n_mesh - 1, y, m, yl, yr);
    return grid_root([&](float x) { return rows_lerp<NB>(tab0, c, x, n_mesh); }, m, yl, yr, y, n_mesh - 1, tol);
}
// ... with plain I-spline rows (TsArgs::i_band_int): at mesh point i only the rows s .. s + k of knot interval s = floor(x_i n_int) are neither 1 nor 0, so
// sum_j c_j T[i][j] = (sum of the c_j left of a window of 12 rows from a multiple of four) + (the window's terms): three 16-byte records per row instead of
// NB / 4, in the order of the full sum -- the same bits (a row of ones adds c_j, a row of zeros nothing).  cs: the walker's coefficients, p4: their prefix
// sums at the multiples of four, both in LDS (the window moves with the mesh point).  A lerp between neighbouring mesh points needs s .. s + k + 1: k <= 7.
template <int NB>
__device__ __forceinline__ float inv_rows_band(const float* __restrict__ tab0, const float* cs, const float* p4, int n_int, int n_mesh, float y, float tol) {
    auto window = [&](int i) { return min(min((i * n_int) / (n_mesh - 1), n_int - 1) & ~3, NB - 12); };
    auto dot_at = [&](int i) {
        const int a0 = window(i);
        const float4_t* r = reinterpret_cast<const float4_t*>(tab0 + (size_t)i * NB + a0);
        const float4_t* cq = reinterpret_cast<const float4_t*>(cs + a0);
        float acc = p4[a0 >> 2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4_t t = r[q], c = cq[q];
            acc = __builtin_fmaf(c.x, t.x, acc);
            acc = __builtin_fmaf(c.y, t.y, acc);
            acc = __builtin_fmaf(c.z, t.z, acc);
            acc = __builtin_fmaf(c.w, t.w, acc);
        }
        return acc;
    };
    auto lerp_at = [&](float x) {
        const LerpN L = nlerp(x, n_mesh);
        const int a0 = window(min(L.il, L.ir));
        const float4_t* ra = reinterpret_cast<const float4_t*>(tab0 + (size_t)L.il * NB + a0);
        const float4_t* rb = reinterpret_cast<const float4_t*>(tab0 + (size_t)L.ir * NB + a0);
        const float4_t* cq = reinterpret_cast<const float4_t*>(cs + a0);
        float acc = p4[a0 >> 2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4_t ta = ra[q], tb = rb[q], c = cq[q];
            acc = __builtin_fmaf(c.x, __builtin_fmaf(tb.x - ta.x, L.t, ta.x), acc);
            acc = __builtin_fmaf(c.y, __builtin_fmaf(tb.y - ta.y, L.t, ta.y), acc);
            acc = __builtin_fmaf(c.z, __builtin_fmaf(tb.z - ta.z, L.t, ta.z), acc);
            acc = __builtin_fmaf(c.w, __builtin_fmaf(tb.w - ta.w, L.t, ta.w), acc);
        }
        return acc;
    };
    int m;
    float yl, yr;
    mesh_search(dot_at, n_mesh - 1, y, m, yl, yr);
    return grid_root(lerp_at, m, yl, yr, y, n_mesh - 1, tol);
}
// channel 0 of the head outputs of walker b: oj[tile][row 0 .. NB)[channel][32 walkers]
template <int NB>
__device__ __forceinline__ float oj0(const float* __restrict__ oj, int64_t b, int row) { return oj[((b >> 5) * NB + row) * 32 + (b & 31)]; }   // (k_etile_cond<., ., 1>: the value channel alone)

// phase 0: prior column 0;  1: prior column 1, then the last layer's dimension 0;  2: dimension 1 of layer `layer`, then dimension 0 of the layer before it
// (layer 0: the box reverse and the result);  3: entry of a plain inverse (latent given): the last layer's dimension 0.
// Between the phases: cur0 = the inverted dimension 0, cur1 = the value waiting for dimension 1, cin = what the conditioner of the next launch sees
// (exact: the inverted prefix; reference mode, made.py:88: the value being inverted).
// NB: padded bases per dimension (32, or 64: two row blocks -- there the rejection loop of the second column stays on the walker's own lane)
template <int PHASE, int NB>
__global__ __launch_bounds__(256, 2) void k_tsample(const TsArgs a, int layer, const float* __restrict__ oj, const float* __restrict__ ug, int64_t B,
                                                 float* __restrict__ cur0, float* __restrict__ cur1, float* __restrict__ cin, float* __restrict__ lat,
                                                 float* __restrict__ latent_out, float* __restrict__ xg) {
    __shared__ float red[256];
    // phase 1, band form: the plain B-spline coefficients q of every walker of the workgroup, one row per lane (+ 4: rows stay 16-byte aligned and
    // fall on different banks)
    constexpr int kQStride = NB + 4;
    constexpr bool kBand2 = PHASE == 2;   // phase 2, band form (inv_rows_band): the walker's spline coefficients and their prefix sums (two row blocks: 90 KB, one
                                                      // workgroup per CU instead of two -- and still 0.537 -> 0.450 ms per 2^17 draws of the 33-knot model)
    __shared__ __attribute__((aligned(16))) float qs[(PHASE == 1 || kBand2) ? 256 * kQStride : 4];
    __shared__ __attribute__((aligned(16))) float p4s[kBand2 ? 256 * (NB / 4 + 4) : 4];
    constexpr int phase = PHASE;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n_mesh = a.n_mesh;
    unsigned long long seed = a.seed;
    if (a.seed_offset_dev) seed += *a.seed_offset_dev * 0x9E3779B97F4A7C15ull;
    // phase 0: piecewise-constant envelope of the first column's density P^2 (the same for every walker): kBins equal bins of [0, 1], M_j = the largest P^2 at
    // the mesh points of the cells that meet bin j (the lerp of P is piecewise linear: P^2 peaks at a mesh point), red[j] = M_j, red[kBins + j] = sum_{i < j} M_i.
    // Round 3 proposed uniformly under the global maximum: the same law at a fifth of the acceptance rate (34 us of the sampler's 228 at 2^17 walkers).
    constexpr int kBins = 64;
    if (phase == 0) {
        const float4_t* cp = a.comp + (size_t)a.n_layers * n_mesh;
        if (threadIdx.x < kBins) {
            const int j = threadIdx.x;
            const int m0 = max((int)floorf((float)j / kBins * (float)(n_mesh - 1)) - 1, 0), m1 = min((int)ceilf((float)(j + 1) / kBins * (float)(n_mesh - 1)) + 1, n_mesh - 1);
            float mx = 0.0f;
            for (int i = m0; i <= m1; ++i) { const float pv = cp[i].x; mx = fmaxf(mx, pv * pv); }
            red[j] = mx;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            float run = 0.0f;
            for (int j = 0; j < kBins; ++j) { red[kBins + j] = run; run += red[j]; }
            red[2 * kBins] = run;
        }
        __syncthreads();
    }
    if (b >= B) return;
    // the next layer's dimension 0 from the pair (va, vb) that leaves a layer (or the prior): Reverse.inverse_fun, then the composite table
    auto start_layer = [&](int l, float va, float vb) {
        const float n0 = vb, n1 = va;
        const float o0 = inv_comp(a.comp + (size_t)l * n_mesh, n_mesh, n0, a.tol);
        cur0[b] = o0;
        cur1[b] = n1;
        cin[b] = a.exact ? o0 : n0;
    };
    if (phase == 0) {
        const float4_t* cp = a.comp + (size_t)a.n_layers * n_mesh;
        const float tot = red[2 * kBins];
        float xs = __builtin_nanf("");
        for (int n = 0; n < 100000; ++n) {
            Philox prop(seed, (unsigned long long)(a.b0 + b));
            prop.c0 = (unsigned)n;
            prop.c1 = 1u;
            const float t = prop.uniform() * tot, u2 = prop.uniform();
            int j = 0;      // the last bin whose prefix sum does not exceed t
#pragma unroll
            for (int step = kBins / 2; step > 0; step >>= 1) j = red[kBins + j + step] <= t ? j + step : j;
            const float mj = red[j];
            if (!(mj > 0.0f)) continue;
            const float xc = fminf(((float)j + fminf((t - red[kBins + j]) / mj, 1.0f)) * (1.0f / kBins), 0.99999994f);
            const float p = comp_lerp_x(cp, xc, n_mesh);
            if (u2 * mj < p * p) { xs = xc; break; }
        }
        lat[b] = xs;
        cin[b] = xs;
        cin[4 * B + b] = 0.0f;
        return;
    }
    if (phase == 3) {
        cin[4 * B + b] = 0.0f;
        start_layer(a.n_layers - 1, ug[b * 2], ug[b * 2 + 1]);
        return;
    }
    if (phase == 1) {
        // e = c / |c| with c = (o keep) @ ob_to_b from the conditioner launch; bound max_i ((e @ b_to_ob)_i)^2 (bsplines_jax.py:164-166)
        float e[NB];
        float ss = 0.0f;
#pragma unroll
        for (int j = 0; j < NB; ++j) { e[j] = j < a.nbP ? oj0<NB>(oj, b, j) : 0.0f; ss = __builtin_fmaf(e[j], e[j], ss); }
        const float rn = 1.0f / sqrtf(ss);
#pragma unroll
        for (int j = 0; j < NB; ++j) e[j] = e[j] * rn;
        // q = e @ b_to_ob are the coefficients of this column's factor f = sum_i q_i b_i in the plain B-splines (non-negative, summing to one), so
        // |f| <= max_i |q_i| (the reference's bound, bsplines_jax.py:164-166) and, on the knot interval s where only b_s .. b_{s + k} live,
        // |f| <= M_s = max(|q_s| .. |q_{s + k}|).  Proposals are drawn from the piecewise-constant envelope M_s^2 (one uniform picks the interval and the
        // point in it) and accepted against M_s^2: the same law as the reference's uniform proposals under the global bound, at 5 - 8 x its acceptance rate.
        float aq[NB];
        const bool band = a.ow != nullptr && a.tabB0 != nullptr;
        if (a.ow) {   // (the boundary map only zeroes coefficients: q = e @ b_to_ob = (o keep) / |c|, the product is the identity; round 4)
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const float qi = i < a.nbP ? oj0<NB>(a.ow, b, i) * rn : 0.0f;
                aq[i] = qi * qi;
                if (PHASE == 1) qs[threadIdx.x * kQStride + i] = qi;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                float acc = 0.0f;
#pragma unroll
                for (int j = 0; j < NB; ++j) acc = __builtin_fmaf(e[j], a.b_to_ob[j * NB + i], acc);
                aq[i] = i < a.nbP ? acc * acc : 0.0f;
            }
        }
        const int n_int = a.nbP - a.degP;       // knot intervals of equal width on [0, 1] (knots: linspace, the end knots (k + 1)-fold)
        float msq[NB], tot = 0.0f;
#pragma unroll
        for (int sI = 0; sI < NB; ++sI) {
            float mx = 0.0f;
#pragma unroll
            for (int d = 0; d <= 8; ++d)
                if (sI + d < NB && d <= a.degP) mx = fmaxf(mx, aq[sI + d]);
            msq[sI] = sI < n_int ? mx : 0.0f;
            tot += msq[sI];
        }
        const float wI = 1.0f / (float)n_int;
        // one proposal (number n of walker wb's sequence) against the envelope (mq, mtot) of the factor with coefficients ec
        auto propose = [&](unsigned long long wb, int n, const float (&ec)[NB], const float (&mq)[NB], float mtot, float& xc, int qrow) {
            Philox prop(seed, wb);
            prop.c0 = (unsigned)n;
            prop.c1 = 2u;
            // (__fmul_rn: the product must not contract into the subtraction t - base below -- k_tsample_p1g draws the same numbers only if both round it)
            const float t = __fmul_rn(prop.uniform(), mtot), u2 = prop.uniform();
            float run = 0.0f, base = 0.0f, msel = mq[0];
            int ssel = 0;
#pragma unroll
            for (int sI = 0; sI < NB; ++sI) {   // (the last interval with a positive bound catches t == mtot)
                const bool hit = t >= run && mq[sI] > 0.0f;
                ssel = hit ? sI : ssel;
                base = hit ? run : base;
                msel = hit ? mq[sI] : msel;
                run += mq[sI];
            }
            xc = fminf(((float)ssel + fminf((t - base) / msel, 1.0f)) * wI, 0.99999994f);
            float v;
            if (band) {
                // f(x) = sum_i q_i b_i(x) over the k + 1 plain B-splines alive on knot interval ssel (b_ssel .. b_{ssel + k}, k <= 8): a window of 12
                // coefficients from a multiple of four (the rest of the window multiplies zeros of the table) -- three 16-byte records per table row
                // and lerp end instead of NB / 4, three of the walker's row in LDS (qrow: its own lane's, or the lane's it is served by)
                const int a0 = min(ssel & ~3, NB - 12);
                const LerpN Lx = nlerp(xc, n_mesh);
                const float4_t* ra = reinterpret_cast<const float4_t*>(a.tabB0 + (size_t)Lx.il * NB + a0);
                const float4_t* rb = reinterpret_cast<const float4_t*>(a.tabB0 + (size_t)Lx.ir * NB + a0);
                const float4_t* qr = reinterpret_cast<const float4_t*>(qs + qrow * kQStride + a0);
                v = 0.0f;
#pragma unroll
                for (int qq = 0; qq < 3; ++qq) {
                    const float4_t ta = ra[qq], tb = rb[qq], qv = qr[qq];
                    v = __builtin_fmaf(qv.x, __builtin_fmaf(tb.x - ta.x, Lx.t, ta.x), v);
                    v = __builtin_fmaf(qv.y, __builtin_fmaf(tb.y - ta.y, Lx.t, ta.y), v);
                    v = __builtin_fmaf(qv.z, __builtin_fmaf(tb.z - ta.z, Lx.t, ta.z), v);
                    v = __builtin_fmaf(qv.w, __builtin_fmaf(tb.w - ta.w, Lx.t, ta.w), v);
                }
            } else {
                v = rows_lerp<NB>(a.tabP0, ec, xc, n_mesh);
            }
            return u2 * msel < v * v;
        };
        // Stage A: every lane proposes for its own walker, kTsOwn times at most (88 % of the walkers are done by then).  Stage B: the wave's remaining
        // walkers get eight lanes each, eight consecutive proposals of a walker's sequence per round, the first accepted one in sequence order taken --
        // the same draws as one lane proposing on alone, without the wave waiting 80 rounds for its unluckiest lane.
        constexpr int kTsOwn = 16;   // (the draws do not depend on it.  2^17 draws, round 4: 16 own proposals 0.281 ms, 12: 0.283, 8: 0.287, 4: 0.294)
        // n_prop (with rounds / rmine below): the walker's number of proposals, which nothing reads any more.  Without them hipcc's code for
        // k_tsample<1, 32> differs (142 spilled SGPRs instead of 140), so they go in a change of their own that is measured on the GPU.
        [[maybe_unused]] int n_prop = 0;
        float xs = __builtin_nanf("");
        bool done = false;
        const unsigned long long wb_own = (unsigned long long)(a.b0 + b);
        for (int n = 0; n < kTsOwn; ++n) {
            float xc;
            n_prop = n + 1;
            if (propose(wb_own, n, e, msq, tot, xc, (int)threadIdx.x)) { xs = xc; done = true; break; }
        }
        if (NB > 32 || __ballot(true) != ~0ull) {
            // the batch's last, partial wave: lanes are missing from the groups, every walker keeps its own lane (and with two row blocks the
            // coefficients of a walker are too many to hand to other lanes)
            for (int n = kTsOwn; n < 100000 && !done; ++n) {
                float xc;
                n_prop = n + 1;
                if (propose(wb_own, n, e, msq, tot, xc, (int)threadIdx.x)) { xs = xc; done = true; }
            }
        } else {
            const int lane = threadIdx.x & 63, g = lane >> 3, r = lane & 7;
            unsigned long long rem = __ballot(!done);
            for (int pass = 0; pass < 64 && rem; ++pass) {
                // group g serves the g-th walker of `rem`
                unsigned long long mm = rem;
                for (int i = 0; i < g; ++i) mm &= mm - 1;
                const bool has = mm != 0;
                const int src = has ? __ffsll((long long)mm) - 1 : lane;
                float ew[NB], mw[NB];
#pragma unroll
                for (int j = 0; j < NB; ++j) { ew[j] = band ? 0.0f : __shfl(e[j], src); mw[j] = __shfl(msq[j], src); }   // (band form: the served walker's coefficients are read from its LDS row)
                const float totw = __shfl(tot, src);
                const unsigned wlo = __shfl((unsigned)(wb_own & 0xFFFFFFFFull), src), whi = __shfl((unsigned)(wb_own >> 32), src);
                const unsigned long long wbw = ((unsigned long long)whi << 32) | wlo;
                float xw = __builtin_nanf("");
                bool found = !has;
                int rounds = 0;
                for (int round = 0; round < (100000 - kTsOwn) / 8; ++round) {
                    float xc = 0.0f;
                    const bool acc = !found && propose(wbw, kTsOwn + round * 8 + r, ew, mw, totw, xc, (int)(threadIdx.x & ~63u) + src);
                    const unsigned long long hits = __ballot(acc);
                    const unsigned gh = (unsigned)(hits >> (8 * g)) & 0xFFu;
                    const float xfirst = __shfl(xc, 8 * g + (gh ? __ffs((int)gh) - 1 : 0));
                    if (!found) rounds = round + 1;
                    if (!found && gh) { xw = xfirst; found = true; }
                    if (__ballot(!found) == 0ull) break;
                }
                // the walkers served in this pass take their draws from the first lane of their group
                const int rank = __popcll(rem & ((1ull << lane) - 1ull));
                const float xmine = __shfl(xw, 8 * (rank & 7));
                const int rmine = __shfl(rounds, 8 * (rank & 7));
                if (!done && rank < 8) { xs = xmine; done = true; n_prop = kTsOwn + 8 * rmine; }
                rem = __ballot(!done);
            }
        }
        const float l0 = lat[b];
        if (latent_out) { latent_out[b * 2] = l0; latent_out[b * 2 + 1] = xs; }
        start_layer(a.n_layers - 1, l0, xs);
        return;
    }
    // phase 2: c_j = g_j (v_j / S0 + reg) / Q (calculate_bijection_params + reg, remove_bias, boundary map), v_j = 1 / (2^o_j + 1)
    float c[NB];
    float S0 = 0.0f, Qv = 0.0f, G = 0.0f;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const float g = a.gI[j];
        const float v = j < a.nbI ? r_of(oj0<NB>(oj, b, j)) : 0.0f;
        c[j] = v;
        S0 += v;
        Qv = __builtin_fmaf(v, g, Qv);
        G += j < a.nbI ? g : 0.0f;
    }
    const float rS = 1.0f / S0, rQ = 1.0f / __builtin_fmaf(Qv, rS, a.i_reg * G);
#pragma unroll
    for (int j = 0; j < NB; ++j) c[j] = j < a.nbI ? (a.gI[j] * __builtin_fmaf(c[j], rS, a.i_reg)) * rQ : 0.0f;
    const float o0 = cur0[b];
    float o1;
    if (kBand2 && a.i_band_int > 0) {
        float* cs = qs + threadIdx.x * kQStride;
        float* p4 = p4s + threadIdx.x * (NB / 4 + 4);
        float run = 0.0f;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            if ((j & 3) == 0) p4[j >> 2] = run;
            cs[j] = c[j];
            run = __builtin_fmaf(c[j], 1.0f, run);     // (as the full sum meets a row of ones)
        }
        o1 = inv_rows_band<NB>(a.tabI0, cs, p4, a.i_band_int, n_mesh, cur1[b], a.tol);
    } else {
        o1 = inv_rows<NB>(a.tabI0, c, n_mesh, cur1[b], a.tol);
    }
    if (layer > 0) {
        start_layer(layer - 1, o0, o1);
        return;
    }
    // BoxTransformLayer.reverse_fun_mean (made.py:186-197), two particles
    const float mean = 0.5f * o0, pm = o1 * (1.0f - o0) - (0.5f - mean);
    xg[b * 2] = ((0.0f - mean) + pm) * 2.0f * a.box_L;
    xg[b * 2 + 1] = ((o0 - mean) + pm) * 2.0f * a.box_L;
}

// Phase 1 of the staged sampler with EIGHT LANES PER WALKER from the start (band form only: TsArgs::ow and ::tabB0 set).  k_tsample<1> walks a walker's
// proposals one after the other on its own lane -- ~20 dependent table round trips per wave at two waves per SIMD (64 % of its cycles wait on memory).  Here lane
// r of a walker's group tests proposal 8 * round + r; the first accepted one in sequence order is taken: the same draws, ~3 round trips, sixteen waves per SIMD.
// Everything whose rounding depends on the order of a sum (|c|^2, the prefix sums of the envelope) is summed by the group's first lane in k_tsample<1>'s order.
template <int NB>
__global__ __launch_bounds__(256) void k_tsample_p1g(const TsArgs a, const float* __restrict__ oj, int64_t B, float* __restrict__ cur0, float* __restrict__ cur1,
                                                    float* __restrict__ cin, const float* __restrict__ lat, float* __restrict__ latent_out) {
    constexpr int kStride = NB + 12;     // (+ 8: the envelope reads aq[s .. s + 8]; rows stay 16-byte aligned)
    __shared__ __attribute__((aligned(16))) float qs[32 * kStride], aqs[32 * kStride], mqs[32 * kStride], cums[32 * kStride];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = t >> 3;
    const int r = threadIdx.x & 7, gl = (threadIdx.x & 63) >> 3, wrow = threadIdx.x >> 3, lane = threadIdx.x & 63;
    const bool valid = b < B;
    const int64_t bl = valid ? b : B - 1;
    const int n_mesh = a.n_mesh;
    unsigned long long seed = a.seed;
    if (a.seed_offset_dev) seed += *a.seed_offset_dev * 0x9E3779B97F4A7C15ull;
    float* q = qs + wrow * kStride;
    float* aq = aqs + wrow * kStride;
    float* mq = mqs + wrow * kStride;
    float* cum = cums + wrow * kStride;
    // |c|^2 in k_tsample<1>'s order (j ascending, fused multiply-adds) by the group's first lane
    float rn = 0.0f;
    if (r == 0) {
        float ss = 0.0f;
#pragma unroll 8
        for (int j = 0; j < NB; ++j) { const float cj = j < a.nbP ? oj0<NB>(oj, bl, j) : 0.0f; ss = __builtin_fmaf(cj, cj, ss); }
        rn = 1.0f / sqrtf(ss);
    }
    rn = __shfl(rn, lane & ~7);
#pragma unroll
    for (int jj = 0; jj < NB / 8 + 1; ++jj) {       // (+ 1: the eight slots behind the row, zeros for the envelope's look-ahead)
        const int j = r + 8 * jj;
        const float qi = (j < a.nbP) ? oj0<NB>(a.ow, bl, j) * rn : 0.0f;
        q[j] = qi;
        aq[j] = qi * qi;
    }
    const int n_int = a.nbP - a.degP;
#pragma unroll
    for (int jj = 0; jj < NB / 8; ++jj) {
        const int sI = r + 8 * jj;
        float mx = 0.0f;
#pragma unroll
        for (int d = 0; d <= 8; ++d)
            if (sI + d < NB && d <= a.degP) mx = fmaxf(mx, aq[sI + d]);
        mq[sI] = sI < n_int ? mx : 0.0f;
    }
    float tot = 0.0f;
    if (r == 0) {
#pragma unroll 8
        for (int sI = 0; sI < NB; ++sI) { cum[sI] = tot; tot += mq[sI]; }
    }
    tot = __shfl(tot, lane & ~7);
    const float wI = 1.0f / (float)n_int;
    const unsigned long long wb = (unsigned long long)(a.b0 + bl);
    bool found = !valid;
    float xw = __builtin_nanf("");
    for (int round = 0; round < 12500; ++round) {
        bool acc = false;
        float xc = 0.0f;
        if (!found) {
            Philox prop(seed, wb);
            prop.c0 = (unsigned)(round * 8 + r);
            prop.c1 = 2u;
            const float tt = __fmul_rn(prop.uniform(), tot), u2 = prop.uniform();
            // the last interval with cum <= tt and a positive bound (k_tsample<1>'s scan)
            int sI = 0;
#pragma unroll
            for (int step = NB / 2; step > 0; step >>= 1) sI = cum[sI + step] <= tt ? sI + step : sI;
            while (sI > 0 && !(mq[sI] > 0.0f)) --sI;
            const float msel = mq[sI], base = cum[sI];
            xc = fminf(((float)sI + fminf((tt - base) / msel, 1.0f)) * wI, 0.99999994f);
            const int a0 = min(sI & ~3, NB - 12);
            const LerpN Lx = nlerp(xc, n_mesh);
            const float4_t* ra = reinterpret_cast<const float4_t*>(a.tabB0 + (size_t)Lx.il * NB + a0);
            const float4_t* rb = reinterpret_cast<const float4_t*>(a.tabB0 + (size_t)Lx.ir * NB + a0);
            const float4_t* qr = reinterpret_cast<const float4_t*>(q + a0);
            float v = 0.0f;
#pragma unroll
            for (int qq = 0; qq < 3; ++qq) {
                const float4_t ta = ra[qq], tb = rb[qq], qv = qr[qq];
                v = __builtin_fmaf(qv.x, __builtin_fmaf(tb.x - ta.x, Lx.t, ta.x), v);
                v = __builtin_fmaf(qv.y, __builtin_fmaf(tb.y - ta.y, Lx.t, ta.y), v);
                v = __builtin_fmaf(qv.z, __builtin_fmaf(tb.z - ta.z, Lx.t, ta.z), v);
                v = __builtin_fmaf(qv.w, __builtin_fmaf(tb.w - ta.w, Lx.t, ta.w), v);
            }
            acc = u2 * msel < v * v;
        }
        const unsigned long long hits = __ballot(acc);
        const unsigned gh = (unsigned)(hits >> (8 * gl)) & 0xFFu;
        const float xfirst = __shfl(xc, 8 * gl + (gh ? __ffs((int)gh) - 1 : 0));
        if (!found && gh) { xw = xfirst; found = true; }
        if (__ballot(!found) == 0ull) break;
    }
    if (valid && r == 0) {
        const float l0 = lat[b];
        if (latent_out) { latent_out[b * 2] = l0; latent_out[b * 2 + 1] = xw; }
        // the last layer's dimension 0 from the pair that leaves the prior (k_tsample: start_layer)
        const int l = a.n_layers - 1;
        const float o0 = inv_comp(a.comp + (size_t)l * n_mesh, n_mesh, xw, a.tol);
        cur0[b] = o0;
        cur1[b] = l0;
        cin[b] = a.exact ? o0 : xw;
    }
}

// mesh_search with the eight lanes of a walker's group (lane r of the group; all eight call it together): eight probes per round between lo and hi instead of the
// midpoint -- four rounds for 2 000 mesh points instead of eleven.  F is monotone on the mesh, so the result (the largest m with F(m) <= y, F(m), F(m + 1)) is the
// one mesh_search finds, bit for bit.
template <class F>
__device__ __forceinline__ void group_mesh_search(F f, int last, float y, int r, int gbase, int& m, float& yl, float& yr) {
    int lo = 0, hi = last;
    const float fe = r == 0 ? f(0) : (r == 1 ? f(last) : 0.0f);
    float flo = __shfl(fe, gbase), fhi = __shfl(fe, gbase + 1);
    const bool beyond = fhi <= y;
    while (hi - lo > 1) {
        const int span = hi - lo;
        const int p = span > 8 ? lo + (int)(((long long)span * (r + 1)) / 9) : lo + 1 + r;      // (distinct, ascending in r, strictly between lo and hi where used)
        const bool use = p < hi;
        const float fp = use ? f(p) : 0.0f;
        const unsigned le = (unsigned)(__ballot(use && fp <= y) >> (gbase & 63)) & 0xFFu;         // monotone: the lanes with F <= y are the first few
        const unsigned usem = (unsigned)(__ballot(use) >> (gbase & 63)) & 0xFFu;
        const int k = __popc(le);                                                                  // probes 0 .. k - 1 lie at or below y
        const int n_use = __popc(usem);
        const int plo = __shfl(p, gbase + (k > 0 ? k - 1 : 0)), phi = __shfl(p, gbase + (k < 8 ? k : 7));
        const float vlo = __shfl(fp, gbase + (k > 0 ? k - 1 : 0)), vhi = __shfl(fp, gbase + (k < 8 ? k : 7));
        if (k > 0) { lo = plo; flo = vlo; }
        if (k < n_use) { hi = phi; fhi = vhi; }
    }
    m = beyond ? last : lo;
    yl = beyond ? fhi : flo;
    yr = fhi;
}
// grid_root with the group: the two lerp values on lanes 0 and 1
template <class FL>
__device__ __forceinline__ float group_grid_root(FL flerp, int m, float yl, float yr, float y, int last, float tol, int r, int gbase) {
    const float n = (float)last;
    float xs = (float)m / n;
    if (yr > yl) xs = xs + (y - yl) / ((yr - yl) * n);
    int K = 0;
    float w = 1.0f;
    while (K < 64 && w * 0.5f > tol * 0.5f) { w *= 0.5f; ++K; }
    const float scale = ldexpf(1.0f, K);
    float q = floorf(xs * scale);
    q = fminf(fmaxf(q, 0.0f), scale - 1.0f);
    const float fv = r == 0 ? flerp(q / scale) - y : (r == 1 ? flerp(fminf(q + 1.0f, scale - 1.0f) / scale) - y : 0.0f);
    const float f_lo = __shfl(fv, gbase), f_hi = __shfl(fv, gbase + 1);
    if (f_hi <= 0.0f && q + 1.0f <= scale - 1.0f) q = q + 1.0f;
    else if (f_lo > 0.0f && q >= 1.0f) q = q - 1.0f;
    return q / scale;
}
// Phase 2 of the staged sampler / inverse with eight lanes per walker (band form of the spline sums: TsArgs::i_band_int > 0): the coefficients of dimension 1 in
// k_tsample<2>'s arithmetic (order-dependent sums by the group's first lane), both mesh searches of the phase as eight-way searches: 12 table round trips instead of 30,
// sixteen waves per SIMD instead of two; the same bits.
template <int NB>
__global__ __launch_bounds__(256) void k_tsample_p2g(const TsArgs a, int layer, const float* __restrict__ oj, int64_t B, float* __restrict__ cur0, float* __restrict__ cur1,
                                                    float* __restrict__ cin, float* __restrict__ xg) {
    constexpr int kStride = NB + 4;
    __shared__ __attribute__((aligned(16))) float cs_all[32 * kStride], p4_all[32 * (NB / 4 + 4)];
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = t >> 3;
    const int r = threadIdx.x & 7, lane = threadIdx.x & 63, gbase = lane & ~7, wrow = threadIdx.x >> 3;
    const bool valid = b < B;
    const int64_t bl = valid ? b : B - 1;
    const int n_mesh = a.n_mesh;
    float* cs = cs_all + wrow * kStride;
    float* p4 = p4_all + wrow * (NB / 4 + 4);
    // v_j = 1 / (2^o_j + 1) on the group's lanes, the sums S0, Qv, G in j order by its first lane (k_tsample<2>)
#pragma unroll
    for (int jj = 0; jj < NB / 8; ++jj) {
        const int j = r + 8 * jj;
        cs[j] = j < a.nbI ? r_of(oj0<NB>(oj, bl, j)) : 0.0f;
    }
    float rS = 0.0f, rQ = 0.0f;
    if (r == 0) {
        float S0 = 0.0f, Qv = 0.0f, G = 0.0f;
#pragma unroll 8
        for (int j = 0; j < NB; ++j) {
            const float g = a.gI[j], v = cs[j];
            S0 += v;
            Qv = __builtin_fmaf(v, g, Qv);
            G += j < a.nbI ? g : 0.0f;
        }
        rS = 1.0f / S0;
        rQ = 1.0f / __builtin_fmaf(Qv, rS, a.i_reg * G);
    }
    rS = __shfl(rS, gbase);
    rQ = __shfl(rQ, gbase);
#pragma unroll
    for (int jj = 0; jj < NB / 8; ++jj) {
        const int j = r + 8 * jj;
        cs[j] = j < a.nbI ? (a.gI[j] * __builtin_fmaf(cs[j], rS, a.i_reg)) * rQ : 0.0f;
    }
    if (r == 0) {
        float run = 0.0f;
#pragma unroll 8
        for (int j = 0; j < NB; ++j) {
            if ((j & 3) == 0) p4[j >> 2] = run;
            run = __builtin_fmaf(cs[j], 1.0f, run);
        }
    }
    const int n_int = a.i_band_int;
    auto window = [&](int i) { return min(min((i * n_int) / (n_mesh - 1), n_int - 1) & ~3, NB - 12); };
    auto dot_at = [&](int i) {
        const int a0 = window(i);
        const float4_t* rr = reinterpret_cast<const float4_t*>(a.tabI0 + (size_t)i * NB + a0);
        const float4_t* cq = reinterpret_cast<const float4_t*>(cs + a0);
        float acc = p4[a0 >> 2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4_t tv = rr[q], c = cq[q];
            acc = __builtin_fmaf(c.x, tv.x, acc);
            acc = __builtin_fmaf(c.y, tv.y, acc);
            acc = __builtin_fmaf(c.z, tv.z, acc);
            acc = __builtin_fmaf(c.w, tv.w, acc);
        }
        return acc;
    };
    auto lerp_at = [&](float x) {
        const LerpN L = nlerp(x, n_mesh);
        const int a0 = window(min(L.il, L.ir));
        const float4_t* ra = reinterpret_cast<const float4_t*>(a.tabI0 + (size_t)L.il * NB + a0);
        const float4_t* rb = reinterpret_cast<const float4_t*>(a.tabI0 + (size_t)L.ir * NB + a0);
        const float4_t* cq = reinterpret_cast<const float4_t*>(cs + a0);
        float acc = p4[a0 >> 2];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const float4_t ta = ra[q], tb = rb[q], c = cq[q];
            acc = __builtin_fmaf(c.x, __builtin_fmaf(tb.x - ta.x, L.t, ta.x), acc);
            acc = __builtin_fmaf(c.y, __builtin_fmaf(tb.y - ta.y, L.t, ta.y), acc);
            acc = __builtin_fmaf(c.z, __builtin_fmaf(tb.z - ta.z, L.t, ta.z), acc);
            acc = __builtin_fmaf(c.w, __builtin_fmaf(tb.w - ta.w, L.t, ta.w), acc);
        }
        return acc;
    };
    const float o0 = cur0[bl], y1 = cur1[bl];
    int m;
    float yl, yr;
    group_mesh_search(dot_at, n_mesh - 1, y1, r, gbase, m, yl, yr);
    const float o1 = group_grid_root(lerp_at, m, yl, yr, y1, n_mesh - 1, a.tol, r, gbase);
    if (layer > 0) {
        // the layer below: Reverse.inverse_fun, then its dimension 0 through the composite table (k_tsample: start_layer(layer - 1, o0, o1))
        const float4_t* comp = a.comp + (size_t)(layer - 1) * n_mesh;
        const float n0 = o1, n1 = o0;
        group_mesh_search([&](int i) { return comp[i].x; }, n_mesh - 1, n0, r, gbase, m, yl, yr);
        const float od = group_grid_root([&](float x) { return comp_lerp_x(comp, x, n_mesh); }, m, yl, yr, n0, n_mesh - 1, a.tol, r, gbase);
        if (valid && r == 0) {
            cur0[b] = od;
            cur1[b] = n1;
            cin[b] = a.exact ? od : n0;
        }
        return;
    }
    if (valid && r == 0) {
        // BoxTransformLayer.reverse_fun_mean (made.py:186-197), two particles
        const float mean = 0.5f * o0, pm = o1 * (1.0f - o0) - (0.5f - mean);
        xg[b * 2] = ((0.0f - mean) + pm) * 2.0f * a.box_L;
        xg[b * 2 + 1] = ((o0 - mean) + pm) * 2.0f * a.box_L;
    }
}

}  // namespace

// ---- host side of the staged inverse / sampler
bool tile_sample_capable(const MfmaDev* mdev) {
    return mdev->D == 2 && (mdev->nbk == 1 || mdev->nbk == 2) && mdev->n_layers > 0 && mdev->n_layers < 8 && !mdev->i_gate && !mdev->p_gate &&
           mdev->comp != nullptr && (mdev->const_floats + mdev->net_floats) * 4 <= 160 * 1024 - 64;
}
// floats of workspace: conditioner input (5 B: the slot of the second input sits 4 B behind the first), cur0, cur1, the latent pair, the prior's sign sums,
// the head outputs of whole tiles (32 nbk rows; sized for three channels -- the conditioner launches have written the value channel alone since round 4)
int64_t tile_sample_floats(int64_t B, int nbk) { return B * 10 + ((B + 31) / 32) * 32 * (32 * nbk * NCH) + 64; }

namespace {
template <int NBK>
int launch_tile_sample_t(const MfmaDev* mdev, const ModelDev& md, const TsArgs& a_in, int draw, const float* u, int64_t B, float* x, float* latent, float* ws, hipStream_t s) {
    constexpr int NB = 32 * NBK;
    float* cin = ws;                 // [5][B]
    float* cur0 = cin + 5 * B;
    float* cur1 = cur0 + B;
    float* lat = cur1 + B;           // [B] (column 0 between the two prior phases)
    float* s1 = lat + 2 * B;
    float* oj = ws + (((size_t)10 * B + 63) / 64) * 64;
    float* ow = (mdev->p_plain_bc && !env_sample_dense_envelope()) ? oj + (size_t)((B + 31) / 32) * 32 * NB : nullptr;   // (behind the one channel oj holds: sized for three)
    TsArgs a = a_in;
    a.ow = ow;
    a.tabB0 = (ow && !env_sample_full_rows()) ? mdev->tabB0 : nullptr;
    const unsigned lane_blocks = (unsigned)((B + 255) / 256);
    const int lds_bytes = (mdev->const_floats + mdev->net_floats) * (int)sizeof(float);
    static DynLdsSlots cfg_flow{}, cfg_prior{};
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(k_etile_cond<false, NBK, 1>), lds_bytes, &cfg_flow)) return rc;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(k_etile_cond<true, NBK, 1>), lds_bytes, &cfg_prior)) return rc;
    const int64_t n_tiles = (B + 31) / 32;
    const unsigned cond_blocks = (unsigned)std::min<int64_t>((n_tiles + kCondWaves - 1) / kCondWaves, 256 * 4);
    const int L = md.n_layers;
    if (draw) {
        hipLaunchKernelGGL((k_tsample<0, NB>), dim3(lane_blocks), dim3(256), 0, s, a, 0, (const float*)oj, u, B, cur0, cur1, cin, lat, latent, x);
        hipLaunchKernelGGL((k_etile_cond<true, NBK, 1>), dim3(cond_blocks), dim3(kCondWaves * 64), lds_bytes, s, *mdev, L, (const float*)cin, B, oj, s1, ow);
        if (a.ow && a.tabB0 && !env_sample_one_lane())   // (the band form: eight lanes per walker)
            hipLaunchKernelGGL((k_tsample_p1g<NB>), dim3((unsigned)((B * 8 + 255) / 256)), dim3(256), 0, s, a, (const float*)oj, B, cur0, cur1, cin, (const float*)lat, latent);
        else
            hipLaunchKernelGGL((k_tsample<1, NB>), dim3(lane_blocks), dim3(256), 0, s, a, 0, (const float*)oj, u, B, cur0, cur1, cin, lat, latent, x);
    } else {
        hipLaunchKernelGGL((k_tsample<3, NB>), dim3(lane_blocks), dim3(256), 0, s, a, 0, (const float*)oj, u, B, cur0, cur1, cin, lat, latent, x);
    }
    for (int l = L - 1; l >= 0; --l) {
        hipLaunchKernelGGL((k_etile_cond<false, NBK, 1>), dim3(cond_blocks), dim3(kCondWaves * 64), lds_bytes, s, *mdev, l, (const float*)cin, B, oj, s1);
        // (the band form with eight lanes per walker: two row blocks only -- 2^17 draws 0.320 -> 0.290 ms; with one row block the walker's own lane is faster,
        // 0.201 against 0.225: WF_SAMPLE_GROUP_PHASE2 forces it, WF_SAMPLE_ONE_LANE the other form)
        if (a.i_band_int > 0 && !env_sample_one_lane() && (NB > 32 || env_sample_group_phase2()))
            hipLaunchKernelGGL((k_tsample_p2g<NB>), dim3((unsigned)((B * 8 + 255) / 256)), dim3(256), 0, s, a, l, (const float*)oj, B, cur0, cur1, cin, x);
        else
            hipLaunchKernelGGL((k_tsample<2, NB>), dim3(lane_blocks), dim3(256), 0, s, a, l, (const float*)oj, u, B, cur0, cur1, cin, lat, latent, x);
    }
    return check();
}
}  // namespace

// draw == 0: x = inverse(u);  draw == 1: latent ~ prior (reported in `latent` if given), x = inverse(latent)
int launch_tile_sample(const MfmaDev* mdev, const ModelDev& md, const float* tabI0, const float* tabP0, const float* fk_nat, int draw, unsigned long long seed,
                       const float* u, int64_t B, float* x, float* latent, int exact, const unsigned long long* seed_offset_dev, int64_t b0, float* ws, void* stream) {
    if (B == 0) return WF_OK;
    TsArgs a{};
    a.comp = mdev->comp;
    a.tabI0 = tabI0;
    a.tabP0 = tabP0;
    a.gI = fk_nat;
    a.b_to_ob = md.b_to_ob;
    a.n_mesh = mdev->n_mesh;
    a.nbI = md.isp.nb;
    a.nbP = md.psp.nb;
    a.degP = md.psp.degree;
    a.i_band_int = (mdev->i_plain_bc && md.isp.degree <= 7 && !env_sample_full_rows()) ? md.isp.nb - md.isp.degree : 0;
    a.n_layers = md.n_layers;
    a.i_reg = md.i_reg;
    a.tol = md.reverse_tol;
    a.box_L = md.box_L;
    a.seed = seed;
    a.seed_offset_dev = seed_offset_dev;
    a.exact = exact;
    a.b0 = b0;
    return mdev->nbk == 1 ? launch_tile_sample_t<1>(mdev, md, a, draw, u, B, x, latent, ws, (hipStream_t)stream)
                          : launch_tile_sample_t<2>(mdev, md, a, draw, u, B, x, latent, ws, (hipStream_t)stream);
}

}  // namespace wf
