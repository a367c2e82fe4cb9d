// wf_kernels_spline.hip -- the reference's spline closures as device entry points (wf_spline_*, include/waveflow_hip.h):
// ISpline_fun / MSpline_fun / BSpline_fun (splines/isplines_jax.py:84-207, msplines_jax.py:67-196, bsplines_jax.py:52-203).
//
// Arithmetic: fp32 throughout, in the reference's operation order, no fused multiply-add (-ffp-contract=off, none by hand).
//   lerp (X_cached, isplines_jax.py:45-56): make_lerp / wrap_clamp of wf_scalar_impl.h (jnp gathers: wrap once, then clamp);
//   y = sum_i c_i * X(T[nd], base + i, x), i ascending, the accumulator starting at 0; dy the same over T[nd + 1] (the defjvp rule,
//   isplines_jax.py:60-66); base = 1 under zero_border (I, M).
//   B closures (bsplines_jax.py:127-137): p_j = sum_i c_i * ob_to_b[i][j] (i ascending), p /= sqrtf(sum_j p_j^2) (j ascending), then
//   the sum over the ORTHOGONAL table -- the reference evaluates the converted weights against cached_o_bases_dict (kept as is).
//   The reference leaves the order of its XLA dot products and reductions unspecified: ascending order is this project's convention,
//   here and in the NumPy restatement of the tests.
// Layout: tables [4][n_mesh][NBP] (mesh-major, bases padded with zeros to NBP = 32 or 64), read with float4 gathers; they are at
// most 256 KB per derivative order and stay L2-resident.  Coefficients [N][nc] row-major: apply and reverse stage each wave's
// contiguous block of 64 rows through LDS with 16-byte loads, then every lane reads its own row from LDS (one lane per row reading
// its row from HBM would put 64 rows under one load instruction).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <new>
#include <string>
#include <vector>

#include "wf_scalar_impl.h"

struct wf_spline {
    wf_spline_desc desc;
    int device = 0;
    int nb = 0, nbp = 0, nc = 0, base = 0, n_mesh = 0, n_knots = 0;
    float* tab = nullptr;    // [4][n_mesh][nbp] the evaluated table (orthogonal B-splines for kind B)
    float* edge = nullptr;   // [4][2][nbp] the table enforce_boundary_conditions reads (plain B-splines for kind B) at mesh points 0 and n_mesh - 1
    float* o2b = nullptr;    // [nbp][nbp] ob_to_b (kind B), zero beyond nb
    float* b2o = nullptr;    // [nbp][nbp] b_to_ob (kind B), zero beyond nb
};

namespace wf {
namespace spline {

using scalar::Lerp;
using scalar::make_lerp;
using scalar::Philox;

constexpr int kWaves = 4;
constexpr int kBlock = 64 * kWaves;   // apply / reverse: one wave = 64 consecutive rows
constexpr int kColBlock = 128;        // enforce_bc / remove_bias / sample: thread-private LDS columns of <= 64 floats (32 KB)
constexpr int kMaxIter = 200;         // bisection: ~log2(1/tol) halvings; correct arithmetic never reaches the cap

struct Args {
    const float* tab;
    const float* o2b;
    const float* b2o;
    const float* edge;
    int nb, nc, base, n_mesh, nbp;
};

// rows [r0, r0 + rows) of c[N][nc] -> s (the wave's LDS block); off = r0 * nc is a multiple of 4 (r0 is), so with a 16-byte aligned
// c the block is read with 16-byte loads.  Every load of the block (<= 64 x 64 floats: <= 16 per lane) is issued before the first LDS store,
// so that a wave waits for HBM once, not once per 1 KB.
__device__ __forceinline__ void stage_rows(const float* __restrict__ c, float* s, int64_t off, int nfl, int lane, int vec) {
    if (vec && nfl >= 4) {
        const float4* g4 = reinterpret_cast<const float4*>(c + off);
        float4* s4 = reinterpret_cast<float4*>(s);
        const int n4 = nfl >> 2;
        float4 v[16];   // (every entry loaded -- past the block's end the last float4 again -- so that the array stays in registers)
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = g4[min(lane + 64 * u, max(n4 - 1, 0))];
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (lane + 64 * u < n4) s4[lane + 64 * u] = v[u];
        for (int e = (n4 << 2) + lane; e < nfl; e += 64) s[e] = c[off + e];
        return;
    }
    for (int e = lane; e < nfl; e += 64) s[e] = c[off + e];
}

// sum_j w_j * X(T, j, x), j ascending over all NBP padded bases: w_j is 0 for the bases the coefficients do not reach and the padded table
// rows are 0, so those terms add exact zeros (the accumulator starts at +0 and can never be -0) and leave the bits of the reference's sum
template <int NBP>
__device__ __forceinline__ float dot_lerp(const float* __restrict__ t, const Lerp& L, const float (&w)[NBP]) {
    const float4* rl = reinterpret_cast<const float4*>(t + (size_t)L.il * NBP);
    const float4* rr = reinterpret_cast<const float4*>(t + (size_t)L.ir * NBP);
    float acc = 0.0f;
#pragma unroll
    for (int q = 0; q < NBP / 4; ++q) {
        const float4 a = rl[q], b = rr[q];
        const float yl[4] = {a.x, a.y, a.z, a.w}, yr[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float slope = (yr[e] - yl[e]) * L.n;
            const float y = yl[e] + slope * L.dx;
            acc = acc + w[4 * q + e] * y;
        }
    }
    return acc;
}

// I / M: the coefficient of table basis j is c[j - base] inside [base, base + nc), 0 elsewhere
template <int NBP>
__device__ __forceinline__ void basis_weights(const Args& a, const float* cr, float (&w)[NBP]) {
#pragma unroll
    for (int j = 0; j < NBP; ++j) {
        const int i = j - a.base;
        const float v = cr[min(max(i, 0), a.nc - 1)];
        w[j] = (i >= 0 && i < a.nc) ? v : 0.0f;
    }
}

// B closures: p = c @ ob_to_b, p /= sqrt(sum p^2) (bsplines_jax.py:133-134); c_i = cr[i]
template <int NBP>
__device__ __forceinline__ void ob_weights(const Args& a, const float* cr, float (&p)[NBP]) {
#pragma unroll
    for (int j = 0; j < NBP; ++j) p[j] = 0.0f;
    for (int i = 0; i < a.nb; ++i) {
        const float ci = cr[i];
        const float* __restrict__ m = a.o2b + (size_t)i * NBP;   // wave-uniform row
#pragma unroll
        for (int j = 0; j < NBP; ++j) p[j] = p[j] + ci * m[j];   // (columns beyond nb are 0 in ob_to_b: p_j stays 0 there)
    }
    float ss = 0.0f;
#pragma unroll
    for (int j = 0; j < NBP; ++j) ss = ss + p[j] * p[j];
    const float nrm = sqrtf(ss);
#pragma unroll
    for (int j = 0; j < NBP; ++j) p[j] = p[j] / nrm;
}

// apply_fun_vec (+ apply_fun_vec_grad with GRAD): y[r] = spline(c[r], x[r]) over T[nd], dy[r] over T[nd + 1]
template <int NBP, bool BK, bool GRAD>
__global__ __launch_bounds__(kBlock) void k_spline_apply(Args a, const float* __restrict__ c, int64_t N, const float* __restrict__ x, int nd,
                                                         float* __restrict__ y, float* __restrict__ dy, int vec) {
    extern __shared__ float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * kWaves + wave) * 64;
    float* s = lds + (size_t)wave * 64 * a.nc;
    if (r0 < N) stage_rows(c, s, r0 * a.nc, (int)min<int64_t>(64, N - r0) * a.nc, lane, vec);
    __syncthreads();
    const int64_t r = r0 + lane;
    if (r >= N) return;
    const float* cr = s + lane * a.nc;
    const Lerp L = make_lerp(x[r], a.n_mesh);
    const float* t0 = a.tab + (size_t)nd * a.n_mesh * NBP;
    float w[NBP];
    if constexpr (BK) ob_weights<NBP>(a, cr, w);
    else basis_weights<NBP>(a, cr, w);
    y[r] = dot_lerp<NBP>(t0, L, w);
    if constexpr (GRAD) dy[r] = dot_lerp<NBP>(t0 + (size_t)a.n_mesh * NBP, L, w);
}

// reverse_fun_vec (isplines_jax.py:153-156): helpers.binary_search (utils/helpers.py:150-166) of spline(c[r], .) - yv[r] on [0, 1]
template <int NBP>
__global__ __launch_bounds__(kBlock) void k_spline_reverse(Args a, const float* __restrict__ c, int64_t N, const float* __restrict__ yv, float tol,
                                                           float* __restrict__ xo, int vec) {
    extern __shared__ float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t r0 = ((int64_t)blockIdx.x * kWaves + wave) * 64;
    float* s = lds + (size_t)wave * 64 * a.nc;
    if (r0 < N) stage_rows(c, s, r0 * a.nc, (int)min<int64_t>(64, N - r0) * a.nc, lane, vec);
    __syncthreads();
    const int64_t r = r0 + lane;
    if (r >= N) return;
    float w[NBP];
    basis_weights<NBP>(a, s + lane * a.nc, w);
    const float target = yv[r], h = tol / 2;
    float low = 0.0f, high = 1.0f;
    for (int it = 0; it < kMaxIter; ++it) {
        const float mid = 0.5f * (low + high);
        if (!((low + h < mid) && (mid < high - h))) break;
        const float f = dot_lerp<NBP>(a.tab, make_lerp(mid, a.n_mesh), w) - target;
        if (f > 0) high = mid; else low = mid;
    }
    xo[r] = low;
}

struct BcArgs {
    int n_left, n_right;
    int left_nd[WF_MAX_BC], right_nd[WF_MAX_BC];
    float left_val[WF_MAX_BC], right_val[WF_MAX_BC];
};

#define COL(j) col[(j) * kColBlock + threadIdx.x]

// enforce_boundary_conditions (isplines_jax.py:158-194, msplines_jax.py:156-184, bsplines_jax.py:173-199), one row per lane.  Table rows
// are indexed with nw = len(weights), not shifted by zero_border, as the reference does.  E(nd, side, j): the constraint table at x = 0 / 1.
__global__ __launch_bounds__(kColBlock) void k_spline_bc(Args a, BcArgs bc, int kind, const float* __restrict__ w, int64_t N, int nw,
                                                         float* __restrict__ out) {
    __shared__ float col[64 * kColBlock];
    const int64_t r = (int64_t)blockIdx.x * kColBlock + threadIdx.x;
    if (r >= N) return;
    auto E = [&](int nd, int side, int j) { return a.edge[((size_t)nd * 2 + side) * a.nbp + j]; };
    for (int j = 0; j < nw; ++j) COL(j) = w[r * nw + j];
    for (int p = 0; p < bc.n_left; ++p) {
        const int nd = bc.left_nd[p];
        float sum = 0.0f;
        for (int j = 0; j < nd; ++j) sum = sum + E(nd, 0, j) * COL(j);
        COL(nd) = (bc.left_val[p] - sum) / E(nd, 0, nd);
    }
    for (int p = 0; p < bc.n_right; ++p) {
        const int nd = bc.right_nd[p];
        if (kind == WF_SPLINE_I && nd == 0) {   // {0: 1.0}: the last weight is set to 0 (isplines_jax.py:174-176)
            COL(nw - 1) = 0.0f;
            continue;
        }
        float sum = 0.0f;
        for (int j = 0; j < nd; ++j) sum = sum + E(nd, 1, nw - 1 - j) * COL(nw - 1 - j);
        COL(nw - 1 - nd) = (bc.right_val[p] - sum) / E(nd, 1, nw - 1 - nd);
    }
    float ss = 0.0f;
    if (kind == WF_SPLINE_B) {
        for (int j = 0; j < nw; ++j) ss = ss + COL(j) * COL(j);
        ss = sqrtf(ss);
    } else {
        for (int j = 0; j < nw; ++j) ss = ss + COL(j);
    }
    for (int j = 0; j < nw; ++j) out[r * nw + j] = COL(j) / ss;
}

// remove_bias (isplines_jax.py:196-202, msplines_jax.py:186-192): one multiply and one divide per scale, in the reference's order
__global__ __launch_bounds__(kColBlock) void k_spline_remove_bias(int kind, int k, const float* __restrict__ p, int64_t N, int nw, float* __restrict__ out) {
    __shared__ float col[64 * kColBlock];
    const int64_t r = (int64_t)blockIdx.x * kColBlock + threadIdx.x;
    if (r >= N) return;
    for (int j = 0; j < nw; ++j) COL(j) = p[r * nw + j];
    for (int i = 0; i < k; ++i) {
        const int lo = kind == WF_SPLINE_I ? i + 1 : i;
        const int hi = kind == WF_SPLINE_I ? nw - i - 2 : nw - i - 1;
        COL(lo) = COL(lo) * (float)(i + 1) / (float)k;
        COL(hi) = COL(hi) * (float)(i + 1) / (float)k;
    }
    float ss = 0.0f;
    for (int j = 0; j < nw; ++j) ss = ss + COL(j);
    for (int j = 0; j < nw; ++j) out[r * nw + j] = COL(j) / ss;
}

#undef COL

// sample_fun_vec (msplines_jax.py:129-154, bsplines_jax.py:144-171): rejection sampling, one lane per output slot (row r, slot s) with its
// own Philox4x32-10 stream keyed by (seed, r, s): the draws do not depend on the launch shape.  Proposal x ~ U[0, 1), y ~ U[0, ymax),
// accepted when y < f(x)^2 (B) / y < f(x) (M).  ymax as the reference bounds it (B: max_j ((normalised c @ ob_to_b) @ b_to_ob)_j^2,
// M: max_j c_j * len(knots)), so the density drawn from is proportional to min(f^2, ymax) / min(f, ymax).  At most max_prop proposals:
// a slot that exhausts them is written as NaN.
template <int NBP, bool BK>
__global__ __launch_bounds__(kColBlock) void k_spline_sample(Args a, unsigned long long seed, const float* __restrict__ c, int64_t N, int ns,
                                                             int max_prop, float n_knots, float* __restrict__ xo) {
    const int64_t slot = (int64_t)blockIdx.x * kColBlock + threadIdx.x;
    if (slot >= N * ns) return;
    const int64_t r = slot / ns;
    const int64_t sl = slot - r * ns;
    Philox rng(seed, ((unsigned long long)r << 32) | (unsigned long long)(unsigned)sl);
    const float* cr = c + r * a.nc;
    float wv[NBP];
    float ymax;
    if constexpr (BK) {
        ob_weights<NBP>(a, cr, wv);
        ymax = 0.0f;
        bool first = true;
        for (int j = 0; j < a.nb; ++j) {
            float q = 0.0f;
#pragma unroll
            for (int i = 0; i < NBP; ++i) q = q + wv[i] * a.b2o[(size_t)i * NBP + j];   // (rows beyond nb: 0 * 0)
            const float q2 = q * q;
            if (first || q2 > ymax || q2 != q2) ymax = q2;   // (jnp max: NaN propagates)
            first = false;
        }
    } else {
        basis_weights<NBP>(a, cr, wv);
        float cmax = cr[0];
        for (int i = 1; i < a.nc; ++i) {
            const float ci = cr[i];
            if (ci > cmax || ci != ci) cmax = ci;
        }
        ymax = cmax * n_knots;
    }
    float out = __builtin_nanf("");
    for (int it = 0; it < max_prop; ++it) {
        const float xv = rng.uniform();
        const float yv = rng.uniform() * ymax;
        const float f = dot_lerp<NBP>(a.tab, make_lerp(xv, a.n_mesh), wv);
        if (yv < (BK ? f * f : f)) {
            out = xv;
            break;
        }
    }
    xo[slot] = out;
}

}  // namespace spline
}  // namespace wf

// ------------------------------------------------------------------------------------------------------------ host side, C ABI
namespace {

using namespace wf;

#define WF_SP_HIP(call)                 \
    do {                                \
        hipError_t e_ = (call);         \
        if (e_ != hipSuccess) {         \
            wf::set_hip_error((int)e_); \
            return WF_ERR_HIP;          \
        }                               \
    } while (0)

struct SpDeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit SpDeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~SpDeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

bool bc_ok(const wf_bc& b) {
    if (b.n < 0 || b.n > WF_MAX_BC) return false;
    for (int p = 0; p < b.n; ++p)
        if (b.n_derivative[p] < 0 || b.n_derivative[p] > 3) return false;
    return true;
}

int upload(const std::vector<float>& h, float** out) {
    void* d = nullptr;
    WF_SP_HIP(hipMalloc(&d, h.size() * sizeof(float)));
    *out = (float*)d;
    WF_SP_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return WF_OK;
}

spline::Args args_of(const wf_spline* sp) {
    return spline::Args{sp->tab, sp->o2b, sp->b2o, sp->edge, sp->nb, sp->nc, sp->base, sp->n_mesh, sp->nbp};
}

int launch_status() {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error((int)e);
        return WF_ERR_HIP;
    }
    return WF_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" {

int wf_spline_create(const wf_spline_desc* desc, const double* tables_host, const double* aux_host, int device, wf_spline** out) {
    if (!desc || !out) return WF_ERR_INVALID;
    *out = nullptr;
    const wf_spline_desc& d = *desc;
    if (d.kind != WF_SPLINE_I && d.kind != WF_SPLINE_M && d.kind != WF_SPLINE_B) return WF_ERR_INVALID;
    if (d.degree < 1 || d.n_internal_knots < 2 || d.n_mesh < 2) return WF_ERR_INVALID;
    if (d.zero_border != 0 && (d.zero_border != 1 || d.kind == WF_SPLINE_B)) return WF_ERR_INVALID;
    if (!bc_ok(d.left) || !bc_ok(d.right)) return WF_ERR_INVALID;
    if (d.kind == WF_SPLINE_I)   // any right value for n_derivative 0 other than 1 makes the reference exit (isplines_jax.py:174-179)
        for (int p = 0; p < d.right.n; ++p)
            if (d.right.n_derivative[p] == 0 && d.right.value[p] != 1.0f) return WF_ERR_INVALID;
    const int nb = n_bases_of(d.kind, d.degree, d.n_internal_knots);
    if (nb < 1 || (d.zero_border && nb < 3)) return WF_ERR_INVALID;
    if (nb > 64) return WF_ERR_UNSUPPORTED;
    if (d.kind == WF_SPLINE_B && tables_host && !aux_host) return WF_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return WF_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return WF_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return WF_ERR_NO_DEVICE;
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return WF_ERR_NO_DEVICE;

    const int nm = d.n_mesh;
    const size_t plane = (size_t)4 * nb * nm;
    std::vector<double> built, plain_b, b2o64, o2b64;
    const double *tab64 = tables_host, *edge64 = tables_host, *b2o = nullptr, *o2b = nullptr;
    try {
        if (!tables_host) {
            built.resize(plane);
            int rc = build_raw_table(d.kind, d.degree, d.n_internal_knots, nm, built.data());
            if (rc < 0) return rc;
            tab64 = edge64 = built.data();
            if (d.kind == WF_SPLINE_B) {
                plain_b.swap(built);
                built.resize(plane);
                b2o64.resize((size_t)nb * nb);
                o2b64.resize((size_t)nb * nb);
                rc = build_ortho_b(d.degree, d.n_internal_knots, nm, plain_b.data(), built.data(), b2o64.data(), o2b64.data());
                if (rc < 0) return rc;
                tab64 = built.data();
                edge64 = plain_b.data();
                b2o = b2o64.data();
                o2b = o2b64.data();
            }
        } else if (d.kind == WF_SPLINE_B) {   // aux: plain [4][nb][n_mesh], b_to_ob [nb][nb], ob_to_b [nb][nb]
            edge64 = aux_host;
            b2o = aux_host + plane;
            o2b = b2o + (size_t)nb * nb;
        }
    } catch (const std::bad_alloc&) {
        return WF_ERR_NOMEM;
    }

    SpDeviceGuard g(device);
    if (!g.ok) return WF_ERR_NO_DEVICE;
    wf_spline* sp = new (std::nothrow) wf_spline();
    if (!sp) return WF_ERR_NOMEM;
    sp->desc = d;
    sp->device = device;
    sp->nb = nb;
    sp->nbp = nb <= 32 ? 32 : 64;
    sp->base = d.zero_border;
    sp->nc = nb - 2 * d.zero_border;
    sp->n_mesh = nm;
    sp->n_knots = (int)make_knots(d.kind, d.degree, d.n_internal_knots).size();
    const int nbp = sp->nbp;
    int rc = WF_OK;
    try {
        // fp64 rounded once to fp32, as jnp.array(np.load(...)) does (isplines_jax.py:122, 131)
        std::vector<float> t((size_t)4 * nm * nbp, 0.0f), e((size_t)4 * 2 * nbp, 0.0f);
        for (int nd = 0; nd < 4; ++nd)
            for (int j = 0; j < nb; ++j) {
                const double* row = tab64 + ((size_t)nd * nb + j) * nm;
                for (int m = 0; m < nm; ++m) t[((size_t)nd * nm + m) * nbp + j] = (float)row[m];
                const double* erow = edge64 + ((size_t)nd * nb + j) * nm;
                e[((size_t)nd * 2 + 0) * nbp + j] = (float)erow[0];
                e[((size_t)nd * 2 + 1) * nbp + j] = (float)erow[nm - 1];
            }
        rc = upload(t, &sp->tab);
        if (rc == WF_OK) rc = upload(e, &sp->edge);
        if (rc == WF_OK && d.kind == WF_SPLINE_B) {
            std::vector<float> mb((size_t)nbp * nbp, 0.0f), mo((size_t)nbp * nbp, 0.0f);
            for (int i = 0; i < nb; ++i)
                for (int j = 0; j < nb; ++j) {
                    mb[(size_t)i * nbp + j] = (float)b2o[(size_t)i * nb + j];
                    mo[(size_t)i * nbp + j] = (float)o2b[(size_t)i * nb + j];
                }
            rc = upload(mb, &sp->b2o);
            if (rc == WF_OK) rc = upload(mo, &sp->o2b);
        }
    } catch (const std::bad_alloc&) {
        rc = WF_ERR_NOMEM;
    }
    if (rc != WF_OK) {
        wf_spline_destroy(sp);
        return rc;
    }
    *out = sp;
    return WF_OK;
}

void wf_spline_destroy(wf_spline* sp) {
    if (!sp) return;
    SpDeviceGuard g(sp->device);
    for (float* p : {sp->tab, sp->edge, sp->o2b, sp->b2o})
        if (p) (void)hipFree(p);
    delete sp;
}

int wf_spline_n_bases(const wf_spline* sp) { return sp ? sp->nb : WF_ERR_INVALID; }

int wf_spline_apply(const wf_spline* sp, const float* c_dev, int64_t N, const float* x_dev, int32_t nd, float* y_dev, float* dy_dev, void* stream) {
    if (!sp || N < 0 || nd < 0 || nd > 3 || (dy_dev && nd > 2)) return WF_ERR_INVALID;
    if (N == 0) return WF_OK;
    if (!c_dev || !x_dev || !y_dev) return WF_ERR_INVALID;
    SpDeviceGuard g(sp->device);
    const spline::Args a = args_of(sp);
    const bool bk = sp->desc.kind == WF_SPLINE_B, grad = dy_dev != nullptr;
    const int vec = aligned16(c_dev);
    const dim3 grid((unsigned)((N + spline::kBlock - 1) / spline::kBlock));
    const size_t lds = (size_t)spline::kBlock * sp->nc * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
#define WF_SP_APPLY(NBP, BK, GR) hipLaunchKernelGGL((spline::k_spline_apply<NBP, BK, GR>), grid, dim3(spline::kBlock), lds, st, a, c_dev, N, x_dev, nd, y_dev, dy_dev, vec)
    if (sp->nbp == 32) {
        if (bk) { if (grad) WF_SP_APPLY(32, true, true); else WF_SP_APPLY(32, true, false); }
        else { if (grad) WF_SP_APPLY(32, false, true); else WF_SP_APPLY(32, false, false); }
    } else {
        if (bk) { if (grad) WF_SP_APPLY(64, true, true); else WF_SP_APPLY(64, true, false); }
        else { if (grad) WF_SP_APPLY(64, false, true); else WF_SP_APPLY(64, false, false); }
    }
#undef WF_SP_APPLY
    return launch_status();
}

int wf_spline_reverse(const wf_spline* sp, const float* c_dev, int64_t N, const float* y_dev, float tol, float* x_dev, void* stream) {
    if (!sp || N < 0) return WF_ERR_INVALID;
    if (sp->desc.kind != WF_SPLINE_I) return WF_ERR_UNSUPPORTED;
    if (N == 0) return WF_OK;
    if (!c_dev || !y_dev || !x_dev) return WF_ERR_INVALID;
    SpDeviceGuard g(sp->device);
    const spline::Args a = args_of(sp);
    const dim3 grid((unsigned)((N + spline::kBlock - 1) / spline::kBlock));
    const size_t lds = (size_t)spline::kBlock * sp->nc * sizeof(float);
    const int vec = aligned16(c_dev);
    if (sp->nbp == 32)
        hipLaunchKernelGGL(spline::k_spline_reverse<32>, grid, dim3(spline::kBlock), lds, (hipStream_t)stream, a, c_dev, N, y_dev, tol, x_dev, vec);
    else
        hipLaunchKernelGGL(spline::k_spline_reverse<64>, grid, dim3(spline::kBlock), lds, (hipStream_t)stream, a, c_dev, N, y_dev, tol, x_dev, vec);
    return launch_status();
}

int wf_spline_enforce_bc(const wf_spline* sp, const float* w_dev, int64_t N, int32_t nw, float* out_dev, void* stream) {
    if (!sp || N < 0 || nw < 1 || nw > sp->nb) return WF_ERR_INVALID;
    const wf_spline_desc& d = sp->desc;
    spline::BcArgs bc{};
    bc.n_left = d.left.n;
    bc.n_right = d.right.n;
    for (int p = 0; p < d.left.n; ++p) {
        bc.left_nd[p] = d.left.n_derivative[p];
        bc.left_val[p] = d.left.value[p];
        if (bc.left_nd[p] >= nw) return WF_ERR_INVALID;
    }
    for (int p = 0; p < d.right.n; ++p) {
        bc.right_nd[p] = d.right.n_derivative[p];
        bc.right_val[p] = d.right.value[p];
        if (bc.right_nd[p] >= nw) return WF_ERR_INVALID;
    }
    if (N == 0) return WF_OK;
    if (!w_dev || !out_dev) return WF_ERR_INVALID;
    SpDeviceGuard g(sp->device);
    const dim3 grid((unsigned)((N + spline::kColBlock - 1) / spline::kColBlock));
    hipLaunchKernelGGL(spline::k_spline_bc, grid, dim3(spline::kColBlock), 0, (hipStream_t)stream, args_of(sp), bc, d.kind, w_dev, N, nw, out_dev);
    return launch_status();
}

int wf_spline_remove_bias(const wf_spline* sp, const float* p_dev, int64_t N, int32_t nw, float* out_dev, void* stream) {
    if (!sp || N < 0 || nw < 1 || nw > 64) return WF_ERR_INVALID;
    const int kind = sp->desc.kind, k = sp->desc.degree;
    if (kind == WF_SPLINE_B) return WF_ERR_UNSUPPORTED;
    if (nw < (kind == WF_SPLINE_I ? k + 2 : k)) return WF_ERR_INVALID;   // every index the reference scales lies inside the row
    if (N == 0) return WF_OK;
    if (!p_dev || !out_dev) return WF_ERR_INVALID;
    SpDeviceGuard g(sp->device);
    const dim3 grid((unsigned)((N + spline::kColBlock - 1) / spline::kColBlock));
    hipLaunchKernelGGL(spline::k_spline_remove_bias, grid, dim3(spline::kColBlock), 0, (hipStream_t)stream, kind, k, p_dev, N, nw, out_dev);
    return launch_status();
}

int wf_spline_sample(const wf_spline* sp, uint64_t seed, const float* c_dev, int64_t N, int32_t num_samples, int32_t max_proposals, float* x_dev,
                     void* stream) {
    if (!sp || N < 0 || num_samples < 0 || max_proposals < 1 || N > ((int64_t)1 << 32)) return WF_ERR_INVALID;
    if (sp->desc.kind == WF_SPLINE_I) return WF_ERR_UNSUPPORTED;
    const int64_t total = N * (int64_t)num_samples;
    if (total == 0) return WF_OK;
    if (!c_dev || !x_dev) return WF_ERR_INVALID;
    if ((total + spline::kColBlock - 1) / spline::kColBlock > 0x7FFFFFFF) return WF_ERR_INVALID;
    SpDeviceGuard g(sp->device);
    const spline::Args a = args_of(sp);
    const dim3 grid((unsigned)((total + spline::kColBlock - 1) / spline::kColBlock));
    const float nk = (float)sp->n_knots;
    hipStream_t st = (hipStream_t)stream;
#define WF_SP_SAMPLE(NBP, BK) hipLaunchKernelGGL((spline::k_spline_sample<NBP, BK>), grid, dim3(spline::kColBlock), 0, st, a, (unsigned long long)seed, c_dev, N, num_samples, max_proposals, nk, x_dev)
    const bool bk = sp->desc.kind == WF_SPLINE_B;
    if (sp->nbp == 32) { if (bk) WF_SP_SAMPLE(32, true); else WF_SP_SAMPLE(32, false); }
    else { if (bk) WF_SP_SAMPLE(64, true); else WF_SP_SAMPLE(64, false); }
#undef WF_SP_SAMPLE
    return launch_status();
}

}  // extern "C"
