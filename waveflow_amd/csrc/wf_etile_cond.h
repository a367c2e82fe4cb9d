// wf_etile_cond.h -- the conditioner of one two-particle net on the matrix cores, in pieces and as the launch-per-net kernel k_etile_cond.
// Shared by the H psi unit (wf_kernels_etile.hip: three channels), the reverse units (wf_etile_bwd.h: cond_out) and the staged sampler
// (wf_kernels_etile_sample.hip: CH = 1): the units instantiate disjoint sets of k_etile_cond, so no kernel is compiled twice.
// Behind wf_etile_common.h, so under its contraction pragma.  Everything sits in an anonymous namespace: each translation unit gets its own copy.
#pragma once
#include "wf_etile_common.h"

namespace wf {
namespace {

constexpr int kCondWaves = 4;   // waves per workgroup, kCondOcc workgroups per CU (unbounded, the three channel chains take 324 registers: one wave per SIMD)
constexpr int kCondOcc = 2;     // workgroups per CU the register budget is sized for: 256 registers, two waves per SIMD (the per-lane store addresses spill: 23 reloads per tile)
// r(x) = 1 / (2^x + 1), the activation of the MFMA images, on a value alone (the reverse helpers of wf_etile_bwd.h, the heads of the staged sampler)
__device__ __forceinline__ float r_of(float x) { return __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(x) + 1.0f); }

// The conditioner of one net for one tile, in pieces (NBK = 32-row blocks per dimension: 1 for <= 32 bases, 2 for <= 64).
//   cond_hidden   the two hidden layers: B fragments (split fp16, derivative channels scaled by 2^-e) of the second hidden layer's activations
//   cond_out      one 32-row output block of dimension 1: Taylor triples (f, f', f'') in u_0 of the head's pre-activations, accumulator layout
//   prior_c       the prior head's c = (o * keep) @ ob_to_b as triples, one 32-row block of c at a time, + the sum of the raw outputs (sign)
template <int NBK, int CH = NCH>
__device__ __forceinline__ void cond_hidden(const float* net, float u0v, float u1v, int lane, Frag (&f)[CH][2], int (&e)[CH]) {
    using O = NetOff<2, NBK>;
    const int h = lane >> 5;
    // the conditioner's inputs: (u_0, u_1) values; the Taylor seed in u_0 is (u_0, 1, 0) (u_1 reaches no hidden unit: masked weights)
    const float in0[2] = {u0v, 1.0f}, in1[2] = {u1v, 0.0f};
    // ---- layer 1 (f32 MFMA, K = 2: the two coordinates), both 32-unit blocks; the second-derivative channel starts at zero
    f32x16 a0[CH], a1[CH];
    init_acc<CH>(a0, net + O::b0 + (0 * 2 + h) * 16);
    init_acc<CH>(a1, net + O::b0 + (1 * 2 + h) * 16);
    {
        const float w0 = net[O::W0 + 0 * 64 + lane], w1 = net[O::W0 + 1 * 64 + lane];
#pragma unroll
        for (int c = 0; c < (CH < 2 ? CH : 2); ++c) {
            a0[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0, h ? in1[c] : in0[c], a0[c], 0, 0, 0);
            a1[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1, h ? in1[c] : in0[c], a1[c], 0, 0, 0);
        }
    }
    act_block<CH>(a0);
    act_block<CH>(a1);
    to_frags<CH>(a0, a1, f, e);
    // ---- layer 2
    const _Float16* W1h = reinterpret_cast<const _Float16*>(net + O::W1h);
    const _Float16* W1l = reinterpret_cast<const _Float16*>(net + O::W1l);
    init_acc<CH>(a0, net + O::b1 + (0 + h) * 16);
    init_acc<CH>(a1, net + O::b1 + (2 + h) * 16);
    dense64_block<CH>(W1h, W1l, f, a0, lane);
    dense64_block<CH>(W1h + 2048, W1l + 2048, f, a1, lane);
    unscale<CH>(a0, e);
    unscale<CH>(a1, e);
    act_block<CH>(a0);
    act_block<CH>(a1);
    to_frags<CH>(a0, a1, f, e);
}
// output block kb of dimension 1 (dimension 0 is table-driven: k_prepare_dim0)
template <int NBK, int CH = NCH>
__device__ __forceinline__ void cond_out(const float* net, const Frag (&f)[CH][2], const int (&e)[CH], int kb, int lane, f32x16 (&a0)[CH]) {
    using O = NetOff<2, NBK>;
    const int h = lane >> 5;
    const _Float16* W2h = reinterpret_cast<const _Float16*>(net + O::W2h);
    const _Float16* W2l = reinterpret_cast<const _Float16*>(net + O::W2l);
    init_acc<CH>(a0, net + O::b2 + ((1 * NBK + kb) * 2 + h) * 16);
    dense64_block<CH>(W2h + kb * 2048, W2l + kb * 2048, f, a0, lane);
    unscale<CH>(a0, e);
}
// the whole conditioner (the launch-per-net path): head triples (PRIOR: of c) in a0, the sum of the raw outputs in s1
// cbP: the constant term of the B prior's boundary map times ob_to_b ([NBK][2][16], accumulator layout) or null; it is added to the VALUE channel only --
// the staged sampler, which reads nothing else, is the one caller with such models (the launch-per-net energy path leaves them to k_efused)
template <bool PRIOR, int NBK = 1, int CH = NCH>
__device__ __forceinline__ void cond_net(const float* net, const float* fkP, const _Float16* obh, float u0v, float u1v, int lane, f32x16 (&a0)[NBK][CH], float& s1,
                                         const float* cbP = nullptr, f32x16* wkeep = nullptr /* PRIOR: [NBK] the value channel of o * keep, or null */) {
    Frag f[CH][2];
    int e[CH];
    cond_hidden<NBK, CH>(net, u0v, u1v, lane, f, e);
    if (!PRIOR) {
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb) cond_out<NBK, CH>(net, f, e, kb, lane, a0[kb]);
    } else {
        f32x16 o[NBK][CH];
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb) cond_out<NBK, CH>(net, f, e, kb, lane, o[kb]);
        Frag of[NBK][CH];
        int eo[CH];
        prior_frags<NBK, CH>(o, fkP, lane, of, eo, s1);
        if (wkeep) {
#pragma unroll
            for (int kb = 0; kb < NBK; ++kb) wkeep[kb] = o[kb][0];
        }
#pragma unroll
        for (int kb = 0; kb < NBK; ++kb) {
            prior_c_block<NBK, CH>(obh, of, eo, kb, lane, a0[kb]);
            if (cbP) {
                const f32x16 cb = load16(cbP + (kb * 2 + (lane >> 5)) * 16);
#pragma unroll
                for (int r = 0; r < 16; ++r) a0[kb][0][r] = __builtin_fmaf(s1, cb[r], a0[kb][0][r]);
            }
        }
    }
}

// NBK row blocks per dimension: the head outputs go out as oj[tile][row 0 .. 32 NBK)[channel][32 walkers] (NBK = 2: the staged sampler of 33 .. 64 bases).
// CH = 1 (the staged sampler: round 4): the value channel alone -- a third of the matrix products, no derivative algebra in the activations, 128 instead of
// 384 B per walker and row block out (oj[tile][row][32 walkers])
template <bool PRIOR, int NBK = 1, int CH = NCH>
__global__ __launch_bounds__(kCondWaves * 64, kCondOcc) void k_etile_cond(const MfmaDev mm, int net_index, const float* __restrict__ st, int64_t B,
                                                                float* __restrict__ oj, float* __restrict__ s1buf, float* __restrict__ ow = nullptr) {
    // ow (PRIOR, CH = 1; may be null): the value channel of o * keep, [tile][row][32 walkers] -- where the boundary map only zeroes coefficients these ARE the
    // plain B-spline coefficients of c (c = (o keep) @ ob_to_b, and ob_to_b @ b_to_ob = 1): the staged sampler's envelope reads them instead of forming c @ b_to_ob
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ int next_tile;
    constexpr int kThreads = kCondWaves * 64;
    if (threadIdx.x == 0) next_tile = 0;
    stage_floats<kThreads>(mm.image + mm.const_img_off, lds, mm.const_floats);
    stage_floats<kThreads>(mm.image + (size_t)net_index * mm.net_floats, lds + mm.const_floats, mm.net_floats);
    __syncthreads();
    const float* net = lds + mm.const_floats;
    const float* fkP = lds + 32 * NBK;
    const _Float16* obh = reinterpret_cast<const _Float16*>(lds + 64 * NBK);
    const int lane = threadIdx.x & 63;
    const int j = lane & 31, h = lane >> 5;
    const int64_t n_tiles = (B + 31) >> 5;
    // this workgroup's tiles: blockIdx.x, blockIdx.x + gridDim.x, ... handed to its waves through a counter (oldest-wave-first arbitration)
    const int64_t my_tiles = n_tiles > (int64_t)blockIdx.x ? (n_tiles - blockIdx.x + gridDim.x - 1) / gridDim.x : 0;
    for (;;) {
        int q = 0;
        if (lane == 0) q = __hip_atomic_fetch_add(&next_tile, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        q = __builtin_amdgcn_readfirstlane(q);
        if (q >= my_tiles) break;
        const int64_t tile = (int64_t)blockIdx.x + (int64_t)q * gridDim.x;
        const int64_t w = tile * 32 + j;
        const bool valid = w < B;
        const int64_t wl = valid ? w : B - 1;
        const float u0v = st[wl], u1v = st[(int64_t)4 * B + wl];
        f32x16 a0[NBK][CH], wk[NBK];
        float s1 = 0.0f;
        cond_net<PRIOR, NBK, CH>(net, fkP, obh, u0v, u1v, lane, a0, s1, (PRIOR && mm.p_bias) ? lds + 64 * NBK + NBK * NBK * 1024 + 64 * NBK : nullptr,
                                 (PRIOR && CH == 1 && ow) ? wk : nullptr);
        if (PRIOR && valid && h == 0) s1buf[w] = s1;
        if (PRIOR && CH == 1 && ow && valid) {
#pragma unroll
            for (int kb = 0; kb < NBK; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) ow[(tile * (32 * NBK) + 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * h) * 32 + j] = wk[kb][r];
        }
        // ---- store: oj[tile][row][c][32 walkers] (one contiguous block per tile), row = accumulator row of register r in lane half h of block kb
        if (valid) {
#pragma unroll
            for (int kb = 0; kb < NBK; ++kb)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = 32 * kb + (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
                    for (int c = 0; c < CH; ++c) oj[(tile * (32 * NBK * CH) + row * CH + c) * 32 + j] = a0[kb][c][r];
                }
        }
    }
}

// (host) the status of the launches just issued, for the launch functions of the two-particle units
int check() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error((int)e);
        return WF_ERR_HIP;
    }
    return WF_OK;
}

}  // namespace
}  // namespace wf
