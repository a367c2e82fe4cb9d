// wf_eloc.h -- the fp32 rule of include/waveflow_observe.h for the five per-walker values (E_L, T_lap, T_grad, V_en, V_ee), written once:
// k_observe (wf_kernels_observe.hip) and the DMC kernels (wf_kernels_dmc.hip) call it, so that a walker's local energy has the same bits
// wherever it is formed.  Every operation is rounded on its own (the _rn intrinsics where an expression could fuse; the units are built
// with -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/waveflow_observe.h"
#include "wf_internal.h"

namespace wf {

// v[0 .. 4] from one walker's x, psi, grad and hdiag; -> 1 / (psi + 1e-8f), the factor of the drift grad[d] * inv as well
template <int D>
__device__ __forceinline__ float local_values(const float (&x)[D], float ps, const float (&gr)[D], const float (&hd)[D], const Protons& pr,
                                              float (&v)[WF_OBSERVE_SCALARS]) {
    const float inv = __fdiv_rn(1.0f, __fadd_rn(ps, 1e-8f));
    float lap = 0.0f, tg = 0.0f;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        lap = d == 0 ? hd[d] : __fadd_rn(lap, hd[d]);
        const float t = __fmul_rn(gr[d], inv);
        tg = __fadd_rn(tg, __fmul_rn(t, t));
    }
    // the potential: the two loops of k_vqmc_seeds (wf_kernels_grad.hip), kept as two numbers
    float v_en = 0.0f, v_ee = 0.0f;
    for (int p = 0; p < pr.n; ++p)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float r = pr.pos[p] - x[d];
            v_en -= 1.0f / sqrtf(1.0f + r * r);
        }
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < i; ++j) {
            const float r = x[i] - x[j];
            v_ee += 1.0f / sqrtf(1.0f + r * r);
        }
    const float half_lap = __fmul_rn(-0.5f, lap);
    v[0] = __fmul_rn(__fadd_rn(half_lap, __fmul_rn(__fadd_rn(v_en, v_ee), ps)), inv);
    v[1] = __fmul_rn(half_lap, inv);
    v[2] = __fmul_rn(0.5f, tg);
    v[3] = v_en;
    v[4] = v_ee;
    return inv;
}

}  // namespace wf
