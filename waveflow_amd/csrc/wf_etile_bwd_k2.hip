// wf_etile_bwd_k2.hip -- the two-row-block instantiations of the matrix-core reverse kernel (k_ebwd<., 2>, wf_etile_bwd.h) as a translation unit of their own,
// compiled under -mllvm -amdgpu-sched-strategy=max-ilp (waveflow_amd/build.py): 1.532 -> 1.444 ms per loss + gradient of 2^17 walkers of the 33-knot model; the same
// strategy costs the one-row-block form 1 %.
#include "wf_etile_bwd.h"

namespace wf {

template __global__ void k_ebwd<true, 2>(const MfmaDev, int, const float*, const float*, const float*, float*, const float*, const float*, int64_t, float*);
template __global__ void k_ebwd<false, 2>(const MfmaDev, int, const float*, const float*, const float*, float*, const float*, const float*, int64_t, float*);
}  // namespace wf
