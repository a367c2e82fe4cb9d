// wf_sr_common.h -- what wf_kernels_sr.hip, wf_kernels_sr_step.hip and wf_kernels_sr_cg.hip share: the launch check, the block sum, the
// predicated 4-column load of the rows, the test for 16-byte loads and the workspace of the apply.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "wf_internal.h"

namespace wf {

constexpr int kSrSlab = 32;       // rows per block of the apply pass
constexpr int64_t kSrMaxRows = 65536;

inline int64_t sr_align(int64_t v) { return (v + 255) / 256 * 256; }
inline int64_t apply_ws_bytes(int64_t B, int64_t P) { return sr_align(B * 8) + (B + kSrSlab - 1) / kSrSlab * P * 8; }
inline bool sr_vec_ok(const float* rows, int64_t ld) { return ((uintptr_t)rows & 15) == 0 && (ld & 3) == 0; }

// what a launcher returns behind its last launch
inline int sr_finish() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_hip_error((int)e);
        return WF_ERR_HIP;
    }
    return WF_OK;
}

// sum of v over the N threads of the block (red[N]), the same in every thread; one fixed tree
template <int N = 256>
__device__ __forceinline__ double sr_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();
    return out;
}

// rows[r][c .. c + 3], of which the entries with r < B and c + i < c_end exist; the others are zeros and nothing of them is read.
// vec: base and ld allow a 16-byte load at every c that is a multiple of 4.
__device__ __forceinline__ float4 sr_load4(const float* __restrict__ rows, int64_t ld, int64_t r, int64_t B, int64_t c, int64_t c_end, bool vec) {
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (r >= B || c >= c_end) return v;
    const float* p = rows + r * ld + c;
    if (vec && c + 4 <= c_end) return *reinterpret_cast<const float4*>(p);
    v.x = p[0];
    if (c + 1 < c_end) v.y = p[1];
    if (c + 2 < c_end) v.z = p[2];
    if (c + 3 < c_end) v.w = p[3];
    return v;
}

}  // namespace wf
