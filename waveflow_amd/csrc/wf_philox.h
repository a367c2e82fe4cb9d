// wf_philox.h -- Philox4x32-10, the one counter-based generator of every sampler (the one-lane and wave samplers of wf_scalar_impl.h /
// wf_kernels_wave.hip, the rqs and spline samplers, the staged sampler of wf_kernels_etile_sample.hip).  Keyed by a 64-bit seed, one stream per
// 64-bit stream id: the samplers that share a seed and a stream id draw the same numbers.
#pragma once
#include <hip/hip_runtime.h>

namespace wf {

struct Philox {
    unsigned key0, key1, c0, c1, c2, c3;
    unsigned out[4];
    int have;
    __device__ Philox(unsigned long long seed, unsigned long long stream) : key0((unsigned)seed), key1((unsigned)(seed >> 32)), c0(0), c1(0), c2((unsigned)stream), c3((unsigned)(stream >> 32)), have(0) {}
    __device__ void round(unsigned& a0, unsigned& a1, unsigned& a2, unsigned& a3, unsigned k0, unsigned k1) {
        const unsigned long long p0 = 0xD2511F53ull * a0, p1 = 0xCD9E8D57ull * a2;
        const unsigned h0 = (unsigned)(p0 >> 32), l0 = (unsigned)p0, h1 = (unsigned)(p1 >> 32), l1 = (unsigned)p1;
        a0 = h1 ^ a1 ^ k0; a1 = l1; a2 = h0 ^ a3 ^ k1; a3 = l0;
    }
    __device__ void refill() {
        unsigned a0 = c0, a1 = c1, a2 = c2, a3 = c3, k0 = key0, k1 = key1;
#pragma unroll
        for (int r = 0; r < 10; ++r) { round(a0, a1, a2, a3, k0, k1); k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        out[0] = a0; out[1] = a1; out[2] = a2; out[3] = a3;
        if (++c0 == 0) ++c1;
        have = 4;
    }
    __device__ float uniform() {   // [0, 1) with 24 random bits, like jax.random.uniform's fp32 mantissa fill
        if (!have) refill();
        return (float)(out[--have] >> 8) * (1.0f / 16777216.0f);
    }
};

}  // namespace wf
