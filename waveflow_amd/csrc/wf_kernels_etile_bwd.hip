// wf_kernels_etile_bwd.hip -- parameter gradients of psi and of its Laplacian on the matrix cores (two-particle family): the one-row-block reverse
// kernels k_ebwd<., 1>, the reduction over the workgroups' partial blocks and the scatter to the reference's leaves, and the host side.  The kernels
// and the sweep are described in wf_etile_bwd.h; k_ebwd<., 2> is compiled in wf_etile_bwd_k2.hip.
#include <hip/hip_runtime.h>

#include "wf_etile_bwd.h"

namespace wf {
namespace {

// (one launch for the nets of a chunk: blockIdx.y = net; partial [n_nets][kESplit][gf] of which the first n_part blocks are live, gacc [n_nets][gf];
// gf = g_floats(row blocks of the model))
__global__ void k_egrad_reduce(const float* __restrict__ partial, int n_part, int accumulate, float* __restrict__ gacc, int gf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= gf) return;
    const float* pn = partial + (size_t)blockIdx.y * kESplit * gf;
    float* gn = gacc + (size_t)blockIdx.y * gf;
    float sacc = accumulate ? gn[i] : 0.0f;
    int p = 0;
    for (; p + 8 <= n_part; p += 8) {   // eight loads in flight, added in block order (a runtime trip count alone left one dependent load per ~230 ns: 60 us)
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = pn[(size_t)(p + k) * gf + i];
#pragma unroll
        for (int k = 0; k < 8; ++k) sacc += v[k];
    }
    for (; p < n_part; ++p) sacc += pn[(size_t)p * gf + i];
    gn[i] = sacc;
}
struct ENetOff {
    int W0, b0, W1, b1, W2, b2, NO, n_out;
    float c2;   // scale of the head's pre-activation: -log2(e) under a sigmoid head, 1 otherwise
};
struct ENetOffs {
    ENetOff n[8];
};
__global__ void k_fill_zero(float* __restrict__ p, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = 0.0f;
}
// image units -> the reference's leaves: scales of describe_mfma_image, and the column sums folded into the biases behind a tanh (k_fold_bias)
__global__ void k_egrad_scatter(const float* __restrict__ gacc, int n_nets, const ENetOffs offs, float* __restrict__ flat, int nbk) {
    const int gf = g_floats(nbk), rows = 32 * nbk;
    const int W1 = 128, b1 = 4224, W2 = 4288, b21 = W2 + 64 * rows, b20 = b21 + rows;   // (GL<nbk>)
    const int net = blockIdx.y, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (net >= n_nets || i >= gf) return;
    const ENetOff q = offs.n[net];
    const float* g = gacc + (size_t)net * gf;
    const float c1 = 2.8853900817779268f;
    if (i < 64) flat[q.W0 + i] = c1 * g[i];                                          // W0[0][u]
    else if (i < 128) flat[q.b0 + (i - 64)] = c1 * g[i];
    else if (i < b1) { const int e = i - W1, u = e & 63; flat[q.W1 + e] = -2.0f * c1 * g[i] + c1 * g[b1 + u]; }
    else if (i < W2) flat[q.b1 + (i - b1)] = c1 * g[i];
    else if (i < b21) {
        const int e = i - W2, k = e / rows, jb = e % rows;
        if (jb < q.n_out) flat[q.W2 + k * q.NO + (jb * 2 + 1)] = -2.0f * q.c2 * g[i] + q.c2 * g[b21 + jb];
    } else if (i < b20) { const int jb = i - b21; if (jb < q.n_out) flat[q.b2 + jb * 2 + 1] = q.c2 * g[i]; }
    else { const int jb = i - b20; if (jb < q.n_out) flat[q.b2 + jb * 2 + 0] = q.c2 * g[i]; }
}

}  // namespace

// ---- host side of the matrix-core gradient path
static int64_t ebwd_lds_floats(const MfmaDev* mdev) {
    // the reverse kernel's LDS: constants, one net's forward and transposed images, the transposed ob_to_b, the workgroup's accumulators of (dW1, dW2)
    return (int64_t)mdev->const_floats + mdev->net_floats + mdev->tnet_floats + mdev->nbk * mdev->nbk * 1024 + acc_sets(mdev->nbk) * acc_blocks(mdev->nbk) * 1024;
}
bool energy_vjp_capable(const MfmaDev* mdev) {
    return mdev->timg_off >= 0 && (mdev->nbk == 1 || mdev->nbk == 2) && energy_tile_fused(mdev) && !mdev->i_gate && !mdev->p_gate &&
           ebwd_lds_floats(mdev) * (int64_t)sizeof(float) <= 160 * 1024 - 1024;
}
// floats of workspace per walker of a chunk (whole tiles), + the fixed part
int64_t energy_vjp_floats_per_walker(int n_nets) { return (int64_t)n_nets * 12 + 12 + 4; }   // per-net input jets, adjoint jets, H psi / psi / seeds
int64_t energy_vjp_fixed_floats(int n_nets, int nbk) { return (int64_t)n_nets * kESplit * g_floats(nbk) + 128; }   // the workgroups' gradient blocks
int energy_vjp_gacc_floats(int n_nets, int nbk) { return n_nets * g_floats(nbk); }

template <int NBK>
static int launch_ebwd_t(const MfmaDev* mdev, const float* tabI4, const float* tabP4, const float* st, float* adjb, const float* w_psi, const float* w_lap, int64_t B,
                         float* partial, unsigned blocks, hipStream_t s) {
    const int n_nets = mdev->n_nets;
    const int lds_bytes = (int)(ebwd_lds_floats(mdev) * (int64_t)sizeof(float));
    static DynLdsSlots cfg_p{}, cfg_f{};
    if (int r2 = ensure_dynamic_lds(reinterpret_cast<const void*>(k_ebwd<true, NBK>), lds_bytes, &cfg_p)) return r2;
    if (int r2 = ensure_dynamic_lds(reinterpret_cast<const void*>(k_ebwd<false, NBK>), lds_bytes, &cfg_f)) return r2;
    for (int n = n_nets - 1; n >= 0; --n) {
        const float* st_n = st + (size_t)n * 12 * B;
        float* part_n = partial + (size_t)n * kESplit * GL<NBK>::floats;
        if (n == n_nets - 1)
            hipLaunchKernelGGL((k_ebwd<true, NBK>), dim3(blocks), dim3(kBwdWaves * 64), lds_bytes, s, *mdev, n, tabI4, tabP4, st_n, adjb, w_psi, w_lap, B, part_n);
        else
            hipLaunchKernelGGL((k_ebwd<false, NBK>), dim3(blocks), dim3(kBwdWaves * 64), lds_bytes, s, *mdev, n, tabI4, tabP4, st_n, adjb, w_psi, w_lap, B, part_n);
    }
    return WF_OK;
}

// One chunk of walkers (B a multiple of 32 except for the last chunk of a batch): forward with the per-net input jets, seeds (mode 2: from H psi of
// this very sweep, e_loc is written; mode 1: w_psi / w_lap given), reverse net by net with the weight-gradient products behind each net.
// gacc [n_nets][g_floats(nbk)]: accumulated over the chunks of a batch (accumulate = 0 for the first one).
int launch_energy_vjp(const MfmaDev* mdev, const ModelDev& md, const float* tabI4, const float* tabP4, const float* x, int64_t B, int mode, const float* w_psi,
                      const float* w_lap, const Protons& pr, float running_avg, const float* running_avg_dev, float inv_count, float* e_loc, float* ws,
                      float* gacc, int accumulate, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (B == 0) return WF_OK;
    const int n_nets = mdev->n_nets, gf = g_floats(mdev->nbk);
    const int64_t n_tiles = (B + 31) / 32;
    float* st = ws;                                  // [n_nets][12][B]
    float* adjb = st + (size_t)n_nets * 12 * B;      // [12][B]
    float* hpsi = adjb + 12 * B;
    float* psi = hpsi + B;
    float* wp = psi + B;
    float* wl = wp + B;
    float* partial = ws + (((size_t)(n_nets * 12 + 12 + 4) * B + 63) / 64) * 64;   // [n_nets][kESplit][gf]
    int rc = launch_energy_tile(mdev, md, tabI4, tabP4, nullptr, x, B, pr, hpsi, psi, nullptr, nullptr, stream, st);
    if (rc) return rc;
    if (mode == 2) {
        rc = launch_vqmc_seeds(x, B, 2, pr, hpsi, psi, running_avg, inv_count, e_loc, wp, wl, running_avg_dev, stream);
        if (rc) return rc;
        w_psi = wp;
        w_lap = wl;
    }
    const unsigned blocks = (unsigned)std::min<int64_t>((n_tiles + kBwdWaves - 1) / kBwdWaves, 256);
    rc = mdev->nbk == 1 ? launch_ebwd_t<1>(mdev, tabI4, tabP4, st, adjb, w_psi, w_lap, B, partial, blocks, s)
                        : launch_ebwd_t<2>(mdev, tabI4, tabP4, st, adjb, w_psi, w_lap, B, partial, blocks, s);
    if (rc) return rc;
    hipLaunchKernelGGL(k_egrad_reduce, dim3((gf + 255) / 256, n_nets), dim3(256), 0, s, (const float*)partial, (int)blocks, accumulate, gacc, gf);
    return check();
}

// gacc -> flat gradient in the reference's leaf order (every entry written: zero first, then the live leaves)
int launch_energy_vjp_finish(const float* gacc, int n_nets, int nbk, const int* offs /* [n_nets][8]: W0, b0, W1, b1, W2, b2, NO, n_out */, const float* c2, float* flat,
                             int64_t n_params, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ENetOffs o{};
    for (int n = 0; n < n_nets && n < 8; ++n) {
        const int* q = offs + 8 * n;
        o.n[n] = ENetOff{q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], c2[n]};
    }
    hipLaunchKernelGGL(k_fill_zero, dim3((unsigned)((n_params + 255) / 256)), dim3(256), 0, s, flat, n_params);
    hipLaunchKernelGGL(k_egrad_scatter, dim3((g_floats(nbk) + 255) / 256, n_nets), dim3(256), 0, s, gacc, n_nets, o, flat, nbk);
    return check();
}

}  // namespace wf
