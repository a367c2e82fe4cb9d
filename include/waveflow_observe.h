/*
 * waveflow_observe.h -- observables of a trained psi on the device: per-walker energy parts, their fp64 moments and integer histograms of
 * the one-body density and the pair distance, accumulated over any number of calls without a host round trip.  Part of libwaveflow_hip.so;
 * conventions, error codes and WF_ABI_VERSION are those of waveflow_hip.h.
 *
 * Per walker (fp32, every operation rounded on its own, in this order), with psi, grad[d] = d psi / d x_d and hdiag[d] = d^2 psi / d x_d^2
 * as wf_psi_coord_derivs writes them:
 *     inv    = 1 / (psi + 1e-8f)
 *     lap    = hdiag[0] + hdiag[1] + ...                                   (d ascending)
 *     V_en   = - sum_p sum_d 1 / sqrtf(1 + r * r),  r = proton_p - x_d      (protons outer: the loops of wf_vqmc_seeds)
 *     V_ee   =   sum_i sum_{j < i} 1 / sqrtf(1 + r * r),  r = x_i - x_j
 *     T_lap  = (-0.5f * lap) * inv
 *     T_grad = 0.5f * sum_d (grad[d] * inv)^2                              (d ascending)
 *     E_L    = (-0.5f * lap + (V_en + V_ee) * psi) * inv                   (H psi / (psi + 1e-8))
 * A walker is SKIPPED if any of its coordinates, psi, grad, hdiag or the five values is not finite (the samplers write NaN for a walker that
 * exhausts its rejection loop): it adds 1 to counts[1] and nothing else.  Every other walker adds 1 to counts[0], its five values and their
 * squares (fp64) to sums, and enters the histograms:
 *     density   t = (x_d - lo) * scale,              scale      = (float)n_density_bins / (hi - lo)   (fp32, on the host)
 *     pair      t = fabsf(x_i - x_j) * scale_pair,   scale_pair = (float)n_pair_bins / (hi - lo)      (j < i)
 *     t >= 0 && t < n_bins: bin (int)t (density: row d) + 1; otherwise counts[2] (density) or counts[3] (pair) + 1.
 * (fp32 rounding puts nextafterf(hi, lo) at t == n_bins, outside: that is the rule.)
 *
 * Reproducibility: the fp64 sums of one call are formed in an order that depends on B alone -- lane sums in walker order over a grid-stride
 * loop (256 lanes per block, min(ceil(B / 256), 1024) blocks), a fixed shuffle tree per wave (offsets 32, 16, .. 1), the four waves of a block
 * in order, block partials in block order from 0 -- and are added to sums_dev by one thread.  This is the one order of every fp64 sum behind
 * waveflow_overlap.h, waveflow_dmc.h and waveflow_dmc_observe.h as well; waveflow_amd/csrc/wf_accum.h states it step by step and
 * waveflow_amd/_accum.py (ordered_sum) restates it in numpy.  No floating-point atomics.  Two calls on the halves of a batch into one
 * accumulator leave the bits of two calls into two accumulators whose sums are then added.  Histograms and counters are integers: their
 * order does not matter.
 *
 * The accumulators are caller-owned and caller-zeroed; calls add to them.  None of the entries synchronises with the host.
 */
#ifndef WAVEFLOW_OBSERVE_H
#define WAVEFLOW_OBSERVE_H

#include "waveflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_OBSERVE_SCALARS 5   /* order: E_L, T_lap, T_grad, V_en, V_ee */

typedef struct wf_observe_acc {
    double*   sums_dev;      /* [5][2]: sum v, sum v^2 over counted walkers */
    uint64_t* counts_dev;    /* [4]: walkers counted, walkers skipped, coordinates outside the density range, pairs outside the pair range */
    uint64_t* density_dev;   /* [n_dim][n_density_bins], column d of the walker array -> row d; NULL iff n_density_bins == 0 */
    uint64_t* pair_dev;      /* [n_pair_bins]; NULL iff n_pair_bins == 0 */
    int32_t   n_density_bins;  /* 0 .. 512 */
    int32_t   n_pair_bins;     /* 0 .. 1024 */
    float     lo, hi;        /* density range [lo, hi), pair range [0, hi - lo); finite, lo < hi */
} wf_observe_acc;            /* 4 pointers, then four 4-byte fields: 48 bytes */

/* Bytes of workspace wf_observe_accumulate needs for B walkers (the block partials: [blocks][10 sums + 4 counts], the number of blocks a
 * function of B alone and capped); 0 for B == 0, WF_ERR_INVALID for B < 0, WF_ERR_UNSUPPORTED for B > 2^36 (the limit of one call). */
int64_t wf_observe_workspace_bytes(int64_t B);

/* Model-free.  x_dev[B][n_dim] (n_dim 2 .. 8), psi_dev[B], grad_dev[B][n_dim], hdiag_dev[B][n_dim]; protons_host: n_protons (<= 8) positions on
 * the host.  values_dev[B][5] (optional) receives the five values of every walker, skipped ones included, as computed; acc may be NULL when
 * values_dev is given (no workspace is needed then); both NULL with B > 0: WF_ERR_INVALID.  B == 0: WF_OK, nothing is touched.
 * WF_ERR_INVALID: more than 8 protons, n_dim outside 2 .. 8, a missing pointer (for a non-zero bin count as well), negative bin counts, lo or hi
 * not finite, lo >= hi, a workspace that is too small.  WF_ERR_UNSUPPORTED: more than 512 density bins, more than 1024 pair bins, or more than
 * 2^36 walkers in one call (a workgroup's 32-bit histogram counters hold that many; split a larger batch over several calls). */
int wf_observe_accumulate(const float* x_dev, const float* psi_dev, const float* grad_dev, const float* hdiag_dev, int64_t B, int32_t n_dim,
                          const float* protons_host, int32_t n_protons, const wf_observe_acc* acc, float* values_dev,
                          void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Bytes of workspace wf_vqmc_observe_step needs for `batch` walkers: walkers, psi, grad, hdiag, the block partials and the staged sampler's
 * pass.  By capability at that batch size, independent of transient state.  WF_ERR_INVALID for a NULL model or batch < 1,
 * WF_ERR_UNSUPPORTED for a model or a batch size the step does not cover (below). */
int64_t wf_vqmc_observe_step_workspace_bytes(const wf_model* m, int64_t batch);

/* One measurement step as one sequence of launches on `stream`: no host work, no wait, nothing allocated -- capturable in a hipGraph.
 *   1. walkers      draw != 0: `batch` walkers from the sampler wf_vqmc_train_step uses at that batch size, stream `seed` advanced by
 *                   *counter_dev; they are also written to x_dev[batch][D] when x_dev is given.  draw == 0: read from x_dev (required).
 *   2. derivatives  wf_psi_coord_derivs on those walkers with psi, grad and hdiag.  The entry is CALLED as it is (same path choice, same
 *                   switch points, its bits): it uses the model's scratch, which it may grow at the first call of a batch size -- a capture
 *                   needs one call outside it first (vqmc.capture_step's warm-up).  Outputs live in the step's workspace.
 *   3. accumulate   wf_observe_accumulate on the outputs; values_dev[batch][5] is passed through (acc or values_dev may be NULL, not both).
 *   4. counter      *counter_dev += 1.
 * The model is const: no parameter, image or table changes.  Models: those wf_psi_coord_derivs covers, n_dim 2 .. 8.  Batches: those a
 * training step has a sampler for -- the staged sampler where it applies, the wave sampler up to 131072 walkers.  Anything else:
 * WF_ERR_UNSUPPORTED, from the size query as well.  The model must hold parameters (WF_ERR_INVALID otherwise). */
int wf_vqmc_observe_step(const wf_model* m, const wf_observe_acc* acc, uint64_t* counter_dev, uint64_t seed, int64_t batch,
                         const float* protons_host, int32_t n_protons, int32_t exact_sampler, float* x_dev, int32_t draw,
                         float* values_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_OBSERVE_H */
