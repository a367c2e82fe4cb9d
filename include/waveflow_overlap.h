/*
 * waveflow_overlap.h -- overlaps between wavefunctions on the device: the ratios psi_k / psi of up to 8 reference states on the walkers of psi,
 * their fp64 moments, the overlap-penalised local energies built from them, and a measurement step that draws, evaluates and accumulates
 * without a host round trip.  Part of libwaveflow_hip.so; conventions, error codes and WF_ABI_VERSION are those of waveflow_hip.h.
 *
 * A Waveflow psi is normalised by construction (2 int_{x1 < x2} psi^2 = 1 for the sorted-walker convention of the samplers), so with walkers
 * x ~ |psi|^2 from psi's own exact sampler
 *     S_k = <psi_k | psi> = E[ psi_k(x) / psi(x) ]
 * is a one-sided estimator of variance 1 - S_k^2; no norm estimate enters.
 *
 * Per walker b (fp32, every operation rounded on its own, in this order):
 *     inv  = 1 / (psi[b] + 1e-8f)
 *     r_k  = ref[k][b] * inv                                              (k = 0 .. K - 1)
 * A walker is SKIPPED if psi[b], any ref[k][b] or any r_k is not finite: it adds 1 to counts[1] and nothing else.  Every other walker adds 1
 * to counts[0] and (double)r_k, (double)r_k * (double)r_k to sums[k][0], sums[k][1].  ratios[k][b] (optional) receives r_k of every walker
 * as computed, skipped walkers included.
 *
 * Reproducibility: the fp64 sums of one call are formed in the order that waveflow_observe.h states ("Reproducibility"), which depends on B
 * alone, and are added to sums_dev by one thread.  No floating-point atomics.  Two calls on the halves of a batch into one accumulator leave
 * the bits of two calls into two accumulators whose sums are then added.
 *
 * The penalty method L = E[psi] + sum_k lambda_k S_k^2 has the gradient 2 E[(e~ - mean e~) O] with
 *     e~_b = e_b + sum_k lambda_k a_k (r_kb - a_k),     a_k = sums[k][0] / counts[0]
 * so every optimiser that consumes local energies and rows O takes e~ in the place of e (wf_overlap_penalise).
 *
 * The accumulator is caller-owned and caller-zeroed; calls add to it.  None of the entries synchronises with the host.
 */
#ifndef WAVEFLOW_OVERLAP_H
#define WAVEFLOW_OVERLAP_H

#include "waveflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_OVERLAP_MAX_REFS 8

typedef struct wf_overlap_acc {
    double*   sums_dev;     /* [K][2]: sum r_k, sum r_k^2 over counted walkers */
    uint64_t* counts_dev;   /* [2]: walkers counted, walkers skipped */
} wf_overlap_acc;           /* two pointers: 16 bytes */

/* Bytes of workspace wf_overlap_accumulate needs for B walkers and K references (the block partials: [blocks][2 K sums + 2 counts], the
 * number of blocks a function of B alone and capped at 1024); 0 for B == 0.  WF_ERR_INVALID for B < 0 or K < 1, WF_ERR_UNSUPPORTED for K > 8. */
int64_t wf_overlap_workspace_bytes(int64_t B, int32_t K);

/* Model-free.  psi_dev[B], ref_dev[K][ld] (row k: psi_k on the same walkers; ld >= B floats between rows), 1 <= K <= 8.  ratios_dev[K][ld]
 * (optional, the same ld) receives r_k; acc may be NULL when ratios_dev is given (no workspace is needed then); both NULL: WF_ERR_INVALID.
 * B == 0: WF_OK, nothing is touched.  WF_ERR_INVALID: B < 0, K < 1, ld < B, a missing pointer (of acc as well), a workspace that is too
 * small.  WF_ERR_UNSUPPORTED: K > 8. */
int wf_overlap_accumulate(const float* psi_dev, const float* ref_dev, int64_t ld, int64_t B, int32_t K, const wf_overlap_acc* acc,
                          float* ratios_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Model-free, one launch, no host read: out[b] = (float)(e[b] + sum_k lambda_k a_k (r_kb - a_k)) from ratios_dev[K][ld] as
 * wf_overlap_accumulate wrote them and an accumulator that holds exactly this batch.  In fp64, rounded once at the end:
 *     n = counts[0];  a_k = sums[k][0] / (double)n;  s = (double)e[b];  for k ascending: s = s + ((double)lambda_k * a_k) * ((double)r_kb - a_k)
 * A walker with any r_kb not finite passes e[b] through unchanged; counts[0] == 0 passes every e[b] through.  out_dev may alias e_dev.
 * lambda_host[K]: on the host, finite and >= 0 (read before the call returns).  B == 0: WF_OK.  WF_ERR_INVALID: B < 0, K < 1, ld < B, a
 * missing pointer, a lambda that is negative or not finite.  WF_ERR_UNSUPPORTED: K > 8. */
int wf_overlap_penalise(const float* e_dev, const float* ratios_dev, int64_t ld, int64_t B, int32_t K, const float* lambda_host,
                        const wf_overlap_acc* acc, float* out_dev, void* stream);

/* Bytes of workspace wf_vqmc_overlap_step needs for `batch` walkers and K references: walkers, psi, the K reference rows, the block
 * partials and the staged sampler's pass.  By capability at that batch size, independent of transient state.  WF_ERR_INVALID for a NULL
 * model, batch < 1 or K < 1; WF_ERR_UNSUPPORTED for K > 8 and for a model or a batch size the step does not cover (below). */
int64_t wf_vqmc_overlap_step_workspace_bytes(const wf_model* m, int64_t batch, int32_t K);

/* One measurement step as one sequence of launches on `stream`: no host work, no wait, nothing allocated -- capturable in a hipGraph.
 *   1. walkers      draw != 0: `batch` walkers from the sampler wf_vqmc_train_step uses for m at that batch size, stream `seed` advanced by
 *                   *counter_dev; they are also written to x_dev[batch][D] when x_dev is given.  draw == 0: read from x_dev (required).
 *   2. psi          wf_psi_fwd of m and of refs[0 .. K - 1] on those walkers, in this order.  The entry is CALLED as it is (same path choice,
 *                   same switch points, its bits): it uses each model's scratch, which it may grow at the first call of a batch size -- a
 *                   capture needs one call outside it first (vqmc.capture_step's warm-up).  Outputs live in the step's workspace.
 *   3. accumulate   wf_overlap_accumulate on the outputs (ld = batch); ratios_dev[K][batch] is passed through (acc or ratios_dev may be
 *                   NULL, not both).
 *   4. counter      *counter_dev += 1.
 * Every model is const: no parameter, image or table changes.  refs[k] may be m itself.  m: the models and batches wf_vqmc_observe_step's
 * sampler covers -- the staged sampler where it applies, the wave sampler up to 131072 walkers; anything else: WF_ERR_UNSUPPORTED, from the
 * size query as well.  WF_ERR_INVALID: a NULL model, reference or counter, batch < 1, K < 1, a reference with another n_dim, on another
 * device or without parameters, m without parameters, a workspace that is too small. */
int wf_vqmc_overlap_step(const wf_model* m, const wf_model* const* refs, int32_t K, const wf_overlap_acc* acc, uint64_t* counter_dev,
                         uint64_t seed, int64_t batch, int32_t exact_sampler, float* x_dev, int32_t draw, float* ratios_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_OVERLAP_H */
