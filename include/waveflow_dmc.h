/*
 * waveflow_dmc.h -- fixed-node diffusion Monte Carlo with a fixed population, on the device.  Part of libwaveflow_hip.so; conventions, error
 * codes and WF_ABI_VERSION are those of waveflow_hip.h; buffers are caller-owned and no entry waits for the host, as in waveflow_observe.h.
 *
 * A walker is x[n_dim] (fp32).  Its DOMAIN is x strictly ascending with every |x_d| < L (the model's box_size; an argument of the model-free
 * entries): in one dimension the coincidence planes x_i = x_j are the nodes of the antisymmetric ground state, so a walk that never leaves
 * one ordering is a fixed-node walk with the exact nodes.  With a walker go psi, grad[d] = d psi / d x_d (wf_psi_coord_derivs) and its
 * local energy e_loc.  One generation is propose -> derivatives at the proposals -> accept -> reconfigure.
 *
 * Random numbers: wf::Philox (Philox4x32-10, the samplers' generator).  Key = seed (low word, high word).  The 128-bit counter is
 * (c0, c1, c2, c3) = (block, 0, stream low, stream high) with the 64-bit stream id
 *     stream = 2^63 | purpose << 60 | (step mod 2^40) << 20 | b        purpose 0: proposal of slot b, 1: acceptance of slot b,
 *                                                                       2: the comb of this step (b = 0), 3: the comb of an init (step = b = 0)
 * and block = 0, 1, ... counting the 4-word outputs drawn from that stream.  Bit 63 is set, which no sampler's stream id has (they are
 * walker indices below 2^36, or (row << 32 | slot) with row < 2^31), so these numbers never coincide with a sampler's for the same seed.
 * Every number is a function of (seed, step, b) alone: not of B, the grid or other walkers.  A 24-bit uniform is (word >> 8) * 2^-24 in
 * [0, 1), words taken in the order wf::Philox::uniform hands them out (word 3, 2, 1, 0 of a block).
 *
 * PROPOSE (per walker, n_dim 2 .. 8)
 *     inv  = 1 / (psi + 1e-8f),  v_d = grad_d * inv                         (fp32, one rounding each: the drift values of waveflow_observe.h)
 *     limit_drift != 0, in fp64:  a = (sum_d v_d^2) * tau  (d ascending);   f = a == 0 ? 1 : (-1 + sqrt(1 + 2 a)) / a;   vbar_d = v_d * f
 *     limit_drift == 0:           vbar_d = (double)v_d
 *     chi: for the pair (2k, 2k + 1) two uniforms u1, u2 in this order, u1' = 1 - u1 in (0, 1];  r = sqrtf(-2 logf(u1')),
 *          chi_2k = r cosf(2 pi u2), chi_2k+1 = r sinf(2 pi u2)   (Box-Muller; an odd n_dim drops the last sine)
 *     x'_d = fl32(((double)x_d + tau * vbar_d) + sqrt(tau) * (double)chi_d)   (fp64, no contraction, one rounding to fp32 at the end)
 * flag[b] = 1 and x' = x (bit for bit) where x' is outside the domain or not finite, or where x, psi, grad or v of the walker is not finite;
 * flag[b] = 0 otherwise.  So the derivative call that follows sees in-domain, sorted walkers wherever the old walker was one.
 *
 * ACCEPT (per walker).  E_L' by the fp32 rule of waveflow_observe.h from (x', psi', grad', hdiag'): bit for bit what wf_observe_accumulate
 * writes to values[b][0].  In fp64 from the fp32 inputs, vbar(.) as above from (psi, grad) and (psi', grad'):
 *     q_f  = sum_d ((x'_d - x_d) - tau vbar_d(x))^2,   q_r = sum_d ((x_d - x'_d) - tau vbar_d(x'))^2        (d ascending)
 *     logA = 2 log(|psi'| / |psi|) + (q_f - q_r) / (2 tau)
 *     u    = the first uniform of the walker's acceptance stream, in [0, 1)
 * The move is accepted iff flag == 0, psi' psi > 0, every one of x', psi', grad', hdiag', E_L' is finite, and u < A with A = 1 for logA >= 0,
 * exp(logA) below (a NaN logA rejects).  An accepted walker takes x', psi', grad', E_L' -- the state is updated in place.  With e_old the
 * local energy before and e_new the one after the decision:
 *     ebar = (e_new + e_old) / 2;   e_cut > 0: ebar clamped to E_T -+ e_cut / sqrt(tau);   w_b = exp(-tau (ebar - E_T))
 * and w_b = 0 for a walker whose old x, psi, grad or e_loc is not finite.  E_T is *e_trial_dev.
 * The generation record (fp64[6]): sum w, sum w e_new, sum w e_new^2, moves accepted, moves rejected for leaving the domain (flag != 0 or
 * psi' psi <= 0), moves rejected because a new value is not finite (flag == 0, psi' psi > 0 or NaN).  Walkers of weight 0 add nothing to the
 * first three.  The sums are formed in the order that waveflow_observe.h states ("Reproducibility"), which depends on B alone.  No
 * floating-point atomics.
 *
 * RECONFIGURE: the comb, in integers -- exact, and independent of any summation order.
 *     w_max = max_b w_b over finite positive weights
 *     q_b   = t < 2^33 ? (uint64)t : 2^33  with  t = w_b * (4294967296.0 / w_max)   (one fp64 division, one product, one truncation;
 *             the cap only matters for a subnormal w_max);   q_b = 0 for a weight that is not finite or not positive
 *     C     = inclusive prefix sums of q (uint64);   W_int = C[B - 1];   S = W_int / B (integer division; >= 4096 since q >= 2^32 at the maximum)
 *     r     = high half of the 64 x 64 bit product rand64 * S,  rand64 = word 0 << 32 | word 1 of block 0 of the comb's stream
 *     tooth of new slot k = k S + r  (< W_int <= 2^53);   src[k] = the smallest j with C[j] > tooth_k (a bounded binary search), clamped to [0, B)
 * x, psi, grad and e_loc are gathered through the workspace (never in place) and every weight is reset to 1.
 * stats (five 8-byte words): w_max (fp64), then uint64 W_int, S, r, the largest multiplicity of a source slot.
 * Without any finite positive weight src is the identity, stats are 0, 0, 0, 0, 1 and *status_dev += 1.
 *
 * THE STEP.  The comb runs in every step and the global weight is dropped, so E_T cancels out of the walk: it is a common factor of all
 * weights of a generation, and the comb only sees their ratios.  It matters for the range of exp and as the centre of the e_cut window.
 * Estimators per generation: the mixed energy sum w e / sum w and the growth energy E_T - log(sum w / B) / tau.
 */
#ifndef WAVEFLOW_DMC_H
#define WAVEFLOW_DMC_H

#include "waveflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_DMC_RECORD 6               /* sum w, sum w e, sum w e^2, accepted, left the domain, not finite */
#define WF_DMC_RING_RECORD 8          /* the record, then E_growth and the E_T the generation ran with */
#define WF_DMC_STATS 5                /* w_max (fp64), W_int, S, r, largest multiplicity (uint64) */
#define WF_DMC_MAX_WALKERS 1048576    /* 2^20 */

typedef struct wf_dmc_state {
    float*    x_dev;         /* [batch][n_dim] */
    float*    psi_dev;       /* [batch] */
    float*    grad_dev;      /* [batch][n_dim] */
    float*    e_loc_dev;     /* [batch] */
    uint64_t* counter_dev;   /* [1]: generations done */
    double*   e_trial_dev;   /* [1]: E_T */
    double*   ring_dev;      /* [ring_len][8]: generation g is in slot g mod ring_len */
    uint64_t* status_dev;    /* [1]: combs that found no finite positive weight */
    int32_t   ring_len;      /* >= 1 */
    int32_t   reserved;      /* 0 */
} wf_dmc_state;              /* 8 pointers, two 4-byte fields: 72 bytes */

/* Model-free.  x_dev[B][n_dim], psi_dev[B], grad_dev[B][n_dim] -> x_new_dev[B][n_dim], flag_dev[B], chi_dev[B][n_dim] (optional: the chi used).
 * B == 0: WF_OK, nothing is touched.  WF_ERR_INVALID: B < 0, n_dim outside 2 .. 8, a missing pointer, box or tau not finite or not positive.
 * WF_ERR_UNSUPPORTED: B > 2^20. */
int wf_dmc_propose(const float* x_dev, const float* psi_dev, const float* grad_dev, int64_t B, int32_t n_dim, float box, double tau,
                   int32_t limit_drift, uint64_t seed, uint64_t step, float* x_new_dev, int32_t* flag_dev, float* chi_dev, void* stream);

/* Bytes of workspace wf_dmc_accept needs (the block partials of the record); 0 for B == 0, WF_ERR_INVALID for B < 0, WF_ERR_UNSUPPORTED
 * for B > 2^20. */
int64_t wf_dmc_accept_workspace_bytes(int64_t B);

/* Model-free.  The old state x_dev, psi_dev, grad_dev, e_loc_dev (updated in place), the proposal x_new_dev, psi_new_dev, grad_new_dev,
 * hdiag_new_dev, flag_dev; protons_host: n_protons (<= 8) positions on the host.  Outputs: w_dev[B] (fp64), record_dev[6] (fp64, overwritten)
 * and, each optional, logA_dev[B] (fp64), u_dev[B], accepted_dev[B] (1 / 0).  Errors as wf_dmc_propose, and WF_ERR_INVALID for more than 8
 * protons, e_cut negative or not finite, or a workspace that is too small. */
int wf_dmc_accept(float* x_dev, float* psi_dev, float* grad_dev, float* e_loc_dev, const float* x_new_dev, const float* psi_new_dev,
                  const float* grad_new_dev, const float* hdiag_new_dev, const int32_t* flag_dev, int64_t B, int32_t n_dim,
                  const float* protons_host, int32_t n_protons, double tau, int32_t limit_drift, double e_cut, const double* e_trial_dev,
                  uint64_t seed, uint64_t step, double* w_dev, double* record_dev, double* logA_dev, float* u_dev, int32_t* accepted_dev,
                  void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Bytes of workspace wf_dmc_reconfigure needs: block maxima and block sums, the prefix sums, src and one copy of the gathered arrays. */
int64_t wf_dmc_reconfigure_workspace_bytes(int64_t B, int32_t n_dim);

/* Model-free.  The state and w_dev[B] (fp64; all 1 afterwards) -> the combed state.  Optional outputs: src_dev[B] (int32), stats_dev[5]
 * (8-byte words, overwritten), status_dev[1] (incremented where no weight is finite and positive).  Errors as wf_dmc_propose (B > 2^20:
 * WF_ERR_UNSUPPORTED), and WF_ERR_INVALID for a workspace that is too small. */
int wf_dmc_reconfigure(float* x_dev, float* psi_dev, float* grad_dev, float* e_loc_dev, double* w_dev, int64_t B, int32_t n_dim, uint64_t seed,
                       uint64_t step, int32_t* src_dev, uint64_t* stats_dev, uint64_t* status_dev, void* workspace_dev, int64_t workspace_bytes,
                       void* stream);

/* Bytes of workspace wf_vqmc_dmc_init and wf_vqmc_dmc_step need for `batch` walkers (one layout for both): the proposals with psi, grad and
 * hdiag, flags, weights, the record and its block partials, the comb's workspace and the staged sampler's pass.  By capability at that batch
 * size.  WF_ERR_INVALID for a NULL model or batch < 1; WF_ERR_UNSUPPORTED for a model or a batch the step does not cover (below). */
int64_t wf_vqmc_dmc_workspace_bytes(const wf_model* m, int64_t batch);

/* Fills the state, as one sequence of launches on `stream` (no host work, no wait, nothing allocated):
 *   counter = 0, status = 0, the ring zeroed;
 *   walkers   draw != 0: `batch` walkers from |psi|^2 by the sampler wf_vqmc_train_step uses at that batch size, stream `seed`, counter 0;
 *             draw == 0: copied from x_dev[batch][n_dim];
 *   wf_psi_coord_derivs on them; e_loc by the rule above; weights 1, or 0 for a walker of which any value is not finite;
 *   E_T = sum w e_loc / sum w (the record's order);  one reconfigure (purpose 3), which replaces the walkers of weight 0.
 * Models: those of check_energy_model (wf_psi_coord_derivs covers them) with a mean-type box and n_dim 2 .. 8.  Batches: those a training step
 * has a sampler for, at most 2^20.  Anything else: WF_ERR_UNSUPPORTED, from the size query too.  The model must hold parameters. */
int wf_vqmc_dmc_init(const wf_model* m, const wf_dmc_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                     int32_t exact_sampler, const float* x_dev, int32_t draw, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* One generation as one sequence of launches on `stream`: no host work, no wait, nothing allocated -- capturable in a hipGraph.
 *   1. propose      with step = *counter_dev, box = the model's box_size
 *   2. derivatives  wf_psi_coord_derivs on x', CALLED as it is (its own path choice and bits; it may grow the model's scratch at the first call
 *                   of a batch size, so a capture needs one call outside it first)
 *   3. accept       E_T = *e_trial_dev
 *   4. reconfigure
 *   5. ring[(*counter_dev) mod ring_len] = the record, E_growth = E_T - log(sum w / batch) / tau, E_T
 *   6. E_T <- sum w e / sum w, where that is finite
 *   7. *counter_dev += 1
 * The model is const.  Coverage and errors as wf_vqmc_dmc_init; WF_ERR_INVALID also for tau or e_cut out of range and ring_len < 1. */
int wf_vqmc_dmc_step(const wf_model* m, const wf_dmc_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                     double tau, int32_t limit_drift, double e_cut, void* workspace_dev, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_DMC_H */
