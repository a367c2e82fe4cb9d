/*
 * waveflow_sr_spring.h -- the SPRING optimiser (Goldshlager, Abrahamsen, Lin 2024) around the B x B solve of waveflow_sr.h: momentum, a cap on the
 * step norm and clipping of the local energies, as two model-free entries and as one whole training step on the device.  Part of
 * libwaveflow_hip.so; conventions, error codes and WF_ABI_VERSION are those of waveflow_hip.h; notation is that of waveflow_sr.h.
 *
 * With phi the previous step's direction (fp32 [P], zeros at the start) and the momentum mu in [0, 1), the direction is the minimiser of
 *     (1 / B) |H O phi' - 2 H e~|^2 + lambda |phi' - mu phi|^2,   i.e.   (S + lambda I) phi' = g + lambda mu phi,
 * which in B x B form is
 *     q = O phi                                   [B], fp64                       wf_sr_matvec
 *     (Tbar + lambda I) y = H (e~ - (mu / 2) q)                                   wf_spring_rhs, wf_sr_gram, wf_sr_solve
 *     d = mu phi + (2 / B) O^T (H y)                                              wf_sr_apply_add
 * and with mu = 0 is the d of waveflow_sr.h.  e~ is e, or with a clip factor k > 0 clamp(e_b, c - k w, c + k w): c the median of the fp32 e_b
 * (even B: the mean of the two middle values in fp64; values that are not finite sort last), w = (1 / B) sum_b |e_b - c| in fp64.
 * Every result is bitwise reproducible: fixed-order fp64 sums, no floating-point atomics.
 */
#ifndef WAVEFLOW_SR_SPRING_H
#define WAVEFLOW_SR_SPRING_H

#include "waveflow_sr_step.h"

#ifdef __cplusplus
extern "C" {
#endif

/* q_dev[b] (fp64, b < B) = sum_{p < P} rows[b][p] v[p]: fp32 operands converted to fp64, every product exact, accumulated in fp64 in one order
 * that depends on P alone.  rows_dev as in wf_sr_gram (read once, 16-byte loads along p where base and ld allow them); v_dev: fp32 [P]. */
int wf_sr_matvec(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const float* v_dev /*fp32 [P]*/, double* q_dev /*fp64 [B]*/, void* stream);

/* out_dev[p] (fp32, p < P) = fl32(mu * prev[p] + scale * sum_b (y[b] - mean y) rows[b][p]): the sum is the fp64 value wf_sr_apply rounds, mu prev is
 * added to it in fp64 and the result rounded once.  prev_dev == NULL or mu == 0: the bits of wf_sr_apply.  0 <= mu < 1.  out_dev may be prev_dev.
 * workspace: that of wf_sr_workspace_bytes(B, P). */
int wf_sr_apply_add(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const double* y_dev, double scale, const float* prev_dev /*fp32 [P] or NULL*/,
                    double mu, float* out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* The right-hand side of the solve from H psi and psi (fp32 [B]), in one workgroup: inv[b] = 1 / (psi[b] + 1e-8), e_loc[b] = hpsi[b] inv[b] (fp32,
 * one rounding per operation: the values wf_vqmc_sr_step computes), r[b] = clamp(e_loc[b], c - clip w, c + clip w) - (mu / 2) q[b] in fp64 and
 * rhs[b] = r[b] - mean(r), the mean summed in a fixed order.  c and w as at the head of this file; clip == 0: no clamp, e~ = e_loc exactly;
 * mu == 0: q_dev is not read and may be NULL.  stats_dev (fp64 [4], may be NULL) = [c, w, c - clip w, c + clip w], zeros when clip == 0.
 * B <= 4096 (beyond: WF_ERR_UNSUPPORTED); 0 <= mu < 1, clip >= 0. */
int wf_spring_rhs(const float* hpsi_dev, const float* psi_dev, int64_t B, const double* q_dev, double mu, double clip, float* e_loc_dev, float* inv_dev,
                  double* rhs_dev, double* stats_dev, void* stream);

typedef struct wf_spring_train_state {
    float* params_dev;         /* the fields of wf_sr_train_state, with their meaning */
    uint64_t* counter_dev;
    float* step_size_dev;
    double* loss_ring_dev;
    double* norm_ring_dev;
    int32_t* status_dev;
    int32_t ring_len;
    int32_t defer_eval_tables;
    float* phi_dev;            /* [n_params]: the previous step's direction d (unscaled); the caller zeroes it once */
    double* eff_ring_dev;      /* [ring_len] = the step size the step applied, 0 for a skipped step; may be NULL */
} wf_spring_train_state;

/* Bytes of workspace wf_vqmc_spring_step needs for `batch` walkers: that of wf_vqmc_sr_step plus q [batch] fp64.  Errors as
 * wf_vqmc_sr_step_workspace_bytes.  What the workspace holds after a step is not part of the interface. */
int64_t wf_vqmc_spring_step_workspace_bytes(const wf_model* m, int64_t batch);

/* One step: the sequence of wf_vqmc_sr_step (see waveflow_sr_step.h) with
 *   4. rhs      q = O phi (momentum > 0), then H (e~ - (momentum / 2) q), e~ the local energies clamped with factor `clip` (0: not clamped);
 *               momentum = 0 and clip = 0: the bits of wf_vqmc_sr_step's right-hand side
 *   5. solve    wf_sr_gram, wf_sr_solve, wf_sr_apply_add(scale 2 / batch, prev = phi, mu = momentum) -> d
 *   7. update   eff64 = lr if norm_cap == 0 or |d|^2 == 0, else min(lr, sqrt(norm_cap / |d|^2)); eff = fl32(eff64);
 *               theta_p <- fl32(theta_p - fl32(eff d_p)), then phi <- d (unscaled).  A step the verdict refuses leaves theta and phi bitwise as
 *               they were and is counted in status[1]; eff_ring holds 0 for it.
 * The loss ring always holds the sums of the unclipped local energies.  With momentum = 0, norm_cap = 0 and clip = 0 parameters, rings, status and
 * counter are bit for bit those of wf_vqmc_sr_step.  Refusals as wf_vqmc_sr_step, and WF_ERR_INVALID for momentum outside [0, 1), norm_cap < 0,
 * clip < 0 or a NULL phi_dev. */
int wf_vqmc_spring_step(wf_model* m, const wf_spring_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                        double damping_abs, double damping_rel, double momentum, double norm_cap, double clip, int32_t exact_sampler, float* x_dev,
                        int32_t draw, void* workspace_dev, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_SR_SPRING_H */
