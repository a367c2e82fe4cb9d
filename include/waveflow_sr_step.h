/*
 * waveflow_sr_step.h -- one whole stochastic-reconfiguration training step on the device: the counterpart of wf_vqmc_train_step with the
 * natural gradient of waveflow_sr.h in the place of Adam.  Part of libwaveflow_hip.so; conventions, error codes and WF_ABI_VERSION are
 * those of waveflow_hip.h.
 *
 * The step is one sequence of launches on `stream`.  Every per-step scalar (step index, learning rate, solver status) lives on the device,
 * nothing waits for the host and nothing is allocated: the sequence is the same from step to step and can be captured once in a hipGraph
 * and replayed.
 *   1. walkers        draw != 0: `batch` walkers from the sampler wf_vqmc_train_step uses at that batch size, stream `seed` advanced by the
 *                     device counter; they are also written to x_dev[batch][D] when x_dev is given.  draw == 0: the walkers are read from x_dev.
 *   2. energies       H psi and psi (the wave sweep of wf_hamiltonian_fwd), inv = 1 / (psi + 1e-8), e_loc = H psi * inv
 *   3. rows           O[b][k] = inv_b d psi_b / d theta_k (wf_psi_jac with w_psi = inv), [batch][n_params] fp32 in the workspace
 *   4. rhs            e_loc - mean(e_loc) in fp64, the mean summed in a fixed order
 *   5. solve          wf_sr_gram, wf_sr_solve (damping_abs, damping_rel), wf_sr_apply with scale 2 / batch -> d[n_params]
 *   6. |d|^2          fp64, fixed order
 *   7. update         theta_p <- fl32(theta_p - fl32(lr d_p)) (two fp32 roundings, no fused multiply-add), lr read from step_size_dev --
 *                     only if the solver's info is 0 and |d|^2 is finite.  Otherwise the parameters stay bitwise as they are, status[0] =
 *                     info (or -1 when info is 0 and |d|^2 is not finite) and status[1] += 1.  A step that updates sets status[0] = 0.
 *   8. images         the model's weight images from params_dev, under the deferral rule of wf_vqmc_train_step
 *   9. loss ring      [sum E_L, sum E_L^2, batch] -> slot (counter mod ring_len); |d|^2 -> the same slot of norm_ring_dev; counter + 1
 * Steps 2, 3 and 5 run the kernels of the entries named there on the same operands: their results are bit for bit those of the entries.
 * (The step's energies always take the wave sweep, which is what wf_hamiltonian_fwd runs at these batch sizes unless WF_ENERGY_TILE_MIN
 * is lowered to them; the sweep reads no table a deferred refresh leaves stale, so a captured step stays valid in every replay.)
 *
 * batch <= 4096, the limit of wf_sr_solve (beyond: WF_ERR_UNSUPPORTED).  Models: those wf_psi_jac and wf_vqmc_train_step both cover
 * (others: WF_ERR_UNSUPPORTED).  damping_abs, damping_rel >= 0 and not both zero (WF_ERR_INVALID).  The model's weight images must hold
 * params_dev on entry (wf_model_set_params_device) and hold the updated parameters on exit.  Single process.
 */
#ifndef WAVEFLOW_SR_STEP_H
#define WAVEFLOW_SR_STEP_H

#include "waveflow_sr.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct wf_sr_train_state {
    float* params_dev;         /* [n_params], updated in place */
    uint64_t* counter_dev;     /* step index: advances the sampler stream, selects ring slot i mod ring_len, +1 at the end */
    float* step_size_dev;      /* learning rate of THIS step, read on the device (the host may rewrite it between replays) */
    double* loss_ring_dev;     /* [ring_len][3] = [sum E_L, sum E_L^2, batch], as wf_vqmc_train_step */
    double* norm_ring_dev;     /* [ring_len] = |d|^2 of the step (fp64, fixed order); may be NULL */
    int32_t* status_dev;       /* [2]: wf_sr_solve's info of this step; number of skipped steps so far (the caller zeroes it once) */
    int32_t ring_len;
    int32_t defer_eval_tables; /* meaning and large-batch override exactly as in wf_train_state */
} wf_sr_train_state;

/* Bytes of workspace wf_vqmc_sr_step needs for `batch` walkers: walkers, H psi, psi, e_loc, inv, rhs, y, d, the rows (batch * n_params * 4
 * bytes), the batch x batch fp64 matrix, the workspace of waveflow_sr.h, the tape of wf_psi_jac and the block sums.  By capability at that
 * batch size, independent of transient state.  WF_ERR_INVALID for a NULL model or batch < 1, WF_ERR_UNSUPPORTED beyond 4096 walkers or for
 * a model the step does not cover. */
int64_t wf_vqmc_sr_step_workspace_bytes(const wf_model* m, int64_t batch);

/* One step (see the head of this file).  protons_host: as wf_hamiltonian_fwd.  x_dev: required when draw == 0, optional output otherwise. */
int wf_vqmc_sr_step(wf_model* m, const wf_sr_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                    double damping_abs, double damping_rel, int32_t exact_sampler, float* x_dev, int32_t draw, void* workspace_dev,
                    int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_SR_STEP_H */
