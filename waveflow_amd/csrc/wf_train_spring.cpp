// wf_train_spring.cpp -- one whole SPRING training step on the device (include/waveflow_sr_spring.h): the sequence of wf_train_sr.cpp with the
// momentum term, the clipped right-hand side and the capped step around the same entries.  wf_psi_jac, wf_sr_gram and wf_sr_solve are called as
// they are; the glue is wf_kernels_sr_spring.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/waveflow_sr_spring.h"
#include "wf_model.h"

using namespace wf;

extern "C" {

int64_t wf_vqmc_spring_step_workspace_bytes(const wf_model* m, int64_t batch) {
    if (!m || batch < 1) return WF_ERR_INVALID;
    if (batch > kSrStepMaxBatch || !sr_step_covered(m)) return WF_ERR_UNSUPPORTED;
    return sr_step_layout(m, batch, true).total;
}

int wf_vqmc_spring_step(wf_model* m, const wf_spring_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                        double damping_abs, double damping_rel, double momentum, double norm_cap, double clip, int32_t exact_sampler, float* x_dev,
                        int32_t draw, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    Protons pr{};
    if (!m || !st || batch < 1 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (!st->params_dev || !st->counter_dev || !st->step_size_dev || !st->loss_ring_dev || !st->status_dev || st->ring_len < 1) return WF_ERR_INVALID;
    if (!(damping_abs >= 0.0) || !(damping_rel >= 0.0) || (damping_abs == 0.0 && damping_rel == 0.0)) return WF_ERR_INVALID;
    if (!(momentum >= 0.0) || !(momentum < 1.0) || !(norm_cap >= 0.0) || !(clip >= 0.0) || !st->phi_dev) return WF_ERR_INVALID;
    if (!draw && !x_dev) return WF_ERR_INVALID;
    if (batch > kSrStepMaxBatch || !sr_step_covered(m)) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev) return WF_ERR_INVALID;
    const SrStepLayout l = sr_step_layout(m, batch, true);
    if (workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    const int64_t P = m->n_params;
    char* w = (char*)workspace_dev;
    float* x = (!draw || x_dev) ? x_dev : (float*)(w + l.x);
    float *hpsi = (float*)(w + l.hpsi), *psi = (float*)(w + l.psi), *e_loc = (float*)(w + l.e_loc), *inv = (float*)(w + l.inv);
    double *rhs = (double*)(w + l.rhs), *y = (double*)(w + l.y), *q = (double*)(w + l.q), *t = (double*)(w + l.t);
    double *stats = (double*)(w + l.scalars), *sums = stats + 8;
    float *d = (float*)(w + l.d), *rows = (float*)(w + l.rows);
    int32_t *info = (int32_t*)(w + l.scalars + 128), *flag = info + 1;
    float* eff = (float*)(info + 2);   // scalars: stats [4] doubles at 0, block sums [3] doubles at 64, info at 128, flag at 132, eff at 136
    void *sums_ws = w + l.sums_ws, *sr_ws = w + l.sr, *tape = w + l.tape;
    unsigned long long* counter = (unsigned long long*)st->counter_dev;
    int rc = WF_OK;
    // walkers ~ the sampler of wf_vqmc_train_step at this batch size, stream advanced by the device counter
    if (draw) {
        rc = sample_step_walkers(m, seed, counter, batch, x, exact_sampler, tape, l.tape_bytes, stream);
        if (rc) return rc;
    }
    // H psi and psi: the wave sweep of wf_hamiltonian_fwd with its tails in the workspace; inv and the local energies, which the rows need
    rc = launch_wave_energy(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, x, batch, pr, hpsi, psi, nullptr, (float*)tape, stream);
    if (rc) return rc;
    rc = launch_spring_eloc(hpsi, psi, batch, e_loc, inv, stream);
    if (rc) return rc;
    // rows O = inv d psi / d theta; q = O phi; the clipped, momentum-corrected, centred right-hand side
    rc = wf_psi_jac(m, x, batch, inv, nullptr, rows, tape, l.tape_bytes, stream);
    if (rc) return rc;
    if (momentum != 0.0) {
        rc = wf_sr_matvec(rows, batch, P, P, st->phi_dev, q, stream);
        if (rc) return rc;
    }
    rc = launch_spring_rhs(hpsi, psi, batch, q, momentum, clip, e_loc, inv, rhs, stats, stream);
    if (rc) return rc;
    // d = momentum phi + (2 / batch) O^T H y with (Tbar + lambda I) y = rhs
    rc = wf_sr_gram(rows, batch, P, P, t, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    rc = wf_sr_solve(t, batch, rhs, damping_abs, damping_rel, y, info, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    rc = wf_sr_apply_add(rows, batch, P, P, y, 2.0 / (double)batch, st->phi_dev, momentum, d, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    // |d|^2, the verdict (status, rings: the counter still holds this step's index), the capped step size, the update of theta and phi it allows
    rc = launch_spring_verdict(d, P, info, st->status_dev, flag, st->norm_ring_dev, st->eff_ring_dev, st->ring_len, counter, st->step_size_dev, norm_cap, eff,
                               stream);
    if (rc) return rc;
    rc = launch_spring_update(st->params_dev, st->phi_dev, d, P, eff, flag, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables || step_reads_eval_tables(m, batch));
    if (rc) return rc;
    // batch sums of the unclipped local energies -> loss ring, step counter + 1
    return launch_block_sums(e_loc, batch, sums, sums_ws, block_sums_ws_bytes(batch), stream, st->loss_ring_dev, st->ring_len, counter);
}

}  // extern "C"
