// wf_train_sr.cpp -- one whole stochastic-reconfiguration training step on the device (include/waveflow_sr_step.h): the sequence of
// wf_vqmc_train_step with the rows of wf_psi_jac and the three entries of waveflow_sr.h in the place of the contracted gradient and Adam.
// The entries are called as they are -- their results inside the step are theirs bit for bit; the glue between them is wf_kernels_sr_step.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/waveflow_sr_step.h"
#include "wf_model.h"

using namespace wf;

namespace wf {

// the models the step covers: those of wf_psi_jac (second-order gradients) that wf_hamiltonian_fwd accepts, wave sweeps and sampler with them
bool sr_step_covered(const wf_model* m) { return grad_supported(m, true) && check_energy_model(m) == WF_OK; }

// (capability, not the current state, as wf_vqmc_train_step_workspace_bytes)
SrStepLayout sr_step_layout(const wf_model* m, int64_t batch, bool with_q) {
    const int D = m->desc.n_dim;
    const int64_t P = m->n_params;
    SrStepLayout l{};
    Bump b;
    l.x = b.take(batch * D * 4);
    l.hpsi = b.take(batch * 4);
    l.psi = b.take(batch * 4);
    l.e_loc = b.take(batch * 4);
    l.inv = b.take(batch * 4);
    l.rhs = b.take(batch * 8);
    l.y = b.take(batch * 8);
    l.q = b.take(with_q ? batch * 8 : 0);
    l.d = b.take(P * 4);
    l.scalars = b.take(256);   // the step's own scalars: block sums, the solver's info, the verdict's flag (each step says where)
    l.sums_ws = b.take(block_sums_ws_bytes(batch));
    l.rows = b.take(batch * P * 4);
    l.t = b.take(batch * batch * 8);
    l.sr_bytes = align256(wf_sr_workspace_bytes(batch, P));
    l.sr = b.take(l.sr_bytes);
    const int64_t energy = batch * std::max(wave_tail_floats(D, 1), wave_tail_floats(D, 3)) * 4;
    l.tape_bytes = align256(std::max(wf_psi_jac_workspace_bytes(m, batch), std::max(energy, step_sampler_bytes(m, batch))));
    l.tape = b.take(l.tape_bytes);
    l.total = b.at;
    return l;
}

}  // namespace wf

extern "C" {

int64_t wf_vqmc_sr_step_workspace_bytes(const wf_model* m, int64_t batch) {
    if (!m || batch < 1) return WF_ERR_INVALID;
    if (batch > kSrStepMaxBatch || !sr_step_covered(m)) return WF_ERR_UNSUPPORTED;
    return sr_step_layout(m, batch, false).total;
}

int wf_vqmc_sr_step(wf_model* m, const wf_sr_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                    double damping_abs, double damping_rel, int32_t exact_sampler, float* x_dev, int32_t draw, void* workspace_dev,
                    int64_t workspace_bytes, void* stream) {
    Protons pr{};
    if (!m || !st || batch < 1 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (!st->params_dev || !st->counter_dev || !st->step_size_dev || !st->loss_ring_dev || !st->status_dev || st->ring_len < 1) return WF_ERR_INVALID;
    if (!(damping_abs >= 0.0) || !(damping_rel >= 0.0) || (damping_abs == 0.0 && damping_rel == 0.0)) return WF_ERR_INVALID;
    if (!draw && !x_dev) return WF_ERR_INVALID;
    if (batch > kSrStepMaxBatch || !sr_step_covered(m)) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev) return WF_ERR_INVALID;
    const SrStepLayout l = sr_step_layout(m, batch, false);
    if (workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    const int D = m->desc.n_dim;
    const int64_t P = m->n_params;
    char* w = (char*)workspace_dev;
    float* x = (!draw || x_dev) ? x_dev : (float*)(w + l.x);
    float *hpsi = (float*)(w + l.hpsi), *psi = (float*)(w + l.psi), *e_loc = (float*)(w + l.e_loc), *inv = (float*)(w + l.inv);
    double *rhs = (double*)(w + l.rhs), *y = (double*)(w + l.y), *sums = (double*)(w + l.scalars), *t = (double*)(w + l.t);
    float *d = (float*)(w + l.d), *rows = (float*)(w + l.rows);
    int32_t *info = (int32_t*)(w + l.scalars + 64), *flag = info + 1;   // scalars: block sums [3] doubles at 0, info at 64, flag at 68
    void *sums_ws = w + l.sums_ws, *sr_ws = w + l.sr, *tape = w + l.tape;
    unsigned long long* counter = (unsigned long long*)st->counter_dev;
    int rc = WF_OK;
    // walkers ~ the sampler of wf_vqmc_train_step at this batch size, stream advanced by the device counter
    if (draw) {
        rc = sample_step_walkers(m, seed, counter, batch, x, exact_sampler, tape, l.tape_bytes, stream);
        if (rc) return rc;
    }
    // H psi and psi: the wave sweep of wf_hamiltonian_fwd with its tails in the workspace; local energies and the centred right-hand side
    rc = launch_wave_energy(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, x, batch, pr, hpsi, psi, nullptr, (float*)tape, stream);
    if (rc) return rc;
    rc = launch_sr_eloc_rhs(hpsi, psi, batch, e_loc, inv, rhs, stream);
    if (rc) return rc;
    // rows O = inv d psi / d theta, then d = (2 / batch) O^T H y with (Tbar + lambda I) y = rhs
    rc = wf_psi_jac(m, x, batch, inv, nullptr, rows, tape, l.tape_bytes, stream);
    if (rc) return rc;
    rc = wf_sr_gram(rows, batch, P, P, t, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    rc = wf_sr_solve(t, batch, rhs, damping_abs, damping_rel, y, info, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    rc = wf_sr_apply(rows, batch, P, P, y, 2.0 / (double)batch, d, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    // |d|^2, the verdict (status, norm ring: the counter still holds this step's index), the update it allows
    rc = launch_sr_verdict(d, P, info, st->status_dev, flag, st->norm_ring_dev, st->ring_len, counter, stream);
    if (rc) return rc;
    rc = launch_sr_update(st->params_dev, d, P, st->step_size_dev, flag, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables || step_reads_eval_tables(m, batch));
    if (rc) return rc;
    // batch sums of the local energies -> loss ring, step counter + 1
    return launch_block_sums(e_loc, batch, sums, sums_ws, block_sums_ws_bytes(batch), stream, st->loss_ring_dev, st->ring_len, counter);
}

}  // extern "C"
