// wf_train_sr.cpp -- one whole stochastic-reconfiguration training step on the device, plain (include/waveflow_sr_step.h) or SPRING
// (include/waveflow_sr_spring.h): the sequence of wf_vqmc_train_step with the rows of wf_psi_jac and the entries of waveflow_sr.h in the place
// of the contracted gradient and Adam.  One sequence, sr_family_step, with switches: momentum (q = O phi and mu phi in d), the clip of the local
// energies, the cap on the step norm, phi and the ring of applied step sizes; wf_vqmc_sr_step is the call with all of them off.  The entries are
// called as they are -- their results inside the step are theirs bit for bit; the glue between them is wf_kernels_sr_step.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/waveflow_sr_spring.h"
#include "wf_model.h"

using namespace wf;

namespace {

constexpr int64_t kSrStepMaxBatch = 4096;   // the batch limit of wf_sr_solve (and of the one-block right-hand side)

// The workspace: fixed-size vectors, rows, the batch x batch matrix, the workspace of waveflow_sr.h, and one area the sampler (staged form
// only), the energy sweep and the tape of wf_psi_jac use one after the other.  q [batch] fp64 exists only `with_q` (SPRING).
struct SrStepLayout {
    int64_t x, hpsi, psi, e_loc, inv, rhs, y, q, d, scalars, sums_ws, rows, t, sr, tape;   // offsets
    int64_t sr_bytes, tape_bytes, total;
};

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
    l.scalars = b.take(256);   // clip stats [4] doubles at 0, block sums [3] doubles at 64, the solver's info at 128, the verdict's flag at 132, eff at 136
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

int64_t step_workspace_bytes(const wf_model* m, int64_t batch, bool with_q) {
    if (!m || batch < 1) return WF_ERR_INVALID;
    if (batch > kSrStepMaxBatch || !sr_step_covered(m)) return WF_ERR_UNSUPPORTED;
    return sr_step_layout(m, batch, with_q).total;
}

// The step of both entries.  st: the fields the two states share; phi (the previous direction) and eff_ring are null for the plain step, which
// is momentum = norm_cap = clip = 0.  with_q: the caller's workspace has the layout with q (every SPRING step, whatever its momentum).
int sr_family_step(wf_model* m, const wf_sr_train_state* st, float* phi, double* eff_ring, double momentum, double norm_cap, double clip, bool with_q,
                   uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons, double damping_abs, double damping_rel,
                   int32_t exact_sampler, float* x_dev, int32_t draw, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    Protons pr{};
    if (!m || !st || batch < 1 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (!st->params_dev || !st->counter_dev || !st->step_size_dev || !st->loss_ring_dev || !st->status_dev || st->ring_len < 1) return WF_ERR_INVALID;
    if (!(damping_abs >= 0.0) || !(damping_rel >= 0.0) || (damping_abs == 0.0 && damping_rel == 0.0)) return WF_ERR_INVALID;
    if (!draw && !x_dev) return WF_ERR_INVALID;
    if (batch > kSrStepMaxBatch || !sr_step_covered(m)) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev) return WF_ERR_INVALID;
    const SrStepLayout l = sr_step_layout(m, batch, with_q);
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
    float* eff = (float*)(info + 2);
    void *sums_ws = w + l.sums_ws, *sr_ws = w + l.sr, *tape = w + l.tape;
    unsigned long long* counter = (unsigned long long*)st->counter_dev;
    int rc = WF_OK;
    // walkers ~ the sampler of wf_vqmc_train_step at this batch size, stream advanced by the device counter
    if (draw) {
        rc = sample_step_walkers(m, seed, counter, batch, x, exact_sampler, tape, l.tape_bytes, stream);
        if (rc) return rc;
    }
    // H psi and psi: the wave sweep of wf_hamiltonian_fwd with its tails in the workspace
    rc = launch_wave_energy(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, x, batch, pr, hpsi, psi, nullptr, (float*)tape, stream);
    if (rc) return rc;
    // inv and the local energies, which the rows need.  Without momentum the right-hand side needs nothing of the rows: its kernel computes inv
    // and e_loc itself and runs here, in the place of the elementwise one; with momentum it follows q = O phi and writes the same inv and e_loc again.
    rc = momentum != 0.0 ? launch_sr_eloc(hpsi, psi, batch, e_loc, inv, stream)
                         : launch_sr_rhs(hpsi, psi, batch, nullptr, 0.0, clip, e_loc, inv, rhs, stats, stream);
    if (rc) return rc;
    // rows O = inv d psi / d theta
    rc = wf_psi_jac(m, x, batch, inv, nullptr, rows, tape, l.tape_bytes, stream);
    if (rc) return rc;
    if (momentum != 0.0) {
        rc = wf_sr_matvec(rows, batch, P, P, phi, q, stream);
        if (rc) return rc;
        rc = launch_sr_rhs(hpsi, psi, batch, q, momentum, clip, e_loc, inv, rhs, stats, stream);
        if (rc) return rc;
    }
    // d = momentum phi + (2 / batch) O^T H y with (Tbar + lambda I) y = rhs
    rc = wf_sr_gram(rows, batch, P, P, t, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    rc = wf_sr_solve(t, batch, rhs, damping_abs, damping_rel, y, info, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    rc = wf_sr_apply_add(rows, batch, P, P, y, 2.0 / (double)batch, phi, momentum, d, sr_ws, l.sr_bytes, stream);
    if (rc) return rc;
    // |d|^2, the verdict (status, rings: the counter still holds this step's index), the capped step size, the update of theta and phi it allows
    rc = launch_sr_verdict(d, P, info, st->status_dev, flag, st->norm_ring_dev, eff_ring, st->ring_len, counter, st->step_size_dev, norm_cap, eff, stream);
    if (rc) return rc;
    rc = launch_sr_update(st->params_dev, phi, d, P, eff, flag, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables || step_reads_eval_tables(m, batch));
    if (rc) return rc;
    // batch sums of the unclipped local energies -> loss ring, step counter + 1
    return launch_block_sums(e_loc, batch, sums, sums_ws, block_sums_ws_bytes(batch), stream, st->loss_ring_dev, st->ring_len, counter);
}

}  // namespace

extern "C" {

int64_t wf_vqmc_sr_step_workspace_bytes(const wf_model* m, int64_t batch) { return step_workspace_bytes(m, batch, false); }

int64_t wf_vqmc_spring_step_workspace_bytes(const wf_model* m, int64_t batch) { return step_workspace_bytes(m, batch, true); }

int wf_vqmc_sr_step(wf_model* m, const wf_sr_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                    double damping_abs, double damping_rel, int32_t exact_sampler, float* x_dev, int32_t draw, void* workspace_dev,
                    int64_t workspace_bytes, void* stream) {
    return sr_family_step(m, st, nullptr, nullptr, 0.0, 0.0, 0.0, false, seed, batch, protons_host, n_protons, damping_abs, damping_rel, exact_sampler, x_dev,
                          draw, workspace_dev, workspace_bytes, stream);
}

int wf_vqmc_spring_step(wf_model* m, const wf_spring_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                        double damping_abs, double damping_rel, double momentum, double norm_cap, double clip, int32_t exact_sampler, float* x_dev,
                        int32_t draw, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    // (every refusal that can come before these is WF_ERR_INVALID as well)
    if (!st || !(momentum >= 0.0) || !(momentum < 1.0) || !(norm_cap >= 0.0) || !(clip >= 0.0) || !st->phi_dev) return WF_ERR_INVALID;
    const wf_sr_train_state common = {st->params_dev,   st->counter_dev, st->step_size_dev, st->loss_ring_dev,
                                      st->norm_ring_dev, st->status_dev,  st->ring_len,      st->defer_eval_tables};
    return sr_family_step(m, &common, st->phi_dev, st->eff_ring_dev, momentum, norm_cap, clip, true, seed, batch, protons_host, n_protons, damping_abs,
                          damping_rel, exact_sampler, x_dev, draw, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
