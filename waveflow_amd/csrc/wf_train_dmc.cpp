// wf_train_dmc.cpp -- fixed-node DMC with a model (include/waveflow_dmc.h): wf_vqmc_dmc_init fills a state from |psi|^2 (or from given walkers),
// wf_vqmc_dmc_step is one generation -- the model-free launches of wf_kernels_dmc.hip around wf_psi_coord_derivs, which is called as it is (its
// results inside the step are its own bit for bit; it uses the model's scratch, so a capture needs one call outside it first).  The pattern is
// that of wf_train_observe.cpp: one Bump layout for the query and the entries, the staged sampler's pass inside it.  Nothing of the model changes.
#include <hip/hip_runtime.h>

#include <cmath>

#include "wf_dmc.h"
#include "wf_model.h"

using namespace wf;

namespace {

struct DmcStepLayout {
    int64_t x, psi, grad, hdiag, flag, w, partials, record, comb, sampler;   // offsets
    int64_t sampler_bytes, total;
};

// (capability, not the current state, as wf_vqmc_train_step_workspace_bytes)
DmcStepLayout dmc_step_layout(const wf_model* m, int64_t batch) {
    const int D = m->desc.n_dim;
    DmcStepLayout l{};
    Bump b;
    l.x = b.take(batch * D * 4);
    l.psi = b.take(batch * 4);
    l.grad = b.take(batch * D * 4);
    l.hdiag = b.take(batch * D * 4);
    l.flag = b.take(batch * 4);
    l.w = b.take(batch * 8);
    l.partials = b.take(dmc_accept_ws_bytes(batch));
    l.record = b.take(WF_DMC_RECORD * 8);
    l.comb = b.take(dmc_comb_layout(batch, D).total);
    l.sampler_bytes = align256(step_sampler_bytes(m, batch));
    l.sampler = b.take(l.sampler_bytes);
    l.total = b.at;
    return l;
}

// the models of wf_psi_coord_derivs whose walkers live in the domain of the header: sorted, inside the mean-type box
bool dmc_model_covered(const wf_model* m) {
    return check_energy_model(m) == WF_OK && m->desc.box_kind == WF_BOX_MEAN && m->desc.n_dim >= 2 && m->desc.n_dim <= 8 &&
           std::isfinite(m->desc.box_size) && m->desc.box_size > 0.0f;
}
// a sampler for B walkers, as a training step has one (wf_train_observe.cpp), within the comb's limit.  drawing: at call time the staged sampler
// also needs fresh tables, as sample_step_walkers decides.
bool dmc_batch_covered(const wf_model* m, int64_t B, bool drawing) {
    if (B > kDmcMaxWalkers) return false;
    if (B <= kWaveSampleMax) return true;
    if (step_sampler_bytes(m, B) == 0) return false;
    return !drawing || (!m->eval_tables_stale && !f16_overflow(m));
}

bool state_complete(const wf_dmc_state* st) {
    return st && st->x_dev && st->psi_dev && st->grad_dev && st->e_loc_dev && st->counter_dev && st->e_trial_dev && st->ring_dev && st->status_dev &&
           st->ring_len >= 1;
}

}  // namespace

// ---- what wf_vqmc_dmc_step and wf_vqmc_dmc_fw_step (wf_train_dmc_observe.cpp) share (wf_dmc.h)
namespace wf {

int64_t dmc_step_bytes(const wf_model* m, int64_t batch) {
    if (!m || batch < 1) return WF_ERR_INVALID;
    if (!dmc_model_covered(m) || !dmc_batch_covered(m, batch, false)) return WF_ERR_UNSUPPORTED;
    return dmc_step_layout(m, batch).total;
}

int dmc_step_check(const wf_model* m, const wf_dmc_state* st, int64_t batch, const float* protons_host, int n_protons, double tau, double e_cut,
                   Protons* pr) {
    if (!m || batch < 1 || !state_complete(st) || !make_protons(protons_host, n_protons, pr)) return WF_ERR_INVALID;
    if (!std::isfinite(tau) || !(tau > 0.0) || !std::isfinite(e_cut) || e_cut < 0.0) return WF_ERR_INVALID;
    if (!dmc_model_covered(m) || !dmc_batch_covered(m, batch, false)) return WF_ERR_UNSUPPORTED;
    if (!m->params_set) return WF_ERR_INVALID;
    return WF_OK;
}

int dmc_step_launch(const wf_model* m, const wf_dmc_state* st, uint64_t seed, int64_t batch, const Protons& pr, double tau, int limit_drift,
                    double e_cut, int32_t* src_out, void* workspace_dev, void* stream) {
    const DmcStepLayout l = dmc_step_layout(m, batch);
    DeviceGuard g(m->device);
    const int D = m->desc.n_dim;
    char* w = (char*)workspace_dev;
    float *xn = (float*)(w + l.x), *psn = (float*)(w + l.psi), *grn = (float*)(w + l.grad), *hdn = (float*)(w + l.hdiag);
    int32_t* flag = (int32_t*)(w + l.flag);
    double *wt = (double*)(w + l.w), *record = (double*)(w + l.record);
    const DmcParams p{tau, std::sqrt(tau), e_cut, m->desc.box_size, limit_drift != 0, (unsigned long long)seed, 0ull,
                      (const unsigned long long*)st->counter_dev};
    int rc = launch_dmc_propose(st->x_dev, st->psi_dev, st->grad_dev, batch, D, p, xn, flag, nullptr, stream);
    if (rc) return rc;
    rc = wf_psi_coord_derivs(m, xn, batch, psn, grn, hdn, stream);
    if (rc) return rc;
    rc = launch_dmc_accept(st->x_dev, st->psi_dev, st->grad_dev, st->e_loc_dev, xn, psn, grn, hdn, flag, batch, D, pr, p, st->e_trial_dev, wt, record,
                           nullptr, nullptr, nullptr, 0, w + l.partials, stream);
    if (rc) return rc;
    rc = launch_dmc_reconfigure(st->x_dev, st->psi_dev, st->grad_dev, st->e_loc_dev, wt, batch, D, p, 2, src_out, nullptr,
                                (unsigned long long*)st->status_dev, w + l.comb, stream);
    if (rc) return rc;
    return launch_dmc_finish(st, record, batch, tau, stream);
}

}  // namespace wf

extern "C" {

int64_t wf_vqmc_dmc_workspace_bytes(const wf_model* m, int64_t batch) {
    return dmc_step_bytes(m, batch);
}

int wf_vqmc_dmc_init(const wf_model* m, const wf_dmc_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                     int32_t exact_sampler, const float* x_dev, int32_t draw, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    Protons pr{};
    if (!m || batch < 1 || !state_complete(st) || !make_protons(protons_host, n_protons, &pr) || (!draw && !x_dev)) return WF_ERR_INVALID;
    if (!dmc_model_covered(m) || !dmc_batch_covered(m, batch, draw != 0)) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev) return WF_ERR_INVALID;
    const DmcStepLayout l = dmc_step_layout(m, batch);
    if (workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    const int D = m->desc.n_dim;
    char* w = (char*)workspace_dev;
    float* hdiag = (float*)(w + l.hdiag);
    double *wt = (double*)(w + l.w), *record = (double*)(w + l.record);
    int rc = launch_dmc_reset(st, stream);
    if (rc) return rc;
    if (draw) {
        rc = sample_step_walkers(m, seed, (const unsigned long long*)st->counter_dev, batch, st->x_dev, exact_sampler, w + l.sampler, l.sampler_bytes,
                                 stream);
        if (rc) return rc;
    } else {
        WF_HIP(hipMemcpyAsync(st->x_dev, x_dev, (size_t)batch * D * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    }
    rc = wf_psi_coord_derivs(m, st->x_dev, batch, st->psi_dev, st->grad_dev, hdiag, stream);
    if (rc) return rc;
    const DmcParams p{1.0, 1.0, 0.0, m->desc.box_size, 0, (unsigned long long)seed, 0ull, nullptr};
    rc = launch_dmc_accept(st->x_dev, st->psi_dev, st->grad_dev, st->e_loc_dev, nullptr, nullptr, nullptr, hdiag, nullptr, batch, D, pr, p, nullptr, wt,
                           record, nullptr, nullptr, nullptr, 1, w + l.partials, stream);
    if (rc) return rc;
    rc = launch_dmc_trial_from_record(record, st->e_trial_dev, stream);
    if (rc) return rc;
    return launch_dmc_reconfigure(st->x_dev, st->psi_dev, st->grad_dev, st->e_loc_dev, wt, batch, D, p, 3, nullptr, nullptr,
                                  (unsigned long long*)st->status_dev, w + l.comb, stream);
}

int wf_vqmc_dmc_step(const wf_model* m, const wf_dmc_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                     double tau, int32_t limit_drift, double e_cut, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    Protons pr{};
    const int rc = dmc_step_check(m, st, batch, protons_host, n_protons, tau, e_cut, &pr);
    if (rc) return rc;
    if (!workspace_dev || workspace_bytes < dmc_step_layout(m, batch).total) return WF_ERR_INVALID;
    return dmc_step_launch(m, st, seed, batch, pr, tau, limit_drift, e_cut, nullptr, workspace_dev, stream);
}

}  // extern "C"
