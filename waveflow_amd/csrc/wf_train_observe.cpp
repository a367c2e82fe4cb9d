// wf_train_observe.cpp -- one measurement step on the device (include/waveflow_observe.h): the walkers of a training step, wf_psi_coord_derivs
// on them, the accumulation of wf_kernels_observe.hip, the counter.  The derivative entry is called as it is -- its results inside the step are
// its own bit for bit, and it uses the model's scratch (a capture needs one call outside it first).  Nothing of the model changes.
#include <hip/hip_runtime.h>

#include "wf_model.h"
#include "wf_observe.h"

using namespace wf;

namespace {

struct ObserveStepLayout {
    int64_t x, psi, grad, hdiag, partials, sampler;   // offsets
    int64_t sampler_bytes, total;
};

// (capability, not the current state, as wf_vqmc_train_step_workspace_bytes)
ObserveStepLayout observe_step_layout(const wf_model* m, int64_t batch) {
    const int D = m->desc.n_dim;
    ObserveStepLayout l{};
    Bump b;
    l.x = b.take(batch * D * 4);
    l.psi = b.take(batch * 4);
    l.grad = b.take(batch * D * 4);
    l.hdiag = b.take(batch * D * 4);
    l.partials = b.take(observe_ws_bytes(batch));
    l.sampler_bytes = align256(step_sampler_bytes(m, batch));
    l.sampler = b.take(l.sampler_bytes);
    l.total = b.at;
    return l;
}

// the models of wf_psi_coord_derivs whose walkers wf_observe_accumulate takes
bool observe_model_covered(const wf_model* m) { return check_energy_model(m) == WF_OK && m->desc.n_dim >= 2 && m->desc.n_dim <= 8; }

}  // namespace

bool wf::measure_batch_covered(const wf_model* m, int64_t B, bool current) {
    if (B <= kWaveSampleMax) return true;
    if (B > kObsMaxWalkers) return false;
    if (step_sampler_bytes(m, B) == 0) return false;
    return !current || (!m->eval_tables_stale && !f16_overflow(m));
}

extern "C" {

int64_t wf_vqmc_observe_step_workspace_bytes(const wf_model* m, int64_t batch) {
    if (!m || batch < 1) return WF_ERR_INVALID;
    if (!observe_model_covered(m) || !measure_batch_covered(m, batch, false)) return WF_ERR_UNSUPPORTED;
    return observe_step_layout(m, batch).total;
}

int wf_vqmc_observe_step(const wf_model* m, const wf_observe_acc* acc, uint64_t* counter_dev, uint64_t seed, int64_t batch,
                         const float* protons_host, int32_t n_protons, int32_t exact_sampler, float* x_dev, int32_t draw,
                         float* values_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    Protons pr{};
    if (!m || batch < 1 || !counter_dev || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if ((!acc && !values_dev) || (!draw && !x_dev)) return WF_ERR_INVALID;
    if (acc) {
        const int rc = observe_check_acc(acc);
        if (rc) return rc;
    }
    if (!observe_model_covered(m) || !measure_batch_covered(m, batch, true)) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev) return WF_ERR_INVALID;
    const ObserveStepLayout l = observe_step_layout(m, batch);
    if (workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    char* w = (char*)workspace_dev;
    float* x = (!draw || x_dev) ? x_dev : (float*)(w + l.x);
    float *psi = (float*)(w + l.psi), *grad = (float*)(w + l.grad), *hdiag = (float*)(w + l.hdiag);
    unsigned long long* counter = (unsigned long long*)counter_dev;
    int rc = WF_OK;
    if (draw) {
        rc = sample_step_walkers(m, seed, counter, batch, x, exact_sampler, w + l.sampler, l.sampler_bytes, stream);
        if (rc) return rc;
    }
    rc = wf_psi_coord_derivs(m, x, batch, psi, grad, hdiag, stream);
    if (rc) return rc;
    return launch_observe(x, psi, grad, hdiag, batch, m->desc.n_dim, pr, acc, values_dev, w + l.partials, counter, stream);
}

}  // extern "C"
