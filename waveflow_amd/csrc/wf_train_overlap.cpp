// wf_train_overlap.cpp -- one overlap measurement step on the device (include/waveflow_overlap.h): the walkers of a training step of m, wf_psi_fwd
// of m and of every reference on them, the accumulation of wf_kernels_overlap.hip, the counter.  The psi entry is called as it is -- its results
// inside the step are its own bit for bit, and it uses each model's scratch (a capture needs one call outside it first).  No model changes.
#include <hip/hip_runtime.h>

#include "wf_model.h"
#include "wf_overlap.h"

using namespace wf;

namespace {

struct OverlapStepLayout {
    int64_t x, psi, ref, partials, sampler;   // offsets
    int64_t sampler_bytes, total;
};

// (capability, not the current state, as wf_vqmc_observe_step_workspace_bytes)
OverlapStepLayout overlap_step_layout(const wf_model* m, int64_t batch, int K) {
    OverlapStepLayout l{};
    Bump b;
    l.x = b.take(batch * m->desc.n_dim * 4);
    l.psi = b.take(batch * 4);
    l.ref = b.take((int64_t)K * batch * 4);
    l.partials = b.take(overlap_ws_bytes(batch, K));
    l.sampler_bytes = align256(step_sampler_bytes(m, batch));
    l.sampler = b.take(l.sampler_bytes);
    l.total = b.at;
    return l;
}

// the models the measurement steps draw walkers for (wf_train_observe.cpp: those of the energy sweeps, whose tables the samplers read)
bool overlap_model_covered(const wf_model* m) { return check_energy_model(m) == WF_OK; }

}  // namespace

extern "C" {

int64_t wf_vqmc_overlap_step_workspace_bytes(const wf_model* m, int64_t batch, int32_t K) {
    if (!m || batch < 1 || K < 1) return WF_ERR_INVALID;
    if (K > WF_OVERLAP_MAX_REFS) return WF_ERR_UNSUPPORTED;
    if (!overlap_model_covered(m) || !measure_batch_covered(m, batch, false)) return WF_ERR_UNSUPPORTED;
    return overlap_step_layout(m, batch, K).total;
}

int wf_vqmc_overlap_step(const wf_model* m, const wf_model* const* refs, int32_t K, const wf_overlap_acc* acc, uint64_t* counter_dev,
                         uint64_t seed, int64_t batch, int32_t exact_sampler, float* x_dev, int32_t draw, float* ratios_dev,
                         void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!m || !refs || batch < 1 || K < 1 || !counter_dev) return WF_ERR_INVALID;
    if (K > WF_OVERLAP_MAX_REFS) return WF_ERR_UNSUPPORTED;
    if ((!acc && !ratios_dev) || (!draw && !x_dev)) return WF_ERR_INVALID;
    if (acc) {
        const int rc = overlap_check_acc(acc);
        if (rc) return rc;
    }
    for (int k = 0; k < K; ++k)
        if (!refs[k] || refs[k]->desc.n_dim != m->desc.n_dim || refs[k]->device != m->device || !refs[k]->params_set) return WF_ERR_INVALID;
    if (!overlap_model_covered(m) || !measure_batch_covered(m, batch, true)) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev) return WF_ERR_INVALID;
    const OverlapStepLayout l = overlap_step_layout(m, batch, K);
    if (workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    char* w = (char*)workspace_dev;
    float* x = (!draw || x_dev) ? x_dev : (float*)(w + l.x);
    float *psi = (float*)(w + l.psi), *ref = (float*)(w + l.ref);
    unsigned long long* counter = (unsigned long long*)counter_dev;
    int rc = WF_OK;
    if (draw) {
        rc = sample_step_walkers(m, seed, counter, batch, x, exact_sampler, w + l.sampler, l.sampler_bytes, stream);
        if (rc) return rc;
    }
    rc = wf_psi_fwd(m, x, batch, psi, nullptr, nullptr, stream);
    if (rc) return rc;
    for (int k = 0; k < K; ++k) {
        rc = wf_psi_fwd(refs[k], x, batch, ref + (int64_t)k * batch, nullptr, nullptr, stream);
        if (rc) return rc;
    }
    return launch_overlap(psi, ref, batch, batch, K, acc, ratios_dev, w + l.partials, counter, stream);
}

}  // extern "C"
