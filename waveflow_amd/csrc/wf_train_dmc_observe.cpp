// wf_train_dmc_observe.cpp -- the DMC generation with its forward-walking measurement (include/waveflow_dmc_observe.h): the generation of
// wf_train_dmc.cpp (dmc_step_launch: the same launches, so the same state) with the comb's src kept, then the update of
// wf_kernels_dmc_observe.hip on the combed walkers with the state's own counter as the generation.  The workspace is the step's, then src,
// then the update's.
#include <hip/hip_runtime.h>

#include "wf_dmc_observe.h"
#include "wf_model.h"

using namespace wf;

namespace {

struct DmcFwStepLayout {
    int64_t src, update, total;   // behind the step's own dmc_step_bytes
};

DmcFwStepLayout dmc_fw_step_layout(int64_t step_bytes, int64_t batch, int n_slots) {
    DmcFwStepLayout l{};
    Bump b;
    b.at = align256(step_bytes);
    l.src = b.take(batch * 4);
    l.update = b.take(dmc_fw_layout(batch, n_slots).total);
    l.total = b.at;
    return l;
}

}  // namespace

extern "C" {

int64_t wf_vqmc_dmc_fw_workspace_bytes(const wf_model* m, int64_t batch, int32_t n_slots) {
    const int64_t step_bytes = dmc_step_bytes(m, batch);
    if (step_bytes < 0) return step_bytes;
    if (n_slots < 1 || n_slots > WF_DMC_FW_MAX_SLOTS) return WF_ERR_INVALID;
    return dmc_fw_step_layout(step_bytes, batch, n_slots).total;
}

int wf_vqmc_dmc_fw_step(const wf_model* m, const wf_dmc_state* st, const wf_dmc_fw* fw, uint64_t seed, int64_t batch,
                        const float* protons_host, int32_t n_protons, double tau, int32_t limit_drift, double e_cut, void* workspace_dev,
                        int64_t workspace_bytes, void* stream) {
    Protons pr{};
    int rc = dmc_step_check(m, st, batch, protons_host, n_protons, tau, e_cut, &pr);
    if (rc) return rc;
    rc = dmc_fw_check(fw);
    if (rc) return rc;
    const DmcFwStepLayout l = dmc_fw_step_layout(dmc_step_bytes(m, batch), batch, fw->n_slots);
    if (!workspace_dev || workspace_bytes < l.total) return WF_ERR_INVALID;
    char* w = (char*)workspace_dev;
    int32_t* src = (int32_t*)(w + l.src);
    rc = dmc_step_launch(m, st, seed, batch, pr, tau, limit_drift, e_cut, src, workspace_dev, stream);
    if (rc) return rc;
    DeviceGuard g(m->device);
    return launch_dmc_fw_update(st->x_dev, src, batch, m->desc.n_dim, pr, fw, (const unsigned long long*)st->counter_dev, w + l.update, stream);
}

}  // extern "C"
