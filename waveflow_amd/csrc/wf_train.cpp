// wf_train.cpp -- one whole training step on the device (VQMC, its two distributed halves, maximum likelihood) and the optimiser / reduction
// entry points of the C ABI.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "wf_model.h"

using namespace wf;

extern "C" {

int wf_adam_step(float* params_dev, const float* grad_dev, float* m_dev, float* v_dev, int64_t n, int64_t step, float step_size, float b1,
                 float b2, float eps, void* stream) {
    if (n < 0 || step < 0 || (n > 0 && (!params_dev || !grad_dev || !m_dev || !v_dev))) return WF_ERR_INVALID;
    if (n == 0) return WF_OK;
    return launch_adam(params_dev, grad_dev, m_dev, v_dev, n, step, step_size, b1, b2, eps, nullptr, stream);
}

// ---- one whole training step on the device (see include/waveflow_hip.h)

// Is the train state complete for an entry?  The counter is every entry's; `need`: what else the entry reads or writes -- kUpdate: the
// parameters, Adam's moments and the loss ring (the entries that move the parameters), kAverage: the running average (those that sweep E_L)
enum : unsigned { kUpdate = 1, kAverage = 2 };
static bool state_has(const wf_train_state* st, unsigned need) {
    if (!st->counter_dev || ((need & kAverage) && !st->running_average_dev)) return false;
    return !(need & kUpdate) || (st->params_dev && st->m_dev && st->v_dev && st->loss_ring_dev && st->ring_len >= 1);
}

// Workspace of a fused Adam step over n walkers (VQMC) or rows (maximum likelihood): byte offsets of the walkers (VQMC only), the per-walker
// values (local energies / log_pdf), the flat gradient, the batch sums ([3] doubles) and their workspace, then the sweeps' area, which is
// everything the caller's buffer holds from `sweep` on (`total` counts what the sweeps ask for at least).
struct StepLayout { int64_t x, values, grad, sums, sums_ws, sweep, total; };
static StepLayout step_layout(const wf_model* m, int64_t n, int64_t x_bytes, int64_t sweep_bytes) {
    Bump b;
    StepLayout l{};
    l.x = b.take(x_bytes);
    l.values = b.take(n * 4);
    l.grad = b.take(m->n_params * 4);
    l.sums = b.take(256);
    l.sums_ws = b.take(block_sums_ws_bytes(n));
    l.sweep = b.at;
    l.total = b.at + sweep_bytes;
    return l;
}
// (the staged sampler of large batches works in the gradient's area before the gradient needs it)
static StepLayout vqmc_layout(const wf_model* m, int64_t batch) {
    return step_layout(m, batch, batch * m->desc.n_dim * 4, std::max<int64_t>(vjp_ws_bytes(m, batch, true), align256(step_sampler_bytes(m, batch))));
}
static StepLayout mle_layout(const wf_model* m, int64_t N) { return step_layout(m, N, 0, vjp_ws_bytes(m, N, false)); }

// Adam step of a captured training step: the gradient is either in `grad` (several chunks) or still in the per-split partial images
// of the single chunk (split > 0), in which case the gather is part of the update kernel
static int adam_from_sweep(wf_model* m, const wf_train_state* st, const float* grad, int split, float step_size, float b1, float b2, float eps,
                           void* stream) {
    const unsigned long long* counter = (const unsigned long long*)st->counter_dev;
    if (split > 0) {
        const int64_t n_img = plain_fwd_floats(m->desc.n_dim, m->nbp) * (int64_t)m->nets.size();
        return launch_adam_partials(st->params_dev, m->d_grad_partial, split, n_img, m->d_grad_map, st->m_dev, st->v_dev, m->n_params, step_size, b1,
                                    b2, eps, counter, stream);
    }
    return launch_adam(st->params_dev, grad, st->m_dev, st->v_dev, m->n_params, 0, step_size, b1, b2, eps, counter, stream);
}

// What wf_vqmc_train_step and its local half share: walkers ~ the sampler (stream advanced by the device counter), then the mean local energy and
// its gradient under the custom tangent rule with the running average from the device scalar.  *split as adam_from_sweep takes it (gated heads:
// no deferred gather -- the flat gradient gets its zero_params entries).
static int sample_and_sweep(wf_model* m, const wf_train_state* st, const StepLayout& l, uint64_t seed, int64_t batch, const Protons& pr,
                            float inv_count, int exact_sampler, char* w, int64_t workspace_bytes, int* split, void* stream) {
    float* x = (float*)(w + l.x);
    const int64_t sweep_bytes = workspace_bytes - l.sweep;
    int rc = sample_step_walkers(m, seed, (const unsigned long long*)st->counter_dev, batch, x, exact_sampler, w + l.sweep, sweep_bytes, stream);
    if (rc) return rc;
    return run_vjp_chunks(m, 2, true, x, batch, nullptr, nullptr, &pr, 0.0f, inv_count, (float*)(w + l.values), (float*)(w + l.grad), w + l.sweep,
                          sweep_bytes, stream, st->running_average_dev, m->z_rows ? nullptr : split);
}

int64_t wf_vqmc_train_step_workspace_bytes(const wf_model* m, int64_t batch) {
    if (!m || batch < 1) return WF_ERR_INVALID;
    if (!vqmc_step_covered(m, batch, false)) return WF_ERR_UNSUPPORTED;
    return vqmc_layout(m, batch).total;
}

int wf_vqmc_train_step(wf_model* m, const wf_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                       float step_size, float b1, float b2, float eps, int32_t exact_sampler, void* workspace_dev, int64_t workspace_bytes,
                       void* stream) {
    Protons pr{};
    if (!m || !st || batch < 1 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (!state_has(st, kUpdate | kAverage)) return WF_ERR_INVALID;
    if (!vqmc_step_covered(m, batch, true)) return WF_ERR_UNSUPPORTED;
    const StepLayout l = vqmc_layout(m, batch);
    if (!m->params_set || !workspace_dev || workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    char* w = (char*)workspace_dev;
    int split = 0;
    int rc = sample_and_sweep(m, st, l, seed, batch, pr, 1.0f / (float)batch, exact_sampler, w, workspace_bytes, &split, stream);
    if (rc) return rc;
    rc = adam_from_sweep(m, st, (float*)(w + l.grad), split, step_size, b1, b2, eps, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables || step_reads_eval_tables(m, batch));
    if (rc) return rc;
    // batch sums of the local energies -> loss ring, step counter + 1 (after Adam, which reads the counter as its step index)
    return launch_block_sums((float*)(w + l.values), batch, (double*)(w + l.sums), w + l.sums_ws, block_sums_ws_bytes(batch), stream, st->loss_ring_dev,
                             st->ring_len, (unsigned long long*)st->counter_dev);
}

int wf_vqmc_train_step_local(wf_model* m, const wf_train_state* st, uint64_t seed, int64_t batch_local, const float* protons_host, int32_t n_protons,
                             float inv_global_batch, int32_t exact_sampler, double* reduce_dev, void* workspace_dev, int64_t workspace_bytes,
                             void* stream) {
    Protons pr{};
    if (!m || !st || !reduce_dev || batch_local < 1 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (!state_has(st, kAverage)) return WF_ERR_INVALID;
    if (!vqmc_step_covered(m, batch_local, true)) return WF_ERR_UNSUPPORTED;
    const StepLayout l = vqmc_layout(m, batch_local);
    if (!m->params_set || !workspace_dev || workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    char* w = (char*)workspace_dev;
    int split = 0;
    int rc = sample_and_sweep(m, st, l, seed, batch_local, pr, inv_global_batch, exact_sampler, w, workspace_bytes, &split, stream);
    if (rc) return rc;
    const int64_t n_img = plain_fwd_floats(m->desc.n_dim, m->nbp) * (int64_t)m->nets.size();
    rc = launch_pack_reduce_buffer(m->d_grad_partial, split, n_img, m->d_grad_map, (float*)(w + l.grad), m->n_params, reduce_dev, stream);
    if (rc) return rc;
    m->local_step_tile = step_reads_eval_tables(m, batch_local);   // -> wf_vqmc_train_step_apply refreshes everything
    return launch_block_sums((float*)(w + l.values), batch_local, reduce_dev + m->n_params, w + l.sums_ws, block_sums_ws_bytes(batch_local), stream);
}

int wf_vqmc_train_step_apply(wf_model* m, const wf_train_state* st, const double* reduce_dev, float step_size, float b1, float b2, float eps,
                             void* stream) {
    if (!m || !st || !reduce_dev) return WF_ERR_INVALID;
    if (!state_has(st, kUpdate)) return WF_ERR_INVALID;
    if (!grad_supported(m, false)) return WF_ERR_UNSUPPORTED;
    DeviceGuard g(m->device);
    int rc = launch_adam_reduced(st->params_dev, reduce_dev, st->m_dev, st->v_dev, m->n_params, step_size, b1, b2, eps,
                                 (const unsigned long long*)st->counter_dev, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables || m->local_step_tile);   // (what the local half found: step_reads_eval_tables)
    if (rc) return rc;
    return launch_ring_push(reduce_dev + m->n_params, st->loss_ring_dev, st->ring_len, (unsigned long long*)st->counter_dev, stream);
}

int64_t wf_mle_train_step_workspace_bytes(const wf_model* m, int64_t N) {
    if (!m || N < 1) return WF_ERR_INVALID;
    if (!grad_supported(m, false)) return WF_ERR_UNSUPPORTED;
    return mle_layout(m, N).total;
}

int wf_mle_train_step(wf_model* m, const wf_train_state* st, const float* x_dev, int64_t N, float step_size, float b1, float b2, float eps,
                      void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!m || !st || !x_dev || N < 1) return WF_ERR_INVALID;
    if (!state_has(st, kUpdate)) return WF_ERR_INVALID;
    if (!grad_supported(m, false)) return WF_ERR_UNSUPPORTED;
    const StepLayout l = mle_layout(m, N);
    if (!m->params_set || !workspace_dev || workspace_bytes < l.total) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    char* w = (char*)workspace_dev;
    float *lp = (float*)(w + l.values), *grad = (float*)(w + l.grad);
    // loss = -mean log_pdf (benchmark_tests.py:84-87): value from the forward sweep, gradient from the reverse sweep
    int split = 0;
    int rc = run_vjp_chunks(m, 3, false, x_dev, N, nullptr, nullptr, nullptr, 0.0f, -1.0f / (float)N, lp, grad, w + l.sweep, workspace_bytes - l.sweep,
                            stream, nullptr, m->z_rows ? nullptr : &split);
    if (rc) return rc;
    rc = adam_from_sweep(m, st, grad, split, step_size, b1, b2, eps, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables);   // (no sampler, log_pdf only: this step never reads the evaluation tables)
    if (rc) return rc;
    return launch_block_sums(lp, N, (double*)(w + l.sums), w + l.sums_ws, block_sums_ws_bytes(N), stream, st->loss_ring_dev, st->ring_len,
                             (unsigned long long*)st->counter_dev);
}

int wf_vqmc_seeds(const float* x_dev, int64_t B, int32_t n_dim, const float* protons_host, int32_t n_protons, const float* hpsi_dev,
                  const float* psi_dev, float running_average, float inv_count, float* e_loc_dev, float* w_psi_dev, float* w_lap_dev,
                  void* stream) {
    Protons pr{};
    if (B < 0 || n_dim < 1 || n_dim > WF_MAX_DIM || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (B > 0 && (!x_dev || !hpsi_dev || !psi_dev || !e_loc_dev || !w_psi_dev || !w_lap_dev)) return WF_ERR_INVALID;
    if (B == 0) return WF_OK;
    return launch_vqmc_seeds(x_dev, B, n_dim, pr, hpsi_dev, psi_dev, running_average, inv_count, e_loc_dev, w_psi_dev, w_lap_dev, nullptr, stream);
}

int64_t wf_block_sums_workspace_bytes(int64_t B) { return block_sums_ws_bytes(B); }

int wf_block_sums(const float* v_dev, int64_t B, double* out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (B < 0 || !out_dev || (B > 0 && !v_dev)) return WF_ERR_INVALID;
    if (workspace_bytes < block_sums_ws_bytes(B) || !workspace_dev) return WF_ERR_INVALID;
    return launch_block_sums(v_dev, B, out_dev, workspace_dev, workspace_bytes, stream);
}

}  // extern "C"
