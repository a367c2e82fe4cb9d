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
static int64_t align256(int64_t v) { return (v + 255) / 256 * 256; }

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

int64_t wf_vqmc_train_step_workspace_bytes(const wf_model* m, int64_t batch) {
    if (!m || batch < 1) return WF_ERR_INVALID;
    // (capability, not the current state: a size queried while the evaluation tables are stale holds after the next full refresh as well)
    if (!m->d_grad_map || !m->grad_psi_ok || !m->wave_ok || (batch > kWaveSampleMax && !tile_sample_capable_at(m, batch))) return WF_ERR_UNSUPPORTED;
    // (the staged sampler of large batches works in the gradient's workspace before the gradient needs it)
    return align256(batch * m->desc.n_dim * 4) + align256(batch * 4) + align256(m->n_params * 4) + 256 + align256(block_sums_ws_bytes(batch)) +
           std::max<int64_t>(vjp_ws_bytes(m, batch, true), tile_sample_capable_at(m, batch) ? align256(tile_sample_floats(std::min(batch, kTileSampleChunk), m->mdev.nbk) * 4) : 0);
}

int wf_vqmc_train_step(wf_model* m, const wf_train_state* st, uint64_t seed, int64_t batch, const float* protons_host, int32_t n_protons,
                       float step_size, float b1, float b2, float eps, int32_t exact_sampler, void* workspace_dev, int64_t workspace_bytes,
                       void* stream) {
    Protons pr{};
    if (!m || !st || batch < 1 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (!st->params_dev || !st->m_dev || !st->v_dev || !st->counter_dev || !st->running_average_dev || !st->loss_ring_dev || st->ring_len < 1)
        return WF_ERR_INVALID;
    if (!m->d_grad_map || !m->grad_psi_ok || !m->wave_ok || (batch > kWaveSampleMax && !tile_sample_ok(m, batch))) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev || workspace_bytes < wf_vqmc_train_step_workspace_bytes(m, batch)) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    const int D = m->desc.n_dim;
    char* p = (char*)workspace_dev;
    float* x = (float*)p; p += align256(batch * D * 4);
    float* e_loc = (float*)p; p += align256(batch * 4);
    float* grad = (float*)p; p += align256(m->n_params * 4);
    double* sums = (double*)p; p += 256;
    void* sums_ws = p; p += align256(block_sums_ws_bytes(batch));
    const int64_t vjp_bytes = workspace_bytes - (p - (char*)workspace_dev);
    const unsigned long long* counter = (const unsigned long long*)st->counter_dev;
    // walkers ~ the sampler, stream advanced by the device counter
    int rc = tile_sample_ok(m, batch)
                 ? run_tile_sample(m, 1, seed, nullptr, batch, x, nullptr, exact_sampler, counter, (float*)p, vjp_bytes / 4, stream)
                 : launch_wave_sample(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, 1, (unsigned long long)seed, nullptr, batch, x, nullptr,
                                      exact_sampler, counter, stream);
    if (rc) return rc;
    // mean local energy and its gradient under the custom tangent rule, running average from the device scalar
    int split = 0;   // (gated heads: no deferred gather -- the flat gradient gets its zero_params entries, Adam reads it)
    rc = run_vjp_chunks(m, 2, true, x, batch, nullptr, nullptr, &pr, 0.0f, 1.0f / (float)batch, e_loc, grad, p, vjp_bytes, stream,
                        st->running_average_dev, m->z_rows ? nullptr : &split);
    if (rc) return rc;
    rc = adam_from_sweep(m, st, grad, split, step_size, b1, b2, eps, stream);
    if (rc) return rc;
    // A step whose batch size puts it on the matrix-core sampler / gradient reads the MFMA image and the composite tables: it refreshes them
    // whatever defer_eval_tables says -- a hipGraph of this step replays the kernels chosen at capture, and a deferred refresh would leave
    // them on stale tables from the second replay on (the selection above does not depend on the deferral either: with stale tables at
    // call time the step takes the wave sweeps, which are valid in every replay).
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables || tile_sample_capable_at(m, batch) || grad_tile_capable_at(m, batch));
    if (rc) return rc;
    // batch sums of the local energies -> loss ring, step counter + 1 (after Adam, which reads the counter as its step index)
    return launch_block_sums(e_loc, batch, sums, sums_ws, block_sums_ws_bytes(batch), stream, st->loss_ring_dev, st->ring_len,
                             (unsigned long long*)st->counter_dev);
}

int wf_vqmc_train_step_local(wf_model* m, const wf_train_state* st, uint64_t seed, int64_t batch_local, const float* protons_host, int32_t n_protons,
                             float inv_global_batch, int32_t exact_sampler, double* reduce_dev, void* workspace_dev, int64_t workspace_bytes,
                             void* stream) {
    Protons pr{};
    if (!m || !st || !reduce_dev || batch_local < 1 || !make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    if (!st->counter_dev || !st->running_average_dev) return WF_ERR_INVALID;
    if (!m->d_grad_map || !m->grad_psi_ok || !m->wave_ok || (batch_local > kWaveSampleMax && !tile_sample_ok(m, batch_local))) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev || workspace_bytes < wf_vqmc_train_step_workspace_bytes(m, batch_local)) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    const int D = m->desc.n_dim;
    char* p = (char*)workspace_dev;
    float* x = (float*)p; p += align256(batch_local * D * 4);
    float* e_loc = (float*)p; p += align256(batch_local * 4);
    float* grad = (float*)p; p += align256(m->n_params * 4);
    p += 256;
    void* sums_ws = p; p += align256(block_sums_ws_bytes(batch_local));
    const int64_t vjp_bytes = workspace_bytes - (p - (char*)workspace_dev);
    int rc = tile_sample_ok(m, batch_local)
                 ? run_tile_sample(m, 1, seed, nullptr, batch_local, x, nullptr, exact_sampler, (const unsigned long long*)st->counter_dev, (float*)p,
                                   vjp_bytes / 4, stream)
                 : launch_wave_sample(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, 1, (unsigned long long)seed, nullptr, batch_local, x,
                                      nullptr, exact_sampler, (const unsigned long long*)st->counter_dev, stream);
    if (rc) return rc;
    int split = 0;
    rc = run_vjp_chunks(m, 2, true, x, batch_local, nullptr, nullptr, &pr, 0.0f, inv_global_batch, e_loc, grad, p, vjp_bytes, stream,
                        st->running_average_dev, m->z_rows ? nullptr : &split);
    if (rc) return rc;
    const int64_t n_img = plain_fwd_floats(D, m->nbp) * (int64_t)m->nets.size();
    rc = launch_pack_reduce_buffer(m->d_grad_partial, split, n_img, m->d_grad_map, grad, m->n_params, reduce_dev, stream);
    if (rc) return rc;
    m->local_step_tile = tile_sample_capable_at(m, batch_local) || grad_tile_capable_at(m, batch_local);   // -> wf_vqmc_train_step_apply refreshes everything
    return launch_block_sums(e_loc, batch_local, reduce_dev + m->n_params, sums_ws, block_sums_ws_bytes(batch_local), stream);
}

int wf_vqmc_train_step_apply(wf_model* m, const wf_train_state* st, const double* reduce_dev, float step_size, float b1, float b2, float eps,
                             void* stream) {
    if (!m || !st || !reduce_dev) return WF_ERR_INVALID;
    if (!st->params_dev || !st->m_dev || !st->v_dev || !st->counter_dev || !st->loss_ring_dev || st->ring_len < 1) return WF_ERR_INVALID;
    if (!m->d_grad_map) return WF_ERR_UNSUPPORTED;
    DeviceGuard g(m->device);
    int rc = launch_adam_reduced(st->params_dev, reduce_dev, st->m_dev, st->v_dev, m->n_params, step_size, b1, b2, eps,
                                 (const unsigned long long*)st->counter_dev, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables || m->local_step_tile);   // (see wf_vqmc_train_step)
    if (rc) return rc;
    return launch_ring_push(reduce_dev + m->n_params, st->loss_ring_dev, st->ring_len, (unsigned long long*)st->counter_dev, stream);
}

int64_t wf_mle_train_step_workspace_bytes(const wf_model* m, int64_t N) {
    if (!m || N < 1) return WF_ERR_INVALID;
    if (!m->d_grad_map) return WF_ERR_UNSUPPORTED;
    return align256(N * 4) + align256(m->n_params * 4) + 256 + align256(block_sums_ws_bytes(N)) + vjp_ws_bytes(m, N, false);
}

int wf_mle_train_step(wf_model* m, const wf_train_state* st, const float* x_dev, int64_t N, float step_size, float b1, float b2, float eps,
                      void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (!m || !st || !x_dev || N < 1) return WF_ERR_INVALID;
    if (!st->params_dev || !st->m_dev || !st->v_dev || !st->counter_dev || !st->loss_ring_dev || st->ring_len < 1) return WF_ERR_INVALID;
    if (!m->d_grad_map) return WF_ERR_UNSUPPORTED;
    if (!m->params_set || !workspace_dev || workspace_bytes < wf_mle_train_step_workspace_bytes(m, N)) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    char* p = (char*)workspace_dev;
    float* lp = (float*)p; p += align256(N * 4);
    float* grad = (float*)p; p += align256(m->n_params * 4);
    double* sums = (double*)p; p += 256;
    void* sums_ws = p; p += align256(block_sums_ws_bytes(N));
    const int64_t vjp_bytes = workspace_bytes - (p - (char*)workspace_dev);
    // loss = -mean log_pdf (benchmark_tests.py:84-87): value from the forward sweep, gradient from the reverse sweep
    int split = 0;
    int rc = run_vjp_chunks(m, 3, false, x_dev, N, nullptr, nullptr, nullptr, 0.0f, -1.0f / (float)N, lp, grad, p, vjp_bytes, stream, nullptr,
                            m->z_rows ? nullptr : &split);
    if (rc) return rc;
    rc = adam_from_sweep(m, st, grad, split, step_size, b1, b2, eps, stream);
    if (rc) return rc;
    rc = apply_params(m, st->params_dev, stream, !st->defer_eval_tables);
    if (rc) return rc;
    return launch_block_sums(lp, N, sums, sums_ws, block_sums_ws_bytes(N), stream, st->loss_ring_dev, st->ring_len,
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
