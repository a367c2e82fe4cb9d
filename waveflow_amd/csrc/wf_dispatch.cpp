// wf_dispatch.cpp -- which kernel runs for a call: the path predicates, and the C ABI of evaluation, inverse / sampling, local energy and
// gradients built on them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "wf_model.h"

namespace wf {

// the argument checks every evaluation entry point starts with
static int check_fwd(const wf_model* m, const void* x, int64_t B, const void* out) {
    if (!m || B < 0) return WF_ERR_INVALID;
    if (B > 0 && (!x || !out)) return WF_ERR_INVALID;
    if (!m->params_set && m->n_params > 0) return WF_ERR_INVALID;
    return WF_OK;
}
// the models the reverse sweeps cover; second_order: psi and its Laplacian (Waveflow prior, IMADE layers)
bool grad_supported(const wf_model* m, bool second_order) { return m->d_grad_map && (!second_order || m->grad_psi_ok); }
// ... and every gradient entry point: the gradient is written for an empty batch too; second_order: psi and its Laplacian (wf_psi_vjp, wf_vqmc_loss_grad)
static int check_grad(const wf_model* m, const void* x, int64_t B, const void* grad, bool second_order) {
    int rc = check_fwd(m, x, B, grad);
    if (rc) return rc;
    if (!grad) return WF_ERR_INVALID;
    return grad_supported(m, second_order) ? WF_OK : WF_ERR_UNSUPPORTED;
}
// What wf_hamiltonian_fwd and wf_psi_coord_derivs refuse beyond check_fwd, in this order
int check_energy_model(const wf_model* m) {
    if (m->desc.prior_kind != WF_PRIOR_WAVEFLOW) return WF_ERR_INVALID;
    if (!m->wave_ok || !m->d_tabP3 || !m->d_grad_fk) return WF_ERR_UNSUPPORTED;
    if (m->desc.n_flow_layers > 0 && m->desc.layer_kind != WF_LAYER_IMADE) return WF_ERR_UNSUPPORTED;
    return WF_OK;
}
bool make_protons(const float* host, int n, Protons* out) {
    if (n < 0 || n > 8 || (n > 0 && !host)) return false;
    *out = Protons{};
    out->n = n;
    for (int i = 0; i < n; ++i) out->pos[i] = host[i];
    return true;
}

// ---- which kernel path runs.  Every matrix-core tile path asks the same three questions: does the model belong to the family the tile kernels
// cover (mc_family + the path's own terms), does its knob admit this batch size (at_least), and are the images it reads usable right now
// (tiles_fresh).  The *_capable_at functions answer the first two -- what workspace queries and the training steps' refresh decisions go
// by, independent of transient state; the entry points add tiles_fresh.

// what every matrix-core tile path requires of the model
static bool mc_family(const wf_model* m) {
    const wf_model_desc& d = m->desc;
    return m->mfma_ok && d.box_kind == WF_BOX_MEAN && d.layer_kind == WF_LAYER_IMADE && d.n_flow_layers > 0;
}
// ... and right now: the MFMA image and the composite tables are fresh (not between a deferred training step and the next full refresh), every
// packed weight inside the fp16 range
static bool tiles_fresh(const wf_model* m) { return !m->eval_tables_stale && !f16_overflow(m); }
// a switch point read from the environment: 0 disables the path
static bool at_least(int64_t B, int64_t tile_min) { return tile_min > 0 && B >= tile_min; }

// both H psi tile paths: ungated heads, the chunked tables, not the forced R3 sweep.  (No test of the prior: wf_hamiltonian_fwd has returned
// WF_ERR_INVALID for every prior but Waveflow's before it asks.)
static bool energy_tile_family(const wf_model* m) {
    return mc_family(m) && !m->dev.i_gate && !m->dev.p_gate && m->d_tabI4c && m->d_tabP4c && !env_energy_r3();
}
// D = 2 (wf_kernels_etile.hip).  <= 32 bases: the one-kernel form or, if the nets do not fit LDS together, the launch-per-net form; 33 .. 64 bases
// and a constant term of the prior's boundary map (p_bias): the one-kernel form only
static bool energy_tile2_capable_at(const wf_model* m, int64_t B) {
    const bool fused = energy_tile_fused(&m->mdev);
    return m->desc.n_dim == 2 && (m->nbp == 32 || (m->nbp == 64 && fused)) && energy_tile_family(m) && (!m->mdev.p_bias || fused) && at_least(B, env_energy_tile_min());
}
// D >= 3 (wf_kernels_etile_dir.hip): <= 32 bases
static bool energy_dir_capable_at(const wf_model* m, int64_t B) {
    return m->desc.n_dim >= 3 && m->nbp == 32 && energy_tile_family(m) && energy_dir_capable(&m->mdev) && at_least(B, env_energy_tile_min());
}
// the matrix-core gradient path (wf_kernels_etile_bwd.hip): D = 2, <= 64 bases; WF_GRAD_TILE_MIN (read per call).  d_egacc: the gradient blocks
// grad_prepare allocates where the path exists; gates and the one-kernel form are energy_vjp_capable's business
static bool grad_tile_capable_at(const wf_model* m, int64_t B) {
    if (!m->d_egacc) return false;
    return at_least(B, env_grad_tile_min()) && m->desc.n_dim == 2 && (m->nbp == 32 || m->nbp == 64) && mc_family(m) && m->desc.prior_kind == WF_PRIOR_WAVEFLOW &&
           m->d_tabI4c && m->d_tabP4c && energy_vjp_capable(&m->mdev);
}
// Large batches of the two-particle family (the family of the matrix-core local energy, <= 64 bases): the staged inverse / sampler of
// wf_kernels_etile_sample.hip (conditioners on the matrix cores, one lane per walker for the searches).  WF_SAMPLE_TILE_MIN (read per call) moves the switch
// point; 0 disables the path.  It reads the MFMA image and the composite dimension-0 tables: not while they are stale (deferred training steps).
static bool tile_sample_capable_at(const wf_model* m, int64_t B) {
    const wf_model_desc& d = m->desc;
    // (the piecewise-constant envelope of k_tsample's second prior column takes the maximum over at most 9 coefficients per knot interval:
    // prior degrees above 8 keep the wave / one-lane samplers, whose bound is the global one)
    return at_least(B, env_sample_tile_min()) && d.n_dim == 2 && m->nbp == 32 * m->mdev.nbk && mc_family(m) && d.prior_kind == WF_PRIOR_WAVEFLOW && d.p_degree <= 8 &&
           m->d_tabI4 && m->d_tabP3 && m->dev.b_to_ob && m->d_grad_fk && tile_sample_capable(&m->mdev);
}
static bool tile_sample_ok(const wf_model* m, int64_t B) { return tile_sample_capable_at(m, B) && tiles_fresh(m); }

// Does a training step of B walkers read the evaluation tables (the MFMA image, the composite tables)?  At a batch size of the matrix-core sampler
// or gradient it does, and then refreshes them whatever defer_eval_tables says: a hipGraph of the step replays the kernels chosen at capture, and a
// deferred refresh would leave them on stale tables from the second replay on.  (Capability, not tiles_fresh: with stale tables at call time the
// step takes the wave sweeps, which are valid in every replay.)
bool step_reads_eval_tables(const wf_model* m, int64_t B) { return tile_sample_capable_at(m, B) || grad_tile_capable_at(m, B); }
// What wf_vqmc_train_step and its local half require of a model: the second-order gradient, the wave sweeps, and a sampler for B walkers (the staged
// one beyond kWaveSampleMax).  current = false: capability, for size queries (a size queried while the tables are stale holds after the next
// full refresh as well); true: the state at call time.
bool vqmc_step_covered(const wf_model* m, int64_t B, bool current) {
    return grad_supported(m, true) && m->wave_ok && (B <= kWaveSampleMax || (current ? tile_sample_ok(m, B) : tile_sample_capable_at(m, B)));
}

// presort: the rows of x arrive in any order -- evaluate on the ascending sort of each row, psi (mode 1) times (-1)^inversions (helpers.py:55-58).
// The MFMA kernel sorts in registers; the wave and the scalar kernel read sorted rows from the model's scratch (one small launch in front,
// the sign behind).
static int dispatch(const wf_model* m, int mode, const float* x, int64_t B, float* out, float* u, int32_t* idx, void* stream, bool presort = false) {
    DeviceGuard g(m->device);
    if (B == 0) return WF_OK;
    if (m->is_nsc) {
        if (mode == 1 || idx || presort) return WF_ERR_UNSUPPORTED;
        return launch_nsc_model(m->nsc, mode, x, B, out, u, stream);
    }
    const int Dm = m->desc.n_dim;
    // sorted rows + inversion counts for the kernels that do not sort themselves: behind the first `front` floats of the scratch
    auto presorted = [&](int64_t front, const float** xs, int32_t** inv) -> int {
        int rc = ensure_scratch(m, front + B * (Dm + 1));
        if (rc) return rc;
        float* s = m->d_scratch + front;
        *inv = reinterpret_cast<int32_t*>(s + B * Dm);
        rc = launch_sort_rows(*xs, B, Dm, s, *inv, stream);   // (*xs: the caller's rows -- replaced by the sorted copy only now)
        *xs = s;
        return rc;
    };
    // Small batches: one wave per walker (wf_kernels_wave.hip) takes 14 us for up to ~1000 walkers where the MFMA kernel,
    // which first stages its weight images into LDS, takes 38-42 us whatever the batch; from ~7000 walkers on the MFMA
    // kernel's throughput wins (4096: 30 vs 42 us, 8192: 46 vs 42 us).  The wave kernel does
    // not report bin indices.
    const bool wave_fits = m->wave_ok && !idx;
    const bool use_wave = wave_fits && (m->kernel_kind == WF_KERNEL_WAVE || (m->kernel_kind == WF_KERNEL_AUTO && B <= kWaveEvalMax));
    if (m->kernel_kind == WF_KERNEL_WAVE && !use_wave) return WF_ERR_UNSUPPORTED;
    if (use_wave) {
        const int D = m->desc.n_dim;
        const int64_t chunk = std::min<int64_t>(B, (int64_t)1 << 20);
        int rc = ensure_scratch(m, chunk * wave_tail_floats(D, 0) + (presort ? B * (D + 1) : 0));
        if (rc) return rc;
        int32_t* inv = nullptr;
        if (presort) {
            rc = presorted(chunk * wave_tail_floats(D, 0), &x, &inv);
            if (rc) return rc;
        }
        for (int64_t c0 = 0; c0 < B; c0 += chunk) {
            const int64_t bc = std::min(chunk, B - c0);
            rc = launch_wave_eval(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, mode, x + c0 * D, bc, out + c0, u ? u + c0 * D : nullptr,
                                  m->d_scratch, stream);
            if (rc) return rc;
        }
        return (presort && mode == 1) ? launch_apply_sign(out, inv, B, stream) : WF_OK;
    }
    bool use_mfma = m->mfma_ok && m->kernel_kind != WF_KERNEL_SCALAR;
    if (use_mfma && f16_overflow(m)) {   // a weight outside the fp16 range: the fp32 kernels only
        if (m->kernel_kind == WF_KERNEL_MFMA) return WF_ERR_UNSUPPORTED;
        use_mfma = false;
    }
    if (use_mfma)
        return launch_mfma(m->dev.D, m->mdev.nbk, &m->mdev, (int)(m->mfma_lds_floats * sizeof(float)), mode | (presort ? kModePresort : 0), x, B, out, u, idx, stream);
    int32_t* inv = nullptr;
    if (presort) {
        int rc = presorted(0, &x, &inv);
        if (rc) return rc;
    }
    int rc = launch_scalar(m->dev, m->d_dev, mode, x, B, out, u, idx, stream);
    if (rc || !(presort && mode == 1)) return rc;
    return launch_apply_sign(out, inv, B, stream);
}

// in passes of what the workspace holds; a walker's stream is keyed by its index in the batch, whatever the passes
static int run_tile_sample(const wf_model* m, int draw, uint64_t seed, const float* u_dev, int64_t B, float* x_dev, float* latent_dev, int exact,
                           const unsigned long long* counter_dev, float* ws, int64_t ws_floats, void* stream) {
    int64_t chunk = B;
    while (chunk > 32 && tile_sample_floats(chunk, m->mdev.nbk) > ws_floats) chunk = ((chunk / 2) + 31) / 32 * 32;
    if (tile_sample_floats(chunk, m->mdev.nbk) > ws_floats) return WF_ERR_INVALID;
    for (int64_t c0 = 0; c0 < B; c0 += chunk) {
        const int64_t bc = std::min(chunk, B - c0);
        int rc = launch_tile_sample(&m->mdev, m->dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, draw, (unsigned long long)seed, u_dev ? u_dev + c0 * 2 : nullptr, bc,
                                    x_dev + c0 * 2, latent_dev ? latent_dev + c0 * 2 : nullptr, exact, counter_dev, c0, ws, stream);
        if (rc) return rc;
    }
    return WF_OK;
}

// The walkers of one training step, stream advanced by the device counter: the staged matrix-core sampler where it applies right now (in passes
// of what `scratch` holds), the wave sampler otherwise -- the step's coverage check has made sure that one of them takes B walkers.  (wf_sample
// and wf_inverse_fwd choose for themselves: sample_or_invert.)
int sample_step_walkers(const wf_model* m, uint64_t seed, const unsigned long long* counter_dev, int64_t B, float* x_dev, int exact, void* scratch,
                        int64_t scratch_bytes, void* stream) {
    if (tile_sample_ok(m, B)) return run_tile_sample(m, 1, seed, nullptr, B, x_dev, nullptr, exact, counter_dev, (float*)scratch, scratch_bytes / 4, stream);
    return launch_wave_sample(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, 1, (unsigned long long)seed, nullptr, B, x_dev, nullptr, exact,
                              counter_dev, stream);
}
// what the staged sampler asks of a step's workspace (0 where it does not apply): a pass of at most kTileSampleChunk walkers
int64_t step_sampler_bytes(const wf_model* m, int64_t B) {
    return tile_sample_capable_at(m, B) ? tile_sample_floats(std::min(B, kTileSampleChunk), m->mdev.nbk) * 4 : 0;
}

// Workspace of the taped sweeps for a chunk of walkers, in floats: the tape at 0, then the tails, four floats per walker (H psi, psi, w_psi, w_lap:
// [4][chunk]) and, for gated heads, one zero_params adjoint per (sample, head lane) ([chunk * samples][z_rows]).  Every part is linear in the chunk.
struct SweepWs {
    int kind;                                          // coefficient ring of the sweep
    int64_t samples, tails, per_walker, zws, floats;   // samples per walker; float offsets of the parts behind the tape; the total
};
static SweepWs sweep_ws(const wf_model* m, bool second_order, int64_t chunk) {
    const int D = m->desc.n_dim;
    SweepWs w{};
    w.kind = second_order ? m->ring2 : 0;
    w.samples = ring_samples(D, w.kind);
    w.tails = chunk * w.samples * (int64_t)m->nets.size() * grad_ws_rows(D, m->nbp) * ring_coefs(D, w.kind);
    w.per_walker = w.tails + chunk * wave_tail_floats(D, w.kind);
    w.zws = w.per_walker + 4 * chunk;
    w.floats = w.zws + chunk * w.samples * m->z_rows;
    return w;
}
static int64_t vjp_bytes_per_walker(const wf_model* m, bool second_order) { return sweep_ws(m, second_order, 1).floats * (int64_t)sizeof(float); }

// the tape of up to 32768 walkers: the wave path of every gradient and Jacobian workspace query (the Jacobian entries never take another)
static int64_t tape_ws_bytes(const wf_model* m, int64_t B, bool second_order) {
    if (!m || B < 0) return WF_ERR_INVALID;
    if (!grad_supported(m, second_order)) return WF_ERR_UNSUPPORTED;
    return std::min<int64_t>(std::max<int64_t>(B, 1), 32768) * vjp_bytes_per_walker(m, second_order);
}
int64_t vjp_ws_bytes(const wf_model* m, int64_t B, bool second_order) {
    int64_t bytes = tape_ws_bytes(m, B, second_order);
    if (bytes > 0 && second_order && grad_tile_capable_at(m, B)) {   // the matrix-core gradient path has a fixed part (the partial gradient blocks of every net): only where the path applies (a smaller WF_GRAD_TILE_MIN at query time moves it)
        const int n_nets = (int)m->nets.size();
        const int64_t chunk = std::min<int64_t>(std::max<int64_t>(B, 1), 32768);
        bytes = std::max<int64_t>(bytes, (energy_vjp_fixed_floats(n_nets, m->mdev.nbk) + ((chunk + 31) / 32 * 32) * energy_vjp_floats_per_walker(n_nets)) * (int64_t)sizeof(float));
    }
    return bytes;
}

// mode 0: log_pdf, w1 only;  mode 1: psi (w1) and, with second_order, its Laplacian (w2);
// mode 2: loss_fn_efficient (vqmc.py:193-212): the weights come from H psi of the same forward sweep, e_loc_dev is written
// mode 3: maximum likelihood: every walker carries the weight inv_count (signed), e_loc_dev receives log_pdf of the same sweep
int run_vjp_chunks(const wf_model* m, int mode, bool second_order, const float* x_dev, int64_t B, const float* w1, const float* w2,
                   const Protons* pr, float running_average, float inv_count, float* e_loc_dev, float* grad_dev, void* workspace_dev,
                   int64_t workspace_bytes, void* stream, const float* running_average_dev, int* defer_gather_split) {
    const int D = m->desc.n_dim;
    const int64_t chunk = workspace_bytes / vjp_bytes_per_walker(m, second_order);
    if (B > 0 && chunk < 1) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    hipStream_t s = (hipStream_t)stream;
    const int n_nets = (int)m->nets.size();
    const int64_t fwd = plain_fwd_floats(D, m->nbp);
    const int64_t n_img = fwd * n_nets;
    const SweepWs w = sweep_ws(m, second_order, chunk);
    float* tape = (float*)workspace_dev;
    float *tails = tape + w.tails, *per_walker = tape + w.per_walker, *zws = m->z_rows ? tape + w.zws : nullptr;
    if (B == 0) {   // the gradient of an empty batch is zero
        WF_HIP(hipMemsetAsync(grad_dev, 0, (size_t)m->n_params * sizeof(float), s));
        return WF_OK;
    }
    // Large batches of the two-particle family (the family of the one-kernel H psi, <= 64 bases): forward, reverse and weight-gradient products on the
    // matrix cores (wf_kernels_etile_bwd.hip: k_efused with the per-net input jets, k_ebwd per net with the weight-gradient products inside).  WF_GRAD_TILE_MIN (read per call) moves the
    // switch point; 0 disables the path.
    if ((mode == 1 || mode == 2) && second_order && m->d_egacc) {
        const bool family = grad_tile_capable_at(m, B) && tiles_fresh(m);
        const int64_t per = energy_vjp_floats_per_walker(n_nets) * (int64_t)sizeof(float), fixed = energy_vjp_fixed_floats(n_nets, m->mdev.nbk) * (int64_t)sizeof(float);
        const int64_t tchunk = workspace_bytes > fixed ? ((workspace_bytes - fixed) / per) / 32 * 32 : 0;
        if (family && tchunk >= 32) {
            Protons none{};
            for (int64_t c0 = 0; c0 < B; c0 += tchunk) {
                const int64_t bc = std::min(tchunk, B - c0);
                int rc = launch_energy_vjp(&m->mdev, m->dev, m->d_tabI4c, m->d_tabP4c, x_dev + c0 * D, bc, mode, w1 ? w1 + c0 : nullptr, w2 ? w2 + c0 : nullptr,
                                           pr ? *pr : none, running_average, running_average_dev, inv_count, e_loc_dev ? e_loc_dev + c0 : nullptr,
                                           (float*)workspace_dev, m->d_egacc, c0 > 0, stream);
                if (rc) return rc;
            }
            std::vector<int> offs((size_t)n_nets * 8);
            std::vector<float> c2((size_t)n_nets);
            for (int n = 0; n < n_nets; ++n) {
                const NetOffsets q = net_offsets(m, n);
                int* o = &offs[(size_t)n * 8];
                o[0] = (int)q.W0; o[1] = (int)q.b0; o[2] = (int)q.W1; o[3] = (int)q.b1; o[4] = (int)q.W2; o[5] = (int)q.b2; o[6] = q.NO; o[7] = m->nets[n].n_out;
                c2[n] = net_has_sigmoid_head(m, n) ? -1.4426950408889634f : 1.0f;
            }
            if (defer_gather_split) *defer_gather_split = 0;   // the gradient is in grad_dev
            return launch_energy_vjp_finish(m->d_egacc, n_nets, m->mdev.nbk, offs.data(), c2.data(), grad_dev, m->n_params, stream);
        }
    }
    const bool single = B <= chunk;   // one chunk: the partial images are summed by the gather itself (one launch less)
    int split = 0;
    for (int64_t c0 = 0; c0 < B; c0 += chunk) {
        const int64_t bc = std::min(chunk, B - c0);
        const float* x = x_dev + c0 * D;
        float *wp = per_walker + 2 * chunk, *wl = per_walker + 3 * chunk;
        int rc = launch_wave_fwd(m->dev, m->d_dev, w.kind, m->d_tabI4, m->d_tabP3, m->d_grad_fk, x, bc, tape, tails, 1, stream);
        if (rc) return rc;
        const float *cw1 = w1 ? w1 + c0 : nullptr, *cw2 = w2 ? w2 + c0 : nullptr;
        if (mode == 2) {
            // (writing E_L and the weights from inside the forward kernel -- possible in RF, where a sample is a whole walker -- was
            // measured slower: the kernel grows by more than the 4.6 us launch it saves)
            rc = launch_energy_seeds(D, w.kind, tails, x, bc, m->dev.constrained_mask, *pr, running_average, running_average_dev, inv_count,
                                     e_loc_dev + c0, wp, wl, stream);
            if (rc) return rc;
            cw1 = wp;
            cw2 = wl;
        }
        if (mode == 3) {
            rc = launch_tail_out(m->dev, 0, tails, bc, e_loc_dev + c0, nullptr, stream, wp, inv_count);   // log_pdf values + the constant weights
            if (rc) return rc;
            cw1 = wp;
        }
        rc = launch_wave_bwd(m->dev, m->d_dev, (mode == 0 || mode == 3) ? 0 : 1, w.kind, m->d_tabI4, m->d_tabP3, m->d_grad_fk, bc, cw1, cw2, tape,
                             tails, zws, stream);
        if (rc) return rc;
        if (zws) {
            rc = launch_zgrad_reduce(zws, bc * w.samples, m->z_rows, c0 > 0, m->d_zpart, m->d_zgrad, stream);
            if (rc) return rc;
        }
        rc = launch_wgrad(D, m->nbp, w.kind, n_nets, bc * w.samples, tape, m->d_grad_partial, c0 > 0, m->d_grad_img, fwd,
                          single ? &split : nullptr, stream);
        if (rc) return rc;
    }
    if (defer_gather_split) *defer_gather_split = single ? split : 0;
    if (single && defer_gather_split) return WF_OK;   // the caller reads m->d_grad_partial itself (launch_adam_partials; ungated models only)
    int rc = single ? launch_grad_gather_partials(m->d_grad_partial, split, n_img, m->d_grad_map, m->n_params, grad_dev, stream)
                    : launch_grad_gather(m->d_grad_img, m->d_grad_map, m->n_params, grad_dev, stream);
    if (rc || !zws) return rc;
    // the zero_params leaves (the gather wrote 0 there: they reach no weight-image entry)
    return launch_zgrad_scatter(m->d_zgrad, m->z_rows, m->d_zmap, m->d_zraw_off, m->d_plain, grad_dev, stream);
}

// Per-walker Jacobian rows (wf_logpdf_jac, wf_psi_jac): the taped wave sweeps of run_vjp_chunks, then k_wjac instead of k_wgrad + gather.
// mode 0: log_pdf, every walker seeded with 1 (logp_dev, if given, receives log_pdf of the same forward sweep); mode 1: psi (w1) and its Laplacian
// (w2, null = zeros).  The workspace holds the tape, the tails, four floats per walker and the zero_params adjoints, laid out as there; jac_dev
// [B][n_params] is the caller's.  Chunks of what the workspace holds: a row depends on its walker alone, so the chunking changes no bit.
static int run_jac_chunks(const wf_model* m, int mode, const float* x_dev, int64_t B, const float* w1, const float* w2, float* logp_dev, float* jac_dev,
                          void* workspace_dev, int64_t workspace_bytes, void* stream) {
    const bool second_order = mode == 1;
    const int D = m->desc.n_dim;
    const int64_t chunk = workspace_bytes / vjp_bytes_per_walker(m, second_order);
    if (B > 0 && chunk < 1) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    if (B == 0) return WF_OK;
    const int n_nets = (int)m->nets.size();
    const SweepWs w = sweep_ws(m, second_order, chunk);
    float* tape = (float*)workspace_dev;
    float *tails = tape + w.tails, *per_walker = tape + w.per_walker, *zws = m->z_rows ? tape + w.zws : nullptr;
    // the flat parameters of each net (leaf order: the nets follow each other and cover the vector)
    std::vector<int> seg((size_t)n_nets + 1);
    for (int n = 0; n < n_nets; ++n) seg[(size_t)n] = n == 0 ? 0 : (int)m->nets[(size_t)n].offset;
    seg[(size_t)n_nets] = (int)m->n_params;
    for (int64_t c0 = 0; c0 < B; c0 += chunk) {
        const int64_t bc = std::min(chunk, B - c0);
        int rc = launch_wave_fwd(m->dev, m->d_dev, w.kind, m->d_tabI4, m->d_tabP3, m->d_grad_fk, x_dev + c0 * D, bc, tape, tails, 1, stream);
        if (rc) return rc;
        const float *cw1 = w1 ? w1 + c0 : nullptr, *cw2 = w2 ? w2 + c0 : nullptr;
        if (mode == 0) {   // log_pdf values (to the caller, or to a per-walker slot nobody reads) + the constant seed 1
            float* wp = per_walker + 2 * chunk;
            rc = launch_tail_out(m->dev, 0, tails, bc, logp_dev ? logp_dev + c0 : per_walker, nullptr, stream, wp, 1.0f);
            if (rc) return rc;
            cw1 = wp;
        }
        rc = launch_wave_bwd(m->dev, m->d_dev, mode, w.kind, m->d_tabI4, m->d_tabP3, m->d_grad_fk, bc, cw1, cw2, tape, tails, zws, stream);
        if (rc) return rc;
        rc = launch_wjac(D, m->nbp, w.kind, n_nets, bc, tape, seg.data(), plain_fwd_floats(D, m->nbp), m->d_grad_map, zws ? m->d_zinv : nullptr, zws,
                         m->z_rows, m->d_zraw_off, m->d_plain, m->n_params, jac_dev + c0 * m->n_params, stream);
        if (rc) return rc;
    }
    return WF_OK;
}

}  // namespace wf

using namespace wf;

// The three paths of the local energy, shared by every entry point that runs its kernels: one set of predicates, switch points and chunk sizes.
// tile / dir / wave(c0, bc, ws) launch walkers [c0, c0 + bc) with the exchange buffer ws (tile: null = the one-launch form, the whole batch);
// tile_floats(bc): the exchange buffer of the launch-per-net form of the two-particle tile path.
template <class Tile, class Dir, class Wave>
static int run_energy_paths(const wf_model* m, int64_t B, int64_t (*tile_floats)(int64_t), Tile&& tile, Dir&& dir, Wave&& wave) {
    const int D = m->desc.n_dim;
    // one launch per chunk of the batch
    auto in_chunks = [&](int64_t chunk, int64_t floats, auto&& launch) -> int {
        int rc = ensure_scratch(m, floats);
        if (rc) return rc;
        for (int64_t c0 = 0; c0 < B; c0 += chunk) {
            rc = launch(c0, std::min(chunk, B - c0), m->d_scratch);
            if (rc) return rc;
        }
        return WF_OK;
    };
    // Large batches of the two-particle family: conditioner jets on the matrix cores + lane-per-walker heads (wf_kernels_etile.hip).
    // WF_ENERGY_TILE_MIN (read per call) moves the switch point; 0 disables the path.
    if (energy_tile2_capable_at(m, B) && tiles_fresh(m)) {
        if (energy_tile_fused(&m->mdev))   // every net resident in LDS: one launch for the whole batch, no exchange buffer (k_efused)
            return tile(0, B, nullptr);
        // the conditioner and the head kernels exchange 384 B per walker and net through the scratch buffer: chunks that keep it
        // (and its re-use by the next net and the next chunk) inside the 256 MB memory-side cache instead of HBM
        const int64_t tchunk = std::min<int64_t>(B, std::max<int64_t>(env_energy_tile_chunk(), 1024));
        return in_chunks(tchunk, tile_floats(tchunk), tile);
    }
    // Large batches beyond two particles: one coordinate direction at a time with Taylor triples on the matrix cores (wf_kernels_etile_dir.hip), the same
    // switch point and knobs as the two-particle tile path
    if (energy_dir_capable_at(m, B) && tiles_fresh(m)) {
        const int64_t dchunk = std::min<int64_t>(B, (int64_t)1 << 18);   // 12 D (D + 1) bytes of jets per walker: 226 MB at D = 8
        return in_chunks(dchunk, energy_dir_floats(dchunk, D), dir);
    }
    // the wave sweeps (wf_kernels_wave.hip): every batch size, every model these entry points accept
    const int64_t chunk = std::min<int64_t>(B, (int64_t)1 << 20);
    return in_chunks(chunk, chunk * wave_tail_floats(D, 1), wave);
}

extern "C" {

int wf_logpdf_fwd(const wf_model* m, const float* x_dev, int64_t B, float* logp_dev, float* u_dev, int32_t* bin_idx_dev,
                  void* stream) {
    int rc = check_fwd(m, x_dev, B, logp_dev);
    if (rc) return rc;
    return dispatch(m, 0, x_dev, B, logp_dev, u_dev, bin_idx_dev, stream);
}

int wf_psi_fwd(const wf_model* m, const float* x_dev, int64_t B, float* psi_dev, float* u_dev, int32_t* bin_idx_dev,
               void* stream) {
    int rc = check_fwd(m, x_dev, B, psi_dev);
    if (rc) return rc;
    if (m->desc.prior_kind != WF_PRIOR_WAVEFLOW) return WF_ERR_INVALID;
    return dispatch(m, 1, x_dev, B, psi_dev, u_dev, bin_idx_dev, stream);
}

int wf_psi_antisym_fwd(const wf_model* m, const float* x_dev, int64_t B, float* psi_dev, int32_t* inversions_dev, void* stream) {
    int rc = check_fwd(m, x_dev, B, psi_dev);
    if (rc) return rc;
    if (m->desc.prior_kind != WF_PRIOR_WAVEFLOW) return WF_ERR_INVALID;
    rc = dispatch(m, 1, x_dev, B, psi_dev, nullptr, nullptr, stream, true);
    if (rc || !inversions_dev || B == 0) return rc;
    DeviceGuard g(m->device);
    return launch_sort_rows(x_dev, B, m->desc.n_dim, nullptr, inversions_dev, stream);
}

int wf_logpdf_unsorted_fwd(const wf_model* m, const float* x_dev, int64_t B, float* logp_dev, void* stream) {
    int rc = check_fwd(m, x_dev, B, logp_dev);
    if (rc) return rc;
    return dispatch(m, 0, x_dev, B, logp_dev, nullptr, nullptr, stream, true);
}

int wf_inversion_count(const float* x_dev, int64_t B, int32_t n_dim, int32_t* count_dev, void* stream) {
    if (B < 0 || n_dim < 1 || n_dim > WF_MAX_DIM || (B > 0 && (!x_dev || !count_dev))) return WF_ERR_INVALID;
    if (wf_device_count() <= 0) return WF_ERR_NO_DEVICE;
    return launch_sort_rows(x_dev, B, n_dim, nullptr, count_dev, stream);
}

int wf_flow_fwd(const wf_model* m, const float* x_dev, int64_t B, float* u_dev, float* logdet_dev, void* stream) {
    int rc = check_fwd(m, x_dev, B, logdet_dev);
    if (rc) return rc;
    if (B > 0 && !u_dev) return WF_ERR_INVALID;
    return dispatch(m, 2, x_dev, B, logdet_dev, u_dev, nullptr, stream);
}

int wf_layer_fwd(const wf_model* m, int layer, const float* u_in_dev, int64_t B, float* y_dev, float* logdet_dev,
                 int32_t* bin_idx_dev, void* stream) {
    int rc = check_fwd(m, u_in_dev, B, y_dev);
    if (rc) return rc;
    if (layer < 0 || layer >= m->desc.n_flow_layers || (B > 0 && !logdet_dev)) return WF_ERR_INVALID;
    if (m->is_nsc) return WF_ERR_UNSUPPORTED;
    DeviceGuard g(m->device);
    if (B == 0) return WF_OK;
    return launch_scalar_layer(m->dev, m->d_dev, layer, u_in_dev, B, y_dev, logdet_dev, bin_idx_dev, stream);
}

// wf_sample (draw: from `seed`) and wf_inverse_fwd (of u_dev) behind their coupling-stack branches, any batch size: the staged sampler in the
// model's scratch where it applies, one wave per walker up to WF_WAVE_SAMPLE_MAX walkers (read per call), one lane per walker otherwise.
static int sample_or_invert(const wf_model* m, int draw, uint64_t seed, const float* u_dev, int64_t B, float* x_dev, float* latent_dev, int exact,
                            void* stream) {
    if (tile_sample_ok(m, B)) {
        const int64_t fl = tile_sample_floats(std::min(B, kTileSampleChunk), m->mdev.nbk);
        int rc = ensure_scratch(m, fl);
        if (rc) return rc;
        return run_tile_sample(m, draw, seed, u_dev, B, x_dev, latent_dev, exact, nullptr, m->d_scratch, fl, stream);
    }
    if (m->wave_ok && B <= env_wave_sample_max())
        return launch_wave_sample(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, draw, (unsigned long long)seed, u_dev, B, x_dev, latent_dev,
                                  exact, nullptr, stream);
    return draw ? launch_scalar_sample(m->dev, m->d_dev, (unsigned long long)seed, B, x_dev, latent_dev, exact, stream)
                : launch_scalar_inverse(m->dev, m->d_dev, u_dev, B, x_dev, exact, stream);
}

int wf_inverse_fwd(const wf_model* m, const float* u_dev, int64_t B, float* x_dev, int32_t exact, void* stream) {
    int rc = check_fwd(m, u_dev, B, x_dev);
    if (rc) return rc;
    DeviceGuard g(m->device);
    if (B == 0) return WF_OK;
    if (m->is_nsc) {   // a coupling layer's inverse is exact either way; the log-det of the inverse goes to the model's scratch
        rc = ensure_scratch(m, B);
        if (rc) return rc;
        return launch_nsc_model(m->nsc, 3, u_dev, B, m->d_scratch, x_dev, stream);
    }
    return sample_or_invert(m, 0, 0, u_dev, B, x_dev, nullptr, exact, stream);
}

int wf_sample(const wf_model* m, uint64_t seed, int64_t B, float* x_dev, float* latent_dev, int32_t exact, void* stream) {
    int rc = check_fwd(m, x_dev, B, x_dev);
    if (rc) return rc;
    DeviceGuard g(m->device);
    if (B == 0) return WF_OK;
    if (m->is_nsc) {   // z ~ prior (Philox, keyed like the other samplers), x = inverse(z)
        rc = ensure_scratch(m, B * (m->desc.n_dim + 1));
        if (rc) return rc;
        float* z = latent_dev ? latent_dev : m->d_scratch + B;
        rc = launch_nsc_latent(m->desc.prior_kind, m->desc.n_dim, (unsigned long long)seed, B, z, stream);
        if (rc) return rc;
        return launch_nsc_model(m->nsc, 3, z, B, m->d_scratch, x_dev, stream);
    }
    return sample_or_invert(m, 1, seed, nullptr, B, x_dev, latent_dev, exact, stream);
}

int wf_hamiltonian_fwd(const wf_model* m, const float* x_dev, int64_t B, const float* protons_host, int32_t n_protons, float* hpsi_dev,
                       float* psi_dev, float* laplacian_dev, void* stream) {
    int rc = check_fwd(m, x_dev, B, hpsi_dev);
    if (rc) return rc;
    Protons pr{};
    if (!make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;
    rc = check_energy_model(m);
    if (rc) return rc;
    DeviceGuard g(m->device);
    if (B == 0) return WF_OK;
    const int D = m->desc.n_dim;
    // psi and the Laplacian are optional outputs
    auto psi = [&](int64_t c0) { return psi_dev ? psi_dev + c0 : nullptr; };
    auto lap = [&](int64_t c0) { return laplacian_dev ? laplacian_dev + c0 : nullptr; };
    return run_energy_paths(
        m, B, energy_tile_floats,
        [&](int64_t c0, int64_t bc, float* ws) {
            return launch_energy_tile(&m->mdev, m->dev, m->d_tabI4c, m->d_tabP4c, m->d_grad_fk, x_dev + c0 * D, bc, pr, hpsi_dev + c0, psi(c0), lap(c0), ws, stream);
        },
        [&](int64_t c0, int64_t bc, float* ws) {
            return launch_energy_dir(&m->mdev, m->dev, m->d_tabI4c, m->d_tabP4c, x_dev + c0 * D, bc, pr, hpsi_dev + c0, psi(c0), lap(c0), ws, stream);
        },
        [&](int64_t c0, int64_t bc, float* ws) {
            return launch_wave_energy(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, x_dev + c0 * D, bc, pr, hpsi_dev + c0, psi(c0), lap(c0), ws, stream);
        });
}

int wf_psi_coord_derivs(const wf_model* m, const float* x_dev, int64_t B, float* psi_dev, float* grad_dev, float* hdiag_dev, void* stream) {
    int rc = check_fwd(m, x_dev, B, grad_dev);
    if (rc) return rc;
    rc = check_energy_model(m);
    if (rc) return rc;
    DeviceGuard g(m->device);
    if (B == 0) return WF_OK;
    const int D = m->desc.n_dim;
    auto psi = [&](int64_t c0) { return psi_dev ? psi_dev + c0 : nullptr; };
    auto hd = [&](int64_t c0) { return hdiag_dev ? hdiag_dev + c0 * D : nullptr; };
    return run_energy_paths(
        m, B, derivs_tile_floats,
        // two particles: k_efused (gradient: J's a and b; with the Hessian diagonal: the five-component jet), or launch by launch
        [&](int64_t c0, int64_t bc, float* ws) {
            return launch_derivs_tile(&m->mdev, m->dev, m->d_tabI4c, m->d_tabP4c, m->d_grad_fk, x_dev + c0 * D, bc, psi(c0), grad_dev + c0 * D, hd(c0), ws, stream);
        },
        // beyond two particles: k_edir's prior launch writes every direction's first and second derivative
        [&](int64_t c0, int64_t bc, float* ws) {
            return launch_derivs_dir(&m->mdev, m->dev, m->d_tabI4c, m->d_tabP4c, x_dev + c0 * D, bc, psi(c0), grad_dev + c0 * D, hd(c0), ws, stream);
        },
        // the directional wave sweep (R3) and one lane per walker behind it
        [&](int64_t c0, int64_t bc, float* ws) {
            return launch_wave_derivs(m->dev, m->d_dev, m->d_tabI4, m->d_tabP3, m->d_grad_fk, x_dev + c0 * D, bc, psi(c0), grad_dev + c0 * D, hd(c0), ws, stream);
        });
}

int64_t wf_psi_vjp_workspace_bytes(const wf_model* m, int64_t B) { return vjp_ws_bytes(m, B, true); }
int64_t wf_logpdf_vjp_workspace_bytes(const wf_model* m, int64_t B) { return vjp_ws_bytes(m, B, false); }

int wf_psi_vjp(const wf_model* m, const float* x_dev, int64_t B, const float* w_psi_dev, const float* w_lap_dev, float* grad_dev,
               void* workspace_dev, int64_t workspace_bytes, void* stream) {
    int rc = check_grad(m, x_dev, B, grad_dev, true);
    if (rc) return rc;
    if (B > 0 && (!w_psi_dev || !w_lap_dev || !workspace_dev)) return WF_ERR_INVALID;
    return run_vjp_chunks(m, 1, true, x_dev, B, w_psi_dev, w_lap_dev, nullptr, 0.0f, 0.0f, nullptr, grad_dev, workspace_dev, workspace_bytes, stream);
}

int wf_logpdf_vjp(const wf_model* m, const float* x_dev, int64_t B, const float* w_dev, float* grad_dev, void* workspace_dev,
                  int64_t workspace_bytes, void* stream) {
    int rc = check_grad(m, x_dev, B, grad_dev, false);
    if (rc) return rc;
    if (B > 0 && (!w_dev || !workspace_dev)) return WF_ERR_INVALID;
    return run_vjp_chunks(m, 0, false, x_dev, B, w_dev, nullptr, nullptr, 0.0f, 0.0f, nullptr, grad_dev, workspace_dev, workspace_bytes, stream);
}

int64_t wf_psi_jac_workspace_bytes(const wf_model* m, int64_t B) { return tape_ws_bytes(m, B, true); }
int64_t wf_logpdf_jac_workspace_bytes(const wf_model* m, int64_t B) { return tape_ws_bytes(m, B, false); }

int wf_psi_jac(const wf_model* m, const float* x_dev, int64_t B, const float* w_psi_dev, const float* w_lap_dev, float* jac_dev, void* workspace_dev,
               int64_t workspace_bytes, void* stream) {
    int rc = check_grad(m, x_dev, B, jac_dev, true);
    if (rc) return rc;
    if (B > 0 && (!w_psi_dev || !workspace_dev)) return WF_ERR_INVALID;
    return run_jac_chunks(m, 1, x_dev, B, w_psi_dev, w_lap_dev, nullptr, jac_dev, workspace_dev, workspace_bytes, stream);
}

int wf_logpdf_jac(const wf_model* m, const float* x_dev, int64_t B, float* jac_dev, float* logp_dev, void* workspace_dev, int64_t workspace_bytes,
                  void* stream) {
    int rc = check_grad(m, x_dev, B, jac_dev, false);
    if (rc) return rc;
    if (B > 0 && !workspace_dev) return WF_ERR_INVALID;
    return run_jac_chunks(m, 0, x_dev, B, nullptr, nullptr, logp_dev, jac_dev, workspace_dev, workspace_bytes, stream);
}

int wf_logpdf_loss_grad(const wf_model* m, const float* x_dev, int64_t B, float weight, float* logp_dev, float* grad_dev, void* workspace_dev,
                        int64_t workspace_bytes, void* stream) {
    int rc = check_grad(m, x_dev, B, grad_dev, false);
    if (rc) return rc;
    if (B > 0 && (!logp_dev || !workspace_dev)) return WF_ERR_INVALID;
    return run_vjp_chunks(m, 3, false, x_dev, B, nullptr, nullptr, nullptr, 0.0f, weight, logp_dev, grad_dev, workspace_dev, workspace_bytes, stream);
}

int wf_vqmc_loss_grad(const wf_model* m, const float* x_dev, int64_t B, const float* protons_host, int32_t n_protons, float running_average,
                      float inv_count, float* e_loc_dev, float* grad_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    Protons pr{};
    if (!make_protons(protons_host, n_protons, &pr)) return WF_ERR_INVALID;   // (in front of check_grad: an invalid argument is reported before an unsupported model)
    int rc = check_grad(m, x_dev, B, grad_dev, true);
    if (rc) return rc;
    if (B > 0 && (!e_loc_dev || !workspace_dev)) return WF_ERR_INVALID;
    return run_vjp_chunks(m, 2, true, x_dev, B, nullptr, nullptr, &pr, running_average, inv_count, e_loc_dev, grad_dev, workspace_dev, workspace_bytes,
                          stream);
}

int wf_rqs_fwd(const float* x_dev, const float* uw_dev, const float* uh_dev, const float* ud_dev, int64_t N, int32_t K, int32_t n_deriv,
               int32_t inverse, float left, float right, float bottom, float top, float* y_dev, float* logabsdet_dev, int32_t* bin_dev,
               void* stream) {
    if (N < 0 || K < 1 || K > 256) return WF_ERR_INVALID;
    // the staged kernel keeps a [256][K + 1] fp32 tile in LDS: 160 KiB per CU holds K <= 159.  Refused here, before any device call.
    if (K > WF_RQS_MAX_BINS) return WF_ERR_UNSUPPORTED;
    if (n_deriv != K - 1 && n_deriv != K + 1) return WF_ERR_INVALID;
    if (!(right > left) || !(top > bottom)) return WF_ERR_INVALID;
    if (1e-3f * K > 1.0f) return WF_ERR_INVALID;   // "Minimal bin width too large for the number of bins" (neural_splines.py:91-94)
    if (N > 0 && (!x_dev || !uw_dev || !uh_dev || (!ud_dev && n_deriv > 0) || !y_dev || !logabsdet_dev)) return WF_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return WF_ERR_NO_DEVICE;
    return launch_rqs(x_dev, uw_dev, uh_dev, ud_dev, N, K, n_deriv, inverse, left, right, bottom, top, y_dev, logabsdet_dev, bin_dev, stream);
}

int64_t wf_nsc_workspace_bytes(int64_t B, int32_t dim, int32_t K) {
    if (B < 0 || dim < 2 || dim > WF_MAX_DIM || (dim & 1) || K < 2 || K > 32) return WF_ERR_INVALID;
    return nsc_workspace_floats(B, dim, K) * (int64_t)sizeof(float);
}

int wf_nsc_fwd(const float* x_dev, int64_t B, int32_t dim, int32_t K, float tail_bound, int32_t hidden, const float* params_dev, int32_t inverse,
               float* y_dev, float* logdet_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
    if (B < 0 || dim < 2 || dim > WF_MAX_DIM || (dim & 1) || K < 2 || K > 32 || hidden < 1 || hidden > 64 || !(tail_bound > 0.0f)) return WF_ERR_INVALID;
    if (1e-3f * K > 1.0f) return WF_ERR_INVALID;
    if (B > 0 && (!x_dev || !params_dev || !y_dev || !logdet_dev || !workspace_dev)) return WF_ERR_INVALID;
    if (workspace_bytes < wf_nsc_workspace_bytes(B, dim, K)) return WF_ERR_INVALID;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return WF_ERR_NO_DEVICE;
    // the shapes the one-kernel stack is built for (every reference default) never touch the workspace; WF_NSC_STAGED=1 forces the
    // launch-per-half-step path (the only one for other widths / bin counts)
    if (nsc_model_built(dim, K, hidden) && !env_nsc_staged()) {
        const int dh = dim / 2, per = 3 * K - 1;
        const int64_t net_floats = (int64_t)dh * hidden + hidden + (int64_t)hidden * hidden + hidden + (int64_t)hidden * per * dh + (int64_t)per * dh;
        const NscModelDev md{dim, 1, K, hidden, WF_PRIOR_NORMAL, 0, tail_bound, 0.0f, params_dev, net_floats};
        return launch_nsc_model(md, inverse ? 3 : 2, x_dev, B, logdet_dev, y_dev, stream);
    }
    return launch_nsc(x_dev, B, dim, K, tail_bound, hidden, params_dev, inverse, y_dev, logdet_dev, (float*)workspace_dev, stream);
}

}  // extern "C"
