// wf_dmc.h -- what wf_kernels_dmc.hip (the kernels and the model-free entries of include/waveflow_dmc.h) and wf_train_dmc.cpp (init and the
// step) share: limits, workspace rules and the launchers behind the entries' argument checks.
#pragma once
#include <cstdint>

#include "../../include/waveflow_dmc.h"
#include "wf_accum.h"

namespace wf {

constexpr int64_t kDmcMaxWalkers = WF_DMC_MAX_WALKERS;
constexpr int kDmcBlock = kObsBlock;             // one lane per walker
constexpr int kDmcScanTile = 1024;               // walkers per block of the comb's scan: 256 lanes x 4, at most 1024 blocks at 2^20
constexpr int kDmcScanBlocksMax = (int)(kDmcMaxWalkers / kDmcScanTile);

inline int64_t dmc_scan_blocks(int64_t B) { return (B + kDmcScanTile - 1) / kDmcScanTile; }
// the record's block partials (wf_accum.h): 6 sums per block, no counts
inline int64_t dmc_accept_ws_bytes(int64_t B) { return partial_bytes(observe_blocks(B), WF_DMC_RECORD); }

// the comb's workspace: offsets in bytes
struct DmcCombLayout {
    int64_t bmax, bsum, prefix, src, x, psi, grad, e_loc, total;
};
inline DmcCombLayout dmc_comb_layout(int64_t B, int D) {
    DmcCombLayout l{};
    Bump b;
    l.bmax = b.take(kDmcScanBlocksMax * 8);
    l.bsum = b.take(kDmcScanBlocksMax * 8);
    l.prefix = b.take(B * 8);
    l.src = b.take(B * 4);
    l.x = b.take(B * D * 4);
    l.psi = b.take(B * 4);
    l.grad = b.take(B * D * 4);
    l.e_loc = b.take(B * 4);
    l.total = b.at;
    return l;
}

struct DmcParams {
    double tau, sqrt_tau, e_cut;
    float box;
    int limit_drift;
    unsigned long long seed, step;          // step: used where counter is null
    const unsigned long long* counter;      // the step index on the device (the captured step), or null
};

// The launches behind the entries' checks (B >= 1, D in 2 .. 8, B <= kDmcMaxWalkers, workspaces large enough).
int launch_dmc_propose(const float* x, const float* psi, const float* grad, int64_t B, int D, const DmcParams& p, float* x_new, int32_t* flag,
                       float* chi, void* stream);
// init != 0: the proposal arrays are the walkers themselves (wf_vqmc_dmc_init): every finite walker "accepts" with weight 1, a walker that is
// not finite gets weight 0, and the record holds sum w, sum w e, sum w e^2.
int launch_dmc_accept(float* x, float* psi, float* grad, float* e_loc, const float* x_new, const float* psi_new, const float* grad_new,
                      const float* hdiag_new, const int32_t* flag, int64_t B, int D, const Protons& pr, const DmcParams& p, const double* e_trial,
                      double* w, double* record, double* logA, float* u, int32_t* accepted, int init, void* ws, void* stream);
// purpose: 2 (a step's comb) or 3 (init)
int launch_dmc_reconfigure(float* x, float* psi, float* grad, float* e_loc, double* w, int64_t B, int D, const DmcParams& p, int purpose,
                           int32_t* src_out, unsigned long long* stats, unsigned long long* status, void* ws, void* stream);
// counter = 0, status = 0, ring zeroed (init)
int launch_dmc_reset(const wf_dmc_state* st, void* stream);
// E_T = record[1] / record[0] where finite (init)
int launch_dmc_trial_from_record(const double* record, double* e_trial, void* stream);
// the step's last launch: ring record, E_T, counter
int launch_dmc_finish(const wf_dmc_state* st, const double* record, int64_t B, double tau, void* stream);

// ---- wf_train_dmc.cpp: the generation, shared by wf_vqmc_dmc_step and wf_vqmc_dmc_fw_step (wf_train_dmc_observe.cpp)
// what wf_vqmc_dmc_workspace_bytes returns
int64_t dmc_step_bytes(const wf_model* m, int64_t batch);
// the refusals of wf_vqmc_dmc_step in its order, short of the workspace; fills *pr
int dmc_step_check(const wf_model* m, const wf_dmc_state* st, int64_t batch, const float* protons_host, int n_protons, double tau, double e_cut,
                   Protons* pr);
// the launches of one generation behind those checks, in a workspace of dmc_step_bytes; src_out (optional): the comb's parent indices [batch]
int dmc_step_launch(const wf_model* m, const wf_dmc_state* st, uint64_t seed, int64_t batch, const Protons& pr, double tau, int limit_drift,
                    double e_cut, int32_t* src_out, void* workspace_dev, void* stream);

}  // namespace wf
