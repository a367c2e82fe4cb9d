// wf_dmc_observe.h -- what wf_kernels_dmc_observe.hip (the forward-walking kernels and the model-free entries of
// include/waveflow_dmc_observe.h) and wf_train_dmc_observe.cpp (the generation with its measurement) share: the workspace rule, the argument
// check of a tracker and the launcher behind both entries.
#pragma once
#include <cstdint>

#include "../../include/waveflow_dmc_observe.h"
#include "wf_dmc.h"

namespace wf {

constexpr int kFwSums = 4, kFwCounts = 4;        // sum and sum of squares of V_en and of V_ee; the 4 counts of wf_observe_accumulate
constexpr int kFwPartial = kFwSums + kFwCounts;  // 8-byte words per block partial (wf_accum.h)

// the update's workspace: offsets in bytes
struct DmcFwLayout {
    int64_t anc, mark, partials, distinct, total;
};
inline DmcFwLayout dmc_fw_layout(int64_t B, int n_slots) {
    DmcFwLayout l{};
    Bump b;
    l.anc = b.take((int64_t)n_slots * B * 4);
    l.mark = b.take((int64_t)n_slots * B);
    l.partials = b.take(partial_bytes((int64_t)(n_slots + 1) * observe_blocks(B), kFwPartial));
    l.distinct = b.take((WF_DMC_FW_MAX_SLOTS + 1) * 8);   // per slot, then the measurement number of the call
    l.total = b.at;
    return l;
}

// WF_OK, or what wf_dmc_fw_update returns for this tracker (fw may be null: WF_ERR_INVALID)
int dmc_fw_check(const wf_dmc_fw* fw);

// The four launches of wf_dmc_fw_update behind its checks (B in 1 .. kDmcMaxWalkers, D in 2 .. 8, ws holds dmc_fw_layout(B, n_slots).total).
int launch_dmc_fw_update(const float* x, const int32_t* src, int64_t B, int D, const Protons& pr, const wf_dmc_fw* fw,
                         const unsigned long long* generation, void* ws, void* stream);

}  // namespace wf
