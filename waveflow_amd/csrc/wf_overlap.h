// wf_overlap.h -- what wf_kernels_overlap.hip (the ratio, moment and penalty kernels, wf_overlap_accumulate, wf_overlap_penalise) and
// wf_train_overlap.cpp (the measurement step) share: the words of a block partial (the grid rule and the order of the sums: wf_accum.h), the
// argument check of an accumulator and the launcher behind both entries.
#pragma once
#include <cstdint>

#include "../../include/waveflow_overlap.h"
#include "wf_observe.h"

namespace wf {

// 8-byte words per block partial: 2 K sums, 2 counts
constexpr int overlap_partial_words(int K) { return 2 * K + 2; }
// the block partials of observe_blocks(B) blocks
inline int64_t overlap_ws_bytes(int64_t B, int K) { return partial_bytes(observe_blocks(B), overlap_partial_words(K)); }

// WF_OK, or what wf_overlap_accumulate returns for this accumulator (acc != nullptr)
inline int overlap_check_acc(const wf_overlap_acc* acc) { return acc->sums_dev && acc->counts_dev ? WF_OK : WF_ERR_INVALID; }

// The launches of wf_overlap_accumulate behind its checks (B >= 1, 1 <= K <= 8, ld >= B; acc or ratios given; ws holds overlap_ws_bytes(B, K)
// when acc is given).  counter, if given, is advanced by one behind them (the measurement step's last act, in the launch that adds the block
// partials).
int launch_overlap(const float* psi, const float* ref, int64_t ld, int64_t B, int K, const wf_overlap_acc* acc, float* ratios, void* ws,
                   unsigned long long* counter, void* stream);

}  // namespace wf
