// wf_observe.h -- what wf_kernels_observe.hip (the accumulation kernels, wf_observe_accumulate) and wf_train_observe.cpp (the measurement step)
// share: the grid rule, the argument check of an accumulator and the launcher behind both entries.
#pragma once
#include <cstdint>

#include "../../include/waveflow_observe.h"
#include "wf_internal.h"

namespace wf {

constexpr int kObsBlock = 256;            // one lane per walker
constexpr int64_t kObsMaxBlocks = 1024;   // the grid-stride loop takes the rest: the block partials stay within 112 KB
constexpr int kObsPartial = 14;           // 8-byte words per block partial: 10 sums, 4 counts
constexpr int kObsMaxDensityBins = 512, kObsMaxPairBins = 1024;
constexpr int64_t kObsMaxWalkers = (int64_t)1 << 36;   // per call: a block then sees at most 2^26 walkers of 28 pairs, which a uint32 LDS bin holds

// blocks of the accumulation launch: a function of B alone
inline int64_t observe_blocks(int64_t B) { return B < 1 ? 0 : (B + kObsBlock - 1) / kObsBlock < kObsMaxBlocks ? (B + kObsBlock - 1) / kObsBlock : kObsMaxBlocks; }
inline int64_t observe_ws_bytes(int64_t B) { return (observe_blocks(B) * kObsPartial * 8 + 255) / 256 * 256; }

// WF_OK, or what wf_observe_accumulate returns for this accumulator (acc != nullptr)
int observe_check_acc(const wf_observe_acc* acc);

// The launches of wf_observe_accumulate behind its checks (B >= 1; acc or values given; ws holds observe_ws_bytes(B) when acc is given).
// counter, if given, is advanced by one behind them (the measurement step's last act, in the launch that adds the block partials).
int launch_observe(const float* x, const float* psi, const float* grad, const float* hdiag, int64_t B, int D, const Protons& pr,
                   const wf_observe_acc* acc, float* values, void* ws, unsigned long long* counter, void* stream);

}  // namespace wf
