// wf_observe.h -- what wf_kernels_observe.hip (the accumulation kernels, wf_observe_accumulate) and wf_train_observe.cpp (the measurement step)
// share: the words of a block partial (the grid rule and the order of the sums: wf_accum.h), the argument check of an accumulator, the
// launcher behind both entries, and the batch sizes a measurement step draws walkers for (wf_train_overlap.cpp asks too).
#pragma once
#include <cstdint>

#include "../../include/waveflow_observe.h"
#include "wf_accum.h"

namespace wf {

constexpr int kObsSums = 10, kObsCounts = 4;
constexpr int kObsPartial = kObsSums + kObsCounts;   // 8-byte words per block partial
constexpr int64_t kObsMaxWalkers = (int64_t)1 << 36;   // per call: a block then sees at most 2^26 walkers of 28 pairs, which a uint32 LDS bin holds

inline int64_t observe_ws_bytes(int64_t B) { return partial_bytes(observe_blocks(B), kObsPartial); }

// WF_OK, or what wf_observe_accumulate returns for this accumulator (acc != nullptr)
int observe_check_acc(const wf_observe_acc* acc);

// The launches of wf_observe_accumulate behind its checks (B >= 1; acc or values given; ws holds observe_ws_bytes(B) when acc is given).
// counter, if given, is advanced by one behind them (the measurement step's last act, in the launch that adds the block partials).
int launch_observe(const float* x, const float* psi, const float* grad, const float* hdiag, int64_t B, int D, const Protons& pr,
                   const wf_observe_acc* acc, float* values, void* ws, unsigned long long* counter, void* stream);

// A sampler for B walkers, as a training step has one: the staged sampler where it applies (step_sampler_bytes is non-zero exactly there),
// the wave sampler up to its limit.  current: at call time the staged sampler also needs fresh tables, as sample_step_walkers decides.
bool measure_batch_covered(const wf_model* m, int64_t B, bool current);

}  // namespace wf
