// wf_env.h -- every environment switch of libwaveflow_hip: the one place in csrc/ that reads the environment (host only, no HIP).
//
// One accessor per knob, its default and its parse rule beside it.  Nothing is cached: an accessor reads the environment whenever it is
// called, and the callers decide when that is -- "per call" knobs are read inside the entry point or launcher of every call (the tests flip
// them between two calls on one model), "at model creation" knobs inside wf_model_create only.  README.md ("Environment switches") lists the
// same names; tests/test_abi_host.py compares the two lists.
#pragma once
#include <cstdint>
#include <cstdlib>

namespace wf {

inline const char* env_raw(const char* name) { return std::getenv(name); }
// "set at all": any value counts, NAME=0 and the empty string included
inline bool env_set(const char* name) { return env_raw(name) != nullptr; }
// atoll of the value (0 for text that is no number), the compiled default when unset
inline int64_t env_i64(const char* name, int64_t dflt) {
    const char* e = env_raw(name);
    return e ? atoll(e) : dflt;
}
// atoi of the value, `unset` when unset
inline int env_int(const char* name, int unset) {
    const char* e = env_raw(name);
    return e ? atoi(e) : unset;
}

// ---- switch points between kernel paths (per call; 0 = never the tile path, for the three *_TILE_MIN)
constexpr int64_t kGradTileMin = 16384;    // psi / Laplacian gradients: the matrix-core path (k_efused, k_ebwd) from here on
constexpr int64_t kEnergyTileMin = 16384;  // H psi: the tile path (8 launches, staged weight images) from here on
constexpr int64_t kEnergyTileChunk = (int64_t)1 << 19;   // walkers per pass of the tile path (WF_ENERGY_TILE_CHUNK; 2^20 walkers: 1.20 ms in two passes, 1.30 in one, 1.34 in four)
constexpr int64_t kTileSampleMin = 16384;  // wf_sample / wf_inverse_fwd: the staged sampler of wf_kernels_etile_sample.hip from here on
// Inverse / sampler.  One wave per walker (wf_kernels_wave.hip: 64-way mesh search instead of the halving loop, 64 rejection
// proposals per round) finishes 128 walkers in 29 us where one lane per walker (wf_kernels_scalar.hip, the reference-order
// loops) needs 1.4 ms, and stays ahead up to ~2^18 walkers (65536: 1.1 vs 1.9 ms; 2^18: 4.4 vs 4.2-4.6 ms; 2^20: 17.3 vs
// 15.9-17.3 ms, scratch/sampler_crossover.py): the switch sits at 2^17.
constexpr int64_t kWaveSampleMax = 131072;
// k_mfma, headline family: 8 waves x 2 paired tiles (own-walker layout, wf_mfma_impl.h) from here on, 16 waves x 1 tile below.  At 2^16 walkers
// and fewer the two-tile shape fills half the CUs, and at 2^18 (two pairs per wave) it is still 8 % behind (profiles/mfma_paired_crossover.txt).
constexpr int64_t kMfmaPairMin = 524288;
inline int64_t env_energy_tile_min() { return env_i64("WF_ENERGY_TILE_MIN", kEnergyTileMin); }
inline int64_t env_energy_tile_chunk() { return env_i64("WF_ENERGY_TILE_CHUNK", kEnergyTileChunk); }   // (the caller clamps it to >= 1024)
inline int64_t env_sample_tile_min() { return env_i64("WF_SAMPLE_TILE_MIN", kTileSampleMin); }
inline int64_t env_grad_tile_min() { return env_i64("WF_GRAD_TILE_MIN", kGradTileMin); }
inline int64_t env_wave_sample_max() { return env_i64("WF_WAVE_SAMPLE_MAX", kWaveSampleMax); }

// ---- A/B switches, per call ("set at all" unless said otherwise)
inline bool env_energy_r3() { return env_set("WF_ENERGY_R3"); }   // H psi in R3 (the wave sweeps; it also keeps the call off the tile paths)
// WF_ENERGY_FUSED=0 (a value that parses to 0) switches the one-kernel form of the two-particle H psi off; unset or anything else: on
inline bool env_energy_fused() {
    const char* e = env_raw("WF_ENERGY_FUSED");
    return !(e && atoi(e) == 0);
}
inline bool env_nsc_staged() { return env_set("WF_NSC_STAGED"); }
inline bool env_sample_dense_envelope() { return env_set("WF_SAMPLE_DENSE_ENVELOPE"); }
inline bool env_sample_full_rows() { return env_set("WF_SAMPLE_FULL_ROWS"); }
inline bool env_sample_one_lane() { return env_set("WF_SAMPLE_ONE_LANE"); }
inline bool env_sample_group_phase2() { return env_set("WF_SAMPLE_GROUP_PHASE2"); }
// workgroup shape of k_mfma (at every launch): the value as a number, 0 when unset; the launcher accepts the shapes it was built with
inline int env_mfma_waves() { return env_int("WF_MFMA_WAVES", 0); }
inline int env_mfma_tiles() { return env_int("WF_MFMA_TILES", 0); }
// per call by the energy sweep, at model creation for the gradients (second_order_rf, wf_internal.h)
inline bool env_wide_rf() { return env_set("WF_WIDE_RF"); }

// ---- at model creation
inline bool env_grad_r3() { return env_set("WF_GRAD_R3"); }
inline bool env_mfma_no_band() { return env_set("WF_MFMA_NO_BAND"); }
inline bool env_prior_quotient() { return env_int("WF_PRIOR_QUOTIENT", 0) != 0; }   // a value that parses to non-zero

// ---- at every device allocation of a model
inline bool env_poison() { return env_set("WF_POISON"); }

}  // namespace wf
