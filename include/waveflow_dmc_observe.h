/*
 * waveflow_dmc_observe.h -- observables of a fixed-node DMC walk by forward walking, on the device: the one-body density, the pair
 * distribution and the potential energies V_en, V_ee of |Phi_0|^2 (not of psi Phi_0, which is what the walkers themselves sample).  Part of
 * libwaveflow_hip.so; conventions, error codes and WF_ABI_VERSION are those of waveflow_hip.h; buffers are caller-owned and no entry waits
 * for the host, as in waveflow_dmc.h.
 *
 * The walkers of a generation are distributed as psi Phi_0.  The number of descendants a walker has K generations later is, for large K,
 * proportional to Phi_0 / psi at that walker (Liu, Kalos, Chester 1974; Casulleras, Boronat 1995): counting an ancestor's configuration once
 * per descendant samples |Phi_0|^2.  The comb hands out the parent index src[k] of every new slot k in every generation
 * (wf_dmc_reconfigure), so the genealogy is the composition of those maps, and a TRACKER keeps it for n_slots tagged generations at once.
 *
 * THE TRACKER of B walkers of n_dim coordinates holds n_slots tag slots (1 .. 16) and n_slots + 1 accumulators: accumulator 0 is lag 0 (the
 * mixed estimator: the current walkers), accumulator j is lag j * stride generations.
 *     snap [n_slots][B][n_dim]  fp32    the walkers as they were when the slot was tagged
 *     anc  [n_slots][B]         int32   for every current walker the index into snap[s] of its ancestor at tag time
 *     tag  [n_slots]            uint64  the generation at which the slot was tagged; all ones: empty.  The caller initialises it to empty.
 * Accumulators (caller-owned, caller-zeroed; calls add to them; zeroing them in the middle of a run, after equilibration, is legal and leaves
 * the tags alone):
 *     counts  [n_slots + 1][4]                       uint64  configurations counted, skipped (a coordinate not finite), coordinates outside
 *                                                            the density range, pairs outside the pair range
 *     density [n_slots + 1][n_dim][n_density_bins]   uint64
 *     pair    [n_slots + 1][n_pair_bins]             uint64
 *     sums    [n_slots + 1][2][2]                    fp64    (V_en, V_ee) x (sum v, sum v^2) over counted configurations
 *     measurements [1]                               uint64  measurements made
 *     series  [series_len][n_slots + 1][4]           fp64    measurement number m (the value of measurements before it) is row m mod
 *                                                            series_len: per lag sum V_en, sum V_ee, configurations counted and distinct
 *                                                            ancestors of that measurement alone; zeros for a lag no slot serves
 *
 * THE UPDATE, once per generation behind the comb.  g = *generation_dev, read on the device: the number of generations done, this one
 * included.  "measuring" means g mod stride == 0.
 *   1. COMPOSE   for every non-empty slot s and every k:  anc[s][k] <- anc[s][clamp(src[k], 0, B - 1)], through the workspace, never in
 *                place.  A NULL src_dev is the identity.
 *   2. MEASURE   only when measuring.  The current x goes into accumulator 0: B configurations.  A non-empty slot s SERVES lag
 *                j = (g - tag[s]) / stride if g >= tag[s] and 1 <= j <= n_slots (anything else: the slot is not measured); its B
 *                configurations snap[s][anc[s][k]], k = 0 .. B - 1 (the composed anc), go into accumulator j: every current walker votes once
 *                for its ancestor.  Per configuration: V_en and V_ee by the fp32 rule of waveflow_observe.h (the same bits), the density and
 *                pair bins by its bin rule (scale = (float)n_bins / (hi - lo) in fp32 on the host, t = (x_d - lo) * scale and
 *                t = fabsf(x_i - x_j) * scale_pair, bin (int)t where 0 <= t < n_bins, otherwise counts[2] or counts[3]); a configuration with
 *                a coordinate that is not finite adds 1 to counts[1] and nothing else.  The fp64 sums of one lag are formed over k in the
 *                order that waveflow_observe.h states ("Reproducibility"), which depends on B alone.  No floating-point atomics; histograms
 *                and counters are integers.  Distinct ancestors of a served slot: the number of different values in anc[s], an integer; B
 *                for lag 0.  Then the series row is written and measurements += 1.
 *   3. RETAG     only when measuring, slot s* = (g / stride) mod n_slots:  snap[s*] <- x, anc[s*][k] <- k, tag[s*] <- g.  In a run that calls
 *                the update once per generation, s* is the slot that has just been measured at lag n_slots, if it was not empty.
 * Every kernel is launched in every call and decides from g on the device, so the sequence can be captured in a hipGraph with stride > 1.
 * Four launches: compose (all slots), measure (lags x walker blocks), store / retag / count the distinct ancestors (slots x walker blocks),
 * and the ordered reduction (one workgroup per lag).
 *
 * Trackers of independent populations (one per rank) can be summed by the caller: all accumulators are integers or plain sums.
 */
#ifndef WAVEFLOW_DMC_OBSERVE_H
#define WAVEFLOW_DMC_OBSERVE_H

#include "waveflow_dmc.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WF_DMC_FW_MAX_SLOTS 16
#define WF_DMC_FW_COUNTS 4            /* counted, skipped, coordinates outside the density range, pairs outside the pair range */
#define WF_DMC_FW_SERIES 4            /* sum V_en, sum V_ee, configurations counted, distinct ancestors */
#define WF_DMC_FW_EMPTY 0xFFFFFFFFFFFFFFFFull   /* the tag of an empty slot */

typedef struct wf_dmc_fw {
    float*    snap_dev;          /* [n_slots][B][n_dim] */
    int32_t*  anc_dev;           /* [n_slots][B] */
    uint64_t* tag_dev;           /* [n_slots] */
    uint64_t* counts_dev;        /* [n_slots + 1][4] */
    uint64_t* density_dev;       /* [n_slots + 1][n_dim][n_density_bins]; NULL iff n_density_bins == 0 */
    uint64_t* pair_dev;          /* [n_slots + 1][n_pair_bins]; NULL iff n_pair_bins == 0 */
    double*   sums_dev;          /* [n_slots + 1][2][2] */
    uint64_t* measurements_dev;  /* [1] */
    double*   series_dev;        /* [series_len][n_slots + 1][4] */
    int32_t   n_slots;           /* 1 .. 16 */
    int32_t   stride;            /* >= 1: generations between two measurements, and per lag */
    int32_t   series_len;        /* >= 1 */
    int32_t   n_density_bins;    /* 0 .. 512 */
    int32_t   n_pair_bins;       /* 0 .. 1024 */
    float     lo, hi;            /* density range [lo, hi), pair range [0, hi - lo); finite, lo < hi */
    int32_t   reserved;          /* 0 */
} wf_dmc_fw;                     /* 9 pointers (offsets 0 .. 64), then eight 4-byte fields (offsets 72 .. 100): 104 bytes */

/* Bytes of workspace wf_dmc_fw_update needs: the composed anc [n_slots][B] (int32), one mark byte per (slot, snapshot index), the block
 * partials [n_slots + 1][blocks][4 sums + 4 counts] (8-byte words; blocks as wf_observe_workspace_bytes) and the distinct-ancestor counts.
 * 0 for B == 0; WF_ERR_INVALID for B < 0, n_dim outside 2 .. 8 or n_slots outside 1 .. 16; WF_ERR_UNSUPPORTED for B > 2^20. */
int64_t wf_dmc_fw_workspace_bytes(int64_t B, int32_t n_dim, int32_t n_slots);

/* Model-free: the update above.  x_dev[B][n_dim]: the walkers behind the comb; src_dev[B] (int32): the comb's parent indices, or NULL for the
 * identity; protons_host: n_protons (<= 8) positions on the host; generation_dev[1]: g.  B == 0: WF_OK, nothing is touched.
 * WF_ERR_INVALID: B < 0, n_dim outside 2 .. 8, n_slots outside 1 .. 16, stride or series_len < 1, negative bin counts, lo >= hi or not finite,
 * more than 8 protons, a missing pointer (for a non-zero bin count as well), a workspace that is too small.  WF_ERR_UNSUPPORTED: B > 2^20,
 * more than 512 density bins or more than 1024 pair bins. */
int wf_dmc_fw_update(const float* x_dev, const int32_t* src_dev, int64_t B, int32_t n_dim, const float* protons_host, int32_t n_protons,
                     const wf_dmc_fw* fw, const uint64_t* generation_dev, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* Bytes of workspace wf_vqmc_dmc_fw_step needs: what wf_vqmc_dmc_workspace_bytes gives, then the comb's src and the update's workspace.
 * Refusals as wf_vqmc_dmc_workspace_bytes; WF_ERR_INVALID also for n_slots outside 1 .. 16. */
int64_t wf_vqmc_dmc_fw_workspace_bytes(const wf_model* m, int64_t batch, int32_t n_slots);

/* One generation with its measurement, as one sequence of launches on `stream`: no host work, no wait, nothing allocated -- capturable in a
 * hipGraph.  It is the sequence of wf_vqmc_dmc_step (the same code; the DMC state it leaves is bit for bit the state that entry leaves) with
 * the comb's src kept in the workspace, and behind its last launch wf_dmc_fw_update(st->x_dev, src, ..., generation_dev = st->counter_dev).
 * Coverage and refusals as wf_vqmc_dmc_step and wf_dmc_fw_update. */
int wf_vqmc_dmc_fw_step(const wf_model* m, const wf_dmc_state* st, const wf_dmc_fw* fw, uint64_t seed, int64_t batch,
                        const float* protons_host, int32_t n_protons, double tau, int32_t limit_drift, double e_cut, void* workspace_dev,
                        int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_DMC_OBSERVE_H */
