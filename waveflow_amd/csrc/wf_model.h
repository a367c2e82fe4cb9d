// wf_model.h -- private header of the host units (wf_runtime.cpp, wf_model_build.cpp, wf_model_images.cpp, wf_dispatch.cpp, wf_train.cpp, wf_train_sr.cpp):
// struct wf_model and the few helpers those units share.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "wf_internal.h"
#include "wf_layout.h"

#define WF_HIP(call)                                   \
    do {                                               \
        hipError_t e_ = (call);                        \
        if (e_ != hipSuccess) {                        \
            wf::set_hip_error((int)e_);                \
            return WF_ERR_HIP;                         \
        }                                              \
    } while (0)

namespace wf {

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

struct NetLayout {
    int n_out;       // bases per dimension (IMADE/prior) or 2 (MADE)
    bool has_zero;   // trailing zero_params[D][n_out] leaf (model_factory.py:84-87)
    int64_t offset;  // offset of W0 in the flat parameter vector
    int64_t count;
};

}  // namespace wf

struct wf_model {
    wf_model_desc desc{};
    int device = 0;
    int kernel_kind = WF_KERNEL_AUTO;
    int i_nb = 0, p_nb = 0;
    int nbp = 32;
    std::vector<wf::NetLayout> nets;  // flow layers then (optionally) the prior net
    int64_t n_params = 0;
    bool params_set = false;
    // a deferred training step (wf_train_state.defer_eval_tables) refreshed the weight images only: the MFMA image then holds unfolded
    // biases and the composite dimension-0 tables are those of older parameters.  Cleared by the next full refresh; while it is set,
    // wf_hamiltonian_fwd stays on the wave sweeps (which read neither) -- include/waveflow_hip.h promises it needs no refresh.
    bool eval_tables_stale = false;
    // fp16 range of the matrix-core operand images: k_fold_bias leaves one flag per net in d_f16_ovf at every upload; the host copy arrives through
    // pinned memory behind ovf_event (f16_overflow() below waits for it when an entry point needs the answer before the upload has finished).
    int* d_f16_ovf = nullptr;
    int* h_f16_ovf = nullptr;
    hipEvent_t ovf_event = nullptr;
    bool ovf_pending = false;
    bool f16_overflow = false;
    bool local_step_tile = false;    // the last wf_vqmc_train_step_local ran at a batch size of the matrix-core sampler / gradient: _apply refreshes every table
    wf::ModelDev dev{};
    std::vector<void*> allocs;
    // device images
    float* d_plain = nullptr;  // all NetPlain arrays, one allocation
    int64_t plain_floats = 0;
    std::vector<int64_t> plain_off;  // per net: offset of W0 in d_plain
    float* d_mfma = nullptr;
    int64_t mfma_floats = 0;
    wf::ModelDev* d_dev = nullptr;  // device copy of `dev`
    bool mfma_ok = false;           // the MFMA kernel covers this configuration
    wf::MfmaDev mdev{};
    wf::MfmaDev* d_mdev = nullptr;
    std::vector<float> mfma_consts;  // constants block of the LDS image (host copy)
    int64_t mfma_lds_floats = 0;
    float* d_tabI = nullptr;
    float* d_tabP = nullptr;
    float* d_fk_nat = nullptr;       // [2][32] natural-order row factors (I layers, prior) for k_prepare_dim0
    void* d_comp = nullptr;          // composite tables [n_nets][n_mesh] float4
    const float* d_tabI4 = nullptr;  // [4][n_mesh][nbp]: I-spline derivative orders 0..3 (local energy)
    const float* d_tabP3 = nullptr;  // [4][n_mesh][nbp]: orthogonal-B derivative orders 0..3 (the energy uses 0..2)
    const float* d_tabB0 = nullptr;  // [n_mesh][nbp]: the PLAIN B-splines (order 0): the staged sampler's band-limited evaluation of a proposal
    // the same two tables regrouped for the lane-per-walker heads of wf_kernels_etile.hip (nbp == 32 only): [n_mesh][8 row chunks][4 orders][4 rows],
    // so that the four orders of four rows of one mesh point are one 64-byte segment
    const float* d_tabI4c = nullptr;
    const float* d_tabP4c = nullptr;
    float* d_flat = nullptr;         // staging copy of a host parameter vector (wf_model_set_params)
    wf::PackRec* d_pack = nullptr;   // descriptions of every entry of the plain, wave and mfma images
    int64_t n_pack = 0;
    float* d_scratch = nullptr;      // private scratch of wf_hamiltonian_fwd (grown on demand)
    int64_t scratch_floats = 0;
    float* d_wave = nullptr;         // NetWave images
    float* d_grad_fk = nullptr;      // [2][64] natural-order row factors for the reverse pass (flow rows, prior rows)
    float* d_egacc = nullptr;        // [n_nets][6400] gradient blocks of the matrix-core gradient path, accumulated over the chunks of a batch
    bool wave_ok = false;            // the wave-cooperative sweeps and sampler cover this model (homogeneous constraints, gated heads included)
    // boundary conditions as a linear map on the coefficient vector (bc_map below): column sums a~ of A, per spline (I layers / prior);
    // bc_*_ok: homogeneous (no constant term) and every column with a~_j == 0 is entirely zero -> the table-driven kernels apply
    bool is_nsc = false;             // layer_kind WF_LAYER_NSC: the coupling stack (k_nsc_model), none of the conditioner-net machinery
    float* d_nsc = nullptr;          // its parameters on the device (the model's own copy)
    wf::NscModelDev nsc{};
    std::vector<double> bc_i_colsum, bc_p_colsum;
    std::vector<float> p_cb;          // constant term of the B prior's boundary map times ob_to_b, natural order [nbp] (empty: homogeneous constraints)
    bool bc_i_ok = true, bc_p_ok = true;
    bool bc_i_plain = false;   // I layers: the same of their boundary map (the rows of the evaluation table are then the plain I-splines: exactly 1 left of a band of k + 1, 0 right of it)
    bool bc_p_plain = false;   // B prior: the boundary map only zeroes coefficients (a masked identity, no constant term): (o keep) ARE the plain B-spline coefficients of c
    bool grad_psi_ok = false;        // wf_psi_vjp (Waveflow prior, IMADE layers)
    int ring2 = 2;                   // coefficient ring of the second-order sweeps (ring_coefs, wf_internal.h): 2 = RF, 1 = R3
    int32_t* d_grad_map = nullptr;   // [n_params]: forward-image entry (over all nets) that holds each parameter, -1 = none
    float* d_grad_partial = nullptr; // per-split partial gradient images of k_wgrad
    float* d_grad_img = nullptr;     // [n_nets * fwd image floats]: gradient accumulator in forward-image layout
    // gated heads: gradient of the zero_params leaves (rows = n_nets * passes * 64 head lanes of the wave layout)
    int z_rows = 0;
    float* d_zpart = nullptr;        // [64 splits][z_rows]
    float* d_zgrad = nullptr;        // [z_rows]
    int32_t* d_zmap = nullptr;       // row -> index of its leaf entry in the flat vector (-1: padding lane / ungated net)
    int32_t* d_zraw_off = nullptr;   // row -> offset of the raw leaf value in the plain image for |z| heads (-1: signed head)
    int32_t* d_zinv = nullptr;       // [n_params]: the inverse of d_zmap, -1 for every parameter that is no zero_params entry of a gated head (k_wjac)
};

namespace wf {

struct NetOffsets {   // flat-vector offsets of the leaves of one conditioner (model_factory.py:72-87 leaf order)
    int64_t W0, b0, W1, b1, W2, b2;
    int NO;
};

constexpr int64_t kWaveEvalMax = 6144;   // measured crossover ~7000 walkers (scratch/crossover.py)
constexpr int64_t kTileSampleChunk = 1 << 18;   // walkers per pass of a call without a caller's workspace (the model's scratch: 111 MB)

// ---- wf_runtime.cpp
int dev_alloc_bytes(wf_model* m, void** p, size_t bytes);   // device memory owned by the model (freed by wf_model_destroy)
template <class T>
inline int dev_alloc(wf_model* m, T** p, size_t count) {
    void* q = nullptr;
    int rc = dev_alloc_bytes(m, &q, std::max<size_t>(count, 1) * sizeof(T));
    if (rc) return rc;
    *p = (T*)q;
    return WF_OK;
}
int ensure_scratch(const wf_model* cm, int64_t floats);

// ---- wf_model_images.cpp: sizes and descriptions of the device weight images
int64_t plain_fwd_floats(int D, int nbp);
int64_t plain_net_floats(int D, int nbp);
int64_t wave_net_floats(int D, int nbp);
inline int wave_passes(int D, int nbp) { return nbp == 32 ? (D + 1) / 2 : D; }   // output passes: 2 dimensions x 32 rows, or 1 x 64
NetOffsets net_offsets(const wf_model* m, int n);
bool net_has_sigmoid_head(const wf_model* m, int n);
bool net_is_gated(const wf_model* m, int n);
void row_factors(int kind, bool with_remove_bias, int k, int nb, int nbk, const std::vector<double>& bc_colsum, float* out_acc, float* natural64 = nullptr);
int mfma_prepare(wf_model* m, const std::vector<double>& i64, const std::vector<double>& p64, const std::vector<double>& o2b);
int pack_prepare(wf_model* m, std::vector<PackRec>& plain);

// ---- wf_model_build.cpp
int upload_table(wf_model* m, const std::vector<float>& h, const float** out);
int apply_params(wf_model* m, const float* flat_dev, void* stream, bool eval_tables = true);
bool f16_overflow(const wf_model* cm);

// ---- wf_dispatch.cpp: path predicates and chunk loops the training steps share with the entry points
bool grad_supported(const wf_model* m, bool second_order);
int check_energy_model(const wf_model* m);
bool step_reads_eval_tables(const wf_model* m, int64_t B);
bool vqmc_step_covered(const wf_model* m, int64_t B, bool current);
int sample_step_walkers(const wf_model* m, uint64_t seed, const unsigned long long* counter_dev, int64_t B, float* x_dev, int exact, void* scratch,
                        int64_t scratch_bytes, void* stream);
int64_t step_sampler_bytes(const wf_model* m, int64_t B);
int64_t vjp_ws_bytes(const wf_model* m, int64_t B, bool second_order);
int run_vjp_chunks(const wf_model* m, int mode, bool second_order, const float* x_dev, int64_t B, const float* w1, const float* w2,
                   const Protons* pr, float running_average, float inv_count, float* e_loc_dev, float* grad_dev, void* workspace_dev,
                   int64_t workspace_bytes, void* stream, const float* running_average_dev = nullptr, int* defer_gather_split = nullptr);

}  // namespace wf
