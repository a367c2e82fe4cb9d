// wf_model_images.cpp -- the device weight images of a model: their sizes, their descriptions as PackRec lists (plain, wave, MFMA operand
// order) and the parameter-independent parts of the MFMA image (mfma_prepare).
//
// Reference behaviour mirrored here (paths relative to /root/reference/waveflow):
//   masks / MaskedDense / tiling ........ model_factory.py:8-35, 72-82
//   parameter pytree order .............. wavefunctions.py:110, distributions.py:192, made.py:38,102
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "wf_model.h"

namespace wf {

// get_masks, model_factory.py:8-19
static inline int deg_in(int a) { return a; }
static inline int deg_hidden(int a, int D) { return a % (D - 1); }
static inline int deg_out(int d) { return d - 1; }

// forward-orientation part of a net's image (W0, b0, W1t, b1, W2t, b2): also the layout of the gradient accumulator
int64_t plain_fwd_floats(int D, int nbp) {
    return (int64_t)D * kHidden + kHidden + (int64_t)kHidden * kHidden + kHidden + (int64_t)D * nbp * kHidden + (int64_t)D * nbp;
}
// ... followed by W1n, W2n, zero
int64_t plain_net_floats(int D, int nbp) {
    return plain_fwd_floats(D, nbp) + (int64_t)kHidden * kHidden + (int64_t)kHidden * D * nbp + 2 * (int64_t)D * nbp;   // ..., zero, zero_raw
}

// Every entry of a device weight image is scale * flat[src] (or a constant): the images are described once per model as
// PackRec lists and filled on the device by k_pack (wf_kernels_grad.hip) whenever the parameters change.
struct ImageWriter {
    std::vector<PackRec>& out;
    uint32_t o;   // running float offset inside the image
    void f32(int64_t src, double scale = 1.0) { out.push_back(PackRec{(int32_t)src, 0, o++, 0u, src >= 0 ? scale : 0.0}); }
    void f32_abs(int64_t src) { out.push_back(PackRec{(int32_t)src, 0x10, o++, 0u, src >= 0 ? 1.0 : 0.0}); }
    void cst(double value) { out.push_back(PackRec{-1, 0, o++, 0u, value}); }
};

NetOffsets net_offsets(const wf_model* m, int n) {
    const int D = m->desc.n_dim, H = kHidden;
    const NetLayout& nl = m->nets[n];
    NetOffsets q;
    q.NO = nl.n_out * D;
    q.W0 = nl.offset;
    q.b0 = q.W0 + (int64_t)D * H;
    q.W1 = q.b0 + H;
    q.b1 = q.W1 + (int64_t)H * H;
    q.W2 = q.b1 + H;
    q.b2 = q.W2 + (int64_t)H * q.NO;
    return q;
}

bool net_is_gated(const wf_model* m, int n) { return n == m->desc.n_flow_layers ? m->desc.p_gate != 0 : m->desc.i_gate != 0; }

// Masked, transposed weight image of net n (NetPlain), float offset `base` inside d_plain.
static void describe_plain_image(const wf_model* m, int n, uint32_t base, std::vector<PackRec>& out) {
    const int D = m->desc.n_dim, H = kHidden, nbp = m->nbp;
    const NetLayout& nl = m->nets[n];
    const NetOffsets q = net_offsets(m, n);
    ImageWriter w{out, base};
    // W0 * mask0: [D][H]
    for (int a = 0; a < D; ++a)
        for (int j = 0; j < H; ++j) w.f32(deg_hidden(j, D) >= deg_in(a) ? q.W0 + (int64_t)a * H + j : -1);
    for (int j = 0; j < H; ++j) w.f32(q.b0 + j);
    // (W1 * mask1)^T: [j out][a in]
    for (int j = 0; j < H; ++j)
        for (int a = 0; a < H; ++a) w.f32(deg_hidden(j, D) >= deg_hidden(a, D) ? q.W1 + (int64_t)a * H + j : -1);
    for (int j = 0; j < H; ++j) w.f32(q.b1 + j);
    // (W2 * tile(mask2))^T regrouped: [d][jb][a], reference output column c = jb*D + d (model_factory.py:59-60,81)
    for (int dd = 0; dd < D; ++dd)
        for (int jb = 0; jb < nbp; ++jb)
            for (int a = 0; a < H; ++a)
                w.f32((jb < nl.n_out && deg_out(dd) >= deg_hidden(a, D)) ? q.W2 + (int64_t)a * q.NO + (jb * D + dd) : -1);
    for (int dd = 0; dd < D; ++dd)
        for (int jb = 0; jb < nbp; ++jb) w.f32(jb < nl.n_out ? q.b2 + jb * D + dd : -1);
    // reverse-pass orientation: W1 * mask1 [a in][j out], W2 * mask2 [a in][d][jb]
    for (int a = 0; a < H; ++a)
        for (int j = 0; j < H; ++j) w.f32(deg_hidden(j, D) >= deg_hidden(a, D) ? q.W1 + (int64_t)a * H + j : -1);
    for (int a = 0; a < H; ++a)
        for (int dd = 0; dd < D; ++dd)
            for (int jb = 0; jb < nbp; ++jb)
                w.f32((jb < nl.n_out && deg_out(dd) >= deg_hidden(a, D)) ? q.W2 + (int64_t)a * q.NO + (jb * D + dd) : -1);
    // zero_params[d][j] of a gated head (the leaf follows b2; model_factory.py:84), |z| under a sigmoid head (:62-63); zeros otherwise
    const bool gated = nl.has_zero && net_is_gated(m, n), sig = net_has_sigmoid_head(m, n);
    for (int dd = 0; dd < D; ++dd)
        for (int jb = 0; jb < nbp; ++jb) {
            const int64_t src = (gated && jb < nl.n_out) ? q.b2 + q.NO + (int64_t)dd * nl.n_out + jb : -1;
            if (sig) w.f32_abs(src);
            else w.f32(src);
        }
    for (int dd = 0; dd < D; ++dd)   // the same leaf without the |.| (zero_raw)
        for (int jb = 0; jb < nbp; ++jb) w.f32((gated && jb < nl.n_out) ? q.b2 + q.NO + (int64_t)dd * nl.n_out + jb : -1);
}

// Wave-kernel image of net n (NetWave): W0 [D][64], b0, b1, b2 [P][64], W1f, W1b [16][64][4], W2f, W2b [P][16][64][4]
int64_t wave_net_floats(int D, int nbp) {
    const int P = wave_passes(D, nbp);
    return (int64_t)D * kHidden + 2 * kHidden + (int64_t)P * 64 + 2 * 4096 + (int64_t)P * 2 * 4096 + (int64_t)P * 64;   // ..., z
}

static void describe_wave_image(const wf_model* m, int n, uint32_t base, std::vector<PackRec>& out) {
    const int D = m->desc.n_dim, H = kHidden, P = wave_passes(D, m->nbp);
    const bool wide = m->nbp == 64;
    const NetLayout& nl = m->nets[n];
    const NetOffsets q = net_offsets(m, n);
    auto w1m = [&](int a, int j) -> int64_t { return deg_hidden(j, D) >= deg_hidden(a, D) ? q.W1 + (int64_t)a * H + j : -1; };
    // column of output lane c of pass p: (d, jb) = (2p + (c >> 5), c & 31), or (p, c) in the 64-row layout
    auto w2m = [&](int a, int p, int c) -> int64_t {
        const int d = wide ? p : 2 * p + (c >> 5), jb = wide ? c : (c & 31);
        if (d >= D || jb >= nl.n_out || deg_out(d) < deg_hidden(a, D)) return -1;
        return q.W2 + (int64_t)a * q.NO + (jb * D + d);
    };
    ImageWriter w{out, base};
    for (int a = 0; a < D; ++a)
        for (int j = 0; j < H; ++j) w.f32(deg_hidden(j, D) >= deg_in(a) ? q.W0 + (int64_t)a * H + j : -1);
    for (int j = 0; j < H; ++j) w.f32(q.b0 + j);
    for (int j = 0; j < H; ++j) w.f32(q.b1 + j);
    for (int p = 0; p < P; ++p)
        for (int c = 0; c < 64; ++c) {
            const int d = wide ? p : 2 * p + (c >> 5), jb = wide ? c : (c & 31);
            w.f32((d < D && jb < nl.n_out) ? q.b2 + jb * D + d : -1);
        }
    for (int g = 0; g < 16; ++g)
        for (int j = 0; j < 64; ++j)
            for (int e = 0; e < 4; ++e) w.f32(w1m(4 * g + e, j));
    for (int g = 0; g < 16; ++g)
        for (int a = 0; a < 64; ++a)
            for (int e = 0; e < 4; ++e) w.f32(w1m(a, 4 * g + e));
    for (int p = 0; p < P; ++p)
        for (int g = 0; g < 16; ++g)
            for (int c = 0; c < 64; ++c)
                for (int e = 0; e < 4; ++e) w.f32(w2m(4 * g + e, p, c));
    for (int p = 0; p < P; ++p)
        for (int g = 0; g < 16; ++g)
            for (int a = 0; a < 64; ++a)
                for (int e = 0; e < 4; ++e) w.f32(w2m(a, p, 4 * g + e));
    // zero_params of a gated head in the lane order of b2 (|z| under a sigmoid head); zeros otherwise
    const bool gated = nl.has_zero && net_is_gated(m, n), sig = net_has_sigmoid_head(m, n);
    for (int p = 0; p < P; ++p)
        for (int c = 0; c < 64; ++c) {
            const int d = wide ? p : 2 * p + (c >> 5), jb = wide ? c : (c & 31);
            const int64_t src = (gated && d < D && jb < nl.n_out) ? q.b2 + q.NO + (int64_t)d * nl.n_out + jb : -1;
            if (sig) w.f32_abs(src);
            else w.f32(src);
        }
}

// ---------------------------------------------------------------------------- MFMA kernel images
static inline int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

static int mfma_net_floats(int D, int nbk) {
    const int S0 = (D + 1) / 2;
    return 128 * S0 + 64 + 4096 + 64 + (D - 1) * nbk * 2048 + 32 * D * nbk + 32 * D * nbk + 64;   // ..., biases, zero_params, reserved tail (NetOff::reserved)
}

// per-row factor: remove_bias scaling (isplines_jax.py:196-202 / msplines_jax.py:186-192) times the
// 0/1 "kept by the boundary conditions" mask; 0 beyond the real bases.  Layout [half][16] in accumulator order.
void row_factors(int kind, bool with_remove_bias, int k, int nb, int nbk, const std::vector<double>& bc_colsum, float* out_acc,
                 float* natural64) {
    std::vector<float> f(64, 0.0f);
    for (int j = 0; j < nb; ++j) f[j] = 1.0f;
    if (with_remove_bias)
        for (int i = 0; i < k; ++i) {
            const int a = kind == WF_SPLINE_I ? i + 1 : i;
            const int b = kind == WF_SPLINE_I ? nb - (i + 2) : nb - (i + 1);
            const float fac = (float)(i + 1) / (float)k;
            f[a] *= fac;
            f[b] *= fac;
        }
    for (int j = 0; j < nb; ++j) f[j] = (float)((double)f[j] * bc_colsum[j]);   // a~ of bc_map: 0 / 1 for zero-only constraints
    for (int kb = 0; kb < nbk; ++kb)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) out_acc[(kb * 2 + h) * 16 + r] = f[32 * kb + acc_row(r, h)];
    if (natural64)
        for (int j = 0; j < 64; ++j) natural64[j] = f[j];
}

// Spline table of the MFMA kernel: [n_mesh][8 * nbk pieces][n_orders][2 sides][4 rows].  Piece p = natural rows 4p .. 4p+3 (a lane of
// walker half h holds the pieces 8 kb + 2q + h, q = 0..3, of every 32-row block in its accumulator registers); side 0 = mesh point m,
// side 1 = mesh point min(m + 1, n_mesh - 1): the two ends of the reference's lerp (isplines_jax.py:45-56) and both derivative orders of
// a piece are one 64-byte record (32 bytes for the one-order prior table), so a lane's four records are all it reads for a spline
// evaluation.  Rows scaled by fk (acc layout [kb][h][16], may be null); rowsum (may be null): [n_mesh][n_orders].
static void pack_rows_pairs(const std::vector<double>& t64, int nb, int n_mesh, int n_orders, int nbk, const float* fk_acc,
                            std::vector<float>& out, std::vector<float>* rowsum) {
    const int n_pieces = 8 * nbk;
    out.assign((size_t)n_mesh * n_pieces * n_orders * 8, 0.0f);
    if (rowsum) rowsum->assign((size_t)n_mesh * n_orders, 0.0f);
    auto entry = [&](int nd, int row, int m) {
        const float t = (float)t64[((size_t)nd * nb + row) * n_mesh + m];   // the reference's fp32 table entry
        if (!fk_acc) return t;
        const int kb = row >> 5, w = row & 31, h = (w >> 2) & 1, r = (w & 3) + 4 * (w >> 3);   // acc_row(r, h) == w
        return (float)((double)fk_acc[(kb * 2 + h) * 16 + r] * (double)t);
    };
    for (int m = 0; m < n_mesh; ++m)
        for (int nd = 0; nd < n_orders; ++nd) {
            double rs = 0.0;
            for (int row = 0; row < nb; ++row) {
                const int pc = row >> 2, e = row & 3;
                for (int sd = 0; sd < 2; ++sd)
                    out[((((size_t)m * n_pieces + pc) * n_orders + nd) * 2 + sd) * 4 + e] = entry(nd, row, std::min(m + sd, n_mesh - 1));
                rs += (double)entry(nd, row, m);
            }
            if (rowsum) (*rowsum)[(size_t)m * n_orders + nd] = (float)rs;
        }
}

// Support bounds of the records of a pack_rows_pairs table: for piece 8 kb + 2q + h, bnd[(kb*2+h)*16+q*2+0] = the last mesh index up
// to which the piece's record equals the one at mesh point 0, bnd[(kb*2+h)*16+q*2+1] = the first one from which it equals the one
// at the last mesh point.  Spline bases have local support (I-splines: 0 below it, their full value above), so a read at
// clamp(m, lo, hi) returns the bits of the read at m, and the walkers outside a piece's support share two records instead of
// touching their own: found by comparing the table's actual fp32 entries, whatever the boundary map or the row factors made of them.
static void piece_bounds(const std::vector<float>& rows, int n_mesh, int n_orders, int nbk, int32_t* bnd) {
    const int n_pieces = 8 * nbk, rec = n_orders * 8;
    for (int kb = 0; kb < nbk; ++kb)
        for (int h = 0; h < 2; ++h)
            for (int q = 0; q < 4; ++q) {
                const int pc = 8 * kb + 2 * q + h;
                auto same = [&](int m, int ref) {
                    return memcmp(&rows[((size_t)m * n_pieces + pc) * rec], &rows[((size_t)ref * n_pieces + pc) * rec], rec * sizeof(float)) == 0;
                };
                int lo = 0, hi = n_mesh - 1;
                while (lo + 1 < n_mesh && same(lo + 1, 0)) ++lo;
                while (hi - 1 >= 0 && same(hi - 1, n_mesh - 1)) --hi;
                bnd[(kb * 2 + h) * 16 + q * 2 + 0] = lo;
                bnd[(kb * 2 + h) * 16 + q * 2 + 1] = hi;
            }
}

bool net_has_sigmoid_head(const wf_model* m, int n) {
    const bool is_prior = n == m->desc.n_flow_layers;
    if (is_prior) return m->desc.prior_kind == WF_PRIOR_MFLOW;
    return m->desc.layer_kind == WF_LAYER_IMADE;
}

// LDS image of net n in MFMA operand order (wf_kernels_mfma.hip: NetOff<D>), float offset `base` inside d_mfma.  fp16 operand
// pairs: x = hi + lo with hi, lo in fp16 (round to nearest; lo may be subnormal: absolute precision 2^-25), k_pack splits them.
static void describe_mfma_image(const wf_model* m, int n, uint32_t base, std::vector<PackRec>& out) {
    const int D = m->desc.n_dim, H = kHidden, nbk = m->mdev.nbk;
    const int S0 = (D + 1) / 2;
    const NetLayout& nl = m->nets[n];
    const NetOffsets q = net_offsets(m, n);
    // folded activation scales: tanh(x) = 1 - 2/(2^(c1 x) + 1), sigmoid(x) = 1/(1 + 2^(c2 x)).  The kernel feeds the layers behind a
    // tanh with r = 1/(2^(c1 x) + 1) instead of tanh = 1 - 2r: their weights carry the factor -2 here, their biases get the column
    // sums of the weights from k_fold_bias (wf_kernels_mfma.hip) after every k_pack.
    const double c1 = 2.0 * 1.4426950408889634074;
    const bool sig = net_has_sigmoid_head(m, n);
    const double c2 = sig ? -1.4426950408889634074 : 1.0;
    ImageWriter w{out, base};
    auto f16_block = [&](uint32_t n_pairs, auto&& src_of) {   // hi halves then lo halves; returns nothing, advances w.o
        uint32_t hi = 2 * w.o, lo = hi + n_pairs;
        for (uint32_t e = 0; e < n_pairs; ++e) {
            const std::pair<int64_t, double> sv = src_of(e);
            out.push_back(PackRec{(int32_t)sv.first, 1, hi++, lo++, sv.first >= 0 ? sv.second : 0.0});
        }
        w.o += n_pairs;
    };
    // layer 0 (f32 MFMA): A[i = unit 32*ob + (lane&31)][k = 2s + (lane>>5)]
    for (int ob = 0; ob < 2; ++ob)
        for (int s = 0; s < S0; ++s)
            for (int lane = 0; lane < 64; ++lane) {
                const int unit = 32 * ob + (lane & 31), k = 2 * s + (lane >> 5);
                w.f32((k < D && deg_hidden(unit, D) >= deg_in(k)) ? q.W0 + (int64_t)k * H + unit : -1, c1);
            }
    for (int ob = 0; ob < 2; ++ob)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) w.f32(q.b0 + 32 * ob + acc_row(r, h), c1);
    // layer 1 (f16 MFMA, K = 16 per step): step (t, s), element j of lane half h contracts hidden unit
    // kk = 32t + acc_row(8s + j, h);  images [ob][t][s][lane][8] for hi then lo
    f16_block(4096, [&](uint32_t e) {
        const int j = e & 7, lane = (e >> 3) & 63, s_ = (e >> 9) & 1, t = (e >> 10) & 1, ob = (e >> 11) & 1;
        const int unit = 32 * ob + (lane & 31), kk = 32 * t + acc_row(8 * s_ + j, lane >> 5);
        return std::make_pair(deg_hidden(unit, D) >= deg_hidden(kk, D) ? q.W1 + (int64_t)kk * H + unit : (int64_t)-1, -2.0 * c1);
    });
    for (int ob = 0; ob < 2; ++ob)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) w.f32(q.b1 + 32 * ob + acc_row(r, h), c1);
    // output layer, dimensions 1..D-1, row blocks kb: A[i = basis 32*kb + (lane&31)][k = kk]
    f16_block((uint32_t)((D - 1) * nbk * 2048), [&](uint32_t e) {
        const int j = e & 7, lane = (e >> 3) & 63, s_ = (e >> 9) & 1, t = (e >> 10) & 1;
        const int blk = e >> 11, kb = blk % nbk, d = 1 + blk / nbk;
        const int jb = 32 * kb + (lane & 31), kk = 32 * t + acc_row(8 * s_ + j, lane >> 5);
        const bool live = jb < nl.n_out && deg_out(d) >= deg_hidden(kk, D);
        return std::make_pair(live ? q.W2 + (int64_t)kk * q.NO + (jb * D + d) : (int64_t)-1, -2.0 * c2);
    });
    // biases; padding rows of sigmoid heads get +1e30 so that sigmoid(-x) -> 0 exactly
    for (int d = 0; d < D; ++d)
        for (int kb = 0; kb < nbk; ++kb)
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 16; ++r) {
                    const int jb = 32 * kb + acc_row(r, h);
                    if (jb < nl.n_out) w.f32(q.b2 + jb * D + d, c2);
                    else w.cst(sig ? 1e30 : 0.0);
                }
    // zero_params of a gated head, accumulator layout like the biases (|z| under a sigmoid head); zeros otherwise
    const bool gated = nl.has_zero && net_is_gated(m, n);
    for (int d = 0; d < D; ++d)
        for (int kb = 0; kb < nbk; ++kb)
            for (int h = 0; h < 2; ++h)
                for (int r = 0; r < 16; ++r) {
                    const int jb = 32 * kb + acc_row(r, h);
                    const int64_t src = (gated && jb < nl.n_out) ? q.b2 + q.NO + (int64_t)d * nl.n_out + jb : -1;
                    if (sig) w.f32_abs(src);
                    else w.f32(src);
                }
    // NetOff::reserved: the image's last 64 floats, which no kernel reads.  They keep what was always written there (the second hidden layer's
    // bias as c1 * b1, which k_fold_bias leaves alone), so that the image stays byte for byte what it was.
    for (int ob = 0; ob < 2; ++ob)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) w.f32(q.b1 + 32 * ob + acc_row(r, h), c1);
}

// Transposed operand images of net n for the reverse sweep of the matrix-core gradient path (k_ebwd, wf_etile_bwd.h; D = 2, <= 64 bases):
// hbar_1[k] = sum_u W1'[k][u] zbar_2[u] and hbar_2[k] = sum_j W2'[k][j] obar[j] are MFMA products whose A operand is the weight matrix with the
// INPUT unit on the row, same entries and scales as the forward image.  Layout (floats, base = float offset inside d_mfma; nbk = 32-row blocks of the head):
//   TW1 hi [ob 2][t 2][s 2][lane 64][8 halves] (2048 floats), TW1 lo (2048), TW2 hi [ob 2][kb nbk][s 2][64][8] (1024 nbk), TW2 lo (1024 nbk), W0'[0][unit] in
//   accumulator layout [ob][h][16] (64): the adjoint of the conditioner's input s is sum_u W0'[0][u] zbar_1[u].
static int tnet_floats_of(int nbk) { return 2048 + 2048 + 2048 * nbk + 64; }
static void describe_mfma_image_t(const wf_model* m, int n, uint32_t base, std::vector<PackRec>& out) {
    const int D = m->desc.n_dim, H = kHidden, nbk = m->mdev.nbk;
    const NetLayout& nl = m->nets[n];
    const NetOffsets q = net_offsets(m, n);
    const double c1 = 2.0 * 1.4426950408889634074;
    const double c2 = net_has_sigmoid_head(m, n) ? -1.4426950408889634074 : 1.0;
    ImageWriter w{out, base};
    auto f16_block = [&](uint32_t n_pairs, auto&& src_of) {
        uint32_t hi = 2 * w.o, lo = hi + n_pairs;
        for (uint32_t e = 0; e < n_pairs; ++e) {
            const std::pair<int64_t, double> sv = src_of(e);
            out.push_back(PackRec{(int32_t)sv.first, 1, hi++, lo++, sv.first >= 0 ? sv.second : 0.0});
        }
        w.o += n_pairs;
    };
    // A[m = input unit k = 32 ob + (lane & 31)][kk = output unit u = 32 t + acc_row(8 s + j, lane >> 5)] = W1'[k][u]
    f16_block(4096, [&](uint32_t e) {
        const int j = e & 7, lane = (e >> 3) & 63, s_ = (e >> 9) & 1, t = (e >> 10) & 1, ob = (e >> 11) & 1;
        const int k = 32 * ob + (lane & 31), u = 32 * t + acc_row(8 * s_ + j, lane >> 5);
        return std::make_pair(deg_hidden(u, D) >= deg_hidden(k, D) ? q.W1 + (int64_t)k * H + u : (int64_t)-1, -2.0 * c1);
    });
    // A[m = hidden unit k][kk = basis row jb = 32 kb + acc_row(8 s + j, lane >> 5)] = W2'[k][(jb, d = 1)]
    f16_block((uint32_t)(2048 * nbk), [&](uint32_t e) {
        const int j = e & 7, lane = (e >> 3) & 63, s_ = (e >> 9) & 1, blk = e >> 10, kb = blk % nbk, ob = blk / nbk;
        const int k = 32 * ob + (lane & 31), jb = 32 * kb + acc_row(8 * s_ + j, lane >> 5);
        const bool live = jb < nl.n_out && deg_out(1) >= deg_hidden(k, D);
        return std::make_pair(live ? q.W2 + (int64_t)k * q.NO + (jb * D + 1) : (int64_t)-1, -2.0 * c2);
    });
    for (int ob = 0; ob < 2; ++ob)
        for (int h = 0; h < 2; ++h)
            for (int r = 0; r < 16; ++r) w.f32(q.W0 + 32 * ob + acc_row(r, h), c1);   // W0[k = 0][unit]
}

// Decides whether the MFMA kernel covers this model and builds its parameter-independent parts.
// i64 / p64: the fp64 tables already built by model_build (I: [4][nb][n_mesh]; prior: OB or M), o2b: [nb][nb].
int mfma_prepare(wf_model* m, const std::vector<double>& i64, const std::vector<double>& p64, const std::vector<double>& o2b) {
    const wf_model_desc& d = m->desc;
    const int D = d.n_dim;
    m->mfma_ok = false;
    const int nbk = m->nbp / 32;
    if (!mfma_shape_built(D, nbk)) return WF_OK;
    const bool imade = d.layer_kind == WF_LAYER_IMADE && d.n_flow_layers > 0;
    if (imade && !m->bc_i_ok) return WF_OK;
    const bool spline_prior = d.prior_kind == WF_PRIOR_WAVEFLOW || d.prior_kind == WF_PRIOR_MFLOW;
    if (spline_prior && !m->bc_p_ok) return WF_OK;
    const int n_nets = (int)m->nets.size();
    const int consts = 64 * nbk + nbk * nbk * 1024 + 64 * nbk + 32 * nbk;   // fkI, fkP, ob_to_b image, piece bounds (flow table, prior table), cbP (constant term of the B prior's boundary map)
    const int net_floats = mfma_net_floats(D, nbk);
    const int64_t lds_cap = 160 * 1024 / 4 - 64;   // floats (the kernel also holds a few bytes of static LDS: its tile counter)
    int staged;
    if ((int64_t)consts + (int64_t)net_floats * n_nets <= lds_cap) staged = 0;        // every net resident
    else if ((int64_t)consts + net_floats + 16 * kStagedGroups * (D + 1) * 32 <= lds_cap) staged = 1;   // one slot + the state area, re-staged per super-chunk
    else return WF_OK;
    // the matrix-core gradient path (two particles, <= 64 bases, Waveflow prior, IMADE layers): transposed operand images behind the constants block
    const bool timg = D == 2 && (nbk == 1 || nbk == 2) && d.prior_kind == WF_PRIOR_WAVEFLOW && (d.layer_kind == WF_LAYER_IMADE || d.n_flow_layers == 0);
    const int tconsts = nbk * nbk * 1024;   // ob_to_b transposed: blocks [ka][ki]{hi [s 2][lane 64][8 halves] (512 floats), lo (512)}
    const int tnet_floats = tnet_floats_of(nbk);
    const int64_t total = (int64_t)net_floats * n_nets + consts + (timg ? (int64_t)tnet_floats * n_nets + tconsts : 0);

    MfmaDev& md = m->mdev;
    md = MfmaDev{};
    md.D = D; md.n_layers = d.n_flow_layers; md.layer_kind = d.layer_kind; md.box_kind = d.box_kind; md.prior_kind = d.prior_kind;
    md.box_L = d.box_size; md.i_reg = d.i_reg; md.normal_offset = d.normal_offset; md.constrained_mask = m->dev.constrained_mask;
    md.i_nb = m->i_nb; md.p_nb = m->p_nb; md.n_mesh = d.n_mesh; md.nbk = nbk;
    md.n_nets = n_nets; md.net_floats = net_floats; md.const_img_off = net_floats * n_nets; md.const_floats = consts; md.staged = staged;
    md.exact_div = mfma_div_ok(md.n_mesh) ? 0 : 1;
    md.prior_quotient = env_prior_quotient() ? 1 : 0;
    md.i_gate = m->dev.i_gate; md.p_gate = m->dev.p_gate;
    md.p_bias = (d.prior_kind == WF_PRIOR_WAVEFLOW && !m->p_cb.empty()) ? 1 : 0;
    md.p_plain_bc = (d.prior_kind == WF_PRIOR_WAVEFLOW && m->bc_p_plain) ? 1 : 0;
    md.tabB0 = m->d_tabB0;
    md.i_plain_bc = (imade && m->bc_i_plain) ? 1 : 0;
    md.timg_off = timg ? net_floats * n_nets + consts : -1;
    md.tnet_floats = tnet_floats;
    md.tconst_off = timg ? md.timg_off + tnet_floats * n_nets : -1;
    // staged mode: one net slot + the state area of the super-chunk (16 waves x kStagedGroups tile groups x (D + 1) x 32 floats: the
    // built staged shapes run 8 waves of one tile; sized for the largest workgroup)
    m->mfma_lds_floats = consts + (staged ? net_floats + 16 * kStagedGroups * (D + 1) * 32 : net_floats * n_nets);

    m->mfma_consts.assign(consts, 0.0f);
    int32_t* bnd = reinterpret_cast<int32_t*>(m->mfma_consts.data() + 64 * nbk + nbk * nbk * 1024);   // [2 tables][nbk][2 halves][16: 4 pieces x (lo, hi), 8 unused -- the lane stride of the fk blocks]
    for (int i = 0; i < 64 * nbk; ++i) bnd[i] = (i & 1) ? d.n_mesh - 1 : 0;   // (no clamp until a table says otherwise)
    if (md.p_bias) {   // cbP[kb][h][r] = p_cb[row of register r in lane half h of block kb]
        float* cb = m->mfma_consts.data() + 64 * nbk + nbk * nbk * 1024 + 64 * nbk;
        for (int kb = 0; kb < nbk; ++kb)
            for (int hh = 0; hh < 2; ++hh)
                for (int r = 0; r < 16; ++r) cb[(kb * 2 + hh) * 16 + r] = m->p_cb[32 * kb + acc_row(r, hh)];
    }
    std::vector<float> fk_nat(128, 0.0f);
    if (imade) {
        float* fk = m->mfma_consts.data();
        row_factors(WF_SPLINE_I, true, d.i_degree, m->i_nb, nbk, m->bc_i_colsum, fk, fk_nat.data());
        double F = 0;
        for (int i = 0; i < 32 * nbk; ++i) F += fk[i];
        md.F_I = (float)F;
        std::vector<float> rows, rowsum;
        pack_rows_pairs(i64, m->i_nb, d.n_mesh, 2, nbk, fk, rows, &rowsum);
        if (!env_mfma_no_band()) piece_bounds(rows, d.n_mesh, 2, nbk, bnd);   // (the switch: tests compare both, bit for bit)
        int rc = upload_table(m, rows, &md.tabI);
        if (rc) return rc;
        {   // [mesh][2] -> [mesh]{R0_m, R1_m, R0_{m+1}, R1_{m+1}} (the last mesh point repeats itself: it is a right end only)
            std::vector<float> pairs((size_t)d.n_mesh * 4);
            for (int mi = 0; mi < d.n_mesh; ++mi) {
                const int mr = std::min(mi + 1, d.n_mesh - 1);
                pairs[(size_t)mi * 4 + 0] = rowsum[(size_t)mi * 2]; pairs[(size_t)mi * 4 + 1] = rowsum[(size_t)mi * 2 + 1];
                pairs[(size_t)mi * 4 + 2] = rowsum[(size_t)mr * 2]; pairs[(size_t)mi * 4 + 3] = rowsum[(size_t)mr * 2 + 1];
            }
            rc = upload_table(m, pairs, &md.rsI);
            if (rc) return rc;
        }
    }
    if (spline_prior) {
        const bool mflow = d.prior_kind == WF_PRIOR_MFLOW;
        float* fk = m->mfma_consts.data() + 32 * nbk;
        row_factors(mflow ? WF_SPLINE_M : WF_SPLINE_B, mflow, d.p_degree, m->p_nb, nbk, m->bc_p_colsum, fk, fk_nat.data() + 64);
        double F = 0;
        for (int i = 0; i < 32 * nbk; ++i) F += fk[i];
        md.F_P = (float)F;
        std::vector<float> rows;
        // M prior: the row factors are folded into the table; B prior: they act on the weights before ob_to_b
        pack_rows_pairs(p64, m->p_nb, d.n_mesh, 1, nbk, mflow ? fk : nullptr, rows, nullptr);
        if (!env_mfma_no_band()) piece_bounds(rows, d.n_mesh, 1, nbk, bnd + 32 * nbk);
        int rc = upload_table(m, rows, &md.tabP);
        if (rc) return rc;
        if (!mflow) {
            // c[i] = sum_a w[a] * ob_to_b[a][i] as split-fp16 MFMA products: block (ko, ki), K step s:
            // A[i = 32*ko + (lane&31)][k = a = 32*ki + acc_row(8*s + j, lane>>5)], hi halves [s][lane][8] then lo halves (1024 each)
            _Float16* o = reinterpret_cast<_Float16*>(m->mfma_consts.data() + 64 * nbk);
            const int nb = m->p_nb;
            for (int ko = 0; ko < nbk; ++ko)
                for (int ki = 0; ki < nbk; ++ki) {
                    _Float16* blk = o + (size_t)(ko * nbk + ki) * 2048;
                    for (int s_ = 0; s_ < 2; ++s_)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int j = 0; j < 8; ++j) {
                                const int i = 32 * ko + (lane & 31), a = 32 * ki + acc_row(8 * s_ + j, lane >> 5);
                                const float v = (i < nb && a < nb) ? (float)o2b[(size_t)a * nb + i] : 0.0f;
                                const _Float16 hi = (_Float16)v;
                                blk[(s_ * 64 + lane) * 8 + j] = hi;
                                blk[1024 + (s_ * 64 + lane) * 8 + j] = (_Float16)(v - (float)hi);
                            }
                }
        }
    }
    int rc = dev_alloc(m, &m->d_mfma, (size_t)total);
    if (rc) return rc;
    md.image = m->d_mfma;
    rc = dev_alloc(m, &m->d_fk_nat, 128);
    if (rc) return rc;
    WF_HIP(hipMemcpy(m->d_fk_nat, fk_nat.data(), 128 * sizeof(float), hipMemcpyHostToDevice));
    {
        float* comp = nullptr;
        // [comp][coefficients of k_dim0_coeffs][comp2]
        const size_t comp_floats = (size_t)std::max(n_nets, 1) * d.n_mesh * 4, coef_floats = (size_t)dim0_coef_floats(std::max(n_nets, 1));
        rc = dev_alloc(m, &comp, comp_floats + ((coef_floats + 3) & ~(size_t)3) + comp_floats);
        if (rc) return rc;
        m->d_comp = comp;
        md.comp = reinterpret_cast<const float4_t*>(comp);
        md.comp2 = reinterpret_cast<const float4_t*>(comp + comp_floats + ((coef_floats + 3) & ~(size_t)3));
    }
    {   // fp16-range flags of the operand images (one per net), their pinned host copy and the event that says it has arrived
        rc = dev_alloc(m, &m->d_f16_ovf, (size_t)kMaxNets);
        if (rc) return rc;
        WF_HIP(hipMemset(m->d_f16_ovf, 0, kMaxNets * sizeof(int)));
        WF_HIP(hipHostMalloc(reinterpret_cast<void**>(&m->h_f16_ovf), kMaxNets * sizeof(int), hipHostMallocDefault));
        memset(m->h_f16_ovf, 0, kMaxNets * sizeof(int));
        WF_HIP(hipEventCreateWithFlags(&m->ovf_event, hipEventDisableTiming));
        md.f16_ovf = m->d_f16_ovf;
    }
    m->mfma_floats = total;
    m->mfma_ok = true;
    // the constants block does not depend on the parameters: upload it once
    WF_HIP(hipMemset(m->d_mfma, 0, (size_t)total * sizeof(float)));
    WF_HIP(hipMemcpy(m->d_mfma + md.const_img_off, m->mfma_consts.data(), m->mfma_consts.size() * sizeof(float), hipMemcpyHostToDevice));
    if (timg && spline_prior) {
        // wbar[a] = sum_i M[a][i] cbar[i] (M = ob_to_b with the boundary map folded in, as the forward image holds it): block (ka, ki) in the order
        // prior_c_block reads (output block first): A[m = a = 32 ka + (lane & 31)][kk = i = 32 ki + acc_row(8 s + j, lane >> 5)]
        std::vector<float> tc(tconsts, 0.0f);
        _Float16* o = reinterpret_cast<_Float16*>(tc.data());
        const int nb = m->p_nb;
        for (int ka = 0; ka < nbk; ++ka)
            for (int ki = 0; ki < nbk; ++ki) {
                _Float16* blk = o + (size_t)(ka * nbk + ki) * 2048;
                for (int s_ = 0; s_ < 2; ++s_)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int a = 32 * ka + (lane & 31), i = 32 * ki + acc_row(8 * s_ + j, lane >> 5);
                            const float v = (i < nb && a < nb) ? (float)o2b[(size_t)a * nb + i] : 0.0f;
                            const _Float16 hi = (_Float16)v;
                            blk[(s_ * 64 + lane) * 8 + j] = hi;
                            blk[1024 + (s_ * 64 + lane) * 8 + j] = (_Float16)(v - (float)hi);
                        }
            }
        WF_HIP(hipMemcpy(m->d_mfma + md.tconst_off, tc.data(), tc.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return WF_OK;
}

// Describes every weight image (PackRec lists on the device) and derives the gradient scatter map: forward-image entry ->
// flat parameter (masked and padding entries have no source: no gradient).
int pack_prepare(wf_model* m, std::vector<PackRec>& plain) {
    const int D = m->desc.n_dim;
    const int n_nets = (int)m->nets.size();
    std::vector<PackRec> wave, mfma;
    for (int n = 0; n < n_nets; ++n) {
        describe_plain_image(m, n, (uint32_t)m->plain_off[n], plain);
        if (m->d_wave) describe_wave_image(m, n, (uint32_t)(wave_net_floats(D, m->nbp) * n), wave);
        if (m->mfma_ok) describe_mfma_image(m, n, (uint32_t)((int64_t)m->mdev.net_floats * n), mfma);
        if (m->mfma_ok && m->mdev.timg_off >= 0) describe_mfma_image_t(m, n, (uint32_t)(m->mdev.timg_off + (int64_t)m->mdev.tnet_floats * n), mfma);
    }
    std::vector<PackRec> all;
    all.reserve(plain.size() + wave.size() + mfma.size());
    std::vector<PackRec>* lists[3] = {&plain, &wave, &mfma};
    for (int i = 0; i < 3; ++i)
        for (PackRec r : *lists[i]) {
            r.kind |= i << 8;
            all.push_back(r);
        }
    m->n_pack = (int64_t)all.size();
    if (!all.empty()) {
        int rc = dev_alloc(m, &m->d_pack, all.size());
        if (rc) return rc;
        WF_HIP(hipMemcpy(m->d_pack, all.data(), all.size() * sizeof(PackRec), hipMemcpyHostToDevice));
    }
    return dev_alloc(m, &m->d_flat, (size_t)std::max<int64_t>(m->n_params, 1));
}

}  // namespace wf
