// wf_model_build.cpp -- wf_model: host-side model build (boundary-condition algebra, tables, device images, gradient maps), parameter upload
// and the model's life cycle in the C ABI.
//
// Reference behaviour mirrored here (paths relative to /root/reference/waveflow):
//   table dtype ......................... jnp.array(np.load(...)) => fp32 (isplines_jax.py:131)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "wf_model.h"

namespace wf {

static int check_bc(const wf_bc& bc, int nb) {
    if (bc.n < 0 || bc.n > WF_MAX_BC) return WF_ERR_INVALID;
    for (int i = 0; i < bc.n; ++i)
        if (bc.n_derivative[i] < 0 || bc.n_derivative[i] > 3 || bc.n_derivative[i] >= nb) return WF_ERR_INVALID;
    return WF_OK;
}

// Dense-row device table: [n_orders][n_mesh][nbp], fp32 cast of the fp64 table.
static void pack_rows(const std::vector<double>& t64, int nb, int n_mesh, int n_orders, int nbp, std::vector<float>& out) {
    out.assign((size_t)n_orders * n_mesh * nbp, 0.0f);
    for (int nd = 0; nd < n_orders; ++nd)
        for (int i = 0; i < nb; ++i)
            for (int m = 0; m < n_mesh; ++m)
                out[((size_t)nd * n_mesh + m) * nbp + i] = (float)t64[((size_t)nd * nb + i) * n_mesh + m];
}

// Boundary-condition constants (enforce_boundary_conditions: isplines_jax.py:158-194,
// bsplines_jax.py:173-199, msplines_jax.py:156-184): X_cached(0.0, j, nd) == T[nd][j][0] and
// X_cached(1.0, j, nd) == T[nd][j][n_mesh-1] in fp32.
static void fill_bc(SplineDev& s, const wf_bc& left, const wf_bc& right, const std::vector<double>& t64, int nb, int n_mesh) {
    auto T = [&](int nd, int j, int m) { return (float)t64[((size_t)nd * nb + j) * n_mesh + m]; };
    s.n_left = left.n;
    s.n_right = right.n;
    for (int p = 0; p < left.n; ++p) {
        const int nd = left.n_derivative[p];
        s.left_nd[p] = nd;
        s.left_val[p] = left.value[p];
        for (int j = 0; j < nd; ++j) s.left_prev[p][j] = T(nd, j, 0);
        s.left_value[p] = T(nd, nd, 0);
    }
    for (int p = 0; p < right.n; ++p) {
        const int nd = right.n_derivative[p];
        s.right_nd[p] = nd;
        s.right_val[p] = right.value[p];
        for (int j = 0; j < nd; ++j) s.right_prev[p][j] = T(nd, nb - j - 1, n_mesh - 1);
        s.right_value[p] = T(nd, nb - nd - 1, n_mesh - 1);
    }
}

// ---- boundary conditions as a linear map.  enforce_boundary_conditions (isplines_jax.py:166-190, msplines_jax.py:155-180,
// bsplines_jax.py:176-189) overwrites coefficient nd (left) / nb-1-nd (right) of every constraint {nd: value} with
// (value - sum_{j<nd} T^(nd)_j(end) c_j) / T^(nd)_nd(end), in dictionary order, before the final normalisation: c' = A c + b with A, b
// fixed per model.  With b == 0 (every value 0; the I-spline's right {0: 1} zeroes the last coefficient, isplines_jax.py:174-179) the
// normalised spline  sum_j c'_j T_j(x) / sum_j c'_j  equals  sum_j (c_j a~_j) T^_j(x) / sum_j (c_j a~_j)  with a~ = A^T 1 (column sums)
// and T^_j = (A^T T)_j / a~_j: the same expression the kernels evaluate for "zero the first / last coefficient" (a~ in {0, 1}, T^ = T),
// so the table-driven kernels (MFMA, wave sweeps, gradients) cover every homogeneous dictionary through their tables and row factors
// alone.  The per-walker scalar kernel keeps the literal sequence (enforce_bc, wf_scalar_impl.h) and also covers the B-spline prior with b != 0.
static void bc_apply(const SplineDev& s, int kind, int nb, std::vector<double>& c) {
    for (int p = 0; p < s.n_left; ++p) {
        const int nd = s.left_nd[p];
        double sum = 0;
        for (int j = 0; j < nd; ++j) sum += (double)s.left_prev[p][j] * c[j];
        c[nd] = ((double)s.left_val[p] - sum) / (double)s.left_value[p];
    }
    for (int p = 0; p < s.n_right; ++p) {
        const int nd = s.right_nd[p];
        if (kind == WF_SPLINE_I && nd == 0) { c[nb - 1] = 0.0; continue; }
        double sum = 0;
        for (int j = 0; j < nd; ++j) sum += (double)s.right_prev[p][j] * c[nb - 1 - j];
        c[nb - nd - 1] = ((double)s.right_val[p] - sum) / (double)s.right_value[p];
    }
}
// -> A [nb][nb] (c' = A c), column sums; false when the map keeps a constant term or has a column that sums to zero without being zero
static bool bc_map(const SplineDev& s, int kind, int nb, std::vector<double>& A, std::vector<double>& colsum, std::vector<double>* bconst = nullptr) {
    A.assign((size_t)nb * nb, 0.0);
    colsum.assign(nb, 0.0);
    std::vector<double> c(nb, 0.0);
    bc_apply(s, kind, nb, c);
    bool ok = true, constant = false;
    for (int i = 0; i < nb; ++i) constant = constant || c[i] != 0.0;
    // A constant term b (a constraint with a non-zero value).  The I- and M-spline coefficients enter the constraints normalised
    // (remove_bias ends with p / sum p: isplines_jax.py:196-202, msplines_jax.py:186-192), so b = b (1^T c) and the map is the linear
    // A + b 1^T on them.  The B-spline prior's weights reach the constraints divided by their signed sum S (model_factory.py:69) and are
    // normalised only afterwards: w' = (A o + S b) / S, so the kernels carry b as a separate term (bconst; round 3) scaled by S = sum o.
    const bool fold = constant && (kind == WF_SPLINE_I || kind == WF_SPLINE_M);
    if (constant && !fold) {
        if (bconst) *bconst = c;
        else ok = false;
    }
    for (int j = 0; j < nb; ++j) {
        std::vector<double> e(nb, 0.0);
        e[j] = 1.0;
        bc_apply(s, kind, nb, e);
        bool all_zero = true;
        for (int i = 0; i < nb; ++i) {
            const double a = e[i] - c[i] + (fold ? c[i] : 0.0);
            A[(size_t)i * nb + j] = a;
            colsum[j] += a;
            all_zero = all_zero && a == 0.0;
        }
        if (all_zero) colsum[j] = 0.0;
        else if (std::fabs(colsum[j]) < 1e-9 || (fold && colsum[j] < 0.0)) ok = false;   // (the kernels' row factors of a folded map stay positive)
    }
    return ok;
}
// rows of a table indexed by the coefficient ([orders][nb][n_mesh] fp64, or [nb][cols] with n_mesh := cols, orders := 1): X^_j = (A^T X)_j / a~_j
static void bc_transform_rows(const std::vector<double>& A, const std::vector<double>& colsum, int nb, int orders, int n_mesh, std::vector<double>& t) {
    std::vector<double> out(t.size(), 0.0);
    for (int nd = 0; nd < orders; ++nd)
        for (int j = 0; j < nb; ++j) {
            if (colsum[j] == 0.0) continue;
            double* o = &out[((size_t)nd * nb + j) * n_mesh];
            for (int i = 0; i < nb; ++i) {
                const double a = A[(size_t)i * nb + j];
                if (a == 0.0) continue;
                const double* src = &t[((size_t)nd * nb + i) * n_mesh];
                for (int m = 0; m < n_mesh; ++m) o[m] += a * src[m];
            }
            for (int m = 0; m < n_mesh; ++m) o[m] /= colsum[j];
        }
    t.swap(out);
}

int upload_table(wf_model* m, const std::vector<float>& h, const float** out) {
    float* d = nullptr;
    int rc = dev_alloc(m, &d, h.size());
    if (rc) return rc;
    WF_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    *out = d;
    return WF_OK;
}

// [4][n_mesh][nbp] -> [n_mesh][nbp / 4 chunks][4 orders][4 rows] (see d_tabI4c), + the chunks' support bounds
static int upload_chunked(wf_model* m, const std::vector<float>& rows4, int n_mesh, int nbp, const float** out) {
    const int chunks = nbp / 4, stride = nbp * 4;   // floats per mesh point
    std::vector<float> c((size_t)n_mesh * stride);
    for (int mm = 0; mm < n_mesh; ++mm)
        for (int ch = 0; ch < chunks; ++ch)
            for (int k = 0; k < 4; ++k)
                for (int q = 0; q < 4; ++q) c[(((size_t)mm * chunks + ch) * 4 + k) * 4 + q] = rows4[((size_t)k * n_mesh + mm) * nbp + 4 * ch + q];
    // behind the table: int32 [chunks][lo, hi], the support bounds of the chunks (as piece_bounds below: a chunk read at clamp(m, lo, hi)
    // returns the bits of the chunk at m; the head code of the energy path clamps, and walkers outside a chunk's support share lines)
    std::vector<int32_t> bnd(2 * chunks);
    for (int ch = 0; ch < chunks; ++ch) {
        auto same = [&](int a, int b) { return memcmp(&c[((size_t)a * chunks + ch) * 16], &c[((size_t)b * chunks + ch) * 16], 16 * sizeof(float)) == 0; };
        int lo = 0, hi = n_mesh - 1;
        if (!env_mfma_no_band()) {
            while (lo + 1 < n_mesh && same(lo + 1, 0)) ++lo;
            while (hi - 1 >= 0 && same(hi - 1, n_mesh - 1)) --hi;
        }
        bnd[2 * ch] = lo;
        bnd[2 * ch + 1] = hi;
    }
    c.resize(c.size() + 2 * chunks);
    memcpy(&c[(size_t)n_mesh * stride], bnd.data(), 2 * chunks * sizeof(int32_t));
    return upload_table(m, c, out);
}

// layer_kind WF_LAYER_NSC: Flow(Serial((NeuralSplineCoupling [, Reverse]) x L), Normal | Uniform)
static int nsc_build(wf_model* m) {
    const wf_model_desc& d = m->desc;
    const int D = d.n_dim, K = d.nsc_bins, h = d.nsc_hidden;
    if (D < 2 || D > WF_MAX_DIM || (D % 2) != 0) return WF_ERR_INVALID;          // (dim // 2 coordinates per half, neural_splines.py:256)
    if (d.n_flow_layers < 1 || d.n_flow_layers > kMaxLayers) return WF_ERR_INVALID;
    if (K < 2 || h < 1 || !(d.nsc_tail_bound > 0.0f)) return WF_ERR_INVALID;
    if (d.prior_kind != WF_PRIOR_NORMAL && d.prior_kind != WF_PRIOR_UNIFORM) return WF_ERR_UNSUPPORTED;
    if (!nsc_model_built(D, K, h)) return WF_ERR_UNSUPPORTED;
    const int dh = D / 2, per = 3 * K - 1;
    const int64_t net_floats = (int64_t)dh * h + h + (int64_t)h * h + h + (int64_t)h * per * dh + (int64_t)per * dh;
    m->n_params = net_floats * 2 * d.n_flow_layers;
    int rc = dev_alloc(m, &m->d_flat, (size_t)m->n_params);
    if (rc) return rc;
    rc = dev_alloc(m, &m->d_nsc, (size_t)m->n_params);
    if (rc) return rc;
    m->dev = ModelDev{};
    m->dev.D = D;
    m->dev.prior_kind = d.prior_kind;
    m->nbp = 32;
    m->nsc = NscModelDev{D, d.n_flow_layers, K, h, d.prior_kind, d.nsc_reverse != 0 ? 1 : 0, d.nsc_tail_bound, d.normal_offset, m->d_nsc, net_floats};
    m->is_nsc = true;
    return WF_OK;
}

static int grad_prepare(wf_model* m);

static int model_build(wf_model* m) {
    const wf_model_desc& d = m->desc;
    const int D = d.n_dim;
    if (d.layer_kind == WF_LAYER_NSC) return nsc_build(m);
    if (D < 2 || D > WF_MAX_DIM) return WF_ERR_INVALID;
    if (d.hidden != kHidden) return WF_ERR_UNSUPPORTED;
    if (d.n_flow_layers < 0 || d.n_flow_layers > kMaxLayers) return WF_ERR_INVALID;
    if (d.layer_kind != WF_LAYER_IMADE && d.layer_kind != WF_LAYER_MADE) return WF_ERR_INVALID;
    if (d.box_kind < WF_BOX_NONE || d.box_kind > WF_BOX_FIRST) return WF_ERR_INVALID;
    if (d.prior_kind < WF_PRIOR_WAVEFLOW || d.prior_kind > WF_PRIOR_NORMAL) return WF_ERR_INVALID;
    if (d.n_mesh < 2) return WF_ERR_INVALID;
    if (d.n_constrained_left < 0 || d.n_constrained_left > WF_MAX_DIM) return WF_ERR_INVALID;

    ModelDev& md = m->dev;
    md = ModelDev{};
    md.D = D;
    md.n_layers = d.n_flow_layers;
    md.layer_kind = d.layer_kind;
    md.box_kind = d.box_kind;
    md.box_L = d.box_size;
    md.i_reg = d.i_reg;
    md.prior_kind = d.prior_kind;
    md.normal_offset = d.normal_offset;
    md.reverse_tol = d.i_reverse_tol > 0.0f ? d.i_reverse_tol : 1.0f / (float)d.n_mesh;   // isplines_jax.py:89-90
    md.i_gate = (d.i_gate != 0 && d.layer_kind == WF_LAYER_IMADE && d.n_flow_layers > 0) ? 1 : 0;
    md.p_gate = (d.p_gate != 0 && (d.prior_kind == WF_PRIOR_WAVEFLOW || d.prior_kind == WF_PRIOR_MFLOW)) ? 1 : 0;
    for (int i = 0; i < d.n_constrained_left; ++i) {
        if (d.constrained_left[i] < 0 || d.constrained_left[i] >= D) return WF_ERR_INVALID;
        md.constrained_mask |= 1u << d.constrained_left[i];
    }

    // padded bases per dimension: 32 covers every shipped configuration; 64 e.g. the 33-knot ("32-bin") variant
    {
        int nb_max = 2;
        if (d.layer_kind == WF_LAYER_IMADE && d.n_flow_layers > 0) nb_max = std::max(nb_max, n_bases_of(WF_SPLINE_I, d.i_degree, d.i_knots));
        if (d.prior_kind == WF_PRIOR_WAVEFLOW) nb_max = std::max(nb_max, n_bases_of(WF_SPLINE_B, d.p_degree, d.p_knots));
        if (d.prior_kind == WF_PRIOR_MFLOW) nb_max = std::max(nb_max, n_bases_of(WF_SPLINE_M, d.p_degree, d.p_knots));
        m->nbp = nb_max <= 32 ? 32 : 64;
        if (nb_max > 64) return WF_ERR_UNSUPPORTED;
    }
    md.nbp = m->nbp;
    std::vector<double> keep_i64, keep_p64, keep_o2b;
    // ---- tables
    if (d.layer_kind == WF_LAYER_IMADE && d.n_flow_layers > 0) {
        const int nb = n_bases_of(WF_SPLINE_I, d.i_degree, d.i_knots);
        if (d.i_degree < 1 || d.i_knots < 2 || nb < 2) return WF_ERR_INVALID;
        if (nb > m->nbp) return WF_ERR_UNSUPPORTED;
        int rc = check_bc(d.i_left, nb);
        if (rc) return rc;
        rc = check_bc(d.i_right, nb);
        if (rc) return rc;
        // right constraint {0: v}: the reference supports v == 1 only (isplines_jax.py:174-179)
        for (int p = 0; p < d.i_right.n; ++p)
            if (d.i_right.n_derivative[p] == 0 && d.i_right.value[p] != 1.0f) return WF_ERR_INVALID;
        std::vector<double> t64((size_t)4 * nb * d.n_mesh);
        rc = build_raw_table(WF_SPLINE_I, d.i_degree, d.i_knots, d.n_mesh, t64.data());
        if (rc < 0) return rc;
        std::vector<float> rows;
        pack_rows(t64, nb, d.n_mesh, 2, m->nbp, rows);
        rc = upload_table(m, rows, &md.isp.tab);
        if (rc) return rc;
        md.isp.nb = nb; md.isp.nbp = m->nbp; md.isp.n_mesh = d.n_mesh; md.isp.degree = d.i_degree;
        fill_bc(md.isp, d.i_left, d.i_right, t64, nb, d.n_mesh);
        {   // the table-driven kernels read the rows with the boundary map folded in (identical rows for zero-only constraints)
            std::vector<double> A;
            m->bc_i_ok = bc_map(md.isp, WF_SPLINE_I, nb, A, m->bc_i_colsum);
            m->bc_i_plain = m->bc_i_ok;
            for (int i = 0; i < nb && m->bc_i_plain; ++i)
                for (int j = 0; j < nb; ++j)
                    if (A[(size_t)i * nb + j] != ((i == j && m->bc_i_colsum[j] != 0.0) ? 1.0 : 0.0)) { m->bc_i_plain = false; break; }
            if (m->bc_i_ok) bc_transform_rows(A, m->bc_i_colsum, nb, 4, d.n_mesh, t64);
        }
        {   // derivative orders 0..3 for the wave kernels
            std::vector<float> rows4;
            pack_rows(t64, nb, d.n_mesh, 4, m->nbp, rows4);
            rc = upload_table(m, rows4, &m->d_tabI4);
            if (rc) return rc;
            rc = upload_chunked(m, rows4, d.n_mesh, m->nbp, &m->d_tabI4c);   // (the matrix-core energy path: D = 2 only, but the tables are small)
            if (rc) return rc;
        }
        m->i_nb = nb;
        keep_i64.swap(t64);
    }
    if (d.prior_kind == WF_PRIOR_WAVEFLOW) {
        const int nb = n_bases_of(WF_SPLINE_B, d.p_degree, d.p_knots);
        if (d.p_degree < 1 || d.p_knots < 2 || nb < 2) return WF_ERR_INVALID;
        if (nb > m->nbp) return WF_ERR_UNSUPPORTED;
        int rc = check_bc(d.p_left, nb);
        if (rc) return rc;
        rc = check_bc(d.p_right, nb);
        if (rc) return rc;
        std::vector<double> b64((size_t)4 * nb * d.n_mesh), ob64((size_t)4 * nb * d.n_mesh), o2b((size_t)nb * nb), b2o((size_t)nb * nb);
        rc = build_raw_table(WF_SPLINE_B, d.p_degree, d.p_knots, d.n_mesh, b64.data());
        if (rc < 0) return rc;
        rc = build_ortho_b(d.p_degree, d.p_knots, d.n_mesh, b64.data(), ob64.data(), b2o.data(), o2b.data());
        if (rc < 0) return rc;
        std::vector<float> rows;
        pack_rows(ob64, nb, d.n_mesh, 1, m->nbp, rows);
        rc = upload_table(m, rows, &md.psp.tab);
        if (rc) return rc;
        md.psp.nb = nb; md.psp.nbp = m->nbp; md.psp.n_mesh = d.n_mesh; md.psp.degree = d.p_degree;
        {
            std::vector<float> rows3;
            pack_rows(ob64, nb, d.n_mesh, 4, m->nbp, rows3);
            rc = upload_table(m, rows3, &m->d_tabP3);
            if (rc) return rc;
            rc = upload_chunked(m, rows3, d.n_mesh, m->nbp, &m->d_tabP4c);
            if (rc) return rc;
        }
        {
            std::vector<float> rowsB;
            pack_rows(b64, nb, d.n_mesh, 1, m->nbp, rowsB);
            rc = upload_table(m, rowsB, &m->d_tabB0);
            if (rc) return rc;
        }
        fill_bc(md.psp, d.p_left, d.p_right, b64, nb, d.n_mesh);  // BCs use the plain-B table, bsplines_jax.py:176-189
        std::vector<float> o2b32((size_t)m->nbp * m->nbp, 0.0f);   // full [nbp][nbp]: the wave kernels contract over all 32 rows
        for (int a = 0; a < nb; ++a)
            for (int j = 0; j < nb; ++j) o2b32[(size_t)a * m->nbp + j] = (float)o2b[(size_t)a * nb + j];
        rc = upload_table(m, o2b32, &md.ob_to_b);
        if (rc) return rc;
        {   // the constraints act on the net's outputs w before c = w @ ob_to_b: fold the map into the matrix's rows (row a = coefficient a)
            std::vector<double> A, bconst;
            m->bc_p_ok = bc_map(md.psp, WF_SPLINE_B, nb, A, m->bc_p_colsum, &bconst);
            m->bc_p_plain = m->bc_p_ok && bconst.empty();
            for (int i = 0; i < nb && m->bc_p_plain; ++i)
                for (int j = 0; j < nb; ++j)
                    if (A[(size_t)i * nb + j] != ((i == j && m->bc_p_colsum[j] != 0.0) ? 1.0 : 0.0)) { m->bc_p_plain = false; break; }
            if (m->bc_p_ok && !bconst.empty()) {   // constant term: cb = b @ ob_to_b (the matrix as it is, before the map is folded into its rows)
                m->p_cb.assign(m->nbp, 0.0f);
                for (int i = 0; i < nb; ++i) {
                    double acc = 0;
                    for (int a = 0; a < nb; ++a) acc += bconst[a] * o2b[(size_t)a * nb + i];
                    m->p_cb[i] = (float)acc;
                }
                rc = upload_table(m, m->p_cb, &md.p_cb);
                if (rc) return rc;
            }
            if (m->bc_p_ok) bc_transform_rows(A, m->bc_p_colsum, nb, 1, nb, o2b);
            for (int a = 0; a < nb; ++a)
                for (int j = 0; j < nb; ++j) o2b32[(size_t)a * m->nbp + j] = (float)o2b[(size_t)a * nb + j];
            rc = upload_table(m, o2b32, &md.ob_to_b_t);
            if (rc) return rc;
        }
        std::vector<float> b2o32((size_t)m->nbp * m->nbp, 0.0f);
        for (int a = 0; a < nb; ++a)
            for (int j = 0; j < nb; ++j) b2o32[(size_t)a * m->nbp + j] = (float)b2o[(size_t)a * nb + j];
        rc = upload_table(m, b2o32, &md.b_to_ob);
        if (rc) return rc;
        m->p_nb = nb;
        keep_p64.swap(ob64);
        keep_o2b.swap(o2b);
    } else if (d.prior_kind == WF_PRIOR_MFLOW) {
        const int nb = n_bases_of(WF_SPLINE_M, d.p_degree, d.p_knots);
        if (d.p_degree < 2 || d.p_knots < 2 || nb < 2) return WF_ERR_INVALID;
        if (nb > m->nbp) return WF_ERR_UNSUPPORTED;
        int rc = check_bc(d.p_left, nb);
        if (rc) return rc;
        rc = check_bc(d.p_right, nb);
        if (rc) return rc;
        std::vector<double> t64((size_t)4 * nb * d.n_mesh);
        rc = build_raw_table(WF_SPLINE_M, d.p_degree, d.p_knots, d.n_mesh, t64.data());
        if (rc < 0) return rc;
        std::vector<float> rows;
        pack_rows(t64, nb, d.n_mesh, 1, m->nbp, rows);
        rc = upload_table(m, rows, &md.psp.tab);
        if (rc) return rc;
        md.psp.nb = nb; md.psp.nbp = m->nbp; md.psp.n_mesh = d.n_mesh; md.psp.degree = d.p_degree;
        fill_bc(md.psp, d.p_left, d.p_right, t64, nb, d.n_mesh);
        {
            std::vector<double> A;
            m->bc_p_ok = bc_map(md.psp, WF_SPLINE_M, nb, A, m->bc_p_colsum);
            if (m->bc_p_ok) bc_transform_rows(A, m->bc_p_colsum, nb, 4, d.n_mesh, t64);
        }
        {
            std::vector<float> rows4;
            pack_rows(t64, nb, d.n_mesh, 4, m->nbp, rows4);
            rc = upload_table(m, rows4, &m->d_tabP3);
            if (rc) return rc;
        }
        m->p_nb = nb;
        keep_p64.swap(t64);
    }

    // ---- parameter layout (pytree leaf order)
    m->nets.clear();
    int64_t off = 0;
    auto add_net = [&](int n_out, bool has_zero) {
        NetLayout nl;
        nl.n_out = n_out;
        nl.has_zero = has_zero;
        nl.offset = off;
        nl.count = (int64_t)D * kHidden + kHidden + (int64_t)kHidden * kHidden + kHidden + (int64_t)kHidden * n_out * D +
                   (int64_t)n_out * D + (has_zero ? (int64_t)D * n_out : 0);
        off += nl.count;
        m->nets.push_back(nl);
    };
    for (int l = 0; l < d.n_flow_layers; ++l) {
        if (d.layer_kind == WF_LAYER_IMADE) add_net(m->i_nb, true);
        else add_net(2, false);
    }
    if (d.prior_kind == WF_PRIOR_WAVEFLOW || d.prior_kind == WF_PRIOR_MFLOW) add_net(m->p_nb, true);
    m->n_params = off;

    // ---- device weight images
    const int n_nets = (int)m->nets.size();
    m->plain_floats = plain_net_floats(D, m->nbp) * n_nets;
    int rc = dev_alloc(m, &m->d_plain, (size_t)m->plain_floats);
    if (rc) return rc;
    m->plain_off.assign(n_nets, 0);
    for (int n = 0; n < n_nets; ++n) {
        const int64_t base = plain_net_floats(D, m->nbp) * n;
        m->plain_off[n] = base;
        float* p = m->d_plain + base;
        NetPlain& np = md.nets[n];
        np.W0 = p; p += (int64_t)D * kHidden;
        np.b0 = p; p += kHidden;
        np.W1t = p; p += (int64_t)kHidden * kHidden;
        np.b1 = p; p += kHidden;
        np.W2t = p; p += (int64_t)D * m->nbp * kHidden;
        np.b2 = p; p += (int64_t)D * m->nbp;
        np.W1n = p; p += (int64_t)kHidden * kHidden;
        np.W2n = p; p += (int64_t)kHidden * D * m->nbp;
        np.zero = p; p += (int64_t)D * m->nbp;
        np.zero_raw = p;
    }
    {
        const int P = wave_passes(D, m->nbp);
        rc = dev_alloc(m, &m->d_wave, (size_t)(wave_net_floats(D, m->nbp) * n_nets));
        if (rc) return rc;
        for (int n = 0; n < n_nets; ++n) {
            float* p = m->d_wave + wave_net_floats(D, m->nbp) * n;
            NetWave& nw = md.wnets[n];
            nw.W0 = p; p += (int64_t)D * kHidden;
            nw.b0 = p; p += kHidden;
            nw.b1 = p; p += kHidden;
            nw.b2 = p; p += (int64_t)P * 64;
            nw.W1f = reinterpret_cast<const float4_t*>(p); p += 4096;
            nw.W1b = reinterpret_cast<const float4_t*>(p); p += 4096;
            nw.W2f = reinterpret_cast<const float4_t*>(p); p += (int64_t)P * 4096;
            nw.W2b = reinterpret_cast<const float4_t*>(p); p += (int64_t)P * 4096;
            nw.z = p;
        }
    }
    rc = dev_alloc(m, &m->d_dev, 1);
    if (rc) return rc;
    WF_HIP(hipMemcpy(m->d_dev, &md, sizeof(ModelDev), hipMemcpyHostToDevice));
    rc = mfma_prepare(m, keep_i64, keep_p64, keep_o2b);
    if (rc) return rc;
    return grad_prepare(m);
}

// The wave-cooperative kernels (wf_kernels_wave.hip): <= 32 bases, constraints that only zero the end weights.
static bool wave_capable(const wf_model* m) {
    const wf_model_desc& d = m->desc;
    if (!m->d_wave) return false;
    const bool imade = d.layer_kind == WF_LAYER_IMADE && d.n_flow_layers > 0;
    if (imade && (!m->d_tabI4 || !m->bc_i_ok)) return false;
    const bool spline_prior = d.prior_kind == WF_PRIOR_WAVEFLOW || d.prior_kind == WF_PRIOR_MFLOW;
    if (spline_prior && (!m->d_tabP3 || !m->bc_p_ok)) return false;
    return true;
}
// ... which is also what the reverse pass and the local energy need (every D the library supports, 2..8, is instantiated)
static bool grad_capable(const wf_model* m) { return m->wave_ok && !m->nets.empty(); }   // (gated heads included: run_vjp_chunks)

static int grad_prepare(wf_model* m) {
    const wf_model_desc& d = m->desc;
    const int D = d.n_dim;
    std::vector<PackRec> plain;
    {
        int rc = pack_prepare(m, plain);
        if (rc) return rc;
    }
    m->wave_ok = wave_capable(m);
    if (m->wave_ok) {
        std::vector<float> fk(128, 0.0f), acc(64);
        if (d.layer_kind == WF_LAYER_IMADE && d.n_flow_layers > 0)
            row_factors(WF_SPLINE_I, true, d.i_degree, m->i_nb, m->nbp / 32, m->bc_i_colsum, acc.data(), fk.data());
        if (d.prior_kind == WF_PRIOR_WAVEFLOW) row_factors(WF_SPLINE_B, false, d.p_degree, m->p_nb, m->nbp / 32, m->bc_p_colsum, acc.data(), fk.data() + 64);
        if (d.prior_kind == WF_PRIOR_MFLOW) row_factors(WF_SPLINE_M, true, d.p_degree, m->p_nb, m->nbp / 32, m->bc_p_colsum, acc.data(), fk.data() + 64);
        int rc = dev_alloc(m, &m->d_grad_fk, fk.size());
        if (rc) return rc;
        WF_HIP(hipMemcpy(m->d_grad_fk, fk.data(), fk.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    if (m->wave_ok) {
        // scratch for the small-batch wave path (tails of up to kWaveEvalMax walkers, first or second order) is reserved here
        // so that those calls never allocate: they can be captured in a hipGraph
        int rc = ensure_scratch(m, kWaveEvalMax * std::max(wave_tail_floats(D, 0), wave_tail_floats(D, 1)));
        if (rc) return rc;
    }
    if (!grad_capable(m) || m->n_params >= (1 << 24)) return WF_OK;
    m->grad_psi_ok = d.prior_kind == WF_PRIOR_WAVEFLOW && (d.layer_kind == WF_LAYER_IMADE || d.n_flow_layers == 0);
    // One taped sample per walker in RF (value, gradient, Laplacian / 2: D + 2 channels), or D samples in R3 (3 channels each); 33 .. 64 bases
    // at D >= 5: R3 (second_order_rf, wf_internal.h).  Fixed per model, because workspace sizes depend on it; WF_GRAD_R3 (read here) selects R3 for A/B tests.
    m->ring2 = (env_grad_r3() || !second_order_rf(D, m->nbp)) ? 1 : 2;
    if (m->grad_psi_ok && m->mfma_ok && energy_vjp_capable(&m->mdev)) {
        int rc = dev_alloc(m, &m->d_egacc, (size_t)energy_vjp_gacc_floats((int)m->nets.size(), m->mdev.nbk));
        if (rc) return rc;
    }
    const int n_nets = (int)m->nets.size();
    const int64_t fwd = plain_fwd_floats(D, m->nbp);
    // the plain description lists net n's forward-orientation entries first (plain_net_floats per net)
    std::vector<int32_t> map((size_t)(fwd * n_nets));
    const int64_t per_net = plain_net_floats(D, m->nbp);
    for (int n = 0; n < n_nets; ++n)
        for (int64_t i = 0; i < fwd; ++i) map[(size_t)(fwd * n + i)] = plain[(size_t)(per_net * n + i)].src;
    // inverse: parameter -> its (unique) forward-image entry, -1 for parameters that reach none
    std::vector<int32_t> inv((size_t)std::max<int64_t>(m->n_params, 1), -1);
    for (size_t i = 0; i < map.size(); ++i)
        if (map[i] >= 0) inv[(size_t)map[i]] = (int32_t)i;
    int rc = dev_alloc(m, &m->d_grad_map, inv.size());
    if (rc) return rc;
    WF_HIP(hipMemcpy(m->d_grad_map, inv.data(), inv.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    if (m->dev.i_gate || m->dev.p_gate) {
        // zero_params gradient rows in the wave layout: row = (net * P + p) * 64 + lane  <->  leaf entry (d, jb) of that net
        const int P = wave_passes(D, m->nbp);
        const bool wide = m->nbp == 64;
        m->z_rows = n_nets * P * 64;
        std::vector<int32_t> zmap((size_t)m->z_rows, -1), zoff((size_t)m->z_rows, -1);
        for (int n = 0; n < n_nets; ++n) {
            const NetLayout& nl = m->nets[n];
            if (!nl.has_zero || !net_is_gated(m, n)) continue;
            const NetOffsets q = net_offsets(m, n);
            const bool sig = net_has_sigmoid_head(m, n);
            for (int p = 0; p < P; ++p)
                for (int c = 0; c < 64; ++c) {
                    const int dd = wide ? p : 2 * p + (c >> 5), jb = wide ? c : (c & 31);
                    if (dd >= D || jb >= nl.n_out) continue;
                    const size_t r = ((size_t)n * P + p) * 64 + c;
                    zmap[r] = (int32_t)(q.b2 + q.NO + (int64_t)dd * nl.n_out + jb);
                    if (sig) zoff[r] = (int32_t)(m->plain_off[n] + (m->dev.nets[n].zero_raw - m->dev.nets[n].W0) + (int64_t)dd * m->nbp + jb);
                }
        }
        rc = dev_alloc(m, &m->d_zmap, zmap.size());
        if (rc) return rc;
        WF_HIP(hipMemcpy(m->d_zmap, zmap.data(), zmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        rc = dev_alloc(m, &m->d_zraw_off, zoff.size());
        if (rc) return rc;
        WF_HIP(hipMemcpy(m->d_zraw_off, zoff.data(), zoff.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        // the inverse, over the flat vector: what the per-walker Jacobian (k_wjac) walks
        std::vector<int32_t> zinv((size_t)std::max<int64_t>(m->n_params, 1), -1);
        for (size_t r = 0; r < zmap.size(); ++r)
            if (zmap[r] >= 0) zinv[(size_t)zmap[r]] = (int32_t)r;
        rc = dev_alloc(m, &m->d_zinv, zinv.size());
        if (rc) return rc;
        WF_HIP(hipMemcpy(m->d_zinv, zinv.data(), zinv.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        rc = dev_alloc(m, &m->d_zpart, (size_t)64 * m->z_rows);
        if (rc) return rc;
        rc = dev_alloc(m, &m->d_zgrad, (size_t)m->z_rows);
        if (rc) return rc;
    }
    rc = dev_alloc(m, &m->d_grad_partial, (size_t)wgrad_partial_floats(n_nets, fwd));
    if (rc) return rc;
    return dev_alloc(m, &m->d_grad_img, map.size());
}

// fills every weight image from a device-resident flat vector (asynchronous on `stream`)
int apply_params(wf_model* m, const float* flat_dev, void* stream, bool eval_tables) {
    if (m->is_nsc) {   // the kernel reads the Dense leaves as they are: keep the model's own copy
        if (m->n_params > 0 && flat_dev != m->d_nsc)
            WF_HIP(hipMemcpyAsync(m->d_nsc, flat_dev, (size_t)m->n_params * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
        m->params_set = true;
        return WF_OK;
    }
    {
        int rc = launch_pack(flat_dev, m->d_pack, m->n_pack, m->d_plain, m->d_wave, m->d_mfma, stream);
        if (rc) return rc;
    }
    if (m->mfma_ok && eval_tables) {
        // biases of the layers behind a tanh: + column sums of their weights (the kernel's activations are r, tanh = 1 - 2r)
        int rc0 = launch_fold_bias(m->d_mfma, (int)m->nets.size(), m->mdev.net_floats, m->desc.n_dim, m->mdev.nbk, m->d_f16_ovf, stream);
        if (rc0) return rc0;
        // the flags follow the images to the host (not while the stream is being captured: a replayed step keeps the answer of its capture
        // and the kernels' own NaN poisoning is what shows)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing((hipStream_t)stream, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone) {
            WF_HIP(hipMemcpyAsync(m->h_f16_ovf, m->d_f16_ovf, m->nets.size() * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
            WF_HIP(hipEventRecord(m->ovf_event, (hipStream_t)stream));
            m->ovf_pending = true;
        }
        // composite tables of output dimension 0 (reads the plain image filled above)
        int rc = launch_prepare_dim0(m->d_dev, (int)m->nets.size(), m->desc.n_mesh, m->d_fk_nat, m->mdev.F_I, m->mdev.F_P, m->d_tabI4, m->d_tabP3, m->d_comp, stream);
        if (rc) return rc;
    }
    if (m->mfma_ok) m->eval_tables_stale = !eval_tables;
    m->params_set = true;
    return WF_OK;
}

// Is a packed weight of the current parameters outside the fp16 range?  Then every path that feeds fp16 operand images to the matrix cores
// (k_mfma, the tile kernels of wf_kernels_etile.hip) is off: `auto` takes the fp32 scalar / wave kernels, an explicit request for the MFMA
// kernel returns WF_ERR_UNSUPPORTED.  Waits for the upload's flag copy if it is still in flight (a host wait of the pack kernels, ~50 us,
// only in the call that follows an asynchronous upload).
bool f16_overflow(const wf_model* cm) {
    wf_model* m = const_cast<wf_model*>(cm);
    if (!m->mfma_ok) return false;
    if (m->ovf_pending) {
        if (hipEventSynchronize(m->ovf_event) != hipSuccess) return true;
        m->ovf_pending = false;
        bool any = false;
        for (size_t n = 0; n < m->nets.size(); ++n) any |= m->h_f16_ovf[n] != 0;
        m->f16_overflow = any;
    }
    return m->f16_overflow;
}

}  // namespace wf

// ------------------------------------------------------------------------------------------ C ABI
using namespace wf;

extern "C" {

int wf_model_create(const wf_model_desc* desc, int device, wf_model** out) {
    if (!desc || !out) return WF_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return WF_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return WF_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return WF_ERR_NO_DEVICE;
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) return WF_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return WF_ERR_NO_DEVICE;
    wf_model* m = new (std::nothrow) wf_model();
    if (!m) return WF_ERR_NOMEM;
    m->desc = *desc;
    m->device = device;
    int rc;
    try {
        rc = model_build(m);
    } catch (const std::bad_alloc&) {
        rc = WF_ERR_NOMEM;
    }
    if (rc != WF_OK) {
        wf_model_destroy(m);
        return rc;
    }
    *out = m;
    return WF_OK;
}

void wf_model_destroy(wf_model* m) {
    if (!m) return;
    DeviceGuard g(m->device);
    for (void* p : m->allocs) (void)hipFree(p);
    if (m->ovf_event) (void)hipEventDestroy(m->ovf_event);
    if (m->h_f16_ovf) (void)hipHostFree(m->h_f16_ovf);
    delete m;
}

int64_t wf_model_param_count(const wf_model* m) { return m ? m->n_params : WF_ERR_INVALID; }

int wf_model_n_bases(const wf_model* m, int which) {
    if (!m) return WF_ERR_INVALID;
    return which == 0 ? m->i_nb : m->p_nb;
}

int wf_model_set_kernel(wf_model* m, int kernel_kind) {
    if (!m || kernel_kind < WF_KERNEL_AUTO || kernel_kind > WF_KERNEL_WAVE) return WF_ERR_INVALID;
    if (kernel_kind == WF_KERNEL_MFMA && !m->mfma_ok) return WF_ERR_UNSUPPORTED;
    if (kernel_kind == WF_KERNEL_WAVE && !m->wave_ok) return WF_ERR_UNSUPPORTED;
    m->kernel_kind = kernel_kind;
    return WF_OK;
}

int wf_model_set_params(wf_model* m, const float* flat_host, int64_t n, void* stream) {
    if (!m || !flat_host) return WF_ERR_INVALID;
    if (n != m->n_params) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    hipStream_t s = (hipStream_t)stream;
    if (n > 0) WF_HIP(hipMemcpyAsync(m->d_flat, flat_host, (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    int rc = apply_params(m, m->d_flat, stream);
    if (rc) return rc;
    WF_HIP(hipStreamSynchronize(s));   // the caller may reuse flat_host
    return WF_OK;
}

int wf_model_set_params_device(wf_model* m, const float* flat_dev, int64_t n, void* stream) {
    if (!m || !flat_dev) return WF_ERR_INVALID;
    if (n != m->n_params) return WF_ERR_INVALID;
    DeviceGuard g(m->device);
    return apply_params(m, flat_dev, stream);   // the images are packed straight from the caller's vector (m->d_flat only stages host uploads)
}

}  // extern "C"
