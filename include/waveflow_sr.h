/*
 * waveflow_sr.h -- stochastic reconfiguration (the natural gradient of variational Monte Carlo) from per-walker
 * Jacobian rows, in its B x B ("minSR") form.  Part of libwaveflow_hip.so; conventions, error codes and
 * WF_ABI_VERSION are those of waveflow_hip.h.  The entries are model-free: they take the rows wf_psi_jac wrote
 * (or any other fp32 matrix) and know nothing of the wave function.
 *
 * With O[b][k] = d ln psi_b / d theta_k (B walkers, P parameters), local energies e, the centring matrix
 * H = I - 1 1^T / B and a shift lambda > 0, the parameter-space update
 *     S = O^T H O / B,   g = (2 / B) O^T H e,   d = (S + lambda I)^-1 g
 * equals (push-through identity)
 *     Tbar = H (O O^T) H / B,   (Tbar + lambda I) y = H e,   d = (2 / B) O^T (H y),
 * which needs a B x B matrix instead of a P x P one: wf_sr_gram, wf_sr_solve, wf_sr_apply.  The rows are read
 * twice and never centred or rewritten; the centring happens on the B x B matrix and on B-vectors in fp64.
 * Every result is bitwise reproducible: fixed-order fp64 sums, no floating-point atomics.
 *
 * All three device entries share one workspace of wf_sr_workspace_bytes(B, P) bytes; none synchronises with the host.
 */
#ifndef WAVEFLOW_SR_H
#define WAVEFLOW_SR_H

#include "waveflow_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace wf_sr_gram, wf_sr_solve and wf_sr_apply need for B rows of P columns (the largest of the three);
 * WF_ERR_INVALID for B < 1 or P < 1. */
int64_t wf_sr_workspace_bytes(int64_t B, int64_t P);

/* t_dev[B][B] (fp64, full and exactly symmetric) = H G H / B with G[a][b] = sum_{k < P} rows[a][k] rows[b][k] and
 * H = I - 1 1^T / B, i.e. (G[a][b] - mean_b G[a][.] - mean_a G[.][b] + mean G) / B.  rows_dev: fp32 [B][ld], ld >= P,
 * only the first P columns of a row are read.  The products run on the fp64 matrix cores (fp32 operands convert
 * exactly, every product is exact in fp64); the P axis is split into fixed-size chunks whose fp64 partial tiles are
 * summed in a fixed order. */
int wf_sr_gram(const float* rows_dev, int64_t B, int64_t P, int64_t ld, double* t_dev, void* workspace_dev, int64_t workspace_bytes,
               void* stream);

/* In place: the lower triangle of t_dev[B][B] + lambda I, lambda = damping_abs + damping_rel * trace(t) / B, is overwritten
 * by its lower Cholesky factor L (the strict upper triangle is left as it was), then y_dev[B] = (L L^T)^-1 rhs_dev (fp64; rhs_dev
 * is only read).  info_dev[0] (int32) = 0, or the 1-based index of the first pivot that is not positive (LAPACK's potrf):
 * the factorisation stops there and y_dev is filled with NaN.  Trace, shift and pivot test run on the device.
 * B <= 4096 (beyond: WF_ERR_UNSUPPORTED); damping_abs, damping_rel >= 0. */
int wf_sr_solve(double* t_dev, int64_t B, const double* rhs_dev, double damping_abs, double damping_rel, double* y_dev, int32_t* info_dev,
                void* workspace_dev, int64_t workspace_bytes, void* stream);

/* out_dev[p] (fp32, p < P) = scale * sum_b (y[b] - mean y) rows[b][p]: the product O^T (H y), accumulated in fp64 in a fixed
 * order and rounded to fp32 once.  rows_dev as in wf_sr_gram (read once, 16-byte loads along p where base and ld allow them). */
int wf_sr_apply(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const double* y_dev, double scale, float* out_dev,
                void* workspace_dev, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_SR_H */
