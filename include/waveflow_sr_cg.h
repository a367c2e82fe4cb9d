/*
 * waveflow_sr_cg.h -- the B x B solve of waveflow_sr.h without the B x B matrix: preconditioned conjugate gradients on (Tbar + lambda I) y = rhs,
 * Tbar applied as two passes over the Jacobian rows, for batches beyond the 4096 walkers of wf_sr_solve.  Part of libwaveflow_hip.so; conventions,
 * error codes and WF_ABI_VERSION are those of waveflow_hip.h; notation is that of waveflow_sr.h.  Model-free, like the entries there.
 *
 * With the rows O (fp32 [B][P]), H = I - 1 1^T / B, obar[k] = (1 / B) sum_b O[b][k] and a B-vector v:
 *     pass A     z[k] = sum_b (v[b] - mean v) O[b][k]                                   fp64 [P]
 *     pass B     q[b] = sum_k O[b][k] z[k]                                              fp64 [B]
 *     Tbar v   = (q - mean q) / B,        v^T Tbar v = |z|^2 / B   (exact algebra: Tbar = H O O^T H / B)
 *     diag[b]  = (1 / B) sum_k (O[b][k] - obar[k])^2 = Tbar[b][b],     trace(Tbar) = sum_b diag[b]
 *     lambda   = damping_abs + damping_rel * trace(Tbar) / B          (the shift of wf_sr_solve)
 *     M        = diag + lambda (precondition != 0: Jacobi) or 1
 * and the recurrences, all in fp64 (A = Tbar + lambda I):
 *     start      y = 0, r = rhs, p = r / M, rho = r^T p, it = 0
 *     iteration  zz = |z|^2 with z = pass A of p;  q = pass B of z
 *                pAp = zz / B + lambda p^T p;  alpha = rho / pAp
 *                y += alpha p;  r -= alpha ((q - mean q) / B + lambda p);  it += 1
 *                converged when r^T r <= tol^2 rhs^T rhs; otherwise
 *                rho' = r^T (r / M);  p = r / M + (rho' / rho) p;  rho = rho'
 *
 * Orders of summation (each depends on B and P alone, so every result is bitwise reproducible; no floating-point atomics):
 *   - pass A: rows in chunks of 32; a chunk's partial sums its rows first row first, one fp64 multiply and one add per row (fp32 entries convert
 *     exactly); z[k] adds the chunk partials chunk 0 first.  obar is pass A with v = 1 and no centring, times 1 / B.
 *   - pass B and diag: one workgroup of 256 threads per 4 rows; thread t takes columns 4 t .. 4 t + 3, then + 1024, ... into four sums (one per
 *     column of its group), ((s0 + s1) + (s2 + s3)), then a binary tree over the 256 threads (stride 128, 64, ... 1).
 *   - zz: per 256 entries of z a tree over the squares; the partials are then added like a B-vector below.
 *   - every sum over a B-vector (mean v, mean q, p^T p, r^T r, r^T (r / M), trace, rhs^T rhs) and the sum of the zz partials: one workgroup of
 *     1024 threads; thread t adds entries t, t + 1024, ... in that order, then a binary tree over the 1024 threads.
 *
 * Nothing here waits for the host, allocates or copies: a call enqueues a fixed sequence of launches on `stream` (4 per iteration), every kernel of
 * which first reads the status word in the workspace and returns at once when the solve has finished, so the same sequence serves any convergence
 * point and can be captured in a graph.
 */
#ifndef WAVEFLOW_SR_CG_H
#define WAVEFLOW_SR_CG_H

#include "waveflow_sr_spring.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace wf_sr_cg_solve needs for B rows of P columns: a control block (status word, iteration count, rho, rhs^T rhs, r^T r, lambda,
 * mean p), the fp64 B-vectors r, p, q and diag, fp64 z [P] and obar [P], the zz partials and the chunk partials of pass A
 * (ceil(B / 32) x P fp64).  It is at least the workspace of wf_sr_apply for the same B and P.  WF_ERR_INVALID for B < 1 or P < 1,
 * WF_ERR_UNSUPPORTED for B > 65536 (the limit of the row passes of waveflow_sr.h). */
int64_t wf_sr_cg_workspace_bytes(int64_t B, int64_t P);

/* (Tbar + lambda I) y = rhs by the recurrences at the head of this file.  rows_dev: fp32 [B][ld], ld >= P, only read (16-byte loads along p where
 * base and ld allow them; every row is read once per pass); rhs_dev: fp64 [B], only read, already centred (wf_spring_rhs, or H e).
 * restart != 0: obar, diag, lambda and the start of the recurrences, then n_iter iterations.  restart == 0: n_iter more iterations from what the
 * workspace holds -- rows_dev, rhs_dev, y_dev, workspace_dev and precondition must be those of the call that started the solve (rhs_dev, the
 * dampings are not read then).
 * y_dev: fp64 [B], the current iterate.  info_dev: fp64 [4] = status, iterations done, sqrt(r^T r / rhs^T rhs) of the recurrence's r, lambda;
 * written by every call.  status:
 *   0  converged: r^T r <= tol^2 rhs^T rhs.  rhs == 0 converges at once: y = 0, no iteration.  B == 1 (Tbar = 0): y = rhs / lambda, no iteration.
 *   1  not yet converged; y_dev holds the iterate after `iterations` steps
 *   2  a value that is not finite (trace, rhs^T rhs, pAp or r^T r), lambda not positive, or a breakdown pAp <= 0: y_dev is filled with NaN
 * After status 0 or 2 further calls with restart == 0 change neither y_dev, nor info_dev's values, nor the workspace.
 * WF_ERR_INVALID: B < 1, P < 1, ld < P, a damping that is negative (or NaN), tol not in (0, 1), n_iter < 0, a NULL pointer, workspace_bytes below
 * wf_sr_cg_workspace_bytes(B, P).  B > 65536: WF_ERR_UNSUPPORTED.  Numerical trouble is never a return value: it is status 2, on the device. */
int wf_sr_cg_solve(const float* rows_dev, int64_t B, int64_t P, int64_t ld, const double* rhs_dev, double damping_abs, double damping_rel, double tol,
                   int32_t n_iter, int32_t restart, int32_t precondition, double* y_dev, double* info_dev, void* workspace_dev, int64_t workspace_bytes,
                   void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WAVEFLOW_SR_CG_H */
