/*
 * trs_sizing.h - member sizing: fully stressed design with a displacement envelope (the stress-ratio method), iterated
 * on the device (csrc/sizing.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h, whose
 * conventions hold here word for word: every pointer is a DEVICE pointer owned by the caller, the library allocates
 * nothing, every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t,
 * there is no process-wide state that a result depends on, no floating-point atomic is used and every sum runs in one
 * fixed order - the results are bit-reproducible from run to run and from stream to stream, and the numbers of truss b
 * do not depend on B or on the other trusses; every kernel trims nJ[b], nM[b] and n_free[b] to the arrays and clamps
 * end-joint ids to them through the truss view (csrc/trs_view.h): whatever the inputs hold, nothing is read or written
 * outside the arrays).
 *
 * The method (the numpy yardstick tests/sizing_reference.py and the kernel state it in the same words).  Inputs: L load
 * cases (joint forces), the scalars (the three allowables per batch or per truss) allow_tension > 0, allow_compression > 0, allow_displace (0 = no limit),
 * euler_kappa >= 0 (the member's second moment of area as I = kappa A^2, 1/(4 pi) for a solid round bar, 0 = no member
 * buckling check), relax in (0, 1], tol >= 0, max_iters >= 0, and per member a_min > 0 and a_max >= a_min (equal bounds
 * fix a member).  The initial design is the batch's own A (> 0).  Analysis k (k = 0, 1, ...) of design A_k:
 *   - for each case l, N_ml = (E A_k / L0) c.(u_j1 - u_j0);
 *   - the required area in case l is N / allow_tension for N > 0; for P = -N > 0 it is
 *     max(P / allow_compression, sqrt(P L0^2 / (pi^2 E kappa))), the second term only when kappa > 0;
 *   - req_m is the maximum over the cases, taken in ascending l; on a tie the lowest l governs;
 *   - d = max over cases and the truss's joints of |u_j| / allow_displace; 0 without a limit;
 *   - r_m = max(req_m / A_m, d);
 *   - A'_m = clamp(A_m ((1 - relax) + relax r_m), a_min_m, a_max_m);
 *   - change = max_m |A'_m - A_m| / A_m over the truss's live members;
 *   - if change <= tol the truss is converged (status 0) and keeps A_k;
 *   - otherwise, if k = max_iters, the truss gets status 1 and keeps A_k;
 *   - otherwise A_{k+1} = A' and the truss's `iterations` becomes k + 1;
 *   - if the factorisation of A_k reports info != 0 the truss gets status 2, its design goes back to A_{k-1}, and its
 *     outputs (iterations among them) stay those of analysis k - 1; for k = 0 the outputs are zero (governing -1: nothing
 *     was analysed), the areas are the initial ones and `iterations` is 0.
 * No thresholds on small forces: a zero-force member has r = d and ends on its lower bound.
 * The status is sticky, exactly as in trs_nonlinear.h: once a truss has left TRS_SZ_ACTIVE nothing changes its areas or
 * its outputs, so its results depend neither on B nor on the other trusses, nor on how often the host looks at
 * `active`, nor on max_iters beyond its own count.  (The caller goes on assembling and factoring a frozen truss with
 * its unchanged design: the same bits.)
 *
 * One iteration is five launches, the last of them here: trs_assemble and trs_potrf_batched of the design A_k,
 * trs_gather_cases, trs_potrs_cases (trs_solver.h, unchanged; the substitution overwrites its right-hand sides, so the
 * gather is repeated), trs_sz_step.  The step reads the L reduced solutions straight from the case block
 * [B][L][ld_f] that trs_potrs_cases left: there is no trs_recover_cases, and neither u nor N per case goes to HBM.
 *
 * State of a run (device; the caller allocates and ZEROES it before analysis 0):
 *   prev    double [B][nM_max]   the design before the last resizing (what a truss of status 2 goes back to)
 *   st      int32  [B][4]        (status, iterations, info latched with status 2 - 0 until then -, reserved); the
 *                                status codes: TRS_SZ_ACTIVE -1 (inside a run only), 0 converged, 1 iteration limit,
 *                                2 the design could not be factored
 *   active  int32, one word per analysis: += 1 for every truss that is still active after the call
 * Outputs per truss, all describing the last design analysed with info == 0, in the CALLER's member order (a joint
 * order - trs_joint_order, trs_apply_joint_order - renumbers joints only: "members keep their order", trs_solver.h;
 * nothing here is per joint, so the step takes no joint_out):
 *   areas [B][nM_max]; weight [B] = sum A L0 rho (every thread adds its members tid, tid + 256, ... in ascending m, the
 *   64 partials of a wave are folded by the butterfly lane ^ 32, ^ 16, ... ^ 1 and the four waves' sums are added in
 *   wave order); utilisation [B][nM_max] = req_m / A_m (stress and member buckling only; <= 1 is feasible); governing
 *   int32 [B][nM_max]: the case l whose requirement governs r_m, or -1 where the displacement ratio does (d > req_m /
 *   A_m); disp_ratio [B] = d; weight_history [B][H]: the weight of every design the truss analysed, entry k by
 *   analysis k (the caller zeroes it: zero beyond the truss's own count).  Padding members get zeros, governing -1.
 *
 * trs_sz_step, analysis `it` (0 <= it) with `mode`:
 *   0  iterate;
 *   1  the iteration limit: a truss that is not converged gets status 1 instead of a new design;
 *   2  report only (the catalogue pass): every truss of status 0 or 1 whose info is 0 gets its outputs rewritten for
 *      the design A it holds now - no status, no count, no area and no history entry changes; a truss of status 0 or 1
 *      whose info is NOT 0 keeps its outputs and gets that info latched.
 * With mode 0 or 1 and it = 0 the run begins: every truss becomes active with 0 iterations.  Only active trusses are
 * touched.  An active truss writes its outputs at EVERY analysis (that is what a truss of status 2 falls back on), so a
 * host that has seen that no truss is active has nothing left to ask for: there is no report call at the end of a run.
 *
 * The kernel.  One 256-thread work-group per truss, one launch per analysis.  A thread owns the members tid, tid + 256,
 * ...: their geometry (c, E A / L0, the Euler coefficient L0^2 / (pi^2 E kappa)) is formed ONCE ahead of the case loop
 * and kept in LDS with the running requirement and its case; one case's displacement vector at a time is staged in LDS
 * through the view's row_of (held DOFs read 0), double-buffered: one barrier per case.  The displacement ratio and the
 * change are work-group maxima, exact in any order.
 * LDS per work-group (trs_sz_fits): two displacement vectors (6 nJ_max doubles), eight doubles for the reductions, six
 * doubles and three ints per member, the reduced row of every DOF (3 nJ_max ints): 60 nJ_max + 64 + 60 nM_max bytes,
 * rounded up to 16, within 160 KB.
 *
 * General member form only: the kernel WRITES areas, one per member, which a type table (<= 256 shared triples) cannot
 * hold - there is no `_tab` twin; convert a table-form batch first.
 *
 * trs_sz_snap, the catalogue pass over the areas: `catalog` [T] ascending, 1 <= T <= 256.  Every live member of a truss
 * of status 0 or 1 goes to the smallest catalogue area >= its area, the largest where there is none, and its index goes
 * to catalog_index (uint8 [B][nM_max]); everything else gets index 0 and keeps its area.  ONE more analysis (assemble
 * ... trs_sz_step with mode 2) then rewrites those trusses' outputs.
 */
#ifndef TRS_SIZING_H
#define TRS_SIZING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_SZ_ABI_VERSION 1

#define TRS_SZ_ACTIVE (-1)
#define TRS_SZ_CONVERGED 0
#define TRS_SZ_ITER_LIMIT 1
#define TRS_SZ_NOT_PD 2

#define TRS_SZ_MAX_CATALOG 256

int trs_sz_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS (see above; otherwise trs_sz_step returns
 * hipErrorInvalidValue). */
int trs_sz_fits(int nJ_max, int nM_max);

/* xyz, conn, E, rho, free_index, n_free, nJ, nM: the batch's arrays as assembled; A [B][nM_max]: the design, resized in
 * place; F [B][L][ld_f]: the case block as trs_potrs_cases left it; info [B]: of the factorisation of this design;
 * allow: [B][3] = (allow_tension, allow_compression, allow_displace) per truss, or NULL for the three scalars (the
 * library cannot look at device values: the caller has checked them); a_min / a_max: [B][nM_max], or NULL for the
 * scalar beside it; weight_history [B][H] (entry `it` is written when it < H). */
int trs_sz_step(int B, int L, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E, double *A,
                const double *rho, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ, const int32_t *nM,
                const double *F /* [B][L][ld_f] */, int ld_f, const int32_t *info, double allow_tension,
                double allow_compression, double allow_displace, const double *allow /* [B][3] or NULL */,
                double euler_kappa, double relax, double tol,
                const double *a_min /* [B][nM_max] or NULL */, double a_min_all,
                const double *a_max /* [B][nM_max] or NULL */, double a_max_all, int it, int mode,
                double *prev /* [B][nM_max] */, int32_t *st /* [B][4] */, int32_t *active /* one word */, double *areas,
                double *weight, double *utilisation, int32_t *governing, double *disp_ratio, double *weight_history,
                int H, void *stream);

int trs_sz_snap(int B, int nM_max, const int32_t *nM, const int32_t *st /* [B][4] */, const double *catalog /* [T] */,
                int T, double *A /* [B][nM_max] */, uint8_t *catalog_index /* [B][nM_max] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_SIZING_H */
