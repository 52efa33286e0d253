/*
 * trs_compliance.h - compliance sizing: the stiffest design at a given weight (or volume), the optimality-criteria
 * method iterated on the device (csrc/compliance.hip; the entry points live in libtrs_hip.so beside those of
 * trs_solver.h and trs_sizing.h, whose conventions hold here word for word: every pointer is a DEVICE pointer owned by
 * the caller, the library allocates nothing, every call only enqueues work on `stream` (a hipStream_t passed as void*)
 * and returns 0 or a hipError_t, there is no process-wide state that a result depends on, no floating-point atomic is
 * used and every sum runs in one fixed order - the results are bit-reproducible from run to run and from stream to
 * stream, and the numbers of truss b do not depend on B or on the other trusses; every kernel trims nJ[b], nM[b] and
 * n_free[b] to the arrays and clamps end-joint ids to them through the truss view (csrc/trs_view.h): whatever the
 * inputs hold, nothing is read or written outside the arrays).
 *
 * The method (the numpy yardstick tests/compliance_reference.py and the kernel state it in the same words).  Inputs: L
 * load cases (joint forces), weights alpha[L], each >= 0 and not all zero; the measure: "weight" gives w_m = rho_m L0_m,
 * "volume" gives w_m = L0_m; the target W > 0 per truss; eta in (0, 1]; move in (0, 1]; per member a_min > 0 and
 * a_max >= a_min (equal bounds fix a member); tol >= 0 and max_iters >= 0.  The initial design is the batch's own A
 * (> 0).  Analysis k (k = 0, 1, ...) of design A = A_k:
 *   - proj_ml = c_m.(u_l,j1 - u_l,j0);
 *   - C_l = sum_m (E_m A_m / L0_m) proj_ml^2: the compliance as twice the strain energy (f_l.u_l but for rounding);
 *   - J = sum_l alpha_l C_l, summed in ascending l;
 *   - s_m = sum_l alpha_l (E_m / L0_m) proj_ml^2, summed in ascending l: -dJ/dA_m;
 *   - lo_m = clamp((1 - move) A_m, a_min_m, a_max_m) and hi_m = clamp((1 + move) A_m, a_min_m, a_max_m);
 *   - a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m);
 *   - p_m = A_m (s_m / w_m)^eta (0 for a member with w_m <= 0);
 *   - t_m(x) = min(max(p_m x, lo_m), hi_m);
 *   - V(x) = sum_m w_m t_m(x), non-decreasing in x; eta enters only through p_m: the search below needs no pow;
 *   - the new design A', with x0 = min and x1 = max over the members with p_m > 0 of lo_m / p_m and hi_m / p_m:
 *       sum w lo >= W                A' = lo       multiplier 0
 *       sum w hi <= W                A' = hi       multiplier 0
 *       no member has p_m > 0        A' = lo       multiplier 0
 *       V(x1) <= W                   A' = t(x1)    multiplier x1^(-1/eta)
 *       otherwise                    A' = t(x0) after the bisection below, multiplier x0^(-1/eta)
 *     (the first line that applies);
 *   - the bisection runs 64 times: xm = sqrt(x0 x1); if V(xm) <= W then x0 = xm, else x1 = xm;
 *   - change = max_m |A'_m - A_m| / A_m over the truss's live members;
 *   - if change <= tol the truss is converged (status 0) and keeps A_k;
 *   - otherwise, if k = max_iters, the truss gets status 1 and keeps A_k;
 *   - otherwise A_{k+1} = A' and the truss's `iterations` becomes k + 1;
 *   - if the factorisation of A_k reports info != 0 the truss gets status 2, its design goes back to A_{k-1}, and its
 *     outputs (iterations among them) stay those of analysis k - 1; for k = 0 the outputs are zero (nothing was
 *     analysed), the areas are the initial ones and `iterations` is 0.
 * The status is sticky, exactly as in trs_sizing.h: once a truss has left TRS_CM_ACTIVE nothing changes its areas or its
 * outputs, so its results depend neither on B nor on the other trusses, nor on how often the host looks at `active`,
 * nor on max_iters beyond its own count.  (The caller goes on assembling and factoring a frozen truss with its
 * unchanged design: the same bits.)
 *
 * One iteration is five launches, the last of them here: trs_assemble and trs_potrf_batched of the design A_k,
 * trs_gather_cases, trs_potrs_cases (trs_solver.h, unchanged; the substitution overwrites its right-hand sides, so the
 * gather is repeated), trs_cm_step.  The step reads the L reduced solutions straight from the case block [B][L][ld_f]
 * that trs_potrs_cases left: there is no trs_recover_cases, and neither u nor N per case goes to HBM.  The
 * sensitivities are the members' own strain energies: no adjoint solve, no virtual load case.
 *
 * State of a run (device; the caller allocates and ZEROES it before analysis 0):
 *   prev    double [B][nM_max]   the design before the last resizing (what a truss of status 2 goes back to)
 *   st      int32  [B][4]        (status, iterations, info latched with status 2 - 0 until then -, reserved); the
 *                                status codes: TRS_CM_ACTIVE -1 (inside a run only), 0 converged, 1 iteration limit,
 *                                2 the design could not be factored
 *   active  int32, one word per analysis: += 1 for every truss that is still active after the call
 *   target  double [B]           W; an entry <= 0 is replaced at analysis 0 by the measure of the initial design, and
 *                                the kernel writes it back
 * Outputs per truss, all describing the last design analysed with info == 0, in the CALLER's member order (a joint
 * order renumbers joints only, and nothing here is per joint, so the step takes no joint_out):
 *   areas [B][nM_max]; measure [B] = sum w A; compliance [B][L] = C_l; objective [B] = J; objective_history [B][H]: J of
 *   every design the truss analysed, entry k by analysis k (the caller zeroes it: zero beyond the truss's own count);
 *   sensitivity [B][nM_max] = s_m; multiplier [B] of this analysis's resizing.  Padding members get zeros.
 * Every sum - C_l, the measure, sum w lo, sum w hi, V(x) - runs in one order: every thread adds its members tid,
 * tid + 256, ... in ascending m (V(x) by fma(w, t, sum)), the 64 partials of a wave are folded by the butterfly
 * lane ^ 32, ^ 16, ... ^ 1 and the four waves' sums are added in wave order.  x0, x1 and the change are extremes, exact
 * in any order.  After a run the slab holds the factor of the returned design for every truss of status 0 or 1.
 *
 * trs_cm_step, analysis `it` (0 <= it) with `mode`: 0 iterate; 1 the iteration limit: a truss that is not converged
 * gets status 1 instead of a new design.  With it = 0 the run begins: every truss becomes active with 0 iterations.
 * Only active trusses are touched.  An active truss writes its outputs at EVERY analysis (that is what a truss of
 * status 2 falls back on): there is no report call at the end of a run.
 *
 * The kernel.  One 256-thread work-group per truss, one launch per analysis.  A thread owns the members tid, tid + 256,
 * ...: their geometry (c, E A / L0, E / L0, w) is formed ONCE ahead of the case loop and kept in LDS with the running
 * sensitivity; one case's displacement vector at a time is staged in LDS through the view's row_of (held DOFs read 0),
 * double-buffered: one barrier per case.  The bisection evaluates `levels` (1, 2 or 3; 0: the library's choice) levels
 * of the search tree per round - with two levels m1 = sqrt(x0 x1), m0 = sqrt(x0 m1) and m2 = sqrt(m1 x1) are summed
 * together and the round takes the two decisions the definition takes - with one barrier per round: the same bits for
 * every value of `levels`.  Where a thread owns at most four members (nM_max <= 1024) their p, lo, hi and w stay in
 * registers through the bisection; the library's choice is then one level per round, else two (as measured).
 * LDS per work-group (trs_cm_fits): two displacement vectors (6 nJ_max doubles), 64 doubles for the reductions, seven
 * doubles and two ints per member, the reduced row of every DOF (3 nJ_max ints): 60 nJ_max + 512 + 64 nM_max bytes,
 * rounded up to 16, within 160 KB.  (bar-942, 244 joints: 75 440 bytes, two work-groups per CU.)
 *
 * General member form only, for the reason trs_sizing.h gives: the kernel WRITES areas, one per member, which a type
 * table cannot hold - there is no `_tab` twin; convert a table-form batch first.
 */
#ifndef TRS_COMPLIANCE_H
#define TRS_COMPLIANCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_CM_ABI_VERSION 1

#define TRS_CM_ACTIVE (-1)
#define TRS_CM_CONVERGED 0
#define TRS_CM_ITER_LIMIT 1
#define TRS_CM_NOT_PD 2

#define TRS_CM_WEIGHT 0
#define TRS_CM_VOLUME 1

#define TRS_CM_BISECTIONS 64

int trs_cm_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS (see above; otherwise trs_cm_step returns
 * hipErrorInvalidValue). */
int trs_cm_fits(int nJ_max, int nM_max);

/* xyz, conn, E, rho, free_index, n_free, nJ, nM: the batch's arrays as assembled; A [B][nM_max]: the design, resized in
 * place; F [B][L][ld_f]: the case block as trs_potrs_cases left it; info [B]: of the factorisation of this design;
 * alpha [L] (device; the library cannot look at device values: the caller has checked them); measure: TRS_CM_WEIGHT or
 * TRS_CM_VOLUME; target [B], read and (see above) written; a_min / a_max: [B][nM_max], or NULL for the scalar beside
 * it; objective_history [B][H] (entry `it` is written when it < H). */
int trs_cm_step(int B, int L, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E, double *A,
                const double *rho, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ, const int32_t *nM,
                const double *F /* [B][L][ld_f] */, int ld_f, const int32_t *info, const double *alpha /* [L] */,
                int measure, double *target /* [B] */, double eta, double move, double tol,
                const double *a_min /* [B][nM_max] or NULL */, double a_min_all,
                const double *a_max /* [B][nM_max] or NULL */, double a_max_all, int it, int mode, int levels,
                double *prev /* [B][nM_max] */, int32_t *st /* [B][4] */, int32_t *active /* one word */, double *areas,
                double *measure_out, double *compliance /* [B][L] */, double *objective, double *objective_history,
                int H, double *sensitivity, double *multiplier, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_COMPLIANCE_H */
