/*
 * trs_minweight.h - minimum weight under displacement limits: the lightest design whose named joint displacements stay
 * within named limits, the optimality-criteria method with one multiplier per limit, iterated on the device
 * (csrc/minweight.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h, trs_sizing.h and
 * trs_compliance.h, whose conventions hold here word for word: every pointer is a DEVICE pointer owned by the caller, the
 * library allocates nothing, every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or
 * a hipError_t, there is no process-wide state that a result depends on, no floating-point atomic is used and every sum
 * runs in one fixed order - the results are bit-reproducible from run to run and from stream to stream, and the numbers
 * of truss b do not depend on B or on the other trusses; every kernel trims nJ[b], nM[b] and n_free[b] to the arrays and
 * clamps end-joint ids to them through the truss view (csrc/trs_view.h), and a limit whose joint or case lies outside
 * the truss is switched off: whatever the inputs hold, nothing is read or written outside the arrays).
 *
 * The method (the numpy yardstick tests/minweight_reference.py and the kernel state it in the same words).  Inputs: L
 * load cases (joint forces); J limits, 1 <= J <= TRS_MW_MAX_LIMITS = 8, limit j naming a case l_j (shared by the batch),
 * per truss a joint, a direction d_j of unit length (normalised by the host) and a value ubar_j > 0, and meaning
 * d_j.u_{l_j}(joint) <= ubar_j (a two-sided limit is two limits with +-d); an infinite value or a joint of -1 switches
 * a limit off for that truss; the measure: "weight" gives w_m = rho_m L0_m, "volume" gives w_m = L0_m; move in (0, 1];
 * per member a_min > 0 and a_max >= a_min (equal bounds fix a member); tol >= 0, max_iters >= 0, sweeps >= 1 and
 * limit_tol >= 0.  The initial design is the batch's own A (> 0).  Analysis k (k = 0, 1, ...) of design A = A_k:
 *   - the case block holds L + J columns: the real cases, then the unit loads d_j at the limits' joints, with solutions
 *     v_j (a limit that is switched off has a zero column);
 *   - proj_m(x) = c_m.(x_j1 - x_j0);
 *   - c_mj = (E_m / L0_m) proj_m(v_j) proj_m(u_{l_j}) = -dg_j/dA_m;
 *   - g_j = d_j.u_{l_j}(joint), summed in ascending component (0 for a limit that is switched off);
 *   - q_mj = max(c_mj, 0) A_m^2 and n_mj = max(-c_mj, 0) where |c_mj| A_m > 2^-30 max_m |c_mj| A_m, else q_mj = n_mj = 0
 *     (a member off the limit's load path: where a step cannot reach a limit every member with q > 0 goes to hi and
 *     every member with n > 0 to lo, which must not hang on the SIGN of the rounding noise in a c_mj that is zero);
 *   - lo_m = clamp((1 - move) A_m, a_min_m, a_max_m) and hi_m = clamp((1 + move) A_m, a_min_m, a_max_m);
 *   - a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m);
 *   - the subproblem: minimise sum_m w_m A'_m subject to gt_j(A') = sum_m (q_mj / A'_m - n_mj A'_m) <= ubar_j and
 *     lo <= A' <= hi (the convex linearisation: reciprocal in A where c > 0, linear where c < 0);
 *   - at multipliers mu >= 0, P_m = sum_j mu_j q_mj and D_m = w_m + sum_j mu_j n_mj, both summed in ascending j;
 *   - A'_m(mu) = clamp(sqrt(P_m / D_m), lo_m, hi_m), and lo_m where P_m <= 0; gt_j never rises in mu_j;
 *   - the dual solve: mu starts from the previous analysis (zeros at analysis 0) and takes `sweeps` passes over
 *     j = 0 .. J - 1 (a limit that is switched off keeps mu_j = 0), the other multipliers held fixed:
 *       gt_j at mu_j = 0 is <= ubar_j         mu_j = 0  (one evaluation: what a limit that is not active costs)
 *       otherwise, with x1 = max(0, the largest over the members of (hi_m^2 D_m - P_m) / q_mj where q_mj > 0 and of
 *       (P_m / lo_m^2 - D_m) / n_mj where n_mj > 0), P_m and D_m taken at mu_j = 0 (beyond x1 nothing moves any more):
 *       gt_j at mu_j = x1 is > ubar_j         mu_j = x1  (the move limits do not let this step reach the limit)
 *       otherwise                             mu_j = x1 after the bisection below
 *     (the first line that applies);
 *   - the bisection runs 64 times from x0 = 2^-300 x1: xm = sqrt(x0 x1); if gt_j(xm) <= ubar_j then x1 = xm, else x0 = xm
 *     (geometric: rounding noise in q puts x1 near 1e30 where the root lies near 1e6, which no arithmetic bisection from 0
 *     resolves in 64 steps);
 *   - A' = A'(mu); change = max_m |A'_m - A_m| / A_m over the truss's live members;
 *   - worst = max_j g_j / ubar_j over the limits that are switched on (0 where there is none): from the true g, not gt;
 *   - if change <= tol the truss keeps A_k: status 0 if worst <= 1 + limit_tol, else status 3 (converged on its bounds
 *     without meeting a limit);
 *   - otherwise, if k = max_iters, the truss gets status 1 and keeps A_k;
 *   - otherwise A_{k+1} = A' and the truss's `iterations` becomes k + 1;
 *   - if the factorisation of A_k reports info != 0 the truss gets status 2, its design goes back to A_{k-1}, and its
 *     outputs (iterations among them) stay those of analysis k - 1; for k = 0 the outputs are zero (nothing was
 *     analysed), the areas are the initial ones and `iterations` is 0.
 * The status is sticky, exactly as in trs_sizing.h and trs_compliance.h: once a truss has left TRS_MW_ACTIVE nothing
 * changes its areas or its outputs, so its results depend neither on B nor on the other trusses, nor on how often the
 * host looks at `active`, nor on max_iters beyond its own count.
 *
 * One iteration is five launches, the last of them here: trs_assemble and trs_potrf_batched of the design A_k,
 * trs_gather_cases, trs_potrs_cases (trs_solver.h, unchanged: the J unit loads are just more columns of the case block),
 * trs_mw_step.  The step reads the L + J reduced solutions straight from the case block [B][L + J][ld_f].
 *
 * State of a run (device; the caller allocates and ZEROES it before analysis 0):
 *   prev    double [B][nM_max]   the design before the last resizing (what a truss of status 2 goes back to)
 *   mu      double [B][J]        the multipliers of the last analysis (what the next dual solve starts from)
 *   st      int32  [B][4]        (status, iterations, info latched with status 2 - 0 until then -, reserved); the
 *                                status codes: TRS_MW_ACTIVE -1 (inside a run only), 0 converged and within its limits,
 *                                1 iteration limit, 2 the design could not be factored, 3 converged on its bounds
 *                                without meeting a limit
 *   active  int32, one word per analysis: += 1 for every truss that is still active after the call
 * Outputs per truss, all describing the last design analysed with info == 0, in the CALLER's member order:
 *   areas [B][nM_max]; measure [B] = sum w A; measure_history, worst_history [B][H]: the measure and `worst` of every
 *   design the truss analysed, entry k by analysis k (the caller zeroes them); displacement [B][J] = g_j; ratio [B][J] =
 *   g_j / ubar_j (0 for a limit that is switched off); multipliers [B][J] of this analysis's dual solve; sensitivity
 *   [B][J][nM_max] = c_mj, or NULL.  Padding members get zeros.
 * Every sum - gt_j, the measure - runs in one order: every thread adds its members tid, tid + 256, ... in ascending m,
 * the 64 partials of a wave are folded by the butterfly lane ^ 32, ^ 16, ... ^ 1 and the four waves' sums are added in
 * wave order.  x1, max_m |c_mj| A_m and the change are extremes, exact in any order.  No floating-point atomic; one integer atomic per
 * truss (the `active` counter).  After a run the slab holds the factor of the returned design for every truss of status
 * 0, 1 or 3.
 *
 * trs_mw_step, analysis `it` (0 <= it) with `mode`: 0 iterate; 1 the iteration limit: a truss that is not converged
 * gets status 1 instead of a new design.  With it = 0 the run begins: every truss becomes active with 0 iterations and
 * multipliers of zero.  Only active trusses are touched, and an active truss writes its outputs at EVERY analysis.
 *
 * The kernel.  One 256-thread work-group per truss, one launch per analysis.  A thread owns the members tid, tid + 256,
 * ...: their geometry (c, E / L0, w, A) is formed ONCE ahead of the case loop and kept in LDS; the L real solutions and
 * the J virtual ones are staged one at a time in LDS through the view's row_of (held DOFs read 0), double-buffered: one
 * barrier per column.  Each member's c_mj (J doubles), A, lo, hi and w stay in LDS through the dual solve, whose every
 * evaluation of gt_j is one work-group reduction behind one barrier (two alternating slot sets): sweeps x J x (1 to 67)
 * dependent reductions, latency-bound.
 * LDS per work-group (trs_mw_fits): two displacement vectors (6 nJ_max doubles), 64 doubles for the reductions, 6 + J
 * doubles and two ints per member, the reduced row of every DOF (3 nJ_max ints):
 * 60 nJ_max + 512 + (56 + 8 J) nM_max bytes, rounded up to 16, within 160 KB.  (bar-942, 244 joints, J = 8: 128 192
 * bytes.)
 *
 * General member form only, for the reason trs_sizing.h gives: there is no `_tab` twin; convert a table-form batch first.
 * Stress limits in the same run: trs_minweight_stress.h (trs_mw_step_stress, a second instantiation of the same kernel).
 */
#ifndef TRS_MINWEIGHT_H
#define TRS_MINWEIGHT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_MW_ABI_VERSION 1

#define TRS_MW_ACTIVE (-1)
#define TRS_MW_CONVERGED 0
#define TRS_MW_ITER_LIMIT 1
#define TRS_MW_NOT_PD 2
#define TRS_MW_INFEASIBLE 3

#define TRS_MW_WEIGHT 0
#define TRS_MW_VOLUME 1

#define TRS_MW_MAX_LIMITS 8
#define TRS_MW_BISECTIONS 64
/* x0 = 2^-TRS_MW_BRACKET_BITS x1: the positive lower end of the geometric bracket */
#define TRS_MW_BRACKET_BITS 300
/* a member with |c_mj| A_m <= 2^-TRS_MW_CUT_BITS max_m |c_mj| A_m is off limit j's load path */
#define TRS_MW_CUT_BITS 30

int trs_mw_abi_version(void);

/* Whether the tables of a truss of this shape with J limits fit a CU's LDS (see above; otherwise trs_mw_step returns
 * hipErrorInvalidValue). */
int trs_mw_fits(int nJ_max, int nM_max, int J);

/* xyz, conn, E, rho, free_index, n_free, nJ, nM: the batch's arrays as assembled; A [B][nM_max]: the design, resized in
 * place; F [B][L + J][ld_f]: the case block as trs_potrs_cases left it; info [B]: of the factorisation of this design;
 * limit_case [J] (device; a case outside 0 .. L - 1 switches the limit off), limit_joint [B][J] in the DEVICE's joint
 * numbering (the batch's joint order applied; outside the truss: switched off), limit_dir [B][J][3], limit_value [B][J]
 * (not finite or <= 0: switched off); measure: TRS_MW_WEIGHT or TRS_MW_VOLUME; a_min / a_max: [B][nM_max], or NULL for
 * the scalar beside it; measure_history, worst_history [B][H] (entry `it` is written when it < H); sensitivity
 * [B][J][nM_max] or NULL. */
int trs_mw_step(int B, int L, int J, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                double *A, const double *rho, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                const int32_t *nM, const double *F /* [B][L + J][ld_f] */, int ld_f, const int32_t *info,
                const int32_t *limit_case /* [J] */, const int32_t *limit_joint /* [B][J] */,
                const double *limit_dir /* [B][J][3] */, const double *limit_value /* [B][J] */, int measure, double move,
                double tol, double limit_tol, int sweeps, const double *a_min /* [B][nM_max] or NULL */, double a_min_all,
                const double *a_max /* [B][nM_max] or NULL */, double a_max_all, int it, int mode,
                double *prev /* [B][nM_max] */, double *mu /* [B][J] */, int32_t *st /* [B][4] */,
                int32_t *active /* one word */, double *areas, double *measure_out, double *measure_history,
                double *worst_history, int H, double *displacement /* [B][J] */, double *ratio /* [B][J] */,
                double *multipliers /* [B][J] */, double *sensitivity /* [B][J][nM_max] or NULL */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_MINWEIGHT_H */
