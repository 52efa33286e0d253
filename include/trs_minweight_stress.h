/*
 * trs_minweight_stress.h - minimum weight under stress AND displacement limits in one run: the optimality-criteria
 * method of trs_minweight.h with the stress-ratio area of every member (trs_sizing.h, Euler term included) as the
 * member's LOWER bound in the subproblem (csrc/minweight.hip; the entry points live in libtrs_hip.so beside those of
 * trs_minweight.h, whose conventions, run state, outputs, summation order and launch protocol hold here word for word).
 * trs_minweight.h itself - its three symbols, its version, the code path and the bits of trs_mw_step - is unchanged; this
 * header has a version of its own.
 *
 * The method (the numpy yardstick tests/minweight_stress_reference.py and the kernel state it in the same words).
 * Everything in trs_minweight.h stays as it is; the stress variant adds the following.  Inputs:
 * allow_tension > 0 and allow_compression > 0, per batch or per truss (+inf switches a side off for that truss), and
 * euler_kappa >= 0 as in trs_sizing.h (it models I = kappa A^2; 0: no member buckling term).  Analysis k of design A:
 *   - for every REAL case l < L, N_ml = ((E_m / L0_m) A_m) proj_m(u_l);
 *   - the required area in case l is N / allow_tension for N > 0; for P = -N > 0 it is
 *     max(P / allow_compression, sqrt(P L0^2 / (pi^2 E kappa))), the second term only when kappa > 0 (trs_sizing.h's
 *     words and its expression order);
 *   - req_m is the maximum over the cases in ascending l; on a tie the lowest l governs; governing_m is that l, or -1
 *     where req_m = 0;
 *   - the floor: lo_m = min(max(lo_m, req_m), hi_m), lo_m and hi_m the move-and-bound interval of trs_minweight.h: a member that
 *     needs more than (1 + move) A_m grows at the move limit, and a member with w_m <= 0 keeps lo_m = hi_m;
 *   - the subproblem, the cut (TRS_MW_CUT_BITS), the dual solve, the bisection, A'(mu) and `change` are unchanged: only
 *     lo differs.  Members governed by stress sit on the floor, members governed by a displacement limit are sized by
 *     the multipliers;
 *   - utilisation_m = req_m / A_m, and stress_worst = its maximum over the live members; `worst` and worst_history stay
 *     the displacement figure; stress_history[k] = stress_worst;
 *   - if change <= tol: status 0 if max(worst, stress_worst) <= 1 + limit_tol, else status 3; statuses 1 and 2, the
 *     roll-back, the freezing and the counter are those of trs_minweight.h, unchanged.
 * Further outputs: utilisation [B][nM_max], governing int32 [B][nM_max] (padding members get 0 and -1; a truss of status
 * 2 at analysis 0 gets 0 and -1 too), stress_history [B][H] (the caller zeroes it).  Maxima are exact in any order; no
 * floating-point sum is added to those of trs_minweight.h.
 * The kernel is trs_minweight.h's as a template on `bool STRESS`: the instantiation without stress limits is compiled from
 * the statements it had before, and it is the one trs_mw_step launches - that entry point keeps its code path and its
 * bits.  The stress instantiation keeps three more words per member in LDS, formed ahead of the case loop - the running
 * req_m (a double), its case (an int) and the Euler coefficient L0^2 / (pi^2 E kappa) (a double) - and updates the
 * running requirement as each real case passes through the stage: there is no further pass over the case block, and no u
 * or N goes to HBM.  Every real case is projected, not only those a limit names.
 * LDS per work-group (trs_mw_fits_stress): 60 nJ_max + 512 + (76 + 8 J) nM_max bytes, rounded up to 16, within 160 KB.
 * (bar-942, 244 joints, J = 8: 14 640 + 512 + 140 x 942 = 147 032, rounded 147 040 bytes of 163 840.)
 */
#ifndef TRS_MINWEIGHT_STRESS_H
#define TRS_MINWEIGHT_STRESS_H

#include "trs_minweight.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_MWS_ABI_VERSION 1

int trs_mws_abi_version(void);

/* Whether the tables of the stress variant fit (see above; otherwise trs_mw_step_stress returns hipErrorInvalidValue). */
int trs_mw_fits_stress(int nJ_max, int nM_max, int J);

/* trs_mw_step with stress limits (see above): the same arguments, and allow_tension, allow_compression (> 0; +inf
 * switches a side off) or allow [B][2] (device; tension, compression per truss - then the two scalars are not read),
 * euler_kappa >= 0 and finite; utilisation [B][nM_max], governing [B][nM_max], stress_history [B][H] (entry `it` is
 * written when it < H). */
int trs_mw_step_stress(int B, int L, int J, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                       double *A, const double *rho, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                       const int32_t *nM, const double *F /* [B][L + J][ld_f] */, int ld_f, const int32_t *info,
                       const int32_t *limit_case /* [J] */, const int32_t *limit_joint /* [B][J] */,
                       const double *limit_dir /* [B][J][3] */, const double *limit_value /* [B][J] */, int measure,
                       double move, double tol, double limit_tol, int sweeps, const double *a_min /* [B][nM_max] or NULL */,
                       double a_min_all, const double *a_max /* [B][nM_max] or NULL */, double a_max_all,
                       double allow_tension, double allow_compression, const double *allow /* [B][2] or NULL */,
                       double euler_kappa, int it, int mode, double *prev /* [B][nM_max] */, double *mu /* [B][J] */,
                       int32_t *st /* [B][4] */, int32_t *active /* one word */, double *areas, double *measure_out,
                       double *measure_history, double *worst_history, int H, double *displacement /* [B][J] */,
                       double *ratio /* [B][J] */, double *multipliers /* [B][J] */,
                       double *sensitivity /* [B][J][nM_max] or NULL */, double *utilisation /* [B][nM_max] */,
                       int32_t *governing /* [B][nM_max] */, double *stress_history /* [B][H] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_MINWEIGHT_STRESS_H */
