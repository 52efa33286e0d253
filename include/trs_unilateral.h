/*
 * trs_unilateral.h - tension-only and compression-only members: the active-set iteration, iterated on the device
 * (csrc/unilateral.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h, whose conventions hold
 * here word for word: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call
 * only enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide
 * state that a result depends on, no floating-point atomic is used and the one sum here is an integer count - the
 * results are bit-reproducible from run to run and from stream to stream, and the numbers of truss b do not depend on B
 * or on the other trusses; the kernel trims nJ[b], nM[b] and n_free[b] to the arrays and clamps end-joint ids to them
 * through the truss view (csrc/trs_view.h): whatever the inputs hold, nothing is read or written outside the arrays).
 *
 * The method (the numpy yardstick tests/unilateral_reference.py and the kernel state it in the same words).  Inputs per
 * truss: one load case (joint forces), optionally a member pre-strain eps0 [nM] (the meaning it has in trs_effects.h),
 * per member kind in {0 bilateral, +1 tension-only, -1 compression-only}, slack_factor >= 0 (the fraction of its area a
 * slack member keeps; 0 removes it exactly), max_iters >= 0, optionally an initial state (1 active, 0 slack; default all
 * active), and the nominal areas A.  Analysis k (k = 0, 1, ...) of state s_k:
 *   - A_eff,m = A_m if s_k,m is active, else slack_factor A_m; bilateral members are always active;
 *   - solve K(A_eff) u = f, the right-hand side formed with A_eff (trs_effects_rhs): a slack member contributes
 *     slack_factor times its pre-strain load;
 *   - e_m = c_m.(u_j1 - u_j0) - eps0_m L0_m, the elongation beyond the stress-free length, for every member, slack ones
 *     included (that is what lets a slack member come back);
 *   - want_m = active if kind_m = 0 or kind_m e_m > 0, else slack: the test is strict (e_m = 0 means slack), no
 *     thresholds;
 *   - changed = the number of members with want_m != s_k,m;
 *   - changed = 0: status 0 (converged), the truss keeps s_k;
 *   - otherwise, if k = max_iters: status 1, the truss keeps s_k;
 *   - otherwise s_{k+1} = want (all flips at once) and the truss's `iterations` becomes k + 1;
 *   - if the factorisation of analysis k reports info != 0: status 2, the state goes back to s_{k-1} (the initial state
 *     for k = 0), `iterations` to k - 1 (0 for k = 0) and `violations` stays the `changed` of analysis k - 1 (0 for
 *     k = 0); the info is latched, as in trs_sizing.h.
 * The status is sticky, exactly as in trs_sizing.h and trs_nonlinear.h: once a truss has left TRS_UN_ACTIVE nothing
 * changes its state, its areas or its outputs, so its results depend neither on B nor on the other trusses, nor on how
 * often the host looks at `active`, nor on max_iters beyond its own count.  (The caller goes on assembling and factoring
 * a frozen truss with its unchanged areas: the same bits.)
 *
 * One analysis is five launches, the last of them here: trs_assemble and trs_potrf_batched of A_eff, trs_effects_rhs
 * with A_eff (L = 1; eps0 or NULL), trs_potrs_cases (all unchanged), trs_un_step.  The step reads the reduced solution
 * from the case block [B][1][ld_f] that trs_potrs_cases left and writes the next state and the next A_eff into the
 * batch's A in place.  After the run the caller recovers u, f_ext and N of the final structure with trs_effects_recover
 * and A_eff; where a truss ended with status 2 the slab holds the failed factor of a state the truss no longer has, so
 * the caller analyses the final states once more (the same four launches, then trs_un_step with mode 2).
 *
 * State of a run (device; the caller allocates and ZEROES all of it before analysis 0):
 *   state        int8  [B][nM_max]  1 active, 0 slack; live members only are written, the padding stays 0
 *   prev_state   int8  [B][nM_max]  the state before the last flips (what a truss of status 2 goes back to)
 *   st           int32 [B][4]       (status, iterations, info latched with status 2 - 0 until then -, reserved); the
 *                                   status codes: TRS_UN_ACTIVE -1 (inside a run only), 0 converged, 1 iteration
 *                                   limit, 2 a structure could not be factored
 *   active       int32, one word per analysis: += 1 for every truss that is still active after the call
 *   violations   int32 [B]          the `changed` of the last analysis written
 *   flips_history int32 [B][H]      entry k by analysis k (written when k < H), zero beyond the truss's own count
 * A_nom [B][nM_max] (const): the nominal areas, a copy the caller takes before analysis 0.  The caller also forms
 * A = A_eff(s_0) before analysis 0 where it hands in an initial state (with all members active A_eff = A_nom).
 *
 * trs_un_step, analysis `it` (0 <= it) with `mode`:
 *   0  iterate;
 *   1  the iteration limit: a truss that is not converged gets status 1 instead of a new state;
 *   2  report only: `violations` is recomputed for every truss of status 0, 1 or 2 whose info (of THIS factorisation) is
 *      0, for the state it holds - nothing else changes.
 * With mode 0 or 1 and it = 0 the run begins: every truss becomes active with 0 iterations and its state is the initial
 * one - all active with state0 == NULL, else state0 != 0 per member, bilateral members forced active.  Only active
 * trusses are touched.
 *
 * The kernel.  One 256-thread work-group per truss, one launch per analysis.  The reduced solution is staged into LDS
 * through the view's rows(j) (one test per joint; held DOFs and the padding read 0); thread tid then walks the members
 * tid, tid + 256, ...: c, L0 and e_m from the coordinates, want_m, and the comparison with the state; `changed` is an
 * integer work-group sum, exact in any order: the wave's popcount of the flips, then the four waves through LDS.  Each
 * thread keeps (want, state) of its members in one LDS byte and is the only thread that touches it.
 * LDS per work-group (trs_un_fits): one displacement vector (3 nJ_max doubles), four ints for the wave counts, one byte
 * per member: 24 nJ_max + 16 + nM_max bytes, rounded up to 16, within 160 KB.
 *
 * General member form only: the kernel WRITES areas, one per member, which a type table (<= 256 shared triples) cannot
 * hold - there is no `_tab` twin; convert a table-form batch first.
 */
#ifndef TRS_UNILATERAL_H
#define TRS_UNILATERAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_UN_ABI_VERSION 1

#define TRS_UN_ACTIVE (-1)
#define TRS_UN_CONVERGED 0
#define TRS_UN_ITER_LIMIT 1
#define TRS_UN_NOT_PD 2

int trs_un_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS (see above; otherwise trs_un_step returns
 * hipErrorInvalidValue). */
int trs_un_fits(int nJ_max, int nM_max);

/* xyz, conn, free_index, n_free, nJ, nM: the batch's arrays as assembled; A [B][nM_max]: A_eff of the state analysed,
 * rewritten in place for the next state; F [B][1][ld_f]: the case block as trs_potrs_cases left it; info [B]: of the
 * factorisation of this structure; eps0 [B][nM_max] or NULL; kind int8 [B][nM_max] (the library cannot look at device
 * values: the caller has checked them; anything but +1 and -1 is read as bilateral); state0 int8 [B][nM_max] or NULL:
 * the initial state, read with it = 0 only. */
int trs_un_step(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, double *A,
                const int32_t *free_index, const int32_t *n_free, const int32_t *nJ, const int32_t *nM,
                const double *F /* [B][1][ld_f] */, int ld_f, const int32_t *info, const double *eps0 /* or NULL */,
                const int8_t *kind, const double *A_nom, double slack_factor, const int8_t *state0 /* or NULL */, int it,
                int mode, int8_t *state, int8_t *prev_state, int32_t *st /* [B][4] */, int32_t *active /* one word */,
                int32_t *violations, int32_t *flips_history, int H, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_UNILATERAL_H */
