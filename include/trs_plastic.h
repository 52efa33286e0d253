/*
 * trs_plastic.h - collapse load: elastic-plastic members, the event-to-event analysis iterated on the device
 * (csrc/plastic.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h, whose conventions hold here
 * word for word: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only
 * enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide
 * state that a result depends on, no floating-point atomic and no floating-point sum across threads is used - the
 * reductions are maxima, minima with an index and integer counts, exact in any order - so the results are
 * bit-reproducible from run to run and from stream to stream, and the numbers of truss b do not depend on B or on the
 * other trusses; the kernels trim nJ[b], nM[b] and n_free[b] to the arrays and clamp end-joint ids to them through the
 * truss view (csrc/trs_view.h): whatever the inputs hold, nothing is read or written outside the arrays).
 *
 * The method (the numpy yardstick tests/plastic_reference.py and the kernel state it in the same words).  Inputs per
 * truss: one reference load pattern P (joint forces), scaled by the load factor lambda; member capacities
 * cap_tension_m > 0 and cap_compression_m > 0 (forces); hardening h >= 0, the fraction of its stiffness a yielded member
 * keeps (0: perfectly plastic, the area is scaled to exactly 0); lambda_max > 0; disp_limit >= 0 (0: none);
 * collapse_ratio > 1; tie_tol >= 0; max_events >= 0; and the nominal areas A.  State per truss: s_m in {0 elastic, +1
 * yielded in tension, -1 yielded in compression}, N [nM], u [DOFs], lambda and r_0, all accumulated, all zero at first.
 * Analysis k (k = 0, 1, ...) of state s_k:
 *   1. A_eff,m = A_m where s_m = 0, else h A_m; assemble and factor K(A_eff);
 *   2. info != 0: status 2 (mechanism); nothing advances, the info is latched;
 *   3. otherwise solve K du = P;
 *   4. the softening test: r_k = max over DOFs of |du|; analysis 0 stores r_0; if NOT (r_k <= collapse_ratio r_0):
 *      status 2 (mechanism) with info left 0; a non-finite r_k counts as collapse (the tangent is softer than the elastic
 *      structure by that ratio: the mechanism that got through the factorisation on rounding noise);
 *   5. de_m = c_m.(du_j1 - du_j0) and dN_m = (E_m A_eff,m / L0_m) de_m, for every member;
 *   6. the release test: a yielded member with s_m de_m < 0 unloads (strict, no threshold); if any member unloads:
 *      at k = max_events status 1; otherwise those members return to s = 0, nothing advances, and the analysis counts
 *      as an event: its member_history entry is -1 and its count the number released;
 *   7. otherwise advance: for every elastic member dl_m = (cap_tension_m - N_m) / dN_m where dN_m > 0,
 *      (-cap_compression_m - N_m) / dN_m where dN_m < 0, +inf where dN_m = 0, negative values clamped to 0;
 *      dl_y = the minimum of the dl_m, the governing member the lowest index that attains it;
 *      dl_L = lambda_max - lambda; dl_u = min over free DOFs with du != 0 of (disp_limit - sign(du) u) / |du|, clamped
 *      at 0, +inf with disp_limit = 0;
 *      if min(dl_L, dl_u) <= dl_y: advance lambda, N and u by that step; status 0 (lambda_max reached) where
 *      dl_L <= dl_u, else status 3 (displacement limit);
 *      otherwise, at k = max_events: status 1 without advancing;
 *      otherwise advance by dl_y; every elastic member with dl_m <= dl_y (1 + tie_tol) yields with s_m = sign(dN_m) and
 *      takes N_m = +cap_tension_m or -cap_compression_m exactly (where the advance brought it, up to rounding and
 *      tie_tol), unless it lay beyond that capacity already (dl_m was clamped: a member that hardened past its capacity,
 *      unloaded and loads again keeps its force, and the joints their equilibrium); `events` = k + 1;
 *   8. the history: analysis k writes entry k (k < H = max_events + 1) of lambda_history, member_history (the governing
 *      member, -1 for a release, -2 for a terminal analysis), count_history (the members that yielded or were released,
 *      0 for a terminal analysis) and umax_history (the largest |u_d| over the DOFs after the analysis: the pushover
 *      curve).
 * "Advance by dl": lambda += dl, N_m += dl dN_m for every member, u += dl du.  A truss that ends is always left in the
 * equilibrium state of its last completed event; nothing is ever rolled back.  The status is sticky, exactly as in
 * trs_sizing.h and trs_unilateral.h: once a truss has left TRS_PL_ACTIVE nothing changes its state, its areas or its
 * outputs, so its results depend neither on B nor on the other trusses, nor on how often the host looks at `active`,
 * nor on a larger max_events.  (The caller goes on assembling and factoring a frozen truss with its unchanged areas:
 * the same bits.)
 *
 * One analysis is five launches, the last of them here: trs_assemble and trs_potrf_batched of A_eff, trs_gather_cases of
 * P (L = 1), trs_potrs_cases (all unchanged), trs_pl_step.  The step reads the reduced solution from the case block
 * [B][1][ld_f] that trs_potrs_cases left and writes the next state and the next A_eff into the batch's A in place.  After
 * the run trs_pl_finish writes u and f_ext in the caller's joint layout from the accumulated state (trs_effects_recover
 * cannot serve: N is not a function of u); no re-analysis is needed.  Where a truss ended with status 2 by `info` the
 * slab holds no valid factor of it.
 *
 * State of a run (device; the caller allocates and ZEROES all of it before analysis 0):
 *   state          int8   [B][nM_max]    0 elastic, +1 / -1 yielded; live members only are written
 *   N              double [B][nM_max]    the accumulated member forces
 *   U              double [B][3 nJ_max]  the accumulated displacements, the device's joint numbering, 0 at held DOFs
 *   acc            double [B][4]         (lambda, r_0, the largest |u_d|, reserved)
 *   st             int32  [B][4]         (status, events, info latched with status 2 - 0 until then -, reserved); the
 *                                        status codes: TRS_PL_ACTIVE -1 (inside a run only), 0 lambda_max reached, 1 event
 *                                        limit, 2 mechanism, 3 displacement limit
 *   active         int32, one word per analysis: += 1 for every truss that is still active after the call
 *   lambda_history, umax_history double [B][H]; member_history, count_history int32 [B][H]: entry k by analysis k
 *                                        (written when k < H), zero beyond the truss's own count
 * A_nom [B][nM_max] (const): the nominal areas, a copy the caller takes before analysis 0 (A = A_nom then).
 *
 * trs_pl_step, analysis `it` (0 <= it) with `mode`:
 *   0  iterate;
 *   1  the event limit (it = max_events): a truss that would release or yield gets status 1 instead.
 * (The report mode 2 of trs_un_step is an entry point of its own here, trs_pl_finish: the results are the accumulated
 * state, nothing is analysed again.)  With it = 0 the run begins: every truss becomes active with 0 events.  Only active
 * trusses are touched.
 *
 * The kernel.  One 256-thread work-group per truss, one launch per analysis.  du is staged into LDS through the view's
 * rows(j) (one test per joint; held DOFs and the padding read 0); thread tid then walks the members tid, tid + 256, ...:
 * c, L0, de_m, dN_m and dl_m on the spot, dl_m and dN_m kept in LDS for the second pass (each thread is the only one that
 * touches its members' entries).  The reductions - the maximum for r_k and for |u_d|, the lexicographic minimum of
 * (dl_m, m), the DOF minimum for dl_u, the integer counts - are exact in any order: within the wave first, then the four
 * waves through LDS.  The second pass updates N, u, s, lambda, the history and A_eff in place, from A_nom.
 * LDS per work-group (trs_pl_fits): one displacement vector (3 nJ_max doubles), two doubles per member, sixteen doubles
 * and twelve ints for the waves' partial results: 24 nJ_max + 16 nM_max + 176 bytes, rounded up to 16, within 160 KB.
 * trs_pl_finish keeps the member-end lists of the joints with a held DOF (2 nJ_max + 1 + 2 nM_max ints):
 * 8 nJ_max + 8 nM_max + 4 bytes, always less; trs_pl_fits answers for both.
 *
 * General member form only: the kernel WRITES areas, one per member, which a type table (<= 256 shared triples) cannot
 * hold - there is no `_tab` twin; convert a table-form batch first.
 */
#ifndef TRS_PLASTIC_H
#define TRS_PLASTIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_PL_ABI_VERSION 1

#define TRS_PL_ACTIVE (-1)
#define TRS_PL_LAMBDA_MAX 0
#define TRS_PL_EVENT_LIMIT 1
#define TRS_PL_MECHANISM 2
#define TRS_PL_DISP_LIMIT 3

int trs_pl_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS (see above; otherwise trs_pl_step and trs_pl_finish return
 * hipErrorInvalidValue). */
int trs_pl_fits(int nJ_max, int nM_max);

/* xyz, conn, E, free_index, n_free, nJ, nM: the batch's arrays as assembled; A [B][nM_max]: A_eff of the state analysed,
 * rewritten in place for the next state; F [B][1][ld_f]: the case block as trs_potrs_cases left it; info [B]: of the
 * factorisation of this structure; cap_tension, cap_compression [B][nM_max] (the library cannot look at device values:
 * the caller has checked them). */
int trs_pl_step(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E, double *A,
                const int32_t *free_index, const int32_t *n_free, const int32_t *nJ, const int32_t *nM,
                const double *F /* [B][1][ld_f] */, int ld_f, const int32_t *info, const double *cap_tension,
                const double *cap_compression, const double *A_nom, double hardening, double lambda_max,
                double disp_limit, double collapse_ratio, double tie_tol, int it, int mode, int8_t *state, double *N,
                double *U /* [B][3 nJ_max] */, double *acc /* [B][4] */, int32_t *st /* [B][4] */,
                int32_t *active /* one word */, double *lambda_history, int32_t *member_history,
                int32_t *count_history, double *umax_history, int H, void *stream);

/* The report: u [B][nJ_max][3] (= U in the caller's joint layout through joint_out, or NULL for the device's own) and
 * f_ext [B][nJ_max][3]: lambda P at the free DOFs, at the held ones the sum of N_m c_m over the joint's member ends in
 * ascending member index (+ at joint1, - at joint0), 0 on the padding.  loads [B][nJ_max][3]: P in the caller's joint
 * numbering, as trs_gather_cases read it. */
int trs_pl_finish(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const int32_t *free_index,
                  const int32_t *n_free, const int32_t *nJ, const int32_t *nM, int ld_f, const double *loads,
                  const double *N, const double *U, const double *acc, const int32_t *joint_out /* or NULL */,
                  double *u, double *f_ext, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_PLASTIC_H */
