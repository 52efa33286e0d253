/*
 * trs_nonlinear.h - geometrically nonlinear statics: Newton's method on the batch's tangent factor
 * (csrc/nonlinear.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h, whose conventions hold here
 * word for word: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only
 * enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state
 * that a result depends on, no floating-point atomic is used and every sum runs in one fixed order - the results are
 * bit-reproducible from run to run, from stream to stream and between the two member forms, and the numbers of truss b
 * do not depend on B or on the other trusses).
 *
 * The formulation (corotational bar, large displacements, small strains; the numpy yardstick tests/nonlinear_reference.py
 * and the kernels state it in the same words).  Per member m with ends j0, j1, undeformed coordinates X, displacement u:
 *     D  = X_j1 - X_j0          L0 = |D|
 *     dl = u_j1 - u_j0          (Delta)
 *     d  = D + dl               l  = |d|            n = d / l
 *     e  = (2 D.dl + dl.dl) / (L0 (l + L0))         = (l - L0) / L0 exactly, without subtracting two lengths
 *     N  = E A e
 *     internal force: +N n at j1, -N n at j0
 *     tangent block k_t = (EA / L0) n n^T + (N / l)(I - n n^T), entering K_t as +k_t on the two diagonal blocks and
 *     -k_t on the two off-diagonal ones
 * Residual on the free DOFs: r = lambda P - f_int.  Held DOFs stay at zero (settlements are out of scope).
 * A truss is converged at load factor lambda when |r|_inf <= tol |lambda P|_inf over its free DOFs; for lambda P = 0
 * the answer is u unchanged (converged at once).
 *
 * One Newton iteration is six launches, three of them here:
 *   trs_nl_state      N, f_int, Xc = X + u, R = lambda P - f_int, the norms, the convergence test, the member table W
 *   trs_assemble      called as it is with xyz = Xc, loads = R: writes sum (EA / l) n n^T and the reduced residual
 *                     (trs_solver.h, unchanged; topology, joint order, envelope and tile masks are those of the
 *                     undeformed truss: they are built from joint spans, not from values)
 *   trs_nl_tangent    S += delta_m per member, delta_m = (EA/L0 - EA/l - N/l) n n^T + (N/l) I: the slab holds K_t
 *                     (entry (r, s) as w (n_r n_s): symmetric to the bit, as the assembly's k (c_r c_s))
 *   trs_potrf_batched, trs_potrs_batched   unchanged: uf = du; info[b] != 0 now says that the tangent at this iterate
 *                     is not positive definite
 *   trs_nl_update     u += du for the trusses that are active with info == 0
 *
 * State of a run (device, the caller allocates and zeroes it before the first load step):
 *   U   double [B][nJ_max][3]  the displacements in joint layout, the batch's own (device) numbering, zero at held DOFs
 *   st  int32  [B][4]          (status, iterations of this load step, info of the tangent that was not positive
 *                              definite - latched by trs_nl_update with status 2, 0 until then -, reserved).  Status codes:
 *                              TRS_NL_ACTIVE -1 (inside a step only), 0 converged, 1 iteration limit, 2 tangent not
 *                              positive definite, 3 not attempted because an earlier step failed.
 * The status is sticky: once a truss has left TRS_NL_ACTIVE in a step nothing changes its U or its counters until the
 * next step begins, so a result does not depend on how long the others iterate (nor on max_iters beyond the truss's
 * own count, nor on how often the host looks at `active`).  A truss that is not active gets R = 0, the substitution
 * then returns du = 0 for it exactly, and nothing else needs gating.
 *
 * trs_nl_state, iteration it of a load step (it = 0: the step begins - a truss whose last step ended with status 1, 2
 * or 3 gets status 3, the others become active with 0 iterations):
 *   - an active truss with |r|_inf <= tol |lambda P|_inf (or lambda P = 0) becomes converged;
 *   - `last` = 2: a call that ONLY writes the outputs (the host has seen that no truss is active): the step does not
 *     begin again, whatever `it` is;
 *   - `last` != 0 (1: the iteration limit; 2: as above): a truss still active gets
 *     status 1, and the outputs of load step `step` are written for EVERY truss, in the CALLER's joint numbering
 *     through joint_out (as trs_recover writes u), from the U the truss holds (its last accepted iterate):
 *       u [B][S][nJ_max][3], N [B][S][nM_max], f_ext [B][S][nJ_max][3] (the applied load lambda P at free DOFs, f_int -
 *       the reaction - at held ones), iters, status (int32 [B][S]), residual [B][S] = |r|_inf (absolute);
 *     zero on the padding joints and members;
 *   - active (int32, one word, zeroed by the caller): += 1 for every truss that is still active after this call.
 * W [B][nM_max][6] = (n0, n1, n2, EA/L0 - EA/l - N/l, N/l, N) per member, for trs_nl_tangent.
 *
 * trs_nl_tangent updates exactly the entries that trs_assemble stores for a row (trs_solver.h "Slab layout"): columns
 * from the row's diagonal tile on (from 0 with TRS_ASM_FULL_SYMMETRIC, passed in `flags`), inside cend, and only tiles
 * whose mask bit is set (env as trs_assemble wrote it, or NULL for the dense mode).  Owner-computes: 16 threads per slab
 * row; thread 15 adds the sum of +delta_m over the joint's member ends (in list order, below; formed once per joint
 * ahead of the row loop) to the joint's own block,
 * threads 0..14 take the member ends: the first end of every neighbour adds the sum of -delta_m over the members to
 * that neighbour (parallel members, in member-id order) to the coupling block.  No entry is touched by two threads,
 * there is no atomic, and an entry whose sum is exactly zero is not written: at u = 0 the slab keeps its bits.
 * Both kernels sum over a joint's member ends in the order (far joint, member id) - build_end_lists' lists, re-sorted:
 * the order of trs_assemble's adjacency lists.  Sums here then round as the assembly's do, and a member listed twice
 * gives the bits of one member of twice the area wherever the linear solve does (where the pair leads both ends' lists).
 * The compact member form of the assembly (TRS_ASM_COMPACT) writes no slab and cannot be amended: callers must not
 * combine the two.
 *
 * LDS per work-group (trs_nl_fits): the state kernel holds u (3 nJ_max doubles), N and n per member (4 nM_max doubles),
 * four doubles for the norms, the member-end lists and the far joint of every list entry (2 nJ_max + 1 + 4 nM_max ints):
 * 32 nJ_max + 48 nM_max + 36 bytes, rounded up to 16, within 160 KB.  The tangent kernel holds the joints' own
 * delta blocks (6 nJ_max doubles, summed once per launch), the end lists, the far joints, free_index and the row table:
 * 5 nJ_max + 1 + 4 nM_max + slab_rows ints, with slab_rows <= round_up(3 nJ_max, 64) in trs_nl_fits; both must fit.
 * Every kernel trims nJ[b], nM[b] and n_free[b] to the arrays and clamps end-joint ids to them (as the stage of the
 * column analyses does): whatever the inputs hold, nothing is read or written outside the arrays.
 */
#ifndef TRS_NONLINEAR_H
#define TRS_NONLINEAR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_NL_ABI_VERSION 1

#define TRS_NL_ACTIVE (-1)
#define TRS_NL_CONVERGED 0
#define TRS_NL_ITER_LIMIT 1
#define TRS_NL_NOT_PD 2
#define TRS_NL_NOT_ATTEMPTED 3

int trs_nl_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS (see above; otherwise the entry points return
 * hipErrorInvalidValue). */
int trs_nl_fits(int nJ_max, int nM_max);

/* Iteration `it` (>= 0) of load step `step` (0 <= step < S) at load factor lambda; one 256-thread work-group per truss.
 * xyz, the members, loads, free_index, n_free, nJ, nM: the batch's arrays as assembled (loads [B][nJ_max][3] = P in the
 * batch's own numbering).  Xc, R [B][nJ_max][3]: the inputs of the trs_assemble call that follows.  The `_tab` twin takes
 * (conn16, type_idx, types) where the general form takes (conn, E, A); the same bits either way. */
int trs_nl_state(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E, const double *A,
                 const double *loads, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                 const int32_t *nM, int ld_f, double lambda, double tol, int it, int last, int step, int S,
                 const double *U, int32_t *st, double *Xc, double *R, double *W, int32_t *active, double *u, double *N,
                 double *f_ext, int32_t *iters, int32_t *status, double *residual,
                 const int32_t *joint_out /* [B][nJ_max] or NULL */, void *stream);
int trs_nl_state_tab(int B, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16, const uint8_t *type_idx,
                     const double *types, const double *loads, const int32_t *free_index, const int32_t *n_free,
                     const int32_t *nJ, const int32_t *nM, int ld_f, double lambda, double tol, int it, int last,
                     int step, int S, const double *U, int32_t *st, double *Xc, double *R, double *W, int32_t *active,
                     double *u, double *N, double *f_ext, int32_t *iters, int32_t *status, double *residual,
                     const int32_t *joint_out, void *stream);

/* S += delta on the ASSEMBLED slab [B][slab_rows][ld], between trs_assemble and trs_potrf_batched; W as trs_nl_state
 * wrote it, env as trs_assemble wrote it (or NULL), flags: the TRS_ASM_* word of that assembly. */
int trs_nl_tangent(int B, int nJ_max, int nM_max, const int32_t *conn, const double *E, const double *A,
                   const int32_t *free_index, const int32_t *n_free, const int32_t *nJ, const int32_t *nM, int ld,
                   int slab_rows, double *S, const int32_t *env /* or NULL */, int flags, const double *W, void *stream);
int trs_nl_tangent_tab(int B, int nJ_max, int nM_max, const uint16_t *conn16, const uint8_t *type_idx,
                       const double *types, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                       const int32_t *nM, int ld, int slab_rows, double *S, const int32_t *env, int flags,
                       const double *W, void *stream);

/* U += du (uf [B][ld_uf] as trs_potrs_batched left it) for the trusses that are active with info[b] == 0, and their
 * iteration count becomes `it` (the 1-based number of this update); an active truss with info[b] != 0 keeps its U and
 * its count and gets TRS_NL_NOT_PD.  It reads no member: one entry point serves both member forms. */
int trs_nl_update(int B, int nJ_max, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                  const double *uf, int ld_uf, const int32_t *info, int it, double *U, int32_t *st, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_NONLINEAR_H */
