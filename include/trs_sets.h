/*
 * trs_sets.h - member-set scenarios: the state of a truss after up to TRS_SETS_MAX of its members are removed, damaged or
 * strengthened AT ONCE, for any number of such scenarios, from the resident Cholesky factor (csrc/sets.hip; the entry
 * points live in libtrs_hip.so beside those of trs_solver.h and trs_loss.h, whose conventions hold here word for word:
 * every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only enqueues work on
 * `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state that a result
 * depends on, no floating-point atomic is used and every sum runs in one fixed order - the results are bit-reproducible
 * from run to run, from stream to stream and between the two member forms, and the numbers of (truss b, scenario s,
 * load case l) do not depend on B, L, the other scenarios, the place of the scenario's columns in Z or the other
 * trusses of the batch).
 *
 * Notation as in trs_loss.h: member m runs from joint j0 to j1, c its direction, k_m = E A / len, tension positive,
 * b_m,f its DOF vector on the free DOFs, z_j = inv(K_ff) b_j,f.  A scenario is an ORDERED set of k <= TRS_SETS_MAX
 * distinct members e_0 .. e_{k-1}, each with an area factor gamma_j >= 0 (0: removed, below 1: damaged, above 1:
 * strengthened, 1: unchanged).  With theta_j = gamma_j - 1 the stiffness becomes K' = K_ff + sum_j theta_j k_j b_j b_j^T,
 * a change of rank k, so nothing is factored again:
 *   P_ij  = c_i . (z_j at i's j1 - z_j at i's j0)     (z_j spread over the joints, zero at constrained DOFs)
 *   W_ij  = k_i P_ij                                  the force a unit pull-apart of member j's ends puts into member i:
 *                                                     the q of trs_loss_apply for member i under column j
 *   A     = I + W diag(theta),   A_ij = fma(theta_j k_i, P_ij, delta_ij)                                     (k x k)
 * A is eliminated by Gauss WITHOUT pivoting, in the set's order; the diagonal of U holds the PIVOTS p_j = det K' with
 * the first j + 1 changes / det K' with the first j: for removals the redundancy of member j once the members before
 * it are gone.  p_j lies in [0, 1] for theta_j < 0 and is >= 1 for theta_j > 0, which is why no pivoting is needed.
 * p_0 of a removal is fma(-k_e, P_ee, 1): the very operation that forms r_e in trs_loss_apply, so a single removal's
 * pivot equals member_loss's r_e bit for bit.  The first p_j <= r_tol makes the scenario UNSTABLE (a mechanism from
 * that member on): first_unstable = j, otherwise -1.  For a stable scenario and load case l, with the intact forces
 * n_i = N_l,e_i = k c . D u_l (the expression that forms W):
 *   a     = diag(theta) inv(A) n                      by the stored L and U, forward then backward, ascending fma
 *   u'    = u_l - sum_j a_j z_j                       ascending j, one fused multiply-add per term
 *   N'_m  = gamma_m k_m c_m . D u'                    (gamma_m = 1 outside the set; exactly 0 for gamma_m = 0)
 *   stress of m = |k_m c_m . D u'| / A_m              = |N'_m| / (gamma_m A_m): it does not depend on gamma
 * and a member with gamma = 0 is left out of the stress peak, as the removed member is in trs_loss_apply.  An EMPTY set
 * (k = 0) returns the intact state: it pads ragged scenario lists.
 *
 *   trs_sets_rhs       b_e,f of the members e = cols[b][i]  -> Z [B][C][ld_f]
 *   trs_potrs_cases    K_ff z = b against the factored slab, L = C                 (trs_solver.h, unchanged)
 *   trs_sets_apply     Z, the intact U -> pivots, unstable, first_unstable, the two peaks and their places, N_after, u_after
 *
 * The caller cuts the scenario axis into ranges whose distinct members fit C columns, and loops over the ranges.
 *
 * The apply kernel is one work-group of four waves per (truss, slice of the range's scenarios), the shape of
 * trs_loss_apply: the member table, free_index, joint_out and u and N of a pass of cases are staged in LDS once; every
 * wave takes one scenario at a time, gathers P from Z through free_index (lane 8 i + j forms P_ij), eliminates in
 * lockstep, and per case forms u' in the ONE joint-layout LDS vector of its own and runs its lanes over the members
 * and the joints, with wave max-reductions that carry the index with the value.
 */
#ifndef TRS_SETS_H
#define TRS_SETS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_SETS_ABI_VERSION 1
#define TRS_SETS_MAX 8 /* members per scenario at most */

int trs_sets_abi_version(void);

/* Whether the apply kernel's tables of a truss of this shape fit a CU's LDS (otherwise trs_sets_apply /
 * trs_sets_tab_apply return hipErrorInvalidValue).  Within 160 KB the kernel holds
 *   per member  5 doubles + 2 ints                (c, k, 1 / A, the end joints)
 *   per joint   3 doubles per wave (four waves) + 4 ints   (u'; free_index, joint_out)
 *   per wave    128 doubles                       (the eliminated k x k system; a of the cases of a pass)
 *   per load case of a pass   3 nJ_max + nM_max doubles    (u, N)
 * and takes the L cases in ceil(L / g) equal passes, g the largest number of cases (at most 8) that fits: the shape
 * fits when L >= 0 and ONE case does. */
int trs_sets_fits(int nJ_max, int nM_max, int L);

/* Z [B][C][ld_f] in the layout trs_potrs_cases reads: row (b, i) is b_e,f of member e = cols[b][i] (int32 [B][C]), formed
 * by the device code of trs_loss_rhs (the same bits); an entry of -1 (any negative) or >= nM[b] gives a zero row.  The
 * other arguments as trs_loss_rhs takes them; the table-form twin takes (conn16, type_idx, types) where the general form
 * takes (conn, E, A). */
int trs_sets_rhs(int B, int C, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                 const double *A, const int32_t *free_index, const int32_t *n_free, const int32_t *nM,
                 const int32_t *cols, double *Z /* out [B][C][ld_f] */, int ld_f, void *stream);
int trs_sets_tab_rhs(int B, int C, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                     const uint8_t *type_idx, const double *types, const int32_t *free_index, const int32_t *n_free,
                     const int32_t *nM, const int32_t *cols, double *Z, int ld_f, void *stream);

/* The results of the scenarios s0 <= s < s0 + Sc (of S in all) of every truss.
 *   slot   [B][Sc][8] int32   the place in cols[b] of the scenario's j-th member, -1 beyond the set (the set ends at the
 *                             first entry that is negative, >= C, or names a column whose member is not in [0, nM[b]))
 *   gamma  [B][Sc][8]         the area factors, or NULL: every member removed
 *   cols   [B][C] int32       as trs_sets_rhs took it;  Z as trs_potrs_cases left it
 *   U      [B][L][ld_f]       the intact reduced displacements as trs_potrs_cases left them (read only)
 * Per (b, s), the index s running over all S scenarios:
 *   pivot          [B][S][8]            p_j; NaN beyond the set and after the failing position
 *   unstable       [B][S] int32         1 when some p_j <= r_tol
 *   first_unstable [B][S] int32         that j, else -1
 * Per (b, l, s):
 *   peak_stress    [B][L][S]            max over the members with gamma != 0 of |k_m c_m . D u'| / A_m
 *   peak_member    [B][L][S] int32      where: the lowest member id on a tie (-1: no member is left)
 *   peak_displace  [B][L][S]            max over the joints of the Euclidean norm of u'_j
 *   peak_joint     [B][L][S] int32      where, in the CALLER's numbering through joint_out (or NULL): lowest id on a tie
 *   N_after        [B][L][S][nM_max]    or NULL: N' of every member, padding members zero
 *   u_after        [B][L][S][nJ_max][3] or NULL: u' in the caller's joint numbering, padding joints zero
 * An unstable scenario: both peaks +inf, both indices -1, its N_after and u_after rows NaN (padding zero).  A truss
 * whose factorisation failed (info[b] != 0) gets meaningless numbers; the others are unaffected.  B == 0, L == 0 or
 * Sc == 0 launches nothing and is no error. */
int trs_sets_apply(int B, int L, int S, int s0, int Sc, int C, int nJ_max, int nM_max, const double *xyz,
                   const int32_t *conn, const double *E, const double *A, const int32_t *free_index, const int32_t *nJ,
                   const int32_t *nM, const int32_t *cols, const int32_t *slot, const double *gamma /* or NULL */,
                   const double *Z, const double *U, int ld_f, double r_tol, double *pivot, int32_t *unstable,
                   int32_t *first_unstable, double *peak_stress, int32_t *peak_member, double *peak_displace,
                   int32_t *peak_joint, double *N_after /* or NULL */, double *u_after /* or NULL */,
                   const int32_t *joint_out /* [B][nJ_max] or NULL */, void *stream);
int trs_sets_tab_apply(int B, int L, int S, int s0, int Sc, int C, int nJ_max, int nM_max, const double *xyz,
                       const uint16_t *conn16, const uint8_t *type_idx, const double *types, const int32_t *free_index,
                       const int32_t *nJ, const int32_t *nM, const int32_t *cols, const int32_t *slot,
                       const double *gamma, const double *Z, const double *U, int ld_f, double r_tol, double *pivot,
                       int32_t *unstable, int32_t *first_unstable, double *peak_stress, int32_t *peak_member,
                       double *peak_displace, int32_t *peak_joint, double *N_after, double *u_after,
                       const int32_t *joint_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_SETS_H */
