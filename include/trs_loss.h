/*
 * trs_loss.h - member-loss analysis: the state of a truss after the removal of any ONE of its members, for every member,
 * from the resident Cholesky factor (csrc/loss.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h,
 * whose conventions hold here word for word: every pointer is a DEVICE pointer owned by the caller, the library
 * allocates nothing, every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a
 * hipError_t, there is no process-wide state that a result depends on, no floating-point atomic is used and every sum
 * runs in one fixed order - the results are bit-reproducible from run to run, from stream to stream and between the two
 * member forms, and the numbers of (truss b, removed member e, load case l) do not depend on B, L, the chunk (e0, C) or
 * the other trusses of the batch).
 *
 * Removing a member is a rank-one change of K_ff, so nothing is factored again.  Member m runs from joint j0 to joint
 * j1, len its length, c = (x_j1 - x_j0) / len, k_m = E A / len, tension positive; b_m is the DOF vector with +c at j1
 * and -c at j0 and b_m,f its restriction to the free DOFs: K_ff = sum_m k_m b_m,f b_m,f^T.  For the removed member e
 *   z_e   = inv(K_ff) b_e,f                       one column of trs_potrs_cases
 *   q_m   = k_m c_m . (z_e,j1 - z_e,j0)           (z_e spread over the joints, zero at constrained DOFs)
 *   r_e   = 1 - q_e                               the member's REDUNDANCY, 0 <= r_e <= 1; over a truss the r_e sum to
 *                                                 nM - n_free, its degree of statical indeterminacy
 *   e is CRITICAL when r_e <= r_tol: without it K_ff is singular, the truss is a mechanism
 * and otherwise, for load case l with the intact displacements u_l and member forces N_l,m = k_m c_m . (u_l,j1 - u_l,j0)
 * (the expression that forms q_m),
 *   alpha = N_l,e / r_e,   u' = u_l + alpha z_e,   N'_m = N_l,m + alpha q_m  (m != e),   N'_e = 0
 * each by one fused multiply-add.  A member with both ends held has b_f = 0: r = 1 and nothing else changes.
 *
 *   trs_loss_rhs       b_e,f of the members e0 <= e < e0 + C  -> Z [B][C][ld_f]
 *   trs_potrs_cases    K_ff z = b against the factored slab, L = C                 (trs_solver.h, unchanged)
 *   trs_loss_apply     Z, the intact U -> r, critical, the two peaks and their places, N_after
 *
 * The members are taken in chunks [e0, e0 + C) so that Z stays small; the caller loops e0 = 0, C, 2 C, ... < nM_max.
 *
 * The apply kernel is one work-group of four waves per (truss, slice of the chunk): per member the end joints, c, k and
 * 1 / A are staged in LDS once, beside free_index, joint_out and the intact u (joint layout) and N of as many load
 * cases as fit (the cases are taken in equal passes when they do not all fit); every wave then takes one removed member
 * at a time, spreads z_e into a joint-layout LDS vector of its own and runs its lanes over the members and the joints,
 * with wave max-reductions that carry the index with the value.
 */
#ifndef TRS_LOSS_H
#define TRS_LOSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_LOSS_ABI_VERSION 1

int trs_loss_abi_version(void);

/* Whether the apply kernel's tables of a truss of this shape fit a CU's LDS (otherwise trs_loss_apply /
 * trs_loss_tab_apply return hipErrorInvalidValue).  Within 160 KB the kernel holds
 *   per member  5 doubles + 2 ints                (c, k, 1 / A, the end joints)
 *   per joint   3 doubles per wave (four waves) + 4 ints   (z_e; free_index, joint_out)
 *   per load case of a pass   3 nJ_max + nM_max doubles    (u, N)
 * and takes the L cases in ceil(L / g) equal passes, g the largest number of cases (at most 8) that fits: the shape
 * fits when L >= 0 and ONE case does. */
int trs_loss_fits(int nJ_max, int nM_max, int L);

/* Z [B][C][ld_f] in the layout trs_potrs_cases reads: row (b, i) is b_{e0 + i},f - at most six non-zeros, +c at the free
 * DOFs of j1 and -c at those of j0 through free_index (DOF -> reduced index, -1 = held) - the other entries
 * c < n_pad = round_up(n_free[b], 64) zero; a row with e0 + i >= nM[b] is all zero.  xyz, the members, free_index,
 * n_free, nM: the batch's arrays as assembled.  The table-form twin carries the form in the middle of its name, as
 * trs_recover_tab_cases does, and takes (conn16, type_idx, types) where the general form takes (conn, E, A); the same
 * bits either way. */
int trs_loss_rhs(int B, int e0, int C, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                 const double *A, const int32_t *free_index, const int32_t *n_free, const int32_t *nM,
                 double *Z /* out [B][C][ld_f] */, int ld_f, void *stream);
int trs_loss_tab_rhs(int B, int e0, int C, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                     const uint8_t *type_idx, const double *types, const int32_t *free_index, const int32_t *n_free,
                     const int32_t *nM, double *Z, int ld_f, void *stream);

/* The results of the removed members e0 <= e < min(e0 + C, nM_max) of every truss.  Z as trs_potrs_cases left it;
 * U [B][L][ld_f]: the intact reduced displacements of the L load cases as trs_potrs_cases left them (read only).
 *   r             [B][nM_max]            the redundancy r_e
 *   critical      [B][nM_max] int32      1 when r_e <= r_tol
 *   peak_stress   [B][L][nM_max]         max over the surviving members m != e of |N'_m| * (1 / A_m)
 *   peak_member   [B][L][nM_max] int32   where: the lowest member id on a tie (-1: no member survives)
 *   peak_displace [B][L][nM_max]         max over the joints of the Euclidean norm of u'_j
 *   peak_joint    [B][L][nM_max] int32   where, in the CALLER's numbering through joint_out (the batch's joint order, or
 *                                        NULL): the lowest caller id on a tie
 *   N_after       [B][L][nM_max][nM_max] or NULL (then not computed): row e holds N' of every member, entry e itself and
 *                                        the padding members zero
 * A critical member: both peaks +inf, both indices -1, its N_after row NaN.  A padding member (nM[b] <= e < nM_max):
 * r = 0, critical = 0, peaks 0, indices -1, its N_after row zero.  A truss whose factorisation failed (info[b] != 0)
 * gets meaningless numbers; the others are unaffected. */
int trs_loss_apply(int B, int L, int e0, int C, int nJ_max, int nM_max, const double *xyz, const int32_t *conn,
                   const double *E, const double *A, const int32_t *free_index, const int32_t *nJ, const int32_t *nM,
                   const double *Z, const double *U, int ld_f, double r_tol, double *r, int32_t *critical,
                   double *peak_stress, int32_t *peak_member, double *peak_displace, int32_t *peak_joint,
                   double *N_after /* or NULL */, const int32_t *joint_out /* [B][nJ_max] or NULL */, void *stream);
int trs_loss_tab_apply(int B, int L, int e0, int C, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                       const uint8_t *type_idx, const double *types, const int32_t *free_index, const int32_t *nJ,
                       const int32_t *nM, const double *Z, const double *U, int ld_f, double r_tol, double *r,
                       int32_t *critical, double *peak_stress, int32_t *peak_member, double *peak_displace,
                       int32_t *peak_joint, double *N_after, const int32_t *joint_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_LOSS_H */
