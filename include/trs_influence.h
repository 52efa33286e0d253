/*
 * trs_influence.h - influence lines and moving-load envelopes of the member forces, from the resident Cholesky factor
 * (csrc/influence.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h and trs_loss.h, whose
 * conventions hold here word for word: every pointer is a DEVICE pointer owned by the caller, the library allocates
 * nothing, every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there
 * is no process-wide state that a result depends on, no floating-point atomic is used and every sum runs in one fixed
 * order - the results are bit-reproducible from run to run, from stream to stream and between the two member forms, and
 * the numbers of (truss b, member m) do not depend on B, the chunk (e0, C) or the other trusses of the batch).
 *
 * Member m runs from joint j0 to joint j1, len its length, c = (x_j1 - x_j0) / len, k_m = E A / len (formed as
 * csrc/loss.hip forms it), tension positive; b_m is the DOF vector with +c at j1 and -c at j0, b_m,f its restriction to
 * the free DOFs.  The column z_m = inv(K_ff) b_m,f is what trs_loss_rhs and trs_potrs_cases produce for the member-loss
 * analysis, and the force in m under ANY load vector f is N_m = k_m z_m . f_f (Maxwell / Mueller-Breslau): k_m z_m is the
 * influence line of N_m for a unit load at every joint in every direction at once.  Nothing is factored again.
 *
 *   path      P joints path[0..P) in the CALLER's numbering, consecutive ones at distinct positions (a joint may recur);
 *             arc length s_0 = 0, s_p = s_{p-1} + |x_path[p] - x_path[p-1]| (each segment sqrt(fma(dz, dz, fma(dy, dy,
 *             dx dx))), summed in ascending p by one lane), S = s_{P-1}
 *   load      a vector d in R^3 per unit axle weight (any length), A axles of weights w_a at offsets
 *             0 = o_0 <= o_1 <= ... <= o_{A-1} behind the lead axle
 *   eta[m][p] = k_m (d . z_m at joint path[p]): z_m spread over the joints, zero at held DOFs; the dot product runs over
 *             the free axes in ascending order with fma from 0
 *   eta_m(s)  piecewise linear through (s_p, eta[m][p]) - an axle between two path joints is shared between them by the
 *             lever rule: on s_q <= s < s_{q+1}, eta_m(s) = fma((s - s_q) / (s_{q+1} - s_q), eta[q+1] - eta[q], eta[q]),
 *             and eta[q+1] itself at s = s_{q+1} - and 0 off the path; with eps = 1e-12 S an axle at -eps <= s <= S + eps stands on the path, s clamped into
 *             [0, S].  For P = 1 the line is eta[m][0] at s = 0 and 0 elsewhere
 *   N_m(x)    = sum over a ascending of w_a eta_m(x - o_a), accumulated with fma from 0; x the lead axle's arc position
 *   envelope  N_m is piecewise linear with jumps only at the ends of the path, so its extremes lie where some axle stands
 *             on a path joint: the P A candidates (p, a), x = s_p + o_a.  At candidate (p, a) axle a takes eta[m][p]
 *             itself and axle a' stands at s_p + (o_a - o_a') (NOT x - o_a': the round trip through x can push an axle
 *             off the end of the path by one ulp).  N_max[m], N_min[m]: the largest and the smallest candidate value,
 *             x_max[m], x_min[m] the lead positions s_p + o_a that attain them; the values are compared exactly, as
 *             numbers (+0 and -0 count as equal; a NaN, which only a failed factorisation gives, never wins), and
 *             among equal values the lowest candidate p A + a wins
 *   areas     area_pos[m] = integral of max(eta_m, 0) ds, area_neg[m] = integral of min(eta_m, 0) ds over [0, S], summed
 *             segment by segment in ascending p; a segment with ends u, v of the same sign gives 0.5 h (u + v), one whose
 *             ends differ in sign is split at the crossing t = u / (u - v): 0.5 u (h t) and 0.5 v (h - h t).  Times a
 *             line load q these are the classical maximum and minimum under a uniform live load placed on the
 *             favourable or the adverse lengths
 *
 *   trs_loss_rhs          b_m,f of the members e0 <= m < e0 + C  -> Z [B][C][ld_f]        (trs_loss.h, unchanged)
 *   trs_potrs_cases       K_ff z = b against the factored slab, L = C                    (trs_solver.h, unchanged)
 *   trs_influence_apply   Z, the path, d, the train -> eta, the envelope and the areas
 *
 * The members are taken in chunks [e0, e0 + C) as in trs_loss.h; the caller loops e0 = 0, C, 2 C, ... < nM_max.
 *
 * The apply kernel is one work-group of four waves per (truss, slice of the chunk).  Staged in LDS once per work-group:
 * the inverse of joint_out, the path translated through it into the solver's numbering, the s_p, per path joint the at
 * most three (reduced index, weight) pairs of d through free_index, and the train.  Every wave then takes one member at
 * a time: it gathers its 3 P entries of the Z row into an eta vector of its own in LDS, scaled by k_m, spreads its lanes
 * over the P A candidates (each axle's segment by binary search on the s_p), reduces max and min over the wave with the
 * candidate index carried beside the value, and sums the areas segment by segment in ascending p.  No scratch, no
 * atomics.
 *
 * OUT OF SCOPE: influence lines of support reactions and of joint displacements (reaction lines are linear combinations
 * of the eta this returns; a later change can sweep them); a subset of members; both travel directions in one call (the
 * caller reverses the path); several trains per call.
 */
#ifndef TRS_INFLUENCE_H
#define TRS_INFLUENCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_INFLUENCE_ABI_VERSION 1

int trs_influence_abi_version(void);

/* Whether the apply kernel's tables fit a CU's LDS (otherwise trs_influence_apply / trs_influence_tab_apply return
 * hipErrorInvalidValue).  Within 160 KB the kernel holds
 *   per path joint  8 doubles + 4 ints    (s_p, three weights of d, eta of each of the four waves; the translated joint,
 *                                          three reduced indices)
 *   per joint       1 int                 (the inverse of joint_out)
 *   per axle        2 doubles             (w_a, o_a)
 * the bytes rounded up to 16: the shape fits when nJ_max >= 0, P_max >= 0, A >= 1 and that sum does. */
int trs_influence_fits(int nJ_max, int P_max, int A);

/* The influence ordinates, envelopes and areas of the members e0 <= m < min(e0 + C, nM_max) of every truss (formulas:
 * the head of this file).  xyz, the members, free_index, nJ, nM: the batch's arrays as assembled (solver's numbering);
 * Z [B][C][ld_f] as trs_potrs_cases left it after trs_loss_rhs(e0, C).
 *   path      [B][P_max] int32    caller's numbering; entries at or beyond path_len[b] are ignored (an entry outside
 *                                 [0, nJ[b]) is read as the nearest joint id: the caller validates)
 *   path_len  [B] int32           P of truss b, 0 <= P <= P_max
 *   dir       [B][3]              the load vector d
 *   train_w, train_o  [A]         the axle weights and offsets, shared by the batch
 *   eta_out   [B][nM_max][P_max] or NULL (then not written): eta[m][p]; entries at or beyond path_len[b] zero
 *   N_max, N_min, x_max, x_min, area_pos, area_neg   [B][nM_max]
 *   joint_out [B][nJ_max] or NULL: the batch's joint order (solver's joint j is the caller's joint joint_out[b][j]); the
 *                                 kernel stages its inverse and translates the path through it
 * P = 0: both extremes and both areas 0, both positions NaN.  P = 1: the candidates are x = o_a, the areas 0.  A padding
 * member (nM[b] <= m < nM_max): zeros, positions NaN, its eta row zero.  A member with both ends held: eta identically 0.
 * A truss whose factorisation failed (info[b] != 0) gets meaningless numbers; the others are unaffected.  The table-form
 * twin carries the form in the middle of its name and takes (conn16, type_idx, types) where the general form takes
 * (conn, E, A); the same bits either way. */
int trs_influence_apply(int B, int e0, int C, int nJ_max, int nM_max, int P_max, int A, const double *xyz,
                        const int32_t *conn, const double *E, const double *Amem, const int32_t *free_index,
                        const int32_t *nJ, const int32_t *nM, const int32_t *path, const int32_t *path_len,
                        const double *dir, const double *train_w, const double *train_o, const double *Z, int ld_f,
                        double *eta_out /* or NULL */, double *N_max, double *N_min, double *x_max, double *x_min,
                        double *area_pos, double *area_neg, const int32_t *joint_out /* [B][nJ_max] or NULL */,
                        void *stream);
int trs_influence_tab_apply(int B, int e0, int C, int nJ_max, int nM_max, int P_max, int A, const double *xyz,
                            const uint16_t *conn16, const uint8_t *type_idx, const double *types,
                            const int32_t *free_index, const int32_t *nJ, const int32_t *nM, const int32_t *path,
                            const int32_t *path_len, const double *dir, const double *train_w, const double *train_o,
                            const double *Z, int ld_f, double *eta_out, double *N_max, double *N_min, double *x_max,
                            double *x_min, double *area_pos, double *area_neg, const int32_t *joint_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_INFLUENCE_H */
