/*
 * trs_spectrum.h - response spectrum analysis from the converged mode block (csrc/spectrum.hip; the entry points live
 * in libtrs_hip.so beside those of trs_solver.h, trs_modes.h and trs_modegrad.h, whose conventions hold here word for
 * word: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only enqueues
 * work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state that a
 * result depends on, no floating-point atomic is used and every sum runs in one fixed order - the results are
 * bit-reproducible from run to run, from stream to stream and between the two member forms, and the numbers of truss b
 * do not depend on B or on the other trusses of the batch).
 *
 * The problem.  The M-orthonormal block X and the Ritz values lam that trs_modes_step left, the lumped mass Mf and
 * n_mass of trs_modes_mass, and the ground-motion convention of trs_dynamics.h: every free DOF takes the component of
 * the direction vector on its own axis, the results are relative to the ground, only the mass on free DOFs takes part.
 * Shared by the batch: dirs [G][3] (1 <= G <= 3; need not be unit vectors, the length is a scale), a spectrum table
 * T [K], Sa [G][K] (2 <= K <= 64; T strictly ascending, T[0] >= 0; Sa finite and >= 0), zpa [G], a damping ratio zeta,
 * a rule (TRS_RS_SRSS, TRS_RS_CQC, TRS_RS_ABS) and the switch missing_mass.  1 <= p <= 8, n_modes = min(p, n_mass[b]).
 *
 * Per direction g and mode k < n_modes, over the free DOFs c (iota_c = dirs[g][axis(c)]):
 *     Gamma = sum_c Mf_c X_kc iota_c        mtot_g = sum_c Mf_c iota_c^2
 *     omega = sqrt(lam_k), T_k = 2 pi / omega
 *     sa    = the table at T_k, linear in T: i the largest index with T_i <= T_k, t = (T_k - T_i) / (T_(i+1) - T_i),
 *             sa = fma(t, Sa_(i+1) - Sa_i, Sa_i); below T[0] Sa[g][0], at or beyond T[K-1] Sa[g][K-1]
 *     q     = Gamma sa / lam_k              meff = Gamma^2 / mtot_g (0 where mtot_g = 0)
 * A mode whose lam_k is not positive and finite contributes nothing (Gamma, sa, meff, q = 0): no NaN reaches an output.
 * Order of the two sums: the DOFs are walked in JOINT layout d = 3 j + axis (d ascending, through free_index); thread
 * t of the 256 adds its d = t, t + 256, ... in that order, the 64 partials of a wave are folded by the butterfly
 * lane ^ 32, ^ 16, ... ^ 1, and the four waves' sums are added in wave order.
 *
 * Modal responses (signed; the sign is that of Gamma_k phi_k, so the sign of phi cancels), slot k < p:
 *     u_k = q_k phi_k      N_(m,k) = q_k ((E A / len) c . (phi_k(j1) - phi_k(j0)))      V_k = Gamma_k^2 sa_k
 *     R_k at a held DOF = the sum of the member end forces (+N c at end j1, -N c at end j0) of the joint's member ends
 *     in member-id order: the convention of trs_recover.
 * Missing mass (missing_mass != 0), slot p: f_g = zpa_g Mf (iota_g - sum_(k < n_modes) Gamma_kg X_k), k ascending by
 * fused multiply-adds from iota, goes to column g of the case block F (vector-major [B][16][ld_f]; the other 16 - G
 * columns and the padding are zero); the caller solves F by ONE trs_potrs_cases (L = 16, trs_solver.h, unchanged) and
 * hands it to trs_rs_combine: the solution is one more response vector per direction, correlated 0 with every mode and
 * 1 with itself, of base shear zpa_g (mtot_g - sum Gamma^2).
 *
 * Combination, for every displacement component, member force, reaction component and the base shear, over the slots
 * i, j of the V = p + 1:  sqrt(max(0, sum_i sum_j rho_ij r_i r_j)), i ascending and j ascending inside it.
 *     SRSS  rho = I (only the diagonal is summed)
 *     CQC   rho_ij = 8 zeta^2 (1 + b) b^1.5 / ((1 - b^2)^2 + 4 zeta^2 b (1 + b)^2), b = omega_j / omega_i (zeta > 0);
 *           rho_ii = 1 exactly; rho_ij = 0 where mode i or j contributes nothing
 *     ABS   sum_i |r_i|, the missing-mass slot included
 *
 * Outputs (any may be NULL, and then it is not computed), V = p + 1 slots:
 *     gamma, sa, meff      [B][G][p]                  mtot, base   [B][G]
 *     u, R                 [B][G][nJ_max][3]          caller's joint numbering, through joint_out
 *     N                    [B][G][nM_max]
 *     modal_u, modal_R     [B][G][V][nJ_max][3]       signed
 *     modal_N              [B][G][V][nM_max]          signed
 * u is zero at held DOFs, R is zero at free DOFs, both are zero on padding joints.  Zeros are written for the modes
 * k >= n_modes, for padding members and joints and for members of zero length; without missing_mass slot p of the modal
 * outputs is zeros.  nJ[b], nM[b] and end-joint ids are trimmed and clamped to the arrays: whatever the inputs hold,
 * nothing is read or written outside them; a member with an end joint outside the truss's own joints is on no end list
 * and gives zeros to N as to R.  A column of X whose lam contributes nothing is not read into any result.  A truss
 * whose factorisation failed gets meaningless numbers; the others are unaffected.
 *
 * Kernels.  trs_rs_modal: one work-group of 256 threads per truss over the DOF axis.  trs_rs_combine: one work-group of
 * 256 threads per truss; ALL response vectors of the truss (the p mode shapes once, plus the G missing-mass solutions
 * read from F) are staged in LDS in joint layout through free_index; every member is visited once by one thread, its
 * geometry in registers; one thread per joint forms u; for a joint with a held DOF one thread walks the joint's
 * member-end list in member-id order for R.  A shape whose vectors do not all fit is refused (trs_rs_fits).
 */
#ifndef TRS_SPECTRUM_H
#define TRS_SPECTRUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_RS_ABI_VERSION 1
#define TRS_RS_BLOCK 16 /* vectors per truss in X, F and lam: TRS_MODES_BLOCK of trs_modes.h */
#define TRS_RS_MAX_MODES 8 /* p at most: what one block delivers */
#define TRS_RS_MAX_VEC 9 /* response vectors per direction at most: the modes and the missing-mass slot */
#define TRS_RS_MAX_DIRS 3 /* G at most */
#define TRS_RS_MAX_TABLE 64 /* K at most */
#define TRS_RS_SRSS 0
#define TRS_RS_CQC 1
#define TRS_RS_ABS 2

int trs_rs_abi_version(void);

/* Whether a batch shape fits the combine kernel's LDS (160 KB per CU) with all its vectors, and 1 <= p <= 8:
 * 24 nJ_max (p + 3) bytes of response vectors, 704 bytes of rho and q and 4 (2 nJ_max + 1 + 2 nM_max) of end lists,
 * rounded up to 16.  Otherwise trs_rs_modal / trs_rs_combine / trs_rs_combine_tab return hipErrorInvalidValue. */
int trs_rs_fits(int nJ_max, int nM_max, int p);

/* free_index, n_free, nJ: the batch's arrays as assembled; X [B][16][ld_f], lam [B][16] as trs_modes_step left them;
 * Mf [B][ld_f], n_mass [B] of trs_modes_mass; dirs [G][3], T [K], Sa [G][K], zpa [G] (device).
 * Out: gamma, sa, meff [B][G][p], mtot, base [B][G] (each or NULL); q [B][G][p] and rho [B][8][8] (required: what
 * trs_rs_combine reads); F [B][16][ld_f] (required with missing_mass != 0: all 16 columns are written). */
int trs_rs_modal(int B, int nJ_max, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                 const double *X /* [B][16][ld_f] */, int ld_f, const double *lam /* [B][16] */,
                 const double *Mf /* [B][ld_f] */, const int32_t *n_mass /* [B] */, int p, int G,
                 const double *dirs /* [G][3] */, int K, const double *T /* [K] */, const double *Sa /* [G][K] */,
                 const double *zpa /* [G] */, double zeta, int rule, int missing_mass, double *gamma, double *sa,
                 double *meff /* [B][G][p] or NULL */, double *mtot, double *base /* [B][G] or NULL */,
                 double *q /* [B][G][p] */, double *rho /* [B][8][8] */, double *F /* [B][16][ld_f] or NULL */,
                 void *stream);

/* xyz, the members, free_index, n_free, nJ, nM: the batch's arrays as assembled (in the batch's joint order);
 * joint_out [B][nJ_max] (where the results of joint j go: the caller's id) or NULL; X as above; q and rho as
 * trs_rs_modal wrote them; F the SOLVED case block (missing_mass != 0) or NULL.  The `_tab` twin takes
 * (conn16, type_idx, types) where the general form takes (conn, E, A); the same bits either way. */
int trs_rs_combine(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                   const double *A, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                   const int32_t *nM, const int32_t *joint_out /* [B][nJ_max] or NULL */,
                   const double *X /* [B][16][ld_f] */, int ld_f, const int32_t *n_mass /* [B] */, int p, int G,
                   const double *q /* [B][G][p] */, const double *rho /* [B][8][8] */, int rule, int missing_mass,
                   const double *F /* [B][16][ld_f] or NULL */, double *u, double *R /* [B][G][nJ_max][3] or NULL */,
                   double *N /* [B][G][nM_max] or NULL */, double *modal_u,
                   double *modal_R /* [B][G][p + 1][nJ_max][3] or NULL */,
                   double *modal_N /* [B][G][p + 1][nM_max] or NULL */, void *stream);
int trs_rs_combine_tab(int B, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                       const uint8_t *type_idx, const double *types, const int32_t *free_index, const int32_t *n_free,
                       const int32_t *nJ, const int32_t *nM, const int32_t *joint_out, const double *X, int ld_f,
                       const int32_t *n_mass, int p, int G, const double *q, const double *rho, int rule,
                       int missing_mass, const double *F, double *u, double *R, double *N, double *modal_u,
                       double *modal_R, double *modal_N, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_SPECTRUM_H */
