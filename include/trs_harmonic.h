/*
 * trs_harmonic.h - steady-state harmonic response over a frequency sweep, by mode superposition on the converged mode
 * block with a static correction for the truncated modes (csrc/harmonic.hip; the entry points live in libtrs_hip.so
 * beside those of trs_solver.h, trs_modes.h, trs_modegrad.h and trs_spectrum.h, whose conventions hold here word for
 * word: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only enqueues
 * work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state that a
 * result depends on, no floating-point atomic is used and every sum runs in one fixed order - the results are
 * bit-reproducible from run to run, from stream to stream and between the two member forms, the numbers of case l do
 * not depend on L or on the other cases, and the numbers of truss b do not depend on B or on the other trusses).
 *
 * The problem.  Over the free DOFs:  M u'' + C u' + K_ff u = Re(f e^(i W t)),  u(t) = Re(U e^(i W t)),  with the
 * M-orthonormal block X and the Ritz values lam that trs_modes_step left, the lumped mass Mf and n_mass of
 * trs_modes_mass, 1 <= p <= 8 and n_modes = min(p, n_mass[b]).  Per case l (1 <= L <= 16: one case group of
 * trs_potrs_cases) the load is real, so all loads of a case share one phase:
 *     f_lc = fma(-Mf_c, ag_l[axis(c)], P_lc)
 * P_l a joint load pattern reduced by trs_gather_cases (Pr, or none: 0), ag_l a ground-acceleration amplitude [3] (or
 * none: 0); with a ground acceleration every free DOF takes the component of its own axis and the results are relative
 * to the ground (the convention of trs_dynamics.h).  Shared by the batch: the circular forcing frequencies omega [S]
 * (every value >= 0 and finite, any order, S >= 1), a modal damping ratio zeta and Rayleigh's damp_mass (alpha) and
 * damp_stiff (beta_R) of trs_dynamics.h: all three >= 0 and at least one > 0, else hipErrorInvalidValue.
 *
 * A mode k < n_modes takes part when lam_k is positive and finite; any other mode contributes nothing and its column of
 * X is never read.  w_k = sqrt(lam_k), zeta_k = zeta + damp_mass / (2 w_k) + damp_stiff w_k / 2 > 0: no denominator
 * below can vanish and no NaN or Inf reaches an output of a healthy truss.
 *     g_lk   = sum_c X_kc f_lc             the DOFs are walked in JOINT layout d = 3 j + axis (d ascending, through
 *                                          free_index); thread t of the 256 adds its d = t, t + 256, ... in that order by
 *                                          fused multiply-adds, the 64 partials of a wave are folded by the butterfly
 *                                          lane ^ 32, ^ 16, ... ^ 1, and the four waves' sums are added in wave order
 *     rhs_lc = f_lc, then fma(-g_lk, Mf_c X_kc, .) for k ascending      -> column l of F [B][16][ld_f]
 *     u_res  = inv(K_ff) rhs_l             ONE trs_potrs_cases (L = 16, trs_solver.h, unchanged) by the caller, between
 *                                          the two kernels; real, the same for every W
 *     dr = fma(-W, W, lam_k);  di = (2 zeta_k w_k) W;  n2 = fma(dr, dr, di di);  Hr = dr / n2;  Hi = -di / n2
 *     c_lk(W) = (g_lk Hr, g_lk Hi)
 * For any linear response quantity y (a displacement component, a member force N = (E A / len) c . (u(j1) - u(j0)), a
 * reaction component), y_k its real value under mode shape k and y_res its value under u_res (0 with residual = 0):
 *     Re y = y_res, then fma(y_k, Re c_lk, .) for k ascending;   Im y = 0, then fma(y_k, Im c_lk, .) for k ascending
 *     |y|  = sqrt(fma(Re y, Re y, Im y Im y))
 * At W = 0, Im y is exactly 0 and Re y is the static solution of f_l.  A reaction at a held DOF is the sum of the member
 * end forces (+N c at end j1, -N c at end j0) of the joint's member ends in member-id order: the convention of
 * trs_recover.
 *
 * What this does not claim.  The residual is STATIC: damping and inertia of the truncated modes are ignored.  The
 * answer is the standard mode-acceleration one, good for W well below the w of the first mode left out; near or above
 * it, more modes are needed.
 *
 * Outputs of the sweep (any may be NULL, and then it is not computed; caller's joint numbering through joint_out,
 * except the monitors):
 *     u_amp, R_amp   [B][L][nJ_max][3]     N_amp   [B][L][nM_max]      the largest amplitude |y| over the sweep
 *     u_at, R_at, N_at (int32, same shapes)                            the FIRST index s that attains it: index 0
 *                                                                      initialises, a later s replaces only when
 *                                                                      strictly greater
 *     frf_u   [B][L][S][Pj][3][2]          frf_N   [B][L][S][Pm][2]    (Re, Im) at every frequency for the monitored
 *                                                                      joints mon_joint [B][Pj] and members mon_member
 *                                                                      [B][Pm] (int32, DEVICE numbering, -1 = none, as
 *                                                                      in trs_dyn_step); zeros for -1 or an id outside
 *                                                                      the truss
 * Amplitude and index are both 0 for u at held DOFs, R at free DOFs, padding joints and members, members of zero
 * length and members with an end outside the truss.  Every entry of every output that is asked for is written, whatever
 * it held before.  nJ[b], nM[b] and end-joint ids are trimmed and clamped to the arrays: whatever the inputs hold,
 * nothing is read or written outside them.  A truss whose factorisation failed gets meaningless numbers; the others are
 * unaffected.
 *
 * Kernels.  trs_hr_modal: grid (B, L), 256 threads over the DOF axis.  trs_hr_sweep: grid (B, L), 256 threads; the p
 * mode shapes and the case's u_res are staged in LDS in joint layout through free_index (zero at held DOFs and past the
 * truss's own joints); c_lk(W_s) of one chunk of TRS_HR_CHUNK frequencies is built cooperatively in LDS ([chunk][8]
 * complex) and read by all lanes at the same address; three passes (members, joints for u, joints with a held DOF for
 * R) each form the p + 1 real coefficients of an item once, in registers, and run the frequencies against the table.
 * The monitors take the same path, so their values and the envelopes are the same numbers.
 */
#ifndef TRS_HARMONIC_H
#define TRS_HARMONIC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_HR_ABI_VERSION 1
#define TRS_HR_BLOCK 16 /* vectors per truss in X, F and lam: TRS_MODES_BLOCK of trs_modes.h; L at most */
#define TRS_HR_MAX_MODES 8 /* p at most: what one block delivers */
#define TRS_HR_MAX_VEC 9 /* response vectors per case: the modes and the residual */
#define TRS_HR_CHUNK 64 /* frequencies per coefficient table */

int trs_hr_abi_version(void);

/* Whether a batch shape fits the sweep kernel's LDS (160 KB per CU), and 1 <= p <= 8: 24 nJ_max (p + 1) bytes of
 * response vectors, 8192 bytes of coefficient table (64 x 8 complex), 64 bytes of g and 4 (2 nJ_max + 1 + 2 nM_max) of
 * end lists, rounded up to 16.  Otherwise trs_hr_sweep / trs_hr_sweep_tab return hipErrorInvalidValue. */
int trs_hr_fits(int nJ_max, int nM_max, int p);

/* free_index, n_free, nJ: the batch's arrays as assembled; X [B][16][ld_f], lam [B][16] as trs_modes_step left them;
 * Mf [B][ld_f], n_mass [B] of trs_modes_mass; Pr [B][L][ld_f] (reduced load patterns) or NULL, ag [B][L][3] or NULL, at
 * least one of them.  Out: g [B][L][p] (zeros for the modes that contribute nothing); with residual != 0 all 16 columns
 * of F [B][16][ld_f]: column l the residual load, columns L .. 15 and the padding zero. */
int trs_hr_modal(int B, int L, int nJ_max, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                 const double *X /* [B][16][ld_f] */, int ld_f, const double *lam /* [B][16] */,
                 const double *Mf /* [B][ld_f] */, const int32_t *n_mass /* [B] */, int p,
                 const double *Pr /* [B][L][ld_f] or NULL */, const double *ag /* [B][L][3] or NULL */, int residual,
                 double *g /* [B][L][p] */, double *F /* [B][16][ld_f] or NULL */, void *stream);

/* xyz, the members, free_index, n_free, nJ, nM: the batch's arrays as assembled (in the batch's joint order);
 * joint_out [B][nJ_max] (where the results of joint j go: the caller's id) or NULL; X, lam, n_mass as above; g as
 * trs_hr_modal wrote it; F the SOLVED case block (the residual is on) or NULL (off); omega [S] (device).  The `_tab`
 * twin takes (conn16, type_idx, types) where the general form takes (conn, E, A); the same bits either way. */
int trs_hr_sweep(int B, int L, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                 const double *A, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                 const int32_t *nM, const int32_t *joint_out /* [B][nJ_max] or NULL */,
                 const double *X /* [B][16][ld_f] */, int ld_f, const double *lam /* [B][16] */,
                 const int32_t *n_mass /* [B] */, int p, const double *g /* [B][L][p] */,
                 const double *F /* [B][16][ld_f] or NULL */, int S, const double *omega /* [S] */, double zeta,
                 double damp_mass, double damp_stiff, double *u_amp, int32_t *u_at /* [B][L][nJ_max][3] or NULL */,
                 double *R_amp, int32_t *R_at /* [B][L][nJ_max][3] or NULL */, double *N_amp,
                 int32_t *N_at /* [B][L][nM_max] or NULL */, const int32_t *mon_joint /* [B][Pj] */, int Pj,
                 const int32_t *mon_member /* [B][Pm] */, int Pm, double *frf_u /* [B][L][S][Pj][3][2] or NULL */,
                 double *frf_N /* [B][L][S][Pm][2] or NULL */, void *stream);
int trs_hr_sweep_tab(int B, int L, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                     const uint8_t *type_idx, const double *types, const int32_t *free_index, const int32_t *n_free,
                     const int32_t *nJ, const int32_t *nM, const int32_t *joint_out, const double *X, int ld_f,
                     const double *lam, const int32_t *n_mass, int p, const double *g, const double *F, int S,
                     const double *omega, double zeta, double damp_mass, double damp_stiff, double *u_amp,
                     int32_t *u_at, double *R_amp, int32_t *R_at, double *N_amp, int32_t *N_at,
                     const int32_t *mon_joint, int Pj, const int32_t *mon_member, int Pm, double *frf_u,
                     double *frf_N, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_HARMONIC_H */
