/*
 * trs_dynamics.h - transient response by Newmark time stepping on a resident Cholesky factor of K_ff + sigma M
 * (csrc/dynamics.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h, whose conventions hold here
 * word for word: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only
 * enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state
 * that a result depends on, no floating-point atomic is used and every sum runs in one fixed order - the results are
 * bit-reproducible from run to run, from stream to stream and between the two member forms, case l does not depend on L
 * or on the other cases, and the numbers of truss b do not depend on B or on the other trusses).
 *
 * The problem.  M u'' + C u' + K_ff u = f(t) over the free DOFs of a truss; M the LUMPED mass Mf of trs_modes.h
 * (trs_modes_mass, called as it is), C = damp_mass M + damp_stiff K_ff (Rayleigh: alpha, beta_R >= 0).  Case l at step n
 * is loaded with
 *     f = scale[b][l][n] P[b][l]  -  M iota(ag[b][l][n][:])
 * P a load pattern, reduced ONCE by trs_gather_cases; scale a time function (NULL: 1); ag a ground acceleration (NULL:
 * 0), of which every free DOF takes the component of its own axis - the displacements are then relative to the ground.
 *
 * The scheme (Newmark beta, gamma; step dt).  With
 *     a0 = 1 / (beta dt^2)    a1 = gamma / (beta dt)   a2 = 1 / (beta dt)
 *     a3 = 1 / (2 beta) - 1   a4 = gamma / beta - 1    a5 = dt / 2 (gamma / beta - 2)
 *     s = 1 + a1 beta_R       sigma = (a0 + a1 alpha) / s
 * the matrix K_ff + sigma M is factored ONCE (trs_assemble, trs_dyn_shift, trs_potrf_batched) and every step is
 *     w       = a1 u + a4 v + a5 a
 *     rhs     = f_(n+1) + M [(a0 + alpha a1) u + (a2 + alpha a4) v + (a3 + alpha a5) a] + beta_R K_ff w
 *     (K_ff + sigma M) u_(n+1) = rhs / s                        trs_potrs_cases (trs_solver.h, unchanged)
 *     a_(n+1) = a0 (u_(n+1) - u_n) - a2 v_n - a3 a_n
 *     v_(n+1) = v_n + dt ((1 - gamma) a_n + gamma a_(n+1))
 * K_ff w is formed member by member (the slab holds the factor, no K): s_m = k c . (w_j1 - w_j0) with w zero at held
 * DOFs (trs_rec::member_axial), then per joint the sum of +- s_m c over its member ends in member-id order
 * (build_end_lists, add_end_force) - the shape of trs_effects_rhs.  With beta_R = 0 none of this is built or run.
 * Start: u_0 = v_0 = 0, a_0 = f_0 / M at the DOFs of positive mass and 0 elsewhere (first = 1); or the state U, V, Acc that
 * an earlier run left (first = 2).
 *
 *   trs_modes_mass    Mf                                                      once      (trs_modes.h, unchanged)
 *   trs_assemble      K_ff into the slab                                      once      (trs_solver.h, unchanged)
 *   trs_dyn_shift     S[c][c] += sigma Mf[c]                                  once
 *   trs_potrf_batched the factor of K_ff + sigma M                            once      (trs_solver.h, unchanged)
 *   trs_gather_cases  P -> Pr [B][L][ld_f]                                    once      (trs_solver.h, unchanged)
 *   trs_dyn_step      first != 0: step 0 and the right-hand side of step 1    once
 *   repeat  trs_potrs_cases   F <- u_n                                        two launches per time step
 *           trs_dyn_step      step n = 1 .. T
 *   trs_dyn_collect   u, v, a of the last step in the caller's numbering      once
 *
 * The diagonal in the slab (trs_solver.h "Slab layout"): truss b owns slab_rows * ld doubles, row c of
 * which holds K_ff[c][i] for 16 floor(c / 16) <= i, so the diagonal entry of row c is S[b][c][c] = S[(b * slab_rows + c)
 * * ld + c] in every mode that writes a slab.  trs_assemble always writes the diagonal 16 x 16 tile of every row chunk:
 * a row's stored columns start at its diagonal tile (i_lo = 16 chunk, or 0 in the full-symmetric mode) and end at
 * cend[chunk] >= chunk + 1 with envelope metadata (the whole row without), and bit 0 of a chunk's tile mask is set before
 * any member is looked at ("the diagonal tile always holds entries"), so the masked row loop never skips it.
 * trs_dyn_shift therefore touches written entries only.  The compact member form of the assembly (TRS_ASM_COMPACT)
 * writes no slab and cannot be shifted: callers must not combine the two.
 *
 * Buffers (device, double unless said otherwise).  Pr, F, U, V, Acc: CASE-MAJOR [B][L][ld_f], ld_f >= slab_rows, row
 * (b, l) the reduced vector of case l (entries c < n_free[b] in the order of free_index, the padding up to n_pad =
 * round_up(n_free, 64) zero).  Mf [B][ld_f] as trs_modes_mass wrote it.  scale [B][L][T1], ag [B][L][T1][3], T1 = T + 1
 * the number of time points of this run, point 0 the start.
 * Envelopes, per (b, l), over the time points 0 .. T of THIS run, in the CALLER's joint numbering (through joint_out, as
 * trs_recover_cases writes u):
 *   u_peak [B][L][nJ_max][3] = max |u|, u_step (int32) the FIRST point that attains it
 *   N_max, N_min [B][L][nM_max] the signed extremes of N_m = k c . (u_j1 - u_j0), N_max_step, N_min_step (int32) likewise
 * (point 0 initialises them, a later point replaces an entry only when strictly greater / smaller: exact and
 * deterministic; held DOFs, padding joints and padding members hold 0 at step 0).
 * Monitors: mon_joint [B][Pj], mon_member [B][Pm] (int32, DEVICE joint numbering - the batch's order -, -1 = none) select
 * what is written at every point: hist_u [B][L][T1][Pj][3], hist_N [B][L][T1][Pm] (zeros for -1 or an id outside the truss).
 * A truss whose factorisation failed (info[b] != 0) gets meaningless numbers; the others are unaffected.
 *
 * LDS per work-group (trs_dyn_fits): one DOF vector, 3 nJ_max doubles = 24 nJ_max bytes; with beta_R > 0 also one double
 * per member and the member-end lists, (3 nJ_max + nM_max) doubles and (2 nJ_max + 1 + 2 nM_max) ints = 32 nJ_max +
 * 16 nM_max + 4 bytes - the rule of trs_effects_fits -, rounded up to 16, within 160 KB.
 * The step kernel trims nJ[b], nM[b] and n_free[b] to the arrays, clamps end-joint ids to them (as the stage of the
 * column analyses does) and builds the end lists of the truss's own joints only: whatever the inputs hold, nothing is
 * read or written outside the arrays.
 */
#ifndef TRS_DYNAMICS_H
#define TRS_DYNAMICS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_DYN_ABI_VERSION 1

int trs_dyn_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS (see above; otherwise trs_dyn_step / trs_dyn_tab_step
 * return hipErrorInvalidValue).  damped != 0: beta_R > 0. */
int trs_dyn_fits(int nJ_max, int nM_max, int damped);

/* S[b][c][c] = fma(sigma, Mf[b][c], S[b][c][c]) for c < n_free[b], on the ASSEMBLED slab [B][slab_rows][ld], between
 * trs_assemble and trs_potrf_batched. */
int trs_dyn_shift(int B, const int32_t *n_free, int ld, int slab_rows, double *S, const double *Mf, int ld_f,
                  double sigma, void *stream);

/* Time point n of this run (0 <= n < T1) for all L cases of every truss; one 256-thread work-group per truss.
 * first = 1 (n = 0): U = V = 0, Acc = f_0 / M; first = 2 (n = 0): U, V, Acc as they are.  Either way the envelopes and
 * the monitor rows of point 0 are written and F receives the right-hand side of point 1 (unless T1 = 1).
 * first = 0 (n >= 1): F holds u_n as trs_potrs_cases left it; U, V, Acc are updated in place, the envelopes updated, the
 * monitor rows of point n written, and F receives the right-hand side of point n + 1 unless n = T1 - 1.
 * xyz, the members, free_index, n_free, nJ, nM: the batch's arrays as assembled.  The `_tab` twin carries the form in
 * the middle of its name, as trs_recover_tab_cases does, and takes (conn16, type_idx, types) where the general form
 * takes (conn, E, A); the same bits either way. */
int trs_dyn_step(int B, int L, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                 const double *A, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                 const int32_t *nM, const double *Mf, const double *Pr /* [B][L][ld_f] */,
                 const double *scale /* [B][L][T1] or NULL */, const double *ag /* [B][L][T1][3] or NULL */, int T1,
                 int n, int first, double dt, double beta, double gamma, double damp_mass, double damp_stiff,
                 double *F /* inout [B][L][ld_f] */, double *U, double *V, double *Acc, int ld_f, double *u_peak,
                 int32_t *u_step, double *N_max, int32_t *N_max_step, double *N_min, int32_t *N_min_step,
                 const int32_t *mon_joint /* [B][Pj] */, int Pj, const int32_t *mon_member /* [B][Pm] */, int Pm,
                 double *hist_u, double *hist_N, const int32_t *joint_out /* [B][nJ_max] or NULL */, void *stream);
int trs_dyn_tab_step(int B, int L, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                     const uint8_t *type_idx, const double *types, const int32_t *free_index, const int32_t *n_free,
                     const int32_t *nJ, const int32_t *nM, const double *Mf, const double *Pr, const double *scale,
                     const double *ag, int T1, int n, int first, double dt, double beta, double gamma,
                     double damp_mass, double damp_stiff, double *F, double *U, double *V, double *Acc, int ld_f,
                     double *u_peak, int32_t *u_step, double *N_max, int32_t *N_max_step, double *N_min,
                     int32_t *N_min_step, const int32_t *mon_joint, int Pj, const int32_t *mon_member, int Pm,
                     double *hist_u, double *hist_N, const int32_t *joint_out, void *stream);

/* u, v, a [B][L][nJ_max][3] from U, V, Acc, written through joint_out into the caller's numbering; zero at held DOFs
 * and on the padding joints. */
int trs_dyn_collect(int B, int L, int nJ_max, const double *U, const double *V, const double *Acc, int ld_f,
                    const int32_t *free_index, const int32_t *nJ, const int32_t *joint_out /* [B][nJ_max] or NULL */,
                    double *u, double *v, double *a, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_DYNAMICS_H */
