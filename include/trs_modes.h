/*
 * trs_modes.h - natural frequencies and mode shapes from the resident Cholesky factor (csrc/modes.hip; the entry
 * points live in libtrs_hip.so beside those of trs_solver.h, whose conventions hold here word for word: every pointer
 * is a DEVICE pointer owned by the caller, the library allocates nothing, every call only enqueues work on `stream`
 * (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state that a result depends
 * on, no floating-point atomic is used and every sum runs in one fixed order - the results are bit-reproducible from
 * run to run, from stream to stream and between the two member forms, and the numbers of truss b do not depend on B
 * or on the other trusses of the batch).
 *
 * The problem.  K_ff phi = lambda M phi over the free DOFs of a truss, M the LUMPED mass matrix: joint j carries
 *     m_j = mass_scale * sum over the member ends at j of 1/2 (a * length * density)  +  joint_mass_j
 * on each of its three DOFs (the member term is half of the reference's Member.weight, the product formed in that
 * order; the ends of a joint are summed in member-id order).  mass_scale lets a caller whose densities are weight
 * densities pass 1 / g; joint_mass (caller's joint numbering, or NULL) is non-structural mass.  The lowest pairs
 * (lambda_i = omega_i^2, phi_i) are found by block inverse (subspace) iteration against the factor that
 * trs_potrf_batched left in the slab - no second factorisation, no product with K:
 *
 *   trs_modes_mass    Mf, n_mass                                    once
 *   trs_modes_step    first = 1: the start block X and F = M X      once
 *   repeat   trs_potrs_cases (L = 16)     F <- Y = inv(K_ff) F      (trs_solver.h "Load cases", unchanged)
 *            trs_modes_step               one Rayleigh-Ritz step:  K_r = Y^T M X (= Y^T K Y),  M_r = Y^T M Y,
 *                                         K_r Q = M_r Q Lambda (Cholesky of M_r, cyclic Jacobi, ascending order),
 *                                         X <- Y Q (M-orthonormal),  F <- M X,  lam = diag(Lambda)
 *   trs_modes_shapes  the first p columns of X in the caller's joint numbering
 *
 * Buffers (device, double unless said otherwise).  X and F are blocks of TRS_MODES_BLOCK = 16 vectors per truss in the
 * layout of the load cases' right-hand sides: VECTOR-MAJOR [B][16][ld_f], ld_f >= slab_rows, row (b, k) the reduced
 * vector k of truss b (entries c < n_free[b] in the order of free_index, the padding n_free[b] <= c < n_pad zero,
 * n_pad = round_up(n_free, 64)).  Mf [B][ld_f]: the mass of every free DOF in the same numbering, zero on the padding.
 * n_mass [B] (int32): the number of free DOFs of positive mass.  Truss b iterates q_b = min(16, n_mass[b]) vectors (the
 * other columns of X and F stay zero and out of the reduced problem) and delivers n_modes = min(p, n_mass[b]) pairs.
 * lam, resid [B][16]; state [B] (int32): 0 while the truss iterates, else the iteration number at which it was frozen.
 *
 * Residual.  K (Y Q) = M (X Q), so with Phi = Y Q the kernel forms, without a stiffness product, the true relative
 * residual of pair i,  resid_i = |(X Q)_i - lam_i Phi_i|_M / |lam_i Phi_i|_M  (|v|_M^2 = sum_c Mf_c v_c^2).  It is
 * computed on the steps with check != 0 only (it costs one more read of X); other steps leave resid as it was.
 * Freezing.  On a step with check != 0 a truss whose first n_modes residuals are all <= tol is marked
 * state[b] = iter; its F rows are zeroed once (the substitutions that still run over the whole batch then work on
 * zeros instead of powers of inv(K) that would overflow) and every later call leaves its X, lam, resid untouched.
 * A truss therefore stops at its own check point: its bits do not depend on the slowest truss of the batch.
 * A truss whose factorisation failed (info[b] != 0) gets meaningless numbers; the others are unaffected.
 * lam_i for i >= q_b is NaN.  The slab is only read (by trs_potrs_cases).
 *
 * Start block: X[c][k] = a fixed integer hash (one splitmix64 step) of 16 c + k mapped into (-1, 1), c the reduced
 * DOF index: no state, no dependence on b or B.
 *
 * Cost per truss and step: the kernel is one wave per truss; both Gram matrices and the rotation are 16-wide products
 * over the DOF axis on v_mfma_f64_16x16x4_f64, the 16 x 16 reduced problem lives in the wave's LDS.  It reads Y twice
 * and X once (twice on a checking step) and writes X and F: five (six) streams of 16 n_pad doubles.
 */
#ifndef TRS_MODES_H
#define TRS_MODES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_MODES_ABI_VERSION 1
#define TRS_MODES_BLOCK 16 /* vectors per truss = one case group of trs_potrs_cases */

int trs_modes_abi_version(void);

/* The mass kernel holds one int2 and one double per member of a truss in a CU's LDS: whether a batch shape qualifies
 * (otherwise trs_modes_mass / trs_modes_tab_mass return hipErrorInvalidValue). */
int trs_modes_fits(int nJ_max, int nM_max);

/* Lumped masses of the free DOFs.  xyz, the members, free_index, n_free, nJ, nM: the batch's arrays as assembled (in
 * the batch's joint order); joint_mass [B][nJ_max] in the CALLER's numbering with joint_in [B][nJ_max] the batch's joint
 * order (the perm of trs_joint_order: the old id of the joint that became joint j; NULL = none), or NULL.
 * The `_tab` twin carries the form in the middle of its name, as trs_recover_tab_cases does, and takes
 * (conn16, type_idx, types) where the general form takes (conn, A, rho); the same bits either way. */
int trs_modes_mass(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *A,
                   const double *rho, const double *joint_mass /* [B][nJ_max] or NULL */,
                   const int32_t *joint_in /* [B][nJ_max] or NULL */, double mass_scale, const int32_t *free_index,
                   const int32_t *n_free, const int32_t *nJ, const int32_t *nM, double *Mf /* out [B][ld_f] */,
                   int ld_f, int32_t *n_mass /* out [B] */, void *stream);
int trs_modes_tab_mass(int B, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                       const uint8_t *type_idx, const double *types, const double *joint_mass,
                       const int32_t *joint_in, double mass_scale, const int32_t *free_index, const int32_t *n_free,
                       const int32_t *nJ, const int32_t *nM, double *Mf, int ld_f, int32_t *n_mass, void *stream);

/* One Rayleigh-Ritz step of every truss with state[b] == 0 (see above).  first != 0: there is no Y yet - state, lam
 * and resid are reset (0, NaN, NaN), the start block goes to X and M X to F; check and iter are ignored.
 * Otherwise F holds Y as trs_potrs_cases left it and X the block of the previous step; iter >= 1 is the number of this
 * step, 1 <= p <= 16 the number of pairs whose residuals decide (check != 0) whether the truss is frozen. */
int trs_modes_step(int B, int p, const int32_t *n_free, const int32_t *n_mass, const double *Mf,
                   double *F /* inout [B][16][ld_f] */, double *X /* inout [B][16][ld_f] */, int ld_f,
                   double *lam /* [B][16] */, double *resid /* [B][16] */, int32_t *state /* [B] */, int first,
                   int check, int iter, double tol, void *stream);

/* phi [B][p][nJ_max][3]: column k < p of X at the free DOFs of every joint, written through joint_out (the batch's joint
 * order, or NULL) into the caller's numbering; zero at constrained DOFs and on the padding joints.  Sign: the
 * component of largest magnitude (the first one in the caller's DOF order on a tie) is positive. */
int trs_modes_shapes(int B, int p, int nJ_max, const double *X, int ld_f, const int32_t *free_index,
                     const int32_t *nJ, const int32_t *joint_out /* [B][nJ_max] or NULL */,
                     double *phi /* out [B][p][nJ_max][3] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_MODES_H */
