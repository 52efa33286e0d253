/*
 * trs_buckling.h - linear buckling: critical load factors from shifted factors of K + theta Kg (csrc/buckling.hip; the
 * entry points live in libtrs_hip.so beside those of trs_solver.h, whose conventions hold here word for word: every
 * pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only enqueues work on
 * `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state that a result
 * depends on, no floating-point atomic is used and every sum runs in one fixed order - the results are bit-reproducible
 * from run to run, from stream to stream and between the two member forms, and the numbers of truss b do not depend on B
 * or on the other trusses).
 *
 * The mathematics (the numpy yardstick tests/buckling_reference.py and the kernels state it in the same words).
 * Reference state.  N_m is the linear member force under the batch's own loads, formed with trs_rec::member_axial from
 * the reduced linear solution uf, so that it has the bits of trs_recover.  g_m = N_m / L0_m, n_m the undeformed direction.
 * Problem.  K_ff phi = lambda H phi with H = -Kg.  Per member Kg is g_m (I - n n^T), entered as + on the two diagonal
 * joint blocks and - on the two off-diagonal ones.  A positive lambda scales the load as applied; a negative lambda
 * means buckling under the reversed load.
 * Shift.  For a per-truss shift theta_b >= 0 with Kbar = K_ff + theta Kg positive definite, iterate on
 * H phi = nu Kbar phi.  Then lambda = theta + 1 / nu, and the largest |nu| is the eigenvalue nearest theta.
 *
 * One iteration on a block of TRS_BK_BLOCK = 16 vectors, in the VECTOR-MAJOR layout of the load cases ([B][16][ld_f],
 * row (b, k) the reduced vector k of truss b, entries c < n_free[b] in the order of free_index, the padding
 * n_free[b] <= c < n_pad = round_up(n_free, 64) zero; ld_f a multiple of 64):
 *     trs_potrs_cases (L = 16)   F <- Y = inv(Kbar) F         (trs_solver.h "Load cases", unchanged)
 *     trs_bk_product             G = H Y
 *     trs_bk_step                A_r = Y^T G,  B_r = Y^T Fk  (Fk: the copy of F that the last step kept; B_r equals
 *                                Y^T Kbar Y, so no stiffness product is needed),
 *                                A_r Q = B_r Q diag(nu), ordered by |nu| descending (ties by index),
 *                                X <- Y Q,  F <- G Q,  Fk <- G Q,  lam = theta + 1 / nu,
 *                                residual of pair i = |(G Q)_i - nu_i (Fk Q)_i|_2 / |nu_i (Fk Q)_i|_2
 *                                (no further product: H X_new = G Q and Kbar X_new = Fk Q)
 * This is one product launch, one substitution and one step launch per iteration.  The first block F = Fk is the start
 * block of trs_modes.h (one splitmix64 step of 16 c + k, columns k < min(16, n_free)): the first step is a Rayleigh-Ritz
 * step on inv(Kbar) of it, every later F is H X.
 *
 * Rank.  H can have any rank - zero for zero load, low when few members carry force.  The step deflates B_r: with
 * B_r = V D V^T (cyclic Jacobi on the 16 x 16 matrix) the directions with D_k <= 2^-40 max D are dropped; r_b are left,
 * T = V_r D_r^-1/2, C = T^T A_r T = W diag(nu) W^T (cyclic Jacobi, r_b x r_b), Q = T W.  The truss then iterates
 * r_b < 16 vectors and the remaining columns of X, F, Fk are zero.  After the first step B_r is about diag(nu^2) in
 * the basis of X, so a pair with |nu| below 2^-20 of the largest leaves the block with the exact null directions.
 * rank[b] = r_b; n_modes = min(p, r_b); r_b = 0 gives n_modes = 0.  lam_i and resid_i for i >= r_b are NaN.
 *
 * State and freezing (as trs_modes_step).  state [B] (int32): 0 while the truss iterates, > 0 the iteration number at
 * which it was frozen, < 0 (set by the caller before the call with first != 0) the truss takes no part in this round.
 * On a step with check != 0 a truss whose first n_modes residuals are all <= tol is marked state[b] = iter; its F rows
 * are zeroed once (the substitutions that still run over the whole batch then work on zeros) and every later call leaves
 * its X, lam, resid and rank untouched.  A truss therefore stops at its own check point: its bits do not depend on the
 * slowest truss of the batch.
 *
 * The search for the smallest positive factor is the host's (DeviceBatch.buckling): round 0 at theta = 0 on the plain
 * factor; a truss is done with its critical factor once the p converged pairs nearest theta contain a positive lambda
 * (the smallest of them is the smallest positive eigenvalue, since Kbar positive definite leaves none in (0, theta]); it
 * is done without one once r_b < p (the whole spectrum has been seen); otherwise all p pairs are negative and converged,
 * no eigenvalue lies within d = max_i |lambda_i - theta| of theta, and theta' = theta + d is strictly below the smallest
 * positive factor: Kbar stays positive definite and theta at least doubles per round.  Per round: trs_bk_members with
 * the new theta (the table W), trs_assemble, trs_nl_tangent with W - delta_m = -theta g n n^T + theta g I, so the slab
 * holds K + theta Kg -, trs_potrf_batched, then the iteration above.
 *
 * LDS per work-group (trs_bk_fits): the member kernel holds u in joint layout (3 nJ_max doubles); the product kernel
 * the member table (4 nM_max doubles), the member-end lists with the far joint of every entry (2 nJ_max + 1 + 4 nM_max
 * ints) and a chunk of vc vectors in joint layout (3 nJ_max vc doubles), vc the largest of 16, 8, 4, 2, 1 that fits
 * 160 KB; a shape fits when vc = 1 does.  Every kernel trims nJ[b], nM[b] and n_free[b] to the arrays and clamps
 * end-joint ids to them (as the stage of the column analyses does): whatever the inputs hold, nothing is read or
 * written outside the arrays.
 */
#ifndef TRS_BUCKLING_H
#define TRS_BUCKLING_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_BK_ABI_VERSION 1
#define TRS_BK_BLOCK 16 /* vectors per truss = one case group of trs_potrs_cases */

int trs_bk_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS (see above; otherwise trs_bk_members and trs_bk_product
 * return hipErrorInvalidValue). */
int trs_bk_fits(int nJ_max, int nM_max);

/* The reference state; one 256-thread work-group per truss.  xyz, the members, free_index, n_free, nJ, nM: the batch's
 * arrays as assembled; uf [B][ld_uf]: the reduced linear solution (trs_potrs_batched / trs_potrs_cases); theta [B] or
 * NULL (= 0).  Out: N [B][nM_max] (zero on the padding members), ends [B][nM_max][2] (int32: the end joints, for
 * trs_bk_product - one entry point then serves both member forms), Mt [B][nM_max][4] = (n0, n1, n2, g) and the table of
 * trs_nl_tangent W [B][nM_max][6] = (n0, n1, n2, -theta g, +theta g, N).  The `_tab` twin takes (conn16, type_idx,
 * types) where the general form takes (conn, E, A); the same bits either way. */
int trs_bk_members(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E, const double *A,
                   const int32_t *free_index, const int32_t *n_free, const int32_t *nJ, const int32_t *nM,
                   const double *uf, int ld_uf, const double *theta, double *N, int32_t *ends, double *Mt, double *W,
                   void *stream);
int trs_bk_members_tab(int B, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16, const uint8_t *type_idx,
                       const double *types, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                       const int32_t *nM, const double *uf, int ld_uf, const double *theta, double *N, int32_t *ends,
                       double *Mt, double *W, void *stream);

/* G = H Y for the 16 vectors of every truss; one 256-thread work-group per truss.  Owner-computes by joint over the
 * member-end lists (trs_rec::build_end_lists, re-sorted by (far joint, member id) as the nonlinear kernels do): the
 * thread of (joint j, vector k) sums -g_m [D - n (n . D)], D = y_j - y_far, over the joint's ends in list order.
 * Rows of the padding are zero; a held DOF has no row and enters as y = 0.  ends, Mt as trs_bk_members wrote them. */
int trs_bk_product(int B, int nJ_max, int nM_max, const int32_t *ends, const double *Mt, const int32_t *free_index,
                   const int32_t *n_free, const int32_t *nJ, const int32_t *nM, const double *Y /* [B][16][ld_f] */,
                   double *G /* out [B][16][ld_f] */, int ld_f, void *stream);

/* One step of every truss with state[b] == 0 (see above); one wave per truss, the Gram products and the three rotations
 * on v_mfma_f64_16x16x4_f64.  first != 0: there is no Y yet - a truss with state[b] == 0 gets the start block in F and
 * Fk, lam and resid NaN and rank 0; any other truss gets its F rows zeroed and nothing else; G, X, check and iter are
 * ignored.  Otherwise F holds Y as trs_potrs_cases left it, G = H Y, Fk the right-hand sides Y was solved from;
 * iter >= 1 is the number of this step, 1 <= p <= 16 the number of pairs whose residuals decide (check != 0) whether
 * the truss is frozen. */
int trs_bk_step(int B, int p, const int32_t *n_free, const double *theta /* [B] or NULL */,
                double *F /* inout [B][16][ld_f] */, const double *G, double *Fk /* inout */, double *X /* out */,
                int ld_f, double *lam /* [B][16] */, double *resid /* [B][16] */, int32_t *rank /* [B] */,
                int32_t *state /* [B] */, int first, int check, int iter, double tol, void *stream);

/* phi [B][p][nJ_max][3]: column k < min(p, rank[b]) of X at the free DOFs of every joint, written through joint_out (the
 * batch's joint order, or NULL) into the caller's numbering and scaled so that the component of largest magnitude (the
 * first one in the caller's DOF order on a tie) is +1; zero at held DOFs, on the padding joints and for
 * k >= min(p, rank[b]). */
int trs_bk_shapes(int B, int p, int nJ_max, const double *X, int ld_f, const int32_t *free_index, const int32_t *n_free,
                  const int32_t *nJ, const int32_t *rank, const int32_t *joint_out /* [B][nJ_max] or NULL */,
                  double *phi /* out [B][p][nJ_max][3] */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_BUCKLING_H */
