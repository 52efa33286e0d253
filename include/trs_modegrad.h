/*
 * trs_modegrad.h - gradients of the natural frequencies from the converged mode block (csrc/modegrad.hip; the entry
 * points live in libtrs_hip.so beside those of trs_solver.h and trs_modes.h, whose conventions hold here word for
 * word: every pointer is a DEVICE pointer owned by the caller, the library allocates nothing, every call only enqueues
 * work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there is no process-wide state that a
 * result depends on, no floating-point atomic is used and every sum runs in one fixed order - the results are
 * bit-reproducible from run to run, from stream to stream and between the two member forms, and the numbers of truss b
 * do not depend on B or on the other trusses of the batch).
 *
 * The problem.  K_ff phi = lambda M phi with the lumped mass M of trs_modes.h, phi M-orthonormal (the block X that
 * trs_modes_step left, lam its Ritz values).  For a SIMPLE eigenvalue the derivative needs no solve:
 * d lambda = phi^T (dK - lambda dM) phi.  With member m from j0 to j1, D = x_j1 - x_j0, len = |D|, c = D / len,
 * k = E A / len, Dphi = phi_j1 - phi_j0 (phi = 0 at held DOFs), s = c . Dphi, h = |phi_j0|^2 + |phi_j1|^2,
 * mu = mass_scale, rho the member's density:
 *
 *     d lambda / dA_m   = (E / len) s^2  -  lambda mu 1/2 len rho h
 *     d lambda / dE_m   = (A / len) s^2
 *     d lambda / drho_m = -lambda mu 1/2 A len h
 *     d lambda / dm_j   = -lambda |phi_j|^2                         (m_j: the caller's joint_mass)
 *     g_m               = (k / len) s (2 Dphi - 3 s c)  -  lambda mu 1/2 A rho h c
 *     d lambda / dx_j   = sum over the member ends at j (member-id order) of  +g_m at end j1, -g_m at end j0
 *
 * d lambda / dx_j is formed at EVERY joint, held ones included (moving a support changes lambda); z is exactly 0 on a
 * 2D truss.  A member of a repeated eigenvalue has no derivative of its own - the formula is evaluated all the same;
 * the SUM over a closed cluster (equal weights) is invariant and differentiable.  The caller judges by the gaps of lam.
 *
 * Outputs (any may be NULL, and then it is not computed), R rows per truss:
 *     gA, gE, grho   [B][R][nM_max]       per member (also in the table member form)
 *     gxyz           [B][R][nJ_max][3]    caller's joint numbering, through joint_out
 *     gmass          [B][R][nJ_max]       caller's joint numbering, through joint_out
 * w == NULL: R = p, row k is the gradient of lambda_k (Jacobian form).  w [B][p] given: R = 1, the row is
 * sum_k w_k d lambda_k, accumulated as acc = fma(w_k, g_k, acc) from zero for k ascending (vector-Jacobian form): a
 * call with w = e_k gives Jacobian row k.
 * Zeros are written for: the rows k >= n_modes = min(p, n_mass[b]) of the Jacobian form (in the weighted form w_k of
 * such a k is not read into any result, whatever it holds - the NaN Ritz values never reach an output); padding
 * members and padding joints; members of zero length.
 * nJ[b], nM[b] and end-joint ids are trimmed and clamped to the arrays: whatever the inputs hold, nothing is read or
 * written outside them.  A truss whose factorisation failed gets meaningless numbers; the others are unaffected.
 *
 * Kernel: one work-group of 256 threads per truss.  c, len, k / len and the mass factor of every member go to LDS ONCE;
 * phi_k goes to LDS in joint layout through free_index, as many modes per pass as fit (three per pass on bar-942, so
 * that two work-groups share a CU); one thread per member forms the member outputs, one thread per joint walks its
 * member-end list in member-id order for gxyz and forms gmass.
 */
#ifndef TRS_MODEGRAD_H
#define TRS_MODEGRAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_MG_ABI_VERSION 1
#define TRS_MG_BLOCK 16 /* vectors per truss in X and lam: TRS_MODES_BLOCK of trs_modes.h */
#define TRS_MG_MAX_MODES 8 /* p at most: what one block delivers */

int trs_mg_abi_version(void);

/* Whether a batch shape fits the kernel's LDS (160 KB per CU) with at least one mode per pass, and 1 <= p <= 8:
 * 64 nM_max + 8 nJ_max + 4 bytes of tables and lists plus 24 nJ_max per staged mode.  Otherwise trs_mg_grad /
 * trs_mg_tab_grad return hipErrorInvalidValue. */
int trs_mg_fits(int nJ_max, int nM_max, int p);

/* xyz, the members, free_index, n_free, nJ, nM: the batch's arrays as assembled (in the batch's joint order);
 * joint_out [B][nJ_max] (where the results of joint j go: the caller's id) or NULL; X [B][16][ld_f] and lam [B][16] as
 * trs_modes_step left them; n_mass [B] of trs_modes_mass; 1 <= p <= 8; mass_scale as given to trs_modes_mass;
 * w [B][p] or NULL.  The `_tab` twin takes (conn16, type_idx, types) where the general form takes (conn, E, A, rho);
 * the same bits either way. */
int trs_mg_grad(int B, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E, const double *A,
                const double *rho, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                const int32_t *nM, const int32_t *joint_out /* [B][nJ_max] or NULL */,
                const double *X /* [B][16][ld_f] */, int ld_f, const double *lam /* [B][16] */,
                const int32_t *n_mass /* [B] */, int p, double mass_scale, const double *w /* [B][p] or NULL */,
                double *gA, double *gE, double *grho /* [B][R][nM_max] or NULL */,
                double *gxyz /* [B][R][nJ_max][3] or NULL */, double *gmass /* [B][R][nJ_max] or NULL */, void *stream);
int trs_mg_tab_grad(int B, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16, const uint8_t *type_idx,
                    const double *types, const int32_t *free_index, const int32_t *n_free, const int32_t *nJ,
                    const int32_t *nM, const int32_t *joint_out, const double *X, int ld_f, const double *lam,
                    const int32_t *n_mass, int p, double mass_scale, const double *w, double *gA, double *gE,
                    double *grho, double *gxyz, double *gmass, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_MODEGRAD_H */
