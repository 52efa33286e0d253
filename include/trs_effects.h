/*
 * trs_effects.h - load cases with support settlements, member pre-strain and self-weight, solved against the resident
 * Cholesky factor (csrc/effects.hip; the entry points live in libtrs_hip.so beside those of trs_solver.h, whose
 * conventions hold here word for word: every pointer is a DEVICE pointer owned by the caller, the library allocates
 * nothing, every call only enqueues work on `stream` (a hipStream_t passed as void*) and returns 0 or a hipError_t, there
 * is no process-wide state that a result depends on, no floating-point atomic is used and every sum runs in one fixed
 * order - the results are bit-reproducible from run to run, from stream to stream and between the two member forms, case
 * k does not depend on L or on the other cases, and the numbers of truss b do not depend on B or on the other trusses).
 *
 * All three effects are equivalent joint loads plus a correction in the recovery: they change the right-hand side, never
 * K_ff, so they ride on the "factor once, many cases" path of trs_solver.h "Load cases":
 *
 *   trs_effects_rhs       loads, eps0, ubar, accel -> reduced right-hand sides F   (in place of trs_gather_cases)
 *   trs_potrs_cases       K_ff x = f against the factored slab                     (trs_solver.h, unchanged)
 *   trs_effects_recover   F, eps0, ubar, accel -> u, f_ext, N, body                (in place of trs_recover_cases)
 *
 * Definitions.  Member m runs from joint j0 to joint j1, len its length, c = (x_j1 - x_j0) / len, k = E A / len, tension
 * positive.  A case may carry any subset of
 *   loads [B][L][nJ_max][3]   joint forces
 *   eps0  [B][L][nM_max]      member initial strain (alpha dT for a temperature change, dL / L for lack of fit)
 *   ubar  [B][L][nJ_max][3]   prescribed displacements, READ AT CONSTRAINED DOFS ONLY (entries at free DOFs are ignored)
 *   accel [B][L][3]           body-force vector g per unit weight: member m loads each of its end joints with
 *                             1/2 (a * len * density) g (the product formed in the order Member.weight forms it, as
 *                             trs_modes_mass does)
 * (a NULL pointer = that effect is absent; the joint arrays are in the CALLER's numbering through joint_in / joint_out,
 * the batch's joint order as trs_gather_cases / trs_recover_cases take it).  Then
 *   u        the solved value at free DOFs, ubar at constrained DOFs (zero without ubar)
 *   N_m      k c . (u_j1 - u_j0) - E A eps0_m
 *   body_j   sum over the member ends at j, in member-id order, of 1/2 (a * len * density) g - accumulated per axis by
 *            fused multiply-add
 *   rhs      of free DOF (j, a):  loads + body + sum over the ends at j (+ at j1, - at j0) of
 *            (E A eps0_m - k c . (ubar_j1 - ubar_j0)) c_a         (the second term is -K_fc ubar_c)
 *   f_ext    at a free DOF the case's `loads` entry as given (zero without loads); at a constrained DOF what the support
 *            and any load there supply, sum over the ends (+ at j1, - at j0) of N_m c_a  -  body_(j, a).
 * f_ext never contains the self-weight: over all DOFs of a truss f_ext + body sums to zero, component by component.
 *
 * With eps0, ubar and accel all NULL every output equals trs_gather_cases -> trs_potrs_cases -> trs_recover_cases bit for
 * bit: N and the constrained-DOF sums are formed by the same functions (csrc/trs_recover.h) in the same order, and an
 * effect's term is added only where its pointer is non-NULL.  A truss whose factorisation failed (info[b] != 0) gets
 * meaningless numbers; the others are unaffected.
 *
 * Both kernels are one work-group per truss: the member-end lists of every joint are built once in LDS (integer atomics,
 * then sorted by member id), then a loop over the cases with one DOF vector (ubar, or u) and one double per member (the
 * member term, or N) in LDS.
 */
#ifndef TRS_EFFECTS_H
#define TRS_EFFECTS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_EFFECTS_ABI_VERSION 1

int trs_effects_abi_version(void);

/* Whether the tables of a truss of this shape fit a CU's LDS: (3 nJ_max + nM_max) doubles and (2 nJ_max + 1 + 2 nM_max)
 * ints within 160 KB (otherwise the entry points below return hipErrorInvalidValue). */
int trs_effects_fits(int nJ_max, int nM_max);

/* The reduced right-hand sides F [B][L][ld_f] in the layout trs_potrs_cases reads (entries c < n_free[b] in the order of
 * free_index, the padding n_free[b] <= c < n_pad zeroed).  xyz, the members, free_index, n_free, nJ, nM: the batch's
 * arrays as assembled; rho is read only when accel is given (general form: rho == NULL with accel != NULL is refused).
 * The table-form twin carries the form in the middle of its name, as trs_recover_tab_cases does, and takes
 * (conn16, type_idx, types) where the general form takes (conn, E, A, rho); the same bits either way. */
int trs_effects_rhs(int B, int L, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                    const double *A, const double *rho, const double *loads /* [B][L][nJ_max][3] or NULL */,
                    const double *eps0 /* [B][L][nM_max] or NULL */, const double *ubar /* [B][L][nJ_max][3] or NULL */,
                    const double *accel /* [B][L][3] or NULL */, const int32_t *free_index, const int32_t *n_free,
                    const int32_t *nJ, const int32_t *nM, const int32_t *joint_in /* [B][nJ_max] or NULL */,
                    double *F /* out [B][L][ld_f] */, int ld_f, void *stream);
int trs_effects_tab_rhs(int B, int L, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                        const uint8_t *type_idx, const double *types, const double *loads, const double *eps0,
                        const double *ubar, const double *accel, const int32_t *free_index, const int32_t *n_free,
                        const int32_t *nJ, const int32_t *nM, const int32_t *joint_in, double *F, int ld_f, void *stream);

/* u, f_ext [B][L][nJ_max][3] and N [B][L][nM_max] of every case from F as trs_potrs_cases left it, written through
 * joint_out as trs_recover_cases writes them (padding joints and members zero); body [B][L][nJ_max][3] (or NULL): the
 * self-weight load of every joint, zero without accel.  The effect pointers must be the ones trs_effects_rhs saw. */
int trs_effects_recover(int B, int L, int nJ_max, int nM_max, const double *xyz, const int32_t *conn, const double *E,
                        const double *A, const double *rho, const double *loads, const double *eps0, const double *ubar,
                        const double *accel, const int32_t *free_index, const int32_t *nJ, const int32_t *nM,
                        const double *F, int ld_f, double *u, double *f_ext, double *N,
                        double *body /* out [B][L][nJ_max][3] or NULL */, const int32_t *joint_out, void *stream);
int trs_effects_tab_recover(int B, int L, int nJ_max, int nM_max, const double *xyz, const uint16_t *conn16,
                            const uint8_t *type_idx, const double *types, const double *loads, const double *eps0,
                            const double *ubar, const double *accel, const int32_t *free_index, const int32_t *nJ,
                            const int32_t *nM, const double *F, int ld_f, double *u, double *f_ext, double *N,
                            double *body, const int32_t *joint_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_EFFECTS_H */
