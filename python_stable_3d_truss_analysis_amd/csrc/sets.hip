// Member-set scenarios (include/trs_sets.h): what removing, damaging or strengthening up to eight members AT ONCE does
// to a truss, from the factor in the slab - the change K_ff + sum_j theta_j k_j b_j b_j^T has rank k, so one substitution
// column per DISTINCT member of a range of scenarios (trs_potrs_cases, cases.hip, as it is) and one k x k elimination
// per scenario replace one factorisation per scenario.
//
//   trs_sets_rhs      Z [B][C][ld_f]: row i = b_e,f of e = cols[b][i] (the rhs kernel of loss.hip)
//   trs_potrs_cases   z_e = inv(K_ff) b_e,f
//   trs_sets_apply    P_ij = c_i . D z_j,  A = I + diag(k) P diag(theta) = L U in the set's order,  a = theta inv(A) n,
//                     u' = u - sum_j a_j z_j,  N'_m = gamma_m k_m c_m . D u', and the maxima of |k_m c_m . D u'| / A_m over
//                     the members with gamma != 0 and of |u'_j| over the joints
//
// The apply kernel is one work-group of four waves per (truss, slice of the range's scenarios) on the staged tables of
// trs_columns.h.  Every wave takes one scenario at a time.  Lane 8 i + j gathers P_ij from Z through free_index - the
// expression that forms r_e in trs_loss_apply, so a single removal's pivot has r_e's bits - and holds A_ij during the
// elimination, which runs in lockstep with wave shuffles; L and U go to 64 doubles of LDS of the wave's own.  Lane
// 8 l + i then substitutes case l of the pass (forward, backward, ascending) and leaves a_i = theta_i x_i in 64 more.
// Per case the wave forms u' = u - sum_j a_j z_j in its ONE joint-layout LDS vector (ascending j, one fma per term, the
// k rows of Z streamed through free_index) and runs its lanes over the members and the joints.  Max is exact and every
// other number is one fixed expression of staged values: the result of (s, l) does not depend on the range, the slice,
// the pass, L, B, the place of the columns in Z or the member form.
#include "../../include/trs_sets.h"
#include "trs_common.h"
#include "trs_columns.h"
#include "trs_recover.h"

#include <math.h>

namespace {

using namespace trs_rec;
using namespace trs_col;

constexpr int WAVES = 4;          // waves per work-group; trs_sets_fits' rule counts their u' vectors
constexpr int KMAX = TRS_SETS_MAX;
constexpr int OWN = 128;          // doubles of a wave's own: L and U of its scenario, then a_i of case l at 8 l + i
#ifndef TRS_SETS_SLICE
#define TRS_SETS_SLICE 32         // scenarios per work-group
#endif
static_assert(KMAX * KMAX == 64 && MAX_PASS * KMAX == 64, "one lane per entry of the k x k system / per (case, member)");

// ---- the apply kernel ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WAVES) void trs_sets_apply_kernel(
    const TrsBatch bt, const int L, const int g, const int S, const int s0, const int Sc, const int C, const int slice,
    const int* __restrict__ cols, const int* __restrict__ slot, const double* __restrict__ gamma,
    const double* __restrict__ Z, const double* __restrict__ U, const double r_tol, double* __restrict__ piv_out,
    int* __restrict__ unst_out, int* __restrict__ first_out, double* __restrict__ ps_out, int* __restrict__ pm_out,
    double* __restrict__ pd_out, int* __restrict__ pj_out, double* __restrict__ NA, double* __restrict__ UA) {
    extern __shared__ double sh[];
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f;
    const int slices = (Sc + slice - 1) / slice;   // work-groups per truss
    const int b = blockIdx.x / slices, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the scenarios of this work-group, counted within the range: first <= sl < last
    const int first = (blockIdx.x - b * slices) * slice;
    const int last = min(first + slice, Sc);
    if (first >= last) return;
    const TrussView v = bt.truss(b);
    const int joints = v.joints, members = v.members, ndof = v.ndof, ndof_max = v.ndof_max;
    trs_lds::Carve carve(sh);
    const Tables t = layout(carve, nJ_max, nM_max, g, WAVES, OWN);
    double* zw = t.z + (size_t)wave * ndof_max;
    double* luw = t.own + OWN * wave;
    double* aw = luw + 64;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");
    const int hi = lane >> 3, lo = lane & 7;   // lane = 8 hi + lo

    stage(t, tid, 64 * WAVES, v);
    for (int l0 = 0; l0 < L; l0 += g) {
        const int lg = min(g, L - l0);   // the cases of this pass: l0 .. l0 + lg - 1
        stage_pass(t, tid, 64 * WAVES, lg, members, nJ_max, nM_max, U + ((size_t)b * L + l0) * ld_f, ld_f);

        for (int sl = first + wave; sl < last; sl += WAVES) {
            const size_t sb = (size_t)b * S + s0 + sl;            // (b, s) of the per-scenario outputs
            const size_t out0 = ((size_t)b * L + l0) * S + s0 + sl;   // (b, l0, s); the next case lies S further
            // the set: lane j < 8 holds its j-th member, column and factor; it ends at the first entry that names none
            const size_t in0 = ((size_t)b * Sc + sl) * KMAX;
            int my_col = -1, my_e = -1;
            double my_gamma = 0.0;
            if (lane < KMAX) {
                my_col = slot[in0 + lane];
                if (my_col >= 0 && my_col < C) {
                    const int e = cols[(size_t)b * C + my_col];
                    if (e >= 0 && e < members) my_e = e;
                }
                if (gamma != nullptr) my_gamma = gamma[in0 + lane];
            }
            const unsigned ends_at = (unsigned)(__ballot(lane < KMAX && my_e < 0) & 0xffu);
            const int k = ends_at != 0 ? __builtin_ctz(ends_at) : KMAX;
            int e_of[KMAX], col_of[KMAX];
            double gam[KMAX];
#pragma unroll
            for (int j = 0; j < KMAX; ++j) {
                e_of[j] = __builtin_amdgcn_readfirstlane(__shfl(my_e, j));
                col_of[j] = __builtin_amdgcn_readfirstlane(__shfl(my_col, j));
                gam[j] = __shfl(my_gamma, j);
            }
            // A_ij = delta_ij + theta_j k_i c_i . (z_j at i's j1 - z_j at i's j0) in lane 8 i + j
            const int e_hi = __shfl(my_e, hi), e_lo = __shfl(my_e, lo), cj = __shfl(my_col, lo);
            const double theta = __shfl(my_gamma, lo) - 1.0;   // of member lo: column lo of A, and a_lo below
            double Aij = hi == lo ? 1.0 : 0.0;
            if (hi < k && lo < k) {
                const int ei = e_hi;
                const double* zj = Z + ((size_t)b * C + cj) * ld_f;
                const int2 ce = t.ends[ei];
                double v[6];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int r1 = t.fi[3 * ce.y + a], r0 = t.fi[3 * ce.x + a];
                    v[a] = r1 >= 0 ? zj[r1] : 0.0;
                    v[3 + a] = r0 >= 0 ? zj[r0] : 0.0;
                }
                Aij = fma(theta * t.k[ei], along(t, ei, v[0] - v[3], v[1] - v[4], v[2] - v[5]), Aij);
            }
            // Gauss without pivoting, in the set's order
            int fail = -1;
            double my_pivot = nan;   // lane j < 8: p_j
#pragma unroll
            for (int p = 0; p < KMAX; ++p) {
                if (p >= k || fail >= 0) break;
                const double piv = __shfl(Aij, 9 * p);
                if (lane == p) my_pivot = piv;
                if (!(piv > r_tol)) {
                    fail = p;
                    break;
                }
                const double aip = __shfl(Aij, 8 * hi + p), apj = __shfl(Aij, 8 * p + lo);
                if (hi > p) {
                    const double f = aip / piv;
                    if (lo == p) Aij = f;
                    else if (lo > p) Aij = fma(-f, apj, Aij);
                }
            }
            if (l0 == 0) {
                if (lane < KMAX) piv_out[sb * KMAX + lane] = my_pivot;
                if (lane == 0) {
                    unst_out[sb] = fail >= 0 ? 1 : 0;
                    first_out[sb] = fail;
                }
            }
            if (fail >= 0) {
                if (lane < lg) {
                    const size_t o = out0 + (size_t)lane * S;
                    ps_out[o] = inf;
                    pd_out[o] = inf;
                    pm_out[o] = -1;
                    pj_out[o] = -1;
                }
                for (int l = 0; l < lg; ++l) {
                    const size_t o = out0 + (size_t)l * S;
                    if (NA != nullptr)
                        for (int m = lane; m < nM_max; m += 64) NA[o * nM_max + m] = m < members ? nan : 0.0;
                    if (UA != nullptr)
                        for (int j = lane; j < nJ_max; j += 64) {
                            double* dst = UA + (o * nJ_max + t.jo[j]) * 3;
                            dst[0] = dst[1] = dst[2] = j < joints ? nan : 0.0;
                        }
                }
                continue;
            }
            // a = theta inv(A) n of the cases of the pass: lane 8 l + i
            luw[lane] = Aij;
            __builtin_amdgcn_wave_barrier();
            {
                const bool mine = hi < lg && lo < k;
                double y = 0.0;
                if (mine) y = t.N[(size_t)hi * nM_max + e_lo];
#pragma unroll
                for (int j = 0; j < KMAX; ++j) {   // L y = n (unit diagonal)
                    if (j >= k) break;
                    const double yj = __shfl(y, 8 * hi + j);
                    if (mine && lo > j) y = fma(-luw[8 * lo + j], yj, y);
                }
#pragma unroll
                for (int j = KMAX - 1; j >= 0; --j) {   // U x = y
                    if (j >= k) continue;
                    if (mine && lo == j) y = y / luw[9 * j];
                    const double xj = __shfl(y, 8 * hi + j);
                    if (mine && lo < j) y = fma(-luw[8 * lo + j], xj, y);
                }
                aw[lane] = mine ? theta * y : 0.0;
            }
            __builtin_amdgcn_wave_barrier();

            for (int l = 0; l < lg; ++l) {
                const size_t o = out0 + (size_t)l * S;
                // u' = u - sum_j a_j z_j in joint layout (this wave's own vector: written and read by this wave only)
                {
                    const double* ul = t.u + (size_t)l * ndof_max;
                    double al[KMAX];
#pragma unroll
                    for (int j = 0; j < KMAX; ++j) al[j] = aw[8 * l + j];
                    for (int d = lane; d < ndof; d += 64) {
                        double v = ul[d];
                        const int row = t.fi[d];
                        if (row >= 0) {
#pragma unroll
                            for (int j = 0; j < KMAX; ++j) {
                                if (j >= k) break;
                                v = fma(-al[j], Z[((size_t)b * C + col_of[j]) * ld_f + row], v);
                            }
                        }
                        zw[d] = v;
                    }
                }
                __builtin_amdgcn_wave_barrier();
                // the members
                double best = -1.0;
                int where = INT_MAX;
                for (int m0 = 0; m0 < nM_max; m0 += 64) {
                    const int m = m0 + lane;
                    const bool real = m < members;
                    double after = 0.0;
                    if (real) {
                        const double n = t.k[m] * along(t, m, zw);
                        double gm = 1.0;
                        bool changed = false;
#pragma unroll
                        for (int j = 0; j < KMAX; ++j)
                            if (j < k && m == e_of[j]) {
                                gm = gam[j];
                                changed = true;
                            }
                        after = !changed ? n : gm == 0.0 ? 0.0 : gm * n;
                        const double s = fabs(n) * t.ia[m];
                        if (gm != 0.0 && s > best) {   // (ascending m per lane: the first of equals stays)
                            best = s;
                            where = m;
                        }
                    }
                    if (NA != nullptr && m < nM_max) NA[o * nM_max + m] = after;
                }
                close_peak(best, where, lane, ps_out + o, pm_out + o);
                // the joints
                best = -1.0;
                where = INT_MAX;
                for (int j = lane; j < nJ_max; j += 64) {
                    const int id = t.jo[j];
                    const double a0 = zw[3 * j], a1 = zw[3 * j + 1], a2 = zw[3 * j + 2];   // (zero past the truss's joints)
                    if (j < joints) {
                        const double d = sqrt(fma(a2, a2, fma(a1, a1, a0 * a0)));
                        if (d > best || (d == best && id < where)) {
                            best = d;
                            where = id;
                        }
                    }
                    if (UA != nullptr) {
                        double* dst = UA + (o * nJ_max + id) * 3;
                        dst[0] = a0;
                        dst[1] = a1;
                        dst[2] = a2;
                    }
                }
                close_peak(best, where, lane, pd_out + o, pj_out + o);
                __builtin_amdgcn_wave_barrier();   // (the next case's u' overwrites zw)
            }
        }
    }
}

int sets_rhs_launch(int B, const TrsBatch& bt, int C, const int* cols, double* Z, hipStream_t stream) {
    if (B > 0 && C > 0 && (!bt.mem.conn || !bt.xyz || !bt.free_index || !bt.n_free || !bt.nM || !cols || !Z))
        return (int)hipErrorInvalidValue;   // (without `cols` the kernel would take the members 0 .. C - 1)
    return rhs_launch(B, bt, 0, cols, C, Z, stream);
}

int sets_apply_launch(int B, const TrsBatch& bt, int L, int S, int s0, int Sc, int C, const int* cols, const int* slot,
                      const double* gamma, const double* Z, const double* U, double r_tol, double* pivot, int* unstable,
                      int* first_unstable, double* peak_stress, int* peak_member, double* peak_displace, int* peak_joint,
                      double* N_after, double* u_after, hipStream_t stream) {
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max;
    const TrsMembers& mem = bt.mem;
    if (B < 0 || L < 0 || S < 0 || s0 < 0 || Sc < 0 || C < 0 || nJ_max < 0 || nM_max < 0 || bt.ld_f < 0)
        return (int)hipErrorInvalidValue;
    if ((long long)s0 + Sc > S) return (int)hipErrorInvalidValue;   // (the outputs hold S scenarios)
    if (B == 0 || L == 0 || Sc == 0) return 0;
    if (nJ_max == 0 && nM_max > 0) return (int)hipErrorInvalidValue;   // (members without joints to end at)
    if (!trs_sets_fits(nJ_max, nM_max, L)) return (int)hipErrorInvalidValue;
    if (!mem.conn || (mem.tidx == nullptr && (!mem.E || !mem.A)) || !bt.xyz || !bt.free_index || !bt.nJ || !bt.nM ||
        !slot || !U || !pivot || !unstable || !first_unstable || !peak_stress || !peak_member || !peak_displace ||
        !peak_joint || (C > 0 && (!cols || !Z)))
        return (int)hipErrorInvalidValue;
    const int g = pass(nJ_max, nM_max, L, WAVES, OWN);
    if (g <= 0) return (int)hipErrorInvalidValue;   // (the kernel's pass loop steps by g)
    trs_lds::raise_lds_once<trs_sets_apply_kernel>();
    const int slices = (Sc + TRS_SETS_SLICE - 1) / TRS_SETS_SLICE;
    hipLaunchKernelGGL(trs_sets_apply_kernel, dim3((unsigned)slices * (unsigned)B), dim3(64 * WAVES),
                       lds(nJ_max, nM_max, g, WAVES, OWN), stream, bt, L, g, S, s0, Sc, C, TRS_SETS_SLICE, cols, slot, gamma,
                       Z, U, r_tol, pivot, unstable, first_unstable, peak_stress, peak_member, peak_displace, peak_joint,
                       N_after, u_after);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_sets_abi_version(void) { return TRS_SETS_ABI_VERSION; }

int trs_sets_fits(int nJ_max, int nM_max, int L) {
    return fits(nJ_max, nM_max, L, WAVES, OWN);
}

int trs_sets_rhs(int B, int C, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                 const double* A, const int32_t* free_index, const int32_t* n_free, const int32_t* nM,
                 const int32_t* cols, double* Z, int ld_f, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nullptr, nM,
                                  nullptr, ld_f);
    return sets_rhs_launch(B, bt, C, cols, Z, (hipStream_t)stream);
}

int trs_sets_tab_rhs(int B, int C, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                     const uint8_t* type_idx, const double* types, const int32_t* free_index, const int32_t* n_free,
                     const int32_t* nM, const int32_t* cols, double* Z, int ld_f, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free,
                                  nullptr, nM, nullptr, ld_f);
    return sets_rhs_launch(B, bt, C, cols, Z, (hipStream_t)stream);
}

int trs_sets_apply(int B, int L, int S, int s0, int Sc, int C, int nJ_max, int nM_max, const double* xyz,
                   const int32_t* conn, const double* E, const double* A, const int32_t* free_index, const int32_t* nJ,
                   const int32_t* nM, const int32_t* cols, const int32_t* slot, const double* gamma, const double* Z,
                   const double* U, int ld_f, double r_tol, double* pivot, int32_t* unstable, int32_t* first_unstable,
                   double* peak_stress, int32_t* peak_member, double* peak_displace, int32_t* peak_joint,
                   double* N_after, double* u_after, const int32_t* joint_out, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, nullptr, nJ, nM,
                                  joint_out, ld_f);
    return sets_apply_launch(B, bt, L, S, s0, Sc, C, cols, slot, gamma, Z, U, r_tol, pivot, unstable, first_unstable,
                             peak_stress, peak_member, peak_displace, peak_joint, N_after, u_after, (hipStream_t)stream);
}

int trs_sets_tab_apply(int B, int L, int S, int s0, int Sc, int C, int nJ_max, int nM_max, const double* xyz,
                       const uint16_t* conn16, const uint8_t* type_idx, const double* types, const int32_t* free_index,
                       const int32_t* nJ, const int32_t* nM, const int32_t* cols, const int32_t* slot,
                       const double* gamma, const double* Z, const double* U, int ld_f, double r_tol, double* pivot,
                       int32_t* unstable, int32_t* first_unstable, double* peak_stress, int32_t* peak_member,
                       double* peak_displace, int32_t* peak_joint, double* N_after, double* u_after,
                       const int32_t* joint_out, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, nullptr, nJ,
                                  nM, joint_out, ld_f);
    return sets_apply_launch(B, bt, L, S, s0, Sc, C, cols, slot, gamma, Z, U, r_tol, pivot, unstable, first_unstable,
                             peak_stress, peak_member, peak_displace, peak_joint, N_after, u_after, (hipStream_t)stream);
}

}  // extern "C"
