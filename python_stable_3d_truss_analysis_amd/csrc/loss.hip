// Member-loss analysis (include/trs_loss.h): what every single-member removal does to a truss, from the factor in the
// slab - a removal is the rank-one change K_ff - k_e b_e b_e^T, so one substitution column per member (trs_potrs_cases,
// cases.hip, as it is) and one gather kernel replace one factorisation per member.
//
//   trs_loss_rhs      Z [B][C][ld_f]: row i = b_{e0 + i},f (six non-zeros at most; the kernel serves trs_sets_rhs too)
//   trs_potrs_cases   z_e = inv(K_ff) b_e,f
//   trs_loss_apply    q_m = k_m c_m . D z_e,  r_e = 1 - q_e,  alpha = N_e / r_e,  u' = u + alpha z_e,  N'_m = N_m + alpha q_m
//                     and the maxima of |N'_m| / A_m over m != e and of |u'_j| over the joints
//
// The apply kernel is one work-group per (truss, slice of the chunk) on the staged tables of trs_columns.h.  Every wave
// takes one removed member at a time: z_e goes into the wave's joint-layout vector (zeros at held DOFs), the lanes run
// over the members and over the joints with the per-case maxima in registers, and a wave reduction that carries the
// index with the value closes each (e, l).  Max is exact and every other number is one fixed expression of staged
// values: the result of (e, l) does not depend on the chunk, the slice, the pass, L, B or the member form.
#include "../../include/trs_loss.h"
#include "trs_common.h"
#include "trs_columns.h"
#include "trs_recover.h"

#include <math.h>

namespace {

using namespace trs_rec;
using namespace trs_col;

constexpr int WAVES = TRS_LOSS_WAVES;   // each owns one z vector in LDS; trs_loss_fits' rule counts them
#ifndef TRS_LOSS_SLICE
#define TRS_LOSS_SLICE 32         // removed members per work-group (EXPERIMENTS R14)
#endif

// ---- the right-hand sides: one wave per row --------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WAVES) void trs_columns_rhs_kernel(const TrsBatch bt, const int e0,
                                                                     const int* __restrict__ cols, const int C,
                                                                     double* __restrict__ Z) {
    const int per_truss = (C + WAVES - 1) / WAVES;   // work-groups per truss
    const int b = blockIdx.x / per_truss, lane = threadIdx.x & 63;
    const int i = (blockIdx.x - b * per_truss) * WAVES + (threadIdx.x >> 6);
    if (i >= C) return;
    const TrussView v = bt.truss(b);
    const int e = cols != nullptr ? cols[(size_t)b * C + i] : e0 + i;
    const bool real = e >= 0 && e < v.members;
    const int npad = min(trs_round_up(v.nfree, TRS_NB), bt.ld_f);
    write_row(Z + ((size_t)b * C + i) * bt.ld_f, npad, lane, real, real ? e : 0, v);
}

// ---- the apply kernel ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WAVES) void trs_loss_apply_kernel(
    const TrsBatch bt, const int L, const int g, const int e0, const int C, const int slice, const double* __restrict__ Z,
    const double* __restrict__ U, const double r_tol, double* __restrict__ r_out, int* __restrict__ crit_out,
    double* __restrict__ ps_out, int* __restrict__ pm_out, double* __restrict__ pd_out, int* __restrict__ pj_out,
    double* __restrict__ NA) {
    extern __shared__ double sh[];
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f;
    const int slices = (C + slice - 1) / slice;   // work-groups per truss
    const int b = blockIdx.x / slices, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the removed members of this work-group: first <= e < last (inside the chunk and inside the arrays)
    const int first = e0 + (blockIdx.x - b * slices) * slice;
    const int last = min(min(first + slice, e0 + C), nM_max);
    if (first >= last) return;
    const TrussView v = bt.truss(b);
    const int joints = v.joints, members = v.members, ndof = v.ndof, ndof_max = v.ndof_max;
    trs_lds::Carve carve(sh);
    const Tables t = layout(carve, nJ_max, nM_max, g, WAVES, 0);
    const size_t mbase = v.mbase;
    double* zw = t.z + (size_t)wave * ndof_max;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");

    stage(t, tid, 64 * WAVES, v);
    for (int l0 = 0; l0 < L; l0 += g) {
        const int lg = min(g, L - l0);   // the cases of this pass: l0 .. l0 + lg - 1
        stage_pass(t, tid, 64 * WAVES, lg, members, nJ_max, nM_max, U + ((size_t)b * L + l0) * ld_f, ld_f);

        for (int e = first + wave; e < last; e += WAVES) {
            // where the results of (b, l0 + l, e) go
            const size_t out0 = ((size_t)b * L + l0) * nM_max + e;
            if (e >= members) {   // a padding member
                if (l0 == 0 && lane == 0) {
                    r_out[mbase + e] = 0.0;
                    crit_out[mbase + e] = 0;
                }
                if (lane < lg) {
                    const size_t o = out0 + (size_t)lane * nM_max;
                    ps_out[o] = 0.0;
                    pd_out[o] = 0.0;
                    pm_out[o] = -1;
                    pj_out[o] = -1;
                }
                if (NA != nullptr)
                    for (int l = 0; l < lg; ++l)
                        for (int m = lane; m < nM_max; m += 64) NA[(out0 + (size_t)l * nM_max) * nM_max + m] = 0.0;
                continue;
            }
            // z_e in joint layout, zeros at the held DOFs (this wave's own vector: written and read by this wave only)
            const double* ze = Z + ((size_t)b * C + (e - e0)) * ld_f;
            for (int d = lane; d < ndof; d += 64) {
                const int row = t.fi[d];
                zw[d] = row >= 0 ? ze[row] : 0.0;
            }
            __builtin_amdgcn_wave_barrier();
            // r_e = 1 - k_e c_e . (z_j1 - z_j0): the same expression as q_m below, by every lane (broadcast reads)
            const double re = 1.0 - t.k[e] * along(t, e, zw);
            const bool critical = re <= r_tol;
            if (l0 == 0 && lane == 0) {
                r_out[mbase + e] = re;
                crit_out[mbase + e] = critical ? 1 : 0;
            }
            if (critical) {
                if (lane < lg) {
                    const size_t o = out0 + (size_t)lane * nM_max;
                    ps_out[o] = inf;
                    pd_out[o] = inf;
                    pm_out[o] = -1;
                    pj_out[o] = -1;
                }
                if (NA != nullptr)
                    for (int l = 0; l < lg; ++l)
                        for (int m = lane; m < nM_max; m += 64)
                            NA[(out0 + (size_t)l * nM_max) * nM_max + m] = m < members ? nan : 0.0;
                continue;
            }
            double alpha[MAX_PASS], best[MAX_PASS];
            int where[MAX_PASS];
#pragma unroll
            for (int l = 0; l < MAX_PASS; ++l) {
                alpha[l] = l < lg ? t.N[(size_t)l * nM_max + e] / re : 0.0;
                best[l] = -1.0;
                where[l] = INT_MAX;
            }
            // the surviving members
            for (int m0 = 0; m0 < nM_max; m0 += 64) {
                const int m = m0 + lane;
                const bool real = m < members, counts = real && m != e;
                double q = 0.0, ia = 0.0;
                if (counts) {
                    q = t.k[m] * along(t, m, zw);
                    ia = t.ia[m];
                }
#pragma unroll
                for (int l = 0; l < MAX_PASS; ++l) {
                    if (l >= lg) break;
                    const double after = counts ? fma(alpha[l], q, t.N[(size_t)l * nM_max + m]) : 0.0;
                    const double s = fabs(after) * ia;
                    if (counts && s > best[l]) {   // (ascending m per lane: the first of equals stays)
                        best[l] = s;
                        where[l] = m;
                    }
                    if (NA != nullptr && m < nM_max) NA[(out0 + (size_t)l * nM_max) * nM_max + m] = after;
                }
            }
#pragma unroll
            for (int l = 0; l < MAX_PASS; ++l) {
                if (l >= lg) break;
                const size_t o = out0 + (size_t)l * nM_max;
                close_peak(best[l], where[l], lane, ps_out + o, pm_out + o);
                best[l] = -1.0;
                where[l] = INT_MAX;
            }
            // the joints
            for (int j = lane; j < joints; j += 64) {
                const double z0 = zw[3 * j], z1 = zw[3 * j + 1], z2 = zw[3 * j + 2];
                const int id = t.jo[j];
#pragma unroll
                for (int l = 0; l < MAX_PASS; ++l) {
                    if (l >= lg) break;
                    const double* ul = t.u + (size_t)l * ndof_max + 3 * j;
                    const double a0 = fma(alpha[l], z0, ul[0]), a1 = fma(alpha[l], z1, ul[1]),
                                 a2 = fma(alpha[l], z2, ul[2]);
                    const double d = sqrt(fma(a2, a2, fma(a1, a1, a0 * a0)));
                    if (d > best[l] || (d == best[l] && id < where[l])) {
                        best[l] = d;
                        where[l] = id;
                    }
                }
            }
#pragma unroll
            for (int l = 0; l < MAX_PASS; ++l) {
                if (l >= lg) break;
                const size_t o = out0 + (size_t)l * nM_max;
                close_peak(best[l], where[l], lane, pd_out + o, pj_out + o);
            }
            __builtin_amdgcn_wave_barrier();   // (the next member's z overwrites zw)
        }
    }
}

int loss_apply_launch(int B, const TrsBatch& bt, int L, int e0, int C, const double* Z, const double* U, double r_tol,
                      double* r, int* critical, double* peak_stress, int* peak_member, double* peak_displace,
                      int* peak_joint, double* N_after, hipStream_t stream) {
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max;
    if (B < 0 || L < 0 || e0 < 0 || C < 0 || nJ_max < 0 || nM_max < 0 || bt.ld_f < 0) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0 || C == 0 || e0 >= nM_max) return 0;
    if (nJ_max == 0) return (int)hipErrorInvalidValue;   // (members without joints to end at)
    if (!trs_loss_fits(nJ_max, nM_max, L)) return (int)hipErrorInvalidValue;
    const int g = pass(nJ_max, nM_max, L, WAVES, 0);
    if (g <= 0) return (int)hipErrorInvalidValue;   // (the kernel's pass loop steps by g)
    trs_lds::raise_lds_once<trs_loss_apply_kernel>();
    const int slices = (C + TRS_LOSS_SLICE - 1) / TRS_LOSS_SLICE;
    hipLaunchKernelGGL(trs_loss_apply_kernel, dim3((unsigned)slices * (unsigned)B), dim3(64 * WAVES),
                       lds(nJ_max, nM_max, g, WAVES, 0), stream, bt, L, g, e0, C, TRS_LOSS_SLICE, Z, U, r_tol, r, critical,
                       peak_stress, peak_member, peak_displace, peak_joint, N_after);
    return (int)hipGetLastError();
}

}  // namespace

int trs_col::rhs_launch(int B, const TrsBatch& bt, int e0, const int* cols, int C, double* Z, hipStream_t stream) {
    if (B < 0 || e0 < 0 || C < 0 || bt.nJ_max < 0 || bt.nM_max < 0 || bt.ld_f < 0) return (int)hipErrorInvalidValue;
    if (B == 0 || C == 0) return 0;
    hipLaunchKernelGGL(trs_columns_rhs_kernel, dim3((unsigned)((C + WAVES - 1) / WAVES) * (unsigned)B), dim3(64 * WAVES),
                       0, stream, bt, e0, cols, C, Z);
    return (int)hipGetLastError();
}

extern "C" {

int trs_loss_abi_version(void) { return TRS_LOSS_ABI_VERSION; }

int trs_loss_fits(int nJ_max, int nM_max, int L) {
    return fits(nJ_max, nM_max, L, WAVES, 0);
}

int trs_loss_rhs(int B, int e0, int C, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                 const double* A, const int32_t* free_index, const int32_t* n_free, const int32_t* nM, double* Z,
                 int ld_f, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nullptr, nM,
                                  nullptr, ld_f);
    return rhs_launch(B, bt, e0, nullptr, C, Z, (hipStream_t)stream);
}

int trs_loss_tab_rhs(int B, int e0, int C, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                     const uint8_t* type_idx, const double* types, const int32_t* free_index, const int32_t* n_free,
                     const int32_t* nM, double* Z, int ld_f, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free,
                                  nullptr, nM, nullptr, ld_f);
    return rhs_launch(B, bt, e0, nullptr, C, Z, (hipStream_t)stream);
}

int trs_loss_apply(int B, int L, int e0, int C, int nJ_max, int nM_max, const double* xyz, const int32_t* conn,
                   const double* E, const double* A, const int32_t* free_index, const int32_t* nJ, const int32_t* nM,
                   const double* Z, const double* U, int ld_f, double r_tol, double* r, int32_t* critical,
                   double* peak_stress, int32_t* peak_member, double* peak_displace, int32_t* peak_joint,
                   double* N_after, const int32_t* joint_out, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, nullptr, nJ, nM,
                                  joint_out, ld_f);
    return loss_apply_launch(B, bt, L, e0, C, Z, U, r_tol, r, critical, peak_stress, peak_member, peak_displace, peak_joint,
                             N_after, (hipStream_t)stream);
}

int trs_loss_tab_apply(int B, int L, int e0, int C, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                       const uint8_t* type_idx, const double* types, const int32_t* free_index, const int32_t* nJ,
                       const int32_t* nM, const double* Z, const double* U, int ld_f, double r_tol, double* r,
                       int32_t* critical, double* peak_stress, int32_t* peak_member, double* peak_displace,
                       int32_t* peak_joint, double* N_after, const int32_t* joint_out, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, nullptr, nJ,
                                  nM, joint_out, ld_f);
    return loss_apply_launch(B, bt, L, e0, C, Z, U, r_tol, r, critical, peak_stress, peak_member, peak_displace, peak_joint,
                             N_after, (hipStream_t)stream);
}

}  // extern "C"
