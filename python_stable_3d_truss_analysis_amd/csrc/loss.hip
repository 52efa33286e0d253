// Member-loss analysis (include/trs_loss.h): what every single-member removal does to a truss, from the factor in the
// slab - a removal is the rank-one change K_ff - k_e b_e b_e^T, so one substitution column per member (trs_potrs_cases,
// cases.hip, as it is) and one gather kernel replace one factorisation per member.
//
//   trs_loss_rhs      Z [B][C][ld_f]: row i = b_{e0 + i},f (six non-zeros at most)
//   trs_potrs_cases   z_e = inv(K_ff) b_e,f
//   trs_loss_apply    q_m = k_m c_m . D z_e,  r_e = 1 - q_e,  alpha = N_e / r_e,  u' = u + alpha z_e,  N'_m = N_m + alpha q_m
//                     and the maxima of |N'_m| / A_m over m != e and of |u'_j| over the joints
//
// The apply kernel is one work-group of four waves per (truss, slice of the chunk).  Staged in LDS once per work-group:
// per member the end joints, c, k and 1 / A (the geometry is formed once, not once per removed member and case), the
// DOF map, joint_out, and the intact u (joint layout) and N (k c . D u from the staged c and k, the expression that
// forms q_m) of the cases of one pass.  Every wave then takes one removed member at a time: z_e goes into a joint-layout LDS
// vector of the wave's own (zeros at held DOFs), the lanes run over the members and over the joints with the per-case
// maxima in registers, and a wave reduction that carries the index with the value closes each (e, l).  Max is exact and
// every other number is one fixed expression of staged values: the result of (e, l) does not depend on the chunk, the
// slice, the pass, L, B or the member form.
#include "../../include/trs_loss.h"
#include "trs_common.h"
#include "trs_loss_row.h"
#include "trs_recover.h"

#include <limits.h>
#include <math.h>

namespace {

using namespace trs_rec;
using trs_loss_row::wave_max_index;

#ifndef TRS_LOSS_WAVES
#define TRS_LOSS_WAVES 4          // waves per work-group (EXPERIMENTS R14); trs_loss_fits' rule counts their z vectors
#endif
constexpr int WAVES = TRS_LOSS_WAVES;   // each owns one z vector in LDS
constexpr int MAX_PASS = 8;       // load cases per pass at most (their maxima live in registers)
constexpr size_t LDS_BUDGET = 160 * 1024;   // a CU's LDS: the ONE number behind trs_loss_fits, the passes and the launch
                                             // (bar-942 needs 86 KB with one case, so two work-groups per CU never fit it)
#ifndef TRS_LOSS_SLICE
#define TRS_LOSS_SLICE 32         // removed members per work-group (EXPERIMENTS R14)
#endif

// LDS of the apply kernel with g cases per pass (the rule of trs_loss_fits)
size_t loss_lds(int nJ_max, int nM_max, int g) {
    const size_t doubles = (size_t)5 * nM_max + (size_t)3 * nJ_max * WAVES + (size_t)g * ((size_t)3 * nJ_max + nM_max);
    const size_t ints = (size_t)2 * nM_max + (size_t)4 * nJ_max;
    return (doubles * sizeof(double) + ints * sizeof(int) + 15) / 16 * 16;
}

// cases per pass: the largest g <= min(L, MAX_PASS) that fits, evened out over the passes it makes necessary; 0 = none
int loss_pass(int nJ_max, int nM_max, int L) {
    int g = L < MAX_PASS ? L : MAX_PASS;
    while (g > 0 && loss_lds(nJ_max, nM_max, g) > LDS_BUDGET) --g;
    if (g <= 0) return 0;
    const int passes = (L + g - 1) / g;
    return (L + passes - 1) / passes;
}

struct LossTables {
    double *cx, *cy, *cz, *k, *ia;   // [nM_max] each
    double* z;                       // [WAVES][3 nJ_max]
    double* u;                       // [g][3 nJ_max]
    double* N;                       // [g][nM_max]
    int2* ends;                      // [nM_max]
    int* fi;                         // [3 nJ_max]
    int* jo;                         // [nJ_max]
};

__device__ __forceinline__ LossTables loss_tables(double* sh, int nJ_max, int nM_max, int g) {
    LossTables t;
    t.cx = sh;
    t.cy = t.cx + nM_max;
    t.cz = t.cy + nM_max;
    t.k = t.cz + nM_max;
    t.ia = t.k + nM_max;
    t.z = t.ia + nM_max;
    t.u = t.z + (size_t)WAVES * 3 * nJ_max;
    t.N = t.u + (size_t)g * 3 * nJ_max;
    t.ends = reinterpret_cast<int2*>(t.N + (size_t)g * nM_max);
    t.fi = reinterpret_cast<int*>(t.ends + nM_max);
    t.jo = t.fi + 3 * nJ_max;
    return t;
}

// ---- the right-hand sides: one wave per row --------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WAVES) void trs_loss_rhs_kernel(const int e0, const int C, const double* __restrict__ xyz,
                                                           const TrsMembers mem, const int* __restrict__ free_index,
                                                           const int* __restrict__ n_free, const int* __restrict__ nM,
                                                           const int nJ_max, const int nM_max, double* __restrict__ Z,
                                                           const int ld_f) {
    const int per_truss = (C + WAVES - 1) / WAVES;   // work-groups per truss
    const int b = blockIdx.x / per_truss, lane = threadIdx.x & 63;
    const int i = (blockIdx.x - b * per_truss) * WAVES + (threadIdx.x >> 6);
    if (i >= C) return;
    const int e = e0 + i;
    const int npad = trs_round_up(n_free[b], TRS_NB);
    double* row = Z + ((size_t)b * C + i) * ld_f;
    trs_loss_row::write_row(row, npad, lane, e < nM[b], (size_t)b * nM_max + e, mem, xyz + (size_t)b * 3 * nJ_max,
                            free_index + (size_t)b * 3 * nJ_max);
}

// ---- the apply kernel ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * WAVES) void trs_loss_apply_kernel(
    const int L, const int g, const int e0, const int C, const int slice, const double* __restrict__ xyz,
    const TrsMembers mem, const int* __restrict__ free_index, const int* __restrict__ nJ, const int* __restrict__ nM,
    const int nJ_max, const int nM_max, const double* __restrict__ Z, const double* __restrict__ U, const int ld_f,
    const double r_tol, double* __restrict__ r_out, int* __restrict__ crit_out, double* __restrict__ ps_out,
    int* __restrict__ pm_out, double* __restrict__ pd_out, int* __restrict__ pj_out, double* __restrict__ NA,
    const int* __restrict__ joint_out) {
    extern __shared__ double sh[];
    const int slices = (C + slice - 1) / slice;   // work-groups per truss
    const int b = blockIdx.x / slices, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the removed members of this work-group: first <= e < last (inside the chunk and inside the arrays)
    const int first = e0 + (blockIdx.x - b * slices) * slice;
    const int last = min(min(first + slice, e0 + C), nM_max);
    if (first >= last) return;
    const int joints = nJ[b], members = nM[b];
    const int ndof = 3 * joints, ndof_max = 3 * nJ_max;
    const LossTables t = loss_tables(sh, nJ_max, nM_max, g);
    const size_t mbase = (size_t)b * nM_max;
    const double* X = xyz + (size_t)b * ndof_max;
    double* zw = t.z + (size_t)wave * ndof_max;
    const double inf = __builtin_huge_val(), nan = __builtin_nan("");

    // once per work-group: the member table, the DOF map, the joint order
    for (int m = tid; m < members; m += 64 * WAVES) {
        const int2 c = mem.ends(mbase + m);
        const MemberGeom mg = member_geom(X, c.x, c.y);
        t.ends[m] = c;
        t.cx[m] = mg.c[0];
        t.cy[m] = mg.c[1];
        t.cz[m] = mg.c[2];
        t.k[m] = mem.EA(mbase + m) / mg.len;
        t.ia[m] = 1.0 / mem.area(mbase + m);
    }
    for (int d = tid; d < ndof; d += 64 * WAVES) t.fi[d] = free_index[(size_t)b * ndof_max + d];
    for (int j = tid; j < joints; j += 64 * WAVES) t.jo[j] = joint_out != nullptr ? joint_out[(size_t)b * nJ_max + j] : j;

    for (int l0 = 0; l0 < L; l0 += g) {
        const int lg = min(g, L - l0);   // the cases of this pass: l0 .. l0 + lg - 1
        __syncthreads();                 // (the tables above are written; the previous pass's readers of u and N are done)
        for (int x = tid; x < lg * ndof; x += 64 * WAVES) {
            const int l = x / ndof, d = x - l * ndof;
            const int row = t.fi[d];
            t.u[(size_t)l * ndof_max + d] = row >= 0 ? U[((size_t)b * L + l0 + l) * ld_f + row] : 0.0;
        }
        __syncthreads();
        for (int x = tid; x < lg * members; x += 64 * WAVES) {   // N = k c . (u_j1 - u_j0) from the staged c and k: the
            const int l = x / members, m = x - l * members;      // geometry is not formed again per case and pass
            const double* ul = t.u + (size_t)l * ndof_max;
            const int2 c = t.ends[m];
            double p = t.cx[m] * (ul[3 * c.y] - ul[3 * c.x]);
            p = fma(t.cy[m], ul[3 * c.y + 1] - ul[3 * c.x + 1], p);
            p = fma(t.cz[m], ul[3 * c.y + 2] - ul[3 * c.x + 2], p);
            t.N[(size_t)l * nM_max + m] = t.k[m] * p;
        }
        __syncthreads();

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
            const int2 ce = t.ends[e];
            double pe = t.cx[e] * (zw[3 * ce.y] - zw[3 * ce.x]);
            pe = fma(t.cy[e], zw[3 * ce.y + 1] - zw[3 * ce.x + 1], pe);
            pe = fma(t.cz[e], zw[3 * ce.y + 2] - zw[3 * ce.x + 2], pe);
            const double re = 1.0 - t.k[e] * pe;
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
                    const int2 c = t.ends[m];
                    double p = t.cx[m] * (zw[3 * c.y] - zw[3 * c.x]);
                    p = fma(t.cy[m], zw[3 * c.y + 1] - zw[3 * c.x + 1], p);
                    p = fma(t.cz[m], zw[3 * c.y + 2] - zw[3 * c.x + 2], p);
                    q = t.k[m] * p;
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
                double v = best[l];
                int i = where[l];
                wave_max_index(v, i);
                if (lane == 0) {
                    const size_t o = out0 + (size_t)l * nM_max;
                    ps_out[o] = i == INT_MAX ? 0.0 : v;
                    pm_out[o] = i == INT_MAX ? -1 : i;
                }
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
                double v = best[l];
                int i = where[l];
                wave_max_index(v, i);
                if (lane == 0) {
                    const size_t o = out0 + (size_t)l * nM_max;
                    pd_out[o] = i == INT_MAX ? 0.0 : v;
                    pj_out[o] = i == INT_MAX ? -1 : i;
                }
            }
            __builtin_amdgcn_wave_barrier();   // (the next member's z overwrites zw)
        }
    }
}

int loss_rhs_launch(int B, int e0, int C, int nJ_max, int nM_max, const double* xyz, const TrsMembers& mem,
                    const int* free_index, const int* n_free, const int* nM, double* Z, int ld_f, hipStream_t stream) {
    if (B < 0 || e0 < 0 || C < 0 || nJ_max < 0 || nM_max < 0 || ld_f < 0) return (int)hipErrorInvalidValue;
    if (B == 0 || C == 0) return 0;
    hipLaunchKernelGGL(trs_loss_rhs_kernel, dim3((unsigned)((C + WAVES - 1) / WAVES) * (unsigned)B), dim3(64 * WAVES), 0,
                       stream, e0, C, xyz, mem, free_index, n_free, nM, nJ_max, nM_max, Z, ld_f);
    return (int)hipGetLastError();
}

int loss_apply_launch(int B, int L, int e0, int C, int nJ_max, int nM_max, const double* xyz, const TrsMembers& mem,
                      const int* free_index, const int* nJ, const int* nM, const double* Z, const double* U, int ld_f,
                      double r_tol, double* r, int* critical, double* peak_stress, int* peak_member,
                      double* peak_displace, int* peak_joint, double* N_after, const int* joint_out,
                      hipStream_t stream) {
    if (B < 0 || L < 0 || e0 < 0 || C < 0 || nJ_max < 0 || nM_max < 0 || ld_f < 0)
        return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0 || C == 0 || e0 >= nM_max) return 0;
    if (!trs_loss_fits(nJ_max, nM_max, L)) return (int)hipErrorInvalidValue;
    const int g = loss_pass(nJ_max, nM_max, L);
    if (g <= 0) return (int)hipErrorInvalidValue;   // (the kernel's pass loop steps by g)
    static const int lds_limit_set = (int)hipFuncSetAttribute(   // once per process, not per launch
        reinterpret_cast<const void*>(trs_loss_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_BUDGET);
    (void)lds_limit_set;
    const int slices = (C + TRS_LOSS_SLICE - 1) / TRS_LOSS_SLICE;
    hipLaunchKernelGGL(trs_loss_apply_kernel, dim3((unsigned)slices * (unsigned)B), dim3(64 * WAVES),
                       loss_lds(nJ_max, nM_max, g), stream, L, g, e0, C, TRS_LOSS_SLICE, xyz, mem, free_index, nJ, nM,
                       nJ_max, nM_max, Z, U, ld_f, r_tol, r, critical, peak_stress, peak_member, peak_displace,
                       peak_joint, N_after, joint_out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_loss_abi_version(void) { return TRS_LOSS_ABI_VERSION; }

int trs_loss_fits(int nJ_max, int nM_max, int L) {
    return nJ_max >= 0 && nM_max >= 0 && L >= 0 && loss_lds(nJ_max, nM_max, 1) <= LDS_BUDGET;
}

int trs_loss_rhs(int B, int e0, int C, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                 const double* A, const int32_t* free_index, const int32_t* n_free, const int32_t* nM, double* Z,
                 int ld_f, void* stream) {
    return loss_rhs_launch(B, e0, C, nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nM, Z,
                           ld_f, (hipStream_t)stream);
}

int trs_loss_tab_rhs(int B, int e0, int C, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                     const uint8_t* type_idx, const double* types, const int32_t* free_index, const int32_t* n_free,
                     const int32_t* nM, double* Z, int ld_f, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    return loss_rhs_launch(B, e0, C, nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free,
                           nM, Z, ld_f, (hipStream_t)stream);
}

int trs_loss_apply(int B, int L, int e0, int C, int nJ_max, int nM_max, const double* xyz, const int32_t* conn,
                   const double* E, const double* A, const int32_t* free_index, const int32_t* nJ, const int32_t* nM,
                   const double* Z, const double* U, int ld_f, double r_tol, double* r, int32_t* critical,
                   double* peak_stress, int32_t* peak_member, double* peak_displace, int32_t* peak_joint,
                   double* N_after, const int32_t* joint_out, void* stream) {
    return loss_apply_launch(B, L, e0, C, nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, nJ, nM, Z, U,
                             ld_f, r_tol, r, critical, peak_stress, peak_member, peak_displace, peak_joint, N_after,
                             joint_out, (hipStream_t)stream);
}

int trs_loss_tab_apply(int B, int L, int e0, int C, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                       const uint8_t* type_idx, const double* types, const int32_t* free_index, const int32_t* nJ,
                       const int32_t* nM, const double* Z, const double* U, int ld_f, double r_tol, double* r,
                       int32_t* critical, double* peak_stress, int32_t* peak_member, double* peak_displace,
                       int32_t* peak_joint, double* N_after, const int32_t* joint_out, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    return loss_apply_launch(B, L, e0, C, nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, nJ,
                             nM, Z, U, ld_f, r_tol, r, critical, peak_stress, peak_member, peak_displace, peak_joint,
                             N_after, joint_out, (hipStream_t)stream);
}

}  // extern "C"
