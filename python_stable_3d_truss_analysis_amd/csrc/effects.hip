// Load cases with support settlements, member pre-strain and self-weight (include/trs_effects.h): equivalent joint
// loads on the way in, a correction of N and of the support forces on the way out - the factor in the slab and
// trs_potrs_cases (cases.hip) are used as they are.
//
//   trs_effects_rhs      loads, eps0 [B][L][nM_max], ubar, accel [B][L][3] -> reduced right-hand sides F [B][L][ld_f]
//   trs_potrs_cases      K_ff x = f (cases.hip, unchanged)
//   trs_effects_recover  u (ubar at the constrained DOFs), f_ext, N = k c . D u - E A eps0, body
//
// With k = E A / len, c the direction cosines, D. = (.)_j1 - (.)_j0 and g the case's body-force vector:
//   s_m    = E A eps0_m - k c . D ubar                   member term of the right-hand side
//   body_j = sum_ends 1/2 (a len density) g              the same vector on every axis' DOF, per axis
//   rhs_f  = loads_f + body_f + sum_ends (+- s_m c)      free DOFs
//   f_c    = sum_ends (+- N_m c) - body_c                constrained DOFs; f_f = loads_f
//
// One work-group per truss, the shape of trs_adjoint_rhs / trs_recover_cases: the member-end lists of EVERY joint are
// built in LDS once (integer atomics, then sorted by member id), every joint's sums run over its list in member-id
// order, and no floating-point atomic is used anywhere.  N and the support sums are formed by the functions of
// trs_recover.h in trs_recover_cases' order and an effect's term is added only where its pointer is non-null: without
// effects the bits are those of the plain load cases.  The list builder is trs_rec::build_end_lists (trs_recover.h),
// the one that trs_recover_cases and the adjoint kernels use.
#include "../../include/trs_effects.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace {

using namespace trs_rec;

// LDS tables of one truss (both kernels)
struct EffTables : EndLists {  // (the member-end lists of EVERY joint: trs_recover.h)
    double* v;    // [3 nJ_max]  ubar (right-hand side) or u (recovery) of one case, device numbering
    double* pm;   // [nM_max]    one double per member: s_m or N_m of that case
};

template <class Arena>
__host__ __device__ inline EffTables layout(Arena& a, int nJ_max, int nM_max) {
    EffTables t;
    t.v = a.template take<double>(3, nJ_max);
    t.pm = a.template take<double>(nM_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

size_t effects_lds(int nJ_max, int nM_max) { return trs_lds::count([&](auto& a) { layout(a, nJ_max, nM_max); }); }

// Half the weight of member mm on one of its end joints, added to the joint's running body load: the product in
// Member.weight's order (trs_modes_mass forms the same half), ONE function with explicit fused multiply-adds for both
// kernels - the body load in the right-hand side and the one taken out of the support forces are the same bits.
__device__ __forceinline__ void add_end_weight(double (&bd)[3], const TrsMembers& mem, const size_t mm, const double len,
                                               const double* g) {
    const double half = 0.5 * (mem.area(mm) * len * mem.density(mm));
#pragma unroll
    for (int a = 0; a < 3; ++a) bd[a] = fma(half, g[a], bd[a]);
}

// ---- the reduced right-hand side ------------------------------------------------------------------------------------
// (The batch's joint_out slot holds joint_in here: the same map, read the other way.)
__global__ __launch_bounds__(256) void trs_effects_rhs_kernel(const TrsBatch bt, const int L,
                                                              const double* __restrict__ loads,
                                                              const double* __restrict__ eps0,
                                                              const double* __restrict__ ubar,
                                                              const double* __restrict__ accel, double* __restrict__ F) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nM_max = bt.nM_max, ld_f = bt.ld_f, ndof_max = v.ndof_max;
    const size_t mbase = v.mbase;
    trs_lds::Carve lds(sh);
    const EffTables t = layout(lds, bt.nJ_max, nM_max);
    double* ub = t.v;   // ubar at the constrained DOFs, zero elsewhere, device numbering
    double* s = t.pm;   // member term
    const int n = v.nfree, npad = min(trs_round_up(n, TRS_NB), ld_f);
    const bool member_terms = (eps0 != nullptr) | (ubar != nullptr);
    const bool lists = member_terms | (accel != nullptr);
    if (lists) {
        build_end_lists(t, v, tid);
        __syncthreads();
    }
    for (int k = 0; k < L; ++k) {
        const size_t bk = (size_t)b * L + k;
        const double* lk = loads != nullptr ? loads + bk * ndof_max : nullptr;  // caller's numbering
        const double* ubk = ubar != nullptr ? ubar + bk * ndof_max : nullptr;
        const double* ek = eps0 != nullptr ? eps0 + bk * nM_max : nullptr;
        const double* gk = accel != nullptr ? accel + bk * 3 : nullptr;
        double* f = F + bk * ld_f;
        if (member_terms) {
            __syncthreads();  // (the previous case's readers of ub and s are done)
            if (ubk != nullptr)
                for (int d = tid; d < v.ndof; d += 256) {
                    const int o = 3 * v.place(d / 3) + d % 3;
                    ub[d] = v.row_of(d) < 0 ? ubk[o] : 0.0;
                }
            __syncthreads();
            for (int m = tid; m < v.members; m += 256) {
                const int2 c = v.ends(m).c;
                const MemberGeom g = member_geom(v.X, c.x, c.y);
                const double EA = v.mem.EA(mbase + m);
                // - k c . (ubar_j1 - ubar_j0): what the settled supports push into the free DOFs (-K_fc ubar_c)
                double sm = ubk != nullptr ? -member_axial(g, EA, ub, c.x, c.y) : 0.0;
                if (ek != nullptr) sm = fma(EA, ek[m], sm);
                s[m] = sm;
            }
            __syncthreads();
        }
        for (int j = tid; j < v.joints; j += 256) {
            const TrussView::Rows rows = v.rows(j);
            if (rows.all_held()) continue;  // no free DOF here
            double r[3] = {0.0, 0.0, 0.0}, bd[3] = {0.0, 0.0, 0.0};
            if (lists) {
                const int* list = t.ends + t.start[j];
                const int deg = t.cnt[j];
                for (int i = 0; i < deg; ++i) {
                    const int m = list[i] >> 1, end = list[i] & 1;
                    const int2 c = v.ends(m).c;
                    const MemberGeom g = member_geom(v.X, c.x, c.y);
                    if (member_terms) add_end_force(r, g.c, s[m], end);
                    if (gk != nullptr) add_end_weight(bd, v.mem, mbase + m, g.len, gk);
                }
            }
            const int o = 3 * v.place(j);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int row = rows.r[a];
                if (row < 0) continue;
                double val = lk != nullptr ? lk[o + a] : 0.0;
                if (gk != nullptr) val += bd[a];
                if (member_terms) val += r[a];
                f[row] = val;
            }
        }
        for (int c = n + tid; c < npad; c += 256) f[c] = 0.0;
    }
}

// ---- the recovery ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trs_effects_recover_kernel(
    const TrsBatch bt, const int L, const double* __restrict__ loads, const double* __restrict__ eps0,
    const double* __restrict__ ubar, const double* __restrict__ accel, const double* __restrict__ F,
    double* __restrict__ u_out, double* __restrict__ f_out, double* __restrict__ N_out, double* __restrict__ body_out) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nM_max = bt.nM_max, ld_f = bt.ld_f, ndof = v.ndof, ndof_max = v.ndof_max;
    const size_t mbase = v.mbase;
    trs_lds::Carve lds(sh);
    const EffTables t = layout(lds, bt.nJ_max, nM_max);
    double* u = t.v;    // displacements of one case, device numbering: solved at the free DOFs, ubar at the others
    double* Nm = t.pm;  // axial forces of that case
    build_end_lists(t, v, tid);
    __syncthreads();
    for (int k = 0; k < L; ++k) {
        const size_t bk = (size_t)b * L + k;
        const double* fk = F + bk * ld_f;
        const double* lk = loads != nullptr ? loads + bk * ndof_max : nullptr;  // caller's numbering
        const double* ubk = ubar != nullptr ? ubar + bk * ndof_max : nullptr;
        const double* ek = eps0 != nullptr ? eps0 + bk * nM_max : nullptr;
        const double* gk = accel != nullptr ? accel + bk * 3 : nullptr;
        double* uo = u_out + bk * ndof_max;
        double* fo = f_out + bk * ndof_max;
        double* bo = body_out != nullptr ? body_out + bk * ndof_max : nullptr;
        __syncthreads();  // (the previous case's readers of u and Nm are done)
        for (int d = tid; d < ndof_max; d += 256) {
            const int r = v.row_of(d);
            const int o = 3 * v.place(d / 3) + d % 3;
            const double val = r >= 0 ? fk[r] : ((ubk != nullptr && d < ndof) ? ubk[o] : 0.0);
            u[d] = val;
            uo[o] = val;
            if (r >= 0) fo[o] = lk != nullptr ? lk[o] : 0.0;  // free DOF: the applied load
            else if (d >= ndof) fo[o] = 0.0;                  // padding
            if (bo != nullptr && d >= ndof) bo[o] = 0.0;
        }
        __syncthreads();
        for (int m = tid; m < nM_max; m += 256) {
            double axial = 0.0;
            if (m < v.members) {
                const int2 c = v.ends(m).c;
                const MemberGeom g = member_geom(v.X, c.x, c.y);
                const double EA = v.mem.EA(mbase + m);
                axial = member_axial(g, EA, u, c.x, c.y);
                if (ek != nullptr) axial = fma(-EA, ek[m], axial);
                Nm[m] = axial;
            }
            N_out[bk * nM_max + m] = axial;
        }
        __syncthreads();
        for (int j = tid; j < v.joints; j += 256) {
            const TrussView::Rows rows = v.rows(j);
            const bool held = rows.any_held();
            if (!held && bo == nullptr) continue;  // nothing of this joint is written here
            double r[3] = {0.0, 0.0, 0.0}, bd[3] = {0.0, 0.0, 0.0};
            const int* list = t.ends + t.start[j];
            const int deg = t.cnt[j];
            for (int i = 0; i < deg; ++i) {
                const int m = list[i] >> 1, end = list[i] & 1;
                const int2 c = v.ends(m).c;
                const MemberGeom g = member_geom(v.X, c.x, c.y);
                if (held) add_end_force(r, g.c, Nm[m], end);
                if (gk != nullptr) add_end_weight(bd, v.mem, mbase + m, g.len, gk);
            }
            const int o = 3 * v.place(j);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                if (rows.held(a)) fo[o + a] = gk != nullptr ? r[a] - bd[a] : r[a];
                if (bo != nullptr) bo[o + a] = bd[a];
            }
        }
    }
}

bool effects_args_ok(const TrsBatch& bt, int B, int L, const double* accel) {
    if (B < 0 || L < 0 || bt.nJ_max < 0 || bt.nM_max < 0 || bt.ld_f < 0) return false;
    if (B == 0 || L == 0) return true;
    return trs_effects_fits(bt.nJ_max, bt.nM_max) && !(accel != nullptr && bt.mem.tidx == nullptr && bt.mem.rho == nullptr);
}

int effects_rhs_launch(int B, const TrsBatch& bt, int L, const double* loads, const double* eps0, const double* ubar,
                       const double* accel, double* F, hipStream_t stream) {
    if (!effects_args_ok(bt, B, L, accel)) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0) return 0;
    trs_lds::raise_lds_once<trs_effects_rhs_kernel>();
    hipLaunchKernelGGL(trs_effects_rhs_kernel, dim3(B), dim3(256), effects_lds(bt.nJ_max, bt.nM_max), stream, bt, L, loads,
                       eps0, ubar, accel, F);
    return (int)hipGetLastError();
}

int effects_recover_launch(int B, const TrsBatch& bt, int L, const double* loads, const double* eps0, const double* ubar,
                           const double* accel, const double* F, double* u, double* f_ext, double* N, double* body,
                           hipStream_t stream) {
    if (!effects_args_ok(bt, B, L, accel)) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0) return 0;
    trs_lds::raise_lds_once<trs_effects_recover_kernel>();
    hipLaunchKernelGGL(trs_effects_recover_kernel, dim3(B), dim3(256), effects_lds(bt.nJ_max, bt.nM_max), stream, bt, L,
                       loads, eps0, ubar, accel, F, u, f_ext, N, body);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_effects_abi_version(void) { return TRS_EFFECTS_ABI_VERSION; }

int trs_effects_fits(int nJ_max, int nM_max) {
    return nJ_max >= 0 && nM_max >= 0 && effects_lds(nJ_max, nM_max) <= TRS_LDS_BYTES;
}

int trs_effects_rhs(int B, int L, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                    const double* A, const double* rho, const double* loads, const double* eps0, const double* ubar,
                    const double* accel, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                    const int32_t* nM, const int32_t* joint_in, double* F, int ld_f, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A, rho), free_index, n_free, nJ, nM,
                                  joint_in, ld_f);
    return effects_rhs_launch(B, bt, L, loads, eps0, ubar, accel, F, (hipStream_t)stream);
}

int trs_effects_tab_rhs(int B, int L, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                        const uint8_t* type_idx, const double* types, const double* loads, const double* eps0,
                        const double* ubar, const double* accel, const int32_t* free_index, const int32_t* n_free,
                        const int32_t* nJ, const int32_t* nM, const int32_t* joint_in, double* F, int ld_f,
                        void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, joint_in, ld_f);
    return effects_rhs_launch(B, bt, L, loads, eps0, ubar, accel, F, (hipStream_t)stream);
}

int trs_effects_recover(int B, int L, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                        const double* A, const double* rho, const double* loads, const double* eps0, const double* ubar,
                        const double* accel, const int32_t* free_index, const int32_t* nJ, const int32_t* nM,
                        const double* F, int ld_f, double* u, double* f_ext, double* N, double* body,
                        const int32_t* joint_out, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A, rho), free_index, nullptr, nJ, nM,
                                  joint_out, ld_f);
    return effects_recover_launch(B, bt, L, loads, eps0, ubar, accel, F, u, f_ext, N, body, (hipStream_t)stream);
}

int trs_effects_tab_recover(int B, int L, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                            const uint8_t* type_idx, const double* types, const double* loads, const double* eps0,
                            const double* ubar, const double* accel, const int32_t* free_index, const int32_t* nJ,
                            const int32_t* nM, const double* F, int ld_f, double* u, double* f_ext, double* N,
                            double* body, const int32_t* joint_out, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, nullptr, nJ,
                                  nM, joint_out, ld_f);
    return effects_recover_launch(B, bt, L, loads, eps0, ubar, accel, F, u, f_ext, N, body, (hipStream_t)stream);
}

}  // extern "C"
