// Adjoint gradients of a factored, solved batch (include/trs_solver.h "Adjoint gradients"): the vector-Jacobian
// product of the results (u, f_ext, N of every load case) with respect to the design (A, E, xyz, loads), from ONE
// more substitution against the resident factor - no factorisation, no finite differences.
//
//   trs_adjoint_rhs    cotangents gu, gf [B][L][nJ_max][3], gN [B][L][nM_max] (caller's numbering) -> reduced
//                      right-hand sides r_f, F [B][L][ld_f] in the layout trs_potrs_cases reads
//   trs_potrs_cases    K_ff lambda = r_f (cases.hip, unchanged, on a buffer of its own)
//   trs_adjoint_grad   forward field u (reduced, as trs_potrs_cases left it) x adjoint field mu -> gA, gE [B][nM_max],
//                      gxyz [B][nJ_max][3] (summed over the cases), gloads [B][L][nJ_max][3]
//
// With g^ = gf at the constrained DOFs (zero elsewhere), k = E A / len, c the direction cosines, D. = (.)_j1 - (.)_j0:
//   s_m  = k (gN_m + c . D g^)                     member pseudo-force
//   r_f  = gu_f + sum_ends (+- s_m c_m)            free DOFs
//   mu_f = lambda, mu_c = -g^_c
//   t_m  = gN_m - c . D mu,   gA_m = N_m t_m / A_m,   gE_m = N_m t_m / E_m,   gloads_f = mu_f + gf_f
//   g_m  = (k / len) { t_m D u - (c . D u) D mu + (c . D u) (3 c . D mu - 2 gN_m) c },   gxyz_j = sum_ends (+- g_m)
//
// One work-group per truss, as trs_recover_cases: the member-end lists of EVERY joint are built in LDS once
// (trs_rec::build_end_lists in trs_recover.h: integer atomics, then sorted by member id), every joint's sum runs over
// its list in member-id order, the cases are accumulated in the order k = 0 .. L - 1, and no floating-point atomic is
// used anywhere: the results are bit-reproducible from run to run, from stream to stream and between the two member
// forms.
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace {

using namespace trs_rec;

// LDS tables of one truss (both kernels; the right-hand-side kernel uses one of the two DOF vectors)
struct AdjTables : EndLists {  // (the member-end lists of EVERY joint: trs_recover.h)
    double* v0;   // [3 nJ_max]
    double* v1;   // [3 nJ_max]
    double* pm;   // [nM_max]    one double per member
};

template <class Arena>
__host__ __device__ inline AdjTables layout(Arena& a, int nJ_max, int nM_max) {
    AdjTables t;
    t.v0 = a.template take<double>(3, nJ_max);
    t.v1 = a.template take<double>(3, nJ_max);
    t.pm = a.template take<double>(nM_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

// ---- step 1: the reduced right-hand side of the adjoint system ------------------------------------------------------
// (The batch's joint_out slot holds joint_in here: the same map, read the other way.)
__global__ __launch_bounds__(256) void trs_adjoint_rhs_kernel(const TrsBatch bt, const int L,
                                                              const double* __restrict__ gu, const double* __restrict__ gf,
                                                              const double* __restrict__ gN, double* __restrict__ F) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nM_max = bt.nM_max, ld_f = bt.ld_f, ndof_max = v.ndof_max;
    trs_lds::Carve lds(sh);
    const AdjTables t = layout(lds, bt.nJ_max, nM_max);
    double* gh = t.v0;  // g^: gf at the constrained DOFs, device numbering
    double* s = t.pm;   // member pseudo-force
    const int n = v.nfree, npad = min(trs_round_up(n, TRS_NB), ld_f);
    build_end_lists(t, v, tid);
    __syncthreads();
    for (int k = 0; k < L; ++k) {
        const size_t bk = (size_t)b * L + k;
        const double* guk = gu != nullptr ? gu + bk * ndof_max : nullptr;  // caller's numbering
        const double* gfk = gf != nullptr ? gf + bk * ndof_max : nullptr;
        const double* gNk = gN != nullptr ? gN + bk * nM_max : nullptr;
        double* f = F + bk * ld_f;
        __syncthreads();  // (the previous case's readers of gh and s are done)
        for (int d = tid; d < v.ndof; d += 256) {
            const int o = 3 * v.place(d / 3) + d % 3;
            gh[d] = (gfk != nullptr && v.row_of(d) < 0) ? gfk[o] : 0.0;
        }
        __syncthreads();
        for (int m = tid; m < v.members; m += 256) {
            const int2 c = v.ends(m).c;
            const MemberGeom g = member_geom(v.X, c.x, c.y);
            // k c . (g^_j1 - g^_j0): the axial "force" of the field g^
            const double proj = member_axial(g, v.mem.EA(v.mbase + m), gh, c.x, c.y);
            s[m] = gNk != nullptr ? fma(v.mem.EA(v.mbase + m) / g.len, gNk[m], proj) : proj;
        }
        __syncthreads();
        for (int j = tid; j < v.joints; j += 256) {
            const TrussView::Rows rows = v.rows(j);
            if (rows.all_held()) continue;  // no free DOF here
            double r[3] = {0.0, 0.0, 0.0};
            const int* list = t.ends + t.start[j];
            const int deg = t.cnt[j];
            for (int i = 0; i < deg; ++i) {
                const int m = list[i] >> 1, end = list[i] & 1;
                const int2 c = v.ends(m).c;
                const MemberGeom g = member_geom(v.X, c.x, c.y);
                add_end_force(r, g.c, s[m], end);
            }
            const int o = 3 * v.place(j);
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int row = rows.r[a];
                if (row >= 0) f[row] = guk != nullptr ? r[a] + guk[o + a] : r[a];
            }
        }
        for (int c = n + tid; c < npad; c += 256) f[c] = 0.0;
    }
}

// ---- step 3: contraction of the adjoint field with the forward field ------------------------------------------------
__global__ __launch_bounds__(256) void trs_adjoint_grad_kernel(
    const TrsBatch bt, const int L, const double* __restrict__ gf, const double* __restrict__ gN,
    const double* __restrict__ Fu, const double* __restrict__ Lam, double* __restrict__ gA, double* __restrict__ gE,
    double* __restrict__ gxyz, double* __restrict__ gloads) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f, ndof = v.ndof, ndof_max = v.ndof_max;
    const size_t mbase = v.mbase;
    trs_lds::Carve lds(sh);
    const AdjTables t = layout(lds, nJ_max, nM_max);
    double* u = t.v0;    // forward displacements of one case, device numbering
    double* mu = t.v1;   // adjoint field of that case
    double* acc = t.pm;  // sum over the cases of N_m t_m
    const bool want_sections = (gA != nullptr) | (gE != nullptr);
    double* gx = gxyz != nullptr ? gxyz + (size_t)b * ndof_max : nullptr;
    if (gx != nullptr) {
        build_end_lists(t, v, tid);
        __syncthreads();
    }
    for (int k = 0; k < L; ++k) {
        const size_t bk = (size_t)b * L + k;
        const double* uk = Fu + bk * ld_f;
        const double* lk = Lam + bk * ld_f;
        const double* gfk = gf != nullptr ? gf + bk * ndof_max : nullptr;  // caller's numbering
        const double* gNk = gN != nullptr ? gN + bk * nM_max : nullptr;
        double* glk = gloads != nullptr ? gloads + bk * ndof_max : nullptr;
        __syncthreads();  // (the previous case's readers of u and mu are done)
        for (int d = tid; d < ndof_max; d += 256) {
            const int r = v.row_of(d);
            const int o = 3 * v.place(d / 3) + d % 3;
            const double gfo = (gfk != nullptr && d < ndof) ? gfk[o] : 0.0;
            const double lam = r >= 0 ? lk[r] : 0.0;
            u[d] = r >= 0 ? uk[r] : 0.0;
            mu[d] = r >= 0 ? lam : -gfo;
            if (glk != nullptr) glk[o] = r >= 0 ? lam + gfo : 0.0;
        }
        __syncthreads();
        if (want_sections)
            for (int m = tid; m < v.members; m += 256) {
                const int2 c = v.ends(m).c;
                const MemberGeom g = member_geom(v.X, c.x, c.y);
                const double EA = v.mem.EA(mbase + m);
                const double axial = member_axial(g, EA, u, c.x, c.y);  // the bits of the recovery's N
                double cm = 0.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) cm += g.c[a] * (mu[3 * c.y + a] - mu[3 * c.x + a]);
                const double tm = (gNk != nullptr ? gNk[m] : 0.0) - cm;
                acc[m] = k == 0 ? axial * tm : fma(axial, tm, acc[m]);
            }
        if (gx != nullptr)
            for (int j = tid; j < v.joints; j += 256) {
                double r[3] = {0.0, 0.0, 0.0};
                const int* list = t.ends + t.start[j];
                const int deg = t.cnt[j];
                for (int i = 0; i < deg; ++i) {
                    const int m = list[i] >> 1, end = list[i] & 1;
                    const int2 c = v.ends(m).c;
                    const MemberGeom g = member_geom(v.X, c.x, c.y);
                    const double kl = v.mem.EA(mbase + m) / g.len / g.len;
                    double du[3], dm[3], cu = 0.0, cm = 0.0;
#pragma unroll
                    for (int a = 0; a < 3; ++a) {
                        du[a] = u[3 * c.y + a] - u[3 * c.x + a];
                        dm[a] = mu[3 * c.y + a] - mu[3 * c.x + a];
                        cu += g.c[a] * du[a];
                        cm += g.c[a] * dm[a];
                    }
                    const double gn = gNk != nullptr ? gNk[m] : 0.0;
                    const double tm = gn - cm, along = cu * (3.0 * cm - 2.0 * gn);
                    double gm[3];
#pragma unroll
                    for (int a = 0; a < 3; ++a) gm[a] = tm * du[a] - cu * dm[a] + along * g.c[a];
                    add_end_force(r, gm, kl, end);
                }
                // accumulated over the cases in the output itself: joint j is this thread's in every case
                const int o = 3 * v.place(j);
#pragma unroll
                for (int a = 0; a < 3; ++a) gx[o + a] = k == 0 ? r[a] : gx[o + a] + r[a];
            }
    }
    __syncthreads();
    for (int m = tid; m < nM_max; m += 256) {
        const bool live = m < v.members;
        if (gA != nullptr) gA[mbase + m] = live ? acc[m] / v.mem.area(mbase + m) : 0.0;
        if (gE != nullptr) gE[mbase + m] = live ? acc[m] / modulus(v.mem, mbase + m) : 0.0;
    }
    if (gx != nullptr)
        for (int j = v.joints + tid; j < nJ_max; j += 256) {
            const int o = 3 * v.place(j);
            gx[o] = gx[o + 1] = gx[o + 2] = 0.0;
        }
}

}  // namespace

extern "C" size_t trs_adjoint_lds(int nJ_max, int nM_max) {
    return trs_lds::count([&](auto& a) { layout(a, nJ_max, nM_max); });
}

int trs_adjoint_rhs_launch(int B, const TrsBatch& bt, int L, const double* gu, const double* gf, const double* gN, double* F,
                           hipStream_t stream) {
    if (B <= 0 || L <= 0) return 0;
    const size_t lds = trs_adjoint_lds(bt.nJ_max, bt.nM_max);
    if (lds > TRS_LDS_BYTES) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_adjoint_rhs_kernel>();
    hipLaunchKernelGGL(trs_adjoint_rhs_kernel, dim3(B), dim3(256), lds, stream, bt, L, gu, gf, gN, F);
    return (int)hipGetLastError();
}

int trs_adjoint_grad_launch(int B, const TrsBatch& bt, int L, const double* gf, const double* gN, const double* Fu,
                            const double* Lam, double* gA, double* gE, double* gxyz, double* gloads, hipStream_t stream) {
    if (B <= 0 || L <= 0) return 0;
    const size_t lds = trs_adjoint_lds(bt.nJ_max, bt.nM_max);
    if (lds > TRS_LDS_BYTES) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_adjoint_grad_kernel>();
    hipLaunchKernelGGL(trs_adjoint_grad_kernel, dim3(B), dim3(256), lds, stream, bt, L, gf, gN, Fu, Lam, gA, gE, gxyz,
                       gloads);
    return (int)hipGetLastError();
}
