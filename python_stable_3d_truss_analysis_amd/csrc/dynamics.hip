// Transient response by Newmark time stepping on a resident factor of K_ff + sigma M (include/trs_dynamics.h).  The
// substitution of every step is trs_potrs_cases (cases.hip) and the mass is trs_modes_mass (modes.hip), both as they
// are; this file holds what goes around them:
//
//   trs_dyn_shift     S[c][c] += sigma Mf[c] on the assembled slab, before the factorisation
//   trs_dyn_step      one time point: state update, envelopes, monitor rows, the right-hand side of the next point
//   trs_dyn_collect   the last u, v, a in the caller's joint numbering
//
// trs_dyn_step: one 256-thread work-group per truss, a loop over the L cases.  Per case
//   phase 1  one thread per DOF d (joint layout; its reduced row r = free_index[d]): u_n from F, the Newmark update of U,
//            V, Acc [r] in place, u_n to LDS in joint layout, the peak of |u|; with beta_R = 0 the same thread writes the
//            right-hand side of the next point into F[r] - it holds everything that needs
//   phase 2  one thread per member: N_m = k c . (u_j1 - u_j0) by trs_rec::member_axial (the recovery's own function),
//            the signed extremes; then the monitor rows
//   phase 3  (beta_R > 0 only) w = a1 u + a4 v + a5 a to LDS, s_m = member_axial(w) per member, then one thread per joint
//            sums +- s_m c over its end list in member-id order (trs_rec::build_end_lists, add_end_force) - K_ff w - and
//            writes the right-hand side of its three DOFs.  The shape of trs_effects_rhs.
// One thread owns a DOF, a member or a joint in every phase; no floating-point atomic; every sum in one fixed order.
// The member geometry is formed again per case and time point (sqrt and four divisions per member), which keeps the
// LDS at one DOF vector and N the recovery's bits; EXPERIMENTS R18 has what that costs (bar-942 x 4096: 0.12 ms per case
// and time point, latency- and geometry-bound, not memory-bound).
#include "../../include/trs_dynamics.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace {

using namespace trs_rec;

// the scheme's constants (include/trs_dynamics.h), formed once on the host in plain double arithmetic
struct DynCoef {
    double a0, a2, a3;       // a_(n+1) = a0 (u_(n+1) - u_n) - a2 v_n - a3 a_n
    double dt_old, dt_new;   // v_(n+1) = v_n + dt (1 - gamma) a_n + dt gamma a_(n+1)
    double cu, cv, ca;       // M [cu u + cv v + ca a],  cu = a0 + alpha a1, cv = a2 + alpha a4, ca = a3 + alpha a5
    double a1, a4, a5;       // w = a1 u + a4 v + a5 a
    double beta_r, s;        // rhs = (... + beta_r K w) / s,  s = 1 + a1 beta_r
};

DynCoef dyn_coef(double dt, double beta, double gamma, double damp_mass, double damp_stiff) {
    DynCoef c;
    const double a1 = gamma / (beta * dt), a4 = gamma / beta - 1.0, a5 = 0.5 * dt * (gamma / beta - 2.0);
    c.a0 = 1.0 / (beta * dt * dt);
    c.a2 = 1.0 / (beta * dt);
    c.a3 = 1.0 / (2.0 * beta) - 1.0;
    c.dt_old = dt * (1.0 - gamma);
    c.dt_new = dt * gamma;
    c.cu = c.a0 + damp_mass * a1;
    c.cv = c.a2 + damp_mass * a4;
    c.ca = c.a3 + damp_mass * a5;
    c.a1 = a1;
    c.a4 = a4;
    c.a5 = a5;
    c.beta_r = damp_stiff;
    c.s = 1.0 + a1 * damp_stiff;
    return c;
}

// LDS tables of one truss
struct DynTables : EndLists {   // (the member-end lists: beta_R > 0 only)
    double* v;    // [3 nJ_max]  u_n, then w, of one case in joint layout; zero at held DOFs and past the truss's joints
    double* pm;   // [nM_max]    s_m of that case (beta_R > 0 only)
};

// (an undamped launch allocates v alone; the kernel carves with damped = true and touches nothing behind v then)
template <class Arena>
__host__ __device__ inline DynTables layout(Arena& a, int nJ_max, int nM_max, bool damped) {
    DynTables t = {};
    t.v = a.template take<double>(3, nJ_max);
    if (!damped) return t;
    t.pm = a.template take<double>(nM_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

size_t dyn_lds(int nJ_max, int nM_max, int damped) {
    return trs_lds::count([&](auto& a) { layout(a, nJ_max, nM_max, damped != 0); });
}

// k c . (v_j1 - v_j0) of member m for a joint-layout vector v
__device__ __forceinline__ double member_force(const TrussView& tr, const int m, const double* v) {
    const int2 c = tr.ends(m).c;
    const MemberGeom g = member_geom(tr.X, c.x, c.y);
    return member_axial(g, tr.mem.EA(tr.mbase + m), v, c.x, c.y);
}

// The right-hand side of the next point at one free DOF: f + M [cu u + cv v + ca a] (+ beta_R (K w)) over s.  ONE
// function for the undamped and the damped path.
__device__ __forceinline__ double next_rhs(const DynCoef& c, const bool damped, const double f, const double m,
                                           const double u, const double v, const double a, const double kw) {
    const double inert = fma(c.ca, a, fma(c.cv, v, c.cu * u));
    double r = fma(m, inert, f);
    if (damped) r = fma(c.beta_r, kw, r) / c.s;
    return r;
}

// f at one free DOF: scale P - M ag (the term of an absent input is not formed)
__device__ __forceinline__ double load_at(const double sc, const double p, const double m, const double* ag, const int axis) {
    const double f = sc * p;
    return ag != nullptr ? fma(-m, ag[axis], f) : f;
}

// strict extremes in step order: the first point that attains a value keeps it
__device__ __forceinline__ void take_max(double* __restrict__ peak, int* __restrict__ at, const size_t i, const double v,
                                         const int step, const bool init) {
    if (init || v > peak[i]) {
        peak[i] = v;
        at[i] = step;
    }
}
__device__ __forceinline__ void take_min(double* __restrict__ peak, int* __restrict__ at, const size_t i, const double v,
                                         const int step, const bool init) {
    if (init || v < peak[i]) {
        peak[i] = v;
        at[i] = step;
    }
}

__global__ __launch_bounds__(256) void trs_dyn_step_kernel(
    const TrsBatch bt, const int L, const double* __restrict__ Mf, const double* __restrict__ Pr,
    const double* __restrict__ scale, const double* __restrict__ ag, const int T1, const int step, const int first,
    const DynCoef co, double* F, double* U, double* V, double* Acc, double* __restrict__ u_peak, int* __restrict__ u_step,
    double* __restrict__ N_max, int* __restrict__ N_max_step, double* __restrict__ N_min, int* __restrict__ N_min_step,
    const int* __restrict__ mon_joint, const int Pj, const int* __restrict__ mon_member, const int Pm,
    double* __restrict__ hist_u, double* __restrict__ hist_N) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView tr = bt.truss(b);
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max, ld_f = bt.ld_f;
    const int joints = tr.joints, members = tr.members, ndof_max = tr.ndof_max;
    const int n = tr.nfree, npad = min(trs_round_up(n, TRS_NB), ld_f);
    trs_lds::Carve lds(sh);
    const DynTables t = layout(lds, nJ_max, nM_max, true);
    double* ush = t.v;
    const double* mf = Mf + (size_t)b * ld_f;
    const bool last = step == T1 - 1, init = first != 0;
    const bool damped = co.beta_r > 0.0;
    const bool stiff_term = damped & !last;
    // (the case loop opens with the barrier that the builder leaves to its caller)
    if (stiff_term) build_end_lists(t, tr, tid);
    for (int l = 0; l < L; ++l) {
        const size_t bl = (size_t)b * L + l;
        double* f = F + bl * ld_f;
        double* Uc = U + bl * ld_f;
        double* Vc = V + bl * ld_f;
        double* Ac = Acc + bl * ld_f;
        const double* pr = Pr + bl * ld_f;
        const double sc_now = scale != nullptr ? scale[bl * T1 + step] : 1.0;
        const double sc_next = (scale != nullptr && !last) ? scale[bl * T1 + step + 1] : 1.0;
        const double* ag_now = ag != nullptr ? ag + (bl * T1 + step) * 3 : nullptr;
        const double* ag_next = (ag != nullptr && !last) ? ag + (bl * T1 + step + 1) * 3 : nullptr;
        __syncthreads();   // (the previous case's readers of ush and pm are done; the end lists are sorted)
        // ---- phase 1: the state, one thread per DOF ----
        for (int d = tid; d < ndof_max; d += 256) {
            const int r = tr.row_of(d);
            const int axis = d % 3;
            double u = 0.0;
            if (r >= 0) {
                const double m = mf[r];
                double v, a;
                if (first == 1) {
                    v = 0.0;
                    const double f0 = load_at(sc_now, pr[r], m, ag_now, axis);
                    a = m > 0.0 ? f0 / m : 0.0;
                } else if (first == 0) {
                    u = f[r];
                    const double u_old = Uc[r], v_old = Vc[r], a_old = Ac[r];
                    a = co.a0 * (u - u_old) - co.a2 * v_old - co.a3 * a_old;
                    v = v_old + co.dt_old * a_old + co.dt_new * a;
                } else {
                    u = Uc[r];
                    v = Vc[r];
                    a = Ac[r];
                }
                if (first != 2) {
                    Uc[r] = u;
                    Vc[r] = v;
                    Ac[r] = a;
                }
                if (!last && !damped)
                    f[r] = next_rhs(co, false, load_at(sc_next, pr[r], m, ag_next, axis), m, u, v, a, 0.0);
            }
            ush[d] = u;
            take_max(u_peak, u_step, bl * ndof_max + 3 * tr.place(d / 3) + axis, fabs(u), step, init);
        }
        for (int c = n + tid; c < npad; c += 256) {   // the padding rows
            if (!last) f[c] = 0.0;
            if (first == 1) {
                Uc[c] = 0.0;
                Vc[c] = 0.0;
                Ac[c] = 0.0;
            }
        }
        __syncthreads();
        // ---- phase 2: member forces, envelopes, monitor rows ----
        for (int m = tid; m < nM_max; m += 256) {
            const double axial = m < members ? member_force(tr, m, ush) : 0.0;
            take_max(N_max, N_max_step, bl * nM_max + m, axial, step, init);
            take_min(N_min, N_min_step, bl * nM_max + m, axial, step, init);
        }
        for (int x = tid; x < 3 * Pj; x += 256) {
            const int j = mon_joint[(size_t)b * Pj + x / 3];
            hist_u[((bl * T1 + step) * Pj) * 3 + x] = ((j >= 0) & (j < joints)) ? ush[3 * j + x % 3] : 0.0;
        }
        for (int p = tid; p < Pm; p += 256) {
            const int m = mon_member[(size_t)b * Pm + p];
            hist_N[(bl * T1 + step) * Pm + p] =
                ((m >= 0) & (m < members)) ? member_force(tr, m, ush) : 0.0;
        }
        if (!stiff_term) continue;
        // ---- phase 3: beta_R K_ff w into the right-hand side of the next point ----
        __syncthreads();   // (the readers of u in ush are done)
        for (int d = tid; d < ndof_max; d += 256) {
            const int r = tr.row_of(d);
            ush[d] = r >= 0 ? fma(co.a5, Ac[r], fma(co.a4, Vc[r], co.a1 * Uc[r])) : 0.0;
        }
        __syncthreads();
        for (int m = tid; m < members; m += 256) t.pm[m] = member_force(tr, m, ush);
        __syncthreads();
        for (int j = tid; j < joints; j += 256) {
            const int r3[3] = {tr.row_of(3 * j), tr.row_of(3 * j + 1), tr.row_of(3 * j + 2)};
            if ((r3[0] & r3[1] & r3[2]) < 0) continue;   // no free DOF here
            double kw[3] = {0.0, 0.0, 0.0};
            const int* list = t.ends + t.start[j];
            const int deg = t.cnt[j];
            for (int i = 0; i < deg; ++i) {
                const int m = list[i] >> 1, end = list[i] & 1;
                const int2 c = tr.ends(m).c;
                const MemberGeom g = member_geom(tr.X, c.x, c.y);
                add_end_force(kw, g.c, t.pm[m], end);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int r = r3[a];
                if (r < 0) continue;
                const double m = mf[r];
                f[r] = next_rhs(co, true, load_at(sc_next, pr[r], m, ag_next, a), m, Uc[r], Vc[r], Ac[r], kw[a]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void trs_dyn_shift_kernel(const int* __restrict__ n_free, const int ld,
                                                            const int slab_rows, double* __restrict__ S,
                                                            const double* __restrict__ Mf, const int ld_f,
                                                            const double sigma) {
    const int per = (slab_rows + 255) / 256;   // blocks per truss
    const int b = blockIdx.x / per, c = (blockIdx.x - b * per) * 256 + threadIdx.x;
    if (c >= min(n_free[b], slab_rows)) return;
    double* diag = S + ((size_t)b * slab_rows + c) * ld + c;
    *diag = fma(sigma, Mf[(size_t)b * ld_f + c], *diag);
}

__global__ __launch_bounds__(256) void trs_dyn_collect_kernel(const TrsBatch bt, const int L, const double* __restrict__ U,
                                                              const double* __restrict__ V, const double* __restrict__ Acc,
                                                              double* __restrict__ u, double* __restrict__ v,
                                                              double* __restrict__ a) {
    const int bl = blockIdx.x, b = bl / L, tid = threadIdx.x;
    const TrussView tr = bt.truss(b);
    const size_t in = (size_t)bl * bt.ld_f, out = (size_t)bl * tr.ndof_max;
    for (int d = tid; d < tr.ndof_max; d += 256) {
        const int r = tr.row_of(d);
        const size_t o = out + tr.place_dof(d);
        u[o] = r >= 0 ? U[in + r] : 0.0;
        v[o] = r >= 0 ? V[in + r] : 0.0;
        a[o] = r >= 0 ? Acc[in + r] : 0.0;
    }
}

int dyn_step_launch(int B, const TrsBatch& bt, int L, const double* Mf, const double* Pr, const double* scale,
                    const double* ag, int T1, int n, int first, double dt, double beta, double gamma, double damp_mass,
                    double damp_stiff, double* F, double* U, double* V, double* Acc, double* u_peak, int* u_step,
                    double* N_max, int* N_max_step, double* N_min, int* N_min_step, const int* mon_joint, int Pj,
                    const int* mon_member, int Pm, double* hist_u, double* hist_N, hipStream_t stream) {
    if (B < 0 || L < 0 || bt.nJ_max <= 0 || bt.nM_max < 0 || bt.ld_f < 0 || Pj < 0 || Pm < 0)
        return (int)hipErrorInvalidValue;
    if (T1 < 1 || n < 0 || n >= T1 || first < 0 || first > 2 || (first != 0) != (n == 0)) return (int)hipErrorInvalidValue;
    if (!(dt > 0.0) || !(beta > 0.0) || !(gamma >= 0.5) || !(damp_mass >= 0.0) || !(damp_stiff >= 0.0))
        return (int)hipErrorInvalidValue;
    if ((Pj > 0 && (!mon_joint || !hist_u)) || (Pm > 0 && (!mon_member || !hist_N))) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0) return 0;
    const int damped = damp_stiff > 0.0;
    if (!trs_dyn_fits(bt.nJ_max, bt.nM_max, damped)) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_dyn_step_kernel>();
    hipLaunchKernelGGL(trs_dyn_step_kernel, dim3(B), dim3(256), dyn_lds(bt.nJ_max, bt.nM_max, damped), stream, bt, L, Mf,
                       Pr, scale, ag, T1, n, first, dyn_coef(dt, beta, gamma, damp_mass, damp_stiff), F, U, V, Acc, u_peak,
                       u_step, N_max, N_max_step, N_min, N_min_step, mon_joint, Pj, mon_member, Pm, hist_u, hist_N);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_dyn_abi_version(void) { return TRS_DYN_ABI_VERSION; }

int trs_dyn_fits(int nJ_max, int nM_max, int damped) {
    return nJ_max >= 0 && nM_max >= 0 && dyn_lds(nJ_max, nM_max, damped != 0) <= TRS_LDS_BYTES;
}

int trs_dyn_shift(int B, const int32_t* n_free, int ld, int slab_rows, double* S, const double* Mf, int ld_f,
                  double sigma, void* stream) {
    if (B < 0 || slab_rows <= 0 || ld < slab_rows || ld_f < slab_rows) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    hipLaunchKernelGGL(trs_dyn_shift_kernel, dim3((unsigned)B * (unsigned)((slab_rows + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, n_free, ld, slab_rows, S, Mf, ld_f, sigma);
    return (int)hipGetLastError();
}

int trs_dyn_step(int B, int L, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                 const double* A, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
                 const double* Mf, const double* Pr, const double* scale, const double* ag, int T1, int n, int first,
                 double dt, double beta, double gamma, double damp_mass, double damp_stiff, double* F, double* U,
                 double* V, double* Acc, int ld_f, double* u_peak, int32_t* u_step, double* N_max, int32_t* N_max_step,
                 double* N_min, int32_t* N_min_step, const int32_t* mon_joint, int Pj, const int32_t* mon_member, int Pm,
                 double* hist_u, double* hist_N, const int32_t* joint_out, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nJ, nM,
                                  joint_out, ld_f);
    return dyn_step_launch(B, bt, L, Mf, Pr, scale, ag, T1, n, first, dt, beta, gamma, damp_mass, damp_stiff, F, U, V, Acc,
                           u_peak, u_step, N_max, N_max_step, N_min, N_min_step, mon_joint, Pj, mon_member, Pm, hist_u,
                           hist_N, (hipStream_t)stream);
}

int trs_dyn_tab_step(int B, int L, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16,
                     const uint8_t* type_idx, const double* types, const int32_t* free_index, const int32_t* n_free,
                     const int32_t* nJ, const int32_t* nM, const double* Mf, const double* Pr, const double* scale,
                     const double* ag, int T1, int n, int first, double dt, double beta, double gamma, double damp_mass,
                     double damp_stiff, double* F, double* U, double* V, double* Acc, int ld_f, double* u_peak,
                     int32_t* u_step, double* N_max, int32_t* N_max_step, double* N_min, int32_t* N_min_step,
                     const int32_t* mon_joint, int Pj, const int32_t* mon_member, int Pm, double* hist_u, double* hist_N,
                     const int32_t* joint_out, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, joint_out, ld_f);
    return dyn_step_launch(B, bt, L, Mf, Pr, scale, ag, T1, n, first, dt, beta, gamma, damp_mass, damp_stiff, F, U, V, Acc,
                           u_peak, u_step, N_max, N_max_step, N_min, N_min_step, mon_joint, Pj, mon_member, Pm, hist_u,
                           hist_N, (hipStream_t)stream);
}

int trs_dyn_collect(int B, int L, int nJ_max, const double* U, const double* V, const double* Acc, int ld_f,
                    const int32_t* free_index, const int32_t* nJ, const int32_t* joint_out, double* u, double* v,
                    double* a, void* stream) {
    if (B < 0 || L < 0 || nJ_max < 0 || ld_f < 0) return (int)hipErrorInvalidValue;
    if (B == 0 || L == 0 || nJ_max == 0) return 0;
    hipLaunchKernelGGL(trs_dyn_collect_kernel, dim3((unsigned)B * (unsigned)L), dim3(256), 0, (hipStream_t)stream,
                       trs_batch_dofs(nJ_max, free_index, nullptr, nJ, joint_out, ld_f), L, U, V, Acc, u, v, a);
    return (int)hipGetLastError();
}

}  // extern "C"
