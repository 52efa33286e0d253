// Minimum weight under displacement limits: the optimality-criteria method with one multiplier per limit, iterated on
// the device (include/trs_minweight.h).  The assembly, the factorisation, the gather and the multi-case substitution of
// every iteration are trs_assemble, trs_potrf_batched, trs_gather_cases and trs_potrs_cases as they are - the virtual
// unit loads of the limits are just more columns of the case block; this file holds what turns the L + J reduced
// solutions into the next design:
//
//   trs_mw_step   one analysis: the limit values g_j, the sensitivities c_mj, the dual solve (per limit a geometric
//                 bisection on its multiplier, `sweeps` passes), the resizing, the convergence test and the outputs
//
// The method, analysis k of design A (the header and tests/minweight_reference.py state it in the same words):
//     proj_m(x) = c_m.(x_j1 - x_j0);  c_mj = (E_m / L0_m) proj_m(v_j) proj_m(u_{l_j}) = -dg_j/dA_m
//     g_j = d_j.u_{l_j}(joint), summed in ascending component
//     q_mj = max(c_mj, 0) A_m^2 and n_mj = max(-c_mj, 0) where |c_mj| A_m > 2^-30 max_m |c_mj| A_m, else q_mj = n_mj = 0
//     lo_m = clamp((1 - move) A_m, a_min_m, a_max_m), hi_m = clamp((1 + move) A_m, a_min_m, a_max_m);
//     a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m)
//     gt_j(A') = sum_m (q_mj / A'_m - n_mj A'_m);  P_m = sum_j mu_j q_mj, D_m = w_m + sum_j mu_j n_mj, ascending j
//     A'_m(mu) = clamp(sqrt(P_m / D_m), lo_m, hi_m), and lo_m where P_m <= 0
//     per sweep and limit: gt_j at mu_j = 0 <= ubar_j: mu_j = 0;  else x1 = max(0, the members' thresholds
//     (hi_m^2 D_m - P_m) / q_mj and (P_m / lo_m^2 - D_m) / n_mj);  gt_j at x1 > ubar_j: mu_j = x1;  else 64 times from
//     x0 = 2^-300 x1: xm = sqrt(x0 x1); if gt_j(xm) <= ubar_j then x1 = xm, else x0 = xm;  mu_j = x1
//     change = max_m |A'_m - A_m| / A_m;  worst = max_j g_j / ubar_j
//     change <= tol: status 0 if worst <= 1 + limit_tol, else 3; else k = max_iters: status 1; else A_{k+1} = A'
//
// trs_mw_step: one 256-thread work-group per truss.  A thread owns the members tid, tid + 256, ...: it forms their
// geometry once (c, E / L0, w, A), keeps it in LDS, and is the only thread that ever touches those entries - the member
// tables need no barrier.  The L real solutions and the J virtual ones are staged in LDS through row_of one at a time,
// in two buffers: the next column is staged behind the work on this one, one barrier per column.  A real case leaves
// proj_m(u_l) in the row of every limit that names it; the limit's own column turns that row into c_mj.  Every thread
// holds the truss's multipliers, limit values and limits in registers (the same numbers in every thread: each is read
// from the same reduction slots), so the dual solve needs no broadcast.  Every evaluation of gt_j is one reduction
// behind ONE barrier: reduction e writes the slot set e & 1, whose readers of reduction e - 2 passed the barrier of
// reduction e - 1.  Every sum runs per thread in ascending m, then by the wave butterfly, then over the four waves in
// order.  No floating-point atomic.
#include "../../include/trs_minweight.h"
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_iterate.h"
#include "trs_lds.h"

namespace {

using Run = trs_iter::Run<TRS_MW_ACTIVE, TRS_MW_NOT_PD>;
using trs_iter::wave_max;
using trs_iter::wave_sum;

constexpr int RED = 64;          // doubles for the reductions: two sets of four wave partials, rounded up
constexpr int JMAX = TRS_MW_MAX_LIMITS;

// LDS tables of the step kernel
struct StepTables {
    double* u;      // [2][3 nJ_max]  two columns of the case block, joint layout, device numbering
    double* red;    // [RED]          the wave partials of the reductions
    double* c0;     // [nM_max] x 3   direction cosines; behind the columns lo, hi, A'
    double* c1;
    double* c2;
    double* ek;     // [nM_max]       E / L0
    double* w;      // [nM_max]       rho L0 or L0
    double* a;      // [nM_max]       A
    double* c;      // [J][nM_max]    proj_m(u_{l_j}), then c_mj
    int2* ends;     // [nM_max]       end joints, clamped
    int* row;       // [3 nJ_max]     row_of every DOF (-1: reads 0), formed once: a column's staging is one load deep
};

template <class Arena>
__host__ __device__ inline StepTables step_layout(Arena& a, int nJ_max, int nM_max, int J) {
    StepTables t;
    t.u = a.template take<double>(6, nJ_max);
    t.red = a.template take<double>(RED);
    t.c0 = a.template take<double>(nM_max);
    t.c1 = a.template take<double>(nM_max);
    t.c2 = a.template take<double>(nM_max);
    t.ek = a.template take<double>(nM_max);
    t.w = a.template take<double>(nM_max);
    t.a = a.template take<double>(nM_max);
    t.c = a.template take<double>(J, nM_max);
    t.ends = a.template take<int2>(nM_max);
    t.row = a.template take<int>(3, nJ_max);
    return t;
}

size_t step_lds(int nJ_max, int nM_max, int J) {
    return trs_lds::count([&](auto& a) { step_layout(a, nJ_max, nM_max, J); });
}

struct StepArgs {
    const double* F;          // [B][L + J][ld_f]
    const int* info;          // [B]
    const int* limit_case;    // [J]
    const int* limit_joint;   // [B][J]
    const double* limit_dir;  // [B][J][3]
    const double* limit_value;   // [B][J]
    double move, tol, limit_tol;
    trs_iter::AreaBounds bounds;
    int L, J, it, mode, H, measure, sweeps;
    double* A;                // [B][nM_max]
    double* prev;             // [B][nM_max]
    double* mu;               // [B][J]
    int* st;                  // [B][4]
    int* active;
    double* areas;            // [B][nM_max]
    double* measure_out;      // [B]
    double* measure_history;  // [B][H]
    double* worst_history;    // [B][H]
    double* displacement;     // [B][J]
    double* ratio;            // [B][J]
    double* multipliers;      // [B][J]
    double* sens;             // [B][J][nM_max] or null
};

// One reduction of the work-group behind one barrier; `e` counts the reductions of the kernel (uniform).
struct Reducer {
    double* red;
    int e, tid;
    __device__ __forceinline__ double* slot() { return red + (e++ & 1) * 4; }
    __device__ __forceinline__ double sum(double v) {
        v = wave_sum(v);
        double* q = slot();
        if ((tid & 63) == 0) q[tid >> 6] = v;
        __syncthreads();
        return ((q[0] + q[1]) + q[2]) + q[3];
    }
    __device__ __forceinline__ double max(double v) {
        v = wave_max(v);
        double* q = slot();
        if ((tid & 63) == 0) q[tid >> 6] = v;
        __syncthreads();
        return fmax(fmax(q[0], q[1]), fmax(q[2], q[3]));
    }
};

// What the dual solve reads of one truss; mu in registers, the same in every thread
struct Dual {
    const StepTables& t;
    int J, members, nM_max, tid;
    double mu[JMAX];

    // P_m and D_m with mu_j = x (j = -1: mu as it is), both summed in ascending j
    __device__ __forceinline__ void sums(const int m, const int j, const double x, double& P, double& D) const {
        const double A = t.a[m], A2 = A * A;
        P = 0.0;
        D = t.w[m];
#pragma unroll
        for (int i = 0; i < JMAX; ++i) {
            if (i < J) {
                const double ci = t.c[i * nM_max + m], mi = i == j ? x : mu[i];
                P = P + mi * (fmax(ci, 0.0) * A2);
                D = D + mi * fmax(-ci, 0.0);
            }
        }
    }
    // A'_m(mu) = clamp(sqrt(P_m / D_m), lo_m, hi_m), and lo_m where P_m <= 0
    __device__ __forceinline__ double design(const int m, const int j, const double x) const {
        double P, D;
        sums(m, j, x, P, D);
        const double lo = t.c0[m], hi = t.c1[m];
        return P > 0.0 ? fmin(fmax(sqrt(P / D), lo), hi) : lo;
    }
    // gt_j with mu_j = x
    __device__ __forceinline__ double gt(const int j, const double x, Reducer& r) const {
        double s = 0.0;
        for (int m = tid; m < members; m += 256) {
            const double A = t.a[m], cj = t.c[j * nM_max + m], next = design(m, j, x);
            s += (fmax(cj, 0.0) * (A * A)) / next - fmax(-cj, 0.0) * next;
        }
        return r.sum(s);
    }
    // x1 = max(0, the largest threshold beyond which no member moves any more), P and D taken at mu_j = 0
    __device__ __forceinline__ double top(const int j, Reducer& r) const {
        double x1 = 0.0;
        for (int m = tid; m < members; m += 256) {
            double P, D;
            sums(m, j, 0.0, P, D);
            const double A = t.a[m], cj = t.c[j * nM_max + m], lo = t.c0[m], hi = t.c1[m];
            const double q = fmax(cj, 0.0) * (A * A), n = fmax(-cj, 0.0);
            if (q > 0.0) x1 = fmax(x1, (hi * hi * D - P) / q);
            if (n > 0.0) x1 = fmax(x1, (P / (lo * lo) - D) / n);
        }
        return r.max(x1);
    }
};

__global__ __launch_bounds__(256) void trs_mw_step_kernel(const TrsBatch bt, const StepArgs g) {
    extern __shared__ double sh[];   // (no static LDS beside it: the dynamic ceiling is the whole of a CU's)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nM_max = bt.nM_max, ld_f = bt.ld_f;
    const int mode = g.mode, it = g.it, L = g.L, J = g.J;
    Run run(g.st + 4 * b, it == 0);
    if (!run.active()) return;        // (uniform over the work-group) frozen: nothing is touched
    const TrussView tr = bt.truss(b);
    const int members = tr.members, ndof_max = tr.ndof_max;
    const size_t mbase = tr.mbase;
    double* Ab = g.A + mbase;
    const int pivot = g.info[b];
    if (pivot != 0) {
        // status 2: back to A_{k-1}; the outputs stay those of analysis k - 1 (k = 0: zeros, the initial areas)
        for (int m = tid; m < nM_max; m += 256) {
            if (it == 0) {
                g.areas[mbase + m] = m < members ? Ab[m] : 0.0;
                if (g.sens != nullptr)
                    for (int j = 0; j < J; ++j) g.sens[((size_t)b * J + j) * nM_max + m] = 0.0;
            } else if (m < members) {
                Ab[m] = g.prev[mbase + m];
            }
        }
        if (it == 0 && tid < J) {
            g.displacement[(size_t)b * J + tid] = 0.0;
            g.ratio[(size_t)b * J + tid] = 0.0;
            g.multipliers[(size_t)b * J + tid] = 0.0;
        }
        run.fail(pivot, run.one_back(), tid);
        if (tid == 0 && it == 0) g.measure_out[b] = 0.0;
        return;
    }
    trs_lds::Carve lds(sh);
    const StepTables t = step_layout(lds, bt.nJ_max, nM_max, J);
    const int columns = L + J;
    const trs_iter::CaseStage cases = {t.u, t.row, g.F + (size_t)b * columns * ld_f, ndof_max, ld_f};
    cases.form_rows(tr, tid);
    cases.stage(0, tid);
    // ---- the limits of this truss (the same in every thread); the multipliers of the analysis before ----
    Dual dual = {t, J, members, nM_max, tid, {}};
    double ubar[JMAX], gval[JMAX];
    int lcase[JMAX], ljoint[JMAX];
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        ubar[j] = INFINITY;
        gval[j] = 0.0;
        lcase[j] = -1;     // (-1: switched off)
        ljoint[j] = 0;
        dual.mu[j] = 0.0;
        if (j < J) {
            const int l = g.limit_case[j], joint = g.limit_joint[(size_t)b * J + j];
            const double value = g.limit_value[(size_t)b * J + j];
            if (l >= 0 && l < L && tr.in_truss(joint) && value > 0.0 && value < INFINITY) {
                ubar[j] = value;
                lcase[j] = l;
                ljoint[j] = joint;
                if (it > 0) dual.mu[j] = g.mu[(size_t)b * J + j];
            }
        }
    }
    // ---- the member geometry, once; the measure of the design ----
    const bool by_weight = g.measure == TRS_MW_WEIGHT;
    double msum = 0.0;
    for (int m = tid; m < members; m += 256) {
        const int2 c = tr.ends(m).c;
        const trs_rec::MemberGeom geo = trs_rec::member_geom(tr.X, c.x, c.y);
        const double E = tr.mem.E[mbase + m], A = Ab[m];
        const double w = by_weight ? tr.mem.rho[mbase + m] * geo.len : geo.len;
        t.ends[m] = c;
        t.c0[m] = geo.c[0];
        t.c1[m] = geo.c[1];
        t.c2[m] = geo.c[2];
        t.ek[m] = E / geo.len;
        t.w[m] = w;
        t.a[m] = A;
        msum += w * A;
#pragma unroll
        for (int j = 0; j < JMAX; ++j)
            if (j < J) t.c[j * nM_max + m] = 0.0;   // (a limit that is switched off keeps c_mj = 0)
    }
    __syncthreads();   // (column 0 is staged)
    // ---- the columns: a real case leaves proj_m(u_l) with every limit that names it, limit j's own column makes c_mj ----
    for (int col = 0; col < columns; ++col) {
        const double* u = cases.buffer(col);
        const int own = col - L;   // (>= 0: the column of limit `own`)
        if (own < 0) {
#pragma unroll
            for (int j = 0; j < JMAX; ++j) {
                if (j < J && lcase[j] == col) {
                    const double* d = g.limit_dir + ((size_t)b * J + j) * 3;
                    const double* uj = u + 3 * ljoint[j];
                    double s = d[0] * uj[0];   // ascending component
                    s = s + d[1] * uj[1];
                    s = s + d[2] * uj[2];
                    gval[j] = s;
                }
            }
        }
        bool wanted = own >= 0;
        if (own < 0) {
#pragma unroll
            for (int j = 0; j < JMAX; ++j) wanted |= j < J && lcase[j] == col;
        } else {
#pragma unroll
            for (int j = 0; j < JMAX; ++j) wanted &= j != own || lcase[j] >= 0;
        }
        if (wanted) {   // (uniform)
            for (int m = tid; m < members; m += 256) {
                const int2 c = t.ends[m];
                const double* u0 = u + 3 * c.x;
                const double* u1 = u + 3 * c.y;
                double proj = t.c0[m] * (u1[0] - u0[0]);
                proj += t.c1[m] * (u1[1] - u0[1]);
                proj += t.c2[m] * (u1[2] - u0[2]);
                if (own < 0) {
#pragma unroll
                    for (int j = 0; j < JMAX; ++j)
                        if (j < J && lcase[j] == col) t.c[j * nM_max + m] = proj;
                } else {
                    t.c[own * nM_max + m] = (t.ek[m] * proj) * t.c[own * nM_max + m];
                }
            }
        }
        if (col + 1 < columns) cases.stage(col + 1, tid);   // (the other buffer: its readers passed the barrier before)
        __syncthreads();
    }
    // ---- the outputs of this design; lo, hi of the resizing (over c0, c1: the columns are behind) ----
    const double move = g.move;
    for (int m = tid; m < nM_max; m += 256) {
        double area = 0.0;
        if (m < members) {
            area = t.a[m];
            const double a_lo = g.bounds.lo(mbase + m), a_hi = g.bounds.hi(mbase + m);
            double lo, hi;
            if (t.w[m] > 0.0) {
                lo = fmin(fmax((1.0 - move) * area, a_lo), a_hi);
                hi = fmin(fmax((1.0 + move) * area, a_lo), a_hi);
            } else {
                lo = hi = fmin(fmax(area, a_lo), a_hi);
            }
            t.c0[m] = lo;
            t.c1[m] = hi;
        }
        g.areas[mbase + m] = area;
        if (g.sens != nullptr) {
            for (int j = 0; j < J; ++j) g.sens[((size_t)b * J + j) * nM_max + m] = m < members ? t.c[j * nM_max + m] : 0.0;
        }
    }
    Reducer red = {t.red, 0, tid};
    const double measure = red.sum(msum);
    // ---- a member off a limit's load path (|c_mj| A_m <= 2^-30 max_m |c_mj| A_m) counts with q_mj = n_mj = 0 ----
    for (int j = 0; j < J; ++j) {
        double top = 0.0;
        for (int m = tid; m < members; m += 256) top = fmax(top, fabs(t.c[j * nM_max + m]) * t.a[m]);
        const double cut = ldexp(red.max(top), -TRS_MW_CUT_BITS);
        for (int m = tid; m < members; m += 256) {
            if (!(fabs(t.c[j * nM_max + m]) * t.a[m] > cut)) t.c[j * nM_max + m] = 0.0;
        }
    }
    // ---- the dual solve: `sweeps` passes over the limits, each a search on its own multiplier ----
    for (int sweep = 0; sweep < g.sweeps; ++sweep) {
        for (int j = 0; j < J; ++j) {
            // (ubar[j], lcase[j] and mu[j] through select chains: j is known only at run time, and they live in registers)
            double most = INFINITY;
            bool on = false;
#pragma unroll
            for (int i = 0; i < JMAX; ++i) {
                most = i == j ? ubar[i] : most;
                on = i == j ? lcase[i] >= 0 : on;
            }
            if (!on) continue;   // (uniform)
            double x = 0.0;
            if (!(dual.gt(j, 0.0, red) <= most)) {
                double x1 = dual.top(j, red);
                if (dual.gt(j, x1, red) <= most) {
                    double x0 = ldexp(x1, -TRS_MW_BRACKET_BITS);
                    for (int r = 0; r < TRS_MW_BISECTIONS; ++r) {
                        const double xm = sqrt(x0 * x1);
                        if (dual.gt(j, xm, red) <= most)
                            x1 = xm;
                        else
                            x0 = xm;
                    }
                }
                x = x1;
            }
#pragma unroll
            for (int i = 0; i < JMAX; ++i) dual.mu[i] = i == j ? x : dual.mu[i];
        }
    }
    // ---- the next design, the convergence test ----
    double change = 0.0;
    for (int m = tid; m < members; m += 256) {
        const double area = t.a[m], next = dual.design(m, -1, 0.0);
        change = fmax(change, fabs(next - area) / area);
        t.c2[m] = next;
    }
    change = red.max(change);
    double worst = -INFINITY;
    bool any = false;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
        if (j < J && lcase[j] >= 0) {
            worst = fmax(worst, gval[j] / ubar[j]);
            any = true;
        }
    }
    if (!any) worst = 0.0;
    if (change <= g.tol)
        run.status = worst <= 1.0 + g.limit_tol ? TRS_MW_CONVERGED : TRS_MW_INFEASIBLE;
    else if (mode == 1)
        run.status = TRS_MW_ITER_LIMIT;
    if (run.active()) {
        for (int m = tid; m < members; m += 256) {   // (the thread that owns member m wrote t.c2[m])
            g.prev[mbase + m] = Ab[m];
            Ab[m] = t.c2[m];
        }
    }
    if (tid == 0) {
        g.measure_out[b] = measure;
        if (it < g.H) {
            g.measure_history[(size_t)b * g.H + it] = measure;
            g.worst_history[(size_t)b * g.H + it] = worst;
        }
#pragma unroll
        for (int j = 0; j < JMAX; ++j) {
            if (j < J) {
                const size_t at = (size_t)b * J + j;
                g.displacement[at] = gval[j];
                g.ratio[at] = lcase[j] >= 0 ? gval[j] / ubar[j] : 0.0;
                g.multipliers[at] = dual.mu[j];
                g.mu[at] = dual.mu[j];
            }
        }
        run.finish(it, g.active);
    }
}

}  // namespace

extern "C" {

int trs_mw_abi_version(void) { return TRS_MW_ABI_VERSION; }

int trs_mw_fits(int nJ_max, int nM_max, int J) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535 || J < 1 || J > TRS_MW_MAX_LIMITS) return 0;
    return step_lds(nJ_max, nM_max, J) <= TRS_LDS_BYTES;
}

int trs_mw_step(int B, int L, int J, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                double* A, const double* rho, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                const int32_t* nM, const double* F, int ld_f, const int32_t* info, const int32_t* limit_case,
                const int32_t* limit_joint, const double* limit_dir, const double* limit_value, int measure, double move,
                double tol, double limit_tol, int sweeps, const double* a_min, double a_min_all, const double* a_max,
                double a_max_all, int it, int mode, double* prev, double* mu, int32_t* st, int32_t* active, double* areas,
                double* measure_out, double* measure_history, double* worst_history, int H, double* displacement,
                double* ratio, double* multipliers, double* sensitivity, void* stream) {
    if (B < 0 || L < 1 || J < 1 || J > TRS_MW_MAX_LIMITS || nJ_max <= 0 || nM_max < 0 || ld_f < 0 || it < 0 || mode < 0 ||
        mode > 1 || H < 0 || sweeps < 1 || (measure != TRS_MW_WEIGHT && measure != TRS_MW_VOLUME))
        return (int)hipErrorInvalidValue;
    if (!(move > 0.0) || !(move <= 1.0) || !(tol >= 0.0) || !(limit_tol >= 0.0)) return (int)hipErrorInvalidValue;
    const trs_iter::AreaBounds bounds = {a_min, a_max, a_min_all, a_max_all};
    if (!bounds.valid()) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !conn || !E || !A || !rho || !free_index || !F || !info || !limit_case || !limit_joint || !limit_dir ||
        !limit_value || !prev || !mu || !st || !active || !areas || !measure_out ||
        (H > 0 && (!measure_history || !worst_history)) || !displacement || !ratio || !multipliers)
        return (int)hipErrorInvalidValue;
    if (!trs_mw_fits(nJ_max, nM_max, J)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A, rho), free_index, n_free, nJ, nM,
                                  nullptr, ld_f);
    const StepArgs g = {F, info, limit_case, limit_joint, limit_dir, limit_value, move, tol, limit_tol, bounds, L, J, it,
                        mode, H, measure, sweeps, A, prev, mu, st, active, areas, measure_out, measure_history,
                        worst_history, displacement, ratio, multipliers, sensitivity};
    trs_lds::raise_lds_once<trs_mw_step_kernel>();
    hipLaunchKernelGGL(trs_mw_step_kernel, dim3(B), dim3(256), step_lds(nJ_max, nM_max, J), (hipStream_t)stream, bt, g);
    return (int)hipGetLastError();
}

}  // extern "C"
