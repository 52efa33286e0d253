// Minimum weight under displacement limits: the optimality-criteria method with one multiplier per limit, iterated on
// the device (include/trs_minweight.h; with stress limits include/trs_minweight_stress.h).  The assembly, the factorisation, the gather and the multi-case substitution of
// every iteration are trs_assemble, trs_potrf_batched, trs_gather_cases and trs_potrs_cases as they are - the virtual
// unit loads of the limits are just more columns of the case block; this file holds what turns the L + J reduced
// solutions into the next design:
//
//   trs_mw_step          one analysis: the limit values g_j, the sensitivities c_mj, the dual solve (per limit a
//                        geometric bisection on its multiplier, `sweeps` passes), the resizing, the convergence test and
//                        the outputs
//   trs_mw_step_stress   the same with stress limits: the stress-ratio area of every member as its lower bound
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
// With stress limits (trs_mw_step_stress; tests/minweight_stress_reference.py), all of the above and:
//     N_ml = ((E_m / L0_m) A_m) proj_m(u_l) for every REAL case l < L;  the required area in case l is N / allow_tension
//     for N > 0; for P = -N > 0 it is max(P / allow_compression, sqrt(P L0^2 / (pi^2 E kappa))), the second term only
//     when kappa > 0 (trs_sizing.h's words and its expression order)
//     req_m = the maximum over the cases in ascending l, on a tie the lowest l governs; governing_m = that l, or -1
//     where req_m = 0
//     the floor: lo_m = min(max(lo_m, req_m), hi_m) - a member that needs more than (1 + move) A_m grows at the move
//     limit, a member with w_m <= 0 keeps lo_m = hi_m;  the subproblem, the cut, the dual solve, the bisection, A'(mu)
//     and `change` are unchanged: only lo differs
//     utilisation_m = req_m / A_m;  stress_worst = its maximum over the live members (an extreme: exact in any order)
//     change <= tol: status 0 if max(worst, stress_worst) <= 1 + limit_tol, else 3
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
//
// The kernel is a template on `bool STRESS`: the instantiation without stress limits is compiled from the statements it
// had before the stress limits came (every addition stands under `if constexpr (STRESS)`), and it is the one trs_mw_step
// launches.  The other keeps three more words per member in LDS, formed ahead of the case loop - the running req_m, its
// case, the Euler coefficient L0^2 / (pi^2 E kappa) - and updates the running requirement as each real case passes
// through the stage: no further pass over the case block, no u and no N to HBM.
#include "../../include/trs_minweight.h"
#include "../../include/trs_minweight_stress.h"
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
    // with stress limits only:
    double* req;    // [nM_max]       the running required area
    double* eul;    // [nM_max]       L0^2 / (pi^2 E kappa), 0 without a member buckling term
    int* gov;       // [nM_max]       the case that set req (-1: none)
};

template <bool STRESS, class Arena>
__host__ __device__ inline StepTables step_layout(Arena& a, int nJ_max, int nM_max, int J) {
    StepTables t = {};
    t.u = a.template take<double>(6, nJ_max);
    t.red = a.template take<double>(RED);
    t.c0 = a.template take<double>(nM_max);
    t.c1 = a.template take<double>(nM_max);
    t.c2 = a.template take<double>(nM_max);
    t.ek = a.template take<double>(nM_max);
    t.w = a.template take<double>(nM_max);
    t.a = a.template take<double>(nM_max);
    t.c = a.template take<double>(J, nM_max);
    if constexpr (STRESS) {
        t.req = a.template take<double>(nM_max);
        t.eul = a.template take<double>(nM_max);
    }
    t.ends = a.template take<int2>(nM_max);
    t.row = a.template take<int>(3, nJ_max);
    if constexpr (STRESS) t.gov = a.template take<int>(nM_max);
    return t;
}

template <bool STRESS>
size_t step_lds(int nJ_max, int nM_max, int J) {
    return trs_lds::count([&](auto& a) { step_layout<STRESS>(a, nJ_max, nM_max, J); });
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
    // with stress limits only (behind the rest: the words above keep their places)
    double allow_tension, allow_compression, euler_kappa;
    const double* allow;      // [B][2] or null
    double* util;             // [B][nM_max]
    int* governing;           // [B][nM_max]
    double* stress_history;   // [B][H]
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

template <bool STRESS>
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
                if constexpr (STRESS) {
                    g.util[mbase + m] = 0.0;
                    g.governing[mbase + m] = -1;
                }
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
    const StepTables t = step_layout<STRESS>(lds, bt.nJ_max, nM_max, J);
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
        if constexpr (STRESS) {
            constexpr double PI = 3.14159265358979323846;
            t.req[m] = 0.0;
            t.gov[m] = -1;
            t.eul[m] = g.euler_kappa > 0.0 ? (geo.len * geo.len) / (((PI * PI) * E) * g.euler_kappa) : 0.0;
        }
    }
    double at = 0.0, ac = 0.0;   // (the allowables of this truss)
    if constexpr (STRESS) {
        at = g.allow != nullptr ? g.allow[2 * b] : g.allow_tension;
        ac = g.allow != nullptr ? g.allow[2 * b + 1] : g.allow_compression;
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
            if constexpr (STRESS) wanted = true;   // (every real case sets the members' requirement)
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
                    if constexpr (STRESS) {
                        const double N = (t.ek[m] * t.a[m]) * proj;
                        double r = 0.0;
                        if (N > 0.0) {
                            r = N / at;
                        } else if (N < 0.0) {
                            const double P = -N;
                            r = P / ac;
                            if (g.euler_kappa > 0.0) r = fmax(r, sqrt(P * t.eul[m]));
                        }
                        if (r > t.req[m]) {   // (strictly: on a tie the lowest l governs)
                            t.req[m] = r;
                            t.gov[m] = col;
                        }
                    }
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
    double stress_worst = 0.0;
    for (int m = tid; m < nM_max; m += 256) {
        double area = 0.0;
        [[maybe_unused]] double util = 0.0;
        [[maybe_unused]] int gov = -1;
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
            if constexpr (STRESS) {   // the floor: what the member's worst case demands, within the interval
                lo = fmin(fmax(lo, t.req[m]), hi);
                util = t.req[m] / area;
                gov = t.gov[m];
                stress_worst = fmax(stress_worst, util);
            }
            t.c0[m] = lo;
            t.c1[m] = hi;
        }
        g.areas[mbase + m] = area;
        if constexpr (STRESS) {
            g.util[mbase + m] = util;
            g.governing[mbase + m] = gov;
        }
        if (g.sens != nullptr) {
            for (int j = 0; j < J; ++j) g.sens[((size_t)b * J + j) * nM_max + m] = m < members ? t.c[j * nM_max + m] : 0.0;
        }
    }
    Reducer red = {t.red, 0, tid};
    const double measure = red.sum(msum);
    if constexpr (STRESS) stress_worst = red.max(stress_worst);
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
    double bound = worst;   // (what a converged truss must keep within 1 + limit_tol)
    if constexpr (STRESS) bound = fmax(worst, stress_worst);
    if (change <= g.tol)
        run.status = bound <= 1.0 + g.limit_tol ? TRS_MW_CONVERGED : TRS_MW_INFEASIBLE;
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
            if constexpr (STRESS) g.stress_history[(size_t)b * g.H + it] = stress_worst;
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

// What trs_mw_step_stress takes beyond trs_mw_step
struct StressIO {
    double allow_tension, allow_compression, euler_kappa;
    const double* allow;
    double* util;
    int* governing;
    double* stress_history;
};

// The argument rules and the launch that the two entry points share
template <bool STRESS>
int step(int B, int L, int J, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, double* A,
         const double* rho, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
         const double* F, int ld_f, const int32_t* info, const int32_t* limit_case, const int32_t* limit_joint,
         const double* limit_dir, const double* limit_value, int measure, double move, double tol, double limit_tol,
         int sweeps, const double* a_min, double a_min_all, const double* a_max, double a_max_all, int it, int mode,
         double* prev, double* mu, int32_t* st, int32_t* active, double* areas, double* measure_out, double* measure_history,
         double* worst_history, int H, double* displacement, double* ratio, double* multipliers, double* sensitivity,
         const StressIO s, void* stream) {
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
    if (step_lds<STRESS>(nJ_max, nM_max, J) > TRS_LDS_BYTES || nJ_max > 65535) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A, rho), free_index, n_free, nJ, nM,
                                  nullptr, ld_f);
    const StepArgs g = {F, info, limit_case, limit_joint, limit_dir, limit_value, move, tol, limit_tol, bounds, L, J, it,
                        mode, H, measure, sweeps, A, prev, mu, st, active, areas, measure_out, measure_history,
                        worst_history, displacement, ratio, multipliers, sensitivity, s.allow_tension,
                        s.allow_compression, s.euler_kappa, s.allow, s.util, s.governing, s.stress_history};
    trs_lds::raise_lds_once<trs_mw_step_kernel<STRESS>>();
    hipLaunchKernelGGL(trs_mw_step_kernel<STRESS>, dim3(B), dim3(256), step_lds<STRESS>(nJ_max, nM_max, J),
                       (hipStream_t)stream, bt, g);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_mw_abi_version(void) { return TRS_MW_ABI_VERSION; }

int trs_mws_abi_version(void) { return TRS_MWS_ABI_VERSION; }

int trs_mw_fits(int nJ_max, int nM_max, int J) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535 || J < 1 || J > TRS_MW_MAX_LIMITS) return 0;
    return step_lds<false>(nJ_max, nM_max, J) <= TRS_LDS_BYTES;
}

int trs_mw_fits_stress(int nJ_max, int nM_max, int J) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535 || J < 1 || J > TRS_MW_MAX_LIMITS) return 0;
    return step_lds<true>(nJ_max, nM_max, J) <= TRS_LDS_BYTES;
}

int trs_mw_step(int B, int L, int J, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                double* A, const double* rho, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                const int32_t* nM, const double* F, int ld_f, const int32_t* info, const int32_t* limit_case,
                const int32_t* limit_joint, const double* limit_dir, const double* limit_value, int measure, double move,
                double tol, double limit_tol, int sweeps, const double* a_min, double a_min_all, const double* a_max,
                double a_max_all, int it, int mode, double* prev, double* mu, int32_t* st, int32_t* active, double* areas,
                double* measure_out, double* measure_history, double* worst_history, int H, double* displacement,
                double* ratio, double* multipliers, double* sensitivity, void* stream) {
    return step<false>(B, L, J, nJ_max, nM_max, xyz, conn, E, A, rho, free_index, n_free, nJ, nM, F, ld_f, info, limit_case,
                       limit_joint, limit_dir, limit_value, measure, move, tol, limit_tol, sweeps, a_min, a_min_all, a_max,
                       a_max_all, it, mode, prev, mu, st, active, areas, measure_out, measure_history, worst_history, H,
                       displacement, ratio, multipliers, sensitivity, {}, stream);
}

int trs_mw_step_stress(int B, int L, int J, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E,
                       double* A, const double* rho, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                       const int32_t* nM, const double* F, int ld_f, const int32_t* info, const int32_t* limit_case,
                       const int32_t* limit_joint, const double* limit_dir, const double* limit_value, int measure,
                       double move, double tol, double limit_tol, int sweeps, const double* a_min, double a_min_all,
                       const double* a_max, double a_max_all, double allow_tension, double allow_compression,
                       const double* allow, double euler_kappa, int it, int mode, double* prev, double* mu, int32_t* st,
                       int32_t* active, double* areas, double* measure_out, double* measure_history, double* worst_history,
                       int H, double* displacement, double* ratio, double* multipliers, double* sensitivity,
                       double* utilisation, int32_t* governing, double* stress_history, void* stream) {
    if (!allow && (!(allow_tension > 0.0) || !(allow_compression > 0.0))) return (int)hipErrorInvalidValue;
    if (!(euler_kappa >= 0.0) || !(euler_kappa < INFINITY)) return (int)hipErrorInvalidValue;
    if (B > 0 && (!utilisation || !governing || (H > 0 && !stress_history))) return (int)hipErrorInvalidValue;
    const StressIO s = {allow_tension, allow_compression, euler_kappa, allow, utilisation, governing, stress_history};
    return step<true>(B, L, J, nJ_max, nM_max, xyz, conn, E, A, rho, free_index, n_free, nJ, nM, F, ld_f, info, limit_case,
                      limit_joint, limit_dir, limit_value, measure, move, tol, limit_tol, sweeps, a_min, a_min_all, a_max,
                      a_max_all, it, mode, prev, mu, st, active, areas, measure_out, measure_history, worst_history, H,
                      displacement, ratio, multipliers, sensitivity, s, stream);
}

}  // extern "C"
