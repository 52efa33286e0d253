// Compliance sizing: the stiffest design at a given weight, the optimality-criteria method iterated on the device
// (include/trs_compliance.h).  The assembly, the factorisation, the gather and the multi-case substitution of every
// iteration are trs_assemble, trs_potrf_batched, trs_gather_cases and trs_potrs_cases as they are; this file holds what
// turns the L reduced solutions into the next design:
//
//   trs_cm_step   one analysis: the compliance of every case, the objective, the sensitivities, the resizing at the
//                 target measure (a bisection on one multiplier), the convergence test and the truss's outputs
//
// The method, analysis k of design A (the header and tests/compliance_reference.py state it in the same words):
//     proj_ml = c_m.(u_l,j1 - u_l,j0);  C_l = sum_m (E_m A_m / L0_m) proj_ml^2;  J = sum_l alpha_l C_l, ascending l
//     s_m = sum_l alpha_l (E_m / L0_m) proj_ml^2, ascending l: -dJ/dA_m
//     lo_m = clamp((1 - move) A_m, a_min_m, a_max_m), hi_m = clamp((1 + move) A_m, a_min_m, a_max_m);
//     a member with w_m <= 0 keeps lo_m = hi_m = clamp(A_m, a_min_m, a_max_m)
//     p_m = A_m (s_m / w_m)^eta;  t_m(x) = min(max(p_m x, lo_m), hi_m);  V(x) = sum_m w_m t_m(x)
//     x0 = min, x1 = max over the members with p_m > 0 of lo_m / p_m and hi_m / p_m
//     sum w lo >= W: A' = lo;  sum w hi <= W: A' = hi;  no member has p_m > 0: A' = lo  (multiplier 0)
//     V(x1) <= W: A' = t(x1), multiplier x1^(-1/eta)
//     otherwise 64 times xm = sqrt(x0 x1); V(xm) <= W ? x0 = xm : x1 = xm;  A' = t(x0), multiplier x0^(-1/eta)
//     change = max_m |A'_m - A_m| / A_m;  change <= tol: converged; else k = max_iters: status 1; else A_{k+1} = A'
//
// trs_cm_step: one 256-thread work-group per truss.  A thread owns the members tid, tid + 256, ...: it forms their
// geometry once (c, E A / L0, E / L0, w), keeps it in LDS beside the running sensitivity, and is the only thread that
// ever touches those entries - the member tables need no barrier.  One case's displacement vector at a time is staged in
// LDS through row_of, in two buffers: the next case is staged behind the work on this one, one barrier per case; the
// wave partials of C_l go through two alternating slots behind that same barrier, and thread 0 folds them one case
// later.  Every sum runs per thread in ascending m, then by the wave butterfly, then over the four waves in order.  The
// bisection sums the 2^levels - 1 points of `levels` levels of its search tree together, one barrier per round (two
// alternating slot sets), and takes the decisions the definition takes: the same bits for 1, 2 or 3 levels.  Where a
// thread owns at most four members (nM_max <= 1024) it holds their p, lo, hi, w in registers through the bisection.  No
// floating-point atomic.
#include <type_traits>

#include "../../include/trs_compliance.h"
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_iterate.h"
#include "trs_lds.h"

namespace {

using Run = trs_iter::Run<TRS_CM_ACTIVE, TRS_CM_NOT_PD>;
using trs_iter::wave_max;
using trs_iter::wave_sum;

constexpr int RED = 64;          // doubles for the reductions: two sets of (7 points x 4 waves), rounded up

// LDS tables of the step kernel
struct StepTables {
    double* u;      // [2][3 nJ_max]  the displacements of two cases, joint layout, device numbering
    double* red;    // [RED]          the wave partials of the reductions
    double* c0;     // [nM_max] x 3   direction cosines; behind the case loop p, lo, hi
    double* c1;
    double* c2;
    double* k;      // [nM_max]       E A / L0; behind the case loop A'
    double* ek;     // [nM_max]       E / L0
    double* s;      // [nM_max]       the running sensitivity
    double* w;      // [nM_max]       rho L0 or L0
    int2* ends;     // [nM_max]       end joints, clamped
    int* row;       // [3 nJ_max]     row_of every DOF (-1: reads 0), formed once: a case's staging is one load deep
};

template <class Arena>
__host__ __device__ inline StepTables step_layout(Arena& a, int nJ_max, int nM_max) {
    StepTables t;
    t.u = a.template take<double>(6, nJ_max);
    t.red = a.template take<double>(RED);
    t.c0 = a.template take<double>(nM_max);
    t.c1 = a.template take<double>(nM_max);
    t.c2 = a.template take<double>(nM_max);
    t.k = a.template take<double>(nM_max);
    t.ek = a.template take<double>(nM_max);
    t.s = a.template take<double>(nM_max);
    t.w = a.template take<double>(nM_max);
    t.ends = a.template take<int2>(nM_max);
    t.row = a.template take<int>(3, nJ_max);
    return t;
}

size_t step_lds(int nJ_max, int nM_max) { return trs_lds::count([&](auto& a) { step_layout(a, nJ_max, nM_max); }); }

// K sums and two maxima of a 256-thread work-group behind one pair of barriers: slot [4 (K + 2)]
template <int K>
__device__ __forceinline__ void block_reduce(double (&sum)[K], double (&top)[2], double* slot, const int tid) {
#pragma unroll
    for (int i = 0; i < K; ++i) sum[i] = wave_sum(sum[i]);
    top[0] = wave_max(top[0]);
    top[1] = wave_max(top[1]);
    __syncthreads();   // (the previous readers of slot are done)
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < K; ++i) slot[4 * i + (tid >> 6)] = sum[i];
        slot[4 * K + (tid >> 6)] = top[0];
        slot[4 * K + 4 + (tid >> 6)] = top[1];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < K; ++i) sum[i] = ((slot[4 * i] + slot[4 * i + 1]) + slot[4 * i + 2]) + slot[4 * i + 3];
    top[0] = fmax(fmax(slot[4 * K], slot[4 * K + 1]), fmax(slot[4 * K + 2], slot[4 * K + 3]));
    top[1] = fmax(fmax(slot[4 * K + 4], slot[4 * K + 5]), fmax(slot[4 * K + 6], slot[4 * K + 7]));
}

struct StepArgs {
    const double* F;          // [B][L][ld_f]
    const int* info;          // [B]
    const double* alpha;      // [L]
    double* target;           // [B]
    double eta, move, tol;
    trs_iter::AreaBounds bounds;
    int L, it, mode, H, measure;
    double* A;                // [B][nM_max]
    double* prev;             // [B][nM_max]
    int* st;                  // [B][4]
    int* active;
    double* areas;            // [B][nM_max]
    double* measure_out;      // [B]
    double* compliance;       // [B][L]
    double* objective;        // [B]
    double* history;          // [B][H]
    double* sens;             // [B][nM_max]
    double* multiplier;       // [B]
};

constexpr int HELD_MEMBERS = 4;   // members per thread that the bisection keeps in registers
// levels = 0, the measured choice (bar-942 x 4096, 8 cases): one level per round where the members are held in registers
// (0.617 ms against 0.638 with two levels and 0.765 with three), two where they stay in LDS (0.695 against 0.760 / 0.802)
inline int default_levels(int nM_max) { return nM_max <= 256 * HELD_MEMBERS ? 1 : 2; }
struct Held {
    double p[HELD_MEMBERS], lo[HELD_MEMBERS], hi[HELD_MEMBERS], w[HELD_MEMBERS];
};

// `rounds` rounds of LV levels each of the bisection on [x0, x1]: the points of the search tree in heap order (1 the
// root sqrt(x0 x1), 2 i the point below it, 2 i + 1 the point above), V at all of them summed together, then the walk
// down the tree: exactly the LV decisions that LV rounds of one level take, on the same operands.  One barrier per round:
// round r writes the slot set r & 1, whose readers of round r - 2 passed the barrier of round r - 1.
// HELD: the work-group's trusses have at most 4 x 256 members and the thread's p, lo, hi, w are in registers (`own`; a
// place without a member holds zeros and adds fma(0, 0, sum) = sum: the bits of the loop over LDS).
template <int LV, bool HELD>
__device__ __forceinline__ void bisect(double& x0, double& x1, const int rounds, const int first, const double W,
                                       const StepTables& t, const Held& own, const int members, const int tid) {
    constexpr int P = (1 << LV) - 1;
    for (int r = 0; r < rounds; ++r) {
        double pt[P + 1], below[P + 1], above[P + 1], v[P + 1];
        below[1] = x0;
        above[1] = x1;
#pragma unroll
        for (int i = 1; i <= P; ++i) {
            pt[i] = sqrt(below[i] * above[i]);
            v[i] = 0.0;
            if (2 * i + 1 <= P) {
                below[2 * i] = below[i];
                above[2 * i] = pt[i];
                below[2 * i + 1] = pt[i];
                above[2 * i + 1] = above[i];
            }
        }
        if constexpr (HELD) {
#pragma unroll
            for (int k = 0; k < HELD_MEMBERS; ++k) {
#pragma unroll
                for (int i = 1; i <= P; ++i)
                    v[i] = fma(own.w[k], fmin(fmax(own.p[k] * pt[i], own.lo[k]), own.hi[k]), v[i]);
            }
        } else {
            for (int m = tid; m < members; m += 256) {
                const double p = t.c0[m], lo = t.c1[m], hi = t.c2[m], w = t.w[m];
#pragma unroll
                for (int i = 1; i <= P; ++i) v[i] = fma(w, fmin(fmax(p * pt[i], lo), hi), v[i]);
            }
        }
        double* slot = t.red + ((first + r) & 1) * (RED / 2);
        // (the butterflies of the P sums step by step side by side: P exchanges are in flight at once, and each sum
        // takes the additions of wave_sum in wave_sum's order)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            double other[P + 1];
#pragma unroll
            for (int i = 1; i <= P; ++i) other[i] = __shfl_xor(v[i], off);
#pragma unroll
            for (int i = 1; i <= P; ++i) v[i] += other[i];
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int i = 1; i <= P; ++i) slot[4 * (i - 1) + (tid >> 6)] = v[i];
        }
        __syncthreads();
        int i = 1;
#pragma unroll
        for (int lev = 0; lev < LV; ++lev) {
            const double* q = slot + 4 * (i - 1);
            const double V = ((q[0] + q[1]) + q[2]) + q[3];
            // (pt[i] through a select chain: i is known only at run time, and the points live in registers)
            double x = pt[1];
#pragma unroll
            for (int j = 2; j <= P; ++j) x = i == j ? pt[j] : x;
            if (V <= W) {
                x0 = x;
                i = 2 * i + 1;
            } else {
                x1 = x;
                i = 2 * i;
            }
        }
    }
}

__global__ __launch_bounds__(256) void trs_cm_step_kernel(const TrsBatch bt, const StepArgs g, const int levels) {
    extern __shared__ double sh[];   // (no static LDS beside it: the dynamic ceiling is the whole of a CU's)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nM_max = bt.nM_max, ld_f = bt.ld_f;
    const int mode = g.mode, it = g.it, L = g.L;
    Run run(g.st + 4 * b, it == 0);   // (no report mode here: nothing follows the last resizing)
    if (!run.active()) return;        // (uniform over the work-group) frozen: nothing is touched
    double W = g.target[b];           // (read by every thread here; thread 0 writes it behind the barriers below)
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
                g.sens[mbase + m] = 0.0;
            } else if (m < members) {
                Ab[m] = g.prev[mbase + m];
            }
        }
        if (it == 0)
            for (int l = tid; l < L; l += 256) g.compliance[(size_t)b * L + l] = 0.0;
        run.fail(pivot, run.one_back(), tid);
        if (tid == 0 && it == 0) {
            g.measure_out[b] = 0.0;
            g.objective[b] = 0.0;
            g.multiplier[b] = 0.0;
        }
        return;
    }
    trs_lds::Carve lds(sh);
    const StepTables t = step_layout(lds, bt.nJ_max, nM_max);
    const trs_iter::CaseStage cases = {t.u, t.row, g.F + (size_t)b * L * ld_f, ndof_max, ld_f};
    cases.form_rows(tr, tid);
    cases.stage(0, tid);
    // ---- the member geometry, once; the measure of the design ----
    const bool by_weight = g.measure == TRS_CM_WEIGHT;
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
        t.k[m] = E * A / geo.len;
        t.ek[m] = E / geo.len;
        t.s[m] = 0.0;
        t.w[m] = w;
        msum += w * A;
    }
    __syncthreads();   // (case 0 is staged)
    // ---- the cases: the compliance of each, the objective, the sensitivities ----
    double J = 0.0;   // (thread 0's)
    auto fold = [&](int l) {   // thread 0: C_l from the wave partials that case l left in slot set l & 1
        const double* q = t.red + (l & 1) * 4;
        const double C = ((q[0] + q[1]) + q[2]) + q[3];
        g.compliance[(size_t)b * L + l] = C;
        J += g.alpha[l] * C;
    };
    for (int l = 0; l < L; ++l) {
        const double* u = cases.buffer(l);
        const double al = g.alpha[l];
        double csum = 0.0;
        for (int m = tid; m < members; m += 256) {
            const int2 c = t.ends[m];
            const double* u0 = u + 3 * c.x;
            const double* u1 = u + 3 * c.y;
            double proj = t.c0[m] * (u1[0] - u0[0]);
            proj += t.c1[m] * (u1[1] - u0[1]);
            proj += t.c2[m] * (u1[2] - u0[2]);
            const double pp = proj * proj;
            csum += t.k[m] * pp;
            t.s[m] += al * (t.ek[m] * pp);
        }
        csum = wave_sum(csum);
        // (slot set l & 1: thread 0 read it for case l - 2 before the barrier of case l - 1)
        if ((tid & 63) == 0) t.red[(l & 1) * 4 + (tid >> 6)] = csum;
        if (tid == 0 && l > 0) fold(l - 1);
        if (l + 1 < L) cases.stage(l + 1, tid);   // (the other buffer: its readers passed the barrier of case l - 1)
        __syncthreads();
    }
    if (tid == 0) fold(L - 1);
    // ---- the outputs of this design; p, lo, hi of the resizing (over c0, c1, c2: the case loop is behind) ----
    const double move = g.move, eta = g.eta;
    double sums[3] = {msum, 0.0, 0.0};                  // the measure, sum w lo, sum w hi
    double tops[2] = {-INFINITY, -INFINITY};            // -x0, x1
    for (int m = tid; m < nM_max; m += 256) {
        double area = 0.0, s = 0.0;
        if (m < members) {
            area = Ab[m];
            s = t.s[m];
            const double w = t.w[m];
            const double a_lo = g.bounds.lo(mbase + m), a_hi = g.bounds.hi(mbase + m);
            double lo, hi, p = 0.0;
            if (w > 0.0) {
                lo = fmin(fmax((1.0 - move) * area, a_lo), a_hi);
                hi = fmin(fmax((1.0 + move) * area, a_lo), a_hi);
                p = area * pow(s / w, eta);
            } else {
                lo = hi = fmin(fmax(area, a_lo), a_hi);
            }
            t.c0[m] = p;
            t.c1[m] = lo;
            t.c2[m] = hi;
            sums[1] += w * lo;
            sums[2] += w * hi;
            if (p > 0.0) {
                tops[0] = fmax(tops[0], -(lo / p));
                tops[1] = fmax(tops[1], hi / p);
            }
        }
        g.areas[mbase + m] = area;
        g.sens[mbase + m] = s;
    }
    block_reduce<3>(sums, tops, t.red + 8, tid);   // (behind the case slots, which thread 0 may still be folding)
    const double measure = sums[0];
    if (it == 0 && !(W > 0.0)) W = measure;
    double x0 = -tops[0], x1 = tops[1], mult = 0.0, x = 0.0;
    int pick = 0;   // 0: lo, 1: hi, 2: t(x)
    if (sums[1] >= W) {
        pick = 0;
    } else if (sums[2] <= W) {
        pick = 1;
    } else if (!(x1 > 0.0)) {   // (no member has p > 0: x1 is still -inf)
        pick = 0;
    } else {
        double v1[1] = {0.0}, none[2] = {0.0, 0.0};
        for (int m = tid; m < members; m += 256) v1[0] = fma(t.w[m], fmin(fmax(t.c0[m] * x1, t.c1[m]), t.c2[m]), v1[0]);
        block_reduce<1>(v1, none, t.red + 32, tid);
        pick = 2;
        if (v1[0] <= W) {
            x = x1;
        } else {
            __syncthreads();   // (every thread has read the slots of the reductions above: the rounds write them again)
            Held own;
#pragma unroll
            for (int k = 0; k < HELD_MEMBERS; ++k) {
                const int m = tid + 256 * k;
                const bool live = m < members;
                own.p[k] = live ? t.c0[m] : 0.0;
                own.lo[k] = live ? t.c1[m] : 0.0;
                own.hi[k] = live ? t.c2[m] : 0.0;
                own.w[k] = live ? t.w[m] : 0.0;
            }
            auto search = [&](auto held) {
                constexpr bool HELD = decltype(held)::value;
                if (levels == 3) {
                    constexpr int deep = TRS_CM_BISECTIONS / 3;
                    bisect<3, HELD>(x0, x1, deep, 0, W, t, own, members, tid);
                    bisect<1, HELD>(x0, x1, TRS_CM_BISECTIONS % 3, deep, W, t, own, members, tid);
                } else if (levels == 2) {
                    bisect<2, HELD>(x0, x1, TRS_CM_BISECTIONS / 2, 0, W, t, own, members, tid);
                } else {
                    bisect<1, HELD>(x0, x1, TRS_CM_BISECTIONS, 0, W, t, own, members, tid);
                }
            };
            if (nM_max <= 256 * HELD_MEMBERS)   // (uniform over the launch)
                search(std::true_type{});
            else
                search(std::false_type{});
            x = x0;
        }
        mult = pow(x, -1.0 / eta);
    }
    // ---- the next design, the convergence test ----
    double change = 0.0;
    for (int m = tid; m < members; m += 256) {   // (the thread that owns member m wrote its p, lo, hi)
        const double area = Ab[m], lo = t.c1[m], hi = t.c2[m];
        const double next = pick == 0 ? lo : pick == 1 ? hi : fmin(fmax(t.c0[m] * x, lo), hi);
        change = fmax(change, fabs(next - area) / area);
        t.k[m] = next;
    }
    {
        double none[1] = {0.0}, top[2] = {change, 0.0};
        block_reduce<1>(none, top, t.red + 8, tid);   // (the rounds' last readers passed the barrier inside)
        change = top[0];
    }
    if (change <= g.tol)
        run.status = TRS_CM_CONVERGED;
    else if (mode == 1)
        run.status = TRS_CM_ITER_LIMIT;
    if (run.active()) {
        for (int m = tid; m < members; m += 256) {   // (the thread that owns member m wrote t.k[m])
            g.prev[mbase + m] = Ab[m];
            Ab[m] = t.k[m];
        }
    }
    if (tid == 0) {
        g.measure_out[b] = measure;
        g.objective[b] = J;
        g.multiplier[b] = mult;
        if (it == 0) g.target[b] = W;
        if (it < g.H) g.history[(size_t)b * g.H + it] = J;
        run.finish(it, g.active);
    }
}

}  // namespace

extern "C" {

int trs_cm_abi_version(void) { return TRS_CM_ABI_VERSION; }

int trs_cm_fits(int nJ_max, int nM_max) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535) return 0;
    return step_lds(nJ_max, nM_max) <= TRS_LDS_BYTES;
}

int trs_cm_step(int B, int L, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, double* A,
                const double* rho, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
                const double* F, int ld_f, const int32_t* info, const double* alpha, int measure, double* target,
                double eta, double move, double tol, const double* a_min, double a_min_all, const double* a_max,
                double a_max_all, int it, int mode, int levels, double* prev, int32_t* st, int32_t* active, double* areas,
                double* measure_out, double* compliance, double* objective, double* objective_history, int H,
                double* sensitivity, double* multiplier, void* stream) {
    if (B < 0 || L < 1 || nJ_max <= 0 || nM_max < 0 || ld_f < 0 || it < 0 || mode < 0 || mode > 1 || H < 0 ||
        levels < 0 || levels > 3 || (measure != TRS_CM_WEIGHT && measure != TRS_CM_VOLUME))
        return (int)hipErrorInvalidValue;
    if (!(eta > 0.0) || !(eta <= 1.0) || !(move > 0.0) || !(move <= 1.0) || !(tol >= 0.0)) return (int)hipErrorInvalidValue;
    const trs_iter::AreaBounds bounds = {a_min, a_max, a_min_all, a_max_all};
    if (!bounds.valid()) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !conn || !E || !A || !rho || !free_index || !F || !info || !alpha || !target || !prev || !st || !active ||
        !areas || !measure_out || !compliance || !objective || (H > 0 && !objective_history) || !sensitivity || !multiplier)
        return (int)hipErrorInvalidValue;
    if (!trs_cm_fits(nJ_max, nM_max)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A, rho), free_index, n_free, nJ, nM,
                                  nullptr, ld_f);
    const StepArgs g = {F, info, alpha, target, eta, move, tol, bounds, L, it, mode, H,
                        measure, A, prev, st, active, areas, measure_out, compliance, objective, objective_history,
                        sensitivity, multiplier};
    trs_lds::raise_lds_once<trs_cm_step_kernel>();
    hipLaunchKernelGGL(trs_cm_step_kernel, dim3(B), dim3(256), step_lds(nJ_max, nM_max), (hipStream_t)stream, bt, g,
                       levels == 0 ? default_levels(nM_max) : levels);
    return (int)hipGetLastError();
}

}  // extern "C"
