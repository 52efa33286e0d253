// Collapse load: elastic-plastic members, the event-to-event analysis on the device (include/trs_plastic.h).  The
// assembly, the factorisation, the gather and the substitution of every analysis are trs_assemble, trs_potrf_batched,
// trs_gather_cases and trs_potrs_cases as they are, given the effective areas; this file holds what turns the reduced
// solution into the next state, and the report:
//
//   trs_pl_step     one analysis: the softening test, the increments of every member, the release test, the step to the
//                   next yield or to a cap, the accumulated forces, displacements and load factor, the next state and
//                   the next effective areas, the history
//   trs_pl_finish   u and f_ext in the caller's joint layout from the accumulated state
//
// The method, analysis k of state s_k (the header and tests/plastic_reference.py state it in the same words):
//     1. A_eff,m = A_m where s_m = 0, else h A_m; assemble and factor K(A_eff)
//     2. info != 0: status 2 (mechanism); nothing advances, the info is latched
//     3. otherwise solve K du = P
//     4. the softening test: r_k = max over DOFs of |du|; analysis 0 stores r_0; if NOT (r_k <= collapse_ratio r_0):
//        status 2 (mechanism) with info left 0; a non-finite r_k counts as collapse
//     5. de_m = c_m.(du_j1 - du_j0) and dN_m = (E_m A_eff,m / L0_m) de_m, for every member
//     6. the release test: a yielded member with s_m de_m < 0 unloads (strict, no threshold); if any member unloads:
//        at k = max_events status 1; otherwise those members return to s = 0, nothing advances, and the analysis counts
//        as an event: its member_history entry is -1 and its count the number released
//     7. otherwise advance: for every elastic member dl_m = (cap_tension_m - N_m) / dN_m where dN_m > 0,
//        (-cap_compression_m - N_m) / dN_m where dN_m < 0, +inf where dN_m = 0, negative values clamped to 0;
//        dl_y = the minimum of the dl_m, the governing member the lowest index that attains it;
//        dl_L = lambda_max - lambda; dl_u = min over free DOFs with du != 0 of (disp_limit - sign(du) u) / |du|, clamped
//        at 0, +inf with disp_limit = 0;
//        if min(dl_L, dl_u) <= dl_y: advance lambda, N and u by that step; status 0 where dl_L <= dl_u, else status 3;
//        otherwise, at k = max_events: status 1 without advancing;
//        otherwise advance by dl_y; every elastic member with dl_m <= dl_y (1 + tie_tol) yields with s_m = sign(dN_m) and
//        takes N_m = +cap_tension_m or -cap_compression_m exactly, unless it lay beyond that capacity already;
//        `events` = k + 1
//     8. the history: analysis k writes entry k of lambda_history, member_history, count_history and umax_history
//
// One 256-thread work-group per truss.  du is staged into LDS through rows(j), one test per joint; thread tid owns the
// members tid, tid + 256, ...: it is the only thread that touches their dl_m and dN_m in LDS, so those tables need no
// barrier.  The member loops run the same number of trips in every lane, so that the releases and the yields of a trip
// are counted by the wave's ballot.  Every reduction is exact in any order - maxima, the lexicographic minimum of
// (dl_m, m), integer counts -: within the wave first, then the four waves through LDS.  No floating-point sum across
// threads and no floating-point atomic anywhere.
#include "../../include/trs_plastic.h"
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_iterate.h"
#include "trs_lds.h"

#include <cfloat>
#include <climits>
#include <cmath>

namespace {

using Run = trs_iter::Run<TRS_PL_ACTIVE, TRS_PL_MECHANISM>;

// LDS tables of the step kernel
struct StepTables {
    double* du;     // [3 nJ_max]  the displacement increments per unit load factor, joint layout, device numbering
    double* dlam;   // [nM_max]    dl_m of an elastic member; of a yielded one -1 where it unloads, else +inf
    double* dN;     // [nM_max]
    double* red;    // [16]        the waves' r_k, dl_u, dl_y and largest |u_d|
    int* redi;      // [12]        the waves' governing members, releases and yields
};

template <class Arena>
__host__ __device__ inline StepTables step_layout(Arena& a, int nJ_max, int nM_max) {
    StepTables t;
    t.du = a.template take<double>(3, nJ_max);
    t.dlam = a.template take<double>(nM_max);
    t.dN = a.template take<double>(nM_max);
    t.red = a.template take<double>(16);
    t.redi = a.template take<int>(12);
    return t;
}

size_t step_lds(int nJ_max, int nM_max) { return trs_lds::count([&](auto& a) { step_layout(a, nJ_max, nM_max); }); }

// LDS tables of the report: the member-end lists of the joints with a held DOF
template <class Arena>
__host__ __device__ inline trs_rec::EndLists finish_layout(Arena& a, int nJ_max, int nM_max) {
    trs_rec::EndLists t;
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    return t;
}

size_t finish_lds(int nJ_max, int nM_max) { return trs_lds::count([&](auto& a) { finish_layout(a, nJ_max, nM_max); }); }

struct StepArgs {
    const double* F;       // [B][1][ld_f]
    const int* info;       // [B]
    const double* cap_t;   // [B][nM_max]
    const double* cap_c;   // [B][nM_max]
    const double* A_nom;   // [B][nM_max]
    double hardening, lambda_max, disp_limit, collapse_ratio, tie_tol;
    int it, mode, H;
    double* A;             // [B][nM_max]
    signed char* state;    // [B][nM_max]
    double* N;             // [B][nM_max]
    double* U;             // [B][3 nJ_max]
    double* acc;           // [B][4]
    int* st;               // [B][4]
    int* active;
    double* lambda_history;   // [B][H]
    int* member_history;
    int* count_history;
    double* umax_history;
};

// what an analysis does to its truss
enum { TERMINAL = 0, RELEASE = 1, ADVANCE_CAP = 2, ADVANCE_YIELD = 3 };

__global__ __launch_bounds__(256) void trs_pl_step_kernel(const TrsBatch bt, const StepArgs g) {
    extern __shared__ double sh[];   // (no static LDS beside it: the dynamic ceiling is the whole of a CU's)
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mode = g.mode, it = g.it;
    // (every thread reads the accumulated state here; thread 0 writes it behind the barriers below)
    double lam = g.acc[4 * b], r0 = g.acc[4 * b + 1], umax = g.acc[4 * b + 2];
    const int pivot = g.info[b];
    const bool begin = it == 0;
    Run run(g.st + 4 * b, begin);   // (the count: events)
    if (begin) lam = r0 = umax = 0.0;   // this analysis's own: the accumulated state begins with the run
    if (!run.active()) return;   // (uniform over the work-group) frozen: nothing is touched
    const size_t hist = (size_t)b * g.H + it;
    if (pivot != 0) {   // 2. status 2: nothing advances - the events stay, no roll-back -, the info is latched
        run.fail(pivot, run.count, tid);
        if (tid == 0 && it < g.H) {
            g.lambda_history[hist] = lam;
            g.member_history[hist] = -2;
            g.count_history[hist] = 0;
            g.umax_history[hist] = umax;
        }
        return;
    }
    const TrussView tr = bt.truss(b);
    const int members = tr.members, ndof_max = tr.ndof_max;
    const size_t mbase = tr.mbase;
    double* Ab = g.A + mbase;
    const double* An = g.A_nom + mbase;
    const double* ct = g.cap_t + mbase;
    const double* cc = g.cap_c + mbase;
    signed char* state = g.state + mbase;
    double* Nb = g.N + mbase;
    double* Ub = g.U + (size_t)b * ndof_max;
    trs_lds::Carve lds(sh);
    const StepTables t = step_layout(lds, bt.nJ_max, bt.nM_max);
    const double* f = g.F + (size_t)b * bt.ld_f;
    const double limit = g.disp_limit;
    // ---- 3./4. du into LDS (held DOFs and the padding read 0), r_k and dl_u on the way ----
    double rk = 0.0, dlu = INFINITY;
    for (int j = tid; j < bt.nJ_max; j += 256) {
        const TrussView::Rows q = tr.rows(j);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double v = q.r[a] >= 0 ? f[q.r[a]] : 0.0;
            t.du[3 * j + a] = v;
            double mag = fabs(v);
            if (!(mag <= DBL_MAX)) mag = INFINITY;   // (a NaN would be lost in fmax)
            rk = fmax(rk, mag);
            if (limit > 0.0 && q.r[a] >= 0 && v != 0.0) {
                const double u = begin ? 0.0 : Ub[3 * j + a];
                dlu = fmin(dlu, fmax((limit - (v > 0.0 ? u : -u)) / mag, 0.0));
            }
        }
    }
    __syncthreads();
    // ---- 5./6./7. de_m, dN_m, the release test, dl_m; every lane runs every trip (the ballot counts a wave's trip) ----
    double dly = INFINITY;
    int gov = INT_MAX, nrel = 0;   // nrel: of this wave
    for (int m0 = 0; m0 < members; m0 += 256) {
        const int m = m0 + tid;
        bool rel = false;
        if (m < members) {
            const int2 c = tr.ends(m).c;
            const trs_rec::MemberGeom geo = trs_rec::member_geom(tr.X, c.x, c.y);
            const double* u0 = t.du + 3 * c.x;
            const double* u1 = t.du + 3 * c.y;
            double de = geo.c[0] * (u1[0] - u0[0]);
            de += geo.c[1] * (u1[1] - u0[1]);
            de += geo.c[2] * (u1[2] - u0[2]);
            const double dN = (tr.mem.E[mbase + m] * Ab[m] / geo.len) * de;
            const int s = begin ? 0 : state[m];
            double dl = INFINITY;
            if (s != 0) {
                rel = (double)s * de < 0.0;   // (strictly: de = 0 stays yielded)
                if (rel) dl = -1.0;
            } else {
                if (dN > 0.0)
                    dl = fmax((ct[m] - Nb[m]) / dN, 0.0);
                else if (dN < 0.0)
                    dl = fmax((-cc[m] - Nb[m]) / dN, 0.0);
                if (dl < dly) {   // (strictly: ascending m, so the lowest index keeps a tie)
                    dly = dl;
                    gov = m;
                }
            }
            t.dlam[m] = dl;
            t.dN[m] = dN;
        }
        nrel += __popcll(__ballot(rel));
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        rk = fmax(rk, __shfl_xor(rk, off));
        dlu = fmin(dlu, __shfl_xor(dlu, off));
        const double ov = __shfl_xor(dly, off);
        const int oi = __shfl_xor(gov, off);
        if (ov < dly || (ov == dly && oi < gov)) {
            dly = ov;
            gov = oi;
        }
    }
    if (lane == 0) {
        t.red[wave] = rk;
        t.red[4 + wave] = dlu;
        t.red[8 + wave] = dly;
        t.redi[wave] = gov;
        t.redi[4 + wave] = nrel;
    }
    __syncthreads();
    rk = fmax(fmax(t.red[0], t.red[1]), fmax(t.red[2], t.red[3]));
    dlu = fmin(fmin(t.red[4], t.red[5]), fmin(t.red[6], t.red[7]));
    dly = t.red[8];
    gov = t.redi[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const double ov = t.red[8 + w];
        const int oi = t.redi[w];
        if (ov < dly || (ov == dly && oi < gov)) {
            dly = ov;
            gov = oi;
        }
    }
    nrel = (t.redi[4] + t.redi[5]) + (t.redi[6] + t.redi[7]);
    // ---- the decision (uniform over the work-group) ----
    if (begin) r0 = rk;
    int what = TERMINAL;
    double step = 0.0;
    if (!(rk <= g.collapse_ratio * r0) || !(rk <= DBL_MAX)) {
        run.status = TRS_PL_MECHANISM;   // 4. (info stays 0)
    } else if (nrel > 0) {
        if (mode == 1)
            run.status = TRS_PL_EVENT_LIMIT;
        else
            what = RELEASE;
    } else {
        const double dlL = g.lambda_max - lam;
        const double cap = fmin(dlL, dlu);
        if (cap <= dly) {
            what = ADVANCE_CAP;
            step = cap;
            run.status = dlL <= dlu ? TRS_PL_LAMBDA_MAX : TRS_PL_DISP_LIMIT;
        } else if (mode == 1) {
            run.status = TRS_PL_EVENT_LIMIT;
        } else {
            what = ADVANCE_YIELD;
            step = dly;
        }
    }
    // ---- the second pass: N, u, s, A_eff in place ----
    int count = 0;
    if (what == RELEASE) {
        for (int m = tid; m < members; m += 256) {   // (the thread that owns member m wrote t.dlam[m])
            if (state[m] != 0 && t.dlam[m] < 0.0) {
                state[m] = 0;
                Ab[m] = An[m];
            }
        }
        count = nrel;
    } else if (what != TERMINAL) {
        const double reach = dly * (1.0 + g.tie_tol);
        const double h = g.hardening;
        int nyield = 0;   // of this wave
        for (int m0 = 0; m0 < members; m0 += 256) {
            const int m = m0 + tid;
            bool yields = false;
            if (m < members) {
                const double dN = t.dN[m];
                const double before = begin ? 0.0 : Nb[m];
                double Nn = before + step * dN;
                const int s = begin ? 0 : state[m];
                yields = what == ADVANCE_YIELD && s == 0 && t.dlam[m] <= reach;
                if (yields) {
                    const bool tension = dN > 0.0;
                    // (beyond its capacity already - dl_m was clamped -: it keeps its force)
                    if (!(tension ? before > ct[m] : before < -cc[m])) Nn = tension ? ct[m] : -cc[m];
                    state[m] = tension ? 1 : -1;
                    Ab[m] = h * An[m];
                }
                Nb[m] = Nn;
            }
            nyield += __popcll(__ballot(yields));
        }
        double top = 0.0;
        for (int d = tid; d < ndof_max; d += 256) {
            const double un = (begin ? 0.0 : Ub[d]) + step * t.du[d];
            Ub[d] = un;
            top = fmax(top, fabs(un));
        }
        top = trs_iter::wave_max(top);
        if (lane == 0) {
            t.red[12 + wave] = top;
            t.redi[8 + wave] = nyield;
        }
        __syncthreads();
        umax = fmax(fmax(t.red[12], t.red[13]), fmax(t.red[14], t.red[15]));
        count = (t.redi[8] + t.redi[9]) + (t.redi[10] + t.redi[11]);
        lam += step;
    }
    if (tid == 0) {
        const bool still = run.active();
        g.acc[4 * b] = lam;
        g.acc[4 * b + 1] = r0;
        g.acc[4 * b + 2] = umax;
        if (it < g.H) {
            g.lambda_history[hist] = lam;
            g.member_history[hist] = what == ADVANCE_YIELD ? gov : what == RELEASE ? -1 : -2;
            g.count_history[hist] = still ? count : 0;
            g.umax_history[hist] = umax;
        }
        run.finish(it, g.active);
    }
}

struct FinishArgs {
    const double* loads;   // [B][nJ_max][3]  the caller's numbering
    const double* N;       // [B][nM_max]
    const double* U;       // [B][3 nJ_max]
    const double* acc;     // [B][4]
    double* u;             // [B][nJ_max][3]
    double* f_ext;         // [B][nJ_max][3]
};

// u and f_ext of the accumulated state: lambda P at the free DOFs, the members' end forces at the held ones, summed per
// joint in ascending member index (the lists come sorted by member id)
__global__ __launch_bounds__(256) void trs_pl_finish_kernel(const TrsBatch bt, const FinishArgs g) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int ndof_max = v.ndof_max;
    trs_lds::Carve lds(sh);
    const trs_rec::EndLists t = finish_layout(lds, bt.nJ_max, bt.nM_max);
    build_end_lists(t, v, tid, [&](int j) { return v.any_held(j); });
    const double lam = g.acc[4 * b];
    const double* P = g.loads + (size_t)b * ndof_max;
    const double* Ub = g.U + (size_t)b * ndof_max;
    const double* Nb = g.N + v.mbase;
    double* uo = g.u + (size_t)b * ndof_max;
    double* fo = g.f_ext + (size_t)b * ndof_max;
    for (int d = tid; d < ndof_max; d += 256) {
        const int r = v.row_of(d);
        const int o = v.place_dof(d);
        uo[o] = r >= 0 ? Ub[d] : 0.0;
        if (r >= 0)
            fo[o] = lam * P[o];   // free DOF: the applied load
        else if (d >= v.ndof)
            fo[o] = 0.0;          // padding
    }
    // (thread j % 256 sorted joint j's list and is the one that reads it: no barrier behind the builder)
    for (int j = tid; j < v.joints; j += 256) {
        const TrussView::Rows rows = v.rows(j);
        if (!rows.any_held()) continue;
        const int* list = t.ends + t.start[j];
        const int deg = t.cnt[j];
        double r[3] = {0.0, 0.0, 0.0};   // (a constrained joint without members: zero reaction)
        for (int i = 0; i < deg; ++i) {
            const int m = list[i] >> 1, end = list[i] & 1;
            const int2 c = v.ends(m).c;
            const trs_rec::MemberGeom geo = trs_rec::member_geom(v.X, c.x, c.y);
            trs_rec::add_end_force(r, geo.c, Nb[m], end);
        }
        const int o = 3 * v.place(j);
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (rows.held(a)) fo[o + a] = r[a];
    }
}

bool finite_at_least(double x, double least) { return x >= least && x <= 1.7e308; }

}  // namespace

extern "C" {

int trs_pl_abi_version(void) { return TRS_PL_ABI_VERSION; }

int trs_pl_fits(int nJ_max, int nM_max) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535) return 0;
    return step_lds(nJ_max, nM_max) <= TRS_LDS_BYTES && finish_lds(nJ_max, nM_max) <= TRS_LDS_BYTES;
}

int trs_pl_step(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, double* A,
                const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM, const double* F,
                int ld_f, const int32_t* info, const double* cap_tension, const double* cap_compression,
                const double* A_nom, double hardening, double lambda_max, double disp_limit, double collapse_ratio,
                double tie_tol, int it, int mode, int8_t* state, double* N, double* U, double* acc, int32_t* st,
                int32_t* active, double* lambda_history, int32_t* member_history, int32_t* count_history,
                double* umax_history, int H, void* stream) {
    if (B < 0 || nJ_max <= 0 || nM_max < 0 || ld_f < 0 || it < 0 || mode < 0 || mode > 1 || H < 0)
        return (int)hipErrorInvalidValue;
    if (!finite_at_least(hardening, 0.0) || !finite_at_least(lambda_max, 0.0) || !(lambda_max > 0.0) ||
        !finite_at_least(disp_limit, 0.0) || !finite_at_least(collapse_ratio, 1.0) || !(collapse_ratio > 1.0) ||
        !finite_at_least(tie_tol, 0.0))
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !conn || !E || !A || !free_index || !F || !info || !cap_tension || !cap_compression || !A_nom || !state ||
        !N || !U || !acc || !st || !active ||
        (H > 0 && (!lambda_history || !member_history || !count_history || !umax_history)))
        return (int)hipErrorInvalidValue;
    if (!trs_pl_fits(nJ_max, nM_max)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nJ, nM,
                                  nullptr, ld_f);
    const StepArgs g = {F, info, cap_tension, cap_compression, A_nom, hardening, lambda_max, disp_limit, collapse_ratio,
                        tie_tol, it, mode, H, A, reinterpret_cast<signed char*>(state), N, U, acc, st, active,
                        lambda_history, member_history, count_history, umax_history};
    trs_lds::raise_lds_once<trs_pl_step_kernel>();
    hipLaunchKernelGGL(trs_pl_step_kernel, dim3(B), dim3(256), step_lds(nJ_max, nM_max), (hipStream_t)stream, bt, g);
    return (int)hipGetLastError();
}

int trs_pl_finish(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const int32_t* free_index,
                  const int32_t* n_free, const int32_t* nJ, const int32_t* nM, int ld_f, const double* loads,
                  const double* N, const double* U, const double* acc, const int32_t* joint_out, double* u, double* f_ext,
                  void* stream) {
    if (B < 0 || nJ_max <= 0 || nM_max < 0 || ld_f < 0) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !conn || !free_index || !loads || !N || !U || !acc || !u || !f_ext) return (int)hipErrorInvalidValue;
    if (!trs_pl_fits(nJ_max, nM_max)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, nullptr, nullptr), free_index, n_free, nJ,
                                  nM, joint_out, ld_f);
    const FinishArgs g = {loads, N, U, acc, u, f_ext};
    trs_lds::raise_lds_once<trs_pl_finish_kernel>();
    hipLaunchKernelGGL(trs_pl_finish_kernel, dim3(B), dim3(256), finish_lds(nJ_max, nM_max), (hipStream_t)stream, bt, g);
    return (int)hipGetLastError();
}

}  // extern "C"
