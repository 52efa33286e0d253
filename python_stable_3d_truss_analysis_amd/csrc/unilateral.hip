// Tension-only and compression-only members: the active-set iteration on the device (include/trs_unilateral.h).  The
// assembly, the factorisation, the right-hand side and the substitution of every analysis are trs_assemble,
// trs_potrf_batched, trs_effects_rhs and trs_potrs_cases as they are, given the effective areas; this file holds what
// turns the reduced solution into the next state:
//
//   trs_un_step   one analysis: the elongation of every member beyond its stress-free length, the state every
//                 unilateral member wants, the count of the flips, the next state and the next effective areas
//
// The method, analysis k of state s_k (the header and tests/unilateral_reference.py state it in the same words):
//     A_eff,m = A_m if s_k,m is active, else slack_factor A_m; bilateral members are always active
//     solve K(A_eff) u = f, the right-hand side formed with A_eff
//     e_m = c_m.(u_j1 - u_j0) - eps0_m L0_m, for every member, slack ones included
//     want_m = active if kind_m = 0 or kind_m e_m > 0, else slack: the test is strict, no thresholds
//     changed = the number of members with want_m != s_k,m
//     changed = 0: converged; else k = max_iters: status 1; else s_{k+1} = want (all flips at once)
//     info != 0: status 2, back to s_{k-1} (the initial state for k = 0)
//
// One 256-thread work-group per truss.  The reduced solution is staged into LDS through rows(j), one test per joint;
// thread tid owns the members tid, tid + 256, ...: it is the only thread that touches their LDS byte (want, state), so
// the byte table needs no barrier.  The member loop runs the same number of trips in every lane, so that the flips of a
// trip are counted by the wave's ballot; the four waves' counts meet in LDS.  No floating-point sum anywhere.
#include "../../include/trs_unilateral.h"
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_iterate.h"
#include "trs_lds.h"

namespace {

using Run = trs_iter::Run<TRS_UN_ACTIVE, TRS_UN_NOT_PD>;

// LDS tables of the step kernel
struct StepTables {
    double* u;            // [3 nJ_max]  the displacements, joint layout, device numbering
    int* cnt;             // [4]         the waves' flip counts
    signed char* flag;    // [nM_max]    bit 0: want, bit 1: the state analysed
};

template <class Arena>
__host__ __device__ inline StepTables step_layout(Arena& a, int nJ_max, int nM_max) {
    StepTables t;
    t.u = a.template take<double>(3, nJ_max);
    t.cnt = a.template take<int>(4);
    t.flag = a.template take<signed char>(nM_max);
    return t;
}

size_t step_lds(int nJ_max, int nM_max) { return trs_lds::count([&](auto& a) { step_layout(a, nJ_max, nM_max); }); }

struct StepArgs {
    const double* F;             // [B][1][ld_f]
    const int* info;             // [B]
    const double* eps0;          // [B][nM_max] or null
    const signed char* kind;     // [B][nM_max]
    const double* A_nom;         // [B][nM_max]
    const signed char* state0;   // [B][nM_max] or null
    double slack_factor;
    int it, mode, H;
    double* A;                   // [B][nM_max]
    signed char* state;          // [B][nM_max]
    signed char* prev_state;     // [B][nM_max]
    int* st;                     // [B][4]
    int* active;
    int* violations;             // [B]
    int* history;                // [B][H]
};

__global__ __launch_bounds__(256) void trs_un_step_kernel(const TrsBatch bt, const StepArgs g) {
    extern __shared__ double sh[];   // (no static LDS beside it: the dynamic ceiling is the whole of a CU's)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int mode = g.mode, it = g.it;
    const int pivot = g.info[b];
    const bool begin = it == 0 && mode != 2;
    Run run(g.st + 4 * b, begin);
    // mode 2, this analysis's own: the violations of the state a truss ended with, whatever its status
    const bool report = mode == 2 && !run.active();
    if (!run.active() && !report) return;   // (uniform over the work-group) frozen: nothing is touched
    if (report && pivot != 0) return;                 // the state it holds could not be analysed: nothing changes
    const TrussView tr = bt.truss(b);
    const int members = tr.members;
    const size_t mbase = tr.mbase;
    double* Ab = g.A + mbase;
    const double* An = g.A_nom + mbase;
    const signed char* kind = g.kind + mbase;
    signed char* state = g.state + mbase;
    const double slack = g.slack_factor;
    // the state this analysis is of: the initial one when the run begins, else the one the last call left
    auto analysed = [&](int m, int k) -> int {
        if (k == 0) return 1;
        if (!begin) return state[m] != 0;
        return g.state0 != nullptr ? g.state0[mbase + m] != 0 : 1;
    };
    auto unilateral = [](int k) -> int { return k == 1 || k == -1 ? k : 0; };
    if (pivot != 0) {
        // status 2: back to s_{k-1} and its areas (k = 0: the initial state); `violations` stays that of analysis k - 1
        for (int m = tid; m < members; m += 256) {
            const int k = unilateral(kind[m]);
            const int s = begin ? analysed(m, k) : (k == 0 || g.prev_state[mbase + m] != 0);
            state[m] = (signed char)s;
            Ab[m] = s ? An[m] : slack * An[m];
        }
        run.fail(pivot, run.one_back(), tid);
        if (tid == 0 && begin) g.violations[b] = 0;
        return;
    }
    trs_lds::Carve lds(sh);
    const StepTables t = step_layout(lds, bt.nJ_max, bt.nM_max);
    const double* f = g.F + (size_t)b * bt.ld_f;
    for (int j = tid; j < bt.nJ_max; j += 256) {   // held DOFs and the padding read 0
        const TrussView::Rows q = tr.rows(j);
#pragma unroll
        for (int a = 0; a < 3; ++a) t.u[3 * j + a] = q.r[a] >= 0 ? f[q.r[a]] : 0.0;
    }
    __syncthreads();
    // ---- e_m, want_m and the flips; every lane runs every trip (the ballot counts a whole wave's trip) ----
    const double* eps0 = g.eps0 != nullptr ? g.eps0 + mbase : nullptr;
    int flips = 0;   // of this wave
    for (int m0 = 0; m0 < members; m0 += 256) {
        const int m = m0 + tid;
        bool flip = false;
        if (m < members) {
            const int2 c = tr.ends(m).c;
            const trs_rec::MemberGeom geo = trs_rec::member_geom(tr.X, c.x, c.y);
            const double* u0 = t.u + 3 * c.x;
            const double* u1 = t.u + 3 * c.y;
            double e = geo.c[0] * (u1[0] - u0[0]);
            e += geo.c[1] * (u1[1] - u0[1]);
            e += geo.c[2] * (u1[2] - u0[2]);
            if (eps0 != nullptr) e -= eps0[m] * geo.len;
            const int k = unilateral(kind[m]);
            const int cur = analysed(m, k);
            const int want = k == 0 || (double)k * e > 0.0;   // (strictly: e = 0 means slack)
            flip = want != cur;
            t.flag[m] = (signed char)(want | (cur << 1));
            if (begin) state[m] = (signed char)cur;
        }
        flips += __popcll(__ballot(flip));
    }
    if ((tid & 63) == 0) t.cnt[tid >> 6] = flips;
    __syncthreads();
    const int changed = (t.cnt[0] + t.cnt[1]) + (t.cnt[2] + t.cnt[3]);
    if (report) {
        if (tid == 0) g.violations[b] = changed;
        return;
    }
    if (changed == 0)
        run.status = TRS_UN_CONVERGED;
    else if (mode == 1)
        run.status = TRS_UN_ITER_LIMIT;
    if (run.active()) {
        for (int m = tid; m < members; m += 256) {   // (the thread that owns member m wrote t.flag[m])
            const int fl = t.flag[m];
            g.prev_state[mbase + m] = (signed char)(fl >> 1);
            state[m] = (signed char)(fl & 1);
            Ab[m] = (fl & 1) ? An[m] : slack * An[m];
        }
    }
    if (tid == 0) {
        g.violations[b] = changed;
        if (it < g.H) g.history[(size_t)b * g.H + it] = changed;
        run.finish(it, g.active);
    }
}

}  // namespace

extern "C" {

int trs_un_abi_version(void) { return TRS_UN_ABI_VERSION; }

int trs_un_fits(int nJ_max, int nM_max) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535) return 0;
    return step_lds(nJ_max, nM_max) <= TRS_LDS_BYTES;
}

int trs_un_step(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, double* A,
                const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM, const double* F,
                int ld_f, const int32_t* info, const double* eps0, const int8_t* kind, const double* A_nom,
                double slack_factor, const int8_t* state0, int it, int mode, int8_t* state, int8_t* prev_state,
                int32_t* st, int32_t* active, int32_t* violations, int32_t* flips_history, int H, void* stream) {
    if (B < 0 || nJ_max <= 0 || nM_max < 0 || ld_f < 0 || it < 0 || mode < 0 || mode > 2 || H < 0)
        return (int)hipErrorInvalidValue;
    if (!(slack_factor >= 0.0) || !(slack_factor <= 1.7e308)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !conn || !A || !free_index || !F || !info || !kind || !A_nom || !state || !prev_state || !st || !active ||
        !violations || (H > 0 && !flips_history))
        return (int)hipErrorInvalidValue;
    if (!trs_un_fits(nJ_max, nM_max)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, nullptr, A), free_index, n_free, nJ, nM,
                                  nullptr, ld_f);
    const StepArgs g = {F, info, eps0, reinterpret_cast<const signed char*>(kind), A_nom,
                        reinterpret_cast<const signed char*>(state0), slack_factor, it, mode, H, A,
                        reinterpret_cast<signed char*>(state), reinterpret_cast<signed char*>(prev_state), st, active,
                        violations, flips_history};
    trs_lds::raise_lds_once<trs_un_step_kernel>();
    hipLaunchKernelGGL(trs_un_step_kernel, dim3(B), dim3(256), step_lds(nJ_max, nM_max), (hipStream_t)stream, bt, g);
    return (int)hipGetLastError();
}

}  // extern "C"
