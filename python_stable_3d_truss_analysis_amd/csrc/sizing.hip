// Member sizing: fully stressed design with a displacement envelope, iterated on the device (include/trs_sizing.h).
// The assembly, the factorisation, the gather and the multi-case substitution of every iteration are trs_assemble,
// trs_potrf_batched, trs_gather_cases and trs_potrs_cases as they are; this file holds what turns the L reduced
// solutions into the next design:
//
//   trs_sz_step   one analysis: member forces of every case, the required areas, the displacement ratio, the resizing,
//                 the convergence test and the truss's outputs
//   trs_sz_snap   the catalogue pass over the areas
//
// The method, analysis k of design A_k (the header and tests/sizing_reference.py state it in the same words):
//     for each case l, N_ml = (E A_k / L0) c.(u_j1 - u_j0)
//     the required area in case l is N / allow_tension for N > 0; for P = -N > 0 it is
//       max(P / allow_compression, sqrt(P L0^2 / (pi^2 E kappa))), the second term only when kappa > 0
//     req_m is the maximum over the cases, taken in ascending l; on a tie the lowest l governs
//     d = max over cases and the truss's joints of |u_j| / allow_displace; 0 without a limit
//     r_m = max(req_m / A_m, d);  A'_m = clamp(A_m ((1 - relax) + relax r_m), a_min_m, a_max_m)
//     change = max_m |A'_m - A_m| / A_m;  change <= tol: converged; else k = max_iters: status 1; else A_{k+1} = A'
//
// trs_sz_step: one 256-thread work-group per truss.  A thread owns the members tid, tid + 256, ...: it forms their
// geometry once (c, E A / L0, the Euler coefficient), keeps it in LDS beside the running requirement and its case, and
// is the only thread that ever touches those entries - the member tables need no barrier.  One case's displacement
// vector at a time is staged in LDS through row_of, in two buffers: the next case is staged behind the work on this
// one, one barrier per case.  The displacement ratio and the change are maxima; the weight is summed per thread in
// ascending m, then by the wave butterfly, then over the four waves in order.  No floating-point atomic.
#include "../../include/trs_sizing.h"
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_iterate.h"
#include "trs_lds.h"

namespace {

using Run = trs_iter::Run<TRS_SZ_ACTIVE, TRS_SZ_NOT_PD>;

// LDS tables of the step kernel
struct StepTables {
    double* u;      // [2][3 nJ_max]  the displacements of two cases, joint layout, device numbering
    double* red;    // [8]            the wave partials of a reduction
    double* c0;     // [nM_max] x 3   direction cosines
    double* c1;
    double* c2;
    double* k;      // [nM_max]       E A / L0
    double* eul;    // [nM_max]       L0^2 / (pi^2 E kappa), 0 without the member buckling check
    double* req;    // [nM_max]       the running requirement, then A'
    int2* ends;     // [nM_max]       end joints, clamped
    int* gov;       // [nM_max]       the case of the running requirement
    int* row;       // [3 nJ_max]     row_of every DOF (-1: reads 0), formed once: a case's staging is one load deep
};

template <class Arena>
__host__ __device__ inline StepTables step_layout(Arena& a, int nJ_max, int nM_max) {
    StepTables t;
    t.u = a.template take<double>(6, nJ_max);
    t.red = a.template take<double>(8);
    t.c0 = a.template take<double>(nM_max);
    t.c1 = a.template take<double>(nM_max);
    t.c2 = a.template take<double>(nM_max);
    t.k = a.template take<double>(nM_max);
    t.eul = a.template take<double>(nM_max);
    t.req = a.template take<double>(nM_max);
    t.ends = a.template take<int2>(nM_max);
    t.gov = a.template take<int>(nM_max);
    t.row = a.template take<int>(3, nJ_max);
    return t;
}

size_t step_lds(int nJ_max, int nM_max) { return trs_lds::count([&](auto& a) { step_layout(a, nJ_max, nM_max); }); }

__device__ __forceinline__ double block_max(double v, double* slot, const int tid) {   // slot [4], 256 threads
    v = trs_iter::wave_max(v);
    __syncthreads();   // (the previous readers of slot are done)
    if ((tid & 63) == 0) slot[tid >> 6] = v;
    __syncthreads();
    return fmax(fmax(slot[0], slot[1]), fmax(slot[2], slot[3]));
}

// the wave butterfly, then the four waves in wave order
__device__ __forceinline__ double block_sum(double v, double* slot, const int tid) {
    v = trs_iter::wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) slot[tid >> 6] = v;
    __syncthreads();
    return ((slot[0] + slot[1]) + slot[2]) + slot[3];
}

struct StepArgs {
    const double* F;          // [B][L][ld_f]
    const int* info;          // [B]
    double allow_tension, allow_compression, allow_displace, euler_kappa, relax, tol;
    const double* allow;      // [B][3] or null: the three allowables per truss
    trs_iter::AreaBounds bounds;
    int L, it, mode, H;
    double* A;                // [B][nM_max]
    double* prev;             // [B][nM_max]
    int* st;                  // [B][4]
    int* active;
    double* areas;            // [B][nM_max]
    double* weight;           // [B]
    double* util;             // [B][nM_max]
    int* governing;           // [B][nM_max]
    double* disp_ratio;       // [B]
    double* history;          // [B][H]
};

__global__ __launch_bounds__(256) void trs_sz_step_kernel(const TrsBatch bt, const StepArgs g) {
    extern __shared__ double sh[];   // (no static LDS beside it: the dynamic ceiling is the whole of a CU's)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int nM_max = bt.nM_max, ld_f = bt.ld_f;
    const int mode = g.mode, it = g.it, L = g.L;
    Run run(g.st + 4 * b, it == 0 && mode != 2);
    // mode 2, this analysis's own: the snapped design of a truss that ended with status 0 or 1 is reported
    const bool report = mode == 2 && (run.status == TRS_SZ_CONVERGED || run.status == TRS_SZ_ITER_LIMIT);
    if (!run.active() && !report) return;   // (uniform over the work-group) frozen: nothing is touched
    const TrussView tr = bt.truss(b);
    const int members = tr.members, joints = tr.joints, ndof_max = tr.ndof_max;
    const size_t mbase = tr.mbase;
    double* Ab = g.A + mbase;
    const int pivot = g.info[b];
    if (pivot != 0) {
        if (report) {   // the snapped design could not be analysed: the outputs stay, the info is latched
            if (tid == 0 && g.st[4 * b + 2] == 0) g.st[4 * b + 2] = pivot;
            return;
        }
        // status 2: back to A_{k-1}; the outputs stay those of analysis k - 1 (k = 0: zeros, the initial areas)
        for (int m = tid; m < nM_max; m += 256) {
            if (it == 0) {
                g.areas[mbase + m] = m < members ? Ab[m] : 0.0;
                g.util[mbase + m] = 0.0;
                g.governing[mbase + m] = -1;
            } else if (m < members) {
                Ab[m] = g.prev[mbase + m];
            }
        }
        run.fail(pivot, run.one_back(), tid);
        if (tid == 0 && it == 0) {
            g.weight[b] = 0.0;
            g.disp_ratio[b] = 0.0;
        }
        return;
    }
    trs_lds::Carve lds(sh);
    const StepTables t = step_layout(lds, bt.nJ_max, nM_max);
    const trs_iter::CaseStage cases = {t.u, t.row, g.F + (size_t)b * L * ld_f, ndof_max, ld_f};
    cases.form_rows(tr, tid);
    cases.stage(0, tid);
    // ---- the member geometry, once; the weight of the design ----
    const double kappa = g.euler_kappa;
    constexpr double PI = 3.14159265358979323846;
    double wsum = 0.0;
    for (int m = tid; m < members; m += 256) {
        const int2 c = tr.ends(m).c;
        const trs_rec::MemberGeom geo = trs_rec::member_geom(tr.X, c.x, c.y);
        const double E = tr.mem.E[mbase + m], A = Ab[m];
        t.ends[m] = c;
        t.c0[m] = geo.c[0];
        t.c1[m] = geo.c[1];
        t.c2[m] = geo.c[2];
        t.k[m] = E * A / geo.len;
        t.eul[m] = kappa > 0.0 ? (geo.len * geo.len) / (((PI * PI) * E) * kappa) : 0.0;
        t.req[m] = 0.0;
        t.gov[m] = 0;
        wsum += (A * geo.len) * tr.mem.rho[mbase + m];
    }
    __syncthreads();   // (case 0 is staged)
    // ---- the cases: requirement and governing case per member, the largest joint displacement ----
    const double at = g.allow != nullptr ? g.allow[3 * b] : g.allow_tension;
    const double ac = g.allow != nullptr ? g.allow[3 * b + 1] : g.allow_compression;
    const double ad = g.allow != nullptr ? g.allow[3 * b + 2] : g.allow_displace;
    double umax = 0.0;
    for (int l = 0; l < L; ++l) {
        const double* u = cases.buffer(l);
        for (int m = tid; m < members; m += 256) {
            const int2 c = t.ends[m];
            const double* u0 = u + 3 * c.x;
            const double* u1 = u + 3 * c.y;
            double proj = t.c0[m] * (u1[0] - u0[0]);
            proj += t.c1[m] * (u1[1] - u0[1]);
            proj += t.c2[m] * (u1[2] - u0[2]);
            const double N = t.k[m] * proj;
            double r = 0.0;
            if (N > 0.0) {
                r = N / at;
            } else if (N < 0.0) {
                const double P = -N;
                r = P / ac;
                if (kappa > 0.0) r = fmax(r, sqrt(P * t.eul[m]));
            }
            if (r > t.req[m]) {   // (strictly: on a tie the lowest l governs)
                t.req[m] = r;
                t.gov[m] = l;
            }
        }
        for (int j = tid; j < joints; j += 256) {
            const double x = u[3 * j], y = u[3 * j + 1], z = u[3 * j + 2];
            umax = fmax(umax, sqrt(x * x + y * y + z * z));
        }
        if (l + 1 < L) cases.stage(l + 1, tid);   // (the other buffer: its readers passed the barrier of case l - 1)
        __syncthreads();
    }
    umax = block_max(umax, t.red, tid);
    const double d = ad > 0.0 ? umax / ad : 0.0;
    // ---- the outputs of this design, the next design ----
    const double relax = g.relax, keep = 1.0 - g.relax;
    double change = 0.0;
    for (int m = tid; m < nM_max; m += 256) {
        double util = 0.0, area = 0.0;
        int gov = -1;
        if (m < members) {
            area = Ab[m];
            util = t.req[m] / area;
            gov = d > util ? -1 : t.gov[m];
            if (!report) {
                const double r = fmax(util, d);
                const double lo = g.bounds.lo(mbase + m), hi = g.bounds.hi(mbase + m);
                const double next = fmin(fmax(area * (keep + relax * r), lo), hi);
                change = fmax(change, fabs(next - area) / area);
                t.req[m] = next;
            }
        }
        g.util[mbase + m] = util;
        g.governing[mbase + m] = gov;
        g.areas[mbase + m] = area;
    }
    const double weight = block_sum(wsum, t.red, tid);
    if (report) {
        if (tid == 0) {
            g.weight[b] = weight;
            g.disp_ratio[b] = d;
        }
        return;
    }
    change = block_max(change, t.red + 4, tid);
    if (change <= g.tol)
        run.status = TRS_SZ_CONVERGED;
    else if (mode == 1)
        run.status = TRS_SZ_ITER_LIMIT;
    if (run.active()) {
        for (int m = tid; m < members; m += 256) {   // (the thread that owns member m wrote t.req[m])
            g.prev[mbase + m] = Ab[m];
            Ab[m] = t.req[m];
        }
    }
    if (tid == 0) {
        g.weight[b] = weight;
        g.disp_ratio[b] = d;
        if (it < g.H) g.history[(size_t)b * g.H + it] = weight;
        run.finish(it, g.active);
    }
}

// one thread per member; T <= 256 ascending areas
__global__ __launch_bounds__(256) void trs_sz_snap_kernel(const int nM_max, const int* __restrict__ nM,
                                                          const int* __restrict__ st, const double* __restrict__ catalog,
                                                          const int T, double* __restrict__ A,
                                                          unsigned char* __restrict__ index) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int status = st[4 * b];
    const bool live = status == TRS_SZ_CONVERGED || status == TRS_SZ_ITER_LIMIT;
    const int members = min(max(nM[b], 0), nM_max);
    for (int m = tid; m < nM_max; m += 256) {
        const size_t mm = (size_t)b * nM_max + m;
        int pick = 0;
        if (live && m < members) {
            const double a = A[mm];
            int lo = 0, hi = T - 1;   // the first entry >= a, or the last entry
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (catalog[mid] >= a)
                    hi = mid;
                else
                    lo = mid + 1;
            }
            pick = lo;
            A[mm] = catalog[pick];
        }
        index[mm] = (unsigned char)pick;
    }
}

}  // namespace

extern "C" {

int trs_sz_abi_version(void) { return TRS_SZ_ABI_VERSION; }

int trs_sz_fits(int nJ_max, int nM_max) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535) return 0;
    return step_lds(nJ_max, nM_max) <= TRS_LDS_BYTES;
}

int trs_sz_step(int B, int L, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, double* A,
                const double* rho, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
                const double* F, int ld_f, const int32_t* info, double allow_tension, double allow_compression,
                double allow_displace, const double* allow, double euler_kappa, double relax, double tol,
                const double* a_min, double a_min_all, const double* a_max, double a_max_all, int it, int mode,
                double* prev, int32_t* st,
                int32_t* active, double* areas, double* weight, double* utilisation, int32_t* governing,
                double* disp_ratio, double* weight_history, int H, void* stream) {
    if (B < 0 || L < 1 || nJ_max <= 0 || nM_max < 0 || ld_f < 0 || it < 0 || mode < 0 || mode > 2 || H < 0)
        return (int)hipErrorInvalidValue;
    if (!allow && (!(allow_tension > 0.0) || !(allow_compression > 0.0) || !(allow_displace >= 0.0)))
        return (int)hipErrorInvalidValue;
    if (!(euler_kappa >= 0.0) || !(relax > 0.0) || !(relax <= 1.0) || !(tol >= 0.0)) return (int)hipErrorInvalidValue;
    const trs_iter::AreaBounds bounds = {a_min, a_max, a_min_all, a_max_all};
    if (!bounds.valid()) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!xyz || !conn || !E || !A || !rho || !free_index || !F || !info || !prev || !st || !active || !areas || !weight ||
        !utilisation || !governing || !disp_ratio || (H > 0 && !weight_history))
        return (int)hipErrorInvalidValue;
    if (!trs_sz_fits(nJ_max, nM_max)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A, rho), free_index, n_free, nJ, nM,
                                  nullptr, ld_f);
    const StepArgs g = {F, info, allow_tension, allow_compression, allow_displace, euler_kappa, relax, tol, allow,
                        bounds, L, it, mode, H, A, prev, st, active, areas, weight, utilisation, governing, disp_ratio,
                        weight_history};
    trs_lds::raise_lds_once<trs_sz_step_kernel>();
    hipLaunchKernelGGL(trs_sz_step_kernel, dim3(B), dim3(256), step_lds(nJ_max, nM_max), (hipStream_t)stream, bt, g);
    return (int)hipGetLastError();
}

int trs_sz_snap(int B, int nM_max, const int32_t* nM, const int32_t* st, const double* catalog, int T, double* A,
                uint8_t* catalog_index, void* stream) {
    if (B < 0 || nM_max < 0 || T < 1 || T > TRS_SZ_MAX_CATALOG) return (int)hipErrorInvalidValue;
    if (B == 0 || nM_max == 0) return 0;
    if (!nM || !st || !catalog || !A || !catalog_index) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(trs_sz_snap_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, nM_max, nM, st, catalog, T, A,
                       catalog_index);
    return (int)hipGetLastError();
}

}  // extern "C"
