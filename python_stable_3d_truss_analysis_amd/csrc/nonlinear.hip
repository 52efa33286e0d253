// Geometrically nonlinear statics: Newton's method on the batch's tangent factor (include/trs_nonlinear.h).  The
// assembly, the factorisation and the substitution of every iteration are trs_assemble, trs_potrf_batched and
// trs_potrs_batched as they are; this file holds what goes around them:
//
//   trs_nl_state     one iterate: member forces, internal forces, Xc = X + u, R = lambda P - f_int, the convergence test,
//                    the member table of the tangent kernel and - at the end of a load step - the step's outputs
//   trs_nl_tangent   S += delta_m per member on the assembled slab: it then holds the tangent stiffness
//   trs_nl_update    u += du for the trusses that are still iterating
//
// The formulation, per member m with ends j0, j1, undeformed coordinates X and displacement u:
//     D = X_j1 - X_j0, L0 = |D|, dl = u_j1 - u_j0, d = D + dl, l = |d|, n = d / l
//     e = (2 D.dl + dl.dl) / (L0 (l + L0))   (= (l - L0) / L0 exactly, without subtracting two lengths),  N = E A e
//     internal force +N n at j1, -N n at j0
//     k_t = (EA / L0) n n^T + (N / l)(I - n n^T);  trs_assemble at X + u writes (EA / l) n n^T, so
//     delta_m = (EA/L0 - EA/l - N/l) n n^T + (N/l) I is what is missing: + on the diagonal blocks, - on the coupling ones
//
// trs_nl_state: one 256-thread work-group per truss.  One thread per DOF stages u in LDS (joint layout) and writes Xc;
// one thread per member forms n, l, N; one thread per joint sums +- N n over its end list (trs_rec::build_end_lists,
// add_end_force - the shape of trs_effects_rhs and trs_dyn_step -, the lists then re-sorted by (far joint, member id):
// order_by_neighbour); the two norms are maxima, which do not depend on the order of the reduction.
// trs_nl_tangent: one 256-thread work-group per truss, 16 slab rows (one 16-row chunk: one cend, one mask word) per pass,
// 16 threads per row.  One thread owns a slab entry; no floating-point atomic; every sum in the lists' order.
#include "../../include/trs_nonlinear.h"
#include "../../include/trs_solver.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace {

using namespace trs_rec;

constexpr int NL_W = 6;   // doubles per member of the table W

// LDS tables of the state kernel
struct StateTables : EndLists {
    double* red;  // [4]         the wave maxima of the two norms
    double* v;    // [3 nJ_max]  u in joint layout, then r (free DOFs) / f_int (held DOFs)
    double* pm;   // [nM_max]    N
    double* pn;   // [3 nM_max]  n
    int* oth;     // [2 nM_max]  the far joint of every list entry
};

template <class Arena>
__host__ __device__ inline StateTables state_layout(Arena& a, int nJ_max, int nM_max) {
    StateTables t;
    t.red = a.template take<double>(4);
    t.v = a.template take<double>((size_t)3 * nJ_max);
    t.pm = a.template take<double>(nM_max);
    t.pn = a.template take<double>((size_t)3 * nM_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    t.oth = a.template take<int>((size_t)2 * nM_max);
    return t;
}

// LDS tables of the tangent kernel
struct TangentTables : EndLists {
    double* own;   // [nJ_max][6]   the sum of +delta_m over a joint's member ends: xx xy xz yy yz zz
    int* oth;      // [2 nM_max]    the joint at the far end of every list entry
    int* fi;       // [3 nJ_max]    reduced row per DOF, -1: none
    int* rowdof;   // [slab_rows]   DOF of a reduced row, -1: none
};

template <class Arena>
__host__ __device__ inline TangentTables tangent_layout(Arena& a, int nJ_max, int nM_max, int slab_rows) {
    TangentTables t;
    t.own = a.template take<double>(6, nJ_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    t.oth = a.template take<int>(2, nM_max);
    t.fi = a.template take<int>(3, nJ_max);
    t.rowdof = a.template take<int>(slab_rows);
    return t;
}

size_t state_lds(int nJ_max, int nM_max) { return trs_lds::count([&](auto& a) { state_layout(a, nJ_max, nM_max); }); }

size_t tangent_lds(int nJ_max, int nM_max, int slab_rows) {
    return trs_lds::count([&](auto& a) { tangent_layout(a, nJ_max, nM_max, slab_rows); });
}

// a maximum that keeps a NaN of either side (a NaN residual must never pass the convergence test)
__device__ __forceinline__ double nan_max(const double a, const double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ double block_nan_max(double v, double* slot, const int tid) {   // slot [4], 256 threads
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_xor(v, off));
    __syncthreads();   // (the previous readers of slot are done)
    if ((tid & 63) == 0) slot[tid >> 6] = v;
    __syncthreads();
    return nan_max(nan_max(slot[0], slot[1]), nan_max(slot[2], slot[3]));
}

__global__ __launch_bounds__(256) void trs_nl_state_kernel(
    const TrsBatch bt, const double* __restrict__ loads, const double lambda, const double tol, const int it,
    const int last, const int step, const int S, const double* __restrict__ U, int* __restrict__ st,
    double* __restrict__ Xc, double* __restrict__ R, double* __restrict__ W, int* __restrict__ active,
    double* __restrict__ u_out, double* __restrict__ N_out, double* __restrict__ f_out, int* __restrict__ iters,
    int* __restrict__ status_out, double* __restrict__ residual) {
    extern __shared__ double sh[];   // (no static LDS beside it: the dynamic ceiling is the whole of a CU's)
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView tr = bt.truss(b);
    const int nJ_max = bt.nJ_max, nM_max = bt.nM_max;
    const int joints = tr.joints, members = tr.members, ndof = tr.ndof, ndof_max = tr.ndof_max;
    trs_lds::Carve lds(sh);
    const StateTables t = state_layout(lds, nJ_max, nM_max);
    double* ush = t.v;
    const double* __restrict__ X = tr.X;
    const double* P = loads + (size_t)b * ndof_max;
    const double* Ub = U + (size_t)b * ndof_max;
    const size_t mbase = tr.mbase;
    // (every thread reads the status word before the barriers below; thread 0 writes it behind them)
    int status = st[4 * b], its = st[4 * b + 1];
    if (it == 0 && last != 2) {   // the load step begins (not again in a call that only writes the outputs)
        status = status >= TRS_NL_ITER_LIMIT ? TRS_NL_NOT_ATTEMPTED : TRS_NL_ACTIVE;
        its = 0;
    }
    build_end_lists(t, tr, tid);
    order_by_neighbour(t, t.oth, tr, tid);
    // ---- the state, one thread per DOF ----
    for (int d = tid; d < ndof_max; d += 256) {
        const double u = tr.row_of(d) >= 0 ? Ub[d] : 0.0;
        ush[d] = u;
        Xc[(size_t)b * ndof_max + d] = X[d] + u;
    }
    __syncthreads();   // (u is staged, the end lists are sorted)
    // ---- one thread per member: n, l, N ----
    for (int m = tid; m < members; m += 256) {
        const int2 c = tr.ends(m).c;
        double D[3], dl[3], d[3], L02 = 0.0, l2 = 0.0, Ddl = 0.0, dldl = 0.0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            D[a] = X[3 * c.y + a] - X[3 * c.x + a];
            dl[a] = ush[3 * c.y + a] - ush[3 * c.x + a];
            d[a] = D[a] + dl[a];
            L02 += D[a] * D[a];
            l2 += d[a] * d[a];
            Ddl += D[a] * dl[a];
            dldl += dl[a] * dl[a];
        }
        const double L0 = sqrt(L02), l = sqrt(l2);
        const double EA = tr.mem.EA(mbase + m);
        const double e = (2.0 * Ddl + dldl) / (L0 * (l + L0));
        const double N = EA * e;
        const double g = N / l;
        double* w = W + (mbase + m) * NL_W;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double na = d[a] / l;
            t.pn[3 * m + a] = na;
            w[a] = na;
        }
        t.pm[m] = N;
        w[3] = EA / L0 - EA / l - g;
        w[4] = g;
        w[5] = N;
    }
    __syncthreads();   // (the readers of u in ush are done; N and n are in place)
    // ---- one thread per joint: f_int, r = lambda P - f_int at its free DOFs ----
    double rmax = 0.0, pmax = 0.0;
    for (int j = tid; j < joints; j += 256) {
        double f[3] = {0.0, 0.0, 0.0};
        const int* list = t.ends + t.start[j];
        const int deg = t.cnt[j];
        for (int i = 0; i < deg; ++i) {
            const int m = list[i] >> 1, end = list[i] & 1;
            const double c3[3] = {t.pn[3 * m], t.pn[3 * m + 1], t.pn[3 * m + 2]};
            add_end_force(f, c3, t.pm[m], end);
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int d = 3 * j + a;
            if (tr.row_of(d) >= 0) {
                const double p = lambda * P[d];
                const double r = p - f[a];
                ush[d] = r;
                rmax = nan_max(rmax, fabs(r));
                pmax = nan_max(pmax, fabs(p));
            } else {
                ush[d] = f[a];   // the reaction
            }
        }
    }
    rmax = block_nan_max(rmax, t.red, tid);
    pmax = block_nan_max(pmax, t.red, tid);
    if (status == TRS_NL_ACTIVE) {
        if (pmax == 0.0 || rmax <= tol * pmax)
            status = TRS_NL_CONVERGED;
        else if (last)
            status = TRS_NL_ITER_LIMIT;
    }
    const bool still = status == TRS_NL_ACTIVE;
    for (int d = tid; d < ndof_max; d += 256) R[(size_t)b * ndof_max + d] = (still && tr.row_of(d) >= 0) ? ush[d] : 0.0;
    if (tid == 0) {
        st[4 * b] = status;
        st[4 * b + 1] = its;
        if (still) atomicAdd(active, 1);
    }
    if (!last) return;
    // ---- the outputs of this load step, in the caller's numbering ----
    const size_t bs = (size_t)b * S + step;
    for (int d = tid; d < ndof_max; d += 256) {
        const size_t o = bs * ndof_max + tr.place_dof(d);
        const bool free_dof = tr.row_of(d) >= 0;
        u_out[o] = free_dof ? Ub[d] : 0.0;
        f_out[o] = d < ndof ? (free_dof ? lambda * P[d] : ush[d]) : 0.0;
    }
    for (int m = tid; m < nM_max; m += 256) N_out[bs * nM_max + m] = m < members ? t.pm[m] : 0.0;
    if (tid == 0) {
        iters[bs] = its;
        status_out[bs] = status;
        residual[bs] = rmax;
    }
}

// (The batch's ld_f is slab_rows here: the reduced rows are the slab's.)
__global__ __launch_bounds__(256) void trs_nl_tangent_kernel(const TrsBatch bt, const int ld, double* __restrict__ S_all,
                                                             const int* __restrict__ env_all, const int full,
                                                             const double* __restrict__ W) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView tr = bt.truss(b);
    const int slab_rows = bt.ld_f, joints = tr.joints, ndof_max = tr.ndof_max;
    const int n = tr.nfree, npad = min(trs_round_up(n, TRS_NB), slab_rows);
    const int nch = npad / 16;
    trs_lds::Carve lds(sh);
    const TangentTables t = tangent_layout(lds, bt.nJ_max, bt.nM_max, slab_rows);
    double* own = t.own;
    int *oth = t.oth, *fi = t.fi, *rowdof = t.rowdof;
    const size_t mbase = tr.mbase;
    for (int c = tid; c < slab_rows; c += 256) rowdof[c] = -1;
    build_end_lists(t, tr, tid);
    __syncthreads();   // (the lists are sorted; rowdof is cleared)
    for (int d = tid; d < ndof_max; d += 256) {
        const int r = tr.row_of(d);
        fi[d] = r;
        if (r >= 0) rowdof[r] = d;
    }
    order_by_neighbour(t, oth, tr, tid);
    const double* Wb = W + mbase * NL_W;
    // delta_m = w3 n n^T + w4 I, entry (r, s) formed as w3 (n_r n_s) [+ w4]: symmetric to the bit, as the assembly's k (c_r c_s)
    auto delta = [&](int m, double (&v)[6]) {
        const double* w = Wb + (size_t)m * NL_W;
        const d2 n01 = *reinterpret_cast<const d2*>(w), n2a = *reinterpret_cast<const d2*>(w + 2);
        const double g = w[4];
        v[0] = n2a.y * (n01.x * n01.x) + g;
        v[1] = n2a.y * (n01.x * n01.y);
        v[2] = n2a.y * (n01.x * n2a.x);
        v[3] = n2a.y * (n01.y * n01.y) + g;
        v[4] = n2a.y * (n01.y * n2a.x);
        v[5] = n2a.y * (n2a.x * n2a.x) + g;
    };
    // one thread per joint, once: its own block (every row pass below would otherwise walk the whole list again, one
    // dependent load of W after the other; the thread that owns the joint's lists sums them, so no barrier before)
    for (int j = tid; j < joints; j += 256) {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        const int s0 = t.start[j], deg = t.cnt[j];
        for (int i = 0; i < deg; ++i) {
            if (oth[s0 + i] < 0 || oth[s0 + i] == j) continue;
            double v[6];
            delta(t.ends[s0 + i] >> 1, v);
#pragma unroll
            for (int q = 0; q < 6; ++q) acc[q] += v[q];
        }
#pragma unroll
        for (int q = 0; q < 6; ++q) own[6 * j + q] = acc[q];
    }
    __syncthreads();
    const int* cend = nullptr;
    const int* kmask = nullptr;
    if (env_all != nullptr) {
        const int* env = env_all + (size_t)b * trs_env_stride(slab_rows);
        cend = env + trs_env_cend_offset(slab_rows);
        kmask = env + trs_env_kmask_offset(slab_rows);
    }
    double* Sb = S_all + (size_t)b * slab_rows * ld;
    const int rr = tid >> 4, e = tid & 15;
    for (int c0 = 0; c0 < n; c0 += 16) {
        const int c = c0 + rr;
        if (c >= n) continue;
        const int dof = rowdof[c];
        if (dof < 0) continue;
        const int a = dof / 3, r = dof - 3 * a;
        const int chunk = c0 >> 4;
        // the stored part of this row (trs_assemble's row loop): columns [i_lo, i_hi), the tiles of the mask word
        const int i_lo = full ? 0 : 16 * chunk;
        const int i_hi = (cend != nullptr && !full) ? 16 * min(max(cend[chunk], 0), nch) : npad;
        const int km = (kmask != nullptr && !full) ? kmask[chunk] : -1;
        auto stored = [&](int q) {
            if (q < i_lo || q >= i_hi) return false;
            if (km == -1) return true;
            const int tl = (q >> 4) - chunk;
            return tl >= 0 && tl < 32 && (((unsigned)km >> tl) & 1u) != 0u;
        };
        // row r of [xx xy xz; xy yy yz; xz yz zz]
        const int k0 = r, k1 = r == 0 ? 1 : (r == 1 ? 3 : 4), k2 = r == 0 ? 2 : (r == 1 ? 4 : 5);
        const int s0 = t.start[a], deg = t.cnt[a];
        double* row = Sb + (size_t)c * ld;
        if (e == 15) {   // the joint's own block: + delta_m over all its member ends, summed above in list order
            const double acc[3] = {own[6 * a + k0], own[6 * a + k1], own[6 * a + k2]};
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int q = fi[3 * a + s];
                if (q >= 0 && stored(q) && acc[s] != 0.0) row[q] += acc[s];
            }
            continue;
        }
        for (int i = e; i < deg; i += 15) {   // the coupling block of the neighbour whose FIRST end this is
            const int other = oth[s0 + i];
            if (other < 0 || other == a) continue;
            if (i > 0 && oth[s0 + i - 1] == other) continue;   // (the lists are sorted by neighbour)
            double acc[3] = {0.0, 0.0, 0.0};
            for (int p = i; p < deg && oth[s0 + p] == other; ++p) {   // parallel members: side by side, in member-id order
                double v[6];
                delta(t.ends[s0 + p] >> 1, v);
                acc[0] -= v[k0];
                acc[1] -= v[k1];
                acc[2] -= v[k2];
            }
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int q = fi[3 * other + s];
                if (q >= 0 && stored(q) && acc[s] != 0.0) row[q] += acc[s];
            }
        }
    }
}

// (The batch's ld_f is ld_uf here.)
__global__ __launch_bounds__(256) void trs_nl_update_kernel(const TrsBatch bt, const double* __restrict__ uf,
                                                            const int* __restrict__ info, const int it,
                                                            double* __restrict__ U, int* __restrict__ st) {
    const int b = blockIdx.x, tid = threadIdx.x;
    if (st[4 * b] != TRS_NL_ACTIVE) return;   // (uniform over the work-group; only thread 0 writes it, behind the barrier)
    const int pivot = info[b];
    const bool ok = pivot == 0;
    __syncthreads();
    if (tid == 0) {
        if (ok) {
            st[4 * b + 1] = it;
        } else {
            st[4 * b] = TRS_NL_NOT_PD;
            st[4 * b + 2] = pivot;   // (latched: later factorisations of the frozen tangent do not count)
        }
    }
    if (!ok) return;
    const TrussView tr = bt.truss(b);
    for (int d = tid; d < tr.ndof; d += 256) {
        const int r = tr.row_of(d);
        if (r < 0) continue;
        double* u = U + (size_t)b * tr.ndof_max + d;
        const double du = uf[(size_t)b * bt.ld_f + r];
        *u = *u == 0.0 ? du : *u + du;   // (0 + du is du, bits and all: the first iterate is the substitution's output)
    }
}

int nl_state_launch(int B, const TrsBatch& bt, const double* loads, double lambda, double tol, int it, int last, int step,
                    int S, const double* U, int* st, double* Xc, double* R, double* W, int* active, double* u, double* N,
                    double* f_ext, int* iters, int* status, double* residual, hipStream_t stream) {
    if (B < 0 || bt.nJ_max <= 0 || bt.nM_max < 0 || bt.ld_f < 0 || it < 0 || last < 0 || last > 2 || S < 1 || step < 0 ||
        step >= S)
        return (int)hipErrorInvalidValue;
    if (!(tol >= 0.0) || !U || !st || !Xc || !R || !W || !active) return (int)hipErrorInvalidValue;
    if (last && (!u || !N || !f_ext || !iters || !status || !residual)) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!trs_nl_fits(bt.nJ_max, bt.nM_max)) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_nl_state_kernel>();
    hipLaunchKernelGGL(trs_nl_state_kernel, dim3(B), dim3(256), state_lds(bt.nJ_max, bt.nM_max), stream, bt, loads, lambda,
                       tol, it, last, step, S, U, st, Xc, R, W, active, u, N, f_ext, iters, status, residual);
    return (int)hipGetLastError();
}

// (bt.ld_f = slab_rows)
int nl_tangent_launch(int B, const TrsBatch& bt, int ld, double* S, const int* env, int flags, const double* W,
                      hipStream_t stream) {
    const int slab_rows = bt.ld_f;
    if (B < 0 || bt.nJ_max <= 0 || bt.nM_max < 0 || slab_rows <= 0 || slab_rows % TRS_NB != 0 || ld < slab_rows || !S || !W)
        return (int)hipErrorInvalidValue;
    if ((flags & TRS_ASM_COMPACT) != 0) return (int)hipErrorInvalidValue;   // (no slab to amend)
    if (B == 0) return 0;
    const size_t lds = tangent_lds(bt.nJ_max, bt.nM_max, slab_rows);
    if (lds > TRS_LDS_BYTES) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_nl_tangent_kernel>();
    hipLaunchKernelGGL(trs_nl_tangent_kernel, dim3(B), dim3(256), lds, stream, bt, ld, S, env,
                       (flags & TRS_ASM_FULL_SYMMETRIC) != 0 ? 1 : 0, W);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_nl_abi_version(void) { return TRS_NL_ABI_VERSION; }

int trs_nl_fits(int nJ_max, int nM_max) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535) return 0;
    return state_lds(nJ_max, nM_max) <= TRS_LDS_BYTES &&
           tangent_lds(nJ_max, nM_max, trs_round_up(3 * nJ_max < 1 ? 1 : 3 * nJ_max, TRS_NB)) <= TRS_LDS_BYTES;
}

int trs_nl_state(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, const double* A,
                 const double* loads, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                 const int32_t* nM, int ld_f, double lambda, double tol, int it, int last, int step, int S,
                 const double* U, int32_t* st, double* Xc, double* R, double* W, int32_t* active, double* u, double* N,
                 double* f_ext, int32_t* iters, int32_t* status, double* residual, const int32_t* joint_out,
                 void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nJ, nM,
                                  joint_out, ld_f);
    return nl_state_launch(B, bt, loads, lambda, tol, it, last, step, S, U, st, Xc, R, W, active, u, N, f_ext, iters,
                           status, residual, (hipStream_t)stream);
}

int trs_nl_state_tab(int B, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16, const uint8_t* type_idx,
                     const double* types, const double* loads, const int32_t* free_index, const int32_t* n_free,
                     const int32_t* nJ, const int32_t* nM, int ld_f, double lambda, double tol, int it, int last,
                     int step, int S, const double* U, int32_t* st, double* Xc, double* R, double* W, int32_t* active,
                     double* u, double* N, double* f_ext, int32_t* iters, int32_t* status, double* residual,
                     const int32_t* joint_out, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, joint_out, ld_f);
    return nl_state_launch(B, bt, loads, lambda, tol, it, last, step, S, U, st, Xc, R, W, active, u, N, f_ext, iters,
                           status, residual, (hipStream_t)stream);
}

int trs_nl_tangent(int B, int nJ_max, int nM_max, const int32_t* conn, const double* E, const double* A,
                   const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM, int ld,
                   int slab_rows, double* S, const int32_t* env, int flags, const double* W, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, nullptr, trs_members_general(conn, E, A), free_index, n_free, nJ, nM,
                                  nullptr, slab_rows);
    return nl_tangent_launch(B, bt, ld, S, env, flags, W, (hipStream_t)stream);
}

int trs_nl_tangent_tab(int B, int nJ_max, int nM_max, const uint16_t* conn16, const uint8_t* type_idx,
                       const double* types, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                       const int32_t* nM, int ld, int slab_rows, double* S, const int32_t* env, int flags,
                       const double* W, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, nullptr, trs_members_table(conn16, type_idx, types), free_index, n_free,
                                  nJ, nM, nullptr, slab_rows);
    return nl_tangent_launch(B, bt, ld, S, env, flags, W, (hipStream_t)stream);
}

int trs_nl_update(int B, int nJ_max, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                  const double* uf, int ld_uf, const int32_t* info, int it, double* U, int32_t* st, void* stream) {
    if (B < 0 || nJ_max <= 0 || ld_uf < 0 || it < 1 || !uf || !info || !U || !st) return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    hipLaunchKernelGGL(trs_nl_update_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream,
                       trs_batch_dofs(nJ_max, free_index, n_free, nJ, nullptr, ld_uf), uf, info, it, U, st);
    return (int)hipGetLastError();
}

}  // extern "C"
