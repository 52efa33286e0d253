// Linear buckling: critical load factors from shifted factors of K + theta Kg (include/trs_buckling.h).  The assembly,
// the amendment of the slab (trs_nl_tangent with the table W), the factorisation and the solves Y = inv(Kbar) F
// (trs_potrs_cases on a block of 16 vectors) are used as they are; this file holds what goes around them:
//
//   trs_bk_members   the reference state: N, the member table (n, g = N / L0) and W(theta) for trs_nl_tangent
//   trs_bk_product   G = H Y, H = -Kg, for the 16 vectors: owner-computes by joint over the member-end lists
//   trs_bk_step      one step per truss: A_r = Y^T G, B_r = Y^T Fk, deflation of B_r, the reduced eigenproblem,
//                    X <- Y Q, F <- G Q, lam = theta + 1 / nu, residuals, freezing of the converged trusses
//   trs_bk_shapes    the delivered columns of X in the caller's joint numbering, largest component +1
//
// The mathematics, per member m with ends j0, j1: N_m the linear member force (trs_rec::member_axial), g_m = N_m / L0_m,
// n_m the undeformed direction; Kg is g_m (I - n n^T), + on the two diagonal joint blocks and - on the off-diagonal ones;
// K_ff phi = lambda H phi with H = -Kg; with Kbar = K_ff + theta Kg positive definite the iteration runs on
// H phi = nu Kbar phi and lambda = theta + 1 / nu.
//
// trs_bk_step: ONE WAVE per truss, shaped after trs_modes_step (modes.hip; what the two share is trs_ritz.h): pass 1
// forms the two Gram matrices with the value a lane loaded serving as A element of Y and as B element of G / Fk; the
// reduced problem lives in the wave's LDS; pass 2 rotates Y, G (and, on a checking step, Fk) by Q^T, each lane reading
// and writing its own elements only.
#include "../../include/trs_buckling.h"
#include "trs_common.h"
#include "trs_lds.h"
#include "trs_ritz.h"

namespace {

using namespace trs_rec;
using namespace trs_ritz;

static_assert(QB == TRS_BK_BLOCK, "the block of trs_buckling.h is the one of trs_ritz.h");
constexpr double BK_DEFLATE = 9.094947017729282e-13;   // 2^-40

// ---- the reference state --------------------------------------------------------------------------------------------
struct MemberTables { double* u; };   // [3 nJ_max] u in joint layout

template <class Arena>
__host__ __device__ inline MemberTables members_layout(Arena& a, int nJ_max) {
    return MemberTables{a.template take<double>(3, nJ_max)};
}

size_t members_lds(int nJ_max) { return trs_lds::count([&](auto& a) { members_layout(a, nJ_max); }); }

// (The batch's ld_f is ld_uf here.)
__global__ __launch_bounds__(256) void trs_bk_members_kernel(const TrsBatch bt, const double* __restrict__ uf,
                                                             const double* __restrict__ theta_all,
                                                             double* __restrict__ N_out, int* __restrict__ ends_out,
                                                             double* __restrict__ Mt, double* __restrict__ W) {
    extern __shared__ double sh[];
    trs_lds::Carve lds(sh);
    double* u = members_layout(lds, bt.nJ_max).u;
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int nM_max = bt.nM_max;
    const size_t mbase = v.mbase;
    const double theta = theta_all != nullptr ? theta_all[b] : 0.0;
    for (int d = tid; d < v.ndof_max; d += 256) {
        const int r = v.row_of(d);
        u[d] = r >= 0 ? uf[(size_t)b * bt.ld_f + r] : 0.0;
    }
    __syncthreads();
    for (int m = tid; m < nM_max; m += 256) {
        double* mt = Mt + (mbase + m) * 4;
        double* w = W + (mbase + m) * 6;
        int* e = ends_out + (mbase + m) * 2;
        if (m >= v.members) {
            N_out[mbase + m] = 0.0;
            e[0] = e[1] = -1;
#pragma unroll
            for (int a = 0; a < 4; ++a) mt[a] = 0.0;
#pragma unroll
            for (int a = 0; a < 6; ++a) w[a] = 0.0;
            continue;
        }
        const int2 raw = v.raw_ends(m), c = v.ends(m).c;   // (the ids go out as they are: the product tests them again)
        e[0] = raw.x;
        e[1] = raw.y;
        const MemberGeom geo = member_geom(v.X, c.x, c.y);
        const double N = member_axial(geo, v.mem.EA(mbase + m), u, c.x, c.y);
        const double g = N / geo.len;
        N_out[mbase + m] = N;
#pragma unroll
        for (int a = 0; a < 3; ++a) mt[a] = w[a] = geo.c[a];
        mt[3] = g;
        w[3] = -(theta * g);
        w[4] = theta * g;
        w[5] = N;
    }
}

// ---- G = H Y --------------------------------------------------------------------------------------------------------
struct ProductTables : EndLists {
    double* tab;   // [nM_max][4]      n, g
    double* ysh;   // [vc][3 nJ_max]   the vectors of this chunk in joint layout
    int* far;      // [2 nM_max]       the joint at the far end of every list entry
};

template <class Arena>
__host__ __device__ inline ProductTables product_layout(Arena& a, int nJ_max, int nM_max, int vc) {
    ProductTables t;
    t.tab = a.template take<double>((size_t)4 * nM_max);
    t.ysh = a.template take<double>((size_t)vc * 3 * nJ_max);
    trs_lds::take_end_lists(a, t, nJ_max, nM_max);
    t.far = a.template take<int>(2, nM_max);
    return t;
}

size_t product_lds(int nJ_max, int nM_max, int vc) {
    return trs_lds::count([&](auto& a) { product_layout(a, nJ_max, nM_max, vc); });
}

// the vectors staged at once: the largest of 16, 8, 4, 2, 1 that fits the LDS, 0: none does
int product_chunk(int nJ_max, int nM_max) {
    for (int vc = QB; vc >= 1; vc >>= 1)
        if (product_lds(nJ_max, nM_max, vc) <= TRS_LDS_BYTES) return vc;
    return 0;
}

// (The batch's members are the int32 end joints that trs_bk_members wrote, nothing else.)
__global__ __launch_bounds__(256) void trs_bk_product_kernel(const TrsBatch bt, const double* __restrict__ Mt,
                                                             const double* __restrict__ Y_all, double* __restrict__ G_all,
                                                             const int vc) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const int ld_f = bt.ld_f, joints = v.joints, members = v.members, ndof_max = v.ndof_max;
    const int n = v.nfree, npad = trs_round_up(n, TRS_NB);   // (ld_f is a multiple of TRS_NB)
    trs_lds::Carve lds(sh);
    const ProductTables t = product_layout(lds, bt.nJ_max, bt.nM_max, vc);
    double *tab = t.tab, *ysh = t.ysh;
    int* far = t.far;
    const size_t mbase = v.mbase;
    const double* Y = Y_all + (size_t)b * QB * ld_f;
    double* G = G_all + (size_t)b * QB * ld_f;
    build_end_lists(t, v, tid);
    order_by_neighbour(t, far, v, tid);
    for (int i = tid; i < 4 * members; i += 256) tab[i] = Mt[mbase * 4 + i];
    for (int i = tid; i < QB * (npad - n); i += 256) {
        const int k = i / (npad - n), c = n + i - k * (npad - n);
        G[(size_t)k * ld_f + c] = 0.0;
    }
    for (int v0 = 0; v0 < QB; v0 += vc) {
        __syncthreads();   // (the lists are sorted, the table is in place; the readers of the last chunk are done)
        for (int i = tid; i < vc * ndof_max; i += 256) {
            const int k = i / ndof_max, d = i - k * ndof_max;
            const int r = v.row_of(d);
            ysh[i] = r >= 0 ? Y[(size_t)(v0 + k) * ld_f + r] : 0.0;
        }
        __syncthreads();
        for (int i = tid; i < vc * joints; i += 256) {
            const int k = i / joints, j = i - k * joints;
            const int rows[3] = {v.row_of(3 * j), v.row_of(3 * j + 1), v.row_of(3 * j + 2)};
            if ((rows[0] & rows[1] & rows[2]) < 0) continue;   // a joint without a free DOF owns no row
            const double* yk = ysh + (size_t)k * ndof_max;
            const double yj[3] = {yk[3 * j], yk[3 * j + 1], yk[3 * j + 2]};
            double acc[3] = {0.0, 0.0, 0.0};
            const int s0 = t.start[j], deg = t.cnt[j];
            for (int e = 0; e < deg; ++e) {
                const int o = far[s0 + e];
                if (o < 0 || o == j) continue;
                const double* mt = tab + 4 * (t.ends[s0 + e] >> 1);
                const double dl[3] = {yj[0] - yk[3 * o], yj[1] - yk[3 * o + 1], yj[2] - yk[3 * o + 2]};
                const double pr = mt[0] * dl[0] + mt[1] * dl[1] + mt[2] * dl[2];
#pragma unroll
                for (int a = 0; a < 3; ++a) acc[a] -= mt[3] * (dl[a] - mt[a] * pr);
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (rows[a] >= 0) G[(size_t)(v0 + k) * ld_f + rows[a]] = acc[a];
        }
    }
}

// ---- the step (the start block, the Jacobi sweeps, the rank sort and the residual vote: trs_ritz.h) -----------------
struct ReducedLds {
    double A[QB][LP];   // A_r, then C = T^T A_r T, then the rotated C
    double B[QB][LP];   // B_r, rotated to diag(D); then A_r T
    double T[QB][LP];   // V_r D_r^-1/2, the kept directions in the leading columns
    double W[QB][LP];   // Jacobi rotations accumulated (V, then W)
    double Q[QB][LP];   // T W, columns in descending order of |nu|
    double cs[QB], tn[QB], d[QB], nu[QB];
    int partner[QB], place[QB], order[QB];
    int r;
};

// A_r Q = B_r Q diag(nu) of one truss with deflation, by the whole wave.  In: R.A, R.B (as the accumulators left them).
// Out: R.r, R.Q (columns >= r zero), R.nu (NaN beyond r), |nu| descending.
__device__ void reduced_eigenproblem(ReducedLds& R, const int lane) {
    const int li = lane & 15, lq = lane >> 4;
    const JacobiScratch scratch = {R.cs, R.tn, R.partner};
    double v[4], w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        v[r] = symmetric(R.A, lq + 4 * r, li);
        w[r] = symmetric(R.B, lq + 4 * r, li);
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        R.A[i][li] = v[r];
        R.B[i][li] = w[r];
        R.W[i][li] = i == li ? 1.0 : 0.0;
        R.T[i][li] = 0.0;
        R.Q[i][li] = 0.0;
    }
    __syncthreads();
    // B_r = V D V^T; the directions with D_k <= 2^-40 max D are dropped, the others keep their order
    jacobi16(R.B, R.W, scratch, QB, lane);
    if (lane < QB) R.d[lane] = R.B[lane][lane];
    __syncthreads();
    if (lane < QB) {
        double dmax = R.d[0];
        for (int k = 1; k < QB; ++k) dmax = R.d[k] > dmax ? R.d[k] : dmax;
        int place = 0, kept = 0;
        for (int k = 0; k < QB; ++k) {
            const int keep = R.d[k] > BK_DEFLATE * dmax;
            place += keep & (k < lane);
            kept += keep;
        }
        R.place[lane] = R.d[lane] > BK_DEFLATE * dmax ? place : -1;
        if (lane == 0) R.r = kept;
    }
    __syncthreads();
    const int q = R.r;
    {   // T[:, place[k]] = V[:, k] / sqrt(D_k)
        const int dst = R.place[li];
        if (dst >= 0) {
            const double s = 1.0 / sqrt(R.d[li]);
#pragma unroll
            for (int r = 0; r < 4; ++r) R.T[lq + 4 * r][dst] = R.W[lq + 4 * r][li] * s;
        }
    }
    __syncthreads();
    // C = T^T (A_r T): entry (i, j) by lane (li = j, lq + 4 r = i), sums over k ascending
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        double s = 0.0;
        for (int k = 0; k < QB; ++k) s += R.A[i][k] * R.T[k][li];
        v[r] = s;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) R.B[lq + 4 * r][li] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        double s = 0.0;
        for (int k = 0; k < QB; ++k) s += R.T[k][i] * R.B[k][li];
        v[r] = s;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) R.A[lq + 4 * r][li] = v[r];
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = symmetric(R.A, lq + 4 * r, li);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        R.A[i][li] = v[r];
        R.W[i][li] = i == li ? 1.0 : 0.0;
    }
    __syncthreads();
    jacobi16(R.A, R.W, scratch, q, lane);
    // |nu| descending (ties by index), then Q = T W[:, order]
    if (lane < QB) R.d[lane] = lane < q ? R.A[lane][lane] : 0.0;
    __syncthreads();
    if (lane < QB) {
        R.nu[lane] = quiet_nan();
        rank_sort(R.d, q, lane, R.order, [](double x) { return -fabs(x); });
    }
    __syncthreads();
    if (lane < q) R.nu[lane] = R.d[R.order[lane]];
    if (li < q) {
        const int src = R.order[li];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = lq + 4 * r;
            double s = 0.0;
            for (int k = 0; k < q; ++k) s += R.T[i][k] * R.W[k][src];
            R.Q[i][li] = s;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void trs_bk_step_kernel(const int p, const int* __restrict__ n_free,
                                                         const double* __restrict__ theta_all, double* F_all,
                                                         const double* __restrict__ G_all, double* Fk_all,
                                                         double* __restrict__ X_all, const int ld_f,
                                                         double* __restrict__ lam_all, double* __restrict__ resid_all,
                                                         int* __restrict__ rank_all, int* __restrict__ state,
                                                         const int first, const int check, const int iter,
                                                         const double tol) {
    __shared__ ReducedLds R;
    const int b = blockIdx.x, lane = threadIdx.x, li = lane & 15, lq = lane >> 4;
    const int st = state[b];
    if (!first && st != 0) return;  // frozen, or no part in this round
    const int n = min(max(n_free[b], 0), ld_f), npad = trs_round_up(n, TRS_NB), nch = npad / 16;
    double* F = F_all + (size_t)b * QB * ld_f;
    double* Fk = Fk_all + (size_t)b * QB * ld_f;
    const double* G = G_all + (size_t)b * QB * ld_f;
    double* X = X_all + (size_t)b * QB * ld_f;
    double* lam = lam_all + (size_t)b * QB;
    double* resid = resid_all + (size_t)b * QB;
    const double nan = quiet_nan();
    if (first) {
        // vector lq + 4 r, DOF 16 t + li: runs of 128 contiguous bytes
        const int q = min(QB, n);
        for (int t = 0; t < nch; ++t) {
            const int c = 16 * t + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = lq + 4 * r;
                const double x = (st == 0 && c < n && k < q) ? start_value(c, k) : 0.0;
                F[(size_t)k * ld_f + c] = x;
                if (st == 0) Fk[(size_t)k * ld_f + c] = x;
            }
        }
        if (st == 0) {
            if (lane < QB) lam[lane] = nan, resid[lane] = nan;
            if (lane == 0) rank_all[b] = 0;
        }
        return;
    }
    const double theta = theta_all != nullptr ? theta_all[b] : 0.0;
    // ---- pass 1: A_r = Y^T G, B_r = Y^T Fk
    d4 aacc = {0.0, 0.0, 0.0, 0.0}, bacc = {0.0, 0.0, 0.0, 0.0};
    {
        const double* yp = F + (size_t)li * ld_f + 4 * lq;
        const double* gp = G + (size_t)li * ld_f + 4 * lq;
        const double* fp = Fk + (size_t)li * ld_f + 4 * lq;
        for (int t = 0; t < nch; ++t) {
            const d4 y = *reinterpret_cast<const d4*>(yp + 16 * t);
            const d4 g = *reinterpret_cast<const d4*>(gp + 16 * t);
            const d4 f = *reinterpret_cast<const d4*>(fp + 16 * t);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                aacc = mfma_f64(y[s], g[s], aacc);
                bacc = mfma_f64(y[s], f[s], bacc);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        R.A[lq + 4 * r][li] = aacc[r];
        R.B[lq + 4 * r][li] = bacc[r];
    }
    __syncthreads();
    reduced_eigenproblem(R, lane);
    const int q = R.r, n_modes = min(p, q);
    // ---- pass 2: X <- Y Q, F <- G Q, Fk <- G Q (and, on a checking step, the residuals with Fk Q)
    double qa[4], nk[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qa[s] = R.Q[4 * s + lq][li];   // A[k = li][j = 4 s + lq] = Q[j][k]
        nk[s] = R.nu[lq + 4 * s];      // nu of this lane's output vectors
    }
    double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < nch; ++t) {
        const int c = 16 * t + li;
        double yb[4], gb[4], fb[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            yb[s] = F[(size_t)(4 * s + lq) * ld_f + c];
            gb[s] = G[(size_t)(4 * s + lq) * ld_f + c];
        }
        if (check) {
#pragma unroll
            for (int s = 0; s < 4; ++s) fb[s] = Fk[(size_t)(4 * s + lq) * ld_f + c];
        }
        d4 x = {0.0, 0.0, 0.0, 0.0}, gq = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            x = mfma_f64(qa[s], yb[s], x);
            gq = mfma_f64(qa[s], gb[s], gq);
        }
        if (check) {
            d4 fq = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s) fq = mfma_f64(qa[s], fb[s], fq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double nf = nk[r] * fq[r], e = gq[r] - nf;
                num[r] += e * e;
                den[r] += nf * nf;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            X[(size_t)(lq + 4 * r) * ld_f + c] = x[r];
            F[(size_t)(lq + 4 * r) * ld_f + c] = gq[r];
            Fk[(size_t)(lq + 4 * r) * ld_f + c] = gq[r];
        }
    }
    if (lane < QB) lam[lane] = lane < q ? theta + 1.0 / R.nu[lane] : nan;
    if (lane == 0) rank_all[b] = q;
    if (!check) return;
    if (!step_converged(num, den, q, n_modes, tol, resid, lane)) return;
    // converged: frozen from here on, and the substitutions that still run over this truss get zeros
    for (int t = 0; t < nch; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) F[(size_t)(lq + 4 * r) * ld_f + 16 * t + li] = 0.0;
    if (lane == 0) state[b] = iter;
}

// ---- shapes ---------------------------------------------------------------------------------------------------------
// One work-group per (truss, mode): the component of largest magnitude - the first in the caller's DOF order on a
// tie - becomes +1 (an exact, order-free reduction), then the column goes out through free_index and joint_out.
__global__ __launch_bounds__(256) void trs_bk_shapes_kernel(const TrsBatch bt, const int p,
                                                            const double* __restrict__ X_all,
                                                            const int* __restrict__ rank, double* __restrict__ phi) {
    const int b = blockIdx.x / p, k = blockIdx.x - b * p, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const bool delivered = k < min(p, rank[b]);
    const double* x = X_all + ((size_t)b * QB + k) * bt.ld_f;
    double* out = phi + (size_t)blockIdx.x * v.ndof_max;
    auto shape_row = [&](int d) { return delivered ? v.row_of(d) : -1; };   // (a mode that was not delivered: zeros)
    const double top = largest_component(x, v.ndof, tid, shape_row, [&](int d) { return v.place_dof(d); });
    for (int d = tid; d < v.ndof_max; d += 256) {
        const int r = shape_row(d);
        out[v.place_dof(d)] = (r >= 0 && top != 0.0) ? x[r] / top : 0.0;
    }
}

int bk_members_launch(int B, const TrsBatch& bt, const double* uf, const double* theta, double* N, int* ends, double* Mt,
                      double* W, hipStream_t stream) {
    if (B < 0 || bt.nJ_max <= 0 || bt.nM_max < 0 || bt.ld_f < 0 || !uf || !N || !ends || !Mt || !W)
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    if (!trs_bk_fits(bt.nJ_max, bt.nM_max)) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_bk_members_kernel>();
    hipLaunchKernelGGL(trs_bk_members_kernel, dim3(B), dim3(256), members_lds(bt.nJ_max), stream, bt, uf, theta, N, ends,
                       Mt, W);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_bk_abi_version(void) { return TRS_BK_ABI_VERSION; }

int trs_bk_fits(int nJ_max, int nM_max) {
    if (nJ_max < 0 || nM_max < 0 || nJ_max > 65535) return 0;
    return members_lds(nJ_max) <= TRS_LDS_BYTES && product_chunk(nJ_max, nM_max) >= 1;
}

int trs_bk_members(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* E, const double* A,
                   const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
                   const double* uf, int ld_uf, const double* theta, double* N, int32_t* ends, double* Mt, double* W,
                   void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, A), free_index, n_free, nJ, nM,
                                  nullptr, ld_uf);
    return bk_members_launch(B, bt, uf, theta, N, ends, Mt, W, (hipStream_t)stream);
}

int trs_bk_members_tab(int B, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16, const uint8_t* type_idx,
                       const double* types, const int32_t* free_index, const int32_t* n_free, const int32_t* nJ,
                       const int32_t* nM, const double* uf, int ld_uf, const double* theta, double* N, int32_t* ends,
                       double* Mt, double* W, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, nullptr, ld_uf);
    return bk_members_launch(B, bt, uf, theta, N, ends, Mt, W, (hipStream_t)stream);
}

int trs_bk_product(int B, int nJ_max, int nM_max, const int32_t* ends, const double* Mt, const int32_t* free_index,
                   const int32_t* n_free, const int32_t* nJ, const int32_t* nM, const double* Y, double* G, int ld_f,
                   void* stream) {
    if (B < 0 || nJ_max <= 0 || nM_max < 0 || ld_f < TRS_NB || ld_f % TRS_NB != 0 || !ends || !Mt || !Y || !G)
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    const int vc = nJ_max <= 65535 ? product_chunk(nJ_max, nM_max) : 0;
    if (vc < 1) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_bk_product_kernel>();
    const TrsBatch bt = trs_batch(nJ_max, nM_max, nullptr, trs_members_general(ends, nullptr, nullptr), free_index, n_free,
                                  nJ, nM, nullptr, ld_f);
    hipLaunchKernelGGL(trs_bk_product_kernel, dim3(B), dim3(256), product_lds(nJ_max, nM_max, vc), (hipStream_t)stream, bt,
                       Mt, Y, G, vc);
    return (int)hipGetLastError();
}

int trs_bk_step(int B, int p, const int32_t* n_free, const double* theta, double* F, const double* G, double* Fk,
                double* X, int ld_f, double* lam, double* resid, int32_t* rank, int32_t* state, int first, int check,
                int iter, double tol, void* stream) {
    if (B < 0 || p < 1 || p > QB || ld_f < TRS_NB || ld_f % TRS_NB != 0 || (!first && iter < 1) || !F || !Fk || !lam ||
        !resid || !rank || !state || (!first && (!G || !X)))
        return (int)hipErrorInvalidValue;
    if (B == 0) return 0;
    hipLaunchKernelGGL(trs_bk_step_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, p, n_free, theta, F, G, Fk, X,
                       ld_f, lam, resid, rank, state, first, check, iter, tol);
    return (int)hipGetLastError();
}

int trs_bk_shapes(int B, int p, int nJ_max, const double* X, int ld_f, const int32_t* free_index, const int32_t* n_free,
                  const int32_t* nJ, const int32_t* rank, const int32_t* joint_out, double* phi, void* stream) {
    if (B < 0 || p < 0 || p > QB || nJ_max <= 0 || ld_f < 0 || !X || !rank || !phi) return (int)hipErrorInvalidValue;
    if (B == 0 || p == 0) return 0;
    hipLaunchKernelGGL(trs_bk_shapes_kernel, dim3((unsigned)B * (unsigned)p), dim3(256), 0, (hipStream_t)stream,
                       trs_batch_dofs(nJ_max, free_index, n_free, nJ, joint_out, ld_f), p, X, rank, phi);
    return (int)hipGetLastError();
}

}  // extern "C"
