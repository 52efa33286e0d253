// Natural frequencies and mode shapes from the resident factor (include/trs_modes.h): block inverse iteration with a
// lumped mass matrix.  The solves Y = inv(K_ff) (M X) are trs_potrs_cases (cases.hip) on a block of 16 vectors - one
// MFMA case group; this file holds what goes around them:
//
//   trs_modes_mass     lumped masses of the free DOFs, reduced numbering, and the number of DOFs with mass
//   trs_modes_step     one Rayleigh-Ritz step per truss: Gram matrices, the 16 x 16 reduced eigenproblem, X <- Y Q,
//                      F <- M X, Ritz values, residuals, freezing of the converged trusses
//   trs_modes_shapes   the delivered columns of X in the caller's joint numbering, sign fixed
//
// trs_modes_step: ONE WAVE per truss, no barrier between waves, every sum in one fixed order.  X and F are
// vector-major ([16][ld_f]), so along the DOF axis every vector is contiguous:
//   pass 1  K_r = Y^T (M X), M_r = Y^T (M Y): lane (li = l & 15, lq = l >> 4) reads FOUR CONSECUTIVE doubles of vector
//           li at DOF 16 t + 4 lq (one 32-byte load; a wave covers 16 x 128 contiguous bytes) from Y and X and the same
//           four masses.  The k index of the MFMA is only summed over, so slice s of chunk t is taken to be the DOFs
//           16 t + 4 k + s (k = lq): the value a lane loaded is then BOTH its A element (vector li, k = lq) and, times
//           the mass, its B element (k = lq, vector li) - no transposition, no strided read.
//   reduced problem in LDS: Cholesky M_r = L L^T, C = inv(L) K_r inv(L)^T, cyclic Jacobi in the round-robin order
//           (eight disjoint rotations per round), ascending rank sort, Q = inv(L)^T W.
//   pass 2  X^T <- Q^T Y^T: A = Q^T (four registers for the whole pass), B element (k = lq, DOF li) of slice s is
//           Y[vector 4 s + lq][16 t + li], and D holds (vector lq + 4 r, DOF 16 t + li): loads and stores of a wave are
//           four runs of 128 contiguous bytes.  On a checking step X Q is formed the same way for the residuals.
#include "../../include/trs_modes.h"
#include "trs_common.h"
#include "trs_lds.h"
#include "trs_ritz.h"

namespace {

using namespace trs_rec;
using namespace trs_ritz;

static_assert(QB == TRS_MODES_BLOCK, "the block of trs_modes.h is the one of trs_ritz.h");

// ---- lumped mass ----------------------------------------------------------------------------------------------------
// One work-group per truss.  Half the mass of every member and its end joints go to LDS, then one thread per joint
// walks the members in id order and sums the halves that end at its joint.
struct MassTables {
    double* half;   // [nM_max]  half the mass of every member
    int2* ends;     // [nM_max]  its end joints
    int* count;     // [1]       DOFs with mass (no static LDS beside the dynamic part)
};

template <class Arena>
__host__ __device__ inline MassTables mass_layout(Arena& a, int nM_max) {
    MassTables t;
    t.half = a.template take<double>(nM_max);
    t.ends = a.template take<int2>(nM_max);
    t.count = a.template take<int>(1);
    return t;
}

// (The batch's joint_out slot holds joint_in here: the same map, read the other way.)
__global__ __launch_bounds__(256) void trs_modes_mass_kernel(const TrsBatch bt, const double* __restrict__ joint_mass,
                                                             const double mass_scale, double* __restrict__ Mf,
                                                             int* __restrict__ n_mass) {
    extern __shared__ double sh[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    trs_lds::Carve lds(sh);
    const MassTables t = mass_layout(lds, bt.nM_max);
    double* half = t.half;
    int2* ends = t.ends;
    int& count = *t.count;
    double* mf = Mf + (size_t)b * bt.ld_f;
    const int n = v.nfree, npad = min(trs_round_up(n, TRS_NB), bt.ld_f);
    if (tid == 0) count = 0;
    for (int m = tid; m < v.members; m += 256) {
        const int2 c = v.ends(m).c;
        const MemberGeom g = member_geom(v.X, c.x, c.y);
        ends[m] = v.raw_ends(m);   // (compared with joint ids, never an index)
        half[m] = 0.5 * (v.mem.area(v.mbase + m) * g.len * v.mem.density(v.mbase + m));
    }
    for (int c = n + tid; c < npad; c += 256) mf[c] = 0.0;
    __syncthreads();
    int with_mass = 0;
    for (int j = tid; j < v.joints; j += 256) {
        double sum = 0.0;
        for (int m = 0; m < v.members; ++m) {
            const int2 c = ends[m];
            if (c.x == j) sum += half[m];
            if (c.y == j) sum += half[m];
        }
        double mj = mass_scale * sum;
        if (joint_mass != nullptr) mj += joint_mass[(size_t)b * bt.nJ_max + v.place(j)];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int row = v.row_of(3 * j + a);
            if (row >= 0) {
                mf[row] = mj;
                with_mass += mj > 0.0;
            }
        }
    }
    if (with_mass) atomicAdd(&count, with_mass);  // (integer: exact in any order)
    __syncthreads();
    if (tid == 0) n_mass[b] = count;
}

// ---- the Rayleigh-Ritz step (the pieces shared with buckling.hip: trs_ritz.h) ----------------------------------------
struct ReducedLds {
    double K[QB][LP];   // K_r, then C = inv(L) K_r inv(L)^T, then the rotated C
    double M[QB][LP];   // M_r, eliminated in place
    double L[QB][LP];   // Cholesky factor of M_r (lower)
    double W[QB][LP];   // Jacobi rotations accumulated
    double Q[QB][LP];   // inv(L)^T W, columns in ascending order of the Ritz values
    double cs[QB], tn[QB], theta[QB], lam[QB];
    int partner[QB], order[QB];
};

// The q x q generalised eigenproblem K_r Q = M_r Q Lambda of one truss (q <= 16; the rest of Q is zero), by the whole
// wave.  In: R.K, R.M (as the accumulators left them).  Out: R.Q, R.lam (NaN beyond q).
__device__ void reduced_eigenproblem(ReducedLds& R, const int q, const int lane) {
    const int li = lane & 15, lq = lane >> 4;
    double v[4], w[4];
    // symmetric parts, restricted to q x q
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        const bool in = (i < q) & (li < q);
        v[r] = in ? symmetric(R.K, i, li) : 0.0;
        w[r] = in ? symmetric(R.M, i, li) : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        R.K[i][li] = v[r];
        R.M[i][li] = w[r];
        R.W[i][li] = i == li ? 1.0 : 0.0;
        R.Q[i][li] = 0.0;
        R.L[i][li] = 0.0;
    }
    __syncthreads();
    // right-looking elimination of M_r: step j touches (i, k) with i, k > j and reads row / column j only
    for (int j = 0; j < q; ++j) {
        const double d = R.M[j][j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = lq + 4 * r;
            if (i > j && li > j && i < q && li < q) R.M[i][li] -= R.M[i][j] * R.M[j][li] / d;
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        if (li <= i && i < q) R.L[i][li] = R.M[i][li] / sqrt(R.M[li][li]);  // (a pivot <= 0 gives NaN: reported as such)
    }
    __syncthreads();
    // C = inv(L) K_r inv(L)^T: columns first (lane k owns column k), then rows (lane i owns row i), in place
    if (lane < q) {
        for (int i = 0; i < q; ++i) {
            double t = R.K[i][lane];
            for (int j = 0; j < i; ++j) t -= R.L[i][j] * R.K[j][lane];
            R.K[i][lane] = t / R.L[i][i];
        }
    }
    __syncthreads();
    if (lane < q) {
        for (int k = 0; k < q; ++k) {
            double t = R.K[lane][k];
            for (int j = 0; j < k; ++j) t -= R.K[lane][j] * R.L[k][j];
            R.K[lane][k] = t / R.L[k][k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = symmetric(R.K, lq + 4 * r, li);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) R.K[lq + 4 * r][li] = v[r];
    __syncthreads();
    jacobi16(R.K, R.W, {R.cs, R.tn, R.partner}, q, lane);
    // ascending order (ties by index), then Q = inv(L)^T W[:, order]
    if (lane < QB) R.theta[lane] = lane < q ? R.K[lane][lane] : 0.0;
    __syncthreads();
    if (lane < QB) {
        R.lam[lane] = quiet_nan();
        rank_sort(R.theta, q, lane, R.order, [](double x) { return x; });
    }
    __syncthreads();
    if (lane < q) {
        const int src = R.order[lane];
        R.lam[lane] = R.theta[src];
        for (int i = q - 1; i >= 0; --i) {
            double t = R.W[i][src];
            for (int j = i + 1; j < q; ++j) t -= R.L[j][i] * R.Q[j][lane];
            R.Q[i][lane] = t / R.L[i][i];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void trs_modes_step_kernel(const int p, const int* __restrict__ n_free,
                                                            const int* __restrict__ n_mass,
                                                            const double* __restrict__ Mf_all, double* F_all,
                                                            double* X_all, const int ld_f, double* __restrict__ lam_all,
                                                            double* __restrict__ resid_all, int* __restrict__ state,
                                                            const int first, const int check, const int iter,
                                                            const double tol) {
    __shared__ ReducedLds R;
    const int b = blockIdx.x, lane = threadIdx.x, li = lane & 15, lq = lane >> 4;
    if (!first && state[b] != 0) return;  // frozen
    const int n = n_free[b], npad = trs_round_up(n, TRS_NB), nch = npad / 16;
    const int q = min(QB, n_mass[b]), n_modes = min(p, q);
    const double* mf = Mf_all + (size_t)b * ld_f;
    double* F = F_all + (size_t)b * QB * ld_f;
    double* X = X_all + (size_t)b * QB * ld_f;
    double* lam = lam_all + (size_t)b * QB;
    double* resid = resid_all + (size_t)b * QB;
    const double nan = quiet_nan();
    if (first) {
        // vector lq + 4 r, DOF 16 t + li: runs of 128 contiguous bytes
        for (int t = 0; t < nch; ++t) {
            const int c = 16 * t + li;
            const double m = mf[c];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = lq + 4 * r;
                const double x = (c < n && k < q) ? start_value(c, k) : 0.0;
                X[(size_t)k * ld_f + c] = x;
                F[(size_t)k * ld_f + c] = m * x;
            }
        }
        if (lane < QB) lam[lane] = nan, resid[lane] = nan;
        if (lane == 0) state[b] = 0;
        return;
    }
    // ---- pass 1: the Gram matrices
    d4 kacc = {0.0, 0.0, 0.0, 0.0}, macc = {0.0, 0.0, 0.0, 0.0};
    {
        const double* yp = F + (size_t)li * ld_f + 4 * lq;
        const double* xp = X + (size_t)li * ld_f + 4 * lq;
        const double* mp = mf + 4 * lq;
        for (int t = 0; t < nch; ++t) {
            const d4 y = *reinterpret_cast<const d4*>(yp + 16 * t);
            const d4 x = *reinterpret_cast<const d4*>(xp + 16 * t);
            const d4 m = *reinterpret_cast<const d4*>(mp + 16 * t);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                kacc = mfma_f64(y[s], m[s] * x[s], kacc);
                macc = mfma_f64(y[s], m[s] * y[s], macc);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        R.K[lq + 4 * r][li] = kacc[r];
        R.M[lq + 4 * r][li] = macc[r];
    }
    __syncthreads();
    reduced_eigenproblem(R, q, lane);
    // ---- pass 2: X <- Y Q, F <- M X (and, on a checking step, the residuals from X Q)
    double qa[4], lk[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        qa[s] = R.Q[4 * s + lq][li];   // A[k = li][j = 4 s + lq] = Q[j][k]
        lk[s] = R.lam[lq + 4 * s];     // Ritz value of this lane's output vectors
    }
    double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = 0; t < nch; ++t) {
        const int c = 16 * t + li;
        const double m = mf[c];
        double yb[4], xb[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) yb[s] = F[(size_t)(4 * s + lq) * ld_f + c];
        if (check) {
#pragma unroll
            for (int s = 0; s < 4; ++s) xb[s] = X[(size_t)(4 * s + lq) * ld_f + c];
        }
        d4 phi = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int s = 0; s < 4; ++s) phi = mfma_f64(qa[s], yb[s], phi);
        if (check) {
            d4 xq = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int s = 0; s < 4; ++s) xq = mfma_f64(qa[s], xb[s], xq);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double lp = lk[r] * phi[r], e = xq[r] - lp;
                num[r] += m * (e * e);
                den[r] += m * (lp * lp);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            X[(size_t)(lq + 4 * r) * ld_f + c] = phi[r];
            F[(size_t)(lq + 4 * r) * ld_f + c] = m * phi[r];
        }
    }
    if (lane < QB) lam[lane] = R.lam[lane];
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
// tie - decides the sign (an exact, order-free reduction), then the column goes out through free_index and joint_out.
__global__ __launch_bounds__(256) void trs_modes_shapes_kernel(const TrsBatch bt, const int p,
                                                               const double* __restrict__ X_all,
                                                               double* __restrict__ phi) {
    const int b = blockIdx.x / p, k = blockIdx.x - b * p, tid = threadIdx.x;
    const TrussView v = bt.truss(b);
    const double* x = X_all + ((size_t)b * QB + k) * bt.ld_f;
    double* out = phi + (size_t)blockIdx.x * v.ndof_max;
    const bool flip = largest_component(x, v.ndof, tid, [&](int d) { return v.row_of(d); },
                                        [&](int d) { return v.place_dof(d); }) < 0.0;
    for (int d = tid; d < v.ndof_max; d += 256) {
        const int r = v.row_of(d);
        const double val = r >= 0 ? x[r] : 0.0;
        out[v.place_dof(d)] = (flip && r >= 0) ? -val : val;
    }
}

size_t modes_mass_lds(int nM_max) { return trs_lds::count([&](auto& a) { mass_layout(a, nM_max); }); }

int modes_mass_launch(int B, const TrsBatch& bt, const double* joint_mass, double mass_scale, double* Mf, int* n_mass,
                      hipStream_t stream) {
    if (B <= 0) return 0;
    if (!trs_modes_fits(bt.nJ_max, bt.nM_max)) return (int)hipErrorInvalidValue;
    trs_lds::raise_lds_once<trs_modes_mass_kernel>();
    hipLaunchKernelGGL(trs_modes_mass_kernel, dim3(B), dim3(256), modes_mass_lds(bt.nM_max), stream, bt, joint_mass,
                       mass_scale, Mf, n_mass);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_modes_abi_version(void) { return TRS_MODES_ABI_VERSION; }

int trs_modes_fits(int nJ_max, int nM_max) {
    return nJ_max >= 0 && nM_max >= 0 && modes_mass_lds(nM_max) <= TRS_LDS_BYTES;
}

int trs_modes_mass(int B, int nJ_max, int nM_max, const double* xyz, const int32_t* conn, const double* A,
                   const double* rho, const double* joint_mass, const int32_t* joint_in, double mass_scale,
                   const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM, double* Mf,
                   int ld_f, int32_t* n_mass, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, nullptr, A, rho), free_index, n_free, nJ,
                                  nM, joint_in, ld_f);
    return modes_mass_launch(B, bt, joint_mass, mass_scale, Mf, n_mass, (hipStream_t)stream);
}

int trs_modes_tab_mass(int B, int nJ_max, int nM_max, const double* xyz, const uint16_t* conn16, const uint8_t* type_idx,
                       const double* types, const double* joint_mass, const int32_t* joint_in, double mass_scale,
                       const int32_t* free_index, const int32_t* n_free, const int32_t* nJ, const int32_t* nM,
                       double* Mf, int ld_f, int32_t* n_mass, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, n_free, nJ,
                                  nM, joint_in, ld_f);
    return modes_mass_launch(B, bt, joint_mass, mass_scale, Mf, n_mass, (hipStream_t)stream);
}

int trs_modes_step(int B, int p, const int32_t* n_free, const int32_t* n_mass, const double* Mf, double* F, double* X,
                   int ld_f, double* lam, double* resid, int32_t* state, int first, int check, int iter, double tol,
                   void* stream) {
    if (B <= 0) return 0;
    if (p < 1 || p > QB || ld_f < TRS_NB || ld_f % 4 != 0 || (!first && iter < 1)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(trs_modes_step_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, p, n_free, n_mass, Mf, F, X,
                       ld_f, lam, resid, state, first, check, iter, tol);
    return (int)hipGetLastError();
}

int trs_modes_shapes(int B, int p, int nJ_max, const double* X, int ld_f, const int32_t* free_index, const int32_t* nJ,
                     const int32_t* joint_out, double* phi, void* stream) {
    if (B <= 0 || p <= 0) return 0;
    if (p > QB) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(trs_modes_shapes_kernel, dim3((unsigned)B * (unsigned)p), dim3(256), 0, (hipStream_t)stream,
                       trs_batch_dofs(nJ_max, free_index, nullptr, nJ, joint_out, ld_f), p, X, phi);
    return (int)hipGetLastError();
}

}  // extern "C"
