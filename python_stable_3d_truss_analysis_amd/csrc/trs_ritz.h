// trs_ritz.h - the Rayleigh-Ritz core that the two block iterations share (modes.hip: K phi = lambda M phi;
// buckling.hip: H phi = nu Kbar phi).  Both run ONE WAVE per truss on a block of 16 vectors and keep their 16 x 16
// reduced problem in the wave's LDS; what they have in common lives here, so a truss gets the same bits from either:
//   - the start block;
//   - on the 16 x 16 matrices in LDS: the symmetric part, the cyclic Jacobi in the round-robin order, the rank sort of
//     the eigenvalues;
//   - the end of a checking step: the residuals and the convergence vote;
//   - for the shapes kernels (one work-group of 256 per (truss, mode)): the component of largest magnitude.
// The Gram passes, the reduction to a standard problem (Cholesky there, deflation here), the rotation passes and the
// layout of the LDS differ and stay in their files.
#pragma once
#include "trs_common.h"

namespace trs_ritz {

constexpr int QB = 16;             // vectors per truss (TRS_MODES_BLOCK, TRS_BK_BLOCK)
constexpr int LP = QB + 1;         // padded leading dimension of the 16 x 16 matrices in LDS
constexpr int JACOBI_SWEEPS = 30;  // (a sweep without a rotation ends the loop; 6-9 are taken)

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// Entry (DOF c, vector k) of the start block: a hash of the pair, in (-1, 1).
__device__ __forceinline__ double start_value(int c, int k) {
    unsigned long long z = ((unsigned long long)c * QB + (unsigned long long)k + 1ULL) * 0x9e3779b97f4a7c15ULL;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) * (1.0 / 4503599627370496.0) - 1.0;
}

// Entry (i, j) of the symmetric part of A.
__device__ __forceinline__ double symmetric(const double (*A)[LP], int i, int j) { return 0.5 * (A[i][j] + A[j][i]); }

// Where jacobi16 keeps a round's rotations: 16 entries each, in the caller's LDS.
struct JacobiScratch {
    double *cs, *tn;
    int* partner;
};

// Cyclic Jacobi on the leading q x q part of the symmetric M, in the round-robin order (eight disjoint rotations per
// round: round r pairs 15 with r and (r + k) % 15 with (r - k) % 15, k = 1 .. 7), by the whole wave; the rotations are
// accumulated into W (the identity on entry).  On exit the diagonal of M holds the eigenvalues, unsorted.
__device__ __forceinline__ void jacobi16(double (*M)[LP], double (*W)[LP], const JacobiScratch R, const int q,
                                         const int lane) {
    const int li = lane & 15, lq = lane >> 4;
    double v[4], w[4];
    for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int round = 0; round < QB - 1; ++round) {
            if (lane < 8) {
                const int a = lane == 0 ? QB - 1 : (round + lane) % (QB - 1);
                const int c = lane == 0 ? round : (round + QB - 1 - lane) % (QB - 1);
                double cc = 1.0, ss = 0.0;
                if (a < q && c < q) {
                    const double app = M[a][a], aqq = M[c][c], apq = M[a][c];
                    if (fabs(apq) > 1.1102230246251565e-16 * sqrt(fabs(app * aqq)) && fabs(apq) > 0.0) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        cc = 1.0 / sqrt(1.0 + t * t);
                        ss = t * cc;
                        rotated = 1;
                    }
                }
                R.cs[a] = cc, R.tn[a] = -ss, R.partner[a] = c;
                R.cs[c] = cc, R.tn[c] = ss, R.partner[c] = a;
            }
            __syncthreads();
            const int pj = R.partner[li];
            const double cj = R.cs[li], tj = R.tn[li];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = lq + 4 * r, pi = R.partner[i];
                const double ci = R.cs[i], ti = R.tn[i];
                v[r] = ci * (cj * M[i][li] + tj * M[i][pj]) + ti * (cj * M[pi][li] + tj * M[pi][pj]);
                w[r] = cj * W[i][li] + tj * W[i][pj];
            }
            __syncthreads();
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                M[lq + 4 * r][li] = v[r];
                W[lq + 4 * r][li] = w[r];
            }
            __syncthreads();
        }
        if (!__any(rotated)) break;
    }
}

// order[rank] = lane for the lanes below q: the rank of val[lane] among val[0 .. q) by ascending key(val), ties by
// index (equal keys of two lanes give them different ranks, so order[0 .. q) is a permutation).
template <class Key>
__device__ __forceinline__ void rank_sort(const double* val, const int q, const int lane, int* order, Key key) {
    if (lane >= q) return;
    const double mine = key(val[lane]);
    int rank = 0;
    for (int j = 0; j < q; ++j) rank += (key(val[j]) < mine) | ((key(val[j]) == mine) & (j < lane));
    order[rank] = lane;
}

// The vote at the end of a checking step, by the whole wave.  num[r], den[r]: this lane's share of the squared residual
// and of its norm for vector lq + 4 r, summed over the 16 lanes of one lq in a fixed tree; resid[k] = sqrt(num / den)
// (NaN from vector q on).  True: the first n_modes residuals are all <= tol.
__device__ __forceinline__ bool step_converged(double (&num)[4], double (&den)[4], const int q, const int n_modes,
                                               const double tol, double* resid, const int lane) {
    const int li = lane & 15, lq = lane >> 4;
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            num[r] += __shfl_xor(num[r], off);
            den[r] += __shfl_xor(den[r], off);
        }
        const int k = lq + 4 * r;
        const double res = k < q ? sqrt(num[r] / den[r]) : quiet_nan();
        if (li == 0) resid[k] = res;
        bad |= (k < n_modes) & !(res <= tol);
    }
    return !__any(bad);
}

// The component of largest magnitude of the column x, by a work-group of 256: over the DOFs d < ndof with a reduced
// row row_of(d) >= 0, the first in the caller's DOF order place_of(d) on a tie - an exact, order-free reduction.
// Every thread gets the value (0 where no DOF has a row).
template <class RowOf, class PlaceOf>
__device__ __forceinline__ double largest_component(const double* __restrict__ x, const int ndof, const int tid,
                                                    RowOf row_of, PlaceOf place_of) {
    __shared__ double best_v[256];
    __shared__ int best_o[256];
    auto better = [](double v, int o, double bv, int bo) {
        return fabs(v) > fabs(bv) || (fabs(v) == fabs(bv) && o < bo);
    };
    double bv = 0.0;
    int bo = 0x7fffffff;
    for (int d = tid; d < ndof; d += 256) {
        const int r = row_of(d);
        if (r < 0) continue;
        const int o = place_of(d);
        const double v = x[r];
        if (better(v, o, bv, bo)) bv = v, bo = o;
    }
    best_v[tid] = bv;
    best_o[tid] = bo;
    __syncthreads();
    for (int half = 128; half > 0; half >>= 1) {
        if (tid < half && better(best_v[tid + half], best_o[tid + half], best_v[tid], best_o[tid])) {
            best_v[tid] = best_v[tid + half];
            best_o[tid] = best_o[tid + half];
        }
        __syncthreads();
    }
    return best_v[0];
}

}  // namespace trs_ritz
