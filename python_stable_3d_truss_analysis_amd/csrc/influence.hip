// Influence lines and moving-load envelopes (include/trs_influence.h): the column z_m = inv(K_ff) b_m,f that the
// member-loss analysis forms (trs_loss_rhs, trs_potrs_cases, as they are) is, times k_m, the influence line of
// N_m for a unit load at every joint in every direction (Maxwell / Mueller-Breslau).  The one kernel here reads those
// columns along a path, sweeps a load train over it and keeps the extremes.
//
//   eta[m][p]  = k_m (d . z_m at joint path[p])
//   N_m(p, a)  = sum_a' w_a' eta_m(s_p + (o_a - o_a'))       the candidate with axle a on path joint p
//   N_max, N_min and the lead positions s_p + o_a that attain them; the areas of the positive and the negative part
//
// The kernel is one work-group of four waves per (truss, slice of the chunk).  Staged in LDS once per work-group: the
// inverse of joint_out, the path translated through it, the arc lengths s_p, per path joint the (reduced index, weight)
// pairs of d through free_index, and the train.  Every wave then takes one member at a time: its 3 P entries of the Z
// row go, dotted with d and scaled by k_m, into an eta vector of the wave's own; the lanes run over the P A candidates,
// every other axle's segment found by binary search on the s_p; a wave reduction that carries the candidate index with
// the value closes max and min (the values are compared as numbers: +0 and -0 count as equal, a NaN never wins); the
// areas are summed segment by segment in ascending p.  Max and min are exact and every other number is one fixed
// expression of staged values: the result of (b, m) does not depend on the chunk, the slice, B or the member form.
#include "../../include/trs_influence.h"
#include "trs_columns.h"
#include "trs_common.h"
#include "trs_recover.h"

#include <limits.h>
#include <math.h>

namespace {

using namespace trs_rec;
using trs_col::wave_extreme_index;

constexpr int WAVES = 4;                    // waves per work-group; trs_influence_fits' rule counts their eta vectors
#ifndef TRS_INFLUENCE_SLICE
#define TRS_INFLUENCE_SLICE 16              // members per work-group
#endif

// LDS tables of the apply kernel
struct InfluenceTables {
    double* s;        // [P_max]      arc length of path joint p
    double* dw;       // [3 P_max]    d's component on axis a of path joint p
    double* eta;      // [WAVES][P_max]
    double *tw, *to;  // [A] each
    int* pj;          // [P_max]      the path in the solver's numbering
    int* di;          // [3 P_max]    reduced index of that DOF, -1 = held
    int* inv;         // [nJ_max]     caller's joint id -> solver's
};

template <class Arena>
__host__ __device__ inline InfluenceTables layout(Arena& a, int nJ_max, int P_max, int A) {
    InfluenceTables t;
    t.s = a.template take<double>((size_t)P_max);
    t.dw = a.template take<double>((size_t)3 * P_max);
    t.eta = a.template take<double>((size_t)WAVES * P_max);
    t.tw = a.template take<double>((size_t)A);
    t.to = a.template take<double>((size_t)A);
    t.pj = a.template take<int>((size_t)P_max);
    t.di = a.template take<int>((size_t)3 * P_max);
    t.inv = a.template take<int>((size_t)nJ_max);
    return t;
}

size_t influence_lds(int nJ_max, int P_max, int A) {
    return trs_lds::count([&](auto& a) { layout(a, nJ_max, P_max, A); });
}

// eta_m at arc position t of a path of P >= 1 joints (s: its arc lengths, S = s[P - 1], eps = 1e-12 S), 0 off the path
__device__ __forceinline__ double line_at(const double* s, const double* eta, const int P, const double S,
                                          const double eps, double t) {
    if (t < -eps || t > S + eps) return 0.0;
    if (P == 1) return eta[0];
    t = fmin(fmax(t, 0.0), S);
    int lo = 0, hi = P - 1;   // s[lo] <= t, and t < s[hi] or hi = P - 1
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (s[mid] <= t) lo = mid;
        else hi = mid;
    }
    if (t == s[lo + 1]) return eta[lo + 1];   // (t = S: on the last joint, its ordinate itself, not lam = 1 rounded)
    const double lam = (t - s[lo]) / (s[lo + 1] - s[lo]);
    return fma(lam, eta[lo + 1] - eta[lo], eta[lo]);
}

__global__ __launch_bounds__(64 * WAVES) void trs_influence_apply_kernel(
    const TrsBatch bt, const int e0, const int C, const int slice, const int P_max, const int A,
    const int* __restrict__ path, const int* __restrict__ path_len, const double* __restrict__ dir,
    const double* __restrict__ train_w, const double* __restrict__ train_o, const double* __restrict__ Z,
    double* __restrict__ eta_out, double* __restrict__ nmax_out, double* __restrict__ nmin_out,
    double* __restrict__ xmax_out, double* __restrict__ xmin_out, double* __restrict__ apos_out,
    double* __restrict__ aneg_out) {
    extern __shared__ double sh[];
    const int slices = (C + slice - 1) / slice;   // work-groups per truss
    const int b = blockIdx.x / slices, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the members of this work-group: first <= m < last (inside the chunk and inside the arrays)
    const int first = e0 + (blockIdx.x - b * slices) * slice;
    const int last = min(min(first + slice, e0 + C), bt.nM_max);
    if (first >= last) return;
    const TrussView tr = bt.truss(b);
    const int joints = tr.joints, members = tr.members, ld_f = bt.ld_f;
    const int P = joints > 0 ? max(0, min(path_len[b], P_max)) : 0;
    trs_lds::Carve lds(sh);
    const InfluenceTables t = layout(lds, bt.nJ_max, P_max, A);
    const size_t mbase = tr.mbase;
    const double* __restrict__ X = tr.X;
    double* ew = t.eta + (size_t)wave * P_max;
    const double nan = __builtin_nan("");

    // once per work-group: the inverse joint order, the train, the path with its DOF pairs and arc lengths
    for (int j = tid; j < joints; j += 64 * WAVES) t.inv[j] = 0;
    for (int a = tid; a < A; a += 64 * WAVES) {
        t.tw[a] = train_w[a];
        t.to[a] = train_o[a];
    }
    __syncthreads();
    for (int j = tid; j < joints; j += 64 * WAVES) {
        const int id = tr.place(j);
        if (id < joints) t.inv[id] = j;
    }
    __syncthreads();
    for (int p = tid; p < P; p += 64 * WAVES) {
        const int id = min(max(path[(size_t)b * P_max + p], 0), joints - 1);
        const int j = t.inv[id];
        t.pj[p] = j;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            t.di[3 * p + a] = tr.row_of(3 * j + a);
            t.dw[3 * p + a] = dir[(size_t)b * 3 + a];
        }
    }
    __syncthreads();
    for (int p = tid; p < P; p += 64 * WAVES) {   // the segment lengths, then one lane's ascending sum over them
        double h = 0.0;
        if (p > 0) {
            const int j = t.pj[p], i = t.pj[p - 1];
            const double dx = X[3 * j] - X[3 * i], dy = X[3 * j + 1] - X[3 * i + 1], dz = X[3 * j + 2] - X[3 * i + 2];
            h = sqrt(fma(dz, dz, fma(dy, dy, dx * dx)));
        }
        t.s[p] = h;
    }
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int p = 0; p < P; ++p) {
            run = p > 0 ? run + t.s[p] : 0.0;
            t.s[p] = run;
        }
    }
    __syncthreads();
    const double S = P > 0 ? t.s[P - 1] : 0.0, eps = 1e-12 * S;
    const int cands = P * A;

    for (int m = first + wave; m < last; m += WAVES) {
        const size_t o = mbase + m;
        double* line = eta_out != nullptr ? eta_out + o * P_max : nullptr;
        if (m >= members || P == 0) {   // a padding member, or no path: zeros, no position
            if (lane == 0) {
                nmax_out[o] = 0.0;
                nmin_out[o] = 0.0;
                xmax_out[o] = nan;
                xmin_out[o] = nan;
                apos_out[o] = 0.0;
                aneg_out[o] = 0.0;
            }
            if (line != nullptr)
                for (int p = lane; p < P_max; p += 64) line[p] = 0.0;
            continue;
        }
        // k_m as the member-loss kernel forms it (every lane: broadcast reads)
        const int2 c = tr.ends(m).c;
        const MemberGeom mg = member_geom(X, c.x, c.y);
        const double km = tr.mem.EA(o) / mg.len;
        // eta of this member along the path (this wave's own vector: written and read by this wave only)
        const double* zm = Z + ((size_t)b * C + (m - e0)) * ld_f;
        for (int p = lane; p < P_max; p += 64) {
            double e = 0.0;
            if (p < P) {
                double v = 0.0;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int row = t.di[3 * p + a];
                    if (row >= 0) v = fma(t.dw[3 * p + a], zm[row], v);
                }
                e = km * v;
                ew[p] = e;
            }
            if (line != nullptr) line[p] = e;
        }
        __builtin_amdgcn_wave_barrier();
        // the candidates (p, a) in p-major order: ascending per lane, so the first of equals stays
        double hi = 0.0, lo = 0.0;
        int hi_at = INT_MAX, lo_at = INT_MAX;
        for (int cand = lane; cand < cands; cand += 64) {
            const int p = cand / A, a = cand - p * A;
            const double sp = t.s[p], oa = t.to[a];
            double n = 0.0;
            for (int a2 = 0; a2 < A; ++a2) {
                const double e = a2 == a ? ew[p] : line_at(t.s, ew, P, S, eps, sp + (oa - t.to[a2]));
                n = fma(t.tw[a2], e, n);
            }
            if (hi_at == INT_MAX || n > hi) {
                hi = n;
                hi_at = cand;
            }
            if (lo_at == INT_MAX || n < lo) {
                lo = n;
                lo_at = cand;
            }
        }
        // (a lane without a candidate must lose against every value: +-inf with the index INT_MAX)
        if (hi_at == INT_MAX) {
            hi = -__builtin_huge_val();
            lo = __builtin_huge_val();
        }
        wave_extreme_index<true>(hi, hi_at);
        wave_extreme_index<false>(lo, lo_at);
        // the areas, segment by segment in ascending p (every lane runs the same loop on broadcast reads; lane 0 writes)
        double pos = 0.0, neg = 0.0;
        for (int p = 0; p < P - 1; ++p) {
            const double h = t.s[p + 1] - t.s[p], u = ew[p], v = ew[p + 1];
            if (u >= 0.0 && v >= 0.0) {
                pos += 0.5 * h * (u + v);
            } else if (u <= 0.0 && v <= 0.0) {
                neg += 0.5 * h * (u + v);
            } else {
                const double cut = h * (u / (u - v));
                const double au = 0.5 * u * cut, av = 0.5 * v * (h - cut);
                pos += u > 0.0 ? au : av;
                neg += u > 0.0 ? av : au;
            }
        }
        if (lane == 0) {
            const int ph = hi_at / A, pl = lo_at / A;
            nmax_out[o] = hi;
            nmin_out[o] = lo;
            xmax_out[o] = t.s[ph] + t.to[hi_at - ph * A];
            xmin_out[o] = t.s[pl] + t.to[lo_at - pl * A];
            apos_out[o] = pos;
            aneg_out[o] = neg;
        }
        __builtin_amdgcn_wave_barrier();   // (the next member's eta overwrites ew)
    }
}

int influence_launch(int B, const TrsBatch& bt, int e0, int C, int P_max, int A, const int* path, const int* path_len,
                     const double* dir, const double* train_w, const double* train_o, const double* Z, double* eta_out,
                     double* N_max, double* N_min, double* x_max, double* x_min, double* area_pos, double* area_neg,
                     hipStream_t stream) {
    if (B < 0 || e0 < 0 || C < 0 || bt.nJ_max < 0 || bt.nM_max < 0 || P_max < 0 || A < 1 || bt.ld_f < 0)
        return (int)hipErrorInvalidValue;
    if (B == 0 || C == 0 || e0 >= bt.nM_max) return 0;
    if (!trs_influence_fits(bt.nJ_max, P_max, A)) return (int)hipErrorInvalidValue;
    if ((long long)P_max * A > INT_MAX - 64) return (int)hipErrorInvalidValue;   // (the candidate index is an int)
    trs_lds::raise_lds_once<trs_influence_apply_kernel>();
    const int slices = (C + TRS_INFLUENCE_SLICE - 1) / TRS_INFLUENCE_SLICE;
    hipLaunchKernelGGL(trs_influence_apply_kernel, dim3((unsigned)slices * (unsigned)B), dim3(64 * WAVES),
                       influence_lds(bt.nJ_max, P_max, A), stream, bt, e0, C, TRS_INFLUENCE_SLICE, P_max, A, path, path_len,
                       dir, train_w, train_o, Z, eta_out, N_max, N_min, x_max, x_min, area_pos, area_neg);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int trs_influence_abi_version(void) { return TRS_INFLUENCE_ABI_VERSION; }

int trs_influence_fits(int nJ_max, int P_max, int A) {
    return nJ_max >= 0 && P_max >= 0 && A >= 1 && influence_lds(nJ_max, P_max, A) <= TRS_LDS_BYTES;
}

int trs_influence_apply(int B, int e0, int C, int nJ_max, int nM_max, int P_max, int A, const double* xyz,
                        const int32_t* conn, const double* E, const double* Amem, const int32_t* free_index,
                        const int32_t* nJ, const int32_t* nM, const int32_t* path, const int32_t* path_len,
                        const double* dir, const double* train_w, const double* train_o, const double* Z, int ld_f,
                        double* eta_out, double* N_max, double* N_min, double* x_max, double* x_min, double* area_pos,
                        double* area_neg, const int32_t* joint_out, void* stream) {
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_general(conn, E, Amem), free_index, nullptr, nJ, nM,
                                  joint_out, ld_f);
    return influence_launch(B, bt, e0, C, P_max, A, path, path_len, dir, train_w, train_o, Z, eta_out, N_max, N_min, x_max,
                            x_min, area_pos, area_neg, (hipStream_t)stream);
}

int trs_influence_tab_apply(int B, int e0, int C, int nJ_max, int nM_max, int P_max, int A, const double* xyz,
                            const uint16_t* conn16, const uint8_t* type_idx, const double* types,
                            const int32_t* free_index, const int32_t* nJ, const int32_t* nM, const int32_t* path,
                            const int32_t* path_len, const double* dir, const double* train_w, const double* train_o,
                            const double* Z, int ld_f, double* eta_out, double* N_max, double* N_min, double* x_max,
                            double* x_min, double* area_pos, double* area_neg, const int32_t* joint_out, void* stream) {
    if (B > 0 && (!conn16 || !type_idx || !types)) return (int)hipErrorInvalidValue;
    const TrsBatch bt = trs_batch(nJ_max, nM_max, xyz, trs_members_table(conn16, type_idx, types), free_index, nullptr, nJ,
                                  nM, joint_out, ld_f);
    return influence_launch(B, bt, e0, C, P_max, A, path, path_len, dir, train_w, train_o, Z, eta_out, N_max, N_min, x_max,
                            x_min, area_pos, area_neg, (hipStream_t)stream);
}

}  // extern "C"
