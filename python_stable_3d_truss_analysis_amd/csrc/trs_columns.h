// trs_columns.h - what the kernels on the columns z_e = inv(K_ff) b_e,f share (loss.hip, sets.hip, influence.hip):
//   - the right-hand-side row b_e,f, ONE function and ONE kernel (loss.hip), so a member's row has the same bits whoever
//     asks for it: trs_loss_rhs (members e0 .. e0 + C - 1) or trs_sets_rhs (the members of an id list);
//   - the wave extreme that carries the index with the value, and the close of a peak with it;
//   - for the two apply kernels that run one work-group per (truss, slice) over staged tables (trs_loss_apply,
//     trs_sets_apply): the tables and their layout in LDS (trs_lds.h), which is the rule behind trs_loss_fits /
//     trs_sets_fits, the passes and the launch; the stage; and c_m . (v[j1] - v[j0]), the ONE expression behind N, q_m, r_e and a set's pivots.
// The stage works on a truss view (trs_view.h: counts trimmed to the arrays, end-joint ids clamped), fills the DOF map and
// the joint order for all nJ_max joints (-1 = held past the truss's own) and zeroes the waves' vectors: whatever the
// inputs hold, nothing is read or written outside the arrays, and entries past the truss's joints read as zero.
#pragma once
#include "trs_common.h"
#include "trs_lds.h"

#include <limits.h>

namespace trs_col {

#ifndef TRS_LOSS_WAVES
#define TRS_LOSS_WAVES 4   // waves per work-group of trs_loss_apply and of the rhs kernel (EXPERIMENTS R14)
#endif
constexpr int MAX_PASS = 8;   // load cases per pass at most (loss: their maxima live in registers; sets: lane 8 l + i
                              // substitutes case l)

// Row `row` of Z, by one wave: b_e,f of member e of the truss when `real`, else zeros - +c at the free DOFs of j1 and
// -c at those of j0, zeros in the other columns below npad.  One lane writes each entry.
__device__ __forceinline__ void write_row(double* __restrict__ row, const int npad, const int lane, const bool real,
                                          const int e, const TrussView& v) {
    int at[6] = {-1, -1, -1, -1, -1, -1};
    double val[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (real) {
        const int2 c = v.ends(e).c;
        const trs_rec::MemberGeom g = trs_rec::member_geom(v.X, c.x, c.y);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            at[a] = v.row_of(3 * c.y + a);
            val[a] = g.c[a];
            at[3 + a] = v.row_of(3 * c.x + a);
            val[3 + a] = -g.c[a];
        }
    }
    for (int col = lane; col < npad; col += 64) {
        double v = 0.0;
#pragma unroll
        for (int t = 0; t < 6; ++t)
            if (at[t] == col) v = val[t];
        row[col] = v;
    }
}

// The launcher of the rhs kernel (defined in loss.hip): row i of Z [B][C][ld_f] is b_e,f of e = cols[b][i] when `cols`
// is given, else of e = e0 + i; zeros for an e outside [0, nM[b]).  (The batch carries no nJ: every joint of the arrays.)
int rhs_launch(int B, const TrsBatch& bt, int e0, const int* cols, int C, double* Z, hipStream_t stream);

// (value, index) extreme over the wave: the larger (MAX) or the smaller value, the lower index among equal values
template <bool MAX>
__device__ __forceinline__ void wave_extreme_index(double& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if ((MAX ? ov > v : ov < v) || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

// Closes a peak: the wave's maximum of (v, i), written by lane 0 - (0, -1) where no lane had a candidate (i = INT_MAX).
__device__ __forceinline__ void close_peak(double v, int i, const int lane, double* __restrict__ value_out,
                                           int* __restrict__ index_out) {
    wave_extreme_index<true>(v, i);
    if (lane == 0) {
        *value_out = i == INT_MAX ? 0.0 : v;
        *index_out = i == INT_MAX ? -1 : i;
    }
}

// The LDS tables of an apply kernel of `waves` waves with g cases per pass and `extra` doubles of every wave's own
// (bar-942 needs 86 KB with one case, so two work-groups per CU never fit it)
struct Tables {
    double *cx, *cy, *cz, *k, *ia;   // [nM_max] each: direction cosines, E A / len, 1 / A
    double* z;                       // [waves][3 nJ_max]  a joint-layout vector per wave
    double* own;                     // [waves][extra]     what else a wave keeps
    double* u;                       // [g][3 nJ_max]      the intact displacements of the pass, joint layout
    double* N;                       // [g][nM_max]        the intact member forces of the pass
    int2* ends;                      // [nM_max]
    int* fi;                         // [3 nJ_max]
    int* jo;                         // [nJ_max]
};

template <class Arena>
__host__ __device__ inline Tables layout(Arena& a, int nJ_max, int nM_max, int g, int waves, int extra) {
    Tables t;
    t.cx = a.template take<double>(nM_max);
    t.cy = a.template take<double>(nM_max);
    t.cz = a.template take<double>(nM_max);
    t.k = a.template take<double>(nM_max);
    t.ia = a.template take<double>(nM_max);
    t.z = a.template take<double>((size_t)waves * 3 * nJ_max);
    t.own = a.template take<double>((size_t)waves * extra);
    t.u = a.template take<double>((size_t)g * 3 * nJ_max);
    t.N = a.template take<double>((size_t)g * nM_max);
    t.ends = a.template take<int2>(nM_max);
    t.fi = a.template take<int>(3, nJ_max);
    t.jo = a.template take<int>(nJ_max);
    return t;
}

inline size_t lds(int nJ_max, int nM_max, int g, int waves, int extra) {
    return trs_lds::count([&](auto& a) { layout(a, nJ_max, nM_max, g, waves, extra); });
}

// cases per pass: the largest g <= min(L, MAX_PASS) that fits, evened out over the passes it makes necessary; 0 = none
inline int pass(int nJ_max, int nM_max, int L, int waves, int extra) {
    int g = L < MAX_PASS ? L : MAX_PASS;
    while (g > 0 && lds(nJ_max, nM_max, g, waves, extra) > TRS_LDS_BYTES) --g;
    if (g <= 0) return 0;
    const int passes = (L + g - 1) / g;
    return (L + passes - 1) / passes;
}

// the rule of trs_loss_fits and trs_sets_fits: one case per pass fits
inline int fits(int nJ_max, int nM_max, int L, int waves, int extra) {
    return nJ_max >= 0 && nM_max >= 0 && L >= 0 && lds(nJ_max, nM_max, 1, waves, extra) <= TRS_LDS_BYTES;
}


// c_m . d for the staged member m, and c_m . (v[j1] - v[j0]) for a joint-layout vector v: times k_m the member force of
// the displacements v.  The order of the two fused multiply-adds is part of the results' bits.
__device__ __forceinline__ double along(const Tables& t, const int m, const double d0, const double d1, const double d2) {
    return fma(t.cz[m], d2, fma(t.cy[m], d1, t.cx[m] * d0));
}
__device__ __forceinline__ double along(const Tables& t, const int m, const double* v) {
    const int2 c = t.ends[m];
    return along(t, m, v[3 * c.y] - v[3 * c.x], v[3 * c.y + 1] - v[3 * c.x + 1], v[3 * c.y + 2] - v[3 * c.x + 2]);
}

// Once per work-group of `threads` threads (waves = threads / 64), for the truss v: the member table, the DOF map, the
// joint order, zeroed wave vectors.  The first stage_pass synchronises.
__device__ __forceinline__ void stage(const Tables& t, const int tid, const int threads, const TrussView& v) {
    for (int m = tid; m < v.members; m += threads) {
        const int2 c = v.ends(m).c;
        const trs_rec::MemberGeom mg = trs_rec::member_geom(v.X, c.x, c.y);
        t.ends[m] = c;
        t.cx[m] = mg.c[0];
        t.cy[m] = mg.c[1];
        t.cz[m] = mg.c[2];
        t.k[m] = v.mem.EA(v.mbase + m) / mg.len;
        t.ia[m] = 1.0 / v.mem.area(v.mbase + m);
    }
    // staged for every joint of the arrays, -1 (held) past the truss's own: an end joint trimmed to there reads zeros
    for (int d = tid; d < v.ndof_max; d += threads) t.fi[d] = v.row_of(d);
    for (int j = tid; j < v.nJ_max; j += threads) t.jo[j] = v.place(j);
    for (int d = tid; d < threads / 64 * v.ndof_max; d += threads) t.z[d] = 0.0;   // (entries past ndof stay zero)
}

// Per pass: u of the lg cases from Ul (the first case's row of U [..][ld_f]) in joint layout, and N = k c . (u_j1 - u_j0)
// from the staged c and k - the geometry is not formed again per case and pass.
__device__ __forceinline__ void stage_pass(const Tables& t, const int tid, const int threads, const int lg,
                                           const int members, const int nJ_max, const int nM_max,
                                           const double* __restrict__ Ul, const int ld_f) {
    const int ndof_max = 3 * nJ_max;
    __syncthreads();   // (the tables of `stage` are written; the previous pass's readers of u and N are done)
    for (int x = tid; x < lg * ndof_max; x += threads) {
        const int l = x / ndof_max, d = x - l * ndof_max;
        const int row = t.fi[d];
        t.u[(size_t)l * ndof_max + d] = row >= 0 ? Ul[(size_t)l * ld_f + row] : 0.0;
    }
    __syncthreads();
    for (int x = tid; x < lg * members; x += threads) {
        const int l = x / members, m = x - l * members;
        t.N[(size_t)l * nM_max + m] = t.k[m] * along(t, m, t.u + (size_t)l * ndof_max);
    }
    __syncthreads();
}

}  // namespace trs_col
