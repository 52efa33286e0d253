// trs_loss_row.h - what the kernels on the columns z_e = inv(K_ff) b_e,f share: the right-hand-side row b_e,f as
// trs_loss_rhs (loss.hip: members e0 .. e0 + C - 1) and trs_sets_rhs (sets.hip: the members of an id list) write it -
// ONE function, so a member's row has the same bits whichever kernel forms it - and the wave maximum that carries the
// index with the value.
#pragma once
#include "trs_common.h"
#include "trs_recover.h"

namespace trs_loss_row {

// Row `row` of Z, by one wave: b_e,f of member `member` (= b * nM_max + e) when `real`, else zeros - +c at the free
// DOFs of j1 and -c at those of j0 through fi (the truss's free_index), zeros in the other columns below npad.  One
// lane writes each entry.
__device__ __forceinline__ void write_row(double* __restrict__ row, const int npad, const int lane, const bool real,
                                          const size_t member, const TrsMembers& mem, const double* __restrict__ X,
                                          const int* __restrict__ fi) {
    int at[6] = {-1, -1, -1, -1, -1, -1};
    double val[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (real) {
        const int2 c = mem.ends(member);
        const trs_rec::MemberGeom g = trs_rec::member_geom(X, c.x, c.y);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            at[a] = fi[3 * c.y + a];
            val[a] = g.c[a];
            at[3 + a] = fi[3 * c.x + a];
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

// (value, index) maximum over the wave: the larger value, the lower index on a tie
__device__ __forceinline__ void wave_max_index(double& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov > v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

}  // namespace trs_loss_row
