// trs_modal.h - the mode-superposition core that the two analyses on the resident mode block share (spectrum.hip:
// response spectrum; harmonic.hip: frequency sweeps).  Both turn the block X that trs_modes_step left resident into
// displacements, member forces and reactions by the same steps, one work-group of 256 threads per truss (and case), and
// what the steps have in common lives here, so a third consumer of the block is not written as a third copy:
//   - which modes take part: mode_count, takes_part and part_mask - a column of X whose lam contributes nothing is read
//     by no kernel;
//   - the projection of a load onto the modes: the walk over the DOFs in joint layout (each_dof hands over the reduced
//     row, the axis, the mass and the eight values of X) and the reduction of the threads' partial sums (block_sums: a butterfly
//     inside the wave, the four waves in ascending order);
//   - zero_columns, for the block of right-hand sides of the extra substitution;
//   - the stage of the response vectors in LDS in joint layout (stage_vectors), zero at held DOFs and past the truss's
//     own joints;
//   - one member as the passes see it (Member, load_member; m = -1 is "no member"), the axial value of every mode shape
//     in it (member_axials) and of one more vector (slot_axial);
//   - the end forces of a joint with a held DOF from its member-end list, in member-id order (end_list, add_end_forces).
// The arithmetic of a projection and of a residual load stays in the callable of each kernel (the two residual formulas
// round differently, and each analysis keeps its bits), as do the layout of the LDS and everything that combines the
// per-mode values: combine, cqc_rho, spectrum_at and the modal outputs there; the table, sweep_chunk, sweep_all, Envelope
// and Monitor here.  Everything is __forceinline__ and every array is indexed at compile time: trs_rs_combine and
// trs_hr_sweep sit just under the 128 registers of their fourth wave per SIMD (EXPERIMENTS R28).
#pragma once
#include "../../include/trs_harmonic.h"
#include "../../include/trs_modes.h"
#include "../../include/trs_spectrum.h"
#include "trs_common.h"
#include "trs_lds.h"

namespace trs_modal {

using trs_rec::EndLists;
using trs_rec::MemberGeom;

constexpr int MODES = 8;              // modes per truss at most
constexpr int VEC = MODES + 1;        // response vectors per item: the modes, and the static correction in slot 8
constexpr int BLOCK = TRS_MODES_BLOCK;   // columns of X, and of the block of right-hand sides
static_assert(MODES == TRS_RS_MAX_MODES && MODES == TRS_HR_MAX_MODES, "one count of modes for both analyses");
static_assert(VEC == TRS_RS_MAX_VEC && VEC == TRS_HR_MAX_VEC, "the modes and one more slot, for both analyses");
static_assert(TRS_RS_BLOCK == BLOCK && TRS_HR_BLOCK == BLOCK, "the block of both headers is the one of trs_modes.h");

// ---- which modes take part: k < n_modes, and lam positive and finite
__device__ __forceinline__ int mode_count(const int* n_mass, const int b, const int p) { return min(p, max(n_mass[b], 0)); }
__device__ __forceinline__ bool takes_part(const double* lam, const int k, const int n_modes) {
    const double l = k < n_modes ? lam[k] : 0.0;
    return (l > 0.0) & (l < INFINITY);
}
__device__ __forceinline__ unsigned part_mask(const double* lam, const int n_modes) {
    unsigned mask = 0;
#pragma unroll
    for (int k = 0; k < MODES; ++k)
        if (takes_part(lam, k, n_modes)) mask |= 1u << k;
    return mask;
}
__device__ __forceinline__ bool in_mask(const unsigned mask, const int k) { return ((mask >> k) & 1u) != 0; }

// ---- the projection: body(row, axis, m, x) for this thread's DOFs in ascending order that have a reduced row; m the
// lumped mass of the row, x [8] the entries of X's columns at that row, 0 for a mode outside `mask`.  (m is read first:
// behind the eight guarded reads of X it cost trs_rs_modal eight registers and a wave per SIMD.)
template <class Body>
__device__ __forceinline__ void each_dof(const TrussView& v, const double* __restrict__ Mf, const double* __restrict__ Xb,
                                         const int ld_f, const unsigned mask, const int tid, Body body) {
    for (int d = tid; d < v.ndof; d += 256) {
        const int row = v.row_of(d), axis = d % 3;
        if (row < 0) continue;
        const double m = Mf[row];
        double x[MODES];
#pragma unroll
        for (int k = 0; k < MODES; ++k) x[k] = in_mask(mask, k) ? Xb[(size_t)k * ld_f + row] : 0.0;
        body(row, axis, m, x);
    }
}

// The N sums over the work-group of the threads' partials acc: the wave's 64 by the butterfly, then the four waves in
// order.  Thread i < N gets sum i (the others 0); part [4][N] in LDS.  Called by ALL threads: a barrier is inside.
template <int N>
__device__ __forceinline__ double block_sums(const double (&acc)[N], double (*part)[N], const int tid) {
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double s = acc[i];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        if (lane == 0) part[wave][i] = s;
    }
    __syncthreads();
    return tid < N ? ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid] : 0.0;
}

// zeros in the columns c0 .. c1 - 1 of a block of right-hand sides; the caller fences and meets the barrier before
// anybody fills a row (the zeros of another thread lie under a thread's entries)
__device__ __forceinline__ void zero_columns(double* __restrict__ Fb, const int ld_f, const int c0, const int c1,
                                             const int tid) {
    for (int x = c0 * ld_f + tid; x < c1 * ld_f; x += 256) Fb[x] = 0.0;
}

// ---- the stage: nvec response vectors into vec [nvec][3 nJ_max], joint layout.  Slot k < p is column k of X (zeros
// for a mode outside `mask`), slot p + i is extra(i, row); zero at held DOFs and past the truss's own joints.
template <class Extra>
__device__ __forceinline__ void stage_vectors(double* vec, const TrussView& v, const double* __restrict__ Xb,
                                              const int ld_f, const unsigned mask, const int p, const int nvec,
                                              const int tid, Extra extra) {
    const int ndof_max = v.ndof_max;
    for (int x = tid; x < nvec * ndof_max; x += 256) {
        const int k = x / ndof_max, d = x - k * ndof_max;
        const int row = v.row_of(d);
        double val = 0.0;
        if (row >= 0) {
            if (k >= p)
                val = extra(k - p, row);
            else if (in_mask(mask, k))
                val = Xb[(size_t)k * ld_f + row];
        }
        vec[x] = val;
    }
}

// ---- one member as the passes see it
struct Member {
    MemberGeom g;
    double ea;
    int2 c;       // end joints, clamped
    bool live;    // inside the truss and of positive length
};
// member m of the truss; any m outside it (-1: no member) is not live
__device__ __forceinline__ Member load_member(const TrussView& v, const int m) {
    Member r;
    r.live = TrussView::below(m, v.members);
    r.c = int2{0, 0};
    r.ea = 0.0;
    r.g.len = 0.0;
    r.g.c[0] = r.g.c[1] = r.g.c[2] = 0.0;
    if (r.live) {
        // an end outside the truss is on no end list: the member then gives zeros to N as it does to R
        const TrussView::Ends e = v.ends(m);
        r.c = e.c;
        r.g = trs_rec::member_geom(v.X, e.c.x, e.c.y);
        r.ea = v.mem.EA(v.mbase + m);
        r.live = e.inside & (r.g.len > 0.0);
    }
    return r;
}

// The axial value of the staged vector `slot` in a member; 0 for a member that is not live
__device__ __forceinline__ double slot_axial(const double* vec, const Member& mb, const int ndof_max, const int slot) {
    return mb.live ? trs_rec::member_axial(mb.g, mb.ea, vec + (size_t)slot * ndof_max, mb.c.x, mb.c.y) : 0.0;
}

// The axial value of every mode shape in a member, into ax[0 .. 7]: zeros for a member that is not live and for the
// slots p .. 7.  ONE function, so that the member forces, the reactions and the monitors see the same values.
template <int N>
__device__ __forceinline__ void member_axials(const double* vec, const Member& mb, const int ndof_max, const int p,
                                              double (&ax)[N]) {
    static_assert(N >= MODES, "room for every mode");
#pragma unroll
    for (int k = 0; k < MODES; ++k) {   // (ONE test of live and k < p in front of the value: EXPERIMENTS R28)
        ax[k] = 0.0;
        if (mb.live & (k < p)) ax[k] = trs_rec::member_axial(mb.g, mb.ea, vec + (size_t)k * ndof_max, mb.c.x, mb.c.y);
    }
}

// ---- the end forces at a joint with a held DOF, acc [9][3] for the nine response vectors: end_list zeroes acc and
// gives the joint's member-end list (trs_rec::build_end_lists: 2 m + end, member-id order); the kernel walks it, forms
// every member's nine axial values r and adds them with add_end_forces.  The walk stands in each kernel: as a loop
// inside a function that took the middle as a callable it cost trs_rs_combine four registers and with them a wave per
// SIMD, whatever form the callable took (EXPERIMENTS R28).
struct EndList {
    const int* ends;
    int deg;   // 0 for a joint without a held DOF
};
__device__ __forceinline__ EndList end_list(const EndLists& t, const int j, const bool any_held, double (&acc)[VEC][3]) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    return EndList{t.ends + (any_held ? t.start[j] : 0), any_held ? t.cnt[j] : 0};
}
__device__ __forceinline__ void add_end_forces(double (&acc)[VEC][3], const Member& mb, const double (&r)[VEC],
                                               const int end) {
    if (mb.live) {
#pragma unroll
        for (int k = 0; k < VEC; ++k) trs_rec::add_end_force(acc[k], mb.g.c, r[k], end);
    }
}

}  // namespace trs_modal
