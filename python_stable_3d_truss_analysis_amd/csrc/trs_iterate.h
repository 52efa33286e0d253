// trs_iterate.h - what the step kernels of the five iterated analyses share (sizing.hip, compliance.hip, minweight.hip,
// unilateral.hip, plastic.hip): each iterates analyse -> step -> one counter on a resident batch, one 256-thread
// work-group per truss.
//   - Run: the run protocol on the status words st [B][4] - status, count, latched info, spare - that DESIGN 3r states:
//     begin, frozen, fail (the latch), finish (the `active` counter).  The status values are the analysis's own, so they
//     are template parameters; what differs between the analyses - a report mode 2, the count a failure leaves, what
//     else `begin` resets - is said at the call, and the type has no flag for it;
//   - wave_sum, wave_max: the butterfly lane ^ 32, ^ 16, ... ^ 1 - the order every sum of these kernels is promised in;
//   - CaseStage: the L cases of the case block through LDS, one at a time in two buffers (sizing, compliance, minweight);
//   - AreaBounds: area_min / area_max of those three, each one number or one per member, and their argument rule.
// Everything is __forceinline__: trs_cm_step sits ten registers under the 128 of its fourth wave per SIMD.
#pragma once
#include "trs_view.h"

namespace trs_iter {

template <int ACTIVE, int FAILED>
struct Run {
    int* st;   // the truss's four words
    int status, count;

    __device__ __forceinline__ Run(int* words, const bool begin) : st(words), status(words[0]), count(words[1]) {
        if (begin) {
            status = ACTIVE;
            count = 0;
        }
    }
    __device__ __forceinline__ bool active() const { return status == ACTIVE; }
    // every thread calls it, behind the analysis's own roll-back (the barrier: every thread has read the status words)
    __device__ __forceinline__ void fail(const int pivot, const int count_left, const int tid) const {
        __syncthreads();
        if (tid == 0) {
            st[0] = FAILED;
            st[1] = count_left;
            st[2] = pivot;
        }
    }
    __device__ __forceinline__ int one_back() const { return count > 0 ? count - 1 : 0; }
    // thread 0, behind a barrier that every thread's read of the words lies before
    __device__ __forceinline__ void finish(const int it, int* active_count) const {
        const bool still = active();
        st[0] = status;
        st[1] = still ? it + 1 : count;
        if (still) atomicAdd(active_count, 1);
    }
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

// One case's displacement vector at a time in LDS, joint layout, device numbering: case l in buffer l & 1 of u
// [2][3 nJ_max], through row [3 nJ_max] = row_of every DOF (-1: a held DOF or the padding, which read 0), formed once so
// that a case's staging is one load deep.  Thread d % 256 forms row[d] and is the one that reads it: no barrier between
// the table and the staging.  The caller's barrier per case separates the staging of case l + 1 from its readers.
struct CaseStage {
    double* u;
    int* row;
    const double* F;   // the truss's cases [L][ld_f]
    int ndof_max, ld_f;

    __device__ __forceinline__ void form_rows(const TrussView& tr, const int tid) const {
        for (int d = tid; d < ndof_max; d += 256) row[d] = tr.row_of(d);
    }
    __device__ __forceinline__ const double* buffer(const int l) const { return u + (size_t)(l & 1) * ndof_max; }
    __device__ __forceinline__ void stage(const int l, const int tid) const {
        double* to = u + (size_t)(l & 1) * ndof_max;
        const double* f = F + (size_t)l * ld_f;
        for (int d = tid; d < ndof_max; d += 256) {
            const int r = row[d];
            to[d] = r >= 0 ? f[r] : 0.0;
        }
    }
};

struct AreaBounds {
    const double* a_min;   // [B][nM_max] or null: a_min_all for every member
    const double* a_max;
    double a_min_all, a_max_all;

    __device__ __forceinline__ double lo(const size_t m) const { return a_min != nullptr ? a_min[m] : a_min_all; }
    __device__ __forceinline__ double hi(const size_t m) const { return a_max != nullptr ? a_max[m] : a_max_all; }
    // the argument rule of the C entry points: what is one number is checked here, an array is the caller's
    bool valid() const { return (a_min || a_min_all > 0.0) && (a_min || a_max || a_max_all >= a_min_all); }
};

}  // namespace trs_iter
