// trs_view.h - what an analysis kernel is handed: the resident batch as ONE by-value argument (TrsBatch) and the truss
// of a work-group inside it (TrussView = TrsBatch::truss(b)).  The view is the one place where the counts are trimmed
// and the ids are clamped, by the rule of trs_columns.h: whatever the inputs hold, nothing is read or written outside
// the arrays.  On well-formed input every trim and clamp is the identity.
//   counts    joints, members, nfree trimmed to nJ_max, nM_max, ld_f; members = 0 when nJ_max == 0 (no end to clamp to)
//   row_of    the reduced row of a DOF, or -1: held, past the truss's own joints, or outside nfree (<= ld_f)
//   place     where joint j's results go (joint_out; the same map reads a caller's input): an id outside the arrays
//             falls back to j
//   ends      a member's end joints clamped into [0, nJ_max), and whether both lay inside the truss
// Everything here is integer and pointer work and __host__ __device__, so the rule is exercised on plain host arrays
// (tests/view_rule.cpp).  A field that a kernel does not need is null or 0 (a null count stands for the arrays' own
// size); the pointers of a by-value struct carry no __restrict__, as TrsMembers'
// never did.  Offsets are formed as the kernels formed them: (size_t)b * ... bases.
#pragma once
#include "trs_common.h"

struct TrussView {
    int joints, members, ndof, ndof_max, nfree, nJ_max;
    const int* fi;       // [3 nJ_max]  free_index of the truss
    const double* X;     // [3 nJ_max]  xyz of the truss
    size_t mbase;        // b * nM_max: the truss's first member in the batch's member arrays
    const int* jo;       // [nJ_max]    joint_out of the truss, or null
    TrsMembers mem;

    struct Ends {
        int2 c;          // clamped into the arrays
        bool inside;     // both ends were joints of the truss
    };

    // 0 <= i < n in one comparison (n >= 0: the counts are trimmed)
    __host__ __device__ __forceinline__ static bool below(int i, int n) { return (unsigned)i < (unsigned)n; }
    __host__ __device__ __forceinline__ bool in_truss(int j) const { return below(j, joints); }
    __host__ __device__ __forceinline__ int row_of(int d) const {
        const int r = d < ndof ? fi[d] : -1;   // (d >= 0: a caller's loop index, or 3 j + a of a clamped joint)
        return below(r, nfree) ? r : -1;
    }
    // The rows of joint j's three DOFs behind ONE test of j: three row_of(3 j + a) are three guarded reads, each waiting
    // for the one before it (the compiler does not see that j < joints bounds all of them; EXPERIMENTS R26).
    struct Rows {
        int r[3];
        __host__ __device__ __forceinline__ bool held(int a) const { return r[a] < 0; }
        __host__ __device__ __forceinline__ bool any_held() const { return (r[0] | r[1] | r[2]) < 0; }
        __host__ __device__ __forceinline__ bool all_held() const { return (r[0] & r[1] & r[2]) < 0; }
    };
    __host__ __device__ __forceinline__ Rows rows(int j) const {
        Rows q = {{-1, -1, -1}};
        if (j < joints) {
            q.r[0] = fi[3 * j];
            q.r[1] = fi[3 * j + 1];
            q.r[2] = fi[3 * j + 2];
        }
        for (int a = 0; a < 3; ++a) q.r[a] = below(q.r[a], nfree) ? q.r[a] : -1;
        return q;
    }
    __host__ __device__ __forceinline__ bool held(int j, int a) const { return row_of(3 * j + a) < 0; }
    __host__ __device__ __forceinline__ bool any_held(int j) const { return rows(j).any_held(); }
    __host__ __device__ __forceinline__ bool all_held(int j) const { return rows(j).all_held(); }
    __host__ __device__ __forceinline__ int place(int j) const {
        const int id = jo != nullptr ? jo[j] : j;
        return below(id, nJ_max) ? id : j;
    }
    // where DOF d (= 3 j + a of the device's numbering) goes in the caller's
    __host__ __device__ __forceinline__ int place_dof(int d) const { return 3 * place(d / 3) + d % 3; }
    // the end joints as the arrays hold them (TrsMembers::ends, for host and device): for a test, never for an index
    __host__ __device__ __forceinline__ int2 raw_ends(int m) const {
#if defined(__HIP_DEVICE_COMPILE__)
        return mem.ends(mbase + m);
#endif
        if (mem.tidx != nullptr) {
            const ushort2 s = reinterpret_cast<const ushort2*>(mem.conn)[mbase + m];
            return int2{(int)s.x, (int)s.y};
        }
        return reinterpret_cast<const int2*>(mem.conn)[mbase + m];
    }
    __host__ __device__ __forceinline__ int into_arrays(int j) const {
        const int lo = j > 0 ? j : 0;
        return lo < nJ_max - 1 ? lo : nJ_max - 1;
    }
    __host__ __device__ __forceinline__ Ends ends(int m) const {
        int2 c = raw_ends(m);
        const bool inside = in_truss(c.x) & in_truss(c.y);
        c.x = into_arrays(c.x);   // (a joint id outside the arrays would index outside them)
        c.y = into_arrays(c.y);
        return Ends{c, inside};
    }
};

struct TrsBatch {
    const double* xyz;        // [B][nJ_max][3]
    TrsMembers mem;
    const int* free_index;    // [B][3 nJ_max]
    const int* n_free;        // [B]            a null count: the arrays' own size (ld_f, nJ_max, nM_max)
    const int* nJ;            // [B]
    const int* nM;            // [B]
    const int* joint_out;     // [B][nJ_max] or null
    int nJ_max, nM_max, ld_f;

    __host__ __device__ __forceinline__ static int trim(int v, int most) { return v < 0 ? 0 : v < most ? v : most; }
    __host__ __device__ __forceinline__ TrussView truss(int b) const {
        // the three counts are read side by side and trimmed afterwards: a trim behind each null test made every
        // read wait for the one before it (three memory round trips at the head of every work-group; EXPERIMENTS R26)
        const int raw_nJ = nJ != nullptr ? nJ[b] : nJ_max;   // (a null count: no tighter bound than the arrays)
        const int raw_nM = nM != nullptr ? nM[b] : nM_max;
        const int raw_nf = n_free != nullptr ? n_free[b] : ld_f;
        TrussView v;
        v.nJ_max = nJ_max;
        v.joints = trim(raw_nJ, nJ_max);
        v.members = nJ_max > 0 ? trim(raw_nM, nM_max) : 0;
        v.ndof = 3 * v.joints;
        v.ndof_max = 3 * nJ_max;
        v.nfree = trim(raw_nf, ld_f);
        v.fi = free_index + (size_t)b * v.ndof_max;
        v.X = xyz != nullptr ? xyz + (size_t)b * v.ndof_max : nullptr;
        v.mbase = (size_t)b * nM_max;
        v.jo = joint_out != nullptr ? joint_out + (size_t)b * nJ_max : nullptr;
        v.mem = mem;
        return v;
    }
};

// The host-side makers, beside trs_members_general / trs_members_table
static inline TrsBatch trs_batch(int nJ_max, int nM_max, const double* xyz, const TrsMembers& mem, const int* free_index,
                                 const int* n_free, const int* nJ, const int* nM, const int* joint_out, int ld_f) {
    return TrsBatch{xyz, mem, free_index, n_free, nJ, nM, joint_out, nJ_max, nM_max, ld_f};
}
// a batch without members: the kernels that only walk the DOF map
static inline TrsBatch trs_batch_dofs(int nJ_max, const int* free_index, const int* n_free, const int* nJ,
                                      const int* joint_out, int ld_f) {
    return trs_batch(nJ_max, 0, nullptr, TrsMembers{}, free_index, n_free, nJ, nullptr, joint_out, ld_f);
}
