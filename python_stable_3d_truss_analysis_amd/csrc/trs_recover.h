// trs_recover.h - the per-member and per-joint arithmetic of the result recovery, shared by trs_recover
// (recover.hip) and the multi-case recovery trs_recover_cases (cases.hip): both paths call the same functions,
// so case k of a multi-case recovery rounds exactly like a single recovery of case k.  Also the builder of the
// per-joint member-end lists in LDS that the analysis kernels sum over (build_end_lists, on a truss view: trs_view.h)
// and order_by_neighbour; where the lists lie in a kernel's LDS is its layout's affair (trs_lds.h).
#pragma once
#include "trs_common.h"
#include "trs_view.h"

namespace trs_rec {

struct MemberGeom {
    double len, c[3];
};

__device__ __forceinline__ MemberGeom member_geom(const double* X, int j0, int j1) {
    MemberGeom g;
    double d[3], len2 = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        d[a] = X[3 * j1 + a] - X[3 * j0 + a];
        len2 += d[a] * d[a];
    }
    g.len = sqrt(len2);
#pragma unroll
    for (int a = 0; a < 3; ++a) g.c[a] = d[a] / g.len;
    return g;
}

// Young's modulus of a member, either member form (not beside TrsMembers::EA: bench.py fingerprints trs_common.h)
__device__ __forceinline__ double modulus(const TrsMembers& mem, size_t mm) {
    return mem.table() ? mem.types[3 * (int)mem.tidx[mm] + 1] : mem.E[mm];
}

// axial force of a member from the displacements of its end joints: N = (E A / L) c . (u1 - u0)
__device__ __forceinline__ double member_axial(const MemberGeom& g, double EA, const double* u, int j0, int j1) {
    const double k = EA / g.len;
    double proj = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) proj += g.c[a] * (u[3 * j1 + a] - u[3 * j0 + a]);
    return k * proj;
}

// The end force of member (g, axial) on its joint `end` (1: +N c on joint1, 0: -N c on joint0), added to a
// running reaction sum.  ONE function with explicit fused multiply-adds for every path of the kernel: the paths
// then round alike and their reactions are equal bit for bit.
__device__ __forceinline__ void add_end_force(double (&r)[3], const double (&c)[3], double axial, int end) {
    const double s = end ? axial : -axial;
#pragma unroll
    for (int a = 0; a < 3; ++a) r[a] = fma(s, c[a], r[a]);
}

// A list of member ends ((member << 1) | end) sorted by member id in place (insertion sort: the lists are short)
template <class ListPtr>
__device__ __forceinline__ void sort_list(ListPtr list, const int deg) {
    for (int i = 1; i < deg; ++i) {
        const int key = list[i];
        int p = i - 1;
        while (p >= 0 && list[p] > key) {
            list[p + 1] = list[p];
            --p;
        }
        list[p + 1] = key;
    }
}

// Reaction at one constrained joint from its list of member ends: the list is sorted by member id in place and summed in
// that order.  The form of trs_recover (recover.hip), whose inputs the solve has checked.
template <class ListPtr>
__device__ __forceinline__ void joint_reaction(ListPtr list, const int deg, const TrsMembers& mem,
                                               const double* __restrict__ X, const size_t mbase, const double* u,
                                               const int* jo, double (&r)[3]) {
    sort_list(list, deg);
    r[0] = r[1] = r[2] = 0.0;
    for (int i = 0; i < deg; ++i) {
        const int m = list[i] >> 1, end = list[i] & 1;
        const int2 c = mem.ends(mbase + m);
        const MemberGeom g = member_geom(X, c.x, c.y);
        const double axial = member_axial(g, mem.EA(mbase + m), u, jo ? jo[c.x] : c.x, jo ? jo[c.y] : c.y);
        add_end_force(r, g.c, axial, end);
    }
}
// The same on a truss view, u in the device's joint numbering: the ends come clamped.
template <class ListPtr>
__device__ __forceinline__ void joint_reaction(ListPtr list, const int deg, const TrussView& v, const double* u,
                                               double (&r)[3]) {
    sort_list(list, deg);
    r[0] = r[1] = r[2] = 0.0;
    for (int i = 0; i < deg; ++i) {
        const int m = list[i] >> 1, end = list[i] & 1;
        const int2 c = v.ends(m).c;
        const MemberGeom g = member_geom(v.X, c.x, c.y);
        add_end_force(r, g.c, member_axial(g, v.mem.EA(v.mbase + m), u, c.x, c.y), end);
    }
}

// The member-end lists of one truss in LDS: joint j's ends are ends[start[j] .. start[j] + cnt[j]), each
// (member << 1) | end, sorted by member id.
struct EndLists {
    int* cnt;     // [nJ_max]
    int* start;   // [nJ_max + 1]
    int* ends;    // [2 nM_max]
};

struct EveryJoint {
    __device__ __forceinline__ bool operator()(int) const { return true; }
};

// Builds the lists of the truss's joints that `keep(j)` admits (the others get empty lists; an end joint outside the
// truss gets no list - it would index LDS outside the lists - and no sum), by a work-group of 256 threads:
// count with integer atomics, scan, fill, then every list is sorted by member id - the order in which every kernel
// sums over a list, whatever order the atomics filled it in.  The ONE builder of every analysis kernel (trs_recover_cases
// keeps the constrained joints only).  There is no barrier after the sort: the caller places one before a thread reads a
// list that it did not sort itself.
template <class Keep = EveryJoint>
__device__ __forceinline__ void build_end_lists(const EndLists& t, const TrussView& v, const int tid, Keep keep = Keep()) {
    const int joints = v.joints, members = v.members;
    for (int j = tid; j < v.nJ_max; j += 256) t.cnt[j] = 0;
    __syncthreads();
    for (int m = tid; m < members; m += 256) {
        const int2 c = v.raw_ends(m);
        if (v.in_truss(c.x) && keep(c.x)) atomicAdd(&t.cnt[c.x], 1);
        if (v.in_truss(c.y) && keep(c.y)) atomicAdd(&t.cnt[c.y], 1);
    }
    __syncthreads();
    if (tid < 64) {  // exclusive scan of cnt by one wave
        int base = 0;
        for (int j0 = 0; j0 < joints; j0 += 64) {
            const int j = j0 + tid;
            const int own = j < joints ? t.cnt[j] : 0;
            int incl = own;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const int up = __shfl_up(incl, off);
                if (tid >= off) incl += up;
            }
            if (j < joints) t.start[j] = base + incl - own;
            base += __shfl(incl, 63);
        }
    }
    __syncthreads();
    for (int j = tid; j < joints; j += 256) t.cnt[j] = 0;  // the fill cursor
    __syncthreads();
    for (int m = tid; m < members; m += 256) {
        const int2 c = v.raw_ends(m);
        if (v.in_truss(c.x) && keep(c.x)) t.ends[t.start[c.x] + atomicAdd(&t.cnt[c.x], 1)] = m << 1;
        if (v.in_truss(c.y) && keep(c.y)) t.ends[t.start[c.y] + atomicAdd(&t.cnt[c.y], 1)] = (m << 1) | 1;
    }
    __syncthreads();
    for (int j = tid; j < joints; j += 256) sort_list(t.ends + t.start[j], t.cnt[j]);
}

// The far joint of every list entry into `far` (-1: outside the truss), and every list re-sorted by (far joint, member id) -
// the order of trs_assemble's adjacency lists, so that a sum over a list rounds as the assembly's own sums do: parallel
// members lie side by side, and a member listed twice gives the bits of one member of twice the area wherever the linear
// solve does.  What the nonlinear kernels (nonlinear.hip) and the buckling product (buckling.hip) sum over.
// The sort is stable and the lists arrive in member-id order.  Thread j % 256 owns joint j here as in build_end_lists'
// own sort, so no barrier is needed between the two; the caller places one before another thread reads a list.
__device__ __forceinline__ void order_by_neighbour(const EndLists& t, int* far_all, const TrussView& v, const int tid) {
    for (int j = tid; j < v.joints; j += 256) {
        int* list = t.ends + t.start[j];
        int* far = far_all + t.start[j];
        const int deg = t.cnt[j];
        for (int i = 0; i < deg; ++i) {
            const int2 c = v.raw_ends(list[i] >> 1);
            const int o = (list[i] & 1) ? c.x : c.y;
            far[i] = v.in_truss(o) ? o : -1;
        }
        for (int i = 1; i < deg; ++i) {
            const int kf = far[i], ke = list[i];
            int p = i - 1;
            while (p >= 0 && far[p] > kf) {
                far[p + 1] = far[p];
                list[p + 1] = list[p];
                --p;
            }
            far[p + 1] = kf;
            list[p + 1] = ke;
        }
    }
}

}  // namespace trs_rec
