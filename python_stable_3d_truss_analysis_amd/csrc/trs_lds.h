// trs_lds.h - the dynamic LDS of the analysis kernels that keep one truss's tables in `extern __shared__ double sh[]`,
// described ONCE per kernel: a `template <class Arena> Tables layout(Arena&, sizes...)` that takes its arrays in order,
// doubles first.  The host calls it with a Count (the bytes behind trs_*_fits, the cases per pass and the launch), the
// kernel with a Carve over sh (the pointers): an array added to a layout is counted and carved, or neither.
// take<T>(n) takes n elements, take<T>(k, n) takes k n of them.  The Carve advances by n in the type the layout hands it
// and forms k n in int, as a carve written out by hand does (the compiler schedules the kernels' LDS traffic on
// knowing that these offsets do not wrap); the Count multiplies in size_t, so no shape overflows on the host.
#pragma once
#include "trs_common.h"
#include "trs_recover.h"

constexpr size_t TRS_LDS_BYTES = 160 * 1024;   // a CU's LDS: the ONE number behind the fits rules, the passes and the launches

namespace trs_lds {

// adds the bytes and hands out nothing; notes an array that would start off its type's alignment
struct Count {
    size_t bytes = 0;
    bool misaligned = false;
    template <class T>
    __host__ __device__ T* take(size_t n) {
        misaligned |= bytes % alignof(T) != 0;
        bytes += n * sizeof(T);
        return nullptr;
    }
    template <class T>
    __host__ __device__ T* take(int k, int n) {
        return take<T>((size_t)k * n);
    }
};

// hands out the arrays of a kernel's LDS one behind the other
struct Carve {
    char* at;
    __device__ __forceinline__ explicit Carve(double* sh) : at(reinterpret_cast<char*>(sh)) {}
    template <class T, class N>
    __device__ __forceinline__ T* take(N n) {
        T* const p = reinterpret_cast<T*>(at);
        at = reinterpret_cast<char*>(p + n);
        return p;
    }
    template <class T>
    __device__ __forceinline__ T* take(int k, int n) {
        return take<T>(k * n);
    }
};

// the bytes of a launch, rounded up to 16; more than any CU has (so nothing fits) for a layout that misaligns an array
__host__ __device__ inline size_t lds_bytes(const Count& c) { return c.misaligned ? SIZE_MAX : (c.bytes + 15) / 16 * 16; }

// the bytes of the layout that `layout(arena)` takes: count([&](auto& a) { layout(a, nJ_max, nM_max); })
template <class Layout>
inline size_t count(Layout layout) {
    Count c;
    layout(c);
    return lds_bytes(c);
}

// the member-end lists of every joint (trs_recover.h), behind a layout's doubles
template <class Arena>
__host__ __device__ inline void take_end_lists(Arena& a, trs_rec::EndLists& t, int nJ_max, int nM_max) {
    t.cnt = a.template take<int>(nJ_max);
    t.start = a.template take<int>(nJ_max);   // [nJ_max + 1]
    a.template take<int>(1);
    t.ends = a.template take<int>(2, nM_max);
}

// Raises `Kernel`'s dynamic-LDS ceiling to the whole of a CU's, once per process and kernel, at its first launch.
// (Not at library load: raising ceilings up front faulted the CU-masked streams, order.hip / EXPERIMENTS R4.7.)
template <auto Kernel>
inline void raise_lds_once() {
    static const int set = (int)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)TRS_LDS_BYTES);
    (void)set;
}

}  // namespace trs_lds
