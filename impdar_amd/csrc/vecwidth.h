// How the steps that stream a (snum, tnum) radargram pick their element type and access width: the vector of V
// consecutive traces a thread owns, its load, and the one place where the host chooses T and V for a launch.
#pragma once
#include <initializer_list>
#include <type_traits>
#include "common.h"

// at most 16 bytes of alignment: that is what the host checks, and the widest single access
template <typename T, int V> struct alignas(sizeof(T) * V < 16 ? sizeof(T) * V : 16) RwVec {
    T v[V];
};

// one access of V elements through the native vector type (the struct alone may be split into narrower loads)
template <typename T, int V> __device__ __forceinline__ RwVec<T, V> rw_load(const T *p)
{
    typedef T Native __attribute__((ext_vector_type(V)));
    const Native n = *reinterpret_cast<const Native *>(p);
    RwVec<T, V> r;
#pragma unroll
    for (int c = 0; c < V; ++c) r.v[c] = n[c];
    return r;
}

static inline bool rw_aligned16(const void *p) { return ((size_t)p & 15) == 0; }

// what the dispatchers hand to their callable: the element type and the access width, fixed at compile time
template <typename T> struct RwType {
    typedef T type;
};
template <int V> using RwWidth = std::integral_constant<int, V>;

// f(RwType<float>()) or f(RwType<double>()) for a dtype the caller has checked (impdar_dtype_ok)
template <class F> static auto rw_typed(int dtype, F &&f)
{
    return dtype == IMPDAR_F32 ? f(RwType<float>()) : f(RwType<double>());
}

// f(RwType<T>(), RwWidth<V>()) with the widest access every row start allows.  The kernels rely on tnum % V == 0
// (every row then starts on a multiple of the access width and no trace is left over) and on 16-byte accesses
// being aligned: 16 bytes (float32 x 4, float64 x 2) when every array of `ptrs` is 16-byte aligned and the row
// pitch a multiple of it, else a narrower form for the whole array; V = 1 serves every other trace count.  VMAX
// caps V for kernels that are not built wider.
template <int VMAX = 4, class F> static void rw_dispatch(int dtype, std::initializer_list<const void *> ptrs, int tnum, F &&f)
{
    bool wide = true;
    for (const void *p : ptrs) wide = wide && rw_aligned16(p);
    rw_typed(dtype, [&](auto t) {
        constexpr int in16 = 16 / (int)sizeof(typename decltype(t)::type);
        constexpr int full = in16 < VMAX ? in16 : VMAX;
        if constexpr (full >= 4) {
            if (wide && tnum % 4 == 0) return f(t, RwWidth<4>());
        }
        if constexpr (full >= 2) {
            if (wide && tnum % 2 == 0) return f(t, RwWidth<2>());
        }
        return f(t, RwWidth<1>());
    });
}
