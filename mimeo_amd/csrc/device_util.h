// device_util.h — plane access and HOXD70 scoring shared by the extension kernels.
#pragma once
#include "common.h"

namespace mimeo {

// ---- global address space for pointers that come out of a device table -----------------------------------------------
// clang promotes a pointer that arrives as a kernel argument (also inside a by-value struct such as ExtQueues) to the
// global address space, and every access through it is a global_load / global_store.  A pointer that a kernel LOADS
// FROM MEMORY — the members of the StrandView / IndexView held in the UnitDesc, FusedUnit and Group tables — stays
// generic: every access through it is a flat_load, which may address LDS, so the compiler will not move it across an
// LDS store, waits for it on vmcnt AND lgkmcnt, and the hardware issues it to both paths.  gptr<T> is a read-only
// pointer that carries address space 1 in its type; the device-side twins below (GStrandView, GIndexView) hold their
// pointers in that form, and a kernel makes one where it copies a view out of its table (once per workgroup), so the
// loops behind it never see a generic pointer.  Not needed for kernel arguments (harmless there: the by-value A/B
// kernels go through the same device functions).  Only valid for device memory: every pointer the tables hold comes
// from hipMalloc, none is an LDS or scratch address.  HIP's uint2 / uint4 are classes whose copy constructors do not
// bind to an address-space-1 lvalue, so those load through the native vector of the same layout (free in the ISA).
#define MIMEO_AS_GLOBAL __attribute__((address_space(1)))
template <class T> struct gnative { using type = T; };
template <> struct gnative<uint2> { using type = uint32_t __attribute__((ext_vector_type(2))); };
template <> struct gnative<uint4> { using type = uint32_t __attribute__((ext_vector_type(4))); };
template <class T>
struct gptr {
    using N = typename gnative<T>::type;
    static_assert(sizeof(N) == sizeof(T), "the native twin has the layout of T");
    const MIMEO_AS_GLOBAL N *p;
    gptr() = default;
    __device__ __forceinline__ gptr(const T *q) : p((const MIMEO_AS_GLOBAL N *)q) {}
    __device__ __forceinline__ explicit gptr(const MIMEO_AS_GLOBAL N *q) : p(q) {}
    template <class I> __device__ __forceinline__ T operator[](I i) const { const N v = p[i]; return __builtin_bit_cast(T, v); }
    template <class I> __device__ __forceinline__ gptr operator+(I i) const { return gptr(p + i); }
    __device__ __forceinline__ explicit operator bool() const { return p != nullptr; }
    // the same address read as another type (reinterpret_cast of a plain pointer)
    template <class U> __device__ __forceinline__ gptr<U> as() const { return gptr<U>((const MIMEO_AS_GLOBAL typename gnative<U>::type *)p); }
};
struct GStrandView {   // StrandView (common.h) on the device
    gptr<uint4> pw;
    gptr<uint32_t> svt;
    gptr<uint2> p2;
    uint32_t len, has_n;
    GStrandView() = default;
    __device__ __forceinline__ GStrandView(const StrandView &v) : pw(v.pw), svt(v.svt), p2(v.p2), len(v.len), has_n(v.has_n) {}
};
struct GIndexView {    // IndexView
    gptr<uint32_t> off, pos;
    gptr<uint4> fr;
    uint32_t fr_stride, n;
    GIndexView() = default;
    __device__ __forceinline__ GIndexView(const IndexView &v) : off(v.off), pos(v.pos), fr(v.fr), fr_stride(v.fr_stride), n(v.n) {}
};
struct GFusedUnit {    // FusedUnit
    GIndexView T, Q;
    GStrandView Tv, Qv;
    uint32_t unit, same;
    uint64_t walk_base, walk_cap;
    GFusedUnit() = default;
    __device__ __forceinline__ GFusedUnit(const FusedUnit &u)
        : T(u.T), Q(u.Q), Tv(u.Tv), Qv(u.Qv), unit(u.unit), same(u.same), walk_base(u.walk_base), walk_cap(u.walk_cap) {}
};

// 12 care bits of the 19-bit window of the 12of19 seed 1110100110010101111: offsets {0,1,2,4,7,8,11,13,15,16,17,18}
__device__ __forceinline__ uint32_t pext12(uint32_t x) {
    return (x & 0x7u) | ((x >> 1) & 0x8u) | ((x >> 3) & 0x30u) | ((x >> 5) & 0x40u) | ((x >> 6) & 0x80u) |
           ((x >> 7) & 0xF00u);
}

// inclusive prefix sum of c over the 64 lanes of a wavefront: DPP (VALU latency), not six trips through the LDS crossbar
__device__ __forceinline__ uint32_t wave_inclusive_sum(uint32_t c) {
    uint32_t inc = c;
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x111, 0xf, 0xf, false);   // row_shr:1
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x112, 0xf, 0xf, false);   // row_shr:2
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x114, 0xf, 0xf, false);   // row_shr:4
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x118, 0xf, 0xf, false);   // row_shr:8
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x142, 0xa, 0xf, false);   // row_bcast:15
    inc += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)inc, 0x143, 0xc, 0xf, false);   // row_bcast:31
    return inc;
}

struct Win32 { uint32_t lo, hi, nm, sv; };
struct Win64 { uint64_t lo, hi, nm, sv; };

// 32 consecutive bases of every plane starting at (possibly negative, padded) base index s:
// two 16-byte loads, normally from the same cache line
__device__ __forceinline__ Win32 win32(const GStrandView &v, int32_t s) {
    const int32_t w = s >> 5;
    const uint32_t b = (uint32_t)s & 31u;
    const uint4 a = v.pw[w], c = v.pw[w + 1];
    Win32 r;
    r.lo = (uint32_t)((((uint64_t)c.x << 32) | a.x) >> b);
    r.hi = (uint32_t)((((uint64_t)c.y << 32) | a.y) >> b);
    r.nm = (uint32_t)((((uint64_t)c.z << 32) | a.z) >> b);
    r.sv = (uint32_t)((((uint64_t)c.w << 32) | a.w) >> b);
    return r;
}
// 64 consecutive bases of every plane
__device__ __forceinline__ Win64 win64(const GStrandView &v, int32_t s) {
    const int32_t w = s >> 5;
    const uint32_t b = (uint32_t)s & 31u;
    const uint4 a = v.pw[w], c = v.pw[w + 1], e = v.pw[w + 2];
    Win64 r;
    uint64_t l;
    l = ((uint64_t)c.x << 32) | a.x; r.lo = b ? (l >> b) | ((uint64_t)e.x << (64 - b)) : l;
    l = ((uint64_t)c.y << 32) | a.y; r.hi = b ? (l >> b) | ((uint64_t)e.y << (64 - b)) : l;
    l = ((uint64_t)c.z << 32) | a.z; r.nm = b ? (l >> b) | ((uint64_t)e.z << (64 - b)) : l;
    l = ((uint64_t)c.w << 32) | a.w; r.sv = b ? (l >> b) | ((uint64_t)e.w << (64 - b)) : l;
    return r;
}
// 32 bits of a plain (non-interleaved) plane
template <class P>   // const uint32_t * or gptr<uint32_t>
__device__ __forceinline__ uint32_t get32(const P pl, int32_t s) {
    int32_t w = s >> 5;
    uint32_t b = (uint32_t)s & 31u;
    uint64_t v = (uint64_t)pl[w] | ((uint64_t)pl[w + 1] << 32);
    return (uint32_t)(v >> b);
}
// seed-start validity of 32 starts in the role the view was made for
__device__ __forceinline__ uint32_t seedvalid32(const GStrandView &v, int32_t s, uint32_t sv_from_window) {
    return v.svt ? get32(v.svt, s) : sv_from_window;
}
// the three base bits at one position
struct Base1 { uint32_t lo, hi, nm; };
__device__ __forceinline__ Base1 base_at(const GStrandView &v, int32_t s) {
    const uint4 a = v.pw[s >> 5];
    const uint32_t b = (uint32_t)s & 31u;
    return Base1{(a.x >> b) & 1u, (a.y >> b) & 1u, (a.z >> b) & 1u};
}

// HOXD70 + N = -100 (lastz fill_score) from the difference planes: dl/dh = xor of the lo/hi
// planes, cg = target base is C or G, nn = either base is N.
constexpr uint32_t SUB_DL1 = 0x83858E8Eu, SUB_DL0 = 0xE1E1645Bu;  // {-114,-114,-123,-125} : {91,100,-31,-31}, one byte per (dh, cg)
constexpr int32_t SUB_N = -100;
__device__ __forceinline__ int32_t sub_score(uint32_t dl, uint32_t dh, uint32_t cg, uint32_t nn) {
    uint32_t tb = dl ? SUB_DL1 : SUB_DL0;
    uint32_t sh = 24u - (((dh << 1) | cg) << 3);
    int32_t s = ((int32_t)(tb << sh)) >> 24;
    return nn ? SUB_N : s;
}
// the largest and the smallest score a column can have: what sub_score can return, from its own tables
constexpr int32_t sub_extreme(bool largest) {
    int32_t e = SUB_N;
    for (int k = 0; k < 8; k++) {
        const int32_t b = (int32_t)(((k < 4 ? SUB_DL0 : SUB_DL1) >> (8 * (k & 3))) & 0xFFu), s = b >= 128 ? b - 256 : b;
        e = largest ? (s > e ? s : e) : (s < e ? s : e);
    }
    return e;
}
constexpr int32_t SUB_MAX = sub_extreme(true), SUB_MIN = sub_extreme(false);
static_assert(SUB_MAX == 100 && SUB_MIN == -125, "HOXD70");

// substitution score and match flag of target base pt against query base pq
__device__ __forceinline__ int32_t pair_score(const GStrandView &T, const GStrandView &Q, int32_t pt, int32_t pq,
                                              bool *is_match) {
    const Base1 a = base_at(T, pt), b = base_at(Q, pq);
    const uint32_t dl = a.lo ^ b.lo, dh = a.hi ^ b.hi, nn = a.nm | b.nm;
    *is_match = !(dl | dh | nn);
    return sub_score(dl, dh, a.lo ^ a.hi, nn);
}

}  // namespace mimeo
