// Wave primitives of the search-tree kernels (one 64-lane wavefront per game):
// store ordering, DPP scans and reductions, readlane helpers and the 16-byte
// loads / stores of the node arrays. Device code shared by tree.hip,
// selfplay.hip and arena.hip (the library is built without relocatable device
// code, so it lives in a header).
#pragma once

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "engine.h"

namespace oamd {

__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }

__device__ __forceinline__ void wait_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Orders this wave's earlier global stores before its later loads of the same
// words, from any lane: the next descent / backup reads the statistics the
// previous one stored. A wavefront-scope fence: the AMDGPU memory model needs
// no wait for it on gfx950 (it emits none; a wave's vector memory operations
// reach the cache in order), so the stores' write-back overlaps the next
// descent's first loads instead of a vmcnt(0) drain per leaf.
// -DOAMD_TREE_DRAIN restores the vmcnt(0) drain (the A/B build that
// shows both orderings give identical results; tests/test_cpu_host.py checks
// in the ISA that k_tree reads no statistics through the scalar cache, which
// would not see these vector stores).
#ifdef OAMD_TREE_DRAIN
__device__ __forceinline__ void wave_order() { wait_stores(); }
#else
__device__ __forceinline__ void wave_order() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
#endif

// Wave reductions with DPP (row_shr / row_bcast inclusive scan, the total ends
// in lane 63): a few cycles per step, where __shfl_xor compiles to a chain of
// ds_bpermute LDS round trips (the dominant cost of a k_select level).
template <int CTRL, int ROW_MASK, int BANK_MASK, typename T>
__device__ __forceinline__ T dpp_move(T x, T id) {
    return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, id), __builtin_bit_cast(int, x),
                                                             CTRL, ROW_MASK, BANK_MASK, false));
}

template <typename T, typename Op>
__device__ __forceinline__ T wave_scan_last(T v, T id, Op op) {
    static_assert(sizeof(T) == 4, "32-bit lanes");
    T t = op(v, dpp_move<0x111, 0xF, 0xF>(v, id));  // row_shr:1
    t = op(t, dpp_move<0x112, 0xF, 0xF>(v, id));    // row_shr:2
    t = op(t, dpp_move<0x113, 0xF, 0xF>(v, id));    // row_shr:3
    t = op(t, dpp_move<0x114, 0xF, 0xE>(t, id));    // row_shr:4, banks 1-3
    t = op(t, dpp_move<0x118, 0xF, 0xC>(t, id));    // row_shr:8, banks 2-3
    t = op(t, dpp_move<0x142, 0xA, 0xF>(t, id));    // row_bcast:15 into rows 1, 3
    t = op(t, dpp_move<0x143, 0xC, 0xF>(t, id));    // row_bcast:31 into rows 2, 3
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), 63));
}

__device__ __forceinline__ int wave_sum(int v) {
    return wave_scan_last(v, 0, [](int a, int b) { return a + b; });
}

__device__ __forceinline__ float wave_max(float v) {
    return wave_scan_last(v, -__builtin_inff(), [](float a, float b) { return fmaxf(a, b); });
}

// The same scans over the first n lanes only (lanes >= n hold the identity):
// with n <= 16 (almost every node: Othello positions rarely have more legal
// moves) row 0 holds them all, so the two row_bcast steps are skipped and the
// total is read from lane 15.
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan_first_n(T v, T id, Op op, int n) {
    static_assert(sizeof(T) == 4, "32-bit lanes");
    T t = op(v, dpp_move<0x111, 0xF, 0xF>(v, id));  // row_shr:1
    t = op(t, dpp_move<0x112, 0xF, 0xF>(v, id));    // row_shr:2
    t = op(t, dpp_move<0x113, 0xF, 0xF>(v, id));    // row_shr:3
    t = op(t, dpp_move<0x114, 0xF, 0xE>(t, id));    // row_shr:4, banks 1-3
    t = op(t, dpp_move<0x118, 0xF, 0xC>(t, id));    // row_shr:8, banks 2-3
    if (n > 16) {
        t = op(t, dpp_move<0x142, 0xA, 0xF>(t, id));  // row_bcast:15 into rows 1, 3
        t = op(t, dpp_move<0x143, 0xC, 0xF>(t, id));  // row_bcast:31 into rows 2, 3
    }
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, t), n > 16 ? 63 : 15));
}

__device__ __forceinline__ int wave_max_i(int v) {
    return wave_scan_last(v, (int)0x80000000, [](int a, int b) { return a > b ? a : b; });
}

// First lane holding the maximum (strict '>' scan in child order,
// search_thread.cpp:222,254): the max, then the lowest lane equal to it.
// Values are finite or -inf (no NaN).
__device__ __forceinline__ int wave_argmax_first(float v, int) {
    const float m = wave_max(v);
    const uint64_t eq = __ballot(v == m);
    return __ffsll((unsigned long long)eq) - 1;
}

// ... over the first n lanes (the others hold -inf)
__device__ __forceinline__ int wave_argmax_first_n(float v, int n) {
    const float m = wave_scan_first_n(v, -__builtin_inff(), [](float a, float b) { return fmaxf(a, b); }, n);
    const uint64_t eq = __ballot(v == m);
    return __ffsll((unsigned long long)eq) - 1;
}

__device__ __forceinline__ int readlane_i(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
    return (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) |
           ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32);
}
__device__ __forceinline__ float readlane_f(float v, int l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

__device__ __forceinline__ NodeStat load_stat(const NodeStat* s) {
    const int4 v = *reinterpret_cast<const int4*>(s);
    NodeStat r;
    r.n = v.x;
    r.w = __int_as_float(v.y);
    r.q = __int_as_float(v.z);
    r.p = __int_as_float(v.w);
    return r;
}

__device__ __forceinline__ void store_stat(NodeStat* s, const NodeStat& r) {
    *reinterpret_cast<int4*>(s) =
        make_int4(r.n, __float_as_int(r.w), __float_as_int(r.q), __float_as_int(r.p));
}

__device__ __forceinline__ NodeLink load_link(const NodeLink* l) {
    const int4 v = *reinterpret_cast<const int4*>(l);
    return NodeLink{v.x, v.y, v.z, v.w};
}

__device__ __forceinline__ void store_link(NodeLink* l, const NodeLink& v) {
    *reinterpret_cast<int4*>(l) = make_int4(v.first_child, v.n_children, v.parent, v.player);
}

__device__ __forceinline__ Pos load_pos(const NodePos* p, int player) {
    Pos r;
    r.player = player;
    r.pad_ = 0;
    r.p1 = p->p1;
    r.p2 = p->p2;
    r.legal = p->legal;
    r.next_legal = p->next_legal;
    return r;
}

__device__ __forceinline__ void store_pos(NodePos* p, const Pos& v) {
    p->p1 = v.p1;
    p->p2 = v.p2;
    p->legal = v.legal;
    p->next_legal = v.next_legal;
}

}  // namespace oamd
