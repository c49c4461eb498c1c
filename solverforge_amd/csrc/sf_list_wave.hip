// Wave-per-replica search engine (gfx950 / CDNA4, wave64) for the list-variable hot path.
//
// One 64-lane wavefront owns one search replica for the whole launch: its routes (flat CSR),
// per-route loads, node -> (route, position) table, per-leaf entity-order tables and the
// per-leaf candidate rings live in that wave's private slice of LDS.  Everything inside a
// replica is wave-synchronous (ballot / shuffle / prefix-scan, LDS in program order), so the
// kernel contains NO workgroup barrier; the CU hides a wave's memory latency behind the other
// replicas resident on it.  Same reference semantics as the block engine in
// sf_list_kernels.hip (citations there); what differs is the GPU formulation:
//
//  * generation reads a PRESORTED neighbour index (k_nbr_presort: every matrix row sorted by
//    (distance, node) once at sf_initialize, the matrix is an immutable problem fact) instead
//    of scanning the whole matrix row per source: the stable bounded top-k of
//    nearby_list_support.rs:3-34 is then "walk the row in distance order until max_nearby
//    valid destinations are complete", usually one 64-entry chunk;
//  * the (distance, enumeration ordinal) order inside a chunk is recovered by counting
//    inversions inside equal-distance groups (lanes are already distance-sorted), not by
//    serial insertion;
//  * trial scoring happens at replay time with all 64 lanes busy (lane i = i-th candidate of
//    the union cursor order), so the rings only hold move coordinates.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "sf_list_model.h"

namespace sf {

constexpr uint32_t RC_MAX = 128;   // ring capacity per leaf when max_nearby > 32 (>= 64 + 64 - 1)
constexpr uint32_t RC_SMALL = 64;  // ring capacity per leaf when max_nearby <= 32 (>= 32 + 32)
constexpr uint32_t NBR_NODE_MASK = 0x7FFFu;  // node id (dim <= 16384 in the wave engine)
constexpr uint32_t NBR_SAME_FLAG = 0x8000u;  // same distance as the previous entry of the row
constexpr uint32_t NBR_END = 0xFFFFu;        // past the finite entries of the row
#ifndef SF_WPB
#define SF_WPB 4
#endif
constexpr int WPB = SF_WPB;  // waves (= replicas) per workgroup

// Constants of the model the kernel runs (fixed when sf_initialize returns).  Each goes through a macro that is the identity in the shipped
// library; the device-only unit sf_tu_list_wave_spec.hip is compiled at run time with the macros defined as the context's literals
// (`-DSF_SPEC_V(x)=100`), so everything derived from them -- the WCarve offsets, ring mask, reciprocals, field widths -- folds.
#ifndef SF_SPEC_V
#define SF_SPEC_V(x) (x)
#endif
#ifndef SF_SPEC_DIM
#define SF_SPEC_DIM(x) (x)
#endif
#ifndef SF_SPEC_NCAP
#define SF_SPEC_NCAP(x) (x)
#endif
#ifndef SF_SPEC_K0
#define SF_SPEC_K0(x) (x)
#endif
#ifndef SF_SPEC_K1
#define SF_SPEC_K1(x) (x)
#endif
// Candidates beyond those five, each behind its own switch and kept in the unit's default only where it measured faster than the unit without
// it: the LateAcceptance history's size, the AcceptedCount limit, whether the internal node numbering exists (ListModel::perm /
// inv), whether explicit step seeds exist -- and SF_SPEC_MODEL_WORDS (level_words below): capacity, weights, depot and the level words.
#ifndef SF_SPEC_LA_SIZE
#define SF_SPEC_LA_SIZE(x) (x)
#endif
#ifndef SF_SPEC_LIMIT
#define SF_SPEC_LIMIT(x) (x)
#endif
#ifndef SF_SPEC_HAS_PERM
#define SF_SPEC_HAS_PERM(x) (x)
#endif
#ifndef SF_SPEC_HAS_EXPLICIT
#define SF_SPEC_HAS_EXPLICIT(x) (x)
#endif
// The run-time unit only (it defines SF_SPEC_L): the write-back forms its lane index again, behind an empty asm.  With V and n_cap literals the
// replica's per-lane addresses of the prologue's state load and of the write-back become the same expressions, and the compiler carried them
// across the whole step loop in scratch memory (16 B, 3 vector registers; the shipped kernels have none): DESIGN 21's finding, at another block.
#ifdef SF_SPEC_L
#define SF_SPEC_OWN_LANE(v) asm volatile("" : "+v"(v))
#else
#define SF_SPEC_OWN_LANE(v)
#endif
// Facts of the neighbour index, fixed like the constants above once sf_initialize has built it (sf_nbr_facts.h).
// The run-time unit may be compiled for them; every macro is the identity in the shipped library.
//   SF_SPEC_NO_WIDE    no equal-distance group has 64 members: gen_rest's serial top-k over the rest of a row is never reached
//   SF_SPEC_NO_TIES    no two entries of a row share a distance: no group has a second member, the inversion correction has nothing to do
//   SF_SPEC_ROWS_FULL  every row has min(dim, 64) finite entries and dim >= 32: no lane of the paired pass is past its row
//   SF_SPEC_TIE_KEY    (with SF_SPEC_RB = bits that hold V - 1, SF_SPEC_PB = bits that hold n_cap, RB + PB <= 22) the inversion correction
//                      compares one packed word per lane (tie_key_fix below); an inter-list ordinal is 1 << (RB + PB) | rank << PB | position
#ifdef SF_SPEC_NO_WIDE
#define SF_SPEC_WIDE_TIES(x) false
#else
#define SF_SPEC_WIDE_TIES(x) (x)
#endif
#ifdef SF_SPEC_NO_TIES
#define SF_SPEC_TIES(x) 0ULL
#else
#define SF_SPEC_TIES(x) (x)
#endif
#ifdef SF_SPEC_ROWS_FULL
#define SF_SPEC_ROW_HAVE(x) true
#define SF_SPEC_ROW_HAVEMASK(x) (~0ULL)
#else
#define SF_SPEC_ROW_HAVE(x) (x)
#define SF_SPEC_ROW_HAVEMASK(x) (x)
#endif


// wavefront-scope ordering of LDS/global traffic between lanes of one wave (no instruction cost:
// a wave executes in lockstep and its DS/VMEM queues are in order; this pins the compiler).
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---------------------------------------------------------------------------------------
// Neighbour index: bitonic sort of every matrix row in LDS.  grid = dim rows.
// ---------------------------------------------------------------------------------------
SF_PLAIN_KERNEL
__global__ __launch_bounds__(256) void k_nbr_presort(const int64_t* __restrict__ mat, int dim, int P,
                                                     uint16_t* __restrict__ keys) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* sk = (uint64_t*)smem;
    const int row = blockIdx.x;
    const int64_t* rp = mat + (size_t)row * dim;
    for (int t = threadIdx.x; t < P; t += blockDim.x) {
        uint64_t k = ~0ULL;
        if (t < dim) {
            const int64_t v = rp[t];
            if (v >= 0 && v != UNREACHABLE) k = ((uint64_t)v << 24) | (uint64_t)(uint32_t)t;  // finite_distance (problem_data.rs:44-47)
        }
        sk[t] = k;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += blockDim.x) {
                const int lo = (t / stride) * 2 * stride + (t % stride);
                const int hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t a = sk[lo], b = sk[hi];
                if ((a > b) == up) {
                    sk[lo] = b;
                    sk[hi] = a;
                }
            }
            __syncthreads();
        }
    for (int t = threadIdx.x; t < dim; t += blockDim.x) {
        const uint64_t k = sk[t];
        uint32_t e = NBR_END;
        if (k != ~0ULL) {
            e = (uint32_t)k & NBR_NODE_MASK;
            if (t > 0 && (sk[t - 1] >> 24) == (k >> 24)) e |= NBR_SAME_FLAG;
        }
        keys[(size_t)row * dim + t] = (uint16_t)e;
    }
}

// LDS carve of ONE replica (bytes); mirrored on the host.
struct WCarve {
    size_t load, off, node, ring, visits, rtab, routeat, total;
    uint32_t rc;  // ring capacity per leaf
    // compact: the COMPACT instantiation's layout -- per-list loads as int32 (MODE 2 guarantees the range) and the node -> slot
    // table as 16 bits per node (NodeSlotT<true>): CVRP-5000 / 500 drops from 43 KB to 31 KB per replica (3 -> 5 replicas per CU)
    // node_global: the node -> slot table lives in HBM (ListModel::node_tab), not in the slice
    __host__ __device__ WCarve(int V, int n_cap, int dim, int max_k, bool compact = false, bool node_global = false) {
        rc = max_k <= 32 ? RC_SMALL : RC_MAX;
        size_t o = 0;
        load = o;
        o = align_up(o + (compact ? sizeof(int32_t) : sizeof(int64_t)) * V, 16);
        off = o;
        o = align_up(o + (node_global ? sizeof(uint16_t) : sizeof(uint32_t)) * (V + 1), 16);  // (node_global layout: 16-bit offsets, n_cap <= 65535)
        node = o;
        o = align_up(o + (node_global ? 0 : (compact ? sizeof(uint16_t) : sizeof(uint32_t)) * dim), 16);
        ring = o;
        o = align_up(o + sizeof(uint32_t) * 2 * rc * MAX_LEAVES, 16);
        visits = o;
        o = align_up(o + sizeof(uint16_t) * n_cap, 16);
        rtab = o;  // [leaf][route] u32: rank of the route in the leaf's entity order | first destination slot ordinal << 16
        o = align_up(o + (node_global ? 0 : sizeof(uint32_t) * V * MAX_LEAVES), 16);  // (the node_global layout computes ranks instead: RouteArith)
        routeat = o;  // [leaf][rank] -> route; the compact layout recomputes it from the leaf's permutation parameters instead
        o = align_up(o + (compact ? 0 : sizeof(uint16_t) * V * MAX_LEAVES), 16);
        total = o;
    }
};

// node -> (route << 16 | position) of the replica's current lists.  Wide: one u32 per node.  Compact: one u16 per node,
// route in the top `rb` bits and the position below; a position that does not fit the field is stored as the field's maximum
// and found by scanning the route from there (routes that long are rare: the field holds 127 positions at 500 routes, 511 at
// 100); the all-ones pattern means "in no list".  get() returns the wide form either way.
template <bool COMPACT>
struct NodeSlotT;
template <>
struct NodeSlotT<false> {
    uint32_t* p;
    __device__ __forceinline__ NodeSlotT(unsigned char* base, int, const uint16_t*, const void*, bool = false) : p((uint32_t*)base) {}
    __device__ __forceinline__ void clear(uint32_t node) const { p[node] = NODE_NONE; }
    __device__ __forceinline__ void set(uint32_t node, uint32_t route, uint32_t pos) const { p[node] = (route << 16) | pos; }
    __device__ __forceinline__ uint32_t get(uint32_t node) const { return p[node]; }
    // the table word, and its wide form (the same thing in this layout): see NodeSlotT<true>
    __device__ __forceinline__ uint32_t word(uint32_t node) const { return p[node]; }
    __device__ __forceinline__ uint32_t wide(uint32_t s, uint32_t) const { return s; }
    __device__ __forceinline__ uint32_t wide_short(uint32_t s) const { return s; }
};
template <>
struct NodeSlotT<true> {
    uint16_t* p;
    const uint16_t* visits;
    const void* off;  // uint32_t[V + 1], or uint16_t[V + 1] when off16
    bool off16;
    uint32_t pb, pmax;  // position bits, the saturated position
    __device__ __forceinline__ uint32_t off_at(uint32_t i) const { return off16 ? (uint32_t)((const uint16_t*)off)[i] : ((const uint32_t*)off)[i]; }
    __device__ __forceinline__ NodeSlotT(unsigned char* base, int V, const uint16_t* visits_, const void* off_, bool off16_ = false)
        : p((uint16_t*)base), visits(visits_), off(off_), off16(off16_) {
        uint32_t rb = 1;
        while ((1u << rb) - 1u < (uint32_t)V) ++rb;  // route ids 0 .. V - 1, the all-ones route is "none"
        pb = 16u - rb;
        pmax = (1u << pb) - 1u;
    }
    __device__ __forceinline__ void clear(uint32_t node) const { p[node] = 0xFFFFu; }
    __device__ __forceinline__ void set(uint32_t node, uint32_t route, uint32_t pos) const {
        p[node] = (uint16_t)((route << pb) | (pos < pmax ? pos : pmax));
    }
    __device__ __forceinline__ uint32_t get(uint32_t node) const { return wide(p[node], node); }
    // get() in two halves, for a caller that wants the LDS read in flight while it does something else: word() is the read, wide() / wide_short()
    // turn the word into (route << 16 | position)
    __device__ __forceinline__ uint32_t word(uint32_t node) const { return p[node]; }
    __device__ __forceinline__ uint32_t wide(uint32_t s, uint32_t node) const {
        const bool none = s == 0xFFFFu;
        const uint32_t route = s >> pb;
        uint32_t pos = s & pmax;
        // saturated: the node sits at position >= pmax of its route.  Rare (routes that long), so the test is ONE wave-uniform branch
        // on a ballot and the common path has no exec-mask region at all
        if (__ballot(!none && pos == pmax) != 0ull) {
            if (!none && pos == pmax) {
                const uint32_t o = off_at(route), len = off_at(route + 1) - o;
                while (pos + 1 < len && (uint32_t)visits[o + pos] != node) ++pos;
            }
        }
        return none ? NODE_NONE : ((route << 16) | pos);
    }
    // wide() for a caller that KNOWS no route is longer than pmax (no position is stored saturated): the word decoded, nothing tested
    __device__ __forceinline__ uint32_t wide_short(uint32_t s) const {
        const uint32_t w = ((s >> pb) << 16) | (s & pmax);
        return s == 0xFFFFu ? NODE_NONE : w;
    }
};
// does the compact layout carry this model?  route ids need a bit pattern below all-ones, positions at least 6 bits
__host__ __device__ inline bool node_slot_compact_ok(int V) { return V >= 1 && V <= 1022; }

// One neighbour-row entry seen from source (se, sp) of a leaf: up to two consecutive keys
// (destination slot dp, and the end slot of its route when the node is the last element).
struct NearbyItem {
    uint32_t w;     // number of valid keys (0, 1, 2)
    uint32_t ord;   // enumeration ordinal of the first valid key (the second is ord + 1)
    uint32_t pay0;  // (route << 16 | position) of the first valid key
    uint32_t pay1;  // second key
};

__device__ __forceinline__ NearbyItem nearby_item(bool is_change, uint32_t slot, uint32_t se, uint32_t sp,
                                                  uint32_t len, uint32_t k, const uint32_t* s_off,
                                                  const uint16_t* sb, const uint16_t* ro) {
    // branch-free: every lane reads its route's length / rank / slot base (route 0 for unassigned nodes)
    const bool some = slot != NODE_NONE;
    const uint32_t r2 = some ? slot >> 16 : 0u, dp = slot & 0xFFFFu;
    const uint32_t len2 = s_off[r2 + 1] - s_off[r2];
    const uint32_t rk = ro[r2];
    const uint32_t inter_ord = ORD_INTER_BASE + (uint32_t)sb[rk] + dp;
    const bool intra = r2 == se;
    const uint32_t end_pay = (r2 << 16) | len2;
    NearbyItem it;
    if (is_change) {  // nearby_change.rs:133-195
        const bool v0 = !intra || (dp != sp && dp != sp + 1);
        const bool v1 = dp + 1 == len2 && (!intra || len != sp + 1);  // end slot `len` probes element len-1
        it.w = some ? (uint32_t)v0 + (uint32_t)v1 : 0u;
        it.ord = intra ? (v0 ? dp : len) : inter_ord;
        it.pay0 = v0 ? slot : end_pay;
        it.pay1 = end_pay;
    } else {  // nearby_swap.rs: intra partners after the source, inter only higher-ranked entities
        const bool v = intra ? dp > sp : rk > k;
        it.w = (some && v) ? 1u : 0u;
        it.ord = intra ? dp : inter_ord;
        it.pay0 = slot;
        it.pay1 = 0;
    }
    return it;
}

// Same item with the per-route facts read from ONE packed table (wave engine): rt[route] = rank of the route in the
// leaf's entity order | ordinal of the route's first destination slot << 16 — one LDS gather instead of the dependent
// pair rank_of[route] -> slot_base[rank].
// The per-route facts of a leaf's entity order as a table (RouteTab: the word above) or as arithmetic (RouteArith, the wave kernel whose tables live in HBM):
// the entity order is the permutation rank -> (start + rank x stride) mod V, so the rank of a route is ((route - start) x stride^-1) mod V
// -- a handful of vector instructions instead of a table that is rebuilt every step (and, in the layout whose tables live in HBM, instead
// of a dependent global gather per row entry).  The enumeration ordinal of an inter-list slot only ever breaks ties inside one
// equal-distance group, i.e. it is compared, never added up: (rank, position) compares exactly like first-slot-ordinal-of-rank + position,
// so the arithmetic form needs no prefix sum over the lists either.
struct RouteTab {
    const uint32_t* rt;
    static constexpr int KEY_SHIFT = 24;  // serial top-k key = distance << KEY_SHIFT | ordinal
    __device__ __forceinline__ uint32_t word(uint32_t route) const { return rt[route]; }
    __device__ __forceinline__ static uint32_t rank(uint32_t w) { return w & 0xFFFFu; }
    __device__ __forceinline__ static uint32_t inter_ord(uint32_t w, uint32_t dp) { return ORD_INTER_BASE + (w >> 16) + dp; }
};
#ifdef SF_SPEC_TIE_KEY
// the same order in the fewest bits (positions <= n_cap < 2^PB, ranks <= V - 1 < 2^RB): an ordinal stays below 2^(RB + PB + 1) <= 2^23
static_assert(SF_SPEC_RB >= 1 && SF_SPEC_PB >= 1 && SF_SPEC_RB + SF_SPEC_PB <= 22, "SF_SPEC_TIE_KEY: the packed word does not fit 32 bits");
constexpr uint32_t ORD_ARITH_BASE = 1u << (SF_SPEC_RB + SF_SPEC_PB);
constexpr int ORD_ARITH_SHIFT = SF_SPEC_PB;
#else
constexpr uint32_t ORD_ARITH_BASE = 1u << 26;  // above every intra-list ordinal (a position, < 2^16); rank << 16 | position stays below 2^27
constexpr int ORD_ARITH_SHIFT = 16;
#endif
struct RouteArith {
    uint32_t st, inv, V, recip;  // permutation start, stride^-1 mod V, V, floor(2^32 / V) (V <= 1022: every product below stays under 2^21)
    static constexpr int KEY_SHIFT = 28;  // (the legs of a COMPACT kernel are < 2^26)
    __device__ __forceinline__ uint32_t word(uint32_t route) const {
        uint32_t x = route + V - st;
        x = x >= V ? x - V : x;
        const uint32_t y = x * inv;
        uint32_t rk = y - __umulhi(y, recip) * V;  // 32-bit Barrett step: the quotient estimate is exact or one short
        return rk >= V ? rk - V : rk;
    }
    __device__ __forceinline__ static uint32_t rank(uint32_t w) { return w; }
    __device__ __forceinline__ static uint32_t inter_ord(uint32_t w, uint32_t dp) { return ORD_ARITH_BASE + (w << ORD_ARITH_SHIFT) + dp; }
};
struct RouteRank {  // RouteTab's table holding the rank alone, RouteArith's ordinals
    const uint32_t* rt;
    static constexpr int KEY_SHIFT = RouteArith::KEY_SHIFT;
    __device__ __forceinline__ uint32_t word(uint32_t route) const { return rt[route]; }
    __device__ __forceinline__ static uint32_t rank(uint32_t w) { return w; }
    __device__ __forceinline__ static uint32_t inter_ord(uint32_t w, uint32_t dp) { return RouteArith::inter_ord(w, dp); }
};
template <class OT, class RT>
__device__ __forceinline__ NearbyItem nearby_item_rt(bool is_change, uint32_t slot, uint32_t se, uint32_t sp,
                                                     uint32_t len, uint32_t k, const OT* s_off, const RT& rt) {
    const bool some = slot != NODE_NONE;
    const uint32_t r2 = some ? slot >> 16 : 0u, dp = slot & 0xFFFFu;
    const uint32_t len2 = s_off[r2 + 1] - s_off[r2];
    const uint32_t t = rt.word(r2);
    const uint32_t rk = RT::rank(t);
    const uint32_t inter_ord = RT::inter_ord(t, dp);
    const bool intra = r2 == se;
    const uint32_t end_pay = (r2 << 16) | len2;
    NearbyItem it;
    if (is_change) {  // nearby_change.rs:133-195
        const bool v0 = !intra || (dp != sp && dp != sp + 1);
        const bool v1 = dp + 1 == len2 && (!intra || len != sp + 1);  // end slot `len` probes element len-1
        it.w = some ? (uint32_t)v0 + (uint32_t)v1 : 0u;
        it.ord = intra ? (v0 ? dp : len) : inter_ord;
        it.pay0 = v0 ? slot : end_pay;
        it.pay1 = end_pay;
    } else {  // nearby_swap.rs: intra partners after the source, inter only higher-ranked entities
        const bool v = intra ? dp > sp : rk > k;
        it.w = (some && v) ? 1u : 0u;
        it.ord = intra ? dp : inter_ord;
        it.pay0 = slot;
        it.pay1 = 0;
    }
    return it;
}

// number of set bits of `mask` below this lane (v_mbcnt: no LDS crossbar involved)
__device__ __forceinline__ uint32_t mbcnt64(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}
#ifdef SF_SPEC_TIE_KEY
// The inversion correction of a lane's sorted position inside its equal-distance group on ONE packed word per lane,
//   Q = group << (RB + PB + 3) | ordinal << 2 | weight,
// `group` = the group starts in lanes 1 .. lane (the inclusive count less lane 0's own bit in every lane alike; <= 63).  It never decreases
// with the lane, so "the lane d away is in my group" and "its ordinal is on the other side of mine" are one unsigned compare: the lane d
// above (a later row entry) precedes me exactly when its Q is below mine, the lane d below follows me exactly when its Q is above mine.  What
// is added is the OTHER lane's weight, so a lane past the wave (bound_ctrl: Q = 0), a lane past the row, a lane of the group still open and
// a lane whose node is unassigned -- whose ordinal may be anything, the group field included -- add zero, and what such a lane works out for
// itself is never stored.  Lanes of non-zero weight in one group never share an ordinal (they address distinct slots), so equal ordinals
// only meet a zero weight.  `nonstart` = the closed lanes that continue the group of the lane before; the trip count is the widest closed
// group's width less one, by the wave-uniform recurrence of the general form.
__device__ __forceinline__ int32_t tie_key_fix(uint64_t startmask, uint64_t nonstart, uint32_t ord, uint32_t wc) {
    const uint32_t q = (mbcnt64(startmask >> 1) << (SF_SPEC_RB + SF_SPEC_PB + 3)) | (ord << 2) | wc;
    uint32_t q_dn = q, q_up = q;
    int32_t fix = 0;
    uint64_t run = nonstart;  // bit t: lanes t-d .. t are one group
    for (uint32_t d = 1; run != 0; ++d) {
        q_dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q_dn, 0x130, 0xf, 0xf, true);  // wave_shl:1: lane i <- lane i + d
        q_up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)q_up, 0x138, 0xf, 0xf, true);  // wave_shr:1: lane i <- lane i - d
        fix += q_dn < q ? (int32_t)(q_dn & 3u) : 0;
        fix -= q_up > q ? (int32_t)(q_up & 3u) : 0;
        run &= nonstart << d;
    }
    return fix;
}
#endif

// Committed move application on the wave's LDS state (ListChange / ListSwap do_move).
// OWN_LANE: the lane index is formed again here, behind an empty asm -- for a caller with no vector register to spare, whose compiler would otherwise
// compute this block's per-lane addresses in the kernel's prologue and carry them to it through scratch memory
template <class LT, class OT, bool OWN_LANE = false>  // LT = the replica's per-list load type in LDS: int64_t, or int32_t in the COMPACT wave layout; OT = offsets, uint32_t or uint16_t
__device__ __forceinline__ void apply_list_move_wave(const ListModel& m, uint16_t* visits, OT* off,
                                                     LT* load, int kind, uint32_t a, uint32_t i, uint32_t b,
                                                     uint32_t j, uint32_t ext = 0) {
    uint32_t lane = threadIdx.x & 63u;
    if constexpr (OWN_LANE) asm volatile("" : "+v"(lane));
    if (kind == 2) {
        const uint32_t P = off[a] + i, Q = off[b] + j;
        const uint32_t x = visits[P];
        wave_sync();
        if (P < Q) {  // [P, Q-2] <- t+1 ; Q-1 <- x   (ascending chunks: reads run ahead of writes)
            for (uint32_t t0 = P; t0 < Q; t0 += 64) {
                const uint32_t t = t0 + lane;
                uint32_t nv = 0;
                if (t < Q) nv = (t + 1 < Q) ? (uint32_t)visits[t + 1] : x;
                wave_sync();
                if (t < Q) visits[t] = (uint16_t)nv;
                wave_sync();
            }
        } else if (P > Q) {  // (Q, P] <- t-1 ; Q <- x   (descending chunks)
            for (uint32_t c0 = 0; c0 <= P - Q; c0 += 64) {
                const uint32_t dd = c0 + lane;
                const bool in = dd <= P - Q;
                const uint32_t t = P - (in ? dd : 0u);
                uint32_t nv = 0;
                if (in) nv = t > Q ? (uint32_t)visits[t - 1] : x;
                wave_sync();
                if (in) visits[t] = (uint16_t)nv;
                wave_sync();
            }
        }
        if (a != b) {
            for (uint32_t rr = lane; rr <= (uint32_t)SF_SPEC_V(m.V); rr += 64) {
                if (a < b && rr > a && rr <= b) off[rr] -= 1;
                if (a > b && rr > b && rr <= a) off[rr] += 1;
            }
            if (lane == 0 && m.demand) {
                const int64_t dx = (int64_t)m.demand[x];
                load[a] = (LT)wsub(load[a], dx);
                load[b] = (LT)wadd(load[b], dx);
            }
        }
    } else if (kind == 6) {  // sublist swap: [i, i + (ext & 0xFFFF)) of a <-> [j, j + (ext >> 16)) of b
        const uint32_t za = ext & 0xFFFFu, zb = ext >> 16;
        const uint32_t PA = off[a] + i, PB = off[b] + j;
        const bool a_first = PA < PB;
        const uint32_t PX = a_first ? PA : PB, zx = a_first ? za : zb, PY = a_first ? PB : PA, zy = a_first ? zb : za;
        const uint32_t ox = a_first ? a : b, oy = a_first ? b : a;
        int64_t da = 0, db = 0;
        if (a != b && m.demand) {
            for (uint32_t t = 0; t < za; ++t) da = wadd(da, (int64_t)m.demand[visits[PA + t]]);
            for (uint32_t t = 0; t < zb; ++t) db = wadd(db, (int64_t)m.demand[visits[PB + t]]);
        }
        wave_sync();
        relocate_flat_segment(visits, PY, zy, PX, lane, 64u, [] { wave_sync(); });            // Y X mid
        relocate_flat_segment(visits, PX + zy, zx, PY + zy, lane, 64u, [] { wave_sync(); });  // Y mid X
        if (a != b) {
            for (uint32_t rr = lane; rr <= (uint32_t)SF_SPEC_V(m.V); rr += 64)
                if (rr > ox && rr <= oy) off[rr] = off[rr] + zy - zx;
            if (lane == 0 && m.demand) {
                load[a] = (LT)wadd(wsub(load[a], da), db);
                load[b] = (LT)wadd(wsub(load[b], db), da);
            }
        }
    } else if (kind == 5) {  // sublist change: segment [i, ext) of list a -> list b at j
        const uint32_t z = ext - i, P = off[a] + i;
        const uint32_t Q = a != b ? off[b] + j : (j <= i ? off[a] + j : off[a] + j + z);
        int64_t dsum = 0;
        if (a != b && m.demand)
            for (uint32_t t = 0; t < z; ++t) dsum = wadd(dsum, (int64_t)m.demand[visits[P + t]]);
        wave_sync();
        relocate_flat_segment(visits, P, z, Q, lane, 64u, [] { wave_sync(); });
        if (a != b) {
            for (uint32_t rr = lane; rr <= (uint32_t)SF_SPEC_V(m.V); rr += 64) {
                if (a < b && rr > a && rr <= b) off[rr] -= z;
                if (a > b && rr > b && rr <= a) off[rr] += z;
            }
            if (lane == 0 && m.demand) {
                load[a] = (LT)wsub(load[a], dsum);
                load[b] = (LT)wadd(load[b], dsum);
            }
        }
    } else if (kind == 4) {  // reverse [i, j) of list a
        const uint32_t lo = off[a] + i, hi = off[a] + j;
        for (uint32_t t = lane; t < (hi - lo) / 2; t += 64) {
            const uint16_t x = visits[lo + t], y = visits[hi - 1 - t];
            visits[lo + t] = y;
            visits[hi - 1 - t] = x;
        }
    } else if (kind == 9) {  // permute the window [i, j) of list a by the ext-th permutation of its positions
        const uint32_t base = off[a] + i, size = j - i;
        const uint32_t perm = nth_permutation_nibbles(size, ext);
        uint32_t nv = 0;
        if (lane < size) nv = visits[base + ((perm >> (4u * lane)) & 15u)];
        wave_sync();
        if (lane < size) visits[base + lane] = (uint16_t)nv;
    } else if (kind == 7) {  // 3-opt: cuts i < b < j of list a (b carries the middle cut), pattern = ext
        const uint32_t base = off[a], c1 = i, c2 = b, c3 = j;
        const uint32_t mask = kopt_reverse_mask(ext);
        const bool rb = (mask >> 1) & 1u, rc = (mask >> 2) & 1u;
        auto reverse_range = [&](uint32_t lo, uint32_t hi) {
            for (uint32_t t = lane; t < (hi - lo) / 2; t += 64) {
                const uint16_t x = visits[base + lo + t], y = visits[base + hi - 1 - t];
                visits[base + lo + t] = y;
                visits[base + hi - 1 - t] = x;
            }
            wave_sync();
        };
        if (!kopt_swaps_segments(ext)) {
            if (rb) reverse_range(c1, c2);
            if (rc) reverse_range(c2, c3);
        } else {
            const uint32_t zc = c3 - c2;
            reverse_range(c1, c3);
            if (!rc) reverse_range(c1, c1 + zc);
            if (!rb) reverse_range(c1 + zc, c3);
        }
    } else if (kind == 3) {
        if (lane == 0) {
            const uint32_t pa = off[a] + i, pb = off[b] + j;
            const uint16_t x = visits[pa], y = visits[pb];
            visits[pa] = y;
            visits[pb] = x;
            if (a != b && m.demand) {
                const int64_t dx = (int64_t)m.demand[x], dy = (int64_t)m.demand[y];
                load[a] = (LT)wadd(wsub(load[a], dx), dy);
                load[b] = (LT)wadd(wsub(load[b], dy), dx);
            }
        }
    }
    wave_sync();
}

// One nearby source into a leaf ring (free-function form of the wave engine's generation loop, used
// by the generic N-leaf engine): walks the presorted neighbour row of element `sx` from offset
// `base`, `key` = the 64 row entries at base; appends at ring position tl + emitted; returns the
// number of candidates appended so far.
__device__ __forceinline__ uint32_t nearby_source_to_ring(const ListModel& m, const NbrIndex& nb, bool is_change, uint32_t se,
                                                          uint32_t sp, uint32_t len, uint32_t k, uint32_t sx,
                                                          const uint32_t* node_slot, const uint32_t* s_off, const uint16_t* sb,
                                                          const uint16_t* ro, uint32_t* rq, uint32_t RCM, uint32_t tl,
                                                          uint32_t key, uint32_t base, uint32_t need, uint32_t emitted) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t lanebit = 1ULL << lane;
    const uint32_t dim = (uint32_t)m.dim;
    const uint16_t* rowk = nb.keys + (size_t)sx * dim;
    const uint32_t mv0 = (se << 16) | sp;
    for (;;) {
        const bool have = key != NBR_END;
        const uint64_t havemask = __ballot(have);
        if (havemask == 0) break;  // finite entries of the row exhausted
        NearbyItem it{0u, 0u, 0u, 0u};
        if (have) it = nearby_item(is_change, node_slot[key & NBR_NODE_MASK], se, sp, len, k, s_off, sb, ro);
        // equal-distance groups are contiguous lane ranges; the index marks entries that
        // continue the previous entry's distance
        const uint64_t startmask = __ballot(have && (lane == 0 || !(key & NBR_SAME_FLAG)));
        const bool more = havemask == ~0ULL && base + 64 < dim;
        const uint32_t fo = 63u - (uint32_t)__clzll((unsigned long long)startmask);  // first lane of the last group
        if (more && fo == 0) {
            // one distance group wider than a chunk (degenerate ties): exact serial
            // insertion top-k over the rest of the row.
            TopK tk{~0ULL, 0u, ~0ULL};
            for (uint32_t b2 = base; b2 < dim; b2 += 64) {
                const uint32_t j2 = b2 + lane;
                const uint32_t ky = j2 < dim ? (uint32_t)rowk[j2] : NBR_END;
                NearbyItem i2{0u, 0u, 0u, 0u};
                uint64_t hk = 0;
                if (ky != NBR_END) {
                    const uint32_t y2 = ky & NBR_NODE_MASK;
                    i2 = nearby_item(is_change, node_slot[y2], se, sp, len, k, s_off, sb, ro);
                    hk = (uint64_t)m.mat[(size_t)sx * dim + y2] << 24;  // finite by construction of the index
                }
                if (!__ballot(ky != NBR_END)) break;
                topk_offer(tk, need, i2.w >= 1 ? (hk | i2.ord) : ~0ULL, i2.pay0);
                topk_offer(tk, need, i2.w == 2 ? (hk | (i2.ord + 1)) : ~0ULL, i2.pay1);
            }
            const uint32_t cnt = (uint32_t)__popcll(__ballot(lane < need && tk.key != ~0ULL));
            if (lane < cnt) {
                const uint32_t qi = (tl + emitted + lane) & RCM;
                rq[qi * 2] = mv0;
                rq[qi * 2 + 1] = tk.pay;
            }
            emitted += cnt;
            break;
        }
        const uint32_t nclosed = more ? fo : (uint32_t)__popcll(havemask);  // lanes [0, nclosed): complete groups
        const uint64_t closedmask = nclosed >= 64 ? ~0ULL : ((1ULL << nclosed) - 1ULL);
        const bool closed = (closedmask & lanebit) != 0;
        const uint32_t wc = closed ? it.w : 0u;
        const uint64_t w1 = __ballot(wc == 1), w2 = __ballot(wc == 2);
        const uint32_t Wc = (uint32_t)__popcll(w1) + 2u * (uint32_t)__popcll(w2);
        if (Wc > 0) {
            // sorted position = weight before me, corrected by the inversions inside my group
            int32_t pos = (int32_t)(mbcnt64(w1) + 2u * mbcnt64(w2));
            const uint64_t nonstart = ~startmask & closedmask;  // lane continues the group of lane-1
            if (nonstart) {
                const uint32_t packed = (it.ord << 2) | wc;
                uint64_t run = nonstart;  // bit t: lanes t-d .. t are one group
                for (uint32_t d = 1; run != 0; ++d) {
                    const uint32_t p_dn = __shfl_down(packed, d), p_up = __shfl_up(packed, d);
                    const bool same_up = (run & lanebit) != 0;
                    const bool same_dn = ((run >> d) & lanebit) != 0;
                    if (same_dn && (p_dn >> 2) < it.ord) pos += (int32_t)(p_dn & 3u);
                    if (same_up && (p_up >> 2) > it.ord) pos -= (int32_t)(p_up & 3u);
                    run &= nonstart << d;
                }
            }
            if (wc >= 1 && (uint32_t)pos < need) {
                const uint32_t qi = (tl + emitted + (uint32_t)pos) & RCM;
                rq[qi * 2] = mv0;
                rq[qi * 2 + 1] = it.pay0;
            }
            if (wc == 2 && (uint32_t)pos + 1 < need) {
                const uint32_t qi = (tl + emitted + (uint32_t)pos + 1) & RCM;
                rq[qi * 2] = mv0;
                rq[qi * 2 + 1] = it.pay1;
            }
            const uint32_t ne = Wc < need ? Wc : need;
            emitted += ne;
            need -= ne;
        }
        if (need == 0 || !more) break;
        base += nclosed;
        const uint32_t jj = base + lane;
        key = jj < dim ? (uint32_t)rowk[jj] : NBR_END;
    }
    return emitted;
}

// SF_WAVE_SYM: the lockstep round of the RBATCH kernels.  -DSF_WAVE_SYM=0 compiles the loop without it; the run-time unit takes the
// same define from the environment switch SF_AMD_NO_WAVE_SYM, read once per process (sf_wave_spec.h).
#ifndef SF_WAVE_SYM
#define SF_WAVE_SYM 1
#endif

#if defined(SF_PHASE_PROFILE) || defined(SF_GEN_COUNT)
#ifdef SF_GEN_COUNT
#define SF_PHASE_WORDS 10
#else
#define SF_PHASE_WORDS 8
#endif
__device__ unsigned long long g_phase[SF_PHASE_WORDS];
#endif
// analysis builds (-DSF_ISA_MARK): comments in the generated assembly that delimit the hot regions, for static instruction counts per region
#ifdef SF_ISA_MARK
#define ISA_MARK(name) asm volatile("; SF_MARK " name)
#else
#define ISA_MARK(name)
#endif
#if defined(SF_PHASE_PROFILE) && !defined(SF_PHASE_PGRP)  // (SF_PHASE_PGRP: the slots belong to the stages of prec_eval_grouped, sf_prec_group.h)
#define PH_DECL uint64_t ph_t = clock64(), ph_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define PH(i)                          \
    {                                  \
        const uint64_t _t = clock64(); \
        ph_acc[i] += _t - ph_t;        \
        ph_t = _t;                     \
    }
#define PH_DUMP \
    if (lane == 0) for (int _k = 0; _k < 8; ++_k) atomicAdd(&g_phase[_k], (unsigned long long)ph_acc[_k]);
#elif defined(SF_GEN_COUNT)  // event counts of the generation instead of clocks (scripts/gen_count.py): 0 paired passes, 1 / 2 single-source passes of leaf 0 / 1,
// 3 / 4 gen_rest calls out of a paired pass for leaf 0 / 1, 5 / 6 gen_rest chunk iterations of leaf 0 / 1, 7 iterations that found no key,
// 8 paired passes of the lockstep round (they count in 0 too), 9 exits from the round into the general loop
#define PH_DECL uint64_t ph_acc[SF_PHASE_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#define PH(i)
#define GC(i) ph_acc[i] += 1;
#define PH_DUMP \
    if (lane == 0) for (int _k = 0; _k < SF_PHASE_WORDS; ++_k) atomicAdd(&g_phase[_k], (unsigned long long)ph_acc[_k]);
#else
#define PH_DECL
#define PH(i)
#define PH_DUMP
#endif
#ifndef GC
#define GC(i)
#endif

// ---- SMALL mode helpers (MODE 2) --------------------------------------------------------------------------------
// wave64 maximum of an int32 over the DPP network (row shifts + row broadcasts, like wave_incl_scan); all lanes active.
__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
    const int lo = (int)0x80000000;
    v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x118, 0xf, 0xf, false));  // row_shr:8
    v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = max(v, __builtin_amdgcn_update_dpp(lo, v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return __builtin_amdgcn_readlane(v, 63);
}
template <int L>
__device__ __forceinline__ bool small_ge(const int32_t (&a)[L], const int32_t (&b)[L]) {  // lexicographic a >= b
    bool ge = true;
#pragma unroll
    for (int k = L - 1; k >= 0; --k) ge = a[k] > b[k] || (a[k] == b[k] && ge);
    return ge;
}
template <int L>
__device__ __forceinline__ bool small_ge0(const int32_t (&a)[L]) {  // lexicographic a >= 0
    bool ge = true;
#pragma unroll
    for (int k = L - 1; k >= 0; --k) ge = a[k] > 0 || (a[k] == 0 && ge);
    return ge;
}
__device__ __forceinline__ int32_t clamp_i64_to_i32(int64_t v) {
    return v > 0x7FFFFFFFll ? 0x7FFFFFFF : v < -0x7FFFFFFFll - 1 ? (int32_t)0x80000000 : (int32_t)v;
}

// Trial delta of a ListChange / ListSwap candidate in 32-bit arithmetic: the same at-most-eight matrix legs as
// eval_list_move_legs, laid out as four "plus" and four "minus" legs so no lane multiplies by a sign, gathered from
// the compact u32 matrix through 32-bit byte offsets; every leg finite (host-checked), sums < 2^30.
// dv[k] = change of score level k.  Returns doable.
template <int L, class LT, bool M16 = false, class OT = uint32_t>
__device__ __forceinline__ bool eval_list_move_small(const ListModel& m, const uint16_t* visits, const OT* off, const LT* load,
                                                     bool chg, uint32_t a, uint32_t i, uint32_t b, uint32_t j, int32_t (&dv)[L]) {
    // Branch-free on purpose: every neighbour is read from a position that always exists (the source position when the real one does
    // not) and replaced by the depot with a select afterwards, the doability tests are one predicate at the end.  Conditional LDS reads
    // cost an exec-mask save / restore pair on the scalar unit each, and the scalar unit -- shared by the 20 waves of a CU -- is the
    // busiest pipe of this kernel.
    const uint32_t oa = off[a], la = off[a + 1] - oa;
    const uint32_t ob = off[b], lb = off[b + 1] - ob;
    const bool intra = a == b;
    // move/list_kernel/change.rs:44-71, swap.rs:30-56
    bool ok = i < la && (chg ? j <= lb : j < lb) && !(intra && (j == i || (chg && j == i + 1)));
    const bool flip = !chg && intra && i > j;
    // A lane whose candidate is not doable prices the empty pattern: positions and lengths 0, so every neighbour predicate is false,
    // every LDS read goes to its list's first slot and every matrix row is the depot's -- nothing is gathered through a value that was
    // not validated (the selects are vector ops; the scalar unit sees none of this).
    const uint32_t i2 = ok ? (flip ? j : i) : 0u, j2 = ok ? (flip ? i : j) : 0u;
    const uint32_t la_ = ok ? la : 0u, lb_ = ok ? lb : 0u;
    const uint32_t depot = (uint32_t)m.depot;
    const uint32_t P = oa + i2, Q = ob + j2;
    const bool has_pa = i2 > 0, has_na = i2 + 1 < la_, has_q = j2 < lb_, has_pb = j2 > 0, has_nb = j2 + 1 < lb_;
    const uint32_t r_x = visits[P];
    const uint32_t x = ok ? r_x : depot;
    const uint32_t r_pa = visits[has_pa ? P - 1 : P], r_na = visits[has_na ? P + 1 : P];
    const uint32_t r_q = visits[has_q ? Q : P], r_pb = visits[has_pb ? Q - 1 : P], r_nb = visits[has_nb ? Q + 1 : P];
    const uint32_t pa = has_pa ? r_pa : depot, na = has_na ? r_na : depot;
    const uint32_t vq = has_q ? r_q : depot;  // change: right neighbour of the slot; swap: y
    const uint32_t pb = has_pb ? r_pb : depot, nb = has_nb ? r_nb : depot;
    ok = ok && (chg || x != vq);
    const bool adj = !chg && intra && j2 == i2 + 1;
    const bool ca = chg || adj;
    const bool src_single = la == 1, dst_empty = !intra && lb == 0;
    // plus legs P0..P3, minus legs M0..M3 (change | swap | adjacent swap):
    //   P0 (pa,na)* | (pa,y) | (pa,y)      M0 (pa,x)  | (pa,x) | (pa,x)
    //   P1 (pb,x)   | (y,na) | (y,x)       M1 (x,na)  | (x,na) | (x,y)
    //   P2 (x,vq)   | (pb,x) | (x,nb)      M2 (pb,vq)*| (pb,y) | (y,nb)
    //   P3   -      | (x,nb) |   -         M3   -     | (y,nb) |   -          (* absent for a single-element source /
    //                                                                            an empty destination route)
    const uint32_t dim4 = (uint32_t)SF_SPEC_DIM(m.dim) * (M16 ? 2u : 4u);
    auto leg = [&](uint32_t f, uint32_t t) -> uint32_t {
        const uint32_t byte_off = f * dim4 + t * (M16 ? 2u : 4u);  // dim <= 16384: < 2^30
        if (M16) return *(const uint16_t*)((const char*)m.mat16 + byte_off);  // every leg finite (MODE 2) and < 65535
        return *(const uint32_t*)((const char*)m.mat32 + byte_off);
    };
    const uint32_t p0 = leg(pa, chg ? na : vq);
    const uint32_t p1 = leg(chg ? pb : vq, ca ? x : na);
    const uint32_t p2 = leg(ca ? x : pb, chg ? vq : (adj ? nb : x));
    const uint32_t p3 = leg(x, nb);
    const uint32_t m0 = leg(pa, x);
    const uint32_t m1 = leg(x, adj ? vq : na);
    const uint32_t m3 = leg(vq, nb);
    const uint32_t m2 = leg(adj ? vq : pb, adj ? nb : vq);
    int32_t d_cap = 0;
    if (m.cap_level >= 0) {
        const int32_t dx = m.demand[x];
        const int32_t dyq = m.demand[vq];  // read for every lane, used by the swaps
        const int32_t dy = chg ? 0 : dyq;
        const int32_t cap = (int32_t)m.capacity;
        const int32_t la0 = (int32_t)load[a], lb0 = (int32_t)load[b];
        const int32_t la1 = la0 - dx + dy, lb1 = lb0 - dy + dx;
        d_cap = max(la1 - cap, 0) + max(lb1 - cap, 0) - max(la0 - cap, 0) - max(lb0 - cap, 0);
        d_cap = intra ? 0 : d_cap;
    }
    const uint32_t plus = ((chg && src_single) ? 0u : p0) + p1 + p2 + (ca ? 0u : p3);
    const uint32_t minus = m0 + m1 + ((chg && dst_empty) ? 0u : m2) + (ca ? 0u : m3);
    const int32_t d_dist = (int32_t)(plus - minus);
    const int32_t cw = (int32_t)m.cap_weight, dw = (int32_t)m.dist_weight;
#pragma unroll
    for (int k = 0; k < L; ++k) {  // penalties: score level -= weight * delta(penalty sum)
        int32_t v = 0;
        if (k == m.cap_level) v -= cw * d_cap;
        if (k == m.dist_level) v -= dw * d_dist;
        dv[k] = ok ? v : 0;
    }
    return ok;
}

// The same trial delta for a candidate the nearby generators of THIS step emitted (the FAST kernels' rings hold nothing else): such a candidate
// is structurally doable by construction -- nearby_change.rs:133-195 / nearby_swap.rs enumerate destinations of the committed lists only, skip the
// source slot and its successor, and pair an intra swap with a LATER position -- so move/list_kernel/change.rs:44-71 / swap.rs:30-56 hold and
// nothing is tested here.  Written for the scalar unit's sake (the kernel's bound): a per-lane predicate is a v_cmp into an SGPR pair, every
// `&&` / `||` of two predicates one scalar instruction, every compare-then-select a wait state on gfx950; so neighbours are addressed with
// min() arithmetic, and `chg` arrives as an integer (1 = ListChange, 0 = ListSwap).
// LevelWords: which score level each constraint feeds, as all-ones / zero words made once per launch (level_words).  The empty asm keeps
// them words: left to itself the compiler turns `k == m.cap_level ? ~0 : 0` back into a compare, i.e. a 64-bit lane mask per (level,
// constraint) -- eight spill lanes read back in every replay batch, and a select with a wait state each.
template <int L>
struct LevelWords {
    uint32_t wc[L], wd[L];  // capacity / distance share of level k
    uint32_t has_cap;       // the capacity constraint exists (m.cap_level >= 0)
    // The replay batch's other launch constants, one word each: taken from the argument struct where they are used, `capacity` and the two
    // weights came back from spill lanes as the whole four-register groups their scalar loads had filled -- eight lane reads per batch for three
    // words -- and the depot as a scalar load from the argument block, in every batch (RBATCH kernels).
    int32_t cap, cw, dw;
    uint32_t depot;
};
template <int L, bool USED, bool KW>  // (USED = false: a kernel that never prices with eval_generated_small -- nothing is pinned; KW: the constants as words too)
__device__ __forceinline__ LevelWords<L> level_words(const ListModel& m) {
    LevelWords<L> w;
    w.cap = w.cw = w.dw = 0;
    w.depot = 0;
#ifdef SF_SPEC_MODEL_WORDS  // the run-time unit, candidate "model words" (DESIGN 22): the literals themselves, nothing pinned in a register
    w.cap = SF_SPEC_CAPACITY, w.cw = SF_SPEC_CAP_WEIGHT, w.dw = SF_SPEC_DIST_WEIGHT, w.depot = SF_SPEC_DEPOT;
#pragma unroll
    for (int k = 0; k < L; ++k) w.wc[k] = k == SF_SPEC_CAP_LEVEL ? 0xFFFFFFFFu : 0u, w.wd[k] = k == SF_SPEC_DIST_LEVEL ? 0xFFFFFFFFu : 0u;
    w.has_cap = SF_SPEC_CAP_LEVEL >= 0 ? 1u : 0u;
    return w;
#endif
    if constexpr (KW) {
        // (through a vector register and back: pinned in place, a field stays a part of the register group its scalar load filled, and the group
        // is what gets spilled and read back)
        auto word = [](uint32_t v) -> uint32_t {
            asm volatile("" : "+v"(v));
            return uni(v);
        };
        w.cap = (int32_t)word((uint32_t)m.capacity);
        w.cw = (int32_t)word((uint32_t)m.cap_weight);
        w.dw = (int32_t)word((uint32_t)m.dist_weight);
        w.depot = word((uint32_t)m.depot);
    }
#pragma unroll
    for (int k = 0; k < L; ++k) {
        w.wc[k] = uni(k == m.cap_level ? 0xFFFFFFFFu : 0u);
        w.wd[k] = uni(k == m.dist_level ? 0xFFFFFFFFu : 0u);
        if constexpr (USED) {
            asm volatile("" : "+s"(w.wc[k]));
            asm volatile("" : "+s"(w.wd[k]));
        }
    }
    w.has_cap = uni(m.cap_level >= 0 ? 1u : 0u);
    if constexpr (USED) asm volatile("" : "+s"(w.has_cap));
    return w;
}
template <int L, class LT, bool M16 = false, class OT = uint32_t, bool KW = false>
__device__ __forceinline__ void eval_generated_small(const ListModel& m, const LevelWords<L>& lw, const uint16_t* visits, const OT* off, const LT* load, uint32_t c,
                                                     uint32_t a, uint32_t i, uint32_t b, uint32_t j, int32_t (&dv)[L]) {
    const uint32_t oa = off[a], la = off[a + 1] - oa;
    const uint32_t ob = off[b], lb = off[b + 1] - ob;
    const uint32_t depot = KW ? lw.depot : (uint32_t)m.depot;
    const uint32_t P = oa + i, Q = ob + j;
    // 1 when the neighbour exists (its position is then one step away; otherwise the read goes to the slot itself and the depot is selected)
    const uint32_t h_pa = min(i, 1u), h_na = min(la - 1u - i, 1u);      // i > 0 ; i + 1 < la   (i < la)
    const uint32_t h_q = min(lb - j, 1u), h_pb = min(j, 1u);            // j < lb ; j > 0       (j <= lb)
    const uint32_t h_nb = min(max(lb, j + 1u) - (j + 1u), 1u);          // j + 1 < lb
    const uint32_t x = visits[P];
    const uint32_t r_pa = visits[P - h_pa], r_na = visits[P + h_na];
    const uint32_t r_q = visits[Q - (1u - h_q)], r_pb = visits[Q - h_pb], r_nb = visits[Q + h_nb];  // (an end slot reads its left neighbour; unused)
    const uint32_t pa = h_pa ? r_pa : depot, na = h_na ? r_na : depot;
    const uint32_t vq = h_q ? r_q : depot;  // change: right neighbour of the slot; swap: y
    const uint32_t pb = h_pb ? r_pb : depot, nb = h_nb ? r_nb : depot;
    const bool chg = c != 0;
    const bool intra = a == b;
    const bool adj = !chg && intra && j == i + 1;
    const bool ca = chg || adj;
    const uint32_t dim4 = (uint32_t)SF_SPEC_DIM(m.dim) * (M16 ? 2u : 4u);
    auto leg = [&](uint32_t f, uint32_t t) -> uint32_t {
        const uint32_t byte_off = __umul24(f, dim4) + t * (M16 ? 2u : 4u);  // node ids and the row pitch are below 2^24: one full-rate v_mad_u32_u24 (a 32-bit v_mul_lo is quarter rate); dim <= 16384: < 2^30
        if (M16) return *(const uint16_t*)((const char*)m.mat16 + byte_off);
        return *(const uint32_t*)((const char*)m.mat32 + byte_off);
    };
    // plus legs P0..P3, minus legs M0..M3: the table of eval_list_move_small
    const uint32_t p0 = leg(pa, chg ? na : vq);
#ifdef SF_SPEC_SYM_ROWS  // the run-time unit, mat[a][b] == mat[b][a] for every pair: the two legs with a source-side endpoint, from its row
    const uint32_t p1 = leg(ca ? x : na, chg ? pb : vq);
    const uint32_t p2 = leg(x, chg ? vq : (adj ? nb : pb));
#else
    const uint32_t p1 = leg(chg ? pb : vq, ca ? x : na);
    const uint32_t p2 = leg(ca ? x : pb, chg ? vq : (adj ? nb : x));
#endif
#ifdef SF_SPEC_LEG_REAIM  // the run-time unit: a leg the lane discards is aimed at m1's address, a line the lane fetches anyway
    const uint32_t o_m1 = __umul24(x, dim4) + (adj ? vq : na) * (M16 ? 2u : 4u);
    auto leg_at = [&](uint32_t byte_off) -> uint32_t {
        if (M16) return *(const uint16_t*)((const char*)m.mat16 + byte_off);
        return *(const uint32_t*)((const char*)m.mat32 + byte_off);
    };
    const uint32_t p3 = leg_at(ca ? o_m1 : __umul24(x, dim4) + nb * (M16 ? 2u : 4u));
    const uint32_t m0 = leg(pa, x);
    const uint32_t m1 = leg_at(o_m1);
    const uint32_t m3 = leg_at(ca ? o_m1 : __umul24(vq, dim4) + nb * (M16 ? 2u : 4u));
#else
    const uint32_t p3 = leg(x, nb);
    const uint32_t m0 = leg(pa, x);
    const uint32_t m1 = leg(x, adj ? vq : na);
    const uint32_t m3 = leg(vq, nb);
#endif
    const uint32_t m2 = leg(adj ? vq : pb, adj ? nb : vq);
    int32_t d_cap = 0;
    if (lw.has_cap != 0u) {
        const int32_t dx = m.demand[x];
#ifdef SF_SPEC_LEG_REAIM
        const int32_t dyq = m.demand[(chg || intra) ? x : vq];  // (discarded below in exactly those lanes)
#else
        const int32_t dyq = m.demand[vq];
#endif
        const int32_t dy = chg ? 0 : dyq;
        const int32_t cap = KW ? lw.cap : (int32_t)m.capacity;
        const int32_t la0 = (int32_t)load[a] - cap, lb0 = (int32_t)load[b] - cap;
        const int32_t sh = dx - dy;
        d_cap = max(la0 - sh, 0) + max(lb0 + sh, 0) - max(la0, 0) - max(lb0, 0);
        d_cap = intra ? 0 : d_cap;
    }
    const uint32_t plus = ((chg && la == 1) ? 0u : p0) + p1 + p2 + (ca ? 0u : p3);
    const uint32_t minus = m0 + m1 + ((chg && !intra && lb == 0) ? 0u : m2) + (ca ? 0u : m3);
    const int32_t d_dist = (int32_t)(plus - minus);
    // penalties: score level -= weight * delta(penalty sum); a level's share is picked with a 32-bit all-ones / zero word per (level, constraint) --
    // two wave-uniform words (LevelWords) instead of a lane mask in a scalar register pair and a select each
    const int32_t tc = -((KW ? lw.cw : (int32_t)m.cap_weight) * d_cap), td = -((KW ? lw.dw : (int32_t)m.dist_weight) * d_dist);
#pragma unroll
    for (int k = 0; k < L; ++k) dv[k] = (int32_t)(((uint32_t)tc & lw.wc[k]) + ((uint32_t)td & lw.wd[k]));
}

// Per-leaf cursor state of one step.  The NEXT source of the leaf is always resolved ahead of use
// and the first 64-entry chunk of its neighbour row is already in flight (`pk`), so the global
// load latency hides behind the other leaf's generation and the replay batches.
struct LeafCursor {
    uint32_t head, tail;  // candidate ring (monotonic counters)
    uint32_t left;        // sources not yet generated
    uint32_t k, o;        // next source: entity rank / offset inside the entity's list
    uint32_t se, len, sp, sx;  // next source resolved: entity, its list length, position, element
    uint32_t vk, vbase;        // entity rank / offset base the leaf's spvec holds (0xFFFFFFFF = none)
    int ex;               // exhausted (union scheduler)
    uint32_t pk;          // per lane: prefetched entry of chunk 0 of the next source's neighbour row
    uint32_t pv;          // per lane: (source position | source element << 16) of offset vbase + lane of entity rank vk
    uint32_t cend;        // offsets o < cend of the current entity are served by `pv` as it stands (0 = nothing cached): resolve()'s one-compare fast path
};

// The kernel's argument block as it lies in the kernarg segment (by-value structs in declaration order, each at its own alignment), and a
// view of it that is read AGAIN at the point of use.  A field taken from the by-value arguments is loaded in the kernel's prologue and then
// carried -- in a scalar register or in a spill lane -- to wherever it is used; the fields that are used once per step or once per launch
// (history, counters and write-back pointers, seeds, budgets) are read through cold_args() instead: one scalar load where the value is
// needed, nothing live across the fill and replay loops.  (The empty asm hides the pointer's origin from the optimiser, which would otherwise
// merge the load with the prologue's and carry the value after all.)
// That WaveArgs and the segment have the same layout rests on the AMDGPU kernarg ABI: the explicit arguments start at offset 0 of the segment,
// in declaration order, each at its own ABI alignment -- the rule that lays out the members of a struct.  It holds only while the members of
// WaveArgs ARE the kernel's parameters, type by type and in order: the static_assert below the kernel refuses to compile anything else (a
// parameter added, removed or moved would otherwise turn every write-back pointer into garbage without a word from the compiler).
struct WaveArgs {
    ListModel m;
    SearchParams p;
    NbrIndex nb;
};
typedef const __attribute__((address_space(4))) WaveArgs* ColdArgs;
__device__ __forceinline__ ColdArgs cold_args() {
    uint64_t u = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(u));
    return (ColdArgs)u;
}

// MODE 1 (FAST): compile-time specialisation for the default list policy (nearby change + nearby swap union,
// LateAcceptance + AcceptedCount, committed steps) — fewer live scalars and branches in the hot loops.
// MODE 2 (FAST + SMALL): additionally every quantity of a trial delta fits 32 bits (host-checked: all matrix legs finite
// and < 2^26, demands / capacity / weights bounded so that |level delta| < 2^30): the replay scores, accepts and forages
// in DELTA space — a candidate is the int32 change of each score level against the step's (wave-uniform) current score,
// `score >= late` becomes `delta >= late - current` with the right-hand side clamped once per step — so no lane carries a
// 64-bit score vector; the committed score is advanced by the winner's delta.  Same decisions bit for bit.
#ifndef SF_WAVES_PER_EU
#define SF_WAVES_PER_EU 4
#endif
// COMPACT (with MODE 2 only): the replica's LDS slice in the compact layout of WCarve, chosen by the host when it lets more
// replicas share a CU (CVRP-5000: 5 instead of 3).
// WPE = waves per SIMD the kernel is compiled for (512 / WPE VGPRs): 4, or 5 / 6 for the COMPACT slice of a model small enough for 20 /
// 24 replicas per CU.  Round 4: with the replica index declared wave-uniform the per-replica base pointers live in scalar registers and
// the MODE 2 kernels need 77 VGPRs and no scratch (they were 96 VGPRs + 120 B: 64-bit pointer pairs spilled in the prologue).
// NODEG (with COMPACT only): the node -> slot table in HBM (ListModel::node_tab) instead of the slice.  A wave's speed does not depend on
// the model size (CVRP-1000 and CVRP-5000 both run 7.4 M moves/s per resident wave: the wave's own chain of dependent accesses is the
// bound), the throughput is the number of resident waves -- and at CVRP-5000 the 29 KB slice holds that at 5 per CU.
template <int L, bool TRACE, int MODE, bool COMPACT = false, int WPE = SF_WAVES_PER_EU, bool NODEG = false>
__global__ __launch_bounds__(64 * WPB, WPE) void k_list_search_wave(ListModel m, SearchParams p, NbrIndex nb) {
    constexpr bool FAST = MODE >= 1, SMALL = MODE == 2;
    // LEAN: the FAST + SMALL kernels -- the ones whose bound is the scalar unit -- have the paired pass of DESIGN 17: row entries and the node-table
    // read in flight across resolve(), half selects as words, a branch-free item, closed groups in lanes; SAT (their COMPACT layouts): the table's
    // saturation scan behind a count; RANKTAB (the COMPACT layouts that keep a route table): the table holds the rank alone.  The general kernels
    // compile the pass they had.  (How each of the five was built and measured on its own: profiles/wave_pair_levers.txt.)
    constexpr bool LEAN = FAST && SMALL;
    constexpr bool SAT = LEAN && COMPACT, RANKTAB = LEAN && COMPACT && !NODEG;
    // RBATCH: the lean replay batch of DESIGN 18 (the AcceptedCount cut and the quit test behind one compare on the batch's accepted count,
    // candidates_scored once per step, the batch's launch constants as pinned words) -- the LEAN kernels that keep the node table in LDS.  The NODEG
    // kernel (launch mode 6) compiles the batch it had: with the same source form its CVRP-5000 leg measured 2.0 % SLOWER than its parent.
    constexpr bool RBATCH = LEAN && !NODEG;
// A cold field of `p` / `m`: the FAST + SMALL kernels -- the ones whose bound is the scalar unit -- read it from the argument block where it
// is used, the others from the by-value structs.  (Local to this kernel: the macros name its `SMALL`, `p` and `m`, and end with it.)
#define SF_COLD_P(f) (SMALL ? cold_args()->p.f : p.f)
#define SF_COLD_M(f) (SMALL ? cold_args()->m.f : m.f)
    static_assert(!COMPACT || SMALL, "COMPACT stores loads in 32 bits: MODE 2 only");
    static_assert(!NODEG || COMPACT, "NODEG: the 16-bit table of the COMPACT layout");
    using LT = typename std::conditional<COMPACT, int32_t, int64_t>::type;
    using OT = typename std::conditional<NODEG, uint16_t, uint32_t>::type;  // list offsets in the slice (NODEG: 16 bits, n_cap <= 65535 in this engine)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t lane = threadIdx.x & 63u;
    // wave-uniform by construction; saying so keeps every per-replica base pointer in scalar registers (they were 64-bit VGPR pairs
    // spilled to scratch in the prologue and reloaded for the write-back)
    const uint32_t wave_in_group = uni(threadIdx.x >> 6);
    const int rr = (int)(blockIdx.x * (blockDim.x >> 6) + wave_in_group);  // 1..WPB replicas per workgroup
    if (rr >= p.n_launch) return;  // no workgroup barrier anywhere below
    const int r = rr + p.replica_base;
    const int V = SF_SPEC_V(m.V);
    const uint32_t dim = (uint32_t)SF_SPEC_DIM(m.dim);

    // leaf constants (no dynamic indexing of the kernarg block)
    const int n_leaves = FAST ? 2 : p.n_leaves;
    const uint32_t K0 = (uint32_t)SF_SPEC_K0(p.leaf[0].max_nearby), K1 = n_leaves > 1 ? (uint32_t)SF_SPEC_K1(p.leaf[1].max_nearby) : 1u;
    const bool chg0 = FAST ? true : p.leaf[0].kind == 16, chg1 = FAST ? false : (n_leaves > 1 && p.leaf[1].kind == 16);
    const int acceptor = FAST ? 1 : p.acceptor, forager = FAST ? 0 : p.forager;
    const bool dry_run = FAST ? false : p.dry_run != 0;
    __shared__ uint64_t s_sa[FAST ? 1 : WPB][FAST ? 1 : SA_WORDS];  // SimulatedAnnealing acceptor state of the resident replicas (FAST: LateAcceptance only, no static LDS -- the host's occupancy plan counts on that)
    uint64_t* saw = s_sa[FAST ? 0 : wave_in_group];
    const bool annealing = !FAST && acceptor == 3;
    if constexpr (!FAST)
        if (annealing) sa_load(saw, p.sa, r, lane);
    // the leaves' descriptor indices as the salts take them (sign-extended to 64 bits).  SMALL carries them as the 32-bit words they are and
    // widens where a salt is formed; the general kernels keep the widened pair (their register allocation is left as it was)
    const int32_t desc0_w = p.leaf[0].descriptor, desc1_w = n_leaves > 1 ? p.leaf[1].descriptor : 0;
    const uint64_t desc0_q = SMALL ? 0 : (uint64_t)p.leaf[0].descriptor, desc1_q = (!SMALL && n_leaves > 1) ? (uint64_t)p.leaf[1].descriptor : 0;
    auto desc0 = [&]() -> uint64_t { return SMALL ? (uint64_t)(int64_t)desc0_w : desc0_q; };
    auto desc1 = [&]() -> uint64_t { return SMALL ? (uint64_t)(int64_t)desc1_w : desc1_q; };

    const WCarve cv(V, SF_SPEC_NCAP(m.n_cap), (int)dim, (int)(K0 > K1 ? K0 : K1), COMPACT, NODEG);
    const uint32_t RCM = cv.rc - 1;
    unsigned char* mem = smem + (size_t)wave_in_group * cv.total;
    LT* s_load = (LT*)(mem + cv.load);
    OT* s_off = (OT*)(mem + cv.off);
    uint32_t* ring = (uint32_t*)(mem + cv.ring);  // [leaf][rc][2]
    uint16_t* s_visits = (uint16_t*)(mem + cv.visits);
    const NodeSlotT<COMPACT> node_slot(NODEG ? (unsigned char*)(m.node_tab + (size_t)r * dim) : mem + cv.node, V, s_visits, (const void*)s_off, NODEG);
    // table writes -> table reads of other lanes: LDS in program order (wave_sync); HBM through the CU's write-through L1 (ring_sync's fences)
    auto node_sync = [&]() {
        if constexpr (NODEG) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        } else {
            wave_sync();
        }
    };
    // [leaf][route] rank | first slot ordinal << 16 (RouteTab).  The NODEG layout computes the rank instead (RouteArith) and carries no table: in
    // round 5 its table lived in HBM, a dependent global gather per row entry behind the node -> slot one -- CVRP-5000 15.9 -> 17.9 G moves/s and
    // 322 -> 227 B of memory-side traffic per candidate without it.  With the table in LDS (CVRP-1000) the lookup is cheaper than the arithmetic
    // (50.4 -> 48.8 G when every COMPACT kernel computed ranks, profiles/r06d_route_arith_ab.txt), so those keep it.
    constexpr bool ARANK = NODEG;
    // RANKTAB: the table holds the rank alone and the inter-list ordinal is (rank << 16 | position), as in
    // RouteArith -- it is only ever compared inside one equal-distance group -- so the prologue needs no prefix scan over the lists
    using RT = typename std::conditional<ARANK, RouteArith, typename std::conditional<RANKTAB, RouteRank, RouteTab>::type>::type;
    uint32_t* rtab = (uint32_t*)(mem + cv.rtab);
    uint16_t* route_at = (uint16_t*)(mem + cv.routeat);  // [leaf][rank] -> route

    // (SMALL uses the replica's base pointers for the load below only and forms them again at the write-back, from the argument block:
    // nothing of them is carried through the step loop)
    uint32_t* g_visits = m.visits + (size_t)r * SF_SPEC_NCAP(m.n_cap);
    uint32_t* g_off = m.off + (size_t)r * (V + 1);
    int64_t* g_load = m.load + (size_t)r * V;
    int64_t* g_score = m.score + (size_t)r * 4;
    const bool tracing = TRACE && r == p.trace_replica;

    // ---- load replica state into LDS ----
    for (uint32_t t = lane; t <= (uint32_t)V; t += 64) s_off[t] = (OT)g_off[t];
    for (uint32_t t = lane; t < (uint32_t)V; t += 64) s_load[t] = (LT)g_load[t];
    for (uint32_t t = lane; t < dim; t += 64) node_slot.clear(t);
    node_sync();
    const uint32_t total0 = uni(s_off[V]);
    if (COMPACT && SF_SPEC_HAS_PERM(m.perm != nullptr)) {  // internal node numbering (ListModel::perm): the lists are renamed on the way in and on every way out
        for (uint32_t t = lane; t < total0; t += 64) s_visits[t] = m.perm[g_visits[t]];
    } else {
        for (uint32_t t = lane; t < total0; t += 64) s_visits[t] = (uint16_t)g_visits[t];
    }
    wave_sync();
    for (uint32_t v = lane; v < (uint32_t)V; v += 64) {
        const uint32_t o = s_off[v], len = s_off[v + 1] - o;
        for (uint32_t q = 0; q < len; ++q) node_slot.set(s_visits[o + q], v, q);
    }
    node_sync();

    // SAT: the number of routes longer than pmax, i.e. with positions stored saturated in the 16-bit table (wave-uniform; kept at the commit).
    // While it is zero the paired pass decodes the table word with wide_short(): no ballot, no region, nothing waits for the read on the spot.
    uint32_t nsat = 0;
    if constexpr (SAT) {
        for (uint32_t base = 0; base < (uint32_t)V; base += 64) {
            const uint32_t v = base + lane;
            const bool lg = v < (uint32_t)V && (uint32_t)(s_off[v + 1] - s_off[v]) > node_slot.pmax;
            nsat += (uint32_t)__popcll(__ballot(lg));
        }
    }
    auto ext_id = [&](uint32_t x) -> uint32_t { return (COMPACT && SF_SPEC_HAS_PERM(m.inv != nullptr)) ? (uint32_t)m.inv[x] : x; };  // an LDS element under the caller's numbering
    int64_t cur[L], best_sol[L];
#pragma unroll
    for (int k = 0; k < L; ++k) {
        cur[k] = (int64_t)uni64((uint64_t)g_score[k]);  // wave-uniform: keep in scalar registers
        best_sol[k] = (int64_t)uni64((uint64_t)m.best_score[(size_t)r * 4 + k]);
    }
    // per-launch counters in 32 bits (wave-uniform: scalar registers), folded into the replica's 64-bit sf_stats words
    // before they can wrap (flush_stats): a long fixed-step launch never loses counts
    uint32_t st_steps = 0, st_gen = 0, st_acc = 0, st_applied = 0, st_calc = 0, st_scored = 0, st_sources = 0;
    uint64_t steps_run = 0;  // (general kernels; SMALL reads the number of steps off the loop counter instead)
    auto flush_stats = [&]() {
        if (lane == 0) {
            uint64_t* gs = SF_COLD_P(stats) + (size_t)r * SF_STATS_WORDS;
            gs[0] += st_steps;
            gs[1] += st_gen;
            gs[2] += st_gen;
            gs[3] += st_acc;
            gs[4] += st_applied;
            gs[5] += st_calc;
            gs[6] += st_gen - st_calc;
            gs[7] += st_scored;
            gs[8] += st_sources;
        }
        if constexpr (!SMALL) steps_run += st_steps;
        st_steps = st_gen = st_acc = st_applied = st_calc = st_scored = st_sources = 0;
    };
    uint64_t trace_n = 0;
    const uint64_t step_index0 = dry_run ? 0 : p.step_index[r];
    const uint64_t seed_draws0 = dry_run ? 0 : p.seed_draws[r];
    const int la_idx0 = dry_run ? 0 : p.la_idx[r];
    int la_cursor = la_idx0;  // (la_idx0 + step) % la_size, kept incrementally (no 64-bit division per step)
    const uint64_t lanebit = 1ULL << lane;
    // LEAN kernels: the paired pass picks a half's facts with a per-lane WORD, not with the 64-bit mask `lane >= 32`: `hm` is all-ones in lanes
    // 32-63 and zero in lanes 0-31, and half(a, b) = a in the lower half, b in the upper one, is a v_and and a v_and_or.  The mask lived in spill
    // lanes and was read back five times per pass; a word select needs no scalar register at all.  (The empty asm keeps it a word: left to itself
    // the compiler turns it back into the compare.)
    uint32_t hm = 0;  // (LEAN kernels only)
    if constexpr (LEAN) {
        hm = (uint32_t)((int32_t)(lane << 26) >> 31);
        asm volatile("" : "+v"(hm));
    }
    auto half = [&](uint32_t lo, uint32_t up) -> uint32_t { return (lo & ~hm) | (up & hm); };
    PH_DECL

    const LevelWords<L> lvl = level_words<L, SMALL, RBATCH>(m);
    bool best_pending = false;  // working == best, snapshot not yet written (see sf_scalar_kernels.hip: deferred clone)
    const FastMod fm_V = make_fastmod(V > 0 ? (uint32_t)V : 1u);
    const FastMod fm_V1 = make_fastmod(V > 1 ? (uint32_t)V - 1u : 1u);
    const uint32_t v_recip32 = V > 1 ? (uint32_t)(0x100000000ull / (uint32_t)V) : 0u;  // floor(2^32 / V): resolve()'s 32-bit remainder (V = 1: every rank maps to list 0)
    // coprimality of every candidate permutation stride of the V list owners, once per launch (lane s tests s and s + 64)
    const bool use_cm = V >= 2 && V <= 128;
    const uint64_t cm_lo = use_cm ? __ballot(lane >= 1 && lane < (uint32_t)V && gcd_u32(lane, (uint32_t)V) == 1) : 0ull;
    const uint64_t cm_hi = use_cm ? __ballot(lane + 64 < (uint32_t)V && gcd_u32(lane + 64, (uint32_t)V) == 1) : 0ull;
    int64_t step = 0;  // SMALL, after the loop: the number of steps that ran (a move budget ends the launch early)
    for (; step < SF_COLD_P(n_steps); ++step) {
        PH(7)
        ISA_MARK("prologue_begin");
        // ---- (A) step start (step.rs:60-74) -------------------------------------------------
        uint64_t sidx, sseed;
        if (dry_run) {
            sidx = p.dry_step_index;
            sseed = p.dry_step_seed;
        } else {
            sidx = step_index0 + (uint64_t)step;
            const uint64_t draw = seed_draws0 + (uint64_t)step;
            const uint64_t* const explicit_seeds = SF_COLD_P(explicit_seeds);
            const int64_t n_explicit = SF_COLD_P(n_explicit);
            if (SF_SPEC_HAS_EXPLICIT(explicit_seeds != nullptr) && (int64_t)draw < n_explicit)
                sseed = explicit_seeds[(size_t)r * n_explicit + draw];
            else
                sseed = step_seed(SF_COLD_P(random_seed) + (uint64_t)r, draw);
        }
        sidx = uni64(sidx);
        sseed = uni64(sseed);
        const StreamCtx ctx{sidx, sseed, FAST ? 3 : p.order};  // FAST: SelectionOrder::Random, the default policy's (host-checked)
        ScoreV<L> late;
#pragma unroll
        for (int k = 0; k < L; ++k) late.v[k] = 0;
        const int la_slot = la_cursor;  // LateAcceptance history slot of this step
        if (acceptor == 1 || acceptor == 4) {
            const int64_t* const lh = SF_COLD_P(la_hist) + ((size_t)r * SF_SPEC_LA_SIZE(SF_COLD_P(la_size)) + la_slot) * 4;
#pragma unroll
            for (int k = 0; k < L; ++k) late.v[k] = (int64_t)uni64((uint64_t)lh[k]);
        }
        ScoreV<L> dla_thr = late;  // DiversifiedLateAcceptance: best step score of the phase minus its tolerance band
        if (acceptor == 4) {
            ScoreV<L> db;
#pragma unroll
            for (int k = 0; k < L; ++k) db.v[k] = (int64_t)uni64((uint64_t)p.dla_best[(size_t)r * 4 + k]);
            dla_thr = dla_threshold<L>(db, p.dla_tolerance);
        }
        [[maybe_unused]] bool thr_on = true;  // GreatDeluge / StepCountingHillClimbing (the TRACE instantiations carry them): their threshold of the step in `late` (sf_step.h)
        if constexpr (TRACE)
            if (acceptor == 5 || acceptor == 6) ax_step_begin<L>(acceptor, p.sa.state + (size_t)r * SA_WORDS, late, thr_on);
        // TabuSearch (the TRACE instantiations carry it too): the memories and the acceptor's best as they stand at step begin -- nothing changes
        // them before tabu_step_ended (sf_tabu.h).  One scope: the list variable; entities are routes, values element ids.
        [[maybe_unused]] TabuStep<L> tabu;
        [[maybe_unused]] const TabuScope tabu_scope{0u, 0u, 0u};
        if constexpr (TRACE)
            if (acceptor == 7) tabu_step_begin<L>(p.sa.state + (size_t)r * SA_WORDS, tabu);
        int has_best = 0;
        typename std::conditional<SMALL, uint32_t, uint64_t>::type equal_count = 0;  // (SMALL: 32 bits -- a step consumes far fewer than 2^32 candidates; reservoir_pick hashes it as 64 bits)
        uint32_t accepted = 0, pulls = 0;
        ScoreV<L> best;
#pragma unroll
        for (int k = 0; k < L; ++k) best.v[k] = 0;
        uint32_t best_m0 = 0, best_m1 = 0;
        int best_leaf = 0;
        uint64_t best_ti = 0;  // trace ordinal (within the step) of the forager's current pick
        // MODE 2: the LateAcceptance threshold and the forager's best as level deltas against `cur` (wave-uniform);
        // |candidate delta| < 2^30, so clamping the threshold to int32 keeps every comparison exact
        int32_t late_d[L], best_d[L];
#pragma unroll
        for (int k = 0; k < L; ++k) {
            late_d[k] = SMALL ? clamp_i64_to_i32(wsub(late.v[k], cur[k])) : 0;
            best_d[k] = 0;
        }
        // (L == 2) the same thresholds as one signed 64-bit key each: hard x 2^32 + soft
        int64_t acc_thr = 0, best_key = 0;
        if constexpr (SMALL && L == 2) {
            // (|candidate level delta| < 2^30: a hard threshold at or below -2^30 accepts every candidate whatever it is, so the clamp is exact and the
            // key cannot leave 64 bits)
            const int64_t lh = late_d[0] < -(1 << 30) ? -(int64_t)(1 << 30) : (int64_t)late_d[0];
            const int64_t late_key = lh * 4294967296ll + (int64_t)late_d[1];
            acc_thr = late_key < 0 ? late_key : 0;  // delta >= 0  ||  delta >= late - current
        }
        const uint32_t total = uni(s_off[V]);
        // union: >1 leaf => StratifiedRandom, equal weights (vec_union.rs:229-245); with two children
        // the stride is always 1, so the order is first, other, first, ...
        // The five hashes a FAST step starts with (the union's first child; start and stride of the two leaves' entity permutations) are
        // computed SIDE BY SIDE, one per lane, on the vector unit: as wave-uniform values they were ~400 scalar instructions per step (64-bit
        // multiplies and Barrett remainders expand to a dozen s_mul each), a tenth of the kernel's scalar work, and the scalar unit -- shared by
        // the 24 waves of a CU -- is its bound (profiles/r05_salu_fit.json: 1,042 scalar instructions per step before this).
        uint32_t hashed = 0;  // lane l < 5: remainder of mixed_seed(salt_l) by its divisor
        const bool lane_hash = FAST && use_cm;
        if (lane_hash) {
            const uint64_t es0 = SALT_NEARBY_CHANGE_ENTITY ^ desc0(), es1 = SALT_NEARBY_SWAP_ENTITY ^ desc1();  // FAST: leaf 0 = nearby change, leaf 1 = nearby swap
            if constexpr (RBATCH && SF_WAVE_SYM != 0) {
                // The kernels with the lockstep round form the lane index again HERE: taken from `lane`, each lane's salt and divisor are computed
                // before the step loop and carried through it in five vector registers, which those kernels do not have (the WPE 6 one went through
                // scratch memory for them) -- a dozen selects per step instead.  The other kernels keep their statements, and so their code.
                uint32_t hl = lane;
                asm volatile("" : "+v"(hl));
                const uint64_t salt = hl == 0 ? SALT_UNION_OFFSET : hl == 1 ? es0 : hl == 2 ? (es0 ^ STRIDE_SALT_MIX) : hl == 3 ? es1 : (es1 ^ STRIDE_SALT_MIX);
                const FastMod fm2 = make_fastmod(2u);
                FastMod f;
                f.M = hl == 0 ? fm2.M : ((hl & 1u) ? fm_V.M : fm_V1.M);
                f.n = hl == 0 ? fm2.n : ((hl & 1u) ? fm_V.n : fm_V1.n);
                hashed = fastmod_u64(ctx.mixed_seed(salt), f);
            } else {
                const uint64_t salt = lane == 0 ? SALT_UNION_OFFSET : lane == 1 ? es0 : lane == 2 ? (es0 ^ STRIDE_SALT_MIX) : lane == 3 ? es1 : (es1 ^ STRIDE_SALT_MIX);
                const FastMod fm2 = make_fastmod(2u);
                FastMod f;
                f.M = lane == 0 ? fm2.M : ((lane & 1u) ? fm_V.M : fm_V1.M);
                f.n = lane == 0 ? fm2.n : ((lane & 1u) ? fm_V.n : fm_V1.n);
                hashed = fastmod_u64(ctx.mixed_seed(salt), f);
            }
        }
        const uint32_t first_leaf = lane_hash ? (uint32_t)__builtin_amdgcn_readlane((int)hashed, 0)
                                              : (n_leaves > 1 ? ctx.random_index((uint32_t)n_leaves, SALT_UNION_OFFSET) : 0u);

        uint32_t perm_st0 = 0, perm_sd0 = 1, perm_st1 = 0, perm_sd1 = 1;  // entity permutations of the two leaves (set in (B))
        uint32_t perm_inv0 = 0, perm_inv1 = 0;                              // ARANK: stride^-1 mod V of each
        auto route_facts = [&](int l) -> RT {
            if constexpr (ARANK)
                return RouteArith{l ? perm_st1 : perm_st0, l ? perm_inv1 : perm_inv0, (uint32_t)V, v_recip32};
            else
                return RT{rtab + l * V};
        };
        // resolve the source at cursor (k, o) of leaf l and put its first key chunk in flight
        auto resolve = [&](LeafCursor& c, int l) {
            const uint16_t* ra = route_at + l * V;
            uint32_t k = c.k, o = c.o, se = c.se, len = c.len;
            // the common case -- the next offset of the same entity inside the 64 offsets `pv` already holds -- is ONE compare: everything below
            // this test is the per-entity / per-chunk path (it used to be entered through two compound tests, ~20 scalar instructions per source)
            if (o >= c.cend) {
            ISA_MARK("resolve_slow_begin");
            if (k != c.vk || o >= len) {  // a new entity: its list owner and length (skip empty routes; left > 0
                                          // guarantees a source exists)
                for (;;) {
                    if constexpr (COMPACT) {  // no rank -> route table in the compact slice: the permutation itself (a few entities per step)
                        // start + k x stride < V^2 + V < 2^21 (V <= 1022 in this layout): a 32-bit Barrett step -- the quotient estimate is exact or one
                        // short -- instead of the 64 x 64 high multiply of fastmod_u64 (two dozen scalar instructions)
                        const uint32_t xx = (l ? perm_st1 : perm_st0) + k * (l ? perm_sd1 : perm_sd0);
                        uint32_t rr_ = xx - __umulhi(xx, v_recip32) * (uint32_t)V;
                        rr_ = rr_ >= (uint32_t)V ? rr_ - (uint32_t)V : rr_;
                        se = uni(rr_);
                    } else
                        se = uni((uint32_t)ra[k]);
                    len = uni(s_off[se + 1] - s_off[se]);
                    if (o < len) break;
                    ++k;
                    o = 0;
                }
            }
            if (k != c.vk || (o & ~63u) != c.vbase) {
                // 64 consecutive offsets of this entity, one per lane: source position and source element, kept in a
                // register (`pv` = position | element << 16); a source is then one v_readlane away, no LDS round trip
                const uint64_t src_salt = ((l ? chg1 : chg0) ? SALT_NEARBY_CHANGE_SOURCE : SALT_NEARBY_SWAP_SOURCE) ^
                                          (uint64_t)se ^ (l ? desc1() : desc0());
                const uint32_t oo = (o & ~63u) + lane;
                const uint32_t spl = oo < len ? ctx.selection_index(oo, len, src_salt) : 0u;
                const uint32_t sxl = oo < len ? (uint32_t)s_visits[s_off[se] + spl] : 0u;
                c.pv = spl | (sxl << 16);
                c.vk = k;
                c.vbase = o & ~63u;
            }
            c.cend = len < (o & ~63u) + 64u ? len : (o & ~63u) + 64u;
            c.k = k;
            c.se = se;
            c.len = len;
            ISA_MARK("resolve_slow_end");
            }
            const uint32_t pvv = (uint32_t)__builtin_amdgcn_readlane((int)c.pv, (int)(o & 63u));
            const uint32_t sp = pvv & 0xFFFFu, sx = pvv >> 16;
            c.o = o;
            c.sp = sp;
            c.sx = sx;
            const uint32_t ent = l ? ((lane + 32u) & 63u) : lane;  // leaf 1: lanes 32-63 hold entries 0-31
            // (the index has dim^2 <= 2^28 entries: a 32-bit byte offset per lane on the scalar base pointer, not a 64-bit scalar row address)
            // unconditional load (a lane past a row shorter than 64 entries reads the row's last entry and is then blanked): no exec-mask region
            const uint32_t entc = ent < dim ? ent : dim - 1u;
            const uint32_t pk_any = (uint32_t) * (const uint16_t*)((const char*)nb.keys + ((sx * dim + entc) << 1));
            // LEAN: the entry stays raw -- blanking it here consumes the load on the spot (a full wait for the row right behind its issue);
            // whoever takes the key blanks the lanes past the row (row_key), one pass later, and the load is in flight until then
            if constexpr (LEAN)
                c.pk = pk_any;
            else
                c.pk = ent < dim ? pk_any : NBR_END;
        };
        // the key of row entry `e` out of a raw prefetched entry
        auto row_key = [&](uint32_t raw, uint32_t e) -> uint32_t { return LEAN ? (e < dim ? raw : NBR_END) : raw; };

        PH(0)
        // ---- (B) per-leaf entity order tables (slot.rs:468-499) --------------------------------
        LeafCursor C0{0, 0, total, 0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0, 0, NBR_END, 0, 0};
        LeafCursor C1{0, 0, n_leaves > 1 ? total : 0u, 0, 0, 0, 0, 0, 0, 0xFFFFFFFFu, 0, n_leaves > 1 ? 0 : 1, NBR_END, 0, 0};
        for (int l = 0; l < n_leaves; ++l) {
            const uint64_t ent_salt = ((l ? chg1 : chg0) ? SALT_NEARBY_CHANGE_ENTITY : SALT_NEARBY_SWAP_ENTITY) ^ (l ? desc1() : desc0());
            uint32_t pst, psd;
            if (lane_hash) {  // perm_params_fm with the two hashes already taken (above)
                pst = (uint32_t)__builtin_amdgcn_readlane((int)hashed, l ? 3 : 1);
                psd = StreamCtx::first_coprime_from((uint32_t)__builtin_amdgcn_readlane((int)hashed, l ? 4 : 2) + 1u, cm_lo, cm_hi);
            } else if (use_cm)
                ctx.perm_params_fm(fm_V, fm_V1, ent_salt, pst, psd, cm_lo, cm_hi);
            else
                ctx.perm_params((uint32_t)V, ent_salt, pst, psd);
            pst = uni(pst);
            psd = uni(psd);
            if (l)
                perm_st1 = pst, perm_sd1 = psd;
            else
                perm_st0 = pst, perm_sd0 = psd;
            if constexpr (ARANK) {
                // stride^-1 mod V (the stride is coprime to V): lane c tests c, c + 64, ... -- one or two rounds at 100 lists, eight at 500
                uint32_t inv = 0;
                for (uint32_t base = 0; base < (uint32_t)V; base += 64) {
                    const uint32_t c = base + lane;
                    const uint32_t xx = psd * c;  // < V^2 + 64 V < 2^21
                    uint32_t rm = xx - __umulhi(xx, v_recip32) * (uint32_t)V;
                    rm = rm >= (uint32_t)V ? rm - (uint32_t)V : rm;
                    const uint64_t hit = __ballot(c < (uint32_t)V && rm == 1u);
                    if (hit) {
                        inv = base + (uint32_t)__ffsll((unsigned long long)hit) - 1u;
                        break;
                    }
                }
                if (l)
                    perm_inv1 = inv;
                else
                    perm_inv0 = inv;
                continue;  // no tables: resolve() and RouteArith work from (start, stride, stride^-1)
            }
            uint16_t* ra = route_at + l * V;
            uint32_t* rt = rtab + l * V;
            [[maybe_unused]] uint32_t carry = 0;  // (not RANKTAB) first slot ordinal of rank k = sum_{k'<k} (len(route_at[k']) + 1)
            for (uint32_t base = 0; base < (uint32_t)V; base += 64) {
                const uint32_t k = base + lane;
                if constexpr (RANKTAB) {  // the rank alone: no list lengths, no prefix scan
                    // start + k x stride < V^2 + V < 2^21 (V <= 1022, node_slot_compact_ok): resolve()'s 32-bit Barrett step, not the 64 x 64 high
                    // multiply of fastmod_u64 (quarter-rate multiplies, two table chunks per leaf and step at 100 lists)
                    if (k < (uint32_t)V) rt[perm_index_recip(pst, psd, k, (uint32_t)V, v_recip32)] = k;
                } else {
                    uint32_t v = 0, e = 0;
                    if (k < (uint32_t)V) {
                        e = fastmod_u64((uint64_t)pst + (uint64_t)k * psd, fm_V);  // (the wide layouts only: every COMPACT kernel is RANKTAB above or, NODEG, has left the loop at ARANK)
                        if constexpr (!COMPACT) ra[k] = (uint16_t)e;
                        v = s_off[e + 1] - s_off[e] + 1;
                    }
                    const uint32_t inc = wave_incl_scan(v);
                    if (k < (uint32_t)V) rt[e] = k | ((carry + inc - v) << 16);
                    carry += __shfl(inc, 63);
                }
            }
        }
        wave_sync();
        if constexpr (SMALL) st_sources += C0.left + C1.left;  // sources generated this step = what leaves the two `left` counts: added here, the remainder taken off at the step's end (nothing to count in the fill loop; the general kernels count there)
        if (total > 0) {
            resolve(C0, 0);
            if (n_leaves > 1) resolve(C1, 1);
        }
        ISA_MARK("prologue_end");

        PH(1)
        // ---- (C) candidate rounds: fill the rings, replay one 64-wide batch, repeat -----------
        int done = 0;
        // SYM: the lockstep round, offered once per step, at the first turn of the loop below (it shares that loop's generation
        // helpers).  Equal max_nearby of at most half a batch, something to scan: at step start both leaves are live with the same `left` and
        // empty rings, and they stay in lockstep for as long as every source emits max_nearby candidates.
        constexpr bool SYM = RBATCH && SF_WAVE_SYM != 0;
        [[maybe_unused]] bool lockstep = SYM && K0 == K1 && K0 <= 32u && total > 0;
        while (!done) {
            PH(4)
            // C1: generation.  Keep >= 32 candidates pending per live leaf (>= min(64, rc - K) when
            // only one leaf is live) so that the replay batch below finds every lane a candidate.
            //
            // gen_rest: one source of leaf l from neighbour-row offset `base` on, `key` = the 64 row
            // entries at base (lane i = entry base + i); returns the number of candidates appended.
            auto gen_rest = [&](int l, uint32_t se, uint32_t sp, uint32_t len, uint32_t k, uint32_t sx, uint32_t tl,
                                uint32_t key, uint32_t base, uint32_t need, uint32_t emitted) -> uint32_t {
                const bool is_change = l ? chg1 : chg0;
                const RT rt = route_facts(l);
                uint32_t* rq = ring + (size_t)l * cv.rc * 2;
                const uint16_t* rowk = nb.keys + (size_t)sx * dim;
                const uint32_t mv0 = (se << 16) | sp;
                for (;;) {
                    const bool have = key != NBR_END;
                    const uint64_t havemask = __ballot(have);
                    if (havemask == 0) break;  // finite entries of the row exhausted
                    NearbyItem it{0u, 0u, 0u, 0u};
                    if (have) it = nearby_item_rt(is_change, node_slot.get(key & NBR_NODE_MASK), se, sp, len, k, s_off, rt);
                    // equal-distance groups are contiguous lane ranges; the index marks entries that
                    // continue the previous entry's distance
                    const uint64_t startmask = __ballot(have && (lane == 0 || !(key & NBR_SAME_FLAG)));
                    const bool more = havemask == ~0ULL && base + 64 < dim;
                    const uint32_t fo = 63u - (uint32_t)__clzll((unsigned long long)startmask);  // first lane of the last group
                    if (SF_SPEC_WIDE_TIES(more && fo == 0)) {
                        // one distance group wider than a chunk (degenerate ties): exact serial
                        // insertion top-k over the rest of the row.
                        TopK tk{~0ULL, 0u, ~0ULL};
                        for (uint32_t b2 = base; b2 < dim; b2 += 64) {
                            const uint32_t j2 = b2 + lane;
                            const uint32_t ky = j2 < dim ? (uint32_t)rowk[j2] : NBR_END;
                            NearbyItem i2{0u, 0u, 0u, 0u};
                            uint64_t hk = 0;
                            if (ky != NBR_END) {
                                const uint32_t y2 = ky & NBR_NODE_MASK;
                                i2 = nearby_item_rt(is_change, node_slot.get(y2), se, sp, len, k, s_off, rt);
                                hk = (uint64_t)m.mat[(size_t)ext_id(sx) * dim + ext_id(y2)] << RT::KEY_SHIFT;  // finite by construction of the index
                            }
                            if (!__ballot(ky != NBR_END)) break;
                            topk_offer(tk, need, i2.w >= 1 ? (hk | i2.ord) : ~0ULL, i2.pay0);
                            topk_offer(tk, need, i2.w == 2 ? (hk | (i2.ord + 1)) : ~0ULL, i2.pay1);
                        }
                        const uint32_t cnt = (uint32_t)__popcll(__ballot(lane < need && tk.key != ~0ULL));
                        if (lane < cnt) {
                            const uint32_t qi = (tl + emitted + lane) & RCM;
                            rq[qi * 2] = mv0;
                            rq[qi * 2 + 1] = tk.pay;
                        }
                        emitted += cnt;
                        break;
                    }
                    const uint32_t nclosed = more ? fo : (uint32_t)__popcll(havemask);  // lanes [0, nclosed): complete groups
                    const uint64_t closedmask = nclosed >= 64 ? ~0ULL : ((1ULL << nclosed) - 1ULL);
                    const bool closed = (closedmask & lanebit) != 0;
                    const uint32_t wc = closed ? it.w : 0u;
                    const uint64_t w1 = __ballot(wc == 1), w2 = __ballot(wc == 2);
                    const uint32_t Wc = (uint32_t)__popcll(w1) + 2u * (uint32_t)__popcll(w2);
                    GC(l ? 6 : 5)
                    if (Wc == 0) { GC(7) }
                    if (Wc > 0) {
                        // sorted position = weight before me, corrected by the inversions inside my group
                        int32_t pos = (int32_t)(mbcnt64(w1) + 2u * mbcnt64(w2));
                        const uint64_t nonstart = SF_SPEC_TIES(~startmask & closedmask);  // lane continues the group of lane-1
#ifdef SF_SPEC_TIE_KEY
                        if (nonstart) pos += tie_key_fix(startmask, nonstart, it.ord, wc);
#else
                        if (nonstart) {
                            const uint32_t packed = (it.ord << 2) | wc;
                            uint64_t run = nonstart;  // bit t: lanes t-d .. t are one group
                            uint32_t p_dn = packed, p_up = packed;
                            for (uint32_t d = 1; run != 0; ++d) {
                                // lane i <- lane i +- d: one whole-wave DPP shift per iteration (no LDS crossbar)
                                p_dn = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p_dn, 0x130, 0xf, 0xf, false);  // wave_shl:1
                                p_up = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)p_up, 0x138, 0xf, 0xf, false);  // wave_shr:1
                                const bool same_up = (run & lanebit) != 0;
                                const bool same_dn = ((run >> d) & lanebit) != 0;
                                if (same_dn && (p_dn >> 2) < it.ord) pos += (int32_t)(p_dn & 3u);
                                if (same_up && (p_up >> 2) > it.ord) pos -= (int32_t)(p_up & 3u);
                                run &= nonstart << d;
                            }
                        }
#endif
                        if (wc >= 1 && (uint32_t)pos < need) {
                            const uint32_t qi = (tl + emitted + (uint32_t)pos) & RCM;
                            rq[qi * 2] = mv0;
                            rq[qi * 2 + 1] = it.pay0;
                        }
                        if (wc == 2 && (uint32_t)pos + 1 < need) {
                            const uint32_t qi = (tl + emitted + (uint32_t)pos + 1) & RCM;
                            rq[qi * 2] = mv0;
                            rq[qi * 2 + 1] = it.pay1;
                        }
                        const uint32_t ne = Wc < need ? Wc : need;
                        emitted += ne;
                        need -= ne;
                    }
                    if (need == 0 || !more) break;
                    base += nclosed;
                    const uint32_t jj = base + lane;
                    key = jj < dim ? (uint32_t)rowk[jj] : NBR_END;
                }
                return emitted;
            };
            // the paired pass's table word into (route << 16 | position).  SAT: the short form, the saturation scan only while some route is longer than
            // pmax -- the common path is one scalar compare (on the count itself: the asm keeps the compiler from carrying `nsat != 0` as a lane mask)
            auto slot_of = [&](uint32_t word, uint32_t node) -> uint32_t {
                if constexpr (SAT) {
                    uint32_t ns = nsat;
                    asm volatile("" : "+s"(ns));
                    if (ns != 0) return node_slot.wide(word, node);
                    return node_slot.wide_short(word);
                } else
                    return node_slot.wide(word, node);
            };
            // ---- the lockstep round.  While every source of both leaves emits max_nearby candidates the two cursors move together: the state of both
            // leaves is ONE triple -- heads sym_h, tails sym_t, sources left sym_left -- and pulls = 2 sym_h, so the union's order puts first_leaf in
            // the even lanes of every batch.  Fill: paired passes while fewer than 32 candidates per leaf are pending.  Batch: 64 lanes, 32 per leaf,
            // all of them valid because the fill loop has just said so: no availability test, no mask.  (The general loop below keeps two cursors,
            // forms `need` for each, and proves the 64 lanes available in every batch: about a fifth of a step's instructions at the default
            // sizes.)  The round ends with the step -- the quota's cut -- or hands the cursors to the general loop for the rest of the step, when a
            // source emits fewer (a short row, a neighbourhood without enough destinations) or no source is left with a batch still short. ----
            if constexpr (SYM) {
                if (lockstep) {
                    lockstep = false;
                    uint32_t sym_h = 0, sym_t = 0, sym_left = total, tA = 0, tB = 0;
                    for (;;) {
                        ISA_MARK("sym_fill_begin");
                        bool leave = false;
                        while (sym_t - sym_h < 32u) {
                            tA = tB = sym_t;
                            if (sym_left == 0) {
                                leave = true;
                                break;
                            }
                            ISA_MARK("pair_begin");
                            GC(0)
                            GC(8)
                            uint32_t sym_left1 = sym_left;  // (one count for both leaves)
#define SF_PAIR_TAIL0 sym_t
#define SF_PAIR_TAIL1 sym_t
#define SF_PAIR_LEFT0 sym_left
#define SF_PAIR_LEFT1 sym_left1
#include "sf_wave_pair_pass.inc"
#undef SF_PAIR_TAIL0
#undef SF_PAIR_TAIL1
#undef SF_PAIR_LEFT0
#undef SF_PAIR_LEFT1
                            ISA_MARK("pair_end");
                            if (emA != K0 || emB != K0) {
                                tA += emA;
                                tB += emB;
                                leave = true;
                                break;
                            }
                            sym_t += K0;
                        }
                        ISA_MARK("sym_fill_end");
                        if (leave) break;
                        wave_sync();
                        ISA_MARK("sym_replay_begin");
                        {
                            constexpr bool valid = true;
                            constexpr uint32_t nvalid = 64u;
                            // the leaf of this lane's candidate is the same in every batch of the round; formed per batch all the same (two vector
                            // instructions against a register carried through the step -- the WPE 6 kernels have none to spare)
                            uint32_t fl = first_leaf, ln = lane;
                            asm volatile("" : "+s"(fl), "+v"(ln));
                            const uint32_t lf = (fl + ln) & 1u, idx = sym_h + (ln >> 1);
                            uint32_t m0, m1, nconsumed = nvalid;
                            uint64_t accmask;
                            [[maybe_unused]] bool doable, acc, consumed;
#include "sf_wave_replay_small.inc"
                            accepted += (uint32_t)__popcll(accmask);
                            if (done) {  // the cut: the step ends inside this batch
                                pulls += nconsumed;
                                break;
                            }
                        }
                        sym_h += 32u;
                        ISA_MARK("sym_replay_end");
                    }
                    // the cursors as the general loop keeps them (after the cut only `pulls` and the `left` counts are read again)
                    pulls += 2u * sym_h;
                    C0.head = C1.head = sym_h;
                    C0.left = C1.left = sym_left;
                    C0.tail = tA;
                    C1.tail = tB;
                    if (!done) { GC(9) }
                    continue;
                }
            }
            const uint32_t single0 = cv.rc - K0 < 64u ? cv.rc - K0 : 64u, single1 = cv.rc - K1 < 64u ? cv.rc - K1 : 64u;
            ISA_MARK("fill_begin");
            for (;;) {
                const bool both_live = !C0.ex && !C1.ex;
                const bool need0 = !C0.ex && C0.left > 0 && C0.tail - C0.head < (both_live ? 32u : single0);
                const bool need1 = n_leaves > 1 && !C1.ex && C1.left > 0 && C1.tail - C1.head < (both_live ? 32u : single1);
                if (!need0 && !need1) break;
                if (need0 && need1) {
                    ISA_MARK("pair_begin");
                    GC(0)
#define SF_PAIR_TAIL0 C0.tail
#define SF_PAIR_TAIL1 C1.tail
#define SF_PAIR_LEFT0 C0.left
#define SF_PAIR_LEFT1 C1.left
#include "sf_wave_pair_pass.inc"
#undef SF_PAIR_TAIL0
#undef SF_PAIR_TAIL1
#undef SF_PAIR_LEFT0
#undef SF_PAIR_LEFT1
                    C0.tail = tlA + emA;
                    C1.tail = tlB + emB;
                    ISA_MARK("pair_end");
                } else {
                    // ---- single source of the one leaf that needs candidates ----
                    const int l = need0 ? 0 : 1;
                    GC(l ? 2 : 1)
                    LeafCursor c = l ? C1 : C0;
                    const uint32_t se = c.se, sp = c.sp, len = c.len, k = c.k, sx = c.sx;
                    // leaf 1 keeps its prefetched entries rotated by 32 lanes for the paired pass
                    uint32_t key = row_key(l ? __shfl(c.pk, (int)((lane + 32u) & 63u)) : c.pk, lane);
                    if constexpr (LEAN) asm volatile("" : "+v"(key)::"memory");  // taken before the next source's row load issues (as in the paired pass)
                    c.left -= 1;
                    c.o += 1;
                    if (c.left > 0) resolve(c, l);
                    if constexpr (!SMALL) st_sources += 1;
                    c.tail += gen_rest(l, se, sp, len, k, sx, c.tail, key, 0u, l ? K1 : K0, 0u);
                    if (l)
                        C1 = c;
                    else
                        C0 = c;
                }
            }
            ISA_MARK("fill_end");
            wave_sync();
            PH(2)

            // C2: replay one batch in union cursor order: trial score, acceptor, forager
            ISA_MARK("replay_begin");
            {
                const bool live0 = !C0.ex, live1 = !C1.ex;
                if (!live0 && !live1) {
                    done = 1;
                    break;
                }
                const bool both = live0 && live1;
                uint32_t lf, idx;
                if (both) {
                    const uint32_t l0 = (first_leaf + pulls) & 1u;
                    lf = (l0 + lane) & 1u;
                    idx = (lf ? C1.head : C0.head) + (lane >> 1);
                } else {
                    lf = live0 ? 0u : 1u;
                    idx = (lf ? C1.head : C0.head) + lane;
                }
                const bool avail = (int32_t)((lf ? C1.tail : C0.tail) - idx) > 0;
                const uint64_t availmask = __ballot(avail);
                const uint32_t nvalid = availmask == ~0ULL ? 64u : (uint32_t)(__ffsll((unsigned long long)~availmask) - 1);
                if (nvalid == 0) {
                    // the scheduler discovers an exhausted child at this pull (vec_union.rs:334-362);
                    // a leaf with sources left was refilled above, so an empty ring means exhausted.
                    const uint32_t lf0 = uni(__shfl(lf, 0));
                    if (lf0)
                        C1.ex = 1;
                    else
                        C0.ex = 1;
                    continue;
                }
                const bool valid = lane < nvalid;
                uint32_t m0 = 0, m1 = 0;
                ScoreV<L> sc;
#pragma unroll
                for (int kk = 0; kk < L; ++kk) sc.v[kk] = 0;
                bool doable = false, acc = false, consumed = false, improving_pick = false;
                uint64_t accmask = 0;
                uint32_t nconsumed = nvalid;
                if constexpr (SMALL) {
#include "sf_wave_replay_small.inc"
                } else {
                    ListDelta dl{0, 0, false};
                    if (valid) {
                        const uint32_t qi = idx & RCM;
                        const uint32_t* rq = ring + ((size_t)lf * cv.rc + qi) * 2;
                        m0 = rq[0];
                        m1 = rq[1];
                        const uint32_t a = m0 >> 16, i = m0 & 0xFFFFu, b = m1 >> 16, j = m1 & 0xFFFFu;
                        dl = eval_list_move_legs<uint16_t, FAST>(m, s_visits, s_off, s_load, lf ? chg1 : chg0, a, i, b, j);
                    }
                    sc = apply_delta<L>(m, cur, dl);
                    ScoreV<L> curv;
    #pragma unroll
                    for (int kk = 0; kk < L; ++kk) curv.v[kk] = cur[kk];
                    doable = valid && dl.doable;
                    if (doable) {
                        if (acceptor == 0)
                            acc = score_cmp<L>(sc, curv) > 0;
                        else if (acceptor == 1)
                            acc = score_cmp<L>(sc, curv) >= 0 || score_cmp<L>(sc, late) >= 0;
                        else if (acceptor == 4)
                            acc = score_cmp<L>(sc, curv) >= 0 || score_cmp<L>(sc, late) >= 0 || score_cmp<L>(sc, dla_thr) >= 0;
                    }
                    if constexpr (TRACE)
                        if (acceptor == 5 || acceptor == 6) acc = ax_accepts<L>(doable, sc, curv, late, thr_on);
                    if constexpr (TRACE)
                        if (acceptor == 7) {  // the candidate's signature from the working lists, which no candidate of the step has changed
                            TabuSig sig{{TABU_NO_TOKEN, TABU_NO_TOKEN}, {TABU_NO_TOKEN, TABU_NO_TOKEN}, {0, 0}, {0, 0}};
                            if (doable) {  // (a doable move's positions lie inside their lists)
                                const uint32_t a = m0 >> 16, i = m0 & 0xFFFFu, b = m1 >> 16, j = m1 & 0xFFFFu;
                                const uint32_t u = ext_id(s_visits[s_off[a] + i]);
                                if (lf ? chg1 : chg0)  // j is the destination before the removal (apply_list_move_wave): adjusted_destination, change.rs:28-34
                                    tabu_sig_list_change(tabu_scope, a, i, b, (a == b && j > i) ? j - 1 : j, u, sig);
                                else
                                    tabu_sig_list_swap(tabu_scope, a, i, u, b, j, ext_id(s_visits[s_off[b] + j]), sig);
                            }
                            acc = tabu_accepts<L>(tabu, doable, sc, sig);
                        }
                    SaChunk sach;
                    if constexpr (!FAST)
                        if (annealing) acc = sa_decide<L>(saw, p.sa, doable, sc, curv, lane, sach);
                    accmask = __ballot(acc);
                    ScoreV<L> forager_thr = curv;  // FirstLastStepScoreImproving: the last step score
                    if (forager == FORAGER_FIRST_BEST_IMPROVING) {  // the best score ever seen (step.rs:53-58)
    #pragma unroll
                        for (int kk = 0; kk < L; ++kk) forager_thr.v[kk] = best_sol[kk];
                    }
                    nconsumed = forager_chunk_cut<L>(forager, (uint32_t)SF_SPEC_LIMIT(p.limit), accepted, acc, sc, forager_thr, nvalid, improving_pick);
                    consumed = lane < nconsumed;
                    if constexpr (!FAST)
                        if (annealing) sa_commit<L>(saw, p.sa, sach, nconsumed, lane);
                    acc = acc && consumed;
                    accmask = __ballot(acc);
                    if (accmask) {
                        if (improving_pick) {  // BestCandidate::replace by the candidate that ends the step (improving.rs:92-95,205-208)
                            const int sel = (int)nconsumed - 1;
    #pragma unroll
                            for (int kk = 0; kk < L; ++kk) best.v[kk] = (int64_t)uni64(shfl_u64((uint64_t)sc.v[kk], sel));
                            best_m0 = __shfl(m0, sel);
                            best_m1 = __shfl(m1, sel);
                            best_leaf = (int)__shfl(lf, sel);
                            if (TRACE) best_ti = trace_n + (uint64_t)sel;
                            equal_count = 1;
                            has_best = 1;
                        } else if (forager == 1) {
                            if (!has_best) {
                                const int sel = __ffsll((unsigned long long)accmask) - 1;
    #pragma unroll
                                for (int kk = 0; kk < L; ++kk) best.v[kk] = (int64_t)uni64(shfl_u64((uint64_t)sc.v[kk], sel));
                                best_m0 = __shfl(m0, sel);
                                best_m1 = __shfl(m1, sel);
                                best_leaf = (int)__shfl(lf, sel);
                                if (TRACE) best_ti = trace_n + (uint64_t)sel;
                                has_best = 1;
                            }
                        } else if (!has_best || __ballot(acc && score_cmp<L>(sc, best) >= 0)) {
                            const ScoreV<L> M = wave_max_score<L>(sc, acc);
                            const int cm = has_best ? score_cmp<L>(M, best) : 1;
                            if (cm >= 0) {
                                const bool newmax = cm > 0;
                                const uint64_t eq_base = newmax ? 0 : equal_count;
                                const bool in_eq = acc && score_cmp<L>(sc, M) == 0;
                                const uint64_t eq = __ballot(in_eq);
                                const uint32_t rank = mbcnt64(eq) + 1u;
                                const uint64_t cntq = eq_base + rank;
                                const bool pick = in_eq && ((newmax && rank == 1) ||
                                                            (p.random_ties && cntq > 1 && reservoir_pick(sseed, cntq)));
                                const uint64_t pm = __ballot(pick);
                                if (pm) {
                                    const int sel = 63 - __clzll((unsigned long long)pm);
                                    best_m0 = __shfl(m0, sel);
                                    best_m1 = __shfl(m1, sel);
                                    best_leaf = (int)__shfl(lf, sel);
                                    if (TRACE) best_ti = trace_n + (uint64_t)sel;
                                }
    #pragma unroll
                                for (int kk = 0; kk < L; ++kk) best.v[kk] = (int64_t)uni64((uint64_t)M.v[kk]);
                                equal_count = eq_base + (uint64_t)__popcll(eq);
                                has_best = 1;
                            }
                        }
                    }
                }
                const uint32_t nacc = (uint32_t)__popcll(accmask);
                accepted += nacc;
                if constexpr (!RBATCH) st_scored += nvalid;  // (RBATCH: a batch scores what it consumes except where the quota cuts it -- added once per step from `pulls`, the cut's remainder at the cut)
                if constexpr (!SMALL) {  // (SMALL: moves_generated / accepted are added once per step from `pulls` / `accepted`; every candidate is doable)
                    st_gen += nconsumed;
                    st_acc += nacc;
                    const uint32_t ndo = (uint32_t)__popcll(__ballot(consumed && doable));
                    st_calc += ndo;
                }
                if (tracing && consumed) {
                    const uint64_t ti = trace_n + lane;
                    if ((int64_t)ti < p.trace_cap) {
                        int32_t* tm = p.trace_moves + ti * 6;
                        tm[0] = (lf ? chg1 : chg0) ? 2 : 3;
                        tm[1] = (int32_t)(m0 >> 16);
                        tm[2] = (int32_t)(m0 & 0xFFFFu);
                        tm[3] = (int32_t)(m1 >> 16);
                        tm[4] = (int32_t)(m1 & 0xFFFFu);
                        tm[5] = -1;
                        for (int kk = 0; kk < L && kk < m.levels; ++kk) p.trace_scores[ti * m.levels + kk] = doable ? sc.v[kk] : 0;
                        p.trace_flags[ti] = (doable ? 1 : 0) | (acc ? 2 : 0) | ((int32_t)lf << 8);
                    }
                }
                if (tracing) trace_n += nconsumed;
                uint32_t c1;
                if constexpr (SMALL) {  // the lanes alternate the two leaves from the batch's first pull on: no ballot needed
                    const uint32_t lfirst = (uint32_t)__builtin_amdgcn_readfirstlane((int)lf);
                    c1 = both ? ((nconsumed + lfirst) >> 1) : (lfirst ? nconsumed : 0u);
                } else {
                    c1 = (uint32_t)__popcll(__ballot(consumed && lf == 1u));
                }
                C1.head += c1;
                C0.head += nconsumed - c1;
                pulls += nconsumed;
                if constexpr (!RBATCH)  // (RBATCH: decided at the cut)
                    if (forager_quits(forager, (uint32_t)SF_SPEC_LIMIT(p.limit), accepted, has_best, improving_pick)) done = 1;
            }
            ISA_MARK("replay_end");
            PH(3)
        }
        PH(4)

        // ---- (D) commit the forager's pick (step.rs:122-221) ----------------------------------
        ISA_MARK("commit_begin");
        if constexpr (SMALL) st_sources -= C0.left + C1.left;
        if constexpr (SMALL) {
            if constexpr (L == 2) {  // the key back into its two level deltas, once per step: key = hard x 2^32 + soft (sign-extended)
                const int32_t soft = (int32_t)(uint32_t)(uint64_t)best_key;
                best_d[1] = soft;
                best_d[0] = (int32_t)(uint32_t)((uint64_t)wsub(best_key, (int64_t)soft) >> 32);
            }
#pragma unroll
            for (int kk = 0; kk < L; ++kk) best.v[kk] = wadd(cur[kk], (int64_t)best_d[kk]);
        }
        const bool applied = has_best && !dry_run;
        [[maybe_unused]] TabuSig pick_sig;  // TabuSearch: the pick's signature, taken before the commit writes the lists
        if (applied) {
            if (best_pending) {
                ScoreV<L> bs;
#pragma unroll
                for (int kk = 0; kk < L; ++kk) bs.v[kk] = best_sol[kk];
                if (!(score_cmp<L>(best, bs) > 0)) {  // leaving the best state: write its snapshot first
                    const uint32_t tot = uni(s_off[V]);
                    uint32_t* const bv = SF_COLD_M(best_visits) + (size_t)r * SF_SPEC_NCAP(SF_COLD_M(n_cap));
                    uint32_t* const bo = SF_COLD_M(best_off) + (size_t)r * (V + 1);
                    // RANKTAB: the lane index is formed again HERE.  Taken from the kernel's `lane`, this cold block's per-lane LDS and global
                    // addresses are computed in the kernel's prologue and carried to it -- the kernel has no free vector register, so with the
                    // table index above they went through scratch memory
                    uint32_t ln = lane;
                    if constexpr (RANKTAB) asm volatile("" : "+v"(ln));
                    for (uint32_t t = ln; t < tot; t += 64) bv[t] = ext_id(s_visits[t]);
                    for (uint32_t t = ln; t <= (uint32_t)V; t += 64) bo[t] = s_off[t];
                    best_pending = false;
                }
            }
            const int kind = (best_leaf ? chg1 : chg0) ? 2 : 3;
            const uint32_t a = uni(best_m0 >> 16), i = uni(best_m0 & 0xFFFFu);
            const uint32_t b = uni(best_m1 >> 16), j = uni(best_m1 & 0xFFFFu);
            if (tracing && lane == 0) {
                p.trace_applied[0] = 1;
                if ((int64_t)best_ti < p.trace_cap) p.trace_flags[best_ti] |= 4;  // Selected + Applied
                p.trace_applied[1] = kind;
                p.trace_applied[2] = (int32_t)a;
                p.trace_applied[3] = (int32_t)i;
                p.trace_applied[4] = (int32_t)b;
                p.trace_applied[5] = (int32_t)j;
                p.trace_applied[6] = -1;
            }
            if constexpr (SAT) {
                if (kind == 2 && a != b) {  // the one committed move that changes list lengths: a loses an element, b gains one
                    const uint32_t la0 = uni(s_off[a + 1] - s_off[a]), lb0 = uni(s_off[b + 1] - s_off[b]);
                    nsat += (lb0 == node_slot.pmax ? 1u : 0u);
                    nsat -= (la0 == node_slot.pmax + 1u ? 1u : 0u);
                }
                nsat = uni(nsat);  // (the move's kind comes out of a shuffle: say that the count is wave-uniform, so the pass branches on a scalar)
            }
            if constexpr (TRACE)
                if (acceptor == 7) {
                    const uint32_t u = ext_id(s_visits[s_off[a] + i]);
                    if (kind == 2)
                        tabu_sig_list_change(tabu_scope, a, i, b, (a == b && j > i) ? j - 1 : j, u, pick_sig);
                    else
                        tabu_sig_list_swap(tabu_scope, a, i, u, b, j, ext_id(s_visits[s_off[b] + j]), pick_sig);
                }
            apply_list_move_wave<LT, OT, RANKTAB && L == 4>(m, s_visits, s_off, s_load, kind, a, i, b, j);  // (the four-level COMPACT kernels: one register short without it)
            {  // refresh node -> (route, position) for the two touched routes
                const uint32_t oa = s_off[a], la = s_off[a + 1] - oa;
                const uint32_t ob = s_off[b], lb = s_off[b + 1] - ob;
                for (uint32_t t = lane; t < la + (a != b ? lb : 0u); t += 64) {
                    if (t < la)
                        node_slot.set(s_visits[oa + t], a, t);
                    else
                        node_slot.set(s_visits[ob + (t - la)], b, t - la);
                }
            }
            node_sync();
#pragma unroll
            for (int kk = 0; kk < L; ++kk) cur[kk] = best.v[kk];
            st_applied += 1;
        } else if (tracing && lane == 0) {
            p.trace_applied[0] = 0;
        }
        if (!dry_run) {
            // update_best_solution (scope_progress.rs:89-107): clone on strict improvement
            bool improved = false;
            if (applied) {
                ScoreV<L> cs, bs;
#pragma unroll
                for (int kk = 0; kk < L; ++kk) {
                    cs.v[kk] = cur[kk];
                    bs.v[kk] = best_sol[kk];
                }
                improved = score_cmp<L>(cs, bs) > 0;
            }
            if (improved) {  // the clone is deferred until the search leaves this state (best_pending)
                best_pending = true;
#pragma unroll
                for (int kk = 0; kk < L; ++kk) best_sol[kk] = cur[kk];
            }
            // acceptor.step_ended(last_step_score) always (step.rs:216-221)
            const int la_size = SF_SPEC_LA_SIZE(SF_COLD_P(la_size));
            if ((acceptor == 1 || acceptor == 4) && lane == 0) {
                int64_t* const lh = SF_COLD_P(la_hist) + ((size_t)r * la_size + la_slot) * 4;
#pragma unroll
                for (int kk = 0; kk < L; ++kk) lh[kk] = cur[kk];
            }
            if (acceptor == 4 && lane == 0) {  // step_ended: the phase's best step score (diversified_late_acceptance.rs:161-170)
                ScoreV<L> cs, db;
#pragma unroll
                for (int kk = 0; kk < L; ++kk) {
                    cs.v[kk] = cur[kk];
                    db.v[kk] = p.dla_best[(size_t)r * 4 + kk];
                }
                if (score_cmp<L>(cs, db) > 0) {
#pragma unroll
                    for (int kk = 0; kk < L; ++kk) p.dla_best[(size_t)r * 4 + kk] = cur[kk];
                }
            }
            if constexpr (TRACE)
                if (acceptor == 5 || acceptor == 6) ax_step_ended<L>(acceptor, lane == 0, cur, p.sa.state + (size_t)r * SA_WORDS);
            if constexpr (TRACE)
                if (acceptor == 7) tabu_step_ended<L>(p.sa.state + (size_t)r * SA_WORDS, lane == 0, cur, applied ? &pick_sig : nullptr);
            if constexpr (!FAST)
                if (annealing) sa_step_ended(saw, p.sa, lane);
            wave_sync();
            st_steps += 1;
            if constexpr (SMALL) {
                st_gen += pulls;
                st_calc += pulls;
                st_acc += accepted;
                if constexpr (RBATCH) st_scored += pulls;
            }
            la_cursor = la_cursor + 1 >= la_size ? 0 : la_cursor + 1;
            const int64_t move_budget = SF_COLD_P(move_budget);
            if (move_budget > 0 && (int64_t)st_gen >= move_budget) {  // work-balanced launch: see sf_solve_moves (budget < 2^31)
                if constexpr (SMALL) ++step;
                break;
            }
            if (move_budget == 0 && st_scored >= 0x70000000u) flush_stats();
        }
        ISA_MARK("commit_end");
        PH(5)
    }
    PH_DUMP

    // ---- write back ----------------------------------------------------------------------
    if (!dry_run) {
        if constexpr (!FAST)
            if (annealing) sa_store(saw, p.sa, r, lane);
        const uint32_t tot = uni(s_off[V]);
        uint32_t wlane = lane;
        SF_SPEC_OWN_LANE(wlane);
        // SMALL: the replica's base pointers, formed again from the argument block
        const size_t n_cap = (size_t)SF_SPEC_NCAP(SF_COLD_M(n_cap));
        uint32_t* const w_visits = SMALL ? SF_COLD_M(visits) + (size_t)r * n_cap : g_visits;
        uint32_t* const w_off = SMALL ? SF_COLD_M(off) + (size_t)r * (V + 1) : g_off;
        int64_t* const w_load = SMALL ? SF_COLD_M(load) + (size_t)r * V : g_load;
        int64_t* const w_score = SMALL ? SF_COLD_M(score) + (size_t)r * 4 : g_score;
        if (best_pending) {  // the launch ends in a best state: its deferred snapshot
            uint32_t* const bv = SF_COLD_M(best_visits) + (size_t)r * n_cap;
            uint32_t* const bo = SF_COLD_M(best_off) + (size_t)r * (V + 1);
            for (uint32_t t = wlane; t < tot; t += 64) bv[t] = ext_id(s_visits[t]);
            for (uint32_t t = wlane; t <= (uint32_t)V; t += 64) bo[t] = s_off[t];
        }
        for (uint32_t t = wlane; t < tot; t += 64) w_visits[t] = ext_id(s_visits[t]);
        for (uint32_t t = wlane; t <= (uint32_t)V; t += 64) w_off[t] = s_off[t];
        for (uint32_t t = wlane; t < (uint32_t)V; t += 64) w_load[t] = (int64_t)s_load[t];
        if (lane == 0) {
#pragma unroll
            for (int kk = 0; kk < L; ++kk) {
                w_score[kk] = cur[kk];
                SF_COLD_P(last_step_score)[(size_t)r * 4 + kk] = cur[kk];
                SF_COLD_M(best_score)[(size_t)r * 4 + kk] = best_sol[kk];
            }
            SF_COLD_P(la_idx)[r] = la_cursor;
            const uint64_t ran = SMALL ? (uint64_t)step : steps_run + (uint64_t)st_steps;  // steps actually run
            SF_COLD_P(step_index)[r] = step_index0 + ran;
            SF_COLD_P(seed_draws)[r] = seed_draws0 + ran;
        }
        flush_stats();
    }
    if (tracing && lane == 0) *p.trace_count = (int64_t)trace_n;
}

#undef SF_COLD_P
#undef SF_COLD_M

// cold_args(): the kernel's parameter list is WaveArgs' member list (one signature for every instantiation)
template <class F>
struct wave_args_are : std::false_type {};
template <>
struct wave_args_are<void (*)(decltype(WaveArgs::m), decltype(WaveArgs::p), decltype(WaveArgs::nb))> : std::true_type {};
static_assert(wave_args_are<decltype(&k_list_search_wave<2, false, 2>)>::value && std::is_standard_layout<WaveArgs>::value,
              "WaveArgs must list k_list_search_wave's parameters, in order: cold_args() reads the kernarg segment through it");

}  // namespace sf
