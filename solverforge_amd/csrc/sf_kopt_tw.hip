// Time windows of the stock CVRP domain on the device: route_hooks::feasible = capacity + time windows
// (crates/solverforge-cvrp/src/helpers.rs:109-119, 168-218) as feasible_mode 2 of the route-local 2-opt phase and as a query over the
// committed lists (sf_list_routes_feasible).
//
// The time recurrence of route_is_time_feasible (helpers.rs:181-218), restated:
//   t = departure; per visit v after prev:  t += travel(prev, v)   [no finite leg, or i64 overflow -> false]
//                                           t = max(t, lo[v]);  service[v] < 0 -> false;  t += service[v]  [overflow -> false]
//                                           t > hi[v] -> false
//   at the end the leg back to the depot must be finite and t + leg must not overflow.
// Unlike capacity this depends on the order of the visits, so inside 2-opt it is judged per improving candidate, on the route as
// it stands then (the reversals already taken in the same row included): k_list_construct_two_opt_tw below.
//
// Two evaluations of one route, both wave-uniform:
//   tw_walk_checked   every lane walks the n visits with checked adds: the recurrence to the letter, n dependent steps.
//   tw_fold_composed  a visit is the map  t -> max(t + leg, lo) + service  with the side condition "result <= hi".  A chain of
//                     visits is again of that shape: (a, b, l, ok) = out(t) = max(t + a, b), admissible iff ok and t <= l.  The maps
//                     compose associatively, so each lane folds a contiguous chunk of the route (plus the leg back to the depot
//                     as a last item) and six ordered cross-lane steps give the whole route: O(n / 64 + 6) instead of n.
//                     Exact only while no intermediate leaves i64: the host range check of sf_list_set_time_windows (TwTables::composed)
//                     admits data whose every sum stays below 2^59 in magnitude, everything else takes the checked walk.
// The tables live in the caller's node ids, like lm.mat / lm.visits.  They are an argument of the kernels of this file only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_clarke_wright.hip"

namespace sf {

struct TwTables {
    const int64_t* lo;       // [dim]
    const int64_t* hi;       // [dim]
    const int64_t* service;  // [dim]
    const int64_t* travel;   // [dim][dim] row-major
    int64_t departure;
    int32_t composed;        // host range check passed: tw_fold_composed is exact on this data
    int32_t* ran;            // [1] the evaluation a kernel took: 1 checked walk, 2 composed fold (nullptr: not recorded)
};

constexpr int64_t TW_BIG = (int64_t)1 << 61;     // "no bound" of the composed maps; the host gate keeps every real quantity below 2^59
constexpr int64_t TW_GATE = (int64_t)1 << 59;

__device__ __forceinline__ bool tw_travel(const ListModel& lm, const TwTables& tw, uint32_t from, uint32_t to, int64_t& out) {  // problem_data.rs:38-41
    const int64_t v = tw.travel[(size_t)from * (size_t)lm.dim + to];
    out = v;
    return v >= 0 && v != UNREACHABLE;
}

// position -> visit of a route held in LDS with [i..=j] read reversed
struct TwLdsRoute {
    const lds_u16* route;
    uint32_t i, j;
    __device__ __forceinline__ uint32_t operator()(uint32_t p) const { return route[(p >= i && p <= j) ? i + j - p : p]; }
};
struct TwGlobalRoute {
    const uint32_t* visits;
    __device__ __forceinline__ uint32_t operator()(uint32_t p) const { return visits[p]; }
};

template <class At>
__device__ __forceinline__ bool tw_walk_checked(const ListModel& lm, const TwTables& tw, const At& at, uint32_t n) {
    int64_t t = tw.departure, leg;
    uint32_t prev = (uint32_t)lm.depot;
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t v = at(p);
        if (!tw_travel(lm, tw, prev, v, leg) || __builtin_add_overflow(t, leg, &t)) return false;
        const int64_t lo = tw.lo[v], s = tw.service[v];
        if (t < lo) t = lo;
        if (s < 0 || __builtin_add_overflow(t, s, &t)) return false;
        if (t > tw.hi[v]) return false;
        prev = v;
    }
    int64_t back;
    return tw_travel(lm, tw, prev, (uint32_t)lm.depot, leg) && !__builtin_add_overflow(t, leg, &back);
}

struct TwMap {
    int64_t a, b, l;  // out(t) = max(t + a, b); admissible entry times t <= l
    bool ok;
};
// x = x followed by y
__device__ __forceinline__ void tw_then(TwMap& x, const TwMap& y) {
    const int64_t l2 = y.l - x.a, b1 = x.b + y.a;
    x.ok = x.ok && y.ok && x.b <= y.l;
    x.l = x.l < l2 ? x.l : l2;
    x.b = b1 > y.b ? b1 : y.b;
    x.a += y.a;
}

template <class At>
__device__ __forceinline__ bool tw_fold_composed(const ListModel& lm, const TwTables& tw, const At& at, uint32_t n, uint32_t lane) {
    const uint32_t items = n + 1u;  // the visits, then the leg back to the depot
    const uint32_t chunk = (items + 63u) / 64u;
    const uint32_t p0 = lane * chunk;
    const uint32_t p1 = p0 + chunk < items ? p0 + chunk : items;
    TwMap x{0, -TW_BIG, TW_BIG, true};
    uint32_t prev = (p0 == 0 || p0 >= items) ? (uint32_t)lm.depot : at(p0 - 1u);
    for (uint32_t p = p0; p < p1; ++p) {
        TwMap y{0, -TW_BIG, TW_BIG, true};
        int64_t leg;
        if (p < n) {
            const uint32_t v = at(p);
            const bool fin = tw_travel(lm, tw, prev, v, leg);
            const int64_t lo = tw.lo[v], hi = tw.hi[v], s = tw.service[v];
            if (fin && s >= 0) {
                y.a = leg + s, y.b = lo + s, y.l = hi - s - leg, y.ok = lo + s <= hi;
            } else {
                y.ok = false;
            }
            prev = v;
        } else {
            y.ok = tw_travel(lm, tw, prev, (uint32_t)lm.depot, leg);
            if (y.ok) y.a = leg;
        }
        tw_then(x, y);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        TwMap o;
        o.a = (int64_t)shfl_xor_u64((uint64_t)x.a, m);
        o.b = (int64_t)shfl_xor_u64((uint64_t)x.b, m);
        o.l = (int64_t)shfl_xor_u64((uint64_t)x.l, m);
        o.ok = __shfl_xor((int)x.ok, m, 64) != 0;
        if (lane & (uint32_t)m) {  // the partner's block comes first
            tw_then(o, x);
            x = o;
        } else {
            tw_then(x, o);
        }
    }
    return x.ok && tw.departure <= x.l;
}

template <class At>
__device__ __forceinline__ bool tw_route_feasible(const ListModel& lm, const TwTables& tw, const At& at, uint32_t n, uint32_t lane) {
    return tw.composed ? tw_fold_composed(lm, tw, at, n, lane) : tw_walk_checked(lm, tw, at, n);
}
// what a kernel that evaluated at least one route records for sf_list_time_window_path (every such wave writes the same value)
__device__ __forceinline__ void tw_record_path(const TwTables& tw, uint32_t lane) {
    if (tw.ran && lane == 0) *tw.ran = tw.composed ? 2 : 1;
}

// ---- ListKOptPhase with the complete route_hooks::feasible (feasible_mode 2).  The shape of k_list_construct_two_opt: one wavefront
// per (route, replica), the route as u16 in LDS, 64 values of j per round, the improving lanes taken in ascending order.  The
// improving predicate of a later j of the row still reads only positions > j0 and the stale a, b, so the ballot stays valid; the hook
// of a later lane depends on the reversals taken before it, so it is evaluated lane by lane on the index-mapped reversed route and the
// reversal is written only when it passes.  Capacity does not depend on the order: one flag per route, as in mode 1.
__global__ __launch_bounds__(64) void k_list_construct_two_opt_tw(ListModel lm, TwTables tw, int max_sweeps, uint64_t* stats) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    lds_u16* route = (lds_u16*)smem;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x;
    const int r = blockIdx.y;
    const uint32_t V = (uint32_t)lm.V;
    uint32_t* g_visits = lm.visits + (size_t)r * lm.n_cap;
    const uint32_t* g_off = lm.off + (size_t)r * (V + 1);
    const uint32_t o = g_off[e], n = g_off[e + 1] - o;
    if (n < 4) return;
    for (uint32_t t = lane; t < n; t += 64) route[t] = (uint16_t)g_visits[o + t];
    wave_sync();
    const bool feas = lm.load[(size_t)r * V + e] <= lm.capacity;
    const uint32_t depot = (uint32_t)lm.depot;
    uint64_t cand = 0, acc = 0;
    bool changed = false, hooked = false;
    int sweeps = 0;
    for (;;) {
        bool improved = false;
        for (uint32_t i = 0; i + 1 < n; ++i) {
            const uint32_t a = i == 0 ? depot : (uint32_t)uni(route[i - 1]);
            const uint32_t b = uni(route[i]);
            const int64_t dab = cw_dist_cost(lm, a, b);
            for (uint32_t j0 = i + 1; j0 < n; j0 += 64) {
                const uint32_t j = j0 + lane;
                bool imp = false;
                if (j < n) {
                    const uint32_t c = route[j];
                    const uint32_t en = j + 1 < n ? (uint32_t)route[j + 1] : depot;
                    imp = cw_dist_cost(lm, a, c) + cw_dist_cost(lm, b, en) < dab + cw_dist_cost(lm, c, en);
                }
                cand += (n - j0) < 64u ? (n - j0) : 64u;
                uint64_t mask = __ballot(imp);
                if (!feas) mask = 0ull;
                while (mask) {
                    const uint32_t jj = j0 + (uint32_t)__builtin_ctzll(mask);
                    mask &= mask - 1ull;
                    const TwLdsRoute at{route, i, jj};
                    hooked = true;
                    if (!tw_route_feasible(lm, tw, at, n, lane)) continue;
                    const uint32_t half = (jj - i + 1u) / 2u;
                    wave_sync();
                    for (uint32_t t = lane; t < half; t += 64) {
                        const uint16_t x = route[i + t], y = route[jj - t];
                        route[i + t] = y;
                        route[jj - t] = x;
                    }
                    wave_sync();
                    ++acc;
                    improved = changed = true;
                }
            }
        }
        if (!improved || ++sweeps >= max_sweeps) break;  // max_sweeps = the termination policy (kernel.rs:117-121)
    }
    if (changed)
        for (uint32_t t = lane; t < n; t += 64) g_visits[o + t] = route[t];
    if (hooked) tw_record_path(tw, lane);
    if (stats && lane == 0) {
        uint64_t* gs = stats + (size_t)r * SF_STATS_WORDS;
        atomicAdd((unsigned long long*)&gs[1], (unsigned long long)cand);
        atomicAdd((unsigned long long*)&gs[2], (unsigned long long)cand);
        atomicAdd((unsigned long long*)&gs[7], (unsigned long long)cand);
        atomicAdd((unsigned long long*)&gs[3], (unsigned long long)acc);
        if (changed) {
            atomicAdd((unsigned long long*)&gs[4], (unsigned long long)acc);
            atomicAdd((unsigned long long*)&gs[0], 1ull);
            atomicAdd((unsigned long long*)&gs[5], 1ull);
        }
    }
}

// ---- route_hooks::feasible on the committed lists: one wavefront per (route, replica).  feasible_mode 1 = capacity, 2 = capacity + time
// windows (tw is read by mode 2 only).  An empty route is feasible (helpers.rs:109-112).
__global__ __launch_bounds__(64) void k_list_routes_feasible(ListModel lm, TwTables tw, int feasible_mode, int32_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t e = blockIdx.x;
    const int r = blockIdx.y;
    const uint32_t V = (uint32_t)lm.V;
    const uint32_t* g_off = lm.off + (size_t)r * (V + 1);
    const uint32_t o = g_off[e], n = g_off[e + 1] - o;
    bool ok = true;
    if (n > 0) {
        ok = lm.load[(size_t)r * V + e] <= lm.capacity;
        if (ok && feasible_mode == 2) {
            const TwGlobalRoute at{lm.visits + (size_t)r * lm.n_cap + o};
            ok = tw_route_feasible(lm, tw, at, n, lane);
            tw_record_path(tw, lane);
        }
    }
    if (lane == 0) out[(size_t)r * V + e] = ok ? 1 : 0;
}

}  // namespace sf
