// The paired pass of k_list_search_wave (sf_list_wave.hip), as statements: included inside the kernel, once in the general fill loop and once in
// the lockstep round (DESIGN 28).  A text fragment and not a lambda on purpose: the kernels without the round must compile to the code they had,
// and they do only while the general loop's statements are the ones it always had.  It names the kernel's locals (C0, C1, resolve, gen_rest,
// slot_of, half, ...) and leaves emA / emB, tlA / tlB in the including scope.  The includer defines, and undefines afterwards:
//   SF_PAIR_TAIL0 / SF_PAIR_TAIL1   the ring tails of the two leaves (read once)
//   SF_PAIR_LEFT0 / SF_PAIR_LEFT1   their sources-left counts (lvalues: decremented; the next source is resolved while one is left)
// ---- paired pass: lanes 0-31 = the first 32 row entries of leaf 0's source, lanes
// 32-63 = the first 32 of leaf 1's (its prefetch is stored rotated by 32 lanes) ----
const bool hi = lane >= 32;
const uint32_t seA = C0.se, spA = C0.sp, lenA = C0.len, kA = C0.k, sxA = C0.sx, tlA = SF_PAIR_TAIL0;
const uint32_t seB = C1.se, spB = C1.sp, lenB = C1.len, kB = C1.k, sxB = C1.sx, tlB = SF_PAIR_TAIL1;
// LEAN: each half blanks the lanes past its row now (resolve() left the entries raw)
uint32_t l31 = lane & 31u;
if constexpr (LEAN) asm volatile("" : "+v"(l31));  // (formed per pass: hoisted out of the loops, `l31 < dim` is a 64-bit mask in spill lanes)
// (SF_SPEC_ROWS_FULL: both halves lie inside their rows and every entry is finite -- `have` is a literal, and with it the blanking
// selects, `havemask`, its halves and the count arm of `ncv` below)
const uint32_t key = LEAN ? (SF_SPEC_ROW_HAVE(false) ? half(C0.pk, C1.pk) : row_key(half(C0.pk, C1.pk), l31)) : (hi ? C1.pk : C0.pk);
const bool have = SF_SPEC_ROW_HAVE(key != NBR_END);
uint32_t nd = have ? (key & NBR_NODE_MASK) : 0u;  // unconditional read below (node 0 for the lanes past the row)
uint32_t slot_word = 0;
if constexpr (LEAN) {
    // the current keys are taken HERE, before the next sources' row loads issue: the only wait for a row load in the pass is this one,
    // for the loads of the pass before (the asm pins the order: the scheduler would otherwise sink the use below the new loads)
    asm volatile("" : "+v"(nd)::"memory");
    slot_word = node_slot.word(nd);  // ... and the table read is in flight across resolve()
}
SF_PAIR_LEFT0 -= 1;
C0.o += 1;
if (SF_PAIR_LEFT0 > 0) resolve(C0, 0);
SF_PAIR_LEFT1 -= 1;
C1.o += 1;
if (SF_PAIR_LEFT1 > 0) resolve(C1, 1);
if constexpr (!SMALL) st_sources += 2;
uint32_t slot_any;
if constexpr (LEAN)
    slot_any = slot_of(slot_word, nd);
else
    slot_any = node_slot.get(nd);
const uint32_t slot = have ? slot_any : NODE_NONE;
NearbyItem it{0u, 0u, 0u, 0u};
uint32_t mv0, tl, Kh, rq_off;  // this lane's half: source (entity << 16 | position), ring tail, max_nearby, ring offset in words
if constexpr (LEAN) {
    // leaf 0 = nearby change (lanes 0-31), leaf 1 = nearby swap (lanes 32-63), as in the FAST item below, but every fact of a half picked
    // with half() and every predicate ONE unsigned compare of two selected words: no `hi` mask, no nested exec-mask regions.
    //   v0  change: another list, or dp - sp >= 2 (unsigned)     swap: intra dp > sp, inter rank > k
    //       as x > y with   intra: x = dp - (change ? sp : 0), y = change ? 1 : sp     inter: x = change ? ~0 : rank, y = change ? 0 : k
    //   v1  change only: dp + 1 == len2 and (another list or len != sp + 1), as one word that is zero exactly then
    const uint32_t sev = half(seA, seB), spv = half(spA, spB);
    mv0 = (sev << 16) | spv;
    tl = half(tlA, tlB);
    Kh = half(K0, K1);
    rq_off = hm & (cv.rc * 2u);
    // (every arm of a select below is a value already computed: a `?:` with work in an arm is compiled as an exec-mask region)
    const bool some = slot != NODE_NONE;
    const uint32_t r_any = slot >> 16, dp = slot & 0xFFFFu;
    const uint32_t r2 = some ? r_any : 0u;
    const uint32_t len2 = s_off[r2 + 1] - s_off[r2];
    uint32_t t;
    if constexpr (ARANK)
        t = RouteArith{half(perm_st0, perm_st1), half(perm_inv0, perm_inv1), (uint32_t)V, v_recip32}.word(r2);
    else
        t = rtab[r2 + (hm & (uint32_t)V)];
    const bool intra = r2 == sev;
    const uint32_t end_pay = (r2 << 16) | len2;
    const uint32_t xi = dp - (spv & ~hm), yi = half(1u, spv);
    const uint32_t xo = RT::rank(t) | ~hm, yo = kB & hm;
    const uint32_t xs = intra ? xi : xo, ys = intra ? yi : yo;
    const bool v0 = xs > ys;
    const uint32_t last = lenA ^ (spv + 1u);  // zero: the source is the last element of its list
    const uint32_t f = intra ? last : 1u;
    const uint32_t z1 = (((dp + 1u) ^ len2) | hm) | (1u - min(f, 1u));
    const bool v1 = z1 == 0u;
    const uint32_t b0 = v0 ? 1u : 0u, b1 = v1 ? 1u : 0u;
    const uint32_t wsum = b0 + b1;
    it.w = some ? wsum : 0u;
    const uint32_t len_or_dp = half(lenA, dp), ord_intra = v0 ? dp : len_or_dp, ord_inter = RT::inter_ord(t, dp);
    it.ord = intra ? ord_intra : ord_inter;
    const uint32_t end_or_slot = half(end_pay, slot);
    it.pay0 = v0 ? slot : end_or_slot;
    it.pay1 = end_pay;
} else {
    const uint32_t se = hi ? seB : seA, sp = hi ? spB : spA, len = hi ? lenB : lenA, kk = hi ? kB : kA;
    mv0 = (se << 16) | sp;
    tl = hi ? tlB : tlA;
    Kh = hi ? K1 : K0;
    rq_off = hi ? cv.rc * 2u : 0u;
    RT rth;
    if constexpr (ARANK)
        rth = RouteArith{hi ? perm_st1 : perm_st0, hi ? perm_inv1 : perm_inv0, (uint32_t)V, v_recip32};
    else
        rth = RT{rtab + (hi ? V : 0)};
    if constexpr (FAST) {
        // leaf 0 = nearby change (lanes 0-31), leaf 1 = nearby swap (lanes 32-63): the two items of nearby_item_rt written as ONE, the
        // facts they share read once and the half a lane belongs to folded into the predicates (nearby_change.rs:133-195, nearby_swap.rs)
        const bool some = slot != NODE_NONE;
        const uint32_t r2 = some ? slot >> 16 : 0u, dp = slot & 0xFFFFu;
        const uint32_t len2 = s_off[r2 + 1] - s_off[r2];
        const uint32_t t = rth.word(r2);
        const bool intra = r2 == se;
        const uint32_t end_pay = (r2 << 16) | len2;
        // change: the slot itself unless it is the source's own or the one behind it (dp - sp is 0 or 1, unsigned); swap: a later position of
        // the source's list, or a list ranked after it
        const bool v0 = hi ? (intra ? dp > sp : RT::rank(t) > kk) : (!intra || dp - sp >= 2u);
        const bool v1 = !hi && dp + 1 == len2 && (!intra || len != sp + 1);  // change only: the end slot `len` probes element len - 1
        it.w = some ? (uint32_t)v0 + (uint32_t)v1 : 0u;
        it.ord = intra ? ((hi || v0) ? dp : len) : RT::inter_ord(t, dp);
        it.pay0 = (hi || v0) ? slot : end_pay;
        it.pay1 = end_pay;
    } else {
        const NearbyItem ic = nearby_item_rt(true, slot, se, sp, len, kk, s_off, rth);
        const NearbyItem is = nearby_item_rt(false, slot, se, sp, len, kk, s_off, rth);
        const bool lane_change = hi ? chg1 : chg0;
        it.w = lane_change ? ic.w : is.w;
        it.ord = lane_change ? ic.ord : is.ord;
        it.pay0 = lane_change ? ic.pay0 : is.pay0;
        it.pay1 = lane_change ? ic.pay1 : is.pay1;
    }
}
const uint64_t havemask = SF_SPEC_ROW_HAVEMASK(__ballot(have));
// a group starts at the half's first lane and wherever the entry does not continue the previous one's distance.  LEAN: one compare,
// key < 0x8000 (no NBR_SAME_FLAG, not NBR_END) in general and key < NBR_END at the half's first lane
const uint64_t startmask = LEAN ? __ballot(key < NBR_END - min(l31, 1u) * (NBR_END - NBR_SAME_FLAG))
                                    : __ballot(have && (l31 == 0 || !(key & NBR_SAME_FLAG)));
const uint32_t hvA = (uint32_t)havemask, hvB = (uint32_t)(havemask >> 32);
const uint32_t stA = (uint32_t)startmask, stB = (uint32_t)(startmask >> 32);
const bool moreA = hvA == 0xFFFFFFFFu && 32u < dim, moreB = hvB == 0xFFFFFFFFu && 32u < dim;
// complete groups of each half (a half whose only group is still open contributes nothing)
uint32_t ncA = 0, ncB = 0;
uint64_t closedmask;
bool closed;
if constexpr (LEAN) {
    // every lane works its own half's count out of its half's two words (vector instructions; the scalar form was ~30 instructions of
    // s_flbit / s_bcnt1 / s_cselect / s_lshl per pass) -- the compare IS the closed mask; ncA / ncB are formed only where gen_rest is called
    const uint32_t hvv = half(hvA, hvB), stv = half(stA, stB);
    const uint32_t ncv = (hvv == 0xFFFFFFFFu && 32u < dim) ? 31u - (uint32_t)__clz(stv) : (uint32_t)__popc(hvv);
    closed = l31 < ncv;
    closedmask = __ballot(closed);
} else {
    ncA = moreA ? 31u - (uint32_t)__clz(stA) : (uint32_t)__popc(hvA);
    ncB = moreB ? 31u - (uint32_t)__clz(stB) : (uint32_t)__popc(hvB);
    closedmask = (uint64_t)(ncA >= 32 ? 0xFFFFFFFFu : ((1u << ncA) - 1u)) |
                 ((uint64_t)(ncB >= 32 ? 0xFFFFFFFFu : ((1u << ncB) - 1u)) << 32);
    closed = (closedmask & lanebit) != 0;
}
const uint32_t wc = closed ? it.w : 0u;
const uint64_t w1 = __ballot(wc == 1), w2 = __ballot(wc == 2);
const uint32_t WcA = (uint32_t)__popc((uint32_t)w1) + 2u * (uint32_t)__popc((uint32_t)w2);
const uint32_t WcB = (uint32_t)__popc((uint32_t)(w1 >> 32)) + 2u * (uint32_t)__popc((uint32_t)(w2 >> 32));
if (WcA + WcB > 0) {
    const uint32_t pa = __builtin_amdgcn_mbcnt_lo((uint32_t)w1, 0u) + 2u * __builtin_amdgcn_mbcnt_lo((uint32_t)w2, 0u);
    const uint32_t pb = __builtin_amdgcn_mbcnt_hi((uint32_t)(w1 >> 32), 0u) + 2u * __builtin_amdgcn_mbcnt_hi((uint32_t)(w2 >> 32), 0u);
    int32_t pos = (int32_t)(LEAN ? half(pa, pb) : (hi ? pb : pa));
    const uint64_t nonstart = SF_SPEC_TIES(~startmask & closedmask);  // never crosses lane 32 (forced start)
#ifdef SF_SPEC_TIE_KEY
    static_assert(!std::is_same<RT, RouteTab>::value, "SF_SPEC_TIE_KEY: the (rank, position) ordinals");
    if (nonstart) pos += tie_key_fix(startmask, nonstart, it.ord, wc);
#else
    if (nonstart) {
        const uint32_t packed = (it.ord << 2) | wc;
        uint64_t run = nonstart;
        uint32_t p_dn = packed, p_up = packed;
        for (uint32_t d = 1; run != 0; ++d) {
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
    uint32_t* rq = ring + rq_off;
    if (wc >= 1 && (uint32_t)pos < Kh) {
        const uint32_t qi = (tl + (uint32_t)pos) & RCM;
        rq[qi * 2] = mv0;
        rq[qi * 2 + 1] = it.pay0;
    }
    if (wc == 2 && (uint32_t)pos + 1 < Kh) {
        const uint32_t qi = (tl + (uint32_t)pos + 1) & RCM;
        rq[qi * 2] = mv0;
        rq[qi * 2 + 1] = it.pay1;
    }
}
uint32_t emA = WcA < K0 ? WcA : K0, emB = WcB < K1 ? WcB : K1;
if (emA < K0 && moreA) {  // rare: leaf 0's source needs entries beyond its half
    GC(3)
    ISA_MARK("pair_rest_begin");
    if constexpr (LEAN) ncA = 31u - (uint32_t)__clz(stA);  // (moreA)
    const uint32_t jj = ncA + lane;
    emA = gen_rest(0, seA, spA, lenA, kA, sxA, tlA, jj < dim ? (uint32_t)nb.keys[(size_t)sxA * dim + jj] : NBR_END, ncA, K0 - emA, emA);
    ISA_MARK("pair_rest_end");
}
if (emB < K1 && moreB) {
    GC(4)
    ISA_MARK("pair_rest_begin");
    if constexpr (LEAN) ncB = 31u - (uint32_t)__clz(stB);  // (moreB)
    const uint32_t jj = ncB + lane;
    emB = gen_rest(1, seB, spB, lenB, kB, sxB, tlB, jj < dim ? (uint32_t)nb.keys[(size_t)sxB * dim + jj] : NBR_END, ncB, K1 - emB, emB);
    ISA_MARK("pair_rest_end");
}
