// TabuSearch on the host side (csrc/sf_tabu.h holds the rules): the policy (sf_solver_configure_tabu), the state row and the arena of every
// replica at phase start, what a launch under it may run, sf_get_tabu_state, and sf_debug_tabu_script -- the header's functions alone on a
// scripted sequence, one 64-lane wave.  Included into sf_api.hip (same translation unit, same build flags as the rest of the library).

static_assert(SF_TABU_STATE_FIXED == TB_WORDS && SF_TABU_MAX_TENURE_MOVE == TABU_MAX_TENURE_MOVE && SF_TABU_NO_TOKEN == TABU_NO_TOKEN,
              "include/solverforge_amd.h documents these");
static_assert(sizeof(sf_tabu_signature) == sizeof(TabuSig) && offsetof(sf_tabu_signature, move_id) == offsetof(TabuSig, mid) &&
                  offsetof(sf_tabu_signature, undo_move_id) == offsetof(TabuSig, uid) && offsetof(sf_tabu_signature, value) == offsetof(TabuSig, val),
              "sf_tabu_signature is TabuSig");
static_assert(sizeof(sf_tabu_record) == (SF_MAX_LEVELS + 64 * SF_MAX_LEVELS) * 8 + 64 * sizeof(sf_tabu_signature) + 16, "sf_tabu_record has no padding");

// normalize_tabu_search_policy (builder/acceptor.rs:383-405) + TabuSearchPolicy::validated (tabu_search.rs:32-62): tenures[4] (0 = absent)
// and the aspiration flag, or the reason the policy is refused.  cfg == nullptr: the default.
static int tabu_policy(sf_ctx* ctx, const sf_tabu_config* cfg, uint64_t tenure[4], int* aspire) {
    static const char* names[4] = {"entity_tabu_size", "value_tabu_size", "move_tabu_size", "undo_move_tabu_size"};
    const int64_t sizes[4] = {cfg ? cfg->entity_tabu_size : -1, cfg ? cfg->value_tabu_size : -1, cfg ? cfg->move_tabu_size : -1, cfg ? cfg->undo_move_tabu_size : -1};
    bool any = false;
    for (int q = 0; q < 4; ++q) {
        if (sizes[q] == 0) return fail(ctx, SF_ERR_INVALID, std::string("tabu_search field `") + names[q] + "` must be greater than 0");
        tenure[q] = sizes[q] > 0 ? (uint64_t)sizes[q] : 0;
        any = any || sizes[q] > 0;
    }
    if (!any) tenure[TB_MEM_MOVE] = 10;  // all four absent: TabuSearchPolicy::move_only(10)
    for (int q = TB_MEM_MOVE; q <= TB_MEM_UNDO; ++q)
        if (tenure[q] > TABU_MAX_TENURE_MOVE) return fail(ctx, SF_ERR_UNSUPPORTED, std::string("tabu search: ") + names[q] + " above 64 (the move and undo memories are rings of at most 64 identities)");
    *aspire = cfg ? (cfg->aspiration_enabled != 0) : 1;
    return SF_OK;
}

extern "C" int32_t sf_solver_configure_tabu(sf_ctx* ctx, const sf_tabu_config* cfg) {
    if (!ctx) return SF_ERR_INVALID;
    uint64_t tenure[4];
    int aspire;
    if (int rc = tabu_policy(ctx, cfg, tenure, &aspire)) return rc;
    for (int q = 0; q < 4; ++q) ctx->tabu_tenure[q] = tenure[q];
    ctx->tabu_aspire = aspire;
    ctx->tabu_configured = true;
    return SF_OK;
}

// The token tables of the context's model: one scope per declared planning variable, the scalar class first (sf_tabu.h: TabuScope).
static void tabu_token_counts(const sf_ctx* ctx, uint64_t* n_ent, uint64_t* n_val) {
    *n_ent = 0, *n_val = 0;
    if (ctx->has_scalar_model) *n_ent += (uint64_t)ctx->sm.n, *n_val += (uint64_t)ctx->sm.n_values + 1;  // + the None slot
    if (ctx->has_list_model) *n_ent += (uint64_t)ctx->lm.V, *n_val += (uint64_t)ctx->lm.dim + 1;  // routes; element ids below the node-id bound
}

// What a launch under TabuSearch can run: the sites that build signatures (DESIGN 25) -- the fused scalar engine, the wave engine's general
// replay and the generic engine, for the leaves whose signature has a fixed size.  nullptr, or the reason of the refusal.
static const char* tabu_launch_refusal(sf_ctx* ctx) {
    bool nearby_scalar = false;
    for (auto& s : ctx->selectors) {
        switch (s.kind) {
            case SF_SEL_SCALAR_CHANGE: case SF_SEL_SCALAR_SWAP: case SF_SEL_LIST_CHANGE: case SF_SEL_LIST_SWAP:
            case SF_SEL_NEARBY_LIST_CHANGE: case SF_SEL_NEARBY_LIST_SWAP: break;
            case SF_SEL_NEARBY_SCALAR_CHANGE: case SF_SEL_NEARBY_SCALAR_SWAP: nearby_scalar = true; break;
            default:
                return "tabu search: move signatures have a fixed size for scalar change / swap and list change / swap leaves (plain and nearby) only; "
                       "reverse, sublist, k-opt, ruin, permute and precedence leaves have variable-length or composite signatures";
        }
    }
    // (launch_search's routing) everything but the two-leaf nearby list union and the plain scalar union runs in the generic engine
    const bool generic = nearby_scalar || (ctx->has_list_model && ctx->has_scalar_model) || (ctx->has_list_model && has_plain_list_leaves(ctx)) ||
                         union_is_custom(ctx) || (ctx->has_list_model && ctx->pm.on);
    if (!generic && ctx->has_list_model && !use_wave_engine(ctx)) return "tabu search: the block engine builds no move signatures (wave and generic engines only)";
    return nullptr;
}

// sf_phase_start under TabuSearch: the rows' host words (tenures, flag, arena address, token counts) and an arena large enough for every
// replica; the phase-start kernels clear it and set best (tabu_phase_started).  `st` = the R rows about to be uploaded.
static int tabu_phase_rows(sf_ctx* ctx, std::vector<uint64_t>& st) {
    uint64_t n_ent, n_val;
    tabu_token_counts(ctx, &n_ent, &n_val);
    if (n_ent >= TABU_FIELD_LIMIT || n_val >= TABU_FIELD_LIMIT || (ctx->has_list_model && (uint64_t)ctx->lm.n_cap >= TABU_FIELD_LIMIT))
        return fail(ctx, SF_ERR_UNSUPPORTED, "tabu search: entity and value indices are 24-bit fields of a move identity");
    uint64_t row[SA_WORDS] = {};
    for (int q = 0; q < 4; ++q) row[TB_TENURE + q] = ctx->tabu_tenure[q];
    row[TB_ASPIRE] = (uint64_t)ctx->tabu_aspire;
    row[TB_NENT] = n_ent, row[TB_NVAL] = n_val;
    const uint64_t words = tabu_arena_offset(row, 4);
    const uint64_t total = words * (uint64_t)ctx->R;
    if (total > ctx->tabu_arena_cap) {
        if (ctx->d_tabu_arena) {  // release the smaller one (no launch is using it: calls on a ctx are not re-entrant)
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            for (auto it = ctx->allocs.begin(); it != ctx->allocs.end(); ++it)
                if (*it == (void*)ctx->d_tabu_arena) {
                    ctx->allocs.erase(it);
                    break;
                }
            (void)hipFree(ctx->d_tabu_arena);
            ctx->d_tabu_arena = nullptr;
            ctx->tabu_arena_cap = 0;
        }
        if (int rc = dalloc(ctx, &ctx->d_tabu_arena, (size_t)total)) return rc;
        ctx->tabu_arena_cap = total;
    }
    for (int r = 0; r < ctx->R; ++r) {
        row[TB_ARENA] = (uint64_t)(uintptr_t)(ctx->d_tabu_arena + (size_t)r * words);
        std::copy(row, row + SA_WORDS, st.data() + (size_t)r * SA_WORDS);
    }
    return SF_OK;
}

extern "C" int32_t sf_get_tabu_state(sf_ctx* ctx, int32_t replica, int64_t* out_best, uint64_t* out_pushes, int64_t cap_entity, uint32_t* out_entity,
                                     int64_t* out_n_entity, int64_t cap_value, uint32_t* out_value, int64_t* out_n_value, uint64_t* out_moves,
                                     int32_t* out_n_moves, uint64_t* out_undo, int32_t* out_n_undo) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->search_alloc || replica < 0 || replica >= ctx->R || !out_best || !out_pushes || cap_entity < 0 || cap_value < 0 ||
        (cap_entity && !out_entity) || (cap_value && !out_value) || !out_n_entity || !out_n_value || !out_moves || !out_n_moves || !out_undo || !out_n_undo)
        return fail(ctx, SF_ERR_INVALID, "bad sf_get_tabu_state");
    if (ctx->sp.acceptor != SF_ACCEPT_TABU_SEARCH) return fail(ctx, SF_ERR_INVALID, "sf_get_tabu_state: the phase was not started under TabuSearch");
    uint64_t row[SA_WORDS];
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(row, ctx->sp.sa.state + (size_t)replica * SA_WORDS, sizeof(row), hipMemcpyDeviceToHost));
    const uint64_t words = tabu_arena_offset(row, 4);
    std::vector<uint64_t> arena((size_t)words + 1);
    if (words) HIPCHK(ctx, hipMemcpy(arena.data(), (const void*)(uintptr_t)row[TB_ARENA], (size_t)words * 8, hipMemcpyDeviceToHost));
    for (int k = 0; k < SF_MAX_LEVELS; ++k) out_best[k] = (int64_t)row[TB_BEST + k];
    for (int q = 0; q < 4; ++q) out_pushes[q] = row[TB_NPUSH + q];
    for (int q = 0; q < 2; ++q) {  // the tokens whose latest push is among the last `tenure` pushes, ascending
        const uint64_t n = q ? row[TB_NVAL] : row[TB_NENT], tenure = row[TB_TENURE + q], npush = row[TB_NPUSH + q];
        const uint64_t* stamp = arena.data() + tabu_arena_offset(row, q);
        const int64_t cap = q ? cap_value : cap_entity;
        uint32_t* out = q ? out_value : out_entity;
        int64_t cnt = 0;
        if (tenure)
            for (uint64_t t = 0; t < n; ++t)
                if (stamp[t] != 0 && npush - stamp[t] < tenure) {
                    if (cnt < cap) out[cnt] = (uint32_t)t;
                    ++cnt;
                }
        *(q ? out_n_value : out_n_entity) = cnt;
    }
    for (int q = 2; q < 4; ++q) {  // oldest to newest
        const uint64_t tenure = row[TB_TENURE + q], npush = row[TB_NPUSH + q];
        const uint64_t* ring = arena.data() + tabu_arena_offset(row, q);
        uint64_t* out = q == TB_MEM_MOVE ? out_moves : out_undo;
        const uint64_t live = npush < tenure ? npush : tenure;
        for (uint64_t k = 0; k < live; ++k) {
            const uint64_t slot = npush <= tenure ? k : (npush + k) % tenure;
            out[2 * k] = ring[2 * slot], out[2 * k + 1] = ring[2 * slot + 1];
        }
        *(q == TB_MEM_MOVE ? out_n_moves : out_n_undo) = (int32_t)live;
    }
    return SF_OK;
}

namespace sf {

// one wave; records [n_records], out_accept [n_records], out_state [n_records][state_words]; row = one state row (SA_WORDS words) whose
// host words are set; the arena behind it holds n_ent + n_val stamps (where the memory has a tenure) and the two rings
template <int L>
__global__ __launch_bounds__(64) void k_debug_tabu_script(int levels, uint64_t* row, const sf_tabu_record* __restrict__ records, int32_t n_records,
                                                          uint32_t n_ent, uint32_t n_val, uint64_t* __restrict__ out_accept, uint64_t* __restrict__ out_state) {
    const uint32_t lane = threadIdx.x;
    const uint64_t state_words = (uint64_t)TB_WORDS + n_ent + n_val + 4 * TABU_MAX_TENURE_MOVE;
    for (int32_t i = 0; i < n_records; ++i) {
        const sf_tabu_record& rec = records[i];
        int64_t cur4[4];
        ScoreV<L> sc;
#pragma unroll
        for (int k = 0; k < 4; ++k) cur4[k] = k < levels ? rec.score[k] : 0;  // levels the score does not have stay zero, as in the engines
#pragma unroll
        for (int k = 0; k < L; ++k) sc.v[k] = k < levels ? rec.sc[lane][k] : 0;
        TabuSig sig;
        __builtin_memcpy(&sig, &rec.sig[lane], sizeof(sig));
        uint64_t accmask = 0;
        if (rec.op == SF_ACCEPTOR_OP_PHASE_STARTED) {
            tabu_phase_started(row, cur4, lane, 64u);
        } else if (rec.op == SF_ACCEPTOR_OP_DECIDE) {
            TabuStep<L> t;
            tabu_step_begin<L>(row, t);
            accmask = __ballot(tabu_accepts<L>(t, (rec.reach >> lane) & 1ULL, sc, sig));
        } else {
            TabuSig first;
            __builtin_memcpy(&first, &rec.sig[0], sizeof(first));
            tabu_step_ended<L>(row, lane == 0, cur4, rec.has_sig ? &first : nullptr);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) out_accept[i] = accmask;
        uint64_t* out = out_state + (size_t)i * state_words;
        const uint64_t* arena = (const uint64_t*)row[TB_ARENA];
        for (uint64_t w = lane; w < state_words; w += 64) {
            uint64_t v = 0;
            if (w < TB_WORDS) {
                v = w == TB_ARENA || w == TB_NENT || w == TB_NVAL ? 0 : row[w];
            } else if (w < (uint64_t)TB_WORDS + n_ent) {
                if (row[TB_TENURE + TB_MEM_ENTITY]) v = arena[tabu_arena_offset(row, TB_MEM_ENTITY) + (w - TB_WORDS)];
            } else if (w < (uint64_t)TB_WORDS + n_ent + n_val) {
                if (row[TB_TENURE + TB_MEM_VALUE]) v = arena[tabu_arena_offset(row, TB_MEM_VALUE) + (w - TB_WORDS - n_ent)];
            } else {
                const uint64_t x = w - TB_WORDS - n_ent - n_val;
                const int q = x < 2 * TABU_MAX_TENURE_MOVE ? TB_MEM_MOVE : TB_MEM_UNDO;
                const uint64_t y = x - (q == TB_MEM_UNDO ? 2 * TABU_MAX_TENURE_MOVE : 0);
                if (y < 2 * row[TB_TENURE + q]) v = arena[tabu_arena_offset(row, q) + y];
            }
            out[w] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

}  // namespace sf

extern "C" int32_t sf_debug_tabu_script(sf_ctx* ctx, const sf_tabu_config* policy, int32_t levels, int32_t n_entity_ids, int32_t n_value_ids,
                                        int32_t n_records, const sf_tabu_record* records, uint64_t* out_accept, uint64_t* out_state) {
    if (!ctx) return sf_device_count() > 0 ? SF_ERR_INVALID : SF_ERR_NO_DEVICE;
    DeviceGuard _dev(ctx);
    if (!records || !out_accept || !out_state) return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: null argument");
    uint64_t tenure[4];
    int aspire;
    if (int rc = tabu_policy(ctx, policy, tenure, &aspire)) return rc;
    if (levels < 1 || levels > SF_MAX_LEVELS) return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: levels in 1..4");
    if (n_entity_ids < 1 || n_entity_ids > 65536 || n_value_ids < 1 || n_value_ids > 65536)
        return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: n_entity_ids and n_value_ids in 1..65536");
    if (n_records < 1 || n_records > SF_ACCEPTOR_DEBUG_MAX_RECORDS) return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: n_records in 1..65536");
    for (int32_t i = 0; i < n_records; ++i) {
        const sf_tabu_record& rec = records[i];
        if (rec.op < SF_ACCEPTOR_OP_PHASE_STARTED || rec.op > SF_ACCEPTOR_OP_STEP_ENDED) return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: op in 0..2");
        const int n_sig = rec.op == SF_ACCEPTOR_OP_DECIDE ? 64 : (rec.op == SF_ACCEPTOR_OP_STEP_ENDED && rec.has_sig) ? 1 : 0;
        for (int l = 0; l < n_sig; ++l)  // the kernel indexes the stamp tables with these
            for (int k = 0; k < 2; ++k)
                if ((rec.sig[l].entity[k] != SF_TABU_NO_TOKEN && rec.sig[l].entity[k] >= (uint32_t)n_entity_ids) ||
                    (rec.sig[l].value[k] != SF_TABU_NO_TOKEN && rec.sig[l].value[k] >= (uint32_t)n_value_ids))
                    return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: a token outside its table");
    }
    if (records[0].op != SF_ACCEPTOR_OP_PHASE_STARTED) return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: the first record starts the phase");

    uint64_t row[SA_WORDS] = {};  // the row as sf_phase_start uploads it
    for (int q = 0; q < 4; ++q) row[TB_TENURE + q] = tenure[q];
    row[TB_ASPIRE] = (uint64_t)aspire;
    row[TB_NENT] = (uint64_t)n_entity_ids, row[TB_NVAL] = (uint64_t)n_value_ids;
    const size_t state_words = (size_t)TB_WORDS + n_entity_ids + n_value_ids + 4 * TABU_MAX_TENURE_MOVE;
    if ((uint64_t)n_records * state_words > ((uint64_t)1 << 27)) return fail(ctx, SF_ERR_INVALID, "sf_debug_tabu_script: more than 2^27 state words to return");
    Scratch<uint64_t> d_row, d_arena, d_accept, d_out;
    Scratch<sf_tabu_record> d_records;
    int rc;
    if ((rc = d_arena.alloc(ctx, (size_t)tabu_arena_offset(row, 4)))) return rc;
    row[TB_ARENA] = (uint64_t)(uintptr_t)d_arena.p;
    if ((rc = d_row.upload(ctx, row, SA_WORDS))) return rc;
    if ((rc = d_records.upload(ctx, records, (size_t)n_records))) return rc;
    if ((rc = d_accept.alloc(ctx, (size_t)n_records))) return rc;
    if ((rc = d_out.alloc(ctx, (size_t)n_records * state_words))) return rc;
    if (levels <= 2)  // the engines' rule for the score width they are built for
        k_debug_tabu_script<2><<<dim3(1), dim3(64), 0, ctx->stream>>>(levels, d_row.p, d_records.p, n_records, (uint32_t)n_entity_ids, (uint32_t)n_value_ids, d_accept.p, d_out.p);
    else
        k_debug_tabu_script<4><<<dim3(1), dim3(64), 0, ctx->stream>>>(levels, d_row.p, d_records.p, n_records, (uint32_t)n_entity_ids, (uint32_t)n_value_ids, d_accept.p, d_out.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_accept, d_accept.p, (size_t)n_records * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_state, d_out.p, (size_t)n_records * state_words * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SF_OK;
}
