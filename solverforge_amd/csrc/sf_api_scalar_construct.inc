// Scalar construction surface of the C ABI: sf_construct_scalar, the reference's ConstructionHeuristicPhase over one scalar variable on every
// replica's current values (kernel: csrc/sf_scalar_construct.hip, a translation unit of its own).  The host validates, sorts the entity order
// once (stable, by the entity key), builds the value order of AllocateToValueFromQueue, launches, and commits the score like the list
// constructions do.  Device buffers of the call are Scratch (sf_api.hip).  Included into sf_api.hip (same translation unit).

extern "C" {

int32_t sf_construct_scalar(sf_ctx* ctx, int32_t descriptor_index, int32_t variable_index, const sf_scalar_construction_config* cfg,
                            const int64_t* entity_order_keys, const int64_t* value_order_keys, int64_t* out_scores) {
    if (!ctx) return sf_device_count() > 0 ? SF_ERR_INVALID : SF_ERR_NO_DEVICE;  // no context can exist without a device, and nothing runs on the CPU
    DeviceGuard _dev(ctx);
    if (ctx->xown_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "sf_construct_scalar: a model with the join of its two planning classes is searched by the fused engine only");
    if (!ctx->initialized) return fail(ctx, SF_ERR_INVALID, "sf_initialize first");
    if (!ctx->has_scalar_model || descriptor_index != ctx->scalar_desc || variable_index != ctx->classes[descriptor_index].var_index)
        return fail(ctx, SF_ERR_INVALID, "scalar construction needs the scalar variable's class and variable");
    if (!cfg) return fail(ctx, SF_ERR_INVALID, "sf_construct_scalar: cfg is NULL");
    const int32_t h = cfg->heuristic;
    if (h < SF_CH_FIRST_FIT || h > SF_CH_ALLOCATE_TO_VALUE_FROM_QUEUE) return fail(ctx, SF_ERR_INVALID, "sf_construct_scalar: heuristic is no sf_construction_heuristic");
    if (cfg->obligation != SF_CO_PRESERVE_UNASSIGNED && cfg->obligation != SF_CO_ASSIGN_WHEN_CANDIDATE_EXISTS)
        return fail(ctx, SF_ERR_INVALID, "sf_construct_scalar: obligation is no sf_construction_obligation");
    if (cfg->value_candidate_limit < 0) return fail(ctx, SF_ERR_INVALID, "sf_construct_scalar: value_candidate_limit must be >= 0 (0 = none)");
    if (cfg->reserved & ~1) return fail(ctx, SF_ERR_INVALID, "sf_construct_scalar: reserved bits set");
    if (cfg->reserved & 1) return fail(ctx, SF_ERR_UNSUPPORTED, "sf_construct_scalar: value order keys that depend on the entity are not built");
    const bool entity_desc = h == SF_CH_FIRST_FIT_DECREASING || h == SF_CH_WEAKEST_FIT_DECREASING || h == SF_CH_STRONGEST_FIT_DECREASING;
    const bool entity_asc = h == SF_CH_ALLOCATE_ENTITY_FROM_QUEUE;
    const bool strength = h == SF_CH_WEAKEST_FIT || h == SF_CH_WEAKEST_FIT_DECREASING || h == SF_CH_STRONGEST_FIT || h == SF_CH_STRONGEST_FIT_DECREASING;
    const bool value_queue = h == SF_CH_ALLOCATE_TO_VALUE_FROM_QUEUE;
    if ((entity_desc || entity_asc) && !entity_order_keys) return fail(ctx, SF_ERR_INVALID, "sf_construct_scalar: the heuristic needs entity_order_keys (construction_entity_order_key)");
    if ((strength || value_queue) && !value_order_keys) return fail(ctx, SF_ERR_INVALID, "sf_construct_scalar: the heuristic needs value_order_keys (construction_value_order_key)");
    int rc;
    if ((rc = alloc_search(ctx))) return rc;
    const ScalarModel& m = ctx->sm;
    const ClassSpec& c = ctx->classes[descriptor_index];
    const size_t lds = scalar_table_bytes(ctx);
    if (lds > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "the per-value tables of the scalar class do not fit one wave's LDS slice");

    ScalarConstructArgs a{};
    a.n_order = m.n;
    a.forager = h == SF_CH_CHEAPEST_INSERTION ? SCF_BEST_FIT
                : (h == SF_CH_WEAKEST_FIT || h == SF_CH_WEAKEST_FIT_DECREASING)     ? SCF_WEAKEST_FIT
                : (h == SF_CH_STRONGEST_FIT || h == SF_CH_STRONGEST_FIT_DECREASING) ? SCF_STRONGEST_FIT
                                                                                    : SCF_FIRST_FIT;
    a.baseline = (m.allows_unassigned && cfg->obligation == SF_CO_PRESERVE_UNASSIGNED) ? 1 : 0;  // keep_current_allowed (decision.rs:145-154)
    a.live_refresh = (h != SF_CH_FIRST_FIT && h != SF_CH_CHEAPEST_INSERTION) ? 1 : 0;             // requires_live_refresh (placement.rs:136-147)
    a.limit = cfg->value_candidate_limit > 0 ? (uint32_t)cfg->value_candidate_limit : 0xFFFFFFFFu;
    a.range_n = (int32_t)std::min<uint32_t>((uint32_t)m.n_values, a.limit);
    a.c_off = m.vl_off, a.c_val = m.vl;
    a.stats = ctx->sp.stats;

    Scratch<uint32_t> d_order, d_coff, d_kept;
    Scratch<int32_t> d_cval, d_perm;
    Scratch<int64_t> d_vkey;
    std::vector<uint32_t> order, coff;  // host buffers outlive the asynchronous uploads: the launch below synchronizes
    std::vector<int32_t> cval, perm;
    if ((entity_desc || entity_asc) && m.n > 0) {  // ordered_entity_indices (placement.rs:174-198): stable, ties by index
        order.resize((size_t)m.n);
        for (int32_t e = 0; e < m.n; ++e) order[(size_t)e] = (uint32_t)e;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            return entity_desc ? entity_order_keys[x] > entity_order_keys[y] : entity_order_keys[x] < entity_order_keys[y];
        });
        if ((rc = d_order.upload(ctx, order.data(), order.size()))) return rc;
        a.order = d_order.p;
    }
    if (value_queue) {  // ordered_values (placement.rs:200-227): the cut list, stable by the value key
        const auto by_key = [&](int32_t x, int32_t y) { return value_order_keys[x] < value_order_keys[y]; };
        if (!c.value_off.empty()) {
            coff.assign((size_t)m.n + 1, 0u);
            for (int32_t e = 0; e < m.n; ++e) {
                const uint32_t b = c.value_off[(size_t)e], len = std::min<uint32_t>(c.value_off[(size_t)e + 1] - b, a.limit);
                cval.insert(cval.end(), c.value_list.begin() + b, c.value_list.begin() + b + len);
                std::stable_sort(cval.end() - len, cval.end(), by_key);
                coff[(size_t)e + 1] = (uint32_t)cval.size();
            }
            if ((rc = d_coff.upload(ctx, coff.data(), coff.size())) || (rc = d_cval.upload(ctx, cval.data(), cval.size()))) return rc;
            a.c_off = d_coff.p, a.c_val = d_cval.p;
        } else {
            perm.resize((size_t)a.range_n);
            for (int32_t v = 0; v < a.range_n; ++v) perm[(size_t)v] = v;
            std::stable_sort(perm.begin(), perm.end(), by_key);
            if ((rc = d_perm.upload(ctx, perm.data(), perm.size()))) return rc;
            a.perm = d_perm.p;
        }
    }
    if (strength) {
        if ((rc = d_vkey.upload(ctx, value_order_keys, (size_t)m.n_values))) return rc;
        a.vkey = d_vkey.p;
    }
    if (a.live_refresh && a.baseline && m.n > 0) {  // only then can an entity keep current and be reopened by a later assignment
        if ((rc = d_kept.alloc(ctx, (size_t)ctx->R * (size_t)m.n))) return rc;
        a.kept = d_kept.p;
    }
    hipError_t e = m.n > 0 ? launch_tu_scalar_construct(m, a, ctx->R, lds, ctx->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    return run_evaluate_all(ctx, out_scores, 1);  // the committed score of the constructed values
}

}  // extern "C"
