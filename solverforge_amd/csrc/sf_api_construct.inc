// Construction surface of the C ABI: the list construction phases (cheapest insertion, regret insertion, round robin, Clarke-Wright),
// the route-local 2-opt phase and the route feasibility query with its time-window tables.  Each phase runs over every replica's current
// lists and ends with the committed score of the constructed lists (run_evaluate_all).  Device buffers of a call are Scratch
// (sf_api.hip).  Included into sf_api.hip (same translation unit).

extern "C" {

// What every construction phase checks first, in this order: `fn` is the entry point's name, `what` the phase as its refusals word it.
// (A phase without an element array passes NULL / 0.)
static int construct_preamble(sf_ctx* ctx, const char* fn, const char* what, int32_t descriptor_index, const uint32_t* elements, int32_t n) {
    if (ctx && ctx->xown_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, std::string(fn) + ": a model with the join of its two planning classes is searched by the fused engine only");
    if (!ctx || !ctx->initialized) return fail(ctx, SF_ERR_INVALID, "sf_initialize first");
    if (!ctx->has_list_model || descriptor_index != ctx->list_desc) return fail(ctx, SF_ERR_INVALID, std::string(what) + " needs the list variable's class");
    if (n < 0 || (n > 0 && !elements)) return fail(ctx, SF_ERR_INVALID, "bad " + std::string(fn) + " arguments");
    return SF_OK;
}
// ... and the gate that follows the checks of the phase's own arguments; n = the element count where the phase packs element indices too (0 otherwise)
static int construct_packs_16_bits(sf_ctx* ctx, int32_t n) {
    if (ctx->lm.n_cap > 65535 || ctx->lm.dim > 65536 || n > 65535) return fail(ctx, SF_ERR_UNSUPPORTED, "construction packs list elements in 16 bits");
    return SF_OK;
}

// The element array of a phase, scanned in source order (the first offence is the one reported): ids in range, no id twice (each phase words
// that refusal after its own source binding), owner hooks >= -1 where the phase takes them
static int check_elements(sf_ctx* ctx, const uint32_t* elements, int32_t n, const int32_t* owners, const char* duplicate) {
    std::vector<bool> seen((size_t)ctx->lm.dim, false);
    for (int32_t k = 0; k < n; ++k) {
        if (elements[k] >= (uint32_t)ctx->lm.dim) return fail(ctx, SF_ERR_INVALID, "element id out of range");
        if (seen[elements[k]]) return fail(ctx, SF_ERR_INVALID, duplicate);
        seen[elements[k]] = true;
        if (owners && owners[k] < -1) return fail(ctx, SF_ERR_INVALID, "owners[k]: -1 = unrestricted, otherwise the owner hook's value");
    }
    return SF_OK;
}

// The elements a phase places, in (construction order key, source index) order (execute.rs:81-88), beside their owner hooks (-1 = unrestricted).
// An element whose owner hook names no list has no candidate entity and is never placed (regret/mod.rs:104-114; OwnerRestriction::Invalid,
// list_placement.rs:66-67): dropped here
static void placed_elements(const sf_ctx* ctx, const uint32_t* elements, int32_t n, const int64_t* order_keys, const int32_t* owners, std::vector<uint32_t>& el,
                            std::vector<int32_t>& ow) {
    std::vector<int32_t> order;
    for (int32_t k = 0; k < n; ++k)
        if (!owners || owners[k] < ctx->lm.V) order.push_back(k);
    if (order_keys) std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return order_keys[a] < order_keys[b]; });
    el.resize(order.size());
    ow.assign(order.size(), -1);
    for (size_t k = 0; k < order.size(); ++k) {
        el[k] = elements[order[k]];
        if (owners) ow[k] = owners[order[k]];
    }
}

// cheapest insertion on a list class scored by the precedence constraint (k_prec_construct_cheapest); with the slot's precedence policy
// the phase has the hooks and re-ranks the elements by their downstream chain (cheapest/kernel.rs:75-81,162-229)
static int construct_cheapest_precedence(sf_ctx* ctx, const uint32_t* elements, int32_t n, int64_t* out_scores) {
    if (ctx->lm.dist_level >= 0 || ctx->lm.cap_level >= 0)
        return fail(ctx, SF_ERR_UNSUPPORTED, "cheapest insertion on a precedence model with distance / capacity constraints");
    if (int rc = ensure_plf(ctx)) return rc;
    std::vector<uint32_t> order(elements, elements + n);
    const PrecSpec& ps = ctx->prec;
    const size_t nodes = ps.dur.size();
    if (ctx->prec_policy && n > 0) {  // precedence_downstream: unassigned elements only (those already in a list are skipped by the kernel anyway)
        std::vector<char> in_list(nodes, 0);
        {
            std::vector<uint32_t> off((size_t)ctx->lm.V + 1), vis;
            if (hipMemcpy(off.data(), ctx->lm.off, off.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, SF_ERR_HIP, "copy of the list offsets");
            vis.resize(off.back());
            if (!vis.empty() && hipMemcpy(vis.data(), ctx->lm.visits, vis.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
                return fail(ctx, SF_ERR_HIP, "copy of the lists");
            for (uint32_t x : vis)
                if (x < nodes) in_list[x] = 1;
        }
        std::vector<uint32_t> el;
        for (uint32_t x : order)
            if (x < nodes && !in_list[x]) el.push_back(x);
        const size_t m = el.size();
        std::vector<int64_t> position(nodes, -1);
        bool ok = true;
        for (size_t i = 0; i < m; ++i) position[el[i]] = (int64_t)i;
        std::vector<std::vector<size_t>> succ(m);
        std::vector<size_t> preds(m, 0);
        for (size_t i = 0; i < m; ++i)
            for (uint32_t t = ps.succ_off[el[i]]; t < ps.succ_off[el[i] + 1]; ++t) {
                const uint32_t to = ps.succ[t];
                if (to >= nodes || position[to] < 0) continue;
                succ[i].push_back((size_t)position[to]);
                preds[(size_t)position[to]] += 1;
            }
        std::vector<size_t> ready, topo;
        for (size_t i = 0; i < m; ++i)
            if (preds[i] == 0) ready.push_back(i);
        while (!ready.empty()) {
            const size_t i = ready.back();
            ready.pop_back();
            topo.push_back(i);
            for (size_t s2 : succ[i])
                if (--preds[s2] == 0) ready.push_back(s2);
        }
        ok = topo.size() == m;
        if (ok) {
            std::vector<int64_t> down(m);
            for (size_t t = m; t-- > 0;) {
                const size_t i = topo[t];
                int64_t tail = 0;
                for (size_t s2 : succ[i]) tail = std::max(tail, down[s2]);
                down[i] = (int64_t)ps.dur[el[i]] + tail;
            }
            std::vector<size_t> idx(m);
            for (size_t i = 0; i < m; ++i) idx[i] = i;
            std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return down[a] > down[b]; });
            order.clear();
            for (size_t i : idx) order.push_back(el[i]);
        }
    }
    const size_t lds = (((size_t)ctx->lm.V + 1 + 3) & ~(size_t)3) * 4 + ((((size_t)ctx->lm.dim + 31) / 32 + 3) & ~(size_t)3) * 4 + (size_t)ctx->lm.n_cap * 2 + 16;
    if (lds > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "list class does not fit one wave's LDS slice");
    Scratch<uint32_t> d_el;  // stays NULL without elements
    int rc;
    if (!order.empty() && (rc = d_el.upload(ctx, order.data(), order.size()))) return rc;
    hipError_t e = launch_with_lds(k_prec_construct_cheapest, dim3(ctx->R), dim3(64), lds, ctx->stream, ctx->lm, ctx->pm, ctx->plf, d_el.p, (int)order.size(),
                                   prec_level_order(ctx), ctx->sp.stats);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    return run_evaluate_all(ctx, out_scores, 1);
}

// ≙ ListCheapestInsertionPhase over every replica's current lists (csrc/sf_construct.hip)
int32_t sf_construct_list_cheapest(sf_ctx* ctx, int32_t descriptor_index, const uint32_t* elements, int32_t n, int64_t* out_scores) {
    DeviceGuard _dev(ctx);
    int rc;
    if ((rc = construct_preamble(ctx, "sf_construct_list_cheapest", "cheapest insertion", descriptor_index, elements, n)) || (rc = construct_packs_16_bits(ctx, 0))) return rc;
    for (int32_t k = 0; k < n; ++k)
        if (elements[k] >= (uint32_t)ctx->lm.dim) return fail(ctx, SF_ERR_INVALID, "element id out of range");
    if ((rc = alloc_search(ctx))) return rc;
    if (ctx->pm.on) return construct_cheapest_precedence(ctx, elements, n, out_scores);
    const ConstructCarve cv(ctx->lm.V, ctx->lm.n_cap, ctx->lm.dim);
    if (cv.total > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "list class does not fit one wave's LDS slice");
    Scratch<uint32_t> d_el;  // stays NULL without elements
    if (n > 0 && (rc = d_el.upload(ctx, elements, (size_t)n))) return rc;
    const auto kern = ctx->levels <= 2 ? k_list_construct_cheapest<2> : k_list_construct_cheapest<4>;
    hipError_t e = launch_with_lds(kern, dim3(ctx->R), dim3(64), cv.total, ctx->stream, ctx->lm, d_el.p, n, ctx->sp.stats);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    return run_evaluate_all(ctx, out_scores, 1);  // finish_construction: the committed score of the constructed lists
}

// ≙ ListRegretInsertionPhase over every replica's current lists (csrc/sf_construct.hip)
int32_t sf_construct_list_regret(sf_ctx* ctx, int32_t descriptor_index, const uint32_t* elements, int32_t n, const int64_t* order_keys,
                                 const int32_t* owners, int64_t* out_scores) {
    DeviceGuard _dev(ctx);
    int rc;
    if ((rc = construct_preamble(ctx, "sf_construct_list_regret", "regret insertion", descriptor_index, elements, n)) || (rc = construct_packs_16_bits(ctx, n))) return rc;
    if (ctx->pm.on) return fail(ctx, SF_ERR_UNSUPPORTED, "regret insertion on a model with precedence hooks");
    if ((rc = check_elements(ctx, elements, n, owners, "duplicate element id (the source binding of the phase refuses it, regret.rs:228-236)"))) return rc;
    if ((rc = alloc_search(ctx))) return rc;
    std::vector<uint32_t> el;
    std::vector<int32_t> ow;
    placed_elements(ctx, elements, n, order_keys, owners, el, ow);
    const int32_t ne = (int32_t)el.size();
    if (owners) {  // kernel/fallback.rs:58-84: all-fixed-owner inputs above the trial budget take bounded fallbacks that are not built.  The
        // budget is checked on the fixed-owner elements handed over (a replica's unassigned subset can only be smaller)
        std::vector<uint64_t> bucket((size_t)(ctx->lm.V > 0 ? ctx->lm.V : 1), 0);
        for (int32_t o : ow)
            if (o >= 0) bucket[o] += 1;
        uint64_t trials = 0;
        for (uint64_t len : bucket) trials += len * (len + 1) * (len + 2) / 6;
        if (trials > 16384) return fail(ctx, SF_ERR_UNSUPPORTED, "owner-restricted regret insertion above the reference's trial budget (regret/kernel/fallback.rs)");
    }
    const RegretCarve cv(ctx->lm.V, ctx->lm.n_cap, ctx->lm.dim, ne);
    if (cv.total > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "list class does not fit one wave's LDS slice");
    Scratch<uint32_t> d_el;  // both stay NULL without elements
    Scratch<int32_t> d_ow;
    if (ne > 0 && ((rc = d_el.upload(ctx, el.data(), (size_t)ne)) || (rc = d_ow.upload(ctx, ow.data(), (size_t)ne)))) return rc;
    const auto kern = ctx->levels <= 2 ? k_list_construct_regret<2> : k_list_construct_regret<4>;
    hipError_t e = launch_with_lds(kern, dim3(ctx->R), dim3(64), cv.total, ctx->stream, ctx->lm, d_el.p, owners ? d_ow.p : (const int32_t*)nullptr, ne, ctx->sp.stats);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    return run_evaluate_all(ctx, out_scores, 1);  // the committed score of the constructed lists
}

// ≙ ListKOptPhase (route-local 2-opt) over every replica's current lists (csrc/sf_clarke_wright.hip)
int32_t sf_construct_list_k_opt(sf_ctx* ctx, int32_t descriptor_index, int32_t k, int32_t feasible_mode, int32_t max_sweeps, int64_t* out_scores) {
    DeviceGuard _dev(ctx);
    int rc;
    if ((rc = construct_preamble(ctx, "sf_construct_list_k_opt", "list k-opt", descriptor_index, nullptr, 0))) return rc;
    if (feasible_mode < 0 || feasible_mode > 2) return fail(ctx, SF_ERR_INVALID, "feasible_mode: 0 no feasibility hook, 1 capacity, 2 capacity + time windows");
    if (max_sweeps < 1) return fail(ctx, SF_ERR_INVALID, "max_sweeps must be >= 1 (the termination policy of the phase)");
    if ((rc = construct_packs_16_bits(ctx, 0))) return rc;
    if (ctx->pm.on) return fail(ctx, SF_ERR_UNSUPPORTED, "list k-opt on a model with precedence hooks");
    if (!ctx->lm.mat) return fail(ctx, SF_ERR_UNSUPPORTED, "list k-opt needs the distance matrix (route_distance)");
    if (feasible_mode >= 1 && !ctx->lm.demand) return fail(ctx, SF_ERR_INVALID, "capacity feasibility needs the demand column");
    if (feasible_mode == 2 && !ctx->tw.uploaded) return fail(ctx, SF_ERR_INVALID, "feasible_mode 2 needs the time windows (sf_list_set_time_windows)");
    if ((rc = alloc_search(ctx))) return rc;
    if (k == 2 && ctx->lm.V > 0) {  // only k = 2 is implemented by the reference: every other value is a scored no-op (kernel.rs:69-77)
        const size_t lds = align_up((size_t)ctx->lm.n_cap * 2, 16) + 16;
        if (lds > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "a route does not fit one wave's LDS slice");
        const dim3 grid((unsigned)ctx->lm.V, (unsigned)ctx->R);
        // the complete hook is a kernel of its own (sf_kopt_tw.hip); modes 0 / 1 launch the instantiation they always did
        hipError_t e = feasible_mode == 2 ? launch_with_lds(k_list_construct_two_opt_tw, grid, dim3(64), lds, ctx->stream, ctx->lm, tw_tables(ctx), max_sweeps, ctx->sp.stats)
                                          : launch_with_lds(k_list_construct_two_opt, grid, dim3(64), lds, ctx->stream, ctx->lm, feasible_mode, max_sweeps, ctx->sp.stats);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if ((rc = hip_rc(ctx, e))) return rc;
    }
    return run_evaluate_all(ctx, out_scores, 1);
}

// ≙ ProblemData{time_windows, service_durations, travel_times, vehicle_departure_time} (solverforge-cvrp problem_data.rs:20-23).  Values are
// data, never refused: what the reference's recurrence makes of them (infeasible routes) is what the device makes of them.
int32_t sf_list_set_time_windows(sf_ctx* ctx, int32_t descriptor_index, int32_t n_nodes, const int64_t* lo, const int64_t* hi, const int64_t* service,
                                 const int64_t* travel, int64_t departure) {
    DeviceGuard _dev(ctx);
    if (!ctx) return SF_ERR_INVALID;
    if (!ctx->classes.count(descriptor_index) || !ctx->classes[descriptor_index].has_list)
        return fail(ctx, SF_ERR_INVALID, "sf_list_set_time_windows: declare the list variable first");
    if (!lo || !hi || !service || !travel) return fail(ctx, SF_ERR_INVALID, "sf_list_set_time_windows: null array");
    const int32_t want = ctx->initialized ? ctx->lm.dim : ctx->classes[descriptor_index].element_bound;
    if (ctx->initialized ? n_nodes != want : n_nodes < want || n_nodes < 1)
        return fail(ctx, SF_ERR_INVALID, "sf_list_set_time_windows: n_nodes must equal the list variable's element id bound (the matrix dimension when a matrix is attached)");
    auto& tw = ctx->tw;
    const size_t n = (size_t)n_nodes;
    tw.lo.assign(lo, lo + n), tw.hi.assign(hi, hi + n), tw.service.assign(service, service + n), tw.travel.assign(travel, travel + n * n);
    tw.departure = departure, tw.n = n_nodes, tw.desc = descriptor_index, tw.set = true;
    return ctx->initialized ? tw_upload(ctx) : SF_OK;
}

// ≙ route_hooks::feasible (helpers.rs:109-119) on every replica's committed lists
int32_t sf_list_routes_feasible(sf_ctx* ctx, int32_t descriptor_index, int32_t feasible_mode, int32_t* out_flags) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->initialized) return fail(ctx, SF_ERR_INVALID, "sf_initialize first");
    if (!ctx->has_list_model || descriptor_index != ctx->list_desc) return fail(ctx, SF_ERR_INVALID, "sf_list_routes_feasible needs the list variable's class");
    if (!out_flags) return fail(ctx, SF_ERR_INVALID, "sf_list_routes_feasible: null argument");
    if (feasible_mode != 1 && feasible_mode != 2) return fail(ctx, SF_ERR_INVALID, "feasible_mode: 1 capacity, 2 capacity + time windows");
    if (!ctx->lm.demand) return fail(ctx, SF_ERR_INVALID, "capacity feasibility needs the demand column");
    if (feasible_mode == 2 && !ctx->tw.uploaded) return fail(ctx, SF_ERR_INVALID, "feasible_mode 2 needs the time windows (sf_list_set_time_windows)");
    if (ctx->lm.V == 0) return SF_OK;
    const size_t n = (size_t)ctx->R * ctx->lm.V;
    Scratch<int32_t> d_out;
    if (int rc = d_out.alloc(ctx, n)) return rc;
    hipLaunchKernelGGL(k_list_routes_feasible, dim3((unsigned)ctx->lm.V, (unsigned)ctx->R), dim3(64), 0, ctx->stream, ctx->lm, tw_tables(ctx), feasible_mode, d_out.p);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out_flags, d_out.p, n * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return hip_rc(ctx, e);
}

// Which evaluation of the time recurrence feasible_mode 2 takes.  A pure query: out_path 0 = no windows set, 1 = the checked lane-serial walk,
// 2 = the composed wave-wide fold (the host range check of the tables passed and the walk is not forced); out_last_ran = the path the last
// mode-2 kernel of this context reports having taken (written by the kernel itself), 0 = none has run since the tables were set.
int32_t sf_list_time_window_path(sf_ctx* ctx, int32_t descriptor_index, int32_t* out_path, int32_t* out_last_ran) {
    DeviceGuard _dev(ctx);
    if (!ctx || !ctx->initialized) return fail(ctx, SF_ERR_INVALID, "sf_initialize first");
    if (!ctx->has_list_model || descriptor_index != ctx->list_desc) return fail(ctx, SF_ERR_INVALID, "sf_list_time_window_path needs the list variable's class");
    if (out_path) *out_path = !ctx->tw.uploaded ? 0 : (ctx->tw.gate_ok && !ctx->tw.force_walk) ? 2 : 1;
    if (out_last_ran) {
        *out_last_ran = 0;
        if (ctx->tw.uploaded) {
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            HIPCHK(ctx, hipMemcpy(out_last_ran, ctx->tw.d_ran, 4, hipMemcpyDeviceToHost));
        }
    }
    return SF_OK;
}

// force_walk != 0: feasible_mode 2 takes the checked walk whatever the range check of the tables says; 0: it follows the range check again.
// (The composed fold cannot be forced: it is exact only on data the check admits.)  For measurements and tests; both paths give the reference's verdict.
int32_t sf_list_force_time_window_walk(sf_ctx* ctx, int32_t descriptor_index, int32_t force_walk) {
    if (!ctx || !ctx->initialized) return fail(ctx, SF_ERR_INVALID, "sf_initialize first");
    if (!ctx->has_list_model || descriptor_index != ctx->list_desc) return fail(ctx, SF_ERR_INVALID, "sf_list_force_time_window_walk needs the list variable's class");
    ctx->tw.force_walk = force_walk != 0;
    return SF_OK;
}

// ≙ ListConstructionPhase (round robin) over every replica's current lists (csrc/sf_construct.hip)
int32_t sf_construct_list_round_robin(sf_ctx* ctx, int32_t descriptor_index, const uint32_t* elements, int32_t n, const int64_t* order_keys,
                                      const int32_t* owners, int64_t* out_scores) {
    DeviceGuard _dev(ctx);
    int rc;
    if ((rc = construct_preamble(ctx, "sf_construct_list_round_robin", "round robin", descriptor_index, elements, n)) || (rc = construct_packs_16_bits(ctx, n))) return rc;
    if ((rc = check_elements(ctx, elements, n, owners, "duplicate element"))) return rc;
    std::vector<uint32_t> el;
    std::vector<int32_t> ow;
    placed_elements(ctx, elements, n, order_keys, owners, el, ow);
    const int ne = (int)el.size();
    if ((rc = alloc_search(ctx))) return rc;
    if (ne == 0 || ctx->lm.V == 0) return run_evaluate_all(ctx, out_scores, 1);
    const RoundRobinCarve cv(ctx->lm.V, ctx->lm.n_cap, ctx->lm.dim, ne);
    if (cv.total > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "list class does not fit one wave's LDS slice");
    Scratch<uint32_t> d_el;
    Scratch<int32_t> d_ow;
    if ((rc = d_el.upload(ctx, el.data(), (size_t)ne)) || (rc = d_ow.upload(ctx, ow.data(), (size_t)ne))) return rc;
    hipError_t e = launch_with_lds(k_list_construct_round_robin, dim3(ctx->R), dim3(64), cv.total, ctx->stream, ctx->lm, d_el.p, owners ? d_ow.p : (const int32_t*)nullptr, ne,
                                   ctx->sp.stats);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    return run_evaluate_all(ctx, out_scores, 1);
}

// ≙ ListClarkeWrightPhase over every replica's current lists with the stock CVRP hook bundle (csrc/sf_clarke_wright.hip)
int32_t sf_construct_list_clarke_wright(sf_ctx* ctx, int32_t descriptor_index, const uint32_t* elements, int32_t n, int32_t feasible_mode,
                                        int64_t* out_scores, int32_t* out_committed) {
    DeviceGuard _dev(ctx);
    int rc;
    if ((rc = construct_preamble(ctx, "sf_construct_list_clarke_wright", "Clarke-Wright", descriptor_index, elements, n))) return rc;
    if (feasible_mode != 0 && feasible_mode != 1) return fail(ctx, SF_ERR_INVALID, "feasible_mode: 0 structural, 1 capacity");
    if ((rc = construct_packs_16_bits(ctx, 0))) return rc;
    if (ctx->pm.on) return fail(ctx, SF_ERR_UNSUPPORTED, "Clarke-Wright on a model with precedence hooks");
    if (!ctx->lm.mat) return fail(ctx, SF_ERR_UNSUPPORTED, "Clarke-Wright needs the distance matrix (savings_distance)");
    if (feasible_mode == 1 && !ctx->lm.demand) return fail(ctx, SF_ERR_INVALID, "capacity feasibility needs the demand column");
    // declared elements in source order; a duplicate source key is a binding error in the reference (runtime_list_source.rs);
    // elements whose value is the depot of the available owners are not routed (kernel.rs:83-91)
    if ((rc = check_elements(ctx, elements, n, nullptr, "duplicate element"))) return rc;
    std::vector<uint32_t> el;
    for (int32_t k = 0; k < n; ++k)
        if ((int32_t)elements[k] != ctx->lm.depot) el.push_back(elements[k]);
    const int ne = (int)el.size();
    if (ne > 65535) return fail(ctx, SF_ERR_UNSUPPORTED, "Clarke-Wright: more than 65535 elements");
    if ((rc = alloc_search(ctx))) return rc;
    if (out_committed) std::fill(out_committed, out_committed + ctx->R, 0);
    if (ne == 0) return run_evaluate_all(ctx, out_scores, 1);
    const CwCarve cv(ctx->lm.V, ctx->lm.n_cap, ctx->lm.dim, ne);
    if (cv.total > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "route state does not fit one wave's LDS slice");
    int monotone = 1;
    if (ctx->lm.demand) {
        std::vector<int32_t> dem((size_t)ctx->lm.dim);
        if ((rc = hip_rc(ctx, hipMemcpy(dem.data(), ctx->lm.demand, dem.size() * 4, hipMemcpyDeviceToHost)))) return rc;
        for (uint32_t x : el)
            if (dem[x] < 0) monotone = 0;
    }
    if (feasible_mode == 0) monotone = 1;  // no load test: every rejection is permanent
    const uint64_t P = (uint64_t)ne * (uint64_t)(ne - 1) / 2;
    Scratch<uint32_t> d_el, d_v0, d_v1;  // the pair buffers stay NULL without pairs
    Scratch<int64_t> d_k0, d_k1;
    Scratch<int32_t> d_flag;
    Scratch<char> d_tmp;
    if ((rc = d_el.upload(ctx, el.data(), (size_t)ne)) || (rc = d_flag.alloc(ctx, (size_t)ctx->R))) return rc;
    if (P > 0) {
        if ((rc = d_k0.alloc(ctx, P)) || (rc = d_k1.alloc(ctx, P)) || (rc = d_v0.alloc(ctx, P)) || (rc = d_v1.alloc(ctx, P))) return rc;
        hipLaunchKernelGGL(k_cw_savings, dim3((unsigned)((ne + 255) / 256), (unsigned)ne), dim3(256), 0, ctx->stream, ctx->lm, d_el.p, ne, d_k0.p, d_v0.p);
        size_t tmp_bytes = 0;
        if ((rc = hip_rc(ctx, hipGetLastError())) ||
            (rc = hip_rc(ctx, rocprim::radix_sort_pairs_desc(nullptr, tmp_bytes, d_k0.p, d_k1.p, d_v0.p, d_v1.p, (size_t)P, 0, 64, ctx->stream))) ||
            (rc = d_tmp.alloc(ctx, tmp_bytes ? tmp_bytes : 16)) ||
            (rc = hip_rc(ctx, rocprim::radix_sort_pairs_desc(d_tmp.p, tmp_bytes, d_k0.p, d_k1.p, d_v0.p, d_v1.p, (size_t)P, 0, 64, ctx->stream))))
            return rc;
    }
    hipError_t e = launch_with_lds(k_cw_merge, dim3(ctx->R), dim3(64), cv.total, ctx->stream, ctx->lm, d_el.p, ne, d_v1.p, P, feasible_mode, monotone, d_flag.p, (uint64_t*)nullptr);
    if (e == hipSuccess && out_committed) e = hipMemcpyAsync(out_committed, d_flag.p, (size_t)ctx->R * 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if ((rc = hip_rc(ctx, e))) return rc;
    return run_evaluate_all(ctx, out_scores, 1);  // the committed score of the constructed lists
}

}  // extern "C"
