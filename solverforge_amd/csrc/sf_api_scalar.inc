// Scalar-model assembly: uploads the scalar planning variable, turns the declared predicate-join
// constraint into the symmetric partner CSR the kernels use, and launches the fused scalar search.

// Effective partner relation of `left.id < right.id && left.neighbors.contains(right.id)`
// (examples/scalar-graph-coloring/src/domain/graph_coloring.rs:33-38): {a, b} is a pair iff b is in
// neighbors(a) for the LOWER index a; duplicates inside a neighbour list do not double count.
static void partners_from_adjacency(int n, const std::vector<uint32_t>& off, const std::vector<uint32_t>& adj,
                                    std::vector<uint32_t>& poff, std::vector<uint32_t>& pn) {
    std::vector<std::vector<uint32_t>> lists((size_t)n);
    for (int a = 0; a < n; ++a) {
        std::vector<uint32_t> seen;
        for (uint32_t p = off[a]; p < off[a + 1]; ++p) {
            uint32_t b = adj[p];
            if ((int)b >= n || b <= (uint32_t)a) continue;
            bool dup = false;
            for (uint32_t s : seen) dup = dup || s == b;
            if (dup) continue;
            seen.push_back(b);
            lists[a].push_back(b);
            lists[b].push_back((uint32_t)a);
        }
    }
    poff.assign((size_t)n + 1, 0);
    pn.clear();
    for (int a = 0; a < n; ++a) {
        std::sort(lists[a].begin(), lists[a].end());
        poff[a] = (uint32_t)pn.size();
        pn.insert(pn.end(), lists[a].begin(), lists[a].end());
    }
    poff[n] = (uint32_t)pn.size();
}

// left.id < right.id && group[left] == group[right] (examples/mixed-job-shop/src/domain/job_shop_plan.rs:50-62)
static void partners_from_groups(int n, const std::vector<int32_t>& group, std::vector<uint32_t>& poff,
                                 std::vector<uint32_t>& pn) {
    std::map<int32_t, std::vector<uint32_t>> members;
    for (int e = 0; e < n; ++e) members[group[e]].push_back((uint32_t)e);
    poff.assign((size_t)n + 1, 0);
    pn.clear();
    for (int e = 0; e < n; ++e) {
        poff[e] = (uint32_t)pn.size();
        for (uint32_t o : members[group[e]])
            if (o != (uint32_t)e) pn.push_back(o);
    }
    poff[n] = (uint32_t)pn.size();
}

// Uni filters / weights as data (sf_constraint_add_uni_program): every program of the class is evaluated on the host for all (entity, value) pairs and
// folded -- with the class's SF_C_VALUE_COST matrix, if it has one -- into ONE cost matrix that the existing value-cost paths price (cost_weight = 1:
// scales and weights are folded in).  The components stay on the host for sf_evaluate_each's per-constraint rows.
static int compile_uni_programs(sf_ctx* ctx, int d, ScalarModel& m) {
    ctx->uni_components.clear();
    bool any = false;
    for (auto& cs : ctx->constraints) any = any || (cs.desc == d && cs.kind == SF_C_UNI_PROGRAM_);
    if (!any) return SF_OK;
    const size_t n = (size_t)m.n, nv = (size_t)m.n_values;
    if (n * nv > ((size_t)1 << 27)) return fail(ctx, SF_ERR_UNSUPPORTED, "uni programs: the (entity, value) table would exceed 2^27 entries");
    std::map<int, std::vector<int32_t>> cols;    // fact id -> host copy of an i32 column
    std::map<int, std::vector<int64_t>> tables;  // fact id -> host copy of an i64 matrix
    auto column = [&](int fact, size_t need, const std::vector<int32_t>*& out) -> int {
        if (!ctx->facts.count(fact) || ctx->facts[fact].type != 2 || (size_t)ctx->facts[fact].rows < need)
            return fail(ctx, SF_ERR_INVALID, "uni program: an operand needs an i32 column fact with one entry per entity / per value");
        if (!cols.count(fact)) {
            std::vector<int32_t> h((size_t)ctx->facts[fact].rows);
            HIPCHK(ctx, hipMemcpy(h.data(), ctx->facts[fact].d0, h.size() * 4, hipMemcpyDeviceToHost));
            cols[fact] = std::move(h);
        }
        out = &cols[fact];
        return SF_OK;
    };
    struct Operand {
        int lhs = 0;
        const std::vector<int32_t>*a = nullptr, *b = nullptr;
        const std::vector<int64_t>* t = nullptr;
        int64_t t_rows = 0, t_cols = 0;
    };
    auto bind = [&](int lhs, int f, int fb, int fc, Operand& op) -> int {
        op.lhs = lhs;
        int r = SF_OK;
        if (lhs == SF_UNI_ROW_COL) r = column(f, n, op.a);
        if (lhs == SF_UNI_VALUE_COL) r = column(f, nv, op.b);
        if (lhs == SF_UNI_COL_DIFF || lhs == SF_UNI_COL_ABSDIFF) {
            r = column(f, n, op.a);
            if (!r) r = column(fb, nv, op.b);
        }
        if (lhs == SF_UNI_TABLE) {
            if (!ctx->facts.count(fc) || ctx->facts[fc].type != 1) return fail(ctx, SF_ERR_INVALID, "uni program: the table operand needs an i64 matrix fact");
            Fact& tf = ctx->facts[fc];
            if (!tables.count(fc)) {
                std::vector<int64_t> h((size_t)tf.rows * tf.cols);
                HIPCHK(ctx, hipMemcpy(h.data(), tf.d0, h.size() * 8, hipMemcpyDeviceToHost));
                tables[fc] = std::move(h);
            }
            op.t = &tables[fc], op.t_rows = tf.rows, op.t_cols = tf.cols;
            if (f >= 0) r = column(f, n, op.a);
            if (!r && fb >= 0) r = column(fb, nv, op.b);
        }
        return r;
    };
    auto value_of = [&](const Operand& op, size_t a, size_t v, bool& ok) -> int64_t {
        switch (op.lhs) {
            case 0: return 1;
            case SF_UNI_ROW_COL: return (*op.a)[a];
            case SF_UNI_VALUE: return (int64_t)v;
            case SF_UNI_VALUE_COL: return (*op.b)[v];
            case SF_UNI_COL_DIFF: return (int64_t)(*op.a)[a] - (int64_t)(*op.b)[v];
            case SF_UNI_COL_ABSDIFF: {
                const int64_t x = (int64_t)(*op.a)[a] - (int64_t)(*op.b)[v];
                return x < 0 ? -x : x;
            }
            default: {  // SF_UNI_TABLE
                const int64_t rk = op.a ? (int64_t)(*op.a)[a] : (int64_t)a, ck = op.b ? (int64_t)(*op.b)[v] : (int64_t)v;
                if (rk < 0 || rk >= op.t_rows || ck < 0 || ck >= op.t_cols) {
                    ok = false;
                    return 0;
                }
                return (*op.t)[(size_t)rk * (size_t)op.t_cols + (size_t)ck];
            }
        }
    };
    int level[2] = {-1, -1};  // the class's value-cost components sit on at most two score levels: one folded matrix each (ScalarModel::cost / cost2)
    std::vector<int64_t> total[2];
    for (size_t ci = 0; ci < ctx->constraints.size(); ++ci) {
        ConstraintSpec& cs = ctx->constraints[ci];
        if (cs.desc != d || (cs.kind != SF_C_UNI_PROGRAM_ && cs.kind != SF_C_VALUE_COST)) continue;
        int slot = cs.level == level[0] ? 0 : (cs.level == level[1] ? 1 : (level[0] < 0 ? 0 : (level[1] < 0 ? 1 : -1)));
        if (slot < 0)
            return fail(ctx, SF_ERR_UNSUPPORTED, "uni programs and the value-cost join of one class fold into one matrix per score level: at most two levels");
        if (level[slot] < 0) level[slot] = cs.level, total[slot].assign(n * nv, 0);
        UniComponent uc;
        uc.constraint_index = ci;
        uc.cost.assign(n * nv, 0);
        uc.pass.assign(n * nv, 0);
        if (cs.kind == SF_C_VALUE_COST) {  // (validated by the caller: an i64 matrix [n][n_values])
            HIPCHK(ctx, hipMemcpy(uc.cost.data(), ctx->facts[cs.fact].d0, n * nv * 8, hipMemcpyDeviceToHost));
            for (size_t q = 0; q < n * nv; ++q) {
                uc.pass[q] = uc.cost[q] != 0;
                uc.cost[q] = (int64_t)((uint64_t)cs.weight * (uint64_t)uc.cost[q]);
            }
        } else {
            std::vector<Operand> lhs(cs.uterms.size());
            for (size_t t = 0; t < cs.uterms.size(); ++t)
                if (int r = bind(cs.uterms[t].lhs, cs.uterms[t].fact, cs.uterms[t].fact_b, cs.uterms[t].fact_c, lhs[t])) return r;
            Operand w;
            if (cs.uweight.lhs != 0)
                if (int r = bind(cs.uweight.lhs, cs.uweight.fact, cs.uweight.fact_b, cs.uweight.fact_c, w)) return r;
            bool keys_ok = true;
            for (size_t a = 0; a < n; ++a)
                for (size_t v = 0; v < nv; ++v) {
                    bool all = true, any_in_clause = false;
                    int clause = -1;
                    for (size_t t = 0; t < cs.uterms.size(); ++t) {
                        const sf_uni_term& ut = cs.uterms[t];
                        if (ut.clause != clause) {
                            all = all && (clause < 0 || any_in_clause);
                            any_in_clause = false;
                            clause = ut.clause;
                        }
                        const int64_t x = value_of(lhs[t], a, v, keys_ok);
                        const bool h = ut.cmp == SF_UNI_EQ ? x == ut.param : ut.cmp == SF_UNI_NE ? x != ut.param : ut.cmp == SF_UNI_LT ? x < ut.param
                                       : ut.cmp == SF_UNI_LE ? x <= ut.param : ut.cmp == SF_UNI_GT ? x > ut.param : x >= ut.param;
                        any_in_clause = any_in_clause || h;
                    }
                    all = all && (clause < 0 || any_in_clause);
                    if (!all) continue;
                    const int64_t wx = value_of(w, a, v, keys_ok);
                    uc.pass[a * nv + v] = 1;
                    uc.cost[a * nv + v] = (int64_t)((uint64_t)cs.weight * (uint64_t)(wx > 0 ? wx : 0));
                }
            if (!keys_ok) return fail(ctx, SF_ERR_INVALID, "uni program: a table key is out of range");
        }
        for (size_t q = 0; q < n * nv; ++q) total[slot][q] += uc.cost[q];
        ctx->uni_components.push_back(std::move(uc));
    }
    int64_t* d_cost = nullptr;
    if (int r = upload(ctx, &d_cost, total[0].data(), total[0].size())) return r;
    m.cost = d_cost;
    m.cost_level = level[0];
    m.cost_weight = 1;
    if (level[1] >= 0) {
        int64_t* d_cost2 = nullptr;
        if (int r = upload(ctx, &d_cost2, total[1].data(), total[1].size())) return r;
        m.cost2 = d_cost2;
        m.cost2_level = level[1];
    }
    return SF_OK;
}

// One predicate join of a scalar class (sf_constraint_add_pair_join, or one of the three presets) compiled into one join record: the program, the
// clause that drives the partner index (built on the host from a CSR or a group column), the residual program, and the specialised loop the
// kernels run for it, if one matches (SF_AMD_IR_INTERPRET=1: always interpret).
static int compile_pair_join(sf_ctx* ctx, int n, const ConstraintSpec& cs, PairJoin& j) {
    j = PairJoin{SC_NONE, cs.level, cs.weight, nullptr, nullptr, nullptr, nullptr, 0, 0};
    int rc;
    std::vector<sf_pair_term> prog = cs.terms;
    if (cs.kind == SF_C_CROSS_ADJACENT_EQUAL)
        prog = {{SF_PAIR_CSR_CONTAINS, 0, cs.fact, -1, 0}, {SF_PAIR_VALUE_EQ, 1, -1, -1, 0}};
    else if (cs.kind == SF_C_CROSS_GROUP_EQUAL)
        prog = {{SF_PAIR_COL_EQ, 0, cs.fact, -1, 0}, {SF_PAIR_VALUE_EQ, 1, -1, -1, 0}};
    else if (cs.kind == SF_C_CROSS_QUEENS)
        prog = {{SF_PAIR_COL_NE, 0, cs.fact, -1, 0}, {SF_PAIR_VALUE_EQ, 1, -1, -1, 0}, {SF_PAIR_VALUE_ABSDIFF_EQ_COL, 1, cs.fact, -1, 0}};
    // facts of every term
    auto col_fact = [&](int id) -> const int32_t* {
        if (!ctx->facts.count(id) || ctx->facts[id].type != 2 || ctx->facts[id].rows < n) return nullptr;
        return (const int32_t*)ctx->facts[id].d0;
    };
    for (auto& pt : prog) {
        if (pt.op == SF_PAIR_CSR_CONTAINS) {
            if (!ctx->facts.count(pt.fact) || ctx->facts[pt.fact].type != 4 || ctx->facts[pt.fact].rows != n)
                return fail(ctx, SF_ERR_INVALID, "pair join: CSR_CONTAINS needs a CSR fact with one row per entity");
        } else if (pt.op == SF_PAIR_TABLE_NONZERO) {
            if (!ctx->facts.count(pt.fact) || ctx->facts[pt.fact].type != 1 || !col_fact(pt.fact_b))
                return fail(ctx, SF_ERR_INVALID, "pair join: TABLE_NONZERO needs an i64 matrix and an i32 key column");
            std::vector<int32_t> key((size_t)n);
            HIPCHK(ctx, hipMemcpy(key.data(), col_fact(pt.fact_b), key.size() * 4, hipMemcpyDeviceToHost));
            for (int32_t k : key)
                if (k < 0 || k >= ctx->facts[pt.fact].rows || k >= ctx->facts[pt.fact].cols) return fail(ctx, SF_ERR_INVALID, "pair join: table key out of range");
        } else if (pt.op != SF_PAIR_VALUE_EQ && pt.op != SF_PAIR_VALUE_NE && pt.op != SF_PAIR_VALUE_ABSDIFF_LE) {
            if (!col_fact(pt.fact)) return fail(ctx, SF_ERR_INVALID, "pair join: the op needs an i32 column with one entry per entity");
        }
    }
    // the clause that drives the partner index: a clause of exactly one CSR_CONTAINS term, else of exactly one COL_EQ term
    std::map<int, int> clause_size;
    for (auto& pt : prog) clause_size[pt.clause] += 1;
    int driver = -1;
    for (int want : {(int)SF_PAIR_CSR_CONTAINS, (int)SF_PAIR_COL_EQ})
        for (size_t t = 0; t < prog.size() && driver < 0; ++t)
            if (prog[t].op == want && clause_size[prog[t].clause] == 1) driver = (int)t;
    if (driver >= 0) {
        std::vector<uint32_t> poff, pn;
        if (prog[(size_t)driver].op == SF_PAIR_CSR_CONTAINS) {
            Fact& f = ctx->facts[prog[(size_t)driver].fact];
            std::vector<uint32_t> off((size_t)n + 1), adj((size_t)f.cols);
            HIPCHK(ctx, hipMemcpy(off.data(), f.d0, off.size() * 4, hipMemcpyDeviceToHost));
            if (f.cols) HIPCHK(ctx, hipMemcpy(adj.data(), f.d1, adj.size() * 4, hipMemcpyDeviceToHost));
            partners_from_adjacency(n, off, adj, poff, pn);
        } else {
            std::vector<int32_t> group((size_t)n);
            HIPCHK(ctx, hipMemcpy(group.data(), col_fact(prog[(size_t)driver].fact), group.size() * 4, hipMemcpyDeviceToHost));
            partners_from_groups(n, group, poff, pn);
        }
        uint32_t *d_off = nullptr, *d_pn = nullptr;
        if ((rc = upload(ctx, &d_off, poff.data(), poff.size()))) return rc;
        if ((rc = upload(ctx, &d_pn, pn.data(), pn.size()))) return rc;
        j.pn_off = d_off;
        j.pn = d_pn;
    }
    std::vector<sf_pair_term> rest;
    for (size_t t = 0; t < prog.size(); ++t)
        if ((int)t != driver) rest.push_back(prog[t]);
    if ((int)rest.size() > SF_IR_MAX) return fail(ctx, SF_ERR_UNSUPPORTED, "pair join: more than six terms left after the partner index took its clause");
    // specialisations of the interpreter for the two programs of the reference's examples (SF_AMD_IR_INTERPRET=1: always interpret)
    const char* ie = std::getenv("SF_AMD_IR_INTERPRET");
    const bool interpret = ie && std::atoi(ie) != 0;
    const bool only_value_eq = rest.size() == 1 && rest[0].op == SF_PAIR_VALUE_EQ;
    const bool queens = driver < 0 && rest.size() == 3 && rest[0].op == SF_PAIR_COL_NE && rest[1].op == SF_PAIR_VALUE_EQ &&
                        rest[2].op == SF_PAIR_VALUE_ABSDIFF_EQ_COL && rest[1].clause == rest[2].clause && rest[0].clause != rest[1].clause &&
                        rest[0].fact == rest[2].fact;
    if (driver >= 0 && only_value_eq && !interpret) {
        j.kind = SC_PARTNERS_EQUAL;
    } else if (queens && !interpret) {
        j.col = col_fact(rest[0].fact);
        j.kind = SC_QUEENS;
    } else {
        std::vector<PairTerm> dev(rest.size());
        for (size_t t = 0; t < rest.size(); ++t) {
            const sf_pair_term& pt = rest[t];
            PairTerm& q = dev[t];
            q.op_clause = pt.op | (pt.clause << 8);
            q.cols = 0;
            q.param = pt.param;
            q.col = nullptr, q.coff = nullptr, q.cval = nullptr, q.table = nullptr;
            if (pt.op == SF_PAIR_CSR_CONTAINS) {
                q.coff = (const uint32_t*)ctx->facts[pt.fact].d0;
                q.cval = (const uint32_t*)ctx->facts[pt.fact].d1;
            } else if (pt.op == SF_PAIR_TABLE_NONZERO) {
                q.table = (const int64_t*)ctx->facts[pt.fact].d0;
                q.cols = ctx->facts[pt.fact].cols;
                q.col = col_fact(pt.fact_b);
            } else if (pt.fact >= 0) {
                q.col = col_fact(pt.fact);
            }
        }
        PairTerm* d_ir = nullptr;
        if ((rc = upload(ctx, &d_ir, dev.data(), dev.size()))) return rc;
        j.ir = d_ir;
        j.ir_n = (int32_t)dev.size();
        j.kind = driver >= 0 ? SC_IR_PARTNERS : SC_IR_DENSE;
    }
    return SF_OK;
}

static int build_scalar_model(sf_ctx* ctx, int d) {
    ClassSpec& c = ctx->classes[d];
    ScalarModel& m = ctx->sm;
    m = ScalarModel{};
    m.n = c.n_rows;
    m.n_values = c.n_values;
    m.allows_unassigned = c.allows_unassigned;
    m.levels = ctx->levels;
    m.descriptor = d;
    m.variable = c.var_index;
    if (m.n_values > 32767) return fail(ctx, SF_ERR_UNSUPPORTED, "scalar value range > 32767");
    for (int32_t v : c.scalar_init)
        if (v < -1 || v >= m.n_values) return fail(ctx, SF_ERR_INVALID, "initial scalar value out of range");
    int rc;
    std::vector<PairJoin> joins;  // the predicate joins of the class, in declaration order
    for (auto& cs : ctx->constraints) {
        if (cs.desc != d) continue;
        if (cs.kind == SF_C_UNI_UNASSIGNED) {
            m.un_level = cs.level;
            m.un_weight = cs.weight;
            if (cs.fact >= 0) {  // filter + per-entity weight as a column: 0 = the filter rejects the entity
                if (!ctx->facts.count(cs.fact) || ctx->facts[cs.fact].type != 2 || ctx->facts[cs.fact].rows < m.n)
                    return fail(ctx, SF_ERR_INVALID, "unassigned: the weight column needs one i32 per entity (or fact -1)");
                m.un_w = (const int32_t*)ctx->facts[cs.fact].d0;
            }
        } else if (cs.kind == SF_C_CROSS_ADJACENT_EQUAL || cs.kind == SF_C_CROSS_GROUP_EQUAL || cs.kind == SF_C_CROSS_QUEENS || cs.kind == SF_C_PAIR_JOIN_) {
            // One compile path for every predicate join: the three model-shaped kinds are PRESETS of the pair-predicate program
            // (include/solverforge_amd.h, sf_pair_term).
            if ((int)joins.size() >= SF_MAX_PAIR_JOINS) return fail(ctx, SF_ERR_UNSUPPORTED, "more than SF_MAX_PAIR_JOINS = 4 predicate joins per scalar class");
            joins.emplace_back();
            if ((rc = compile_pair_join(ctx, m.n, cs, joins.back()))) return rc;
        } else if (cs.kind == SF_C_SELFJOIN_VALUE_EQUAL) {
            if (cs.param != 0 && (cs.param < 2 || cs.param > 5)) return fail(ctx, SF_ERR_INVALID, "self-join arity must be 2..5");
            m.sj_level = cs.level;
            m.sj_weight = cs.weight;
            m.sj_arity = cs.param == 0 ? 2 : (int32_t)cs.param;
        } else if (cs.kind == SF_C_GROUPED_VALUE_SUM) {
            if (m.grp_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "one grouped constraint per scalar class");
            if (!ctx->facts.count(cs.fact) || ctx->facts[cs.fact].type != 2 || ctx->facts[cs.fact].rows < m.n)
                return fail(ctx, SF_ERR_INVALID, "grouped sum needs an i32 column fact");
            m.size = (const int32_t*)ctx->facts[cs.fact].d0;
            m.grp_level = cs.level;
            m.grp_weight = cs.weight;
            m.grp_cap = cs.param;
        } else if (cs.kind == SF_C_COMPLEMENTED_VALUE_SUM) {
            if (m.grp_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "one grouped constraint per scalar class");
            if (!ctx->facts.count(cs.fact) || ctx->facts[cs.fact].type != 2 || ctx->facts[cs.fact].rows < m.n)
                return fail(ctx, SF_ERR_INVALID, "complemented grouped sum needs an i32 column fact");
            m.size = (const int32_t*)ctx->facts[cs.fact].d0;
            m.grp_level = cs.level;
            m.grp_weight = cs.weight;
            m.grp_cap = cs.param;  // the target
            m.grp_shape = 1;
            m.grp_complement = 1;
        } else if (cs.kind == SF_C_LOAD_BALANCE_VALUE) {
            if (m.grp_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "one grouped constraint per scalar class");
            if (!ctx->facts.count(cs.fact) || ctx->facts[cs.fact].type != 2 || ctx->facts[cs.fact].rows < m.n)
                return fail(ctx, SF_ERR_INVALID, "load balance needs an i32 metric column fact");
            {  // zero metrics are skipped by the reference's accumulator (load_balance.rs:194-196): the device keeps one
               // count table for every value-keyed node, so every metric must count
                std::vector<int32_t> metric((size_t)m.n);
                HIPCHK(ctx, hipMemcpy(metric.data(), ctx->facts[cs.fact].d0, metric.size() * 4, hipMemcpyDeviceToHost));
                for (int32_t w : metric)
                    if (w < 1) return fail(ctx, SF_ERR_UNSUPPORTED, "load balance metrics must be >= 1");
            }
            m.size = (const int32_t*)ctx->facts[cs.fact].d0;
            m.grp_level = cs.level;
            m.grp_weight = cs.weight;
            m.grp_mode = 1;
        } else if (cs.kind == SF_C_BALANCE_VALUE) {
            if (m.grp_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "one grouped constraint per scalar class");
            m.grp_level = cs.level;
            m.grp_weight = 1;  // the base score sits inside the rounding: score = -round(base * standard deviation)
            m.bal_base = cs.weight;
            m.grp_mode = 2;
        } else if (cs.kind == SF_C_VALUE_COST) {
            if (m.cost_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "one value-cost join per scalar class");
            if (!ctx->facts.count(cs.fact) || ctx->facts[cs.fact].type != 1 || ctx->facts[cs.fact].rows != m.n || ctx->facts[cs.fact].cols != m.n_values)
                return fail(ctx, SF_ERR_INVALID, "value cost needs an i64 matrix fact [n_rows][n_values]");
            m.cost = (const int64_t*)ctx->facts[cs.fact].d0;
            m.cost_level = cs.level;
            m.cost_weight = cs.weight;
        } else if (cs.kind == SF_C_RUNS_VALUE || cs.kind == SF_C_PRESENCE_VALUE) {
            if (m.run_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "one consecutive-runs / indexed-presence constraint per scalar class");
            if (!ctx->facts.count(cs.fact) || ctx->facts[cs.fact].type != 2 || ctx->facts[cs.fact].rows < m.n)
                return fail(ctx, SF_ERR_INVALID, "consecutive runs need an i32 point column fact");
            if (cs.kind == SF_C_RUNS_VALUE && cs.param < 0) return fail(ctx, SF_ERR_INVALID, "consecutive runs: param is the run length limit (>= 0)");
            const int64_t p_lo = cs.param & 0xFFFF, p_hi = (cs.param >> 16) & 0xFFFF, p_cap = (cs.param >> 32) & 0xFFFF;
            const int64_t p_mode = (cs.param >> 48) & 0xFFFF;
            if (cs.kind == SF_C_PRESENCE_VALUE && (cs.param < 0 || p_mode > 1 || p_lo > p_hi || p_hi > 4096))
                return fail(ctx, SF_ERR_INVALID, "indexed presence: param = lo | hi << 16 | cap << 32 | mode << 48 with 0 <= lo <= hi <= 4096, mode 0 / 1");
            std::vector<int32_t> pts((size_t)m.n);
            HIPCHK(ctx, hipMemcpy(pts.data(), ctx->facts[cs.fact].d0, pts.size() * 4, hipMemcpyDeviceToHost));
            int32_t hi = 0;
            for (int32_t x : pts) {
                if (x < 0) return fail(ctx, SF_ERR_UNSUPPORTED, "consecutive runs: points must be >= 0 (shift the index)");
                hi = x > hi ? x : hi;
            }
            if (hi >= 4096 || runs_table_bytes(m.n_values, hi + 1) > 48 * 1024)
                return fail(ctx, SF_ERR_UNSUPPORTED, "consecutive runs: the [n_values][points] count table must fit 48 KiB of LDS (points < 4096)");
            if (m.n > 65535) return fail(ctx, SF_ERR_UNSUPPORTED, "consecutive runs: more than 65535 entities (16-bit point counts)");
            m.run_point = (const int32_t*)ctx->facts[cs.fact].d0;
            m.run_P = hi + 1;
            m.run_level = cs.level;
            m.run_weight = cs.weight;
            m.run_limit = cs.param;
            if (cs.kind == SF_C_PRESENCE_VALUE) {  // the range clipped to the points that occur: absent points never count
                m.run_mode = 1;
                m.run_limit = 0;
                m.run_lo = (int32_t)(p_lo < m.run_P ? p_lo : m.run_P);
                m.run_hi = (int32_t)(p_hi < m.run_P ? p_hi : m.run_P);
                m.run_cap = p_cap;
                if (p_mode == 1) {  // complement_runs(lo..hi): the horizon is NOT clipped (points beyond the table are absent)
                    m.run_mode = 2;
                    m.run_lo = (int32_t)p_lo;
                    m.run_hi = (int32_t)p_hi;
                    m.run_limit = p_cap;
                    m.run_cap = 0;
                }
            }
        } else if (cs.kind == SF_C_EXISTS_VALUE) {
            if (m.ex_level >= 0) return fail(ctx, SF_ERR_UNSUPPORTED, "one exists-by-value constraint per scalar class");
            if (cs.param != 0 && cs.param != 1) return fail(ctx, SF_ERR_INVALID, "exists-by-value: param is 1 (exists) or 0 (not exists)");
            if (cs.fact >= 0) {
                if (!ctx->facts.count(cs.fact) || ctx->facts[cs.fact].type != 2 || ctx->facts[cs.fact].rows < m.n_values)
                    return fail(ctx, SF_ERR_INVALID, "exists-by-value needs an i32 weight column with one entry per value (or fact -1)");
                m.ex_w = (const int32_t*)ctx->facts[cs.fact].d0;
            }
            m.ex_level = cs.level;
            m.ex_weight = cs.weight;
            m.ex_mode = (int32_t)cs.param;
        } else if (cs.kind == SF_C_CROSS_OWNER_MATCH) {
            // the join with the list class: wired in sf_initialize once both models exist
        } else if (cs.kind == SF_C_UNI_PROGRAM_) {
            // compiled below, once every constraint of the class has been seen
        } else
            return fail(ctx, SF_ERR_UNSUPPORTED, "constraint kind on a scalar class");
    }
    if (joins.size() == 1) {  // one join: the class's own join fields, as the kernels of the single-join classes read them
        const PairJoin& j = joins[0];
        m.cross_kind = j.kind, m.cross_level = j.level, m.cross_weight = j.weight;
        m.pn_off = j.pn_off, m.pn = j.pn, m.col = j.col, m.ir = j.ir, m.ir_n = j.ir_n;
    } else if (joins.size() > 1) {  // several: all of them in the device array of join records (scalar unit 2), the own fields unused
        PairJoin* d_xj = nullptr;
        if ((rc = upload(ctx, &d_xj, joins.data(), joins.size()))) return rc;
        m.xj = d_xj;
        m.n_xj = (int32_t)joins.size();
    }
    if ((rc = compile_uni_programs(ctx, d, m))) return rc;
    // The host-driven kernels of the class (evaluate_all, step evaluate / apply / decide, the construction) keep the per-value tables in
    // the dynamic LDS of one launch, next to at most 1 KiB of static LDS: a class they cannot be launched with is refused here, before
    // any of them runs (DESIGN §14).
    if (scalar_table_bytes(ctx) > SF_LDS_BUDGET)
        return fail(ctx, SF_ERR_UNSUPPORTED, "the per-value tables of the scalar class (12 bytes per value, plus the runs table) do not fit the LDS of one launch");
    if (!c.value_off.empty()) {
        uint32_t* d_off = nullptr;
        int32_t* d_vl = nullptr;
        if ((rc = upload(ctx, &d_off, c.value_off.data(), c.value_off.size()))) return rc;
        if ((rc = upload(ctx, &d_vl, c.value_list.data(), c.value_list.size()))) return rc;
        m.vl_off = d_off;
        m.vl = d_vl;
    }
    const int R = ctx->R;
    if ((rc = dalloc(ctx, &m.vals, (size_t)R * m.n))) return rc;
    if ((rc = dalloc(ctx, &m.score, (size_t)R * 4))) return rc;
    if ((rc = dalloc(ctx, &m.best_vals, (size_t)R * m.n))) return rc;
    if ((rc = dalloc(ctx, &m.best_score, (size_t)R * 4))) return rc;
    // replica 0 from the host, then doubled on the device (as the list class: 1 + log2(R) copies, not R)
    HIPCHK(ctx, hipMemcpyAsync(m.vals, c.scalar_init.data(), (size_t)m.n * 4, hipMemcpyHostToDevice, ctx->stream));
    for (size_t k = 1; k < (size_t)R; k *= 2)
        HIPCHK(ctx, hipMemcpyAsync(m.vals + k * m.n, m.vals, std::min(k, (size_t)R - k) * m.n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->has_scalar_model = true;
    ctx->scalar_desc = d;
    return SF_OK;
}

// per-value count / sum tables (keyed self-join, grouped sum): n_values entries, 0 when unused
static int scalar_table_values(sf_ctx* ctx) {
    return ctx->sm.tables() ? ctx->sm.n_values : 0;
}
static size_t scalar_table_bytes(sf_ctx* ctx) {
    return (size_t)scalar_table_values(ctx) * 12 + 16 + (ctx->sm.run_level >= 0 ? runs_table_bytes(ctx->sm.n_values, ctx->sm.run_P) + 16 : 0);
}

template <int L, class VT>
static int launch_scalar_search_t(sf_ctx* ctx, const SearchParams& p, int n_replicas, bool trace) {
    SCarve<VT> cv(ctx->sm.n, scalar_table_values(ctx), ctx->sm.run_level >= 0 ? ctx->sm.run_P : 0);
    size_t lds = cv.total * 4;
    if (lds > SF_LDS_BUDGET) return fail(ctx, SF_ERR_UNSUPPORTED, "scalar class does not fit the LDS slices of one workgroup");
    SearchParams q = p;
    q.n_launch = n_replicas;
    // the unit with the interpreted joins only for the models that need them (SC_IR_*): the specialised kernels do not carry the interpreter;
    // the classes with several joins take the unit with the loop over their join records
    if (ctx->sm.n_xj > 0)
        HIPCHK(ctx, (launch_tu_scalar<L, (int)sizeof(VT), 2>(trace, make_launch(ctx, &q, (n_replicas + 3) / 4, 256, lds))));
    else if (ctx->sm.cross_kind == SC_IR_PARTNERS || ctx->sm.cross_kind == SC_IR_DENSE)
        HIPCHK(ctx, (launch_tu_scalar<L, (int)sizeof(VT), 1>(trace, make_launch(ctx, &q, (n_replicas + 3) / 4, 256, lds))));
    else
        HIPCHK(ctx, (launch_tu_scalar<L, (int)sizeof(VT), 0>(trace, make_launch(ctx, &q, (n_replicas + 3) / 4, 256, lds))));
    return SF_OK;
}

static int launch_scalar_search(sf_ctx* ctx, SearchParams& p, int grid, bool trace) {
    p.n_leaves = 0;
    // default-policy declaration order: change, then swap (default_local_search/policy/scalar.rs:67-106)
    for (int kind : {SF_SEL_SCALAR_CHANGE, SF_SEL_SCALAR_SWAP})
        for (auto& s : ctx->selectors)
            if (s.kind == kind && s.desc == ctx->scalar_desc) {
                if (p.n_leaves >= MAX_LEAVES) return fail(ctx, SF_ERR_UNSUPPORTED, "more than two scalar leaves");
                p.leaf[p.n_leaves++] = LeafSpec{s.kind, 0, s.desc};
            }
    if (p.n_leaves == 0) return fail(ctx, SF_ERR_INVALID, "no scalar selector configured");
    const bool small = ctx->sm.n_values <= 127;
    ctx->last_scalar_value_bytes = small ? 1 : 2;  // (sf_list_arith_flags)
#define SF_SCALAR_CASE(LV)                                                                                     \
    case LV:                                                                                                   \
        if (small)                                                                                             \
            return launch_scalar_search_t<LV, int8_t>(ctx, p, grid, trace);                                    \
        return launch_scalar_search_t<LV, int16_t>(ctx, p, grid, trace);
    switch (ctx->levels <= 2 ? 2 : 4) {  // 1- / 3-level models run with one padded zero level
        SF_SCALAR_CASE(2)
        default:
            SF_SCALAR_CASE(4)
    }
#undef SF_SCALAR_CASE
}
