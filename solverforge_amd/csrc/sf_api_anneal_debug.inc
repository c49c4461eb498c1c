// sf_debug_anneal_chunks: the SimulatedAnnealing acceptor of the search engines (sf_anneal.h) on a scripted sequence of 64-candidate
// chunks, one 64-lane wave, the state in LDS as in the engines.  The kernel calls sa_load / sa_decide / sa_commit / sa_step_ended /
// sa_store and adds nothing of its own to them; the host validates every argument, so the kernel touches its own buffers only.
// Included into sf_api.hip (same translation unit, same build flags as the rest of the library).

static_assert(SF_ANNEAL_STATE_WORDS == SA_WORDS, "the header's state size is the acceptor's");
static_assert(SA_RNG == 0 && SA_TEMP == 4 && SA_CALIBRATING == 8 && SA_SEEN == 9 && SA_CNT == 10 && SA_SUM_LO == 14 && SA_SUM_HI == 18,
              "include/solverforge_amd.h documents this word layout");
static_assert(sizeof(sf_anneal_chunk) == (SF_MAX_LEVELS + 64 * SF_MAX_LEVELS) * 8 + 16, "sf_anneal_chunk has no padding");

namespace sf {

// one wave; chunks [n_chunks], out_accept [n_chunks], out_state [n_chunks][2][SA_WORDS]; sp.state = the SA_WORDS words of replica 0
template <int L>
__global__ __launch_bounds__(64) void k_debug_anneal_chunks(SaParams sp, const sf_anneal_chunk* __restrict__ chunks, int32_t n_chunks,
                                                            uint64_t* __restrict__ out_accept, uint64_t* __restrict__ out_state) {
    __shared__ uint64_t w[SA_WORDS];
    const uint32_t lane = threadIdx.x;
    sa_load(w, sp, 0, lane);
    for (int32_t c = 0; c < n_chunks; ++c) {
        const sf_anneal_chunk& ch = chunks[c];
        ScoreV<L> cur, sc;
#pragma unroll
        for (int k = 0; k < L; ++k) {  // levels the score does not have stay zero, as in the engines
            cur.v[k] = k < sp.levels ? ch.cur[k] : 0;
            sc.v[k] = k < sp.levels ? ch.sc[lane][k] : 0;
        }
        const bool doable = (ch.doable >> lane) & 1ULL;
        SaChunk o;
        const bool acc = sa_decide<L>(w, sp, doable, sc, cur, lane, o);
        const uint64_t accmask = __ballot(acc);
        sa_commit<L>(w, sp, o, (uint32_t)ch.nconsumed, lane);
        uint64_t* out = out_state + (size_t)c * 2 * SA_WORDS;
        if (lane == 0) out_accept[c] = accmask;
        if (lane < SA_WORDS) out[lane] = w[lane];
        if (ch.step_end) sa_step_ended(w, sp, lane);  // wave-uniform
        if (lane < SA_WORDS) out[SA_WORDS + lane] = w[lane];
    }
    sa_store(w, sp, 0, lane);
}

}  // namespace sf

extern "C" int32_t sf_debug_anneal_chunks(sf_ctx* ctx, const sf_annealing_config* cfg, int32_t levels, int32_t hard_levels, int32_t n_chunks,
                                          const sf_anneal_chunk* chunks, uint64_t* out_accept, uint64_t* out_state) {
    if (!ctx) return sf_device_count() > 0 ? SF_ERR_INVALID : SF_ERR_NO_DEVICE;
    DeviceGuard _dev(ctx);
    if (!cfg || !chunks || !out_accept || !out_state) return fail(ctx, SF_ERR_INVALID, "sf_debug_anneal_chunks: null argument");
    if (levels < 1 || levels > SF_MAX_LEVELS || hard_levels < 0 || hard_levels > levels)
        return fail(ctx, SF_ERR_INVALID, "sf_debug_anneal_chunks: levels in 1..4, hard_levels in 0..levels");
    if (n_chunks < 1 || n_chunks > SF_ANNEAL_DEBUG_MAX_CHUNKS) return fail(ctx, SF_ERR_INVALID, "sf_debug_anneal_chunks: n_chunks in 1..65536");
    if (const char* why = anneal_config_error(cfg, levels)) return fail(ctx, SF_ERR_INVALID, why);
    for (int32_t c = 0; c < n_chunks; ++c)
        if (chunks[c].nconsumed < 0 || chunks[c].nconsumed > 64) return fail(ctx, SF_ERR_INVALID, "sf_debug_anneal_chunks: nconsumed in 0..64");

    SaParams sa{};
    anneal_params(*cfg, levels, hard_levels, sa);
    uint64_t w0[SA_WORDS] = {};
    anneal_init_state(*cfg, levels, cfg->seed, w0);
    Scratch<uint64_t> d_state, d_accept, d_out;
    Scratch<sf_anneal_chunk> d_chunks;
    int rc;
    if ((rc = d_state.upload(ctx, w0, SA_WORDS))) return rc;
    if ((rc = d_chunks.upload(ctx, chunks, (size_t)n_chunks))) return rc;
    if ((rc = d_accept.alloc(ctx, (size_t)n_chunks))) return rc;
    if ((rc = d_out.alloc(ctx, (size_t)n_chunks * 2 * SA_WORDS))) return rc;
    sa.state = d_state.p;
    if (levels <= 2)  // the engines' rule for the score width they are built for
        k_debug_anneal_chunks<2><<<dim3(1), dim3(64), 0, ctx->stream>>>(sa, d_chunks.p, n_chunks, d_accept.p, d_out.p);
    else
        k_debug_anneal_chunks<4><<<dim3(1), dim3(64), 0, ctx->stream>>>(sa, d_chunks.p, n_chunks, d_accept.p, d_out.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_accept, d_accept.p, (size_t)n_chunks * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_state, d_out.p, (size_t)n_chunks * 2 * SA_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SF_OK;
}
