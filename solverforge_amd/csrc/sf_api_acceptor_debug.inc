// sf_debug_acceptor_script: the GreatDeluge and StepCountingHillClimbing acceptors of the search engines (sf_step.h) on a scripted
// sequence of records, one 64-lane wave, the state in a global-memory row as in the engines.  The kernel calls acceptor_phase_started /
// ax_step_begin / ax_accepts / ax_step_ended and adds nothing of its own to them; the host validates every argument, so the
// kernel touches its own buffers only.  Included into sf_api.hip (same translation unit, same build flags as the rest of the library).

static_assert(SF_ACCEPTOR_STATE_WORDS == AX_PARAM && AX_LEVEL == 0 && AX_INCR == 4 && AX_SINCE == 8, "include/solverforge_amd.h documents this word layout");
static_assert(sizeof(sf_acceptor_record) == (SF_MAX_LEVELS + 64 * SF_MAX_LEVELS) * 8 + 16, "sf_acceptor_record has no padding");

namespace sf {

// one wave; records [n_records], out_accept [n_records], out_state [n_records][SF_ACCEPTOR_STATE_WORDS]; ax = one state row (SA_WORDS words)
template <int L>
__global__ __launch_bounds__(64) void k_debug_acceptor_script(int acceptor, int levels, uint64_t* ax, const sf_acceptor_record* __restrict__ records,
                                                              int32_t n_records, uint64_t* __restrict__ out_accept, uint64_t* __restrict__ out_state) {
    const uint32_t lane = threadIdx.x;
    for (int32_t i = 0; i < n_records; ++i) {
        const sf_acceptor_record& rec = records[i];
        int64_t cur4[4];
        ScoreV<L> cur, sc;
#pragma unroll
        for (int k = 0; k < 4; ++k) cur4[k] = k < levels ? rec.cur[k] : 0;  // levels the score does not have stay zero, as in the engines
#pragma unroll
        for (int k = 0; k < L; ++k) {
            cur.v[k] = cur4[k];
            sc.v[k] = k < levels ? rec.sc[lane][k] : 0;
        }
        uint64_t accmask = 0;
        if (rec.op == SF_ACCEPTOR_OP_PHASE_STARTED) {
            if (lane == 0) acceptor_phase_started(acceptor, cur4, ax);
        } else if (rec.op == SF_ACCEPTOR_OP_DECIDE) {
            ScoreV<L> late;
            bool thr_on;
            ax_step_begin<L>(acceptor, ax, late, thr_on);
            accmask = __ballot(ax_accepts<L>((rec.doable >> lane) & 1ULL, sc, cur, late, thr_on));
        } else {
            ax_step_ended<L>(acceptor, lane == 0, cur4, ax);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (lane == 0) out_accept[i] = accmask;
        if (lane < SF_ACCEPTOR_STATE_WORDS) out_state[(size_t)i * SF_ACCEPTOR_STATE_WORDS + lane] = ax[lane];
    }
}

}  // namespace sf

extern "C" int32_t sf_debug_acceptor_script(sf_ctx* ctx, int32_t acceptor, int32_t levels, uint64_t param_bits, int32_t n_records,
                                            const sf_acceptor_record* records, uint64_t* out_accept, uint64_t* out_state) {
    if (!ctx) return sf_device_count() > 0 ? SF_ERR_INVALID : SF_ERR_NO_DEVICE;
    DeviceGuard _dev(ctx);
    if (!records || !out_accept || !out_state) return fail(ctx, SF_ERR_INVALID, "sf_debug_acceptor_script: null argument");
    if (acceptor != SF_ACCEPT_GREAT_DELUGE && acceptor != SF_ACCEPT_STEP_COUNTING_HILL_CLIMBING)
        return fail(ctx, SF_ERR_INVALID, "sf_debug_acceptor_script: GreatDeluge or StepCountingHillClimbing");
    if (levels < 1 || levels > SF_MAX_LEVELS) return fail(ctx, SF_ERR_INVALID, "sf_debug_acceptor_script: levels in 1..4");
    if (n_records < 1 || n_records > SF_ACCEPTOR_DEBUG_MAX_RECORDS) return fail(ctx, SF_ERR_INVALID, "sf_debug_acceptor_script: n_records in 1..65536");
    if (acceptor == SF_ACCEPT_GREAT_DELUGE) {
        double rain_speed;
        std::memcpy(&rain_speed, &param_bits, 8);
        if (!std::isfinite(rain_speed)) return fail(ctx, SF_ERR_INVALID, "great deluge: rain_speed must be finite");
    }
    for (int32_t i = 0; i < n_records; ++i)
        if (records[i].op < SF_ACCEPTOR_OP_PHASE_STARTED || records[i].op > SF_ACCEPTOR_OP_STEP_ENDED)
            return fail(ctx, SF_ERR_INVALID, "sf_debug_acceptor_script: op in 0..2");
    if (records[0].op != SF_ACCEPTOR_OP_PHASE_STARTED) return fail(ctx, SF_ERR_INVALID, "sf_debug_acceptor_script: the first record starts the phase");

    uint64_t w0[SA_WORDS] = {};  // the row as sf_phase_start uploads it
    w0[AX_PARAM] = param_bits;
    Scratch<uint64_t> d_state, d_accept, d_out;
    Scratch<sf_acceptor_record> d_records;
    int rc;
    if ((rc = d_state.upload(ctx, w0, SA_WORDS))) return rc;
    if ((rc = d_records.upload(ctx, records, (size_t)n_records))) return rc;
    if ((rc = d_accept.alloc(ctx, (size_t)n_records))) return rc;
    if ((rc = d_out.alloc(ctx, (size_t)n_records * SF_ACCEPTOR_STATE_WORDS))) return rc;
    if (levels <= 2)  // the engines' rule for the score width they are built for
        k_debug_acceptor_script<2><<<dim3(1), dim3(64), 0, ctx->stream>>>(acceptor, levels, d_state.p, d_records.p, n_records, d_accept.p, d_out.p);
    else
        k_debug_acceptor_script<4><<<dim3(1), dim3(64), 0, ctx->stream>>>(acceptor, levels, d_state.p, d_records.p, n_records, d_accept.p, d_out.p);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_accept, d_accept.p, (size_t)n_records * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(out_state, d_out.p, (size_t)n_records * SF_ACCEPTOR_STATE_WORDS * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return SF_OK;
}
