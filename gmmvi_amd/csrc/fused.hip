// gmmvi_train_iter_samtron: the whole SAMTRON iteration (GMMVI.train_iter, optimization/gmmvi.py:146-174, with a
// component-based sample selector at reuse ratio 0) issued from ONE host call.  It is exactly the composition of the
// public entry points of this library in the order the Python modules call them -- no extra arithmetic lives here --
// (the element-wise bookkeeping between them -- DB mapping offset, model snapshot into the DB, the two stepsize rules,
// the weight-history column -- is folded into one prep kernel / the weight-update kernel, same arithmetic per element)
// so that the fast path and the modular plug-in path produce identical results (tests/test_hip_fused.py).  Purpose:
// the modular path costs ~20 Python->C transitions per iteration (~340 us of host time, more than the kernels take).
#include "common.h"
#include "stepsize_rules.h"
#include "iter_prep.h"
#include "stein_finalize.h"

namespace {
// scratch both iterations carve the same way: ld [K, N] | lq [N] | bg [N] | qgrad [N, D] | H [K, D, D] | g [K, D] | E [K] | success [K]
struct Arena { float *ld, *lq, *bg, *qgrad, *H, *g, *E; int32_t* success; };

// -> the first float behind the carved part
float* carve_arena(float* base, int K, int D, int N, Arena& a) {
    a.ld = base; base += (size_t)K * N;
    a.lq = base; base += N;
    a.bg = base; base += N;
    a.qgrad = base; base += (size_t)N * D;
    a.H = base; base += (size_t)K * D * D;
    a.g = base; base += (size_t)K * D;
    a.E = base; base += K;
    a.success = (int32_t*)base; base += K;
    return base;
}

// What density.hip (gmmvi_sweep_launch) reads from the context about the sweep it is asked for: which sweep of the iteration it is (profile name)
// and whether the next launch carries the merge of its chunk partials.  Holds for the scope, whatever way it is left.
struct SweepScope {
    gmmvi_ctx* ctx; const char* tag; bool defer;
    SweepScope(gmmvi_ctx* c, const char* t, bool d) : ctx(c), tag(c->prof_tag), defer(c->defer_combine) {
        c->prof_tag = t;
        c->defer_combine = d;
    }
    ~SweepScope() { ctx->prof_tag = tag; ctx->defer_combine = defer; }
    SweepScope(const SweepScope&) = delete;
    SweepScope& operator=(const SweepScope&) = delete;
};
}  // namespace

static int arena_reserve(gmmvi_ctx* ctx, size_t floats) {
    if (floats * sizeof(float) <= ctx->arena_bytes) return GMMVI_OK;
    GMMVI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->arena) GMMVI_HIP_CHECK(ctx, hipFree(ctx->arena));
    ctx->arena = nullptr;
    ctx->arena_bytes = 0;
    size_t want = floats * sizeof(float) * 3 / 2;
    GMMVI_HIP_CHECK(ctx, hipMalloc(&ctx->arena, want));
    ctx->arena_bytes = want;
    return GMMVI_OK;
}

#define GMMVI_TRY(call)                \
    do {                               \
        int rc__ = (call);             \
        if (rc__ != GMMVI_OK) return rc__; \
    } while (0)

// Error exit of both entry points.  A deferred merge points into defer_ws and the arena, queued riders into the plan's arrays:
// none may survive the call (a later public call on the context would carry or flush them into memory that may be gone).
static void drop_pending(gmmvi_ctx* ctx) {
    ctx->pending = CombineJob();
    ctx->riders.prep_blocks = ctx->riders.sample_blocks = 0;
    ctx->defer_combine = false;
    ctx->prof_tag = nullptr;
}

static int check_target(gmmvi_ctx* ctx, const gmmvi_target_spec& t, int D) {
    if (!((t.kind >= 0 && t.kind <= 2) || t.kind == 4 || t.kind == 5))
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: target_kind " + std::to_string(t.kind) +
                                                  " (0 mixture, 1 planar robot, 2 logistic regression, 4 Talos, 5 user-defined)");
    if (t.kind == 2 && !(t.logreg_A && t.logreg_M >= 1 && t.logreg_prior_std > 0.f))
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: target_kind 2 needs logreg_A, logreg_M >= 1 and logreg_prior_std > 0");
    if (t.kind == 4 && !(t.talos_model && t.talos_context && D == 34))
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: target_kind 4 needs talos_model, talos_context and D == 34");
    if (t.kind == 5 && !t.custom)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: target_kind 5 needs custom (gmmvi_custom_target_compile)");
    return GMMVI_OK;
}

static int eval_target(gmmvi_ctx* ctx, const gmmvi_target_spec& t, int D, const float* x, int n, float* lp, float* grad) {
    switch (t.kind) {
        case 1: return gmmvi_target_planar(ctx, D, t.planar_prior_std, t.planar_goals_count, t.planar_goals, t.planar_likelihood_std,
                                           x, n, lp, grad);
        case 2: return gmmvi_target_logreg(ctx, D, t.logreg_M, t.logreg_A, t.logreg_prior_mean, t.logreg_prior_std, x, n, lp, grad);
        case 4: return gmmvi_target_talos(ctx, t.talos_model, t.talos_context, x, n, lp, grad);
        case 5: return gmmvi_target_custom(ctx, t.custom, D, t.custom_params, x, n, lp, grad, 0);   // (no riders, no merge: flushed behind it)
        default: {
            SweepScope sweep(ctx, "sweep_target", false);
            return gmmvi_mixture_eval(ctx, t.mix_family, t.mix_nu, t.mix_K, D, t.mix_packed, t.mix_logw, x, n, nullptr, lp, grad);
        }
    }
}

static int max_per_component(int given, int n, int K) { return given > 0 ? given : (n + K - 1) / K; }

// The two stepsize rules of a plan as the prep workgroups take them (iter_prep.h); logw: the weights the weight rule reads.
template <class Plan>
static PrepArgs stepsize_prep(const Plan& p, const float* logw) {
    const gmmvi_stepsize_rule &cs = p.component_stepsize, &ws = p.weight_stepsize;
    PrepArgs q{};
    q.K = p.K; q.stepsizes = p.stepsizes; q.reward_prev = p.reward_prev; q.reward_last = p.reward_last;
    q.cs_mode = cs.mode; q.cs_min = cs.min; q.cs_max = cs.max; q.cs_inc = cs.inc; q.cs_dec = cs.dec;
    q.logw = logw; q.wstate = p.wstate;
    q.ws_mode = ws.mode; q.ws_min = ws.min; q.ws_max = ws.max; q.ws_inc = ws.inc; q.ws_dec = ws.dec;
    return q;
}

// Queues the next iteration's draw of n samples from the plan's components (Philox indices first_index + N ..) as riders of
// the next launch that takes them (riders.h).
template <class Plan>
static void queue_next_draw(gmmvi_ctx* ctx, const Plan& p, int n, int max_pc, float* X, int32_t* mapping, int32_t mapping_base) {
    SampleJob& sj = ctx->riders.sample;
    sj.K = p.K; sj.D = p.D; sj.uniform_count = (long)p.K * max_pc == n ? max_pc : 0;
    sj.means = p.means; sj.chols = p.chols; sj.offsets = p.offsets;
    sj.seed = p.seed; sj.first_index = p.first_index + (uint64_t)p.N;
    sj.X = X; sj.mapping = mapping; sj.mapping_base = mapping_base;
    ctx->riders.sample_blocks = p.K * ((max_pc + 255) / 256);
}

static int train_iter_samtron_body(gmmvi_ctx* ctx, const gmmvi_samtron_plan* p);

extern "C" int gmmvi_train_iter_samtron(gmmvi_ctx* ctx, const gmmvi_samtron_plan* p) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    int rc = gmmvi_flush_pending_combine(ctx);         // no deferred merge is inherited at entry
    if (rc == GMMVI_OK) rc = train_iter_samtron_body(ctx, p);
    if (rc != GMMVI_OK) drop_pending(ctx);
    return rc;
}

static int train_iter_samtron_body(gmmvi_ctx* ctx, const gmmvi_samtron_plan* p) {
    GMMVI_ARG_CHECK(ctx, p != nullptr);
    GMMVI_TRY(check_target(ctx, p->target, p->D));
    const int K = p->K, D = p->D, N = p->N;
    GMMVI_ARG_CHECK(ctx, K >= 1 && D >= 1 && D < GMMVI_MAX_DIM && N >= 1);
    GMMVI_ARG_CHECK(ctx, p->means && p->chols && p->logw && p->packed && p->packed_new && p->stepsizes && p->last_eta &&
                             p->l2 && p->num_updates && p->offsets && p->bg_logw && p->db_samples && p->db_tlp &&
                             p->db_tgrad && p->db_mapping && p->reward_next && p->wstate);
    GMMVI_ARG_CHECK(ctx, p->n_old >= 0 && p->max_per_component >= 0 && p->phase >= 0 && p->phase <= 2);
    GMMVI_ARG_CHECK(ctx, p->n_old == 0 || (p->bg_packed != nullptr && p->bg_K >= 1 && p->bg_old != nullptr && p->bg_logw_new != nullptr));
    const int n_old = p->n_old;
    const int Na = n_old + N;                          // active samples: the reused ones followed by the new ones
    const size_t KN = (size_t)K * Na, ND = (size_t)Na * D;
    const size_t floats = KN + 4 * (size_t)Na + ND + (size_t)K * D * D + (size_t)K * D + 3 * (size_t)K + Na + 64;
    GMMVI_TRY(arena_reserve(ctx, floats));
    Arena a;
    float* bg_a = carve_arena((float*)ctx->arena, K, D, Na, a) + Na;   // (the Na words in front belong to no launch)
    float* bg_b = bg_a + Na;                           // reused samples: the two halves of the background density
    const int max_pc = max_per_component(p->max_per_component, N, K);

    const int phase = p->phase;        // 0: everything; 1: through the component update; 2: the weight update
    float* x = p->db_samples;          // the new samples are written straight into the database
    float* xa = x - (size_t)n_old * D; // the active samples: the n_old database rows in front of them and the new ones
    const float* tlp_a = p->db_tlp - n_old;
    const float* tgrad_a = p->db_tgrad - (size_t)n_old * D;
    if (phase != 2) {
    // ---- sample selection: draw, evaluate the target, append to the DB (sample_selector.py:160-219) --------------------
    // the element-wise bookkeeping (model snapshot into the DB, the two stepsize rules) rides in extra blocks of the
    // sampling launch, and the sampling blocks write the DB mapping (component index + base) directly
    PrepArgs prep_later{};
    bool prep_pending = false;
    {
        PrepArgs q = stepsize_prep(*p, p->logw);
        if (p->db_means && p->db_chols && p->db_packed) {
            q.cdst[0] = (uint32_t*)p->db_means; q.csrc[0] = (const uint32_t*)p->means; q.cwords[0] = (size_t)K * D;
            q.cdst[1] = (uint32_t*)p->db_chols; q.csrc[1] = (const uint32_t*)p->chols; q.cwords[1] = (size_t)K * D * D;
            q.cdst[2] = (uint32_t*)p->db_packed; q.csrc[2] = (const uint32_t*)p->packed;
            q.cwords[2] = (size_t)K * gmmvi_packed_stride(D);
        }
        if (p->presampled && n_old == 0) {
            // the previous call drew this iteration's samples behind its component update (below): only the bookkeeping is
            // left, and it rides in the target evaluation (riders.h) -- nothing before the component update reads what it
            // writes.  (Not in the dual sweep: at one 108 KB workgroup per CU that launch has no room for extra workgroups,
            // 16 riders made it 36 us instead of 24.)
            prep_later = q;
            prep_pending = true;
        } else {
            GMMVI_TRY(gmmvi_sample_components_prep(ctx, K, D, p->means, p->chols, p->offsets, N, max_pc, p->seed,
                                                   p->first_index, x, p->db_mapping, p->mapping_base, q));
        }
    }
    // ---- background + model density / gradient (sample_db.py:194-228, gmm.py:274-300) ------------------------------------
    // issued BEFORE the target evaluation, which does not depend on them: the merge of the model sweep's component-chunk
    // partials rides as extra workgroups in the target launch instead of a launch of its own (combine.h; same arithmetic)
    if (p->bg_packed == nullptr) {
        // nothing reused: the background components are the model's own -- one sweep for both mixtures
        SweepScope sweep(ctx, "sweep_dual", true);
        GMMVI_TRY(gmmvi_mixture_eval_dual(ctx, GMMVI_GAUSS, 0.f, K, D, p->packed, p->logw, p->bg_logw, x, N, a.ld, a.lq, a.qgrad, a.bg));
    } else {
        // reused samples: the background mixture of the window = the mixture the reused samples came from (bg_K snapshot
        // components; its density is KNOWN for the reused samples -- bg_old, from the effective-sample-size step -- and is
        // evaluated for the new samples only) joined with the mixture of the new components over all active samples, each
        // with its share of the window (SampleDB.get_newest_samples takes the same route: optimization/sample_db.py)
        {
            SweepScope sweep(ctx, "sweep_background", false);
            GMMVI_TRY(gmmvi_mixture_eval(ctx, GMMVI_GAUSS, 0.f, p->bg_K, D, p->bg_packed, p->bg_logw, x, N, nullptr, bg_a + n_old, nullptr));
            GMMVI_TRY(gmmvi_mixture_eval(ctx, GMMVI_GAUSS, 0.f, K, D, p->packed, p->bg_logw_new, xa, Na, nullptr, bg_b, nullptr));
        }
        GMMVI_HIP_CHECK(ctx, hipMemcpyAsync(bg_a, p->bg_old, (size_t)n_old * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
        GMMVI_TRY(gmmvi_logaddexp_f32(ctx, a.bg, bg_a, p->bg_log_share_old, bg_b, p->bg_log_share_new, (size_t)Na));
        SweepScope sweep(ctx, "sweep_model", true);
        GMMVI_TRY(gmmvi_mixture_eval(ctx, GMMVI_GAUSS, 0.f, K, D, p->packed, p->logw, xa, Na, a.ld, a.lq, a.qgrad));
    }
    if (prep_pending) {
        ctx->riders.prep = prep_later;
        ctx->riders.prep_blocks = K < 64 ? K : 64;
    }
    GMMVI_TRY(eval_target(ctx, p->target, D, x, N, p->db_tlp, p->db_tgrad));
    GMMVI_TRY(gmmvi_flush_pending_combine(ctx));       // nothing left unless the target launch could not carry it
    GMMVI_TRY(gmmvi_flush_pending_riders(ctx));        // (the planar-robot target kernel carries no riders: their own launch)
    // ---- component update (gmmvi.py:165-169) -----------------------------------------------------------------------------
    // the Stein estimate stops at its partial slab; its last step (slab sum, Sigma^-1, normalisation) is the prologue of the
    // update kernel where that is instantiated, the stand-alone launch otherwise -- the same arithmetic either way
    SteinSlab slab{nullptr, nullptr, 0};
    GMMVI_TRY(gmmvi_stein_partials(ctx, K, D, p->packed, xa, Na, a.ld, a.qgrad, a.bg, tgrad_a, p->stein_flags, &slab));
    GMMVI_TRY(gmmvi_update_components_kl_from_slab(ctx, K, D, slab, Na, p->stein_flags, p->packed, a.H, a.g, p->means, p->chols,
                                                   p->stepsizes, p->temperature, p->l2_init, p->last_eta, p->l2, p->num_updates,
                                                   p->success_out ? p->success_out : a.success, p->packed_new));
    }
    if (phase == 1) return GMMVI_OK;
    // ---- weight update (gmmvi.py:172-173) ---------------------------------------------------------------------------------
    // (the merge of this sweep's log-density partials happens inside the expected-log-ratio kernel)
    {
        SweepScope sweep(ctx, "sweep_post", true);
        GMMVI_TRY(gmmvi_mixture_eval(ctx, GMMVI_GAUSS, 0.f, K, D, p->packed_new, p->logw, xa, Na, a.ld, a.lq, nullptr));
    }
    // the next iteration's draw from the UPDATED components rides in the expected-log-ratio launch, whose K workgroups leave most
    // CUs idle (riders.h; the draw needs neither the weights nor anything this launch writes).  Inside the post-update sweep it
    // would queue behind that launch's workgroups: every workgroup of a launch gets the launch's LDS size, 108 KB there
    if (p->presample_next && n_old == 0)
        queue_next_draw(ctx, *p, N, max_pc, x + (size_t)N * D, p->db_mapping + N, p->mapping_base + K);
    GMMVI_TRY(gmmvi_expected_log_ratios(ctx, K, Na, a.ld, a.bg, tlp_a, a.lq, p->temperature, p->logw,
                                        (p->stein_flags & GMMVI_SELF_NORMALIZED) ? 1 : 0, a.E, p->reward_next, nullptr));
    GMMVI_TRY(gmmvi_flush_pending_riders(ctx));        // (nothing is left normally)
    if (K > 1) {
        GMMVI_TRY(gmmvi_update_weights_internal(ctx, p->weight_update_mode == 0 ? 0 : 1, K, p->logw, a.E, p->wstate,
                                                p->temperature, nullptr, p->weight_slot));
    }
    return GMMVI_OK;
}


// ---- component shards: the iteration in four phases with an all-gather between them (include/gmmvi_hip.h) ---------------
extern "C" size_t gmmvi_sharded_scratch_floats(int K, int D, int N) {
    if (K < 1 || D < 1 || N < 1) return 0;
    return (size_t)K * N + 2 * (size_t)N + (size_t)N * D + (size_t)K * D * D + (size_t)K * D + 2 * (size_t)K + 64;
}

static int sharded_phase_body(gmmvi_ctx* ctx, const gmmvi_sharded_plan* p, int phase) {
    const int R = p->n_ranks, K = p->K, D = p->D, N = p->N;
    const int Nl = N / R, Kt = K * R;
    const size_t s1 = (size_t)Nl * (2 * D + 1) + 2 * (size_t)K, s2 = (size_t)N * (D + 2), s3 = (size_t)N;
    float* my1 = p->e1 + (size_t)p->rank * s1;         // x_loc | tlp_loc | tgrad_loc | E_loc | reward_loc
    float* x_loc = my1;
    float* tlp_loc = my1 + (size_t)Nl * D;
    float* tgrad_loc = tlp_loc + Nl;
    float* E_loc = tgrad_loc + (size_t)Nl * D;
    float* reward_loc = E_loc + K;
    float* my2 = p->e2 + (size_t)p->rank * s2;         // bg_part | lq_part | qgrad_part
    float* my3 = p->e3 + (size_t)p->rank * s3;
    float* logw_loc = p->logw_all + (size_t)p->rank * K;
    Arena a;
    carve_arena(p->scratch, K, D, N, a);
    const int max_pc = max_per_component(p->max_per_component, Nl, K);
    if (phase == 1) {
        // ---- the local draw and its target evaluation, written where the first exchange picks them up -----------------------
        if (!p->presampled)
            GMMVI_TRY(gmmvi_sample_components_bounded(ctx, K, D, p->means, p->chols, p->offsets, Nl, max_pc, p->seed, p->first_index, 0,
                                                      nullptr, x_loc, nullptr));
        return eval_target(ctx, p->target, D, x_loc, Nl, tlp_loc, tgrad_loc);
    }
    if (phase == 2) {
        // ---- de-interleave the first exchange (one rank: the parts ARE the gathered arrays when the caller aliased them) ------
        const bool aliased = R == 1 && p->x_all == x_loc && p->tlp_all == tlp_loc && p->tgrad_all == tgrad_loc &&
                             p->E_all == E_loc && p->reward_all == reward_loc;
        if (!aliased) {
            const size_t words[5] = {(size_t)Nl * D, (size_t)Nl, (size_t)Nl * D, (size_t)K, (size_t)K};
            void* const dst[5] = {p->x_all, p->tlp_all, p->tgrad_all, p->E_all, p->reward_all};
            GMMVI_TRY(gmmvi_unpack_gathered(ctx, p->e1, R, s1, 5, words, dst));
        }
        // ---- the previous iteration's weight step, replicated (weight_updater.py:56-100, gmm_wrapper.py:150-160) --------------
        if (p->has_pending) {
            GMMVI_HIP_CHECK(ctx, hipMemcpyAsync(p->reward_col_pending, p->reward_all, (size_t)Kt * sizeof(float),
                                                hipMemcpyDeviceToDevice, ctx->stream));
            if (Kt > 1)
                GMMVI_TRY(gmmvi_update_weights_internal(ctx, 0, Kt, p->logw_all, p->E_all, p->wstate, p->temperature, nullptr, nullptr));
        }
        // ---- stepsize rules: components local, weights over all components (iter_prep.h); they ride in the dual sweep when that
        // launch has room, else their own small launch
        PrepArgs q = stepsize_prep(*p, p->logw_all);
        q.ws_K = Kt; q.ws_reward_last = p->reward_last_all;
        ctx->riders.prep = q;
        ctx->riders.prep_blocks = 1;
        GMMVI_TRY(gmmvi_flush_pending_riders(ctx));
        // ---- dual sweep over the local components on all samples; its partials are this rank's part of the second exchange ----
        float* bg_out = R > 1 ? my2 : a.bg;
        float* lq_out = R > 1 ? my2 + N : a.lq;
        float* qg_out = R > 1 ? my2 + 2 * (size_t)N : a.qgrad;
        SweepScope sweep(ctx, "sweep_dual", false);
        return gmmvi_mixture_eval_dual(ctx, GMMVI_GAUSS, 0.f, K, D, p->packed, logw_loc, p->bg_logw, p->x_all, N, a.ld, lq_out, qg_out,
                                       bg_out);
    }
    if (phase == 3) {
        if (R > 1) {
            // merge of the ranks' partials: log q and its gradient, the background as the second set of log values
            GMMVI_PROF(ctx, "mixture_combine");
            GMMVI_TRY(gmmvi_combine_partials_internal(ctx, R, N, D, p->e2 + N, p->e2 + 2 * (size_t)N, a.lq, a.qgrad, p->e2, a.bg,
                                                      (long)s2));
        }
        SteinSlab slab{nullptr, nullptr, 0};
        GMMVI_TRY(gmmvi_stein_partials(ctx, K, D, p->packed, p->x_all, N, a.ld, a.qgrad, a.bg, p->tgrad_all, p->stein_flags, &slab));
        GMMVI_TRY(gmmvi_update_components_kl_from_slab(ctx, K, D, slab, N, p->stein_flags, p->packed, a.H, a.g, p->means, p->chols,
                                                       p->stepsizes, p->temperature, p->l2_init, p->last_eta, p->l2, p->num_updates,
                                                       p->success_out ? p->success_out : a.success, p->packed_new));
        // post-update sweep: one rank leaves the merge of its chunk partials to the expected-log-ratio kernel (phase 4); with
        // more ranks the merged local log q is what travels
        SweepScope sweep(ctx, "sweep_post", R == 1);
        return gmmvi_mixture_eval(ctx, GMMVI_GAUSS, 0.f, K, D, p->packed_new, logw_loc, p->x_all, N, a.ld, R > 1 ? my3 : a.lq, nullptr);
    }
    // ---- phase 4: expected log-ratios / rewards of the local components; with more ranks the gathered log q partials are merged
    // while they are read (the kernel's chunk-partial form: [R][N])
    if (R > 1) {
        GMMVI_TRY(gmmvi_flush_pending_combine(ctx));
        ctx->pending.R = R; ctx->pending.N = N; ctx->pending.D = D;
        ctx->pending.lp_parts = p->e3; ctx->pending.lp_out = a.lq;
    }
    // the next iteration's local draw from the updated components, into this rank's part of the first exchange buffer: nothing
    // reads that part any more (x was de-interleaved in phase 2; one rank with aliased views: the sweeps and the Stein estimate
    // are done, this launch reads log values only)
    if (p->presample_next)
        queue_next_draw(ctx, *p, Nl, max_pc, x_loc, nullptr, 0);
    GMMVI_TRY(gmmvi_expected_log_ratios(ctx, K, N, a.ld, a.bg, p->tlp_all, a.lq, p->temperature, logw_loc,
                                        (p->stein_flags & GMMVI_SELF_NORMALIZED) ? 1 : 0, E_loc, reward_loc, nullptr));
    GMMVI_TRY(gmmvi_flush_pending_riders(ctx));
    return GMMVI_OK;
}

extern "C" int gmmvi_train_iter_sharded_phase(gmmvi_ctx* ctx, const gmmvi_sharded_plan* p, int phase) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr && p != nullptr && phase >= 1 && phase <= 4);
    GMMVI_TRY(check_target(ctx, p->target, p->D));
    GMMVI_ARG_CHECK(ctx, p->n_ranks >= 1 && p->rank >= 0 && p->rank < p->n_ranks && p->K >= 1 && p->D >= 1 && p->D < GMMVI_MAX_DIM &&
                             p->N >= p->n_ranks && p->N % p->n_ranks == 0);
    GMMVI_ARG_CHECK(ctx, p->means && p->chols && p->packed && p->packed_new && p->stepsizes && p->last_eta && p->l2 && p->num_updates &&
                             p->logw_all && p->bg_logw && p->offsets && p->e1 && p->e2 && p->e3 && p->x_all && p->tlp_all &&
                             p->tgrad_all && p->E_all && p->reward_all && p->wstate && p->reward_prev && p->reward_last &&
                             p->reward_last_all && p->scratch);
    GMMVI_ARG_CHECK(ctx, !p->has_pending || p->reward_col_pending != nullptr);
    int rc = GMMVI_OK;
    if (phase != 4) rc = gmmvi_flush_pending_combine(ctx);     // (phase 4 consumes the merge phase 3 left for it)
    if (rc == GMMVI_OK) rc = sharded_phase_body(ctx, p, phase);
    if (rc != GMMVI_OK) drop_pending(ctx);
    return rc;
}

extern "C" size_t gmmvi_struct_bytes(int which) {
    const size_t bytes[4] = {sizeof(gmmvi_target_spec), sizeof(gmmvi_stepsize_rule), sizeof(gmmvi_samtron_plan),
                             sizeof(gmmvi_sharded_plan)};
    return which >= 0 && which < 4 ? bytes[which] : 0;
}
