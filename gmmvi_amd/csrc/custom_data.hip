// User-defined targets summed over a data set (custom_target_data.inc, compiled at run time by custom_compile.hip): the launch
// plan, gmmvi_target_custom_data and its own-batch entry, and the predictive density, which a handle of either data mode takes.
#include "custom_target.h"
#include "feistel.h"

// The launch plan.  Auto: the row list is cut into enough chunks that ceil(N / 64) * chunks workgroups reach GMMVI_DATA_PLAN_CUS
// (the compute units of an MI355X: one workgroup of four waves each), but into no more than rows / GMMVI_DATA_MIN_CHUNK_ROWS, so
// that every wave of a chunk has at least GMMVI_DATA_MIN_CHUNK_ROWS / 4 rows to pay for the chunk's merge traffic and launch
// tail.  A request is honoured up to one row per chunk.  Either way the chunks are then as even as whole rows allow, and the
// count is what that row count per chunk needs: the last chunk is never empty.
constexpr int GMMVI_DATA_MIN_CHUNK_ROWS = 32;

extern "C" int gmmvi_custom_data_plan(int N, int64_t rows, int chunks_requested, int* chunks, int* rows_per_chunk) {
    if (N < 1 || rows < 1 || rows > 2147483647ll || chunks_requested < 0 || !chunks || !rows_per_chunk)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_plan needs N >= 1, 1 <= rows < 2^31, "
                                                  "chunks_requested >= 0 and two outputs");
    int64_t want = chunks_requested;
    if (want == 0) {
        const int64_t tiles = ((int64_t)N + 63) / 64;
        const int64_t fill = (GMMVI_DATA_PLAN_CUS + tiles - 1) / tiles;
        const int64_t most = rows / GMMVI_DATA_MIN_CHUNK_ROWS;
        want = fill < most ? fill : most;
    }
    if (want > rows) want = rows;
    if (want > GMMVI_DATA_MAX_CHUNKS) want = GMMVI_DATA_MAX_CHUNKS;
    if (want < 1) want = 1;
    const int64_t per = (rows + want - 1) / want;
    *rows_per_chunk = (int)per;
    *chunks = (int)((rows + per - 1) / per);
    return GMMVI_OK;
}

int gmmvi_custom_check_data_arguments(gmmvi_ctx* ctx, int D, const float* data_dev, int64_t T, int C, int minibatch, int64_t B,
                                      const float* X_dev, int N, const float* lp_out_dev, int chunks_requested) {
    GMMVI_ARG_CHECK(ctx, N >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG && X_dev != nullptr && lp_out_dev != nullptr);
    GMMVI_ARG_CHECK(ctx, data_dev != nullptr && (minibatch == 0 || minibatch == 1) && chunks_requested >= 0);
    if (T < 1 || T > 2147483647ll)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the data set needs 1 <= T < 2^31 rows, got T = " + std::to_string(T));
    if (C < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: a data row needs C >= 1 floats, got C = " + std::to_string(C));
    if (B < 1 || B > T)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the batch size needs 1 <= B <= T = " + std::to_string(T) +
                                                  ", got B = " + std::to_string(B) + " (pass B = T with the full-data mode)");
    return GMMVI_OK;
}

// the row kernel of a launch: a shared batch or own batches, staged or direct, value or gradient
static KernelSlot data_rows_slot(bool own, bool staged, bool want_grad) {
    static const KernelSlot slots[2][2][2] = {
        {{K_DATA_ROWS_DIRECT_LP, K_DATA_ROWS_DIRECT_GRAD}, {K_DATA_ROWS_STAGED_LP, K_DATA_ROWS_STAGED_GRAD}},
        {{K_DATA_ROWS_OWN_DIRECT_LP, K_DATA_ROWS_OWN_DIRECT_GRAD}, {K_DATA_ROWS_OWN_STAGED_LP, K_DATA_ROWS_OWN_STAGED_GRAD}}};
    return slots[own][staged][want_grad];
}

int gmmvi_custom_launch_data(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev, const float* data_dev,
                             int64_t T, int C, int minibatch, int64_t B, uint64_t seed, uint32_t call, const float* X_dev, int N,
                             float* lp_out_dev, float* grad_out_dev, int chunks_requested) {
    const bool want_grad = grad_out_dev != nullptr;
    const bool own = minibatch == GMMVI_DATA_OWN_BATCHES;
    const int64_t length = minibatch ? B : T;
    int chunks = 0, rows_per_chunk = 0;
    if (gmmvi_custom_data_plan(N, length, chunks_requested, &chunks, &rows_per_chunk) != GMMVI_OK)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_plan refused N, the row count or the chunk request");
    const bool staged = D <= GMMVI_CUSTOM_STAGED_MAX_DIM;
    const size_t tiles = ((size_t)N + 63) / 64;
    GMMVI_ARG_CHECK(ctx, tiles <= 2147483647u);
    float* part_lp = nullptr;
    float* part_grad = nullptr;
    if (chunks > 1) {
        const size_t f_lp = (size_t)chunks * (size_t)N;
        const int rc = gmmvi_ws_reserve(ctx, f_lp * (want_grad ? (size_t)D + 1 : 1) * sizeof(float));
        if (rc != GMMVI_OK) return rc;
        part_lp = (float*)ctx->ws;
        part_grad = want_grad ? part_lp + f_lp : nullptr;
    }
    RowList l{C, (unsigned)T, minibatch, (unsigned)length, (unsigned)rows_per_chunk, call,
              gmmvi_feistel_half_bits((uint32_t)T), (unsigned)seed, (unsigned)(seed >> 32)};
    float scale = minibatch ? (float)T / (float)B : 1.f;
    // LDS: the waves' accumulators [3][1 or 1 + W][64], then the staged x image [64][D | 1]: 13056 + 30976 B at D = 120
    const size_t lds = ((size_t)3 * (want_grad ? 1 + GMMVI_CUSTOM_AUTODIFF_TANGENTS : 1) * 64 + (staged ? (size_t)64 * (D | 1) : 0)) *
                       sizeof(float);
    {
        void* args[] = {&D, &params_dev, &X_dev, &N, &data_dev, &l, &scale, &lp_out_dev, &grad_out_dev, &part_lp, &part_grad};
        GMMVI_PROF(ctx, own ? "target_custom_data_own" : "target_custom_data");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[data_rows_slot(own, staged, want_grad)], (unsigned)tiles, (unsigned)chunks, 1,
                                                   256, 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
    }
    if (chunks > 1) {
        const size_t blocks = ((size_t)N + 255) / 256;
        void* args[] = {&D, &params_dev, &X_dev, &N, &chunks, &scale, &lp_out_dev, &grad_out_dev, &part_lp, &part_grad};
        GMMVI_PROF(ctx, "target_custom_data_merge");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[want_grad ? K_DATA_MERGE_GRAD : K_DATA_MERGE_LP], (unsigned)blocks, 1, 1, 256,
                                                   1, 1, 0, ctx->stream, args, nullptr));
    }
    return GMMVI_OK;
}

// gmmvi_target_custom_data (E_DATA) and gmmvi_target_custom_data_own_batches (E_DATA_OWN, minibatch == 1, kernels of its own)
static int target_custom_data(Entry entry, gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                              const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed, uint32_t call,
                              const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int chunks_requested) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    if (const int rc = gmmvi_custom_check_mode(ctx, entry, t)) return rc;
    if (const int rc = gmmvi_custom_check_data_arguments(ctx, D, data_dev, T, C, minibatch, B, X_dev, N, lp_out_dev, chunks_requested))
        return rc;
    if (grad_out_dev != nullptr && D > GMMVI_CUSTOM_AUTODIFF_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the gradient of a differentiated target needs D <= " +
                                                  std::to_string(GMMVI_CUSTOM_AUTODIFF_MAX_DIM) + ", got D = " + std::to_string(D) +
                                                  " (a value call runs above)");
    return gmmvi_custom_launch_data(ctx, t, D, params_dev, data_dev, T, C, entry == E_DATA_OWN ? GMMVI_DATA_OWN_BATCHES : minibatch, B,
                                    seed, call, X_dev, N, lp_out_dev, grad_out_dev, chunks_requested);
}

extern "C" int gmmvi_target_custom_data(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                        const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed,
                                        uint32_t call, const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                        int chunks_requested) {
    return target_custom_data(E_DATA, ctx, t, D, params_dev, data_dev, T, C, minibatch, B, seed, call, X_dev, N, lp_out_dev,
                              grad_out_dev, chunks_requested);
}

extern "C" int gmmvi_target_custom_data_own_batches(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                                    const float* data_dev, int64_t T, int C, int64_t B, uint64_t seed, uint32_t call,
                                                    const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                                    int chunks_requested) {
    return target_custom_data(E_DATA_OWN, ctx, t, D, params_dev, data_dev, T, C, 1, B, seed, call, X_dev, N, lp_out_dev, grad_out_dev,
                              chunks_requested);
}

// ---- predictive density of a data-set target: the reduction over the samples -------------------------------------------------------
extern "C" int gmmvi_custom_data_predictive_plan(int N, int64_t M, int chunks_requested, int* tiles, int* chunks,
                                                 int64_t* rows_per_chunk) {
    if (N < 1 || M < 1 || M > 2147483647ll || chunks_requested < 0 || !tiles || !chunks || !rows_per_chunk)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_predictive_plan needs N >= 1, 1 <= M < 2^31, "
                                                  "chunks_requested >= 0 and three outputs");
    int count = 0, per = 0;
    const int rc = gmmvi_custom_data_plan(N, M, chunks_requested, &count, &per);
    if (rc != GMMVI_OK) return rc;
    *tiles = (int)(((int64_t)N + 63) / 64);
    *chunks = count;
    *rows_per_chunk = per;
    return GMMVI_OK;
}

extern "C" int gmmvi_custom_data_predictive(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                            const float* rows_dev, int64_t M, int C, const float* X_dev, int N, float* lpd_out_dev,
                                            float* mean_out_dev, float* var_out_dev, int chunks_requested) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    if (!t || !rows_dev || !X_dev || !lpd_out_dev)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_predictive needs a target handle, rows_dev, X_dev "
                                              "and lpd_out_dev (only mean_out_dev and var_out_dev may be NULL)");
    if (find_target(ctx, t) == ctx->custom_targets.end())
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the custom target does not belong to this context");
    if (const int rc = gmmvi_custom_check_mode(ctx, E_PREDICTIVE, t)) return rc;
    if (N < 1) return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the predictive density needs N >= 1 samples, got N = " + std::to_string(N));
    if (M < 1 || M > 2147483647ll)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the evaluation set needs 1 <= M < 2^31 rows, got M = " + std::to_string(M));
    if (C < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: a data row needs C >= 1 floats, got C = " + std::to_string(C));
    if (D < 1 || D > GMMVI_MAX_DIM_DIAG)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the predictive density needs 1 <= D <= " +
                                                  std::to_string(GMMVI_MAX_DIM_DIAG) + ", got D = " + std::to_string(D));
    GMMVI_ARG_CHECK(ctx, chunks_requested >= 0);
    int tiles = 0, chunks = 0;
    int64_t per64 = 0;
    if (gmmvi_custom_data_predictive_plan(N, M, chunks_requested, &tiles, &chunks, &per64) != GMMVI_OK)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, g_gmmvi_global_err);
    float* part = nullptr;
    if (tiles > 1) {                                                 // [tiles][M] partials of (max, sumexp, mean, M2)
        const int rc = gmmvi_ws_reserve(ctx, (size_t)tiles * (size_t)M * 4 * sizeof(float));
        if (rc != GMMVI_OK) return rc;
        part = (float*)ctx->ws;
    }
    const bool staged = D <= GMMVI_CUSTOM_STAGED_MAX_DIM;
    const size_t lds = staged ? (size_t)64 * (D | 1) * sizeof(float) : 0;   // the x image [64][D | 1]: 30976 B at D = 120
    unsigned rows = (unsigned)M, per = (unsigned)per64;
    {
        void* args[] = {&D, &params_dev, &X_dev, &N, &rows_dev, &rows, &C, &per, &part, &lpd_out_dev, &mean_out_dev, &var_out_dev};
        GMMVI_PROF(ctx, "custom_data_predictive");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[staged ? K_PRED_STAGED : K_PRED_DIRECT], (unsigned)tiles, (unsigned)chunks, 1,
                                                   256, 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
    }
    if (tiles > 1) {
        const size_t blocks = ((size_t)M + 255) / 256;
        void* args[] = {&N, &rows, &tiles, &part, &lpd_out_dev, &mean_out_dev, &var_out_dev};
        GMMVI_PROF(ctx, "custom_data_predictive_merge");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[K_PRED_MERGE], (unsigned)blocks, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
    }
    return GMMVI_OK;
}
