// User-defined targets differentiated on a tape (custom_target_tape.inc, custom_target_data_tape.inc, compiled at run time by
// custom_compile.hip): the plans, the driver of a gradient call, which both tape modes share, and their entries.
#include "custom_target.h"
#include "feistel.h"

// ---- the gradient driver ------------------------------------------------------------------------------------------------------
static int tape_length(const gmmvi_custom_target* t, int D) {
    const auto it = t->tape_lengths.find(D);
    return it == t->tape_lengths.end() ? 0 : it->second;
}

extern "C" int gmmvi_custom_tape_length(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, int* length) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end() && length != nullptr);
    *length = tape_length(t, D);
    return GMMVI_OK;
}

namespace {
// scratch of one attempt: [needed length, padded to 256 B | records [waves][cap][64] | adjoints, the same shape | whatever else
// wave_bytes counts: the data mode's accumulators [waves][D][64]]
struct TapeScratch { int* needed; char* rec; float* adj; float* acc; };

int reserve_tapes(gmmvi_ctx* ctx, size_t waves, int cap, size_t wave_bytes, TapeScratch& s) {
    const size_t f_rec = waves * 64 * (size_t)cap;
    if (const int rc = gmmvi_ws_reserve(ctx, 256 + waves * wave_bytes)) return rc;
    char* rec = (char*)ctx->ws + 256;
    float* adj = (float*)(rec + f_rec * 16);
    s = {(int*)ctx->ws, rec, adj, adj + f_rec};
    GMMVI_HIP_CHECK(ctx, hipMemsetAsync(s.needed, 0, sizeof(int), ctx->stream));
    return GMMVI_OK;
}

// A gradient call.  wave_bytes(capacity): what a wave takes, affine in the capacity.  attempt(capacity, budget, scratch): plans,
// reserves (reserve_tapes) and launches at that capacity; the kernels leave the tape length they needed in scratch.needed.  The
// first attempt runs at the requested capacity, else the remembered one, else the default; a second one at what the first needed.
// Where the messages of the two modes differ: behind "holds no tape", behind "bytes for 64 lanes", behind "on the same samples".
template <class WaveBytes, class Attempt>
int tape_gradient(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, int tape_capacity, size_t scratch_bytes, WaveBytes wave_bytes,
                  Attempt attempt, int needed_floor, const std::string& no_tape, const char* lanes_with, const char* impure) {
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)GMMVI_CUSTOM_TAPE_SCRATCH_BYTES;
    // the longest tape 64 lanes can have within the budget, beside what else the wave takes
    size_t longest = budget > wave_bytes(0) ? (budget - wave_bytes(0)) / (wave_bytes(1) - wave_bytes(0)) : 0;
    if (longest > (size_t)1 << 30) longest = (size_t)1 << 30;         // node ids are ints: D + record
    if (longest < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: a scratch budget of " + std::to_string(budget) +
                                                  " bytes holds no tape" + no_tape + std::to_string(wave_bytes(1)) + " bytes");
    int cap = tape_capacity > 0 ? tape_capacity : tape_length(t, D);
    if (cap < 1) cap = GMMVI_CUSTOM_TAPE_DEFAULT_CAPACITY;
    if ((size_t)cap > longest) cap = (int)longest;                    // the launch tells what is needed: refused below if that is more
    for (int tries = 0; tries < 2; ++tries) {
        TapeScratch scratch{};
        if (const int rc = attempt(cap, budget, scratch)) return rc;
        int needed = 0;
        GMMVI_HIP_CHECK(ctx, hipMemcpyAsync(&needed, scratch.needed, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        GMMVI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (needed < needed_floor) needed = needed_floor;
        int& remembered = t->tape_lengths[D];
        if (needed > remembered) remembered = needed;
        if (needed <= cap) return GMMVI_OK;
        if ((size_t)needed > longest)
            return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the target needs a tape of " + std::to_string(needed) +
                                                      " records per lane at D = " + std::to_string(D) + ", which takes " +
                                                      std::to_string(wave_bytes(needed)) + " bytes for 64 lanes" + lanes_with +
                                                      "; the scratch budget is " + std::to_string(budget) +
                                                      " bytes (lp_out_dev is written, grad_out_dev is not complete)");
        cap = needed;
    }
    return gmmvi_fail(ctx, GMMVI_ERR_ARG, std::string("invalid argument: the tape of the target grew between two launches on the "
                                                      "same samples") + impure);
}
}  // namespace

// ---- targets differentiated on a tape ----------------------------------------------------------------------------------------
// The slab plan: a wave of 64 lanes takes 64 * capacity records of GMMVI_CUSTOM_TAPE_RECORD_BYTES (16 B of record, 4 B of
// adjoint).  As many whole waves as the budget holds form a slab; the slabs are then as even as whole waves allow, and the count
// is what that slab size needs: the last slab is never empty.
static size_t tape_wave_bytes(int capacity) { return (size_t)64 * (size_t)capacity * GMMVI_CUSTOM_TAPE_RECORD_BYTES; }

extern "C" int gmmvi_custom_tape_plan(int N, int capacity, size_t scratch_bytes, int* slabs, int* lanes_per_slab) {
    if (N < 1 || capacity < 1 || !slabs || !lanes_per_slab)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_tape_plan needs N >= 1, capacity >= 1 and two outputs");
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)GMMVI_CUSTOM_TAPE_SCRATCH_BYTES;
    const size_t fit = budget / tape_wave_bytes(capacity);
    if (fit < 1)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: a tape of " + std::to_string(capacity) + " records per lane takes " +
                                                      std::to_string(tape_wave_bytes(capacity)) + " bytes for 64 lanes, the scratch "
                                                      "budget is " + std::to_string(budget) + " bytes");
    const size_t waves = ((size_t)N + 63) / 64;
    const size_t most = fit < waves ? fit : waves;
    const size_t want = (waves + most - 1) / most;
    const size_t per = (waves + want - 1) / want;
    *lanes_per_slab = (int)(per * 64);
    *slabs = (int)((waves + per - 1) / per);
    return GMMVI_OK;
}

extern "C" int gmmvi_target_custom_tape(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                        const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int tape_capacity,
                                        size_t scratch_bytes) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    if (const int rc = gmmvi_custom_check_mode(ctx, E_TAPE, t)) return rc;
    GMMVI_ARG_CHECK(ctx, N >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG && X_dev != nullptr && lp_out_dev != nullptr);
    GMMVI_ARG_CHECK(ctx, tape_capacity >= 0);
    if (!grad_out_dev) {
        const size_t blocks = ((size_t)N + 255) / 256;
        void* args[] = {&D, &params_dev, &X_dev, &N, &lp_out_dev};
        GMMVI_PROF(ctx, "target_custom_tape");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[K_TAPE_LP], (unsigned)blocks, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
        return GMMVI_OK;
    }
    auto attempt = [&](int cap, size_t budget, TapeScratch& s) -> int {
        int slabs = 0, lanes = 0;
        if (gmmvi_custom_tape_plan(N, cap, budget, &slabs, &lanes) != GMMVI_OK)
            return gmmvi_fail(ctx, GMMVI_ERR_ARG, g_gmmvi_global_err);
        if (const int rc = reserve_tapes(ctx, (size_t)lanes / 64, cap, tape_wave_bytes(cap), s)) return rc;
        for (int slab = 0; slab < slabs; ++slab) {
            int first = slab * lanes;
            const int rest = N - first;
            const unsigned waves = (unsigned)(((rest < lanes ? rest : lanes) + 63) / 64);
            void* args[] = {&D, &params_dev, &X_dev, &N, &lp_out_dev, &grad_out_dev, &first, &s.rec, &s.adj, &cap, &s.needed};
            GMMVI_PROF(ctx, "target_custom_tape");
            GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[K_TAPE_GRAD], waves, 1, 1, 64, 1, 1, 0, ctx->stream, args, nullptr));
        }
        return GMMVI_OK;
    };
    return tape_gradient(ctx, t, D, tape_capacity, scratch_bytes, tape_wave_bytes, attempt, 0, ": one record of 64 lanes takes ", "",
                         ": gmmvi_user_density is not a pure function of x, D and params");
}

// ---- targets summed over a data set, differentiated on a tape --------------------------------------------------------------------
// The plan.  A wave (one tile of 64 samples, one chunk of the row list) takes 64 * (capacity * GMMVI_CUSTOM_TAPE_RECORD_BYTES +
// 4 D) bytes: its tape and its [D][64] gradient accumulator.  Chunks first: the request, or enough chunks that tiles * chunks
// waves reach GMMVI_DATA_TAPE_PLAN_WAVES (four waves on each compute unit of an MI355X) but no more than rows /
// GMMVI_DATA_TAPE_MIN_CHUNK_ROWS; either way at most one per row and at most as many as the budget holds waves, then as even as
// whole rows allow.  Then slabs: as many tiles as the budget holds with that many chunks each, as even as whole tiles allow.
// Neither constant is measured: they restate the rule of gmmvi_custom_data_plan for one-wave workgroups.
constexpr int64_t GMMVI_DATA_TAPE_PLAN_WAVES = 4 * GMMVI_DATA_PLAN_CUS;
constexpr int64_t GMMVI_DATA_TAPE_MIN_CHUNK_ROWS = 8;

static size_t data_tape_wave_bytes(int D, int capacity) {
    return (size_t)64 * ((size_t)capacity * GMMVI_CUSTOM_TAPE_RECORD_BYTES + 4 * (size_t)D);
}

extern "C" int gmmvi_custom_data_tape_plan(int N, int64_t rows, int D, int capacity, int chunks_requested, size_t scratch_bytes,
                                           int* chunks, int* rows_per_chunk, int* slabs, int* tiles_per_slab) {
    if (N < 1 || rows < 1 || rows > 2147483647ll || D < 1 || D > GMMVI_MAX_DIM_DIAG || capacity < 1 || chunks_requested < 0 ||
        !chunks || !rows_per_chunk || !slabs || !tiles_per_slab)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_tape_plan needs N >= 1, 1 <= rows < 2^31, "
                                                  "1 <= D <= " + std::to_string(GMMVI_MAX_DIM_DIAG) + ", capacity >= 1, "
                                                  "chunks_requested >= 0 and four outputs");
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)GMMVI_CUSTOM_TAPE_SCRATCH_BYTES;
    const size_t wave = data_tape_wave_bytes(D, capacity);
    const int64_t fit = (int64_t)(budget / wave);                    // waves the budget holds
    if (fit < 1)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: a tape of " + std::to_string(capacity) + " records per lane and "
                                                      "the gradient accumulator at D = " + std::to_string(D) + " take " +
                                                      std::to_string(wave) + " bytes for 64 lanes, the scratch budget is " +
                                                      std::to_string(budget) + " bytes");
    const int64_t tiles = ((int64_t)N + 63) / 64;
    int64_t want = chunks_requested;
    if (want == 0) {
        const int64_t fill = (GMMVI_DATA_TAPE_PLAN_WAVES + tiles - 1) / tiles;
        const int64_t most = rows / GMMVI_DATA_TAPE_MIN_CHUNK_ROWS;
        want = fill < most ? fill : most;
    }
    if (want > rows) want = rows;
    if (want > GMMVI_DATA_MAX_CHUNKS) want = GMMVI_DATA_MAX_CHUNKS;
    if (want > fit) want = fit;
    if (want < 1) want = 1;
    const int64_t per = (rows + want - 1) / want;
    const int64_t count = (rows + per - 1) / per;
    const int64_t hold = fit / count < tiles ? fit / count : tiles;  // tiles a slab can hold, >= 1
    const int64_t need = (tiles + hold - 1) / hold;
    const int64_t each = (tiles + need - 1) / need;
    *chunks = (int)count;
    *rows_per_chunk = (int)per;
    *tiles_per_slab = (int)each;
    *slabs = (int)((tiles + each - 1) / each);
    return GMMVI_OK;
}

// gmmvi_target_custom_data_tape (E_DATA_TAPE) and gmmvi_target_custom_data_tape_own_batches (E_DATA_TAPE_OWN, minibatch == 1)
static int target_custom_data_tape(Entry entry, gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                   const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed, uint32_t call,
                                   const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int chunks_requested,
                                   int tape_capacity, size_t scratch_bytes) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    if (const int rc = gmmvi_custom_check_mode(ctx, entry, t)) return rc;
    if (const int rc = gmmvi_custom_check_data_arguments(ctx, D, data_dev, T, C, minibatch, B, X_dev, N, lp_out_dev, chunks_requested))
        return rc;
    GMMVI_ARG_CHECK(ctx, tape_capacity >= 0);
    const bool own = entry == E_DATA_TAPE_OWN;
    if (own) minibatch = GMMVI_DATA_OWN_BATCHES;
    if (!grad_out_dev)                                               // the data mode's value call: its kernels, its plan, its bits
        return gmmvi_custom_launch_data(ctx, t, D, params_dev, data_dev, T, C, minibatch, B, seed, call, X_dev, N, lp_out_dev, nullptr,
                                        chunks_requested);
    const int64_t length = minibatch ? B : T;
    RowList l{C, (unsigned)T, minibatch, (unsigned)length, 0u, call, gmmvi_feistel_half_bits((uint32_t)T), (unsigned)seed,
              (unsigned)(seed >> 32)};
    float scale = minibatch ? (float)T / (float)B : 1.f;
    auto wave_bytes = [D](int capacity) { return data_tape_wave_bytes(D, capacity); };
    auto attempt = [&](int cap, size_t budget, TapeScratch& s) -> int {
        int chunks = 0, per = 0, slabs = 0, tiles_per_slab = 0;
        if (gmmvi_custom_data_tape_plan(N, length, D, cap, chunks_requested, budget, &chunks, &per, &slabs, &tiles_per_slab) != GMMVI_OK)
            return gmmvi_fail(ctx, GMMVI_ERR_ARG, g_gmmvi_global_err);
        l.rows_per_chunk = (unsigned)per;
        if (const int rc = reserve_tapes(ctx, (size_t)tiles_per_slab * (size_t)chunks, cap, wave_bytes(cap), s)) return rc;
        const int tiles = (N + 63) / 64;
        for (int slab = 0; slab < slabs; ++slab) {
            int first_tile = slab * tiles_per_slab;
            const unsigned here = (unsigned)(tiles - first_tile < tiles_per_slab ? tiles - first_tile : tiles_per_slab);
            {
                void* args[] = {&D, &params_dev, &X_dev, &N, &data_dev, &l, &first_tile, &s.rec, &s.adj, &s.acc, &cap, &s.needed};
                GMMVI_PROF(ctx, own ? "target_custom_data_tape_own" : "target_custom_data_tape");
                GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[own ? K_DATA_TAPE_ROWS_OWN : K_DATA_TAPE_ROWS], here, (unsigned)chunks, 1,
                                                           64, 1, 1, 0, ctx->stream, args, nullptr));
            }
            {
                void* args[] = {&D, &params_dev, &X_dev, &N, &chunks, &scale, &first_tile, &s.rec, &s.adj, &s.acc, &cap, &s.needed,
                                &lp_out_dev, &grad_out_dev};
                GMMVI_PROF(ctx, "target_custom_data_tape_finish");
                GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[K_DATA_TAPE_FINISH], here, 1, 1, 64, 1, 1, 0, ctx->stream, args, nullptr));
            }
        }
        return GMMVI_OK;
    };
    // floor 1: constants alone leave no record, but one slot still carries the chunk's value
    return tape_gradient(ctx, t, D, tape_capacity, scratch_bytes, wave_bytes, attempt, 1,
                         " at D = " + std::to_string(D) + ": one record and the gradient accumulator of 64 lanes take ",
                         " with their gradient accumulator",
                         " and rows: gmmvi_user_row or gmmvi_user_prior is not a pure function of x, D, the row and params");
}

extern "C" int gmmvi_target_custom_data_tape(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                             const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed,
                                             uint32_t call, const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                             int chunks_requested, int tape_capacity, size_t scratch_bytes) {
    return target_custom_data_tape(E_DATA_TAPE, ctx, t, D, params_dev, data_dev, T, C, minibatch, B, seed, call, X_dev, N, lp_out_dev,
                                   grad_out_dev, chunks_requested, tape_capacity, scratch_bytes);
}

extern "C" int gmmvi_target_custom_data_tape_own_batches(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D,
                                                         const float* params_dev, const float* data_dev, int64_t T, int C, int64_t B,
                                                         uint64_t seed, uint32_t call, const float* X_dev, int N, float* lp_out_dev,
                                                         float* grad_out_dev, int chunks_requested, int tape_capacity,
                                                         size_t scratch_bytes) {
    return target_custom_data_tape(E_DATA_TAPE_OWN, ctx, t, D, params_dev, data_dev, T, C, 1, B, seed, call, X_dev, N, lp_out_dev,
                                   grad_out_dev, chunks_requested, tape_capacity, scratch_bytes);
}
