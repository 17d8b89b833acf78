// Component packing, the batched Cholesky factorisation and the entry points of the register-path density sweeps: the choice
// of a sweep's route (density_sweep.h: one file per route) and the launch tail all routes share.
#include "density_sweep.h"
#include "blocked.h"
#include <cmath>
#include <cstdlib>

// ---------------------------------------------------------------------------------------------------------------
// pack: (means, chols) -> kernel-side blocks; optional explicit inverse (sample_db.py:121)
// ---------------------------------------------------------------------------------------------------------------
template <int DP>
__global__ __launch_bounds__(64) void pack_kernel(int family, float nu, int K, int D, const float* __restrict__ means,
                                                  const float* __restrict__ chols, float* __restrict__ packed,
                                                  float* __restrict__ inv_chols) {
    using P = Pack<DP>;
    const int k = blockIdx.x;
    const int t = threadIdx.x;
    const float* L = chols + (size_t)k * D * D;
    float* out = packed + (size_t)k * P::STRIDE;
    for (int i = t; i < DP; i += 64) {
        out[P::MU + i] = i < D ? means[(size_t)k * D + i] : 0.f;
        out[P::RD + i] = i < D ? 1.f / L[i * D + i] : 1.f;
    }
    for (int e = t; e < DP * DP; e += 64) {
        int i = e / DP, j = e % DP;
        if (j < i) {
            float v = (i < D) ? L[i * D + j] : 0.f;
            out[P::LROW + P::rowofs(i) + j] = v;
            out[P::LCOL + P::colofs(j) + (i - j - 1)] = v;      // entry (row i, col j) lives in column j
        }
    }
    if (t == 0) {
        float s = 0.f;
        for (int i = 0; i < D; ++i) s += logf(L[i * D + i]);
        float c;
        if (family == GMMVI_GAUSS)
            c = -s - 0.5f * D * 1.8378770664093453f;             // log(2 pi)
        else
            c = lgammaf(0.5f * (nu + D)) - lgammaf(0.5f * nu) - 0.5f * D * logf(nu * 3.14159265358979f) - s;
        out[P::CONST] = c;
        for (int i = P::CONST + 1; i < P::FWD; ++i) out[i] = 0.f;
        out[P::SWH + DP] = c;
    }
    gmmvi_write_sweep_stream(out, DP, D, L, D, means + (size_t)k * D, t, 64);
    // L^-1: lane t solves L x = e_t (column t) by forward substitution; the dense inverse is staged in LDS, from where the
    // matrix-core fragments of the block (common.h) and the optional explicit inverse (sample_db.py:121) are written
    __shared__ float Li[DP * DP];
    if (P::FRAGS || inv_chols != nullptr) {
        float x[DP];
#pragma unroll
        for (int i = 0; i < DP; ++i) {
            float sacc = (i == t) ? 1.f : 0.f;
            if (i < D && t < D) {
                for (int j = 0; j < i; ++j) sacc -= L[i * D + j] * x[j];
                x[i] = sacc / L[i * D + i];
            } else {
                x[i] = 0.f;
            }
        }
        if (t < DP) {
#pragma unroll
            for (int i = 0; i < DP; ++i) Li[i * DP + t] = (i >= t) ? x[i] : 0.f;
        }
    }
    __syncthreads();
    if (P::FRAGS) gmmvi_write_inverse_fragments(out, DP, D, Li, DP, t, 64);
    if (inv_chols != nullptr) {
        float* inv = inv_chols + (size_t)k * D * D;
        for (int e = t; e < D * D; e += 64) inv[e] = Li[(e / D) * DP + (e % D)];
    }
}

// ---------------------------------------------------------------------------------------------------------------
// batched Cholesky for model construction / add_component (full_cov_gmm.py:23,:64-68)
// ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void cholesky_kernel(int D, const float* __restrict__ covs, float* __restrict__ chols,
                                                      int32_t* __restrict__ ok) {
    extern __shared__ float sm[];
    const int k = blockIdx.x, t = threadIdx.x;
    const int ld = D + 1;
    for (int e = t; e < D * D; e += 64) sm[(e / D) * ld + (e % D)] = covs[(size_t)k * D * D + e];
    __syncthreads();
    bool good = true;
    for (int j = 0; j < D; ++j) {
        float s = 0.f;
        if (t >= j && t < D) {
            s = sm[t * ld + j];
            for (int c = 0; c < j; ++c) s -= sm[t * ld + c] * sm[j * ld + c];
        }
        float p = __shfl(s, j);
        if (!(p > 0.f)) { good = false; break; }
        float d = sqrtf(p);
        __syncthreads();
        if (t == j) sm[t * ld + j] = d;
        else if (t > j && t < D) sm[t * ld + j] = s / d;
        __syncthreads();
    }
    for (int e = t; e < D * D; e += 64) {
        int i = e / D, j = e % D;
        float v = (j <= i) ? sm[i * ld + j] : 0.f;
        chols[(size_t)k * D * D + e] = good ? v : __builtin_nanf("");
    }
    if (t == 0 && ok) ok[k] = good ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------
// mixture_eval
// ---------------------------------------------------------------------------------------------------------------
// profile name of a density launch: the caller's tag (fused.hip knows which sweep of the iteration it issues), else by shape:
// the dual sweep (model + background over the same components), a sweep with the gradient (target evaluation or model
// density + gradient), a log-value sweep (post-update densities)
static const char* sweep_prof_name(const gmmvi_ctx* ctx, bool want_grad, bool dual) {
    if (ctx->prof_tag) return ctx->prof_tag;
    return dual ? "sweep_dual" : (want_grad ? "sweep_grad" : "sweep_values");
}

// The launch of a sweep once its route has chosen the geometry and the kernel instance.  The order of the steps is what the
// single-call iteration (fused.hip) relies on: which extra workgroups a sweep carries, their order, where a deferred merge is left.
int gmmvi_sweep_launch(gmmvi_ctx* ctx, const SweepArgs& a, const SweepGeom& g, SweepKernel kernel) {
    const int N = a.N, D = a.D, ky = g.ky;
    const bool want_grad = a.grad != nullptr;
    const bool want_merge = want_grad || a.lp != nullptr;
    size_t shmem = g.shmem;
    float* lp_k = a.lp;
    float* grad_k = a.grad;
    float* lp2_k = a.lp2;
    // the merge of the chunk partials: its own launch, or (single-call iteration) left to the next launch
    const bool defer = ctx->defer_combine && ky > 1 && want_merge;
    if (defer) {
        int rc = gmmvi_flush_pending_combine(ctx);
        if (rc != GMMVI_OK) return rc;
    }
    if (ky > 1 && want_merge) {
        size_t need = ((size_t)ky * N * (a.logw2 ? 2 : 1) + (want_grad ? (size_t)ky * N * D : 0)) * sizeof(float);
        int rc = defer ? gmmvi_defer_reserve(ctx, need) : gmmvi_ws_reserve(ctx, need);
        if (rc != GMMVI_OK) return rc;
        lp_k = (float*)(defer ? ctx->defer_ws : ctx->ws);
        lp2_k = a.logw2 ? lp_k + (size_t)ky * N : nullptr;
        grad_k = want_grad ? lp_k + (size_t)ky * N * (a.logw2 ? 2 : 1) : nullptr;
    }
    // block order: the launch's own tiles, the riders (the stepsize block first: it is the longest of them), the carried merge
    const Riders riders = gmmvi_take_pending_riders(ctx, g.tiles, g.threads);
    const CombineJob carried = gmmvi_take_pending_combine(ctx, g.threads, g.tiles + riders.prep_blocks + riders.sample_blocks);
    if (riders_lds_bytes(riders) > shmem) shmem = riders_lds_bytes(riders);
    dim3 grid(g.tiles + carried.blocks + riders.prep_blocks + riders.sample_blocks, ky), block(g.threads);
    {
        GMMVI_PROF_UNITS(ctx, sweep_prof_name(ctx, want_grad, a.logw2 != nullptr), (double)N * a.K);
        if (shmem > 64 * 1024)
            GMMVI_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shmem));
        hipLaunchKernelGGL(kernel, grid, block, shmem, ctx->stream, a.nu, a.K, D, a.packed, a.logw, a.X, N, a.ld, lp_k, grad_k,
                           a.logw2, lp2_k, carried, riders);
    }
    GMMVI_LAUNCH_CHECK(ctx);
    if (defer) {
        CombineJob& j = ctx->pending;
        j.R = ky; j.N = N; j.D = D;
        j.lp_parts = lp_k; j.grad_parts = grad_k; j.lp2_parts = lp2_k;
        j.lp_out = a.lp; j.grad_out = a.grad; j.lp2_out = lp2_k ? a.lp2 : nullptr;
    } else if (ky > 1 && want_merge) {
        GMMVI_PROF(ctx, "mixture_combine");
        int rc = gmmvi_combine_partials_internal(ctx, ky, N, D, lp_k, grad_k, a.lp, a.grad, lp2_k, a.lp2);
        if (rc != GMMVI_OK) return rc;
    }
    return GMMVI_OK;
}

// the route of a sweep at padded dimension dp
static int sweep_route(gmmvi_ctx* ctx, int dp, const SweepArgs& a) {
    const bool frags = dp >= GMMVI_MFMA_DENSITY_FROM_DP;       // Pack<dp>::FRAGS
    {
        // enough (128-sample tile, component) passes to give every SIMD a few: the packed kernel; otherwise the one-sample
        // kernel, whose 64-sample tiles spread a small problem over more CUs (GMMVI_ME_PK: 0 never, 1 always).
        // Padded D >= 32 (GMMVI_ME_PK_WIDE, experiments): the triangular substitution on the packed vector unit does D^2 / 2
        // multiply-adds per pair and side where the matrix-core kernels multiply whole 16 x 4 fragments of the explicit inverse
        static const int env_pk = getenv("GMMVI_ME_PK") ? atoi(getenv("GMMVI_ME_PK")) : -1;
        static const long env_pk_min = getenv("GMMVI_ME_PK_MIN") ? atol(getenv("GMMVI_ME_PK_MIN")) : 4096;
        static const int env_pk_wide = getenv("GMMVI_ME_PK_WIDE") ? atoi(getenv("GMMVI_ME_PK_WIDE")) : 1;
        const long passes = (long)((a.N + 127) / 128) * a.K;
        // measured inside the iteration at K = 100, N = 10^4 (profiles/r04_notes.md): without the gradient the packed kernel wins
        // at D = 40 / 50 (post-update sweep 41.9 -> 33.0 / 53.1 -> 45.7 us; D = 32: 25.8 / 26.1), with the gradient at D = 32 / 40
        // (dual sweep 57.5 -> 52.3 / 79.9 -> 74.4) but not at D = 50 (99 -> 115: 223 registers = two waves per SIMD)
        const bool shape_ok = !frags || (env_pk_wide && (a.grad == nullptr || dp <= 40));
        if (dp <= 50 && shape_ok && env_pk != 0 && (env_pk == 1 || passes >= env_pk_min)) return gmmvi_sweep_pk(ctx, dp, a);
    }
    if (!frags) return gmmvi_sweep_reg(ctx, dp, a);
    // enough samples for the workgroup-shared form (eight waves on one component at a time): the block goes to LDS once per
    // workgroup instead of to every wave through the L2
    // (with the gradient: C3 dual sweep 150 -> 107 us; without it the sweep is bound by the log-sum-exp tails of the 16-sample
    // sub-tiles, not by the fragment traffic, and stays on the per-wave kernel: 61 against 59 us)
    static const int env_ws = getenv("GMMVI_ME_WS") ? atoi(getenv("GMMVI_ME_WS")) : -1;      // experiments: 0 off, else on
    const bool ws = env_ws != 0;
    if (ws && a.N >= 2048 && a.K >= 16 && a.grad != nullptr) return gmmvi_sweep_mfma_ws(ctx, dp, a);
    // sub-tiles of 16 samples per wave pass: four (every fragment fetch of a component serves 64 samples) unless the
    // gradient state of the wide dimensions would not fit the registers
    // (D = 40 with the gradient: 60 us at two sub-tiles, 82 us at four)
    return gmmvi_sweep_mfma(ctx, dp, dp >= 40 && a.grad != nullptr ? 2 : 4, a);
}

// C++ linkage (common.h): the register-path block layout (Pack<padded D>) whatever the blocked threshold says -- gmmvi_more
// reads that layout and re-packs the components of a blocked-path dimension (50 < D <= 63 by default) for its call
int gmmvi_pack_register_layout(gmmvi_ctx* ctx, int K, int D, const float* means_dev, const float* chols_dev, float* packed_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 1 && D >= 1 && D <= GMMVI_MAX_DIM && means_dev && chols_dev && packed_dev);
    int dp = gmmvi_padded_dim(D);
    GMMVI_DISPATCH_DP(dp, hipLaunchKernelGGL((pack_kernel<DP>), dim3(K), dim3(64), 0, ctx->stream, (int)GMMVI_GAUSS, 0.f, K, D,
                                             means_dev, chols_dev, packed_dev, (float*)nullptr));
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

extern "C" {

int gmmvi_pack_components(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* means_dev,
                          const float* chols_dev, float* packed_dev, float* inv_chols_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 0 && D >= 1 && D <= GMMVI_BLOCKED_MAX_DIM);
    GMMVI_ARG_CHECK(ctx, family == GMMVI_GAUSS || family == GMMVI_STUDENT_T);
    if (K == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, means_dev && chols_dev && packed_dev);
    if (gmmvi_is_blocked_dim(D)) return gmmvi_blocked_pack(ctx, family, nu, K, D, means_dev, chols_dev, packed_dev, inv_chols_dev);
    int dp = gmmvi_padded_dim(D);
    GMMVI_PROF(ctx, "pack_components");
    GMMVI_DISPATCH_DP(dp, hipLaunchKernelGGL((pack_kernel<DP>), dim3(K), dim3(64), 0, ctx->stream, family, nu, K, D,
                                             means_dev, chols_dev, packed_dev, inv_chols_dev));
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_cholesky(gmmvi_ctx* ctx, int K, int D, const float* covs_dev, float* chols_dev, int32_t* ok_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 0 && D >= 1 && D <= GMMVI_BLOCKED_MAX_DIM);
    if (K == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, covs_dev && chols_dev);
    if (gmmvi_is_blocked_dim(D)) return gmmvi_blocked_cholesky(ctx, K, D, covs_dev, chols_dev, ok_dev);
    hipLaunchKernelGGL(cholesky_kernel, dim3(K), dim3(64), (size_t)D * (D + 1) * 4, ctx->stream, D, covs_dev,
                       chols_dev, ok_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_mixture_eval(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* packed_dev,
                       const float* logw_dev, const float* X_dev, int N, float* ld_out_dev, float* lp_out_dev,
                       float* grad_out_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 1 && D >= 1 && D <= GMMVI_BLOCKED_MAX_DIM && N >= 0);
    GMMVI_ARG_CHECK(ctx, family == GMMVI_GAUSS || family == GMMVI_STUDENT_T);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, packed_dev && logw_dev && X_dev);
    GMMVI_ARG_CHECK(ctx, ld_out_dev || lp_out_dev || grad_out_dev);
    if (gmmvi_is_blocked_dim(D))
        return gmmvi_blocked_mixture_eval(ctx, family, nu, K, D, packed_dev, logw_dev, nullptr, X_dev, N, ld_out_dev, lp_out_dev,
                                          grad_out_dev, nullptr);
    return sweep_route(ctx, gmmvi_padded_dim(D), SweepArgs{family, nu, K, D, packed_dev, logw_dev, X_dev, N, ld_out_dev, lp_out_dev,
                                                           grad_out_dev, nullptr, nullptr});
}

int gmmvi_mixture_eval_dual(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* packed_dev,
                            const float* logw_dev, const float* logw2_dev, const float* X_dev, int N, float* ld_out_dev,
                            float* lp_out_dev, float* grad_out_dev, float* lp2_out_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 1 && D >= 1 && D <= GMMVI_BLOCKED_MAX_DIM && N >= 0);
    GMMVI_ARG_CHECK(ctx, family == GMMVI_GAUSS || family == GMMVI_STUDENT_T);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, packed_dev && logw_dev && logw2_dev && X_dev && lp_out_dev && lp2_out_dev);
    if (gmmvi_is_blocked_dim(D))
        return gmmvi_blocked_mixture_eval(ctx, family, nu, K, D, packed_dev, logw_dev, logw2_dev, X_dev, N, ld_out_dev,
                                          lp_out_dev, grad_out_dev, lp2_out_dev);
    return sweep_route(ctx, gmmvi_padded_dim(D), SweepArgs{family, nu, K, D, packed_dev, logw_dev, X_dev, N, ld_out_dev, lp_out_dev,
                                                           grad_out_dev, logw2_dev, lp2_out_dev});
}

}  // extern "C"
