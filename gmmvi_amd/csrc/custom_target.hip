// gmmvi_target_custom: the wrapper kernels (custom_target_wrap.inc) of a user-defined target with a hand-written or a dual-number
// gradient, which custom_compile.hip compiled at run time; the entry of target kind 5 of both iteration plans (fused.hip).
#include "custom_target.h"

extern "C" int gmmvi_target_custom(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                   const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int route) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    GMMVI_ARG_CHECK(ctx, N >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG && X_dev != nullptr && lp_out_dev != nullptr);
    GMMVI_ARG_CHECK(ctx, route >= 0 && route <= 2);
    if (const int rc = gmmvi_custom_check_mode(ctx, E_TARGET, t)) return rc;
    if (route == 1 && D > GMMVI_CUSTOM_STAGED_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: route 1 (staged) needs D <= " +
                                                  std::to_string(GMMVI_CUSTOM_STAGED_MAX_DIM) + ", got D = " + std::to_string(D));
    if (t->mode == MODE_AUTODIFF && grad_out_dev != nullptr && D > GMMVI_CUSTOM_AUTODIFF_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the gradient of a differentiated target needs D <= " +
                                                  std::to_string(GMMVI_CUSTOM_AUTODIFF_MAX_DIM) + ", got D = " + std::to_string(D) +
                                                  " (values only, or a hand-written gradient, run above)");
    const bool staged = route == 1 || (route == 0 && D <= GMMVI_CUSTOM_STAGED_MAX_DIM);
    const bool want_grad = grad_out_dev != nullptr;
    const unsigned threads = staged ? 64u : 256u;
    const size_t blocks = ((size_t)N + threads - 1) / threads;
    GMMVI_ARG_CHECK(ctx, blocks <= 2147483647u);
    const size_t lds = staged ? (size_t)(want_grad ? 2 : 1) * 64 * (size_t)(D | 1) * sizeof(float) : 0;   // <= 61952 B
    void* args[] = {&D, &params_dev, &X_dev, &N, &lp_out_dev, &grad_out_dev};
    GMMVI_PROF(ctx, staged ? "target_custom_staged" : "target_custom_direct");
    const KernelSlot slot = staged ? (want_grad ? K_STAGED_GRAD : K_STAGED_LP) : (want_grad ? K_DIRECT_GRAD : K_DIRECT_LP);
    GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[slot], (unsigned)blocks, 1, 1, threads, 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
    return GMMVI_OK;
}
