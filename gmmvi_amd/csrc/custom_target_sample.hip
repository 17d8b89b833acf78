// Build-time check of the wrapper kernels of user-defined targets (custom_target_wrap.inc): the Makefile compiles the wrapper
// text behind this small user function with the flags of the library, so that a mistake in the wrapper fails the build and the
// wrapper's register / scratch / LDS use on gfx950 can be read from build/custom_target_sample.s (kernel table).
// Nothing of this file is linked into the library.
#include <hip/hip_runtime.h>

// log density of a Gaussian with a diagonal precision: params = [m (D) | p (D)]
__device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    float lp = 0.f;
    for (int i = 0; i < D; ++i) {
        const float d = x[i] - params[i];
        lp -= 0.5f * params[D + i] * d * d;
        if (grad) grad[i] = -params[D + i] * d;
    }
    return lp;
}

#include "build/custom_target_wrap_text.inc"
