// Build-time check of the dual-number text of differentiated user-defined targets (custom_target_autodiff.inc): the Makefile
// compiles that text and the wrapper text behind this small value-only density with the flags of the library, so that a mistake
// in the dual text fails the build and the register / scratch / LDS use of the four kernels on gfx950 can be read from
// build/custom_autodiff_sample.s (kernel table).  Nothing of this file is linked into the library.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

// a Gaussian with a diagonal precision times a logistic factor per coordinate: params = [m (D) | p (D)]
template <class T, class X>
__device__ T gmmvi_user_density(X x, int D, const float* params) {
    T lp = 0.f;
    for (int i = 0; i < D; ++i) {
        const T d = x[i] - params[i];
        lp -= 0.5f * params[D + i] * d * d + log1p(exp(-d));
    }
    return lp;
}

#include "build/custom_target_special_text.inc"
#include "build/custom_target_autodiff_text.inc"
#include "build/custom_target_wrap_text.inc"
