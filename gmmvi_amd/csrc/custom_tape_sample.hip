// Build-time check of the tape text of reverse-mode user-defined targets (custom_target_tape.inc): the Makefile compiles that
// text behind this small density with the flags of the library, so that a mistake in it fails the build and the register /
// scratch / LDS use of its two kernels on gfx950 can be read from build/custom_tape_sample.s (kernel table).  Nothing
// of this file is linked into the library.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

__host__ __device__ inline float gmmvi_value(float);

// the density of custom_autodiff_sample.hip: a Gaussian with a diagonal precision times a logistic factor per coordinate
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
#include "build/custom_target_tape_text.inc"
