// Build-time check of the kernels of user-defined targets summed over a data set (custom_target_data.inc): the Makefile compiles
// that text behind this small row term and prior, with the dual-number text (no adapter), the tile mover of the wrapper text
// and the Feistel stream in front of it, as custom_target.hip composes them at run time and with the flags of the library.  A
// mistake in the text fails the build, and the register / scratch / LDS use of the nine kernels (the six of the target, the three
// of its predictive density) on gfx950 can be read from
// build/custom_data_sample.s (kernel table).  Nothing of this file is linked into the library.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

__host__ __device__ inline float gmmvi_value(float);

// logistic regression: row = [features (D) | label +-1], prior N(params[0], params[1]^2) per coordinate
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T z = 0.f;
    for (int i = 0; i < D; ++i) z += row[i] * x[i];
    z *= row[D];
    return -(fmax(-z, 0.f) + log1p(exp(-fabs(z))));
}

template <class T, class X>
__device__ T gmmvi_user_prior(X x, int D, const float* params) {
    T lp = 0.f;
    for (int i = 0; i < D; ++i) {
        const T d = (x[i] - params[0]) / params[1];
        lp -= 0.5f * d * d;
    }
    return lp;
}

#define GMMVI_AD_NO_ADAPTER
#define GMMVI_WRAP_TILE_ONLY
#include "build/custom_target_special_text.inc"
#include "build/custom_target_autodiff_text.inc"
#include "build/custom_target_wrap_text.inc"
#include "feistel.h"
#include "build/custom_target_data_text.inc"
