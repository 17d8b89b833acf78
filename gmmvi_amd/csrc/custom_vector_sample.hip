// Build-time check of the vector primitives of user-defined targets (custom_target_vector.inc and their overloads in the two
// number types) behind the reverse-mode kernels of targets summed over a data set: the Makefile compiles the texts of
// custom_data_tape_sample.hip behind the same logistic regression written with gmmvi_dot and gmmvi_sumsq, as custom_target.hip
// composes them at run time and with the flags of the library.  A mistake in the text fails the build, and the register / scratch /
// LDS use of gmmvi_data_tape_rows with the vector branch of the sweep taken can be read from build/custom_vector_sample.s
// (kernel table), next to what build/custom_data_tape_sample.s gives for the scalar loops.  Nothing of the device code
// is linked into the library.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

__host__ __device__ inline float gmmvi_value(float);
__host__ __device__ inline float gmmvi_dot(const float*, int, const float*, int);
__host__ __device__ inline float gmmvi_sumsq(const float*, int, int, float);

// the logistic regression of the test suite: row = [features (D) | label +-1], prior N(params[0], params[1]^2) per coordinate
template <class T, class X>
__host__ __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T z = gmmvi_dot(x, 0, row, D);
    z *= row[D];
    return -(fmax(-z, 0.f) + log1p(exp(-fabs(z))));
}

template <class T, class X>
__host__ __device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    return -0.5f * gmmvi_sumsq(x, 0, D, m) / (s * s) - D * (logf(s) + 0.9189385332046727f);
}

#define GMMVI_TAPE_NO_KERNELS
#define GMMVI_AD_NO_ADAPTER
#define GMMVI_WRAP_TILE_ONLY
#define GMMVI_TAPE_NO_FLOAT_VALUE
#include "build/custom_target_special_text.inc"
#include "build/custom_target_autodiff_text.inc"
#include "build/custom_target_wrap_text.inc"
#include "feistel.h"
#include "build/custom_target_data_text.inc"
#include "build/custom_target_tape_text.inc"
#include "build/custom_target_data_tape_text.inc"
