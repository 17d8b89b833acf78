// Build-time check of the reverse-mode kernels of user-defined targets summed over a data set (custom_target_data_tape.inc): the
// Makefile compiles that text behind this small row term and prior, with the whole text of the data mode and the tape's number
// type in front of it, as custom_target.hip composes them at run time and with the flags of the library.  A mistake in the text
// fails the build, and the register / scratch / LDS use of the kernels on gfx950 can be read from
// build/custom_data_tape_sample.s (kernel table).  Nothing of the device code is linked into the library;
// data_tape_probe.hip includes this file with GMMVI_DATA_TAPE_PROBE to run the same row term and prior behind the lane bodies
// on the host.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

__host__ __device__ inline float gmmvi_value(float);

// the logistic regression of the test suite: row = [features (D) | label +-1], prior N(params[0], params[1]^2) per coordinate
template <class T, class X>
__host__ __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T z = 0.f;
    for (int i = 0; i < D; ++i) z += row[i] * x[i];
    z *= row[D];
    return -(fmax(-z, 0.f) + log1p(exp(-fabs(z))));
}

template <class T, class X>
__host__ __device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    T q = 0.f;
    for (int i = 0; i < D; ++i) {
        const T r = (x[i] - m) / s;
        q += r * r;
    }
    return -0.5f * q - D * (logf(s) + 0.9189385332046727f);
}

#define GMMVI_TAPE_NO_KERNELS
#include "build/custom_target_special_text.inc"
#ifndef GMMVI_DATA_TAPE_PROBE
#define GMMVI_AD_NO_ADAPTER
#define GMMVI_WRAP_TILE_ONLY
#define GMMVI_TAPE_NO_FLOAT_VALUE
#include "build/custom_target_autodiff_text.inc"
#include "build/custom_target_wrap_text.inc"
#include "feistel.h"
#include "build/custom_target_data_text.inc"
#endif
#include "build/custom_target_tape_text.inc"
#include "build/custom_target_data_tape_text.inc"
