// Build-time check of the special functions of user-defined targets (custom_target_special.inc and their rules in the dual-number
// text): the Makefile compiles the kernels of the data mode behind this negative-binomial row term and prior, composed as
// custom_target.hip composes them at run time and with the flags of the library.  A mistake in the texts fails the build, and what
// lgamma, digamma and the log-sigmoid cost in registers and scratch on gfx950 can be read from build/custom_special_sample.s
// beside build/custom_data_sample.s (kernel table).  Nothing of this file is linked into the library.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

__host__ __device__ inline float gmmvi_value(float); __host__ __device__ inline float gmmvi_digamma(float);
__host__ __device__ inline float gmmvi_trigamma(float); __host__ __device__ inline float gmmvi_sigmoid(float);
__host__ __device__ inline float gmmvi_softplus(float); __host__ __device__ inline float gmmvi_log_sigmoid(float);
__host__ __device__ inline float gmmvi_logaddexp(float, float);

// negative-binomial regression: row = [features (D - 1) | count y], log mean eta = features . x[0 .. D - 2], dispersion
// r = softplus(x[D - 1]); prior N(params[0], params[1]^2) per coordinate
template <class T, class X>
__device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    T eta = 0.f;
    for (int i = 0; i < D - 1; ++i) eta += row[i] * x[i];
    const float y = row[D - 1];
    const T r = gmmvi_softplus(x[D - 1]);
    const T u = log(r) - eta;
    return lgamma(y + r) - lgamma(r) - lgammaf(y + 1.f) + r * gmmvi_log_sigmoid(u) + y * gmmvi_log_sigmoid(-u);
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
