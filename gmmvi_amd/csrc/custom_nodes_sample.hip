// Build-time check of the primitives on arrays of the number type (gmmvi_wdot and gmmvi_logsumexp: custom_target_vector.inc and
// their overloads in the two number types) behind the reverse-mode kernels of targets summed over a data set: the Makefile
// compiles the texts of custom_data_tape_sample.hip behind a multinomial (softmax) regression whose normaliser is one
// gmmvi_logsumexp over a local array of class scores, as custom_target.hip composes them at run time and with the flags of the
// library.  A mistake in the text fails the build, and the register / scratch / LDS use of gmmvi_data_tape_rows with the
// node-array branch of the sweep taken can be read from build/custom_nodes_sample.s (kernel table).  The local array
// is read at a run-time index (z[label]): where the compiler places it is the array's matter, not the primitive's.  Nothing of
// the device code is linked into the library.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

__host__ __device__ inline float gmmvi_value(float);
__host__ __device__ inline float gmmvi_dot(const float*, int, const float*, int);
__host__ __device__ inline float gmmvi_sumsq(const float*, int, int, float);
__host__ __device__ inline float gmmvi_wdot(const float*, int, const float*, int);
__host__ __device__ inline float gmmvi_logsumexp(const float*, int);

// the softmax regression of the test suite: row = [features (F) | label], C = F + 1; x holds K = D / C blocks [weights (F) | bias]
template <class T, class X>
__host__ __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, K = D / C;
    T z[16];
    for (int k = 0; k < K; ++k) z[k] = gmmvi_dot(x, k * C, row, F) + x[k * C + F];
    return z[(int)row[F]] - gmmvi_logsumexp(z, K);
}

template <class T, class X>
__host__ __device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    return -0.5f * gmmvi_sumsq(x, 0, D, m) / (s * s) - D * (logf(s) + 0.9189385332046727f);
}

#define GMMVI_TAPE_NO_KERNELS
#define GMMVI_TAPE_NODES 1                                       // the overloads and the sweep of the node-array record
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
