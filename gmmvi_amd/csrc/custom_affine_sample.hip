// Build-time check of gmmvi_affine (custom_target_vector.inc and its overloads in the two number types) behind the reverse-mode
// kernels of targets summed over a data set: the Makefile compiles the texts of custom_data_tape_sample.hip behind a network with
// two hidden layers, three gmmvi_affine calls per row, as custom_target.hip composes them at run time and with the flags of the
// library.  A mistake in the text fails the build, and the register / scratch / LDS use of gmmvi_data_tape_rows with the
// gmmvi_affine branch of the sweep taken can be read from build/custom_affine_sample.s, beside build/custom_nodes_sample.s, the
// same composition without that branch.  The local arrays are the arrays' matter, not the primitive's.  Nothing of the device
// code is linked into the library.
#include <hip/hip_runtime.h>
#include "gmmvi_hip.h"

__host__ __device__ inline float gmmvi_value(float);
__host__ __device__ inline float gmmvi_sumsq(const float*, int, int, float);
__host__ __device__ inline float gmmvi_logsumexp(const float*, int);
__host__ __device__ inline void gmmvi_affine(const float*, int, int, int, int, int, const float*, int, float*, int);

// the two-hidden-layer network of the test suite: row = [features (F) | label], C = F + 1; params = [prior mean, prior std, H1,
// H2]; x holds, layer by layer, one block [weights | bias] per unit
template <class T, class X>
__host__ __device__ T gmmvi_user_row(X x, int D, const float* row, int C, const float* params) {
    const int F = C - 1, H1 = (int)params[2], H2 = (int)params[3];
    const int o2 = H1 * C, o3 = o2 + H2 * (H1 + 1), K = (D - o3) / (H2 + 1);
    T a[32], h1[32], h2[32], z[16];
    gmmvi_affine(x, 0, 1, C, F, C, row, F, a, H1);
    for (int j = 0; j < H1; ++j) h1[j] = tanh(a[j]);
    gmmvi_affine(x, o2, 1, H1 + 1, o2 + H1, H1 + 1, h1, H1, a, H2);
    for (int j = 0; j < H2; ++j) h2[j] = tanh(a[j]);
    gmmvi_affine(x, o3, 1, H2 + 1, o3 + H2, H2 + 1, h2, H2, z, K);
    return z[(int)row[F]] - gmmvi_logsumexp(z, K);
}

template <class T, class X>
__host__ __device__ T gmmvi_user_prior(X x, int D, const float* params) {
    const float m = params[0], s = params[1];
    return -0.5f * gmmvi_sumsq(x, 0, D, m) / (s * s) - D * (logf(s) + 0.9189385332046727f);
}

#define GMMVI_TAPE_NO_KERNELS
#define GMMVI_TAPE_NODES 1                                       // the overloads and the sweep of the node-array record
#define GMMVI_TAPE_AFFINE 1                                      // gmmvi_affine and its branch of that sweep
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
