// Log-normaliser of the MORE importance weights (ng_estimator.py:353-356), shared by more.hip and more_blocked.hip.
#pragma once
#include "common.h"

namespace {

// log-normaliser of the importance weights of every component over the samples it uses
__global__ __launch_bounds__(1024) void more_lse_kernel(int N, const float* __restrict__ ld, const float* __restrict__ bg,
                                                        const int32_t* __restrict__ mapping, int map_offset, int flags,
                                                        float* __restrict__ lse) {
    __shared__ float s_m[16], s_s[16];
    const int k = blockIdx.x, tid = threadIdx.x;
    const bool own_only = (flags & GMMVI_OWN_SAMPLES_ONLY) != 0;
    float m = -3.0e38f, s = 0.f;
    for (int n = tid; n < N; n += 1024) {
        float a;
        if (own_only) { if (mapping[n] + map_offset != k) continue; a = 0.f; }      // ng_estimator.py:110-118: lw = 0
        else a = ld[(size_t)k * N + n] - bg[n];
        if (!(a > -3.0e38f)) continue;
        if (a > m) { s = s * __expf(m - a) + 1.f; m = a; } else s += __expf(a - m);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o), s2 = __shfl_xor(s, o);
        const float M = fmaxf(m, m2);
        s = s * __expf(m - M) + s2 * __expf(m2 - M);
        m = M;
    }
    if ((tid & 63) == 0) { s_m[tid >> 6] = m; s_s[tid >> 6] = s; }
    __syncthreads();
    if (tid == 0) {
        float M = s_m[0];
        for (int w = 1; w < 16; ++w) M = fmaxf(M, s_m[w]);
        float S = 0.f;
        for (int w = 0; w < 16; ++w) S += s_s[w] * __expf(s_m[w] - M);
        lse[k] = (S > 0.f) ? M + __logf(S) : 0.f;
    }
}

}  // namespace
