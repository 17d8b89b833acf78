// Bayesian logistic-regression target and its analytic gradient (target_distributions/logistic_regression.py:20-67; the
// reference differentiates it with GradientTape, sample_selector.py:70-77).
//
// With a_m = s_m x~_m (s_m = -1 for label 1, +1 for label 0; x~ the standardised features behind a bias 1) the reference's
// tf.where(label == 1, log_sigmoid(-x~ w), log_sigmoid(-x~ w) + x~ w) is log sigma(a_m . w), so for every sample w_n
//     lp[n]   = sum_m log sigma(t_mn) + sum_d log N(w_nd; mu, sd^2),        t_mn = a_m . w_n
//     grad[n] = sum_m sigma(-t_mn) a_m - (w_n - mu) / sd^2
// Two chained contractions over the data matrix with an element-wise map between them, on v_mfma_f32_16x16x4_f32 (exact
// f32).  A workgroup owns 16 samples (their rows of W staged in LDS); its four waves take interleaved 16-row chunks of A:
//     T = A_chunk W^T        A operand: lane l -> A[m0 + (l & 15)][4 s + (l >> 4)], B: W[n0 + (l & 15)][4 s + (l >> 4)]
//     D lane l, register r -> T[m0 + 4 (l >> 4) + r][n0 + (l & 15)]
// log sigma(t) and sigma(-t) are formed in the accumulator registers, and the second contraction G[d][n] += sum_m A[m][d] R[m][n]
// takes its k-slot from the SAME register: step r uses row m0 + 4 (l >> 4) + r (which row sits in which k-slot is free, the
// contraction sums over all of them), so R never leaves the lane.  Rows past M are masked (an unmasked zero row would add
// log sigma(0) = -log 2).  The gradient accumulators cover 128 columns; larger D repeats the first contraction per 128-column
// group.  The four waves' partials are summed through LDS in fixed order; lp and grad are written once.
#include "common.h"

namespace {
typedef float lr_f32x4 __attribute__((ext_vector_type(4)));
constexpr int LR_NT = 16;          // samples per workgroup
constexpr int LR_WAVES = 4;
constexpr int LR_DT = 8;           // 16-column tiles of the gradient per pass
constexpr int LR_GLD = 16 * LR_DT + 1;

__device__ __forceinline__ int lr_ldw(int D) { return ((D + 3) & ~3) + 1; }
}  // namespace

__global__ __launch_bounds__(256) void logreg_kernel(int D, int M, const float* __restrict__ A, float prior_mean,
                                                     float prior_std, const float* __restrict__ W, int N,
                                                     float* __restrict__ lp, float* __restrict__ grad) {
    extern __shared__ float lr_smem[];
    const int ldw = lr_ldw(D);
    float* Ws = lr_smem;                                  // [16][ldw], zero beyond D and past N
    float* Gs = Ws + LR_NT * ldw;                         // [4 waves][16 samples][LR_GLD]
    float* Ls = Gs + LR_WAVES * LR_NT * LR_GLD;           // [4 waves][64 lanes]
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kq = lane >> 4;
    const int n0 = blockIdx.x * LR_NT;
    for (int idx = t; idx < LR_NT * ldw; idx += 256) {
        const int r = idx / ldw, c = idx - r * ldw;
        Ws[idx] = (c < D && n0 + r < N) ? W[(size_t)(n0 + r) * D + c] : 0.f;
    }
    __syncthreads();
    const int KS = (D + 3) >> 2;
    const int nchunks = (M + 15) >> 4;
    const int groups = grad ? (D + 16 * LR_DT - 1) / (16 * LR_DT) : 1;
    float lsum = 0.f;
    for (int g = 0; g < groups; ++g) {
        const int g0 = g * 16 * LR_DT;
        lr_f32x4 acc[LR_DT];
#pragma unroll
        for (int dt = 0; dt < LR_DT; ++dt) acc[dt] = lr_f32x4{0.f, 0.f, 0.f, 0.f};
        for (int c = wave; c < nchunks; c += LR_WAVES) {
            const int m0 = 16 * c;
            const int ma = m0 + i16;
            const float* arow = A + (size_t)ma * D;
            lr_f32x4 tacc = lr_f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < KS; ++s) {
                const int d = 4 * s + kq;
                const float a = (ma < M && d < D) ? arow[d] : 0.f;
                tacc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, Ws[i16 * ldw + d], tacc, 0, 0, 0);
            }
            float rr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = m0 + 4 * kq + r < M;
                const float tv = tacc[r];
                const float e = expf(-fabsf(tv));                           // overflow-safe: e in (0, 1]
                if (g == 0 && valid) lsum += fminf(tv, 0.f) - log1pf(e);    // log sigma(t)
                rr[r] = valid ? (tv >= 0.f ? e : 1.f) / (1.f + e) : 0.f;    // sigma(-t)
            }
            if (grad) {
#pragma unroll
                for (int dt = 0; dt < LR_DT; ++dt) {
                    const int d = g0 + 16 * dt + i16;
                    if (g0 + 16 * dt >= D) break;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int m = m0 + 4 * kq + r;
                        const float a = (m < M && d < D) ? A[(size_t)m * D + d] : 0.f;
                        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, rr[r], acc[dt], 0, 0, 0);
                    }
                }
            }
        }
        if (grad) {
            // acc[dt]: lane l, register r -> G[d = g0 + 16 dt + 4 (l >> 4) + r][n0 + (l & 15)]
            float* gw = Gs + (size_t)wave * LR_NT * LR_GLD + i16 * LR_GLD;
#pragma unroll
            for (int dt = 0; dt < LR_DT; ++dt)
#pragma unroll
                for (int r = 0; r < 4; ++r) gw[16 * dt + 4 * kq + r] = acc[dt][r];
            __syncthreads();
            const int cols = min(16 * LR_DT, D - g0);
            const float inv_var = 1.f / (prior_std * prior_std);
            for (int idx = t; idx < LR_NT * cols; idx += 256) {
                const int n = idx / cols, dl = idx - n * cols;
                if (n0 + n >= N) continue;
                float s = 0.f;
#pragma unroll
                for (int w = 0; w < LR_WAVES; ++w) s += Gs[(size_t)w * LR_NT * LR_GLD + n * LR_GLD + dl];
                const float wv = Ws[n * ldw + g0 + dl];
                grad[(size_t)(n0 + n) * D + g0 + dl] = s - (wv - prior_mean) * inv_var;
            }
            __syncthreads();                              // Gs is rewritten by the next column group
        }
    }
    Ls[wave * 64 + lane] = lsum;
    __syncthreads();
    if (lp && t < LR_NT && n0 + t < N) {
        float s = 0.f;
        for (int w = 0; w < LR_WAVES; ++w)
            for (int q = 0; q < 4; ++q) s += Ls[w * 64 + q * 16 + t];
        const float inv_sd = 1.f / prior_std;
        float quad = 0.f;
        for (int d = 0; d < D; ++d) {
            const float z = (Ws[t * ldw + d] - prior_mean) * inv_sd;
            quad += z * z;
        }
        lp[n0 + t] = s - 0.5f * quad - D * (logf(prior_std) + 0.9189385332046727f);   // 0.5 log(2 pi)
    }
}

extern "C" int gmmvi_target_logreg(gmmvi_ctx* ctx, int D, int M, const float* A_dev, float prior_mean, float prior_std,
                                   const float* W_dev, int N, float* lp_out_dev, float* grad_out_dev) {
    GMMVI_ARG_CHECK(ctx, D >= 1 && D <= GMMVI_MAX_DIM_BLOCKED && M >= 1 && N >= 0 && prior_std > 0.f);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, A_dev && W_dev && lp_out_dev);
    GMMVI_PROF(ctx, "target_logreg");
    const size_t shmem = ((size_t)LR_NT * (((D + 3) & ~3) + 1) + (size_t)LR_WAVES * LR_NT * LR_GLD + LR_WAVES * 64) * sizeof(float);
    if (shmem > 64 * 1024)                                // D > 455: past the default limit of dynamic LDS
        GMMVI_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)logreg_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)shmem));
    hipLaunchKernelGGL(logreg_kernel, dim3((N + LR_NT - 1) / LR_NT), dim3(256), shmem, ctx->stream, D, M, A_dev, prior_mean,
                       prior_std, W_dev, N, lp_out_dev, grad_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}
