// Minibatch logistic-regression target (target_distributions/logistic_regression.py:70-142, upstream's
// LogisticRegression_minibatch) and its analytic gradient.
//
// The posterior of logreg.hip on the T training rows of the signed data matrix A (a_m = s_m x~_m), with the likelihood
// taken on a batch of B rows per sample and scaled by T / B.  The batches: within call c the training rows
// are permuted by rho_c (feistel.h, stream 4, epoch word 0), cut into nb = floor(T / B) batches (nb = 1 when every sample
// shares the first batch), and sample n takes batch b = n mod nb:
//     row(n, j) = rho_c(b B + j),  j < B
//     lp[n]     = (T/B) sum_j log sigma(t_j) + sum_d log N(w_nd; mu, sd^2),   t_j = a_row(n,j) . w_n
//     grad[n]   = (T/B) sum_j sigma(-t_j) a_row(n,j) - (w_n - mu) / sd^2
//
// Mapping: a workgroup owns one batch class b and 16 of its samples (n = b + nb (16 g + i), i < 16), so every batch row
// it gathers serves 16 samples.  Per chunk of 64 batch rows the lanes compute the row indices from the stream (no sort, no
// device state) and stage the signed rows in LDS; each wave then takes one 16-row block and runs logreg.hip's two chained
// contractions on v_mfma_f32_16x16x4_f32:
//     T = A_blk W^T          A operand: lane l -> As[16 wave + (l & 15)][4 s + (l >> 4)], B: Ws[l & 15][4 s + (l >> 4)]
//     D lane l, register r -> T[16 wave + 4 (l >> 4) + r][l & 15]
// log sigma(t) and sigma(-t) are formed in the accumulator registers, and G[d][n] += sum_m A[m][d] R[m][n] takes its k-slot
// from the same register (R never leaves the lane).  Rows past B are zero in LDS and masked (a zero row would add
// log sigma(0)).  The gradient accumulators cover 128 columns, hence D <= 128.  The four waves' partials are summed through
// LDS in fixed order and scaled by T / B once, so a given (seed, call) is bitwise reproducible (no atomics).
#include "common.h"
#include "feistel.h"

namespace {
typedef float lrmb_f32x4 __attribute__((ext_vector_type(4)));
constexpr int LRMB_NT = 16;            // samples per workgroup
constexpr int LRMB_WAVES = 4;
constexpr int LRMB_CHUNK = 16 * LRMB_WAVES;   // batch rows staged per pass
constexpr int LRMB_DT = 8;             // 16-column tiles of the gradient
constexpr int LRMB_DMAX = 16 * LRMB_DT;

__host__ __device__ inline int lrmb_ldw(int D) { return ((D + 3) & ~3) + 1; }
__host__ __device__ inline int lrmb_gld(int D) { return 16 * ((D + 15) / 16) + 1; }

// LDS: Ws [16][ldw] | rows [64] | As [64][ldw], reused after the chunk loop as Gs [4 waves][16 samples][gld] | Ls [4][64]
__host__ __device__ inline int lrmb_as_floats(int D) {
    const int a = LRMB_CHUNK * lrmb_ldw(D), g = LRMB_WAVES * LRMB_NT * lrmb_gld(D);
    return a > g ? a : g;
}
}  // namespace

__global__ __launch_bounds__(256) void logreg_mb_kernel(int D, int T, const float* __restrict__ A, int B, int nb,
                                                        int groups, uint32_t k0, uint32_t k1, uint32_t call,
                                                        uint32_t h, float scale, float prior_mean, float prior_std,
                                                        const float* __restrict__ W, int N, float* __restrict__ lp,
                                                        float* __restrict__ grad) {
    extern __shared__ float lrmb_smem[];
    const int ldw = lrmb_ldw(D), gld = lrmb_gld(D);
    float* Ws = lrmb_smem;                                           // [16][ldw], zero beyond D and past N
    int* rows_s = (int*)(Ws + LRMB_NT * ldw);                        // [64] data rows of the chunk
    float* As = (float*)(rows_s + LRMB_CHUNK);                       // [64][ldw], zero beyond D and past the batch
    float* Gs = As;                                                  // after the chunk loop
    float* Ls = As + lrmb_as_floats(D);                              // [4 waves][64 lanes]
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / groups, g = blockIdx.x - b * groups;
    // sample of local column i: n = b + nb (16 g + i)
    const long long q0 = (long long)LRMB_NT * g;
    if ((long long)b + (long long)nb * q0 >= N) return;              // the whole workgroup: no sample of this class left
    for (int idx = t; idx < LRMB_NT * ldw; idx += 256) {
        const int r = idx / ldw, c = idx - r * ldw;
        const long long n = (long long)b + (long long)nb * (q0 + r);
        Ws[idx] = (c < D && n < N) ? W[(size_t)n * D + c] : 0.f;
    }
    const int KS = (D + 3) >> 2;
    const uint32_t base = (uint32_t)b * (uint32_t)B;                 // b B + j < nb B <= T
    float lsum = 0.f;
    lrmb_f32x4 acc[LRMB_DT];
#pragma unroll
    for (int dt = 0; dt < LRMB_DT; ++dt) acc[dt] = lrmb_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < B; c0 += LRMB_CHUNK) {
        const int rows = min(LRMB_CHUNK, B - c0);
        if (t < rows) rows_s[t] = (int)gmmvi_feistel_permute(base + (uint32_t)(c0 + t), 0u, call, GMMVI_STREAM_LOGREG_MINIBATCH,
                                                             (uint32_t)T, h, k0, k1);
        __syncthreads();                                             // also orders the Ws staging before its first read
        for (int idx = t; idx < LRMB_CHUNK * ldw; idx += 256) {
            const int r = idx / ldw, c = idx - r * ldw;
            As[idx] = (c < D && r < rows) ? A[(size_t)rows_s[r] * D + c] : 0.f;
        }
        __syncthreads();
        const int m0 = 16 * wave;                                    // this wave's block of the chunk
        if (m0 < rows) {
            lrmb_f32x4 tacc = lrmb_f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s = 0; s < KS; ++s) {
                const int d = 4 * s + kq;
                tacc = __builtin_amdgcn_mfma_f32_16x16x4f32(As[(m0 + i16) * ldw + d], Ws[i16 * ldw + d], tacc, 0, 0, 0);
            }
            float rr[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = m0 + 4 * kq + r < rows;
                const float tv = tacc[r];
                const float e = expf(-fabsf(tv));                           // overflow-safe: e in (0, 1]
                if (valid) lsum += fminf(tv, 0.f) - log1pf(e);              // log sigma(t)
                rr[r] = valid ? (tv >= 0.f ? e : 1.f) / (1.f + e) : 0.f;    // sigma(-t)
            }
            if (grad) {
#pragma unroll
                for (int dt = 0; dt < LRMB_DT; ++dt) {
                    if (16 * dt >= D) break;
                    const int d = 16 * dt + i16;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float a = d < D ? As[(m0 + 4 * kq + r) * ldw + d] : 0.f;
                        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, rr[r], acc[dt], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();                                             // rows_s / As are rewritten by the next chunk
    }
    if (grad) {
        // acc[dt]: lane l, register r -> G[d = 16 dt + 4 (l >> 4) + r][l & 15]
        float* gw = Gs + (size_t)wave * LRMB_NT * gld + i16 * gld;
#pragma unroll
        for (int dt = 0; dt < LRMB_DT; ++dt) {
            if (16 * dt >= D) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) gw[16 * dt + 4 * kq + r] = acc[dt][r];
        }
    }
    Ls[wave * 64 + lane] = lsum;
    __syncthreads();
    if (grad) {
        const float inv_var = 1.f / (prior_std * prior_std);
        for (int idx = t; idx < LRMB_NT * D; idx += 256) {
            const int i = idx / D, d = idx - i * D;
            const long long n = (long long)b + (long long)nb * (q0 + i);
            if (n >= N) continue;
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < LRMB_WAVES; ++w) s += Gs[(size_t)w * LRMB_NT * gld + i * gld + d];
            const float wv = Ws[i * ldw + d];
            grad[(size_t)n * D + d] = scale * s - (wv - prior_mean) * inv_var;
        }
    }
    if (t < LRMB_NT) {
        const long long n = (long long)b + (long long)nb * (q0 + t);
        if (n < N) {
            float s = 0.f;
            for (int w = 0; w < LRMB_WAVES; ++w)
                for (int q = 0; q < 4; ++q) s += Ls[w * 64 + q * 16 + t];
            const float inv_sd = 1.f / prior_std;
            float quad = 0.f;
            for (int d = 0; d < D; ++d) {
                const float z = (Ws[t * ldw + d] - prior_mean) * inv_sd;
                quad += z * z;
            }
            lp[n] = scale * s - 0.5f * quad - D * (logf(prior_std) + 0.9189385332046727f);   // 0.5 log(2 pi)
        }
    }
}

extern "C" int gmmvi_target_logreg_mb(gmmvi_ctx* ctx, int D, int T, const float* A_dev, int B, int nb, uint64_t seed,
                                      uint32_t call, float prior_mean, float prior_std, const float* W_dev, int N,
                                      float* lp_out_dev, float* grad_out_dev) {
    GMMVI_ARG_CHECK(ctx, D >= 1 && D <= LRMB_DMAX && T >= 1 && B >= 1 && B <= T && nb >= 1);
    GMMVI_ARG_CHECK(ctx, (long long)nb * (long long)B <= (long long)T && N >= 0 && prior_std > 0.f);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, A_dev && W_dev && lp_out_dev);
    GMMVI_PROF(ctx, "target_logreg_mb");
    const int classes = nb < N ? nb : N;                             // classes b >= N have no sample
    const int per_class = (N + nb - 1) / nb;                         // samples of class 0, the largest
    const int groups = (per_class + LRMB_NT - 1) / LRMB_NT;
    GMMVI_ARG_CHECK(ctx, (long long)classes * groups <= 0x7fffffffLL);
    const size_t shmem = ((size_t)LRMB_NT * lrmb_ldw(D) + LRMB_CHUNK + (size_t)lrmb_as_floats(D) + LRMB_WAVES * 64) *
                         sizeof(float);                              // <= 43 KB at D = 128
    const float scale = (float)T / (float)B;
    hipLaunchKernelGGL(logreg_mb_kernel, dim3(classes * groups), dim3(256), shmem, ctx->stream, D, T, A_dev, B, nb, groups, (uint32_t)seed, (uint32_t)(seed >> 32), call, gmmvi_feistel_half_bits((uint32_t)T),
                       scale, prior_mean, prior_std, W_dev, N, lp_out_dev, grad_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}
