// Bayesian-neural-network regression target (target_distributions/bnn.py:59-311,385-448: the WINE posterior) and its
// analytic gradient (the reference differentiates it with GradientTape, bnn.py:182-194).
//
// Network F -> H1 -> H2 -> 1 with sigmoid, sigmoid, linear layers; the parameter vector of a sample is the reference's
// layout (bnn.py:110-128,151-166): W1 [F, H1] row-major, b1 [H1], W2 [H1, H2], b2 [H2], W3 [H2], b3.  For sample n and
// the rows m of its minibatch
//     lp[n]   = s (-(T / B) sum_m (y_m - f_m)^2 - 0.5 sum_d w_d^2 / sd^2)
//     grad[n] = s (d/dw of the same)
//
// Minibatch stream: row j of sample n's batch has stream position p = n B + j, epoch e = p div T and rank
// r = p mod T; its data row is pi_{seed,call,e}(r), a 4-round balanced Feistel network on 2h bits (h = ceil(ceil(log2 T)
// / 2), cycle walking) whose round function is word 0 of Philox4x32-10 (philox.h) with counter (R | i << 24, e, call, 3).
// feistel.h holds the stream id and the position -> row map for this kernel, bnn_classifier.hip and bnn_mlp.hip.
// Each lane computes its own index; no sort, no device state.
//
// Mapping: one workgroup per sample, one batch row per lane (128 rows per chunk; B > 128 loops over chunks).  The sample's
// weights are staged in LDS (every lane reads the same address: broadcast).  Forward and backward pass of a row stay in
// registers; each lane then writes its row's record [x | 1 | h1 | h2 | d1 | d2 | d3 | r] to LDS, and the gradient is the
// sum over rows of products of two record fields (W1: x_i d1_j, b1: 1 d1_j, W2: h1_j d2_k, ..., the loss: r r).  Thread t
// owns the entries t, t + 128, ...; it sums them over the chunk's rows in row order, so the result is bitwise reproducible
// (no atomics).  The prior term and the loss are summed over the workgroup by fixed-order DPP reductions.
#include "common.h"
#include "feistel.h"
#include "wave_reduce.h"

namespace {
constexpr int BNN_THREADS = 128;                       // batch rows per chunk, one per lane
constexpr int BNN_FMAX = 32, BNN_HMAX = 16;

struct BnnShape {
    int F, H1, H2, D;
    int oW1, ob1, oW2, ob2, oW3, ob3;                  // parameter offsets
    int rX, rOne, rH1, rH2, rD1, rD2, rD3, rR, RS;     // record field offsets, record stride (odd)
};

__host__ __device__ inline BnnShape bnn_shape(int F, int H1, int H2) {
    BnnShape s;
    s.F = F; s.H1 = H1; s.H2 = H2;
    s.oW1 = 0; s.ob1 = F * H1; s.oW2 = s.ob1 + H1; s.ob2 = s.oW2 + H1 * H2; s.oW3 = s.ob2 + H2; s.ob3 = s.oW3 + H2;
    s.D = s.ob3 + 1;
    s.rX = 0; s.rOne = F; s.rH1 = F + 1; s.rH2 = s.rH1 + H1; s.rD1 = s.rH2 + H2; s.rD2 = s.rD1 + H1; s.rD3 = s.rD2 + H2;
    s.rR = s.rD3 + 1;
    s.RS = (s.rR + 1) | 1;                              // odd: the per-lane record writes hit distinct banks
    return s;
}

// overflow-safe logistic function: e = exp(-|z|) lies in (0, 1]
__device__ __forceinline__ float bnn_sigmoid(float z) {
    const float e = expf(-fabsf(z));
    return (z >= 0.f ? 1.f : e) / (1.f + e);
}

// forward pass of one row; EXACT: the shape is (FM, H1M, H2M) at compile time
template <int FM, int H1M, int H2M, bool EXACT>
__device__ __forceinline__ float bnn_forward(const BnnShape& sh, const float* __restrict__ Ws, const float (&x)[FM],
                                             float (&h1)[H1M], float (&h2)[H2M]) {
    const int F = EXACT ? FM : sh.F, H1 = EXACT ? H1M : sh.H1, H2 = EXACT ? H2M : sh.H2;
    const int ob1 = F * H1, oW2 = ob1 + H1, ob2 = oW2 + H1 * H2, oW3 = ob2 + H2, ob3 = oW3 + H2;
#pragma unroll
    for (int j = 0; j < H1M; ++j) {
        if (j < H1) {
            float z = Ws[ob1 + j];
#pragma unroll
            for (int i = 0; i < FM; ++i)
                if (i < F) z = fmaf(x[i], Ws[i * H1 + j], z);
            h1[j] = bnn_sigmoid(z);
        }
    }
#pragma unroll
    for (int k = 0; k < H2M; ++k) {
        if (k < H2) {
            float z = Ws[ob2 + k];
#pragma unroll
            for (int j = 0; j < H1M; ++j)
                if (j < H1) z = fmaf(h1[j], Ws[oW2 + j * H2 + k], z);
            h2[k] = bnn_sigmoid(z);
        }
    }
    float f = Ws[ob3];
#pragma unroll
    for (int k = 0; k < H2M; ++k)
        if (k < H2) f = fmaf(h2[k], Ws[oW3 + k], f);
    return f;
}

template <int FM, int H1M, int H2M, bool EXACT>
__global__ __launch_bounds__(BNN_THREADS) void bnn_target_kernel(int F_, int H1_, int H2_, int T, const float* __restrict__ X,
                                                                 const float* __restrict__ y, uint32_t k0, uint32_t k1,
                                                                 uint32_t call, uint32_t h, int B, float scaling,
                                                                 float inv_var, const float* __restrict__ W, int N,
                                                                 float* __restrict__ lp, float* __restrict__ grad) {
    constexpr int DM = FM * H1M + H1M + H1M * H2M + H2M + H2M + 1;
    constexpr int QM = (DM + 1 + BNN_THREADS - 1) / BNN_THREADS;       // entries per lane (the loss is entry D)
    const BnnShape sh = bnn_shape(EXACT ? FM : F_, EXACT ? H1M : H1_, EXACT ? H2M : H2_);
    const int F = sh.F, H1 = sh.H1, H2 = sh.H2, D = sh.D;
    extern __shared__ float bnn_smem[];
    float* Ws = bnn_smem;                                               // [D]
    float* Rec = bnn_smem + ((D + 3) & ~3);                             // [BNN_THREADS][RS]
    __shared__ float red[BNN_THREADS / 64];
    const int t = threadIdx.x, n = blockIdx.x;
    const float* Wn = W + (size_t)n * D;
    for (int d = t; d < D; d += BNN_THREADS) Ws[d] = Wn[d];

    // the record fields whose product over the rows is each owned entry
    int aoff[QM], boff[QM];
#pragma unroll
    for (int q = 0; q < QM; ++q) {
        const int e = t + q * BNN_THREADS;
        int a = -1, b = -1;
        if (e < sh.ob1)      { a = sh.rX + e / H1;            b = sh.rD1 + e % H1; }
        else if (e < sh.oW2) { a = sh.rOne;                   b = sh.rD1 + (e - sh.ob1); }
        else if (e < sh.ob2) { a = sh.rH1 + (e - sh.oW2) / H2; b = sh.rD2 + (e - sh.oW2) % H2; }
        else if (e < sh.oW3) { a = sh.rOne;                   b = sh.rD2 + (e - sh.ob2); }
        else if (e < sh.ob3) { a = sh.rH2 + (e - sh.oW3);     b = sh.rD3; }
        else if (e == sh.ob3) { a = sh.rOne;                  b = sh.rD3; }
        else if (e == D)     { a = sh.rR;                     b = sh.rR; }
        if (!grad && e != D) a = -1;                                    // log density only: the loss entry alone
        aoff[q] = a; boff[q] = b;
    }
    float acc[QM];
#pragma unroll
    for (int q = 0; q < QM; ++q) acc[q] = 0.f;
    __syncthreads();

    const float c3 = 2.f * (float)T / (float)B;                        // d(-(T/B) sum r^2) / df_m = (2T/B) r_m
    const gmmvi_bnn_stream_origin origin = gmmvi_bnn_stream_origin_of(n, B, T);
    for (int c0 = 0; c0 < B; c0 += BNN_THREADS) {
        const int rows = min(BNN_THREADS, B - c0);
        if (t < rows) {
            const uint32_t row = gmmvi_bnn_stream_row(origin, c0 + t, T, call, h, k0, k1);
            float x[FM], h1[H1M], h2[H2M];
#pragma unroll
            for (int i = 0; i < FM; ++i) x[i] = i < F ? X[(size_t)row * F + i] : 0.f;
            const float f = bnn_forward<FM, H1M, H2M, EXACT>(sh, Ws, x, h1, h2);
            const float res = y[row] - f;
            const float d3 = c3 * res;
            float* rec = Rec + t * sh.RS;
            float d2[H2M];
#pragma unroll
            for (int k = 0; k < H2M; ++k)
                if (k < H2) d2[k] = d3 * Ws[sh.oW3 + k] * h2[k] * (1.f - h2[k]);
#pragma unroll
            for (int j = 0; j < H1M; ++j) {
                if (j < H1) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < H2M; ++k)
                        if (k < H2) s = fmaf(Ws[sh.oW2 + j * H2 + k], d2[k], s);
                    rec[sh.rD1 + j] = s * h1[j] * (1.f - h1[j]);
                    rec[sh.rH1 + j] = h1[j];
                }
            }
#pragma unroll
            for (int i = 0; i < FM; ++i)
                if (i < F) rec[sh.rX + i] = x[i];
            rec[sh.rOne] = 1.f;
#pragma unroll
            for (int k = 0; k < H2M; ++k)
                if (k < H2) { rec[sh.rH2 + k] = h2[k]; rec[sh.rD2 + k] = d2[k]; }
            rec[sh.rD3] = d3;
            rec[sh.rR] = res;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < QM; ++q) {
            if (aoff[q] < 0) continue;
            const float* pa = Rec + aoff[q];
            const float* pb = Rec + boff[q];
            float s = acc[q];
            for (int m = 0; m < rows; ++m) s = fmaf(pa[m * sh.RS], pb[m * sh.RS], s);
            acc[q] = s;
        }
        __syncthreads();                                                // Rec is rewritten by the next chunk
    }

    // lp: -(T/B) sum r^2 (entry D) - 0.5 sum_d w_d^2 / sd^2, summed over the workgroup in fixed order
    float part = 0.f;
#pragma unroll
    for (int q = 0; q < QM; ++q) {
        const int e = t + q * BNN_THREADS;
        if (e < D) {
            const float w = Ws[e];
            part = fmaf(-0.5f * inv_var * w, w, part);
            if (grad) grad[(size_t)n * D + e] = scaling * (acc[q] - w * inv_var);
        } else if (e == D) {
            part -= (float)T / (float)B * acc[q];
        }
    }
    const float wsum = gmmvi_wave_sum(part);
    if ((t & 63) == 0) red[t >> 6] = wsum;
    __syncthreads();
    if (t == 0) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < BNN_THREADS / 64; ++w) s += red[w];
        lp[n] = scaling * s;
    }
}

template <int FM, int H1M, int H2M, bool EXACT>
__global__ __launch_bounds__(BNN_THREADS) void bnn_predict_kernel(int F_, int H1_, int H2_, const float* __restrict__ W,
                                                                  const float* __restrict__ X, int M,
                                                                  float* __restrict__ out) {
    const BnnShape sh = bnn_shape(EXACT ? FM : F_, EXACT ? H1M : H1_, EXACT ? H2M : H2_);
    extern __shared__ float bnn_smem[];
    float* Ws = bnn_smem;
    const int t = threadIdx.x, s = blockIdx.y, m = blockIdx.x * BNN_THREADS + t;
    for (int d = t; d < sh.D; d += BNN_THREADS) Ws[d] = W[(size_t)s * sh.D + d];
    __syncthreads();
    if (m >= M) return;
    float x[FM], h1[H1M], h2[H2M];
#pragma unroll
    for (int i = 0; i < FM; ++i) x[i] = i < sh.F ? X[(size_t)m * sh.F + i] : 0.f;
    out[(size_t)s * M + m] = bnn_forward<FM, H1M, H2M, EXACT>(sh, Ws, x, h1, h2);
}

bool bnn_shape_ok(int F, int H1, int H2) { return F >= 1 && F <= BNN_FMAX && H1 >= 1 && H1 <= BNN_HMAX && H2 >= 1 && H2 <= BNN_HMAX; }
bool bnn_is_wine(int F, int H1, int H2) { return F == 11 && H1 == 8 && H2 == 8; }
}  // namespace

extern "C" int gmmvi_target_bnn(gmmvi_ctx* ctx, int F, int H1, int H2, int T, const float* X_dev, const float* y_dev,
                                uint64_t seed, uint32_t call, int B, float likelihood_scaling, float prior_std,
                                const float* W_dev, int N, float* lp_out_dev, float* grad_out_dev) {
    GMMVI_ARG_CHECK(ctx, bnn_shape_ok(F, H1, H2));
    GMMVI_ARG_CHECK(ctx, T >= 1 && B >= 1 && B <= T && N >= 0 && prior_std > 0.f);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, X_dev && y_dev && W_dev && lp_out_dev);
    GMMVI_PROF(ctx, "target_bnn");
    const uint32_t h = gmmvi_feistel_half_bits((uint32_t)T);
    const BnnShape sh = bnn_shape(F, H1, H2);
    const size_t shmem = ((size_t)((sh.D + 3) & ~3) + (size_t)BNN_THREADS * sh.RS) * sizeof(float);   // <= 54 KB
    const float inv_var = 1.f / (prior_std * prior_std);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (bnn_is_wine(F, H1, H2))
        hipLaunchKernelGGL((bnn_target_kernel<11, 8, 8, true>), dim3(N), dim3(BNN_THREADS), shmem, ctx->stream, F, H1, H2, T,
                           X_dev, y_dev, k0, k1, call, h, B, likelihood_scaling, inv_var, W_dev, N, lp_out_dev, grad_out_dev);
    else
        hipLaunchKernelGGL((bnn_target_kernel<BNN_FMAX, BNN_HMAX, BNN_HMAX, false>), dim3(N), dim3(BNN_THREADS), shmem,
                           ctx->stream, F, H1, H2, T, X_dev, y_dev, k0, k1, call, h, B, likelihood_scaling, inv_var, W_dev, N,
                           lp_out_dev, grad_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

extern "C" int gmmvi_bnn_predict(gmmvi_ctx* ctx, int F, int H1, int H2, const float* W_dev, int S, const float* X_dev, int M,
                                 float* out_dev) {
    GMMVI_ARG_CHECK(ctx, bnn_shape_ok(F, H1, H2));
    GMMVI_ARG_CHECK(ctx, S >= 0 && M >= 0 && S <= 65535);
    if (S == 0 || M == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, W_dev && X_dev && out_dev);
    GMMVI_PROF(ctx, "bnn_predict");
    const BnnShape sh = bnn_shape(F, H1, H2);
    const size_t shmem = (size_t)((sh.D + 3) & ~3) * sizeof(float);
    const dim3 grid((M + BNN_THREADS - 1) / BNN_THREADS, S);
    if (bnn_is_wine(F, H1, H2))
        hipLaunchKernelGGL((bnn_predict_kernel<11, 8, 8, true>), grid, dim3(BNN_THREADS), shmem, ctx->stream, F, H1, H2,
                           W_dev, X_dev, M, out_dev);
    else
        hipLaunchKernelGGL((bnn_predict_kernel<BNN_FMAX, BNN_HMAX, BNN_HMAX, false>), grid, dim3(BNN_THREADS), shmem,
                           ctx->stream, F, H1, H2, W_dev, X_dev, M, out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}
