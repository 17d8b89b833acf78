// Diagonal-covariance GMMs (models/diagonal_gmm.py:6-59 and every `if diagonal_covs` branch of the hot path).
//
// Layout: chol[K, D] holds sigma (square roots of the covariance diagonal).  Densities, gradients, sampling, the
// background density and the Stein contraction run through the dense kernels on the embedded factor
// L = diag(sigma) (gmmvi_diag_embed: the off-diagonal zeros contribute exact zeros, so the results are the
// diagonal formulas' results); the diagonal of the dense Stein estimate IS the diagonal estimate
// (ng_estimator.py:178-181: h[i] = sum_n w g[n,i] y[n,i]), read out by gmmvi_diag_extract.
// The component updates are elementwise and have their own kernels here:
//   KL-constrained trust region  ng_based_component_updater.py:431-524 with kl() :304-318 (diagonal branch)
//   iBLR                         :160-223 (diagonal branch :170-174, :188-189, :195-197)
// D <= 512: one wavefront per component; lane t owns dimensions t, t + 64, ... (at most 8 per lane, in registers).
// All decisions are taken on wave-uniform values (DPP/shuffle all-reduce), so the bracketing search follows the
// reference's stop rules decision for decision.
// 512 < D <= GMMVI_MAX_DIM_DIAG: one workgroup of 1024 threads per component; thread t owns dimensions t, t + 1024, ...  The
// per-dimension state (mu, 1/sigma, rq, rl) lives in LDS up to D = 8192 (128 KB) and is re-derived from the inputs in global
// memory / L2 above; a probe of the search is one pass over D and one workgroup-wide sum (wave shuffles, then the 16 wave
// partials added in a fixed order by every thread), so every decision is taken on a workgroup-uniform value.  The KL is the
// sum of the per-dimension terms log r + 1/r - 1 (r = new precision / precision, each term >= 0), not sum(log r + 1/r) - D:
// at D = 1e5 one fp32 ulp of that sum is 0.008, the size of a trust-region bound.
#include "common.h"
#include <cfloat>

namespace {

constexpr int kMaxPerLane = GMMVI_MAX_DIM_BLOCKED / 64;

__device__ __forceinline__ float wave_sum_all(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ void diag_embed_kernel(const float* __restrict__ diag, int D, size_t total, float* __restrict__ dense) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t k = e / ((size_t)D * D);
    const int r = (int)(e % ((size_t)D * D));
    const int i = r / D, j = r % D;
    dense[e] = (i == j) ? diag[k * D + i] : 0.f;
}

__global__ void diag_extract_kernel(const float* __restrict__ dense, int D, size_t total, float* __restrict__ diag) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const size_t k = e / D;
    const int i = (int)(e % D);
    diag[e] = dense[k * (size_t)D * D + (size_t)i * D + i];
}

__global__ void reciprocal_kernel(const float* __restrict__ src, size_t n, float* __restrict__ dst) {
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n) dst[e] = 1.f / src[e];
}

struct DiagState {
    float mu[kMaxPerLane], prec[kMaxPerLane], lin[kMaxPerLane], rq[kMaxPerLane], rl[kMaxPerLane], icho[kMaxPerLane];
};

// kl() of ng_based_component_updater.py:299-318 at linear eta; `valid` masks the lane's elements beyond D.
// Returns the KL (NaN when a new precision is negative, as the reference's sqrt/log produce).
template <int R>
__device__ __forceinline__ float diag_kl(const DiagState& s, const bool (&valid)[kMaxPerLane], float eta, int D,
                                         float (&new_mean)[kMaxPerLane], float (&new_prec)[kMaxPerLane]) {
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (valid[r]) {
            const float nl = (eta * s.lin[r] + s.rl[r]) / eta;                     // :301
            const float np_ = (eta * s.prec[r] + s.rq[r]) / eta;                   // :302
            const float nm = 1.f / np_ * nl;                                       // :306
            const float diff = s.mu[r] - nm;                                       // :308
            a += logf(np_ / s.prec[r]) + s.prec[r] / np_;                          // :314-315
            const float w = s.icho[r] * diff;
            b += w * w;                                                            // :317
            new_mean[r] = nm;
            new_prec[r] = np_;
        }
    }
    a = wave_sum_all(a) - (float)D;
    b = wave_sum_all(b);
    const float inner = (a != a) ? a : fmaxf(0.f, a);                               // tf.maximum propagates NaN
    return 0.5f * (inner + b);
}

template <int R>
__global__ __launch_bounds__(64) void update_diag_kl_kernel(int D, float* __restrict__ means, float* __restrict__ chols,
                                                            const float* __restrict__ h_neg,
                                                            const float* __restrict__ g_neg,
                                                            const float* __restrict__ stepsizes, float temperature,
                                                            float l2_init, float* __restrict__ last_eta,
                                                            float* __restrict__ l2, float* __restrict__ num_updates,
                                                            int32_t* __restrict__ success_out,
                                                            float* __restrict__ kl_out, int32_t* __restrict__ nprobes_out) {
    const int k = blockIdx.x, t = threadIdx.x;
    const size_t base = (size_t)k * D;
    DiagState s;
    bool valid[kMaxPerLane];
    float sigma[kMaxPerLane];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int d = t + 64 * r;
        valid[r] = d < D;
        if (valid[r]) {
            sigma[r] = chols[base + d];
            s.mu[r] = means[base + d];
            s.rq[r] = h_neg[base + d];
            s.rl[r] = s.rq[r] * s.mu[r] - g_neg[base + d];                         // :448
            s.icho[r] = 1.f / sigma[r];                                            // :450
            s.prec[r] = s.icho[r] * s.icho[r];                                     // :451
            s.lin[r] = s.prec[r] * s.mu[r];                                        // :452
        }
    }
    const float eps = stepsizes[k];
    const float last = last_eta[k];
    float lb, ub;
    if (last < 0.f) { lb = -20.f; ub = 80.f; }                                      // :462-466
    else { lb = fmaxf(0.f, logf(last) - 3.f); ub = logf(last) + 3.f; }              // :467-471
    float eta = 0.5f * (ub + lb);
    bool ub_ok = false;
    int probes = 0;
    float nm[kMaxPerLane], np_[kMaxPerLane];
    for (int it = 0; it < 1000; ++it) {                                             // :399
        const float e_eta = expf(eta);
        const float diff = fminf(expf(ub) - e_eta, e_eta - expf(lb));               // :401
        if (diff < 1e-1f) break;
        const float kl = diag_kl<R>(s, valid, e_eta, D, nm, np_);                    // :407
        ++probes;
        if (fabsf(eps - kl) < 1e-1f * eps) { lb = ub = eta; break; }                // :410-413
        if (eps > kl) { ub = eta; ub_ok = true; } else { lb = eta; }                // :415-419 (NaN: lb = eta)
        eta = 0.5f * (ub + lb);
    }
    if (ub_ok) lb = ub;                                                             // :423-424
    const float lo = expf(lb), hi = expf(ub);                                       // :427
    const float eta_star = fmaxf(lo, temperature);                                  // :476
    bool success = (lo == hi);                                                      // :478
    float kl_val = -1.f;
    if (success) {
        kl_val = diag_kl<R>(s, valid, eta_star, D, nm, np_);                         // :480-482
        success = kl_val < FLT_MAX;                                                 // :488 (false for NaN)
        if (success) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (valid[r]) {
                    const float inv_chol_inv = 1.f / sqrtf(np_[r]);                 // :305,:307
                    chols[base + t + 64 * r] = sqrtf(inv_chol_inv * inv_chol_inv);  // :484, :490
                    means[base + t + 64 * r] = nm[r];
                }
            }
        }
    }
    if (t == 0) {
        last_eta[k] = success ? eta_star : -1.f;                                    // :504,:511,:524
        if (kl_out) kl_out[k] = success ? kl_val : -1.f;
        if (nprobes_out) nprobes_out[k] = probes;
        const float old = l2[k];
        l2[k] = success ? fmaxf(0.5f * old, l2_init) : fminf(1e-6f, 10.f * old);    // :520-523
        num_updates[k] += 1.f;                                                      // :519
        if (success_out) success_out[k] = success ? 1 : 0;
    }
}

// NgBasedComponentUpdaterIblr, diagonal branch (:160-223)
__global__ __launch_bounds__(64) void update_diag_iblr_kernel(int D, float* __restrict__ means, float* __restrict__ chols,
                                                              const float* __restrict__ h_neg,
                                                              const float* __restrict__ g_neg,
                                                              const float* __restrict__ stepsizes, float l2_init,
                                                              float* __restrict__ l2, float* __restrict__ num_updates,
                                                              int32_t* __restrict__ success_out) {
    const int k = blockIdx.x, t = threadIdx.x;
    const size_t base = (size_t)k * D;
    const float step = stepsizes[k];
    const bool first = num_updates[k] == 0.f;
    bool bad = false;
    float nm[kMaxPerLane], nc[kMaxPerLane];
#pragma unroll
    for (int r = 0; r < kMaxPerLane; ++r) {
        const int d = t + 64 * r;
        if (d < D) {
            const float sg = chols[base + d], mu = means[base + d], h = h_neg[base + d];
            const float corr = step / 2.f * h * sg * sg * h;                        // :171-172
            const float icho = 1.f / sg;
            const float prec = icho * icho;                                         // :173-174
            const float dprec = h + corr;                                           // :181
            const float dmean = -g_neg[base + d];                                   // :182
            nm[r] = first ? mu : mu + step * sg * sg * dmean;                       // :184-189
            const float nprec = prec + step * dprec;                                // :194
            nc[r] = sqrtf(1.f / nprec);                                             // :196-197
            bad |= !(nc[r] == nc[r]);                                               // :202
        }
    }
    const bool success = __any(bad) == 0;
    if (success) {
#pragma unroll
        for (int r = 0; r < kMaxPerLane; ++r) {
            const int d = t + 64 * r;
            if (d < D) { means[base + d] = nm[r]; chols[base + d] = nc[r]; }
        }
    }
    if (t == 0) {
        const float old = l2[k];
        l2[k] = success ? fmaxf(0.5f * old, l2_init) : fminf(1e-6f, 10.f * old);    // :217-220
        num_updates[k] += 1.f;                                                      // :223
        if (success_out) success_out[k] = success ? 1 : 0;
    }
}

// ---- 512 < D <= GMMVI_MAX_DIM_DIAG: one workgroup per component ------------------------------------------------------------
constexpr int kHdThreads = 1024, kHdWaves = kHdThreads / 64;
constexpr int kHdLdsMaxDim = 8192;                                                  // 4 floats x D of LDS: 128 KB of a CU's 160 KB

struct HdElem { float mu, icho, rq, rl; };

// the state of dimension d: from LDS [mu (D) | 1/sigma (D) | rq (D) | rl (D)], or re-derived from the inputs
template <bool LDS>
__device__ __forceinline__ HdElem hd_load(const float* st, int D, int d, const float* mu, const float* sigma,
                                          const float* h_neg, const float* g_neg) {
    HdElem e;
    if (LDS) {
        e.mu = st[d]; e.icho = st[D + d]; e.rq = st[2 * D + d]; e.rl = st[3 * D + d];
    } else {
        e.mu = mu[d];
        e.rq = h_neg[d];
        e.rl = e.rq * e.mu - g_neg[d];                                              // :448
        e.icho = 1.f / sigma[d];                                                    // :450
    }
    return e;
}

// new precision and mean at linear eta (:301-306)
__device__ __forceinline__ void hd_step(const HdElem& e, float eta, float& prec, float& np_, float& nm) {
    prec = e.icho * e.icho;                                                         // :451
    const float lin = prec * e.mu;                                                  // :452
    const float nl = (eta * lin + e.rl) / eta;                                      // :301
    np_ = (eta * prec + e.rq) / eta;                                                // :302
    nm = 1.f / np_ * nl;                                                            // :306
}

// workgroup-wide sums of (a, b), the same value in every thread; `red` alternates between two buffers so that one barrier
// per call is enough
__device__ __forceinline__ void hd_block_sum2(float& a, float& b, float (&red)[2][2][kHdWaves], int& parity) {
    a = wave_sum_all(a);
    b = wave_sum_all(b);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[parity][0][wave] = a; red[parity][1][wave] = b; }
    __syncthreads();
    a = 0.f; b = 0.f;
#pragma unroll
    for (int w = 0; w < kHdWaves; ++w) { a += red[parity][0][w]; b += red[parity][1][w]; }
    parity ^= 1;
}

// kl() of :299-318 at linear eta, one pass over D
template <bool LDS>
__device__ __forceinline__ float hd_kl(const float* st, int D, float eta, const float* mu, const float* sigma,
                                       const float* h_neg, const float* g_neg, float (&red)[2][2][kHdWaves], int& parity) {
    float a = 0.f, b = 0.f;
    for (int d = threadIdx.x; d < D; d += kHdThreads) {
        const HdElem e = hd_load<LDS>(st, D, d, mu, sigma, h_neg, g_neg);
        float prec, np_, nm;
        hd_step(e, eta, prec, np_, nm);
        const float u = prec / np_ - 1.f;                                           // 1/r - 1
        a += u - log1pf(u);                                                         // log r + 1/r - 1 (:314-315), NaN for r < 0
        const float w = e.icho * (e.mu - nm);                                       // :308
        b += w * w;                                                                 // :317
    }
    hd_block_sum2(a, b, red, parity);
    const float inner = (a != a) ? a : fmaxf(0.f, a);                               // tf.maximum propagates NaN
    return 0.5f * (inner + b);
}

template <bool LDS>
__global__ __launch_bounds__(kHdThreads) void update_diag_kl_hd_kernel(
    int D, float* __restrict__ means, float* __restrict__ chols, const float* __restrict__ h_neg,
    const float* __restrict__ g_neg, const float* __restrict__ stepsizes, float temperature, float l2_init,
    float* __restrict__ last_eta, float* __restrict__ l2, float* __restrict__ num_updates, int32_t* __restrict__ success_out,
    float* __restrict__ kl_out, int32_t* __restrict__ nprobes_out) {
    extern __shared__ float hd_state[];                                             // [4][D] when LDS
    __shared__ float red[2][2][kHdWaves];
    const int k = blockIdx.x, t = threadIdx.x;
    const size_t base = (size_t)k * D;
    float* mu = means + base;
    float* sigma = chols + base;
    const float* hk = h_neg + base;
    const float* gk = g_neg + base;
    if (LDS) {
        for (int d = t; d < D; d += kHdThreads) {
            const HdElem e = hd_load<false>(nullptr, D, d, mu, sigma, hk, gk);
            hd_state[d] = e.mu; hd_state[D + d] = e.icho; hd_state[2 * D + d] = e.rq; hd_state[3 * D + d] = e.rl;
        }
    }
    const float eps = stepsizes[k];
    const float last = last_eta[k];
    __syncthreads();                                                                // state complete; last_eta[k] read by all
    int parity = 0;
    float lb, ub;
    if (last < 0.f) { lb = -20.f; ub = 80.f; }                                      // :462-466
    else { lb = fmaxf(0.f, logf(last) - 3.f); ub = logf(last) + 3.f; }              // :467-471
    float eta = 0.5f * (ub + lb);
    bool ub_ok = false;
    int probes = 0;
    for (int it = 0; it < 1000; ++it) {                                             // :399
        const float e_eta = expf(eta);
        const float diff = fminf(expf(ub) - e_eta, e_eta - expf(lb));               // :401
        if (diff < 1e-1f) break;
        const float kl = hd_kl<LDS>(hd_state, D, e_eta, mu, sigma, hk, gk, red, parity);   // :407
        ++probes;
        if (fabsf(eps - kl) < 1e-1f * eps) { lb = ub = eta; break; }                // :410-413
        if (eps > kl) { ub = eta; ub_ok = true; } else { lb = eta; }                // :415-419 (NaN: lb = eta)
        eta = 0.5f * (ub + lb);
    }
    if (ub_ok) lb = ub;                                                             // :423-424
    const float lo = expf(lb), hi = expf(ub);                                       // :427
    const float eta_star = fmaxf(lo, temperature);                                  // :476
    bool success = (lo == hi);                                                      // :478
    float kl_val = -1.f;
    if (success) {
        kl_val = hd_kl<LDS>(hd_state, D, eta_star, mu, sigma, hk, gk, red, parity);  // :480-482
        success = kl_val < FLT_MAX;                                                 // :488 (false for NaN)
        if (success) {
            for (int d = t; d < D; d += kHdThreads) {                               // a thread reads and writes its own dimensions only
                const HdElem e = hd_load<LDS>(hd_state, D, d, mu, sigma, hk, gk);
                float prec, np_, nm;
                hd_step(e, eta_star, prec, np_, nm);
                const float inv_chol_inv = 1.f / sqrtf(np_);                        // :305,:307
                sigma[d] = sqrtf(inv_chol_inv * inv_chol_inv);                      // :484, :490
                mu[d] = nm;
            }
        }
    }
    if (t == 0) {
        last_eta[k] = success ? eta_star : -1.f;                                    // :504,:511,:524
        if (kl_out) kl_out[k] = success ? kl_val : -1.f;
        if (nprobes_out) nprobes_out[k] = probes;
        const float old = l2[k];
        l2[k] = success ? fmaxf(0.5f * old, l2_init) : fminf(1e-6f, 10.f * old);    // :520-523
        num_updates[k] += 1.f;                                                      // :519
        if (success_out) success_out[k] = success ? 1 : 0;
    }
}

// new mean and standard deviation of one dimension, NgBasedComponentUpdaterIblr's diagonal branch (:170-197)
__device__ __forceinline__ void iblr_step(float sg, float mu, float h, float g, float step, bool first, float& nm, float& nc) {
    const float corr = step / 2.f * h * sg * sg * h;                                // :171-172
    const float icho = 1.f / sg;
    const float prec = icho * icho;                                                 // :173-174
    const float dprec = h + corr;                                                   // :181
    const float dmean = -g;                                                         // :182
    nm = first ? mu : mu + step * sg * sg * dmean;                                  // :184-189
    const float nprec = prec + step * dprec;                                        // :194
    nc = sqrtf(1.f / nprec);                                                        // :196-197
}

__global__ __launch_bounds__(kHdThreads) void update_diag_iblr_hd_kernel(
    int D, float* __restrict__ means, float* __restrict__ chols, const float* __restrict__ h_neg,
    const float* __restrict__ g_neg, const float* __restrict__ stepsizes, float l2_init, float* __restrict__ l2,
    float* __restrict__ num_updates, int32_t* __restrict__ success_out) {
    const int k = blockIdx.x, t = threadIdx.x;
    const size_t base = (size_t)k * D;
    const float step = stepsizes[k];
    const bool first = num_updates[k] == 0.f;
    int bad = 0;
    for (int d = t; d < D; d += kHdThreads) {
        float nm, nc;
        iblr_step(chols[base + d], means[base + d], h_neg[base + d], g_neg[base + d], step, first, nm, nc);
        bad |= !(nc == nc);                                                         // :202
    }
    const bool success = __syncthreads_or(bad) == 0;                                // (also: num_updates[k] read by all)
    if (success) {
        for (int d = t; d < D; d += kHdThreads) {                                   // a thread reads and writes its own dimensions only
            float nm, nc;
            iblr_step(chols[base + d], means[base + d], h_neg[base + d], g_neg[base + d], step, first, nm, nc);
            means[base + d] = nm;
            chols[base + d] = nc;
        }
    }
    if (t == 0) {
        const float old = l2[k];
        l2[k] = success ? fmaxf(0.5f * old, l2_init) : fminf(1e-6f, 10.f * old);    // :217-220
        num_updates[k] += 1.f;                                                      // :223
        if (success_out) success_out[k] = success ? 1 : 0;
    }
}

}  // namespace

extern "C" {

int gmmvi_diag_embed(gmmvi_ctx* ctx, int K, int D, const float* diag_dev, float* dense_out_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 0 && D >= 1 && D <= GMMVI_MAX_DIM_BLOCKED);
    if (K == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, diag_dev && dense_out_dev);
    const size_t total = (size_t)K * D * D;
    GMMVI_PROF(ctx, "diag_embed");
    hipLaunchKernelGGL(diag_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, diag_dev, D,
                       total, dense_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_diag_extract(gmmvi_ctx* ctx, int K, int D, const float* dense_dev, float* diag_out_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 0 && D >= 1 && D <= GMMVI_MAX_DIM_BLOCKED);
    if (K == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, dense_dev && diag_out_dev);
    const size_t total = (size_t)K * D;
    GMMVI_PROF(ctx, "diag_extract");
    hipLaunchKernelGGL(diag_extract_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, dense_dev,
                       D, total, diag_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_reciprocal_f32(gmmvi_ctx* ctx, const float* src_dev, size_t n, float* dst_dev) {
    if (n == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, src_dev && dst_dev);
    GMMVI_PROF(ctx, "reciprocal");
    hipLaunchKernelGGL(reciprocal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, src_dev, n,
                       dst_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_update_components_diag_kl(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_diag_dev,
                                    const float* h_neg_diag_dev, const float* g_neg_dev, const float* stepsizes_dev,
                                    float temperature, float l2_init, float* last_eta_dev, float* l2_dev,
                                    float* num_received_updates_dev, int32_t* success_out_dev, float* kl_out_dev,
                                    int32_t* n_probes_out_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG);
    GMMVI_ARG_CHECK(ctx, means_dev && chols_diag_dev && h_neg_diag_dev && g_neg_dev && stepsizes_dev && last_eta_dev &&
                             l2_dev && num_received_updates_dev);
    GMMVI_PROF(ctx, "update_diag_kl");
    if (D > GMMVI_MAX_DIM_BLOCKED) {
        if (D <= kHdLdsMaxDim) {
            const size_t lds = (size_t)4 * D * sizeof(float);
            GMMVI_HIP_CHECK(ctx, hipFuncSetAttribute((const void*)update_diag_kl_hd_kernel<true>,
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(update_diag_kl_hd_kernel<true>, dim3(K), dim3(kHdThreads), lds, ctx->stream, D, means_dev,
                               chols_diag_dev, h_neg_diag_dev, g_neg_dev, stepsizes_dev, temperature, l2_init, last_eta_dev,
                               l2_dev, num_received_updates_dev, success_out_dev, kl_out_dev, n_probes_out_dev);
        } else {
            hipLaunchKernelGGL(update_diag_kl_hd_kernel<false>, dim3(K), dim3(kHdThreads), 0, ctx->stream, D, means_dev,
                               chols_diag_dev, h_neg_diag_dev, g_neg_dev, stepsizes_dev, temperature, l2_init, last_eta_dev,
                               l2_dev, num_received_updates_dev, success_out_dev, kl_out_dev, n_probes_out_dev);
        }
        GMMVI_LAUNCH_CHECK(ctx);
        return GMMVI_OK;
    }
    const int per_lane = (D + 63) / 64;
#define GMMVI_DIAG_LAUNCH(R)                                                                                         \
    hipLaunchKernelGGL(update_diag_kl_kernel<R>, dim3(K), dim3(64), 0, ctx->stream, D, means_dev, chols_diag_dev,      \
                       h_neg_diag_dev, g_neg_dev, stepsizes_dev, temperature, l2_init, last_eta_dev, l2_dev,          \
                       num_received_updates_dev, success_out_dev, kl_out_dev, n_probes_out_dev)
    if (per_lane == 1) GMMVI_DIAG_LAUNCH(1);
    else if (per_lane == 2) GMMVI_DIAG_LAUNCH(2);
    else if (per_lane <= 4) GMMVI_DIAG_LAUNCH(4);
    else GMMVI_DIAG_LAUNCH(kMaxPerLane);
#undef GMMVI_DIAG_LAUNCH
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_update_components_diag_iblr(gmmvi_ctx* ctx, int K, int D, float* means_dev, float* chols_diag_dev,
                                      const float* h_neg_diag_dev, const float* g_neg_dev, const float* stepsizes_dev,
                                      float l2_init, float* l2_dev, float* num_received_updates_dev,
                                      int32_t* success_out_dev) {
    GMMVI_ARG_CHECK(ctx, K >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG);
    GMMVI_ARG_CHECK(ctx, means_dev && chols_diag_dev && h_neg_diag_dev && g_neg_dev && stepsizes_dev && l2_dev &&
                             num_received_updates_dev);
    GMMVI_PROF(ctx, "update_diag_iblr");
    if (D > GMMVI_MAX_DIM_BLOCKED) {
        hipLaunchKernelGGL(update_diag_iblr_hd_kernel, dim3(K), dim3(kHdThreads), 0, ctx->stream, D, means_dev,
                           chols_diag_dev, h_neg_diag_dev, g_neg_dev, stepsizes_dev, l2_init, l2_dev,
                           num_received_updates_dev, success_out_dev);
        GMMVI_LAUNCH_CHECK(ctx);
        return GMMVI_OK;
    }
    hipLaunchKernelGGL(update_diag_iblr_kernel, dim3(K), dim3(64), 0, ctx->stream, D, means_dev, chols_diag_dev,
                       h_neg_diag_dev, g_neg_dev, stepsizes_dev, l2_init, l2_dev, num_received_updates_dev,
                       success_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

}  // extern "C"
