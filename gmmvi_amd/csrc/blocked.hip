// Blocked path for 50 < D <= 512 (blocked.h): densities, sampling, Stein estimate and (blocked_update.hip) the KL-constrained
// update with the O(D^2)-per-pair work expressed as batched f32 contractions on the matrix cores (blocked_gemm.hip: on the f32
// instruction, or -- wide and long launches, the default -- on the bf16 instruction through 3-way split operands at f32
// accuracy) and the O(D^3)-per-component factorisations as one-workgroup-per-component kernels on L2-resident matrices
// (blocked_factor.h).
//
// Reference arithmetic: models/full_cov_gmm.py:56-62 (z = L^-1 (x - mu) -- here Z = (X - mu) L^-T with the explicit
// inverse the reference also keeps for its sample database, optimization/sample_db.py:121), models/gmm.py:183-216,274-300,
// :361-386, gmmvi_modules/ng_estimator.py:146-263, gmmvi_modules/ng_based_component_updater.py:244-524.
#include "blocked_gemm.h"
#include "blocked_factor.h"
#include <cstdlib>

namespace {

// ---------------------------------------------------------------------------------------------------------------------------
// component blocks: [mu | const | pad | L^-1]
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(704) void blk_pack_kernel(int family, float nu, int D, const float* __restrict__ means,
                                                       const float* __restrict__ chols, float* __restrict__ packed,
                                                       size_t ps, int lo, float* __restrict__ inv_out) {
    extern __shared__ __align__(16) float dyn[];
    __shared__ float red[16];
    const int k = blockIdx.x, t = threadIdx.x;
    const float* L = chols + (size_t)k * D * D;
    float* out = packed + (size_t)k * ps;
    float* Linv = out + lo;
    if (t < D) out[t] = means[(size_t)k * D + t];
    const float s = block_sum(t < D ? logf(L[(size_t)t * D + t]) : 0.f, red);
    if (t == 0) {
        out[D] = (family == GMMVI_GAUSS)
                     ? -s - 0.5f * D * 1.8378770664093453f
                     : lgammaf(0.5f * (nu + D)) - lgammaf(0.5f * nu) - 0.5f * D * logf(nu * 3.14159265358979f) - s;
        for (int i = D + 1; i < lo; ++i) out[i] = 0.f;
    }
    blk_trsm<false>(D, L, D, [](int i, int tt) { return i == tt ? 1.f : 0.f; }, t, Linv, D, dyn);
    if (inv_out != nullptr) {
        float* o = inv_out + (size_t)k * D * D;
        for (int e = t; e < D * D; e += blockDim.x) o[e] = Linv[e];
    }
}

__global__ __launch_bounds__(704) void blk_cholesky_kernel(int D, const float* __restrict__ covs, float* __restrict__ W,
                                                           float* __restrict__ chols, int32_t* __restrict__ ok) {
    extern __shared__ __align__(16) float dyn[];
    const int k = blockIdx.x, t = threadIdx.x;
    const float* A = covs + (size_t)k * D * D;
    float* Wk = W + (size_t)k * D * D;
    const bool good = blk_cholesky(D, [A, D](int i, int j) { return A[(size_t)i * D + j]; }, Wk, dyn);
    __syncthreads();
    float* o = chols + (size_t)k * D * D;
    for (int e = t; e < D * D; e += blockDim.x) {
        const int i = e / D, j = e % D;
        o[e] = good ? (j <= i ? Wk[(size_t)j * D + i] : 0.f) : __builtin_nanf("");
    }
    if (t == 0 && ok) ok[k] = good ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// densities
// ---------------------------------------------------------------------------------------------------------------------------
// q[row] = sum over the column tiles of the |z|^2 partials the whitening launch left, and the component log-density
__global__ __launch_bounds__(256) void blk_qfinish_kernel(int family, float nu, int D, int N, long long rows, int tiles,
                                                          const float* __restrict__ qpart, const float* __restrict__ packed,
                                                          size_t ps, float* __restrict__ q, float* __restrict__ ld) {
    const long long row = (long long)blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    float s = qpart[row];
    for (int t = 1; t < tiles; ++t) s += qpart[(long long)t * rows + row];
    const float c = packed[(size_t)(row / N) * ps + D];
    if (q) q[row] = s;
    if (ld) ld[row] = (family == GMMVI_GAUSS) ? fmaf(-0.5f, s, c) : c - 0.5f * (nu + D) * log1pf(s / nu);
}

__global__ __launch_bounds__(256) void blk_lse_kernel(int K, int N, const float* __restrict__ ld, const float* __restrict__ logw,
                                                      const float* __restrict__ logw2, float* __restrict__ lp,
                                                      float* __restrict__ lp2) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float m = -3.0e38f, s = 0.f, m2 = -3.0e38f, s2 = 0.f;
    for (int k = 0; k < K; ++k) {
        const float v = ld[(size_t)k * N + n];
        const float a = v + logw[k];
        const float mn = fmaxf(m, a);
        s = fmaf(s, __expf(m - mn), __expf(a - mn));
        m = mn;
        if (logw2) {
            const float a2 = v + logw2[k];
            const float mn2 = fmaxf(m2, a2);
            s2 = fmaf(s2, __expf(m2 - mn2), __expf(a2 - mn2));
            m2 = mn2;
        }
    }
    if (lp) lp[n] = m + __logf(s);
    if (lp2 && logw2) lp2[n] = m2 + __logf(s2);
}

// responsibilities times the family's gradient coefficient: rw[kb][n] = exp(logw_k + ld[k][n] - lp[n]) * coef
__global__ __launch_bounds__(256) void blk_resp_kernel(int family, float nu, int D, int N, int kn, const float* __restrict__ ld,
                                                       const float* __restrict__ logw, const float* __restrict__ lp,
                                                       const float* __restrict__ q, float* __restrict__ rw) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)kn * N) return;
    const int kb = (int)(e / N), n = (int)(e % N);
    const float r = __expf(logw[kb] + ld[e] - lp[n]);
    const float coef = (family == GMMVI_GAUSS) ? -1.f : -(nu + (float)D) / (nu + q[e]);
    rw[e] = r * coef;
}

// dst[b][e] (+)= sum_s src[b * S + s][e]: partial results of a split contraction, summed in fixed order
__global__ __launch_bounds__(256) void blk_sum_slabs_kernel(int S, size_t slab, const float* __restrict__ src,
                                                            float* __restrict__ dst, int accumulate) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= slab) return;
    const float* p = src + (size_t)blockIdx.y * S * slab + e;
    float a = accumulate ? dst[(size_t)blockIdx.y * slab + e] : 0.f;
    for (int s = 0; s < S; ++s) a += p[(size_t)s * slab];
    dst[(size_t)blockIdx.y * slab + e] = a;
}

__global__ void blk_mapping_kernel(int K, const int32_t* __restrict__ offsets, int32_t* __restrict__ mapping) {
    const int k = blockIdx.x;
    const int begin = offsets[k], end = offsets[k + 1];
    for (int n = begin + blockIdx.y * blockDim.x + threadIdx.x; n < end; n += gridDim.y * blockDim.x) mapping[n] = k;
}

size_t z_budget_floats() {
    // scratch budget for the whitened samples of a component chunk (default 4 GiB); read per call so tests can shrink it
    const char* e = getenv("GMMVI_BLOCKED_ZBYTES");
    return e ? (size_t)atoll(e) / 4 : ((size_t)4 << 30) / 4;
}

// Z[kb][n][0:D] = (x_n - mu_k) L_k^-T for the components k0 .. k0 + kn - 1 (row stride ldz)
// qpart != nullptr: the launch also leaves |z|^2 partials, one per column tile: qpart[tile * kn * N + kb * N + n];
// store_z = false: Z itself is not written (a density pass that does not need the gradient)
int blk_forward(gmmvi_ctx* ctx, int D, const float* packed, int k0, int kn, const float* X, int N, float* Z, int ldz,
                float* qpart = nullptr, bool store_z = true) {
    const size_t ps = gmmvi_blocked_stride(D);
    BG g = bg_zero();
    g.A = X; g.lda = D; g.sA = 0; g.a_kmajor = 0;
    g.a_sub = packed + (size_t)k0 * ps; g.s_asub = (long long)ps;
    g.B = packed + (size_t)k0 * ps + gmmvi_blocked_linv_ofs(D); g.ldb = D; g.sB = (long long)ps; g.b_kmajor = 0;
    g.C = Z; g.ldc = ldz; g.sC = (long long)N * ldz;
    g.M = N; g.N = D; g.Kd = D; g.tri = 1;
    g.rowsq = qpart; g.rs_tile = (long long)kn * N; g.rs_batch = N; g.no_store = store_z ? 0 : 1;
    GMMVI_PROF_UNITS(ctx, "blocked_forward", (double)kn * N);
    return gmmvi_bgemm(ctx, g, kn);
}

}  // namespace

// the factorisation kernels stage up to ~70 KB of LDS at D = 512: raise the dynamic limit once
static int blk_lds_attr(gmmvi_ctx* ctx) {
    BLK_TRY(gmmvi_ensure_dynamic_lds(ctx, (const void*)blk_pack_kernel, BLK_LDS_LIMIT));
    return gmmvi_ensure_dynamic_lds(ctx, (const void*)blk_cholesky_kernel, BLK_LDS_LIMIT);
}

int gmmvi_blocked_pack(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* means, const float* chols,
                       float* packed, float* inv_chols) {
    GMMVI_PROF(ctx, "blocked_pack");
    BLK_TRY(blk_lds_attr(ctx));
    hipLaunchKernelGGL(blk_pack_kernel, dim3(K), dim3(blk_threads_mm(D)), blk_trsm_lds_floats(D) * sizeof(float), ctx->stream, family,
                       nu, D, means, chols, packed, gmmvi_blocked_stride(D), gmmvi_blocked_linv_ofs(D), inv_chols);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_blocked_cholesky(gmmvi_ctx* ctx, int K, int D, const float* covs, float* chols, int32_t* ok) {
    BLK_TRY(gmmvi_ws_reserve(ctx, (size_t)K * D * D * sizeof(float)));
    BLK_TRY(blk_lds_attr(ctx));
    hipLaunchKernelGGL(blk_cholesky_kernel, dim3(K), dim3(blk_threads_mm(D)), blk_chol_lds_floats(D) * sizeof(float), ctx->stream, D,
                       covs, (float*)ctx->ws, chols, ok);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

int gmmvi_blocked_mixture_eval(gmmvi_ctx* ctx, int family, float nu, int K, int D, const float* packed, const float* logw,
                               const float* logw2, const float* X, int N, float* ld_out, float* lp, float* grad, float* lp2) {
    const size_t ps = gmmvi_blocked_stride(D);
    const bool need_lse = lp || grad || lp2;
    const int LP = ((D + 1 + 3) / 4) * 4;                  // row stride of Z: the Stein estimate reuses it with [.; 1; 0..] appended
    const size_t zrow = (size_t)N * LP, gslab = (size_t)N * D;
    size_t kc = z_budget_floats() / zrow;
    const int Kc = (int)(kc < 1 ? 1 : (kc > (size_t)K ? (size_t)K : kc));
    const int nchunks = (K + Kc - 1) / Kc;
    const size_t f_z = (size_t)Kc * zrow, f_q = (size_t)Kc * N, f_rw = grad ? (size_t)Kc * N : 0;
    const size_t f_ld = (!ld_out && need_lse) ? (size_t)K * N : 0, f_lp = (grad && !lp) ? (size_t)N : 0;
    // gradient: the component loop runs inside the workgroups of one [N, D] tile grid; with few tiles it is split into S
    // component ranges (≈8 workgroups per CU), each writing a partial gradient
    int S = 1;
    if (grad) {
        const int tiles = ((N + 127) / 128) * ((D + 159) / 160);
        S = (8 * ctx->num_cus + tiles - 1) / tiles;
        if (S > Kc / 4) S = Kc / 4;
        if (S > 16) S = 16;
        if (S < 1) S = 1;
        if (gmmvi_bgemm_use_split(D, D)) {
            // split route: one persistent workgroup per CU walks over the tiles -- the S with the fewest k steps per CU (whole
            // rounds of tiles x components of a range; C5 shard: 156 row tiles x S = 8 ranges of 8 components = 5 rounds, 40
            // components per CU against 39 ideal; the rule above gave 7 ranges of 10: 50)
            const int tc = ((N + 127) / 128) * gmmvi_bgemm_col_tiles(D, D);
            const int spb = (D + BK - 1) / BK;
            long long best = -1;
            for (int c = 1; c <= 16 && c <= (Kc / 4 > 1 ? Kc / 4 : 1); ++c) {
                const int inner = (Kc + c - 1) / c;
                const long long rounds = ((long long)tc * ((Kc + inner - 1) / inner) + ctx->num_cus - 1) / ctx->num_cus;
                const long long cost = rounds * ((long long)inner * spb + 12);          // + the fixed cost of a tile, in steps
                if (best < 0 || cost < best) { best = cost; S = c; }
            }
        }
    }
    const size_t f_gp = S > 1 ? (size_t)S * gslab : 0;
    const int ctiles = gmmvi_bgemm_col_tiles(D, D);              // the whitening launch: D columns, contraction over D
    const size_t f_qp = (size_t)ctiles * Kc * N;              // |z|^2 partials of the whitening launch, one per column tile
    // Z is needed after the whitening launch only by the gradient pass and by the Stein hand-over (which requires the gradient)
    const bool store_z = grad != nullptr;
    BLK_TRY(gmmvi_ws_reserve(ctx, (f_z + f_q + f_rw + f_ld + f_lp + f_gp + f_qp) * sizeof(float)));
    float* Z = (float*)ctx->ws;
    float* q = Z + f_z;
    float* rw = q + f_q;
    float* ldp = ld_out ? ld_out : (f_ld ? rw + f_rw : nullptr);
    float* lpp = lp ? lp : (f_lp ? rw + f_rw + f_ld : nullptr);
    float* gpart = rw + f_rw + f_ld + f_lp;
    float* qpart = gpart + f_gp;
    // the row norms |z|^2 come out of the whitening launch itself (per column tile; Z is not read again)
    auto rowsq = [&](int k0, int kn, bool write_ld) {
        const long long rows = (long long)kn * N;
        GMMVI_PROF(ctx, "blocked_rowsq");
        hipLaunchKernelGGL(blk_qfinish_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, family, nu, D, N,
                           rows, ctiles, qpart, packed + (size_t)k0 * ps, ps, q, (write_ld && ldp) ? ldp + (size_t)k0 * N : nullptr);
    };
    for (int c = 0; c < nchunks; ++c) {
        const int k0 = c * Kc, kn = (K - k0 < Kc) ? K - k0 : Kc;
        BLK_TRY(blk_forward(ctx, D, packed, k0, kn, X, N, Z, LP, qpart, store_z));
        rowsq(k0, kn, true);
        GMMVI_LAUNCH_CHECK(ctx);
    }
    if (need_lse) {
        GMMVI_PROF(ctx, "blocked_lse");
        hipLaunchKernelGGL(blk_lse_kernel, dim3((N + 255) / 256), dim3(256), 0, ctx->stream, K, N, ldp, logw, logw2, lpp, lp2);
        GMMVI_LAUNCH_CHECK(ctx);
    }
    if (grad) {
        for (int c = 0; c < nchunks; ++c) {
            const int k0 = c * Kc, kn = (K - k0 < Kc) ? K - k0 : Kc;
            if (nchunks > 1) {
                BLK_TRY(blk_forward(ctx, D, packed, k0, kn, X, N, Z, LP, qpart, true));
                rowsq(k0, kn, false);
                GMMVI_LAUNCH_CHECK(ctx);
            }
            const long long tot = (long long)kn * N;
            hipLaunchKernelGGL(blk_resp_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, ctx->stream, family, nu, D, N,
                               kn, ldp + (size_t)k0 * N, logw + k0, lpp, q, rw);
            GMMVI_LAUNCH_CHECK(ctx);
            BG g = bg_zero();
            g.A = Z; g.lda = LP; g.sA = (long long)zrow; g.a_kmajor = 0;
            g.a_rscale = rw; g.s_ars = N;
            g.B = packed + (size_t)k0 * ps + gmmvi_blocked_linv_ofs(D); g.ldb = D; g.sB = (long long)ps; g.b_kmajor = 1;
            g.ldc = D;
            g.M = N; g.N = D; g.Kd = D; g.tri = 2; g.inner_total = kn;
            GMMVI_PROF_UNITS(ctx, "blocked_grad", (double)kn * N);
            if (S > 1) {                       // component ranges over blockIdx.z, partial gradients summed in fixed order
                g.C = gpart; g.sC = (long long)gslab; g.inner = (kn + S - 1) / S;
                const int nz = (kn + g.inner - 1) / g.inner;
                BLK_TRY(gmmvi_bgemm(ctx, g, nz));
                hipLaunchKernelGGL(blk_sum_slabs_kernel, dim3((unsigned)((gslab + 255) / 256), 1), dim3(256), 0, ctx->stream, nz,
                                   gslab, gpart, grad, c > 0 ? 1 : 0);
                GMMVI_LAUNCH_CHECK(ctx);
            } else {
                g.C = grad; g.sC = 0; g.inner = kn; g.accumulate = c > 0;
                BLK_TRY(gmmvi_bgemm(ctx, g, 1));
            }
        }
    }
    return GMMVI_OK;
}

int gmmvi_blocked_sample(gmmvi_ctx* ctx, int K, int D, const float* means, const float* chols, const int32_t* offsets, int N,
                         int max_per_component, uint64_t seed, uint64_t first_index, int stream_id, const float* eps,
                         float* X_out, int32_t* mapping_out) {
    if (N == 0) return GMMVI_OK;
    if (eps == nullptr) {
        BLK_TRY(gmmvi_ws_reserve(ctx, (size_t)N * D * sizeof(float)));
        BLK_TRY(gmmvi_philox_normals(ctx, seed, first_index, stream_id, N, D, (float*)ctx->ws));
        eps = (const float*)ctx->ws;
    }
    const int bound = max_per_component < N ? max_per_component : N;
    BG g = bg_zero();
    g.A = eps; g.lda = D; g.sA = 0; g.a_kmajor = 0;
    g.B = chols; g.ldb = D; g.sB = (long long)D * D; g.b_kmajor = 0;       // opB(k = m, n = i) = L[i][m]: zero for m > i
    g.C = X_out; g.ldc = D; g.sC = 0;
    g.c_bias = means; g.s_cb = D;
    g.row_off = offsets;
    g.M = bound; g.N = D; g.Kd = D; g.tri = 1;
    {
        GMMVI_PROF(ctx, "blocked_sample");
        BLK_TRY(gmmvi_bgemm(ctx, g, K));
    }
    if (mapping_out) {
        int by = (bound + 255) / 256;
        if (by < 1) by = 1;
        if (by > 64) by = 64;
        hipLaunchKernelGGL(blk_mapping_kernel, dim3(K, by), dim3(256), 0, ctx->stream, K, offsets, mapping_out);
        GMMVI_LAUNCH_CHECK(ctx);
    }
    return GMMVI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Stein estimate (gmmvi_modules/ng_estimator.py:146-263), moment form as in stein.hip: the estimate is linear in
// y = Sigma^-1 (x - mu), so C_k = sum_n e_kn [x_n - mu_k; 1] [g_n; 1]^T is ONE contraction over the samples per component with
// operands shared by all components (rows [x; 1] and [g; 1]; centring and importance weight enter as the A prologue) --
// nothing whitened is read or kept -- and Sigma_k^-1 = L^-T L^-1 is applied once per component by two triangular contractions:
// H = sym((C[:D,:D]^T L^-T) L^-1) / sum e.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// rows [g_n; 1; 0..] and [x_n; 1; 0..] with the row stride LP = D + 1 rounded up to a multiple of 4 (16-byte aligned rows)
__global__ __launch_bounds__(256) void blk_stein_rows_kernel(int N, int D, int LP, const float* __restrict__ X,
                                                             const float* __restrict__ tgrad, const float* __restrict__ qgrad,
                                                             float* __restrict__ X1, float* __restrict__ G1) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)N * LP) return;
    const int n = (int)(e / LP), i = (int)(e % LP);
    const float one = (i == D) ? 1.f : 0.f;
    G1[e] = (i < D) ? tgrad[(size_t)n * D + i] - qgrad[(size_t)n * D + i] : one;
    X1[e] = (i < D) ? X[(size_t)n * D + i] : one;
}

// rows [mu_k; 0; 0..] (the "1" column is not centred)
__global__ __launch_bounds__(256) void blk_stein_mu_kernel(int D, int LP, size_t ps, const float* __restrict__ packed,
                                                           float* __restrict__ mu1) {
    const int kb = blockIdx.x;
    for (int i = threadIdx.x; i < LP; i += 256) mu1[(size_t)kb * LP + i] = (i < D) ? packed[(size_t)kb * ps + i] : 0.f;
}

// importance weights of one component over all samples, referred to their maximum: e[kb][n] = exp(a_n - M), Mk[kb] = M
__global__ __launch_bounds__(1024) void blk_stein_weights_kernel(int N, int k0, const float* __restrict__ ld,
                                                                 const float* __restrict__ bg, const int32_t* __restrict__ mapping,
                                                                 int map_offset, int flags, float* __restrict__ e,
                                                                 float* __restrict__ Mk) {
    __shared__ float red[16];
    const int kb = blockIdx.x, k = k0 + kb;
    const bool own_only = (flags & GMMVI_OWN_SAMPLES_ONLY) != 0;
    float m = -3.0e38f;
    for (int n = threadIdx.x; n < N; n += 1024) {
        const float a = own_only ? ((mapping[n] + map_offset == k) ? 0.f : -3.0e38f) : ld[(size_t)k * N + n] - bg[n];
        m = fmaxf(m, a);
    }
    const float M = block_max(m, red);
    for (int n = threadIdx.x; n < N; n += 1024) {
        const float a = own_only ? ((mapping[n] + map_offset == k) ? 0.f : -3.0e38f) : ld[(size_t)k * N + n] - bg[n];
        e[(size_t)kb * N + n] = (a > -1.0e38f) ? __expf(a - M) : 0.f;
    }
    if (threadIdx.x == 0) Mk[kb] = M;
}

// C[b][a] = sum e d_b g'_a (row D of C: sum e g'_a), T = sum e g y^T
__global__ __launch_bounds__(256) void blk_stein_finalize_kernel(int D, int N, int flags, const float* __restrict__ Craw,
                                                                 const float* __restrict__ T, const float* __restrict__ Mk,
                                                                 float* __restrict__ H_neg, float* __restrict__ g_neg) {
    const int kb = blockIdx.x, D1 = ((D + 1 + 3) / 4) * 4;          // row stride of the augmented matrix
    const float* C = Craw + (size_t)kb * D1 * D1;
    const float* Tk = T + (size_t)kb * D * D;
    const bool snis = (flags & GMMVI_SELF_NORMALIZED) != 0;
    // own samples only: the divisor is the number of own samples = sum e (weights exp(0), ng_estimator.py:110-118,146-152)
    const bool own = (flags & GMMVI_OWN_SAMPLES_ONLY) != 0;
    // (an empty own-sample set: zeros in the self-normalised branch, NaN in the plain one, as upstream's reductions give)
    const float se = C[(size_t)D * D1 + D];
    const float scale = snis ? (se > 0.f ? 1.f / se : 0.f) : (own ? 1.f / se : __expf(Mk[kb]) / (float)N);
    // (blockIdx.y slices the elements: one workgroup per component left three quarters of the chip idle, 126 us at the C5 shard)
    for (int e = blockIdx.y * 256 + threadIdx.x; e < D * D; e += gridDim.y * 256) {
        const int i = e / D, j = e % D;
        const float v = snis ? 0.5f * (Tk[e] + Tk[(size_t)j * D + i]) : Tk[e];
        H_neg[(size_t)kb * D * D + e] = -v * scale;
    }
    if (blockIdx.y == 0)
        for (int i = threadIdx.x; i < D; i += 256) g_neg[(size_t)kb * D + i] = -C[(size_t)D * D1 + i] * scale;
}

}  // namespace

int gmmvi_blocked_stein(gmmvi_ctx* ctx, int K, int D, const float* packed, const float* X, int N, const float* ld,
                        const float* qgrad, const float* bg, const float* tgrad, const int32_t* mapping, int map_offset,
                        int flags, float* H_neg, float* g_neg) {
    const int LP = ((D + 1 + 3) / 4) * 4;                  // augmented width D + 1, padded to 16-byte rows (pad columns zero)
    const size_t ps = gmmvi_blocked_stride(D);
    const size_t rows = (size_t)N * LP;
    // component chunks only bound the scratch of the weights and the per-component matrices (default budget 4 GiB)
    const size_t per_k = (size_t)N + 2 * (size_t)LP * LP + 2 * (size_t)D * D + LP + 4;
    size_t kc = z_budget_floats() / per_k;
    const int Kc = (int)(kc < 1 ? 1 : (kc > (size_t)K ? (size_t)K : kc));
    // the contraction over the samples is split into S ranges per component so that the launch has ~8 workgroups per CU
    // (a component alone has only ceil(LP/128) * ceil(LP/160) output tiles); the partial matrices are summed in fixed order
    const int tiles = ((LP + 127) / 128) * ((LP + 159) / 160);
    int S = (8 * ctx->num_cus + tiles * Kc - 1) / (tiles * Kc);
    if (S > N / 256) S = N / 256;
    if (S > 16) S = 16;
    if (S < 1) S = 1;
    if (gmmvi_bgemm_use_split(LP, N)) {
        // split route: one persistent workgroup per CU walks over the tiles -- the S that needs the fewest k steps per CU
        // (whole rounds of tiles x steps of a tile; C5 shard: 3 row tiles x 64 components x S = 4 -> exactly 3 tiles per CU)
        const int tc = ((LP + 127) / 128) * gmmvi_bgemm_col_tiles(LP, N) * Kc;
        long long best = -1;
        for (int c = 1; c <= 16 && c <= (N / 256 > 1 ? N / 256 : 1); ++c) {
            const long long rounds = ((long long)tc * c + ctx->num_cus - 1) / ctx->num_cus;
            const long long steps = ((N + c - 1) / c + BK - 1) / BK + 12;            // + the fixed cost of a tile, in steps
            if (best < 0 || rounds * steps < best) { best = rounds * steps; S = c; }
        }
    }
    const size_t f_x = rows, f_g = rows, f_e = (size_t)Kc * N, f_m = ((size_t)Kc + 3) / 4 * 4, f_mu = (size_t)Kc * LP;
    const size_t f_c = (size_t)Kc * LP * LP, f_w = (size_t)Kc * D * D, f_t = (size_t)Kc * D * D;
    const size_t f_p = S > 1 ? (size_t)Kc * S * LP * LP : 0;
    BLK_TRY(gmmvi_ws_reserve(ctx, (f_x + f_g + f_e + f_m + f_mu + f_c + f_w + f_t + f_p) * sizeof(float)));
    float* X1 = (float*)ctx->ws;
    float* G1 = X1 + f_x;
    float* e = G1 + f_g;
    float* Mk = e + f_e;
    float* mu1 = Mk + f_m;
    float* Craw = mu1 + f_mu;
    float* Wt = Craw + f_c;
    float* T = Wt + f_w;
    float* Cpart = T + f_t;
    hipLaunchKernelGGL(blk_stein_rows_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream, N, D, LP, X, tgrad,
                       qgrad, X1, G1);
    GMMVI_LAUNCH_CHECK(ctx);
    for (int k0 = 0; k0 < K; k0 += Kc) {
        const int kn = (K - k0 < Kc) ? K - k0 : Kc;
        hipLaunchKernelGGL(blk_stein_mu_kernel, dim3(kn), dim3(256), 0, ctx->stream, D, LP, ps, packed + (size_t)k0 * ps, mu1);
        hipLaunchKernelGGL(blk_stein_weights_kernel, dim3(kn), dim3(1024), 0, ctx->stream, N, k0, ld, bg, mapping, map_offset,
                           flags, e, Mk);
        GMMVI_LAUNCH_CHECK(ctx);
        {
            BG g = bg_zero();
            g.A = X1; g.lda = LP; g.sA = 0; g.a_kmajor = 1;             // opA(m = b, k = n) = (X1[n][b] - mu1[b]) e[n]
            g.a_kscale = e; g.s_aks = N;
            g.a_rsub = mu1; g.s_arsub = LP;
            g.B = G1; g.ldb = LP; g.sB = 0; g.b_kmajor = 1;             // opB(k = n, n = a) = G1[n][a]
            g.C = S > 1 ? Cpart : Craw; g.ldc = LP; g.sC = (long long)LP * LP;
            g.M = LP; g.N = LP; g.Kd = N; g.ksplit = S;
            GMMVI_PROF_UNITS(ctx, "blocked_stein_accumulate", (double)kn * N);
            BLK_TRY(gmmvi_bgemm(ctx, g, kn));
            if (S > 1) {
                const size_t slab = (size_t)LP * LP;
                hipLaunchKernelGGL(blk_sum_slabs_kernel, dim3((unsigned)((slab + 255) / 256), kn), dim3(256), 0, ctx->stream, S,
                                   slab, Cpart, Craw, 0);
                GMMVI_LAUNCH_CHECK(ctx);
            }
        }
        {
            // Wt[a][i] = sum_j C[j][a] Linv[i][j]  ( = (A L^-T)[a][i] with A = C^T )
            BG g = bg_zero();
            g.A = Craw; g.lda = LP; g.sA = (long long)LP * LP; g.a_kmajor = 1;          // opA(m = a, k = j) = C[j][a]
            g.B = packed + (size_t)k0 * ps + gmmvi_blocked_linv_ofs(D); g.ldb = D; g.sB = (long long)ps; g.b_kmajor = 0;   // opB(k = j, n = i) = Linv[i][j]
            g.C = Wt; g.ldc = D; g.sC = (long long)D * D;
            g.M = D; g.N = D; g.Kd = D; g.tri = 1;                                       // Linv[i][j] = 0 for j > i
            GMMVI_PROF(ctx, "blocked_stein_unwhiten");
            BLK_TRY(gmmvi_bgemm(ctx, g, kn));
        }
        {
            // T = Wt L^-1
            BG g = bg_zero();
            g.A = Wt; g.lda = D; g.sA = (long long)D * D; g.a_kmajor = 0;
            g.B = packed + (size_t)k0 * ps + gmmvi_blocked_linv_ofs(D); g.ldb = D; g.sB = (long long)ps; g.b_kmajor = 1;
            g.C = T; g.ldc = D; g.sC = (long long)D * D;
            g.M = D; g.N = D; g.Kd = D; g.tri = 2;
            GMMVI_PROF(ctx, "blocked_stein_unwhiten");
            BLK_TRY(gmmvi_bgemm(ctx, g, kn));
        }
        const int fin_slices = (D * D + 256 * 32 - 1) / (256 * 32);                 // ~32 elements per thread
        hipLaunchKernelGGL(blk_stein_finalize_kernel, dim3(kn, fin_slices), dim3(256), 0, ctx->stream, D, N, flags, Craw, T, Mk,
                           H_neg + (size_t)k0 * D * D, g_neg + (size_t)k0 * D);
        GMMVI_LAUNCH_CHECK(ctx);
    }
    return GMMVI_OK;
}

