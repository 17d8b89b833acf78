// Gradient-free MORE natural-gradient estimate for DIAGONAL-covariance mixtures (gmmvi_more_diag), gfx950.
//
// Upstream's MoreNgEstimator (ng_estimator.py:296-376) whitens with a dense factor and has no diagonal branch; the project
// defines the diagonal case as upstream's fit_quadratic / RegressionFunc.fit (least_squares.py:34-76,
// :126-191) restricted to a diagonal quadratic.  For component k with mean mu, standard deviations sigma (the diagonal
// model's chol_cov[k]), ridge lambda = l2_regularizers[k], samples x_n, rewards r_n = target_lnpdfs[n] - log q(x_n)
// (ng_estimator.py:347) and importance weights w_n:
//   weights      exactly those of gmmvi_more (more_weight_reward, more_common.h): GMMVI_SELF_NORMALIZED / GMMVI_OWN_SAMPLES_ONLY,
//                mapping and map_offset keep their meaning, the double normalisation of SURVEY 2.2-7 is kept
//   whitening    z = (x - mu) / sigma, elementwise
//   features     phi(z) = [z_1^2 .. z_D^2, z_1 .. z_D, 1]: the sufficient statistics of the component family, F = 2 D + 1
//   regression   theta = (sum_n w_n phi_n phi_n^T + lambda I')^-1 sum_n w_n phi_n r_n, I' the identity with a zero at the bias
//                entry (least_squares.py:69-75); Gram matrix in fp64 from fp32 feature rows, fp64 Cholesky
//   un-whitening R_i = -2 theta_quad,i / sigma_i^2, lin_i = theta_lin,i / sigma_i + R_i mu_i (:177-189);
//                expected_hessian_neg[k] = R ([K, D], as gmmvi_diag_stein returns it),
//                expected_gradient_neg[k] = R mu - lin = -theta_lin / sigma (ng_estimator.py:369-373)
//   failure      a ridge system that is not positive definite gives NaN in both outputs of that component
//
// Kernels:
//   md_stage_kernel    workgroup = (64-sample tile, component).  z from the diagonal component block [mu | 1/sigma | ...]
//                      (gmmvi_diag_pack), transposed through LDS 64 dimensions at a time, STAGED per tile in the workspace --
//                      Zt[component][tile][D + 3 rows][64]: z, ones, reward, sqrt(weight), the layout of mb_whiten_kernel.
//                      O(N D).  A sample without weight is staged as zeros.
//   md_gram_kernel     workgroup = (128 x 128 block of the lower triangle of G, component), 8 waves, over all tiles in fixed
//                      order, so the result does not depend on the grid.  The <= 256 rows sqrt(w) [z^2, z, 1, r] of its two
//                      blocks are formed in LDS from the staged rows they need (a thread owns 4 samples of 8 rows: one
//                      16-byte load each, the next tile's while the matrix cores run) and contracted with
//                      v_mfma_f64_16x16x4_f64, 8 tile pairs per wave.  No [N, F] feature matrix reaches memory.  LDS
//                      256 x 68 words (68 KB) whatever D.
//   Cholesky, back substitution: the panel kernels of more_blocked.hip through gmmvi_more_panel_* (common.h);
//                      F + 1 = 2 050 at D = 1024: 17 panels, LDG = 2 176, 38 MB of G per component.
//   md_unwhiten_kernel elementwise, with the SAME fp32 1 / sigma that whitened the samples (a reward that is a diagonal
//                      quadratic in x is then recovered whatever the rounding of 1 / sigma).
//
// Workspace plan and group loop: those of gmmvi_more_blocked (more_common.h), without its T.
// 1 <= D <= GMMVI_MORE_DIAG_MAX_DIM = 1024; above: GMMVI_ERR_ARG (larger D is out of scope: the dense F x F solve is the limit).
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no scratch, no spills in any kernel):
//   md_gram_kernel 218 VGPR, 0 AGPR, 68 KB LDS (one 512-thread workgroup per CU); md_stage_kernel 14 VGPR, 16.3 KB LDS; md_unwhiten_kernel 10 VGPR.
// Measured deviations: DESIGN.md section 4b.
#include "more_common.h"

namespace {

__global__ __launch_bounds__(256) void md_stage_kernel(int D, int N, int n_tiles, int k0, size_t pstride,
                                                       const float* __restrict__ packed, const float* __restrict__ X,
                                                       const float* __restrict__ ld, const float* __restrict__ bg,
                                                       const float* __restrict__ tlp, const float* __restrict__ logq,
                                                       const int32_t* __restrict__ mapping, int map_offset, int flags,
                                                       const float* __restrict__ lse, float* __restrict__ Zt) {
    __shared__ float zt[64 * 65];                      // [dimension of the chunk][sample]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kk = blockIdx.y, k = k0 + kk, tile = blockIdx.x;
    const float* __restrict__ mu = packed + (size_t)k * pstride;
    const float* __restrict__ rsig = mu + D;
    const int n0 = tile * 64;
    const int n = n0 + lane;                           // every wave holds the weights of the tile's samples, lane = sample
    float sw, rew;
    more_weight_reward(k, n, N, ld, bg, tlp, logq, mapping, map_offset, flags, (flags & GMMVI_SELF_NORMALIZED) ? lse[k] : 0.f,
                       sw, rew);
    const bool live = sw > 0.f;
    float* __restrict__ out = Zt + ((size_t)kk * n_tiles + tile) * (size_t)(D + 3) * 64;
    if (wave == 0) more_write_trailer(out, D, lane, sw, rew);
    for (int c0 = 0; c0 < D; c0 += 64) {
        const int j = c0 + lane;                       // reading: lane = dimension (coalesced rows of X)
        const float m = j < D ? mu[j] : 0.f, r = j < D ? rsig[j] : 0.f;
        __syncthreads();
        for (int s = wave; s < 64; s += 4)
            zt[lane * 65 + s] = (j < D && n0 + s < N) ? (X[(size_t)(n0 + s) * D + j] - m) * r : 0.f;
        __syncthreads();
        const int jn = min(64, D - c0);                // writing: lane = sample
        for (int jj = wave; jj < jn; jj += 4) out[(size_t)(c0 + jj) * 64 + lane] = live ? zt[jj * 65 + lane] : 0.f;
    }
}

// (MFMA operand and result layout: more_common.h)
// Row f of G: f < D z_f^2, f < 2 D z_{f - D}, f = 2 D the bias, f = F = 2 D + 1 the reward.
__global__ __launch_bounds__(512) void md_gram_kernel(int D, int n_tiles, int LDG, const float* __restrict__ Zt,
                                                      double* __restrict__ G) {
    extern __shared__ float phi[];                     // [256][PHI_LD] weighted feature rows of the two blocks
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.y;
    int BI, BC;
    more_block_of(blockIdx.x, BI, BC);
    const bool diag = BI == BC;
    const int F = 2 * D + 1;
    const int ZS = (D + 3) * 64;                       // per tile: rows 0..D-1 z, row D ones, D+1 reward, D+2 sqrt(weight)
    const int n_rows = diag ? 128 : 256;
    // this thread forms the samples c4 .. c4 + 3 of the local rows tid / 16 + 32 q, q = 0 .. 7
    const int c4 = 4 * (tid & 15), rbase = tid >> 4;
    int src[8];                                        // offset of the staged row in a tile, -1: no feature
    unsigned sq = 0;                                   // bit q: the row is the square of its staged row
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int r = rbase + 32 * q;
        const int f = TB * (r < 128 ? BI : BC) + (r & 127);
        int s = -1;
        if (r < n_rows && f <= F) {
            if (f < D) { s = f; sq |= 1u << q; }
            else if (f < 2 * D) s = f - D;
            else if (f == 2 * D) s = D;
            else s = D + 1;
        }
        src[q] = s < 0 ? -1 : s * 64 + c4;
    }
    for (int e = tid; e < 256 * PHI_LD; e += 512) phi[e] = 0.f;         // rows without a feature stay zero
    const float* __restrict__ zsrc = Zt + (size_t)k * n_tiles * ZS;
    const float4 zero4 = float4{0.f, 0.f, 0.f, 0.f};
    float4 pre[8], psw;
#pragma unroll
    for (int q = 0; q < 8; ++q) pre[q] = src[q] >= 0 ? *reinterpret_cast<const float4*>(zsrc + src[q]) : zero4;
    psw = *reinterpret_cast<const float4*>(zsrc + (D + 2) * 64 + c4);
    __syncthreads();

    // wave w owns the tile pairs p = w + 8 pp: row tile p / 8 of block BI, column tile p % 8 of block BC
    f64x4 acc[8];
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) acc[pp] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int r16 = lane & 15, kg = lane >> 4;
    const int col_base = diag ? 0 : 128;
    for (int t = 0; t < n_tiles; ++t) {
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            if (src[q] < 0) continue;
            const float4 v = pre[q];
            float4 o = float4{psw.x * v.x, psw.y * v.y, psw.z * v.z, psw.w * v.w};
            if (sq & (1u << q)) o = float4{o.x * v.x, o.y * v.y, o.z * v.z, o.w * v.w};
            *reinterpret_cast<float4*>(phi + (rbase + 32 * q) * PHI_LD + c4) = o;
        }
        __syncthreads();
        // the next tile's staged rows travel to registers while the matrix cores work on this one
        if (t + 1 < n_tiles) {
            const float* __restrict__ znext = zsrc + (size_t)(t + 1) * ZS;
#pragma unroll
            for (int q = 0; q < 8; ++q) pre[q] = src[q] >= 0 ? *reinterpret_cast<const float4*>(znext + src[q]) : zero4;
            psw = *reinterpret_cast<const float4*>(znext + (D + 2) * 64 + c4);
        }
        more_contract_block(phi, wave, r16, kg, col_base, acc);
        __syncthreads();
    }
    more_store_block(G + (size_t)k * LDG * LDG, LDG, BI, BC, wave, r16, kg, acc);
}

// R_i = -2 theta_quad,i / sigma_i^2 (least_squares.py:177-185 on a diagonal), g_i = R_i mu_i - lin_i = -theta_lin,i / sigma_i
// (:186-188, ng_estimator.py:371-373); NaN for a component whose ridge system was not positive definite
__global__ __launch_bounds__(256) void md_unwhiten_kernel(int D, int LDG, int k0, size_t pstride,
                                                          const float* __restrict__ packed,
                                                          const double* __restrict__ beta_all, const int* __restrict__ fail,
                                                          float* __restrict__ h_neg, float* __restrict__ g_neg) {
    const int i = blockIdx.x * 256 + threadIdx.x, kk = blockIdx.y;
    if (i >= D) return;
    const int k = k0 + kk;
    float h = __int_as_float(0x7fc00000), g = h;
    if (!fail[kk]) {
        const double rs = (double)packed[(size_t)k * pstride + D + i];   // the 1 / sigma_i that whitened the samples
        const double* __restrict__ beta = beta_all + (size_t)kk * LDG;
        h = (float)(-2.0 * beta[i] * rs * rs);
        g = (float)(-beta[D + i] * rs);
    }
    h_neg[(size_t)k * D + i] = h;
    g_neg[(size_t)k * D + i] = g;
}

}  // namespace

extern "C" int gmmvi_more_diag(gmmvi_ctx* ctx, int K, int D, const float* packed_dev, const float* X_dev, int N,
                               const float* ld_dev, const float* logq_dev, const float* bg_dev, const float* tlp_dev,
                               const int32_t* mapping_dev, int map_offset, int flags, const float* l2_dev,
                               float* h_neg_diag_out_dev, float* g_neg_out_dev) {
    if (!ctx) return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_diag: no context");
    if (D < 1 || D > GMMVI_MORE_DIAG_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_diag: D = " + std::to_string(D) +
                                                  " is outside the supported range 1 <= D <= " +
                                                  std::to_string(GMMVI_MORE_DIAG_MAX_DIM) +
                                                  " (the F = 2 D + 1 ridge system is solved densely)");
    if (K < 1 || N < 1) return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_diag: K >= 1 and N >= 1 are required");
    const bool own_only = (flags & GMMVI_OWN_SAMPLES_ONLY) != 0;
    if (!(packed_dev && X_dev && logq_dev && tlp_dev && l2_dev && h_neg_diag_out_dev && g_neg_out_dev) ||
        (own_only ? mapping_dev == nullptr : !(ld_dev && bg_dev)))
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_diag: a required device pointer is null");

    const size_t pstride = gmmvi_diag_packed_stride(D);
    static const MorePanelNames prof = {"more_diag_lse", "more_diag_stage", "more_diag_gram", "more_diag_cholesky",
                                        "more_diag_solve"};
    MorePanelPlan p;
    int rc = more_panel_plan(ctx, K, N, D, 2 * D + 1, 0, &p);
    if (rc != GMMVI_OK) return rc;
    const size_t gram_lds = (size_t)256 * PHI_LD * sizeof(float);
    rc = gmmvi_ensure_dynamic_lds(ctx, (const void*)md_gram_kernel, gram_lds);
    if (rc != GMMVI_OK) return rc;
    return more_panel_run(
        ctx, p, prof, K, N, ld_dev, bg_dev, mapping_dev, map_offset, flags, l2_dev,
        [&](int k0, int kg) {
            hipLaunchKernelGGL(md_stage_kernel, dim3(p.n_tiles, kg), dim3(256), 0, ctx->stream, D, N, p.n_tiles, k0, pstride,
                               packed_dev, X_dev, ld_dev, bg_dev, tlp_dev, logq_dev, mapping_dev, map_offset, flags, p.lse, p.Zt);
        },
        [&](int kg) {
            hipLaunchKernelGGL(md_gram_kernel, dim3(p.nblk * (p.nblk + 1) / 2, kg), dim3(512), gram_lds, ctx->stream, D,
                               p.n_tiles, p.LDG, p.Zt, p.G);
        },
        [&](int k0, int kg) {
            hipLaunchKernelGGL(md_unwhiten_kernel, dim3((D + 255) / 256, kg), dim3(256), 0, ctx->stream, D, p.LDG, k0, pstride,
                               packed_dev, p.beta, p.fail, h_neg_diag_out_dev, g_neg_out_dev);
        });
}
