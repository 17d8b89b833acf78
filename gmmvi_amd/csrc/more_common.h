// What the MORE routes share (more.hip: D <= 63, more_blocked.hip: 64 <= D <= 128, more_diag.hip: diagonal mixtures), gfx950.
// The specification is the banner of more.hip.  Here, once: the importance weight and reward of a sample, the layout of a
// whitened tile, the feature order, the 128 x 128 block contraction of the Gram matrix and the workspace plan and group loop
// of the two routes that solve with the panel kernels (gmmvi_more_panel_*, common.h).
#pragma once
#include <cstdlib>
#include "common.h"

typedef double f64x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int PHI_LD = 68;       // LDS row stride (words) of the feature image: 64 samples + 4 -> b128 reads conflict-free
constexpr int TB = 128;          // tile edge of G = panel width of the factorisation

// log-normaliser of the importance weights of every component over the samples it uses (ng_estimator.py:353-356)
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

inline int more_launch_lse(gmmvi_ctx* ctx, const char* prof_name, int K, int N, const float* ld, const float* bg,
                    const int32_t* mapping, int map_offset, int flags, float* lse) {
    if (!(flags & GMMVI_SELF_NORMALIZED)) return GMMVI_OK;
    GMMVI_PROF(ctx, prof_name);
    hipLaunchKernelGGL(more_lse_kernel, dim3(K), dim3(1024), 0, ctx->stream, N, ld, bg, mapping, map_offset, flags, lse);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

// sw = sqrt of the importance weight of sample n under component k, rew = its reward; both 0 for n >= N.  lse_k: the
// log-normaliser, 0 without GMMVI_SELF_NORMALIZED.  A sample is live if sw > 0.
__device__ __forceinline__ void more_weight_reward(int k, int n, int N, const float* __restrict__ ld, const float* __restrict__ bg,
                                                   const float* __restrict__ tlp, const float* __restrict__ logq,
                                                   const int32_t* __restrict__ mapping, int map_offset, int flags, float lse_k,
                                                   float& sw, float& rew) {
    sw = 0.f; rew = 0.f;
    if (n < N) {
        float a;
        if (flags & GMMVI_OWN_SAMPLES_ONLY) a = (mapping[n] + map_offset == k) ? 0.f : -3.0e38f;   // ng_estimator.py:110-118
        else a = ld[(size_t)k * N + n] - bg[n];
        if (a > -3.0e38f) sw = __expf(0.5f * (a - lse_k));       // sqrt of the importance weight (:353-358)
        rew = tlp[n] - logq[n];                                  // ng_estimator.py:347
    }
}

// A whitened tile is [D + 3][64] floats (LDS or global), lane = sample: rows 0 .. D-1 z, row D ones, D + 1 reward, D + 2
// sqrt(weight); a sample that is not live is zero in every row but the ones.  This writes the three trailer rows.
__device__ __forceinline__ void more_write_trailer(float* __restrict__ tile, int D, int lane, float sw, float rew) {
    const bool live = sw > 0.f;
    tile[D * 64 + lane] = 1.f;
    tile[(D + 1) * 64 + lane] = live ? rew : 0.f;
    tile[(D + 2) * 64 + lane] = live ? sw : 0.f;
}

// Dense quadratic feature f <= F of a tile as the product of its rows ia and ib, coded ia | ib << 16, in the order of
// least_squares.py:113-124: z_i z_j (i <= j, row-major upper triangle), z, 1; f = F is the reward row.
__device__ __forceinline__ int more_feature_code(int f, int D) {
    const int T2 = D * (D + 1) / 2, F = T2 + D + 1;
    int ia, ib;
    if (f < T2) {
        int i = 0, rem = f;
        while (rem >= D - i) { rem -= D - i; ++i; }
        ia = i; ib = i + rem;
    } else if (f < T2 + D) { ia = f - T2; ib = D; }
    else if (f == F - 1) { ia = D; ib = D; }
    else { ia = D + 1; ib = D; }
    return ia | (ib << 16);
}

// workgroup b of a launch over the lower triangle of TB x TB blocks: block row BI >= block column BC
__device__ __forceinline__ void more_block_of(int b, int& BI, int& BC) {
    BI = 0;
    while ((BI + 1) * (BI + 2) / 2 <= b) ++BI;
    BC = b - BI * (BI + 1) / 2;
}

// v_mfma_f64_16x16x4_f64 on gfx950 (probed on the hardware: tools/probe/mfma_f64_layout.hip): D[i][j] sits in lane l,
// register r with i = 4 r + l / 16, j = l % 16; operands A[i = l % 16][k = l / 16], B[k = l / 16][j = l % 16].  Below,
// r16 = lane % 16 and kg = lane / 16.
//
// One 64-sample tile's contribution to a 128 x 128 block of G from the image phi[256][PHI_LD] in LDS (rows 0 .. 127: features
// of the block row, rows col_base .. : of the block column; fp32 widened exactly to fp64).  Wave w owns the 16 x 16 tile pairs
// q = w + 8 pp: row tile q / 8, column tile q % 8; four ds_read_b128 per operand, 16 MFMAs per pair.
__device__ __forceinline__ void more_contract_block(const float* phi, int wave, int r16, int kg, int col_base, f64x4 (&acc)[8]) {
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {
        const int q = wave + 8 * pp;
        const float* pa = phi + (16 * (q >> 3) + r16) * PHI_LD + 4 * kg;
        const float* pb = phi + (col_base + 16 * (q & 7) + r16) * PHI_LD + 4 * kg;
        float4 av[4], bv[4];
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            av[qq] = *reinterpret_cast<const float4*>(pa + 16 * qq);
            bv[qq] = *reinterpret_cast<const float4*>(pb + 16 * qq);
        }
#pragma unroll
        for (int qq = 0; qq < 4; ++qq) {
            acc[pp] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[qq].x, (double)bv[qq].x, acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[qq].y, (double)bv[qq].y, acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[qq].z, (double)bv[qq].z, acc[pp], 0, 0, 0);
            acc[pp] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)av[qq].w, (double)bv[qq].w, acc[pp], 0, 0, 0);
        }
    }
}

// the accumulators of more_contract_block -> block (BI, BC) of Gk[LDG][LDG]; a diagonal block keeps its lower tile pairs
__device__ __forceinline__ void more_store_block(double* Gk, int LDG, int BI, int BC, int wave, int r16, int kg,
                                                 const f64x4 (&acc)[8]) {
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {
        const int q = wave + 8 * pp;
        const int ti = q >> 3, tj = q & 7;
        if (BI == BC && tj > ti) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gi = TB * BI + 16 * ti + 4 * r + kg, gj = TB * BC + 16 * tj + r16;
            Gk[(size_t)gi * LDG + gj] = acc[pp][r];
        }
    }
}

// ---- host: the routes that stage whitened tiles and solve with the panel kernels (more_blocked.hip, more_diag.hip) -------------
// G is LDG^2 doubles per component (LDG = TB ceil((F + 1) / TB): 563 MB at D = 128 dense).  The components are processed in
// groups of KG whose request stays under a budget (default 8 GiB, GMMVI_MORE_WS_GB, read per call so a test can shrink it; at
// least one component per group).  Every component is computed by the same launches whatever its group, so the results do
// not depend on the group size.
inline size_t more_align256(size_t b) { return (b + 255) / 256 * 256; }

inline size_t more_ws_budget_bytes() {
    const char* e = getenv("GMMVI_MORE_WS_GB");
    double gb = e ? atof(e) : 8.0;
    if (!(gb > 0.0)) gb = 8.0;
    return (size_t)(gb * (double)((size_t)1 << 30));
}

// workspace of a group: G | staged tiles Zt[kg][n_tiles][D + 3][64] | beta | T (extra_bytes per component) | fail flags, then
// the K log-normalisers
struct MorePanelPlan {
    int F, LDG, nblk, n_tiles, KG;
    double* G; float* Zt; double* beta; double* T; int* fail; float* lse;
};
struct MorePanelNames { const char *lse, *stage, *gram, *cholesky, *solve; };      // GMMVI_PROF names of a route

inline int more_panel_plan(gmmvi_ctx* ctx, int K, int N, int D, int F, size_t extra_bytes, MorePanelPlan* p) {
    p->F = F;
    p->nblk = (F + 1 + TB - 1) / TB;
    p->LDG = TB * p->nblk;
    p->n_tiles = (N + 63) / 64;
    const size_t g_bytes = (size_t)p->LDG * p->LDG * sizeof(double);
    const size_t z_bytes = more_align256((size_t)p->n_tiles * (D + 3) * 64 * sizeof(float));
    const size_t b_bytes = more_align256((size_t)p->LDG * sizeof(double));
    const size_t t_bytes = more_align256(extra_bytes);
    const size_t per_comp = g_bytes + z_bytes + b_bytes + t_bytes;
    const size_t fixed = more_align256((size_t)K * sizeof(int)) + more_align256((size_t)K * sizeof(float));
    const size_t budget = more_ws_budget_bytes();
    size_t kg_max = budget > fixed ? (budget - fixed) / per_comp : 0;
    if (kg_max < 1) kg_max = 1;
    const size_t KG = kg_max < (size_t)K ? kg_max : (size_t)K;
    p->KG = (int)KG;
    int rc = gmmvi_ws_reserve(ctx, KG * per_comp + fixed);
    if (rc != GMMVI_OK) return rc;
    char* base = (char*)ctx->ws;
    p->G = (double*)base;
    p->Zt = (float*)(base + KG * g_bytes);
    p->beta = (double*)((char*)p->Zt + KG * z_bytes);
    p->T = (double*)((char*)p->beta + KG * b_bytes);
    p->fail = (int*)((char*)p->T + KG * t_bytes);
    p->lse = (float*)((char*)p->fail + more_align256((size_t)K * sizeof(int)));
    return GMMVI_OK;
}

// The launches of a planned call.  stage(k0, kg) fills Zt for the components k0 .. k0 + kg - 1, gram(kg) contracts them into
// G, unwhiten(k0, kg) turns beta into the outputs (NaN where fail is set); each only launches, the errors are collected here.
template <class Stage, class Gram, class Unwhiten>
int more_panel_run(gmmvi_ctx* ctx, const MorePanelPlan& p, const MorePanelNames& prof, int K, int N, const float* ld, const float* bg,
                   const int32_t* mapping, int map_offset, int flags, const float* l2, Stage stage, Gram gram,
                   Unwhiten unwhiten) {
    int rc = gmmvi_more_panel_attrs(ctx);
    if (rc != GMMVI_OK) return rc;
    rc = more_launch_lse(ctx, prof.lse, K, N, ld, bg, mapping, map_offset, flags, p.lse);
    if (rc != GMMVI_OK) return rc;
    for (int k0 = 0; k0 < K; k0 += p.KG) {
        const int kg = K - k0 < p.KG ? K - k0 : p.KG;
        GMMVI_HIP_CHECK(ctx, hipMemsetAsync(p.fail, 0, (size_t)kg * sizeof(int), ctx->stream));
        {
            GMMVI_PROF(ctx, prof.stage);
            stage(k0, kg);
            GMMVI_LAUNCH_CHECK(ctx);
        }
        {
            GMMVI_PROF(ctx, prof.gram);
            gram(kg);
            GMMVI_LAUNCH_CHECK(ctx);
        }
        rc = gmmvi_more_panel_cholesky(ctx, prof.cholesky, p.F, p.LDG, kg, k0, l2, p.G, p.fail);
        if (rc != GMMVI_OK) return rc;
        GMMVI_PROF(ctx, prof.solve);
        rc = gmmvi_more_panel_backsub(ctx, p.F, p.LDG, kg, p.G, p.fail, p.beta);
        if (rc != GMMVI_OK) return rc;
        unwhiten(k0, kg);
        GMMVI_LAUNCH_CHECK(ctx);
    }
    return GMMVI_OK;
}

}  // namespace
