// ---------------------------------------------------------------------------------------------------------------
// mixture_eval on the matrix cores
// ---------------------------------------------------------------------------------------------------------------
// z = L^-1 (x - mu) and y = L^-T z as dense contractions with the explicit inverse (operand fragments in the packed block,
// common.h): v_mfma_f32_16x16x4_f32 with A = a 16-row tile of L^-1 (coalesced 256-byte fragment loads, nothing on the scalar
// path), B = 16 samples x 4 dimensions of (x - mu).  A wave owns NTS sub-tiles of 16 samples (x fragments in registers for
// the whole launch) and walks a strided subset of the components; lane (g = l >> 4, n = l & 15) holds B[k = g][sample n] and
// receives rows 4 g + r of every 16-row tile of the result for sample n.  |z|^2 is completed across the four lane groups by
// two cross-lane adds; for the gradient z goes through a wave-private LDS image ([sample][dimension], permuted so that a
// lane's k-steps are contiguous) to become the B operand of the transposed contraction.  Structural zeros of the triangle
// are skipped per 16 x 4 fragment.  The log-sum-exp over the components, the K split over blockIdx.y and the merge of the
// workgroup's waves are those of the scalar-fed kernel (density_reg.hip).
#include "density_sweep.h"
#include <cmath>

template <int DP, int FAMILY, bool GRAD, int NTS>
__global__ __launch_bounds__(512) void mixture_eval_mfma_kernel(float nu, int K_total, int D, const float* __restrict__ packed,
                                                                const float* __restrict__ logw, const float* __restrict__ X,
                                                                int N, float* __restrict__ ld_out, float* __restrict__ lp_out,
                                                                float* __restrict__ grad_out, const float* __restrict__ logw2,
                                                                float* __restrict__ lp2_out, CombineJob carried, Riders riders) {
    using PK = Pack<DP>;
    constexpr int MT = PK::MT, KS = PK::KS;
    extern __shared__ __align__(16) float sm[];
    if (combine_carried(carried) || riders_carried<DP>(riders, sm)) return;   // workgroups past the sample tiles: the merge of the previous sweep, riders
    constexpr int TS = 16 * NTS;                       // samples per workgroup tile
    constexpr int KSP = ((KS + 3) / 4) * 4;            // k-steps per lane in the z image, padded to 16-byte reads
    constexpr int ZW = 4 * KSP + 4;                    // row stride of the z image
    const int kchunk = (K_total + gridDim.y - 1) / gridDim.y;
    const int k_lo = blockIdx.y * kchunk;
    const int K = min(K_total, k_lo + kchunk);
    if (gridDim.y > 1) {
        if (lp_out) lp_out += (size_t)blockIdx.y * N;
        if (lp2_out) lp2_out += (size_t)blockIdx.y * N;
        if (GRAD && grad_out) grad_out += (size_t)blockIdx.y * N * D;
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nwaves = blockDim.x >> 6;
    const int g = lane >> 4, n16 = lane & 15;
    const int n0 = blockIdx.x * TS;
    const int n_here = min(TS, N - n0);
    // LDS: [nwaves][NTS][16][ZW] wave-private z images (gradient only), then the staging / merge area
    float* Zw = sm + (size_t)wave * (GRAD ? NTS * 16 * ZW : 0);
    float* sm_merge = sm + (size_t)nwaves * (GRAD ? NTS * 16 * ZW : 0);

    // ---- x tile: coalesced load staged through LDS; lane (g, n) keeps x[n][4 s + g] of its NTS sub-tiles -----------------
    const int ldx = D | 1;
    for (int e = threadIdx.x; e < n_here * D; e += blockDim.x) sm_merge[(e / D) * ldx + (e % D)] = X[(size_t)n0 * D + e];
    __syncthreads();
    float xb[NTS][KS];
#pragma unroll
    for (int t = 0; t < NTS; ++t)
#pragma unroll
        for (int s = 0; s < KS; ++s)
            xb[t][s] = (16 * t + n16 < n_here && 4 * s + g < D) ? sm_merge[(16 * t + n16) * ldx + 4 * s + g] : 0.f;
    __syncthreads();

    float m[NTS], sv[NTS], m2[NTS], s2[NTS];
#pragma unroll
    for (int t = 0; t < NTS; ++t) { m[t] = -3.0e38f; sv[t] = 0.f; m2[t] = -3.0e38f; s2[t] = 0.f; }
    const bool dual = logw2 != nullptr;
    me_f32x4 acc[GRAD ? NTS : 1][GRAD ? MT : 1];
    if (GRAD) {
#pragma unroll
        for (int t = 0; t < NTS; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[t][mt][r] = 0.f;
    }
    const float nud = nu + (float)D;

    for (int k = k_lo + wave; k < K; k += nwaves) {
        const float* __restrict__ Pk = packed + (size_t)k * PK::STRIDE;
        float af[PK::NF], ab[GRAD ? PK::NB : 1], mus[KS];
#pragma unroll
        for (int f = 0; f < PK::NF; ++f) af[f] = Pk[PK::FWD + 64 * f + lane];
        if (GRAD) {
#pragma unroll
            for (int f = 0; f < PK::NB; ++f) ab[f] = Pk[PK::BWD + 64 * f + lane];
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) mus[s] = (4 * s + g < DP) ? Pk[PK::MU + 4 * s + g] : 0.f;
        const float cst = Pk[PK::CONST];
        const float lw = logw[k];
        const float lw2 = dual ? logw2[k] : 0.f;
        me_f32x4 z[NTS][MT];
        float ldv[NTS], ev[NTS], scv[NTS], cfv[NTS];
#pragma unroll
        for (int t = 0; t < NTS; ++t)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) z[t][mt][r] = 0.f;
        // k-step outermost: consecutive MFMAs go to different accumulators (NTS x MT independent chains), none waits for the
        // 40-cycle dependent-issue latency of its predecessor.
        // REM rows in the last 16-row tile (D = 50: rows 48, 49 -- two useful rows for 13 of the 37 forward fragments): those
        // rows go to the vector unit instead: lane (g, n) multiplies its own k-slots of row R (the fragment value of lane
        // 16 g + r, fetched by a DPP row broadcast) and the four lane groups are summed; the result lands where the matrix
        // cores would have put it (register r of the lanes of group 0).
        constexpr int REM = me_rem_rows(DP);
        float zr[REM > 0 ? NTS : 1][REM > 0 ? REM : 1];
        if constexpr (REM > 0) {
#pragma unroll
            for (int t = 0; t < NTS; ++t)
#pragma unroll
                for (int r = 0; r < REM; ++r) zr[t][r] = 0.f;
        }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            float bs[NTS];
#pragma unroll
            for (int t = 0; t < NTS; ++t) {
                bs[t] = xb[t][s] - mus[s];
#pragma unroll
                for (int mt = 0; mt < (REM > 0 ? MT - 1 : MT); ++mt)
                    if (s < PK::nf(mt))
                        z[t][mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[PK::fwd_index(mt, s)], bs[t], z[t][mt], 0, 0, 0);
            }
            if constexpr (REM > 0) {
                me_static_rows<REM>([&](auto R) {
                    constexpr int r = R;
                    const float a = me_row_bcast<r>(af[PK::fwd_index(MT - 1, s)]);      // Linv[16 (MT-1) + r][4 s + g]
#pragma unroll
                    for (int t = 0; t < NTS; ++t) zr[t][r] = fmaf(a, bs[t], zr[t][r]);
                });
            }
        }
        if constexpr (REM > 0) {
#pragma unroll
            for (int t = 0; t < NTS; ++t)
#pragma unroll
                for (int r = 0; r < REM; ++r) {
                    float v = zr[t][r];
                    v += __shfl_xor(v, 16);
                    v += __shfl_xor(v, 32);
                    z[t][MT - 1][r] = g == 0 ? v : 0.f;
                }
        }
        if constexpr (!GRAD && NTS == 4) {
            // lane = sample (16 g + n of sub-tile g): after the cross-lane completion every lane group holds |z|^2 of all four
            // sub-tiles; each lane keeps its own sub-tile's and runs ONE log-sum-exp step -- the four groups used to repeat the
            // same four tails (the sweep without the gradient is bound by them, not by the matrix cores)
            float qs = 0.f;
#pragma unroll
            for (int t = 0; t < NTS; ++t) {
                float q = 0.f;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) q = fmaf(z[t][mt][r], z[t][mt][r], q);
                q += __shfl_xor(q, 16);
                q += __shfl_xor(q, 32);
                qs = (g == t) ? q : qs;
            }
            float ld;
            if (FAMILY == GMMVI_GAUSS) ld = fmaf(-0.5f, qs, cst);
            else ld = cst - 0.5f * nud * log1pf(qs / nu);
            const float a = ld + lw;
            const float mn = fmaxf(m[0], a);
            sv[0] = fmaf(sv[0], __expf(m[0] - mn), __expf(a - mn));
            m[0] = mn;
            if (dual) {
                const float a2 = ld + lw2;
                const float mn2 = fmaxf(m2[0], a2);
                s2[0] = fmaf(s2[0], __expf(m2[0] - mn2), __expf(a2 - mn2));
                m2[0] = mn2;
            }
            if (ld_out != nullptr && lane < n_here) ld_out[(size_t)k * N + n0 + lane] = ld;
        } else {
#pragma unroll
        for (int t = 0; t < NTS; ++t) {
            float q = 0.f;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) q = fmaf(z[t][mt][r], z[t][mt][r], q);
            q += __shfl_xor(q, 16);
            q += __shfl_xor(q, 32);
            float ld, coef;
            if (FAMILY == GMMVI_GAUSS) {
                ld = fmaf(-0.5f, q, cst);
                coef = -1.f;
            } else {
                ld = cst - 0.5f * nud * log1pf(q / nu);
                coef = -nud / (nu + q);
            }
            ldv[t] = ld;
            const float a = ld + lw;
            const float mn = fmaxf(m[t], a);
            const float sc = __expf(m[t] - mn);
            const float e = __expf(a - mn);
            sv[t] = fmaf(sv[t], sc, e);
            m[t] = mn;
            ev[t] = e; scv[t] = sc; cfv[t] = coef;
            if (dual) {
                const float a2 = ld + lw2;
                const float mn2 = fmaxf(m2[t], a2);
                s2[t] = fmaf(s2[t], __expf(m2[t] - mn2), __expf(a2 - mn2));
                m2[t] = mn2;
            }
        }
        if (ld_out != nullptr) {
            // lane group g stores sub-tile g: one instruction writes 16 NTS consecutive floats of row k
            float v = ldv[0];
#pragma unroll
            for (int t = 1; t < NTS; ++t) v = (g == t) ? ldv[t] : v;
            if (g < NTS && 16 * g + n16 < n_here) ld_out[(size_t)k * N + n0 + 16 * g + n16] = v;
        }
        }
        if (GRAD) {
            // z -> wave-private image Zs[t][n][p(i)], p(i) = (i & 3) KSP + (i >> 2): lane (g, n) holds i = 16 mt + 4 g + r
#pragma unroll
            for (int t = 0; t < NTS; ++t)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (4 * mt + g < KSP) Zw[(t * 16 + n16) * ZW + r * KSP + 4 * mt + g] = z[t][mt][r];
            ME_WAVE_LDS_SYNC();
#pragma unroll
            for (int t = 0; t < NTS; ++t) {
                float bz[KSP];
#pragma unroll
                for (int q4 = 0; q4 < KSP / 4; ++q4) {
                    const me_f32x4 v4 = *reinterpret_cast<const me_f32x4*>(Zw + (t * 16 + n16) * ZW + g * KSP + 4 * q4);
                    bz[4 * q4] = v4[0]; bz[4 * q4 + 1] = v4[1]; bz[4 * q4 + 2] = v4[2]; bz[4 * q4 + 3] = v4[3];
                }
                const float ec = ev[t] * cfv[t];
                me_f32x4 y[MT];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[mt][r] = 0.f;
#pragma unroll
                for (int s = 0; s < KS; ++s)                           // k-step outermost: MT independent chains
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt)
                        if (s >= 4 * mt)
                            y[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ab[PK::bwd_index(mt, s)], bz[s], y[mt], 0, 0, 0);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[t][mt][r] = fmaf(acc[t][mt][r], scv[t], ec * y[mt][r]);
            }
            ME_WAVE_LDS_SYNC();
        }
    }
    if (lp_out == nullptr && !GRAD) return;

    // merge the W waves' partials: sm_m[w][sample], sm_s[w][sample], sm_acc[w][i][sample]  (sample = 16 t + n).
    // Round 1: the running maxima meet in LDS and every wave rescales ITS sums to the common maximum (one exp per lane and
    // sub-tile instead of one per (dimension, sample, wave) in the reduction); round 2: plain sums in wave order.  The
    // barriers wait for LDS traffic only (ME_LDS_BARRIER): __syncthreads() would also drain the stores of the log densities.
    float* sm_m = sm_merge;
    float* sm_s = sm_merge + nwaves * TS;
    float* sm_acc = sm_merge + 2 * nwaves * TS;
    float* sm_m2 = sm_merge + (size_t)nwaves * TS * ((GRAD ? DP : 0) + 2) + (GRAD ? TS * ldx : 0);
    float* sm_s2 = sm_m2 + nwaves * TS;
    constexpr bool LANE_SAMPLE = !GRAD && NTS == 4;    // lane = sample (16 g + n of sub-tile g) instead of one column per lane group
    if constexpr (LANE_SAMPLE) {
        sm_m[wave * TS + lane] = m[0];
        if (dual) sm_m2[wave * TS + lane] = m2[0];
    } else if (g == 0) {
#pragma unroll
        for (int t = 0; t < NTS; ++t) {
            sm_m[wave * TS + 16 * t + n16] = m[t];
            if (dual) sm_m2[wave * TS + 16 * t + n16] = m2[t];
        }
    }
    ME_LDS_BARRIER();
    if constexpr (LANE_SAMPLE) {
        float M = -3.0e38f;
        for (int w = 0; w < nwaves; ++w) M = fmaxf(M, sm_m[w * TS + lane]);
        sm_s[wave * TS + lane] = sv[0] * __expf(m[0] - M);
        if (dual) {
            float M2 = -3.0e38f;
            for (int w = 0; w < nwaves; ++w) M2 = fmaxf(M2, sm_m2[w * TS + lane]);
            sm_s2[wave * TS + lane] = s2[0] * __expf(m2[0] - M2);
        }
    } else {
#pragma unroll
        for (int t = 0; t < NTS; ++t) {
            const int sidx = 16 * t + n16;
            float M = -3.0e38f;
            for (int w = 0; w < nwaves; ++w) M = fmaxf(M, sm_m[w * TS + sidx]);
            const float f = __expf(m[t] - M);
            if (g == 0) sm_s[wave * TS + sidx] = sv[t] * f;
            if (dual && g == 1) {
                float M2 = -3.0e38f;
                for (int w = 0; w < nwaves; ++w) M2 = fmaxf(M2, sm_m2[w * TS + sidx]);
                sm_s2[wave * TS + sidx] = s2[t] * __expf(m2[t] - M2);
            }
            if (GRAD) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int i = 16 * mt + 4 * g + r;
                        if (i < DP) sm_acc[(wave * DP + i) * TS + sidx] = acc[t][mt][r] * f;
                    }
            }
        }
    }
    ME_LDS_BARRIER();
    // sample si = threadIdx.x (one thread per sample for the log values); 1 / S goes back to LDS for the gradient
    const int si = threadIdx.x;
    if (si < TS) {
        float M = -3.0e38f, S = 0.f;
        for (int w = 0; w < nwaves; ++w) { M = fmaxf(M, sm_m[w * TS + si]); S += sm_s[w * TS + si]; }
        if (si < n_here && lp_out != nullptr) lp_out[n0 + si] = M + __logf(S);
        if (dual && si < n_here && lp2_out != nullptr) {
            float M2 = -3.0e38f, S2 = 0.f;
            for (int w = 0; w < nwaves; ++w) { M2 = fmaxf(M2, sm_m2[w * TS + si]); S2 += sm_s2[w * TS + si]; }
            lp2_out[n0 + si] = M2 + __logf(S2);
        }
        if (GRAD) sm_s[si] = 1.f / S;                  // (row 0 of sm_s is read by this thread only: no hazard)
    }
    if (GRAD && grad_out != nullptr) {
        ME_LDS_BARRIER();
        // thread (dimension i, sample s_i) pairs spread over the workgroup; results go to a [TS][ldx] tile and leave coalesced
        float* outt = sm_acc + (size_t)nwaves * DP * TS;
        for (int e = threadIdx.x; e < D * TS; e += blockDim.x) {
            const int i = e / TS, s_i = e - i * TS;
            float gsum = 0.f;
            for (int w = 0; w < nwaves; ++w) gsum += sm_acc[(w * DP + i) * TS + s_i];
            outt[s_i * ldx + i] = gsum * sm_s[s_i];
        }
        ME_LDS_BARRIER();
        for (int e = threadIdx.x; e < n_here * D; e += blockDim.x)
            grad_out[(size_t)n0 * D + e] = outt[(e / D) * ldx + (e % D)];
    }
}

template <int DP, int NTS>
static int sweep_mfma(gmmvi_ctx* ctx, const SweepArgs& a) {
    using PK = Pack<DP>;
    constexpr int TS = 16 * NTS, KSP = ((PK::KS + 3) / 4) * 4, ZW = 4 * KSP + 4;
    const int K = a.K, D = a.D, N = a.N;
    const float* logw2 = a.logw2;
    const bool want_grad = a.grad != nullptr;
    // The instances the route choice (density.hip) can ask for.  Sub-tiles of 16 samples per wave pass: four (every fragment
    // fetch of a component serves 64 samples) unless the gradient state of the wide dimensions would not fit the registers --
    // from padded D = 40 on the gradient runs at two sub-tiles, and only the gradient does
    const SweepKernel kernel = sweep_instance(a.family, want_grad, [](auto fam, auto g) -> SweepKernel {
        constexpr bool grad = decltype(g)::value;
        if constexpr (NTS == 2 ? (grad && DP >= 40) : (!grad || DP < 40)) return mixture_eval_mfma_kernel<DP, decltype(fam)::value, grad, NTS>;
        else return nullptr;
    });
    if (kernel == nullptr) return gmmvi_fail(ctx, GMMVI_ERR_ARG, "mixture_eval_mfma: no instance for this dimension, gradient and sub-tile count");
    const int env_nw = sweep_env_nw(), env_ky = sweep_env_ky();
    auto lds_floats = [&](int nw) {
        size_t merge = (size_t)nw * TS * ((want_grad ? DP : 0) + 2) + (want_grad ? TS * (size_t)(D | 1) : 0) +
                       (logw2 ? (size_t)nw * 2 * TS : 0);
        size_t stage = TS * (size_t)(D | 1);
        return (want_grad ? (size_t)nw * NTS * 16 * ZW : 0) + (merge > stage ? merge : stage);
    };
    const int tiles = (N + TS - 1) / TS;
    // geometry as for the scalar-fed kernel: ky chunks of components over blockIdx.y (partials merged by combine_partials) so
    // that ~2 workgroups of 8 waves per CU are in flight when there are few sample tiles
    int ky = 1, nw = K < 8 ? K : 8;
    if (env_ky > 0) ky = env_ky < K ? env_ky : K;
    else if (K >= 16 && 2L * tiles <= 3L * ctx->num_cus) {
        ky = (int)((2L * ctx->num_cus + tiles / 2) / tiles);
        if (ky > K / 8) ky = K / 8;
        if (ky < 1) ky = 1;
    }
    const int kchunk = (K + ky - 1) / ky;
    ky = (K + kchunk - 1) / kchunk;
    if (nw > kchunk) nw = kchunk;
    if (env_nw > 0) nw = env_nw < kchunk ? env_nw : kchunk;
    if (nw > 8) nw = 8;
    while (nw > 1 && lds_floats(nw) * 4 > 64 * 1024) --nw;
    size_t shmem = lds_floats(nw) * 4;
    return gmmvi_sweep_launch(ctx, a, {tiles, ky, nw * 64, shmem}, kernel);
}

int gmmvi_sweep_mfma(gmmvi_ctx* ctx, int dp, int sub_tiles, const SweepArgs& a) {
    GMMVI_DISPATCH_DP(dp, if constexpr (Pack<DP>::FRAGS) {
        if (sub_tiles == 2) return sweep_mfma<DP, 2>(ctx, a);
        if (sub_tiles == 4) return sweep_mfma<DP, 4>(ctx, a);
    });
    return gmmvi_fail(ctx, GMMVI_ERR_ARG, "mixture_eval_mfma: no instance for this dimension and sub-tile count");
}
