// The one-sample-per-lane density sweep: the fused {sample tile x component} density / log-sum-exp / gradient kernel of the
// padded dimensions below the matrix-core threshold.
//
// Mapping (DESIGN.md "mixture_eval"): one lane owns one sample (x, z, y and the running gradient live in VGPRs),
// one wave walks a strided subset of the components, a workgroup = 64 samples x W waves.  The component
// parameters are wave-uniform, so they are fetched with scalar loads (s_load_dwordxN through the constant
// cache) and feed v_fma as SGPR operands: no LDS traffic and no per-lane loads in the inner loop.  The triangular
// solve is fully unrolled for the padded dimension DP; partial (max, sum, gradient) of the W waves are merged
// through LDS.
#include "density_sweep.h"
#include "subst_phased.h"
#include <cmath>

#ifdef GMMVI_ME_STAMPS
__device__ long long g_me_wg[2 * 8192];    // experiment builds: wall-clock (100 MHz) start / end of every workgroup of the last launch
__device__ unsigned long long g_me_hw[8192];   // and where it ran (HW_ID, XCC_ID)
extern "C" int gmmvi_debug_wg_times(long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_me_wg), sizeof(long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
extern "C" int gmmvi_debug_wg_hw(unsigned long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_me_hw), sizeof(unsigned long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
__device__ long long g_me_ph[1024 * 16 * 16];  // packed kernel: 16 wall-clock phase stamps of every wave of the first 1024 workgroups
extern "C" int gmmvi_debug_wg_phases(long long* out, int n) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_me_ph), sizeof(long long) * (size_t)n) == hipSuccess ? 0 : -1;
}
#endif
template <int DP, int FAMILY, bool GRAD>
__global__ __launch_bounds__(DP >= GMMVI_ME_WIDE_DP ? 512 : GMMVI_ME_THREADS, GMMVI_ME_MINW) void mixture_eval_kernel(float nu, int K_total, int D, const float* __restrict__ packed,
                                                            const float* __restrict__ logw, const float* __restrict__ X,
                                                            int N, float* __restrict__ ld_out, float* __restrict__ lp_out,
                                                            float* __restrict__ grad_out, const float* __restrict__ logw2,
                                                            float* __restrict__ lp2_out, CombineJob carried, Riders riders) {
    using PK = Pack<DP>;
    extern __shared__ __align__(16) float sm[];
    if (combine_carried(carried) || riders_carried<DP>(riders, sm)) return;   // workgroups past the sample tiles: the merge of the previous sweep, riders
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
    const int n0 = blockIdx.x * 64;
    const int n_here = min(64, N - n0);
    const int n = n0 + lane;
    const bool valid = lane < n_here;
    float* sm_merge = sm;                              // staging, then the merge area
#ifdef GMMVI_ME_STAMPS             // experiment builds (tools/bench_sweep.py): phase time stamps of one wave
    if (threadIdx.x == 0) {
        g_me_wg[2 * (blockIdx.y * gridDim.x + blockIdx.x)] = wall_clock64();
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        g_me_hw[blockIdx.y * gridDim.x + blockIdx.x] = ((unsigned long long)xcc << 32) | hw;
    }
    unsigned long long stamp[16];
    int nstamp = 0, nbackward = 0;
    const long long wc0 = wall_clock64();
#define ME_STAMP() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); if (nstamp < 16) stamp[nstamp++] = __builtin_amdgcn_s_memtime(); } while (0)
    ME_STAMP();
#else
#define ME_STAMP()
#endif

    // ---- x tile: rows that are a whole number of 16- or 8-byte pieces are read straight into the lane's registers (lane = sample:
    // the loads of a row walk the same cache lines, the W waves of the workgroup hit in L1); other shapes are staged
    // through LDS with a coalesced load (rows of a row-major [N, D] array are 4D bytes apart) ---------------------------
    const int ldx = D | 1;
    float x[DP];
    if (DP % 4 == 0 && D == DP && (reinterpret_cast<uintptr_t>(X) & 15) == 0) {
        const float4* xrow = reinterpret_cast<const float4*>(X + (size_t)min(n, N - 1) * D);
#pragma unroll
        for (int q4 = 0; q4 < DP / 4; ++q4) {
            const float4 v4 = xrow[q4];
            x[4 * q4] = v4.x; x[4 * q4 + 1] = v4.y; x[4 * q4 + 2] = v4.z; x[4 * q4 + 3] = v4.w;
        }
        if (!valid) {
#pragma unroll
            for (int i = 0; i < DP; ++i) x[i] = 0.f;
        }
    } else if (DP % 2 == 0 && D == DP && (reinterpret_cast<uintptr_t>(X) & 7) == 0) {       // 8-byte pieces (D = 10)
        const float2* xrow = reinterpret_cast<const float2*>(X + (size_t)min(n, N - 1) * D);
#pragma unroll
        for (int q2 = 0; q2 < DP / 2; ++q2) {
            const float2 v2 = xrow[q2];
            x[2 * q2] = v2.x; x[2 * q2 + 1] = v2.y;
        }
        if (!valid) {
#pragma unroll
            for (int i = 0; i < DP; ++i) x[i] = 0.f;
        }
    } else {
        for (int e = threadIdx.x; e < n_here * D; e += blockDim.x) sm_merge[(e / D) * ldx + (e % D)] = X[(size_t)n0 * D + e];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < DP; ++i) x[i] = (valid && i < D) ? sm_merge[lane * ldx + i] : 0.f;
        __syncthreads();
    }

    float m = -3.0e38f, s = 0.f;
    float m2 = -3.0e38f, s2 = 0.f;                      // second mixture over the same components (logw2), optional
    const bool dual = logw2 != nullptr;
    float acc[GRAD ? DP : 1];
    if (GRAD) {
#pragma unroll
        for (int i = 0; i < DP; ++i) acc[i] = 0.f;
    }
    const float nud = nu + (float)D;
    ME_STAMP();

    for (int k = k_lo + wave; k < K; k += nwaves) {
        ME_STAMP();
        // the block through a constant-address-space pointer, its loads software-pipelined (subst_phased.h)
        const sp_block_ptr blk = sp_block(packed + (size_t)k * PK::STRIDE);
        const float lw = ((sp_const_f32)(uintptr_t)logw)[k];
        const float lw2 = dual ? ((sp_const_f32)(uintptr_t)logw2)[k] : 0.f;
        float z[DP], vrd[DP], q, cst;
        float pc[2][32];
        SpPass<DP>::forward(blk, x, z, vrd, q, cst, pc);
        // the rows again for the backward pass, through a pointer the compiler cannot identify with the first one: otherwise it
        // keeps the values both passes share alive in VGPR lanes instead of loading them again
        sp_block_ptr blkb = blk;
        asm volatile("" : "+s"(blkb));
        if constexpr (GRAD) SpPass<DP>::backward_prefetch(blkb, pc);
        float ld, coef;
        if (FAMILY == GMMVI_GAUSS) {
            ld = fmaf(-0.5f, q, cst);
            coef = -1.f;
        } else {
            ld = cst - 0.5f * nud * log1pf(q / nu);
            coef = -nud / (nu + q);
        }
        const float a = ld + lw;
        const float mn = fmaxf(m, a);
        const float sc = __expf(m - mn);
        const float e = __expf(a - mn);
        s = fmaf(s, sc, e);
        m = mn;
        if (dual) {
            const float a2 = ld + lw2;
            const float mn2 = fmaxf(m2, a2);
            s2 = fmaf(s2, __expf(m2 - mn2), __expf(a2 - mn2));
            m2 = mn2;
        }
        if constexpr (GRAD) {
            SpPass<DP>::backward(blkb, z, vrd, pc);
            const float ec = e * coef;
#pragma unroll
            for (int i = 0; i < DP; ++i) acc[i] = fmaf(acc[i], sc, ec * z[i]);
            sp_pin<DP>(acc);
        }
        // (the store comes last: a branch in the middle of the pass would split it into basic blocks, and the optimiser then
        // sinks the multiply-adds of the backward substitution behind all the loads of its pieces)
        if (ld_out != nullptr && valid) ld_out[(size_t)k * N + n] = ld;
    }
    ME_STAMP();
    if (lp_out == nullptr && !GRAD) return;

    // merge the W waves' partials.  Round 1: the running maxima meet in LDS, every wave rescales ITS sums to the common
    // maximum (one exp per lane instead of one per (wave, dimension) pair in the reduction); round 2: plain sums in wave
    // order.  sm_m[w][lane], sm_s[w][lane], sm_acc[w][quad][lane] (four dimensions per 16-byte LDS access).
    // The barriers wait for LDS traffic only (ME_LDS_BARRIER): __syncthreads() also drains the global stores of the log
    // densities, ~4 000 cycles at the first barrier (profiles/r03_notes.md).
    constexpr int NQ = (DP + 3) / 4;
    float* sm_m = sm_merge;
    float* sm_s = sm_merge + nwaves * 64;
    me_f32x4* sm_acc = reinterpret_cast<me_f32x4*>(sm_merge + 2 * nwaves * 64);
    float* outt = sm_merge + 2 * nwaves * 64 + (GRAD ? (size_t)nwaves * NQ * 256 : 0);       // [64][ldx] tile of the result
    float* sm_m2 = outt + (GRAD ? 64 * ldx : 0);
    float* sm_s2 = sm_m2 + nwaves * 64;
    sm_m[wave * 64 + lane] = m;
    if (dual) sm_m2[wave * 64 + lane] = m2;
    ME_LDS_BARRIER();
    ME_STAMP();
    float M = -3.0e38f, M2 = -3.0e38f;
    for (int w = 0; w < nwaves; ++w) M = fmaxf(M, sm_m[w * 64 + lane]);
    const float f = __expf(m - M);
    sm_s[wave * 64 + lane] = s * f;
    if (dual) {
        for (int w = 0; w < nwaves; ++w) M2 = fmaxf(M2, sm_m2[w * 64 + lane]);
        sm_s2[wave * 64 + lane] = s2 * __expf(m2 - M2);
    }
    if (GRAD) {
#pragma unroll
        for (int q4 = 0; q4 < NQ; ++q4) {
            me_f32x4 v4;
#pragma unroll
            for (int c = 0; c < 4; ++c) v4[c] = 4 * q4 + c < DP ? acc[4 * q4 + c] * f : 0.f;
            sm_acc[(wave * NQ + q4) * 64 + lane] = v4;
        }
    }
    ME_STAMP();
    ME_LDS_BARRIER();
    ME_STAMP();
    float S = 0.f;
    for (int w = 0; w < nwaves; ++w) S += sm_s[w * 64 + lane];
    if (wave == 0 && valid && lp_out != nullptr) lp_out[n] = M + __logf(S);
    if (dual && wave == (nwaves > 1 ? 1 : 0) && valid && lp2_out != nullptr) {
        float S2 = 0.f;
        for (int w = 0; w < nwaves; ++w) S2 += sm_s2[w * 64 + lane];
        lp2_out[n] = M2 + __logf(S2);
    }
    if (GRAD && grad_out != nullptr) {
        const float inv = 1.f / S;
        // wave w reduces the dimension quads w, w + W, ...; results go to the [64][ldx] tile and leave coalesced
        for (int q4 = wave; q4 < NQ; q4 += nwaves) {
            me_f32x4 g4 = {0.f, 0.f, 0.f, 0.f};
            for (int w = 0; w < nwaves; ++w) g4 += sm_acc[(w * NQ + q4) * 64 + lane];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (4 * q4 + c < D) outt[lane * ldx + 4 * q4 + c] = g4[c] * inv;
        }
        ME_STAMP();
        ME_LDS_BARRIER();
        ME_STAMP();
        for (int e = threadIdx.x; e < n_here * D; e += blockDim.x)
            grad_out[(size_t)n0 * D + e] = outt[(e / D) * ldx + (e % D)];
    }
#ifdef GMMVI_ME_STAMPS
    ME_STAMP();
    if (threadIdx.x == 0) g_me_wg[2 * (blockIdx.y * gridDim.x + blockIdx.x) + 1] = wall_clock64();
    if (GRAD && logw2 && blockIdx.x == 60 && blockIdx.y == 1 && threadIdx.x == 64 * 3 && (g_me_wg[2 * 8192 - 1]++ & 15) == 12) {
        const long long wc1 = wall_clock64();
        printf("me stamps (shader cycles; kernel %lld x 10 ns by the 100 MHz clock):", wc1 - wc0);
        for (int i = 1; i < nstamp; ++i) printf(" %llu", stamp[i] - stamp[i - 1]);
        printf("  total %llu, backward passes %d\n", stamp[nstamp - 1] - stamp[0], nbackward);
    }
#endif
}

static size_t reg_env_shmem_min() {       // experiments: caps the workgroups per CU
    static const size_t v = getenv("GMMVI_ME_SHMEM_MIN") ? (size_t)atol(getenv("GMMVI_ME_SHMEM_MIN")) : 0;
    return v;
}

template <int DP>
static int sweep_reg(gmmvi_ctx* ctx, const SweepArgs& a) {
    const int K = a.K, D = a.D, N = a.N;
    const float* logw2 = a.logw2;
    const bool want_grad = a.grad != nullptr;
    const int env_nw = sweep_env_nw(), env_ky = sweep_env_ky();
    auto lds_floats = [&](int nw) {
        size_t merge = (size_t)nw * 64 * ((want_grad ? (DP + 3) / 4 * 4 : 0) + 2) + (want_grad ? 64 * (size_t)(D | 1) : 0) +
                       (logw2 ? (size_t)nw * 128 : 0);
        size_t stage = 64 * (size_t)(D | 1);
        return merge > stage ? merge : stage;
    };
    const int tiles = (N + 63) / 64;
    // geometry: ky chunks of components over blockIdx.y (partials merged by combine_partials), nw waves per workgroup.
    // Measured on MI355X (tools/tune_mixture_eval.py; profiles/r01_notes.md): with few sample tiles (N = 10^4: 157) one
    // 16-wave workgroup per tile leaves 40 % of the CUs idle; 8 waves per workgroup and K split so that ~2 workgroups per CU
    // are in flight is 11-13 % faster including the (coalesced) combine launch.  Plenty of tiles: 16 waves, no split.
    const int nw_max = DP >= GMMVI_ME_WIDE_DP ? 8 : 16;
    int ky = 1, nw = K < nw_max ? K : nw_max;
    if (env_ky > 0) ky = env_ky < K ? env_ky : K;
    else if (K >= 16 && 2L * tiles <= 3L * ctx->num_cus) {
        ky = (int)((2L * ctx->num_cus + tiles / 2) / tiles);
        if (ky > K / 8) ky = K / 8;
        if (ky < 1) ky = 1;
        if (ky > 1) nw = 8;
    }
    const int kchunk = (K + ky - 1) / ky;
    ky = (K + kchunk - 1) / kchunk;
    if (nw > kchunk) nw = kchunk;
    if (env_nw > 0) nw = env_nw < kchunk ? env_nw : kchunk;
    if (nw > nw_max) nw = nw_max;
    while (nw > 1 && lds_floats(nw) * 4 > 96 * 1024) --nw;
    size_t shmem = lds_floats(nw) * 4;
    const size_t env_shmem_min = reg_env_shmem_min();
    if (shmem < env_shmem_min) shmem = env_shmem_min;
    const SweepKernel kernel = sweep_instance(a.family, want_grad, [](auto fam, auto g) -> SweepKernel {
        return mixture_eval_kernel<DP, decltype(fam)::value, decltype(g)::value>;
    });
    return gmmvi_sweep_launch(ctx, a, {tiles, ky, nw * 64, shmem}, kernel);
}

int gmmvi_sweep_reg(gmmvi_ctx* ctx, int dp, const SweepArgs& a) {
    // (from the matrix-core threshold on the blocks carry the operand fragments and the route choice never comes here)
    GMMVI_DISPATCH_DP(dp, if constexpr (!Pack<DP>::FRAGS) return sweep_reg<DP>(ctx, a));
    return gmmvi_fail(ctx, GMMVI_ERR_ARG, "mixture_eval: no scalar-fed instance for this dimension");
}

#ifdef GMMVI_ME_STAMPS
// experiment builds: the packed kernel writes the stamp buffers above too, and device symbols do not cross translation units,
// so it is compiled as part of this one (tools/build_stamps.sh leaves its own object out of the link)
#include "density_pk.hip"
#endif
