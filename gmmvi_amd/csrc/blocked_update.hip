// Component updates of the blocked path (blocked.h: 50 < D <= 512): the KL-constrained update and the direct / iBLR updates, as
// launch sequences over the batched contraction (blocked_gemm.h) and one-workgroup-per-component kernels (blocked_factor.h).
#include "blocked_gemm.h"
#include "blocked_factor.h"
#include "trust_region.h"

// update_kl.hip UKL_TAIL_MIN: a column of the whitened M whose tail sum of squares is at most this counts as already tridiagonal
// (negligible against the unit diagonal of B = I + M / eta; in the fp32 subnormal range 1 / (nrm^2 - alpha x1) overflows)
#define BLK_TAIL_MIN 1e-30f

// ---------------------------------------------------------------------------------------------------------------------------
// KL-constrained component update (ng_based_component_updater.py:431-524): the whitened / tridiagonal route of update_kl.hip
// with the D x D matrices in global memory (L2-resident), one workgroup per component and step.
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// R_sym (lower triangle mirrored, as tf.linalg.cholesky reads it) and g~ = g_neg + (R_sym - R) mu
__global__ __launch_bounds__(256) void blk_upd_prep_kernel(int D, const float* __restrict__ H_neg, const float* __restrict__ g_neg,
                                                           const float* __restrict__ means, float* __restrict__ Rs,
                                                           float* __restrict__ gt) {
    const int k = blockIdx.x;
    const float* R = H_neg + (size_t)k * D * D;
    const float* mu = means + (size_t)k * D;
    float* o = Rs + (size_t)k * D * D;
    for (int e = blockIdx.y * 256 + threadIdx.x; e < D * D; e += gridDim.y * 256) {
        const int i = e / D, j = e % D;
        o[e] = (j <= i) ? R[e] : R[(size_t)j * D + i];
    }
    for (int t = blockIdx.y * 256 + threadIdx.x; t < D; t += gridDim.y * 256) {
        // four independent partial sums: the loads of four terms are in flight together (one chain of D dependent
        // load + multiply-add steps made this loop 100 of the kernel's 112 us at D = 300)
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        int j = t + 1;
        for (; j + 3 < D; j += 4) {
            a0 = fmaf(R[(size_t)j * D + t] - R[(size_t)t * D + j], mu[j], a0);
            a1 = fmaf(R[(size_t)(j + 1) * D + t] - R[(size_t)t * D + j + 1], mu[j + 1], a1);
            a2 = fmaf(R[(size_t)(j + 2) * D + t] - R[(size_t)t * D + j + 2], mu[j + 2], a2);
            a3 = fmaf(R[(size_t)(j + 3) * D + t] - R[(size_t)t * D + j + 3], mu[j + 3], a3);
        }
        for (; j < D; ++j) a0 = fmaf(R[(size_t)j * D + t] - R[(size_t)t * D + j], mu[j], a0);
        gt[(size_t)k * D + t] = g_neg[(size_t)k * D + t] + ((a0 + a1) + (a2 + a3));
    }
}

// M <- (M + M^T)/2, copy to Mc; w = L^T g~ (also the vector the reflectors act on)
__global__ __launch_bounds__(256) void blk_upd_sym_kernel(int D, const float* __restrict__ chols, const float* __restrict__ gt,
                                                          float* __restrict__ M, float* __restrict__ Mc, float* __restrict__ w,
                                                          float* __restrict__ wt) {
    const int k = blockIdx.x;
    float* Mk = M + (size_t)k * D * D;
    float* Ck = Mc + (size_t)k * D * D;
    const float* L = chols + (size_t)k * D * D;
    for (int e = blockIdx.y * 256 + threadIdx.x; e < D * D; e += gridDim.y * 256) {
        const int i = e / D, j = e % D;
        if (j < i) {
            const float m = 0.5f * (Mk[e] + Mk[(size_t)j * D + i]);
            Mk[e] = m; Mk[(size_t)j * D + i] = m;
            Ck[e] = m; Ck[(size_t)j * D + i] = m;
        } else if (j == i) {
            Ck[e] = Mk[e];
        }
    }
    for (int t = blockIdx.y * 256 + threadIdx.x; t < D; t += gridDim.y * 256) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;              // four independent partial sums (as in blk_upd_prep_kernel)
        const float* gk = gt + (size_t)k * D;
        int c = t;
        for (; c + 3 < D; c += 4) {
            a0 = fmaf(L[(size_t)c * D + t], gk[c], a0);
            a1 = fmaf(L[(size_t)(c + 1) * D + t], gk[c + 1], a1);
            a2 = fmaf(L[(size_t)(c + 2) * D + t], gk[c + 2], a2);
            a3 = fmaf(L[(size_t)(c + 3) * D + t], gk[c + 3], a3);
        }
        for (; c < D; ++c) a0 = fmaf(L[(size_t)c * D + t], gk[c], a0);
        const float a = (a0 + a1) + (a2 + a3);
        w[(size_t)k * D + t] = a;
        wt[(size_t)k * D + t] = a;
    }
}

// Householder tridiagonalisation of the symmetric M (in place) with the reflectors applied to wt.  Thread (i, grp): column
// i of the trailing block, rows j = c+1+grp, +G, ... (coalesced over i, eight loads in flight); partial products meet in
// LDS.  ONE sweep over the trailing block per step: the rank-2 update of step c (M -= v q^T + q v^T, exactly symmetric)
// and the product M' v' for the reflector of step c+1 share it -- the next reflector only needs row c+1 of the updated
// matrix, which is formed first (one element per thread).
__global__ __launch_bounds__(1024) void blk_tridiag_kernel(int D, int DT, int G, float* __restrict__ Mall,
                                                           float* __restrict__ wt_all, float* __restrict__ td_all,
                                                           float* __restrict__ te_all) {
    extern __shared__ float sm[];
    float* va = sm;                       // reflector of the current step
    float* vb = sm + D;                   // reflector of the next step
    float* q = sm + 2 * D;
    float* xn = sm + 3 * D;               // row c+1 of the updated matrix
    float* part = sm + 4 * D;
    float* red = part + (size_t)G * DT;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int i = tid % DT, grp = tid / DT;
    float* M = Mall + (size_t)k * D * D;
    float* te = te_all + (size_t)k * D;
    const bool g0 = grp == 0 && i < D;
    float wti = g0 ? wt_all[(size_t)k * D + i] : 0.f;

    // reflector for column c from its sub-diagonal part x (x_i = value of thread i, group 0): v_i, beta; alpha or the
    // untouched sub-diagonal entry goes to te[c].  All results block-uniform except vi.
    float beta = 0.f, vi = 0.f, p = 0.f;
    auto make_reflector = [&](int c, float xi, float x1, float* vdst) {
        const bool mine = g0 && i > c;
        const float tail = block_sum_nb((mine && i > c + 1) ? xi * xi : 0.f, red + 32);
        float v_here = 0.f;
        if (!(tail > BLK_TAIL_MIN)) {              // column already tridiagonal (NaN lands here too: handled by the search)
            beta = 0.f;
            if (tid == 0) te[c] = x1;
        } else {
            const float nrm = sqrtf(tail + x1 * x1);
            const float alpha = (x1 > 0.f) ? -nrm : nrm;
            beta = 1.f / (nrm * nrm - alpha * x1);
            v_here = mine ? (i == c + 1 ? x1 - alpha : xi) : 0.f;
            if (tid == 0) te[c] = alpha;
        }
        if (g0) vdst[i] = v_here;
        return v_here;
    };

    if (D >= 3) {
        // step 0: reflector of column 0, p = beta M v by a plain sweep
        const float x1 = M[1];
        const float xi = (g0 && i > 0) ? M[i] : 0.f;
        vi = make_reflector(0, xi, x1, va);
        __syncthreads();
        float a0 = 0.f;
        if (i > 0 && i < D) {
            float av[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int j = 1 + grp;
            for (; j + 7 * G < D; j += 8 * G) {
#pragma unroll
                for (int u = 0; u < 8; ++u) av[u] = fmaf(M[(size_t)(j + u * G) * D + i], va[j + u * G], av[u]);
            }
            for (; j < D; j += G) a0 = fmaf(M[(size_t)j * D + i], va[j], a0);
            a0 += ((av[0] + av[1]) + (av[2] + av[3])) + ((av[4] + av[5]) + (av[6] + av[7]));
        }
        part[grp * DT + i] = a0;
        __syncthreads();
        p = 0.f;
        if (g0 && i > 0) {
            for (int gi = 0; gi < G; ++gi) p += part[gi * DT + i];
            p *= beta;
        }
    }
    float* v = va;
    float* v2 = vb;
    for (int c = 0; c + 2 < D; ++c) {
        float s_vp = vi * p, s_vw = vi * wti;
        block_sum2_nb(s_vp, s_vw, red);         // red[0..31]; the reflector norm uses red[32..47]
        const float kk = 0.5f * beta * s_vp;
        const float wdot = beta * s_vw;
        if (g0) q[i] = (i > c) ? p - kk * vi : 0.f;
        wti -= wdot * vi;
        __syncthreads();
        const bool more = c + 3 < D;                   // another reflector follows
        float beta_n = 0.f, vi_n = 0.f;
        if (more) {
            // row c+1 of the updated matrix: its entries right of the diagonal are the next column
            float xv = 0.f;
            if (g0 && i > c) {
                xv = M[(size_t)(c + 1) * D + i] - __fadd_rn(__fmul_rn(v[c + 1], q[i]), __fmul_rn(q[c + 1], v[i]));
                xn[i] = xv;
            }
            __syncthreads();
            const float x1n = xn[c + 2];
            const float beta_keep = beta;
            vi_n = make_reflector(c + 1, (g0 && i > c + 1) ? xv : 0.f, x1n, v2);
            beta_n = beta;
            beta = beta_keep;
            __syncthreads();
        }
        // one sweep: M[j][i] -= v_j q_i + q_j v_i, and the partial product with the next reflector
        float a0 = 0.f;
        if (i > c && i < D) {
            const float vi2 = v[i], qi2 = q[i];
            float av[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int j = c + 1 + grp;
            for (; j + 7 * G < D; j += 8 * G) {
                float mv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) mv[u] = M[(size_t)(j + u * G) * D + i];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int jj = j + u * G;
                    const float m = mv[u] - __fadd_rn(__fmul_rn(v[jj], qi2), __fmul_rn(q[jj], vi2));
                    M[(size_t)jj * D + i] = m;
                    if (more) av[u] = fmaf(m, v2[jj], av[u]);
                }
            }
            for (; j < D; j += G) {
                const float m = M[(size_t)j * D + i] - __fadd_rn(__fmul_rn(v[j], qi2), __fmul_rn(q[j], vi2));
                M[(size_t)j * D + i] = m;
                if (more) a0 = fmaf(m, v2[j], a0);
            }
            a0 += ((av[0] + av[1]) + (av[2] + av[3])) + ((av[4] + av[5]) + (av[6] + av[7]));
        }
        part[grp * DT + i] = a0;
        __syncthreads();
        p = 0.f;
        if (more && g0 && i > c + 1) {
            for (int gi = 0; gi < G; ++gi) p += part[gi * DT + i];
            p *= beta_n;
        }
        beta = beta_n;
        vi = vi_n;
        float* tsw = v; v = v2; v2 = tsw;
    }
    __syncthreads();
    if (g0) {
        td_all[(size_t)k * D + i] = M[(size_t)i * D + i];
        wt_all[(size_t)k * D + i] = wti;
        if (i == D - 1 && D >= 2) te[D - 2] = M[(size_t)(D - 1) * D + D - 2];
    }
}

// The same reduction with the matrix in REGISTERS (D <= 320): NW = 8 wavefronts (two per SIMD: 256 registers a thread),
// wavefront tj owns rows j = tj + NW a (a < BR), lane l columns i = l + 64 b (b < BC), a thread keeps its BR x BC elements for
// the whole kernel (D = 300: 38 x 5 on 512 threads, 380 KB of the CU's 512 KB register file; with 16 wavefronts the 128
// registers a thread gets spill ~20 of them to scratch and the kernel is no faster than the global-memory one) -- a step no longer streams the trailing block through the L2 (the
// global-memory kernel above is bound by the ~8 loads a thread keeps in flight: 8 us per step at D = 300).  Per step a thread
// needs the reflector vectors at its rows (uniform in the wavefront: 16-byte broadcast reads from a copy stored in row order
// [tj][a]) and at its columns (one value per lane), 3 BR + 2 BC values for BR BC elements.  Rows / columns that are already
// reduced see v = q = 0 and stay bit-exact; whole 4-row blocks and 64-column blocks of them are skipped.  (The update is
// symmetric up to the rounding of the fused multiply-add the compiler contracts it to.)  Row c+1 of the
// matrix (the source of the next reflector) lives in one wavefront, one value per lane and column block: it goes to LDS.  The per-column state
// (p, v_i, the running w~) lives in thread i.  Four barriers per step: every thread recomputes q_{c+1} from the partial
// sums, so the next column can be formed without waiting for q.
__device__ __forceinline__ float blk_q_elem(float p, float kk, float v) { return p - kk * v; }

template <int NW, int BR, int BC>
__global__ __launch_bounds__(64 * NW) void blk_tridiag_reg_kernel(int D, const float* __restrict__ Mall, float* __restrict__ wt_all,
                                                               float* __restrict__ td_all, float* __restrict__ te_all) {
    constexpr int RBP = (BR + 3) / 4 * 4;          // row slots per wavefront in the row-order copies
    constexpr int NBK = RBP / 4;
    constexpr int DT = 64 * BC;
    constexpr int NWS = NW == 16 ? 4 : (NW == 8 ? 3 : 2);           // log2(NW)
    static_assert(NW == 16 || NW == 8 || NW == 4, "row classes: a power of two");
    static_assert(64 * NW >= DT, "one state thread per column");
    extern __shared__ __align__(16) float sm[];
    float* vNa = sm;                               // reflector (two buffers: current / next), natural order
    float* vNb = sm + DT;
    float* qN = sm + 2 * DT;
    float* xn = sm + 3 * DT;                       // row c+1
    float* vRa = sm + 4 * DT;                      // the same vectors in row order: element j at (j % NW) RBP + j / NW
    float* vRb = sm + 4 * DT + NW * RBP;
    float* qR = sm + 4 * DT + 2 * NW * RBP;
    float* part = sm + 4 * DT + 3 * NW * RBP;      // [NW][DT] partial products
    float* red = part + NW * DT;                   // [48]
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int tj = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* M = Mall + (size_t)k * D * D;
    float* te = te_all + (size_t)k * D;
    const int i = tid;                             // the column whose state this thread keeps
    const bool cs = tid < D;
    const int pr = (i & (NW - 1)) * RBP + (i >> NWS);
    float wti = cs ? wt_all[(size_t)k * D + i] : 0.f;
    for (int e = tid; e < 4 * DT + 3 * NW * RBP; e += 64 * NW) sm[e] = 0.f;

    float m[BR][BC];
#pragma unroll
    for (int a = 0; a < BR; ++a)
#pragma unroll
        for (int b = 0; b < BC; ++b) {
            const int j = tj + NW * a, ci = lane + 64 * b;
            m[a][b] = (j < D && ci < D) ? M[(size_t)j * D + ci] : 0.f;
        }
    __syncthreads();

    // reflector from the sub-diagonal part x of a column (x_i in thread i), tail = sum_{i > c+1} x_i^2: writes v (both orders),
    // alpha or the untouched sub-diagonal entry to te[c]; returns v_i, sets beta_out
    auto reflector = [&](int c, float xi, float x1, float tail, int buf, float& beta_out) {
        float v_here = 0.f;
        if (!(tail > BLK_TAIL_MIN)) {              // column already tridiagonal (NaN lands here too: handled by the search)
            beta_out = 0.f;
            if (tid == 0) te[c] = x1;
        } else {
            const float nrm = sqrtf(tail + x1 * x1);
            const float alpha = (x1 > 0.f) ? -nrm : nrm;
            beta_out = 1.f / (nrm * nrm - alpha * x1);
            v_here = (cs && i > c) ? (i == c + 1 ? x1 - alpha : xi) : 0.f;
            if (tid == 0) te[c] = alpha;
        }
        if (cs) { (buf ? vNb : vNa)[i] = v_here; (buf ? vRb : vRa)[pr] = v_here; }
        return v_here;
    };
    auto column_sum = [&](int col) {               // fixed order over the NW row classes
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < NW; ++g) s += part[g * DT + col];
        return s;
    };

    float beta = 0.f, vi = 0.f, p = 0.f, pc1 = 0.f;
    if (D >= 3) {
        // step 0: reflector of column 0, p = beta M v
        const float x1 = M[1];
        const float xi = (cs && i > 0) ? M[i] : 0.f;
        float t2 = gmmvi_wave_sum((cs && i > 1) ? xi * xi : 0.f);
        if (lane == 0) red[32 + tj] = t2;
        __syncthreads();
        float tail = 0.f;
#pragma unroll
        for (int g = 0; g < NW; ++g) tail += red[32 + g];
        vi = reflector(0, xi, x1, tail, 0, beta);
        __syncthreads();
        {
            float acc[BC];
#pragma unroll
            for (int b = 0; b < BC; ++b) acc[b] = 0.f;
#pragma unroll
            for (int a = 0; a < BR; ++a) {
                const float vr = vRa[tj * RBP + a];
#pragma unroll
                for (int b = 0; b < BC; ++b) acc[b] = fmaf(m[a][b], vr, acc[b]);
            }
#pragma unroll
            for (int b = 0; b < BC; ++b) part[tj * DT + lane + 64 * b] = acc[b];
        }
        __syncthreads();
        p = (cs && i > 0) ? beta * column_sum(i) : 0.f;
        pc1 = beta * column_sum(1);
    }
    int cur = 0;
#ifdef GMMVI_TRI_STAMPS
    long long tacc[6] = {0, 0, 0, 0, 0, 0}, tprev = wall_clock64();
#define TRI_STAMP(x) do { const long long tn = wall_clock64(); tacc[x] += tn - tprev; tprev = tn; } while (0)
#else
#define TRI_STAMP(x)
#endif
    for (int c = 0; c + 2 < D; ++c) {
        const bool more = c + 3 < D;                   // another reflector follows
        const int a_lo = c >= tj ? ((c - tj) >> NWS) + 1 : 0;             // first live row slot of this wavefront (rows > c)
        const int b_lo = (c + 1) >> 6;                                 // first column block with a live column
        const float* vNc = cur ? vNb : vNa;
        const float* vRc = (cur ? vRb : vRa) + tj * RBP;
        // row c+1 (not yet updated) into LDS: it lives in ONE wavefront (tj = (c+1) % NW, slot (c+1) / NW), spread over the lanes
        if (more && tj == ((c + 1) & (NW - 1))) {
            // run-time (uniform) slot -> static register index: two levels of scalar branches
            const int asel = (c + 1) >> NWS, ahi = asel >> 3, alo = asel & 7;
#pragma unroll
            for (int hi = 0; hi < (BR + 7) / 8; ++hi) {
                if (hi == ahi) {
#pragma unroll
                    for (int lo = 0; lo < 8; ++lo) {
                        if (8 * hi + lo < BR && lo == alo) {
#pragma unroll
                            for (int b = 0; b < BC; ++b) xn[lane + 64 * b] = m[8 * hi + lo][b];
                        }
                    }
                }
            }
        }
        float s_vp = gmmvi_wave_sum(vi * p), s_vw = gmmvi_wave_sum(vi * wti);
        if (lane == 0) { red[tj] = s_vp; red[16 + tj] = s_vw; }
        TRI_STAMP(0);
        __syncthreads();                                                               // 1
        TRI_STAMP(1);
        s_vp = 0.f; s_vw = 0.f;
#pragma unroll
        for (int g = 0; g < NW; ++g) { s_vp += red[g]; s_vw += red[16 + g]; }
        const float kk = 0.5f * beta * s_vp;
        const float wdot = beta * s_vw;
        const float q_i = (cs && i > c) ? blk_q_elem(p, kk, vi) : 0.f;
        if (cs) { qN[i] = q_i; qR[pr] = q_i; }
        wti -= wdot * vi;
        float beta_n = 0.f, vi_n = 0.f, xv = 0.f;
        if (more) {
            // row c+1 of the updated matrix: its entries right of the diagonal are the next column
            const float vc1 = vNc[c + 1];
            const float qc1 = blk_q_elem(pc1, kk, vc1);
            if (cs && i > c) {
                xv = xn[i] - __fadd_rn(__fmul_rn(vc1, q_i), __fmul_rn(qc1, vi));
                xn[i] = xv;
            }
            const float t2 = gmmvi_wave_sum((cs && i > c + 2) ? xv * xv : 0.f);
            if (lane == 0) red[32 + tj] = t2;
        }
        __syncthreads();                                                               // 2
        TRI_STAMP(2);
        if (more) {
            float tail = 0.f;
#pragma unroll
            for (int g = 0; g < NW; ++g) tail += red[32 + g];
            vi_n = reflector(c + 1, (cs && i > c + 1) ? xv : 0.f, xn[c + 2], tail, cur ^ 1, beta_n);
        }
        __syncthreads();                                                               // 3
        TRI_STAMP(3);
        // one sweep: M[j][i] -= v_j q_i + q_j v_i, and the partial product with the next reflector.  Row blocks outermost: the
        // three 16-byte broadcast reads of a block serve all the thread's column blocks
        {
            const float* vRn = (cur ? vRa : vRb) + tj * RBP;
            const float* qRc = qR + tj * RBP;
            float vcb[BC], qcb[BC], acc[BC];
#pragma unroll
            for (int b = 0; b < BC; ++b) {
                vcb[b] = vNc[lane + 64 * b]; qcb[b] = qN[lane + 64 * b];
                acc[b] = 0.f;
            }
#pragma unroll
            for (int blk = 0; blk < NBK; ++blk) {
                if (4 * blk + 3 >= a_lo) {
                    const float4 v4 = *reinterpret_cast<const float4*>(vRc + 4 * blk);
                    const float4 q4 = *reinterpret_cast<const float4*>(qRc + 4 * blk);
                    const float4 w4 = *reinterpret_cast<const float4*>(vRn + 4 * blk);
                    const float vv[4] = {v4.x, v4.y, v4.z, v4.w}, qq[4] = {q4.x, q4.y, q4.z, q4.w};
                    const float ww[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                    for (int b = 0; b < BC; ++b) {
                        if (b >= b_lo) {
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                if (4 * blk + u < BR) {
                                    const float mn = m[4 * blk + u][b] - __fadd_rn(__fmul_rn(vv[u], qcb[b]), __fmul_rn(qq[u], vcb[b]));
                                    m[4 * blk + u][b] = mn;
                                    acc[b] = fmaf(mn, ww[u], acc[b]);
                                }
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < BC; ++b)
                if (b >= b_lo) part[tj * DT + lane + 64 * b] = acc[b];
        }
        TRI_STAMP(4);
        __syncthreads();                                                               // 4
        p = (more && cs && i > c + 1) ? beta_n * column_sum(i) : 0.f;
        pc1 = more ? beta_n * column_sum(c + 2) : 0.f;
        beta = beta_n;
        vi = vi_n;
        cur ^= 1;
        TRI_STAMP(5);
    }
#ifdef GMMVI_TRI_STAMPS
    if (blockIdx.x == 0 && (tid == 0 || tid == 64 * NW - 1))
        printf("tridiag stamps (100 MHz ticks) tid %d: dump+sums %lld, barrier1 %lld, q/xv+barrier2 %lld, reflector+barrier3 %lld, sweep %lld, barrier4+colsum %lld\n",
               tid, tacc[0], tacc[1], tacc[2], tacc[3], tacc[4], tacc[5]);
#endif
#pragma unroll
    for (int a = 0; a < BR; ++a)
#pragma unroll
        for (int b = 0; b < BC; ++b) {
            const int j = tj + NW * a, ci = lane + 64 * b;
            if (j == ci && ci < D) td_all[(size_t)k * D + ci] = m[a][b];
            if (D >= 2 && j == D - 1 && ci == D - 2) te[D - 2] = m[a][b];
        }
    if (cs) wt_all[(size_t)k * D + i] = wti;
}

// The instances of the register-resident tridiagonalisation: rows per wavefront BR >= ceil(D / 8), column blocks BC =
// ceil(D / 64).  A dimension takes the first row with D <= max_d; above the last row (D > 320) the global-memory kernel runs.
typedef void (*TridiagRegKernel)(int D, const float* Mall, float* wt_all, float* td_all, float* te_all);
struct TridiagReg { int max_d, br, bc; TridiagRegKernel kernel; };
#define BLK_TRIDIAG_ROW(MAXD, BRV, BCV) {MAXD, BRV, BCV, blk_tridiag_reg_kernel<8, BRV, BCV>}
const TridiagReg blk_tridiag_instances[] = {BLK_TRIDIAG_ROW(64, 8, 1),   BLK_TRIDIAG_ROW(128, 16, 2), BLK_TRIDIAG_ROW(192, 24, 3),
                                            BLK_TRIDIAG_ROW(256, 32, 4), BLK_TRIDIAG_ROW(304, 38, 5), BLK_TRIDIAG_ROW(320, 40, 5)};
#undef BLK_TRIDIAG_ROW

// bracketing search (:335-429) on the tridiagonal form, 63 nodes of the bisection tree per round (as in update_kl.hip);
// state[k] = (eta*, success, KL(eta*), probes)
__global__ __launch_bounds__(64) void blk_search_kernel(int D, const float* __restrict__ td_all, const float* __restrict__ te_all,
                                                        const float* __restrict__ wt_all, const float* __restrict__ stepsizes,
                                                        const float* __restrict__ last_eta, float temperature,
                                                        float* __restrict__ scratch_all, float* __restrict__ state) {
    extern __shared__ float sm[];
    float* td = sm;
    float* te = sm + D;
    float* wt = sm + 2 * D;
    const int k = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < D; i += 64) {
        td[i] = td_all[(size_t)k * D + i];
        te[i] = te_all[(size_t)k * D + i];
        wt[i] = wt_all[(size_t)k * D + i];
    }
    __syncthreads();
    // pivot columns of the 64 lanes: in LDS when they fit (2 D x 64 floats: D <= 310 -- the backward recurrence reads them back
    // one dependent load per step, 262 us per launch from global memory at D = 300), else in global scratch
    float* scratch = scratch_all != nullptr ? scratch_all + (size_t)k * 2 * D * 64 : sm + 3 * D;
    const float eps = stepsizes[k];
    const float last = last_eta[k];
    float lb, ub;
    if (last < 0.f) { lb = -20.f; ub = 80.f; }
    else { lb = fmaxf(0.f, __logf(last) - 3.f); ub = __logf(last) + 3.f; }
    bool ub_ok = false, done = false;
    int probes = 0, iters = 0;
    float kl_ub = -1.f;
    while (!done && iters < 1000) {
        float nlb = lb, nub = ub;
        if (t >= 2) {
            const int depth = 31 - __clz(t);
            for (int b = depth - 1; b >= 0; --b) {
                const float mid = 0.5f * (nub + nlb);
                if ((t >> b) & 1) nlb = mid; else nub = mid;
            }
        }
        const float neta = 0.5f * (nub + nlb);
        const float e_eta = expf(neta);
        const float ndiff = fminf(expf(nub) - e_eta, e_eta - expf(nlb));
        const float nkl = (t >= 1) ? tr_kl_tridiag<0, false>(D, td, te, wt, scratch + t, e_eta) : 0.f;
        int n = 1;
        for (int level = 0; level < 6 && !done && iters < 1000; ++level, ++iters) {
            const float diff = __shfl(ndiff, n), klv = __shfl(nkl, n), eta = __shfl(neta, n);
            if (diff < 1e-1f) { done = true; break; }
            ++probes;
            if (fabsf(eps - klv) < 1e-1f * eps) { lb = ub = eta; kl_ub = klv; done = true; break; }
            if (eps > klv) { ub = eta; ub_ok = true; kl_ub = klv; n = 2 * n; }
            else { lb = eta; n = 2 * n + 1; }
        }
    }
    if (ub_ok) lb = ub;
    const float lo = expf(lb), hi = expf(ub);
    const float eta_star = fmaxf(lo, temperature);
    bool success = (lo == hi);
    float kl_val = -1.f;
    if (success) {
        kl_val = (eta_star == lo && kl_ub >= 0.f)
                     ? kl_ub : __shfl(tr_kl_tridiag<0, false>(D, td, te, wt, scratch + t, eta_star), 0);
        success = kl_val < FLT_MAX;
    }
    if (t == 0) {
        state[4 * k] = eta_star;
        state[4 * k + 1] = success ? 1.f : 0.f;
        state[4 * k + 2] = kl_val;
        state[4 * k + 3] = (float)probes;
    }
}

// mode 0 (KL-constrained): B = I + Mc/eta* = U U^T through the Cholesky factor C of the index-reversed matrix (U = J C J);
// L' = L U^-T and z = U^-1 w by forward substitution with C on the reversed rows of L (one thread per row, thread D: w);
// mu' = mu - L' z / eta*.  Commits means / chols on success and does the bookkeeping of :518-524.
// modes 1 / 2 (direct :97-141, iBLR :160-223): Mc holds the new precision Q' (lower triangle read, as tf.linalg.cholesky
// does); Q' = U U^T the same way, the new factor is L' = U^-T (rows of the identity as right-hand sides), the new mean
// L' (U^-1 lin') for the direct update (w = new linear term), the precomputed mean (w) for iBLR.
__global__ __launch_bounds__(704) void blk_upd_final_kernel(int D, int mode, const float* __restrict__ Mc_all,
                                                            const float* __restrict__ w_all, float* __restrict__ W_all,
                                                            float* __restrict__ X_all, const float* __restrict__ state,
                                                            float* __restrict__ means, float* __restrict__ chols,
                                                            float l2_init, float* __restrict__ last_eta, float* __restrict__ l2,
                                                            float* __restrict__ num_updates, int32_t* __restrict__ success_out,
                                                            float* __restrict__ kl_out, int32_t* __restrict__ nprobes_out) {
    extern __shared__ __align__(16) float dyn[];
    __shared__ int anybad;
    const int k = blockIdx.x, t = threadIdx.x;
    const float eta_star = mode == 0 ? state[4 * k] : 1.f;
    bool success = mode == 0 ? state[4 * k + 1] != 0.f : true;
    const float kl_val = mode == 0 ? state[4 * k + 2] : 0.f;
    const float inv = 1.f / eta_star;
    const float diag_add = mode == 0 ? 1.f : 0.f;
    float* L = chols + (size_t)k * D * D;
    float* mu = means + (size_t)k * D;
    if (success) {
        const float* Mc = Mc_all + (size_t)k * D * D;
        float* W = W_all + (size_t)k * D * D;
        success = blk_cholesky(D, [Mc, D, inv, diag_add](int i, int j) {
            return (i == j ? diag_add : 0.f) + Mc[(size_t)(D - 1 - j) * D + (D - 1 - i)] * inv; }, W, dyn);
        if (success) {
            const float* w = w_all + (size_t)k * D;
            float* X = X_all + (size_t)k * D * (D + 1);
            const int ldx = D + 1;
            if (mode == 0)
                blk_trsm<true>(D, W, D + 1,
                               [L, w, D](int i, int tt) { return tt < D ? L[(size_t)tt * D + (D - 1 - i)] : w[D - 1 - i]; },
                               t < D ? D - 1 - t : 0, X, ldx, dyn);
            else
                blk_trsm<true>(D, W, mode == 1 ? D + 1 : D,
                               [w, D](int i, int tt) { return tt < D ? (tt == D - 1 - i ? 1.f : 0.f) : w[D - 1 - i]; },
                               t < D ? D - 1 - t : 0, X, ldx, dyn);
            if (t == 0) anybad = 0;
            __syncthreads();
            float new_mu = 0.f;
            if (t < D) {
                float acc = 0.f;
                bool bad = false;
                for (int i = 0; i < D; ++i) {
                    const float x = X[(size_t)i * ldx + t];
                    if (mode != 2) acc = fmaf(x, X[(size_t)i * ldx + D], acc);
                    bad |= !(x == x);
                }
                bad |= !(X[(size_t)(D - 1 - t) * ldx + t] > 0.f);          // diagonal of L'
                new_mu = mode == 0 ? mu[t] - acc * inv : (mode == 1 ? acc : w[t]);
                bad |= !(new_mu == new_mu);
                if (bad) anybad = 1;
            }
            __syncthreads();
            success = anybad == 0;                                                         // :493 is_nan(new_chol)
            if (success) {
                for (int e = t; e < D * D; e += blockDim.x) {
                    const int r = e / D, c = e % D;
                    L[e] = (c <= r) ? X[(size_t)(D - 1 - c) * ldx + r] : 0.f;
                }
                if (t < D) mu[t] = new_mu;
            }
        }
    }
    if (t == 0) {
        if (mode == 0) tr_report_search(k, success, eta_star, kl_val, (int32_t)state[4 * k + 3], last_eta, kl_out, nprobes_out);
        tr_finish_bookkeeping(k, success, l2_init, l2, num_updates, success_out);
    }
}

// direct: Qp = Q + step R, vec = Q mu + step (R mu - g_neg).   iBLR: Qp = Q + step (R + step/2 T2) with T2 = R Sigma R,
// vec = mu - step Sigma g_neg (mu itself on the component's first update, :184-186).
__global__ __launch_bounds__(256) void blk_plain_prep_kernel(int mode, int D, const float* __restrict__ Q,
                                                             const float* __restrict__ H_neg, const float* __restrict__ g_neg,
                                                             const float* __restrict__ means, const float* __restrict__ stepsizes,
                                                             const float* __restrict__ num_updates, const float* __restrict__ Sig,
                                                             const float* __restrict__ T2, float* __restrict__ Qp,
                                                             float* __restrict__ vec) {
    const int k = blockIdx.x;
    const size_t o = (size_t)k * D * D;
    const float step = stepsizes[k];
    for (int e = blockIdx.y * 256 + threadIdx.x; e < D * D; e += gridDim.y * 256)
        Qp[o + e] = Q[o + e] + step * (mode == 1 ? H_neg[o + e] : H_neg[o + e] + 0.5f * step * T2[o + e]);
    const float* mu = means + (size_t)k * D;
    const float* g = g_neg + (size_t)k * D;
    for (int t = blockIdx.y * 256 + threadIdx.x; t < D; t += gridDim.y * 256) {
        float a = 0.f;
        if (mode == 1) {
            float b = 0.f;
            for (int j = 0; j < D; ++j) { a = fmaf(Q[o + (size_t)t * D + j], mu[j], a); b = fmaf(H_neg[o + (size_t)t * D + j], mu[j], b); }
            vec[(size_t)k * D + t] = a + step * (b - g[t]);
        } else {
            for (int j = 0; j < D; ++j) a = fmaf(Sig[o + (size_t)t * D + j], g[j], a);
            vec[(size_t)k * D + t] = (num_updates[k] == 0.f) ? mu[t] : mu[t] - step * a;
        }
    }
}

}  // namespace

int gmmvi_blocked_update_kl(gmmvi_ctx* ctx, int K, int D, float* means, float* chols, const float* H_neg, const float* g_neg,
                            const float* stepsizes, float temperature, float l2_init, float* last_eta, float* l2,
                            float* num_updates, int32_t* success_out, float* kl_out, int32_t* nprobes_out, float* packed_out) {
    const size_t DD = (size_t)D * D;
    const size_t f_mat = (size_t)K * DD;
    const size_t f_x = (size_t)K * D * (D + 1), f_vec = (size_t)K * D, f_scr = (size_t)K * 2 * D * 64, f_state = (size_t)K * 4;
    BLK_TRY(gmmvi_ws_reserve(ctx, (4 * f_mat + f_x + 5 * f_vec + f_scr + f_state) * sizeof(float)));
    float* Rs = (float*)ctx->ws;          // R_sym, later the row-major Cholesky factor
    float* T1 = Rs + f_mat;               // R_sym L, later the column-major Cholesky factor
    float* M = T1 + f_mat;                // L^T R L, tridiagonalised in place
    float* Mc = M + f_mat;                // copy of M for the final factorisation
    float* Xs = Mc + f_mat;
    float* gt = Xs + f_x;
    float* w = gt + f_vec;
    float* wt = w + f_vec;
    float* td = wt + f_vec;
    float* te = td + f_vec;
    float* scratch = te + f_vec;
    float* state = scratch + f_scr;
    GMMVI_PROF(ctx, "blocked_update_kl");
    const int slices = (D * D + 256 * 16 - 1) / (256 * 16);          // ~16 elements per thread
    hipLaunchKernelGGL(blk_upd_prep_kernel, dim3(K, slices), dim3(256), 0, ctx->stream, D, H_neg, g_neg, means, Rs, gt);
    GMMVI_LAUNCH_CHECK(ctx);
    {
        BG g = bg_zero();
        g.A = Rs; g.lda = D; g.sA = (long long)DD; g.a_kmajor = 0;
        g.B = chols; g.ldb = D; g.sB = (long long)DD; g.b_kmajor = 1; g.tri = 2;      // opB(k = c, n = j) = L[c][j], zero for c < j
        g.C = T1; g.ldc = D; g.sC = (long long)DD;
        g.M = D; g.N = D; g.Kd = D;
        BLK_TRY(gmmvi_bgemm(ctx, g, K));
    }
    {
        BG g = bg_zero();
        g.A = chols; g.lda = D; g.sA = (long long)DD; g.a_kmajor = 1;                 // opA(m = i, k = c) = L[c][i]
        g.B = T1; g.ldb = D; g.sB = (long long)DD; g.b_kmajor = 1;
        g.C = M; g.ldc = D; g.sC = (long long)DD;
        g.M = D; g.N = D; g.Kd = D;
        BLK_TRY(gmmvi_bgemm(ctx, g, K));
    }
    hipLaunchKernelGGL(blk_upd_sym_kernel, dim3(K, slices), dim3(256), 0, ctx->stream, D, chols, gt, M, Mc, w, wt);
    GMMVI_LAUNCH_CHECK(ctx);
    {
        const TridiagReg* reg = nullptr;
        for (const TridiagReg& r : blk_tridiag_instances)
            if (reg == nullptr && D <= r.max_d) reg = &r;
        if (reg != nullptr) {
            const int br = reg->br, bc = reg->bc;
            const size_t shmem = ((size_t)4 * 64 * bc + (size_t)24 * ((br + 3) / 4 * 4) + (size_t)8 * 64 * bc + 48) * sizeof(float);
            hipLaunchKernelGGL(reg->kernel, dim3(K), dim3(512), shmem, ctx->stream, D, (const float*)M, wt, td, te);
        } else {
            const int DT = blk_threads(D);
            int G = 1024 / DT;
            if (G < 1) G = 1;
            const size_t shmem = ((size_t)4 * D + (size_t)G * DT + 48) * sizeof(float);
            hipLaunchKernelGGL(blk_tridiag_kernel, dim3(K), dim3(G * DT), shmem, ctx->stream, D, DT, G, M, wt, td, te);
        }
        GMMVI_LAUNCH_CHECK(ctx);
    }
    {
        const size_t lds_cols = ((size_t)3 * D + (size_t)2 * D * 64) * sizeof(float);
        const bool in_lds = lds_cols <= BLK_LDS_LIMIT;           // (the kernel's static LDS words need room beside it)
        if (in_lds) BLK_TRY(gmmvi_ensure_dynamic_lds(ctx, (const void*)blk_search_kernel, BLK_LDS_LIMIT));
        hipLaunchKernelGGL(blk_search_kernel, dim3(K), dim3(64), in_lds ? lds_cols : (size_t)3 * D * sizeof(float), ctx->stream, D,
                           td, te, wt, stepsizes, last_eta, temperature, in_lds ? nullptr : scratch, state);
    }
    GMMVI_LAUNCH_CHECK(ctx);
    {
        BLK_TRY(gmmvi_ensure_dynamic_lds(ctx, (const void*)blk_upd_final_kernel, BLK_LDS_LIMIT));
        const size_t a = blk_trsm_lds_floats(D), b = blk_chol_lds_floats(D);
        hipLaunchKernelGGL(blk_upd_final_kernel, dim3(K), dim3(blk_threads_mm(D + 1)), (a > b ? a : b) * sizeof(float), ctx->stream, D,
                           0, Mc, w, T1, Xs, state, means, chols, l2_init, last_eta, l2, num_updates, success_out, kl_out,
                           nprobes_out);
    }
    GMMVI_LAUNCH_CHECK(ctx);
    if (packed_out) BLK_TRY(gmmvi_blocked_pack(ctx, GMMVI_GAUSS, 0.f, K, D, means, chols, packed_out, nullptr));
    return GMMVI_OK;
}

// DirectNgBasedComponentUpdater (:97-141, mode 0) and NgBasedComponentUpdaterIblr (:160-223, mode 1) on the blocked path
int gmmvi_blocked_update_plain(gmmvi_ctx* ctx, int mode, int K, int D, float* means, float* chols, const float* H_neg,
                               const float* g_neg, const float* stepsizes, float l2_init, float* l2, float* num_updates,
                               int32_t* success_out) {
    const size_t DD = (size_t)D * D, ps = gmmvi_blocked_stride(D);
    const size_t f_mat = (size_t)K * DD, f_pk = (size_t)K * ps, f_x = (size_t)K * D * (D + 1), f_vec = (size_t)K * D;
    const int nmat = mode == 0 ? 3 : 6;
    BLK_TRY(gmmvi_ws_reserve(ctx, (f_pk + nmat * f_mat + f_x + f_vec) * sizeof(float)));
    float* pk = (float*)ctx->ws;          // [mu | const | L^-1] of the current components
    float* Q = pk + f_pk;                 // old precision L^-T L^-1
    float* Qp = Q + f_mat;                // new precision
    float* W = Qp + f_mat;                // column-major Cholesky factor
    float* Sig = W + f_mat;               // iBLR: Sigma, R Sigma, R Sigma R
    float* T = Sig + (mode == 0 ? 0 : f_mat);
    float* T2 = T + (mode == 0 ? 0 : f_mat);
    float* Xs = W + (size_t)(nmat - 2) * f_mat;
    float* vec = Xs + f_x;
    GMMVI_PROF(ctx, "blocked_update_plain");
    BLK_TRY(gmmvi_blocked_pack(ctx, GMMVI_GAUSS, 0.f, K, D, means, chols, pk, nullptr));
    const float* Linv = pk + gmmvi_blocked_linv_ofs(D);
    {
        BG g = bg_zero();
        g.A = Linv; g.lda = D; g.sA = (long long)ps; g.a_kmajor = 1;          // opA(m = i, k = c) = L^-1[c][i]
        g.B = Linv; g.ldb = D; g.sB = (long long)ps; g.b_kmajor = 1;
        g.C = Q; g.ldc = D; g.sC = (long long)DD;
        g.M = D; g.N = D; g.Kd = D;
        BLK_TRY(gmmvi_bgemm(ctx, g, K));
    }
    if (mode == 1) {
        BG g = bg_zero();
        g.A = chols; g.lda = D; g.sA = (long long)DD; g.a_kmajor = 0;
        g.B = chols; g.ldb = D; g.sB = (long long)DD; g.b_kmajor = 0;         // opB(k = c, n = j) = L[j][c]
        g.C = Sig; g.ldc = D; g.sC = (long long)DD;
        g.M = D; g.N = D; g.Kd = D;
        BLK_TRY(gmmvi_bgemm(ctx, g, K));
        g.A = H_neg; g.B = Sig; g.b_kmajor = 1; g.C = T;                       // R Sigma
        BLK_TRY(gmmvi_bgemm(ctx, g, K));
        g.A = T; g.B = H_neg; g.C = T2;                                        // (R Sigma) R
        BLK_TRY(gmmvi_bgemm(ctx, g, K));
    }
    const int slices = (D * D + 256 * 16 - 1) / (256 * 16);
    hipLaunchKernelGGL(blk_plain_prep_kernel, dim3(K, slices), dim3(256), 0, ctx->stream, mode == 0 ? 1 : 2, D, Q, H_neg, g_neg,
                       means, stepsizes, num_updates, Sig, T2, Qp, vec);
    GMMVI_LAUNCH_CHECK(ctx);
    {
        BLK_TRY(gmmvi_ensure_dynamic_lds(ctx, (const void*)blk_upd_final_kernel, BLK_LDS_LIMIT));
        const size_t a = blk_trsm_lds_floats(D), b = blk_chol_lds_floats(D);
        hipLaunchKernelGGL(blk_upd_final_kernel, dim3(K), dim3(blk_threads_mm(D + 1)), (a > b ? a : b) * sizeof(float), ctx->stream, D,
                           mode == 0 ? 1 : 2, Qp, vec, W, Xs, nullptr, means, chols, l2_init, nullptr, l2, num_updates,
                           success_out, nullptr, nullptr);
        GMMVI_LAUNCH_CHECK(ctx);
    }
    return GMMVI_OK;
}
