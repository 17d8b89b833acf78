// MORE natural-gradient estimate for the blocked-path dimensions 64 <= D <= 128 (gmmvi_more_blocked), gfx950.
//
// Same mathematics as more.hip (its banner is the specification; the shared pieces, the workspace plan and the group loop are
// in more_common.h).  F + 1 = 2 146 (D = 64) ... 8 386 (D = 128).  What differs from more_gram_big / more_solve_big:
//
//   mb_whiten_kernel   workgroup = (64-sample tile, component).  z comes from the dense L^-1 of the blocked component block
//                      [mu | log-normaliser | pad | L^-1]: the tile of x - mu sits in LDS, wave w computes the rows w, w + 4, ...
//                      of z (L^-1 row wave-uniform, lane = sample).  The result is STAGED in the workspace once per
//                      component -- Zt[component][tile][D + 3 rows][64]: z, ones, reward, sqrt(weight) -- and every Gram
//                      workgroup reads it from there.  Staging rather than whitening into LDS per Gram workgroup, because a
//                      component has up to 2 211 Gram workgroups (66 x 67 / 2 blocks) that all need every tile: whitening
//                      costs N D^2 / 2 multiply-adds per component once instead of 2 211 times, the staged copy is 13 MB per
//                      component at D = 128, N = 3 F (it stays in the last-level cache), and a Gram workgroup's LDS keeps one
//                      tile (33.5 KB at D = 128) beside the 256 feature rows instead of four.
//   mb_gram_kernel     workgroup = (128 x 128 block of the lower triangle of G, component), 8 waves, over all tiles in fixed
//                      order: builds the <= 256 weighted feature rows of its two blocks from the staged tile in LDS and
//                      contracts them with v_mfma_f64_16x16x4_f64, 8 tile pairs per wave; the next staged tile is fetched
//                      into registers while the matrix cores run.  LDS 256 x 68 + (D + 3) x 64 + 256 words (104 KB at D = 128).
//   Cholesky           one launch triple per 128-column panel (<= 66 panels), launch boundaries are the only synchronisation:
//     mb_chol_diag_kernel    one workgroup per component factorises the 128 x 128 diagonal block in LDS (adds the ridge);
//                            a non-positive pivot sets the component's fail flag, the later launches of that component return
//     mb_chol_panel_kernel   workgroup = (64 rows below the block, component): x = a L_jj^-T, one lane per row, rows and the
//                            packed triangle of L_jj in LDS
//     mb_chol_update_kernel  workgroup = (128 x 128 tile of the trailing matrix, component): G_IC -= P_I P_C^T on the matrix
//                            cores (v_mfma_f64_16x16x4_f64, panel staged in LDS in 32-column chunks), so the 2 10^11 fp64
//                            operations of a D = 128 component spread over the chip
//   mb_backsub_kernel  one workgroup per component: L^T beta = y, 32 columns per round, beta in LDS
//   mb_unwhiten_*      H = L^-T Q_w L^-1, g = -L^-T lin_w with the SAME dense fp32 L^-1 that whitened the samples (a reward
//                      that is quadratic in x is then recovered whatever the rounding of L^-1); chols_dev is not read
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage; no scratch, no spills in any kernel):
//   mb_gram_kernel 172 VGPR, 0 AGPR, 104 KB LDS at D = 128 (one 512-thread workgroup per CU); mb_chol_update_kernel 96 VGPR,
//   0 AGPR, 68 KB LDS (two workgroups per CU); mb_chol_diag / _panel / mb_backsub / mb_whiten 26 / 64 / 40 / 16 VGPR.
// Measured deviations and times: DESIGN.md section 4.
// The Cholesky and back-substitution launches are also reachable as gmmvi_more_panel_* (common.h): more_diag.hip solves its
// F = 2 D + 1 systems with them.
#include "more_common.h"
#include "blocked.h"

namespace {

constexpr int A_LD = TB + 1;     // LDS row stride (doubles) of a block whose rows belong to consecutive lanes
constexpr int UP_KC = 32;        // columns of the panel staged per step of the trailing update
constexpr int UP_LD = UP_KC + 2; // LDS row stride (doubles): 16 rows x 2 k-groups of a half-wave fall on 32 distinct bank pairs
constexpr int Z_PRE = 5;         // float4 per thread of one staged tile: ceil((128 + 3) * 16 / 512)

__global__ __launch_bounds__(256) void mb_whiten_kernel(int D, int N, int n_tiles, int k0, size_t pstride, int linv_ofs,
                                                        const float* __restrict__ packed, const float* __restrict__ X,
                                                        const float* __restrict__ ld, const float* __restrict__ bg,
                                                        const float* __restrict__ tlp, const float* __restrict__ logq,
                                                        const int32_t* __restrict__ mapping, int map_offset, int flags,
                                                        const float* __restrict__ lse, float* __restrict__ Zt) {
    extern __shared__ float xs[];                      // [D][65]: (x - mu), coordinate-major
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kk = blockIdx.y, k = k0 + kk, tile = blockIdx.x;
    const float* __restrict__ P = packed + (size_t)k * pstride;
    const float* __restrict__ Linv = P + linv_ofs;
    const int n0 = tile * 64;
    for (int e = tid; e < 64 * D; e += 256) {
        const int s = e / D, j = e - s * D;
        xs[j * 65 + s] = (n0 + s < N) ? X[(size_t)(n0 + s) * D + j] - P[j] : 0.f;
    }
    const int n = n0 + lane;
    float sw, rew;
    more_weight_reward(k, n, N, ld, bg, tlp, logq, mapping, map_offset, flags, (flags & GMMVI_SELF_NORMALIZED) ? lse[k] : 0.f,
                       sw, rew);
    const bool live = sw > 0.f;
    __syncthreads();
    float* __restrict__ out = Zt + ((size_t)kk * n_tiles + tile) * (size_t)(D + 3) * 64;
    for (int i = wave; i < D; i += 4) {
        const float* __restrict__ row = Linv + (size_t)i * D;
        float t = 0.f;
        for (int j = 0; j <= i; ++j) t = fmaf(row[j], xs[j * 65 + lane], t);
        out[i * 64 + lane] = live ? t : 0.f;
    }
    if (wave == 0) more_write_trailer(out, D, lane, sw, rew);
}

// (MFMA operand and result layout: more_common.h)
__global__ __launch_bounds__(512) void mb_gram_kernel(int D, int n_tiles, int LDG, const float* __restrict__ Zt,
                                                      double* __restrict__ G) {
    extern __shared__ float phi[];                     // [256][PHI_LD] feature rows of the two blocks, one staged tile, tab
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int k = blockIdx.y;
    int BI, BC;
    more_block_of(blockIdx.x, BI, BC);
    const bool diag = BI == BC;
    const int F = D * (D + 1) / 2 + D + 1;             // features; row F carries the reward
    const int ZS = (D + 3) * 64;                       // per tile: rows 0..D-1 z, row D ones, D+1 reward, D+2 sqrt(weight)
    float* zs = phi + 256 * PHI_LD;
    int* tab = reinterpret_cast<int*>(zs + ZS);        // local row (0..255) -> (row ia) | (row ib) << 16 of the tile, or -1
    const int n_rows = diag ? 128 : 256;
    for (int r = tid; r < 256; r += 512) {
        const int f = TB * (r < 128 ? BI : BC) + (r & 127);
        tab[r] = (r < n_rows && f <= F) ? more_feature_code(f, D) : -1;
    }
    for (int e = tid; e < 256 * PHI_LD; e += 512) phi[e] = 0.f;         // rows without a feature stay zero
    const float* __restrict__ zsrc = Zt + (size_t)k * n_tiles * ZS;
    for (int e = 4 * tid; e < ZS; e += 2048) *reinterpret_cast<float4*>(zs + e) = *reinterpret_cast<const float4*>(zsrc + e);
    __syncthreads();

    // wave w owns the tile pairs q = w + 8 pp: row tile q / 8 of block BI, column tile q % 8 of block BC
    f64x4 acc[8];
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) acc[pp] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int r16 = lane & 15, kg = lane >> 4;
    const int col_base = diag ? 0 : 128;
    for (int t = 0; t < n_tiles; ++t) {
        {
            const float swn = zs[(D + 2) * 64 + lane];
            for (int r = tid >> 6; r < n_rows; r += 8) {
                const int c = tab[r];
                if (c >= 0) phi[r * PHI_LD + lane] = (swn * zs[(c & 0xffff) * 64 + lane]) * zs[(c >> 16) * 64 + lane];
            }
        }
        __syncthreads();
        // the next staged tile travels to registers while the matrix cores work on this one
        const bool more = t + 1 < n_tiles;
        const float* __restrict__ znext = zsrc + (size_t)(t + 1) * ZS;
        float4 pre[Z_PRE];
#pragma unroll
        for (int q = 0; q < Z_PRE; ++q) {
            const int e = 4 * (tid + 512 * q);
            pre[q] = (more && e < ZS) ? *reinterpret_cast<const float4*>(znext + e) : float4{0.f, 0.f, 0.f, 0.f};
        }
        more_contract_block(phi, wave, r16, kg, col_base, acc);
        if (more) {
#pragma unroll
            for (int q = 0; q < Z_PRE; ++q) {
                const int e = 4 * (tid + 512 * q);
                if (e < ZS) *reinterpret_cast<float4*>(zs + e) = pre[q];
            }
        }
        __syncthreads();
    }
    more_store_block(G + (size_t)k * LDG * LDG, LDG, BI, BC, wave, r16, kg, acc);
}

// Diagonal block of the panel at column jb: right-looking Cholesky in LDS, one barrier per column.  Column j stays
// unscaled while the columns behind it are updated (A_ic -= A_ij A_cj / A_jj); the scaling by 1 / sqrt(A_jj) happens on
// the way back to global memory.
__global__ __launch_bounds__(512) void mb_chol_diag_kernel(int F, int LDG, int jb, int k0, const float* __restrict__ l2,
                                                           double* __restrict__ Gall, int* __restrict__ fail) {
    extern __shared__ double A[];                      // [128][A_LD], then rsq[128]
    double* rsq = A + TB * A_LD;
    const int tid = threadIdx.x;
    const int kk = blockIdx.x;
    if (fail[kk]) return;
    double* G = Gall + (size_t)kk * LDG * LDG;
    const int nbc = min(TB, F - jb);
    const double ridge = (double)l2[k0 + kk];
    for (int e = tid; e < TB * TB; e += 512) {
        const int i = e >> 7, c = e & 127;
        double v = (i < nbc && c <= i) ? G[(size_t)(jb + i) * LDG + jb + c] : (i == c ? 1.0 : 0.0);
        if (i == c && i < nbc && jb + i < F - 1) v += ridge;             // least_squares.py:71-73 (bias unregularised)
        A[i * A_LD + c] = v;
    }
    const int i = tid & 127, cg = tid >> 7;
    bool bad = false;
    for (int j = 0; j < nbc; ++j) {
        __syncthreads();
        const double d = A[j * A_LD + j];
        if (!(d > 0.0)) { bad = true; break; }                           // uniform: every thread reads the same pivot
        if (tid == 0) rsq[j] = 1.0 / sqrt(d);
        if (i > j) {
            const double aij = A[i * A_LD + j] / d;
            for (int c = j + 1 + cg; c <= i; c += 4) A[i * A_LD + c] = fma(-aij, A[c * A_LD + j], A[i * A_LD + c]);
        }
    }
    __syncthreads();
    if (bad) {
        if (tid == 0) fail[kk] = 1;
        return;
    }
    for (int e = tid; e < TB * TB; e += 512) {
        const int r = e >> 7, c = e & 127;
        if (r < nbc && c <= r) G[(size_t)(jb + r) * LDG + jb + c] = A[r * A_LD + c] * rsq[c];
    }
}

// Panel rows below the diagonal block (up to the right-hand side row F): x = a L_jj^-T, lane = row.
__global__ __launch_bounds__(64) void mb_chol_panel_kernel(int F, int LDG, int jb, double* __restrict__ Gall,
                                                           const int* __restrict__ fail) {
    extern __shared__ double R[];                      // [64][A_LD] rows, then the packed lower triangle of L_jj
    double* Lp = R + 64 * A_LD;
    const int lane = threadIdx.x;
    const int kk = blockIdx.y;
    if (fail[kk]) return;
    double* G = Gall + (size_t)kk * LDG * LDG;
    const int nbc = min(TB, F - jb);
    const int r0 = jb + nbc + 64 * (int)blockIdx.x;
    for (int e = lane; e < 64 * TB; e += 64) {
        const int r = e >> 7, c = e & 127;
        R[r * A_LD + c] = (r0 + r <= F && c < nbc) ? G[(size_t)(r0 + r) * LDG + jb + c] : 0.0;
    }
    for (int e = lane; e < TB * TB; e += 64) {
        const int r = e >> 7, c = e & 127;
        if (r < nbc && c <= r) Lp[r * (r + 1) / 2 + c] = G[(size_t)(jb + r) * LDG + jb + c];
    }
    __syncthreads();
    double* my = R + lane * A_LD;
    for (int c = 0; c < nbc; ++c) {
        const double* lrow = Lp + c * (c + 1) / 2;
        double t0 = my[c], t1 = 0.0, t2 = 0.0, t3 = 0.0;
        int u = 0;
        for (; u + 3 < c; u += 4) {
            t0 = fma(-my[u], lrow[u], t0);
            t1 = fma(-my[u + 1], lrow[u + 1], t1);
            t2 = fma(-my[u + 2], lrow[u + 2], t2);
            t3 = fma(-my[u + 3], lrow[u + 3], t3);
        }
        for (; u < c; ++u) t0 = fma(-my[u], lrow[u], t0);
        my[c] = ((t0 + t1) + (t2 + t3)) / lrow[c];
    }
    __syncthreads();
    for (int e = lane; e < 64 * TB; e += 64) {
        const int r = e >> 7, c = e & 127;
        if (r0 + r <= F && c < nbc) G[(size_t)(r0 + r) * LDG + jb + c] = R[r * A_LD + c];
    }
}

// Trailing update behind the full panel jp (columns 128 jp ...): tile (I, C), I >= C > jp, of G loses P_I P_C^T, P_T the
// 128 x 128 panel rows of tile row T.  Rows beyond F are zero in G and stay zero.  k order inside an 8-column group: lane
// group kg holds columns 2 kg, 2 kg + 1 (one 16-byte LDS read), used in two consecutive MFMAs -- the same permutation for both
// operands.
__global__ __launch_bounds__(512) void mb_chol_update_kernel(int LDG, int jp, double* __restrict__ Gall,
                                                             const int* __restrict__ fail) {
    extern __shared__ double As[];                     // [128][UP_LD] rows of tile row I, then of tile row C
    double* Bs = As + TB * UP_LD;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kk = blockIdx.y;
    if (fail[kk]) return;
    double* G = Gall + (size_t)kk * LDG * LDG;
    int ib = 0;
    while ((ib + 1) * (ib + 2) / 2 <= (int)blockIdx.x) ++ib;
    const int cb = (int)blockIdx.x - ib * (ib + 1) / 2;
    const int I = jp + 1 + ib, C = jp + 1 + cb;
    const double* __restrict__ Pi = G + (size_t)TB * I * LDG + TB * jp;
    const double* __restrict__ Pc = G + (size_t)TB * C * LDG + TB * jp;
    f64x4 acc[8];
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) acc[pp] = f64x4{0.0, 0.0, 0.0, 0.0};
    const int r16 = lane & 15, kg = lane >> 4;
    for (int kc = 0; kc < TB; kc += UP_KC) {
        for (int e = tid; e < TB * (UP_KC / 2); e += 512) {
            const int r = e >> 4, c2 = e & 15;
            *reinterpret_cast<double2*>(As + r * UP_LD + 2 * c2) =
                *reinterpret_cast<const double2*>(Pi + (size_t)r * LDG + kc + 2 * c2);
            *reinterpret_cast<double2*>(Bs + r * UP_LD + 2 * c2) =
                *reinterpret_cast<const double2*>(Pc + (size_t)r * LDG + kc + 2 * c2);
        }
        __syncthreads();
#pragma unroll
        for (int pp = 0; pp < 8; ++pp) {
            const int q = wave + 8 * pp;
            const double* pa = As + (16 * (q >> 3) + r16) * UP_LD + 2 * kg;
            const double* pb = Bs + (16 * (q & 7) + r16) * UP_LD + 2 * kg;
#pragma unroll
            for (int m = 0; m < UP_KC / 8; ++m) {
                const double2 a = *reinterpret_cast<const double2*>(pa + 8 * m);
                const double2 b = *reinterpret_cast<const double2*>(pb + 8 * m);
                acc[pp] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.x, b.x, acc[pp], 0, 0, 0);
                acc[pp] = __builtin_amdgcn_mfma_f64_16x16x4f64(a.y, b.y, acc[pp], 0, 0, 0);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int pp = 0; pp < 8; ++pp) {
        const int q = wave + 8 * pp;
        const int ti = q >> 3, tj = q & 7;
        if (I == C && tj > ti) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const size_t o = (size_t)(TB * I + 16 * ti + 4 * r + kg) * LDG + TB * C + 16 * tj + r16;
            G[o] -= acc[pp][r];
        }
    }
}

// One workgroup per component: L^T beta = y (y = row F of the factorised G), 32 columns per round; beta stays in LDS and
// is written out once.
__global__ __launch_bounds__(1024) void mb_backsub_kernel(int F, int LDG, const double* __restrict__ Gall,
                                                          const int* __restrict__ fail, double* __restrict__ beta_all) {
    extern __shared__ double sb[];                     // beta[LDG], Db[32][33], red[32][33]
    double* beta = sb;
    double* Db = sb + LDG;
    double* red = Db + 32 * 33;
    const int tid = threadIdx.x;
    const int kk = blockIdx.x;
    if (fail[kk]) return;
    const double* __restrict__ G = Gall + (size_t)kk * LDG * LDG;
    for (int jb = ((F - 1) / 32) * 32; jb >= 0; jb -= 32) {
        const int nbc = min(32, F - jb);
        // part[c] = sum_{i >= jb + nbc} L[i][jb + c] beta[i]: thread (c = tid % 32, rows tid / 32, + 32, ...)
        {
            const int c = tid & 31, rr = tid >> 5;
            double part = 0.0;
            if (c < nbc)
                for (int i = jb + nbc + rr; i < F; i += 32) part = fma(G[(size_t)i * LDG + jb + c], beta[i], part);
            red[rr * 33 + c] = part;
        }
        {
            const int i = tid >> 5, c = tid & 31;
            Db[i * 33 + c] = (i < nbc && c <= i) ? G[(size_t)(jb + i) * LDG + jb + c] : (i == c ? 1.0 : 0.0);
        }
        __syncthreads();
        if (tid < 32) {
            double rc = 0.0;
            if (tid < nbc) {
                double p = 0.0;
                for (int rr = 0; rr < 32; ++rr) p += red[rr * 33 + tid];
                rc = G[(size_t)F * LDG + jb + tid] - p;
            }
            for (int jj = nbc - 1; jj >= 0; --jj) {
                const double bj = __shfl(rc, jj, 32) / Db[jj * 33 + jj];
                if (tid == jj) beta[jb + jj] = bj;
                if (tid < jj) rc = fma(-Db[jj * 33 + tid], bj, rc);
            }
        }
        __syncthreads();
    }
    double* out = beta_all + (size_t)kk * LDG;
    for (int i = tid; i < F; i += 1024) out[i] = beta[i];
}

// Q_w = -(Qt + Qt^T) with Qt the upper-triangular fill of the quadratic coefficients (least_squares.py:177-179)
__device__ __forceinline__ double mb_quad_w(const double* __restrict__ beta, int D, int i, int j) {
    const int a = min(i, j), b = max(i, j);
    const double q = beta[a * D - a * (a - 1) / 2 + (b - a)];
    return (a == b) ? -2.0 * q : -q;
}

// T = Q_w L^-1: workgroup = (row i, component), thread = column j; L^-1 is lower-triangular
__global__ __launch_bounds__(128) void mb_unwhiten_right_kernel(int D, int LDG, int k0, size_t pstride, int linv_ofs,
                                                                const float* __restrict__ packed,
                                                                const double* __restrict__ beta_all,
                                                                const int* __restrict__ fail, double* __restrict__ T) {
    const int i = blockIdx.x, kk = blockIdx.y, j = threadIdx.x;
    if (fail[kk] || j >= D) return;
    const float* __restrict__ Linv = packed + (size_t)(k0 + kk) * pstride + linv_ofs;
    const double* __restrict__ beta = beta_all + (size_t)kk * LDG;
    double t = 0.0;
    for (int m = j; m < D; ++m) t = fma(mb_quad_w(beta, D, i, m), (double)Linv[(size_t)m * D + j], t);
    T[((size_t)kk * D + i) * D + j] = t;
}

// H = L^-T T (least_squares.py:185), g = Q mu - lin = -L^-T lin_w (:186-188, ng_estimator.py:371-373); NaN for a component
// whose ridge system was not positive definite
__global__ __launch_bounds__(128) void mb_unwhiten_left_kernel(int D, int LDG, int k0, size_t pstride, int linv_ofs,
                                                               const float* __restrict__ packed,
                                                               const double* __restrict__ beta_all,
                                                               const int* __restrict__ fail, const double* __restrict__ T,
                                                               float* __restrict__ H_neg, float* __restrict__ g_neg) {
    const int i = blockIdx.x, kk = blockIdx.y, j = threadIdx.x;
    if (j >= D) return;
    const int k = k0 + kk;
    if (fail[kk]) {
        const float nanv = __int_as_float(0x7fc00000);
        H_neg[((size_t)k * D + i) * D + j] = nanv;
        if (j == 0) g_neg[(size_t)k * D + i] = nanv;
        return;
    }
    const float* __restrict__ Linv = packed + (size_t)k * pstride + linv_ofs;
    const double* __restrict__ Tk = T + (size_t)kk * D * D;
    double h = 0.0;
    for (int m = i; m < D; ++m) h = fma((double)Linv[(size_t)m * D + i], Tk[(size_t)m * D + j], h);
    H_neg[((size_t)k * D + i) * D + j] = (float)h;
    if (j == 0) {
        const double* __restrict__ lin_w = beta_all + (size_t)kk * LDG + D * (D + 1) / 2;
        double g = 0.0;
        for (int m = i; m < D; ++m) g = fma((double)Linv[(size_t)m * D + i], lin_w[m], g);
        g_neg[(size_t)k * D + i] = (float)(-g);
    }
}

}  // namespace

// ---- the panel solver as internal entry points (common.h): gmmvi_more_blocked below and more_diag.hip launch the same kernels ----
int gmmvi_more_panel_attrs(gmmvi_ctx* ctx) {
    const struct { const void* func; size_t bytes; } limits[] = {
        {(const void*)mb_chol_diag_kernel, ((size_t)TB * A_LD + TB) * sizeof(double)},
        {(const void*)mb_chol_panel_kernel, ((size_t)64 * A_LD + (size_t)TB * (TB + 1) / 2) * sizeof(double)},
        {(const void*)mb_chol_update_kernel, (size_t)2 * TB * UP_LD * sizeof(double)},
        {(const void*)mb_backsub_kernel, ((size_t)TB * 66 + 2 * 32 * 33) * sizeof(double)}};
    for (const auto& l : limits) {
        const int rc = gmmvi_ensure_dynamic_lds(ctx, l.func, l.bytes);
        if (rc != GMMVI_OK) return rc;
    }
    return GMMVI_OK;
}

// In-place Cholesky of the kg ridge systems G[kg][LDG][LDG] (lower triangle, F features, right-hand side in row F; ridge
// l2_dev[k0 + kk] on all rows but the bias F - 1): one launch triple per 128-column panel
int gmmvi_more_panel_cholesky(gmmvi_ctx* ctx, const char* prof_name, int F, int LDG, int kg, int k0, const float* l2_dev,
                              double* G, int* fail) {
    const int nblk = LDG / TB;
    const size_t diag_lds = ((size_t)TB * A_LD + TB) * sizeof(double);
    const size_t panel_lds = ((size_t)64 * A_LD + (size_t)TB * (TB + 1) / 2) * sizeof(double);
    const size_t update_lds = (size_t)2 * TB * UP_LD * sizeof(double);
    GMMVI_PROF(ctx, prof_name);
    for (int jp = 0; TB * jp < F; ++jp) {
        const int jb = TB * jp;
        const int nbc = F - jb < TB ? F - jb : TB;
        hipLaunchKernelGGL(mb_chol_diag_kernel, dim3(kg), dim3(512), diag_lds, ctx->stream, F, LDG, jb, k0, l2_dev, G, fail);
        const int rows = F - (jb + nbc) + 1;                     // rows jb + nbc .. F
        hipLaunchKernelGGL(mb_chol_panel_kernel, dim3((rows + 63) / 64, kg), dim3(64), panel_lds, ctx->stream, F, LDG, jb, G,
                           fail);
        const int nt = nblk - (jp + 1);                          // tile rows behind a full panel
        if (nbc == TB && nt > 0)
            hipLaunchKernelGGL(mb_chol_update_kernel, dim3(nt * (nt + 1) / 2, kg), dim3(512), update_lds, ctx->stream, LDG, jp, G,
                               fail);
        GMMVI_LAUNCH_CHECK(ctx);
    }
    return GMMVI_OK;
}

// beta[kk][0 .. F) (stride LDG doubles) from the factorised systems; LDG <= 128 * 66
int gmmvi_more_panel_backsub(gmmvi_ctx* ctx, int F, int LDG, int kg, const double* G, const int* fail, double* beta) {
    const size_t back_lds = ((size_t)LDG + 2 * 32 * 33) * sizeof(double);
    hipLaunchKernelGGL(mb_backsub_kernel, dim3(kg), dim3(1024), back_lds, ctx->stream, F, LDG, G, fail, beta);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

extern "C" int gmmvi_more_blocked(gmmvi_ctx* ctx, int K, int D, const float* packed_dev, const float* chols_dev,
                                  const float* X_dev, int N, const float* ld_dev, const float* logq_dev, const float* bg_dev,
                                  const float* tlp_dev, const int32_t* mapping_dev, int map_offset, int flags,
                                  const float* l2_dev, float* H_neg_out_dev, float* g_neg_out_dev) {
    if (!ctx) return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_blocked: no context");
    if (D < 64 || D > GMMVI_MORE_BLOCKED_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_blocked: D = " + std::to_string(D) +
                                                  " is outside the supported range 64 <= D <= 128 (gmmvi_more serves D <= 63)");
    if (!gmmvi_is_blocked_dim(D))
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_blocked: D = 64 is a register-path dimension in this process "
                                              "(GMMVI_BLOCKED_ABOVE = 64); the route serves the blocked layout, 64 <= D <= 128");
    if (K < 1 || N < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_blocked: K >= 1 and N >= 1 are required (64 <= D <= 128)");
    const bool own_only = (flags & GMMVI_OWN_SAMPLES_ONLY) != 0;
    if (!(packed_dev && chols_dev && X_dev && logq_dev && tlp_dev && l2_dev && H_neg_out_dev && g_neg_out_dev) ||
        (own_only ? mapping_dev == nullptr : !(ld_dev && bg_dev)))
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "gmmvi_more_blocked: a required device pointer is null (64 <= D <= 128)");

    const size_t pstride = gmmvi_blocked_stride(D);
    const int linv_ofs = gmmvi_blocked_linv_ofs(D);
    static const MorePanelNames prof = {"more_blocked_lse", "more_blocked_whiten", "more_blocked_gram", "more_blocked_cholesky",
                                        "more_blocked_solve"};
    MorePanelPlan p;
    int rc = more_panel_plan(ctx, K, N, D, D * (D + 1) / 2 + D + 1, (size_t)D * D * sizeof(double), &p);
    if (rc != GMMVI_OK) return rc;
    const size_t whiten_lds = (size_t)D * 65 * sizeof(float);
    const size_t gram_lds = ((size_t)256 * PHI_LD + (size_t)(D + 3) * 64 + 256) * sizeof(float);
    rc = gmmvi_ensure_dynamic_lds(ctx, (const void*)mb_gram_kernel,                    // once: the limit of D = 128
                                  ((size_t)256 * PHI_LD + (size_t)(128 + 3) * 64 + 256) * sizeof(float));
    if (rc != GMMVI_OK) return rc;
    return more_panel_run(
        ctx, p, prof, K, N, ld_dev, bg_dev, mapping_dev, map_offset, flags, l2_dev,
        [&](int k0, int kg) {
            hipLaunchKernelGGL(mb_whiten_kernel, dim3(p.n_tiles, kg), dim3(256), whiten_lds, ctx->stream, D, N, p.n_tiles, k0,
                               pstride, linv_ofs, packed_dev, X_dev, ld_dev, bg_dev, tlp_dev, logq_dev, mapping_dev, map_offset,
                               flags, p.lse, p.Zt);
        },
        [&](int kg) {
            hipLaunchKernelGGL(mb_gram_kernel, dim3(p.nblk * (p.nblk + 1) / 2, kg), dim3(512), gram_lds, ctx->stream, D,
                               p.n_tiles, p.LDG, p.Zt, p.G);
        },
        [&](int k0, int kg) {
            hipLaunchKernelGGL(mb_unwhiten_right_kernel, dim3(D, kg), dim3(128), 0, ctx->stream, D, p.LDG, k0, pstride, linv_ofs,
                               packed_dev, p.beta, p.fail, p.T);
            hipLaunchKernelGGL(mb_unwhiten_left_kernel, dim3(D, kg), dim3(128), 0, ctx->stream, D, p.LDG, k0, pstride, linv_ofs,
                               packed_dev, p.beta, p.fail, p.T, H_neg_out_dev, g_neg_out_dev);
        });
}
