// Device helpers of the one-workgroup-per-component factorisation kernels of the blocked path (blocked.hip: component blocks,
// Cholesky; blocked_update.hip: tridiagonalisation, final factorisation): block reductions, the blocked triangular solve and
// Cholesky factorisation with their LDS sizes, the workgroup sizes.  Private to these two files.
#pragma once
#include "common.h"
#include "wave_reduce.h"
#include <cfloat>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the dynamic LDS limit the factorisation and search kernels are raised to (the kernels also hold a few static words beside it)
constexpr size_t BLK_LDS_LIMIT = 156 * 1024;

// ---------------------------------------------------------------------------------------------------------------------------
// small helpers
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum(float v, float* red) {          // red: >= 16 floats of LDS; result block-uniform
    v = gmmvi_wave_sum(v);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}
// Variants without the leading barrier: the caller guarantees that a barrier separates this call from the previous readers
// of the same `red` words (the tridiagonalisation alternates between two disjoint ranges, with barriers of its own in between).
__device__ __forceinline__ float block_sum_nb(float v, float* red) {
    v = gmmvi_wave_sum(v);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = 0.f;
    for (int i = 0; i < nw; ++i) s += red[i];
    return s;
}
__device__ __forceinline__ void block_sum2_nb(float& a, float& b, float* red) {
    a = gmmvi_wave_sum(a);
    b = gmmvi_wave_sum(b);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[16 + w] = b; }
    __syncthreads();
    float sa = 0.f, sb = 0.f;
    for (int i = 0; i < nw; ++i) { sa += red[i]; sb += red[16 + i]; }
    a = sa; b = sb;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    v = gmmvi_wave_max(v);
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    float s = -3.0e38f;
    for (int i = 0; i < nw; ++i) s = fmaxf(s, red[i]);
    return s;
}

// Forward substitution T x = r with a lower-triangular T, one thread per right-hand side, 32 rows at a time:
// thread t solves for rhs(i, t), i = 0..D-1, knowing that its solution vanishes for i < i0; X[i * ldx + t] receives it
// (coalesced over t).  Per block of 32 rows the rows of T are staged in LDS (Ts: 32 x (D + 4) floats) and the thread keeps
// its 32 partial sums in registers: every solved x is read back from memory once per block (not once per row), the
// multiplies run on broadcast 16-byte LDS reads.  TCM: T is given column-major (T[i][c] at Tm[c * D + i]).
constexpr int TRB = 32;
// row stride of the staged rows: a multiple of 4 (16-byte reads) whose quarter is odd (the matrix-core operand reads walk the
// rows: stride 4 * odd spreads 32 rows over 16 banks)
__host__ __device__ inline int blk_trsm_ld(int D) {
    const int ld = ((D + 3) / 4) * 4 + 4;
    return (ld / 4) % 2 == 0 ? ld + 4 : ld;
}
inline size_t blk_trsm_lds_floats(int D) { return (size_t)TRB * blk_trsm_ld(D) + (size_t)(D + 1) * (TRB + 1); }     // + sums of up to D + 1 right-hand sides

template <bool TCM, class RhsF>
__device__ void blk_trsm(int D, const float* __restrict__ Tm, int nrhs, RhsF rhs, int i0, float* X, int ldx, float* Ts) {
    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6, nwave = blockDim.x >> 6, col = lane & 31, half = lane >> 5;
    const int ld = blk_trsm_ld(D);
    float* Ss = Ts + (size_t)TRB * ld;                     // [rhs][33]: what the solved rows contribute to the current block
    for (int I = 0; I < D; I += TRB) {
        const int nbk = min(TRB, D - I), w = I + nbk;
        __syncthreads();
        if (TCM) {
            for (int e = t; e < w * TRB; e += blockDim.x) {
                const int c = e / TRB, r = e % TRB;
                if (r < nbk) Ts[r * ld + c] = (c <= I + r) ? Tm[(size_t)c * D + I + r] : 0.f;
            }
        } else {
            for (int c = t; c < w; c += blockDim.x) {          // row by row: no index divisions, every load independent
#pragma unroll 8
                for (int r = 0; r < nbk; ++r) Ts[r * ld + c] = Tm[(size_t)(I + r) * D + c];
            }
        }
        __syncthreads();
        // what the solved rows contribute to this block, S[r][t] = sum_{c < I} T[I + r][c] x_c(t), as matrix-core tiles (wave w
        // takes the 32-rhs tiles w, w + waves, ..: A operand from the staged rows, B operand = dword loads of X from the L2),
        // handed to the right-hand sides' threads through LDS (this sum as per-thread multiply-adds over
        // broadcast LDS reads was the bulk of the 0.96 M cycles of the solve at D = 300)
        if (I > 0) {
            const int ntile = (nrhs + TRB - 1) / TRB;
            for (int tile = wave; tile < ntile; tile += nwave) {
                const int t0 = TRB * tile;
                const float* pa = Ts + col * ld;                               // rows past nbk: unused results
                const float* pb = X + min(t0 + col, nrhs - 1);
                f32x16 sacc;
#pragma unroll
                for (int j = 0; j < 16; ++j) sacc[j] = 0.f;
                for (int c = 0; c < I; c += 16) {                              // I is a multiple of 32
                    float av[8], bv[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        av[u] = pa[c + 2 * u + half];
                        bv[u] = pb[(size_t)(c + 2 * u + half) * ldx];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], sacc, 0, 0, 0);
                }
                if (t0 + col < nrhs) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) Ss[(size_t)(t0 + col) * (TRB + 1) + (j & 3) + 8 * (j >> 2) + 4 * half] = sacc[j];
                }
            }
            __syncthreads();
        }
        if (t >= nrhs) continue;
        float acc[TRB];
        if (I + TRB <= i0) {                                   // structurally zero rows
#pragma unroll
            for (int r = 0; r < TRB; ++r)
                if (r < nbk) X[(size_t)(I + r) * ldx + t] = 0.f;
            continue;
        }
#pragma unroll
        for (int r = 0; r < TRB; ++r) acc[r] = (r < nbk) ? rhs(I + r, t) - (I > 0 ? Ss[(size_t)t * (TRB + 1) + r] : 0.f) : 0.f;
#pragma unroll
        for (int r = 0; r < TRB; ++r) {
            if (r < nbk) {
                float sv = acc[r];
#pragma unroll
                for (int q4 = 0; q4 < r; q4 += 4) {                            // 16-byte broadcast reads of the pivot row
                    const float4 pr = *reinterpret_cast<const float4*>(Ts + r * ld + I + q4);
                    sv = fmaf(-pr.x, acc[q4], sv);
                    if (q4 + 1 < r) sv = fmaf(-pr.y, acc[q4 + 1], sv);
                    if (q4 + 2 < r) sv = fmaf(-pr.z, acc[q4 + 2], sv);
                    if (q4 + 3 < r) sv = fmaf(-pr.w, acc[q4 + 3], sv);
                }
                acc[r] = sv / Ts[r * ld + I + r];
                X[(size_t)(I + r) * ldx + t] = acc[r];
            }
        }
    }
    __syncthreads();
}

// Cholesky factorisation A = C C^T of the symmetric matrix a(i, j) (i >= j read), left-looking over blocks of 32 columns,
// one thread per row; the factor is built column-major (W[c * D + i] = C[i][c]: thread i walks coalesced rows of W).
// Per column block J the sums over the finished columns, S[i][r] = sum_{c < J} C[i][c] C[J + r][c] for the rows i >= J, are
// matrix-core tiles (v_mfma_f32_32x32x2_f32: wave w takes the 32-row tiles w, w + waves, ..; both operands are dword loads of
// W straight from the L2, sixteen k in flight) handed to the row threads through LDS (Sm: D x 33; this accumulation as
// per-thread multiply-adds over broadcast LDS reads was 0.6 M of the factorisation's 1.4 M cycles at D = 300); then every
// thread finishes its 32 entries, one wave factorises the 32 x 32 diagonal block in LDS (Dg), the other rows solve against
// it.  LDS: blk_chol_lds_floats(D).  Returns false (block-uniform) on a non-positive or non-finite pivot.
constexpr int DGS = TRB + 4;                            // row stride of the diagonal block in LDS: 16-byte aligned rows
inline size_t blk_chol_lds_floats(int D) { return (size_t)(((D * (TRB + 1) + 3) / 4) * 4) + TRB * DGS + 4; }

template <class ElemF>
__device__ bool blk_cholesky(int D, ElemF a, float* W, float* lds) {
    float* Sm = lds;                                   // [i][33], rows J <= i < D
    float* Dg = lds + (size_t)(((D * (TRB + 1) + 3) / 4) * 4);          // [32][DGS]
    int* fail = reinterpret_cast<int*>(Dg + TRB * DGS);
    const int i = threadIdx.x;
    const int lane = i & 63, wave = i >> 6, nwave = blockDim.x >> 6;
    const int col = lane & 31, half = lane >> 5;
    if (i == 0) *fail = 0;
    for (int J = 0; J < D; J += TRB) {
        const int nbk = min(TRB, D - J);
        __syncthreads();
        // S tiles: result row m = r (A operand: C[J + r][c]), result column n = matrix row i (B operand: C[i][c]); the lane
        // holds column n = col and the rows m = (j & 3) + 8 (j >> 2) + 4 half of its 16 registers
        const int ntile = (D - J + TRB - 1) / TRB;
        for (int tile = wave; J > 0 && tile < ntile; tile += nwave) {
            const int i0 = J + TRB * tile;
            const float* pa = W + min(J + col, D - 1);             // rows past the matrix read its last row (never used)
            const float* pb = W + min(i0 + col, D - 1);
            f32x16 sacc;
#pragma unroll
            for (int j = 0; j < 16; ++j) sacc[j] = 0.f;
            for (int c = 0; c < J; c += 16) {                      // J is a multiple of 32
                float av[8], bv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    av[u] = pa[(size_t)(c + 2 * u + half) * D];
                    bv[u] = pb[(size_t)(c + 2 * u + half) * D];
                }
#pragma unroll
                for (int u = 0; u < 8; ++u) sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u], sacc, 0, 0, 0);
            }
            if (i0 + col < D) {
#pragma unroll
                for (int j = 0; j < 16; ++j) Sm[(size_t)(i0 + col) * (TRB + 1) + (j & 3) + 8 * (j >> 2) + 4 * half] = sacc[j];
            }
        }
        __syncthreads();
        float acc[TRB];
        const bool mine = i >= J && i < D;
        if (mine) {
#pragma unroll
            for (int r = 0; r < TRB; ++r)
                acc[r] = (r < nbk && J + r <= i) ? a(i, J + r) - (J > 0 ? Sm[(size_t)i * (TRB + 1) + r] : 0.f) : 0.f;
            if (i < J + nbk) {
#pragma unroll
                for (int r = 0; r < TRB; ++r) Dg[(i - J) * DGS + r] = acc[r];
            }
        }
        __syncthreads();
        if (i < 32) {
            // half of wave 0: 32 x 32 Cholesky, lane = row.  The lane keeps ITS row in registers; the pivot row r (complete
            // after step r - 1: every step publishes the new column) comes from LDS as 16-byte broadcast reads; the sums run
            // over q = 0, 1, .. as before (bit-identical), but with static indices: no dependent LDS read per term (that loop
            // was 57 k cycles a block: more than half of the factorisation at D = 300)
            const int l = i;
            float rw[TRB];
#pragma unroll
            for (int c = 0; c < TRB; ++c) rw[c] = Dg[l * DGS + c];
            bool bad = false;
#pragma unroll
            for (int r = 0; r < TRB; ++r) {
                if (r < nbk && !bad) {
                    float sv = rw[r];
#pragma unroll
                    for (int q4 = 0; q4 < r; q4 += 4) {
                        const float4 pr = *reinterpret_cast<const float4*>(Dg + r * DGS + q4);
                        sv = fmaf(-rw[q4], pr.x, sv);
                        if (q4 + 1 < r) sv = fmaf(-rw[q4 + 1], pr.y, sv);
                        if (q4 + 2 < r) sv = fmaf(-rw[q4 + 2], pr.z, sv);
                        if (q4 + 3 < r) sv = fmaf(-rw[q4 + 3], pr.w, sv);
                    }
                    const float pv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(sv), r));
                    if (!(pv > 0.f) || !(pv < FLT_MAX)) {
                        bad = true;
                    } else {
                        const float d = sqrtf(pv);
                        rw[r] = (l == r) ? d : sv / d;
                        if (l >= r && l < nbk) Dg[l * DGS + r] = rw[r];
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        __builtin_amdgcn_wave_barrier();
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    }
                }
            }
            if (bad && i == 0) *fail = 1;
        }
        __syncthreads();
        if (*fail) return false;
        if (mine) {
            if (i < J + nbk) {
                const int l = i - J;
#pragma unroll
                for (int r = 0; r < TRB; ++r)
                    if (r <= l) W[(size_t)(J + r) * D + i] = Dg[l * DGS + r];
            } else {
#pragma unroll
                for (int r = 0; r < TRB; ++r) {
                    if (r < nbk) {
                        float sv = acc[r];
#pragma unroll
                        for (int q4 = 0; q4 < r; q4 += 4) {                    // 16-byte broadcast reads of the pivot row
                            const float4 pr = *reinterpret_cast<const float4*>(Dg + r * DGS + q4);
                            sv = fmaf(-acc[q4], pr.x, sv);
                            if (q4 + 1 < r) sv = fmaf(-acc[q4 + 1], pr.y, sv);
                            if (q4 + 2 < r) sv = fmaf(-acc[q4 + 2], pr.z, sv);
                            if (q4 + 3 < r) sv = fmaf(-acc[q4 + 3], pr.w, sv);
                        }
                        acc[r] = sv / Dg[r * DGS + r];
                        W[(size_t)(J + r) * D + i] = acc[r];
                    }
                }
            }
        }
    }
    __syncthreads();
    return true;
}

inline int blk_threads(int D) { return ((D + 63) / 64) * 64; }
// factorisation kernels: one wavefront per 32-row / 32-rhs tile of the matrix-core sums when that fits (D <= 320: <= 11 waves),
// else one thread per row as everywhere
inline int blk_threads_mm(int D) { return D <= 320 ? 64 * ((D + 31) / 32) : blk_threads(D); }

}  // namespace
