// The batched contraction of the blocked path (blocked_gemm.hip) as its callers see it (blocked.hip: densities, sampling, Stein
// estimate; blocked_update.hip: component updates).  Private to these three files.
#pragma once
#include "blocked.h"
#include <cstring>

// ---------------------------------------------------------------------------------------------------------------------------
// batched contraction  C[b] (+)= alpha * opA(A[b]) * opB(B[b]) (+ bias)   on v_mfma_f32_32x32x2_f32
// ---------------------------------------------------------------------------------------------------------------------------
// Workgroup = 128 x (32 NT) tile of C, 4 waves stacked along M: wave w owns rows 32 w .. 32 w + 31 and NT 32 x 32 MFMA
// tiles (16 NT accumulator registers); NT in {2..5} is chosen per launch so that the padded width wastes the least
// (D = 300: NT = 5, 320 columns).  The k dimension advances 16 at a time through two LDS images per operand, stored
// k-major ([k][row]; row strides of 132 / 32 NT + 4 words keep 16-byte alignment for ds_write_b128 and let the lanes of a
// ds_read_b32 walk consecutive rows).  Every thread moves 4 consecutive elements along the contiguous direction of its
// operand (one 16-byte load when the operand is aligned), global loads of step s+1 are in flight while step s is
// multiplied.  The f32 MFMA shares the vector ALU on gfx950 (it does not co-execute), so the staging code is kept to a
// few vector instructions per 16-byte load: uniform base pointers + per-thread offsets fixed for the whole launch.
// The A operand takes an element-wise prologue (subtract a vector along k, scale along k, scale along rows), which is how
// "x - mu", the importance weights and the responsibilities enter without being materialised.  A triangular opB skips
// the 32-column sub-tiles whose k range is structurally zero.
struct BG {
    const float* A; const float* B; float* C;
    int M, N, Kd;
    int lda, ldb, ldc;
    long long sA, sB, sC;            // batch strides (floats)
    int a_kmajor;                    // 0: A[m * lda + k]      1: A[k * lda + m]
    int b_kmajor;                    // 0: B[n * ldb + k]      1: B[k * ldb + n]
    const float* a_sub; long long s_asub;        // [Kd]  A(m, k) -= a_sub[k]
    const float* a_kscale; long long s_aks;      // [Kd]  A(m, k) *= a_kscale[k]
    const float* a_rscale; long long s_ars;      // [M]   A(m, k) *= a_rscale[m]
    const float* a_rsub; long long s_arsub;      // [M]   with a_kscale (k-major A only): A(m, k) = (A(m, k) - a_rsub[m]) * a_kscale[k]
    const float* c_bias; long long s_cb;         // [N]   C(m, n) += c_bias[n]
    const int32_t* row_off;          // optional [batches + 1]: batch b owns rows [row_off[b], row_off[b+1]) of A and C (M = bound)
    int inner;                       // > 0: workgroup z accumulates the batches [z * inner, min((z+1) * inner, inner_total)) into slab z of C
    int inner_total;
    int tri;                         // 1: opB(k, n) = 0 for k > n   2: opB(k, n) = 0 for k < n
    int accumulate;                  // C += result
    int ksplit;                      // > 1: grid.z = batches * ksplit, slab z of C receives the partial sum over its k range
    float alpha;
    // optional: per-row sums of squares of this workgroup's result columns, rowsq[blockIdx.x * rs_tile + blockIdx.z * rs_batch +
    // row] (one partial per column tile; the caller adds the tiles).  no_store: the result itself is not written.
    float* rowsq; long long rs_tile, rs_batch;
    int no_store;
    int debug;                       // experiments (GMMVI_BG_DEBUG): 1 no MFMAs, 2 no split / LDS writes, 4 no global loads
};

constexpr int BK = 16;               // the k step of both routes

inline BG bg_zero() {
    BG g;
    memset(&g, 0, sizeof(g));
    g.alpha = 1.f;
    return g;
}

#define BLK_TRY(call) do { int rc__ = (call); if (rc__ != GMMVI_OK) return rc__; } while (0)

// C (+)= alpha opA(A) opB(B) for batches_outer batches (slabs with g.inner / g.ksplit): GMMVI_ERR_ARG for an operand layout /
// prologue pair that is not instantiated
int gmmvi_bgemm(gmmvi_ctx* ctx, const BG& g, int batches_outer);
// whether a launch with n result columns and a contraction over kd takes the split-operand route
bool gmmvi_bgemm_use_split(int n, int kd);
// number of column tiles that launch will use
int gmmvi_bgemm_col_tiles(int n, int kd);
