// The batched f32 contraction of the blocked path (blocked_gemm.h: BG, the prologues): on the f32 matrix-core instruction
// (bgemm_kernel), or -- wide and long launches, the default -- on the bf16 instruction through 3-way split operands at f32
// accuracy (bsplit_image_kernel + bgemm_ws_kernel); the route and tile width of a launch, the launch.
#include "blocked_gemm.h"
#include "bf16_split.h"
#include "wave_reduce.h"
#include <cstdlib>

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, LDA_S = BM + 4;

// 4 consecutive floats, the first nvalid of them in range (others 0); one 16-byte load when allowed
__device__ __forceinline__ float4 ld4(const float* p, int nvalid, bool vec) {
    if (vec && nvalid >= 4) return *reinterpret_cast<const float4*>(p);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (nvalid > 0) r.x = p[0];
    if (nvalid > 1) r.y = p[1];
    if (nvalid > 2) r.z = p[2];
    if (nvalid > 3) r.w = p[3];
    return r;
}
__device__ __forceinline__ bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ---- split-operand route (SPLIT = 1): the same f32 contraction on the bf16 matrix cores ------------------------------
// Every f32 operand element is written as x = x1 + x2 + x3 with three bf16 values (round-to-nearest splits: |x2| <= 2^-9 |x|,
// |x3| <= 2^-18 |x|, residual <= 2^-27 |x|); a product x y is the sum of the six partial products x_i y_j with i + j <= 4
// (each EXACT in f32: 8 x 8 significant bits), accumulated in f32 by v_mfma_f32_32x32x16_bf16, smallest terms first.  The
// dropped terms (x2 y3, x3 y2, x3 y3 and the residuals) are below 2^-25 |x y|: less than the rounding of one f32 multiply-add,
// so the result carries the error of an f32 contraction (tests/test_hip_blocked.py measures both routes against fp64).
// Six bf16 MFMAs (6 x 32 cycles per 32 x 32 x 16) replace eight f32 MFMAs (8 x 64 cycles): 2.7 x the matrix-core rate.
// LDS images per operand and plane, 16 k per step: a k-contiguous operand is stored in fragment order ([k / 8][row][k % 8]:
// lane l of a ds_read_b128 reads 16 consecutive bytes after lane l - 1); a k-major operand is stored [k][row] (row stride
// 2 * rowsp bytes = 64 or 192 mod 256: the four k rows of a transposed read fall into disjoint banks) and read with
// ds_read_b64_tr_b16, which hands lane i of a 16-lane group column i of a 4 x 16 block -- the MFMA operand order.
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
// (bf16x2_t, f32x2_t, cvt_pk_bf16, split_pair: bf16_split.h)
constexpr int split_rowsp(int rows) {                  // row stride (elements) of a k-major bf16 image
    int r = rows;
    while (r % 128 != 32 && r % 128 != 96) r += 4;
    return r;
}
__device__ __forceinline__ i32x4 lds_tr_frag(const unsigned char* base, int byte_off, int row_stride_bytes) {
    typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + byte_off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(base + byte_off + 4 * row_stride_bytes));
    i32x4 r;
    r[0] = __builtin_bit_cast(int2, lo).x; r[1] = __builtin_bit_cast(int2, lo).y;
    r[2] = __builtin_bit_cast(int2, hi).x; r[3] = __builtin_bit_cast(int2, hi).y;
    return r;
}

// NT: 32-column MFMA tiles per wave; AK / BKM: operand is k-major in memory; PRO: prologue on A (0 none, 1 subtract a
// vector along k, 2 scale rows, 3 scale along k, 4 subtract a vector along the rows, then scale along k: k-major A only).  Every step takes one of two routes, chosen uniformly: the fast route
// (aligned operands, a full 16-wide k step, every 16-byte piece entirely valid or entirely void -- decided once per thread)
// issues all loads back to back without a branch; the edge route handles ragged ends element by element.
template <int NT, int AK, int BKM, int PRO>
__global__ __launch_bounds__(256, PRO == 2 ? 2 : 3) void bgemm_kernel(BG g) {
    constexpr int BN = 32 * NT, LDB_S = BN + 4;
    constexpr int NVB = (BN * BK / 4 + 255) / 256;          // 16-byte pieces of the B tile per thread
    __shared__ __align__(16) float As[2][BK * LDA_S];
    __shared__ __align__(16) float Bs[2][BK * LDB_S];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 31, half = lane >> 5;
    const int m0 = blockIdx.y * BM, n0 = blockIdx.x * BN;
    const int nsplit = g.ksplit > 1 ? g.ksplit : 1;
    const int bz = blockIdx.z / nsplit, kz = blockIdx.z - bz * nsplit;
    int Mb = g.M;
    long long rowbase = 0;
    if (g.row_off) { rowbase = g.row_off[bz]; Mb = g.row_off[bz + 1] - (int)rowbase; }
    if (m0 >= Mb) return;
    int kb = 0, ke = g.Kd;
    if (g.tri == 1) ke = min(g.Kd, n0 + BN);
    else if (g.tri == 2) kb = min(g.Kd, n0) & ~3;
    if (nsplit > 1) {
        const int chunk = ((g.Kd + nsplit - 1) / nsplit + BK - 1) / BK * BK;
        kb = min(g.Kd, kz * chunk);
        ke = min(g.Kd, kb + chunk);
    }
    const int spb = (ke - kb + BK - 1) / BK;
    const int nb = g.inner > 0 ? min(g.inner, g.inner_total - bz * g.inner) : 1;
    const int total = nb * spb;
    const float* A0 = g.A + (AK ? rowbase : rowbase * g.lda);
    const float* pro = PRO == 1 ? g.a_sub : (PRO == 2 ? g.a_rscale : (PRO >= 3 ? g.a_kscale : nullptr));
    const long long s_pro = PRO == 1 ? g.s_asub : (PRO == 2 ? g.s_ars : (PRO >= 3 ? g.s_aks : 0));
    const bool vecR = PRO != 4 || (al16(g.a_rsub) && (g.s_arsub & 3) == 0);
    const bool vecA = al16(A0) && ((g.lda | g.sA) & 3) == 0;
    const bool vecB = al16(g.B) && ((g.ldb | g.sB) & 3) == 0;
    const bool vecP = PRO == 0 || (al16(pro) && (s_pro & 3) == 0);
    // fast route: no 16-byte piece may straddle the end of its operand
    const bool fast_ok = vecA && vecB && (PRO != 1 || vecP) && vecR && (!AK || (Mb & 3) == 0 || m0 + BM <= Mb) &&
                         (!BKM || (g.N & 3) == 0 || n0 + BN <= g.N);

    // per-thread pieces: A tile = 512 pieces (2 per thread), B tile = 4 BN pieces
    // k-contiguous operand: piece = (row r, 4 consecutive k); k-major operand: piece = (k row, 4 consecutive rows)
    int a_r[2], a_k[2], a_off[2];
    bool a_ok[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int idx = tid + 256 * u;
        if (AK) { a_k[u] = idx >> 5; a_r[u] = 4 * (idx & 31); } else { a_r[u] = idx >> 2; a_k[u] = 4 * (idx & 3); }
        a_ok[u] = m0 + a_r[u] < Mb;
        a_off[u] = a_ok[u] ? (AK ? a_k[u] * g.lda + m0 + a_r[u] : (m0 + a_r[u]) * g.lda + a_k[u]) : 0;
    }
    int b_c[NVB], b_k[NVB], b_off[NVB];
    bool b_ok[NVB];
#pragma unroll
    for (int u = 0; u < NVB; ++u) {
        const int idx = tid + 256 * u;
        if (BKM) { b_k[u] = idx / (BN / 4); b_c[u] = 4 * (idx % (BN / 4)); } else { b_c[u] = idx >> 2; b_k[u] = 4 * (idx & 3); }
        if (idx >= BN * BK / 4) { b_c[u] = BN; b_k[u] = 0; }            // no piece
        b_ok[u] = b_c[u] < BN && n0 + b_c[u] < g.N;
        b_off[u] = b_ok[u] ? (BKM ? b_k[u] * g.ldb + n0 + b_c[u] : (n0 + b_c[u]) * g.ldb + b_k[u]) : 0;
    }

    float4 ra[2], rb[NVB], pv[2], pw[2];
    bool pending = false;                   // fast route: prologue / masking of the staged pieces still to be applied
    auto gload = [&](int step) {
        pending = false;
        const int bi = step / spb;
        const long long b = (long long)bz * (g.inner > 0 ? g.inner : 1) + bi;
        const int k0 = kb + (step - bi * spb) * BK;
        const float* Ab = A0 + b * g.sA;
        const float* Bb = g.B + b * g.sB;
        const float* pb = PRO ? pro + b * s_pro : nullptr;
        const float* pr = PRO == 4 ? g.a_rsub + b * g.s_arsub : nullptr;
        if (fast_ok && k0 + BK <= ke) {
            const float* Ak = Ab + (AK ? (long long)k0 * g.lda : (long long)k0);
            const float* Bk = Bb + (BKM ? (long long)k0 * g.ldb : (long long)k0);
            // loads only: the prologue and the masking wait for the data, so they run in sstore, after this step's MFMAs
#pragma unroll
            for (int u = 0; u < 2; ++u) ra[u] = *reinterpret_cast<const float4*>(Ak + a_off[u]);
#pragma unroll
            for (int u = 0; u < NVB; ++u) rb[u] = *reinterpret_cast<const float4*>(Bk + b_off[u]);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                if (PRO == 1) {
                    if (AK) { const float s = pb[k0 + a_k[u]]; pv[u] = make_float4(s, s, s, s); }
                    else pv[u] = *reinterpret_cast<const float4*>(pb + k0 + a_k[u]);
                } else if (PRO == 2) {
                    // rows that do not exist read element 0 (masked in sstore): no branch around the load
                    if (AK) pv[u] = *reinterpret_cast<const float4*>(pb + (a_ok[u] ? m0 + a_r[u] : 0));
                    else { const float s = pb[a_ok[u] ? m0 + a_r[u] : 0]; pv[u] = make_float4(s, s, s, s); }
                } else if (PRO == 3) {
                    if (AK) { const float s = pb[k0 + a_k[u]]; pv[u] = make_float4(s, s, s, s); }
                    else pv[u] = ld4(pb + k0 + a_k[u], 4, vecP);
                } else if (PRO == 4) {
                    const float s = pb[k0 + a_k[u]];
                    pv[u] = make_float4(s, s, s, s);
                    pw[u] = *reinterpret_cast<const float4*>(pr + (a_ok[u] ? m0 + a_r[u] : 0));
                }
            }
            pending = true;
            return;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int gm = m0 + a_r[u], gk = k0 + a_k[u];
            float4 v;
            if (AK) {                                           // 4 consecutive rows of one k
                const int nv = (gk < ke) ? Mb - gm : 0;
                v = ld4(Ab + (long long)gk * g.lda + gm, nv, vecA);
                if (nv > 0) {
                    if (PRO == 1) { const float s = pb[gk]; v.x -= s; v.y -= s; v.z -= s; v.w -= s; }
                    if (PRO == 3) { const float s = pb[gk]; v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
                    if (PRO == 2) { const float4 s = ld4(pb + gm, nv, vecP); v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w; }
                    if (PRO == 4) {
                        const float4 r4 = ld4(pr + gm, nv, vecR);
                        const float s = pb[gk];
                        v.x = (v.x - r4.x) * s; v.y = (v.y - r4.y) * s; v.z = (v.z - r4.z) * s; v.w = (v.w - r4.w) * s;
                    }
                    if (nv < 4) { if (nv < 2) v.y = 0.f; if (nv < 3) v.z = 0.f; v.w = 0.f; }
                }
            } else {                                            // 4 consecutive k of one row
                const int nv = (gm < Mb) ? ke - gk : 0;
                v = ld4(Ab + (long long)gm * g.lda + gk, nv, vecA);
                if (nv > 0) {
                    if (PRO == 1) { const float4 s = ld4(pb + gk, nv, vecP); v.x -= s.x; v.y -= s.y; v.z -= s.z; v.w -= s.w; }
                    if (PRO == 3) { const float4 s = ld4(pb + gk, nv, vecP); v.x *= s.x; v.y *= s.y; v.z *= s.z; v.w *= s.w; }
                    if (PRO == 2) { const float s = pb[gm]; v.x *= s; v.y *= s; v.z *= s; v.w *= s; }
                    if (nv < 4) { if (nv < 2) v.y = 0.f; if (nv < 3) v.z = 0.f; v.w = 0.f; }
                }
            }
            ra[u] = v;
        }
#pragma unroll
        for (int u = 0; u < NVB; ++u) {
            const int gn = n0 + b_c[u], gk = k0 + b_k[u];
            if (BKM) {
                const int nv = (gk < ke && b_c[u] < BN) ? g.N - gn : 0;
                rb[u] = ld4(Bb + (long long)gk * g.ldb + gn, nv, vecB);
            } else {
                const int nv = (gn < g.N && b_c[u] < BN) ? ke - gk : 0;
                rb[u] = ld4(Bb + (long long)gn * g.ldb + gk, nv, vecB);
            }
        }
    };
    auto sstore = [&](int buf) {
        if (pending) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                float4 v = ra[u];
                if (PRO == 1) { v.x -= pv[u].x; v.y -= pv[u].y; v.z -= pv[u].z; v.w -= pv[u].w; }
                if (PRO == 4) { v.x -= pw[u].x; v.y -= pw[u].y; v.z -= pw[u].z; v.w -= pw[u].w; }
                if (PRO >= 2) { v.x *= pv[u].x; v.y *= pv[u].y; v.z *= pv[u].z; v.w *= pv[u].w; }
                ra[u] = a_ok[u] ? v : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < NVB; ++u) rb[u] = b_ok[u] ? rb[u] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            if (AK) {
                *reinterpret_cast<float4*>(&As[buf][a_k[u] * LDA_S + a_r[u]]) = ra[u];
            } else {
                float* d = &As[buf][a_k[u] * LDA_S + a_r[u]];
                d[0] = ra[u].x; d[LDA_S] = ra[u].y; d[2 * LDA_S] = ra[u].z; d[3 * LDA_S] = ra[u].w;
            }
        }
#pragma unroll
        for (int u = 0; u < NVB; ++u) {
            if (b_c[u] >= BN) continue;
            if (BKM) {
                *reinterpret_cast<float4*>(&Bs[buf][b_k[u] * LDB_S + b_c[u]]) = rb[u];
            } else {
                float* d = &Bs[buf][b_k[u] * LDB_S + b_c[u]];
                d[0] = rb[u].x; d[LDB_S] = rb[u].y; d[2 * LDB_S] = rb[u].z; d[3 * LDB_S] = rb[u].w;
            }
        }
    };
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    if (total > 0) {
        gload(0);
        sstore(0);
    }
    __syncthreads();
    int buf = 0;
    for (int step = 0; step < total; ++step) {
        if (step + 1 < total) gload(step + 1);
        const int k0 = kb + (step % spb) * BK;
        const float* a_ = As[buf] + half * LDA_S + wave * 32 + col;
        const float* b_ = Bs[buf] + half * LDB_S + col;
        float av[BK / 2];
#pragma unroll
        for (int k2 = 0; k2 < BK / 2; ++k2) av[k2] = a_[2 * k2 * LDA_S];
        // sub-tile t (columns n0 + 32 t ..) is skipped for this k range when opB vanishes there or the columns do not exist.
        // (One uniform branch per sub-tile: straight-line variants per live range were measured -- the accumulator copies
        // between the variants double the register count and halve the occupancy, 1.6x slower.)
        // the B operands of sub-tile t + 1 are read (unconditionally) before the MFMAs of sub-tile t are issued, so the LDS
        // latency of a block hides behind the previous block's eight MFMAs.  The MFMAs are issued through inline asm with
        // the accumulators pinned to AGPRs: with the builtin the compiler kept acc[] in VGPRs across the (uniform) branches
        // and copied 16 registers into and out of one AGPR tuple around every block (400 v_accvgpr moves per k step).
        float bv[2][BK / 2];
#pragma unroll
        for (int k2 = 0; k2 < BK / 2; ++k2) bv[0][k2] = b_[2 * k2 * LDB_S];
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t + 1 < NT) {
#pragma unroll
                for (int k2 = 0; k2 < BK / 2; ++k2) bv[(t + 1) & 1][k2] = b_[2 * k2 * LDB_S + 32 * (t + 1)];
            }
            const int c0 = n0 + 32 * t;
            if (c0 < g.N && !(g.tri == 1 && k0 >= c0 + 32) && !(g.tri == 2 && k0 + BK <= c0)) {
#pragma unroll
                for (int k2 = 0; k2 < BK / 2; ++k2)
                    asm volatile("v_mfma_f32_32x32x2_f32 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(av[k2]), "v"(bv[t & 1][k2]));
            }
        }
        if (step + 1 < total) sstore(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }
    // the last MFMA (16 passes) must have retired before its accumulators are read (inline asm: no automatic hazard nops)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    if (g.rowsq != nullptr) {
        // lane (col, half) holds rows (r & 3) + 8 (r >> 2) + 4 half of its column in every sub-tile: square-sum over the
        // sub-tiles, then over the 32 lanes of the half
        float rs[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) rs[r] = 0.f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (n0 + 32 * t + col < g.N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) { const float v = g.alpha * acc[t][r]; rs[r] = fmaf(v, v, rs[r]); }
            }
        }
        float* rq = g.rowsq + (long long)blockIdx.x * g.rs_tile + (long long)blockIdx.z * g.rs_batch + rowbase;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = rs[r];
            v += __shfl_xor(v, 16); v += __shfl_xor(v, 8); v += __shfl_xor(v, 4); v += __shfl_xor(v, 2); v += __shfl_xor(v, 1);
            const int i = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (col == 0 && i < Mb) rq[i] = v;
        }
    }
    if (g.no_store) return;
    float* Cb = g.C + (long long)blockIdx.z * g.sC + rowbase * g.ldc;
    const float* bias = g.c_bias ? g.c_bias + (long long)bz * g.s_cb : nullptr;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = n0 + 32 * t + col;
        if (j >= g.N) continue;
        const float bj = bias ? bias[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (i < Mb) {
                float* p = Cb + (long long)i * g.ldc + j;
                float v = fmaf(g.alpha, acc[t][r], bj);
                if (g.accumulate) v += *p;
                *p = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// the same contraction, split-operand route: role-specialised workgroup on v_mfma_f32_32x32x16_bf16
// ---------------------------------------------------------------------------------------------------------------------------
// A wave issues one instruction every four cycles whatever its kind, an MFMA of this shape occupies the matrix core for 32:
// the kernel is paced by the matrix cores only if fewer than ~7 other instructions are issued per MFMA, address arithmetic
// and loop control included (first version of this route, every wave staging and multiplying: 8.9 vector + 7.4 scalar
// instructions per MFMA, matrix cores 19 % busy).  Hence:
//  * the B operand (component data / shared rows: reused by every row tile) is split ONCE per launch by bsplit_image_kernel
//    into the exact byte order of the LDS stage (per 16-k step: [plane][k half][column][8 k] bf16, transposed, masked for
//    triangular operands, zero-padded): staging B is a 16-byte copy;
//  * 512 threads: waves 0..3 MULTIPLY (wave w owns rows 32 w .. of the 128 x 32 NT tile; NT up to 10, so D <= 320 is ONE
//    column tile and (x - mu) is read and split once per component): LDS fragment reads and MFMAs only, the first fragments
//    of the next step are read before the last MFMAs of this one are issued; waves 4..7 STAGE: global loads (three register
//    stages: the loads of step s + 3 are issued when step s has been handed to LDS), the element-wise prologue and the
//    3-way split of A, the LDS writes;
//  * LDS is a ring of three stages; one LDS-only barrier per step (s_waitcnt lgkmcnt(0) + s_barrier: the stagers' global
//    loads stay in flight across it): during step t the multipliers read stage t % 3 (and the head of stage (t + 1) % 3,
//    complete since the previous barrier) while the stagers fill stage (t + 2) % 3.
#define BG_LDS_BARRIER()                                       \
    do {                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     \
        __builtin_amdgcn_s_barrier();                          \
        asm volatile("" ::: "memory");                         \
    } while (0)

template <int N> using bg_ic = std::integral_constant<int, N>;

// bytes of the B image of one (batch, 16-k step): three planes x two k halves x ncolp columns x 8 bf16
__host__ __device__ inline size_t bimg_step_bytes(int ncolp) { return (size_t)96 * ncolp; }

// B image: thread = (column n, k half h) of one (step, batch): eight k values -> three 16-byte fragments
__global__ __launch_bounds__(256) void bsplit_image_kernel(BG g, int ncolp, int nsteps, unsigned char* img) {
    const int step = blockIdx.x, b = blockIdx.y;
    const float* Bb = g.B + (long long)b * g.sB;
    unsigned char* out = img + ((size_t)b * nsteps + step) * bimg_step_bytes(ncolp);
    for (int e = threadIdx.x; e < 2 * ncolp; e += 256) {
        const int h = e / ncolp, n = e - h * ncolp;
        const int k0 = step * BK + 8 * h;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + j;
            bool live = n < g.N && k < g.Kd;
            if (g.tri == 1) live = live && k <= n;
            if (g.tri == 2) live = live && k >= n;
            v[j] = live ? (g.b_kmajor ? Bb[(long long)k * g.ldb + n] : Bb[(long long)n * g.ldb + k]) : 0.f;
        }
        uint32_t p[3][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) split_pair(v[2 * j], v[2 * j + 1], p[0][j], p[1][j], p[2][j]);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
            *reinterpret_cast<uint4*>(out + ((size_t)(pl * 2 + h) * ncolp + n) * 16) = make_uint4(p[pl][0], p[pl][1], p[pl][2], p[pl][3]);
    }
}

// experiment switches (GMMVI_BG_DEBUG) exist only in -DBG_STAMPS builds: a runtime branch around a load or a hand-over changes
// what the compiler can prove about the loads in flight
#ifdef BG_STAMPS
#define BG_DBG(bit) (g.debug & (bit))
#else
#define BG_DBG(bit) 0
#endif
#ifdef BG_STAMPS
#define BG_CLK() __builtin_readcyclecounter()
#define BG_BARRIER_TIMED(acc_)                                 \
    do {                                                       \
        const unsigned long long b0__ = BG_CLK();              \
        BG_LDS_BARRIER();                                      \
        acc_ += BG_CLK() - b0__;                               \
    } while (0)
#else
#define BG_BARRIER_TIMED(acc_) BG_LDS_BARRIER()
#endif

// bytes of the LDS ring of bgemm_ws_kernel<NT, AK, .>
template <int NT, int AK>
constexpr int bg_ws_ring_bytes() {
    constexpr int BN = 32 * NT;
    constexpr int APL = AK ? BK * split_rowsp(BM) * 2 : 2 * (BM * 16 + 128), BPL = 2 * (BN * 16 + 128);
    return 3 * (3 * (APL + BPL) + 4096);
}

// one tile (bx, by, bzz) of the launch: both roles leave this function after 1 + total3 barriers
template <int NT, int AK, int PRO>
__device__ __forceinline__ void bgemm_ws_tile(const BG& g, const unsigned char* __restrict__ bimg, int ncolp, int nsteps,
                                              unsigned char* ring, const int bx, const int by, const int bzz) {
    constexpr int BN = 32 * NT;
#ifdef BG_STAMPS
    const unsigned long long st0 = BG_CLK();
    unsigned long long bwait = 0;
#endif
    constexpr int RSA = split_rowsp(BM);
    // fragment-order plane of a k-contiguous A: two k halves of [row][8 k] (+128 bytes between them: the two halves a
    // ds_write_b64 touches fall into different banks); B stage = the image slice, k halves BHS apart
    constexpr int AHS = BM * 16 + 128, BHS = BN * 16 + 128;
    constexpr int APL = AK ? BK * RSA * 2 : 2 * AHS, BPL = 2 * BHS;
    // bytes of one ring stage: three planes of each operand (+4 KB: where the staging threads put the chunks that do not
    // exist, so that their stores need no branch)
    constexpr int STG = 3 * (APL + BPL) + 4096;
    constexpr int NCB = (6 * BN + 255) / 256;               // 16-byte chunks of the B stage per staging thread
    static_assert(3 * STG == bg_ws_ring_bytes<NT, AK>(), "ring size");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = by * BM, n0 = bx * BN;
    const int nsplit = g.ksplit > 1 ? g.ksplit : 1;
    const int bz = bzz / nsplit, kz = bzz - bz * nsplit;
    int Mb = g.M;
    long long rowbase = 0;
    if (g.row_off) { rowbase = g.row_off[bz]; Mb = g.row_off[bz + 1] - (int)rowbase; }
    if (m0 >= Mb) return;
    int kb = 0, ke = g.Kd;                                  // kb: a multiple of 16 (the image is cut in 16-k steps from k = 0)
    if (g.tri == 1) ke = min(g.Kd, n0 + BN);
    else if (g.tri == 2) kb = min(g.Kd, n0) & ~15;
    if (nsplit > 1) {
        const int chunk = ((g.Kd + nsplit - 1) / nsplit + BK - 1) / BK * BK;
        kb = min(g.Kd, kz * chunk);
        ke = min(g.Kd, kb + chunk);
    }
    const int spb = (ke - kb + BK - 1) / BK;
    const int nb = g.inner > 0 ? min(g.inner, g.inner_total - bz * g.inner) : 1;
    const int total = nb * spb;
    const int total3 = (total + 2) / 3 * 3;            // barriers after the first one, both roles

    if (wave >= 4) {
        // ------------------------------------------------ staging waves ------------------------------------------------
        // (priority: the multiplying waves are the older ones and win the arbitration for the vector issue port otherwise)
        if (!BG_DBG(256)) __builtin_amdgcn_s_setprio(3);
        const int pt = tid - 256;
        const float* A0 = g.A + (AK ? rowbase : rowbase * g.lda);
        const float* pro = PRO == 1 ? g.a_sub : (PRO == 2 ? g.a_rscale : (PRO >= 3 ? g.a_kscale : nullptr));
        const long long s_pro = PRO == 1 ? g.s_asub : (PRO == 2 ? g.s_ars : (PRO >= 3 ? g.s_aks : 0));
        const bool vecR = PRO != 4 || (al16(g.a_rsub) && (g.s_arsub & 3) == 0);
        const bool vecA = al16(A0) && ((g.lda | g.sA) & 3) == 0;
        const bool vecP = PRO == 0 || (al16(pro) && (s_pro & 3) == 0);
        // A pieces as in bgemm_kernel; a_at: where a piece goes inside a plane (units of 8 bytes)
        int a_r[2], a_k[2], a_at[2];
        bool a_ok[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int idx = pt + 256 * u;
            if (AK) { a_k[u] = idx >> 5; a_r[u] = 4 * (idx & 31); } else { a_r[u] = idx >> 2; a_k[u] = 4 * (idx & 3); }
            a_ok[u] = m0 + a_r[u] < Mb;
            a_at[u] = AK ? (a_k[u] * RSA + a_r[u]) >> 2 : ((a_k[u] >> 3) * AHS + a_r[u] * 16 + ((a_k[u] >> 2) & 1) * 8) >> 3;
        }
        // B chunks: chunk q = (plane-and-half ph = q / BN, column c = q % BN): image offset and LDS offset, fixed for the launch
        unsigned b_go[NCB], b_lo[NCB];
        bool b_has[NCB];
#pragma unroll
        for (int u = 0; u < NCB; ++u) {
            const int q = pt + 256 * u;
            const int ph = q / BN, c = q - ph * BN;
            b_has[u] = q < 6 * BN;
            b_go[u] = b_has[u] ? ((unsigned)ph * ncolp + n0 + c) * 16u : 0u;
            b_lo[u] = b_has[u] ? (unsigned)(3 * APL + (ph >> 1) * BPL + (ph & 1) * BHS + c * 16) : (unsigned)(STG - 4096 + pt * 16);
        }
        const size_t img_step = bimg_step_bytes(ncolp);
        auto split_store_a = [&](unsigned char* sa, const float4* va) {
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                uint32_t lo[3], hi[3];
                split_pair(va[u].x, va[u].y, lo[0], lo[1], lo[2]);
                split_pair(va[u].z, va[u].w, hi[0], hi[1], hi[2]);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) reinterpret_cast<uint2*>(sa + pl * APL)[a_at[u]] = make_uint2(lo[pl], hi[pl]);
            }
        };
        // Fast route (decided once per workgroup): aligned A, every 16-byte piece entirely inside or entirely outside the
        // operand (k range and row range), byte offsets that fit 32 bits.  One straight-line load routine, no merge of
        // register values with another route: the loads of three steps stay in flight.
        const long long extA = AK ? (long long)g.Kd * g.lda : (long long)Mb * g.lda;
        const bool fast = vecA && vecP && vecR && (!AK || (Mb & 3) == 0 || m0 + BM <= Mb) && (AK || ((kb | ke) & 3) == 0) &&
                          extA < (1ll << 29);
        if (fast) {
            // byte offsets of the pieces from the operand's place at (batch, k = kb); pieces outside the row range read piece 0
            unsigned a_bo[2], a_b0[2], p_bo[2], r_bo[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                a_bo[u] = a_ok[u] ? 4u * (unsigned)(AK ? a_k[u] * g.lda + m0 + a_r[u] : (m0 + a_r[u]) * g.lda + a_k[u]) : 0u;
                a_b0[u] = a_ok[u] ? 4u * (unsigned)(AK ? m0 + a_r[u] : (m0 + a_r[u]) * g.lda) : 0u;    // the same piece at k = kb
                // prologue vector: along k (PRO 1, 3, 4) or along the rows (PRO 2); PRO 4: second vector along the rows
                p_bo[u] = PRO == 2 ? 4u * (unsigned)(a_ok[u] ? m0 + a_r[u] : 0) : 4u * (unsigned)a_k[u];
                r_bo[u] = 4u * (unsigned)(a_ok[u] ? m0 + a_r[u] : 0);
            }
            const unsigned a_kstep = 4u * (unsigned)(AK ? g.lda : 1);
            float4 ra[3][2], pv[3][2], pw[3][2];
            i32x4 rb[3][NCB];
            int klim[3] = {0, 0, 0};                 // ke - k0 of the step a register stage holds
            int ld_bi = 0, ld_ks = 0, ld_n = 0;      // (inner batch, k step, index) of the next step to load: steps are loaded in order
            const char* run_A = nullptr; const unsigned char* run_B = nullptr; const unsigned char* run_B0 = nullptr;
            const char* run_pb = nullptr; const char* run_pr = nullptr;
            auto set_batch = [&](long long b) {
                run_A = reinterpret_cast<const char*>(A0 + b * g.sA + (AK ? (long long)kb * g.lda : (long long)kb));
                run_B0 = bimg + ((size_t)(g.sB ? b : 0) * nsteps + (kb >> 4)) * img_step;
                run_B = run_B0;
                run_pb = PRO ? reinterpret_cast<const char*>(pro + b * s_pro + (PRO == 2 ? 0 : kb)) : nullptr;
                run_pr = PRO == 4 ? reinterpret_cast<const char*>(g.a_rsub + b * g.s_arsub) : nullptr;
            };
            set_batch((long long)bz * (g.inner > 0 ? g.inner : 1));
            auto gload = [&](auto rc) {
                constexpr int R = decltype(rc)::value;
                // (behind the last step the last step is loaded again and never handed over: every path through the loop
                // issues the same number of loads, which lets the compiler wait with vmcnt(two stages) instead of vmcnt(0))
                if (BG_DBG(4)) return;
                // running pointers: the places of this step's operands are those of the previous step + one k step; only a new
                // inner batch computes them from scratch (scalar work only, the same loads follow on both paths)
                const int k0 = kb + ld_ks * BK;
                const unsigned kofs = BG_DBG(128) ? 0u : (unsigned)(ld_ks * BK);
                klim[R] = ke - k0;
                const char* Ab = run_A;
                const unsigned char* Bi = BG_DBG(64) ? run_B0 : run_B;
                const char* pb = run_pb;
                const char* pr = run_pr;
                if (++ld_n < total) {
                    run_B += img_step;
                    if (++ld_ks == spb) {
                        ld_ks = 0;
                        ++ld_bi;
                        set_batch((long long)bz * (g.inner > 0 ? g.inner : 1) + ld_bi);
                    }
                }
                // a piece whose k lies behind ke reads the piece of its row at k = kb (inside the operand whatever the length of
                // the tile's k range: kb < ke), masked at the hand-over
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const unsigned at = a_k[u] < klim[R] ? a_bo[u] + kofs * a_kstep : a_b0[u];
                    ra[R][u] = *reinterpret_cast<const float4*>(Ab + at);
                }
#pragma unroll
                for (int u = 0; u < NCB; ++u) rb[R][u] = *reinterpret_cast<const i32x4*>(Bi + b_go[u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    if (PRO == 2) {
                        if (AK) pv[R][u] = *reinterpret_cast<const float4*>(pb + p_bo[u]);
                        else { const float sc = *reinterpret_cast<const float*>(pb + p_bo[u]); pv[R][u] = make_float4(sc, sc, sc, sc); }
                    } else if (PRO != 0) {
                        const unsigned ko = a_k[u] < klim[R] ? kofs : 0u;
                        if (AK) { const float sc = *reinterpret_cast<const float*>(pb + (p_bo[u] + 4u * ko)); pv[R][u] = make_float4(sc, sc, sc, sc); }
                        else pv[R][u] = *reinterpret_cast<const float4*>(pb + (p_bo[u] + 4u * ko));
                        if (PRO == 4) pw[R][u] = *reinterpret_cast<const float4*>(pr + r_bo[u]);
                    }
                }
            };
            auto sstore = [&](auto rc) {
                constexpr int R = decltype(rc)::value;
                unsigned char* stage = ring + R * STG;       // step s lives in register stage and ring stage s % 3
                float4 va[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    float4 v = ra[R][u];
                    if (PRO == 1) { v.x -= pv[R][u].x; v.y -= pv[R][u].y; v.z -= pv[R][u].z; v.w -= pv[R][u].w; }
                    if (PRO == 4) { v.x -= pw[R][u].x; v.y -= pw[R][u].y; v.z -= pw[R][u].z; v.w -= pw[R][u].w; }
                    if (PRO >= 2) { v.x *= pv[R][u].x; v.y *= pv[R][u].y; v.z *= pv[R][u].z; v.w *= pv[R][u].w; }
                    va[u] = (a_ok[u] && a_k[u] < klim[R]) ? v : make_float4(0.f, 0.f, 0.f, 0.f);
                }
                if (!BG_DBG(2)) split_store_a(stage, va);
#pragma unroll
                for (int u = 0; u < NCB; ++u)
                    if (!BG_DBG(8)) *reinterpret_cast<i32x4*>(ring + R * STG + b_lo[u]) = rb[R][u];
            };
            if (total > 0) {
                // (scheduling barriers: the loads must be ISSUED in step order -- the waits count loads issued later)
                gload(bg_ic<0>());
                __builtin_amdgcn_sched_barrier(0);
                gload(bg_ic<1>());
                __builtin_amdgcn_sched_barrier(0);
                gload(bg_ic<2>());
                __builtin_amdgcn_sched_barrier(0);
                sstore(bg_ic<0>());
                gload(bg_ic<0>());
                __builtin_amdgcn_sched_barrier(0);
                if (1 < total) sstore(bg_ic<1>());
                gload(bg_ic<1>());
                __builtin_amdgcn_sched_barrier(0);
            }
            BG_LDS_BARRIER();
            // during step t: fill ring stage (t + 2) % 3 with step t + 2, then load step t + 5 into the freed registers.  The loop
            // runs over total3 steps (total rounded up to a multiple of 3; the extra steps only meet the barrier) and has no
            // early exit: every path to a hand-over has issued the same loads in the same order
#ifdef BG_STAMPS
            const unsigned long long pst1 = BG_CLK();
#endif
#ifdef BG_STAMPS
            unsigned long long tss = 0, tgl = 0, c0_, c1_;
#define BG_T(acc_, stmt)  do { c0_ = BG_CLK(); stmt; c1_ = BG_CLK(); acc_ += c1_ - c0_; } while (0)
#else
#define BG_T(acc_, stmt)  do { stmt; } while (0)
#endif
            for (int t = 0; t < total3; t += 3) {
                BG_T(tss, if (t + 2 < total) sstore(bg_ic<2>()));
                BG_T(tgl, gload(bg_ic<2>()));
                BG_BARRIER_TIMED(bwait);
                BG_T(tss, if (t + 3 < total) sstore(bg_ic<0>()));
                BG_T(tgl, gload(bg_ic<0>()));
                BG_BARRIER_TIMED(bwait);
                BG_T(tss, if (t + 4 < total) sstore(bg_ic<1>()));
                BG_T(tgl, gload(bg_ic<1>()));
                BG_BARRIER_TIMED(bwait);
            }
#ifdef BG_STAMPS
            if ((g.debug & 32) && pt == 0 && blockIdx.x == 7 && bzz == 1) {
                const unsigned long long pst2 = BG_CLK();
                printf("stager  by=%d total=%d: start %llu prime %llu  loop %llu  per step: all %llu  hand-over %llu  loads %llu  barrier %llu\n", by, total,
                       st0 % 100000000ull, pst1 - st0, pst2 - pst1, (pst2 - pst1) / (unsigned long long)total3, tss / (unsigned long long)total3,
                       tgl / (unsigned long long)total3, bwait / (unsigned long long)total3);
            }
#endif
            return;
        }
        // General route (misaligned or ragged A): element-wise loads, one step at a time, same ring protocol
        auto stage_step = [&](int step) {
            const int bi = step / spb;
            const long long b = (long long)bz * (g.inner > 0 ? g.inner : 1) + bi;
            const int k0 = kb + (step - bi * spb) * BK;
            const float* Ab = A0 + b * g.sA;
            const unsigned char* Bi = bimg + ((size_t)(g.sB ? b : 0) * nsteps + (k0 >> 4)) * img_step;
            const float* pb = PRO ? pro + b * s_pro : nullptr;
            const float* pr = PRO == 4 ? g.a_rsub + b * g.s_arsub : nullptr;
            unsigned char* stage = ring + (step % 3) * STG;
            float4 va[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int gm = m0 + a_r[u], gk = k0 + a_k[u];
                float4 v;
                if (AK) {                                           // 4 consecutive rows of one k
                    const int nv = (gk < ke) ? Mb - gm : 0;
                    v = ld4(Ab + (long long)gk * g.lda + gm, nv, vecA);
                    if (nv > 0) {
                        if (PRO == 1) { const float sc = pb[gk]; v.x -= sc; v.y -= sc; v.z -= sc; v.w -= sc; }
                        if (PRO == 3) { const float sc = pb[gk]; v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
                        if (PRO == 2) { const float4 sc = ld4(pb + gm, nv, vecP); v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
                        if (PRO == 4) {
                            const float4 r4 = ld4(pr + gm, nv, vecR);
                            const float sc = pb[gk];
                            v.x = (v.x - r4.x) * sc; v.y = (v.y - r4.y) * sc; v.z = (v.z - r4.z) * sc; v.w = (v.w - r4.w) * sc;
                        }
                        if (nv < 4) { if (nv < 2) v.y = 0.f; if (nv < 3) v.z = 0.f; v.w = 0.f; }
                    }
                } else {                                            // 4 consecutive k of one row
                    const int nv = (gm < Mb) ? ke - gk : 0;
                    v = ld4(Ab + (long long)gm * g.lda + gk, nv, vecA);
                    if (nv > 0) {
                        if (PRO == 1) { const float4 sc = ld4(pb + gk, nv, vecP); v.x -= sc.x; v.y -= sc.y; v.z -= sc.z; v.w -= sc.w; }
                        if (PRO == 3) { const float4 sc = ld4(pb + gk, nv, vecP); v.x *= sc.x; v.y *= sc.y; v.z *= sc.z; v.w *= sc.w; }
                        if (PRO == 2) { const float sc = pb[gm]; v.x *= sc; v.y *= sc; v.z *= sc; v.w *= sc; }
                        if (nv < 4) { if (nv < 2) v.y = 0.f; if (nv < 3) v.z = 0.f; v.w = 0.f; }
                    }
                }
                va[u] = v;
            }
            split_store_a(stage, va);
#pragma unroll
            for (int u = 0; u < NCB; ++u)
                if (b_has[u]) *reinterpret_cast<i32x4*>(stage + b_lo[u]) = *reinterpret_cast<const i32x4*>(Bi + b_go[u]);
        };
        if (0 < total) stage_step(0);
        if (1 < total) stage_step(1);
        BG_LDS_BARRIER();
        for (int t = 0; t < total3; ++t) {
            if (t + 2 < total) stage_step(t + 2);
            BG_LDS_BARRIER();
        }
        return;
    }

    // ---------------------------------------------------- multiplying waves ----------------------------------------------------
    const int col = lane & 31, half = lane >> 5;
    // lane's place in a transposed read (k-major A): group lane / 16 covers operand rows 16 (group & 1) .., k 8 (group >> 1) ..;
    // lane 4 q + p of the group addresses k row q, rows 4 p .. 4 p + 3
    const int tr_k = 8 * (lane >> 5) + ((lane >> 2) & 3), tr_r = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const int a_rd = AK ? (tr_k * RSA + wave * 32 + tr_r) * 2 : half * AHS + (wave * 32 + col) * 16;
    const int b_rd = 3 * APL + half * BHS + col * 16;
    auto aload = [&](const unsigned char* stage, i32x4* dst) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) {
            if (AK) dst[pl] = lds_tr_frag(stage + pl * APL, a_rd, RSA * 2);
            else dst[pl] = *reinterpret_cast<const i32x4*>(stage + pl * APL + a_rd);
        }
    };
    auto bload = [&](const unsigned char* stage, int t, i32x4* dst) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) dst[pl] = *reinterpret_cast<const i32x4*>(stage + pl * BPL + b_rd + 512 * t);
    };
    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    // sub-tile t (columns n0 + 32 t ..) takes part in a step unless opB vanishes there (triangular operands) or the columns do
    // not exist: t_lo <= t < t_hi, from the step's k0
    const int t_end = min(NT, (g.N - n0 + 31) >> 5);
    BG_LDS_BARRIER();
#ifdef BG_STAMPS
    const unsigned long long st1 = BG_CLK();
#endif
    i32x4 af[3], bf[2][3], afn[3], bfn[3];
    if (total > 0) { aload(ring, af); bload(ring, 0, bf[0]); }
    int slot = 0, ks = 0;
    for (int step = 0; step < total; ++step) {
        const int k0 = kb + ks * BK;
        if (++ks == spb) ks = 0;
        const int t_lo = g.tri == 1 ? max(0, (k0 - n0) >> 5) : 0;                       // live iff k0 < n0 + 32 t + 32
        const int t_hi = g.tri == 2 ? min(t_end, (k0 + BK - n0 + 31) >> 5) : t_end;     // live iff k0 + 16 > n0 + 32 t
        const unsigned char* stage = ring + slot * STG;
        slot = slot == 2 ? 0 : slot + 1;
        const unsigned char* next = ring + slot * STG;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            // (fragments of a sub-tile that does not take part are not read: LDS bandwidth is what paces this role)
            if (t + 1 < NT) { if (t + 1 >= t_lo && t + 1 < t_hi) bload(stage, t + 1, bf[(t + 1) & 1]); }
            else if (step + 1 < total) { aload(next, afn); bload(next, 0, bfn); }
            if (t >= t_lo && t < t_hi && !BG_DBG(1)) {
                const i32x4* b = bf[t & 1];
                // smallest partial products first
                asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(af[2]), "v"(b[0]));
                asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(af[0]), "v"(b[2]));
                asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(af[1]), "v"(b[1]));
                asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(af[1]), "v"(b[0]));
                asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(af[0]), "v"(b[1]));
                asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(acc[t]) : "v"(af[0]), "v"(b[0]));
            }
        }
        BG_BARRIER_TIMED(bwait);
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) { af[pl] = afn[pl]; bf[0][pl] = bfn[pl]; }
    }
    for (int step = total; step < total3; ++step) BG_LDS_BARRIER();
#ifdef BG_STAMPS
    const unsigned long long st2 = BG_CLK();
#endif
    // the last MFMA must have retired before its accumulators are read (inline asm: no automatic hazard nops)
    asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
    if (g.rowsq != nullptr) {
        // lane (col, half) holds rows (r & 3) + 8 (r >> 2) + 4 half of its column in every sub-tile: square-sum over the
        // sub-tiles, then over the 32 lanes of the half on the DPP network (four steps inside a row of 16, two v_readlane
        // per half); lane i of the wave collects the sum of row i: one 128-byte store
        float mine = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float v = 0.f;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const float z = g.alpha * acc[t][r];
                if (n0 + 32 * t + col < g.N) v = fmaf(z, z, v);
            }
            v += gmmvi_dpp<0xB1>(v);
            v += gmmvi_dpp<0x4E>(v);
            v += gmmvi_dpp<0x141>(v);
            v += gmmvi_dpp<0x140>(v);
            const float s0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0)) +
                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
            const float s1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32)) +
                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
            const int i0 = (r & 3) + 8 * (r >> 2);
            mine = lane == i0 ? s0 : (lane == i0 + 4 ? s1 : mine);
        }
        float* rq = g.rowsq + (long long)bx * g.rs_tile + (long long)bzz * g.rs_batch + rowbase;
        const int i = m0 + wave * 32 + lane;
        if (lane < 32 && i < Mb) rq[i] = mine;
    }
    if (g.no_store) return;
    float* Cb = g.C + (long long)bzz * g.sC + rowbase * g.ldc;
    const float* bias = g.c_bias ? g.c_bias + (long long)bz * g.s_cb : nullptr;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int j = n0 + 32 * t + col;
        if (j >= g.N) continue;
        const float bj = bias ? bias[j] : 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int i = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (i < Mb) {
                float* p = Cb + (long long)i * g.ldc + j;
                float v = fmaf(g.alpha, acc[t][r], bj);
                if (g.accumulate) v += *p;
                *p = v;
            }
        }
    }
#ifdef BG_STAMPS
    if ((g.debug & 32) && tid == 0 && blockIdx.x == 7 && bzz == 1) {
        const unsigned long long st3 = BG_CLK();
        printf("multipl by=%d total=%d: start %llu  +prime %llu  +loop %llu (barrier %llu)  +epilogue %llu\n", by, total, st0 % 100000000ull, st1 - st0,
               st2 - st1, bwait, st3 - st2);
    }
#endif
}

// Persistent launch: one workgroup per CU walks over the tiles (row tile fastest, then column tile, then batch / k-split slab).
// The stagers leave a tile before the multipliers (which still write their results) and start loading the next one: the
// dispatch gap between two workgroups of a 150 KB-LDS kernel and the first loads of a tile are no longer exposed
// (measured per tile of the whitening launch before: 49 k cycles in the step loop, 36 k around it).
template <int NT, int AK, int PRO>
__global__ __launch_bounds__(512, 1) void bgemm_ws_kernel(BG g, const unsigned char* __restrict__ bimg, int ncolp, int nsteps,
                                                          int ntx, int nty, int ntz) {
    __shared__ __align__(16) unsigned char ring[bg_ws_ring_bytes<NT, AK>()];
    const int G = gridDim.x;
    const int ntiles = ntx * nty * ntz;
    for (int tile = blockIdx.x; tile < ntiles; tile += G) {
        const int by = tile % nty, rest = tile / nty;
        const int bx = rest % ntx, bzz = rest / ntx;
        bgemm_ws_tile<NT, AK, PRO>(g, bimg, ncolp, nsteps, ring, bx, by, bzz);
    }
}

// GMMVI_BLOCKED_F32=1 keeps every contraction on the f32 matrix-core instruction (v_mfma_f32_32x32x2_f32); the default is
// the split-operand route above
bool bgemm_split_enabled() {
    static const bool off = getenv("GMMVI_BLOCKED_F32") != nullptr && atoi(getenv("GMMVI_BLOCKED_F32")) != 0;
    return !off;
}

// tile widths of the two routes: f32 route 32 x {3, 4, 5}, split route 32 x {3, 4, 5, 6, 8, 10}: the least padded total width,
// ties go to the wider tile.  -> NT, *tiles = number of column tiles
int bgemm_tile_width(int n, bool split, int* tiles) {
    static const int f32_nt[] = {5, 4, 3}, split_nt[] = {10, 8, 6, 5, 4, 3};
    const int* cand = split ? split_nt : f32_nt;
    const int nc = split ? 6 : 3;
    int nt = cand[0], best = 1 << 30;
    for (int i = 0; i < nc; ++i) {
        const int w = (n + 32 * cand[i] - 1) / (32 * cand[i]) * 32 * cand[i];
        if (w < best) { best = w; nt = cand[i]; }
    }
    *tiles = best / (32 * nt);
    return nt;
}

int bimg_reserve(gmmvi_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->bimg_bytes) return GMMVI_OK;
    GMMVI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->bimg) GMMVI_HIP_CHECK(ctx, hipFree(ctx->bimg));
    ctx->bimg = nullptr;
    ctx->bimg_bytes = 0;
    const size_t want = bytes + bytes / 4;
    GMMVI_HIP_CHECK(ctx, hipMalloc(&ctx->bimg, want));
    ctx->bimg_bytes = want;
    return GMMVI_OK;
}

template <int AK, int BKM, int PRO>
int bgemm_launch(gmmvi_ctx* ctx, const BG& g0, int batches_outer) {
    const bool split = gmmvi_bgemm_use_split(g0.N, g0.Kd);
    int tiles = 1;
    const int nt = bgemm_tile_width(g0.N, split, &tiles);
    dim3 grid(tiles, (g0.M + BM - 1) / BM, batches_outer * (g0.ksplit > 1 ? g0.ksplit : 1));
    if (!split) {
        switch (nt) {
            case 3: hipLaunchKernelGGL((bgemm_kernel<3, AK, BKM, PRO>), grid, dim3(256), 0, ctx->stream, g0); break;
            case 4: hipLaunchKernelGGL((bgemm_kernel<4, AK, BKM, PRO>), grid, dim3(256), 0, ctx->stream, g0); break;
            default: hipLaunchKernelGGL((bgemm_kernel<5, AK, BKM, PRO>), grid, dim3(256), 0, ctx->stream, g0); break;
        }
        GMMVI_LAUNCH_CHECK(ctx);
        return GMMVI_OK;
    }
    BG g = g0;
#ifdef BG_STAMPS
    static const int dbg = getenv("GMMVI_BG_DEBUG") ? atoi(getenv("GMMVI_BG_DEBUG")) : 0;
    g.debug = dbg;
#endif
    // the B image: every batch of B (one if B is shared: sB == 0), every 16-k step of [0, Kd)
    const int ncolp = tiles * nt * 32, nsteps = (g.Kd + BK - 1) / BK;
    const long long nbatch = g.sB ? (g.inner > 0 ? (long long)g.inner_total : (long long)batches_outer) : 1;
    const size_t bytes = (size_t)nbatch * nsteps * bimg_step_bytes(ncolp);
    int rc = bimg_reserve(ctx, bytes);
    if (rc != GMMVI_OK) return rc;
    unsigned char* img = static_cast<unsigned char*>(ctx->bimg);
    hipLaunchKernelGGL(bsplit_image_kernel, dim3(nsteps, (unsigned)nbatch), dim3(256), 0, ctx->stream, g, ncolp, nsteps, img);
    GMMVI_LAUNCH_CHECK(ctx);
    const int ntiles = (int)(grid.x * grid.y * grid.z);
    int cap = ctx->num_cus;
#ifdef BG_STAMPS
    static const int env_grid = getenv("GMMVI_BG_GRID") ? atoi(getenv("GMMVI_BG_GRID")) : 0;      // experiments: fewer workgroups than CUs
    if (env_grid > 0) cap = env_grid;
#endif
    const dim3 pgrid(ntiles < cap ? ntiles : cap);
#define BG_WS_LAUNCH(NT_) hipLaunchKernelGGL((bgemm_ws_kernel<NT_, AK, PRO>), pgrid, dim3(512), 0, ctx->stream, g, img, ncolp, nsteps, \
                                             (int)grid.x, (int)grid.y, (int)grid.z)
    switch (nt) {
        case 3: BG_WS_LAUNCH(3); break;
        case 4: BG_WS_LAUNCH(4); break;
        case 5: BG_WS_LAUNCH(5); break;
        case 6: BG_WS_LAUNCH(6); break;
        case 8: BG_WS_LAUNCH(8); break;
        default: BG_WS_LAUNCH(10); break;
    }
#undef BG_WS_LAUNCH
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

}  // namespace

// Route of one launch.  The split route pays a pre-pass over B and runs one 512-thread workgroup per CU: measured at K = 64,
// N = 19 968 (tools/time_blocked.py, whitening / whitening + gradient / Stein, us): D = 64: 269 / 609 / 348 against the f32
// route's 188 / 446 / 442; D = 128: 415 / 1132 / 842 against 387 / 987 / 1266; D = 192: 644 / 1649 / 1057 against 950 / 2114 /
// 1731 -- it wins from 160 result columns on, and for long contractions (the Stein sums over the samples) at every width.
bool gmmvi_bgemm_use_split(int n, int kd) { return bgemm_split_enabled() && (n >= 160 || kd >= 512); }

// number of column tiles bgemm_launch will use for a result of n columns
int gmmvi_bgemm_col_tiles(int n, int kd) {
    int tiles = 1;
    (void)bgemm_tile_width(n, gmmvi_bgemm_use_split(n, kd), &tiles);
    return tiles;
}

// the operand layouts / prologues the callers use
int gmmvi_bgemm(gmmvi_ctx* ctx, const BG& g, int batches_outer) {
    if (g.M <= 0 || g.N <= 0 || batches_outer <= 0) return GMMVI_OK;
    const int pro = g.a_sub ? 1 : (g.a_rscale ? 2 : (g.a_kscale ? (g.a_rsub ? 4 : 3) : 0));
    const int key = g.a_kmajor * 100 + g.b_kmajor * 10 + pro;
    switch (key) {
        case 1: return bgemm_launch<0, 0, 1>(ctx, g, batches_outer);      // whitening: (X - mu) L^-T
        case 0: return bgemm_launch<0, 0, 0>(ctx, g, batches_outer);      // sampling: eps L^T
        case 12: return bgemm_launch<0, 1, 2>(ctx, g, batches_outer);     // gradient: (r Z) L^-1
        case 10: return bgemm_launch<0, 1, 0>(ctx, g, batches_outer);     // A L^-1, R L
        case 114: return bgemm_launch<1, 1, 4>(ctx, g, batches_outer);    // Stein: (X1 - mu1)^T diag(e) G1
        case 100: return bgemm_launch<1, 0, 0>(ctx, g, batches_outer);    // C^T L^-T
        case 110: return bgemm_launch<1, 1, 0>(ctx, g, batches_outer);    // L^T (R L)
        default: return gmmvi_fail(ctx, GMMVI_ERR_ARG, "bgemm: operand layout not instantiated");
    }
}
