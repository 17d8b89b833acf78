// Bayesian-neural-network classification target (target_distributions/bnn.py: BNN_LNPDF with BNN_MNIST's network, ReLU
// hidden layer, linear logits, sparse categorical cross-entropy from logits) and its analytic gradient.
//
// Network F -> H (ReLU) -> C (logits); the parameter vector of a sample is the reference's layout: W1 [F, H] row-major,
// b1 [H], W2 [H, C] row-major, b2 [C], so D = F H + H + H C + C.  For sample n and the rows m of its minibatch
//     z1 = x_m W1 + b1,  h = max(z1, 0),  l = h W2 + b2,  CE_m = logsumexp(l) - l[y_m]
//     lp[n]   = s (-(T / B) sum_m CE_m - 0.5 sum_d w_d^2 / sd^2)
//     grad[n] = d lp[n] / d w_n                 (ReLU derivative 1 where z1 > 0, else 0)
// The minibatch rows are bnn.hip's stream (feistel.h, stream id 3): position p = n B + j, epoch p div T, rank p mod T.
//
// Mapping: one workgroup (4 waves) per sample, 128 batch rows per chunk (B > 128 loops over chunks).  b1 is row F of an
// extended W1 (it follows W1 in the parameter vector) and every valid batch row carries x_F = 1, so the bias and its
// gradient ride in the two big contractions.  Both run on v_mfma_f32_16x16x4_f32 (exact f32):
//   forward   Z^T[j][m] = sum_f W1[f][j] X[m][f]:  F is walked in tiles of 32; the gathered rows and the W1 tile are staged
//             in LDS (the next tile's global loads are in flight during the products).  Wave w owns the rows 32 w .. 32 w + 31
//             and every hidden unit, 2 x 8 accumulator tiles.  A operand: lane l -> W1s[4 s + (l >> 4)][16 jt + (l & 15)],
//             B operand: Xs[16 mt + (l & 15)][4 s + (l >> 4)], D lane l, register r -> Z^T[16 jt + 4 (l >> 4) + r][16 mt + (l & 15)].
//   epilogue  the batch row sits on the lane, so logits, softmax, the loss and d lp / d l stay in registers (one sum over
//             the four 16-lane groups); dZ1 = (dl W2^T) [z1 > 0] replaces the accumulators.  h and dl go to LDS for
//             dW2[j][c] = sum_m h[m][j] dl[m][c] (lane = j, rows in order), then dZ1 overwrites h.
//   backward  dW1[f][j] = sum_m X[m][f] dZ1[m][j]: a second walk over the gathered rows, 32 features per tile; wave w owns
//             the hidden units 32 w .. 32 w + 31.  The tile goes straight to the sample's gradient row; a later chunk adds
//             to what the same lane wrote before.
// Every gradient entry is owned by one lane, every sum has a fixed order and there are no atomics: bitwise reproducible
// for a given (seed, call); the log density takes the same path with and without the gradient.
// Rows past the batch are all-zero (x_F = 0 too), their dl is zero and their loss is masked; columns past H or C are zero
// in LDS.  A label outside [0, C) selects no logit (it is compared, never used as an index).
#include "common.h"
#include "feistel.h"
#include "wave_reduce.h"

namespace {
typedef float bc_f32x4 __attribute__((ext_vector_type(4)));
constexpr int BC_THREADS = 256;
constexpr int BC_CHUNK = 128;                      // batch rows per chunk
constexpr int BC_KT = 32;                          // features per tile
constexpr int BC_HP = 128, BC_CP = 16;             // padded hidden units, classes
constexpr int BC_FMAX = 1024, BC_BMAX = 1024;
constexpr int BC_LDX = BC_KT + 2;                  // forward X tile [128][34]: 2 i + k hits 32 distinct banks per half wave
constexpr int BC_LDW = BC_HP + 16;                 // W1 tile [32][144], h / dZ1 [128][144]: 16 k + i likewise
constexpr int BC_LDXB = BC_KT + 16;                // backward X tile [128][48]
constexpr int BC_STAGE = BC_CHUNK * BC_LDX + BC_KT * BC_LDW;       // >= BC_CHUNK * BC_LDXB
static_assert(BC_STAGE >= BC_CHUNK * BC_LDXB, "the backward tile overlays the forward tiles");

// LDS of the predict kernel: W2s [128][16] | b2s [16] | rows [128] | stage; the target kernel adds labels [128] | dl [128][16]
// | CE [128] | red [8] | h / dZ1 [128][144]
constexpr int BC_PREDICT_FLOATS = BC_HP * BC_CP + BC_CP + BC_CHUNK + BC_STAGE;
constexpr int BC_TARGET_FLOATS = BC_PREDICT_FLOATS + BC_CHUNK + BC_CHUNK * BC_CP + BC_CHUNK + 8 + BC_CHUNK * BC_LDW;

// the 16 elements of a 128 x 32 tile of gathered rows that thread t stages: row (t >> 5) + 8 q, column t & 31
__device__ __forceinline__ void bc_load_x(const float* __restrict__ X, int F, int f0, const int (&rowq)[16], int t,
                                          float (&xr)[16]) {
    const int f = f0 + (t & 31);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        float v = 0.f;
        if (rowq[q] >= 0) {
            if (f < F) v = X[(size_t)rowq[q] * F + f];
            else if (f == F) v = 1.f;                                  // the bias column
        }
        xr[q] = v;
    }
}

__device__ __forceinline__ void bc_store_x(float* __restrict__ Xs, int ld, int t, const float (&xr)[16]) {
#pragma unroll
    for (int q = 0; q < 16; ++q) Xs[((t >> 5) + 8 * q) * ld + (t & 31)] = xr[q];
}

// the 16 elements of a 32 x 128 tile of the extended W1 [F + 1][H] that thread t stages: row (t >> 7) + 2 q, column t & 127
__device__ __forceinline__ void bc_load_w(const float* __restrict__ Wn, int F, int H, int f0, int t, float (&wr)[16]) {
    const int j = t & 127;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int f = f0 + (t >> 7) + 2 * q;
        wr[q] = (f <= F && j < H) ? Wn[(size_t)f * H + j] : 0.f;
    }
}

// Z^T = W1ext^T X^T of the chunk whose data rows are rowq (per thread, -1: none); acc[mt][jt] as described above.
// wsq (first chunk of the target kernel): adds the squares of the W1ext entries this thread stages, each entry once.
__device__ __forceinline__ void bc_forward(int F, int H, const float* __restrict__ X, const float* __restrict__ Wn,
                                           const int (&rowq)[16], float* __restrict__ Xs, float* __restrict__ W1s,
                                           bc_f32x4 (&acc)[2][8], float* wsq) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kq = lane >> 4;
    const int NT = (H + 15) >> 4, FE = F + 1;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) acc[mt][jt] = bc_f32x4{0.f, 0.f, 0.f, 0.f};
    float xr[16], wr[16];
    bc_load_x(X, F, 0, rowq, t, xr);
    bc_load_w(Wn, F, H, 0, t, wr);
    for (int f0 = 0; f0 < FE; f0 += BC_KT) {
        __syncthreads();                                               // the previous tile's products have read the stage
        bc_store_x(Xs, BC_LDX, t, xr);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            W1s[((t >> 7) + 2 * q) * BC_LDW + (t & 127)] = wr[q];
            if (wsq) *wsq = fmaf(wr[q], wr[q], *wsq);
        }
        __syncthreads();
        if (f0 + BC_KT < FE) {
            bc_load_x(X, F, f0 + BC_KT, rowq, t, xr);
            bc_load_w(Wn, F, H, f0 + BC_KT, t, wr);
        }
        const int ks = min(BC_KT, FE - f0 + 3) >> 2;                   // 4-feature steps that hold a feature
        for (int s = 0; s < ks; ++s) {
            float xb[2], wa[8];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) xb[mt] = Xs[(32 * wave + 16 * mt + i16) * BC_LDX + 4 * s + kq];
#pragma unroll
            for (int jt = 0; jt < 8; ++jt)
                if (jt < NT) wa[jt] = W1s[(4 * s + kq) * BC_LDW + 16 * jt + i16];
#pragma unroll
            for (int jt = 0; jt < 8; ++jt) {
                if (jt < NT) {
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        acc[mt][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[jt], xb[mt], acc[mt][jt], 0, 0, 0);
                }
            }
        }
    }
}

// the W2 row [16] of hidden unit j
__device__ __forceinline__ void bc_w2_row(const float* __restrict__ W2s, int j, float (&w2)[BC_CP]) {
    const bc_f32x4* p = (const bc_f32x4*)(W2s + j * BC_CP);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const bc_f32x4 x = p[v];
        w2[4 * v] = x[0]; w2[4 * v + 1] = x[1]; w2[4 * v + 2] = x[2]; w2[4 * v + 3] = x[3];
    }
}

// logits[mt][c] of the lane's two batch rows (without b2): the lane's hidden units, then the four 16-lane groups
__device__ __forceinline__ void bc_logits(int H, const bc_f32x4 (&acc)[2][8], const float* __restrict__ W2s,
                                          float (&part)[2][BC_CP]) {
    const int kq = (threadIdx.x & 63) >> 4, NT = (H + 15) >> 4;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int c = 0; c < BC_CP; ++c) part[mt][c] = 0.f;
#pragma unroll
    for (int jt = 0; jt < 8; ++jt) {
        if (jt < NT) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float w2[BC_CP];
                bc_w2_row(W2s, 16 * jt + 4 * kq + r, w2);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const float hv = fmaxf(acc[mt][jt][r], 0.f);
#pragma unroll
                    for (int c = 0; c < BC_CP; ++c) part[mt][c] = fmaf(hv, w2[c], part[mt][c]);
                }
            }
        }
    }
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int c = 0; c < BC_CP; ++c) {
            float v = part[mt][c];
            v += __shfl_xor(v, 16);
            v += __shfl_xor(v, 32);
            part[mt][c] = v;
        }
}

// W2 and b2 of one weight vector, zero padded to [128][16] and [16]; wsq (optional) takes their squares
__device__ __forceinline__ void bc_stage_w2(int F, int H, int C, const float* __restrict__ Wn, float* __restrict__ W2s,
                                            float* __restrict__ b2s, float* wsq) {
    const int t = threadIdx.x;
    const size_t oW2 = (size_t)(F + 1) * H, ob2 = oW2 + (size_t)H * C;
    for (int idx = t; idx < BC_HP * BC_CP; idx += BC_THREADS) {
        const int j = idx >> 4, c = idx & 15;
        const float v = (j < H && c < C) ? Wn[oW2 + (size_t)j * C + c] : 0.f;
        W2s[idx] = v;
        if (wsq) *wsq = fmaf(v, v, *wsq);
    }
    if (t < BC_CP) {
        const float v = t < C ? Wn[ob2 + t] : 0.f;
        b2s[t] = v;
        if (wsq) *wsq = fmaf(v, v, *wsq);
    }
}
}  // namespace

__global__ __launch_bounds__(BC_THREADS) void bnn_classifier_target_kernel(
    int F, int H, int C, int T, const float* __restrict__ X, const int32_t* __restrict__ labels, uint32_t k0, uint32_t k1,
    uint32_t call, uint32_t hbits, int B, float scaling, float inv_var, const float* __restrict__ W, int N,
    float* __restrict__ lp, float* __restrict__ grad) {
    extern __shared__ float bc_smem[];
    float* W2s = bc_smem;                                              // [128][16]
    float* b2s = W2s + BC_HP * BC_CP;                                  // [16]
    int* rows_s = (int*)(b2s + BC_CP);                                 // [128] data rows of the chunk, -1 past the batch
    float* Xs = (float*)(rows_s + BC_CHUNK);                           // stage: forward [128][34] | [32][144], backward [128][48]
    float* W1s = Xs + BC_CHUNK * BC_LDX;
    int* lab_s = (int*)(Xs + BC_STAGE);                                // [128]
    float* DLs = (float*)(lab_s + BC_CHUNK);                           // [128][16] d lp / d logits
    float* CEs = DLs + BC_CHUNK * BC_CP;                               // [128]
    float* red = CEs + BC_CHUNK;                                       // [8]
    float* Hs = red + 8;                                               // [128][144] h, then dZ1
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kq = lane >> 4, n = blockIdx.x;
    const int NT = (H + 15) >> 4, FE = F + 1;
    const size_t oW2 = (size_t)FE * H, ob2 = oW2 + (size_t)H * C, D = ob2 + C;
    const float* Wn = W + (size_t)n * D;
    float* gn = grad ? grad + (size_t)n * D : nullptr;
    float wsq = 0.f;
    bc_stage_w2(F, H, C, Wn, W2s, b2s, &wsq);

    const float coef = -(float)T / (float)B;                           // d(-(T/B) sum CE) / d CE
    const gmmvi_bnn_stream_origin origin = gmmvi_bnn_stream_origin_of(n, B, T);
    const int j2 = t & 127, ch = t >> 7;                               // dW2: hidden unit j2, classes 8 ch .. 8 ch + 7
    float a2[8], sdl[8], ce_acc = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) { a2[q] = 0.f; sdl[q] = 0.f; }

    for (int c0 = 0; c0 < B; c0 += BC_CHUNK) {
        const int rows = min(BC_CHUNK, B - c0);
        if (t < BC_CHUNK) {
            int row = -1, lab = -1;
            if (t < rows) {
                row = (int)gmmvi_bnn_stream_row(origin, c0 + t, T, call, hbits, k0, k1);
                lab = labels[row];
            }
            rows_s[t] = row;
            lab_s[t] = lab;
        }
        __syncthreads();                                               // also orders the W2s staging before its first read
        int rowq[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) rowq[q] = rows_s[(t >> 5) + 8 * q];
        bc_f32x4 acc[2][8];
        bc_forward(F, H, X, Wn, rowq, Xs, W1s, acc, c0 == 0 ? &wsq : nullptr);

        // ---- logits, loss and d lp / d logits of the lane's two rows ------------------------------------------------
        float part[2][BC_CP];
        bc_logits(H, acc, W2s, part);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = 32 * wave + 16 * mt + i16;
            const int y = lab_s[m];
            const bool valid = rows_s[m] >= 0;
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < BC_CP; ++c) {
                part[mt][c] += b2s[c];
                if (c < C) mx = fmaxf(mx, part[mt][c]);
            }
            float se = 0.f, ly = 0.f;
#pragma unroll
            for (int c = 0; c < BC_CP; ++c) {
                if (c < C) se += expf(part[mt][c] - mx);
                if (c == y) ly = part[mt][c];
            }
            const float lse = mx + logf(se);
#pragma unroll
            for (int c = 0; c < BC_CP; ++c) {
                const float p = expf(part[mt][c] - lse) - (c == y ? 1.f : 0.f);
                part[mt][c] = (valid && c < C) ? coef * p : 0.f;
            }
            if (kq == 0) {
                CEs[m] = valid ? lse - ly : 0.f;
                if (grad) {
#pragma unroll
                    for (int v = 0; v < 4; ++v)
                        ((bc_f32x4*)(DLs + m * BC_CP))[v] =
                            bc_f32x4{part[mt][4 * v], part[mt][4 * v + 1], part[mt][4 * v + 2], part[mt][4 * v + 3]};
                }
            }
        }
        if (grad) {
            // h -> LDS; dZ1 = (dl W2^T) [z1 > 0] -> the accumulators
#pragma unroll
            for (int jt = 0; jt < 8; ++jt) {
                if (jt < NT) {
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt) {
                        const bc_f32x4 z = acc[mt][jt];
                        *(bc_f32x4*)(Hs + (32 * wave + 16 * mt + i16) * BC_LDW + 16 * jt + 4 * kq) =
                            bc_f32x4{fmaxf(z[0], 0.f), fmaxf(z[1], 0.f), fmaxf(z[2], 0.f), fmaxf(z[3], 0.f)};
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float w2[BC_CP];
                        bc_w2_row(W2s, 16 * jt + 4 * kq + r, w2);
#pragma unroll
                        for (int mt = 0; mt < 2; ++mt) {
                            float dh = 0.f;
#pragma unroll
                            for (int c = 0; c < BC_CP; ++c) dh = fmaf(part[mt][c], w2[c], dh);
                            acc[mt][jt][r] = acc[mt][jt][r] > 0.f ? dh : 0.f;
                        }
                    }
                }
            }
        }
        __syncthreads();
        if (wave == 0) ce_acc += gmmvi_wave_sum(CEs[lane] + CEs[lane + 64]);
        if (grad) {
            // dW2[j][c] += sum_m h[m][j] dl[m][c], db2[c] += sum_m dl[m][c], rows in order
            if (j2 < 16 * NT) {
                for (int m = 0; m < rows; ++m) {
                    const float hv = Hs[m * BC_LDW + j2];
                    const bc_f32x4 d0 = *(const bc_f32x4*)(DLs + m * BC_CP + 8 * ch);
                    const bc_f32x4 d1 = *(const bc_f32x4*)(DLs + m * BC_CP + 8 * ch + 4);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        a2[q] = fmaf(hv, d0[q], a2[q]);
                        a2[q + 4] = fmaf(hv, d1[q], a2[q + 4]);
                        sdl[q] += d0[q];
                        sdl[q + 4] += d1[q];
                    }
                }
            }
            __syncthreads();                                           // h has been read: dZ1 takes its place
#pragma unroll
            for (int jt = 0; jt < 8; ++jt) {
                if (jt < NT) {
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
                        *(bc_f32x4*)(Hs + (32 * wave + 16 * mt + i16) * BC_LDW + 16 * jt + 4 * kq) = acc[mt][jt];
                }
            }
            // ---- dW1ext[f][j] = sum_m X[m][f] dZ1[m][j], written to the gradient row tile by tile --------------------
            float* Xb = Xs;                                            // [128][48]
            const int ksb = (rows + 3) >> 2;                           // rows past the batch are zero on both sides
            const bool owns = 32 * wave < H;                           // this wave's hidden units 32 wave .. 32 wave + 31
            float xr[16];
            bc_load_x(X, F, 0, rowq, t, xr);
            for (int f0 = 0; f0 < FE; f0 += BC_KT) {
                __syncthreads();                                       // dZ1 is written; the previous tile has been read
                bc_store_x(Xb, BC_LDXB, t, xr);
                __syncthreads();
                if (f0 + BC_KT < FE) bc_load_x(X, F, f0 + BC_KT, rowq, t, xr);
                if (owns) {
                    bc_f32x4 g[2][2];
#pragma unroll
                    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                        for (int u = 0; u < 2; ++u) g[ft][u] = bc_f32x4{0.f, 0.f, 0.f, 0.f};
                    for (int s = 0; s < ksb; ++s) {
                        float xa[2], db[2];
#pragma unroll
                        for (int ft = 0; ft < 2; ++ft) xa[ft] = Xb[(4 * s + kq) * BC_LDXB + 16 * ft + i16];
#pragma unroll
                        for (int u = 0; u < 2; ++u) db[u] = Hs[(4 * s + kq) * BC_LDW + 32 * wave + 16 * u + i16];
#pragma unroll
                        for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                            for (int u = 0; u < 2; ++u)
                                g[ft][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[ft], db[u], g[ft][u], 0, 0, 0);
                    }
                    // g[ft][u]: lane l, register r -> dW1ext[f0 + 16 ft + 4 (l >> 4) + r][32 wave + 16 u + (l & 15)]
#pragma unroll
                    for (int ft = 0; ft < 2; ++ft)
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const int j = 32 * wave + 16 * u + i16;
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                const int f = f0 + 16 * ft + 4 * kq + r;
                                if (f < FE && j < H) {
                                    const size_t e = (size_t)f * H + j;
                                    gn[e] = c0 == 0 ? scaling * (g[ft][u][r] - Wn[e] * inv_var)
                                                    : fmaf(scaling, g[ft][u][r], gn[e]);
                                }
                            }
                        }
                }
            }
        }
        __syncthreads();                                               // rows_s, the stage and Hs are rewritten by the next chunk
    }

    if (grad) {
        if (j2 < H) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = 8 * ch + q;
                if (c < C) gn[oW2 + (size_t)j2 * C + c] = scaling * (a2[q] - W2s[j2 * BC_CP + c] * inv_var);
            }
        }
        if (j2 == 0) {
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int c = 8 * ch + q;
                if (c < C) gn[ob2 + c] = scaling * (sdl[q] - b2s[c] * inv_var);
            }
        }
    }
    // lp: -(T/B) sum CE - 0.5 sum_d w_d^2 / sd^2, summed over the workgroup in fixed order
    const float ws = gmmvi_wave_sum(wsq);
    if (lane == 0) red[wave] = ws;
    __syncthreads();
    if (t == 0) {
        const float tot = (red[0] + red[1]) + (red[2] + red[3]);
        lp[n] = scaling * fmaf(coef, ce_acc, -0.5f * inv_var * tot);
    }
}

__global__ __launch_bounds__(BC_THREADS) void bnn_classifier_predict_kernel(int F, int H, int C, const float* __restrict__ W,
                                                                            const float* __restrict__ X, int M,
                                                                            float* __restrict__ out) {
    extern __shared__ float bc_smem[];
    float* W2s = bc_smem;
    float* b2s = W2s + BC_HP * BC_CP;
    int* rows_s = (int*)(b2s + BC_CP);
    float* Xs = (float*)(rows_s + BC_CHUNK);
    float* W1s = Xs + BC_CHUNK * BC_LDX;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kq = lane >> 4;
    const int s = blockIdx.y, m0 = blockIdx.x * BC_CHUNK;
    const size_t D = (size_t)(F + 1) * H + (size_t)H * C + C;
    const float* Wn = W + (size_t)s * D;
    bc_stage_w2(F, H, C, Wn, W2s, b2s, nullptr);
    if (t < BC_CHUNK) rows_s[t] = m0 + t < M ? m0 + t : -1;
    __syncthreads();
    int rowq[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) rowq[q] = rows_s[(t >> 5) + 8 * q];
    bc_f32x4 acc[2][8];
    bc_forward(F, H, X, Wn, rowq, Xs, W1s, acc, nullptr);
    float part[2][BC_CP];
    bc_logits(H, acc, W2s, part);
    if (kq == 0) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int m = m0 + 32 * wave + 16 * mt + i16;
            if (m < M) {
#pragma unroll
                for (int c = 0; c < BC_CP; ++c)
                    if (c < C) out[((size_t)s * M + m) * C + c] = part[mt][c] + b2s[c];
            }
        }
    }
}

namespace {
bool bc_shape_ok(int F, int H, int C) { return F >= 1 && F <= BC_FMAX && H >= 1 && H <= BC_HP && C >= 2 && C <= BC_CP; }

// the kernel's dynamic LDS lies above the 64 KB default
int bc_lds_attr(gmmvi_ctx* ctx) {
    return gmmvi_ensure_dynamic_lds(ctx, (const void*)bnn_classifier_target_kernel, BC_TARGET_FLOATS * sizeof(float));
}
}  // namespace

extern "C" int gmmvi_target_bnn_classifier(gmmvi_ctx* ctx, int F, int H, int C, int T, const float* X_dev,
                                           const int32_t* labels_dev, uint64_t seed, uint32_t call, int B,
                                           float likelihood_scaling, float prior_std, const float* W_dev, int N,
                                           float* lp_out_dev, float* grad_out_dev) {
    GMMVI_ARG_CHECK(ctx, bc_shape_ok(F, H, C));
    GMMVI_ARG_CHECK(ctx, T >= 1 && B >= 1 && B <= T && B <= BC_BMAX && N >= 0 && prior_std > 0.f);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, X_dev && labels_dev && W_dev && lp_out_dev);
    GMMVI_PROF(ctx, "target_bnn_classifier");
    if (int rc = bc_lds_attr(ctx)) return rc;
    const float inv_var = 1.f / (prior_std * prior_std);
    hipLaunchKernelGGL(bnn_classifier_target_kernel, dim3(N), dim3(BC_THREADS), BC_TARGET_FLOATS * sizeof(float), ctx->stream,
                       F, H, C, T, X_dev, labels_dev, (uint32_t)seed, (uint32_t)(seed >> 32), call,
                       gmmvi_feistel_half_bits((uint32_t)T), B, likelihood_scaling, inv_var, W_dev, N, lp_out_dev,
                       grad_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

extern "C" int gmmvi_bnn_classifier_predict(gmmvi_ctx* ctx, int F, int H, int C, const float* W_dev, int S,
                                            const float* X_dev, int M, float* logits_out_dev) {
    GMMVI_ARG_CHECK(ctx, bc_shape_ok(F, H, C));
    GMMVI_ARG_CHECK(ctx, S >= 0 && M >= 0 && S <= 65535);
    if (S == 0 || M == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, W_dev && X_dev && logits_out_dev);
    GMMVI_PROF(ctx, "bnn_classifier_predict");
    hipLaunchKernelGGL(bnn_classifier_predict_kernel, dim3((M + BC_CHUNK - 1) / BC_CHUNK, S), dim3(BC_THREADS),
                       BC_PREDICT_FLOATS * sizeof(float), ctx->stream, F, H, C, W_dev, X_dev, M, logits_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}
