// Generic Bayesian-neural-network target (target_distributions/bnn.py: BNN_LNPDF for any hidden_units list, one activation
// per layer, MSE or sparse categorical cross-entropy from logits) and its analytic gradient.
//
// Network widths[0] = F -> widths[1] -> ... -> widths[L] (L = n_layers dense layers, 2 <= L <= 4); the parameter vector of a
// sample is the reference's layout: per layer W [in, out] row-major, then b [out].  For sample n and the rows m of its batch
//     h_0 = x_m,  h_l = act_l(h_{l-1} W_l + b_l),  out = h_L (linear),  loss_m = (y_m - out)^2  or  logsumexp(out) - out[y_m]
//     lp[n]   = s (-(T / B) sum_m loss_m - 0.5 sum_d w_d^2 / sd^2)
//     grad[n] = d lp[n] / d w_n          (ReLU derivative 1 where the pre-activation is positive, else 0)
// The minibatch rows are bnn.hip's stream (feistel.h, stream id 3): position p = n B + j, epoch p div T, rank p mod T.
//
// Mapping: one workgroup (4 waves) per sample, 64 batch rows per chunk (B > 64 loops over chunks).  Every contraction runs on
// v_mfma_f32_16x16x4_f32 (exact f32) and walks the layer's input width in tiles of 32 through LDS:
//   forward   Z[m][j] = sum_k h_{l-1}[m][k] W_l[k][j]: the W_l tile [32][J] (and, for layer 0, the tile of gathered rows
//             [64][32]) is staged in LDS; wave w owns the rows 16 w .. 16 w + 15 and every output unit, up to 8 accumulator
//             tiles.  A operand: lane l -> h[16 w + (l & 15)][4 s + (l >> 4)], B operand: Ws[4 s + (l >> 4)][16 jt + (l & 15)],
//             D lane l, register r -> Z[16 w + 4 (l >> 4) + r][16 jt + (l & 15)].  Bias and activation in the epilogue; h_l
//             goes to its own LDS buffer, the outputs to a [64][20] buffer.
//   loss      lane m of wave 0 owns batch row m: loss and d lp / d out replace the outputs.
//   backward  layers from the last to the first, input tile by input tile (the same W_l tile serves both products):
//             dW_l[k][j] = sum_m h_{l-1}[m][k] dZ_l[m][j]   (wave w owns the output tiles 2 w, 2 w + 1; straight to the
//                                                            gradient row, a later chunk adds to what the same lane wrote)
//             dZ_{l-1}[m][k] = act'_{l-1}(h_{l-1}[m][k]) sum_j dZ_l[m][j] W_l[k][j]      (wave w owns its 16 rows)
//             Every derivative is a function of the activation's value (sigmoid h (1 - h), tanh 1 - h^2, ReLU [h > 0]), so no
//             pre-activation is kept: dZ_{l-1} overwrites h_{l-1} in place, element by element, once dW_l has read the tile.
//             db_l[j] = sum_m dZ_l[m][j]: lane j, rows in order.
// LDS budget (the choice among smaller chunks, recomputation and an HBM workspace: 64-row chunks and in-place deltas, so all
// three hidden layers stay resident): rows, labels, reduction 800 B | outputs [64][20] 5 120 B | X tile [64][36] 9 216 B |
// W tile [32][144] 18 432 B | one [64][132] buffer of 33 792 B per hidden layer: 67 360 B, 101 152 B and 134 944 B for one,
// two and three hidden layers (of the CU's 160 KB); the forward-only kernel uses the same layout.
// Every gradient entry is owned by one lane, every sum has a fixed order and there are no atomics: bitwise reproducible
// for a given (seed, call); the log density takes the same path with and without the gradient.
// Rows past the batch are all-zero, their d lp / d out is zero and their loss is masked; columns past a layer's width are
// zero in the W tile and are written as zero deltas.  A label outside [0, C) selects no logit (compared, never an index).
#include "common.h"
#include "feistel.h"
#include "wave_reduce.h"

namespace {
typedef float ml_f32x4 __attribute__((ext_vector_type(4)));
constexpr int ML_THREADS = 256;
constexpr int ML_CHUNK = 64;                       // batch rows per chunk
constexpr int ML_KT = 32;                          // input units per tile
constexpr int ML_HP = 128, ML_CP = 16;             // padded hidden units, outputs
constexpr int ML_FMAX = 1024, ML_BMAX = 1024;
constexpr int ML_LDH = ML_HP + 4;                  // h / dZ [64][132]: 4 i + k hits 64 distinct banks as the forward A operand
constexpr int ML_LDW = ML_HP + 16;                 // W tile [32][144]: 16 k + i likewise as the forward B operand
constexpr int ML_LDX = ML_KT + 4;                  // X tile [64][36]
constexpr int ML_LDO = ML_CP + 4;                  // outputs / d lp / d out [64][20]
constexpr int ML_ACT_LINEAR = 0, ML_ACT_SIGMOID = 1, ML_ACT_RELU = 2, ML_ACT_TANH = 3;
constexpr int ML_LOSS_MSE = 0, ML_LOSS_CE = 1;

constexpr int ML_HBUF = ML_CHUNK * ML_LDH;
constexpr int ML_FIXED_FLOATS = ML_CHUNK + ML_CHUNK + 8 + ML_CHUNK + ML_CHUNK * ML_LDO + ML_CHUNK * ML_LDX + ML_KT * ML_LDW;
inline size_t ml_lds_bytes(int n_layers) { return (size_t)(ML_FIXED_FLOATS + (n_layers - 1) * ML_HBUF) * sizeof(float); }

struct MlpNet {
    int L;                                         // dense layers
    int w[5];                                      // widths: F, hidden ..., outputs
    int act[4];
    int loss;
    int off[4];                                    // start of W_l in the parameter vector; b_l follows at off[l] + w[l] w[l + 1]
    int D;
};

struct MlpLds {
    int* rows;                                     // [64] data rows of the chunk, -1 past the batch
    int* lab;                                      // [64] labels (int32, or the bits of the f32 label)
    float* red;                                    // [8]
    float* Os;                                     // [64][20]
    float* Xs;                                     // [64][36]
    float* Ws;                                     // [32][144]
    float* Hs;                                     // [L - 1][64][132]
};

__device__ __forceinline__ MlpLds ml_carve(float* smem) {
    MlpLds s;
    s.rows = (int*)smem;
    s.lab = s.rows + ML_CHUNK;
    s.red = (float*)(s.lab + ML_CHUNK);
    s.Os = s.red + 8 + ML_CHUNK;                   // (64 spare floats keep the buffers behind 16-byte aligned)
    s.Xs = s.Os + ML_CHUNK * ML_LDO;
    s.Ws = s.Xs + ML_CHUNK * ML_LDX;
    s.Hs = s.Ws + ML_KT * ML_LDW;
    return s;
}

__device__ __forceinline__ float ml_act(int a, float z) {
    switch (a) {
        case ML_ACT_SIGMOID: return 1.f / (1.f + expf(-z));
        case ML_ACT_RELU: return fmaxf(z, 0.f);
        case ML_ACT_TANH: return tanhf(z);
        default: return z;
    }
}

// the activation's derivative from its value h = act(z); ReLU: z > 0 exactly where h > 0
__device__ __forceinline__ float ml_dact(int a, float h) {
    switch (a) {
        case ML_ACT_SIGMOID: return h * (1.f - h);
        case ML_ACT_RELU: return h > 0.f ? 1.f : 0.f;
        case ML_ACT_TANH: return 1.f - h * h;
        default: return 1.f;
    }
}

// rows k0 .. k0 + 31 of W [K][J] -> Ws [32][144], zero past K and J: thread t stages row (t >> 7) + 2 q, column t & 127
__device__ __forceinline__ void ml_stage_w(const float* __restrict__ Wl, int K, int J, int k0, float* __restrict__ Ws) {
    const int t = threadIdx.x, j = t & 127;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
        const int r = (t >> 7) + 2 * q, k = k0 + r;
        Ws[r * ML_LDW + j] = (k < K && j < J) ? Wl[(size_t)k * J + j] : 0.f;
    }
}

// features f0 .. f0 + 31 of the chunk's rows -> Xs [64][36], zero past F and past the batch: row (t >> 5) + 8 q, column t & 31
__device__ __forceinline__ void ml_stage_x(const float* __restrict__ X, int F, int f0, const int* __restrict__ rows_s,
                                           float* __restrict__ Xs) {
    const int t = threadIdx.x, c = t & 31, f = f0 + c;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int m = (t >> 5) + 8 * q, row = rows_s[m];
        Xs[m * ML_LDX + c] = (row >= 0 && f < F) ? X[(size_t)row * F + f] : 0.f;
    }
}

// layer l of the chunk: out[m][j] = act_l(sum_k in[m][k] W_l[k][j] + b_l[j]) for the 64 rows and the columns below 16 ceil(J / 16)
__device__ __forceinline__ void ml_forward_layer(const MlpNet& net, int l, const float* __restrict__ Wn,
                                                 const float* __restrict__ X, const MlpLds& s) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kq = lane >> 4;
    const int K = net.w[l], J = net.w[l + 1], NT = (J + 15) >> 4, a = net.act[l];
    const float* Wl = Wn + net.off[l];
    const float* bl = Wl + (size_t)K * J;
    const float* in = s.Hs + (l > 0 ? l - 1 : 0) * ML_HBUF;
    const bool last = l == net.L - 1;
    float* out = last ? s.Os : s.Hs + l * ML_HBUF;
    const int ldo = last ? ML_LDO : ML_LDH;
    ml_f32x4 acc[8];
#pragma unroll
    for (int jt = 0; jt < 8; ++jt) acc[jt] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < K; k0 += ML_KT) {
        __syncthreads();                                               // the previous tile (and layer) is done with the stage
        ml_stage_w(Wl, K, J, k0, s.Ws);
        if (l == 0) ml_stage_x(X, K, k0, s.rows, s.Xs);
        __syncthreads();
        const int ks = min(ML_KT, K - k0 + 3) >> 2;                    // 4-unit steps that hold an input unit
        for (int st = 0; st < ks; ++st) {
            const float av = l == 0 ? s.Xs[(16 * wave + i16) * ML_LDX + 4 * st + kq]
                                    : in[(16 * wave + i16) * ML_LDH + k0 + 4 * st + kq];
#pragma unroll
            for (int jt = 0; jt < 8; ++jt)
                if (jt < NT)
                    acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s.Ws[(4 * st + kq) * ML_LDW + 16 * jt + i16], acc[jt],
                                                                   0, 0, 0);
        }
    }
#pragma unroll
    for (int jt = 0; jt < 8; ++jt) {
        if (jt < NT) {
            const int j = 16 * jt + i16;
            const float b = j < J ? bl[j] : 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) out[(16 * wave + 4 * kq + r) * ldo + j] = ml_act(a, acc[jt][r] + b);
        }
    }
}

// the loss of batch row m (lane m of wave 0) from its outputs in Os; want_d: d lp / d out (coef = -T / B folded in) replaces
// the outputs.  Returns the row's loss, 0 past the batch.
__device__ __forceinline__ float ml_loss_row(const MlpNet& net, const MlpLds& s, int m, float coef, bool want_d) {
    const bool valid = s.rows[m] >= 0;
    float* o = s.Os + m * ML_LDO;
    float loss, d[ML_CP];
    if (net.loss == ML_LOSS_MSE) {
        const float r = __int_as_float(s.lab[m]) - o[0];
        loss = r * r;
#pragma unroll
        for (int c = 0; c < ML_CP; ++c) d[c] = 0.f;
        d[0] = valid ? -2.f * coef * r : 0.f;
    } else {
        const int C = net.w[net.L], y = s.lab[m];
        float l[ML_CP], mx = -INFINITY;
#pragma unroll
        for (int c = 0; c < ML_CP; ++c) {
            l[c] = o[c];
            if (c < C) mx = fmaxf(mx, l[c]);
        }
        float se = 0.f, ly = 0.f;
#pragma unroll
        for (int c = 0; c < ML_CP; ++c) {
            if (c < C) se += expf(l[c] - mx);
            if (c == y) ly = l[c];
        }
        const float lse = mx + logf(se);
        loss = lse - ly;
#pragma unroll
        for (int c = 0; c < ML_CP; ++c) {
            const float p = expf(l[c] - lse) - (c == y ? 1.f : 0.f);
            d[c] = (valid && c < C) ? coef * p : 0.f;
        }
    }
    if (want_d) {
#pragma unroll
        for (int c = 0; c < ML_CP; ++c) o[c] = d[c];
    }
    return valid ? loss : 0.f;
}

// gradient entry e of the sample: the first chunk writes it with the prior's term, a later chunk adds to it
__device__ __forceinline__ void ml_grad_store(float* __restrict__ gn, const float* __restrict__ Wn, int e, float g, bool first,
                                              float scaling, float inv_var) {
    gn[e] = first ? scaling * (g - Wn[e] * inv_var) : fmaf(scaling, g, gn[e]);
}

// layer l backward over the chunk (rows batch rows): dW_l, db_l -> gn; dZ_{l-1} replaces h_{l-1} (l > 0)
__device__ __forceinline__ void ml_backward_layer(const MlpNet& net, int l, const float* __restrict__ Wn,
                                                  float* __restrict__ gn, const float* __restrict__ X, const MlpLds& s,
                                                  int rows, bool first, float scaling, float inv_var) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i16 = lane & 15, kq = lane >> 4;
    const int K = net.w[l], J = net.w[l + 1], NTJ = (J + 15) >> 4;
    const int oW = net.off[l], ob = oW + K * J;
    const bool last = l == net.L - 1;
    const float* dz = last ? s.Os : s.Hs + l * ML_HBUF;
    const int ldz = last ? ML_LDO : ML_LDH;
    float* in = s.Hs + (l > 0 ? l - 1 : 0) * ML_HBUF;                  // h_{l-1}, then dZ_{l-1}
    const int aprev = l > 0 ? net.act[l - 1] : ML_ACT_LINEAR;
    const int ksb = (rows + 3) >> 2;                                   // rows past the batch have zero deltas
    const int ksj = (J + 3) >> 2;
    __syncthreads();                                                   // dZ_l is complete
    if (t < J) {
        float sum = 0.f;
        for (int m = 0; m < rows; ++m) sum += dz[m * ldz + t];
        ml_grad_store(gn, Wn, ob + t, sum, first, scaling, inv_var);
    }
    for (int k0 = 0; k0 < K; k0 += ML_KT) {
        __syncthreads();                                               // the previous tile is done with the stage
        if (l > 0) ml_stage_w(Wn + oW, K, J, k0, s.Ws);
        else ml_stage_x(X, K, k0, s.rows, s.Xs);
        __syncthreads();
        // ---- dW_l[k0 + ..][j]: this wave's output tiles 2 wave, 2 wave + 1 -------------------------------------------
        if (2 * wave < NTJ) {
            const bool two = 2 * wave + 1 < NTJ;
            ml_f32x4 g[2][2];
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int u = 0; u < 2; ++u) g[kt][u] = ml_f32x4{0.f, 0.f, 0.f, 0.f};
            for (int st = 0; st < ksb; ++st) {
                float xa[2], db[2];
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
                    xa[kt] = l == 0 ? s.Xs[(4 * st + kq) * ML_LDX + 16 * kt + i16]
                                    : in[(4 * st + kq) * ML_LDH + k0 + 16 * kt + i16];
                db[0] = dz[(4 * st + kq) * ldz + 32 * wave + i16];
                db[1] = two ? dz[(4 * st + kq) * ldz + 32 * wave + 16 + i16] : 0.f;
#pragma unroll
                for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        g[kt][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[kt], db[u], g[kt][u], 0, 0, 0);
            }
            // g[kt][u]: lane l, register r -> dW_l[k0 + 16 kt + 4 (l >> 4) + r][32 wave + 16 u + (l & 15)]
#pragma unroll
            for (int kt = 0; kt < 2; ++kt)
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int j = 32 * wave + 16 * u + i16;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = k0 + 16 * kt + 4 * kq + r;
                        if (k < K && j < J) ml_grad_store(gn, Wn, oW + k * J + j, g[kt][u][r], first, scaling, inv_var);
                    }
                }
        }
        // ---- dH_{l-1}[m][k0 + ..] = sum_j dZ_l[m][j] W_l[k][j]: this wave's 16 rows ----------------------------------
        ml_f32x4 d[2] = {ml_f32x4{0.f, 0.f, 0.f, 0.f}, ml_f32x4{0.f, 0.f, 0.f, 0.f}};
        if (l > 0) {
            for (int st = 0; st < ksj; ++st) {
                const float av = dz[(16 * wave + i16) * ldz + 4 * st + kq];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt)
                    d[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, s.Ws[(16 * nt + i16) * ML_LDW + 4 * st + kq], d[nt], 0, 0, 0);
            }
        }
        __syncthreads();                                               // dW_l has read this tile of h_{l-1}
        if (l > 0) {
            // d[nt]: lane l, register r -> row 16 wave + 4 (l >> 4) + r, unit k0 + 16 nt + (l & 15)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt) {
                const int k = k0 + 16 * nt + i16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int idx = (16 * wave + 4 * kq + r) * ML_LDH + k;
                    in[idx] = k < K ? d[nt][r] * ml_dact(aprev, in[idx]) : 0.f;
                }
            }
        }
    }
}
}  // namespace

__global__ __launch_bounds__(ML_THREADS) void bnn_mlp_target_kernel(MlpNet net, int T, const float* __restrict__ X,
                                                                    const int32_t* __restrict__ labels, uint32_t k0,
                                                                    uint32_t k1, uint32_t call, uint32_t hbits, int B,
                                                                    float scaling, float inv_var, const float* __restrict__ W,
                                                                    int N, float* __restrict__ lp, float* __restrict__ grad) {
    extern __shared__ float ml_smem[];
    const MlpLds s = ml_carve(ml_smem);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, n = blockIdx.x;
    const float* Wn = W + (size_t)n * net.D;
    float* gn = grad ? grad + (size_t)n * net.D : nullptr;

    // the prior: every parameter once, in a fixed order
    float wsq = 0.f;
    for (int e = t; e < net.D; e += ML_THREADS) wsq = fmaf(Wn[e], Wn[e], wsq);
    const float ws = gmmvi_wave_sum(wsq);
    if (lane == 0) s.red[wave] = ws;

    const float coef = -(float)T / (float)B;                           // d(-(T/B) sum loss) / d loss
    const gmmvi_bnn_stream_origin origin = gmmvi_bnn_stream_origin_of(n, B, T);
    float loss_acc = 0.f;                                              // wave 0

    for (int c0 = 0; c0 < B; c0 += ML_CHUNK) {
        const int rows = min(ML_CHUNK, B - c0);
        if (t < ML_CHUNK) {
            int row = -1, lab = net.loss == ML_LOSS_CE ? -1 : 0;      // past the batch: no class, label 0.f
            if (t < rows) {
                row = (int)gmmvi_bnn_stream_row(origin, c0 + t, T, call, hbits, k0, k1);
                lab = labels[row];                                     // MSE: the bits of the f32 label
            }
            s.rows[t] = row;
            s.lab[t] = lab;
        }
        for (int l = 0; l < net.L; ++l) ml_forward_layer(net, l, Wn, X, s);   // its first barrier orders rows / lab
        __syncthreads();
        if (wave == 0) loss_acc += gmmvi_wave_sum(ml_loss_row(net, s, lane, coef, grad != nullptr));
        if (grad) {
            for (int l = net.L - 1; l >= 0; --l) ml_backward_layer(net, l, Wn, gn, X, s, rows, c0 == 0, scaling, inv_var);
        }
        __syncthreads();                                               // rows, the stage and the buffers are rewritten
    }
    if (t == 0) {
        const float tot = (s.red[0] + s.red[1]) + (s.red[2] + s.red[3]);
        lp[n] = scaling * fmaf(coef, loss_acc, -0.5f * inv_var * tot);
    }
}

__global__ __launch_bounds__(ML_THREADS) void bnn_mlp_predict_kernel(MlpNet net, const float* __restrict__ W,
                                                                     const float* __restrict__ X, int M,
                                                                     float* __restrict__ out) {
    extern __shared__ float ml_smem[];
    const MlpLds s = ml_carve(ml_smem);
    const int t = threadIdx.x, sm = blockIdx.y, m0 = blockIdx.x * ML_CHUNK;
    const float* Wn = W + (size_t)sm * net.D;
    if (t < ML_CHUNK) s.rows[t] = m0 + t < M ? m0 + t : -1;
    for (int l = 0; l < net.L; ++l) ml_forward_layer(net, l, Wn, X, s);
    __syncthreads();
    const int C = net.w[net.L];
    for (int idx = t; idx < ML_CHUNK * C; idx += ML_THREADS) {
        const int m = idx / C, c = idx - m * C;
        if (m0 + m < M) out[((size_t)sm * M + m0 + m) * C + c] = s.Os[m * ML_LDO + c];
    }
}

namespace {
int ml_fail(gmmvi_ctx* ctx, const std::string& what) { return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: " + what); }

// the checked copy of the descriptor with the layers' offsets; GMMVI_OK or GMMVI_ERR_ARG with the limit in the message
int ml_net(gmmvi_ctx* ctx, const gmmvi_mlp_desc* d, MlpNet* net) {
    if (!d) return ml_fail(ctx, "net is NULL");
    if (d->n_layers < 2 || d->n_layers > GMMVI_MLP_MAX_LAYERS)
        return ml_fail(ctx, "n_layers must lie in [2, " + std::to_string(GMMVI_MLP_MAX_LAYERS) + "] (one to three hidden layers), got " +
                                std::to_string(d->n_layers));
    const int L = d->n_layers;
    if (d->widths[0] < 1 || d->widths[0] > ML_FMAX)
        return ml_fail(ctx, "the network takes 1 to " + std::to_string(ML_FMAX) + " features, got " + std::to_string(d->widths[0]));
    for (int l = 1; l < L; ++l)
        if (d->widths[l] < 1 || d->widths[l] > ML_HP)
            return ml_fail(ctx, "a hidden layer must have 1 to " + std::to_string(ML_HP) + " units, got " +
                                    std::to_string(d->widths[l]));
    if (d->loss != ML_LOSS_MSE && d->loss != ML_LOSS_CE) return ml_fail(ctx, "loss must be 0 (MSE) or 1 (cross-entropy)");
    if (d->loss == ML_LOSS_MSE && d->widths[L] != 1)
        return ml_fail(ctx, "the MSE loss takes one output, got " + std::to_string(d->widths[L]));
    if (d->loss == ML_LOSS_CE && (d->widths[L] < 2 || d->widths[L] > ML_CP))
        return ml_fail(ctx, "the cross-entropy loss takes 2 to " + std::to_string(ML_CP) + " classes, got " +
                                std::to_string(d->widths[L]));
    for (int l = 0; l < L; ++l)
        if (d->activations[l] < ML_ACT_LINEAR || d->activations[l] > ML_ACT_TANH)
            return ml_fail(ctx, "an activation must be 0 (linear), 1 (sigmoid), 2 (ReLU) or 3 (tanh), got " +
                                    std::to_string(d->activations[l]));
    if (d->activations[L - 1] != ML_ACT_LINEAR) return ml_fail(ctx, "the output layer's activation must be 0 (linear)");
    *net = MlpNet{};
    net->L = L;
    net->loss = d->loss;
    long off = 0;
    for (int l = 0; l <= L; ++l) net->w[l] = d->widths[l];
    for (int l = 0; l < L; ++l) {
        net->act[l] = d->activations[l];
        net->off[l] = (int)off;
        off += (long)d->widths[l] * d->widths[l + 1] + d->widths[l + 1];
    }
    if (off > GMMVI_MAX_DIM_DIAG)
        return ml_fail(ctx, "the network has " + std::to_string(off) + " parameters, more than GMMVI_MAX_DIM_DIAG = " +
                                std::to_string(GMMVI_MAX_DIM_DIAG));
    net->D = (int)off;
    return GMMVI_OK;
}

// the kernels' dynamic LDS lies above the 64 KB default
int ml_lds_attr(gmmvi_ctx* ctx) {
    const size_t bytes = ml_lds_bytes(GMMVI_MLP_MAX_LAYERS);
    const int rc = gmmvi_ensure_dynamic_lds(ctx, (const void*)bnn_mlp_target_kernel, bytes);
    return rc != GMMVI_OK ? rc : gmmvi_ensure_dynamic_lds(ctx, (const void*)bnn_mlp_predict_kernel, bytes);
}
}  // namespace

extern "C" int gmmvi_target_mlp(gmmvi_ctx* ctx, const gmmvi_mlp_desc* net, int T, const float* X_dev, const void* y_dev,
                                uint64_t seed, uint32_t call, int B, float likelihood_scaling, float prior_std,
                                const float* W_dev, int N, float* lp_out_dev, float* grad_out_dev) {
    MlpNet k;
    if (int rc = ml_net(ctx, net, &k)) return rc;
    if (T < 1) return ml_fail(ctx, "T must be at least 1");
    if (B < 1 || B > T || B > ML_BMAX)
        return ml_fail(ctx, "B must lie in [1, min(T, " + std::to_string(ML_BMAX) + ")], got B = " + std::to_string(B) + ", T = " +
                                std::to_string(T));
    if (!(prior_std > 0.f)) return ml_fail(ctx, "prior_std must be positive");
    if (N < 0) return ml_fail(ctx, "N must not be negative");
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, X_dev && y_dev && W_dev && lp_out_dev);
    GMMVI_PROF(ctx, "target_mlp");
    if (int rc = ml_lds_attr(ctx)) return rc;
    const float inv_var = 1.f / (prior_std * prior_std);
    hipLaunchKernelGGL(bnn_mlp_target_kernel, dim3(N), dim3(ML_THREADS), ml_lds_bytes(k.L), ctx->stream, k, T, X_dev,
                       (const int32_t*)y_dev, (uint32_t)seed, (uint32_t)(seed >> 32), call,
                       gmmvi_feistel_half_bits((uint32_t)T), B, likelihood_scaling, inv_var, W_dev, N, lp_out_dev,
                       grad_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

extern "C" int gmmvi_mlp_predict(gmmvi_ctx* ctx, const gmmvi_mlp_desc* net, const float* W_dev, int S, const float* X_dev,
                                 int M, float* out_dev) {
    MlpNet k;
    if (int rc = ml_net(ctx, net, &k)) return rc;
    if (S < 0 || S > 65535 || M < 0) return ml_fail(ctx, "S must lie in [0, 65535] and M must not be negative");
    if (S == 0 || M == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, W_dev && X_dev && out_dev);
    GMMVI_PROF(ctx, "mlp_predict");
    if (int rc = ml_lds_attr(ctx)) return rc;
    hipLaunchKernelGGL(bnn_mlp_predict_kernel, dim3((M + ML_CHUNK - 1) / ML_CHUNK, S), dim3(ML_THREADS), ml_lds_bytes(k.L),
                       ctx->stream, k, W_dev, X_dev, M, out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}
