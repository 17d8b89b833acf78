R"GMMVI_DATA(
// ---- kernels of a user-defined target summed over a data set (csrc/custom_target.hip puts this text behind the user's source,
// the dual-number text, the tile mover of custom_target_wrap.inc and the Feistel stream of feistel.h; contract:
// include/gmmvi_hip.h, "user-defined targets summed over a data set") ------------------------------------------------------------
// The text above defines
//     template <class T, class X> __device__ T gmmvi_user_row  (X x, int D, const float* row, int C, const float* params);
//     template <class T, class X> __device__ T gmmvi_user_prior(X x, int D, const float* params);
// and the target is  lp(x) = prior(x) + s * sum over the row list of row(x, data[r]).
//
// gmmvi_data_rows_*: grid (ceil(N / 64), chunks), 256 threads = 4 waves on the same 64 consecutive samples, lane = sample in
// every wave.  A workgroup owns rows_per_chunk consecutive positions of the row list; its wave w takes positions w, w + 4, ...
// of them.  Wave id, position and row index are wave-uniform by construction (readfirstlane), so a minibatch costs one Feistel
// walk per wave and row, and the row's floats come through uniform loads.
// Summation order (fixed, no atomics): within a wave in position order; wave 0 adds waves 1, 2, 3 in that order (LDS); chunks
// in index order (gmmvi_data_merge_*, or not at all with one chunk); then  s * sum,  then  + prior.
// gmmvi_data_rows_own_*: the same geometry, launch plan and summation order for own batches (minibatch == 2): every sample draws
// its own batch, so lane = sample reads its own row: position j of sample n is the stream position n B + j of (seed, call), with
// n the sample's index in the call.  The lane computes the epoch and rank of its j = 0 once (own_origin: the one 64-bit division)
// and walks the Feistel network itself for every position; the row pointer is a per-lane value, never made uniform, and the
// row's floats come through per-lane vector loads.  A gradient call repeats the walk in each of its ceil(D / W) passes: no
// index scratch, no extra launch (DESIGN.md 6 has the timing).
// params, X and the data set are __restrict__ kernel arguments: nothing a kernel stores can change them, which is what lets the
// compiler keep the uniform loads of a row on the scalar path although the passes of a gradient call store in between.
// LDS: [3][1 or 1 + W][64] wave accumulators, then (staged) the x image [64][D | 1].

namespace gmmvi_data {

using gmmvi_ad::Dual;
using gmmvi_ad::Seed;
constexpr int W = gmmvi_ad::W;

struct RowList {                // of the data set data[T, C]
    int C;
    unsigned T;
    int minibatch;              // 0: position p is row p; 1: row pi(p) of the stream of (seed, call); 2: own batches (own_row_at)
    unsigned length;            // T, or the batch size
    unsigned rows_per_chunk;
    unsigned call, hbits, k0, k1;
};

__device__ __forceinline__ const float* row_at(const float* data, const RowList& l, unsigned p) {
    unsigned r = p;
    if (l.minibatch) r = gmmvi_feistel_permute(p, 0u, l.call, GMMVI_STREAM_DATA_MINIBATCH, l.T, l.hbits, l.k0, l.k1);
    r = (unsigned)__builtin_amdgcn_readfirstlane((int)r);
    return data + (size_t)r * (size_t)l.C;
}

// Own batches: stream position n B + j has epoch (n B + j) div T and rank (n B + j) mod T.  The origin is the epoch and rank of
// j = 0 of the lane's sample; j < B <= T, so rank + j wraps at most once.  n < 2^31 and B <= T keep the epoch below 2^31.
struct OwnOrigin { unsigned epoch, rank; };

__device__ __forceinline__ OwnOrigin own_origin(size_t n, const RowList& l) {
    const unsigned long long base = (unsigned long long)n * l.length;
    return {(unsigned)(base / l.T), (unsigned)(base % l.T)};
}

// the row of position j of the lane's batch: a per-lane pointer
__device__ __forceinline__ const float* own_row_at(const float* data, const RowList& l, OwnOrigin o, unsigned j) {
    unsigned r = o.rank + j, e = o.epoch;
    if (r >= l.T) { r -= l.T; ++e; }
    r = gmmvi_feistel_permute(r, e, l.call, GMMVI_STREAM_DATA_MINIBATCH, l.T, l.hbits, l.k0, l.k1);
    return data + (size_t)r * (size_t)l.C;
}

template <bool OWN>
__device__ __forceinline__ const float* row_of(const float* data, const RowList& l, OwnOrigin o, unsigned p) {
    if constexpr (OWN) return own_row_at(data, l, o, p); else return row_at(data, l, p);
}

// wave 0 receives the sum of the four waves' `count` floats per lane, added in the order 0, 1, 2, 3; two barriers
template <int COUNT>
__device__ __forceinline__ void merge_waves(float (&acc)[COUNT], float* red, int w, int lane) {
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < COUNT; ++k) red[((w - 1) * COUNT + k) * 64 + lane] = acc[k];
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int v = 0; v < 3; ++v) {
#pragma unroll
            for (int k = 0; k < COUNT; ++k) acc[k] += red[(v * COUNT + k) * 64 + lane];
        }
    }
    __syncthreads();
}

// s * sum + prior for one pass (GRAD) or the value: what the last stage of either kernel does with a merged row sum
__device__ __forceinline__ float finish_value(float sum, float scale, const float* x, int D, const float* params) {
    const float scaled = scale * sum;
    return scaled + gmmvi_user_prior<float, const float*>(x, D, params);
}
__device__ __forceinline__ Dual finish_pass(const Dual& sum, float scale, const float* x, int first, int D, const float* params) {
    const Dual scaled = scale * sum;
    return scaled + gmmvi_user_prior<Dual, Seed>(Seed{x, first}, D, params);
}

template <bool GRAD, bool STAGED, bool OWN>
__device__ __forceinline__ void rows(int D, const float* params, const float* X, int N, const float* data, RowList l, float scale,
                                     float* lp, float* grad, float* part_lp, float* part_grad) {
    extern __shared__ float gmmvi_data_lds[];
    constexpr int COUNT = GRAD ? 1 + W : 1;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = D | 1;
    const size_t n0 = (size_t)blockIdx.x * 64;
    const int valid = (size_t)N - n0 < 64 ? (int)((size_t)N - n0) : 64;
    const int mine = lane < valid ? lane : valid - 1;     // lanes past N recompute the tile's last sample and write nothing
    float* red = gmmvi_data_lds;
    float* xs = gmmvi_data_lds + 3 * COUNT * 64;
    const float* x;
    if (STAGED) {
        const int r0 = 16 * w;                            // wave w moves rows 16 w .. 16 w + 15 of the tile
        const int count = valid - r0 < 16 ? valid - r0 : 16;
        if (count > 0)
            gmmvi_wrap::move_tile<true>(const_cast<float*>(X) + (n0 + r0) * (size_t)D, xs + r0 * S, D, S, count * D, lane);
        __syncthreads();
        x = xs + mine * S;
    } else {
        x = X + (n0 + mine) * (size_t)D;
    }
    const unsigned chunk = blockIdx.y;
    const bool single = gridDim.y == 1;
    const unsigned begin = chunk * l.rows_per_chunk;
    const unsigned end = l.length - begin < l.rows_per_chunk ? l.length : begin + l.rows_per_chunk;
    const size_t n = n0 + lane;
    const size_t slot = (size_t)chunk * (size_t)N + n;    // of the partials
    OwnOrigin o{};
    if constexpr (OWN) o = own_origin(n0 + mine, l);      // the sample's index in the call; lanes past N walk the last sample's batch

    if constexpr (!GRAD) {
        float acc[1] = {0.f};
        for (unsigned p = begin + w; p < end; p += 4)
            acc[0] += gmmvi_user_row<float, const float*>(x, D, row_of<OWN>(data, l, o, p), l.C, params);
        merge_waves<1>(acc, red, w, lane);
        if (w == 0) {
            if (single) {
                const float v = finish_value(acc[0], scale, x, D, params);
                if (lane < valid) lp[n] = v;
            } else if (lane < valid) {
                part_lp[slot] = acc[0];
            }
        }
    } else {
        for (int first = 0; first < D; first += W) {
            Dual sum(0.f);
            for (unsigned p = begin + w; p < end; p += 4)
                sum += gmmvi_user_row<Dual, Seed>(Seed{x, first}, D, row_of<OWN>(data, l, o, p), l.C, params);
            float acc[COUNT];
            acc[0] = sum.v;
#pragma unroll
            for (int j = 0; j < W; ++j) acc[1 + j] = sum.d[j];
            merge_waves<COUNT>(acc, red, w, lane);
            if (w == 0) {
                sum.v = acc[0];
#pragma unroll
                for (int j = 0; j < W; ++j) sum.d[j] = acc[1 + j];
                if (single) {
                    const Dual t = finish_pass(sum, scale, x, first, D, params);
                    if (lane < valid) {
                        if (first == 0) lp[n] = t.v;
#pragma unroll
                        for (int j = 0; j < W; ++j)
                            if (first + j < D) grad[n * (size_t)D + first + j] = t.d[j];
                    }
                } else if (lane < valid) {
                    if (first == 0) part_lp[slot] = sum.v;
#pragma unroll
                    for (int j = 0; j < W; ++j)
                        if (first + j < D) part_grad[slot * (size_t)D + first + j] = sum.d[j];
                }
            }
        }
    }
}

// chunks > 1: the thread is the sample; adds the chunks' partials in index order, then s * sum + prior
template <bool GRAD>
__device__ __forceinline__ void merge(int D, const float* params, const float* X, int N, int chunks, float scale, float* lp,
                                      float* grad, const float* part_lp, const float* part_grad) {
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)N) return;
    const float* x = X + n * (size_t)D;
    float value = 0.f;
    for (int c = 0; c < chunks; ++c) value += part_lp[(size_t)c * (size_t)N + n];
    if constexpr (!GRAD) {
        lp[n] = finish_value(value, scale, x, D, params);
    } else {
        for (int first = 0; first < D; first += W) {
            Dual sum(0.f);
            sum.v = value;
            for (int c = 0; c < chunks; ++c) {
                const float* g = part_grad + ((size_t)c * (size_t)N + n) * (size_t)D + first;
#pragma unroll
                for (int j = 0; j < W; ++j)
                    if (first + j < D) sum.d[j] += g[j];
            }
            const Dual t = finish_pass(sum, scale, x, first, D, params);
            if (first == 0) lp[n] = t.v;
#pragma unroll
            for (int j = 0; j < W; ++j)
                if (first + j < D) grad[n * (size_t)D + first + j] = t.d[j];
        }
    }
}

}  // namespace gmmvi_data

#define GMMVI_DATA_ROWS_KERNEL(name, GRAD, STAGED, OWN)                                                                        \
    extern "C" __global__ __launch_bounds__(256) void name(int D, const float* __restrict__ params,                         \
                                                           const float* __restrict__ X, int N,                             \
                                                           const float* __restrict__ data, gmmvi_data::RowList l,          \
                                                           float scale, float* lp, float* grad, float* part_lp,            \
                                                           float* part_grad) {                                             \
        gmmvi_data::rows<GRAD, STAGED, OWN>(D, params, X, N, data, l, scale, lp, grad, part_lp, part_grad);                \
    }
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_staged_lp, false, true, false)
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_staged_grad, true, true, false)
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_direct_lp, false, false, false)
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_direct_grad, true, false, false)
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_own_staged_lp, false, true, true)
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_own_staged_grad, true, true, true)
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_own_direct_lp, false, false, true)
GMMVI_DATA_ROWS_KERNEL(gmmvi_data_rows_own_direct_grad, true, false, true)
#undef GMMVI_DATA_ROWS_KERNEL

extern "C" __global__ __launch_bounds__(256) void gmmvi_data_merge_lp(int D, const float* __restrict__ params,
                                                                       const float* __restrict__ X, int N, int chunks, float scale,
                                                                       float* lp, float* grad, const float* part_lp,
                                                                       const float* part_grad) {
    gmmvi_data::merge<false>(D, params, X, N, chunks, scale, lp, grad, part_lp, part_grad);
}
extern "C" __global__ __launch_bounds__(256) void gmmvi_data_merge_grad(int D, const float* __restrict__ params,
                                                                         const float* __restrict__ X, int N, int chunks, float scale,
                                                                         float* lp, float* grad, const float* part_lp,
                                                                         const float* part_grad) {
    gmmvi_data::merge<true>(D, params, X, N, chunks, scale, lp, grad, part_lp, part_grad);
}

// ---- held-out predictive density: the reduction over the SAMPLES (gmmvi_custom_data_predictive; contract: include/gmmvi_hip.h,
// "predictive density of a data-set target") ---------------------------------------------------------------------------------------
// l[n, m] = gmmvi_user_row<float>(x_n, D, rows[m], C, params) for an evaluation set rows[M, C]; the prior takes no part.  Per row:
//     lpd[m] = log sum_n exp(l[n, m]) - log N (max-shifted),  mean[m] = sum_n l[n, m] / N,  var[m] = M2 / (N - 1) (0 for N = 1).
// gmmvi_data_predictive_*: the geometry of gmmvi_data_rows_*: grid (ceil(N / 64), chunks of the evaluation rows), 4 waves on the
// same 64 samples, lane = sample, wave w on positions w, w + 4, ... of its chunk, the row wave-uniform.  For its row the wave
// reduces over its lanes with an xor butterfly (1, 2, ..., 32; every lane ends with the same bits): the maximum, the sum of
// exp(l - shift), the sum of l (hence the tile mean), the sum of (l - tile mean)^2.  Lanes past N take no part: -inf to the
// maximum, 0 to the sums, and the tile's count is the number of valid lanes.  Lane 0 writes the tile's partial (max, sumexp, mean,
// M2) as one 16-byte vector store to part[tile][row], or, with one tile, finishes the row in place.
// gmmvi_data_predictive_merge: thread = row; merges the tiles IN TILE-INDEX ORDER: the log-sum-exp pairs by rescaling to the
// running maximum, mean and M2 by the pairwise update.  No atomics; chunks split the rows only, never a reduction, so a chunk
// request changes no output bit.
// Edge values: shift = the maximum if it is finite, else 0, so a column of -inf gives sumexp = 0 and lpd = -inf with no
// -inf - (-inf); +inf gives +inf; fmaxf drops a NaN, the sum of exponentials carries it into lpd.  A partial whose sumexp is
// exactly 0 (all -inf) is not rescaled (0 * exp(+large) would be NaN).  mean and var of a column that holds a non-finite value
// are whatever IEEE arithmetic gives.
// The functions between the two marker lines are __host__ __device__ over the lane type V: float on the device (one lane of a
// wave), a 64-wide vector in the host probe (csrc/predictive_probe.hip), which the Makefile feeds with exactly these lines.
// GMMVI_PRED_COMBINE_BEGIN
namespace gmmvi_pred {

struct Part { float max, sumexp, mean, m2; };

// one lane's side of the wave operations; the host probe defines the same five for its vector type
__device__ __forceinline__ float lane_xor(float v, int mask) { return __shfl_xor(v, mask, 64); }
__device__ __forceinline__ float lane_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ float lane_exp(float v) { return expf(v); }
__device__ __forceinline__ float lane_pick(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ float lane_first(float v) { return v; }

template <class V>
__host__ __device__ inline V wave_max(V v) {
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) v = lane_max(v, lane_xor(v, mask));
    return v;
}
template <class V>
__host__ __device__ inline V wave_sum(V v) {
#pragma unroll
    for (int mask = 1; mask < 64; mask <<= 1) v = v + lane_xor(v, mask);
    return v;
}

__host__ __device__ inline float shift_of(float mx) { return __builtin_isfinite(mx) ? mx : 0.f; }

// the partial of one tile for one row: l is the lane's row term, valid whether the lane is a sample, count the valid lanes
template <class V, class B>
__host__ __device__ inline Part tile_reduce(const V& l, const B& valid, int count) {
    Part p;
    p.max = lane_first(wave_max(lane_pick(valid, l, V(-__builtin_huge_valf()))));
    const float shift = shift_of(p.max);
    p.sumexp = lane_first(wave_sum(lane_pick(valid, lane_exp(l - V(shift)), V(0.f))));
    p.mean = lane_first(wave_sum(lane_pick(valid, l, V(0.f)))) / (float)count;
    const V d = l - V(p.mean);
    p.m2 = lane_first(wave_sum(lane_pick(valid, d * d, V(0.f))));
    return p;
}

// puts the partial t of c samples behind the running partial of n samples
__host__ __device__ inline void merge_part(Part& run, int n, const Part& t, int c) {
    const float mx = fmaxf(run.max, t.max);
    const float shift = shift_of(mx);
    const float a = run.sumexp == 0.f ? 0.f : run.sumexp * expf(shift_of(run.max) - shift);
    const float b = t.sumexp == 0.f ? 0.f : t.sumexp * expf(shift_of(t.max) - shift);
    run.max = mx;
    run.sumexp = a + b;
    const float total = (float)(n + c);
    const float delta = t.mean - run.mean;
    run.mean += delta * (float)c / total;
    run.m2 += t.m2 + delta * delta * (float)n * (float)c / total;
}

__host__ __device__ inline void finish_part(const Part& p, int N, float& lpd, float& mean, float& var) {
    lpd = (shift_of(p.max) + logf(p.sumexp)) - logf((float)N);
    mean = p.mean;
    var = N > 1 ? p.m2 / (float)(N - 1) : 0.f;
}

}  // namespace gmmvi_pred
// GMMVI_PRED_COMBINE_END

namespace gmmvi_data {

template <bool STAGED>
__device__ __forceinline__ void predictive(int D, const float* params, const float* X, int N, const float* rows, unsigned M, int C,
                                           unsigned rows_per_chunk, float* part, float* lpd, float* mean, float* var) {
    extern __shared__ float gmmvi_pred_lds[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int S = D | 1;
    const size_t n0 = (size_t)blockIdx.x * 64;
    const int valid = (size_t)N - n0 < 64 ? (int)((size_t)N - n0) : 64;
    const int mine = lane < valid ? lane : valid - 1;     // lanes past N read the tile's last sample and are masked out below
    const float* x;
    if (STAGED) {
        float* xs = gmmvi_pred_lds;
        const int r0 = 16 * w;                            // wave w moves rows 16 w .. 16 w + 15 of the tile
        const int count = valid - r0 < 16 ? valid - r0 : 16;
        if (count > 0)
            gmmvi_wrap::move_tile<true>(const_cast<float*>(X) + (n0 + r0) * (size_t)D, xs + r0 * S, D, S, count * D, lane);
        __syncthreads();
        x = xs + mine * S;
    } else {
        x = X + (n0 + mine) * (size_t)D;
    }
    const unsigned begin = blockIdx.y * rows_per_chunk;
    const unsigned end = M - begin < rows_per_chunk ? M : begin + rows_per_chunk;
    const bool single = gridDim.x == 1;
    for (unsigned p = begin + w; p < end; p += 4) {
        const unsigned m = (unsigned)__builtin_amdgcn_readfirstlane((int)p);
        const float l = gmmvi_user_row<float, const float*>(x, D, rows + (size_t)m * (size_t)C, C, params);
        const gmmvi_pred::Part t = gmmvi_pred::tile_reduce(l, lane < valid, valid);
        if (lane == 0) {
            if (single) {
                float a, b, c;
                gmmvi_pred::finish_part(t, N, a, b, c);
                lpd[m] = a;
                if (mean) mean[m] = b;
                if (var) var[m] = c;
            } else {
                reinterpret_cast<float4*>(part)[(size_t)blockIdx.x * (size_t)M + m] = make_float4(t.max, t.sumexp, t.mean, t.m2);
            }
        }
    }
}

}  // namespace gmmvi_data

#define GMMVI_DATA_PREDICTIVE_KERNEL(name, STAGED)                                                                          \
    extern "C" __global__ __launch_bounds__(256) void name(int D, const float* __restrict__ params,                         \
                                                           const float* __restrict__ X, int N,                             \
                                                           const float* __restrict__ rows, unsigned M, int C,              \
                                                           unsigned rows_per_chunk, float* part, float* lpd, float* mean,  \
                                                           float* var) {                                                   \
        gmmvi_data::predictive<STAGED>(D, params, X, N, rows, M, C, rows_per_chunk, part, lpd, mean, var);                 \
    }
GMMVI_DATA_PREDICTIVE_KERNEL(gmmvi_data_predictive_staged, true)
GMMVI_DATA_PREDICTIVE_KERNEL(gmmvi_data_predictive_direct, false)
#undef GMMVI_DATA_PREDICTIVE_KERNEL

// tiles > 1: the thread is the row; merges the tiles' partials in tile-index order and finishes the row
extern "C" __global__ __launch_bounds__(256) void gmmvi_data_predictive_merge(int N, unsigned M, int tiles, const float* part,
                                                                               float* lpd, float* mean, float* var) {
    const size_t m = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= (size_t)M) return;
    const float4* p4 = reinterpret_cast<const float4*>(part);
    float4 q = p4[m];
    gmmvi_pred::Part run{q.x, q.y, q.z, q.w};
    int n = N < 64 ? N : 64;
    for (int t = 1; t < tiles; ++t) {
        const int c = N - 64 * t < 64 ? N - 64 * t : 64;
        q = p4[(size_t)t * (size_t)M + m];
        gmmvi_pred::merge_part(run, n, gmmvi_pred::Part{q.x, q.y, q.z, q.w}, c);
        n += c;
    }
    float a, b, c;
    gmmvi_pred::finish_part(run, N, a, b, c);
    lpd[m] = a;
    if (mean) mean[m] = b;
    if (var) var[m] = c;
}
)GMMVI_DATA"
