// Row permutation of the minibatch streams: pi(r) is a balanced 4-round Feistel network on 2h bits
// (h = ceil(ceil(log2 T) / 2)) walked until it lands in [0, T) (cycle walking); round i maps (L, R) -> (R, L xor
// (F_i(R) & (2^h - 1))) with F_i(R) = word 0 of Philox4x32-10 (philox.h), key (k0, k1) and counter
// (R | i << 24, epoch, call, stream).  Stream ids 0-2 are the samplers of oracle/philox.py; the three below are the
// minibatch streams.  experiments/target_distributions/minibatch_stream.py restates all of this in NumPy.
#pragma once
#include "philox.h"

constexpr uint32_t GMMVI_STREAM_BNN_MINIBATCH = 3;       // bnn.hip, bnn_classifier.hip, bnn_mlp.hip
constexpr uint32_t GMMVI_STREAM_LOGREG_MINIBATCH = 4;    // logreg_mb.hip: epoch word 0, its own position rule
constexpr uint32_t GMMVI_STREAM_DATA_MINIBATCH = 5;      // custom_target_data.inc: epoch word 0, batch row j is pi(j); own batches: the BNN layout

// h for a permutation of [0, T)
__host__ __device__ inline uint32_t gmmvi_feistel_half_bits(uint32_t T) {
    uint32_t bits = 0;
    while ((1ull << bits) < (uint64_t)T) ++bits;                       // ceil(log2 T)
    return (bits + 1) / 2;
}

__device__ __forceinline__ uint32_t gmmvi_feistel_permute(uint32_t r, uint32_t epoch, uint32_t call, uint32_t stream,
                                                           uint32_t T, uint32_t h, uint32_t k0, uint32_t k1) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = r;
    do {
        uint32_t L = x >> h, R = x & mask;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t f = philox4x32_10(R | (i << 24), epoch, call, stream, k0, k1).w[0] & mask;
            const uint32_t nl = R;
            R = L ^ f;
            L = nl;
        }
        x = (L << h) | R;
    } while (x >= T);
    return x;
}

// The BNN stream: row j of sample n's batch of B rows has stream position p = n B + j, epoch p div T and rank p mod T.
// The origin is the epoch and rank of j = 0, the same for a whole workgroup: compute it once, outside the per-lane path.
struct gmmvi_bnn_stream_origin { uint32_t e_base, r_base; };

__device__ inline gmmvi_bnn_stream_origin gmmvi_bnn_stream_origin_of(int n, int B, int T) {
    const uint64_t base = (uint64_t)n * (uint64_t)B;
    return {(uint32_t)(base / (uint64_t)T), (uint32_t)(base % (uint64_t)T)};
}

// data row of batch row j (0 <= j < B <= T, so r_base + j < 2 T: one wrap at most)
__device__ __forceinline__ uint32_t gmmvi_bnn_stream_row(gmmvi_bnn_stream_origin o, int j, int T, uint32_t call,
                                                          uint32_t hbits, uint32_t k0, uint32_t k1) {
    uint32_t r = o.r_base + (uint32_t)j, e = o.e_base;
    if (r >= (uint32_t)T) { r -= (uint32_t)T; ++e; }
    return gmmvi_feistel_permute(r, e, call, GMMVI_STREAM_BNN_MINIBATCH, (uint32_t)T, hbits, k0, k1);
}
