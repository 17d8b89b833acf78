// Row permutation of the minibatch streams: pi(r) is a balanced 4-round Feistel network on 2h bits
// (h = ceil(ceil(log2 T) / 2)) walked until it lands in [0, T) (cycle walking); round i maps (L, R) -> (R, L xor
// (F_i(R) & (2^h - 1))) with F_i(R) = word 0 of Philox4x32-10 (philox.h), key (k0, k1) and counter
// (R | i << 24, epoch, call, stream).  Stream ids: 3 the WINE minibatches (bnn.hip), 4 the minibatch logistic
// regressions (logreg_mb.hip); 0-2 are the samplers of oracle/philox.py.
#pragma once
#include "philox.h"

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
