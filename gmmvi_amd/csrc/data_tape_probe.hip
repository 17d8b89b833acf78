// gmmvi_data_tape_probe (include/gmmvi_hip.h): the two lane bodies of custom_target_data_tape.inc (the rows loop with its sweep,
// the finish with the prior's sweep; raw-string delimiters taken off by the Makefile, without the kernels) run on the host behind
// the row term and prior of custom_data_tape_sample.hip: lane stride 1, one sample after another, one chunk after another.  The
// row list is the device's: position p is row p, or row pi(p) of the Feistel stream (feistel.h and philox.h, restated here for
// the host, where __umulhi does not exist).  Host code only; GMMVI_DATA_TAPE_PROBE_MAIN adds a main() for a stand-alone build.
#include "common.h"

#define GMMVI_DATA_TAPE_PROBE
#define GMMVI_DATA_TAPE_NO_KERNELS
#include "custom_data_tape_sample.hip"

namespace {
constexpr uint32_t kStreamDataMinibatch = 5;                      // GMMVI_STREAM_DATA_MINIBATCH

uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += W0; k1 += W1;
    }
    return c0;
}

uint32_t half_bits(uint32_t T) {
    uint32_t bits = 0;
    while ((1ull << bits) < (uint64_t)T) ++bits;
    return (bits + 1) / 2;
}

uint32_t feistel_permute(uint32_t r, uint32_t call, uint32_t T, uint32_t h, uint32_t k0, uint32_t k1) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t x = r;
    do {
        uint32_t L = x >> h, R = x & mask;
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t f = philox_word0(R | (i << 24), 0u, call, kStreamDataMinibatch, k0, k1) & mask;
            const uint32_t nl = R;
            R = L ^ f;
            L = nl;
        }
        x = (L << h) | R;
    } while (x >= T);
    return x;
}
}  // namespace

extern "C" int gmmvi_data_tape_probe(int D, const float* params, const float* data, int64_t T, int C, int minibatch, int64_t B,
                                     uint64_t seed, uint32_t call, const float* X, int N, int chunks, int rows_per_chunk,
                                     int capacity, float* lp, float* grad, int* needed) {
    using namespace gmmvi_data_tape;
    if (!data || !X || !lp || !grad || !needed || N < 1 || D < 1 || C < D + 1 || T < 1 || T > 2147483647ll ||
        (minibatch != 0 && minibatch != 1) || B < 1 || B > T || capacity < 1)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_data_tape_probe: needs N, D, T >= 1, C >= D + 1 (the sample row term reads "
                                                  "row[D]), 1 <= B <= T, capacity >= 1 and no NULL array but params");
    const int64_t length = minibatch ? B : T;
    if (chunks < 1 || rows_per_chunk < 1 || (int64_t)chunks * rows_per_chunk < length ||
        (int64_t)(chunks - 1) * rows_per_chunk >= length)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_data_tape_probe: the chunk plan does not cover the row list, or its last "
                                                  "chunk is empty");
    const uint32_t hbits = half_bits((uint32_t)T), k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const float scale = minibatch ? (float)T / (float)B : 1.f;
    auto row_at = [&](unsigned p) {
        const uint32_t r = minibatch ? feistel_permute(p, call, (uint32_t)T, hbits, k0, k1) : p;
        return data + (size_t)r * (size_t)C;
    };
    std::vector<gmmvi_tape::Rec4> rec((size_t)chunks * capacity);
    std::vector<float> adj((size_t)chunks * capacity), acc((size_t)chunks * D), g((size_t)D);
    std::vector<float> out((size_t)N * D);
    int longest = 0;
    for (int n = 0; n < N; ++n) {
        const float* x = X + (size_t)n * D;
        for (int c = 0; c < chunks; ++c) {
            const RecPtr rp = (RecPtr)rec.data() + (size_t)c * capacity;
            const AdjPtr ap = (AdjPtr)adj.data() + (size_t)c * capacity;
            gmmvi_tape::tape() = gmmvi_tape::Tape{rp, ap, 1, capacity, D};
            const unsigned begin = (unsigned)c * (unsigned)rows_per_chunk;
            const unsigned end = length - begin < rows_per_chunk ? (unsigned)length : begin + (unsigned)rows_per_chunk;
            const int made = rows_lane(x, D, params, C, row_at, begin, end, rp, ap, 1, capacity, acc.data() + (size_t)c * D);
            if (made > longest) longest = made;
        }
        gmmvi_tape::tape() = gmmvi_tape::Tape{(RecPtr)rec.data(), (AdjPtr)adj.data(), 1, capacity, D};
        const int made = finish_lane(x, D, params, chunks, scale, (RecPtr)rec.data(), (AdjPtr)adj.data(), (size_t)capacity,
                                     acc.data(), (size_t)D, 1, capacity, lp + n, g.data());
        if (made > longest) longest = made;
        memcpy(out.data() + (size_t)n * D, g.data(), sizeof(float) * D);
    }
    *needed = longest;
    if (longest <= capacity) memcpy(grad, out.data(), sizeof(float) * out.size());   // an incomplete tape claims no gradient
    return GMMVI_OK;
}

#ifdef GMMVI_DATA_TAPE_PROBE_MAIN
// Stand-alone run of the probe (for a host sanitizer build): full data in three chunks, a minibatch, and a capacity too small.
#include <cstdio>
std::string g_gmmvi_global_err;                                   // api.hip's, which a stand-alone build does not link
int main() {
    const int D = 7, N = 3, C = D + 1;
    const int64_t T = 13;
    std::vector<float> data((size_t)T * C), X((size_t)N * D), lp(N), grad((size_t)N * D);
    for (size_t i = 0; i < data.size(); ++i) data[i] = i % C == (size_t)D ? (i % 3 ? 1.f : -1.f) : 0.1f * (float)((int)(i % 11) - 5);
    for (size_t i = 0; i < X.size(); ++i) X[i] = 0.25f * (float)((int)(i % 9) - 4);
    const float params[2] = {0.25f, 2.f};
    int needed = 0, bad = 0;
    bad |= gmmvi_data_tape_probe(D, params, data.data(), T, C, 0, T, 9, 0, X.data(), N, 3, 5, 64, lp.data(), grad.data(), &needed);
    printf("full data, 3 chunks: needed %d lp %g grad %g\n", needed, lp[0], grad[0]);
    bad |= gmmvi_data_tape_probe(D, params, data.data(), T, C, 1, 5, 9, 3, X.data(), N, 2, 3, needed, lp.data(), grad.data(), &needed);
    printf("minibatch, 2 chunks: needed %d lp %g grad %g\n", needed, lp[0], grad[0]);
    bad |= gmmvi_data_tape_probe(D, params, data.data(), T, C, 0, T, 9, 0, X.data(), N, 1, 13, 4, lp.data(), grad.data(), &needed);
    printf("capacity 4: needed %d lp %g\n", needed, lp[0]);
    return bad != 0 || needed <= 4;
}
#endif
