// gmmvi_custom_data_predictive_probe (include/gmmvi_hip.h): the tile reduction and the tile merge of the predictive kernels of
// custom_target_data.inc (the lines between its two marker lines, cut out by the Makefile) run on the host on a given matrix
// l[N, M] of row terms.  The lane type of the text is a 64-wide vector here: the xor butterfly exchanges its entries exactly as
// the wave exchanges its lanes, so every combine (the order of the additions, the shift, the guards of the edge values) is the
// device's own code.  The loops follow the launch: tiles of 64 samples, chunks of the rows, lanes past N on the tile's last
// sample and masked out.  Host code only; GMMVI_PREDICTIVE_PROBE_MAIN adds a main() for a stand-alone build.
#include "common.h"

namespace gmmvi_pred {
struct Lanes {
    float v[64];
    Lanes() {}
    Lanes(float s) { for (int i = 0; i < 64; ++i) v[i] = s; }
};
struct Flags { bool b[64]; };

inline Lanes operator+(const Lanes& a, const Lanes& b) { Lanes r; for (int i = 0; i < 64; ++i) r.v[i] = a.v[i] + b.v[i]; return r; }
inline Lanes operator-(const Lanes& a, const Lanes& b) { Lanes r; for (int i = 0; i < 64; ++i) r.v[i] = a.v[i] - b.v[i]; return r; }
inline Lanes operator*(const Lanes& a, const Lanes& b) { Lanes r; for (int i = 0; i < 64; ++i) r.v[i] = a.v[i] * b.v[i]; return r; }
inline Lanes lane_xor(const Lanes& a, int mask) { Lanes r; for (int i = 0; i < 64; ++i) r.v[i] = a.v[i ^ mask]; return r; }
inline Lanes lane_max(const Lanes& a, const Lanes& b) { Lanes r; for (int i = 0; i < 64; ++i) r.v[i] = fmaxf(a.v[i], b.v[i]); return r; }
inline Lanes lane_exp(const Lanes& a) { Lanes r; for (int i = 0; i < 64; ++i) r.v[i] = expf(a.v[i]); return r; }
inline Lanes lane_pick(const Flags& c, const Lanes& a, const Lanes& b) {
    Lanes r;
    for (int i = 0; i < 64; ++i) r.v[i] = c.b[i] ? a.v[i] : b.v[i];
    return r;
}
inline float lane_first(const Lanes& a) { return a.v[0]; }
}  // namespace gmmvi_pred

#include "build/custom_target_predictive_text.inc"

extern "C" int gmmvi_custom_data_predictive_probe(const float* l, int N, int64_t M, int chunks_requested, float* lpd, float* mean,
                                                  float* var) {
    using namespace gmmvi_pred;
    int tiles = 0, chunks = 0;
    int64_t per = 0;
    if (!l || !lpd || !mean || !var)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_custom_data_predictive_probe: no array may be NULL");
    const int rc = gmmvi_custom_data_predictive_plan(N, M, chunks_requested, &tiles, &chunks, &per);
    if (rc != GMMVI_OK) return rc;
    std::vector<Part> part((size_t)tiles * (size_t)M);
    for (int tile = 0; tile < tiles; ++tile) {
        const int n0 = 64 * tile;
        const int valid = N - n0 < 64 ? N - n0 : 64;
        Flags is_sample;
        for (int lane = 0; lane < 64; ++lane) is_sample.b[lane] = lane < valid;
        for (int chunk = 0; chunk < chunks; ++chunk) {
            const int64_t begin = chunk * per, end = M - begin < per ? M : begin + per;
            for (int w = 0; w < 4; ++w) {
                for (int64_t m = begin + w; m < end; m += 4) {
                    Lanes row;
                    for (int lane = 0; lane < 64; ++lane) {
                        const int mine = lane < valid ? lane : valid - 1;
                        row.v[lane] = l[(size_t)(n0 + mine) * (size_t)M + (size_t)m];
                    }
                    part[(size_t)tile * (size_t)M + (size_t)m] = tile_reduce(row, is_sample, valid);
                }
            }
        }
    }
    for (int64_t m = 0; m < M; ++m) {
        Part run = part[(size_t)m];
        int n = N < 64 ? N : 64;
        for (int t = 1; t < tiles; ++t) {
            const int c = N - 64 * t < 64 ? N - 64 * t : 64;
            merge_part(run, n, part[(size_t)t * (size_t)M + (size_t)m], c);
            n += c;
        }
        finish_part(run, N, lpd[m], mean[m], var[m]);
    }
    return GMMVI_OK;
}

#ifdef GMMVI_PREDICTIVE_PROBE_MAIN
// Stand-alone run of the probe (for a host sanitizer build): three tiles with a ragged last one, a column of -inf and a NaN.
#include <cstdio>
std::string g_gmmvi_global_err;                                   // api.hip's, which a stand-alone build does not link
extern "C" int gmmvi_custom_data_plan(int N, int64_t rows, int, int* chunks, int* rows_per_chunk) {   // custom_target.hip's, one chunk
    (void)N;
    *chunks = 1; *rows_per_chunk = (int)rows;
    return GMMVI_OK;
}
extern "C" int gmmvi_custom_data_predictive_plan(int N, int64_t M, int request, int* tiles, int* chunks, int64_t* rows_per_chunk) {
    int per = 0;
    gmmvi_custom_data_plan(N, M, request, chunks, &per);
    *tiles = (N + 63) / 64; *rows_per_chunk = per;
    return GMMVI_OK;
}
int main() {
    const int N = 130, M = 5;
    std::vector<float> l((size_t)N * M), lpd(M), mean(M), var(M);
    for (int n = 0; n < N; ++n)
        for (int m = 0; m < M; ++m) l[(size_t)n * M + m] = -0.01f * (float)((n * 7 + m * 3) % 50) - (float)m;
    for (int n = 0; n < N; ++n) l[(size_t)n * M + 3] = -__builtin_huge_valf();
    l[(size_t)129 * M + 4] = __builtin_nanf("");
    const int bad = gmmvi_custom_data_predictive_probe(l.data(), N, M, 0, lpd.data(), mean.data(), var.data());
    printf("lpd %g %g %g %g %g, mean %g, var %g\n", lpd[0], lpd[1], lpd[2], lpd[3], lpd[4], mean[0], var[0]);
    return bad != 0 || !(lpd[0] < 0.f) || !(lpd[3] < -1e30f) || lpd[4] == lpd[4];
}
#endif
