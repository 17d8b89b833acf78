// The register-path density sweeps (fused {sample tile x component} density / log-sum-exp / gradient kernels): what their four
// routes share.  One translation unit per route (density_reg.hip, density_pk.hip, density_mfma.hip, density_mfma_ws.hip) holds
// the route's kernel, its launch geometry and one entry function; density.hip chooses the route and launches (gmmvi_sweep_launch).
#pragma once
#include "common.h"
#include "combine.h"
#include "riders.h"
#include <cstdlib>
#include <type_traits>

// ---- kernel side ------------------------------------------------------------------------------------------------
// gridDim.y > 1: the components are split over blockIdx.y; lp_out / grad_out then receive per-chunk partials
// ([chunk][N], [chunk][N][D]) that combine_partials merges.
typedef float me_f32x4 __attribute__((ext_vector_type(4)));
// a workgroup barrier for data that travels through LDS only
#define ME_LDS_BARRIER()                                       \
    do {                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     \
        __builtin_amdgcn_s_barrier();                          \
        asm volatile("" ::: "memory");                         \
    } while (0)
// rows of the last 16-row tile of the padded dimension when there are at most four of them (handled on the vector unit by the
// matrix-core kernels), else 0
__host__ __device__ constexpr int me_rem_rows(int dp) { return (dp % 16 != 0 && dp % 16 <= 4 && dp > 16) ? dp % 16 : 0; }
// the value of lane 16 g + R of v in every lane of lane group g (DPP row broadcast)
template <int R>
__device__ __forceinline__ float me_row_bcast(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x150 + R, 0xf, 0xf, false));
}
template <int N, int I = 0, class F>
__device__ __forceinline__ void me_static_rows(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        me_static_rows<N, I + 1>(f);
    }
}
#ifndef GMMVI_ME_THREADS
#define GMMVI_ME_THREADS 1024
#define GMMVI_ME_MINW 1
#endif
// DP >= 40: at most 8 waves per workgroup, so that the compiler may use 256 VGPRs (x, z, y and the gradient accumulators are
// 4 DP registers; under the 128-register cap of a 16-wave workgroup the DP = 50 gradient kernel spilled 196 of them to scratch)
#ifndef GMMVI_ME_WIDE_DP
#define GMMVI_ME_WIDE_DP 40
#endif
// a wave barrier for data that travels through the wave's own LDS image only
#define ME_WAVE_LDS_SYNC()                                     \
    do {                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     \
        __builtin_amdgcn_wave_barrier();                       \
    } while (0)

// ---- host side --------------------------------------------------------------------------------------------------
// one sweep call: gmmvi_mixture_eval / gmmvi_mixture_eval_dual (logw2 / lp2: the second mixture over the same components)
struct SweepArgs {
    int family; float nu; int K, D;
    const float* packed; const float* logw; const float* X; int N;
    float* ld; float* lp; float* grad;
    const float* logw2; float* lp2;
};

// what a route's geometry code decides
struct SweepGeom {
    int tiles;           // sample tiles = the launch's own workgroups along x
    int ky;              // component chunks over blockIdx.y, rounded so that no chunk is empty
    int threads;         // per workgroup
    size_t shmem;        // dynamic LDS of the route's own workgroups (riders may need more)
};

// every sweep kernel instance has this parameter list
typedef void (*SweepKernel)(float nu, int K_total, int D, const float* packed, const float* logw, const float* X, int N,
                            float* ld_out, float* lp_out, float* grad_out, const float* logw2, float* lp2_out,
                            CombineJob carried, Riders riders);

// the (family, gradient) instance of a route: pick(std::integral_constant<int, family>, std::bool_constant<gradient>) returns
// the kernel, or nullptr where the route holds no such instance
template <class Pick>
inline SweepKernel sweep_instance(int family, bool want_grad, Pick&& pick) {
    if (family == GMMVI_GAUSS) {
        if (want_grad) return pick(std::integral_constant<int, GMMVI_GAUSS>{}, std::true_type{});
        return pick(std::integral_constant<int, GMMVI_GAUSS>{}, std::false_type{});
    }
    if (want_grad) return pick(std::integral_constant<int, GMMVI_STUDENT_T>{}, std::true_type{});
    return pick(std::integral_constant<int, GMMVI_STUDENT_T>{}, std::false_type{});
}

// density.hip: the part of a sweep launch that every route shares -- the partial buffers of a component split, the riders and
// the carried merge of the single-call iteration, the launch itself, then the merge of the partials or its deferral
int gmmvi_sweep_launch(gmmvi_ctx* ctx, const SweepArgs& a, const SweepGeom& g, SweepKernel kernel);

// the routes.  dp: the padded dimension; GMMVI_ERR_ARG for a (dp, gradient) the route holds no instance for
int gmmvi_sweep_reg(gmmvi_ctx* ctx, int dp, const SweepArgs& a);                 // one sample per lane, scalar-fed (dp below the matrix-core threshold)
int gmmvi_sweep_pk(gmmvi_ctx* ctx, int dp, const SweepArgs& a);                  // two samples per lane, packed arithmetic (dp <= 50)
int gmmvi_sweep_mfma(gmmvi_ctx* ctx, int dp, int sub_tiles, const SweepArgs& a); // matrix cores, 2 or 4 sub-tiles of 16 samples per wave
int gmmvi_sweep_mfma_ws(gmmvi_ctx* ctx, int dp, const SweepArgs& a);             // matrix cores, component block shared by the workgroup

// experiment knobs, read once
inline int sweep_env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
inline int sweep_env_nw() { static const int v = sweep_env_int("GMMVI_ME_NW", 0); return v; }   // waves per workgroup
inline int sweep_env_ky() { static const int v = sweep_env_int("GMMVI_ME_KY", 0); return v; }   // component chunks
