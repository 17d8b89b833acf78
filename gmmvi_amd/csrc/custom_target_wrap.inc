R"GMMVI_WRAP(
// ---- wrapper kernels of a user-defined target (csrc/custom_target.hip appends this text to the user's source) -------------
// The text above defines   __device__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad);
// (contract: include/gmmvi_hip.h).  Each kernel below has exactly one call site of it, so that it is inlined and the address
// space of the row pointers follows from the call.  With GMMVI_WRAP_TILE_ONLY the text stops behind move_tile: the kernels of
// custom_target_data.inc use the tile mover and have no gmmvi_user_target to call.

namespace gmmvi_wrap {

// Moves a tile of `total` consecutive floats between global memory (`g`, dense rows of D) and an LDS image whose rows are
// S = D | 1 floats apart.  The wave walks the global side as one coalesced stream, 16 bytes per lane where the tile starts on
// a 16-byte boundary; (r, c) is the row / column of the lane's next element, advanced without a division.
template <bool TO_LDS>
__device__ __forceinline__ void move_tile(float* g, float* image, int D, int S, int total, int lane) {
    const bool wide = (reinterpret_cast<unsigned long long>(g) & 15ull) == 0ull;
    int done = 0;                                         // elements handled by the 16-byte part
    if (wide) {
        const int quads = total >> 2;
        const int step_r = 256 / D, step_c = 256 % D;     // one trip of the wave: 64 lanes * 4 floats
        int r = (4 * lane) / D, c = (4 * lane) % D;
        for (int q = lane; q < quads; q += 64) {
            float4* gp = reinterpret_cast<float4*>(g) + q;
            float v[4];
            if (TO_LDS) { const float4 t = *gp; v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
            int rr = r, cc = c;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (TO_LDS) image[rr * S + cc] = v[j]; else v[j] = image[rr * S + cc];
                if (++cc == D) { cc = 0; ++rr; }
            }
            if (!TO_LDS) *gp = make_float4(v[0], v[1], v[2], v[3]);
            r += step_r; c += step_c;
            if (c >= D) { c -= D; ++r; }
        }
        done = quads << 2;
    }
    {
        const int step_r = 64 / D, step_c = 64 % D;
        int r = (done + lane) / D, c = (done + lane) % D;
        for (int e = done + lane; e < total; e += 64) {
            if (TO_LDS) image[r * S + c] = g[e]; else g[e] = image[r * S + c];
            r += step_r; c += step_c;
            if (c >= D) { c -= D; ++r; }
        }
    }
}

#ifndef GMMVI_WRAP_TILE_ONLY
// Staged route: one wavefront per workgroup, 64 consecutive samples.  LDS: x image [64][D | 1], then (GRAD) the gradient
// image of the same shape.  Rows past N are neither read nor written.
template <bool GRAD>
__device__ __forceinline__ void staged(int D, const float* params, const float* X, int N, float* lp, float* grad) {
    extern __shared__ float gmmvi_wrap_lds[];
    const int lane = threadIdx.x;
    const int S = D | 1;
    const size_t n0 = (size_t)blockIdx.x * 64;
    const int rows = (size_t)N - n0 < 64 ? (int)((size_t)N - n0) : 64;
    float* xs = gmmvi_wrap_lds;
    float* gs = gmmvi_wrap_lds + 64 * S;
    move_tile<true>(const_cast<float*>(X) + n0 * (size_t)D, xs, D, S, rows * D, lane);
    __syncthreads();
    if (lane < rows) {
        const float v = gmmvi_user_target(xs + lane * S, D, params, GRAD ? gs + lane * S : nullptr);
        lp[n0 + lane] = v;
    }
    if (GRAD) {
        __syncthreads();
        move_tile<false>(grad + n0 * (size_t)D, gs, D, S, rows * D, lane);
    }
}

// Direct route: the lane is the sample, the rows stay in global memory.
template <bool GRAD>
__device__ __forceinline__ void direct(int D, const float* params, const float* X, int N, float* lp, float* grad) {
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)N) return;
    const float v = gmmvi_user_target(X + n * (size_t)D, D, params, GRAD ? grad + n * (size_t)D : nullptr);
    lp[n] = v;
}

#endif
}  // namespace gmmvi_wrap

#ifndef GMMVI_WRAP_TILE_ONLY
extern "C" __global__ __launch_bounds__(64) void gmmvi_custom_staged_lp(int D, const float* params, const float* X, int N,
                                                                         float* lp, float* grad) {
    gmmvi_wrap::staged<false>(D, params, X, N, lp, grad);
}
extern "C" __global__ __launch_bounds__(64) void gmmvi_custom_staged_grad(int D, const float* params, const float* X, int N,
                                                                           float* lp, float* grad) {
    gmmvi_wrap::staged<true>(D, params, X, N, lp, grad);
}
extern "C" __global__ __launch_bounds__(256) void gmmvi_custom_direct_lp(int D, const float* params, const float* X, int N,
                                                                          float* lp, float* grad) {
    gmmvi_wrap::direct<false>(D, params, X, N, lp, grad);
}
extern "C" __global__ __launch_bounds__(256) void gmmvi_custom_direct_grad(int D, const float* params, const float* X, int N,
                                                                            float* lp, float* grad) {
    gmmvi_wrap::direct<true>(D, params, X, N, lp, grad);
}
#endif
)GMMVI_WRAP"
