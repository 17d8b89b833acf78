R"GMMVI_VECTOR(
// ---- vector primitives of user-defined targets (csrc/custom_compile.hip puts this text behind custom_target_special.inc in every
// mode, in front of the number types, and declares the three float functions in front of the source's first line; contract:
// include/gmmvi_hip.h, "vector primitives") ---------------------------------------------------------------------------------------
//     gmmvi_dot(x, first, c, n)         sum over i < n of c[i] * x[first + i]
//     gmmvi_sqdist(x, first, c, n)      sum over i < n of (x[first + i] - c[i])^2
//     gmmvi_sumsq(x, first, n, center)  sum over i < n of (x[first + i] - center)^2
// Here: the value of each from plain floats, in one fixed order, and the overloads for x = const float* (value calls and the
// hand-written mode).  gmmvi_ad::Seed and gmmvi_tape::Input have overloads of their own in custom_target_autodiff.inc and
// custom_target_tape.inc, which take their values from the functions below: a value call and a gradient call give the same bits.
//
// The order: four partial sums, element i into partial i mod 4 by one fused multiply-add each (fmaf, whatever the contraction
// setting of the compiler), i ascending; the result is (s0 + s1) + (s2 + s3).  n <= 0 gives +0.
namespace gmmvi_vector {

enum Kind { DOT = 0, SQDIST = 1, SUMSQ = 2 };                      // the order of _lib.VECTOR_OPS, and the kind of a tape record

// x: the first element of the range, x + first of the caller
__host__ __device__ inline float dot_value(const float* x, const float* c, int n) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        s0 = ::fmaf(c[i], x[i], s0);
        s1 = ::fmaf(c[i + 1], x[i + 1], s1);
        s2 = ::fmaf(c[i + 2], x[i + 2], s2);
        s3 = ::fmaf(c[i + 3], x[i + 3], s3);
    }
    if (i < n) s0 = ::fmaf(c[i], x[i], s0);
    if (i + 1 < n) s1 = ::fmaf(c[i + 1], x[i + 1], s1);
    if (i + 2 < n) s2 = ::fmaf(c[i + 2], x[i + 2], s2);
    return (s0 + s1) + (s2 + s3);
}

__host__ __device__ inline float sqdist_value(const float* x, const float* c, int n) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const float d0 = x[i] - c[i], d1 = x[i + 1] - c[i + 1], d2 = x[i + 2] - c[i + 2], d3 = x[i + 3] - c[i + 3];
        s0 = ::fmaf(d0, d0, s0);
        s1 = ::fmaf(d1, d1, s1);
        s2 = ::fmaf(d2, d2, s2);
        s3 = ::fmaf(d3, d3, s3);
    }
    if (i < n) { const float d = x[i] - c[i]; s0 = ::fmaf(d, d, s0); }
    if (i + 1 < n) { const float d = x[i + 1] - c[i + 1]; s1 = ::fmaf(d, d, s1); }
    if (i + 2 < n) { const float d = x[i + 2] - c[i + 2]; s2 = ::fmaf(d, d, s2); }
    return (s0 + s1) + (s2 + s3);
}

__host__ __device__ inline float sumsq_value(const float* x, int n, float center) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        const float d0 = x[i] - center, d1 = x[i + 1] - center, d2 = x[i + 2] - center, d3 = x[i + 3] - center;
        s0 = ::fmaf(d0, d0, s0);
        s1 = ::fmaf(d1, d1, s1);
        s2 = ::fmaf(d2, d2, s2);
        s3 = ::fmaf(d3, d3, s3);
    }
    if (i < n) { const float d = x[i] - center; s0 = ::fmaf(d, d, s0); }
    if (i + 1 < n) { const float d = x[i + 1] - center; s1 = ::fmaf(d, d, s1); }
    if (i + 2 < n) { const float d = x[i + 2] - center; s2 = ::fmaf(d, d, s2); }
    return (s0 + s1) + (s2 + s3);
}

}  // namespace gmmvi_vector

__host__ __device__ inline float gmmvi_dot(const float* x, int first, const float* c, int n) {
    return gmmvi_vector::dot_value(x + first, c, n);
}
__host__ __device__ inline float gmmvi_sqdist(const float* x, int first, const float* c, int n) {
    return gmmvi_vector::sqdist_value(x + first, c, n);
}
__host__ __device__ inline float gmmvi_sumsq(const float* x, int first, int n, float center) {
    return gmmvi_vector::sumsq_value(x + first, n, center);
}
)GMMVI_VECTOR"
