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
//
// Two primitives take an array of the mode's number type T (a float here, a Dual or a Var in the gradient modes), typically one
// local to the user's function:
//     gmmvi_wdot(x, first, h, n)        sum over i < n of h[i] * x[first + i], h a const T*
//     gmmvi_logsumexp(a, n)             log of the sum over i < n of exp(a[i]), a a const T*
// Their values come from the two templates over an accessor below (entry i of the array as a float), which all three number
// types call: gmmvi_wdot in the order above, so that on floats it has the bits of gmmvi_dot; gmmvi_logsumexp as m + logf(s) with
// m the maximum by fmaxf, i ascending from -inf, and s the sum of expf(a[i] - m) in four partial sums by plain adds, merged as
// above.  m == -inf (n <= 0, every entry -inf; fmaxf drops NaNs, so an array of NaNs as well) gives -inf and no partials.
//
// A whole affine layer is one call, with strides:
//     gmmvi_affine(x, w, si, sj, b, sb, h, n, out, m)
//         out[j] = (sum over i < n of h[i] * x[w + i * si + j * sj]) + x[b + j * sb], j < m; b < 0: no bias term
// h a const T* or a const float*, out a T*.  The sum of every out[j] comes from affine_value below in the order above (with
// si == 1 it is wdot_value on x + w + j * sj, bit for bit); the bias is one plain add behind it.  n <= 0: out[j] is x[b + j * sb]
// itself, or 0 without a bias.  m <= 0 writes nothing.
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

enum NodeOp { WDOT = 0, LOGSUMEXP = 1 };                           // the order of _lib.NODE_OPS, and z of a node-array record's header
constexpr int AFFINE = 2;                                          // z of the headers of a gmmvi_affine record group
constexpr int NODES = 3;                                           // the kind of the tape's node-array record

struct FloatAt {                                                   // the accessor of a float array
    const float* p;
    __host__ __device__ float operator()(int i) const { return p[i]; }
};

// x: the first element of the range; h(i): the value of entry i.  The order of dot_value.
template <class At>
__host__ __device__ inline float wdot_value(const float* x, At h, int n) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        s0 = ::fmaf(h(i), x[i], s0);
        s1 = ::fmaf(h(i + 1), x[i + 1], s1);
        s2 = ::fmaf(h(i + 2), x[i + 2], s2);
        s3 = ::fmaf(h(i + 3), x[i + 3], s3);
    }
    if (i < n) s0 = ::fmaf(h(i), x[i], s0);
    if (i + 1 < n) s1 = ::fmaf(h(i + 1), x[i + 1], s1);
    if (i + 2 < n) s2 = ::fmaf(h(i + 2), x[i + 2], s2);
    return (s0 + s1) + (s2 + s3);
}

// wdot_value with the elements of x `si` apart: x is &x[w + j * sj] of the caller.  All three number types take the sum of
// gmmvi_affine from here.
template <class At>
__host__ __device__ inline float affine_value(const float* x, int si, At h, int n) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        s0 = ::fmaf(h(i), x[i * si], s0);
        s1 = ::fmaf(h(i + 1), x[(i + 1) * si], s1);
        s2 = ::fmaf(h(i + 2), x[(i + 2) * si], s2);
        s3 = ::fmaf(h(i + 3), x[(i + 3) * si], s3);
    }
    if (i < n) s0 = ::fmaf(h(i), x[i * si], s0);
    if (i + 1 < n) s1 = ::fmaf(h(i + 1), x[(i + 1) * si], s1);
    if (i + 2 < n) s2 = ::fmaf(h(i + 2), x[(i + 2) * si], s2);
    return (s0 + s1) + (s2 + s3);
}
// out[j] of gmmvi_affine for n > 0: the sum, then the bias by one plain add
template <class At>
__host__ __device__ inline float affine_out(const float* x, int w, int si, int sj, int b, int sb, At h, int n, int j) {
    const float s = affine_value(x + w + j * sj, si, h, n);
    return b < 0 ? s : s + x[b + j * sb];
}

// -> m + logf(s); m and s go back to the caller for the partials.  m == -inf: -> -inf, s = 0, and there are no partials.
template <class At>
__host__ __device__ inline float logsumexp_value(At a, int n, float& m, float& s) {
    const float lowest = -__builtin_inff();
    m = lowest;
    s = 0.f;
    for (int i = 0; i < n; ++i) m = ::fmaxf(m, a(i));
    if (m == lowest) return lowest;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int i = 0;
    for (; i + 4 <= n; i += 4) {
        s0 += ::expf(a(i) - m);
        s1 += ::expf(a(i + 1) - m);
        s2 += ::expf(a(i + 2) - m);
        s3 += ::expf(a(i + 3) - m);
    }
    if (i < n) s0 += ::expf(a(i) - m);
    if (i + 1 < n) s1 += ::expf(a(i + 1) - m);
    if (i + 2 < n) s2 += ::expf(a(i + 2) - m);
    s = (s0 + s1) + (s2 + s3);
    return m + ::logf(s);
}

// d logsumexp / d a[i], from the m and s of logsumexp_value: both gradient modes form their partials here
__host__ __device__ inline float logsumexp_partial(float a, float m, float s) { return ::expf(a - m) / s; }

}  // namespace gmmvi_vector

__host__ __device__ inline float gmmvi_wdot(const float* x, int first, const float* h, int n) {
    return gmmvi_vector::wdot_value(x + first, gmmvi_vector::FloatAt{h}, n);
}
__host__ __device__ inline float gmmvi_logsumexp(const float* a, int n) {
    float m, s;
    return gmmvi_vector::logsumexp_value(gmmvi_vector::FloatAt{a}, n, m, s);
}
__host__ __device__ inline void gmmvi_affine(const float* x, int w, int si, int sj, int b, int sb, const float* h, int n, float* out,
                                             int m) {
    for (int j = 0; j < m; ++j) {
        if (n <= 0) out[j] = b < 0 ? 0.f : x[b + j * sb];
        else out[j] = gmmvi_vector::affine_out(x, w, si, sj, b, sb, gmmvi_vector::FloatAt{h}, n, j);
    }
}
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
