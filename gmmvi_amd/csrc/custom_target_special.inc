R"GMMVI_SPECIAL(
// ---- special functions of user-defined targets (csrc/custom_target.hip puts this text behind the user's source in every mode,
// in front of the number types, and declares its nine functions in front of the source's first line; contract:
// include/gmmvi_hip.h, "differentiated user-defined targets") ----------------------------------------------------------------------
// Float functions in plain C++: a user's function may call them on a float, and the number types of custom_target_autodiff.inc
// and custom_target_tape.inc take their values and partial derivatives from them.  lgammaf, erff, erfcf, sinhf, coshf, asinf and
// acosf stay ROCm's (on the host: libm's).

// psi(x), x > 0: the recurrence psi(x) = psi(x + 1) - 1 / x up to x >= 6, then the asymptotic series in 1 / x^2, whose first
// dropped term is below 1e-11 there.  x <= 0 and NaN: NaN (no reflection formula).
__host__ __device__ inline float gmmvi_digamma(float x) {
    if (!(x > 0.f)) return __builtin_nanf("");
    float shift = 0.f;
    while (x < 6.f) { shift += 1.f / x; x += 1.f; }
    const float r = 1.f / x, r2 = r * r;
    const float series = r2 * (1.f / 12.f - r2 * (1.f / 120.f - r2 * (1.f / 252.f - r2 * (1.f / 240.f))));
    return (::logf(x) - 0.5f * r - series) - shift;
}

// psi'(x), x > 0: the recurrence psi'(x) = psi'(x + 1) + 1 / x^2 up to x >= 6, then the asymptotic series.  x <= 0 and NaN: NaN.
__host__ __device__ inline float gmmvi_trigamma(float x) {
    if (!(x > 0.f)) return __builtin_nanf("");
    float shift = 0.f;
    while (x < 6.f) { const float r = 1.f / x; shift += r * r; x += 1.f; }
    const float r = 1.f / x, r2 = r * r;
    const float series = r * (1.f + r * (0.5f + r * (1.f / 6.f - r2 * (1.f / 30.f - r2 * (1.f / 42.f - r2 * (1.f / 30.f))))));
    return series + shift;
}

// 1 / (1 + e^-x): the exponential of -|x| only, so neither branch overflows; exactly 1 and 0 beyond the range of expf
__host__ __device__ inline float gmmvi_sigmoid(float x) {
    const float e = ::expf(-::fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

// log(1 + e^x)
__host__ __device__ inline float gmmvi_softplus(float x) { return ::fmaxf(x, 0.f) + ::log1pf(::expf(-::fabsf(x))); }

// log(1 / (1 + e^-x)) = -softplus(-x)
__host__ __device__ inline float gmmvi_log_sigmoid(float x) { return -gmmvi_softplus(-x); }

// log(e^a + e^b); a == b, equal infinities included: a + ln 2, no NaN
__host__ __device__ inline float gmmvi_logaddexp(float a, float b) {
    if (a == b) return a + 0.69314718f;
    return ::fmaxf(a, b) + ::log1pf(::expf(-::fabsf(a - b)));
}

// ---- the normal distribution function and the scaled complementary error function -------------------------------------------------
// Everything here rests on one polynomial and on expf; erfcf takes no part, so nothing underflows before its logarithm is taken.
// Branches: the sign of x (x < 0 against x >= 0, NaN included) in every function; the overflow of 2 e^(x^2) in gmmvi_erfcx
// (x < -9.38); the underflow of e^(-x^2 / 2) to zero (|x| > 14.4) in half_square_exp; x^2 / 2 = inf in gmmvi_log_ndtr.
namespace gmmvi_special {
// (a - 2) / (a + 2): [0, inf] -> [-1, 1]
__host__ __device__ inline float erfcx_map(float a) { return a <= 3.4028235e38f ? (a - 2.f) / (a + 2.f) : 1.f; }

// (1 + 2a) e^(a^2) erfc(a), a >= 0, by q = (a - 2) / (a + 2): it rises from 1 at a = 0 to 2 / sqrt(pi) at infinity and is a
// polynomial of degree 12 in q to 4.2e-9 (the Chebyshev interpolant of the function in q, rounded to float)
__host__ __device__ inline float erfcx_poly(float q) {
    float g = -2.01089315e-05f;
    g = ::fmaf(g, q, 6.31001822e-05f);
    g = ::fmaf(g, q, 0.000221105453f);
    g = ::fmaf(g, q, -0.000357177894f);
    g = ::fmaf(g, q, -0.00146351173f);
    g = ::fmaf(g, q, 0.00121666549f);
    g = ::fmaf(g, q, 0.0087242946f);
    g = ::fmaf(g, q, -0.00801863614f);
    g = ::fmaf(g, q, -0.0542201847f);
    g = ::fmaf(g, q, 0.164049402f);
    g = ::fmaf(g, q, -0.166030392f);
    g = ::fmaf(g, q, -0.0927637592f);
    return ::fmaf(g, q, 1.27697837f);
}

// e^(a^2) erfc(a), a >= 0.  The quotient by 1 + 2a is formed as 0.5 / (a + 0.5), which does not overflow: 1 / (a sqrt(pi)) for a
// large, 0 at inf, NaN for NaN.
__host__ __device__ inline float erfcx_positive(float a) { return erfcx_poly(erfcx_map(a)) * (0.5f / (a + 0.5f)); }

// d/da of it, a >= 0: -(1 + 2a)^2 / 2 times the derivative rises from 1 / sqrt(pi) at a = 0 to 2 / sqrt(pi) at infinity and is a
// polynomial of its own in q (degree 12, 5.7e-8), because 2a erfcx(a) - 2 / sqrt(pi) cancels: its error would be 2 a^2 ulp of the
// result.  -1 / (a^2 sqrt(pi)) for a large, 0 beyond fp32's range.
__host__ __device__ inline float erfcx_positive_partial(float a) {
    const float q = erfcx_map(a);
    float k = 0.000288576499f;
    k = ::fmaf(k, q, 0.000895215606f);
    k = ::fmaf(k, q, -0.00117904111f);
    k = ::fmaf(k, q, -0.00649741245f);
    k = ::fmaf(k, q, 0.00115126511f);
    k = ::fmaf(k, q, 0.0300110318f);
    k = ::fmaf(k, q, 0.00128418661f);
    k = ::fmaf(k, q, -0.132000074f);
    k = ::fmaf(k, q, 0.101211376f);
    k = ::fmaf(k, q, 0.298102349f);
    k = ::fmaf(k, q, -0.591427743f);
    k = ::fmaf(k, q, 0.0915837362f);
    k = ::fmaf(k, q, 1.33495581f);
    const float r = 0.5f / (a + 0.5f);
    return -2.f * k * r * r;
}

// e^(z^2) erfc(z) at z = a / sqrt(2), a >= 0, without a rounded z: q = (z - 2) / (z + 2) = (a - 2 sqrt(2)) / (a + 2 sqrt(2)) with
// 2 sqrt(2) = 2.82842708f + 4.84064699e-8f in the numerator, which cancels next to it, and 0.5 / (z + 0.5) = sqrt(1/2) / (a + sqrt(1/2)).
__host__ __device__ inline float erfcx_scaled(float a) {
    const float q = a <= 3.4028235e38f ? ((a - 2.82842708f) - 4.84064699e-8f) / (a + 2.82842708f) : 1.f;
    return erfcx_poly(q) * (0.707106769f / (a + 0.707106769f));
}

// e^(-x^2 / 2): the rounding error of x * x / 2 is carried along (it would be x^2 / 4 ulp of the result); exactly 0 where expf
// underflows, x = +-inf included
__host__ __device__ inline float half_square_exp(float x) {
    const float u = 0.5f * x, h = u * x, l = ::fmaf(u, x, -h);
    const float e = ::expf(-h);
    return e == 0.f ? 0.f : ::fmaf(-l, e, e);
}
}  // namespace gmmvi_special

// e^(x^2) erfc(x).  x >= 0: finite and positive, 1 / (x sqrt(pi)) where x^2 overflows.  x < 0: 2 e^(x^2) - erfcx(-x), no cancellation
// (the first term is above 2, the second below 1), +inf where 2 e^(x^2) overflows (x < -9.38).  NaN: NaN.
__host__ __device__ inline float gmmvi_erfcx(float x) {
    const float p = gmmvi_special::erfcx_positive(::fabsf(x));
    if (!(x < 0.f)) return p;
    const float h = x * x, l = ::fmaf(x, x, -h);
    const float e = ::expf(h);                                      // e^(h + l) = e^h (1 + l); doubled last, so that it overflows last
    return e > 3.4028235e38f ? e : ::fmaf(2.f, ::fmaf(e, l, e), -p);
}

// Phi(x) = erfc(-x / sqrt(2)) / 2 = erfcx(|x| / sqrt(2)) e^(-x^2 / 2) / 2 for x < 0, one minus that for x >= 0: the exponential takes
// x^2 / 2, which has no rounded scale in it.  Exactly 0 below fp32's subnormal numbers and exactly 1 within half an ulp of 1.
__host__ __device__ inline float gmmvi_ndtr(float x) {
    const float t = 0.5f * gmmvi_special::erfcx_scaled(::fabsf(x)) * gmmvi_special::half_square_exp(x);
    return x < 0.f ? t : 1.f - t;
}

// log Phi(x).  x < 0: log(erfcx(-x / sqrt(2)) / 2) - x^2 / 2, two negative terms, finite as long as x^2 / 2 is (-inf beyond).
// x >= 0: log1p(-(1 - Phi(x))), 0 where 1 - Phi(x) underflows and at +inf.  NaN: NaN.
__host__ __device__ inline float gmmvi_log_ndtr(float x) {
    const float e = gmmvi_special::erfcx_scaled(::fabsf(x));
    if (x < 0.f) {
        const float u = 0.5f * x, h = u * x, l = ::fmaf(u, x, -h);
        if (!(h <= 3.4028235e38f)) return -h;
        return (::logf(0.5f * e) - l) - h;
    }
    return ::log1pf(-0.5f * e * gmmvi_special::half_square_exp(x));
}

namespace gmmvi_special {
// d/da logaddexp(a, b) = sigmoid(a - b); exactly 1/2 on a tie, equal infinities included
__host__ __device__ inline float logaddexp_partial(float a, float b) { return a == b ? 0.5f : ::gmmvi_sigmoid(a - b); }
// d/da erf(a) = 2 / sqrt(pi) * e^(-a^2); the rounding error of a * a is carried along, it would be a^2 / 2 ulp of the result
__host__ __device__ inline float erf_partial(float a) {
    const float h = a * a, l = ::fmaf(a, a, -h);
    const float e = ::expf(-h);
    return e == 0.f ? 0.f : 1.12837917f * e * (1.f - l);
}
// d/da erfcx(a) = 2 a erfcx(a) - 2 / sqrt(pi).  a < 0: both terms are negative; -inf where the value has overflowed.  a >= 0: the
// difference cancels, the polynomial above does not.
__host__ __device__ inline float erfcx_partial(float a) {
    return a < 0.f ? ::fmaf(2.f * a, ::gmmvi_erfcx(a), -1.12837917f) : erfcx_positive_partial(a);
}
// d/da Phi(a) = phi(a) = e^(-a^2 / 2) / sqrt(2 pi)
__host__ __device__ inline float ndtr_partial(float a) { return 0.398942280f * half_square_exp(a); }
// d/da log Phi(a) = phi(a) / Phi(a).  a < 0: sqrt(2 / pi) / erfcx(-a / sqrt(2)), which is -a for a large and is kept finite for
// every finite a; a >= 0: phi(a) / (1 - (1 - Phi(a))), 0 where phi underflows and at +inf.
__host__ __device__ inline float log_ndtr_partial(float a) {
    const float e = erfcx_scaled(::fabsf(a));
    if (a < 0.f) {
        const float r = 0.797884583f / e;
        return r > 3.4028235e38f && a >= -3.4028235e38f ? 3.4028235e38f : r;
    }
    const float f = half_square_exp(a);
    return 0.398942280f * f / ::fmaf(-0.5f * e, f, 1.f);
}
// d/da asin(a) = 1 / sqrt((1 - a) (1 + a)) (acos: minus that): 1 - a is exact next to 1; inf at |a| = 1, NaN beyond
__host__ __device__ inline float asin_partial(float a) { return 1.f / ::sqrtf((1.f - a) * (1.f + a)); }
}  // namespace gmmvi_special
)GMMVI_SPECIAL"
