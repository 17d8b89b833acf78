R"GMMVI_SPECIAL(
// ---- special functions of user-defined targets (csrc/custom_target.hip puts this text behind the user's source in every mode,
// in front of the number types, and declares its six functions in front of the source's first line; contract:
// include/gmmvi_hip.h, "differentiated user-defined targets") ----------------------------------------------------------------------
// Float functions in plain C++: a user's function may call them on a float, and the number types of custom_target_autodiff.inc
// and custom_target_tape.inc take their values and partial derivatives from them.  lgammaf, erff and erfcf stay ROCm's (on the
// host: libm's).

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

namespace gmmvi_special {
// d/da logaddexp(a, b) = sigmoid(a - b); exactly 1/2 on a tie, equal infinities included
__host__ __device__ inline float logaddexp_partial(float a, float b) { return a == b ? 0.5f : ::gmmvi_sigmoid(a - b); }
// d/da erf(a) = 2 / sqrt(pi) * e^(-a^2); the rounding error of a * a is carried along, it would be a^2 / 2 ulp of the result
__host__ __device__ inline float erf_partial(float a) {
    const float h = a * a, l = ::fmaf(a, a, -h);
    const float e = ::expf(-h);
    return e == 0.f ? 0.f : 1.12837917f * e * (1.f - l);
}
}  // namespace gmmvi_special
)GMMVI_SPECIAL"
