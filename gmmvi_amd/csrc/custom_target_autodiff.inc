R"GMMVI_AD(
// ---- forward-mode differentiation of a user-defined density (csrc/custom_target.hip puts this text between the user's source
// and the wrapper kernels; contract: include/gmmvi_hip.h, "differentiated user-defined targets") --------------------------------
// The text above defines   template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params);
// This text defines the dual number the library instantiates T with on a gradient call (a value and W tangents), the view X
// that seeds it, and gmmvi_user_target on top of the user's function, which is what the wrapper kernels call.
// GMMVI_CUSTOM_AUTODIFF_TANGENTS comes from include/gmmvi_hip.h (the run-time compiler gets it as a -D option).
//
// Tie rules: fabs has tangent 0 at +-0; fmax and fmin take the first operand's tangent on a tie; comparisons look at the values
// only, so a branch on a comparison differentiates the branch taken.  sqrt and rsqrt at 0 and log at 0 have infinite
// derivatives, as in IEEE arithmetic.  lgamma has a NaN tangent at a <= 0; gmmvi_logaddexp has the tangents 1/2 and 1/2 on a tie;
// gmmvi_sigmoid is exactly 1 or 0 with tangent 0 beyond the range of expf; asin and acos have infinite tangents at |a| = 1;
// gmmvi_erfcx has the tangent -inf, not NaN, where its value has overflowed.  There is no conversion from a dual to float:
// gmmvi_value(t) is the only way down.

namespace gmmvi_ad {

constexpr int W = GMMVI_CUSTOM_AUTODIFF_TANGENTS;

#define GMMVI_AD_FN __host__ __device__ __forceinline__
#define GMMVI_AD_EACH _Pragma("unroll") for (int j = 0; j < W; ++j)

GMMVI_AD_FN float rsqrt_value(float a) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ::rsqrtf(a);
#else
    return 1.f / ::sqrtf(a);
#endif
}

struct Dual {
    float v;
    float d[W];
    Dual() = default;
    GMMVI_AD_FN Dual(float value) : v(value) { GMMVI_AD_EACH d[j] = 0.f; }      // a constant: every tangent is 0
};

// value `v`, tangents s * a.d
GMMVI_AD_FN Dual chain(float v, float s, const Dual& a) {
    Dual r; r.v = v;
    GMMVI_AD_EACH r.d[j] = s * a.d[j];
    return r;
}

// ---- arithmetic ------------------------------------------------------------------------------------------------------------
GMMVI_AD_FN Dual operator-(const Dual& a) { Dual r; r.v = -a.v; GMMVI_AD_EACH r.d[j] = -a.d[j]; return r; }
GMMVI_AD_FN Dual operator+(const Dual& a) { return a; }

GMMVI_AD_FN Dual operator+(const Dual& a, const Dual& b) { Dual r; r.v = a.v + b.v; GMMVI_AD_EACH r.d[j] = a.d[j] + b.d[j]; return r; }
GMMVI_AD_FN Dual operator+(const Dual& a, float b) { Dual r = a; r.v = a.v + b; return r; }
GMMVI_AD_FN Dual operator+(float a, const Dual& b) { Dual r = b; r.v = a + b.v; return r; }

GMMVI_AD_FN Dual operator-(const Dual& a, const Dual& b) { Dual r; r.v = a.v - b.v; GMMVI_AD_EACH r.d[j] = a.d[j] - b.d[j]; return r; }
GMMVI_AD_FN Dual operator-(const Dual& a, float b) { Dual r = a; r.v = a.v - b; return r; }
GMMVI_AD_FN Dual operator-(float a, const Dual& b) { Dual r; r.v = a - b.v; GMMVI_AD_EACH r.d[j] = -b.d[j]; return r; }

GMMVI_AD_FN Dual operator*(const Dual& a, const Dual& b) {
    Dual r; r.v = a.v * b.v;
    GMMVI_AD_EACH r.d[j] = a.d[j] * b.v + a.v * b.d[j];
    return r;
}
GMMVI_AD_FN Dual operator*(const Dual& a, float b) { return chain(a.v * b, b, a); }
GMMVI_AD_FN Dual operator*(float a, const Dual& b) { return chain(a * b.v, a, b); }

GMMVI_AD_FN Dual operator/(const Dual& a, const Dual& b) {
    Dual r; r.v = a.v / b.v;
    const float inv = 1.f / b.v;
    GMMVI_AD_EACH r.d[j] = (a.d[j] - r.v * b.d[j]) * inv;
    return r;
}
GMMVI_AD_FN Dual operator/(const Dual& a, float b) { return chain(a.v / b, 1.f / b, a); }
GMMVI_AD_FN Dual operator/(float a, const Dual& b) { const float v = a / b.v; return chain(v, -v / b.v, b); }

GMMVI_AD_FN Dual& operator+=(Dual& a, const Dual& b) { a = a + b; return a; }
GMMVI_AD_FN Dual& operator+=(Dual& a, float b) { a.v += b; return a; }
GMMVI_AD_FN Dual& operator-=(Dual& a, const Dual& b) { a = a - b; return a; }
GMMVI_AD_FN Dual& operator-=(Dual& a, float b) { a.v -= b; return a; }
GMMVI_AD_FN Dual& operator*=(Dual& a, const Dual& b) { a = a * b; return a; }
GMMVI_AD_FN Dual& operator*=(Dual& a, float b) { a = a * b; return a; }
GMMVI_AD_FN Dual& operator/=(Dual& a, const Dual& b) { a = a / b; return a; }
GMMVI_AD_FN Dual& operator/=(Dual& a, float b) { a = a / b; return a; }

// ---- comparisons: on the values ------------------------------------------------------------------------------------------------
#define GMMVI_AD_COMPARE(op)                                                             \
    GMMVI_AD_FN bool operator op(const Dual& a, const Dual& b) { return a.v op b.v; }    \
    GMMVI_AD_FN bool operator op(const Dual& a, float b) { return a.v op b; }            \
    GMMVI_AD_FN bool operator op(float a, const Dual& b) { return a op b.v; }
GMMVI_AD_COMPARE(<)
GMMVI_AD_COMPARE(<=)
GMMVI_AD_COMPARE(>)
GMMVI_AD_COMPARE(>=)
GMMVI_AD_COMPARE(==)
GMMVI_AD_COMPARE(!=)
#undef GMMVI_AD_COMPARE

// ---- functions (each also under its f-suffixed name, below) ---------------------------------------------------------------------
GMMVI_AD_FN Dual exp(const Dual& a) { const float v = ::expf(a.v); return chain(v, v, a); }
GMMVI_AD_FN Dual expm1(const Dual& a) { return chain(::expm1f(a.v), ::expf(a.v), a); }
GMMVI_AD_FN Dual log(const Dual& a) { return chain(::logf(a.v), 1.f / a.v, a); }
GMMVI_AD_FN Dual log1p(const Dual& a) { return chain(::log1pf(a.v), 1.f / (1.f + a.v), a); }
GMMVI_AD_FN Dual sqrt(const Dual& a) { const float v = ::sqrtf(a.v); return chain(v, 0.5f / v, a); }
GMMVI_AD_FN Dual rsqrt(const Dual& a) { const float v = rsqrt_value(a.v); return chain(v, -0.5f * v / a.v, a); }
GMMVI_AD_FN Dual sin(const Dual& a) { return chain(::sinf(a.v), ::cosf(a.v), a); }
GMMVI_AD_FN Dual cos(const Dual& a) { return chain(::cosf(a.v), -::sinf(a.v), a); }
GMMVI_AD_FN Dual tan(const Dual& a) { const float v = ::tanf(a.v); return chain(v, 1.f + v * v, a); }
GMMVI_AD_FN Dual tanh(const Dual& a) {
    const float e = ::expf(-2.f * ::fabsf(a.v));                   // sech^2 = 4 e / (1 + e)^2: no cancellation at large |a|
    return chain(::tanhf(a.v), 4.f * e / ((1.f + e) * (1.f + e)), a);
}
GMMVI_AD_FN Dual atan(const Dual& a) { return chain(::atanf(a.v), 1.f / (1.f + a.v * a.v), a); }
GMMVI_AD_FN Dual fabs(const Dual& a) { return chain(::fabsf(a.v), a.v > 0.f ? 1.f : (a.v < 0.f ? -1.f : 0.f), a); }

// the first operand's tangent unless the second one is strictly the winner (or the first is a NaN, which fmaxf drops)
GMMVI_AD_FN Dual fmax(const Dual& a, const Dual& b) {
    const bool second = b.v > a.v || a.v != a.v;
    Dual r = second ? b : a; r.v = ::fmaxf(a.v, b.v); return r;
}
GMMVI_AD_FN Dual fmin(const Dual& a, const Dual& b) {
    const bool second = b.v < a.v || a.v != a.v;
    Dual r = second ? b : a; r.v = ::fminf(a.v, b.v); return r;
}
GMMVI_AD_FN Dual fmax(const Dual& a, float b) { return fmax(a, Dual(b)); }
GMMVI_AD_FN Dual fmax(float a, const Dual& b) { return fmax(Dual(a), b); }
GMMVI_AD_FN Dual fmin(const Dual& a, float b) { return fmin(a, Dual(b)); }
GMMVI_AD_FN Dual fmin(float a, const Dual& b) { return fmin(Dual(a), b); }

// a^b, b a constant: tangent b a^(b - 1) da, and 0 for b = 0 whatever a is
GMMVI_AD_FN Dual pow(const Dual& a, float b) {
    return chain(::powf(a.v, b), b == 0.f ? 0.f : b * ::powf(a.v, b - 1.f), a);
}
// a^b: b a^(b - 1) da + a^b ln(a) db; a direction in which b does not move takes no part of ln(a) (a <= 0 stays usable there)
GMMVI_AD_FN Dual pow(const Dual& a, const Dual& b) {
    Dual r; r.v = ::powf(a.v, b.v);
    const float da = b.v == 0.f ? 0.f : b.v * ::powf(a.v, b.v - 1.f);
    const float db = r.v * ::logf(a.v);
    GMMVI_AD_EACH r.d[j] = da * a.d[j] + (b.d[j] == 0.f ? 0.f : db * b.d[j]);
    return r;
}
GMMVI_AD_FN Dual pow(float a, const Dual& b) { return pow(Dual(a), b); }

#define GMMVI_AD_ALIAS1(name) GMMVI_AD_FN Dual name##f(const Dual& a) { return name(a); }
GMMVI_AD_ALIAS1(exp) GMMVI_AD_ALIAS1(expm1) GMMVI_AD_ALIAS1(log) GMMVI_AD_ALIAS1(log1p) GMMVI_AD_ALIAS1(sqrt) GMMVI_AD_ALIAS1(rsqrt)
GMMVI_AD_ALIAS1(sin) GMMVI_AD_ALIAS1(cos) GMMVI_AD_ALIAS1(tan) GMMVI_AD_ALIAS1(tanh) GMMVI_AD_ALIAS1(atan) GMMVI_AD_ALIAS1(fabs)
#define GMMVI_AD_ALIAS2(name)                                                              \
    GMMVI_AD_FN Dual name##f(const Dual& a, const Dual& b) { return name(a, b); }          \
    GMMVI_AD_FN Dual name##f(const Dual& a, float b) { return name(a, b); }                \
    GMMVI_AD_FN Dual name##f(float a, const Dual& b) { return name(a, b); }
GMMVI_AD_ALIAS2(fmax) GMMVI_AD_ALIAS2(fmin) GMMVI_AD_ALIAS2(pow)
#undef GMMVI_AD_ALIAS2

// ---- special functions: the float functions of custom_target_special.inc, which custom_target.hip puts in front of this text ------
// lgamma has the tangent digamma(a) da, hence NaN for a <= 0 (the value is still lgammaf's); lgammaf itself stays ROCm's float
// function and takes no dual.  gmmvi_trigamma takes no dual either: there are no second derivatives.
GMMVI_AD_FN Dual lgamma(const Dual& a) { return chain(::lgammaf(a.v), ::gmmvi_digamma(a.v), a); }
GMMVI_AD_FN Dual erf(const Dual& a) { return chain(::erff(a.v), gmmvi_special::erf_partial(a.v), a); }
GMMVI_AD_FN Dual erfc(const Dual& a) { return chain(::erfcf(a.v), -gmmvi_special::erf_partial(a.v), a); }
GMMVI_AD_FN Dual sinh(const Dual& a) { return chain(::sinhf(a.v), ::coshf(a.v), a); }
GMMVI_AD_FN Dual cosh(const Dual& a) { return chain(::coshf(a.v), ::sinhf(a.v), a); }
// tangents +-da / sqrt(1 - a^2): infinite at |a| = 1, NaN beyond
GMMVI_AD_FN Dual asin(const Dual& a) { return chain(::asinf(a.v), gmmvi_special::asin_partial(a.v), a); }
GMMVI_AD_FN Dual acos(const Dual& a) { return chain(::acosf(a.v), -gmmvi_special::asin_partial(a.v), a); }
GMMVI_AD_ALIAS1(erf) GMMVI_AD_ALIAS1(erfc) GMMVI_AD_ALIAS1(sinh) GMMVI_AD_ALIAS1(cosh) GMMVI_AD_ALIAS1(asin) GMMVI_AD_ALIAS1(acos)
#undef GMMVI_AD_ALIAS1
// gmmvi_erfcx has the tangent -inf where its value has overflowed; gmmvi_log_ndtr a finite one for every finite a
GMMVI_AD_FN Dual gmmvi_erfcx(const Dual& a) { return chain(::gmmvi_erfcx(a.v), gmmvi_special::erfcx_partial(a.v), a); }
GMMVI_AD_FN Dual gmmvi_ndtr(const Dual& a) { return chain(::gmmvi_ndtr(a.v), gmmvi_special::ndtr_partial(a.v), a); }
GMMVI_AD_FN Dual gmmvi_log_ndtr(const Dual& a) { return chain(::gmmvi_log_ndtr(a.v), gmmvi_special::log_ndtr_partial(a.v), a); }
GMMVI_AD_FN Dual gmmvi_digamma(const Dual& a) { return chain(::gmmvi_digamma(a.v), ::gmmvi_trigamma(a.v), a); }
// s sigmoid(-a), not s (1 - s), which cancels for large a
GMMVI_AD_FN Dual gmmvi_sigmoid(const Dual& a) { const float s = ::gmmvi_sigmoid(a.v); return chain(s, s * ::gmmvi_sigmoid(-a.v), a); }
GMMVI_AD_FN Dual gmmvi_softplus(const Dual& a) { return chain(::gmmvi_softplus(a.v), ::gmmvi_sigmoid(a.v), a); }
GMMVI_AD_FN Dual gmmvi_log_sigmoid(const Dual& a) { return chain(::gmmvi_log_sigmoid(a.v), ::gmmvi_sigmoid(-a.v), a); }
// tangents sigmoid(a - b) da + sigmoid(b - a) db: exactly 1/2 and 1/2 on a tie
GMMVI_AD_FN Dual gmmvi_logaddexp(const Dual& a, const Dual& b) {
    Dual r; r.v = ::gmmvi_logaddexp(a.v, b.v);
    const float pa = gmmvi_special::logaddexp_partial(a.v, b.v), pb = gmmvi_special::logaddexp_partial(b.v, a.v);
    GMMVI_AD_EACH r.d[j] = pa * a.d[j] + pb * b.d[j];
    return r;
}
GMMVI_AD_FN Dual gmmvi_logaddexp(const Dual& a, float b) {
    return chain(::gmmvi_logaddexp(a.v, b), gmmvi_special::logaddexp_partial(a.v, b), a);
}
GMMVI_AD_FN Dual gmmvi_logaddexp(float a, const Dual& b) {
    return chain(::gmmvi_logaddexp(a, b.v), gmmvi_special::logaddexp_partial(b.v, a), b);
}

GMMVI_AD_FN float gmmvi_value(const Dual& a) { return a.v; }

// What a gradient call passes as x: reading entry i builds {x[i], e_(i - first)}, so the seeded input is never stored.
struct Seed {
    const float* x;
    int first;
    GMMVI_AD_FN Dual operator[](int i) const {
        Dual r; r.v = x[i];
        GMMVI_AD_EACH r.d[j] = i - first == j ? 1.f : 0.f;
        return r;
    }
};

// ---- vector primitives on the inputs (custom_target_vector.inc has their values): tangent j is the partial derivative by
// x[x.first + j] where that index lies in [first, first + n), else 0; no loop over n carries tangents ----------------------------
GMMVI_AD_FN Dual gmmvi_dot(const Seed& x, int first, const float* c, int n) {
    Dual r; r.v = ::gmmvi_vector::dot_value(x.x + first, c, n);
    GMMVI_AD_EACH { const int k = x.first + j - first; r.d[j] = k >= 0 && k < n ? c[k] : 0.f; }
    return r;
}
GMMVI_AD_FN Dual gmmvi_sqdist(const Seed& x, int first, const float* c, int n) {
    Dual r; r.v = ::gmmvi_vector::sqdist_value(x.x + first, c, n);
    GMMVI_AD_EACH { const int k = x.first + j - first; r.d[j] = k >= 0 && k < n ? 2.f * (x.x[first + k] - c[k]) : 0.f; }
    return r;
}
GMMVI_AD_FN Dual gmmvi_sumsq(const Seed& x, int first, int n, float center) {
    Dual r; r.v = ::gmmvi_vector::sumsq_value(x.x + first, n, center);
    GMMVI_AD_EACH { const int k = x.first + j - first; r.d[j] = k >= 0 && k < n ? 2.f * (x.x[first + k] - center) : 0.f; }
    return r;
}

// ---- primitives on arrays of duals (custom_target_vector.inc has their values, from the same two templates as the float
// overloads; the user's call finds these by argument-dependent lookup on the element type).  One pass over n per call: entry i
// adds its share to all W tangents at once, by fmaf, i ascending -----------------------------------------------------------------
struct ValueAt {
    const Dual* p;
    GMMVI_AD_FN float operator()(int i) const { return p[i].v; }
};
// tangent j: sum over i of x[first + i] * h[i].d[j], and h[k].v where x[x.first + j] is x[first + k]
GMMVI_AD_FN Dual gmmvi_wdot(const Seed& x, int first, const Dual* h, int n) {
    Dual r(::gmmvi_vector::wdot_value(x.x + first, ValueAt{h}, n));
    for (int i = 0; i < n; ++i) {
        const float xi = x.x[first + i];
        GMMVI_AD_EACH r.d[j] = ::fmaf(xi, h[i].d[j], r.d[j]);
    }
    GMMVI_AD_EACH { const int k = x.first + j - first; if (k >= 0 && k < n) r.d[j] += h[k].v; }
    return r;
}
// tangent j: sum over i of p_i * a[i].d[j]; the constant -inf where the maximum is -inf
GMMVI_AD_FN Dual gmmvi_logsumexp(const Dual* a, int n) {
    float m, s;
    Dual r(::gmmvi_vector::logsumexp_value(ValueAt{a}, n, m, s));
    if (m == -__builtin_inff()) return r;
    for (int i = 0; i < n; ++i) {
        const float p = ::gmmvi_vector::logsumexp_partial(a[i].v, m, s);
        GMMVI_AD_EACH r.d[j] = ::fmaf(p, a[i].d[j], r.d[j]);
    }
    return r;
}

// ---- gmmvi_affine: out[j] = (sum over i of h[i] * x[w + i * si + j * sj]) + x[b + j * sb], j < m (custom_target_vector.inc has
// the value).  One pass over n * m.  Tangent t of out[j]: the sum over i of x[..] * h[i].d[t] by fmaf, i ascending; then h[i].v
// where the seeded input x[x.first + t] is the weight (i, j), which at most one i is (the contract: distinct (i, j) have distinct
// indices); then 1 where it is the bias of j.  The second overload takes constants for h, and only the last two terms are left.
// n <= 0: out[j] is the bias, an input, or the constant 0.
GMMVI_AD_FN void gmmvi_affine(const Seed& x, int w, int si, int sj, int b, int sb, const Dual* h, int n, Dual* out, int m) {
    for (int o = 0; o < m; ++o) {
        if (n <= 0) { out[o] = b < 0 ? Dual(0.f) : x[b + o * sb]; continue; }
        Dual r(::gmmvi_vector::affine_out(x.x, w, si, sj, b, sb, ValueAt{h}, n, o));
        float own[W];                                                   // h[i].v where tangent t is weight (i, o)'s
        GMMVI_AD_EACH own[j] = 0.f;
        for (int i = 0; i < n; ++i) {
            const int at = w + i * si + o * sj;
            const float xi = x.x[at];
            GMMVI_AD_EACH r.d[j] = ::fmaf(xi, h[i].d[j], r.d[j]);
            const int t = at - x.first;
            if (t >= 0 && t < W) { GMMVI_AD_EACH own[j] = j == t ? h[i].v : own[j]; }
        }
        const int tb = b < 0 ? -1 : b + o * sb - x.first;
        GMMVI_AD_EACH r.d[j] = (r.d[j] + own[j]) + (j == tb ? 1.f : 0.f);
        out[o] = r;
    }
}
GMMVI_AD_FN void gmmvi_affine(const Seed& x, int w, int si, int sj, int b, int sb, const float* h, int n, Dual* out, int m) {
    for (int o = 0; o < m; ++o) {
        if (n <= 0) { out[o] = b < 0 ? Dual(0.f) : x[b + o * sb]; continue; }
        Dual r(::gmmvi_vector::affine_out(x.x, w, si, sj, b, sb, ::gmmvi_vector::FloatAt{h}, n, o));
        for (int i = 0; i < n; ++i) {
            const int t = w + i * si + o * sj - x.first;
            if (t >= 0 && t < W) { GMMVI_AD_EACH r.d[j] = j == t ? h[i] : r.d[j]; }
        }
        const int tb = b < 0 ? -1 : b + o * sb - x.first;
        GMMVI_AD_EACH r.d[j] += j == tb ? 1.f : 0.f;
        out[o] = r;
    }
}

}  // namespace gmmvi_ad

// (csrc/custom_target.hip declares this one in front of the user's text as well: the user's float instantiation needs it there)
__host__ __device__ inline float gmmvi_value(float a) { return a; }

#ifndef GMMVI_AD_NO_ADAPTER
// The function of the wrapper kernels on top of the user's: values by one float instantiation; the gradient by ceil(D / W)
// passes of the dual instantiation, pass `first` carrying d / d x[first .. first + W).
__device__ __forceinline__ float gmmvi_user_target(const float* x, int D, const float* params, float* grad) {
    if (!grad) return gmmvi_user_density<float, const float*>(x, D, params);
    float value = 0.f;
    for (int first = 0; first < D; first += gmmvi_ad::W) {
        const gmmvi_ad::Dual r = gmmvi_user_density<gmmvi_ad::Dual, gmmvi_ad::Seed>(gmmvi_ad::Seed{x, first}, D, params);
        if (first == 0) value = r.v;
        _Pragma("unroll") for (int j = 0; j < gmmvi_ad::W; ++j)
            if (first + j < D) grad[first + j] = r.d[j];
    }
    return value;
}
#endif
#undef GMMVI_AD_EACH
#undef GMMVI_AD_FN
)GMMVI_AD"
