// gmmvi_autodiff_probe (include/gmmvi_hip.h): one operation of the dual-number text of differentiated user-defined targets,
// evaluated on the host; gmmvi_autodiff_probe_special and gmmvi_autodiff_probe_extra: the same for its special functions, two
// lists of their own (the second one the normal distribution's functions and sinh, cosh, asin, acos).  The text is
// the one the run-time compiler gets (custom_target_special.inc and custom_target_autodiff.inc, their raw-string delimiters
// taken off by the Makefile), without the adapter, which needs a user's function.  Host code only.
#include "common.h"

#define GMMVI_AD_NO_ADAPTER
#include "build/custom_target_special_text.inc"
#include "build/custom_target_autodiff_text.inc"

namespace {
using gmmvi_ad::Dual;

Dual flag(bool c) { return Dual(c ? 1.f : 0.f); }

// the three operand forms of a binary operation and (ASSIGN) its compound forms, in the order of _lib.AUTODIFF_OPS
#define PROBE_ARITH(op)                                         \
    case __COUNTER__ - kBase: r = A op B; break;                \
    case __COUNTER__ - kBase: r = A op b; break;                \
    case __COUNTER__ - kBase: r = a op B; break;                \
    case __COUNTER__ - kBase: r = A; r op## = B; break;         \
    case __COUNTER__ - kBase: r = A; r op## = b; break;
#define PROBE_COMPARE(op)                                       \
    case __COUNTER__ - kBase: r = flag(A op B); break;          \
    case __COUNTER__ - kBase: r = flag(A op b); break;          \
    case __COUNTER__ - kBase: r = flag(a op B); break;
#define PROBE_UNARY(fn)                                         \
    case __COUNTER__ - kBase: r = fn(A); break;                 \
    case __COUNTER__ - kBase: r = fn##f(A); break;
#define PROBE_BINARY(fn)                                        \
    case __COUNTER__ - kBase: r = fn(A, B); break;              \
    case __COUNTER__ - kBase: r = fn(A, b); break;              \
    case __COUNTER__ - kBase: r = fn(a, B); break;              \
    case __COUNTER__ - kBase: r = fn##f(A, B); break;           \
    case __COUNTER__ - kBase: r = fn##f(A, b); break;           \
    case __COUNTER__ - kBase: r = fn##f(a, B); break;

constexpr int kBase = __COUNTER__ + 1;
}  // namespace

extern "C" int gmmvi_autodiff_probe(int op, float a, float da, float b, float db, float* value, float* tangent) {
    if (!value || !tangent) return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe: value and tangent must not be NULL");
    Dual A(a), B(b), r;
    A.d[0] = da;
    B.d[0] = db;
    switch (op) {
        PROBE_ARITH(+) PROBE_ARITH(-) PROBE_ARITH(*) PROBE_ARITH(/)
        case __COUNTER__ - kBase: r = -A; break;
        PROBE_COMPARE(<) PROBE_COMPARE(<=) PROBE_COMPARE(>) PROBE_COMPARE(>=) PROBE_COMPARE(==) PROBE_COMPARE(!=)
        PROBE_UNARY(exp) PROBE_UNARY(expm1) PROBE_UNARY(log) PROBE_UNARY(log1p) PROBE_UNARY(sqrt) PROBE_UNARY(rsqrt)
        PROBE_UNARY(sin) PROBE_UNARY(cos) PROBE_UNARY(tan) PROBE_UNARY(tanh) PROBE_UNARY(atan) PROBE_UNARY(fabs)
        PROBE_BINARY(fmax) PROBE_BINARY(fmin) PROBE_BINARY(pow)
        case __COUNTER__ - kBase: r = Dual(gmmvi_value(A)); break;
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe: unknown operation " + std::to_string(op));
    }
    *value = r.v;
    *tangent = r.d[0];
    return GMMVI_OK;
}

// the special functions (custom_target_special.inc and their rules in the dual-number text), in the order of _lib.SPECIAL_OPS
extern "C" int gmmvi_autodiff_probe_special(int op, float a, float da, float b, float db, float* value, float* tangent) {
    if (!value || !tangent)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_special: value and tangent must not be NULL");
    constexpr int kBase = __COUNTER__ + 1;
    Dual A(a), B(b), r;
    A.d[0] = da;
    B.d[0] = db;
    switch (op) {
        case __COUNTER__ - kBase: r = lgamma(A); break;                    // lgammaf stays a float function
        PROBE_UNARY(erf) PROBE_UNARY(erfc)
        case __COUNTER__ - kBase: r = gmmvi_digamma(A); break;
        case __COUNTER__ - kBase: r = gmmvi_sigmoid(A); break;
        case __COUNTER__ - kBase: r = gmmvi_softplus(A); break;
        case __COUNTER__ - kBase: r = gmmvi_log_sigmoid(A); break;
        case __COUNTER__ - kBase: r = gmmvi_logaddexp(A, B); break;
        case __COUNTER__ - kBase: r = gmmvi_logaddexp(A, b); break;
        case __COUNTER__ - kBase: r = gmmvi_logaddexp(a, B); break;
        case __COUNTER__ - kBase: r = Dual(gmmvi_trigamma(a)); break;      // a float function only: a constant
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_special: unknown operation " + std::to_string(op));
    }
    *value = r.v;
    *tangent = r.d[0];
    return GMMVI_OK;
}

// the normal distribution's functions and the four elementary ones that came with them, in the order of _lib.EXTRA_OPS
extern "C" int gmmvi_autodiff_probe_extra(int op, float a, float da, float* value, float* tangent) {
    if (!value || !tangent)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_extra: value and tangent must not be NULL");
    constexpr int kBase = __COUNTER__ + 1;
    Dual A(a), r;
    A.d[0] = da;
    switch (op) {
        case __COUNTER__ - kBase: r = gmmvi_erfcx(A); break;
        case __COUNTER__ - kBase: r = gmmvi_ndtr(A); break;
        case __COUNTER__ - kBase: r = gmmvi_log_ndtr(A); break;
        PROBE_UNARY(sinh) PROBE_UNARY(cosh) PROBE_UNARY(asin) PROBE_UNARY(acos)
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_extra: unknown operation " + std::to_string(op));
    }
    *value = r.v;
    *tangent = r.d[0];
    return GMMVI_OK;
}

// one vector primitive on the inputs (custom_target_vector.inc and its Seed overloads), in the order of _lib.VECTOR_OPS, in the
// pass seeded at `seed_first`: tangents[j] is the partial derivative by x[seed_first + j]
extern "C" int gmmvi_autodiff_probe_vector(int op, const float* x, int D, int first, int n, const float* c, float center,
                                           int seed_first, float* value, float* tangents) {
    if (!x || !value || !tangents || D < 1 || first < 0 || seed_first < 0 || (n > 0 && (first > D - n || (op < 2 && !c))))
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_vector: needs x, value, tangents, D >= 1, seed_first >= 0, "
                                                  "0 <= first, first + n <= D and, for n > 0 and the first two operations, c");
    const gmmvi_ad::Seed seed{x, seed_first};
    Dual r;
    switch (op) {
        case gmmvi_vector::DOT: r = gmmvi_dot(seed, first, c, n); break;
        case gmmvi_vector::SQDIST: r = gmmvi_sqdist(seed, first, c, n); break;
        case gmmvi_vector::SUMSQ: r = gmmvi_sumsq(seed, first, n, center); break;
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_vector: unknown operation " + std::to_string(op));
    }
    *value = r.v;
    for (int j = 0; j < gmmvi_ad::W; ++j) tangents[j] = r.d[j];
    return GMMVI_OK;
}

// one primitive on an array of duals (gmmvi_wdot, gmmvi_logsumexp), in the order of _lib.NODE_OPS, in the pass seeded at
// `seed_first`: the array is h[i] = tanh(x[src + i]), i < n, with every `every`-th entry (i % every == every - 1) the constant
// tanhf(x[src + i]) instead; tangents[j] is the derivative by x[seed_first + j]
extern "C" int gmmvi_autodiff_probe_nodes(int op, const float* x, int D, int first, int n, int src, int every, int seed_first,
                                          float* value, float* tangents) {
    constexpr int kMax = 64;
    if (!x || !value || !tangents || op < 0 || op > gmmvi_vector::LOGSUMEXP || D < 1 || first < 0 || n < 0 || src < 0 || every < 0 ||
        seed_first < 0 || n > kMax || src > D - n || first > D - n)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_nodes: needs a known operation, x, value, tangents, D >= 1, "
                                                  "0 <= n <= 64, 0 <= first, 0 <= src, 0 <= every, 0 <= seed_first, "
                                                  "first + n <= D and src + n <= D");
    const gmmvi_ad::Seed seed{x, seed_first};
    Dual h[kMax];
    for (int i = 0; i < n; ++i)
        h[i] = every > 0 && i % every == every - 1 ? Dual(::tanhf(x[src + i])) : tanh(seed[src + i]);
    const Dual r = op == gmmvi_vector::WDOT ? gmmvi_wdot(seed, first, h, n) : gmmvi_logsumexp(h, n);
    *value = r.v;
    for (int j = 0; j < gmmvi_ad::W; ++j) tangents[j] = r.d[j];
    return GMMVI_OK;
}

// the same call on an array whose entries are the inputs themselves, h[i] = x[src + i]: the tangents of gmmvi_logsumexp are then
// its partials p_i bit for bit, and x may hold -inf (an array of -inf is the constant -inf)
extern "C" int gmmvi_autodiff_probe_nodes_inputs(int op, const float* x, int D, int first, int n, int src, int seed_first,
                                                 float* value, float* tangents) {
    constexpr int kMax = 64;
    if (!x || !value || !tangents || op < 0 || op > gmmvi_vector::LOGSUMEXP || D < 1 || first < 0 || n < 0 || src < 0 ||
        seed_first < 0 || n > kMax || src > D - n || first > D - n)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_nodes_inputs: needs a known operation, x, value, tangents, "
                                                  "D >= 1, 0 <= n <= 64, 0 <= first, 0 <= src, 0 <= seed_first, first + n <= D and "
                                                  "src + n <= D");
    const gmmvi_ad::Seed seed{x, seed_first};
    Dual h[kMax];
    for (int i = 0; i < n; ++i) h[i] = seed[src + i];
    const Dual r = op == gmmvi_vector::WDOT ? gmmvi_wdot(seed, first, h, n) : gmmvi_logsumexp(h, n);
    *value = r.v;
    for (int j = 0; j < gmmvi_ad::W; ++j) tangents[j] = r.d[j];
    return GMMVI_OK;
}

// one gmmvi_affine call in the pass seeded at `seed_first`: the array of gmmvi_autodiff_probe_nodes (h[i] = tanh(x[src + i]), every
// `every`-th entry a constant), or with `inputs` the inputs themselves (h[i] = x[src + i]), or with `floats` the same values as a
// const float* (the overload that takes constants).  values[j] = out[j], j < m; the output is out[pick], or with pick == -1
// gmmvi_logsumexp(out, m), which consumes every output; tangents[t] is its derivative by x[seed_first + t].  Distinct (i, j)
// with distinct indices w + i si + j sj stay the caller's duty, as in the primitive's contract.
extern "C" int gmmvi_autodiff_probe_affine(const float* x, int D, int w, int si, int sj, int b, int sb, int n, int m, int src, int every,
                                           int inputs, int floats, int pick, int seed_first, float* values, float* value,
                                           float* tangents) {
    constexpr int kMax = 64;
    if (!x || !values || !value || !tangents || D < 1 || n < 0 || m < 0 || n > kMax || m > kMax || w < 0 || si < 1 || sj < 1 ||
        src < 0 || every < 0 || seed_first < 0 || src > D - n || pick < -1 || pick >= (m > 0 ? m : 1) ||
        (n > 0 && m > 0 && (long long)w + (long long)(n - 1) * si + (long long)(m - 1) * sj >= D) ||
        (b >= 0 && (sb < 1 || (m > 0 && (long long)b + (long long)(m - 1) * sb >= D))))
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_autodiff_probe_affine: needs x, values, value, tangents, D >= 1, 0 <= n <= 64, "
                                                  "0 <= m <= 64, 0 <= w, 1 <= si, 1 <= sj, 1 <= sb with a bias, 0 <= src, 0 <= every, "
                                                  "0 <= seed_first, src + n <= D, every weight and bias index below D and "
                                                  "-1 <= pick < max(m, 1)");
    const gmmvi_ad::Seed seed{x, seed_first};
    Dual h[kMax], out[kMax];
    float hf[kMax];
    for (int i = 0; i < n; ++i) {
        hf[i] = inputs ? x[src + i] : ::tanhf(x[src + i]);
        if (inputs) h[i] = seed[src + i];
        else h[i] = every > 0 && i % every == every - 1 ? Dual(hf[i]) : tanh(seed[src + i]);
    }
    if (floats) gmmvi_affine(seed, w, si, sj, b, sb, (const float*)hf, n, out, m);
    else gmmvi_affine(seed, w, si, sj, b, sb, (const Dual*)h, n, out, m);
    for (int j = 0; j < m; ++j) values[j] = out[j].v;
    const Dual r = m == 0 ? Dual(0.f) : (pick >= 0 ? out[pick] : gmmvi_logsumexp(out, m));
    *value = r.v;
    for (int t = 0; t < gmmvi_ad::W; ++t) tangents[t] = r.d[t];
    return GMMVI_OK;
}
