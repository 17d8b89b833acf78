// gmmvi_autodiff_probe (include/gmmvi_hip.h): one operation of the dual-number text of differentiated user-defined targets,
// evaluated on the host.  The text is the one the run-time compiler gets (custom_target_autodiff.inc, its raw-string
// delimiters taken off by the Makefile), without the adapter, which needs a user's function.  Host code only.
#include "common.h"

#define GMMVI_AD_NO_ADAPTER
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
