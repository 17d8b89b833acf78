// gmmvi_tape_probe (include/gmmvi_hip.h): one operation of the tape's number type (custom_target_tape.inc, its raw-string
// delimiters taken off by the Makefile, without the kernels, which need a user's function), run on a tape in host memory.  The
// operations and their order are those of autodiff_probe.hip, gmmvi_tape_probe_special's those of
// gmmvi_autodiff_probe_special, gmmvi_tape_probe_extra's those of gmmvi_autodiff_probe_extra.  Host code only.
#include "common.h"

#define GMMVI_TAPE_NO_KERNELS
#define GMMVI_TAPE_NODES 1                                       // the overloads and the sweep of the node-array record
#define GMMVI_TAPE_AFFINE 1                                      // gmmvi_affine and its branch of that sweep
#include "build/custom_target_special_text.inc"
#include "build/custom_target_tape_text.inc"

namespace {
using gmmvi_tape::Var;

Var flag(bool c) { return Var(c ? 1.f : 0.f); }

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

// what both probes report of the operation's result and of the one record it made
static int report(const Var& r, const gmmvi_tape::Rec4* rec, float* value, float* pa, float* pb, int* records) {
    *value = r.v;
    *records = gmmvi_tape::count();
    *pa = *pb = 0.f;
    // the partials of the operation's one record, by the id of the parent they belong to (a is node 0, b is node 1)
    if (*records == 1) {
        const int ids[2] = {rec[0].x, rec[0].y};
        const float partials[2] = {gmmvi_tape::bits_float(rec[0].z), gmmvi_tape::bits_float(rec[0].w)};
        for (int j = 0; j < 2; ++j) {
            if (ids[j] == 0) *pa += partials[j];
            if (ids[j] == 1) *pb += partials[j];
        }
    }
    return GMMVI_OK;
}

extern "C" int gmmvi_tape_probe(int op, float a, float b, int a_is_const, int b_is_const, float* value, float* pa, float* pb,
                                int* records) {
    if (!value || !pa || !pb || !records)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe: value, pa, pb and records must not be NULL");
    constexpr int kCap = 4;
    gmmvi_tape::Rec4 rec[kCap] = {};
    float adj[kCap] = {};
    gmmvi_tape::tape() = gmmvi_tape::Tape{(gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, kCap, 2};   // stride 1, D = 2
    gmmvi_tape::count() = 0;
    const Var A = a_is_const ? Var(a) : Var(a, 0), B = b_is_const ? Var(b) : Var(b, 1);
    Var r;
    switch (op) {
        PROBE_ARITH(+) PROBE_ARITH(-) PROBE_ARITH(*) PROBE_ARITH(/)
        case __COUNTER__ - kBase: r = -A; break;
        PROBE_COMPARE(<) PROBE_COMPARE(<=) PROBE_COMPARE(>) PROBE_COMPARE(>=) PROBE_COMPARE(==) PROBE_COMPARE(!=)
        PROBE_UNARY(exp) PROBE_UNARY(expm1) PROBE_UNARY(log) PROBE_UNARY(log1p) PROBE_UNARY(sqrt) PROBE_UNARY(rsqrt)
        PROBE_UNARY(sin) PROBE_UNARY(cos) PROBE_UNARY(tan) PROBE_UNARY(tanh) PROBE_UNARY(atan) PROBE_UNARY(fabs)
        PROBE_BINARY(fmax) PROBE_BINARY(fmin) PROBE_BINARY(pow)
        case __COUNTER__ - kBase: r = Var(gmmvi_value(A)); break;
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe: unknown operation " + std::to_string(op));
    }
    return report(r, rec, value, pa, pb, records);
}

extern "C" int gmmvi_tape_probe_special(int op, float a, float b, int a_is_const, int b_is_const, float* value, float* pa, float* pb,
                                        int* records) {
    if (!value || !pa || !pb || !records)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_special: value, pa, pb and records must not be NULL");
    constexpr int kBase = __COUNTER__ + 1;
    constexpr int kCap = 4;
    gmmvi_tape::Rec4 rec[kCap] = {};
    float adj[kCap] = {};
    gmmvi_tape::tape() = gmmvi_tape::Tape{(gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, kCap, 2};   // stride 1, D = 2
    gmmvi_tape::count() = 0;
    const Var A = a_is_const ? Var(a) : Var(a, 0), B = b_is_const ? Var(b) : Var(b, 1);
    Var r;
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
        case __COUNTER__ - kBase: r = Var(gmmvi_trigamma(a)); break;       // a float function only: a constant
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_special: unknown operation " + std::to_string(op));
    }
    return report(r, rec, value, pa, pb, records);
}

// the operations of gmmvi_autodiff_probe_extra, in its order: one operand, node 0 or a constant
extern "C" int gmmvi_tape_probe_extra(int op, float a, int a_is_const, float* value, float* pa, int* records) {
    if (!value || !pa || !records)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_extra: value, pa and records must not be NULL");
    constexpr int kBase = __COUNTER__ + 1;
    constexpr int kCap = 4;
    gmmvi_tape::Rec4 rec[kCap] = {};
    float adj[kCap] = {};
    gmmvi_tape::tape() = gmmvi_tape::Tape{(gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, kCap, 2};   // stride 1, D = 2
    gmmvi_tape::count() = 0;
    const Var A = a_is_const ? Var(a) : Var(a, 0);
    Var r;
    switch (op) {
        case __COUNTER__ - kBase: r = gmmvi_erfcx(A); break;
        case __COUNTER__ - kBase: r = gmmvi_ndtr(A); break;
        case __COUNTER__ - kBase: r = gmmvi_log_ndtr(A); break;
        PROBE_UNARY(sinh) PROBE_UNARY(cosh) PROBE_UNARY(asin) PROBE_UNARY(acos)
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_extra: unknown operation " + std::to_string(op));
    }
    float pb = 0.f;
    return report(r, rec, value, pa, &pb, records);
}

// one vector primitive on the inputs (custom_target_vector.inc and its Input overloads), in the order of _lib.VECTOR_OPS: the
// value, the record count, and the gradient [D] that gmmvi_tape::sweep, the sweep of both tape modes, leaves at stride 1
extern "C" int gmmvi_tape_probe_vector(int op, const float* x, int D, int first, int n, const float* c, float center, float* value,
                                       float* grad, int* records) {
    if (!x || !value || !grad || !records || D < 1 || first < 0 || (n > 0 && (first > D - n || (op < 2 && !c))))
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_vector: needs x, value, grad, records, D >= 1, 0 <= first, "
                                                  "first + n <= D and, for n > 0 and the first two operations, c");
    constexpr int kCap = 4;
    gmmvi_tape::Rec4 rec[kCap] = {};
    float adj[kCap] = {};
    gmmvi_tape::tape() = gmmvi_tape::Tape{(gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, kCap, D};
    gmmvi_tape::count() = 0;
    const gmmvi_tape::Input in{x};
    Var r;
    switch (op) {
        case gmmvi_vector::DOT: r = gmmvi_dot(in, first, c, n); break;
        case gmmvi_vector::SQDIST: r = gmmvi_sqdist(in, first, c, n); break;
        case gmmvi_vector::SUMSQ: r = gmmvi_sumsq(in, first, n, center); break;
        default:
            return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_vector: unknown operation " + std::to_string(op));
    }
    *value = r.v;
    *records = gmmvi_tape::count();
    for (int i = 0; i < D; ++i) grad[i] = 0.f;
    gmmvi_tape::sweep(r, D, (gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, x, grad, 1);
    return GMMVI_OK;
}

// one primitive on an array of nodes (gmmvi_wdot, gmmvi_logsumexp), in the order of _lib.NODE_OPS: the array of
// gmmvi_autodiff_probe_nodes, one tanh record per entry that is not a constant; the value, the lane's record count (those
// records and the 1 + ceil(n / 2) slots of the node-array record), and the gradient [D] that gmmvi_tape::sweep leaves at stride 1
extern "C" int gmmvi_tape_probe_nodes(int op, const float* x, int D, int first, int n, int src, int every, float* value, float* grad,
                                      int* records) {
    constexpr int kMax = 64;
    if (!x || !value || !grad || !records || op < 0 || op > gmmvi_vector::LOGSUMEXP || D < 1 || first < 0 || n < 0 || src < 0 ||
        every < 0 || n > kMax || src > D - n || first > D - n)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_nodes: needs a known operation, x, value, grad, records, D >= 1, "
                                                  "0 <= n <= 64, 0 <= first, 0 <= src, 0 <= every, first + n <= D and src + n <= D");
    constexpr int kCap = kMax + 1 + kMax / 2;                       // a record per entry, the header and its payload
    gmmvi_tape::Rec4 rec[kCap] = {};
    float adj[kCap] = {};
    gmmvi_tape::tape() = gmmvi_tape::Tape{(gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, kCap, D};
    gmmvi_tape::count() = 0;
    const gmmvi_tape::Input in{x};
    Var h[kMax];
    for (int i = 0; i < n; ++i)
        h[i] = every > 0 && i % every == every - 1 ? Var(::tanhf(x[src + i])) : tanh(in[src + i]);
    const Var r = op == gmmvi_vector::WDOT ? gmmvi_wdot(in, first, h, n) : gmmvi_logsumexp(h, n);
    *value = r.v;
    *records = gmmvi_tape::count();
    for (int i = 0; i < D; ++i) grad[i] = 0.f;
    gmmvi_tape::sweep(r, D, (gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, x, grad, 1);
    return GMMVI_OK;
}

// the same call on an array whose entries are the input nodes themselves, h[i] = x[src + i] (no record of their own): the
// gradient of gmmvi_logsumexp is then its partials p_i bit for bit, and x may hold -inf
extern "C" int gmmvi_tape_probe_nodes_inputs(int op, const float* x, int D, int first, int n, int src, float* value, float* grad,
                                             int* records) {
    constexpr int kMax = 64;
    if (!x || !value || !grad || !records || op < 0 || op > gmmvi_vector::LOGSUMEXP || D < 1 || first < 0 || n < 0 || src < 0 ||
        n > kMax || src > D - n || first > D - n)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_nodes_inputs: needs a known operation, x, value, grad, records, "
                                                  "D >= 1, 0 <= n <= 64, 0 <= first, 0 <= src, first + n <= D and src + n <= D");
    constexpr int kCap = 1 + kMax / 2;
    gmmvi_tape::Rec4 rec[kCap] = {};
    float adj[kCap] = {};
    gmmvi_tape::tape() = gmmvi_tape::Tape{(gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, kCap, D};
    gmmvi_tape::count() = 0;
    const gmmvi_tape::Input in{x};
    Var h[kMax];
    for (int i = 0; i < n; ++i) h[i] = in[src + i];
    const Var r = op == gmmvi_vector::WDOT ? gmmvi_wdot(in, first, h, n) : gmmvi_logsumexp(h, n);
    *value = r.v;
    *records = gmmvi_tape::count();
    for (int i = 0; i < D; ++i) grad[i] = 0.f;
    gmmvi_tape::sweep(r, D, (gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, x, grad, 1);
    return GMMVI_OK;
}

// one gmmvi_affine call on a tape: the arguments, the array and the output of gmmvi_autodiff_probe_affine (an entry that is not a
// constant is one tanh record; with `inputs` or `floats` the entries make no record).  values[j] = out[j]; *records is the lane's
// count behind the gmmvi_affine call, in front of the gmmvi_logsumexp of pick == -1; grad [D] is what gmmvi_tape::sweep leaves at
// stride 1, entering the group at header `pick`, or at header m - 1 from the record of the gmmvi_logsumexp
extern "C" int gmmvi_tape_probe_affine(const float* x, int D, int w, int si, int sj, int b, int sb, int n, int m, int src, int every,
                                       int inputs, int floats, int pick, float* values, float* value, float* grad, int* records) {
    constexpr int kMax = 64;
    if (!x || !values || !value || !grad || !records || D < 1 || n < 0 || m < 0 || n > kMax || m > kMax || w < 0 || si < 1 || sj < 1 ||
        src < 0 || every < 0 || src > D - n || pick < -1 || pick >= (m > 0 ? m : 1) ||
        (n > 0 && m > 0 && (long long)w + (long long)(n - 1) * si + (long long)(m - 1) * sj >= D) ||
        (b >= 0 && (sb < 1 || (m > 0 && (long long)b + (long long)(m - 1) * sb >= D))))
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "gmmvi_tape_probe_affine: needs x, values, value, grad, records, D >= 1, 0 <= n <= 64, "
                                                  "0 <= m <= 64, 0 <= w, 1 <= si, 1 <= sj, 1 <= sb with a bias, 0 <= src, 0 <= every, "
                                                  "src + n <= D, every weight and bias index below D and -1 <= pick < max(m, 1)");
    // a record per entry, the group's payload, descriptors and headers, the gmmvi_logsumexp of the outputs
    constexpr int kCap = kMax + (kMax / 2 + 2 + kMax) + (kMax / 2 + 1);
    gmmvi_tape::Rec4 rec[kCap] = {};
    float adj[kCap] = {};
    gmmvi_tape::tape() = gmmvi_tape::Tape{(gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, kCap, D};
    gmmvi_tape::count() = 0;
    const gmmvi_tape::Input in{x};
    Var h[kMax], out[kMax];
    float hf[kMax];
    for (int i = 0; i < n; ++i) {
        hf[i] = inputs ? x[src + i] : ::tanhf(x[src + i]);
        if (floats) continue;
        if (inputs) h[i] = in[src + i];
        else h[i] = every > 0 && i % every == every - 1 ? Var(hf[i]) : tanh(in[src + i]);
    }
    if (floats) gmmvi_affine(in, w, si, sj, b, sb, (const float*)hf, n, out, m);
    else gmmvi_affine(in, w, si, sj, b, sb, (const Var*)h, n, out, m);
    *records = gmmvi_tape::count();
    for (int j = 0; j < m; ++j) values[j] = out[j].v;
    const Var r = m == 0 ? Var(0.f) : (pick >= 0 ? out[pick] : gmmvi_logsumexp(out, m));
    *value = r.v;
    for (int i = 0; i < D; ++i) grad[i] = 0.f;
    gmmvi_tape::sweep(r, D, (gmmvi_tape::RecPtr)rec, (gmmvi_tape::AdjPtr)adj, 1, x, grad, 1);
    return GMMVI_OK;
}
