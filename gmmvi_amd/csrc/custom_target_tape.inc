R"GMMVI_TAPE(
// ---- reverse-mode differentiation of a user-defined density on a tape (csrc/custom_target.hip puts this text behind the user's
// source; contract: include/gmmvi_hip.h, "differentiated user-defined targets on a tape") ------------------------------------------
// The text above defines   template <class T, class X> __device__ T gmmvi_user_density(X x, int D, const float* params);
// the text of the forward mode, unchanged.  This text defines the number the library instantiates T with on a gradient call (a
// value and the id of a node), the view X whose entries are the input nodes, and the kernels: one lane is one sample, records
// its evaluation and walks its own records back in the same launch.
//
// Node ids: id < 0 a constant; 0 <= id < D the input x[id]; id >= D record id - D.  A record is {ia, ib, pa, pb}: the ids of
// the parents and the partial derivatives of the node by them (ib = -1: one parent; a constant parent keeps its negative id
// and takes no part in the sweep).  ia <= -2 marks a vector record, the one node of a gmmvi_dot, gmmvi_sqdist or gmmvi_sumsq
// call on the inputs (custom_target_vector.inc): ia = -2 - (4 n + kind), ib = first, and {pa, pb} hold the 64-bit address of
// c, or the bits of center in pa.  Kind 3 is the node-array record of gmmvi_wdot and gmmvi_logsumexp, a header behind
// ceil(n / 2) payload slots ("primitives on arrays of nodes", below), and of gmmvi_affine, m headers behind one payload and two
// descriptor slots ("gmmvi_affine", below).  Record r of lane l lies at rec[r * stride + l], its
// adjoint at adj[r * stride + l]: on the device stride = 64, a wave's record r is 1 KiB of consecutive memory and every access
// below is an ordinary per-lane vector load or store; on the host (csrc/tape_probe.hip) stride = 1 and l = 0.
// The partial derivatives and the tie rules are those of the forward mode (custom_target_autodiff.inc): fabs has partial 0 at
// +-0; fmax and fmin give the first operand the partial 1 on a tie; comparisons look at the values only; pow with exponent 0
// has partial 0 by the base; a constant exponent takes no part of ln(a).  An operation whose operands are all constants makes no
// record.  There is no conversion from a Var to float: gmmvi_value(t) is the only way down.

namespace gmmvi_tape {

#define GMMVI_TAPE_FN __host__ __device__ __forceinline__

#if defined(__HIP_DEVICE_COMPILE__)
#define GMMVI_TAPE_GLOBAL __attribute__((address_space(1)))      // tape traffic is global memory: it cannot alias the LDS state below
#else
#define GMMVI_TAPE_GLOBAL
#endif
typedef int Rec4 __attribute__((ext_vector_type(4)));             // one record as it is stored: {ia, ib, bits of pa, bits of pb}
typedef GMMVI_TAPE_GLOBAL Rec4* RecPtr;
typedef GMMVI_TAPE_GLOBAL float* AdjPtr;

struct Tape {
    RecPtr rec;          // record 0 of lane 0
    AdjPtr adj;          // adjoint slot 0 of lane 0
    int stride;          // lanes per record row
    int cap;             // records a lane may store
    int D;               // ids below D are inputs
};

// The tape the operations below write to, and the lane's count of records made so far.  Device: the wave's tape is wave-uniform
// state in LDS, set by the kernel before the user's function runs; the count is the lane's own LDS word, which the compiler
// keeps in a register between the records of straight-line code (nothing else can write it).  Host: one tape per thread.
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ Tape& tape() { __shared__ Tape t; return t; }
__device__ __forceinline__ int lane() { return (int)threadIdx.x; }
__device__ __forceinline__ int& count() { __shared__ int c[64]; return c[threadIdx.x]; }
GMMVI_TAPE_FN float rsqrt_value(float a) { return ::rsqrtf(a); }
#else
inline Tape& tape() { static thread_local Tape t; return t; }
inline int lane() { return 0; }
inline int& count() { static thread_local int c; return c; }
GMMVI_TAPE_FN float rsqrt_value(float a) { return 1.f / ::sqrtf(a); }
#endif

GMMVI_TAPE_FN int float_bits(float f) { union { float f; int i; } u; u.f = f; return u.i; }
GMMVI_TAPE_FN float bits_float(int i) { union { float f; int i; } u; u.i = i; return u.f; }

// Appends {ia, ib, z, w} and zeroes the record's adjoint; -> the id of the new node.  Beyond the capacity nothing is stored,
// the count still advances: the values stay right and the lane knows how long its tape would have been.
GMMVI_TAPE_FN int push_bits(int ia, int ib, int z, int w) {
    const Tape& t = tape();
    int& c = count();
    const int r = c;
    if (r < t.cap) {
        const size_t at = (size_t)r * (size_t)t.stride + (size_t)lane();
        Rec4 v; v.x = ia; v.y = ib; v.z = z; v.w = w;
        t.rec[at] = v;                                                  // one 16-byte store
        t.adj[at] = 0.f;
    }
    c = r + 1;
    return t.D + r;
}
GMMVI_TAPE_FN int push(int ia, int ib, float pa, float pb) { return push_bits(ia, ib, float_bits(pa), float_bits(pb)); }

struct Var {
    float v;
    int id;
    Var() = default;
    GMMVI_TAPE_FN Var(float value) : v(value), id(-1) {}                // a constant
    GMMVI_TAPE_FN Var(float value, int node) : v(value), id(node) {}
};

// value `v` with one parent / two parents; all parents constants: a constant
GMMVI_TAPE_FN Var node(float v, const Var& a, float pa) { return a.id < 0 ? Var(v) : Var(v, push(a.id, -1, pa, 0.f)); }
GMMVI_TAPE_FN Var node(float v, const Var& a, float pa, const Var& b, float pb) {
    if (a.id < 0 && b.id < 0) return Var(v);
    return Var(v, push(a.id, b.id, a.id < 0 ? 0.f : pa, b.id < 0 ? 0.f : pb));
}

// ---- arithmetic ------------------------------------------------------------------------------------------------------------
GMMVI_TAPE_FN Var operator-(const Var& a) { return node(-a.v, a, -1.f); }
GMMVI_TAPE_FN Var operator+(const Var& a) { return a; }

GMMVI_TAPE_FN Var operator+(const Var& a, const Var& b) { return node(a.v + b.v, a, 1.f, b, 1.f); }
GMMVI_TAPE_FN Var operator+(const Var& a, float b) { return node(a.v + b, a, 1.f); }
GMMVI_TAPE_FN Var operator+(float a, const Var& b) { return node(a + b.v, b, 1.f); }

GMMVI_TAPE_FN Var operator-(const Var& a, const Var& b) { return node(a.v - b.v, a, 1.f, b, -1.f); }
GMMVI_TAPE_FN Var operator-(const Var& a, float b) { return node(a.v - b, a, 1.f); }
GMMVI_TAPE_FN Var operator-(float a, const Var& b) { return node(a - b.v, b, -1.f); }

GMMVI_TAPE_FN Var operator*(const Var& a, const Var& b) { return node(a.v * b.v, a, b.v, b, a.v); }
GMMVI_TAPE_FN Var operator*(const Var& a, float b) { return node(a.v * b, a, b); }
GMMVI_TAPE_FN Var operator*(float a, const Var& b) { return node(a * b.v, b, a); }

GMMVI_TAPE_FN Var operator/(const Var& a, const Var& b) {
    const float v = a.v / b.v, inv = 1.f / b.v;
    return node(v, a, inv, b, -v * inv);
}
GMMVI_TAPE_FN Var operator/(const Var& a, float b) { return node(a.v / b, a, 1.f / b); }
GMMVI_TAPE_FN Var operator/(float a, const Var& b) { const float v = a / b.v; return node(v, b, -v / b.v); }

GMMVI_TAPE_FN Var& operator+=(Var& a, const Var& b) { a = a + b; return a; }
GMMVI_TAPE_FN Var& operator+=(Var& a, float b) { a = a + b; return a; }
GMMVI_TAPE_FN Var& operator-=(Var& a, const Var& b) { a = a - b; return a; }
GMMVI_TAPE_FN Var& operator-=(Var& a, float b) { a = a - b; return a; }
GMMVI_TAPE_FN Var& operator*=(Var& a, const Var& b) { a = a * b; return a; }
GMMVI_TAPE_FN Var& operator*=(Var& a, float b) { a = a * b; return a; }
GMMVI_TAPE_FN Var& operator/=(Var& a, const Var& b) { a = a / b; return a; }
GMMVI_TAPE_FN Var& operator/=(Var& a, float b) { a = a / b; return a; }

// ---- comparisons: on the values, no record ---------------------------------------------------------------------------------------
#define GMMVI_TAPE_COMPARE(op)                                                          \
    GMMVI_TAPE_FN bool operator op(const Var& a, const Var& b) { return a.v op b.v; }   \
    GMMVI_TAPE_FN bool operator op(const Var& a, float b) { return a.v op b; }          \
    GMMVI_TAPE_FN bool operator op(float a, const Var& b) { return a op b.v; }
GMMVI_TAPE_COMPARE(<)
GMMVI_TAPE_COMPARE(<=)
GMMVI_TAPE_COMPARE(>)
GMMVI_TAPE_COMPARE(>=)
GMMVI_TAPE_COMPARE(==)
GMMVI_TAPE_COMPARE(!=)
#undef GMMVI_TAPE_COMPARE

// ---- functions (each also under its f-suffixed name, below) ---------------------------------------------------------------------
GMMVI_TAPE_FN Var exp(const Var& a) { const float v = ::expf(a.v); return node(v, a, v); }
GMMVI_TAPE_FN Var expm1(const Var& a) { return node(::expm1f(a.v), a, ::expf(a.v)); }
GMMVI_TAPE_FN Var log(const Var& a) { return node(::logf(a.v), a, 1.f / a.v); }
GMMVI_TAPE_FN Var log1p(const Var& a) { return node(::log1pf(a.v), a, 1.f / (1.f + a.v)); }
GMMVI_TAPE_FN Var sqrt(const Var& a) { const float v = ::sqrtf(a.v); return node(v, a, 0.5f / v); }
GMMVI_TAPE_FN Var rsqrt(const Var& a) { const float v = rsqrt_value(a.v); return node(v, a, -0.5f * v / a.v); }
GMMVI_TAPE_FN Var sin(const Var& a) { return node(::sinf(a.v), a, ::cosf(a.v)); }
GMMVI_TAPE_FN Var cos(const Var& a) { return node(::cosf(a.v), a, -::sinf(a.v)); }
GMMVI_TAPE_FN Var tan(const Var& a) { const float v = ::tanf(a.v); return node(v, a, 1.f + v * v); }
GMMVI_TAPE_FN Var tanh(const Var& a) {
    const float e = ::expf(-2.f * ::fabsf(a.v));                   // sech^2 = 4 e / (1 + e)^2: no cancellation at large |a|
    return node(::tanhf(a.v), a, 4.f * e / ((1.f + e) * (1.f + e)));
}
GMMVI_TAPE_FN Var atan(const Var& a) { return node(::atanf(a.v), a, 1.f / (1.f + a.v * a.v)); }
GMMVI_TAPE_FN Var fabs(const Var& a) { return node(::fabsf(a.v), a, a.v > 0.f ? 1.f : (a.v < 0.f ? -1.f : 0.f)); }

// the first operand takes the partial 1 unless the second one is strictly the winner (or the first is a NaN, which fmaxf drops)
GMMVI_TAPE_FN Var fmax(const Var& a, const Var& b) {
    const bool second = b.v > a.v || a.v != a.v;
    return node(::fmaxf(a.v, b.v), a, second ? 0.f : 1.f, b, second ? 1.f : 0.f);
}
GMMVI_TAPE_FN Var fmin(const Var& a, const Var& b) {
    const bool second = b.v < a.v || a.v != a.v;
    return node(::fminf(a.v, b.v), a, second ? 0.f : 1.f, b, second ? 1.f : 0.f);
}
GMMVI_TAPE_FN Var fmax(const Var& a, float b) { return fmax(a, Var(b)); }
GMMVI_TAPE_FN Var fmax(float a, const Var& b) { return fmax(Var(a), b); }
GMMVI_TAPE_FN Var fmin(const Var& a, float b) { return fmin(a, Var(b)); }
GMMVI_TAPE_FN Var fmin(float a, const Var& b) { return fmin(Var(a), b); }

// a^b, b a float: partial b a^(b - 1), and 0 for b = 0 whatever a is
GMMVI_TAPE_FN Var pow(const Var& a, float b) { return node(::powf(a.v, b), a, b == 0.f ? 0.f : b * ::powf(a.v, b - 1.f)); }
// a^b: partials b a^(b - 1) and a^b ln(a); a constant exponent takes no part of ln(a) (a <= 0 stays usable there)
GMMVI_TAPE_FN Var pow(const Var& a, const Var& b) {
    const float v = ::powf(a.v, b.v);
    const float da = a.id < 0 || b.v == 0.f ? 0.f : b.v * ::powf(a.v, b.v - 1.f);
    const float db = b.id < 0 ? 0.f : v * ::logf(a.v);
    return node(v, a, da, b, db);
}
GMMVI_TAPE_FN Var pow(float a, const Var& b) { return pow(Var(a), b); }

#define GMMVI_TAPE_ALIAS1(name) GMMVI_TAPE_FN Var name##f(const Var& a) { return name(a); }
GMMVI_TAPE_ALIAS1(exp) GMMVI_TAPE_ALIAS1(expm1) GMMVI_TAPE_ALIAS1(log) GMMVI_TAPE_ALIAS1(log1p) GMMVI_TAPE_ALIAS1(sqrt)
GMMVI_TAPE_ALIAS1(rsqrt) GMMVI_TAPE_ALIAS1(sin) GMMVI_TAPE_ALIAS1(cos) GMMVI_TAPE_ALIAS1(tan) GMMVI_TAPE_ALIAS1(tanh)
GMMVI_TAPE_ALIAS1(atan) GMMVI_TAPE_ALIAS1(fabs)
#define GMMVI_TAPE_ALIAS2(name)                                                          \
    GMMVI_TAPE_FN Var name##f(const Var& a, const Var& b) { return name(a, b); }         \
    GMMVI_TAPE_FN Var name##f(const Var& a, float b) { return name(a, b); }              \
    GMMVI_TAPE_FN Var name##f(float a, const Var& b) { return name(a, b); }
GMMVI_TAPE_ALIAS2(fmax) GMMVI_TAPE_ALIAS2(fmin) GMMVI_TAPE_ALIAS2(pow)
#undef GMMVI_TAPE_ALIAS2

// ---- special functions: the float functions of custom_target_special.inc, which custom_target.hip puts in front of this text; one
// record per call, the partials of the forward mode (lgamma: digamma(a), NaN for a <= 0; gmmvi_logaddexp: 1/2 and 1/2 on a tie) -----
GMMVI_TAPE_FN Var lgamma(const Var& a) { return node(::lgammaf(a.v), a, ::gmmvi_digamma(a.v)); }
GMMVI_TAPE_FN Var erf(const Var& a) { return node(::erff(a.v), a, gmmvi_special::erf_partial(a.v)); }
GMMVI_TAPE_FN Var erfc(const Var& a) { return node(::erfcf(a.v), a, -gmmvi_special::erf_partial(a.v)); }
GMMVI_TAPE_FN Var sinh(const Var& a) { return node(::sinhf(a.v), a, ::coshf(a.v)); }
GMMVI_TAPE_FN Var cosh(const Var& a) { return node(::coshf(a.v), a, ::sinhf(a.v)); }
GMMVI_TAPE_FN Var asin(const Var& a) { return node(::asinf(a.v), a, gmmvi_special::asin_partial(a.v)); }
GMMVI_TAPE_FN Var acos(const Var& a) { return node(::acosf(a.v), a, -gmmvi_special::asin_partial(a.v)); }
GMMVI_TAPE_ALIAS1(erf) GMMVI_TAPE_ALIAS1(erfc) GMMVI_TAPE_ALIAS1(sinh) GMMVI_TAPE_ALIAS1(cosh) GMMVI_TAPE_ALIAS1(asin)
GMMVI_TAPE_ALIAS1(acos)
#undef GMMVI_TAPE_ALIAS1
GMMVI_TAPE_FN Var gmmvi_erfcx(const Var& a) { return node(::gmmvi_erfcx(a.v), a, gmmvi_special::erfcx_partial(a.v)); }
GMMVI_TAPE_FN Var gmmvi_ndtr(const Var& a) { return node(::gmmvi_ndtr(a.v), a, gmmvi_special::ndtr_partial(a.v)); }
GMMVI_TAPE_FN Var gmmvi_log_ndtr(const Var& a) { return node(::gmmvi_log_ndtr(a.v), a, gmmvi_special::log_ndtr_partial(a.v)); }
GMMVI_TAPE_FN Var gmmvi_digamma(const Var& a) { return node(::gmmvi_digamma(a.v), a, ::gmmvi_trigamma(a.v)); }
GMMVI_TAPE_FN Var gmmvi_sigmoid(const Var& a) { const float s = ::gmmvi_sigmoid(a.v); return node(s, a, s * ::gmmvi_sigmoid(-a.v)); }
GMMVI_TAPE_FN Var gmmvi_softplus(const Var& a) { return node(::gmmvi_softplus(a.v), a, ::gmmvi_sigmoid(a.v)); }
GMMVI_TAPE_FN Var gmmvi_log_sigmoid(const Var& a) { return node(::gmmvi_log_sigmoid(a.v), a, ::gmmvi_sigmoid(-a.v)); }
GMMVI_TAPE_FN Var gmmvi_logaddexp(const Var& a, const Var& b) {
    return node(::gmmvi_logaddexp(a.v, b.v), a, gmmvi_special::logaddexp_partial(a.v, b.v), b,
                gmmvi_special::logaddexp_partial(b.v, a.v));
}
GMMVI_TAPE_FN Var gmmvi_logaddexp(const Var& a, float b) {
    return node(::gmmvi_logaddexp(a.v, b), a, gmmvi_special::logaddexp_partial(a.v, b));
}
GMMVI_TAPE_FN Var gmmvi_logaddexp(float a, const Var& b) {
    return node(::gmmvi_logaddexp(a, b.v), b, gmmvi_special::logaddexp_partial(b.v, a));
}

GMMVI_TAPE_FN float gmmvi_value(const Var& a) { return a.v; }

// What a gradient call passes as x: entry i is the input node i, and reading it makes no record.
struct Input {
    const float* x;
    GMMVI_TAPE_FN Var operator[](int i) const { return Var(x[i], i); }
};

// ---- vector primitives on the inputs (custom_target_vector.inc has their values): one record per call whatever n is, none for
// n <= 0.  The record keeps the address of c, not its contents: the sweep reads c[0 .. n) and the lane's x after the user's
// function has returned ---------------------------------------------------------------------------------------------------------
GMMVI_TAPE_FN int push_vector(int kind, int first, int n, int z, int w) { return push_bits(-2 - (4 * n + kind), first, z, w); }
GMMVI_TAPE_FN int push_vector(int kind, int first, int n, const float* c) {
    union { const float* p; int i[2]; } u; u.p = c;
    return push_vector(kind, first, n, u.i[0], u.i[1]);
}
GMMVI_TAPE_FN Var gmmvi_dot(const Input& x, int first, const float* c, int n) {
    if (n <= 0) return Var(0.f);
    return Var(::gmmvi_vector::dot_value(x.x + first, c, n), push_vector(::gmmvi_vector::DOT, first, n, c));
}
GMMVI_TAPE_FN Var gmmvi_sqdist(const Input& x, int first, const float* c, int n) {
    if (n <= 0) return Var(0.f);
    return Var(::gmmvi_vector::sqdist_value(x.x + first, c, n), push_vector(::gmmvi_vector::SQDIST, first, n, c));
}
GMMVI_TAPE_FN Var gmmvi_sumsq(const Input& x, int first, int n, float center) {
    if (n <= 0) return Var(0.f);
    return Var(::gmmvi_vector::sumsq_value(x.x + first, n, center), push_vector(::gmmvi_vector::SUMSQ, first, n, float_bits(center), 0));
}

// ---- primitives on arrays of nodes (custom_target_vector.inc has their values, from the same two templates as the float
// overloads; the user's call finds these by argument-dependent lookup on the element type).  A call makes a node-array record,
// kind 3 of the vector records, which spans 1 + ceil(n / 2) slots: the payload first, slot j = {id of entry 2 j, id of entry
// 2 j + 1 or -1, 32 bits for each}, the bits h[i].v for gmmvi_wdot and the partial p_i for gmmvi_logsumexp; then the header
// {-2 - (4 n + 3), first or -1, operation, 0}, behind its payload because the sweep walks backwards.  The result is the header's
// node; no Var refers to a payload slot, whose zeroed adjoint is never read.  The record copies what the sweep needs: the array
// may be local to the user's function.  Beyond the capacity nothing is stored and the count advances by slots, as for any record.
// GMMVI_TAPE_NODES: csrc/custom_compile.hip defines it where the user's text names one of the two primitives.  Without it
// neither the overloads nor the node-array branch of the sweep exist, so a kernel whose source does not call them is the kernel
// it was before they came, and a text that reaches them under another spelling does not compile instead of making a record that
// its sweep cannot read.
#ifdef GMMVI_TAPE_NODES
struct ValueAt {
    const Var* p;
    GMMVI_TAPE_FN float operator()(int i) const { return p[i].v; }
};
GMMVI_TAPE_FN Var gmmvi_wdot(const Input& x, int first, const Var* h, int n) {
    if (n <= 0) return Var(0.f);
    const float v = ::gmmvi_vector::wdot_value(x.x + first, ValueAt{h}, n);
    for (int i = 0; i < n; i += 2) {
        const bool two = i + 1 < n;
        push_bits(h[i].id, two ? h[i + 1].id : -1, float_bits(h[i].v), two ? float_bits(h[i + 1].v) : 0);
    }
    return Var(v, push_vector(::gmmvi_vector::NODES, first, n, ::gmmvi_vector::WDOT, 0));
}
// the constant -inf where the maximum is -inf, and a constant where every entry is one
GMMVI_TAPE_FN Var gmmvi_logsumexp(const Var* a, int n) {
    float m, s;
    const float v = ::gmmvi_vector::logsumexp_value(ValueAt{a}, n, m, s);
    bool constant = true;
    for (int i = 0; i < n; ++i) constant = constant && a[i].id < 0;
    if (constant || m == -__builtin_inff()) return Var(v);
    for (int i = 0; i < n; i += 2) {
        const bool two = i + 1 < n;
        push_bits(a[i].id, two ? a[i + 1].id : -1, float_bits(::gmmvi_vector::logsumexp_partial(a[i].v, m, s)),
                  two ? float_bits(::gmmvi_vector::logsumexp_partial(a[i + 1].v, m, s)) : 0);
    }
    return Var(v, push_vector(::gmmvi_vector::NODES, -1, n, ::gmmvi_vector::LOGSUMEXP, 0));
}
#endif

// ---- gmmvi_affine: out[j] = (sum over i of h[i] * x[w + i * si + j * sj]) + x[b + j * sb], j < m, a whole layer as one record
// group of ceil(n / 2) + 2 + m slots: the payload of gmmvi_wdot (the ids and the bits of h, once for all m outputs; a constant
// entry keeps its negative id, and every entry of the const float* overload is one), two descriptor slots {w, si, sj, b} and
// {sb, m, 0, 0}, then m headers {-2 - (4 n + 3), j, 2, 0}: node-array records with operation 2, header j the node of out[j].  No
// Var refers to a payload or descriptor slot.  The sweep (sweep_vector, below) enters the group at the first header it meets
// walking backwards and leaves it behind the payload: one visit handles every output.  n <= 0: out[j] is the input x[b + j * sb]
// itself, or the constant 0; m <= 0 writes nothing; neither makes a record.
// GMMVI_TAPE_AFFINE: csrc/custom_compile.hip defines it, and GMMVI_TAPE_NODES with it, where the user's text names gmmvi_affine.
#ifdef GMMVI_TAPE_AFFINE
#ifndef GMMVI_TAPE_NODES
#error "GMMVI_TAPE_AFFINE needs GMMVI_TAPE_NODES: its headers are node-array records"
#endif
struct IdAt {
    const Var* p;
    GMMVI_TAPE_FN int operator()(int i) const { return p[i].id; }
};
struct ConstantId {
    GMMVI_TAPE_FN int operator()(int) const { return -1; }
};
template <class At, class Id>
GMMVI_TAPE_FN void affine(const Input& x, int w, int si, int sj, int b, int sb, At h, Id id, int n, Var* out, int m) {
    if (m <= 0) return;
    if (n <= 0) {
        for (int j = 0; j < m; ++j) out[j] = b < 0 ? Var(0.f) : x[b + j * sb];
        return;
    }
    for (int i = 0; i < n; i += 2) {
        const bool two = i + 1 < n;
        push_bits(id(i), two ? id(i + 1) : -1, float_bits(h(i)), two ? float_bits(h(i + 1)) : 0);
    }
    push_bits(w, si, sj, b);
    push_bits(sb, m, 0, 0);
    for (int j = 0; j < m; ++j)
        out[j] = Var(::gmmvi_vector::affine_out(x.x, w, si, sj, b, sb, h, n, j),
                     push_vector(::gmmvi_vector::NODES, j, n, ::gmmvi_vector::AFFINE, 0));
}
GMMVI_TAPE_FN void gmmvi_affine(const Input& x, int w, int si, int sj, int b, int sb, const Var* h, int n, Var* out, int m) {
    affine(x, w, si, sj, b, sb, ValueAt{h}, IdAt{h}, n, out, m);
}
GMMVI_TAPE_FN void gmmvi_affine(const Input& x, int w, int si, int sj, int b, int sb, const float* h, int n, Var* out, int m) {
    affine(x, w, si, sj, b, sb, ::gmmvi_vector::FloatAt{h}, ConstantId{}, n, out, m);
}
#endif

// The vector record v at record index r with adjoint w: adds w * d node / d x[first + i] into g[(first + i) * g_stride], i
// ascending; a node-array record also adds w * d node / d entry i into the adjoint of every entry that is not a constant, from
// its payload in the slots below r.  x: the lane's inputs.  -> the slots the record spans, which the sweep steps back over.
GMMVI_TAPE_FN int sweep_vector(const Rec4& v, float w, int r, int D, RecPtr rp, AdjPtr ap, size_t stride, const float* x, float* g,
                               size_t g_stride) {
    const int code = -2 - v.x, kind = code & 3, n = code >> 2;
#ifdef GMMVI_TAPE_NODES
    if (kind == ::gmmvi_vector::NODES) {
        const int slots = (n + 1) >> 1;
#ifdef GMMVI_TAPE_AFFINE
        // Header j = v.y of a gmmvi_affine group, the first header of the group the lane meets: a later record consumed the
        // outputs (then j = m - 1), or the function's output is out[j] itself.  Every consumer of out[0 .. j] has been swept, so
        // the adjoints a_0 .. a_j of headers 0 .. j are final (a header above j has no swept consumer: its adjoint is 0 and it is
        // left out).  Entry i, ascending, reads its payload once; jj ascending inside it: h[i].v a_jj goes to the gradient of weight
        // (i, jj), and the sum over jj of x[weight (i, jj)] a_jj, by fmaf from 0, goes once to the entry's adjoint.  Then a_jj to
        // the gradient of bias jj, jj ascending.  The whole group is stepped over: no other header of it is visited.
        if (v.z == ::gmmvi_vector::AFFINE) {
            const int j = v.y, group = r - j - 2 - slots;               // the group's first slot
            const Rec4 lay = rp[(size_t)(group + slots) * stride];       // {w, si, sj, b}
            const int sb = rp[(size_t)(group + slots + 1) * stride].x;
            const AdjPtr a = ap + (size_t)(group + slots + 2) * stride;  // a[jj * stride]: the adjoint of out[jj]
            for (int i = 0; i < n; ++i) {
                const Rec4 e = rp[(size_t)(group + (i >> 1)) * stride];
                const int id = i & 1 ? e.y : e.x;
                const float hv = bits_float(i & 1 ? e.w : e.z);
                float d = 0.f;
                for (int jj = 0; jj <= j; ++jj) {
                    const int at = lay.x + i * lay.y + jj * lay.z;
                    const float ajj = a[(size_t)jj * stride];
                    g[(size_t)at * g_stride] += hv * ajj;
                    d = ::fmaf(x[at], ajj, d);
                }
                if (id >= 0) {
                    if (id < D) g[(size_t)id * g_stride] += d; else ap[(size_t)(id - D) * stride] += d;
                }
            }
            if (lay.w >= 0)
                for (int jj = 0; jj <= j; ++jj) g[(size_t)(lay.w + jj * sb) * g_stride] += a[(size_t)jj * stride];
            return j + 1 + 2 + slots;
        }
#endif
        const bool wdot = v.z == ::gmmvi_vector::WDOT;
        for (int i = 0; i < n; ++i) {
            const Rec4 e = rp[(size_t)(r - slots + (i >> 1)) * stride];
            const int id = i & 1 ? e.y : e.x;
            float d = bits_float(i & 1 ? e.w : e.z) * w;              // gmmvi_logsumexp: p_i w, the entry's share
            if (wdot) {
                g[(size_t)(v.y + i) * g_stride] += d;                   // h[i].v w, the input's share; the entry's is x[first + i] w
                d = x[v.y + i] * w;
            }
            if (id >= 0) {
                if (id < D) g[(size_t)id * g_stride] += d; else ap[(size_t)(id - D) * stride] += d;
            }
        }
        return 1 + slots;
    }
#endif
    x += v.y;
    g += (size_t)v.y * g_stride;
    if (kind == ::gmmvi_vector::SUMSQ) {
        const float center = bits_float(v.z);
        for (int i = 0; i < n; ++i) g[(size_t)i * g_stride] += 2.f * (x[i] - center) * w;
        return 1;
    }
    union { const float* p; int i[2]; } u; u.i[0] = v.z; u.i[1] = v.w;
    const float* c = u.p;
    if (kind == ::gmmvi_vector::DOT) {
        for (int i = 0; i < n; ++i) g[(size_t)i * g_stride] += c[i] * w;
    } else {
        for (int i = 0; i < n; ++i) g[(size_t)i * g_stride] += 2.f * (x[i] - c[i]) * w;
    }
    return 1;
}

// The sweep of one lane: adds d out / d x[i] into g[i * g_stride] for every input i, walking the records from the output's own back
// to record 0 (records made after the output node are never visited).  rp / ap: the lane's record 0 and adjoint slot 0, `stride`
// floats / records from one record to the next.  A lane takes the branch of its own record's kind, whatever its neighbours hold.
GMMVI_TAPE_FN void sweep(const Var& out, int D, RecPtr rp, AdjPtr ap, size_t stride, const float* x, float* g, size_t g_stride) {
    if (out.id < 0) return;                                           // a constant: nothing to add
    if (out.id < D) { g[(size_t)out.id * g_stride] += 1.f; return; }  // an input
    int r = out.id - D;
    ap[(size_t)r * stride] = 1.f;
    while (r >= 0) {
        // the loop of the scalar records, which a vector record leaves: its code stands outside this loop
        Rec4 v;
        float w;
        for (;;) {
            v = rp[(size_t)r * stride];
            w = ap[(size_t)r * stride];
            if (v.x < -1) break;
            if (v.x >= 0) {
                const float d = bits_float(v.z) * w;
                if (v.x < D) g[(size_t)v.x * g_stride] += d; else ap[(size_t)(v.x - D) * stride] += d;
            }
            if (v.y >= 0) {
                const float d = bits_float(v.w) * w;
                if (v.y < D) g[(size_t)v.y * g_stride] += d; else ap[(size_t)(v.y - D) * stride] += d;
            }
            if (--r < 0) return;
        }
        r -= sweep_vector(v, w, r, D, rp, ap, stride, x, g, g_stride);
    }
}

}  // namespace gmmvi_tape

// (csrc/custom_target.hip declares this one in front of the user's text as well: the user's float instantiation needs it there;
// behind the dual-number text, which defines it too, GMMVI_TAPE_NO_FLOAT_VALUE leaves it out)
#ifndef GMMVI_TAPE_NO_FLOAT_VALUE
__host__ __device__ inline float gmmvi_value(float a) { return a; }
#endif

#ifndef GMMVI_TAPE_NO_KERNELS
// Value call: one float instantiation per sample, no tape.
extern "C" __global__ __launch_bounds__(256) void gmmvi_tape_lp(int D, const float* params, const float* X, int N, float* lp) {
    const size_t n = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (n >= (size_t)N) return;
    lp[n] = gmmvi_user_density<float, const float*>(X + n * (size_t)D, D, params);
}

// Gradient call: one wave per workgroup, lane = sample first + 64 blockIdx.x + lane of X[first .. N).  The lane records its
// evaluation on the wave's tape (rec / adj + 64 cap blockIdx.x records), then walks its own records from the output back to record 0;
// the adjoints of the inputs add up in the lane's own gradient row, which the lane zeroes first.  No other lane touches the
// row or the lane's tape column, so no sum involves an atomic: the same inputs give the same bits.  Every lane raises *needed
// to its record count (an integer maximum); a lane whose count exceeds cap has an incomplete tape and writes no gradient.
extern "C" __global__ __launch_bounds__(64) void gmmvi_tape_grad(int D, const float* params, const float* X, int N, float* lp,
                                                                  float* grad, int first, void* rec, float* adj, int cap, int* needed) {
    using namespace gmmvi_tape;
    const int l = (int)threadIdx.x;
    const size_t wave_at = (size_t)blockIdx.x * 64 * (size_t)cap;
    if (l == 0) {
        Tape& t = tape();
        t.rec = (RecPtr)rec + wave_at;
        t.adj = (AdjPtr)adj + wave_at;
        t.stride = 64; t.cap = cap; t.D = D;
    }
    count() = 0;
    __syncthreads();
    const size_t n = (size_t)first + (size_t)blockIdx.x * 64 + l;
    if (n >= (size_t)N) return;
    const Var out = gmmvi_user_density<Var, Input>(Input{X + n * (size_t)D}, D, params);
    lp[n] = out.v;
    const int made = count();
    atomicMax(needed, made);
    if (made > cap) return;
    float* g = grad + n * (size_t)D;
    for (int i = 0; i < D; ++i) g[i] = 0.f;
    sweep(out, D, (RecPtr)rec + wave_at + l, (AdjPtr)adj + wave_at + l, 64, X + n * (size_t)D, g, 1);
}
#endif
#undef GMMVI_TAPE_FN
)GMMVI_TAPE"
