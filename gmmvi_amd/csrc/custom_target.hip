// User-defined targets compiled at run time (include/gmmvi_hip.h, "user-defined device targets"): the user's source defines
// gmmvi_user_target, this file appends the wrapper kernels of custom_target_wrap.inc, compiles both with hiprtc for the device
// of the context, loads the code object and launches the wrapper on the context's stream.  hiprtc is bound with dlopen on
// first use: the library links without it, and only a call that needs the compiler can miss it.
// Differentiated targets (gmmvi_custom_target_compile_autodiff): the user's source defines gmmvi_user_density instead, and the
// dual-number text of custom_target_autodiff.inc, which defines gmmvi_user_target on top of it, goes between the two.
#include "common.h"
#include <hip/hiprtc.h>
#include <dlfcn.h>

static const char* const kWrapText =
#include "custom_target_wrap.inc"
    ;
static const char* const kAutodiffText =
#include "custom_target_autodiff.inc"
    ;
// Goes in front of the user's first line, on that line: a float has no namespace for argument-dependent lookup to search, so
// the float instantiation of the user's template finds gmmvi_value only if it is declared before the template.
static const char* const kAutodiffPrelude = "__host__ __device__ inline float gmmvi_value(float); ";
#define GMMVI_STR2(x) #x
#define GMMVI_STR(x) GMMVI_STR2(x)

namespace {
struct Hiprtc {
    void* so = nullptr;
    decltype(&hiprtcCreateProgram) create = nullptr;
    decltype(&hiprtcCompileProgram) compile = nullptr;
    decltype(&hiprtcGetProgramLogSize) log_size = nullptr;
    decltype(&hiprtcGetProgramLog) log = nullptr;
    decltype(&hiprtcGetCodeSize) code_size = nullptr;
    decltype(&hiprtcGetCode) code = nullptr;
    decltype(&hiprtcDestroyProgram) destroy = nullptr;
    decltype(&hiprtcGetErrorString) error_string = nullptr;
    std::string why;                                   // non-empty: the binding failed, and how
};

template <class F>
bool bind(Hiprtc& h, F& fn, const char* name) {
    fn = reinterpret_cast<F>(dlsym(h.so, name));
    if (!fn) h.why = std::string("libhiprtc.so has no symbol ") + name;
    return fn != nullptr;
}

const Hiprtc& hiprtc() {
    static const Hiprtc h = [] {
        Hiprtc b;
        for (const char* name : {"libhiprtc.so", "libhiprtc.so.7", "libhiprtc.so.6"}) {
            b.so = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (b.so) break;
        }
        if (!b.so) {
            const char* e = dlerror();
            b.why = std::string("libhiprtc.so could not be loaded (user-defined targets need the ROCm run-time compiler): ") +
                    (e ? e : "?");
            return b;
        }
        (void)(bind(b, b.create, "hiprtcCreateProgram") && bind(b, b.compile, "hiprtcCompileProgram") &&
               bind(b, b.log_size, "hiprtcGetProgramLogSize") && bind(b, b.log, "hiprtcGetProgramLog") &&
               bind(b, b.code_size, "hiprtcGetCodeSize") && bind(b, b.code, "hiprtcGetCode") &&
               bind(b, b.destroy, "hiprtcDestroyProgram") && bind(b, b.error_string, "hiprtcGetErrorString"));
        return b;
    }();
    return h;
}

// user's text (+ dual-number text) + wrapper kernels -> code object for `arch`.  GMMVI_OK, or the status with the compiler log /
// reason in `log`.  The user's text stays first (behind one declaration on its first line): the compiler's line numbers are the
// user's.
int compile_source(const char* source, bool autodiff, const char* arch, std::vector<char>& code, std::string& log) {
    const Hiprtc& rt = hiprtc();
    if (!rt.why.empty()) { log = rt.why; return GMMVI_ERR_HIP; }
    const std::string text = autodiff ? std::string(kAutodiffPrelude) + source + "\n" + kAutodiffText + "\n" + kWrapText
                                      : std::string(source) + "\n" + kWrapText;
    const char* const entry = autodiff ? "gmmvi_user_density" : "gmmvi_user_target";
    hiprtcProgram prog = nullptr;
    hiprtcResult r = rt.create(&prog, text.c_str(), "gmmvi_user_target.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) { log = std::string("hiprtcCreateProgram: ") + rt.error_string(r); return GMMVI_ERR_HIP; }
    const std::string arch_opt = std::string("--offload-arch=") + arch;
    const char* opts[] = {arch_opt.c_str(), "-O3", "-std=c++17",
                          "-DGMMVI_CUSTOM_AUTODIFF_TANGENTS=" GMMVI_STR(GMMVI_CUSTOM_AUTODIFF_TANGENTS)};   // autodiff only
    r = rt.compile(prog, autodiff ? 4 : 3, opts);
    size_t n = 0;
    if (rt.log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) {
        log.resize(n);
        if (rt.log(prog, &log[0]) != HIPRTC_SUCCESS) log.clear();
        while (!log.empty() && log.back() == '\0') log.pop_back();
    }
    int rc = GMMVI_OK;
    if (r != HIPRTC_SUCCESS) {
        std::string head = std::string("user target does not compile (") + rt.error_string(r) + ")";
        if (log.find(std::string("undeclared identifier '") + entry + "'") != std::string::npos)
            head += std::string(": the source does not define ") + entry;
        log = head + ":\n" + log;
        rc = GMMVI_ERR_ARG;
    } else {
        size_t bytes = 0;
        r = rt.code_size(prog, &bytes);
        if (r == HIPRTC_SUCCESS) { code.resize(bytes); r = rt.code(prog, code.data()); }
        if (r != HIPRTC_SUCCESS) { log = std::string("hiprtcGetCode: ") + rt.error_string(r); rc = GMMVI_ERR_HIP; }
    }
    (void)rt.destroy(&prog);
    return rc;
}

uint64_t fnv1a(const char* s) {
    uint64_t h = 1469598103934665603ull;
    for (; *s; ++s) { h ^= (unsigned char)*s; h *= 1099511628211ull; }
    return h;
}
}  // namespace

struct gmmvi_custom_target {
    uint64_t hash = 0;
    std::string source;
    bool autodiff = false;                 // compiled through gmmvi_user_density and the dual-number text
    int refs = 0;
    hipModule_t module = nullptr;
    hipFunction_t fn[4] = {};              // staged lp, staged lp + grad, direct lp, direct lp + grad
};

static std::vector<gmmvi_custom_target*>::iterator find_target(gmmvi_ctx* ctx, const gmmvi_custom_target* t) {
    auto it = ctx->custom_targets.begin();
    while (it != ctx->custom_targets.end() && *it != t) ++it;
    return it;
}

void gmmvi_custom_targets_destroy(gmmvi_ctx* ctx) {
    for (gmmvi_custom_target* t : ctx->custom_targets) {
        if (t->module) (void)hipModuleUnload(t->module);
        delete t;
    }
    ctx->custom_targets.clear();
}

static int check_source(const char* what, const char* source, bool autodiff, const char* arch, char* log_out, size_t log_cap) {
    if (log_out && log_cap) log_out[0] = '\0';
    if (!source || !arch) return gmmvi_fail(nullptr, GMMVI_ERR_ARG, std::string(what) + ": source and arch must not be NULL");
    std::vector<char> code;
    std::string log;
    const int rc = compile_source(source, autodiff, arch, code, log);
    if (log_out && log_cap) {
        const size_t n = log.size() < log_cap - 1 ? log.size() : log_cap - 1;
        memcpy(log_out, log.data(), n);
        log_out[n] = '\0';
    }
    return rc == GMMVI_OK ? rc : gmmvi_fail(nullptr, rc, log);
}

extern "C" int gmmvi_custom_target_check(const char* source, const char* arch, char* log_out, size_t log_cap) {
    return check_source("gmmvi_custom_target_check", source, false, arch, log_out, log_cap);
}

extern "C" int gmmvi_custom_target_check_autodiff(const char* source, const char* arch, char* log_out, size_t log_cap) {
    return check_source("gmmvi_custom_target_check_autodiff", source, true, arch, log_out, log_cap);
}

// The context's modules are keyed by (hash of the source, mode): the same text compiled both ways gives two handles.
static int compile_target(gmmvi_ctx* ctx, const char* source, bool autodiff, gmmvi_custom_target** out) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr && out != nullptr);
    *out = nullptr;
    GMMVI_ARG_CHECK(ctx, source != nullptr);
    const uint64_t hash = fnv1a(source);
    for (gmmvi_custom_target* t : ctx->custom_targets)
        if (t->hash == hash && t->autodiff == autodiff && t->source == source) { ++t->refs; *out = t; return GMMVI_OK; }
    hipDeviceProp_t prop;
    GMMVI_HIP_CHECK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    std::vector<char> code;
    std::string log;
    const int rc = compile_source(source, autodiff, prop.gcnArchName, code, log);
    if (rc != GMMVI_OK) return gmmvi_fail(ctx, rc, log);
    gmmvi_custom_target* t = new gmmvi_custom_target();
    t->hash = hash; t->source = source; t->autodiff = autodiff; t->refs = 1;
    static const char* const names[4] = {"gmmvi_custom_staged_lp", "gmmvi_custom_staged_grad", "gmmvi_custom_direct_lp",
                                         "gmmvi_custom_direct_grad"};
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipModuleLoadData(&t->module, code.data());
    for (int i = 0; e == hipSuccess && i < 4; ++i) e = hipModuleGetFunction(&t->fn[i], t->module, names[i]);
    if (e != hipSuccess) {
        if (t->module) (void)hipModuleUnload(t->module);
        delete t;
        return gmmvi_fail(ctx, GMMVI_ERR_HIP, std::string("loading the code object of a user target: ") + hipGetErrorString(e));
    }
    ctx->custom_targets.push_back(t);
    *out = t;
    return GMMVI_OK;
}

extern "C" int gmmvi_custom_target_compile(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out) {
    return compile_target(ctx, source, false, out);
}

extern "C" int gmmvi_custom_target_compile_autodiff(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out) {
    return compile_target(ctx, source, true, out);
}

extern "C" int gmmvi_custom_target_release(gmmvi_ctx* ctx, gmmvi_custom_target* t) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    if (!t) return GMMVI_OK;
    auto it = find_target(ctx, t);
    if (it == ctx->custom_targets.end())
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the custom target does not belong to this context");
    if (--t->refs > 0) return GMMVI_OK;
    GMMVI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));       // launches of its kernels may still be queued
    ctx->custom_targets.erase(it);
    const hipError_t e = hipModuleUnload(t->module);
    delete t;
    GMMVI_HIP_CHECK(ctx, e);
    return GMMVI_OK;
}

extern "C" int gmmvi_target_custom(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                   const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int route) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    GMMVI_ARG_CHECK(ctx, N >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG && X_dev != nullptr && lp_out_dev != nullptr);
    GMMVI_ARG_CHECK(ctx, route >= 0 && route <= 2);
    if (route == 1 && D > GMMVI_CUSTOM_STAGED_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: route 1 (staged) needs D <= " +
                                                  std::to_string(GMMVI_CUSTOM_STAGED_MAX_DIM) + ", got D = " + std::to_string(D));
    if (t->autodiff && grad_out_dev != nullptr && D > GMMVI_CUSTOM_AUTODIFF_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the gradient of a differentiated target needs D <= " +
                                                  std::to_string(GMMVI_CUSTOM_AUTODIFF_MAX_DIM) + ", got D = " + std::to_string(D) +
                                                  " (values only, or a hand-written gradient, run above)");
    const bool staged = route == 1 || (route == 0 && D <= GMMVI_CUSTOM_STAGED_MAX_DIM);
    const bool want_grad = grad_out_dev != nullptr;
    const unsigned threads = staged ? 64u : 256u;
    const size_t blocks = ((size_t)N + threads - 1) / threads;
    GMMVI_ARG_CHECK(ctx, blocks <= 2147483647u);
    const size_t lds = staged ? (size_t)(want_grad ? 2 : 1) * 64 * (size_t)(D | 1) * sizeof(float) : 0;   // <= 61952 B
    void* args[] = {&D, &params_dev, &X_dev, &N, &lp_out_dev, &grad_out_dev};
    GMMVI_PROF(ctx, staged ? "target_custom_staged" : "target_custom_direct");
    GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[(staged ? 0 : 2) + (want_grad ? 1 : 0)], (unsigned)blocks, 1, 1, threads, 1, 1,
                                               (unsigned)lds, ctx->stream, args, nullptr));
    return GMMVI_OK;
}
