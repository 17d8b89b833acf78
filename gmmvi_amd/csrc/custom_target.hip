// User-defined targets compiled at run time (include/gmmvi_hip.h, "user-defined device targets"): the user's source defines
// gmmvi_user_target, this file appends the wrapper kernels of custom_target_wrap.inc, compiles both with hiprtc for the device
// of the context, loads the code object and launches the wrapper on the context's stream.  hiprtc is bound with dlopen on
// first use: the library links without it, and only a call that needs the compiler can miss it.
// In every mode the float special functions of custom_target_special.inc go directly behind the user's source.
// Differentiated targets (gmmvi_custom_target_compile_autodiff): the user's source defines gmmvi_user_density instead, and the
// dual-number text of custom_target_autodiff.inc, which defines gmmvi_user_target on top of it, goes between the two.
// Targets summed over a data set (gmmvi_custom_target_compile_data): the user's source defines gmmvi_user_row and
// gmmvi_user_prior; behind it go the dual-number text without its adapter, the tile mover of the wrapper text, the Feistel
// stream (feistel.h and philox.h, made one string by the Makefile) and the kernels of custom_target_data.inc, which
// gmmvi_target_custom_data launches, and gmmvi_target_custom_data_own_batches their own-batch instances.  The same text ends
// with the predictive kernels (the reduction over the samples of the row terms on an evaluation set), which
// gmmvi_custom_data_predictive launches for a handle of either data mode.
// Targets differentiated on a tape (gmmvi_custom_target_compile_tape): the source of the differentiated mode, unchanged; behind it
// goes custom_target_tape.inc alone, the tape's number type and its two kernels, which gmmvi_target_custom_tape launches.
// Targets summed over a data set and differentiated on a tape (gmmvi_custom_target_compile_data_tape): the source of the data
// mode, unchanged; behind it go the whole text of the data mode (its value kernels are this mode's value call), the tape's number
// type without its kernels and custom_target_data_tape.inc, whose two kernels gmmvi_target_custom_data_tape launches.
#include "common.h"
#include "feistel.h"
#include <hip/hiprtc.h>
#include <dlfcn.h>

static const char* const kWrapText =
#include "custom_target_wrap.inc"
    ;
static const char* const kSpecialText =
#include "custom_target_special.inc"
    ;
static const char* const kAutodiffText =
#include "custom_target_autodiff.inc"
    ;
static const char* const kDataText =
    "using __hip_internal::uint32_t; using __hip_internal::uint64_t;\n"    // the run-time compiler has no <cstdint>
#include "build/feistel_text.inc"
#include "custom_target_data.inc"
    ;
static const char* const kTapeText =
#include "custom_target_tape.inc"
    ;
static const char* const kDataTapeText =
#include "custom_target_data_tape.inc"
    ;
// Goes in front of the user's first line, on that line: a float has no namespace for argument-dependent lookup to search, so
// the float instantiation of the user's template finds gmmvi_value and the six functions of custom_target_special.inc only if
// they are declared before the template.  The hand-written mode gets the same line: its float code calls the six too.
static const char* const kAutodiffPrelude =
    "__host__ __device__ inline float gmmvi_value(float); __host__ __device__ inline float gmmvi_digamma(float); "
    "__host__ __device__ inline float gmmvi_trigamma(float); __host__ __device__ inline float gmmvi_sigmoid(float); "
    "__host__ __device__ inline float gmmvi_softplus(float); __host__ __device__ inline float gmmvi_log_sigmoid(float); "
    "__host__ __device__ inline float gmmvi_logaddexp(float, float); ";
#define GMMVI_STR2(x) #x
#define GMMVI_STR(x) GMMVI_STR2(x)

// what the source defines: gmmvi_user_target; gmmvi_user_density; gmmvi_user_row and gmmvi_user_prior; gmmvi_user_density again;
// gmmvi_user_row and gmmvi_user_prior again
enum Mode { MODE_HAND = 0, MODE_AUTODIFF = 1, MODE_DATA = 2, MODE_TAPE = 3, MODE_DATA_TAPE = 4 };

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
int compile_source(const char* source, Mode mode, const char* arch, std::vector<char>& code, std::string& log) {
    const Hiprtc& rt = hiprtc();
    if (!rt.why.empty()) { log = rt.why; return GMMVI_ERR_HIP; }
    std::string text = kAutodiffPrelude;
    if (source[strspn(source, " \t")] == '#') text += "\n#line 1\n";   // a directive has to begin its line; the numbers stay the user's
    text += std::string(source) + "\n" + kSpecialText;
    if (mode == MODE_TAPE) {
        text += kTapeText;
    } else {
        if (mode != MODE_HAND) text += kAutodiffText;
        text += std::string("\n") + kWrapText;
        if (mode == MODE_DATA || mode == MODE_DATA_TAPE) text += std::string("\n") + kDataText;
        if (mode == MODE_DATA_TAPE) text += std::string("\n") + kTapeText + "\n" + kDataTapeText;
    }
    static const char* const entries[5][2] = {{"gmmvi_user_target", nullptr}, {"gmmvi_user_density", nullptr},
                                              {"gmmvi_user_row", "gmmvi_user_prior"}, {"gmmvi_user_density", nullptr},
                                              {"gmmvi_user_row", "gmmvi_user_prior"}};
    hiprtcProgram prog = nullptr;
    hiprtcResult r = rt.create(&prog, text.c_str(), "gmmvi_user_target.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) { log = std::string("hiprtcCreateProgram: ") + rt.error_string(r); return GMMVI_ERR_HIP; }
    const std::string arch_opt = std::string("--offload-arch=") + arch;
    const char* opts[] = {arch_opt.c_str(), "-O3", "-std=c++17",
                          "-DGMMVI_CUSTOM_AUTODIFF_TANGENTS=" GMMVI_STR(GMMVI_CUSTOM_AUTODIFF_TANGENTS),   // not MODE_HAND
                          "-DGMMVI_AD_NO_ADAPTER", "-DGMMVI_WRAP_TILE_ONLY",                               // the data modes only
                          "-DGMMVI_TAPE_NO_KERNELS", "-DGMMVI_TAPE_NO_FLOAT_VALUE", "-DGMMVI_CUSTOM_TAPE=1"};   // MODE_DATA_TAPE only
    if (mode == MODE_TAPE) opts[4] = "-DGMMVI_CUSTOM_TAPE=1";
    r = rt.compile(prog, mode == MODE_HAND ? 3 : mode == MODE_AUTODIFF ? 4 : mode == MODE_TAPE ? 5 : mode == MODE_DATA ? 6 : 9, opts);
    size_t n = 0;
    if (rt.log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) {
        log.resize(n);
        if (rt.log(prog, &log[0]) != HIPRTC_SUCCESS) log.clear();
        while (!log.empty() && log.back() == '\0') log.pop_back();
    }
    int rc = GMMVI_OK;
    if (r != HIPRTC_SUCCESS) {
        std::string head = std::string("user target does not compile (") + rt.error_string(r) + ")";
        for (const char* entry : entries[mode])
            if (entry && log.find(std::string("undeclared identifier '") + entry + "'") != std::string::npos)
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
    Mode mode = MODE_HAND;
    int refs = 0;
    hipModule_t module = nullptr;
    hipFunction_t fn[16] = {};             // staged lp, staged lp + grad, direct lp, direct lp + grad; MODE_DATA: merge lp, lp + grad;
                                           // MODE_TAPE: lp, lp + grad; MODE_DATA_TAPE: the six of MODE_DATA, tape rows, tape finish;
                                           // both data modes: fn[8 .. 10] predictive staged, direct, merge; fn[11 .. 14] own-batch
                                           // rows in the order of fn[0 .. 3]; MODE_DATA_TAPE: fn[15] own-batch tape rows
    mutable std::vector<std::pair<int, int>> tape_lengths;   // the tape modes: (D, the longest tape a gradient launch at that D has needed)
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

static int check_source(const char* what, const char* source, Mode mode, const char* arch, char* log_out, size_t log_cap) {
    if (log_out && log_cap) log_out[0] = '\0';
    if (!source || !arch) return gmmvi_fail(nullptr, GMMVI_ERR_ARG, std::string(what) + ": source and arch must not be NULL");
    std::vector<char> code;
    std::string log;
    const int rc = compile_source(source, mode, arch, code, log);
    if (log_out && log_cap) {
        const size_t n = log.size() < log_cap - 1 ? log.size() : log_cap - 1;
        memcpy(log_out, log.data(), n);
        log_out[n] = '\0';
    }
    return rc == GMMVI_OK ? rc : gmmvi_fail(nullptr, rc, log);
}

extern "C" int gmmvi_custom_target_check(const char* source, const char* arch, char* log_out, size_t log_cap) {
    return check_source("gmmvi_custom_target_check", source, MODE_HAND, arch, log_out, log_cap);
}

extern "C" int gmmvi_custom_target_check_autodiff(const char* source, const char* arch, char* log_out, size_t log_cap) {
    return check_source("gmmvi_custom_target_check_autodiff", source, MODE_AUTODIFF, arch, log_out, log_cap);
}

extern "C" int gmmvi_custom_target_check_data(const char* source, const char* arch, char* log_out, size_t log_cap) {
    return check_source("gmmvi_custom_target_check_data", source, MODE_DATA, arch, log_out, log_cap);
}

extern "C" int gmmvi_custom_target_check_tape(const char* source, const char* arch, char* log_out, size_t log_cap) {
    return check_source("gmmvi_custom_target_check_tape", source, MODE_TAPE, arch, log_out, log_cap);
}

extern "C" int gmmvi_custom_target_check_data_tape(const char* source, const char* arch, char* log_out, size_t log_cap) {
    return check_source("gmmvi_custom_target_check_data_tape", source, MODE_DATA_TAPE, arch, log_out, log_cap);
}

// The context's modules are keyed by (hash of the source, mode): the same text compiled in two modes gives two handles.
static int compile_target(gmmvi_ctx* ctx, const char* source, Mode mode, gmmvi_custom_target** out) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr && out != nullptr);
    *out = nullptr;
    GMMVI_ARG_CHECK(ctx, source != nullptr);
    const uint64_t hash = fnv1a(source);
    for (gmmvi_custom_target* t : ctx->custom_targets)
        if (t->hash == hash && t->mode == mode && t->source == source) { ++t->refs; *out = t; return GMMVI_OK; }
    hipDeviceProp_t prop;
    GMMVI_HIP_CHECK(ctx, hipGetDeviceProperties(&prop, ctx->device));
    std::vector<char> code;
    std::string log;
    const int rc = compile_source(source, mode, prop.gcnArchName, code, log);
    if (rc != GMMVI_OK) return gmmvi_fail(ctx, rc, log);
    gmmvi_custom_target* t = new gmmvi_custom_target();
    t->hash = hash; t->source = source; t->mode = mode; t->refs = 1;
    static const char* const wrap_names[4] = {"gmmvi_custom_staged_lp", "gmmvi_custom_staged_grad", "gmmvi_custom_direct_lp",
                                              "gmmvi_custom_direct_grad"};
    static const char* const data_names[6] = {"gmmvi_data_rows_staged_lp", "gmmvi_data_rows_staged_grad", "gmmvi_data_rows_direct_lp",
                                              "gmmvi_data_rows_direct_grad", "gmmvi_data_merge_lp", "gmmvi_data_merge_grad"};
    static const char* const tape_names[2] = {"gmmvi_tape_lp", "gmmvi_tape_grad"};
    static const char* const data_tape_names[8] = {"gmmvi_data_rows_staged_lp", "gmmvi_data_rows_staged_grad",
                                                   "gmmvi_data_rows_direct_lp", "gmmvi_data_rows_direct_grad", "gmmvi_data_merge_lp",
                                                   "gmmvi_data_merge_grad", "gmmvi_data_tape_rows", "gmmvi_data_tape_finish"};
    const char* const* names = mode == MODE_DATA ? data_names : mode == MODE_TAPE ? tape_names :
                               mode == MODE_DATA_TAPE ? data_tape_names : wrap_names;
    const int count = mode == MODE_DATA ? 6 : mode == MODE_TAPE ? 2 : mode == MODE_DATA_TAPE ? 8 : 4;
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipModuleLoadData(&t->module, code.data());
    for (int i = 0; e == hipSuccess && i < count; ++i) e = hipModuleGetFunction(&t->fn[i], t->module, names[i]);
    static const char* const predictive_names[3] = {"gmmvi_data_predictive_staged", "gmmvi_data_predictive_direct",
                                                    "gmmvi_data_predictive_merge"};
    for (int i = 0; e == hipSuccess && i < 3 && (mode == MODE_DATA || mode == MODE_DATA_TAPE); ++i)
        e = hipModuleGetFunction(&t->fn[8 + i], t->module, predictive_names[i]);
    static const char* const own_names[5] = {"gmmvi_data_rows_own_staged_lp", "gmmvi_data_rows_own_staged_grad",
                                             "gmmvi_data_rows_own_direct_lp", "gmmvi_data_rows_own_direct_grad",
                                             "gmmvi_data_tape_rows_own"};
    for (int i = 0; e == hipSuccess && i < (mode == MODE_DATA ? 4 : mode == MODE_DATA_TAPE ? 5 : 0); ++i)
        e = hipModuleGetFunction(&t->fn[11 + i], t->module, own_names[i]);
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
    return compile_target(ctx, source, MODE_HAND, out);
}

extern "C" int gmmvi_custom_target_compile_autodiff(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out) {
    return compile_target(ctx, source, MODE_AUTODIFF, out);
}

extern "C" int gmmvi_custom_target_compile_data(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out) {
    return compile_target(ctx, source, MODE_DATA, out);
}

extern "C" int gmmvi_custom_target_compile_tape(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out) {
    return compile_target(ctx, source, MODE_TAPE, out);
}

extern "C" int gmmvi_custom_target_compile_data_tape(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out) {
    return compile_target(ctx, source, MODE_DATA_TAPE, out);
}

// what gmmvi_target_custom, gmmvi_target_custom_data and gmmvi_target_custom_tape answer to a handle of MODE_DATA_TAPE
static int refuse_data_tape(gmmvi_ctx* ctx) {
    return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the target was compiled by gmmvi_custom_target_compile_data_tape (a row "
                                          "term and a prior, differentiated on a tape that needs scratch and a readback): "
                                          "gmmvi_target_custom_data_tape launches it");
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
    if (t->mode == MODE_DATA_TAPE) return refuse_data_tape(ctx);
    if (t->mode == MODE_DATA)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the target was compiled by gmmvi_custom_target_compile_data (a row "
                                              "term and a prior, no gmmvi_user_target): gmmvi_target_custom_data launches it");
    if (t->mode == MODE_TAPE)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the target was compiled by gmmvi_custom_target_compile_tape (its "
                                              "gradient comes from a tape, which needs scratch and a readback): "
                                              "gmmvi_target_custom_tape launches it");
    if (route == 1 && D > GMMVI_CUSTOM_STAGED_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: route 1 (staged) needs D <= " +
                                                  std::to_string(GMMVI_CUSTOM_STAGED_MAX_DIM) + ", got D = " + std::to_string(D));
    if (t->mode == MODE_AUTODIFF && grad_out_dev != nullptr && D > GMMVI_CUSTOM_AUTODIFF_MAX_DIM)
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

// ---- targets summed over a data set ----------------------------------------------------------------------------------------
// The launch plan.  Auto: the row list is cut into enough chunks that ceil(N / 64) * chunks workgroups reach GMMVI_DATA_PLAN_CUS
// (the compute units of an MI355X: one workgroup of four waves each), but into no more than rows / GMMVI_DATA_MIN_CHUNK_ROWS, so
// that every wave of a chunk has at least GMMVI_DATA_MIN_CHUNK_ROWS / 4 rows to pay for the chunk's merge traffic and launch
// tail.  A request is honoured up to one row per chunk.  Either way the chunks are then as even as whole rows allow, and the
// count is what that row count per chunk needs: the last chunk is never empty.
constexpr int GMMVI_DATA_PLAN_CUS = 256;
constexpr int GMMVI_DATA_MIN_CHUNK_ROWS = 32;
constexpr int64_t GMMVI_DATA_MAX_CHUNKS = 65535;           // gridDim.y

extern "C" int gmmvi_custom_data_plan(int N, int64_t rows, int chunks_requested, int* chunks, int* rows_per_chunk) {
    if (N < 1 || rows < 1 || rows > 2147483647ll || chunks_requested < 0 || !chunks || !rows_per_chunk)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_plan needs N >= 1, 1 <= rows < 2^31, "
                                                  "chunks_requested >= 0 and two outputs");
    int64_t want = chunks_requested;
    if (want == 0) {
        const int64_t tiles = ((int64_t)N + 63) / 64;
        const int64_t fill = (GMMVI_DATA_PLAN_CUS + tiles - 1) / tiles;
        const int64_t most = rows / GMMVI_DATA_MIN_CHUNK_ROWS;
        want = fill < most ? fill : most;
    }
    if (want > rows) want = rows;
    if (want > GMMVI_DATA_MAX_CHUNKS) want = GMMVI_DATA_MAX_CHUNKS;
    if (want < 1) want = 1;
    const int64_t per = (rows + want - 1) / want;
    *rows_per_chunk = (int)per;
    *chunks = (int)((rows + per - 1) / per);
    return GMMVI_OK;
}

namespace {
struct RowList {                 // gmmvi_data::RowList of custom_target_data.inc, member for member
    int C;
    unsigned T;
    int minibatch;
    unsigned length;
    unsigned rows_per_chunk;
    unsigned call, hbits, k0, k1;
};
static_assert(sizeof(RowList) == 36, "RowList is a kernel argument: its layout is the device text's");
}  // namespace

// minibatch inside the library: the flag of gmmvi_target_custom_data (0, 1), or own batches, which only the _own_batches entries pass
constexpr int GMMVI_DATA_OWN_BATCHES = 2;

// the refusals the two data modes share, in the order and with the messages of gmmvi_target_custom_data
static int check_data_arguments(gmmvi_ctx* ctx, int D, const float* data_dev, int64_t T, int C, int minibatch, int64_t B,
                                const float* X_dev, int N, const float* lp_out_dev, int chunks_requested) {
    GMMVI_ARG_CHECK(ctx, N >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG && X_dev != nullptr && lp_out_dev != nullptr);
    GMMVI_ARG_CHECK(ctx, data_dev != nullptr && (minibatch == 0 || minibatch == 1) && chunks_requested >= 0);
    if (T < 1 || T > 2147483647ll)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the data set needs 1 <= T < 2^31 rows, got T = " + std::to_string(T));
    if (C < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: a data row needs C >= 1 floats, got C = " + std::to_string(C));
    if (B < 1 || B > T)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the batch size needs 1 <= B <= T = " + std::to_string(T) +
                                                  ", got B = " + std::to_string(B) + " (pass B = T with the full-data mode)");
    return GMMVI_OK;
}

// the launches of the data mode's kernels (fn[0 .. 5] of a handle of either data mode, fn[11 .. 14] in place of fn[0 .. 3] for own
// batches), dual-number gradient or value alone
static int launch_data(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev, const float* data_dev, int64_t T,
                       int C, int minibatch, int64_t B, uint64_t seed, uint32_t call, const float* X_dev, int N, float* lp_out_dev,
                       float* grad_out_dev, int chunks_requested) {
    const bool want_grad = grad_out_dev != nullptr;
    const bool own = minibatch == GMMVI_DATA_OWN_BATCHES;
    const int64_t length = minibatch ? B : T;
    int chunks = 0, rows_per_chunk = 0;
    if (gmmvi_custom_data_plan(N, length, chunks_requested, &chunks, &rows_per_chunk) != GMMVI_OK)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_plan refused N, the row count or the chunk request");
    const bool staged = D <= GMMVI_CUSTOM_STAGED_MAX_DIM;
    const size_t tiles = ((size_t)N + 63) / 64;
    GMMVI_ARG_CHECK(ctx, tiles <= 2147483647u);
    float* part_lp = nullptr;
    float* part_grad = nullptr;
    if (chunks > 1) {
        const size_t f_lp = (size_t)chunks * (size_t)N;
        const int rc = gmmvi_ws_reserve(ctx, f_lp * (want_grad ? (size_t)D + 1 : 1) * sizeof(float));
        if (rc != GMMVI_OK) return rc;
        part_lp = (float*)ctx->ws;
        part_grad = want_grad ? part_lp + f_lp : nullptr;
    }
    RowList l{C, (unsigned)T, minibatch, (unsigned)length, (unsigned)rows_per_chunk, call,
              gmmvi_feistel_half_bits((uint32_t)T), (unsigned)seed, (unsigned)(seed >> 32)};
    float scale = minibatch ? (float)T / (float)B : 1.f;
    // LDS: the waves' accumulators [3][1 or 1 + W][64], then the staged x image [64][D | 1]: 13056 + 30976 B at D = 120
    const size_t lds = ((size_t)3 * (want_grad ? 1 + GMMVI_CUSTOM_AUTODIFF_TANGENTS : 1) * 64 + (staged ? (size_t)64 * (D | 1) : 0)) *
                       sizeof(float);
    {
        void* args[] = {&D, &params_dev, &X_dev, &N, &data_dev, &l, &scale, &lp_out_dev, &grad_out_dev, &part_lp, &part_grad};
        GMMVI_PROF(ctx, own ? "target_custom_data_own" : "target_custom_data");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[(own ? 11 : 0) + (staged ? 0 : 2) + (want_grad ? 1 : 0)], (unsigned)tiles,
                                                   (unsigned)chunks, 1, 256, 1, 1, (unsigned)lds, ctx->stream, args, nullptr));
    }
    if (chunks > 1) {
        const size_t blocks = ((size_t)N + 255) / 256;
        void* args[] = {&D, &params_dev, &X_dev, &N, &chunks, &scale, &lp_out_dev, &grad_out_dev, &part_lp, &part_grad};
        GMMVI_PROF(ctx, "target_custom_data_merge");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[4 + (want_grad ? 1 : 0)], (unsigned)blocks, 1, 1, 256, 1, 1, 0, ctx->stream,
                                                   args, nullptr));
    }
    return GMMVI_OK;
}

// gmmvi_target_custom_data (own == false) and gmmvi_target_custom_data_own_batches (own == true, minibatch == 1): one set of
// refusals, one plan; own batches launch the kernels of their own
static int target_custom_data(const char* entry, gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                              const float* data_dev, int64_t T, int C, int minibatch, bool own, int64_t B, uint64_t seed,
                              uint32_t call, const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                              int chunks_requested) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    if (t->mode == MODE_DATA_TAPE) return refuse_data_tape(ctx);
    if (t->mode != MODE_DATA)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, std::string("invalid argument: ") + entry + " needs a target compiled by "
                                              "gmmvi_custom_target_compile_data; gmmvi_target_custom launches the other two kinds");
    const int rc = check_data_arguments(ctx, D, data_dev, T, C, minibatch, B, X_dev, N, lp_out_dev, chunks_requested);
    if (rc != GMMVI_OK) return rc;
    if (grad_out_dev != nullptr && D > GMMVI_CUSTOM_AUTODIFF_MAX_DIM)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the gradient of a differentiated target needs D <= " +
                                                  std::to_string(GMMVI_CUSTOM_AUTODIFF_MAX_DIM) + ", got D = " + std::to_string(D) +
                                                  " (a value call runs above)");
    return launch_data(ctx, t, D, params_dev, data_dev, T, C, own ? GMMVI_DATA_OWN_BATCHES : minibatch, B, seed, call, X_dev, N,
                       lp_out_dev, grad_out_dev, chunks_requested);
}

extern "C" int gmmvi_target_custom_data(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                        const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed,
                                        uint32_t call, const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                        int chunks_requested) {
    return target_custom_data("gmmvi_target_custom_data", ctx, t, D, params_dev, data_dev, T, C, minibatch, false, B, seed, call, X_dev,
                              N, lp_out_dev, grad_out_dev, chunks_requested);
}

extern "C" int gmmvi_target_custom_data_own_batches(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                                    const float* data_dev, int64_t T, int C, int64_t B, uint64_t seed, uint32_t call,
                                                    const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                                    int chunks_requested) {
    return target_custom_data("gmmvi_target_custom_data_own_batches", ctx, t, D, params_dev, data_dev, T, C, 1, true, B, seed, call,
                              X_dev, N, lp_out_dev, grad_out_dev, chunks_requested);
}

// ---- predictive density of a data-set target: the reduction over the samples -------------------------------------------------------
extern "C" int gmmvi_custom_data_predictive_plan(int N, int64_t M, int chunks_requested, int* tiles, int* chunks,
                                                 int64_t* rows_per_chunk) {
    if (N < 1 || M < 1 || M > 2147483647ll || chunks_requested < 0 || !tiles || !chunks || !rows_per_chunk)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_predictive_plan needs N >= 1, 1 <= M < 2^31, "
                                                  "chunks_requested >= 0 and three outputs");
    int count = 0, per = 0;
    const int rc = gmmvi_custom_data_plan(N, M, chunks_requested, &count, &per);
    if (rc != GMMVI_OK) return rc;
    *tiles = (int)(((int64_t)N + 63) / 64);
    *chunks = count;
    *rows_per_chunk = per;
    return GMMVI_OK;
}

extern "C" int gmmvi_custom_data_predictive(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                            const float* rows_dev, int64_t M, int C, const float* X_dev, int N, float* lpd_out_dev,
                                            float* mean_out_dev, float* var_out_dev, int chunks_requested) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    if (!t || !rows_dev || !X_dev || !lpd_out_dev)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_predictive needs a target handle, rows_dev, X_dev "
                                              "and lpd_out_dev (only mean_out_dev and var_out_dev may be NULL)");
    if (find_target(ctx, t) == ctx->custom_targets.end())
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the custom target does not belong to this context");
    if (t->mode != MODE_DATA && t->mode != MODE_DATA_TAPE)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_predictive needs a target compiled by "
                                              "gmmvi_custom_target_compile_data or gmmvi_custom_target_compile_data_tape (a row term "
                                              "to evaluate on held-out rows); this handle has none");
    if (N < 1) return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the predictive density needs N >= 1 samples, got N = " + std::to_string(N));
    if (M < 1 || M > 2147483647ll)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the evaluation set needs 1 <= M < 2^31 rows, got M = " + std::to_string(M));
    if (C < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: a data row needs C >= 1 floats, got C = " + std::to_string(C));
    if (D < 1 || D > GMMVI_MAX_DIM_DIAG)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the predictive density needs 1 <= D <= " +
                                                  std::to_string(GMMVI_MAX_DIM_DIAG) + ", got D = " + std::to_string(D));
    GMMVI_ARG_CHECK(ctx, chunks_requested >= 0);
    int tiles = 0, chunks = 0;
    int64_t per64 = 0;
    if (gmmvi_custom_data_predictive_plan(N, M, chunks_requested, &tiles, &chunks, &per64) != GMMVI_OK)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, g_gmmvi_global_err);
    float* part = nullptr;
    if (tiles > 1) {                                                 // [tiles][M] partials of (max, sumexp, mean, M2)
        const int rc = gmmvi_ws_reserve(ctx, (size_t)tiles * (size_t)M * 4 * sizeof(float));
        if (rc != GMMVI_OK) return rc;
        part = (float*)ctx->ws;
    }
    const bool staged = D <= GMMVI_CUSTOM_STAGED_MAX_DIM;
    const size_t lds = staged ? (size_t)64 * (D | 1) * sizeof(float) : 0;   // the x image [64][D | 1]: 30976 B at D = 120
    unsigned rows = (unsigned)M, per = (unsigned)per64;
    {
        void* args[] = {&D, &params_dev, &X_dev, &N, &rows_dev, &rows, &C, &per, &part, &lpd_out_dev, &mean_out_dev, &var_out_dev};
        GMMVI_PROF(ctx, "custom_data_predictive");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[staged ? 8 : 9], (unsigned)tiles, (unsigned)chunks, 1, 256, 1, 1, (unsigned)lds,
                                                   ctx->stream, args, nullptr));
    }
    if (tiles > 1) {
        const size_t blocks = ((size_t)M + 255) / 256;
        void* args[] = {&N, &rows, &tiles, &part, &lpd_out_dev, &mean_out_dev, &var_out_dev};
        GMMVI_PROF(ctx, "custom_data_predictive_merge");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[10], (unsigned)blocks, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
    }
    return GMMVI_OK;
}

// ---- targets differentiated on a tape ----------------------------------------------------------------------------------------
// The slab plan: a wave of 64 lanes takes 64 * capacity records of GMMVI_CUSTOM_TAPE_RECORD_BYTES (16 B of record, 4 B of
// adjoint).  As many whole waves as the budget holds form a slab; the slabs are then as even as whole waves allow, and the count
// is what that slab size needs: the last slab is never empty.
static size_t tape_wave_bytes(int capacity) { return (size_t)64 * (size_t)capacity * GMMVI_CUSTOM_TAPE_RECORD_BYTES; }

extern "C" int gmmvi_custom_tape_plan(int N, int capacity, size_t scratch_bytes, int* slabs, int* lanes_per_slab) {
    if (N < 1 || capacity < 1 || !slabs || !lanes_per_slab)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_tape_plan needs N >= 1, capacity >= 1 and two outputs");
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)GMMVI_CUSTOM_TAPE_SCRATCH_BYTES;
    const size_t fit = budget / tape_wave_bytes(capacity);
    if (fit < 1)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: a tape of " + std::to_string(capacity) + " records per lane takes " +
                                                      std::to_string(tape_wave_bytes(capacity)) + " bytes for 64 lanes, the scratch "
                                                      "budget is " + std::to_string(budget) + " bytes");
    const size_t waves = ((size_t)N + 63) / 64;
    const size_t most = fit < waves ? fit : waves;
    const size_t want = (waves + most - 1) / most;
    const size_t per = (waves + want - 1) / want;
    *lanes_per_slab = (int)(per * 64);
    *slabs = (int)((waves + per - 1) / per);
    return GMMVI_OK;
}

static int tape_length(const gmmvi_custom_target* t, int D) {
    for (const auto& e : t->tape_lengths)
        if (e.first == D) return e.second;
    return 0;
}

extern "C" int gmmvi_custom_tape_length(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, int* length) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end() && length != nullptr);
    *length = tape_length(t, D);
    return GMMVI_OK;
}

extern "C" int gmmvi_target_custom_tape(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                        const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev, int tape_capacity,
                                        size_t scratch_bytes) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    if (t->mode == MODE_DATA_TAPE) return refuse_data_tape(ctx);
    if (t->mode != MODE_TAPE)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: gmmvi_target_custom_tape needs a target compiled by "
                                              "gmmvi_custom_target_compile_tape; gmmvi_target_custom and gmmvi_target_custom_data "
                                              "launch the other kinds");
    GMMVI_ARG_CHECK(ctx, N >= 1 && D >= 1 && D <= GMMVI_MAX_DIM_DIAG && X_dev != nullptr && lp_out_dev != nullptr);
    GMMVI_ARG_CHECK(ctx, tape_capacity >= 0);
    if (!grad_out_dev) {
        const size_t blocks = ((size_t)N + 255) / 256;
        void* args[] = {&D, &params_dev, &X_dev, &N, &lp_out_dev};
        GMMVI_PROF(ctx, "target_custom_tape");
        GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[0], (unsigned)blocks, 1, 1, 256, 1, 1, 0, ctx->stream, args, nullptr));
        return GMMVI_OK;
    }
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)GMMVI_CUSTOM_TAPE_SCRATCH_BYTES;
    size_t longest = budget / tape_wave_bytes(1);                     // the longest tape 64 lanes can have within the budget
    if (longest > (size_t)1 << 30) longest = (size_t)1 << 30;         // node ids are ints: D + record
    if (longest < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: a scratch budget of " + std::to_string(budget) +
                                                  " bytes holds no tape: one record of 64 lanes takes " +
                                                  std::to_string(tape_wave_bytes(1)) + " bytes");
    int cap = tape_capacity > 0 ? tape_capacity : tape_length(t, D);
    if (cap < 1) cap = GMMVI_CUSTOM_TAPE_DEFAULT_CAPACITY;
    if ((size_t)cap > longest) cap = (int)longest;                    // the launch tells what is needed: refused below if that is more
    for (int attempt = 0; attempt < 2; ++attempt) {
        int slabs = 0, lanes = 0;
        if (gmmvi_custom_tape_plan(N, cap, budget, &slabs, &lanes) != GMMVI_OK)
            return gmmvi_fail(ctx, GMMVI_ERR_ARG, g_gmmvi_global_err);
        // scratch: [needed length, padded to 256 B | records [lanes / 64][cap][64] | adjoints, the same shape]
        const size_t f_rec = (size_t)lanes * (size_t)cap;
        const int rc = gmmvi_ws_reserve(ctx, 256 + f_rec * GMMVI_CUSTOM_TAPE_RECORD_BYTES);
        if (rc != GMMVI_OK) return rc;
        int* needed_dev = (int*)ctx->ws;
        char* rec = (char*)ctx->ws + 256;
        float* adj = (float*)(rec + f_rec * 16);
        GMMVI_HIP_CHECK(ctx, hipMemsetAsync(needed_dev, 0, sizeof(int), ctx->stream));
        for (int s = 0; s < slabs; ++s) {
            int first = s * lanes;
            const int rest = N - first;
            const unsigned waves = (unsigned)(((rest < lanes ? rest : lanes) + 63) / 64);
            void* args[] = {&D, &params_dev, &X_dev, &N, &lp_out_dev, &grad_out_dev, &first, &rec, &adj, &cap, &needed_dev};
            GMMVI_PROF(ctx, "target_custom_tape");
            GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[1], waves, 1, 1, 64, 1, 1, 0, ctx->stream, args, nullptr));
        }
        int needed = 0;
        GMMVI_HIP_CHECK(ctx, hipMemcpyAsync(&needed, needed_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        GMMVI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        bool known = false;
        for (auto& e : t->tape_lengths)
            if (e.first == D) { known = true; if (needed > e.second) e.second = needed; }
        if (!known) t->tape_lengths.emplace_back(D, needed);
        if (needed <= cap) return GMMVI_OK;
        if ((size_t)needed > longest)
            return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the target needs a tape of " + std::to_string(needed) +
                                                      " records per lane at D = " + std::to_string(D) + ", which takes " +
                                                      std::to_string(tape_wave_bytes(needed)) + " bytes for 64 lanes; the scratch "
                                                      "budget is " + std::to_string(budget) + " bytes (lp_out_dev is written, "
                                                      "grad_out_dev is not complete)");
        cap = needed;
    }
    return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the tape of the target grew between two launches on the same samples: "
                                          "gmmvi_user_density is not a pure function of x, D and params");
}

// ---- targets summed over a data set, differentiated on a tape --------------------------------------------------------------------
// The plan.  A wave (one tile of 64 samples, one chunk of the row list) takes 64 * (capacity * GMMVI_CUSTOM_TAPE_RECORD_BYTES +
// 4 D) bytes: its tape and its [D][64] gradient accumulator.  Chunks first: the request, or enough chunks that tiles * chunks
// waves reach GMMVI_DATA_TAPE_PLAN_WAVES (four waves on each compute unit of an MI355X) but no more than rows /
// GMMVI_DATA_TAPE_MIN_CHUNK_ROWS; either way at most one per row and at most as many as the budget holds waves, then as even as
// whole rows allow.  Then slabs: as many tiles as the budget holds with that many chunks each, as even as whole tiles allow.
// Neither constant is measured: they restate the rule of gmmvi_custom_data_plan for one-wave workgroups.
constexpr int64_t GMMVI_DATA_TAPE_PLAN_WAVES = 4 * GMMVI_DATA_PLAN_CUS;
constexpr int64_t GMMVI_DATA_TAPE_MIN_CHUNK_ROWS = 8;

static size_t data_tape_wave_bytes(int D, int capacity) {
    return (size_t)64 * ((size_t)capacity * GMMVI_CUSTOM_TAPE_RECORD_BYTES + 4 * (size_t)D);
}

extern "C" int gmmvi_custom_data_tape_plan(int N, int64_t rows, int D, int capacity, int chunks_requested, size_t scratch_bytes,
                                           int* chunks, int* rows_per_chunk, int* slabs, int* tiles_per_slab) {
    if (N < 1 || rows < 1 || rows > 2147483647ll || D < 1 || D > GMMVI_MAX_DIM_DIAG || capacity < 1 || chunks_requested < 0 ||
        !chunks || !rows_per_chunk || !slabs || !tiles_per_slab)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: gmmvi_custom_data_tape_plan needs N >= 1, 1 <= rows < 2^31, "
                                                  "1 <= D <= " + std::to_string(GMMVI_MAX_DIM_DIAG) + ", capacity >= 1, "
                                                  "chunks_requested >= 0 and four outputs");
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)GMMVI_CUSTOM_TAPE_SCRATCH_BYTES;
    const size_t wave = data_tape_wave_bytes(D, capacity);
    const int64_t fit = (int64_t)(budget / wave);                    // waves the budget holds
    if (fit < 1)
        return gmmvi_fail(nullptr, GMMVI_ERR_ARG, "invalid argument: a tape of " + std::to_string(capacity) + " records per lane and "
                                                      "the gradient accumulator at D = " + std::to_string(D) + " take " +
                                                      std::to_string(wave) + " bytes for 64 lanes, the scratch budget is " +
                                                      std::to_string(budget) + " bytes");
    const int64_t tiles = ((int64_t)N + 63) / 64;
    int64_t want = chunks_requested;
    if (want == 0) {
        const int64_t fill = (GMMVI_DATA_TAPE_PLAN_WAVES + tiles - 1) / tiles;
        const int64_t most = rows / GMMVI_DATA_TAPE_MIN_CHUNK_ROWS;
        want = fill < most ? fill : most;
    }
    if (want > rows) want = rows;
    if (want > GMMVI_DATA_MAX_CHUNKS) want = GMMVI_DATA_MAX_CHUNKS;
    if (want > fit) want = fit;
    if (want < 1) want = 1;
    const int64_t per = (rows + want - 1) / want;
    const int64_t count = (rows + per - 1) / per;
    const int64_t hold = fit / count < tiles ? fit / count : tiles;  // tiles a slab can hold, >= 1
    const int64_t need = (tiles + hold - 1) / hold;
    const int64_t each = (tiles + need - 1) / need;
    *chunks = (int)count;
    *rows_per_chunk = (int)per;
    *tiles_per_slab = (int)each;
    *slabs = (int)((tiles + each - 1) / each);
    return GMMVI_OK;
}

// gmmvi_target_custom_data_tape (own == false) and gmmvi_target_custom_data_tape_own_batches (own == true, minibatch == 1)
static int target_custom_data_tape(const char* entry, gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                   const float* data_dev, int64_t T, int C, int minibatch, bool own, int64_t B, uint64_t seed,
                                   uint32_t call, const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                   int chunks_requested, int tape_capacity, size_t scratch_bytes) {
    GMMVI_ARG_CHECK(ctx, ctx != nullptr);
    GMMVI_ARG_CHECK(ctx, t != nullptr && find_target(ctx, t) != ctx->custom_targets.end());
    if (t->mode != MODE_DATA_TAPE)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, std::string("invalid argument: ") + entry + " needs a target compiled by "
                                              "gmmvi_custom_target_compile_data_tape; gmmvi_target_custom, gmmvi_target_custom_data "
                                              "and gmmvi_target_custom_tape launch the other kinds");
    const int rc = check_data_arguments(ctx, D, data_dev, T, C, minibatch, B, X_dev, N, lp_out_dev, chunks_requested);
    if (rc != GMMVI_OK) return rc;
    GMMVI_ARG_CHECK(ctx, tape_capacity >= 0);
    if (own) minibatch = GMMVI_DATA_OWN_BATCHES;
    if (!grad_out_dev)                                               // the data mode's value call: its kernels, its plan, its bits
        return launch_data(ctx, t, D, params_dev, data_dev, T, C, minibatch, B, seed, call, X_dev, N, lp_out_dev, nullptr,
                           chunks_requested);
    const size_t budget = scratch_bytes ? scratch_bytes : (size_t)GMMVI_CUSTOM_TAPE_SCRATCH_BYTES;
    // the longest tape 64 lanes can have within the budget, beside their accumulator
    size_t longest = budget / 64 > 4 * (size_t)D ? (budget / 64 - 4 * (size_t)D) / GMMVI_CUSTOM_TAPE_RECORD_BYTES : 0;
    if (longest > (size_t)1 << 30) longest = (size_t)1 << 30;        // node ids are ints: D + record
    if (longest < 1)
        return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: a scratch budget of " + std::to_string(budget) +
                                                  " bytes holds no tape at D = " + std::to_string(D) + ": one record and the gradient "
                                                  "accumulator of 64 lanes take " + std::to_string(data_tape_wave_bytes(D, 1)) +
                                                  " bytes");
    int cap = tape_capacity > 0 ? tape_capacity : tape_length(t, D);
    if (cap < 1) cap = GMMVI_CUSTOM_TAPE_DEFAULT_CAPACITY;
    if ((size_t)cap > longest) cap = (int)longest;                   // the launch tells what is needed: refused below if that is more
    const int64_t length = minibatch ? B : T;
    RowList l{C, (unsigned)T, minibatch, (unsigned)length, 0u, call, gmmvi_feistel_half_bits((uint32_t)T), (unsigned)seed,
              (unsigned)(seed >> 32)};
    float scale = minibatch ? (float)T / (float)B : 1.f;
    for (int attempt = 0; attempt < 2; ++attempt) {
        int chunks = 0, per = 0, slabs = 0, tiles_per_slab = 0;
        if (gmmvi_custom_data_tape_plan(N, length, D, cap, chunks_requested, budget, &chunks, &per, &slabs, &tiles_per_slab) != GMMVI_OK)
            return gmmvi_fail(ctx, GMMVI_ERR_ARG, g_gmmvi_global_err);
        l.rows_per_chunk = (unsigned)per;
        // scratch: [needed length, padded to 256 B | records [waves][cap][64] | adjoints, the same shape | accumulators [waves][D][64]]
        const size_t waves = (size_t)tiles_per_slab * (size_t)chunks;
        const size_t f_rec = waves * 64 * (size_t)cap;
        const int rc2 = gmmvi_ws_reserve(ctx, 256 + waves * data_tape_wave_bytes(D, cap));
        if (rc2 != GMMVI_OK) return rc2;
        int* needed_dev = (int*)ctx->ws;
        char* rec = (char*)ctx->ws + 256;
        float* adj = (float*)(rec + f_rec * 16);
        float* acc = adj + f_rec;
        GMMVI_HIP_CHECK(ctx, hipMemsetAsync(needed_dev, 0, sizeof(int), ctx->stream));
        const int tiles = (N + 63) / 64;
        for (int s = 0; s < slabs; ++s) {
            int first_tile = s * tiles_per_slab;
            const unsigned here = (unsigned)(tiles - first_tile < tiles_per_slab ? tiles - first_tile : tiles_per_slab);
            {
                void* args[] = {&D, &params_dev, &X_dev, &N, &data_dev, &l, &first_tile, &rec, &adj, &acc, &cap, &needed_dev};
                GMMVI_PROF(ctx, own ? "target_custom_data_tape_own" : "target_custom_data_tape");
                GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[own ? 15 : 6], here, (unsigned)chunks, 1, 64, 1, 1, 0, ctx->stream, args, nullptr));
            }
            {
                void* args[] = {&D, &params_dev, &X_dev, &N, &chunks, &scale, &first_tile, &rec, &adj, &acc, &cap, &needed_dev,
                                &lp_out_dev, &grad_out_dev};
                GMMVI_PROF(ctx, "target_custom_data_tape_finish");
                GMMVI_HIP_CHECK(ctx, hipModuleLaunchKernel(t->fn[7], here, 1, 1, 64, 1, 1, 0, ctx->stream, args, nullptr));
            }
        }
        int needed = 0;
        GMMVI_HIP_CHECK(ctx, hipMemcpyAsync(&needed, needed_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        GMMVI_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (needed < 1) needed = 1;                                  // constants alone: one slot still carries the chunk's value
        bool known = false;
        for (auto& e : t->tape_lengths)
            if (e.first == D) { known = true; if (needed > e.second) e.second = needed; }
        if (!known) t->tape_lengths.emplace_back(D, needed);
        if (needed <= cap) return GMMVI_OK;
        if ((size_t)needed > longest)
            return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the target needs a tape of " + std::to_string(needed) +
                                                      " records per lane at D = " + std::to_string(D) + ", which takes " +
                                                      std::to_string(data_tape_wave_bytes(D, needed)) + " bytes for 64 lanes with "
                                                      "their gradient accumulator; the scratch budget is " + std::to_string(budget) +
                                                      " bytes (lp_out_dev is written, grad_out_dev is not complete)");
        cap = needed;
    }
    return gmmvi_fail(ctx, GMMVI_ERR_ARG, "invalid argument: the tape of the target grew between two launches on the same samples and "
                                          "rows: gmmvi_user_row or gmmvi_user_prior is not a pure function of x, D, the row and params");
}

extern "C" int gmmvi_target_custom_data_tape(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev,
                                             const float* data_dev, int64_t T, int C, int minibatch, int64_t B, uint64_t seed,
                                             uint32_t call, const float* X_dev, int N, float* lp_out_dev, float* grad_out_dev,
                                             int chunks_requested, int tape_capacity, size_t scratch_bytes) {
    return target_custom_data_tape("gmmvi_target_custom_data_tape", ctx, t, D, params_dev, data_dev, T, C, minibatch, false, B, seed,
                                   call, X_dev, N, lp_out_dev, grad_out_dev, chunks_requested, tape_capacity, scratch_bytes);
}

extern "C" int gmmvi_target_custom_data_tape_own_batches(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D,
                                                         const float* params_dev, const float* data_dev, int64_t T, int C, int64_t B,
                                                         uint64_t seed, uint32_t call, const float* X_dev, int N, float* lp_out_dev,
                                                         float* grad_out_dev, int chunks_requested, int tape_capacity,
                                                         size_t scratch_bytes) {
    return target_custom_data_tape("gmmvi_target_custom_data_tape_own_batches", ctx, t, D, params_dev, data_dev, T, C, 1, true, B, seed,
                                   call, X_dev, N, lp_out_dev, grad_out_dev, chunks_requested, tape_capacity, scratch_bytes);
}
