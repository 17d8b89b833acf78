// User-defined targets compiled at run time (include/gmmvi_hip.h, "user-defined device targets"): the text pieces of the mode's
// row of kModes go behind the user's source, hiprtc compiles the whole for the device of the context, and the code object's
// kernels are loaded into a handle, which custom_target.hip, custom_data.hip and custom_tape.hip launch on the context's stream.
// hiprtc is bound with dlopen on first use: the library links without it, and only a call that needs the compiler can miss it.
// MODE_DATA_TAPE repeats the whole text of MODE_DATA because the value kernels of that mode are its value call as well.
#include "custom_target.h"
#include <hip/hiprtc.h>
#include <dlfcn.h>

static const char* const kWrapText =
#include "custom_target_wrap.inc"
    ;
static const char* const kSpecialText =                                   // the float functions: special, then the vector primitives
#include "custom_target_special.inc"
#include "custom_target_vector.inc"
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
static const char* const kLine = "\n";
// Goes in front of the user's first line, on that line: a float has no namespace for argument-dependent lookup to search, so
// the float instantiation of the user's template finds gmmvi_value, the nine functions of custom_target_special.inc and the six
// of custom_target_vector.inc only if they are declared before the template.  The hand-written mode gets the same line: its float
// code calls them too.  gmmvi_wdot, gmmvi_logsumexp and gmmvi_affine on an array of duals or nodes are found by argument-dependent lookup at
// the point of instantiation, in gmmvi_ad and gmmvi_tape: every row of kModes puts kSpecialText, which holds the two value
// templates they call, in front of the number types, and the number types in front of the kernels that instantiate the user's
// template with them.
static const char* const kAutodiffPrelude =
    "__host__ __device__ inline float gmmvi_value(float); __host__ __device__ inline float gmmvi_digamma(float); "
    "__host__ __device__ inline float gmmvi_trigamma(float); __host__ __device__ inline float gmmvi_sigmoid(float); "
    "__host__ __device__ inline float gmmvi_softplus(float); __host__ __device__ inline float gmmvi_log_sigmoid(float); "
    "__host__ __device__ inline float gmmvi_logaddexp(float, float); __host__ __device__ inline float gmmvi_erfcx(float); "
    "__host__ __device__ inline float gmmvi_ndtr(float); __host__ __device__ inline float gmmvi_log_ndtr(float); "
    "__host__ __device__ inline float gmmvi_dot(const float*, int, const float*, int); "
    "__host__ __device__ inline float gmmvi_sqdist(const float*, int, const float*, int); "
    "__host__ __device__ inline float gmmvi_sumsq(const float*, int, int, float); "
    "__host__ __device__ inline float gmmvi_wdot(const float*, int, const float*, int); "
    "__host__ __device__ inline float gmmvi_logsumexp(const float*, int); "
    "__host__ __device__ inline void gmmvi_affine(const float*, int, int, int, int, int, const float*, int, float*, int); ";
#define GMMVI_STR2(x) #x
#define GMMVI_STR(x) GMMVI_STR2(x)

// ---- the mode table ---------------------------------------------------------------------------------------------------------
namespace {
struct ModeRow {                          // every list ends at its first null / E_NONE / K_NONE
    const char* compile_entry;            // the public entry that makes a handle of this mode
    const char* user_entries[3];          // what the source has to define
    const char* pieces[11];               // the text behind the user's source, in this order
    const char* defines[7];               // the options behind --offload-arch, -O3 and -std=c++17, in this order
    Entry launchers[4];                   // the entries that accept the handle
    KernelSlot kernels[K_COUNT];          // what the handle holds
};

#define GMMVI_TANGENTS_OPT "-DGMMVI_CUSTOM_AUTODIFF_TANGENTS=" GMMVI_STR(GMMVI_CUSTOM_AUTODIFF_TANGENTS)
#define GMMVI_WRAP_KERNELS K_STAGED_LP, K_STAGED_GRAD, K_DIRECT_LP, K_DIRECT_GRAD
// the dual numbers without their adapter, the tile mover of the wrapper text, then the Feistel stream and the kernels
#define GMMVI_DATA_PIECES kSpecialText, kAutodiffText, kLine, kWrapText, kLine, kDataText
#define GMMVI_DATA_OPTS GMMVI_TANGENTS_OPT, "-DGMMVI_AD_NO_ADAPTER", "-DGMMVI_WRAP_TILE_ONLY"
#define GMMVI_DATA_KERNELS                                                                                                         \
    K_DATA_ROWS_STAGED_LP, K_DATA_ROWS_STAGED_GRAD, K_DATA_ROWS_DIRECT_LP, K_DATA_ROWS_DIRECT_GRAD, K_DATA_ROWS_OWN_STAGED_LP,    \
        K_DATA_ROWS_OWN_STAGED_GRAD, K_DATA_ROWS_OWN_DIRECT_LP, K_DATA_ROWS_OWN_DIRECT_GRAD, K_DATA_MERGE_LP, K_DATA_MERGE_GRAD,  \
        K_PRED_STAGED, K_PRED_DIRECT, K_PRED_MERGE

const ModeRow kModes[MODE_COUNT] = {
    // MODE_HAND, MODE_AUTODIFF
    {"gmmvi_custom_target_compile", {"gmmvi_user_target"}, {kSpecialText, kLine, kWrapText}, {}, {E_TARGET}, {GMMVI_WRAP_KERNELS}},
    {"gmmvi_custom_target_compile_autodiff", {"gmmvi_user_density"}, {kSpecialText, kAutodiffText, kLine, kWrapText},
     {GMMVI_TANGENTS_OPT}, {E_TARGET}, {GMMVI_WRAP_KERNELS}},
    // MODE_DATA
    {"gmmvi_custom_target_compile_data", {"gmmvi_user_row", "gmmvi_user_prior"}, {GMMVI_DATA_PIECES}, {GMMVI_DATA_OPTS},
     {E_DATA, E_DATA_OWN, E_PREDICTIVE}, {GMMVI_DATA_KERNELS}},
    // MODE_TAPE: the source of MODE_AUTODIFF, unchanged
    {"gmmvi_custom_target_compile_tape", {"gmmvi_user_density"}, {kSpecialText, kTapeText},
     {GMMVI_TANGENTS_OPT, "-DGMMVI_CUSTOM_TAPE=1"}, {E_TAPE}, {K_TAPE_LP, K_TAPE_GRAD}},
    // MODE_DATA_TAPE: the source of MODE_DATA, unchanged; the tape's number type without its kernels
    {"gmmvi_custom_target_compile_data_tape", {"gmmvi_user_row", "gmmvi_user_prior"},
     {GMMVI_DATA_PIECES, kLine, kTapeText, kLine, kDataTapeText},
     {GMMVI_DATA_OPTS, "-DGMMVI_TAPE_NO_KERNELS", "-DGMMVI_TAPE_NO_FLOAT_VALUE", "-DGMMVI_CUSTOM_TAPE=1"},
     {E_DATA_TAPE, E_DATA_TAPE_OWN, E_PREDICTIVE}, {GMMVI_DATA_KERNELS, K_DATA_TAPE_ROWS, K_DATA_TAPE_ROWS_OWN, K_DATA_TAPE_FINISH}},
};
static_assert(MODE_HAND == 0 && MODE_AUTODIFF == 1 && MODE_DATA == 2 && MODE_TAPE == 3 && MODE_DATA_TAPE == 4, "the order of kModes");

const char* const kEntryNames[E_COUNT] = {nullptr, GMMVI_CUSTOM_ENTRIES(GMMVI_X_NAME)};
const char* const kKernelNames[K_COUNT] = {nullptr, GMMVI_CUSTOM_KERNELS(GMMVI_X_NAME)};

bool accepts(const ModeRow& row, Entry entry) {
    return std::find(std::begin(row.launchers), std::end(row.launchers), entry) != std::end(row.launchers);
}
}  // namespace

int gmmvi_custom_check_mode(gmmvi_ctx* ctx, Entry entry, const gmmvi_custom_target* t) {
    const ModeRow& mine = kModes[t->mode];
    if (accepts(mine, entry)) return GMMVI_OK;
    std::string takes, launch;
    for (const ModeRow& row : kModes)
        if (accepts(row, entry)) takes += std::string(takes.empty() ? "" : " or ") + row.compile_entry;
    for (Entry e : mine.launchers)
        if (e != E_NONE) launch += std::string(launch.empty() ? "" : " or ") + kEntryNames[e];
    return gmmvi_fail(ctx, GMMVI_ERR_ARG, std::string("invalid argument: ") + kEntryNames[entry] + " takes a target compiled by " +
                                              takes + "; this one was compiled by " + mine.compile_entry + ": pass it to " + launch);
}

// ---- the run-time compiler --------------------------------------------------------------------------------------------------
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

// user's text + the pieces of the mode's row -> code object for `arch`.  GMMVI_OK, or the status with the compiler log / reason
// in `log`.  The user's text stays first (behind one declaration on its first line): the compiler's line numbers are the user's.
int compile_source(const char* source, Mode mode, const char* arch, std::vector<char>& code, std::string& log) {
    const Hiprtc& rt = hiprtc();
    if (!rt.why.empty()) { log = rt.why; return GMMVI_ERR_HIP; }
    const ModeRow& row = kModes[mode];
    std::string text = kAutodiffPrelude;
    if (source[strspn(source, " \t")] == '#') text += "\n#line 1\n";   // a directive has to begin its line; the numbers stay the user's
    text += std::string(source) + "\n";
    for (const char* piece : row.pieces)
        if (piece) text += piece;
    hiprtcProgram prog = nullptr;
    hiprtcResult r = rt.create(&prog, text.c_str(), "gmmvi_user_target.hip", 0, nullptr, nullptr);
    if (r != HIPRTC_SUCCESS) { log = std::string("hiprtcCreateProgram: ") + rt.error_string(r); return GMMVI_ERR_HIP; }
    const std::string arch_opt = std::string("--offload-arch=") + arch;
    std::vector<const char*> opts = {arch_opt.c_str(), "-O3", "-std=c++17"};
    for (const char* define : row.defines)
        if (define) opts.push_back(define);
    // the node-array record (custom_target_tape.inc): its overloads and its branch of the sweep only where the text names them
    const bool affine = strstr(source, "gmmvi_affine") != nullptr;     // its record group: headers of the node-array kind
    if (affine || strstr(source, "gmmvi_wdot") || strstr(source, "gmmvi_logsumexp")) opts.push_back("-DGMMVI_TAPE_NODES=1");
    if (affine) opts.push_back("-DGMMVI_TAPE_AFFINE=1");
    r = rt.compile(prog, (int)opts.size(), opts.data());
    size_t n = 0;
    if (rt.log_size(prog, &n) == HIPRTC_SUCCESS && n > 1) {
        log.resize(n);
        if (rt.log(prog, &log[0]) != HIPRTC_SUCCESS) log.clear();
        while (!log.empty() && log.back() == '\0') log.pop_back();
    }
    int rc = GMMVI_OK;
    if (r != HIPRTC_SUCCESS) {
        std::string head = std::string("user target does not compile (") + rt.error_string(r) + ")";
        for (const char* entry : row.user_entries)
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
    hipError_t e = hipSetDevice(ctx->device);
    if (e == hipSuccess) e = hipModuleLoadData(&t->module, code.data());
    for (KernelSlot k : kModes[mode].kernels)
        if (e == hipSuccess && k != K_NONE) e = hipModuleGetFunction(&t->fn[k], t->module, kKernelNames[k]);
    if (e != hipSuccess) {
        if (t->module) (void)hipModuleUnload(t->module);
        delete t;
        return gmmvi_fail(ctx, GMMVI_ERR_HIP, std::string("loading the code object of a user target: ") + hipGetErrorString(e));
    }
    ctx->custom_targets.push_back(t);
    *out = t;
    return GMMVI_OK;
}

// the check and the compile entry of each mode: gmmvi_custom_target_check<suffix>, gmmvi_custom_target_compile<suffix>
#define GMMVI_MODE_ENTRIES(suffix, mode)                                                                                        \
    extern "C" int gmmvi_custom_target_check##suffix(const char* source, const char* arch, char* log_out, size_t log_cap) {     \
        return check_source("gmmvi_custom_target_check" #suffix, source, mode, arch, log_out, log_cap);                         \
    }                                                                                                                           \
    extern "C" int gmmvi_custom_target_compile##suffix(gmmvi_ctx* ctx, const char* source, gmmvi_custom_target** out) {         \
        return compile_target(ctx, source, mode, out);                                                                          \
    }
GMMVI_MODE_ENTRIES(, MODE_HAND)
GMMVI_MODE_ENTRIES(_autodiff, MODE_AUTODIFF)
GMMVI_MODE_ENTRIES(_data, MODE_DATA)
GMMVI_MODE_ENTRIES(_tape, MODE_TAPE)
GMMVI_MODE_ENTRIES(_data_tape, MODE_DATA_TAPE)

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
