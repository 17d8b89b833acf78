// User-defined targets compiled at run time, what their four host files share: custom_compile.hip fills a handle from its mode's
// row of the mode table; custom_target.hip, custom_data.hip and custom_tape.hip launch the kernels it holds.
#pragma once
#include "common.h"
#include <algorithm>
#include <map>

// the source defines gmmvi_user_target; gmmvi_user_density; gmmvi_user_row and gmmvi_user_prior; then the last two again
enum Mode { MODE_HAND, MODE_AUTODIFF, MODE_DATA, MODE_TAPE, MODE_DATA_TAPE, MODE_COUNT };

// X(slot, public name) of the entries that launch from a handle; a mode's row lists those that accept it
#define GMMVI_CUSTOM_ENTRIES(X)                                                                                                   \
    X(E_TARGET, "gmmvi_target_custom") X(E_DATA, "gmmvi_target_custom_data") X(E_DATA_OWN, "gmmvi_target_custom_data_own_batches") \
    X(E_TAPE, "gmmvi_target_custom_tape") X(E_DATA_TAPE, "gmmvi_target_custom_data_tape")                                         \
    X(E_DATA_TAPE_OWN, "gmmvi_target_custom_data_tape_own_batches") X(E_PREDICTIVE, "gmmvi_custom_data_predictive")
// X(slot, symbol) of the kernels a handle can hold; it holds those its mode's row lists
#define GMMVI_CUSTOM_KERNELS(X)                                                                                           \
    X(K_STAGED_LP, "gmmvi_custom_staged_lp") X(K_STAGED_GRAD, "gmmvi_custom_staged_grad") X(K_DIRECT_LP, "gmmvi_custom_direct_lp") \
    X(K_DIRECT_GRAD, "gmmvi_custom_direct_grad") X(K_DATA_MERGE_LP, "gmmvi_data_merge_lp") X(K_DATA_MERGE_GRAD, "gmmvi_data_merge_grad") \
    X(K_DATA_ROWS_STAGED_LP, "gmmvi_data_rows_staged_lp") X(K_DATA_ROWS_STAGED_GRAD, "gmmvi_data_rows_staged_grad")       \
    X(K_DATA_ROWS_DIRECT_LP, "gmmvi_data_rows_direct_lp") X(K_DATA_ROWS_DIRECT_GRAD, "gmmvi_data_rows_direct_grad")       \
    X(K_DATA_ROWS_OWN_STAGED_LP, "gmmvi_data_rows_own_staged_lp") X(K_DATA_ROWS_OWN_STAGED_GRAD, "gmmvi_data_rows_own_staged_grad") \
    X(K_DATA_ROWS_OWN_DIRECT_LP, "gmmvi_data_rows_own_direct_lp") X(K_DATA_ROWS_OWN_DIRECT_GRAD, "gmmvi_data_rows_own_direct_grad") \
    X(K_PRED_STAGED, "gmmvi_data_predictive_staged") X(K_PRED_DIRECT, "gmmvi_data_predictive_direct")                     \
    X(K_PRED_MERGE, "gmmvi_data_predictive_merge") X(K_TAPE_LP, "gmmvi_tape_lp") X(K_TAPE_GRAD, "gmmvi_tape_grad")        \
    X(K_DATA_TAPE_ROWS, "gmmvi_data_tape_rows") X(K_DATA_TAPE_ROWS_OWN, "gmmvi_data_tape_rows_own") X(K_DATA_TAPE_FINISH, "gmmvi_data_tape_finish")
#define GMMVI_X_SLOT(slot, name) slot,
#define GMMVI_X_NAME(slot, name) name,
enum Entry { E_NONE, GMMVI_CUSTOM_ENTRIES(GMMVI_X_SLOT) E_COUNT };          // E_NONE and K_NONE end a row's list
enum KernelSlot { K_NONE, GMMVI_CUSTOM_KERNELS(GMMVI_X_SLOT) K_COUNT };

struct gmmvi_custom_target {
    uint64_t hash = 0;
    std::string source;
    Mode mode = MODE_HAND;
    int refs = 0;
    hipModule_t module = nullptr;
    hipFunction_t fn[K_COUNT] = {};                          // by KernelSlot; null where the mode's row does not list the slot
    mutable std::map<int, int> tape_lengths;                 // the tape modes: D -> the longest tape a gradient launch at that D has needed
};

inline auto find_target(gmmvi_ctx* ctx, const gmmvi_custom_target* t) {
    return std::find(ctx->custom_targets.begin(), ctx->custom_targets.end(), t);
}

// custom_compile.hip: GMMVI_OK where the row of t's mode lists `entry`; else the refusal, which names the compile entry the
// handle came from and the entries that launch it
int gmmvi_custom_check_mode(gmmvi_ctx* ctx, Entry entry, const gmmvi_custom_target* t);

// ---- custom_data.hip, for the data-tape entries of custom_tape.hip ----------------------------------------------------------------
// gmmvi_data::RowList of custom_target_data.inc, member for member
struct RowList { int C; unsigned T; int minibatch; unsigned length, rows_per_chunk, call, hbits, k0, k1; };
static_assert(sizeof(RowList) == 36, "RowList is a kernel argument: its layout is the device text's");

// minibatch inside the library: the flag of gmmvi_target_custom_data (0, 1), or own batches, which only the _own_batches entries pass
constexpr int GMMVI_DATA_OWN_BATCHES = 2;
constexpr int GMMVI_DATA_PLAN_CUS = 256;
constexpr int64_t GMMVI_DATA_MAX_CHUNKS = 65535;           // gridDim.y

// the refusals the two data modes share, in the order and with the messages of gmmvi_target_custom_data
int gmmvi_custom_check_data_arguments(gmmvi_ctx* ctx, int D, const float* data_dev, int64_t T, int C, int minibatch, int64_t B,
                                      const float* X_dev, int N, const float* lp_out_dev, int chunks_requested);
// the launches of the data mode's kernels from a handle of either data mode, dual-number gradient or value alone
int gmmvi_custom_launch_data(gmmvi_ctx* ctx, const gmmvi_custom_target* t, int D, const float* params_dev, const float* data_dev,
                             int64_t T, int C, int minibatch, int64_t B, uint64_t seed, uint32_t call, const float* X_dev, int N,
                             float* lp_out_dev, float* grad_out_dev, int chunks_requested);
