// What the full-covariance and blocked routes of the KL-constrained component update share
// (gmmvi_modules/ng_based_component_updater.py): the search report and the l2 / num_updates bookkeeping (:504-524) and KL(eta)
// on the tridiagonal form.  The search loops stay with their kernels (update_kl.hip, blocked_update.hip, diag.hip, and the
// reference-form kernel of update.hip as the cross-check): every form of them that went through a function here changed the
// register allocation of the update_kl_fast_kernel and diag.hip instances, and those figures are held equal.
#pragma once
#include <hip/hip_runtime.h>
#include <cfloat>
#include <cstdint>

// what a search leaves behind for the next iteration and for the caller's info arrays (:504, :511, :524); one thread calls it
__device__ __forceinline__ void tr_report_search(int k, bool success, float eta_star, float kl, int probes,
                                                 float* last_eta, float* kl_out, int32_t* nprobes_out) {
    last_eta[k] = success ? eta_star : -1.f;
    if (kl_out) kl_out[k] = success ? kl : -1.f;
    if (nprobes_out) nprobes_out[k] = probes;
}

// l2 regulariser and update count of every component updater (:519-523, iBLR :217-223; min on failure); one thread calls it
__device__ __forceinline__ void tr_finish_bookkeeping(int k, bool success, float l2_init, float* l2, float* num_updates,
                                                      int32_t* success_out) {
    const float old = l2[k];
    l2[k] = success ? fmaxf(0.5f * old, l2_init) : fminf(1e-6f, 10.f * old);
    num_updates[k] += 1.f;
    if (success_out) success_out[k] = success ? 1 : 0;
}

// KL(eta) from the tridiagonal form T = H^T M H of the whitened reward (update_kl.hip's header):
// B = I + T/eta, KL = 1/2 [logdet B - D + tr B^-1 + |B^-1 wt|^2 / eta^2] by two pivot recurrences and a Thomas solve, O(D).
// Every lane may evaluate a different eta: dcol is the lane's scratch column (d_i at [i * 64], c_i at [(D + i) * 64]).
// DC > 0: dimension known at compile time, loops unrolled.  RCP: v_rcp_f32 (1 ulp) instead of the IEEE division sequence in
// the two chains of D dependent steps.  A non-positive pivot or a NaN gives FLT_MAX, the reference's "Cholesky failed" (:320-324).
template <bool RCP>
__device__ __forceinline__ float tr_recip(float x) { return RCP ? __builtin_amdgcn_rcpf(x) : 1.f / x; }
template <bool RCP>
__device__ __forceinline__ float tr_div(float x, float y) { return RCP ? x * __builtin_amdgcn_rcpf(y) : x / y; }

template <int DC, bool RCP>
__device__ __forceinline__ float tr_kl_tridiag(int Drt, const float* td, const float* te, const float* wt, float* dcol,
                                               float eta) {
    const int D = DC > 0 ? DC : Drt;
    const float inv = 1.f / eta;
    float dprev = 1.f, cprev = 0.f, logdet = 0.f;
    bool ok = true;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        const float a = fmaf(td[i], inv, 1.f);
        float d = a, c = wt[i];
        if (i > 0) {
            const float b = te[i - 1] * inv;
            const float r = tr_div<RCP>(b, dprev);
            d = fmaf(-b, r, a);
            c = fmaf(-r, cprev, c);
        }
        ok = ok && (d > 0.f);
        logdet += __logf(d);
        dcol[(size_t)i * 64] = d;
        dcol[(size_t)(D + i) * 64] = c;
        dprev = d; cprev = c;
    }
    float dnext = 1.f, ynext = 0.f, tr = 0.f, yy = 0.f;
#pragma unroll
    for (int i = D - 1; i >= 0; --i) {
        const float a = fmaf(td[i], inv, 1.f);
        const float d = dcol[(size_t)i * 64], c = dcol[(size_t)(D + i) * 64];
        float delta = a, y = tr_div<RCP>(c, d);
        if (i < D - 1) {
            const float b = te[i] * inv;
            delta = fmaf(-b, tr_div<RCP>(b, dnext), a);
            y = tr_div<RCP>(c - b * ynext, d);
        }
        tr += tr_recip<RCP>(d + delta - a);
        yy = fmaf(y, y, yy);
        dnext = delta; ynext = y;
    }
    float kl = 0.5f * (logdet - (float)D + tr + yy * inv * inv);
    if (!ok || !(kl == kl)) kl = FLT_MAX;
    return kl;
}
