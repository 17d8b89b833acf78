// Talos humanoid inverse-kinematics target (target_distributions/talos_ik.py; DESIGN.md 6, "Talos (defined, not
// reproduced)") with its analytic gradient, and the forward kinematics behind its metrics.
//
// One lane per sample.  x = [q (28 joint angles), p_b (3), roll, pitch, yaw]; the table (talos_ik.py, TalosModel) holds
// the walk over the 28 revolute joints: each joint's frame is its parent frame (the base, the previous joint's or a saved
// branch frame) times the folded origin times Rot(axis, q).  All positions are taken relative to p_b, so nothing large is
// subtracted when p_b is; p_b is added back where a world position meets a target.
//
// Gradient (geometric Jacobian).  With g / G the upstream gradients of a tip's position / rotation and g_c that of the
// centre of mass c, each tip is a force g with the torque y x g + sum_k R[:,k] x G[:,k] about p_b, and each frame's lumped
// mass a force (M_f / M) g_c at its mass point.  Summing those over the subtree of joint i gives (f_i, t_i), and
//     d lp / d q_i = a_i . (t_i - o_i x f_i)             (a_i world axis, o_i the joint's origin)
// The base rotation acts as three such joints at p_b with axes Rz Ry e_x, Rz e_y, e_z; d lp / d p_b is the total force.
// The second pass walks the joints backwards and recomputes each frame from its child's (one inverse step) or, at the
// end of a branch, from the leaf frame the first pass kept for that branch's tip: four leaf frames stay live instead of 28.
//
// log Phi and phi / Phi go through erfcx below zero, so that they stay finite and accurate to z = -1e4 and beyond.
// No atomics: every lane writes its own outputs, so results are bitwise reproducible.
#include "common.h"
#include "combine.h"
#include "riders.h"

namespace {
constexpr int TL_NJ = 28, TL_NT = 4, TL_D = TL_NJ + 6, TL_SLOTS = 2;
constexpr int TL_HDR = 8, TL_JS = 28, TL_TS = 16;                 // table layout: talos_ik.py
constexpr int TL_WG = 64, TL_LDX = TL_D + 1;                      // samples per workgroup, LDS row stride (odd)
constexpr float TL_LOG_2PI = 1.8378770664093453f;
constexpr float TL_INV_SQRT2 = 0.7071067811865476f;
constexpr float TL_SQRT_2_OVER_PI = 0.7978845608028654f;
constexpr float TL_INV_SQRT_2PI = 0.3989422804014327f;
constexpr float TL_JOINT_STD = 0.05f, TL_COM_LIMIT = 0.14f, TL_COM_STD = 0.01f;
constexpr float TL_POS_STD = 0.02f, TL_ROT_STD = 0.1f;            // feet: position, rotation; the left gripper: position

struct Frame {
    float R[9];    // row-major
    float p[3];    // relative to p_b
};

struct Wrench {
    float f[3], t[3];   // force, torque about p_b
};

__device__ __forceinline__ void cross3(const float* a, const float* b, float* c) {
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// r = c ? a : r, element by element (no aggregate copies: the arrays below stay in registers)
__device__ __forceinline__ void select(Frame& r, const Frame& a, bool c) {
#pragma unroll
    for (int i = 0; i < 9; ++i) r.R[i] = c ? a.R[i] : r.R[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) r.p[i] = c ? a.p[i] : r.p[i];
}

__device__ __forceinline__ void select(Wrench& r, const Wrench& a, bool c) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { r.f[i] = c ? a.f[i] : r.f[i]; r.t[i] = c ? a.t[i] : r.t[i]; }
}

// entry k of a frame (or wrench) array, k wave-uniform: every index is a constant after unrolling
template <typename T, int NS>
__device__ __forceinline__ T pick(const T (&arr)[NS], int k) {
    T r = arr[0];
#pragma unroll
    for (int i = 1; i < NS; ++i) select(r, arr[i], i == k);
    return r;
}

template <typename T, int NS>
__device__ __forceinline__ void put(T (&arr)[NS], int k, const T& v) {
#pragma unroll
    for (int i = 0; i < NS; ++i) select(arr[i], v, i == k);
}

__device__ __forceinline__ void wrench_add(Wrench& a, const Wrench& b) {
#pragma unroll
    for (int i = 0; i < 3; ++i) { a.f[i] += b.f[i]; a.t[i] += b.t[i]; }
}

// log Phi(z); *psi = phi(z) / Phi(z) = d log Phi / dz
__device__ __forceinline__ float log_ndtr(float z, float* psi) {
    if (z < 0.f) {
        const float e = erfcxf(-z * TL_INV_SQRT2);     // Phi(z) = 0.5 erfcx(t) exp(-t^2), t = -z / sqrt(2)
        *psi = TL_SQRT_2_OVER_PI / e;
        return logf(0.5f * e) - 0.5f * z * z;
    }
    const float Q = 0.5f * erfcf(z * TL_INV_SQRT2);    // Phi(-z) <= 1/2
    *psi = expf(-0.5f * z * z) * TL_INV_SQRT_2PI / (1.f - Q);
    return log1pf(-Q);
}

// rows of A times Rot(a, q): C_r = c A_r + s (A_r x a) + (1 - c)(A_r . a) a
__device__ __forceinline__ void rot_rows(const float* A, const float* a, float c, float s, float* C) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float v0 = A[3 * r], v1 = A[3 * r + 1], v2 = A[3 * r + 2];
        const float d = (v0 * a[0] + v1 * a[1] + v2 * a[2]) * (1.f - c);
        C[3 * r + 0] = c * v0 + s * (v1 * a[2] - v2 * a[1]) + d * a[0];
        C[3 * r + 1] = c * v1 + s * (v2 * a[0] - v0 * a[2]) + d * a[1];
        C[3 * r + 2] = c * v2 + s * (v0 * a[1] - v1 * a[0]) + d * a[2];
    }
}

// joint record: [0] parent joint, [1] parent source, [2] saved slot, [3] tip, [4] mass, [5..7] mass moment,
// [8..16] origin rotation, [17..19] origin translation, [20..22] axis, [23] lower, [24] upper
__device__ __forceinline__ void compose(const Frame& P, const float* __restrict__ rec, float q, Frame& C) {
    float A[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            A[3 * r + k] = P.R[3 * r] * rec[8 + k] + P.R[3 * r + 1] * rec[11 + k] + P.R[3 * r + 2] * rec[14 + k];
        C.p[r] = P.p[r] + P.R[3 * r] * rec[17] + P.R[3 * r + 1] * rec[18] + P.R[3 * r + 2] * rec[19];
    }
    float s, c;
    sincosf(q, &s, &c);
    rot_rows(A, rec + 20, c, s, C.R);
}

// the parent frame back from the child's: P.R = C.R Rot(a, -q) R0^T, P.p = C.p - P.R p0
__device__ __forceinline__ void step_back(const Frame& C, const float* __restrict__ rec, float q, Frame& P) {
    float s, c;
    sincosf(q, &s, &c);
    float B[9];
    rot_rows(C.R, rec + 20, c, -s, B);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
            P.R[3 * r + k] = B[3 * r] * rec[8 + 3 * k] + B[3 * r + 1] * rec[9 + 3 * k] + B[3 * r + 2] * rec[10 + 3 * k];
        P.p[r] = C.p[r] - (P.R[3 * r] * rec[17] + P.R[3 * r + 1] * rec[18] + P.R[3 * r + 2] * rec[19]);
    }
}

__device__ __forceinline__ void base_rotation(const float* x, float* R) {
    float sr, cr, sp, cp, sy, cy;
    sincosf(x[TL_NJ + 3], &sr, &cr);
    sincosf(x[TL_NJ + 4], &sp, &cp);
    sincosf(x[TL_NJ + 5], &sy, &cy);
    R[0] = cy * cp; R[1] = cy * sp * sr - sy * cr; R[2] = cy * sp * cr + sy * sr;
    R[3] = sy * cp; R[4] = sy * sp * sr + cy * cr; R[5] = sy * sp * cr - cy * sr;
    R[6] = -sp;     R[7] = cp * sr;                R[8] = cp * cr;
}

// first pass: the leaf frames of the four tips and the mass moment sum_f (R_f S_f + M_f p_f) about p_b
__device__ __forceinline__ void forward_pass(const float* __restrict__ tab, const float* x, Frame& base, Frame (&leaf)[TL_NT],
                                             float* cw) {
    base_rotation(x, base.R);
    base.p[0] = base.p[1] = base.p[2] = 0.f;
#pragma unroll
    for (int r = 0; r < 3; ++r) cw[r] = base.R[3 * r] * tab[5] + base.R[3 * r + 1] * tab[6] + base.R[3 * r + 2] * tab[7];
    Frame cur = base;
    Frame slot[TL_SLOTS];
#pragma unroll
    for (int k = 0; k < TL_SLOTS; ++k) slot[k] = base;
#pragma unroll
    for (int k = 0; k < TL_NT; ++k) leaf[k] = base;
#pragma unroll 1
    for (int j = 0; j < TL_NJ; ++j) {
        const float* rec = tab + TL_HDR + j * TL_JS;
        const int src = (int)rec[1], save = (int)rec[2], tip = (int)rec[3];
        Frame P = cur;
        if (src == -1) P = base;
        else if (src >= 0) P = pick(slot, src);
        compose(P, rec, x[j], cur);
        if (save >= 0) put(slot, save, cur);
        const float m = rec[4];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            cw[r] += cur.R[3 * r] * rec[5] + cur.R[3 * r + 1] * rec[6] + cur.R[3 * r + 2] * rec[7] + m * cur.p[r];
        if (tip >= 0) put(leaf, tip, cur);
    }
}

// tip t's pose from its leaf frame: y = L.p + L.R o, R = L.R Ro
__device__ __forceinline__ void tip_pose(const float* __restrict__ tab, int t, const Frame& L, float* y, float* R) {
    const float* rec = tab + TL_HDR + TL_NJ * TL_JS + t * TL_TS;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        y[r] = L.p[r] + L.R[3 * r] * rec[1] + L.R[3 * r + 1] * rec[2] + L.R[3 * r + 2] * rec[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            R[3 * r + k] = L.R[3 * r] * rec[4 + k] + L.R[3 * r + 1] * rec[7 + k] + L.R[3 * r + 2] * rec[10 + k];
    }
}
}  // namespace

// one kernel for both uses (grad == nullptr: log density only), so that lp comes from the same instructions either way
__global__ __launch_bounds__(TL_WG) void talos_kernel(const float* __restrict__ tab, const float* __restrict__ goal,
                                                      const float* __restrict__ X, int N, float* __restrict__ lp_out,
                                                      float* __restrict__ grad, CombineJob carried, Riders riders) {
    if (combine_carried(carried) || riders_carried_prep(riders)) return;   // workgroups past the samples: the merge of the previous sweep, bookkeeping
    __shared__ float xs[TL_WG * TL_LDX];
    __shared__ float gs[TL_WG * TL_LDX];
    const bool want_grad = grad != nullptr;
    const int t = threadIdx.x;
    const int n0 = blockIdx.x * TL_WG;
    const int rows = min(TL_WG, N - n0);
    for (int i = t; i < rows * TL_D; i += TL_WG) {
        const int r = i / TL_D;
        xs[r * TL_LDX + i - r * TL_D] = X[(size_t)n0 * TL_D + i];
    }
    __syncthreads();
    if (t < rows) {
        const float* x = xs + t * TL_LDX;
        const float* pb = x + TL_NJ;
        Frame base, leaf[TL_NT];
        float cw[3];
        forward_pass(tab, x, base, leaf, cw);
        const float invM = 1.f / tab[2];
        // ---- tips: left gripper at the goal, feet at their targets ----------------------------------------------------
        float lp = -3.f * (logf(TL_POS_STD) + 0.5f * TL_LOG_2PI)
                   - 2.f * (3.f * logf(TL_POS_STD) + 9.f * logf(TL_ROT_STD) + 6.f * TL_LOG_2PI);
        Wrench tw[TL_NT];
        float ylf[3];
#pragma unroll
        for (int k = 1; k < TL_NT; ++k) {          // tip 0 (the right gripper) has no term
            float y[3], R[9], g[3], G[9];
            tip_pose(tab, k, leaf[k], y, R);
            if (k == 1) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float e = (y[r] + pb[r] - goal[r]) * (1.f / TL_POS_STD);
                    lp -= 0.5f * e * e;
                    g[r] = -e * (1.f / TL_POS_STD);
                }
#pragma unroll
                for (int i = 0; i < 9; ++i) G[i] = 0.f;
            } else {
                const float target[3] = {-0.02f, k == 2 ? -0.09f : 0.09f, 0.f};
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const float e = (y[r] + pb[r] - target[r]) * (1.f / TL_POS_STD);
                    lp -= 0.5f * e * e;
                    g[r] = -e * (1.f / TL_POS_STD);
                }
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    const float e = (R[i] - (i % 4 == 0 ? 1.f : 0.f)) * (1.f / TL_ROT_STD);
                    lp -= 0.5f * e * e;
                    G[i] = -e * (1.f / TL_ROT_STD);
                }
            }
            if (k == TL_NT - 1) { ylf[0] = y[0]; ylf[1] = y[1]; ylf[2] = y[2]; }
            if (want_grad) {
                float tq[3], c[3];
                cross3(y, g, tq);
#pragma unroll
                for (int col = 0; col < 3; ++col) {
                    const float Rc[3] = {R[col], R[3 + col], R[6 + col]}, Gc[3] = {G[col], G[3 + col], G[6 + col]};
                    cross3(Rc, Gc, c);
                    tq[0] += c[0]; tq[1] += c[1]; tq[2] += c[2];
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) { tw[k].f[r] = g[r]; tw[k].t[r] = tq[r]; }
            }
        }
        // ---- centre of mass over the left foot (both relative to p_b) ------------------------------------------------
        float gc[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float d = cw[k] * invM - ylf[k];
            float s1, s2;
            lp += log_ndtr((d + TL_COM_LIMIT) * (1.f / TL_COM_STD), &s1) + log_ndtr((TL_COM_LIMIT - d) * (1.f / TL_COM_STD), &s2);
            gc[k] = (s1 - s2) * (1.f / TL_COM_STD);
        }
        // ---- joint limits -----------------------------------------------------------------------------------------------
        float* gq = gs + t * TL_LDX;
#pragma unroll 4
        for (int j = 0; j < TL_NJ; ++j) {
            const float* rec = tab + TL_HDR + j * TL_JS;
            float s1, s2;
            lp += log_ndtr((x[j] - rec[23]) * (1.f / TL_JOINT_STD), &s1) + log_ndtr((rec[24] - x[j]) * (1.f / TL_JOINT_STD), &s2);
            if (want_grad) gq[j] = (s1 - s2) * (1.f / TL_JOINT_STD);
        }
        lp_out[n0 + t] = lp;
        if (want_grad) {
            // the left foot also carries -g_c (d = c - p_lfoot)
            {
                float c[3];
                cross3(ylf, gc, c);
#pragma unroll
                for (int r = 0; r < 3; ++r) { tw[TL_NT - 1].f[r] -= gc[r]; tw[TL_NT - 1].t[r] -= c[r]; }
            }
#pragma unroll
            for (int r = 0; r < 3; ++r) tw[0].f[r] = tw[0].t[r] = 0.f;
            // ---- second pass: the joints backwards, subtree wrenches ------------------------------------------------------
            const Wrench zero = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
            Wrench cur = zero, base_acc = zero, slot[TL_SLOTS];
#pragma unroll
            for (int k = 0; k < TL_SLOTS; ++k) slot[k] = zero;
            Frame F = leaf[TL_NT - 1];                   // the last joint carries the last tip (talos_ik.py checks)
#pragma unroll 1
            for (int j = TL_NJ - 1; j >= 0; --j) {
                const float* rec = tab + TL_HDR + j * TL_JS;
                const int src = (int)rec[1], save = (int)rec[2], tip = (int)rec[3];
                const float m = rec[4];
                Wrench w;
                float wm[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    wm[r] = (F.R[3 * r] * rec[5] + F.R[3 * r + 1] * rec[6] + F.R[3 * r + 2] * rec[7] + m * F.p[r]) * invM;
                    w.f[r] = m * invM * gc[r];
                }
                cross3(wm, gc, w.t);
                if (tip >= 0) wrench_add(w, pick(tw, tip));
                wrench_add(w, save >= 0 ? pick(slot, save) : cur);
                float a[3], ox[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) a[r] = F.R[3 * r] * rec[20] + F.R[3 * r + 1] * rec[21] + F.R[3 * r + 2] * rec[22];
                cross3(F.p, w.f, ox);
                gq[j] += a[0] * (w.t[0] - ox[0]) + a[1] * (w.t[1] - ox[1]) + a[2] * (w.t[2] - ox[2]);
                if (src == -2) {
                    cur = w;
                } else {
                    cur = zero;
                    if (src == -1) wrench_add(base_acc, w);
                    else {
#pragma unroll
                        for (int k = 0; k < TL_SLOTS; ++k)
                            if (k == src) wrench_add(slot[k], w);
                    }
                }
                if (j > 0) {
                    if ((int)rec[0] == j - 1) {
                        Frame P;
                        step_back(F, rec, x[j], P);
                        F = P;
                    } else {
                        F = pick(leaf, (int)tab[TL_HDR + (j - 1) * TL_JS + 3]);
                    }
                }
            }
            // the base's own mass point, then p_b and the three base rotations
            {
                float wm[3], c[3];
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    wm[r] = (base.R[3 * r] * tab[5] + base.R[3 * r + 1] * tab[6] + base.R[3 * r + 2] * tab[7]) * invM;
                    base_acc.f[r] += tab[4] * invM * gc[r];
                }
                cross3(wm, gc, c);
#pragma unroll
                for (int r = 0; r < 3; ++r) base_acc.t[r] += c[r];
            }
            // R_b = Rz Ry Rx: roll axis Rz Ry e_x = first column of R_b, pitch axis Rz e_y = (-sin y, cos y, 0), yaw axis e_z
            float sy, cy;
            sincosf(x[TL_NJ + 5], &sy, &cy);
            gq[TL_NJ + 0] = base_acc.f[0];
            gq[TL_NJ + 1] = base_acc.f[1];
            gq[TL_NJ + 2] = base_acc.f[2];
            gq[TL_NJ + 3] = base.R[0] * base_acc.t[0] + base.R[3] * base_acc.t[1] + base.R[6] * base_acc.t[2];
            gq[TL_NJ + 4] = -sy * base_acc.t[0] + cy * base_acc.t[1];
            gq[TL_NJ + 5] = base_acc.t[2];
        }
    }
    if (want_grad) {
        __syncthreads();
        for (int i = t; i < rows * TL_D; i += TL_WG) {
            const int r = i / TL_D;
            grad[(size_t)n0 * TL_D + i] = gs[r * TL_LDX + i - r * TL_D];
        }
    }
}

__global__ __launch_bounds__(TL_WG) void talos_fk_kernel(const float* __restrict__ tab, const float* __restrict__ X, int N,
                                                         float* __restrict__ poses, float* __restrict__ com) {
    const int n = blockIdx.x * TL_WG + threadIdx.x;
    if (n >= N) return;
    const float* x = X + (size_t)n * TL_D;
    Frame base, leaf[TL_NT];
    float cw[3];
    forward_pass(tab, x, base, leaf, cw);
    const float invM = 1.f / tab[2];
#pragma unroll
    for (int k = 0; k < TL_NT; ++k) {
        float y[3], R[9];
        tip_pose(tab, k, leaf[k], y, R);
        float* o = poses + ((size_t)n * TL_NT + k) * 12;
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = y[r] + x[TL_NJ + r];
#pragma unroll
        for (int i = 0; i < 9; ++i) o[3 + i] = R[i];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) com[(size_t)n * 3 + r] = cw[r] * invM + x[TL_NJ + r];
}

extern "C" int gmmvi_target_talos(gmmvi_ctx* ctx, const float* model_dev, const float* context_dev, const float* X_dev, int N,
                                  float* lp_out_dev, float* grad_out_dev) {
    GMMVI_ARG_CHECK(ctx, N >= 0);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, model_dev && context_dev && X_dev && lp_out_dev);
    GMMVI_PROF(ctx, "target_talos");
    const int blocks = (N + TL_WG - 1) / TL_WG;
    const Riders riders = gmmvi_take_pending_riders(ctx, blocks, TL_WG, true);
    const CombineJob carried = gmmvi_take_pending_combine(ctx, TL_WG, blocks + riders.prep_blocks, true);
    const dim3 grid(blocks + riders.prep_blocks + carried.blocks);
    hipLaunchKernelGGL(talos_kernel, grid, dim3(TL_WG), 0, ctx->stream, model_dev, context_dev, X_dev, N, lp_out_dev, grad_out_dev,
                       carried, riders);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}

extern "C" int gmmvi_talos_fk(gmmvi_ctx* ctx, const float* model_dev, const float* X_dev, int N, float* poses_out_dev,
                              float* com_out_dev) {
    GMMVI_ARG_CHECK(ctx, N >= 0);
    if (N == 0) return GMMVI_OK;
    GMMVI_ARG_CHECK(ctx, model_dev && X_dev && poses_out_dev && com_out_dev);
    int rc = gmmvi_flush_pending_combine(ctx);          // work queued for a carrying launch: this one carries none
    if (rc == GMMVI_OK) rc = gmmvi_flush_pending_riders(ctx);
    if (rc != GMMVI_OK) return rc;
    GMMVI_PROF(ctx, "talos_fk");
    hipLaunchKernelGGL(talos_fk_kernel, dim3((N + TL_WG - 1) / TL_WG), dim3(TL_WG), 0, ctx->stream, model_dev, X_dev, N,
                       poses_out_dev, com_out_dev);
    GMMVI_LAUNCH_CHECK(ctx);
    return GMMVI_OK;
}
