// Per-camera pose deltas for gfx950: the pose path of CameraOptimizer / PrevNextCamOptimizer (lsenerf_amd/cameras.py: forward over
// hom_exp_map_SO3xR3 / exp_map_SE3, applied to a table the way lsenerf_amd.data.camera_tables applies it;
// R:lse_nerf/ns_camera_optimizer.py:214-414) as device code, so that a captured training step evaluates the pose tables of its composer
// from the pose_adjustment parameters' own storage.
//   pose_delta_fwd_kernel  one thread per table row: exp_map(adj[c]) -> [R_corr R0 | t0 + t_corr]; a frozen camera copies (R0 | t0).
//   pose_delta_bwd_kernel  one thread per (parameter block, camera): the one or two table rows the camera owns -> d adj[c], ONE launch.
//                          No sums across threads, so no atomics: two runs are bit-equal; a frozen camera writes zeros; every element
//                          of every output is written.
// With (v, w) = adj[c], t2 = |w|^2, W = hat(w), W^2 = w w^T - t2 I both exponentials are  R = I + a W + b W^2  and SE3 adds
// t_corr = v + b (w x v) + c W^2 v.  The coefficients a = sin t / t, b = (1 - cos t) / t^2, c = (t - sin t) / t^3 and
//   e = (1/2 - b) / t^2,  f = (1/6 - c) / t^2,   da/dt2 = (c - b) / 2,  db/dt2 = e - c / 2,  dc/dt2 = (3 f - e) / 2
// are alternating series in t2 below t = 2 (ten terms: the first one left out is below 2^-33 of the sum) and closed forms above, b
// through the half angle -- float32 cameras.py loses four digits to cancellation just above the SE3 branch point, this does not.
// The branch points and the small branch's polynomials are those of cameras.py.  The derivative is the one torch autograd takes:
// `where` selects a branch, clamp(t2, 1e-4) passes no gradient below its bound.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr float kSmall = 1e-4f;        // clamp bound of hom_exp_map_SO3xR3 and branch point of exp_map_SE3, both on |w|^2

template <int N>
struct InvFact {
    static constexpr double v = InvFact<N - 1>::v / N;
};
template <>
struct InvFact<0> {
    static constexpr double v = 1.0;
};

// sum_{k = K}^{9} (-x)^(k - K) / (2 k + M)!
template <int M, int K>
__host__ __device__ __forceinline__ float alt_series(float x)
{
    if constexpr (K == 9)
        return (float)InvFact<2 * K + M>::v;
    else
        return (float)InvFact<2 * K + M>::v - x * alt_series<M, K + 1>(x);
}

struct Coef {
    float a, b, c;           // sin t / t, (1 - cos t) / t^2, (t - sin t) / t^3
    float da, db, dc;        // their derivatives with respect to t2 = t^2
};

// the closed forms at t2 = x, evaluated without cancellation
__host__ __device__ __forceinline__ Coef coef_exact(float x)
{
    Coef k;
    float e, f;
    if (x < 4.0f) {
        k.a = alt_series<1, 0>(x);
        k.b = alt_series<2, 0>(x);
        k.c = alt_series<3, 0>(x);
        e = alt_series<4, 0>(x);
        f = alt_series<5, 0>(x);
    } else {
        const float t = sqrtf(x);
        float s, c;
        sincosf(t, &s, &c);
        const float sh = sinf(0.5f * t);
        k.a = s / t;
        k.b = 2.0f * sh * sh / x;
        k.c = (t - s) / (x * t);
        e = (0.5f - k.b) / x;
        f = (1.0f / 6.0f - k.c) / x;
    }
    k.da = 0.5f * (k.c - k.b);
    k.db = e - 0.5f * k.c;
    k.dc = 0.5f * (3.0f * f - e);
    return k;
}

// the coefficients cameras.py uses at rotation vector w (t2 = |w|^2) in `mode`, and their derivatives w.r.t. t2 as autograd sees them
__host__ __device__ __forceinline__ Coef coef_of(int mode, float t2)
{
    Coef k;
    if (mode == LSE_POSE_SE3) {
        if (t2 < kSmall) {
            k.a = 1.0f - t2 / 6.0f;
            k.b = 0.5f - t2 / 24.0f;
            k.c = 1.0f / 6.0f - t2 / 120.0f;
            k.da = -1.0f / 6.0f;
            k.db = -1.0f / 24.0f;
            k.dc = -1.0f / 120.0f;
            return k;
        }
        return coef_exact(t2);
    }
    k = coef_exact(fmaxf(t2, kSmall));
    k.c = k.dc = 0.f;                       // (SO3xR3: the translation is v itself)
    if (t2 < kSmall) k.da = k.db = 0.f;     // below the clamp's bound the coefficients are constants
    return k;
}

__host__ __device__ __forceinline__ float dot3(const float x[3], const float y[3]) { return x[0] * y[0] + x[1] * y[1] + x[2] * y[2]; }

__host__ __device__ __forceinline__ void cross3(const float x[3], const float y[3], float o[3])
{
    o[0] = x[1] * y[2] - x[2] * y[1];
    o[1] = x[2] * y[0] - x[0] * y[2];
    o[2] = x[0] * y[1] - x[1] * y[0];
}

// (R_corr | t_corr) = exp_map(p), p = (v, w)
__host__ __device__ __forceinline__ void exp_fwd(int mode, const float p[6], float R[9], float T[3])
{
    const float *v = p, *w = p + 3;
    const float t2 = dot3(w, w);
    const Coef k = coef_of(mode, t2);
    const float xx = w[0] * w[0], yy = w[1] * w[1], zz = w[2] * w[2];
    const float xy = w[0] * w[1], xz = w[0] * w[2], yz = w[1] * w[2];
    R[0] = 1.0f - k.b * (yy + zz);
    R[1] = k.b * xy - k.a * w[2];
    R[2] = k.b * xz + k.a * w[1];
    R[3] = k.b * xy + k.a * w[2];
    R[4] = 1.0f - k.b * (xx + zz);
    R[5] = k.b * yz - k.a * w[0];
    R[6] = k.b * xz - k.a * w[1];
    R[7] = k.b * yz + k.a * w[0];
    R[8] = 1.0f - k.b * (xx + yy);
    if (mode == LSE_POSE_SE3) {             // V v = v + b (w x v) + c (w (w . v) - t2 v)
        float wxv[3];
        cross3(w, v, wxv);
        const float wv = dot3(w, v);
#pragma unroll
        for (int i = 0; i < 3; ++i) T[i] = v[i] + k.b * wxv[i] + k.c * (w[i] * wv - t2 * v[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) T[i] = v[i];
    }
}

// backward of exp_fwd: gR [3, 3], gT [3] -> gp [6]
__host__ __device__ __forceinline__ void exp_bwd(int mode, const float p[6], const float gR[9], const float gT[3], float gp[6])
{
    const float *v = p, *w = p + 3;
    const float t2 = dot3(w, w);
    const Coef k = coef_of(mode, t2);
    // through M = I + alpha W + beta W^2 with upstream G:  d alpha = w . u,  d beta = w^T G w - t2 tr G,
    // d w = alpha u + beta (G w + G^T w - 2 w tr G),  u = (G21 - G12, G02 - G20, G10 - G01)
    const float u[3] = {gR[7] - gR[5], gR[2] - gR[6], gR[3] - gR[1]};
    const float Gw[3] = {gR[0] * w[0] + gR[1] * w[1] + gR[2] * w[2], gR[3] * w[0] + gR[4] * w[1] + gR[5] * w[2],
                         gR[6] * w[0] + gR[7] * w[1] + gR[8] * w[2]};
    const float Gtw[3] = {gR[0] * w[0] + gR[3] * w[1] + gR[6] * w[2], gR[1] * w[0] + gR[4] * w[1] + gR[7] * w[2],
                          gR[2] * w[0] + gR[5] * w[1] + gR[8] * w[2]};
    const float tr = gR[0] + gR[4] + gR[8];
    const float g_a = dot3(w, u);
    float g_b = dot3(w, Gw) - t2 * tr;
    float g_c = 0.f;
    float gw[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) gw[i] = k.a * u[i] + k.b * (Gw[i] + Gtw[i] - 2.0f * w[i] * tr);
    if (mode == LSE_POSE_SE3) {             // the same through V = I + b W + c W^2 with upstream gT v^T
        float vxg[3], wxg[3];
        cross3(v, gT, vxg);                 // u of gT v^T
        cross3(w, gT, wxg);
        const float vw = dot3(v, w), gw_ = dot3(gT, w), gv_ = dot3(gT, v);
        g_b += dot3(w, vxg);
        g_c = gw_ * vw - t2 * gv_;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            gw[i] += k.b * vxg[i] + k.c * (gT[i] * vw + v[i] * gw_ - 2.0f * w[i] * gv_);
            gp[i] = gT[i] - k.b * wxg[i] + k.c * (w[i] * gw_ - t2 * gT[i]);         // V^T gT
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) gp[i] = gT[i];
    }
    const float g_t2 = g_a * k.da + g_b * k.db + g_c * k.dc;
#pragma unroll
    for (int i = 0; i < 3; ++i) gp[3 + i] = gw[i] + 2.0f * w[i] * g_t2;
}

// which block of rows thread i works on (selects: no dynamic index into the kernel arguments)
struct Seg {
    int s, c, mode;
    const float *base, *adj;
    bool frozen;
};

__device__ __forceinline__ Seg locate(const lse_pose_delta_desc &D, int i)
{
    Seg r;
    const int n0 = D.n_cam[0], n1 = D.n_cam[1];
    r.s = i < n0 ? 0 : (i < n0 + n1 ? 1 : 2);
    r.c = i - (r.s == 0 ? 0 : (r.s == 1 ? n0 : n0 + n1));
    r.mode = r.s == 0 ? D.mode[0] : (r.s == 1 ? D.mode[1] : D.mode[2]);
    r.base = (r.s == 0 ? D.base[0] : (r.s == 1 ? D.base[1] : D.base[2])) + 12 * (int64_t)r.c;
    r.adj = (r.s == 0 ? D.adj[0] : (r.s == 1 ? D.adj[1] : D.adj[2])) + 6 * (int64_t)r.c;
    const uint8_t *fz = r.s == 0 ? D.frozen[0] : (r.s == 1 ? D.frozen[1] : D.frozen[2]);
    r.frozen = fz != nullptr && fz[r.c] != 0;
    return r;
}

__global__ __launch_bounds__(kThreads) void pose_delta_fwd_kernel(lse_pose_delta_desc D, float *__restrict__ o_col,
                                                                  float *__restrict__ o_prev, float *__restrict__ o_next, int n_total)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_total) return;
    const Seg r = locate(D, i);
    float *dst = (r.s == 0 ? o_col : (r.s == 1 ? o_prev : o_next)) + 12 * (int64_t)r.c;
    float B[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) B[e] = r.base[e];
    if (r.frozen) {                          // (I | 0): the row is the base pose, bit for bit
#pragma unroll
        for (int e = 0; e < 12; ++e) dst[e] = B[e];
        return;
    }
    float p[6], R[9], T[3];
#pragma unroll
    for (int e = 0; e < 6; ++e) p[e] = r.adj[e];
    exp_fwd(r.mode, p, R, T);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int j = 0; j < 3; ++j) dst[4 * a + j] = R[3 * a] * B[j] + R[3 * a + 1] * B[4 + j] + R[3 * a + 2] * B[8 + j];
        dst[4 * a + 3] = B[4 * a + 3] + T[a];
    }
}

// a table row's gradient g [3, 4] over base pose B [3, 4]: d R_corr = g[:, :3] R0^T, d t_corr = g[:, 3].  Every product and sum is
// rounded on its own, so that the sum of two rows does not depend on which of them the compiler would have fused into the other
__device__ __forceinline__ void row_to_corr(const float *__restrict__ g, const float *__restrict__ B, float gR[9], float gT[3])
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int m = 0; m < 3; ++m)
            gR[3 * a + m] = __fadd_rn(__fadd_rn(__fmul_rn(g[4 * a], B[4 * m]), __fmul_rn(g[4 * a + 1], B[4 * m + 1])),
                                      __fmul_rn(g[4 * a + 2], B[4 * m + 2]));
        gT[a] = g[4 * a + 3];
    }
}

__global__ __launch_bounds__(kThreads) void pose_delta_bwd_kernel(lse_pose_delta_desc D, const float *__restrict__ g_col,
                                                                  const float *__restrict__ g_prev, const float *__restrict__ g_next,
                                                                  float *__restrict__ o_col, float *__restrict__ o_prev,
                                                                  float *__restrict__ o_next, int n_total)
{
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n_total) return;                // (shared_prev_next: n_total = n_cam[0] + n_cam[1], the next block has no threads)
    const Seg r = locate(D, i);
    float *dst = (r.s == 0 ? o_col : (r.s == 1 ? o_prev : o_next)) + 6 * (int64_t)r.c;
    if (r.frozen) {
#pragma unroll
        for (int e = 0; e < 6; ++e) dst[e] = 0.f;
        return;
    }
    const float *g = (r.s == 0 ? g_col : (r.s == 1 ? g_prev : g_next)) + 12 * (int64_t)r.c;
    float gR[9], gT[3];
    row_to_corr(g, r.base, gR, gT);
    if (r.s == 1 && D.shared_prev_next) {    // row(prev) + row(next), in that order
        float gR2[9], gT2[3];
        row_to_corr(g_next + 12 * (int64_t)r.c, D.base[2] + 12 * (int64_t)r.c, gR2, gT2);
#pragma unroll
        for (int e = 0; e < 9; ++e) gR[e] = __fadd_rn(gR[e], gR2[e]);
#pragma unroll
        for (int e = 0; e < 3; ++e) gT[e] = __fadd_rn(gT[e], gT2[e]);
    }
    float p[6], gp[6];
#pragma unroll
    for (int e = 0; e < 6; ++e) p[e] = r.adj[e];
    exp_bwd(r.mode, p, gR, gT, gp);
#pragma unroll
    for (int e = 0; e < 6; ++e) dst[e] = gp[e];
}

int check_desc(const lse_pose_delta_desc *d, const char *what, int64_t *n_total)
{
    LSE_REQUIRE(d, "%s: null descriptor", what);
    int64_t n = 0;
    for (int s = 0; s < 3; ++s) {
        LSE_REQUIRE(d->n_cam[s] >= 0, "%s: n_cam[%d] < 0", what, s);
        if (d->n_cam[s] == 0) continue;
        LSE_REQUIRE(d->mode[s] == LSE_POSE_SO3XR3 || d->mode[s] == LSE_POSE_SE3, "%s: unknown mode %d of segment %d", what, d->mode[s], s);
        LSE_REQUIRE(d->base[s] && d->adj[s], "%s: null base poses or parameters of segment %d", what, s);
        n += d->n_cam[s];
    }
    LSE_REQUIRE(n >= 1 && n < (1 << 24), "%s: %lld rows (1 .. 2^24 - 1)", what, (long long)n);
    LSE_REQUIRE(d->shared_prev_next == 0 || d->shared_prev_next == 1, "%s: shared_prev_next must be 0 or 1 (got %d)", what,
                d->shared_prev_next);
    if (d->shared_prev_next)
        LSE_REQUIRE(d->n_cam[1] > 0 && d->n_cam[1] == d->n_cam[2] && d->mode[1] == d->mode[2] && d->adj[1] == d->adj[2] &&
                        d->frozen[1] == d->frozen[2],
                    "%s: a shared parameter block feeds prev and next with one count, mode, parameter and mask pointer", what);
    *n_total = n;
    return LSE_OK;
}

}  // namespace

extern "C" int lse_pose_delta_tables(const lse_pose_delta_desc *desc, float *col_pose, float *prev_pose, float *next_pose,
                                     lse_stream_t stream)
{
    const char *what = "lse_pose_delta_tables";
    int64_t n = 0;
    const int rc = check_desc(desc, what, &n);
    if (rc != LSE_OK) return rc;
    float *out[3] = {col_pose, prev_pose, next_pose};
    for (int s = 0; s < 3; ++s) LSE_REQUIRE(desc->n_cam[s] == 0 || out[s], "%s: null pose table of segment %d", what, s);
    hipLaunchKernelGGL(pose_delta_fwd_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, lse::as_stream(stream),
                       *desc, col_pose, prev_pose, next_pose, (int)n);
    return lse::check_launch(what);
}

extern "C" int lse_pose_delta_tables_bwd(const lse_pose_delta_desc *desc, const float *d_col_pose, const float *d_prev_pose,
                                         const float *d_next_pose, float *d_adj_col, float *d_adj_prev, float *d_adj_next,
                                         lse_stream_t stream)
{
    const char *what = "lse_pose_delta_tables_bwd";
    int64_t n = 0;
    const int rc = check_desc(desc, what, &n);
    if (rc != LSE_OK) return rc;
    const float *g[3] = {d_col_pose, d_prev_pose, d_next_pose};
    float *out[3] = {d_adj_col, d_adj_prev, d_adj_next};
    for (int s = 0; s < 3; ++s) {
        LSE_REQUIRE(desc->n_cam[s] == 0 || g[s], "%s: null table gradient of segment %d", what, s);
        LSE_REQUIRE(desc->n_cam[s] == 0 || out[s] || (s == 2 && desc->shared_prev_next), "%s: null output of segment %d", what, s);
    }
    if (desc->shared_prev_next) n -= desc->n_cam[2];
    hipLaunchKernelGGL(pose_delta_bwd_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, lse::as_stream(stream),
                       *desc, d_col_pose, d_prev_pose, d_next_pose, d_adj_col, d_adj_prev, d_adj_next, (int)n);
    return lse::check_launch(what);
}
