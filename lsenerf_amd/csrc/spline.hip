// Spline camera poses for gfx950: the pose path of SplineCameraOptimizer (lsenerf_amd/cameras.py: get_rgb_cameras / get_evs_cameras /
// get_deblur_cameras over exp_map_to_quat_map, vectorized_generalized_interpolation, slerp, quat_map_to_mtx;
// R:lse_nerf/ns_camera_optimizer.py:130-197, R:lse_nerf/interpolation_utils.py:56-233) as device code, so that a captured training
// step evaluates the pose tables of its composer from the parameters' own storage.
//   spline_fwd_kernel  one thread per query (= one 3x4 row of a pose table): the two bracketing control tangents -> quaternions,
//                      lerp of the translation, slerp of the rotation, quaternion -> matrix, and for an "evs" segment the product
//                      with dM' (dM with its translation column times the learnable scale).  The bracketing index and the fraction
//                      of every query are inputs: they depend on buffers that never change (control times, camera times, exposure),
//                      so the host computes them once with the torch expressions of cameras.py.
//   spline_bwd_kernel  d tables -> d ctrl_tangents, d scale, ONE launch.  One wave per control point: every lane walks the control
//                      point's query list (CSR over idx and idx + 1, ascending query order, built once on the host) with stride 64,
//                      differentiates its queries and keeps its share in list order; a fixed butterfly joins the 64 partial sums.
//                      The last block reduces d scale over the "evs" queries the same way (stride 256, butterfly, four wave sums
//                      added in wave order).  No atomics: two runs are bit-equal; a control point with an empty list writes zero.
// The derivative is the one torch autograd takes of the Python: `where` selects a branch, norm at exactly zero has gradient zero
// (a zero rotation vector gets no rotation gradient), a clamped value passes none.  Both launches are latency-bound (hundreds to a
// few thousand queries); everything is f32 and held against a float64 restatement, so the file is built with the default contraction.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr float kEps = 1e-6f;          // EPS of cameras.py (R:lse_nerf/utils.py:12)
constexpr float kNear = 0.9995f;       // slerp falls back to a lerp above this |dot|

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// exp_map_to_quat: rotation vector -> (w, x, y, z); theta == 0 gives the zero axis
__device__ __forceinline__ void rotvec_to_quat(const float v[3], float q[4])
{
    const float theta = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    float s, c;
    sincosf(0.5f * theta, &s, &c);
    const float k = theta > 0.f ? s / theta : 0.f;
    q[0] = c;
    q[1] = v[0] * k;
    q[2] = v[1] * k;
    q[3] = v[2] * k;
}

// backward of rotvec_to_quat: g_q -> g_v (zero at theta == 0: torch.norm's subgradient there is zero and `where` picks the zeros)
__device__ __forceinline__ void rotvec_to_quat_bwd(const float v[3], const float gq[4], float gv[3])
{
    const float theta = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(theta > 0.f)) {
        gv[0] = gv[1] = gv[2] = 0.f;
        return;
    }
    float s, c;
    sincosf(0.5f * theta, &s, &c);
    const float inv = 1.0f / theta;
    const float ax[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
    // q = (cos(theta / 2), axis sin(theta / 2)), axis = v / theta
    const float g_dot_ax = gq[1] * ax[0] + gq[2] * ax[1] + gq[3] * ax[2];
    // d theta: through cos, through sin, and through the division of the axis
    const float g_theta = -0.5f * s * gq[0] + 0.5f * c * g_dot_ax - s * inv * g_dot_ax;
    const float k = s * inv;
#pragma unroll
    for (int i = 0; i < 3; ++i) gv[i] = gq[1 + i] * k + g_theta * ax[i];
}

struct Slerp {
    float a[4], b[4];      // normalised inputs; b with the shortest-arc flip applied
    float na, nb;          // the norms
    float w0, w1;          // out = w0 a + w1 b
    float theta0, s0;      // slerp branch only
    bool near, flip;
};

// slerp of cameras.py, every branch: normalise, clamp the dot to +-(1 - EPS), flip when dot < 0, un-renormalised lerp when
// |dot| > 0.9995 (or NaN), the s0 == 0 guard
__device__ __forceinline__ void slerp_fwd(const float q0[4], const float q1[4], float t, Slerp &S, float out[4])
{
    S.na = sqrtf(q0[0] * q0[0] + q0[1] * q0[1] + q0[2] * q0[2] + q0[3] * q0[3]);
    S.nb = sqrtf(q1[0] * q1[0] + q1[1] * q1[1] + q1[2] * q1[2] + q1[3] * q1[3]);
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        S.a[i] = q0[i] / S.na;
        S.b[i] = q1[i] / S.nb;
        dot += S.a[i] * S.b[i];
    }
    dot = fminf(fmaxf(dot, -1.0f + kEps), 1.0f - kEps);
    S.near = !(fabsf(dot) <= kNear);           // |dot| > 0.9995, or NaN
    S.flip = dot < 0.f;
    if (S.flip) {
        dot = -dot;
#pragma unroll
        for (int i = 0; i < 4; ++i) S.b[i] = -S.b[i];
    }
    if (S.near) {
        S.w0 = 1.0f - t;
        S.w1 = t;
        S.theta0 = 0.f;
        S.s0 = 1.f;
    } else {
        S.theta0 = acosf(dot);
        float s0 = sinf(S.theta0);
        S.s0 = s0 == 0.f ? 1.0f : s0;
        S.w0 = sinf(S.theta0 - S.theta0 * t) / S.s0;
        S.w1 = sinf(S.theta0 * t) / S.s0;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = S.w0 * S.a[i] + S.w1 * S.b[i];
}

// backward of slerp_fwd: g_out -> g_q0, g_q1.  On the lerp branch the weights are constants of t.  On the slerp branch |dot| is at
// most 0.9995, so the clamp is inactive (it passes the gradient) and s0 = sin(acos(dot)) >= 0.03 is never the guarded zero.
__device__ __forceinline__ void slerp_bwd(const Slerp &S, float t, const float g_out[4], float g_q0[4], float g_q1[4])
{
    float ga[4], gb[4];       // w.r.t. a and the FLIPPED b (S.b)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ga[i] = S.w0 * g_out[i];
        gb[i] = S.w1 * g_out[i];
    }
    if (!S.near) {
        float g_w0 = 0.f, g_w1 = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            g_w0 += g_out[i] * S.a[i];
            g_w1 += g_out[i] * S.b[i];
        }
        const float c0 = cosf(S.theta0 - S.theta0 * t), c1 = cosf(S.theta0 * t);
        const float cth = cosf(S.theta0);           // = the flipped, clamped dot up to rounding
        // w0 = sin(theta0 (1 - t)) / s0, w1 = sin(theta0 t) / s0, s0 = sin(theta0)
        const float g_s0 = -(g_w0 * S.w0 + g_w1 * S.w1) / S.s0;
        const float g_theta0 = (g_w0 * c0 * (1.0f - t) + g_w1 * c1 * t) / S.s0 + g_s0 * cth;
        // theta0 = acos(dot'):  d theta0 / d dot' = -1 / sqrt(1 - dot'^2) = -1 / sin(theta0)
        const float g_dotf = -g_theta0 / S.s0;
        // dot' = (a . b'), b' = the flipped b: the two sign changes of the flip cancel in d a and meet in d b'
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ga[i] += g_dotf * S.b[i];
            gb[i] += g_dotf * S.a[i];
        }
    }
    // b' = +-b, then a = q0 / |q0|, b = q1 / |q1|
    float da = 0.f, db = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        da += ga[i] * S.a[i];
        db += gb[i] * S.b[i];
    }
    const float sgn = S.flip ? -1.0f : 1.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        g_q0[i] = (ga[i] - S.a[i] * da) / S.na;
        g_q1[i] = sgn * (gb[i] - S.b[i] * db) / S.nb;
    }
}

// quat_to_rot_mat, without normalisation
__device__ __forceinline__ void quat_to_rot(const float q[4], float R[9])
{
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0f - 2.0f * (y * y + z * z);
    R[1] = 2.0f * (x * y - w * z);
    R[2] = 2.0f * (x * z + w * y);
    R[3] = 2.0f * (x * y + w * z);
    R[4] = 1.0f - 2.0f * (x * x + z * z);
    R[5] = 2.0f * (y * z - w * x);
    R[6] = 2.0f * (x * z - w * y);
    R[7] = 2.0f * (y * z + w * x);
    R[8] = 1.0f - 2.0f * (x * x + y * y);
}

__device__ __forceinline__ void quat_to_rot_bwd(const float q[4], const float g[9], float gq[4])
{
    const float w = q[0], x = q[1], y = q[2], z = q[3];
    gq[0] = 2.0f * (-z * g[1] + y * g[2] + z * g[3] - x * g[5] - y * g[6] + x * g[7]);
    gq[1] = 2.0f * (y * g[1] + z * g[2] + y * g[3] - 2.0f * x * g[4] - w * g[5] + z * g[6] + w * g[7] - 2.0f * x * g[8]);
    gq[2] = 2.0f * (-2.0f * y * g[0] + x * g[1] + w * g[2] + x * g[3] + z * g[5] - w * g[6] + z * g[7] - 2.0f * y * g[8]);
    gq[3] = 2.0f * (-2.0f * z * g[0] - w * g[1] + x * g[2] + w * g[3] - 2.0f * z * g[4] + y * g[5] + x * g[6] + y * g[7]);
}

// what both kernels need of a query: where its row lives and whether it is an "evs" row
struct Row {
    int seg;          // 0 colour | 1 prev | 2 next
    int row;          // row of that table
    bool evs;
};

__device__ __forceinline__ Row locate(const lse_spline_desc &D, int q)
{
    Row r;
    const int n0 = D.n_query[0], n1 = D.n_query[1];
    r.seg = q < n0 ? 0 : (q < n0 + n1 ? 1 : 2);
    r.row = q - (r.seg == 0 ? 0 : (r.seg == 1 ? n0 : n0 + n1));
    r.evs = (r.seg == 0 ? D.evs[0] : (r.seg == 1 ? D.evs[1] : D.evs[2])) != 0;      // (selects: no dynamic index into the arguments)
    return r;
}

// dM' = dM with its translation column times scale (row 3 as it is)
__device__ __forceinline__ float dm_entry(const lse_spline_desc &D, float scale, int k, int j)
{
    const float v = D.dM[4 * k + j];
    return (j == 3 && k < 3) ? v * scale : v;
}

// forward of one query up to the slerp (kept for the backward) and the plain pose [R | T]
__device__ __forceinline__ void query_pose(const lse_spline_desc &D, int q, Slerp &S, float quat[4], float P[12], int *k_out, float *t_out)
{
    const int k = clampi(D.idx[q], 0, D.n_ctrl - 2);       // (a descriptor whose indices leave the table must not leave memory)
    const float t = D.frac[q];
    const float *c0 = D.ctrl_tangents + 6 * (int64_t)k, *c1 = c0 + 6;
    float q0[4], q1[4];
    rotvec_to_quat(c0 + 3, q0);
    rotvec_to_quat(c1 + 3, q1);
    slerp_fwd(q0, q1, t, S, quat);
    float R[9];
    quat_to_rot(quat, R);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        P[4 * i] = R[3 * i];
        P[4 * i + 1] = R[3 * i + 1];
        P[4 * i + 2] = R[3 * i + 2];
        P[4 * i + 3] = (1.0f - t) * c0[i] + t * c1[i];
    }
    *k_out = k;
    *t_out = t;
}

__global__ __launch_bounds__(kThreads) void spline_fwd_kernel(lse_spline_desc D, float *__restrict__ o_col, float *__restrict__ o_prev,
                                                              float *__restrict__ o_next, int n_total)
{
    const int q = blockIdx.x * kThreads + threadIdx.x;
    if (q >= n_total) return;
    const Row r = locate(D, q);
    Slerp S;
    float quat[4], P[12], t;
    int k;
    query_pose(D, q, S, quat, P, &k, &t);
    float *dst = (r.seg == 0 ? o_col : (r.seg == 1 ? o_prev : o_next)) + 12 * (int64_t)r.row;
    if (!r.evs) {
#pragma unroll
        for (int e = 0; e < 12; ++e) dst[e] = P[e];
        return;
    }
    const float scale = *D.scale;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float acc = 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) acc += P[4 * i + m] * dm_entry(D, scale, m, j);
            dst[4 * i + j] = acc;
        }
}

// the share of an "evs" row in d scale: only the translation column of dM' depends on scale, so with out = P dM'
// d scale = sum_{m < 3} dM[m][3] sum_i P[i][m] g[i][3] -- the forward pose and the row's gradient, no derivative of the spline
__device__ __forceinline__ float query_dscale(const lse_spline_desc &D, int q, const float *__restrict__ g_col, const float *__restrict__ g_prev,
                                              const float *__restrict__ g_next)
{
    const Row r = locate(D, q);
    Slerp S;
    float quat[4], P[12], t;
    int k;
    query_pose(D, q, S, quat, P, &k, &t);
    const float *g = (r.seg == 0 ? g_col : (r.seg == 1 ? g_prev : g_next)) + 12 * (int64_t)r.row;
    float ds = 0.f;
#pragma unroll
    for (int m = 0; m < 3; ++m) ds += D.dM[4 * m + 3] * (P[m] * g[3] + P[4 + m] * g[7] + P[8 + m] * g[11]);
    return ds;
}

// the derivative of one query's table row: d0 / d1 = the shares of control points idx / idx + 1 (translation, rotation vector)
__device__ __forceinline__ void query_bwd(const lse_spline_desc &D, int q, const float *__restrict__ g_col, const float *__restrict__ g_prev,
                                          const float *__restrict__ g_next, float d0[6], float d1[6], int *k_out)
{
    const Row r = locate(D, q);
    Slerp S;
    float quat[4], P[12], t;
    int k;
    query_pose(D, q, S, quat, P, &k, &t);
    const float *g = (r.seg == 0 ? g_col : (r.seg == 1 ? g_prev : g_next)) + 12 * (int64_t)r.row;
    float gP[12];
    if (r.evs) {          // out = P dM':  d P[i][m] = sum_j g[i][j] dM'[m][j]
        const float scale = *D.scale;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc += g[4 * i + j] * dm_entry(D, scale, m, j);
                gP[4 * i + m] = acc;
            }
    } else {
#pragma unroll
        for (int e = 0; e < 12; ++e) gP[e] = g[e];
    }
    const float gR[9] = {gP[0], gP[1], gP[2], gP[4], gP[5], gP[6], gP[8], gP[9], gP[10]};
    float g_quat[4], g_q0[4], g_q1[4];
    quat_to_rot_bwd(quat, gR, g_quat);
    slerp_bwd(S, t, g_quat, g_q0, g_q1);
    const float *c0 = D.ctrl_tangents + 6 * (int64_t)k, *c1 = c0 + 6;
    rotvec_to_quat_bwd(c0 + 3, g_q0, d0 + 3);
    rotvec_to_quat_bwd(c1 + 3, g_q1, d1 + 3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d0[i] = (1.0f - t) * gP[4 * i + 3];
        d1[i] = t * gP[4 * i + 3];
    }
    *k_out = k;
}

// blocks [0, ctrl_blocks): one wave per control point; block ctrl_blocks: d scale
__global__ __launch_bounds__(kThreads) void spline_bwd_kernel(lse_spline_desc D, const float *__restrict__ g_col,
                                                              const float *__restrict__ g_prev, const float *__restrict__ g_next,
                                                              float *__restrict__ d_ctrl, float *__restrict__ d_scale_out, int n_total,
                                                              int ctrl_blocks)
{
    __shared__ float part[kThreads / 64];
    const int lane = lse::lane_id();
    if ((int)blockIdx.x == ctrl_blocks) {        // (the whole block takes this branch: the barrier below is reached by all of it)
        float acc = 0.f;
        for (int q = threadIdx.x; q < n_total; q += kThreads) {
            if (!locate(D, q).evs) continue;
            acc += query_dscale(D, q, g_col, g_prev, g_next);
        }
        acc = lse::wave_sum(acc);
        if (lane == 0) part[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float v = part[0];
#pragma unroll
            for (int w = 1; w < kThreads / 64; ++w) v += part[w];
            d_scale_out[0] = v;
        }
        return;
    }
    const int cp = (blockIdx.x * kThreads + threadIdx.x) >> 6;
    if (cp >= D.n_ctrl) return;                  // (whole waves leave together: `cp` is wave-uniform)
    const int lo = clampi(D.csr_start[cp], 0, D.csr_len), hi = clampi(D.csr_start[cp + 1], lo, D.csr_len);
    float acc[6], d0[6], d1[6];
    int k;
#pragma unroll
    for (int e = 0; e < 6; ++e) acc[e] = 0.f;
    for (int j = lo + lane; j < hi; j += 64) {
        const int q = clampi(D.csr_query[j], 0, n_total - 1);
        query_bwd(D, q, g_col, g_prev, g_next, d0, d1, &k);
        const bool first = k == cp;              // this control point is the query's idx, else its idx + 1
#pragma unroll
        for (int e = 0; e < 6; ++e) acc[e] += first ? d0[e] : d1[e];
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) acc[e] = lse::wave_sum(acc[e]);
    if (lane < 6) {
        float v = acc[0];
#pragma unroll
        for (int e = 1; e < 6; ++e) v = lane == e ? acc[e] : v;
        d_ctrl[6 * (int64_t)cp + lane] = v;
    }
}

int check_desc(const lse_spline_desc *d, const char *what, int64_t *n_total)
{
    LSE_REQUIRE(d, "%s: null descriptor", what);
    LSE_REQUIRE(d->n_ctrl >= 2, "%s: a spline needs at least two control points (got %d)", what, d->n_ctrl);
    int64_t n = 0;
    for (int s = 0; s < 3; ++s) {
        LSE_REQUIRE(d->n_query[s] >= 0, "%s: n_query[%d] < 0", what, s);
        LSE_REQUIRE(d->evs[s] == 0 || d->evs[s] == 1, "%s: evs[%d] must be 0 or 1 (got %d)", what, s, d->evs[s]);
        n += d->n_query[s];
    }
    LSE_REQUIRE(n >= 1 && n < (1 << 24), "%s: %lld queries (1 .. 2^24 - 1)", what, (long long)n);
    LSE_REQUIRE(d->ctrl_tangents && d->scale && d->idx && d->frac, "%s: null parameter or bracket table", what);
    *n_total = n;
    return LSE_OK;
}

}  // namespace

extern "C" int lse_spline_poses(const lse_spline_desc *desc, float *col_pose, float *prev_pose, float *next_pose, lse_stream_t stream)
{
    const char *what = "lse_spline_poses";
    int64_t n = 0;
    const int rc = check_desc(desc, what, &n);
    if (rc != LSE_OK) return rc;
    float *out[3] = {col_pose, prev_pose, next_pose};
    for (int s = 0; s < 3; ++s) LSE_REQUIRE(desc->n_query[s] == 0 || out[s], "%s: null pose table of segment %d", what, s);
    hipLaunchKernelGGL(spline_fwd_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, lse::as_stream(stream),
                       *desc, col_pose, prev_pose, next_pose, (int)n);
    return lse::check_launch(what);
}

extern "C" int lse_spline_poses_bwd(const lse_spline_desc *desc, const float *d_col_pose, const float *d_prev_pose,
                                    const float *d_next_pose, float *d_ctrl_tangents, float *d_scale, lse_stream_t stream)
{
    const char *what = "lse_spline_poses_bwd";
    int64_t n = 0;
    const int rc = check_desc(desc, what, &n);
    if (rc != LSE_OK) return rc;
    const float *g[3] = {d_col_pose, d_prev_pose, d_next_pose};
    for (int s = 0; s < 3; ++s) LSE_REQUIRE(desc->n_query[s] == 0 || g[s], "%s: null table gradient of segment %d", what, s);
    LSE_REQUIRE(d_ctrl_tangents && d_scale, "%s: null output", what);
    LSE_REQUIRE(desc->csr_start && desc->csr_query, "%s: null query lists", what);
    LSE_REQUIRE(desc->csr_len == 2 * n, "%s: csr_len %d, but every one of the %lld queries is on two lists", what, desc->csr_len,
                (long long)n);
    const int waves_per_block = kThreads / 64;
    const int ctrl_blocks = (desc->n_ctrl + waves_per_block - 1) / waves_per_block;
    hipLaunchKernelGGL(spline_bwd_kernel, dim3((unsigned)ctrl_blocks + 1), dim3(kThreads), 0, lse::as_stream(stream), *desc, d_col_pose,
                       d_prev_pose, d_next_pose, d_ctrl_tangents, d_scale, (int)n, ctrl_blocks);
    return lse::check_launch(what);
}
