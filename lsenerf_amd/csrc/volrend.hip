// Packed per-ray transmittance scan + alpha compositing for gfx950, forward and backward:
//   nerfacc.render_weight_from_density            R:lse_nerf/lsenerf.py:301-306
//   nerfacc.render_visibility_from_density        R:lse_nerf/lse_grid_estimator.py:120-127
//   RGB / accumulation / depth renderers          R:lse_nerf/lsenerf.py:309-318, R:lse_nerf/lse_renderer.py:6-10
//
// One 64-lane wave owns one ray: its samples are contiguous (packed, ray-sorted), so a chunk of 64 samples is
// one coalesced load per stream, the exclusive sum of sigma*dt is a wave prefix scan with a scalar carry between
// chunks, and the per-ray sums (rgb, accumulation, depth numerator) are wave reductions -- no atomics, no
// index_add_, deterministic.  The backward is the same walk in reverse with suffix scans:
//     dL/d(sd_k) = dw_k * T_{k+1} - sum_{i>k} dw_i w_i ,   T_{k+1} = T_end + sum_{i>k} w_i ,  T_end = 1 - sum_i w_i
// (T_{k+1} = T_k - w_k exactly, so no transmittance array is stored and no cancellation-prone prefix is formed).
#include "common.h"

namespace {

__device__ __forceinline__ float wave_inclusive_sum_rev(float v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        float nb = __shfl_down(v, off, 64);
        if (lse::lane_id() + off < 64) v += nb;
    }
    return v;
}

// Weights of one 64-sample group of a ray (sample k of the ray on lane k mod 64): T, alpha and w = T * alpha of this lane's sample
// [a, b) with density sg; `carry` is the optical depth in front of the group and is advanced past it.  The SINGLE definition of the
// scan: the training forward and the three eval compositors call it and so agree bit for bit (tests/test_gpu_eval.py,
// tests/test_gpu_compositing.py).  Contraction is off and the one fused step is written out: the first step of the sigma * dt prefix
// scan is fmaf(sg, dt, neighbour); the other five steps, excl + carry and the carry update are plain adds, T * alpha a plain product.
// The exclusive prefix is the inclusive one shifted by a lane (as in visibility_kernel), not `incl - sd`: a surface sample of a
// trained scene has sd = 1e2 .. 1e5 and beyond, and the subtraction would return the optical depth in front of it -- which decides
// that sample's weight, the largest of the ray -- to half an ulp of sd; at sd = +inf it is inf - inf = NaN.
// tau_front / tau_behind: the optical depth in front of and behind this lane's sample (excl + carry and incl + carry, the carry as it
// stood before the group) -- the accumulated weight through the sample is 1 - exp(-tau_behind), and on lane 63 tau_behind is the
// bit pattern the next group's carry starts from.  The depth-quantile kernels search them; the compositors do not read them.
struct GroupWeights { float w, T, alpha, tau_front, tau_behind; };

__device__ __forceinline__ GroupWeights group_weights(float a, float b, float sg, bool valid, int lane, float &carry)
{
#pragma clang fp contract(off)
    const float dt = b - a;
    const float sd = sg * dt;
    float incl = sd;
    {
        const float nb = __shfl_up(incl, 1, 64);
        if (lane >= 1) incl = fmaf(sg, dt, nb);
    }
#pragma unroll
    for (int off = 2; off < 64; off <<= 1) {
        const float nb = __shfl_up(incl, off, 64);
        if (lane >= off) incl = incl + nb;
    }
    float excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.f;
    GroupWeights g;
    g.tau_front = excl + carry;
    g.tau_behind = incl + carry;
    g.T = expf(-(excl + carry));
    g.alpha = 1.f - expf(-sd);
    g.w = valid ? g.T * g.alpha : 0.f;
    carry = carry + __shfl(incl, 63, 64);
    return g;
}

// smallest / largest interval mid-point over the wave (DepthRenderer's clip range of the ray); min / max are exact in any order
__device__ __forceinline__ void wave_mid_range(float &mlo, float &mhi)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mlo = fminf(mlo, __shfl_xor(mlo, off, 64));
        mhi = fmaxf(mhi, __shfl_xor(mhi, off, 64));
    }
}

__global__ __launch_bounds__(256) void volrend_fwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                          const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                          int rgb_stride, const int64_t *__restrict__ packed, int n_rays,
                                                          float *__restrict__ weights, float *__restrict__ out_rgb,
                                                          float *__restrict__ out_acc, float *__restrict__ out_dep,
                                                          float *__restrict__ trans, float *__restrict__ alphas,
                                                          float *__restrict__ mid_range)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    float carry = 0.f, ar = 0.f, ag = 0.f, ab = 0.f, aw = 0.f, ad = 0.f;
    float mlo = INFINITY, mhi = -INFINITY;   // smallest / largest interval mid-point of this ray (DepthRenderer's clip range)
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float a = 0.f, b = 0.f, sg = 0.f;
        if (valid) { a = ts[i]; b = te[i]; sg = sigma[i]; }
        const GroupWeights g = group_weights(a, b, sg, valid, lane, carry);
        const float w = g.w;
        if (valid) {
            weights[i] = w;
            if (trans) trans[i] = g.T;
            if (alphas) alphas[i] = g.alpha;
            mlo = fminf(mlo, (a + b) * 0.5f);
            mhi = fmaxf(mhi, (a + b) * 0.5f);
            if (rgb) {
                const float *c = rgb + i * rgb_stride;
                ar = fmaf(w, c[0], ar);
                ag = fmaf(w, c[1], ag);
                ab = fmaf(w, c[2], ab);
            }
            aw += w;
            ad = fmaf(w, (a + b) * 0.5f, ad);
        }
    }
    ar = lse::wave_sum(ar); ag = lse::wave_sum(ag); ab = lse::wave_sum(ab);
    aw = lse::wave_sum(aw); ad = lse::wave_sum(ad);
    if (mid_range) wave_mid_range(mlo, mhi);
    if (lane == 0) {
        if (out_rgb) { out_rgb[ray * 3 + 0] = ar; out_rgb[ray * 3 + 1] = ag; out_rgb[ray * 3 + 2] = ab; }
        if (out_acc) out_acc[ray] = aw;
        if (out_dep) out_dep[ray] = ad;
        if (mid_range) { mid_range[2 * ray] = mlo; mid_range[2 * ray + 1] = mhi; }
    }
}

// DepthRenderer("expected") epilogue (nerfstudio 0.3.2): depth = num / (acc + 1e-10), clipped to the
// GLOBAL [min, max] of the interval mid-points.  Samples are sorted inside a ray, so the global range is the min / max over
// the per-ray ranges the forward kernel leaves in mid_range[R][2] -- an O(R) reduction in one workgroup instead of two
// reductions over all N samples.  range_out[2] keeps (lo, hi) for the backward.
__global__ __launch_bounds__(1024) void depth_finish_kernel(const float *__restrict__ num, const float *__restrict__ acc,
                                                            const float *__restrict__ mid_range, int n_rays,
                                                            float *__restrict__ depth, float *__restrict__ range_out)
{
    __shared__ float s_lo[16], s_hi[16];
    float lo = INFINITY, hi = -INFINITY;
    for (int r = threadIdx.x; r < n_rays; r += 1024) {
        lo = fminf(lo, mid_range[2 * r]);
        hi = fmaxf(hi, mid_range[2 * r + 1]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    lo = s_lo[0]; hi = s_hi[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) { lo = fminf(lo, s_lo[w]); hi = fmaxf(hi, s_hi[w]); }
    if (threadIdx.x == 0 && range_out) { range_out[0] = lo; range_out[1] = hi; }
    const bool any = lo <= hi;     // no sample at all: nerfstudio's clip is skipped (steps is empty)
    for (int r = threadIdx.x; r < n_rays; r += 1024) {
        float d = num[r] / (acc[r] + 1e-10f);
        if (any) d = fminf(fmaxf(d, lo), hi);
        depth[r] = d;
    }
}

// torch.nan_to_num with its defaults: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX
__device__ __forceinline__ float nan_to_num(float v)
{
    if (v != v) return 0.f;
    if (v == INFINITY) return 3.402823466e+38f;
    if (v == -INFINITY) return -3.402823466e+38f;
    return v;
}

// torch.clamp(v, 0, 1): NaN stays NaN
__device__ __forceinline__ float clamp01(float v)
{
    if (v != v) return v;
    return v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
}

// Lane accumulators of an eval render's ray: colour, accumulation, depth numerator and the range of the interval mid-points
struct RayAccum {
    float r, g, b, w, d, mlo, mhi;
};

// One valid sample into the lane accumulators (eval_composite_kernel and its segmented form): colour and depth numerator by fmaf,
// the accumulation by a plain add, as volrend_fwd_kernel forms them.
__device__ __forceinline__ void accumulate_sample(RayAccum &acc, float w, float a, float b, const float *__restrict__ c, bool fix_nan)
{
#pragma clang fp contract(off)
    const float mid = (a + b) * 0.5f;
    acc.mlo = fminf(acc.mlo, mid);
    acc.mhi = fmaxf(acc.mhi, mid);
    float c0 = c[0], c1 = c[1], c2 = c[2];
    if (fix_nan) { c0 = nan_to_num(c0); c1 = nan_to_num(c1); c2 = nan_to_num(c2); }
    acc.r = fmaf(w, c0, acc.r);
    acc.g = fmaf(w, c1, acc.g);
    acc.b = fmaf(w, c2, acc.b);
    acc.w = acc.w + w;
    acc.d = fmaf(w, mid, acc.d);
}

// The end of an eval render's ray (eval_composite_kernel and eval_segment_finish_kernel): the five wave reductions in this order,
// then on lane 0 the renderer epilogue of LSENeRFModel.render_packed; the depth numerator and the ray's mid-point range (acc.mlo /
// acc.mhi, already reduced) go to the workspace for depth_finish_kernel (the chunk-wide clip range of DepthRenderer("expected")).
__device__ __forceinline__ void finish_ray(RayAccum acc, int64_t nsamples, int lane, int ray, int flags, float background,
                                           float *__restrict__ mid_range, float *__restrict__ num, float *__restrict__ out_rgb,
                                           float *__restrict__ out_acc, int64_t *__restrict__ out_nsamples)
{
#pragma clang fp contract(off)
    float ar = lse::wave_sum(acc.r), ag = lse::wave_sum(acc.g), ab = lse::wave_sum(acc.b);
    const float aw = lse::wave_sum(acc.w), ad = lse::wave_sum(acc.d);
    if (lane == 0) {
        if (flags & LSE_EVAL_BACKGROUND) {     // rgb + bg * (1 - acc)
            const float rest = background * (1.f - aw);
            ar = ar + rest; ag = ag + rest; ab = ab + rest;
        }
        if (flags & LSE_EVAL_CLAMP) { ar = clamp01(ar); ag = clamp01(ag); ab = clamp01(ab); }
        out_rgb[ray * 3 + 0] = ar; out_rgb[ray * 3 + 1] = ag; out_rgb[ray * 3 + 2] = ab;
        out_acc[ray] = aw;
        num[ray] = ad;
        mid_range[2 * ray] = acc.mlo; mid_range[2 * ray + 1] = acc.mhi;
        out_nsamples[ray] = nsamples;
    }
}

// Forward-only compositing of an evaluation render (lse_eval_composite): the per-ray walk of volrend_fwd_kernel with its weights
// (group_weights) and no per-sample output; eval_depth_finish follows (depth_finish_kernel).
__global__ __launch_bounds__(256) void eval_composite_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                             const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                             int rgb_stride, const int64_t *__restrict__ packed, int n_rays,
                                                             int flags, float background, float *__restrict__ mid_range,
                                                             float *__restrict__ num, float *__restrict__ out_rgb,
                                                             float *__restrict__ out_acc, int64_t *__restrict__ out_nsamples)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    const bool fix_nan = (flags & LSE_EVAL_NAN_TO_NUM) != 0;
    float carry = 0.f;
    RayAccum acc = {0.f, 0.f, 0.f, 0.f, 0.f, INFINITY, -INFINITY};
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float a = 0.f, b = 0.f, sg = 0.f;
        if (valid) { a = ts[i]; b = te[i]; sg = sigma[i]; }
        const float w = group_weights(a, b, sg, valid, lane, carry).w;
        if (valid) accumulate_sample(acc, w, a, b, rgb + i * rgb_stride, fix_nan);
    }
    wave_mid_range(acc.mlo, acc.mhi);
    finish_ray(acc, cnt, lane, ray, flags, background, mid_range, num, out_rgb, out_acc, out_nsamples);
}

#include "positions.h"      // Box, positions_bwd_sample: the world-space Jacobian of the normals

// Rendered normals of an evaluation render (lse_eval_composite_normals): the sample-to-lane walk and the weights of
// eval_composite_kernel (group_weights), with a vector in place of the colour.  Per sample: g = d_x01 (the gradient of the density
// logit), optionally through the transposed Jacobian of the position map at the sample's position (LSE_NORMALS_WORLD),
// n = -g / max(|g|, 1e-12) (F.normalize: a zero gradient gives a zero normal); per ray N = sum w n, then N / (|N| + 1e-10) with
// LSE_NORMALS_RENORMALIZE (NormalsRenderer).  A ray without samples writes zeros.
__global__ __launch_bounds__(256) void eval_composite_normals_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                     const float *__restrict__ sigma, const float *__restrict__ dx01,
                                                                     const int64_t *__restrict__ packed, int n_rays,
                                                                     const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                                     int contraction, Box box, int flags, float *__restrict__ out)
{
#pragma clang fp contract(off)   // the normal arithmetic below rounds step by step; the weights are group_weights'
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    const bool world = (flags & LSE_NORMALS_WORLD) != 0;
    float ro[3] = {0.f, 0.f, 0.f}, rd[3] = {0.f, 0.f, 0.f};
    if (world) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { ro[k] = rays_o[(int64_t)ray * 3 + k]; rd[k] = rays_d[(int64_t)ray * 3 + k]; }
    }
    float carry = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float a = 0.f, b = 0.f, sg = 0.f;
        if (valid) { a = ts[i]; b = te[i]; sg = sigma[i]; }
        const float w = group_weights(a, b, sg, valid, lane, carry).w;
        if (valid) {
            float g[3] = {dx01[i * 3 + 0], dx01[i * 3 + 1], dx01[i * 3 + 2]};
            if (world) {
                const float s = a + b;
                float p[3], gw[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = ro[k] + rd[k] * s / 2.f;      // the sample position of lse_positions_fwd
                positions_bwd_sample(p, g, contraction, box, gw);
#pragma unroll
                for (int k = 0; k < 3; ++k) g[k] = gw[k];
            }
            const float len = sqrtf(fmaf(g[2], g[2], fmaf(g[1], g[1], g[0] * g[0])));
            const float inv = -1.f / fmaxf(len, 1e-12f);
            nx = fmaf(w, g[0] * inv, nx);
            ny = fmaf(w, g[1] * inv, ny);
            nz = fmaf(w, g[2] * inv, nz);
        }
    }
    nx = lse::wave_sum(nx); ny = lse::wave_sum(ny); nz = lse::wave_sum(nz);
    if (lane == 0) {
        if (flags & LSE_NORMALS_RENORMALIZE) {
            const float len = sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx))) + 1e-10f;
            nx = nx / len; ny = ny / len; nz = nz / len;
        }
        out[(int64_t)ray * 3 + 0] = nx; out[(int64_t)ray * 3 + 1] = ny; out[(int64_t)ray * 3 + 2] = nz;
    }
}

// Early ray termination of the eval render (lse_eval_segment_begin / lse_eval_composite_segment / lse_eval_composite_finish): the
// walk of eval_composite_kernel cut into segments of the ray, with the field evaluated between two segments only for the rays that
// are still alive.  Sample k of a ray goes to lane k mod 64 there; every segment starts at a multiple of 64, so here the same lane
// meets the same samples, and the loop body is that kernel's (group_weights, accumulate_sample): compositing the first m samples of
// a ray in segments gives the bits eval_composite_kernel gives for a ray of m samples.  That needs the lane accumulators carried as
// they are -- the wave reduction happens once, in the finishing kernel (finish_ray).  State of one ray (kSegStateFloats floats,
// 1312 bytes):
//   [a * 64 + lane], a = 0..4   lane accumulators: r, g, b, weight, depth numerator
//   [320] carry                 the optical depth in front of the next 64-sample group (the very value the scan carries)
//   [321], [322]                smallest / largest interval mid-point composited so far (min / max are exact: reduced per segment)
//   [323], [324] as int32       samples composited so far; alive (1 while the ray still takes part)
constexpr int kSegStateFloats = 328;     // padded to a multiple of 4 floats: every ray's row is 16-byte aligned
constexpr int kSegCarry = 320, kSegMidLo = 321, kSegMidHi = 322, kSegInts = 323;

__global__ __launch_bounds__(256) void eval_segment_begin_kernel(const int64_t *__restrict__ ray_cnts, int n_rays, int64_t first_len,
                                                                 float *__restrict__ state, int64_t *__restrict__ seg_cnts)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    float *st = state + (int64_t)ray * kSegStateFloats;
#pragma unroll
    for (int a = 0; a < 5; ++a) st[a * 64 + lane] = 0.f;
    if (lane == 0) {
        st[kSegCarry] = 0.f;
        st[kSegMidLo] = INFINITY;
        st[kSegMidHi] = -INFINITY;
        int32_t *si = reinterpret_cast<int32_t *>(st + kSegInts);
        si[0] = 0;
        si[1] = 1;
        st[325] = 0.f; st[326] = 0.f; st[327] = 0.f;
        const int64_t c = ray_cnts[ray];
        seg_cnts[ray] = c < 0 ? 0 : (c < first_len ? c : first_len);
    }
}

__global__ __launch_bounds__(256) void eval_composite_segment_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                     const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                                     int rgb_stride, const int64_t *__restrict__ seg_packed,
                                                                     const int64_t *__restrict__ ray_cnts, int n_rays, int flags,
                                                                     int64_t seg_end, int64_t next_len, float tau_stop,
                                                                     float *state, int64_t *__restrict__ next_seg_cnts)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    float *st = state + (int64_t)ray * kSegStateFloats;
    int32_t *si = reinterpret_cast<int32_t *>(st + kSegInts);
    // (the packed count is authoritative for what is composited: on segment 0 it may hold nerfstudio's fake sample of a ray
    // whose own count is 0; a finished ray has 0 here and touches none of its accumulators)
    const int64_t s0 = seg_packed[2 * ray], cnt = seg_packed[2 * ray + 1];
    const bool fix_nan = (flags & LSE_EVAL_NAN_TO_NUM) != 0;
    const bool alive = si[1] != 0;
    float carry = st[kSegCarry];
    if (cnt > 0) {
        RayAccum acc = {st[lane], st[64 + lane], st[128 + lane], st[192 + lane], st[256 + lane], st[kSegMidLo], st[kSegMidHi]};
        for (int64_t base = 0; base < cnt; base += 64) {
            const int64_t i = s0 + base + lane;
            const bool valid = base + lane < cnt;
            float a = 0.f, b = 0.f, sg = 0.f;
            if (valid) { a = ts[i]; b = te[i]; sg = sigma[i]; }
            const float w = group_weights(a, b, sg, valid, lane, carry).w;
            if (valid) accumulate_sample(acc, w, a, b, rgb + i * rgb_stride, fix_nan);
        }
        st[lane] = acc.r; st[64 + lane] = acc.g; st[128 + lane] = acc.b; st[192 + lane] = acc.w; st[256 + lane] = acc.d;
        wave_mid_range(acc.mlo, acc.mhi);
        if (lane == 0) {
            st[kSegCarry] = carry;
            st[kSegMidLo] = acc.mlo;
            st[kSegMidHi] = acc.mhi;
            si[0] += (int32_t)cnt;
        }
    }
    if (lane == 0) {
        // finished: no sample left, or the optical depth so far has reached tau_stop (+inf does; a NaN never compares true, so
        // that ray is rendered in full)
        const int64_t left = ray_cnts[ray] - seg_end;
        const bool go = alive && left > 0 && !(carry >= tau_stop);
        si[1] = go ? 1 : 0;
        if (next_seg_cnts) next_seg_cnts[ray] = go ? (left < next_len ? left : next_len) : 0;
    }
}

// The end of eval_composite_kernel for a segmented ray: finish_ray on the state the segments left.
__global__ __launch_bounds__(256) void eval_segment_finish_kernel(const float *__restrict__ state, int n_rays, int flags,
                                                                  float background, float *__restrict__ mid_range,
                                                                  float *__restrict__ num, float *__restrict__ out_rgb,
                                                                  float *__restrict__ out_acc, int64_t *__restrict__ out_nsamples)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const float *st = state + (int64_t)ray * kSegStateFloats;
    const RayAccum acc = {st[lane], st[64 + lane], st[128 + lane], st[192 + lane], st[256 + lane], st[kSegMidLo], st[kSegMidHi]};
    finish_ray(acc, reinterpret_cast<const int32_t *>(st + kSegInts)[0], lane, ray, flags, background, mid_range, num, out_rgb,
               out_acc, out_nsamples);
}

// Quantile depths of an evaluation render (lse_eval_depth_quantiles and its segmented form; include/lse_hip.h has the definition):
// the walk of eval_composite_kernel with its scan (group_weights), searched instead of summed.  The accumulated weight through
// sample k is 1 - exp(-tau_behind(k)), so "the weights up to k reach q" is tau_behind(k) >= tau_q = -ln(1 - q): one comparison per
// lane, the first crossing of a group by a ballot and a find-first-set, its depth fetched from that lane.  Everything that is kept
// (the depths, the found mask) is the same on all 64 lanes; no atomics, no LDS.
struct DepthTaus { float v[4]; };

__device__ __forceinline__ float pick4(const float (&v)[4], int j)      // v[j] without a dynamically indexed register array
{
    return j == 0 ? v[0] : (j == 1 ? v[1] : (j == 2 ? v[2] : v[3]));
}

// One 64-sample group into the search: for every quantile not found yet, the first valid lane with tau_behind >= tau_q (a NaN never
// compares true, +inf does) gives the depth -- the sample's mid-point, or with `interp` the crossing under piecewise-constant
// density, a + (tau_q - tau_front) / sigma clamped to [a, b] (sigma = +inf: a; a NaN quotient: the mid-point).
__device__ __forceinline__ void quantile_group(const GroupWeights &g, float a, float b, float sg, float mid, bool valid,
                                               const DepthTaus &tau, int n_q, bool interp, float (&dq)[4], int &found)
{
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= n_q || ((found >> j) & 1)) continue;
        const unsigned long long hit = __ballot(valid && g.tau_behind >= tau.v[j]);
        if (hit == 0ull) continue;
        float d = mid;
        if (interp) {
            const float x = (tau.v[j] - g.tau_front) / sg;
            if (x == x) d = fminf(fmaxf(a + x, a), b);
        }
        dq[j] = __shfl(d, __ffsll(hit) - 1, 64);
        found |= 1 << j;
    }
}

// depth_sel of one ray from its quantile depths: depth_q[sel] where quantile sel was reached and -- with a finite max_spread -- the
// last quantile was reached too and lies at most max_spread behind the first; NaN ("no usable depth") otherwise.
__device__ __forceinline__ float select_depth(const float (&dq)[4], int found, int n_q, int flags, float max_spread)
{
#pragma clang fp contract(off)
    const int sel = (flags >> 8) & 3;
    bool ok = ((found >> sel) & 1) != 0;
    if (max_spread < INFINITY) ok = ok && ((found >> (n_q - 1)) & 1) && (pick4(dq, n_q - 1) - dq[0] <= max_spread);
    return ok ? pick4(dq, sel) : NAN;
}

__global__ __launch_bounds__(256) void eval_depth_quantiles_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                   const float *__restrict__ sigma, const int64_t *__restrict__ packed,
                                                                   int n_rays, DepthTaus tau, int n_q, int flags, float max_spread,
                                                                   float *__restrict__ depth_q, uint8_t *__restrict__ reached,
                                                                   float *__restrict__ depth_sel)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    const bool interp = (flags & LSE_DEPTH_INTERPOLATE) != 0;
    const int full = (1 << n_q) - 1;
    float carry = 0.f, mid = 0.f;
    float dq[4] = {0.f, 0.f, 0.f, 0.f};
    int found = 0;
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float a = 0.f, b = 0.f, sg = 0.f;
        if (valid) { a = ts[i]; b = te[i]; sg = sigma[i]; }
        const GroupWeights g = group_weights(a, b, sg, valid, lane, carry);
        mid = (a + b) * 0.5f;
        quantile_group(g, a, b, sg, mid, valid, tau, n_q, interp, dq, found);
        if (found == full) break;        // (the same on every lane) nothing behind the last crossing is needed
    }
    if (found != full && cnt > 0) {      // the loop ran to the ray's end: `mid` is the last group's, the last sample's lane holds it
        const float last = __shfl(mid, (int)((cnt - 1) & 63), 64);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (!((found >> j) & 1)) dq[j] = last;
    }
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < n_q) depth_q[(int64_t)ray * n_q + j] = dq[j];
        reached[ray] = (uint8_t)found;
        if (depth_sel) depth_sel[ray] = select_depth(dq, found, n_q, flags, max_spread);
    }
}

// The same search over one segment of the early-stop route.  State of a ray, [2] floats: the carry, and the found mask as int32; a
// zero-filled state is the start.  The carry is group_weights' own, so it has the bits the compositor's state carries.  The depths
// themselves live in depth_q between the segments: a quantile found in an earlier segment is read back, not written again.
__global__ __launch_bounds__(256) void eval_depth_quantiles_segment_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                                           const float *__restrict__ sigma,
                                                                           const int64_t *__restrict__ seg_packed, int n_rays,
                                                                           DepthTaus tau, int n_q, int flags, float max_spread,
                                                                           float *state, float *depth_q, uint8_t *__restrict__ reached,
                                                                           float *__restrict__ depth_sel)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = seg_packed[2 * ray], cnt = seg_packed[2 * ray + 1];
    if (cnt <= 0) return;                // a finished (or empty) ray is left alone
    const bool interp = (flags & LSE_DEPTH_INTERPOLATE) != 0;
    const int full = (1 << n_q) - 1;
    float *st = state + 2 * (int64_t)ray;
    float carry = st[0], mid = 0.f;
    const int before = reinterpret_cast<const int32_t *>(st)[1] & full;
    if (before == full) return;          // every quantile was found in an earlier segment: the outputs are final
    float dq[4] = {0.f, 0.f, 0.f, 0.f};
    int found = before;
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float a = 0.f, b = 0.f, sg = 0.f;
        if (valid) { a = ts[i]; b = te[i]; sg = sigma[i]; }
        const GroupWeights g = group_weights(a, b, sg, valid, lane, carry);
        mid = (a + b) * 0.5f;
        quantile_group(g, a, b, sg, mid, valid, tau, n_q, interp, dq, found);
        if (found == full) break;
    }
    const float last = __shfl(mid, (int)((cnt - 1) & 63), 64);      // used only where the loop ran to the segment's end
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= n_q) continue;
            float *out = depth_q + (int64_t)ray * n_q + j;
            if ((before >> j) & 1) dq[j] = *out;
            else {
                if (!((found >> j) & 1)) dq[j] = last;
                *out = dq[j];
            }
        }
        st[0] = carry;
        reinterpret_cast<int32_t *>(st)[1] = found;
        reached[ray] = (uint8_t)found;
        if (depth_sel) depth_sel[ray] = select_depth(dq, found, n_q, flags, max_spread);
    }
}

__global__ __launch_bounds__(256) void volrend_bwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                          const float *__restrict__ sigma, const float *__restrict__ rgb,
                                                          int rgb_stride, const int64_t *__restrict__ packed, int n_rays,
                                                          const float *__restrict__ weights,
                                                          const float *__restrict__ g_rgb, const float *__restrict__ g_acc,
                                                          const float *__restrict__ g_dep, float *__restrict__ d_sigma,
                                                          float *__restrict__ d_rgb, const float *__restrict__ g_w)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    if (cnt == 0) return;
    const float gr = g_rgb ? g_rgb[ray * 3 + 0] : 0.f, gg = g_rgb ? g_rgb[ray * 3 + 1] : 0.f,
                gb = g_rgb ? g_rgb[ray * 3 + 2] : 0.f;
    const float ga = g_acc ? g_acc[ray] : 0.f, gd = g_dep ? g_dep[ray] : 0.f;
    float wtot = 0.f;
    for (int64_t base = 0; base < cnt; base += 64)
        if (base + lane < cnt) wtot += weights[s0 + base + lane];
    wtot = lse::wave_sum(wtot);
    const float t_end = 1.f - wtot;
    float carry_w = 0.f, carry_g = 0.f;
    const int64_t n_chunks = (cnt + 63) / 64;
    for (int64_t ch = n_chunks - 1; ch >= 0; --ch) {
        const int64_t base = ch * 64;
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float w = 0.f, dw = 0.f, dt = 0.f;
        if (valid) {
            w = weights[i];
            const float a = ts[i], b = te[i];
            dt = b - a;
            dw = ga + gd * ((a + b) * 0.5f);
            if (g_w) dw += g_w[i];            // per-sample gradient of the weights themselves (render_weight_from_density)
            if (rgb && g_rgb) {
                const float *c = rgb + i * rgb_stride;
                dw += gr * c[0] + gg * c[1] + gb * c[2];
            }
        }
        const float gw = dw * w;
        const float incl_w = wave_inclusive_sum_rev(w);
        const float incl_g = wave_inclusive_sum_rev(gw);
        const float sw = (incl_w - w) + carry_w;     // sum_{i>k} w_i
        const float sg = (incl_g - gw) + carry_g;    // sum_{i>k} dw_i w_i
        if (valid) {
            const float dsd = dw * (t_end + sw) - sg;
            d_sigma[i] = dsd * dt;
            if (d_rgb) {
                float *dc = d_rgb + i * rgb_stride;
                if (rgb_stride == 4) *reinterpret_cast<float4 *>(dc) = make_float4(w * gr, w * gg, w * gb, 0.f);   // pad column too
                else { dc[0] = w * gr; dc[1] = w * gg; dc[2] = w * gb; }
            }
        }
        carry_w += __shfl(incl_w, 0, 64);
        carry_g += __shfl(incl_g, 0, 64);
    }
}

// Distortion loss of mip-NeRF 360 on the render weights (lse_distortion_fwd / lse_distortion_bwd; include/lse_hip.h has the
// definition).  The mid-point of a sample is taken relative to the ray's first mid-point and formed from differences of the
// interval ends, m = t_scale * ((a - a_0) + (b - b_0)) / 2: every rounding is then relative to the ray's extent, not to its distance
// from the origin, and so are the products m W and the sums M whose difference the loss is.
__device__ __forceinline__ float distortion_mid(float a, float b, float a0, float b0, float t_scale)
{
#pragma clang fp contract(off)
    return t_scale * (((a - a0) + (b - b0)) * 0.5f);
}

// the exclusive prefix / suffix of an inclusive wave scan: the neighbour lane's value, never `incl - v`
__device__ __forceinline__ float wave_exclusive_from(float incl, int lane)
{
    const float e = __shfl_up(incl, 1, 64);
    return lane == 0 ? 0.f : e;
}

__device__ __forceinline__ float wave_exclusive_from_rev(float incl, int lane)
{
    const float e = __shfl_down(incl, 1, 64);
    return lane == 63 ? 0.f : e;
}

// Forward: one walk from the ray's first sample to its last.  Per 64-sample group two inclusive wave scans (w, w * m) with scalar
// carries give W_<i and M_<i; every lane adds its samples' terms 2 w (m W_< - M_<) + w^2 delta / 3 and one wave reduction ends the
// ray.  The carries behind the last group are (W_tot, M_tot).  Each of t_starts, t_ends, weights is read once (12 bytes per sample,
// and the ray's first interval once more); 4 (+ 8) bytes are written per ray.
__global__ __launch_bounds__(256) void distortion_fwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                             const float *__restrict__ weights, const int64_t *__restrict__ packed,
                                                             int n_rays, float t_scale, float *__restrict__ out_loss,
                                                             float *__restrict__ out_totals)
{
#pragma clang fp contract(off)
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    float carry_w = 0.f, carry_m = 0.f, acc = 0.f;
    if (cnt > 0) {
        const float a0 = ts[s0], b0 = te[s0];
        for (int64_t base = 0; base < cnt; base += 64) {
            const int64_t i = s0 + base + lane;
            const bool valid = base + lane < cnt;
            float a = a0, b = b0, w = 0.f;
            if (valid) { a = ts[i]; b = te[i]; w = weights[i]; }
            const float m = distortion_mid(a, b, a0, b0, t_scale);
            const float wm = w * m;
            const float incl_w = lse::wave_inclusive_sum(w), incl_m = lse::wave_inclusive_sum(wm);
            const float w_lt = wave_exclusive_from(incl_w, lane) + carry_w;      // W_<i
            const float m_lt = wave_exclusive_from(incl_m, lane) + carry_m;      // M_<i
            const float delta = t_scale * (b - a);
            acc = acc + ((2.f * w) * (m * w_lt - m_lt) + (w * w) * delta * (1.f / 3.f));      // (an invalid lane has w = 0)
            carry_w = carry_w + __shfl(incl_w, 63, 64);
            carry_m = carry_m + __shfl(incl_m, 63, 64);
        }
        acc = lse::wave_sum(acc);
    }
    if (lane == 0) {
        out_loss[ray] = acc;
        if (out_totals) { out_totals[2 * ray] = carry_w; out_totals[2 * ray + 1] = carry_m; }
    }
}

// Backward: one walk from the ray's last sample to its first.  The suffix scans of w and w * m give W_>i and M_>i; with the
// forward's totals W_<i = W_tot - W_>i - w_i and M_<i = M_tot - M_>i - w_i m_i, so
//     dw_i = g (2 [m_i (W_<i - W_>i) - (M_<i - M_>i)] + (2/3) w_i delta_i)
// is complete on the lane that holds sample i, and the same walk is the recurrence of volrend_bwd_kernel,
//     d_sigma_k = dt_k (dw_k (T_end + W_>k) - sum_{i>k} dw_i w_i),
// with W_>k shared and a third suffix scan for dw w.  (The subtraction from the totals is harmless where it cancels: W_<i and M_<i
// are small at the ray's start, where m_i is small too, and the error is an ulp of the total against a dw of the total's size.)
// T_end is another matter.  1 - W_tot is 0 or +-2^-24 on an opaque ray, by the last bits of the forward's expf, and here dw is not
// one value per ray as under a gradient on the accumulation: it grows with the distance from the ray's centre of mass, so behind a
// surface dw_k 2^-24 dt_k stands against a true d_sigma of ~ 0 -- 2.3e-2 of the per-ray scale on long cone-step rays
// (tests/test_distortion_cpu.py).  With `sigma` given, T_end = exp(-sum sigma dt) from a pass over the densities in front of the
// walk: a relative error, and every term of the recurrence is then as accurate as the weights are.
// Reads: weights once; t_starts and t_ends once, or twice with `sigma` (the second time out of the cache: a ray's intervals are
// 8 KB at 1024 samples); sigma once or never; the first interval and the two totals once per ray -- 12 bytes per sample from
// memory without sigma, 16 with it.  4 bytes are written per sample and output.
__global__ __launch_bounds__(256) void distortion_bwd_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                             const float *__restrict__ sigma,
                                                             const float *__restrict__ weights, const int64_t *__restrict__ packed,
                                                             int n_rays, float t_scale, const float *__restrict__ totals,
                                                             const float *__restrict__ g_loss, int g_stride,
                                                             float *__restrict__ d_weights, float *__restrict__ d_sigma)
{
#pragma clang fp contract(off)
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    if (cnt == 0) return;
    const float g = g_loss[(int64_t)ray * g_stride];
    const float w_tot = totals[2 * ray], m_tot = totals[2 * ray + 1];
    float t_end = 1.f - w_tot;
    if (sigma && d_sigma) {
        float tau = 0.f;
        for (int64_t base = 0; base < cnt; base += 64) {
            const int64_t i = s0 + base + lane;
            if (base + lane < cnt) tau = tau + sigma[i] * (te[i] - ts[i]);
        }
        t_end = expf(-lse::wave_sum(tau));
    }
    const float a0 = ts[s0], b0 = te[s0];
    float carry_w = 0.f, carry_m = 0.f, carry_g = 0.f;
    const int64_t n_chunks = (cnt + 63) / 64;
    for (int64_t ch = n_chunks - 1; ch >= 0; --ch) {
        const int64_t base = ch * 64;
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float a = a0, b = b0, w = 0.f;
        if (valid) { a = ts[i]; b = te[i]; w = weights[i]; }
        const float m = distortion_mid(a, b, a0, b0, t_scale);
        const float wm = w * m;
        const float incl_w = wave_inclusive_sum_rev(w), incl_m = wave_inclusive_sum_rev(wm);
        const float w_gt = wave_exclusive_from_rev(incl_w, lane) + carry_w;      // W_>i
        const float m_gt = wave_exclusive_from_rev(incl_m, lane) + carry_m;      // M_>i
        const float w_lt = (w_tot - w_gt) - w, m_lt = (m_tot - m_gt) - wm;
        const float delta = t_scale * (b - a);
        const float dw = g * (2.f * (m * (w_lt - w_gt) - (m_lt - m_gt)) + (2.f / 3.f) * w * delta);
        if (valid && d_weights) d_weights[i] = dw;
        carry_w = carry_w + __shfl(incl_w, 0, 64);
        carry_m = carry_m + __shfl(incl_m, 0, 64);
        if (d_sigma) {                       // (the same on every lane)
            const float gw = valid ? dw * w : 0.f;
            const float incl_g = wave_inclusive_sum_rev(gw);
            const float sg = wave_exclusive_from_rev(incl_g, lane) + carry_g;    // sum_{i>k} dw_i w_i
            if (valid) d_sigma[i] = (dw * (t_end + w_gt) - sg) * (b - a);
            carry_g = carry_g + __shfl(incl_g, 0, 64);
        }
    }
}

__global__ __launch_bounds__(256) void visibility_kernel(const float *__restrict__ ts, const float *__restrict__ te,
                                                         const float *__restrict__ sigma,
                                                         const int64_t *__restrict__ packed, int n_rays, float eps,
                                                         float alpha_thre, uint8_t *__restrict__ mask,
                                                         int64_t *__restrict__ new_cnts, int from_alpha,
                                                         const float *__restrict__ alpha_cap)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    if (alpha_cap != nullptr) alpha_thre = fminf(alpha_thre, *alpha_cap);      // min(alpha_thre, occs.mean()) without the .item()
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    float carry = 0.f;
    int64_t kept = 0;
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool valid = base + lane < cnt;
        float a = 0.f, b = 0.f, sg = 0.f;
        if (valid) {
            sg = sigma[i];
            if (!from_alpha) { a = ts[i]; b = te[i]; }
        }
        // from_alpha (nerfacc.render_visibility_from_alpha): `sigma` holds opacities; T_k = prod_{i<k} (1 - alpha_i) is
        // formed as exp(-sum -log(1 - alpha_i)) with the same scan, the alpha threshold is tested on the input value itself
        const float sd = from_alpha ? -log1pf(-fminf(sg, 1.f)) : sg * (b - a);
        const float incl = lse::wave_inclusive_sum(sd);
        // exclusive prefix = the inclusive one shifted by a lane, not `incl - sd`: a fully opaque sample (alpha == 1.0f, which
        // sigma * dt > ~17 rounds to) has sd = +inf, and inf - inf = NaN would cull the sample although its own transmittance
        // prod_{i<k} (1 - alpha_i) is finite (nerfacc's exclusive product keeps it); everything behind it gets T = 0
        float excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.f;
        const float T = expf(-(excl + carry));
        const float alpha = from_alpha ? sg : 1.f - expf(-sd);
        bool vis = valid && (T >= eps);
        if (alpha_thre > 0.f) vis = vis && (alpha >= alpha_thre);
        if (valid) mask[i] = vis ? 1 : 0;
        kept += __popcll(__ballot(vis));
        carry += __shfl(incl, 63, 64);
    }
    if (lane == 0 && new_cnts) new_cnts[ray] = kept;
}

__global__ __launch_bounds__(256) void compact_kernel(const uint8_t *__restrict__ mask, const int64_t *__restrict__ packed,
                                                      const int64_t *__restrict__ new_packed, int n_rays,
                                                      const int32_t *__restrict__ ri, const float *__restrict__ ts,
                                                      const float *__restrict__ te, int32_t *__restrict__ o_ri,
                                                      float *__restrict__ o_ts, float *__restrict__ o_te)
{
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    int64_t dst = new_packed[2 * ray];
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool keep = (base + lane < cnt) && mask[i];
        const unsigned long long bal = __ballot(keep);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (keep) {
            o_ri[dst + before] = ri[i];
            o_ts[dst + before] = ts[i];
            o_te[dst + before] = te[i];
        }
        dst += __popcll(bal);
    }
}

// The visibility pre-pass has already encoded every candidate sample (unit-cube position, selector, hash features); the
// survivors of the culling keep theirs instead of being encoded a second time by the main pass: same per-ray ballot /
// popcount compaction as compact_kernel, applied to x01[N,3], selector[N] and the level-major features y[L][N][2]
// (a wave's 64 lanes read 512 contiguous bytes per level).  256 B moved per survivor against 1024 B gathered by a re-encode.
__global__ __launch_bounds__(256) void compact_features_kernel(const uint8_t *__restrict__ mask, const int64_t *__restrict__ packed,
                                                               const int64_t *__restrict__ new_packed, int n_rays,
                                                               const float *__restrict__ x01, const uint8_t *__restrict__ sel,
                                                               const float2 *__restrict__ y, int n_levels, int64_t n_old,
                                                               int64_t n_new, float *__restrict__ o_x01,
                                                               uint8_t *__restrict__ o_sel, float2 *__restrict__ o_y)
{
    // blockIdx.y = level group: one wave per (ray, group of levels).  A wave per RAY alone is 3.4 waves per SIMD at 3510 rays, each
    // walking its ray's candidates 64 at a time with dependent trips to memory -- latency-bound at 3.4 TB/s; with the levels split over
    // gridDim.y groups (every group recomputes the cheap ballot / popcount positions; group 0 also moves x01 and the selector) the
    // same bytes move with gridDim.y times the waves in flight.
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= n_rays) return;
    const int lane = threadIdx.x & 63;
    const int per = (n_levels + (int)gridDim.y - 1) / (int)gridDim.y;
    const int l_lo = (int)blockIdx.y * per, l_hi = min(n_levels, l_lo + per);
    const bool first = blockIdx.y == 0;
    const int64_t s0 = packed[2 * ray], cnt = packed[2 * ray + 1];
    int64_t dst = new_packed[2 * ray];
    for (int64_t base = 0; base < cnt; base += 64) {
        const int64_t i = s0 + base + lane;
        const bool keep = (base + lane < cnt) && mask[i];
        const unsigned long long bal = __ballot(keep);
        const int64_t o = dst + __popcll(bal & ((1ull << lane) - 1ull));
        if (keep) {
            if (first) {
                o_x01[o * 3 + 0] = x01[i * 3 + 0];
                o_x01[o * 3 + 1] = x01[i * 3 + 1];
                o_x01[o * 3 + 2] = x01[i * 3 + 2];
                o_sel[o] = sel[i];
            }
            int l = l_lo;
            for (; l + 4 <= l_hi; l += 4) {        // 4 independent loads in flight, then 4 stores
                float2 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = y[(int64_t)(l + u) * n_old + i];
#pragma unroll
                for (int u = 0; u < 4; ++u) o_y[(int64_t)(l + u) * n_new + o] = v[u];
            }
            for (; l < l_hi; ++l) o_y[(int64_t)l * n_new + o] = y[(int64_t)l * n_old + i];
        }
        dst += __popcll(bal);
    }
}

}  // namespace

extern "C" int lse_compact_features(const uint8_t *mask, const int64_t *packed_info, const int64_t *new_packed_info,
                                    int32_t n_rays, const float *x01, const uint8_t *selector, const float *y,
                                    int32_t n_levels, int64_t n_old, int64_t n_new, float *out_x01,
                                    uint8_t *out_selector, float *out_y, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0 && n_old >= 0 && n_new >= 0 && n_levels >= 1, "lse_compact_features: bad sizes");
    if (n_rays == 0 || n_new == 0) return LSE_OK;
    LSE_REQUIRE(mask && packed_info && new_packed_info && x01 && selector && y && out_x01 && out_selector && out_y,
                "lse_compact_features: null pointer");
    const int groups = (int)std::min<int64_t>(std::max<int64_t>(lse::option("compact_features_groups"), 1), n_levels);
    hipLaunchKernelGGL(compact_features_kernel, dim3((n_rays + 3) / 4, groups), dim3(256), 0, lse::as_stream(stream), mask, packed_info,
                       new_packed_info, n_rays, x01, selector, reinterpret_cast<const float2 *>(y), n_levels, n_old, n_new,
                       out_x01, out_selector, reinterpret_cast<float2 *>(out_y));
    return lse::check_launch("lse_compact_features");
}

extern "C" int lse_volrend_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                               int32_t rgb_stride, const int64_t *packed_info, int32_t n_rays, float *weights,
                               float *out_rgb, float *out_acc, float *out_depth_num, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_volrend_fwd: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && weights, "lse_volrend_fwd: null pointer");
    LSE_REQUIRE(!rgb || rgb_stride >= 3, "lse_volrend_fwd: rgb_stride < 3");
    hipLaunchKernelGGL(volrend_fwd_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, rgb, rgb_stride, packed_info, n_rays, weights, out_rgb, out_acc, out_depth_num,
                       (float *)nullptr, (float *)nullptr, (float *)nullptr);
    return lse::check_launch("lse_volrend_fwd");
}

extern "C" int lse_volrend_depth_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                                     int32_t rgb_stride, const int64_t *packed_info, int32_t n_rays, float *weights,
                                     float *out_rgb, float *out_acc, float *out_depth_num, float *mid_range /*[R,2]*/,
                                     float *out_depth, float *depth_range /*[2]*/, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_volrend_depth_fwd: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && weights && out_acc && out_depth_num && mid_range && out_depth,
                "lse_volrend_depth_fwd: null pointer");
    LSE_REQUIRE(!rgb || rgb_stride >= 3, "lse_volrend_depth_fwd: rgb_stride < 3");
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(volrend_fwd_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, st, t_starts, t_ends, sigmas, rgb,
                       rgb_stride, packed_info, n_rays, weights, out_rgb, out_acc, out_depth_num, (float *)nullptr,
                       (float *)nullptr, mid_range);
    hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(1024), 0, st, out_depth_num, out_acc, mid_range, n_rays,
                       out_depth, depth_range);
    return lse::check_launch("lse_volrend_depth_fwd");
}

extern "C" int lse_eval_composite(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                                  int32_t rgb_stride, const int64_t *packed_info, int32_t n_rays, int32_t flags, float background,
                                  float *workspace, float *out_rgb, float *out_acc, float *out_depth, int64_t *out_nsamples,
                                  lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_eval_composite: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && rgb && packed_info && workspace && out_rgb && out_acc && out_depth && out_nsamples,
                "lse_eval_composite: null pointer");
    LSE_REQUIRE(rgb_stride >= 3, "lse_eval_composite: rgb_stride < 3");
    LSE_REQUIRE((flags & ~(LSE_EVAL_NAN_TO_NUM | LSE_EVAL_BACKGROUND | LSE_EVAL_CLAMP)) == 0, "lse_eval_composite: unknown flags %d",
                flags);
    hipStream_t st = lse::as_stream(stream);
    float *mid_range = workspace, *num = workspace + 2 * (int64_t)n_rays;
    hipLaunchKernelGGL(eval_composite_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, st, t_starts, t_ends, sigmas, rgb, rgb_stride,
                       packed_info, n_rays, flags, background, mid_range, num, out_rgb, out_acc, out_nsamples);
    hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(1024), 0, st, (const float *)num, (const float *)out_acc,
                       (const float *)mid_range, n_rays, out_depth, (float *)nullptr);
    return lse::check_launch("lse_eval_composite");
}

extern "C" int lse_eval_composite_normals(const float *t_starts, const float *t_ends, const float *sigmas, const float *d_x01,
                                          const int64_t *packed_info, int32_t n_rays, const float *rays_o, const float *rays_d,
                                          int32_t contraction, const float *h_aabb, int32_t flags, float *out_normals,
                                          lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_eval_composite_normals: n_rays < 0");
    LSE_REQUIRE((flags & ~(LSE_NORMALS_WORLD | LSE_NORMALS_RENORMALIZE)) == 0, "lse_eval_composite_normals: unknown flags %d", flags);
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && d_x01 && packed_info && out_normals, "lse_eval_composite_normals: null pointer");
    Box box;
    for (int k = 0; k < 3; ++k) { box.lo[k] = h_aabb ? h_aabb[k] : -1.f; box.hi[k] = h_aabb ? h_aabb[3 + k] : 1.f; }
    if (flags & LSE_NORMALS_WORLD) {
        LSE_REQUIRE(rays_o && rays_d, "lse_eval_composite_normals: world space needs rays_o and rays_d");
        LSE_REQUIRE(contraction || h_aabb, "lse_eval_composite_normals: aabb normalisation needs h_aabb");
    }
    hipLaunchKernelGGL(eval_composite_normals_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, d_x01, packed_info, n_rays, rays_o, rays_d, contraction, box, flags, out_normals);
    return lse::check_launch("lse_eval_composite_normals");
}

extern "C" int lse_eval_segment_state_bytes(int32_t n_rays, int64_t *h_bytes)
{
    LSE_REQUIRE(n_rays >= 0 && h_bytes, "lse_eval_segment_state_bytes: n_rays < 0 or null pointer");
    *h_bytes = (int64_t)n_rays * kSegStateFloats * (int64_t)sizeof(float);
    return LSE_OK;
}

extern "C" int lse_eval_segment_begin(const int64_t *ray_cnts, int32_t n_rays, int64_t first_len, void *state, int64_t *seg_cnts,
                                      lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_eval_segment_begin: n_rays < 0");
    LSE_REQUIRE(first_len >= 1, "lse_eval_segment_begin: first_len < 1");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(ray_cnts && state && seg_cnts, "lse_eval_segment_begin: null pointer");
    LSE_REQUIRE(((uintptr_t)state & 15) == 0, "lse_eval_segment_begin: state is not 16-byte aligned");
    hipLaunchKernelGGL(eval_segment_begin_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), ray_cnts, n_rays,
                       first_len, static_cast<float *>(state), seg_cnts);
    return lse::check_launch("lse_eval_segment_begin");
}

extern "C" int lse_eval_composite_segment(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                                          int32_t rgb_stride, const int64_t *seg_packed, const int64_t *ray_cnts, int32_t n_rays,
                                          int32_t flags, int64_t seg_end, int64_t next_len, float tau_stop, void *state,
                                          int64_t *next_seg_cnts, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_eval_composite_segment: n_rays < 0");
    LSE_REQUIRE(seg_end >= 1 && next_len >= 0, "lse_eval_composite_segment: seg_end < 1 or next_len < 0");
    LSE_REQUIRE(next_len == 0 || (seg_end & 63) == 0,
                "lse_eval_composite_segment: seg_end %lld is not a multiple of 64 and a segment follows (next_len %lld)",
                (long long)seg_end, (long long)next_len);
    LSE_REQUIRE((flags & ~(LSE_EVAL_NAN_TO_NUM | LSE_EVAL_BACKGROUND | LSE_EVAL_CLAMP)) == 0,
                "lse_eval_composite_segment: unknown flags %d", flags);
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && rgb && seg_packed && ray_cnts && state, "lse_eval_composite_segment: null pointer");
    LSE_REQUIRE(next_len == 0 || next_seg_cnts, "lse_eval_composite_segment: null pointer (next_seg_cnts with a segment to follow)");
    LSE_REQUIRE(rgb_stride >= 3, "lse_eval_composite_segment: rgb_stride < 3");
    LSE_REQUIRE(((uintptr_t)state & 15) == 0, "lse_eval_composite_segment: state is not 16-byte aligned");
    hipLaunchKernelGGL(eval_composite_segment_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, rgb, rgb_stride, seg_packed, ray_cnts, n_rays, flags, seg_end, next_len, tau_stop,
                       static_cast<float *>(state), next_seg_cnts);
    return lse::check_launch("lse_eval_composite_segment");
}

extern "C" int lse_eval_composite_finish(const void *state, int32_t n_rays, int32_t flags, float background, float *workspace,
                                         float *out_rgb, float *out_acc, float *out_depth, int64_t *out_nsamples,
                                         lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_eval_composite_finish: n_rays < 0");
    LSE_REQUIRE((flags & ~(LSE_EVAL_NAN_TO_NUM | LSE_EVAL_BACKGROUND | LSE_EVAL_CLAMP)) == 0,
                "lse_eval_composite_finish: unknown flags %d", flags);
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(state && workspace && out_rgb && out_acc && out_depth && out_nsamples, "lse_eval_composite_finish: null pointer");
    LSE_REQUIRE(((uintptr_t)state & 15) == 0, "lse_eval_composite_finish: state is not 16-byte aligned");
    hipStream_t st = lse::as_stream(stream);
    float *mid_range = workspace, *num = workspace + 2 * (int64_t)n_rays;
    hipLaunchKernelGGL(eval_segment_finish_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, st, static_cast<const float *>(state),
                       n_rays, flags, background, mid_range, num, out_rgb, out_acc, out_nsamples);
    hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(1024), 0, st, (const float *)num, (const float *)out_acc,
                       (const float *)mid_range, n_rays, out_depth, (float *)nullptr);
    return lse::check_launch("lse_eval_composite_finish");
}

// the argument checks the two depth-quantile entry points share; fills `tau`
static int depth_quantile_args(const char *who, int32_t n_rays, int32_t n_q, const float *h_tau_q, int32_t flags, float max_spread,
                               DepthTaus &tau)
{
    LSE_REQUIRE(n_rays >= 0, "%s: n_rays < 0", who);
    LSE_REQUIRE(n_q >= 1 && n_q <= 4, "%s: n_q %d outside 1..4", who, n_q);
    LSE_REQUIRE(h_tau_q, "%s: null pointer (tau_q)", who);
    for (int j = 0; j < 4; ++j) tau.v[j] = j < n_q ? h_tau_q[j] : INFINITY;
    LSE_REQUIRE(tau.v[0] > 0.f, "%s: tau_q[0] = %g is not positive", who, (double)tau.v[0]);
    for (int j = 1; j < n_q; ++j)
        LSE_REQUIRE(tau.v[j] > tau.v[j - 1], "%s: tau_q is not ascending (tau_q[%d] = %g after %g)", who, j, (double)tau.v[j],
                    (double)tau.v[j - 1]);
    LSE_REQUIRE((flags & ~(LSE_DEPTH_INTERPOLATE | (3 << 8))) == 0, "%s: unknown flags %d", who, flags);
    LSE_REQUIRE(((flags >> 8) & 3) < n_q, "%s: selected quantile %d of %d", who, (flags >> 8) & 3, n_q);
    LSE_REQUIRE(max_spread >= 0.f, "%s: max_spread %g is negative or NaN", who, (double)max_spread);
    return LSE_OK;
}

extern "C" int lse_eval_depth_quantiles(const float *t_starts, const float *t_ends, const float *sigmas, const int64_t *packed_info,
                                        int32_t n_rays, int32_t n_q, const float *h_tau_q, int32_t flags, float max_spread,
                                        float *depth_q, uint8_t *reached, float *depth_sel, lse_stream_t stream)
{
    DepthTaus tau;
    if (int rc = depth_quantile_args("lse_eval_depth_quantiles", n_rays, n_q, h_tau_q, flags, max_spread, tau)) return rc;
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && depth_q && reached, "lse_eval_depth_quantiles: null pointer");
    hipLaunchKernelGGL(eval_depth_quantiles_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, packed_info, n_rays, tau, n_q, flags, max_spread, depth_q, reached, depth_sel);
    return lse::check_launch("lse_eval_depth_quantiles");
}

extern "C" int lse_eval_depth_quantiles_segment(const float *t_starts, const float *t_ends, const float *sigmas,
                                                const int64_t *seg_packed, int32_t n_rays, int32_t n_q, const float *h_tau_q,
                                                int32_t flags, float max_spread, void *state, float *depth_q, uint8_t *reached,
                                                float *depth_sel, lse_stream_t stream)
{
    DepthTaus tau;
    if (int rc = depth_quantile_args("lse_eval_depth_quantiles_segment", n_rays, n_q, h_tau_q, flags, max_spread, tau)) return rc;
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && seg_packed && state && depth_q && reached,
                "lse_eval_depth_quantiles_segment: null pointer");
    LSE_REQUIRE(((uintptr_t)state & 3) == 0, "lse_eval_depth_quantiles_segment: state is not 4-byte aligned");
    hipLaunchKernelGGL(eval_depth_quantiles_segment_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts,
                       t_ends, sigmas, seg_packed, n_rays, tau, n_q, flags, max_spread, static_cast<float *>(state), depth_q, reached,
                       depth_sel);
    return lse::check_launch("lse_eval_depth_quantiles_segment");
}

extern "C" int lse_render_weight_fwd(const float *t_starts, const float *t_ends, const float *sigmas,
                                     const int64_t *packed_info, int32_t n_rays, float *weights, float *trans,
                                     float *alphas, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_render_weight_fwd: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && weights, "lse_render_weight_fwd: null pointer");
    hipLaunchKernelGGL(volrend_fwd_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, (const float *)nullptr, 0, packed_info, n_rays, weights, (float *)nullptr, (float *)nullptr,
                       (float *)nullptr, trans, alphas, (float *)nullptr);
    return lse::check_launch("lse_render_weight_fwd");
}

extern "C" int lse_render_weight_bwd(const float *t_starts, const float *t_ends, const float *sigmas,
                                     const int64_t *packed_info, int32_t n_rays, const float *weights,
                                     const float *d_weights, float *d_sigmas, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_render_weight_bwd: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && weights && d_weights && d_sigmas,
                "lse_render_weight_bwd: null pointer");
    hipLaunchKernelGGL(volrend_bwd_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, (const float *)nullptr, 0, packed_info, n_rays, weights, (const float *)nullptr,
                       (const float *)nullptr, (const float *)nullptr, d_sigmas, (float *)nullptr, d_weights);
    return lse::check_launch("lse_render_weight_bwd");
}

extern "C" int lse_volrend_bwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                               int32_t rgb_stride, const int64_t *packed_info, int32_t n_rays, const float *weights,
                               const float *d_out_rgb, const float *d_out_acc, const float *d_out_depth_num,
                               float *d_sigmas, float *d_rgb, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_volrend_bwd: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && weights && d_sigmas, "lse_volrend_bwd: null pointer");
    LSE_REQUIRE(!rgb || rgb_stride >= 3, "lse_volrend_bwd: rgb_stride < 3");
    hipLaunchKernelGGL(volrend_bwd_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, rgb, rgb_stride, packed_info, n_rays, weights, d_out_rgb, d_out_acc, d_out_depth_num,
                       d_sigmas, d_rgb, (const float *)nullptr);
    return lse::check_launch("lse_volrend_bwd");
}

extern "C" int lse_distortion_fwd(const float *t_starts, const float *t_ends, const float *weights, const int64_t *packed_info,
                                  int32_t n_rays, float t_scale, float *out_loss, float *out_totals, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_distortion_fwd: n_rays < 0");
    LSE_REQUIRE(t_scale >= 0.f && t_scale < INFINITY, "lse_distortion_fwd: t_scale %g is negative or not finite", (double)t_scale);
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && weights && packed_info && out_loss, "lse_distortion_fwd: null pointer");
    hipLaunchKernelGGL(distortion_fwd_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends, weights,
                       packed_info, n_rays, t_scale, out_loss, out_totals);
    return lse::check_launch("lse_distortion_fwd");
}

extern "C" int lse_distortion_bwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *weights,
                                  const int64_t *packed_info, int32_t n_rays, float t_scale, const float *totals, const float *g_loss,
                                  int32_t g_stride, float *d_weights, float *d_sigmas, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_distortion_bwd: n_rays < 0");
    LSE_REQUIRE(t_scale >= 0.f && t_scale < INFINITY, "lse_distortion_bwd: t_scale %g is negative or not finite", (double)t_scale);
    LSE_REQUIRE(g_stride == 0 || g_stride == 1, "lse_distortion_bwd: g_stride %d is neither 0 nor 1", g_stride);
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && weights && packed_info && totals && g_loss, "lse_distortion_bwd: null pointer");
    LSE_REQUIRE(d_weights || d_sigmas, "lse_distortion_bwd: null pointer (neither d_weights nor d_sigmas)");
    hipLaunchKernelGGL(distortion_bwd_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends, sigmas,
                       weights, packed_info, n_rays, t_scale, totals, g_loss, g_stride, d_weights, d_sigmas);
    return lse::check_launch("lse_distortion_bwd");
}

extern "C" int lse_visibility_mask(const float *t_starts, const float *t_ends, const float *sigmas,
                                   const int64_t *packed_info, int32_t n_rays, float early_stop_eps, float alpha_thre,
                                   uint8_t *mask, int64_t *new_cnts, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_visibility_mask: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && mask, "lse_visibility_mask: null pointer");
    hipLaunchKernelGGL(visibility_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, packed_info, n_rays, early_stop_eps, alpha_thre, mask, new_cnts, 0, (const float *)nullptr);
    return lse::check_launch("lse_visibility_mask");
}

extern "C" int lse_visibility_mask_cap(const float *t_starts, const float *t_ends, const float *sigmas,
                                       const int64_t *packed_info, int32_t n_rays, float early_stop_eps, float alpha_thre,
                                       const float *alpha_cap, uint8_t *mask, int64_t *new_cnts, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_visibility_mask_cap: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(t_starts && t_ends && sigmas && packed_info && mask && alpha_cap, "lse_visibility_mask_cap: null pointer");
    hipLaunchKernelGGL(visibility_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), t_starts, t_ends,
                       sigmas, packed_info, n_rays, early_stop_eps, alpha_thre, mask, new_cnts, 0, alpha_cap);
    return lse::check_launch("lse_visibility_mask_cap");
}

extern "C" int lse_visibility_mask_alpha(const float *alphas, const int64_t *packed_info, int32_t n_rays,
                                         float early_stop_eps, float alpha_thre, uint8_t *mask, int64_t *new_cnts,
                                         lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_visibility_mask_alpha: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(alphas && packed_info && mask, "lse_visibility_mask_alpha: null pointer");
    hipLaunchKernelGGL(visibility_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream),
                       (const float *)nullptr, (const float *)nullptr, alphas, packed_info, n_rays, early_stop_eps,
                       alpha_thre, mask, new_cnts, 1, (const float *)nullptr);
    return lse::check_launch("lse_visibility_mask_alpha");
}

extern "C" int lse_compact_samples(const uint8_t *mask, const int64_t *packed_info, const int64_t *new_packed_info,
                                   int32_t n_rays, const int32_t *ray_indices, const float *t_starts,
                                   const float *t_ends, int32_t *out_ray_indices, float *out_t_starts,
                                   float *out_t_ends, lse_stream_t stream)
{
    LSE_REQUIRE(n_rays >= 0, "lse_compact_samples: n_rays < 0");
    if (n_rays == 0) return LSE_OK;
    LSE_REQUIRE(mask && packed_info && new_packed_info && ray_indices && t_starts && t_ends && out_ray_indices &&
                    out_t_starts && out_t_ends, "lse_compact_samples: null pointer");
    hipLaunchKernelGGL(compact_kernel, dim3((n_rays + 3) / 4), dim3(256), 0, lse::as_stream(stream), mask, packed_info,
                       new_packed_info, n_rays, ray_indices, t_starts, t_ends, out_ray_indices, out_t_starts, out_t_ends);
    return lse::check_launch("lse_compact_samples");
}
