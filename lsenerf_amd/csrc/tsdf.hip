// TSDF fusion for gfx950: depth renders of a batch of views folded into a truncated signed distance (and a colour) per lattice
// point, and the fused colours blended at mesh vertices.  The definition is in include/lse_hip.h ("TSDF fusion") and, as numpy, in
// tests/tsdf_ref.py; the kernels restate it operation by operation, hence -ffp-contract=off.
//   integrate_kernel      one thread per lattice point, iz fastest: a wave's state accesses are consecutive float2 / float4 rows.
//                         The state is loaded once, the batch's views are folded in ascending order in registers, the state is stored
//                         once: 16 B (tsdf, weight) + 32 B (colour) per point and LAUNCH, whatever the number of views.  Poses and
//                         camera constants are uniform across the launch; the per-view traffic is the gather of the pixel the point
//                         projects to (neighbouring points hit neighbouring pixels).  A point leaves a view at the first failed test.
//   vertex_colors_kernel  one thread per vertex: 8 float4 gathers around its cell.
// No LDS, no atomics: a point is owned by one thread, so two runs give the same bytes.
#include "compact.h"        // blocks_for

namespace {

#include "positions.h"      // Box
#include "lattice.h"        // Lattice, point_coords, point_position, make_lattice, make_box

constexpr int kThreads = 256;

template <bool COLOR>
__global__ __launch_bounds__(kThreads) void integrate_kernel(float2 *__restrict__ tw, float4 *__restrict__ cw, Lattice L, Box box,
                                                             lse_camera_desc cam, const float *__restrict__ poses, int n_views,
                                                             const float *__restrict__ depth, const float *__restrict__ acc,
                                                             const float *__restrict__ rgb, float truncation, float min_acc,
                                                             int carve, float r2_max)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= L.points) return;
    int i[3];
    point_coords(L, p, i);
    float x[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = point_position(L, box, i, k);
    float2 s = tw[p];                       // (tsdf, weight)
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (COLOR) c = cw[p];                   // (r, g, b, colour weight)
    const int64_t hw = (int64_t)cam.H * cam.W;
    const float fw = (float)cam.W, fh = (float)cam.H;
    for (int j = 0; j < n_views; ++j) {
        const float *__restrict__ M = poses + 12 * (int64_t)j;      // (uniform: scalar loads)
        const float v0 = x[0] - M[3], v1 = x[1] - M[7], v2 = x[2] - M[11];
        const float xc = (v0 * M[0] + v1 * M[4]) + v2 * M[8];
        const float yc = (v0 * M[1] + v1 * M[5]) + v2 * M[9];
        const float zc = (v0 * M[2] + v1 * M[6]) + v2 * M[10];
        const float z = -zc;
        if (!(z > 0.f)) continue;                                   // behind the camera (or NaN)
        float X = xc / z, Y = yc / z;
        if (cam.distort) {
            const float k1 = cam.dist[0], k2 = cam.dist[1], k3 = cam.dist[2], k4 = cam.dist[3], p1 = cam.dist[4], p2 = cam.dist[5];
            const float r = X * X + Y * Y;
            if (!(r <= r2_max)) continue;                           // beyond the image's own radius: the polynomial may fold back
            const float d = 1.0f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
            const float xd = (d * X + ((2.f * p1) * X) * Y) + p2 * (r + (2.f * X) * X);
            const float yd = (d * Y + ((2.f * p2) * X) * Y) + p1 * (r + (2.f * Y) * Y);
            X = xd, Y = yd;
        }
        const float u = rintf(X * cam.fx + cam.cx), v = rintf(cam.cy - Y * cam.fy);
        if (!(u >= 0.f && u < fw && v >= 0.f && v < fh)) continue;  // outside the image (NaN and inf fail): compared in float
        const int64_t pix = (int64_t)j * hw + (int64_t)(int)v * cam.W + (int)u;
        const float dp = depth[pix], a = acc[pix];
        const float dist = sqrtf((v0 * v0 + v1 * v1) + v2 * v2);
        float sdf;
        const bool surface = a >= min_acc;
        if (surface) {
            if (!(dp > 0.f && dp < INFINITY)) continue;             // no usable depth
            sdf = dp - dist;
        } else if (carve) {
            sdf = INFINITY;                                         // the ray sees through: observed empty
        } else {
            continue;
        }
        if (sdf < -truncation) continue;                            // occluded
        const float t = fminf(1.f, sdf / truncation);
        s.x = (s.x * s.y + t) / (s.y + 1.f);
        s.y = s.y + 1.f;
        if (COLOR && surface && sdf <= truncation) {
            const float *__restrict__ q = rgb + 3 * pix;
            c.x = (c.x * c.w + q[0]) / (c.w + 1.f);
            c.y = (c.y * c.w + q[1]) / (c.w + 1.f);
            c.z = (c.z * c.w + q[2]) / (c.w + 1.f);
            c.w = c.w + 1.f;
        }
    }
    tw[p] = s;
    if (COLOR) cw[p] = c;
}

__global__ __launch_bounds__(kThreads) void vertex_colors_kernel(const float4 *__restrict__ cw, Lattice L, Box box,
                                                                 const float *__restrict__ vertices, int64_t n,
                                                                 const int64_t *__restrict__ n_dev, float *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= lse::clamp_count(n, n_dev)) return;
    int cc[3];
    float f[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = ((vertices[j * 3 + k] - box.lo[k]) / (box.hi[k] - box.lo[k])) * (float)L.n[k];
        const float fl = floorf(u);
        cc[k] = fl >= (float)(L.n[k] - 1) ? L.n[k] - 1 : (fl > 0.f ? (int)fl : 0);       // (NaN -> 0)
        f[k] = fminf(fmaxf(u - (float)cc[k], 0.f), 1.f);                                 // (NaN -> 0)
    }
    const int64_t p0 = (int64_t)cc[0] * L.sx + (int64_t)cc[1] * L.sy + cc[2];
    float sum[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
        const float4 c = cw[p0 + dx * L.sx + dy * L.sy + dz];
        const float wt = ((dx ? f[0] : 1.f - f[0]) * (dy ? f[1] : 1.f - f[1])) * (dz ? f[2] : 1.f - f[2]);
        if (c.w > 0.f) {
            sum[0] = sum[0] + wt * c.x;
            sum[1] = sum[1] + wt * c.y;
            sum[2] = sum[2] + wt * c.z;
            wsum = wsum + wt;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out[j * 3 + k] = wsum > 0.f ? sum[k] / wsum : 0.f;
}

}  // namespace

extern "C" int lse_tsdf_integrate(float *tw, float *cw, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi,
                                  const lse_camera_desc *cam, const float *poses, int32_t n_views, const float *depth,
                                  const float *acc, const float *rgb, float truncation, float min_acc, int32_t carve, float r2_max,
                                  lse_stream_t stream)
{
    const char *what = "lse_tsdf_integrate";
    Lattice L;
    LSE_REQUIRE(make_lattice(nx, ny, nz, L), "%s: resolution %d x %d x %d: every count >= 1 and fewer than 2^31 points", what, nx, ny,
                nz);
    LSE_REQUIRE(n_views >= 0, "%s: n_views < 0", what);
    LSE_REQUIRE(truncation > 0.f && truncation < INFINITY, "%s: truncation must be positive and finite", what);
    LSE_REQUIRE(cam && h_lo && h_hi, "%s: null camera or box", what);
    LSE_REQUIRE(cam->fx != 0.f && cam->fy != 0.f, "%s: zero focal length", what);
    LSE_REQUIRE(cam->H >= 1 && cam->W >= 1 && cam->H <= (1 << 24) && cam->W <= (1 << 24) && (int64_t)cam->H * cam->W < (1ll << 31),
                "%s: image %d x %d: H, W in [1, 2^24] and fewer than 2^31 pixels", what, cam->H, cam->W);
    LSE_REQUIRE(tw, "%s: null state", what);
    LSE_REQUIRE(((uintptr_t)tw & 7) == 0 && ((uintptr_t)cw & 15) == 0, "%s: tw must be 8-byte and cw 16-byte aligned", what);
    if (n_views == 0) return LSE_OK;
    LSE_REQUIRE(poses && depth && acc, "%s: null pointer", what);
    const dim3 grid(lse::blocks_for(L.points, kThreads)), block(kThreads);
    hipStream_t st = lse::as_stream(stream);
    const Box box = make_box(h_lo, h_hi);
    if (cw && rgb)
        hipLaunchKernelGGL(integrate_kernel<true>, grid, block, 0, st, reinterpret_cast<float2 *>(tw), reinterpret_cast<float4 *>(cw), L,
                           box, *cam, poses, (int)n_views, depth, acc, rgb, truncation, min_acc, (int)carve, r2_max);
    else
        hipLaunchKernelGGL(integrate_kernel<false>, grid, block, 0, st, reinterpret_cast<float2 *>(tw), (float4 *)nullptr, L, box, *cam,
                           poses, (int)n_views, depth, acc, (const float *)nullptr, truncation, min_acc, (int)carve, r2_max);
    return lse::check_launch(what);
}

extern "C" int lse_tsdf_vertex_colors(const float *cw, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi,
                                      const float *vertices, int64_t n, const int64_t *n_dev, float *out, lse_stream_t stream)
{
    const char *what = "lse_tsdf_vertex_colors";
    Lattice L;
    LSE_REQUIRE(make_lattice(nx, ny, nz, L), "%s: resolution %d x %d x %d: every count >= 1 and fewer than 2^31 points", what, nx, ny,
                nz);
    LSE_REQUIRE(n >= 0, "%s: n < 0", what);
    LSE_REQUIRE(h_lo && h_hi, "%s: null box", what);
    LSE_REQUIRE(cw && ((uintptr_t)cw & 15) == 0, "%s: cw must be a non-null, 16-byte aligned device pointer", what);
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(vertices && out, "%s: null pointer", what);
    hipLaunchKernelGGL(vertex_colors_kernel, dim3(lse::blocks_for(n, kThreads)), dim3(kThreads), 0, lse::as_stream(stream),
                       reinterpret_cast<const float4 *>(cw), L, make_box(h_lo, h_hi), vertices, n, n_dev, out);
    return lse::check_launch(what);
}
