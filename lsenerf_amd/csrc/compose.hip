// Batch composer for gfx950: the data manager's hot loop (R:lse_nerf/lse_datamanager.py:337-372) as device code.
//   compose_kernel   one thread per sampled pixel: Philox draw (or given indices), target / mask / id gathers, the rays of
//                    EdCameras.generate_rays (lsenerf_amd/cameras.py, R:lse_nerf/lse_cameras.py:340-586) from a pose table, and the
//                    metadata of add_metadata / CameraIdxFixer (R:lse_nerf/utils.py:153-194, R:lse_nerf/data_components.py:70-90).
//                    A colour pixel writes its G rays, an event pixel one ray into the previous and one into the next bundle.
//   camera_rays_kernel  one thread per pixel of a row-major pixel range of ONE camera (the eval set's whole images): the same ray
//                    device functions, so its rays are bit-equal to the composer's for the same (pose, y, x).
//   advance_kernel   one thread: *step += 1, in stream order behind the composer (so the counter is part of a replayed graph).
//   rays_bwd_kernel  d origins / d directions -> d pose table.  One wave per table row: every lane walks the rays of the row's
//                    bundle(s) with stride 64, keeps the contributions of the rays that read this row in ray order, then a
//                    fixed butterfly joins the 64 partial sums -- no atomics, two runs are bit-equal.
// Both are latency-bound launches of a few thousand threads.  This file is compiled with -ffp-contract=off: the ray arithmetic
// restates the torch expressions operation by operation, and the targets are stated as single roundings.
#include "common.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;

using lse::load_pix;
using lse::philox4x32_10;
using lse::U4;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// radial_and_tangential_undistort of lsenerf_amd/cameras.py: 10 Newton steps from the distorted point, a step is skipped where
// |det| <= 1e-3
__device__ __forceinline__ void undistort(const float *k, float xd, float yd, float *xo, float *yo)
{
    const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3], p1 = k[4], p2 = k[5];
    float x = xd, y = yd;
    for (int it = 0; it < 10; ++it) {
        const float r = x * x + y * y;
        const float d = 1.0f + r * (k1 + r * (k2 + r * (k3 + r * k4)));
        const float fx = d * x + 2.f * p1 * x * y + p2 * (r + 2.f * x * x) - xd;
        const float fy = d * y + 2.f * p2 * x * y + p1 * (r + 2.f * y * y) - yd;
        const float d_r = k1 + r * (2.0f * k2 + r * (3.0f * k3 + r * 4.0f * k4));
        const float d_x = 2.0f * x * d_r, d_y = 2.0f * y * d_r;
        const float fx_x = d + d_x * x + 2.0f * p1 * y + 6.0f * p2 * x;
        const float fx_y = d_y * x + 2.0f * p1 * x + 2.0f * p2 * y;
        const float fy_x = d_x * y + 2.0f * p2 * y + 2.0f * p1 * x;
        const float fy_y = d + d_y * y + 2.0f * p2 * x + 6.0f * p1 * y;
        const float det = fy_x * fx_y - fx_x * fy_y;
        if (fabsf(det) > 1e-3f) {
            const float sx = (fx * fy_y - fy * fx_y) / det;
            const float sy = (fy * fx_x - fx * fy_x) / det;
            x = x + sx;
            y = y + sy;
        }
    }
    *xo = x;
    *yo = y;
}

// camera-frame point of pixel (px, py): ((x - cx) / fx, -(y - cy) / fy), undistorted
__device__ __forceinline__ void cam_point(const lse_compose_stream &s, float px, float py, float *xo, float *yo)
{
    const float xc = (px - s.cx) / s.fx;
    const float yc = -(py - s.cy) / s.fy;
    if (s.distort)
        undistort(s.dist, xc, yc, xo, yo);
    else {
        *xo = xc;
        *yo = yc;
    }
}

// world = R (x, y, -1), summed in column order like torch.sum(stack[..., None, :] * c2w[:, :3, :3], -1)
__device__ __forceinline__ void rotate(const float *__restrict__ pose, float x, float y, float w[3])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) w[i] = (x * pose[4 * i] + y * pose[4 * i + 1]) + (-1.0f) * pose[4 * i + 2];
}

__device__ __forceinline__ float norm3(const float w[3]) { return sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]); }

struct Pts {
    float x0, y0, x1, y1, x2, y2;    // (x, y), (x + 1, y), (x, y + 1) in the camera frame
};

__device__ __forceinline__ Pts pixel_points(const lse_compose_stream &s, int y, int x)
{
    Pts p;
    const float fx = (float)x, fy = (float)y;
    cam_point(s, fx, fy, &p.x0, &p.y0);
    cam_point(s, fx + 1.0f, fy, &p.x1, &p.y1);
    cam_point(s, fx, fy + 1.0f, &p.x2, &p.y2);
    return p;
}

// one ray of one pixel through the pose at `pose` into row `row`
__device__ __forceinline__ void write_ray(const lse_compose_out &o, int64_t row, const float *__restrict__ pose, const Pts &p)
{
    float w0[3], w1[3], w2[3];
    rotate(pose, p.x0, p.y0, w0);
    rotate(pose, p.x1, p.y1, w1);
    rotate(pose, p.x2, p.y2, w2);
    const float n0 = norm3(w0), n1 = norm3(w1), n2 = norm3(w2);
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        w0[i] = w0[i] / n0;
        const float a = w0[i] - w1[i] / n1, b = w0[i] - w2[i] / n2;
        sx = i == 0 ? a * a : sx + a * a;
        sy = i == 0 ? b * b : sy + b * b;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.origins[3 * row + i] = pose[4 * i + 3];
        o.directions[3 * row + i] = w0[i];
    }
    o.pixel_area[row] = sqrtf(sx) * sqrtf(sy);
    o.directions_norm[row] = n0;
}

__global__ __launch_bounds__(kThreads) void compose_kernel(lse_compose_desc D, lse_compose_scene S, lse_compose_out O,
                                                           const int64_t *__restrict__ step_dev, int64_t step_arg,
                                                           const int32_t *__restrict__ col_in, const int32_t *__restrict__ evs_in)
{
    const int t = blockIdx.x * kThreads + threadIdx.x;
    const int n_col = D.col.n_pixels, n_evs = D.evs.n_pixels;
    if (t >= n_col + n_evs) return;
    const bool is_evs = t >= n_col;
    const int i = is_evs ? t - n_col : t;
    const lse_compose_stream &s = is_evs ? D.evs : D.col;
    const int32_t *given = is_evs ? evs_in : col_in;
    int c, y, x;
    if (given != nullptr) {
        c = clampi(given[3 * i], 0, s.n_images - 1);
        y = clampi(given[3 * i + 1], 0, s.H - 1);
        x = clampi(given[3 * i + 2], 0, s.W - 1);
    } else {
        const int64_t step = step_dev != nullptr ? *step_dev : step_arg;
        const U4 r = philox4x32_10(U4{(uint32_t)step, (uint32_t)i, is_evs ? 1u : 0u, 0u}, (uint32_t)D.seed, (uint32_t)(D.seed >> 32));
        c = (int)__umulhi(r.x, (uint32_t)s.n_images);
        y = (int)__umulhi(r.y, (uint32_t)s.H);
        x = (int)__umulhi(r.z, (uint32_t)s.W);
    }
    const int64_t pix = ((int64_t)c * s.H + y) * s.W + x;
    const Pts p = pixel_points(s, y, x);
    if (!is_evs) {
        const int cam = clampi(S.col_image_idx[c], 0, s.n_cameras - 1);
        const int G = D.G;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) O.col_image[3 * i + ch] = (float)S.col_images[3 * pix + ch] / 255.0f;
        if (O.col_msk != nullptr) O.col_msk[i] = load_pix(S.col_msk, s.msk_type, pix);
        const int app = S.col_appearance_id[c];
        O.col_batch_appearance_id[i] = app;
        O.col_indices[3 * i] = cam;
        O.col_indices[3 * i + 1] = y;
        O.col_indices[3 * i + 2] = x;
        const float time = S.col_times[cam];
        for (int k = 0; k < G; ++k) {
            const int64_t row = (int64_t)O.row_col + (int64_t)i * G + k;
            const int slot = cam * G + k;
            write_ray(O, row, S.col_pose + 12 * (int64_t)slot, p);
            O.times[row] = time;
            O.camera_indices[row] = cam;
            O.appearance_id[row] = G > 1 ? clampi(app + (k - G / 2), 0, D.num_embd - 1) : app;
            O.cam_type[row] = 0;
            O.ray_px[3 * row] = slot;
            O.ray_px[3 * row + 1] = y;
            O.ray_px[3 * row + 2] = x;
            // fix_datashape tiles the pixel list: block k of the colour rows is the whole list again
            const int64_t crow = (int64_t)O.row_col + (int64_t)k * n_col + i;
            O.coords[3 * crow] = cam;
            O.coords[3 * crow + 1] = y;
            O.coords[3 * crow + 2] = x;
        }
        return;
    }
    const int off = D.consecutive ? 1 : 0;
    const int cam = clampi(S.evs_image_idx[c], 0, s.n_cameras - 1 - off);
    O.evs_image[i] = load_pix(S.evs_images, s.pix_type, pix) * D.e_scale;
    if (O.evs_msk != nullptr) O.evs_msk[i] = load_pix(S.evs_msk, s.msk_type, pix);
    O.evs_e_thresh[i] = D.e_thresh;
    const int app = S.evs_appearance_id[c];
    O.evs_batch_appearance_id[i] = app;
    O.evs_indices[3 * i] = cam;
    O.evs_indices[3 * i + 1] = y;
    O.evs_indices[3 * i + 2] = x;
#pragma unroll
    for (int side = 0; side < 2; ++side) {
        const int64_t row = (int64_t)(side ? O.row_next : O.row_prev) + i;
        const int slot = side ? cam + off : cam;
        write_ray(O, row, (side ? S.next_pose : S.prev_pose) + 12 * (int64_t)slot, p);
        O.times[row] = (side ? S.next_times : S.prev_times)[slot];
        O.camera_indices[row] = (side ? S.next_closest : S.prev_closest)[slot];
        O.appearance_id[row] = app;
        O.cam_type[row] = 1;
        O.ray_px[3 * row] = slot;
        O.ray_px[3 * row + 1] = y;
        O.ray_px[3 * row + 2] = x;
        O.coords[3 * row] = cam;
        O.coords[3 * row + 1] = y;
        O.coords[3 * row + 2] = x;
    }
}

// the rays of the row-major pixels [first, first + n) of one camera: compose_kernel's ray arithmetic (pixel_points, write_ray) with the
// pixel taken from the thread index instead of a draw, so a ray is bit-equal to what the composer writes for the same (pose, y, x)
__global__ __launch_bounds__(kThreads) void camera_rays_kernel(lse_compose_stream s, lse_compose_out O, const float *__restrict__ pose,
                                                               int64_t first, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t pix = first + i;
    const int y = (int)(pix / s.W);
    const int x = (int)(pix - (int64_t)y * s.W);
    write_ray(O, i, pose, pixel_points(s, y, x));
}

__global__ void advance_kernel(int64_t *step)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *step = *step + 1;
}

// the 12 entries of d pose[3, 4] of one ray:  d = w / |w|, w = R p  ->  dL/dw = (g_d - d (d . g_d)) / |w|,  dL/dR = dL/dw p^T,  dL/dt = g_o
__device__ __forceinline__ void ray_pose_grad(const lse_compose_stream &s, const float *__restrict__ pose, int y, int x,
                                              const float *__restrict__ g_o, const float *__restrict__ g_d, float acc[12])
{
    float px, py;
    cam_point(s, (float)x, (float)y, &px, &py);
    float w[3];
    rotate(pose, px, py, w);
    const float n = norm3(w);
    const float d0 = w[0] / n, d1 = w[1] / n, d2 = w[2] / n;
    const float dot = (d0 * g_d[0] + d1 * g_d[1]) + d2 * g_d[2];
    const float gw[3] = {(g_d[0] - d0 * dot) / n, (g_d[1] - d1 * dot) / n, (g_d[2] - d2 * dot) / n};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        acc[4 * i] += gw[i] * px;
        acc[4 * i + 1] += gw[i] * py;
        acc[4 * i + 2] += -gw[i];
        acc[4 * i + 3] += g_o[i];
    }
}

// one wave per table row.  Rows: [col table: col.n_cameras * G | prev table: evs.n_cameras | next table: evs.n_cameras (absent
// when consecutive)]
__global__ __launch_bounds__(kThreads) void rays_bwd_kernel(lse_compose_desc D, lse_compose_scene S, lse_compose_out O,
                                                            const float *__restrict__ d_o, const float *__restrict__ d_d,
                                                            float *__restrict__ g_col, float *__restrict__ g_prev,
                                                            float *__restrict__ g_next, int n_col_rows, int n_evs_rows, int total)
{
    const int wave = (blockIdx.x * kThreads + threadIdx.x) >> 6;
    if (wave >= total) return;                  // (whole waves leave together: `wave` is wave-uniform)
    const int lane = lse::lane_id();
    int table, slot;
    if (wave < n_col_rows) { table = 0; slot = wave; }
    else if (wave < n_col_rows + n_evs_rows) { table = 1; slot = wave - n_col_rows; }
    else { table = 2; slot = wave - n_col_rows - n_evs_rows; }
    const lse_compose_stream &s = table == 0 ? D.col : D.evs;
    const float *pose = (table == 0 ? S.col_pose : (table == 1 ? S.prev_pose : S.next_pose)) + 12 * (int64_t)slot;
    float *dst = (table == 0 ? g_col : (table == 1 ? g_prev : g_next)) + 12 * (int64_t)slot;
    float acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.f;
    // the ray blocks that index this table: colour rays; prev rays; next rays (the prev table too when consecutive)
    const int n_evs = D.evs.n_pixels;
    const int64_t lo[2] = {table == 0 ? O.row_col : (table == 1 ? O.row_prev : O.row_next), O.row_next};
    const int len[2] = {table == 0 ? D.col.n_pixels * D.G : n_evs, (table == 1 && D.consecutive) ? n_evs : 0};
    for (int b = 0; b < 2; ++b)
        for (int r = lane; r < len[b]; r += 64) {
            const int64_t row = lo[b] + r;
            if (O.ray_px[3 * row] != slot) continue;
            ray_pose_grad(s, pose, O.ray_px[3 * row + 1], O.ray_px[3 * row + 2], d_o + 3 * row, d_d + 3 * row, acc);
        }
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = lse::wave_sum(acc[q]);
    if (lane < 12) {
        float v = acc[0];
#pragma unroll
        for (int q = 1; q < 12; ++q) v = lane == q ? acc[q] : v;
        dst[lane] = v;
    }
}

int check_stream(const lse_compose_stream &s, const char *what, const char *name)
{
    LSE_REQUIRE(s.n_pixels >= 0, "%s: %s.n_pixels < 0", what, name);
    if (s.n_pixels == 0) return LSE_OK;
    LSE_REQUIRE(s.H >= 1 && s.W >= 1 && s.n_images >= 1 && s.n_cameras >= 1, "%s: %s needs H, W, n_images, n_cameras >= 1", what, name);
    LSE_REQUIRE(s.fx != 0.f && s.fy != 0.f, "%s: %s has a zero focal length", what, name);
    LSE_REQUIRE(s.pix_type >= LSE_PIX_I8 && s.pix_type <= LSE_PIX_F32, "%s: %s.pix_type %d", what, name, s.pix_type);
    LSE_REQUIRE(s.msk_type == LSE_PIX_NONE || s.msk_type == LSE_PIX_U8 || s.msk_type == LSE_PIX_F32, "%s: %s.msk_type %d", what, name,
                s.msk_type);
    return LSE_OK;
}

int check_common(const lse_compose_desc *d, const lse_compose_scene *s, const lse_compose_out *o, const char *what)
{
    LSE_REQUIRE(d && s && o, "%s: null descriptor", what);
    int rc = check_stream(d->col, what, "col");
    if (rc != LSE_OK) return rc;
    rc = check_stream(d->evs, what, "evs");
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(d->col.n_pixels + d->evs.n_pixels > 0, "%s: no pixels", what);
    LSE_REQUIRE(d->G == 1 || d->G == 4, "%s: G must be 1 or 4 (got %d)", what, d->G);
    LSE_REQUIRE(d->G == 1 || d->num_embd >= 1, "%s: num_embd must be >= 1 with G = 4", what);
    const int64_t n_col = (int64_t)d->col.n_pixels * d->G, n_evs = d->evs.n_pixels;
    LSE_REQUIRE(o->n_rows >= 1 && o->row_col >= 0 && o->row_prev >= 0 && o->row_next >= 0, "%s: negative row offset", what);
    LSE_REQUIRE(o->row_col + n_col <= o->n_rows && o->row_prev + n_evs <= o->n_rows && o->row_next + n_evs <= o->n_rows,
                "%s: a bundle's row block leaves the %d rows of the buffers", what, o->n_rows);
    LSE_REQUIRE(o->ray_px, "%s: null ray_px", what);
    if (d->col.n_pixels > 0) LSE_REQUIRE(s->col_pose, "%s: null colour pose table", what);
    if (d->evs.n_pixels > 0) {
        LSE_REQUIRE(s->prev_pose && (d->consecutive || s->next_pose), "%s: null event pose table", what);
        LSE_REQUIRE(!d->consecutive || d->evs.n_cameras >= 2, "%s: consecutive event cameras need at least two cameras", what);
    }
    return LSE_OK;
}

}  // namespace

extern "C" int lse_compose_batch(const lse_compose_desc *desc, const lse_compose_scene *scene, const lse_compose_out *out,
                                 int64_t *step_dev, int64_t step, int32_t advance, const int32_t *col_indices_in,
                                 const int32_t *evs_indices_in, lse_stream_t stream)
{
    const char *what = "lse_compose_batch";
    const int rc = check_common(desc, scene, out, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(!advance || step_dev, "%s: advance needs step_dev", what);
    LSE_REQUIRE(out->origins && out->directions && out->pixel_area && out->directions_norm && out->times && out->camera_indices &&
                    out->appearance_id && out->cam_type && out->coords, "%s: null per-ray output", what);
    if (desc->col.n_pixels > 0) {
        LSE_REQUIRE(desc->col.pix_type == LSE_PIX_U8, "%s: colour images are uint8", what);
        LSE_REQUIRE(scene->col_images && scene->col_appearance_id && scene->col_image_idx && scene->col_times, "%s: null colour table", what);
        LSE_REQUIRE(out->col_image && out->col_indices && out->col_batch_appearance_id, "%s: null colour batch output", what);
        LSE_REQUIRE((out->col_msk != nullptr) == (desc->col.msk_type != LSE_PIX_NONE) && (!out->col_msk || scene->col_msk),
                    "%s: colour mask pointers and col.msk_type disagree", what);
    }
    if (desc->evs.n_pixels > 0) {
        LSE_REQUIRE(scene->evs_images && scene->evs_appearance_id && scene->evs_image_idx && scene->prev_times && scene->prev_closest,
                    "%s: null event table", what);
        LSE_REQUIRE(desc->consecutive || (scene->next_times && scene->next_closest), "%s: null next-camera table", what);
        LSE_REQUIRE(out->evs_image && out->evs_e_thresh && out->evs_indices && out->evs_batch_appearance_id,
                    "%s: null event batch output", what);
        LSE_REQUIRE((out->evs_msk != nullptr) == (desc->evs.msk_type != LSE_PIX_NONE) && (!out->evs_msk || scene->evs_msk),
                    "%s: event mask pointers and evs.msk_type disagree", what);
    }
    lse_compose_scene S = *scene;
    if (desc->consecutive) {                    // one table, read at camera and camera + 1
        S.next_pose = S.prev_pose;
        S.next_times = S.prev_times;
        S.next_closest = S.prev_closest;
    }
    hipStream_t st = lse::as_stream(stream);
    const int n = desc->col.n_pixels + desc->evs.n_pixels;
    hipLaunchKernelGGL(compose_kernel, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, *desc, S, *out,
                       (const int64_t *)step_dev, step, col_indices_in, evs_indices_in);
    if (advance) hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, st, step_dev);
    return lse::check_launch(what);
}

extern "C" int lse_camera_rays(const lse_camera_desc *cam, const float *pose, int64_t first, int64_t n, float *origins,
                               float *directions, float *pixel_area, float *directions_norm, lse_stream_t stream)
{
    const char *what = "lse_camera_rays";
    LSE_REQUIRE(cam, "%s: null descriptor", what);
    LSE_REQUIRE(cam->H >= 1 && cam->W >= 1, "%s: H and W must be >= 1 (got H=%d, W=%d)", what, cam->H, cam->W);
    const int64_t pixels = (int64_t)cam->H * cam->W;
    LSE_REQUIRE(pixels <= INT32_MAX, "%s: %lld pixels exceed the supported image size", what, (long long)pixels);
    LSE_REQUIRE(cam->fx != 0.f && cam->fy != 0.f, "%s: zero focal length", what);
    LSE_REQUIRE(first >= 0, "%s: first < 0", what);
    LSE_REQUIRE(n >= 0, "%s: n < 0", what);
    LSE_REQUIRE(first <= pixels && n <= pixels - first, "%s: pixels [%lld, %lld) leave the %d x %d image", what, (long long)first,
                (long long)(first + n), cam->H, cam->W);
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(pose, "%s: null pose", what);
    LSE_REQUIRE(origins && directions && pixel_area && directions_norm, "%s: null output", what);
    lse_compose_stream s = {};
    s.fx = cam->fx; s.fy = cam->fy; s.cx = cam->cx; s.cy = cam->cy;
    for (int k = 0; k < 6; ++k) s.dist[k] = cam->dist[k];
    s.H = cam->H; s.W = cam->W;
    s.distort = cam->distort;
    lse_compose_out o = {};
    o.origins = origins; o.directions = directions; o.pixel_area = pixel_area; o.directions_norm = directions_norm;
    hipLaunchKernelGGL(camera_rays_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, lse::as_stream(stream),
                       s, o, pose, first, n);
    return lse::check_launch(what);
}

extern "C" int lse_compose_rays_bwd(const lse_compose_desc *desc, const lse_compose_scene *scene, const lse_compose_out *out,
                                    const float *d_origins, const float *d_directions, float *d_col_pose, float *d_prev_pose,
                                    float *d_next_pose, lse_stream_t stream)
{
    const char *what = "lse_compose_rays_bwd";
    const int rc = check_common(desc, scene, out, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(d_origins && d_directions, "%s: null ray gradient", what);
    const int n_col_rows = desc->col.n_pixels > 0 ? desc->col.n_cameras * desc->G : 0;
    const int n_evs_rows = desc->evs.n_pixels > 0 ? desc->evs.n_cameras : 0;
    LSE_REQUIRE(n_col_rows == 0 || d_col_pose, "%s: null d_col_pose", what);
    LSE_REQUIRE(n_evs_rows == 0 || (d_prev_pose && (desc->consecutive || d_next_pose)), "%s: null event table gradient", what);
    const int total = n_col_rows + n_evs_rows * (desc->consecutive ? 1 : 2);
    const int64_t threads = (int64_t)total * 64;
    hipLaunchKernelGGL(rays_bwd_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                       lse::as_stream(stream), *desc, *scene, *out, d_origins, d_directions, d_col_pose, d_prev_pose, d_next_pose,
                       n_col_rows, n_evs_rows, total);
    return lse::check_launch(what);
}
