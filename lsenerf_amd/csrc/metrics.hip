// Whole-image metrics for gfx950: SSIM and MSE of two [B,C,H,W] f32 images in three launches, no atomics, no host read-back.
//   torchmetrics structural_similarity_index_measure(preds, target) with the defaults the reference evaluates with
//   (R:lse_nerf/lsenerf.py:206, :512): data_range = max(p.max - p.min, t.max - t.min), C1 = (0.01 R)^2, C2 = (0.03 R)^2, an 11-tap
//   Gaussian window (sigma 1.5) used as its outer product, sigma^2 = E[x^2] - mu^2, mean over B*C and the (H-10) x (W-10) map of
//   "valid" windows (torchmetrics pads by reflection and crops the pad again, so the padding never reaches the mean).
//
//   1. stats_kernel: per-workgroup min / max of both images and the sum of squared differences over every pixel (the MSE);
//   2. ssim_tile_kernel: one workgroup per 16 x 16 output tile of one plane.  Each workgroup first reduces the stats partials to the
//      data range itself (a few hundred values: cheaper than a launch), loads the (16+10)^2 input patch of both images into LDS,
//      runs the horizontal 11-tap pass for the five moments, then the vertical pass, then SSIM per pixel, and leaves the tile's sum;
//   3. metrics_final_kernel: one workgroup sums the tile partials and the squared-difference partials in a fixed order.
// Moments, SSIM and every sum are formed in double (FP64 is full-rate vector arithmetic here): sigma^2 = E[x^2] - mu^2 cancels badly
// in f32 when the data range is small against the values, and the fixed-order sums make the result bit-reproducible.
//
// In front of them, for a whole eval set (lsenerf_amd/eval_set.py):
//   eval_prep_kernel: one launch per image -- resident ground truth (uint8 / 255.0f, a division, or f32) and rendered rgb, times the
//      optional mask, as the two [3, H, W] planes above; optionally the per-workgroup double sums of x, x^2, y, x y of the event-only
//      metric (R:lse_nerf/lse_pipeline.py:149-164): y = log(gray(masked gt) + 1e-6), x = log((pred_r + pred_g) + 1e-6) of the
//      UNMASKED prediction, both formed in double from the float32 pixels (below) -- the reference passes the image dictionary's halves, of which only the ground truth is masked;
//   log_scale_correct_kernel: the reference's correct_img_scale / solve_normal_equations (R:lse_nerf/utils.py:109-135) -- every
//      workgroup sums the partials in the same order, solves y ~ a x + b in double (NaN -> 5/255; a singular system, where the
//      reference's torch.linalg.inv raises, counts as NaN) and writes expf(a x + b) and the grey ground truth as [1, H, W] planes.
// The fit's x and y are double logarithms of double sums: the reference takes them in float32, and where the prediction's spread is
// small against its level (1e-3 of it) float32 logarithms alone move the slope of the exact fit by 5e-3 (the reference's own float32
// normal equations: by 2).  In double the result is the float64 least-squares fit of the float32 images whatever the conditioning.
// expf is the accurate library function; the grey PLANE is float32, its sum written with single roundings (no contraction).
#include "common.h"

namespace {

constexpr int kTile = 16;
constexpr int kWin = 11;
constexpr int kPatch = kTile + kWin - 1;    // 26
constexpr int kStatsThreads = 256;
constexpr int kMaxStatsBlocks = 512;
constexpr int kFinalThreads = 1024;

struct Window {
    float w[kWin];
};

using lse::gray3;
using lse::wave_sum_d;

__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

int stats_blocks(int64_t total)
{
    const int64_t b = (total + 4095) / 4096;
    return (int)std::min<int64_t>(std::max<int64_t>(b, 1), kMaxStatsBlocks);
}

// partials (doubles): [pmin G][pmax G][tmin G][tmax G][sse G]
__global__ __launch_bounds__(kStatsThreads) void stats_kernel(const float *__restrict__ p, const float *__restrict__ t, int64_t total,
                                                              double *__restrict__ part)
{
    __shared__ float s_f[4][kStatsThreads / 64];
    __shared__ double s_d[kStatsThreads / 64];
    float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    double sse = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kStatsThreads;
    for (int64_t i = (int64_t)blockIdx.x * kStatsThreads + threadIdx.x; i < total; i += stride) {
        const float a = p[i], b = t[i];
        pmin = fminf(pmin, a); pmax = fmaxf(pmax, a);
        tmin = fminf(tmin, b); tmax = fmaxf(tmax, b);
        const double d = (double)a - (double)b;
        sse += d * d;
    }
    pmin = wave_min(pmin); pmax = wave_max(pmax); tmin = wave_min(tmin); tmax = wave_max(tmax);
    sse = wave_sum_d(sse);
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_f[0][wv] = pmin; s_f[1][wv] = pmax; s_f[2][wv] = tmin; s_f[3][wv] = tmax; s_d[wv] = sse; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kStatsThreads / 64; ++k) {
            pmin = fminf(pmin, s_f[0][k]); pmax = fmaxf(pmax, s_f[1][k]);
            tmin = fminf(tmin, s_f[2][k]); tmax = fmaxf(tmax, s_f[3][k]);
        }
        double s = s_d[0];
        for (int k = 1; k < kStatsThreads / 64; ++k) s += s_d[k];
        const int G = gridDim.x;
        part[blockIdx.x] = pmin; part[G + blockIdx.x] = pmax;
        part[2 * G + blockIdx.x] = tmin; part[3 * G + blockIdx.x] = tmax;
        part[4 * G + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(256) void ssim_tile_kernel(const float *__restrict__ p, const float *__restrict__ t, int H, int W,
                                                        int tiles_x, int tiles_per_plane, const double *__restrict__ stats, int G,
                                                        Window win, double *__restrict__ tile_sums)
{
    __shared__ float s_red[4][4];
    __shared__ float s_x[kPatch][kPatch], s_y[kPatch][kPatch];
    __shared__ double s_h[5][kPatch][kTile];
    __shared__ double s_sum[4];
    const int tid = threadIdx.x;
    const int wv = tid >> 6;

    // data range from the stats partials (every workgroup reduces the same values in the same order: one R for all)
    float pmin = INFINITY, pmax = -INFINITY, tmin = INFINITY, tmax = -INFINITY;
    for (int k = tid; k < G; k += 256) {
        pmin = fminf(pmin, (float)stats[k]); pmax = fmaxf(pmax, (float)stats[G + k]);
        tmin = fminf(tmin, (float)stats[2 * G + k]); tmax = fmaxf(tmax, (float)stats[3 * G + k]);
    }
    pmin = wave_min(pmin); pmax = wave_max(pmax); tmin = wave_min(tmin); tmax = wave_max(tmax);
    if ((tid & 63) == 0) { s_red[0][wv] = pmin; s_red[1][wv] = pmax; s_red[2][wv] = tmin; s_red[3][wv] = tmax; }

    const int64_t plane = blockIdx.x / tiles_per_plane;
    const int tile = blockIdx.x - (int)(plane * tiles_per_plane);
    const int y0 = (tile / tiles_x) * kTile, x0 = (tile % tiles_x) * kTile;
    const float *pp = p + plane * (int64_t)H * W;
    const float *tp = t + plane * (int64_t)H * W;
    for (int idx = tid; idx < kPatch * kPatch; idx += 256) {
        const int r = idx / kPatch, c = idx - r * kPatch;
        const int gy = y0 + r, gx = x0 + c;
        const bool in = gy < H && gx < W;        // outside the image: feeds only outputs outside the valid map
        s_x[r][c] = in ? pp[(int64_t)gy * W + gx] : 0.f;
        s_y[r][c] = in ? tp[(int64_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    float a0 = s_red[0][0], a1 = s_red[1][0], a2 = s_red[2][0], a3 = s_red[3][0];
    for (int k = 1; k < 4; ++k) {
        a0 = fminf(a0, s_red[0][k]); a1 = fmaxf(a1, s_red[1][k]);
        a2 = fminf(a2, s_red[2][k]); a3 = fmaxf(a3, s_red[3][k]);
    }
    const float range = fmaxf(a1 - a0, a3 - a2);
    const double c1 = (0.01 * range) * (0.01 * range);
    const double c2 = (0.03 * range) * (0.03 * range);

    // horizontal pass: 26 rows x 16 output columns, five moments
    for (int idx = tid; idx < kPatch * kTile; idx += 256) {
        const int r = idx / kTile, c = idx - r * kTile;
        double mx = 0.0, my = 0.0, xx = 0.0, yy = 0.0, xy = 0.0;
#pragma unroll
        for (int k = 0; k < kWin; ++k) {
            const double w = win.w[k];
            const double x = s_x[r][c + k], y = s_y[r][c + k];
            mx += w * x; my += w * y;
            xx += w * (x * x); yy += w * (y * y); xy += w * (x * y);
        }
        s_h[0][r][c] = mx; s_h[1][r][c] = my; s_h[2][r][c] = xx; s_h[3][r][c] = yy; s_h[4][r][c] = xy;
    }
    __syncthreads();
    // vertical pass + SSIM of this thread's output pixel
    const int ty = tid / kTile, tx = tid - ty * kTile;
    double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < kWin; ++k) {
        const double w = win.w[k];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] += w * s_h[q][ty + k][tx];
    }
    double v = 0.0;
    if (y0 + ty < H - (kWin - 1) && x0 + tx < W - (kWin - 1)) {
        const double mu_x2 = m[0] * m[0], mu_y2 = m[1] * m[1], mu_xy = m[0] * m[1];
        const double sxx = m[2] - mu_x2, syy = m[3] - mu_y2, sxy = m[4] - mu_xy;
        v = ((2.0 * mu_xy + c1) * (2.0 * sxy + c2)) / ((mu_x2 + mu_y2 + c1) * (sxx + syy + c2));
    }
    v = wave_sum_d(v);
    if ((tid & 63) == 0) s_sum[wv] = v;
    __syncthreads();
    if (tid == 0) tile_sums[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
}

__global__ __launch_bounds__(kFinalThreads) void metrics_final_kernel(const double *__restrict__ tile_sums, int64_t n_tiles,
                                                                      const double *__restrict__ sse_part, int G, double n_valid,
                                                                      double n_total, float *__restrict__ out_ssim,
                                                                      float *__restrict__ out_mse)
{
    __shared__ double s_a[kFinalThreads / 64], s_b[kFinalThreads / 64];
    double a = 0.0, b = 0.0;
    for (int64_t k = threadIdx.x; k < n_tiles; k += kFinalThreads) a += tile_sums[k];
    for (int k = threadIdx.x; k < G; k += kFinalThreads) b += sse_part[k];
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    if ((threadIdx.x & 63) == 0) { s_a[threadIdx.x >> 6] = a; s_b[threadIdx.x >> 6] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = s_a[0]; b = s_b[0];
        for (int k = 1; k < kFinalThreads / 64; ++k) { a += s_a[k]; b += s_b[k]; }
        *out_ssim = (float)(a / n_valid);
        *out_mse = (float)(b / n_total);
    }
}

// ---- eval images: ground truth + render -> metric planes, and the event-only metric's log-space scale correction ----------------
constexpr int kPrepThreads = 256;

// log of the prediction's R + G (its blue channel zeroed, then summed over the channels), unmasked
__device__ __forceinline__ double log_pred(const float *__restrict__ rgb, int64_t p)
{
    return log(((double)rgb[3 * p] + (double)rgb[3 * p + 1]) + 1e-6);
}

// log of the grey level of a (masked) ground-truth pixel
__device__ __forceinline__ double log_gray(float r, float g, float b)
{
    return log((((double)r * 0.2989 + (double)g * 0.5870) + (double)b * 0.1140) + 1e-6);
}

// partials (doubles): [sum x G][sum x^2 G][sum y G][sum x y G]; part == nullptr: planes only
__global__ __launch_bounds__(kPrepThreads) void eval_prep_kernel(const void *__restrict__ gt, int gt_type, const void *__restrict__ msk,
                                                                 int msk_type, const float *__restrict__ rgb, int64_t HW,
                                                                 float *__restrict__ gt_pl, float *__restrict__ pr_pl,
                                                                 double *__restrict__ part)
{
    __shared__ double s_d[4][kPrepThreads / 64];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const int64_t stride = (int64_t)gridDim.x * kPrepThreads;
    for (int64_t p = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; p < HW; p += stride) {
        float v[3], q[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            v[c] = gt_type == LSE_PIX_U8 ? (float)static_cast<const uint8_t *>(gt)[3 * p + c] / 255.0f
                                         : static_cast<const float *>(gt)[3 * p + c];
            q[c] = rgb[3 * p + c];
        }
        if (msk_type != LSE_PIX_NONE) {
            const float m = lse::load_pix(msk, msk_type, p);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = v[c] * m;
                q[c] = q[c] * m;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            gt_pl[c * HW + p] = v[c];
            pr_pl[c * HW + p] = q[c];
        }
        if (part != nullptr) {
            const double x = log_pred(rgb, p);
            const double y = log_gray(v[0], v[1], v[2]);
            acc[0] += x; acc[1] += x * x; acc[2] += y; acc[3] += x * y;
        }
    }
    if (part == nullptr) return;
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] = wave_sum_d(acc[q]);
        if ((threadIdx.x & 63) == 0) s_d[q][wv] = acc[q];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int q = threadIdx.x;
        double s = s_d[q][0];
        for (int k = 1; k < kPrepThreads / 64; ++k) s += s_d[q][k];
        part[(int64_t)q * gridDim.x + blockIdx.x] = s;
    }
}

// every workgroup sums the G partials in the same order and solves the same 2 x 2 system: one (a, b) for all
__global__ __launch_bounds__(kPrepThreads) void log_scale_correct_kernel(const float *__restrict__ gt_pl, const float *__restrict__ rgb,
                                                                         int64_t HW, const double *__restrict__ part, int G,
                                                                         float *__restrict__ coef, float *__restrict__ corrected,
                                                                         float *__restrict__ gray)
{
    __shared__ double s_d[4][kPrepThreads / 64];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < G; k += kPrepThreads) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += part[(int64_t)q * G + k];
    }
    const int wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[q] = wave_sum_d(acc[q]);
        if ((threadIdx.x & 63) == 0) s_d[q][wv] = acc[q];
    }
    __syncthreads();
    double S[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        S[q] = s_d[q][0];
        for (int k = 1; k < kPrepThreads / 64; ++k) S[q] += s_d[q][k];
    }
    const double N = (double)HW, Sx = S[0], Sxx = S[1], Sy = S[2], Sxy = S[3];
    const double det = N * Sxx - Sx * Sx;
    double a = NAN, b = NAN;
    if (isfinite(det) && fabs(det) > 0x1p-40 * fabs(N * Sxx)) {
        a = (N * Sxy - Sx * Sy) / det;
        b = (Sxx * Sy - Sx * Sxy) / det;
    }
    if (isnan(a)) a = 5.0 / 255.0;
    if (isnan(b)) b = 5.0 / 255.0;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        coef[0] = (float)a;
        coef[1] = (float)b;
    }
    const int64_t stride = (int64_t)gridDim.x * kPrepThreads;
    for (int64_t p = (int64_t)blockIdx.x * kPrepThreads + threadIdx.x; p < HW; p += stride) {
        const double x = log_pred(rgb, p);
        corrected[p] = expf((float)(a * x + b));
        gray[p] = gray3(gt_pl[p], gt_pl[HW + p], gt_pl[2 * HW + p]);
    }
}

int prep_shape(int32_t H, int32_t W, int *G, const char *what)
{
    LSE_REQUIRE(H >= 1 && W >= 1, "%s: H and W must be >= 1 (got H=%d, W=%d)", what, H, W);
    LSE_REQUIRE((int64_t)H * W <= INT32_MAX, "%s: %lld pixels exceed the supported image size", what, (long long)H * W);
    *G = stats_blocks((int64_t)H * W);
    return LSE_OK;
}

struct Layout {
    int G, tiles_x, tiles_y;
    int64_t n_tiles;
    int64_t bytes;
};

int layout(int32_t B, int32_t C, int32_t H, int32_t W, Layout *L, const char *what)
{
    LSE_REQUIRE(B >= 1 && C >= 1, "%s: B and C must be >= 1 (got B=%d, C=%d)", what, B, C);
    LSE_REQUIRE(H >= kWin && W >= kWin, "%s: H and W must be >= %d for an 11x11 SSIM window (got H=%d, W=%d)", what, kWin, H, W);
    const int64_t total = (int64_t)B * C * H * W;
    L->G = stats_blocks(total);
    L->tiles_x = (W - (kWin - 1) + kTile - 1) / kTile;
    L->tiles_y = (H - (kWin - 1) + kTile - 1) / kTile;
    L->n_tiles = (int64_t)B * C * L->tiles_x * L->tiles_y;
    LSE_REQUIRE(L->n_tiles < (int64_t)1 << 31, "%s: image too large (%lld tiles)", what, (long long)L->n_tiles);
    L->bytes = (int64_t)sizeof(double) * (5 * (int64_t)L->G + L->n_tiles);
    return LSE_OK;
}

}  // namespace

extern "C" int lse_image_metrics_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int64_t *h_bytes)
{
    LSE_REQUIRE(h_bytes, "lse_image_metrics_workspace: null pointer");
    Layout L;
    const int rc = layout(B, C, H, W, &L, "lse_image_metrics_workspace");
    if (rc != LSE_OK) return rc;
    *h_bytes = L.bytes;
    return LSE_OK;
}

extern "C" int lse_image_metrics(const float *preds, const float *target, int32_t B, int32_t C, int32_t H, int32_t W,
                                 const float *h_window, void *workspace, int64_t workspace_bytes, float *out_ssim,
                                 float *out_mse, lse_stream_t stream)
{
    Layout L;
    const int rc = layout(B, C, H, W, &L, "lse_image_metrics");
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(preds && target && h_window && workspace && out_ssim && out_mse, "lse_image_metrics: null pointer");
    LSE_REQUIRE(workspace_bytes >= L.bytes, "lse_image_metrics: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)L.bytes);
    LSE_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % sizeof(double) == 0, "lse_image_metrics: workspace not 8-byte aligned");
    Window win;
    for (int k = 0; k < kWin; ++k) win.w[k] = h_window[k];
    double *stats = static_cast<double *>(workspace);
    double *tiles = stats + 5 * (int64_t)L.G;
    const int64_t total = (int64_t)B * C * H * W;
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(stats_kernel, dim3(L.G), dim3(kStatsThreads), 0, st, preds, target, total, stats);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)L.n_tiles), dim3(256), 0, st, preds, target, (int)H, (int)W, L.tiles_x,
                       L.tiles_x * L.tiles_y, (const double *)stats, L.G, win, tiles);
    const double n_valid = (double)B * C * (double)(H - (kWin - 1)) * (double)(W - (kWin - 1));
    hipLaunchKernelGGL(metrics_final_kernel, dim3(1), dim3(kFinalThreads), 0, st, (const double *)tiles, L.n_tiles,
                       (const double *)(stats + 4 * (int64_t)L.G), L.G, n_valid, (double)total, out_ssim, out_mse);
    return lse::check_launch("lse_image_metrics");
}

extern "C" int lse_log_scale_correct_workspace(int32_t H, int32_t W, int64_t *h_bytes)
{
    const char *what = "lse_log_scale_correct_workspace";
    LSE_REQUIRE(h_bytes, "%s: null pointer", what);
    int G;
    const int rc = prep_shape(H, W, &G, what);
    if (rc != LSE_OK) return rc;
    *h_bytes = (int64_t)sizeof(double) * 4 * G;
    return LSE_OK;
}

extern "C" int lse_eval_image_prep(const void *gt, int32_t gt_type, const void *msk, int32_t msk_type, const float *rgb, int32_t H,
                                   int32_t W, int32_t flags, float *gt_planes, float *pred_planes, void *stats, int64_t stats_bytes,
                                   lse_stream_t stream)
{
    const char *what = "lse_eval_image_prep";
    int G;
    const int rc = prep_shape(H, W, &G, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(gt_type == LSE_PIX_U8 || gt_type == LSE_PIX_F32, "%s: gt_type %d (uint8 or f32 images)", what, gt_type);
    LSE_REQUIRE(msk_type == LSE_PIX_NONE || msk_type == LSE_PIX_U8 || msk_type == LSE_PIX_F32, "%s: msk_type %d", what, msk_type);
    LSE_REQUIRE((flags & ~LSE_PREP_EVENT_STATS) == 0, "%s: unknown flags %d", what, flags);
    LSE_REQUIRE(gt && rgb && gt_planes && pred_planes, "%s: null pointer", what);
    LSE_REQUIRE(msk_type == LSE_PIX_NONE || msk, "%s: null mask with msk_type %d", what, msk_type);
    double *part = nullptr;
    if (flags & LSE_PREP_EVENT_STATS) {
        LSE_REQUIRE(stats, "%s: null stats workspace", what);
        LSE_REQUIRE(stats_bytes >= (int64_t)sizeof(double) * 4 * G, "%s: stats workspace of %lld bytes, %lld needed", what,
                    (long long)stats_bytes, (long long)(sizeof(double) * 4 * G));
        LSE_REQUIRE(reinterpret_cast<uintptr_t>(stats) % sizeof(double) == 0, "%s: stats workspace not 8-byte aligned", what);
        part = static_cast<double *>(stats);
    }
    hipLaunchKernelGGL(eval_prep_kernel, dim3(G), dim3(kPrepThreads), 0, lse::as_stream(stream), gt, (int)gt_type, msk, (int)msk_type,
                       rgb, (int64_t)H * W, gt_planes, pred_planes, part);
    return lse::check_launch(what);
}

extern "C" int lse_log_scale_correct(const float *gt_planes, const float *rgb, int32_t H, int32_t W, const void *stats,
                                     int64_t stats_bytes, float *coef, float *corrected, float *gray, lse_stream_t stream)
{
    const char *what = "lse_log_scale_correct";
    int G;
    const int rc = prep_shape(H, W, &G, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(gt_planes && rgb && stats && coef && corrected && gray, "%s: null pointer", what);
    LSE_REQUIRE(stats_bytes >= (int64_t)sizeof(double) * 4 * G, "%s: stats workspace of %lld bytes, %lld needed", what,
                (long long)stats_bytes, (long long)(sizeof(double) * 4 * G));
    LSE_REQUIRE(reinterpret_cast<uintptr_t>(stats) % sizeof(double) == 0, "%s: stats workspace not 8-byte aligned", what);
    hipLaunchKernelGGL(log_scale_correct_kernel, dim3(G), dim3(kPrepThreads), 0, lse::as_stream(stream), gt_planes, rgb, (int64_t)H * W,
                       static_cast<const double *>(stats), G, coef, corrected, gray);
    return lse::check_launch(what);
}
