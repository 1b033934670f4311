// Weighted pixel draw for the batch composer (gfx950, wave64): pixels of a resident camera set are drawn with integer weights --
// 0 where the mask is 0, else 1 (colour) or `w_active` / `w_idle` by whether the event frame's value is != 0 -- instead of uniformly.
// The arithmetic is that of include/lse_hip.h ("weighted pixel draw"), integers from end to end; tests/pixel_draw_ref.py restates it.
//   rows_sum_kernel   one wave per image row r = c * H + y: lanes stride over the row, a butterfly gives the row sum.
//   rows_scan_kernel  one kScanThreads block: row sums -> exclusive offsets row_off [rows + 1] in place, the total at [rows].
//                     Both run once per scene, not per step.
//   draw_kernel       one wave per drawn pixel: Philox -> t in [0, total), a 64-ary search of row_off for the row (one probe per lane
//                     and a ballot per round), then a walk of that row 64 pixels at a time (wave prefix sum + ballot) for the pixel.
// The only state is row_off, 8 bytes per image row: the weights are recomputed from the images and masks, which are resident anyway.
// No LDS in the draw, no atomics, plain vector stores; the grids are fixed by (rows, n), so a captured graph can replay the draw.
#include "common.h"
#include "compact.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;

using lse::load_pix;

struct Weights {
    const void *images;     // event frames [rows, W] of pix_type, or null: every unmasked pixel weighs w_idle (== w_active then)
    const void *msk;        // [rows, W] of msk_type, or null: nothing is masked out
    int pix_type, msk_type;
    int w_active, w_idle;
};

__device__ __forceinline__ int pixel_weight(const Weights &w, int64_t pix)
{
    if (w.msk != nullptr && load_pix(w.msk, w.msk_type, pix) == 0.0f) return 0;
    if (w.images == nullptr) return w.w_idle;
    return load_pix(w.images, w.pix_type, pix) != 0.0f ? w.w_active : w.w_idle;
}

__device__ __forceinline__ int wave_sum_i(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void rows_sum_kernel(Weights w, int64_t rows, int W, int64_t *__restrict__ row_off)
{
    const int64_t r = ((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
    if (r >= rows) return;                      // (whole waves leave together: `r` is wave-uniform)
    int sum = 0;
    for (int x = lse::lane_id(); x < W; x += 64) sum += pixel_weight(w, r * W + x);
    sum = wave_sum_i(sum);
    if (lse::lane_id() == 0) row_off[r] = sum;
}

__global__ __launch_bounds__(lse::kScanThreads) void rows_scan_kernel(int64_t *__restrict__ row_off, int rows)
{
    const int64_t total = lse::block_exclusive_scan<int64_t>(row_off, rows, (int64_t)0);
    if (threadIdx.x == 0) row_off[rows] = total;
}

__global__ __launch_bounds__(kThreads) void draw_kernel(Weights w, int64_t rows, int H, int W, const int64_t *__restrict__ row_off,
                                                        uint64_t seed, uint32_t stream_id, const int64_t *__restrict__ step_dev,
                                                        int64_t step_arg, int n, int32_t *__restrict__ indices,
                                                        int32_t *__restrict__ weights)
{
    const int i = (int)(((int64_t)blockIdx.x * kThreads + threadIdx.x) >> 6);
    if (i >= n) return;                         // wave-uniform
    const int lane = lse::lane_id();
    const int64_t step = step_dev != nullptr ? *step_dev : step_arg;
    const lse::U4 p = lse::philox4x32_10(lse::U4{(uint32_t)step, (uint32_t)i, stream_id, 0u}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t total = (uint64_t)row_off[rows];
    const int64_t t = (int64_t)__umul64hi(((uint64_t)p.x << 32) | p.y, total);
    // row: the last r with row_off[r] <= t.  Invariant: row_off[lo] <= t, and hi == rows or row_off[hi] > t.
    int64_t lo = 0, hi = rows;
    while (hi - lo > 1) {
        const int64_t stride = (hi - lo + 63) >> 6;
        const int64_t probe = lo + lane * stride;
        const bool le = probe < hi && row_off[probe] <= t;
        const int k = __popcll(__ballot(le));   // row_off does not decrease: the lanes that hold are lanes 0 .. k - 1, and lane 0 holds
        const int64_t nlo = lo + (int64_t)(k > 0 ? k - 1 : 0) * stride;
        hi = nlo + stride < hi ? nlo + stride : hi;
        lo = nlo;
    }
    const int64_t r = lo;
    const int64_t v = t - row_off[r];
    // pixel: the last x whose exclusive prefix E(r, x) <= v, found 64 pixels at a time
    int64_t run = 0;
    int cnt = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        const int wt = x < W ? pixel_weight(w, r * W + x) : 0;
        const int inc = lse::wave_inclusive_sum_i(wt);
        cnt += __popcll(__ballot(x < W && run + (inc - wt) <= v));
        run += __shfl(inc, 63, 64);
        if (run > v) break;                     // wave-uniform: every later prefix is beyond v
    }
    const int x = cnt > 0 ? cnt - 1 : 0;
    if (lane == 0) {
        indices[3 * (int64_t)i] = (int32_t)(r / H);
        indices[3 * (int64_t)i + 1] = (int32_t)(r % H);
        indices[3 * (int64_t)i + 2] = x;
        weights[i] = pixel_weight(w, r * W + x);
    }
}

int check_weights(const char *what, const void *images, int pix_type, const void *msk, int msk_type, int n_images, int H, int W,
                  int w_active, int w_idle, Weights *out)
{
    LSE_REQUIRE(n_images >= 1 && H >= 1 && W >= 1, "%s: n_images, H and W must be >= 1 (got %d, %d, %d)", what, n_images, H, W);
    LSE_REQUIRE((int64_t)n_images * H <= INT32_MAX, "%s: %lld image rows exceed the supported %d", what,
                (long long)((int64_t)n_images * H), INT32_MAX);
    LSE_REQUIRE(W <= INT32_MAX / 255, "%s: rows of %d pixels: a row sum must fit 32 bits", what, W);
    LSE_REQUIRE(w_active >= 0 && w_active <= 255 && w_idle >= 0 && w_idle <= 255, "%s: weights %d / %d outside [0, 255]", what,
                w_active, w_idle);
    LSE_REQUIRE(w_active + w_idle > 0, "%s: both weights are zero", what);
    if (images != nullptr)
        LSE_REQUIRE(pix_type >= LSE_PIX_I8 && pix_type <= LSE_PIX_F32, "%s: pix_type %d", what, pix_type);
    else
        LSE_REQUIRE(w_active == w_idle, "%s: without images every pixel weighs the same: w_active must equal w_idle", what);
    if (msk != nullptr)
        LSE_REQUIRE(msk_type == LSE_PIX_U8 || msk_type == LSE_PIX_F32, "%s: msk_type %d", what, msk_type);
    else
        LSE_REQUIRE(msk_type == LSE_PIX_NONE, "%s: msk_type %d without a mask", what, msk_type);
    *out = Weights{images, msk, pix_type, msk_type, w_active, w_idle};
    return LSE_OK;
}

}  // namespace

extern "C" int lse_pixel_rows_build(const void *images, int32_t pix_type, const void *msk, int32_t msk_type, int32_t n_images,
                                    int32_t H, int32_t W, int32_t w_active, int32_t w_idle, int64_t *row_off, lse_stream_t stream)
{
    const char *what = "lse_pixel_rows_build";
    Weights w;
    const int rc = check_weights(what, images, pix_type, msk, msk_type, n_images, H, W, w_active, w_idle, &w);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(row_off && ((uintptr_t)row_off & 7) == 0, "%s: row_off must be a non-null, 8-byte aligned device pointer", what);
    const int64_t rows = (int64_t)n_images * H;
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(rows_sum_kernel, dim3(lse::blocks_for(rows * 64, kThreads)), dim3(kThreads), 0, st, w, rows, W, row_off);
    hipLaunchKernelGGL(rows_scan_kernel, dim3(1), dim3(lse::kScanThreads), 0, st, row_off, (int)rows);
    return lse::check_launch(what);
}

extern "C" int lse_pixel_draw(const void *images, int32_t pix_type, const void *msk, int32_t msk_type, int32_t n_images, int32_t H,
                              int32_t W, int32_t w_active, int32_t w_idle, const int64_t *row_off, uint64_t seed, int32_t stream_id,
                              const int64_t *step_dev, int64_t step, int32_t n, int32_t *indices, int32_t *weights,
                              lse_stream_t stream)
{
    const char *what = "lse_pixel_draw";
    Weights w;
    const int rc = check_weights(what, images, pix_type, msk, msk_type, n_images, H, W, w_active, w_idle, &w);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(n >= 0, "%s: n < 0", what);
    LSE_REQUIRE(stream_id == 0 || stream_id == 1, "%s: stream_id %d (0 colour / 1 events)", what, stream_id);
    LSE_REQUIRE(step_dev || step >= 0, "%s: a negative step without step_dev", what);
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(row_off && ((uintptr_t)row_off & 7) == 0, "%s: row_off must be a non-null, 8-byte aligned device pointer", what);
    LSE_REQUIRE(indices && weights, "%s: null output", what);
    hipLaunchKernelGGL(draw_kernel, dim3(lse::blocks_for((int64_t)n * 64, kThreads)), dim3(kThreads), 0, lse::as_stream(stream), w,
                       (int64_t)n_images * H, H, W, row_off, seed, (uint32_t)stream_id, step_dev, step, n, indices, weights);
    return lse::check_launch(what);
}
