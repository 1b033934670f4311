// Eval image panels on the device: 8-bit grey, Canny edges (classification + a host-free hysteresis) and the uint8 panel grid the
// reference's writer saves (include/lse_hip.h, "eval panels").  Compiled with -ffp-contract=off: every float operation of a panel
// value is rounded once, as the torch expression of evaluation.py rounds it.  Integer arithmetic everywhere in the Canny kernels.
#include "common.h"
#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 32;                       // Canny tile: kTile x kTile pixels per workgroup, four pixels per thread
constexpr int kTilePix = kTile * kTile;
constexpr int kNoLabel = INT_MAX;               // label of a pixel that is no candidate
constexpr int kMinMaxBlocks = 256;              // at most this many partials of the depth range

// (uint8) trunc(min(max(v * 255, 0), 255)); a NaN gives 0 (fmaxf returns its other argument)
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int)fminf(fmaxf(v * 255.0f, 0.0f), 255.0f); }

using lse::gray3;       // the grey of lse_eval_image_prep

__global__ __launch_bounds__(kThreads) void gray8_kernel(const float *__restrict__ a, const float *__restrict__ b, int64_t HW,
                                                         uint8_t *__restrict__ out)
{
    const float *src = blockIdx.y == 0 ? a : b;
    uint8_t *dst = out + (int64_t)blockIdx.y * HW;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += stride)
        dst[p] = to_u8(gray3(src[p], src[HW + p], src[2 * HW + p]));
}

// ---------------------------------------------------------------------------------------------------- Canny: classification
// One workgroup per tile.  s_gray: the tile plus a 2-pixel halo (replicated at the image border, as the Sobel border is);
// s_mag: |dx| + |dy| of the tile plus a 1-pixel halo, 0 outside the image.
__global__ __launch_bounds__(kThreads) void canny_classify_kernel(const uint8_t *__restrict__ gray, int H, int W, int tiles_x,
                                                                  int low, int high, uint8_t *__restrict__ cls)
{
    constexpr int GW = kTile + 4, MW = kTile + 2;
    __shared__ int16_t s_gray[GW * GW];
    __shared__ int s_mag[MW * MW];
    const int64_t img = (int64_t)blockIdx.y * H * W;
    const int y0 = (blockIdx.x / tiles_x) * kTile, x0 = (blockIdx.x % tiles_x) * kTile;
    for (int k = threadIdx.x; k < GW * GW; k += kThreads) {
        const int y = min(max(y0 - 2 + k / GW, 0), H - 1), x = min(max(x0 - 2 + k % GW, 0), W - 1);
        s_gray[k] = gray[img + (int64_t)y * W + x];
    }
    __syncthreads();
    for (int k = threadIdx.x; k < MW * MW; k += kThreads) {
        const int my = k / MW, mx = k % MW, y = y0 - 1 + my, x = x0 - 1 + mx;
        int m = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const int16_t *g = s_gray + (my + 1) * GW + (mx + 1);          // centre of the 3 x 3 window
            const int dx = (g[-GW + 1] + 2 * g[1] + g[GW + 1]) - (g[-GW - 1] + 2 * g[-1] + g[GW - 1]);
            const int dy = (g[GW - 1] + 2 * g[GW] + g[GW + 1]) - (g[-GW - 1] + 2 * g[-GW] + g[-GW + 1]);
            m = abs(dx) + abs(dy);
        }
        s_mag[k] = m;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kTilePix; k += kThreads) {
        const int ty = k / kTile, tx = k % kTile, y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const int16_t *g = s_gray + (ty + 2) * GW + (tx + 2);
        const int *mg = s_mag + (ty + 1) * MW + (tx + 1);
        const int dx = (g[-GW + 1] + 2 * g[1] + g[GW + 1]) - (g[-GW - 1] + 2 * g[-1] + g[GW - 1]);
        const int dy = (g[GW - 1] + 2 * g[GW] + g[GW + 1]) - (g[-GW - 1] + 2 * g[-GW] + g[-GW + 1]);
        const int m = mg[0];
        uint8_t c = 0;
        if (m > low) {
            const int ax = abs(dx), ay = abs(dy) << 15, tg22x = ax * 13573;
            bool pass;
            if (ay < tg22x) {
                pass = m > mg[-1] && m >= mg[1];
            } else if (ay > tg22x + (ax << 16)) {
                pass = m > mg[-MW] && m >= mg[MW];
            } else {
                const int s = ((dx ^ dy) < 0) ? -1 : 1;
                pass = m > mg[-MW - s] && m > mg[MW + s];
            }
            if (pass) c = m > high ? 2 : 1;
        }
        cls[img + (int64_t)y * W + x] = c;
    }
}

// ---------------------------------------------------------------------------------------------------- Canny: hysteresis
// Union-find over the candidates (weak or strong), 8-connected.  The key of pixel p is p when it is strong and HW + p when it is
// weak; label[p] holds the key of p's parent, a root holds its own key.  Links only ever go to a SMALLER key, so the root of a
// component is its smallest key: a component holds a strong pixel iff its root's key is below HW -- no flag array, no second pass.
// Every chase follows strictly decreasing keys, so it ends within 2 HW steps; the explicit bounds below only restate that.

// tile-local: keys are (strong ? 0 : kTilePix) + local index, the same order as the global keys of these pixels
__device__ __forceinline__ int find_lds(const volatile int *lab, int k)
{
    for (int it = 0; it < 2 * kTilePix; ++it) {
        const int p = lab[k & (kTilePix - 1)];
        if (p == k) break;
        k = p;
    }
    return k;
}

__device__ __forceinline__ void union_lds(int *lab, int a, int b)
{
    for (int it = 0; it < 4 * kTilePix; ++it) {
        a = find_lds(lab, a);
        b = find_lds(lab, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // a > b: hang a under b
        const int old = atomicMin(&lab[a & (kTilePix - 1)], b);
        if (old == a) return;                                   // a was still a root: linked
        a = old;                                                // somebody linked a first: merge that parent with b
    }
}

__global__ __launch_bounds__(kThreads) void canny_label_tiles_kernel(const uint8_t *__restrict__ cls, int H, int W, int tiles_x,
                                                                     int *__restrict__ label)
{
    __shared__ uint8_t s_cls[kTilePix];
    __shared__ int s_lab[kTilePix];
    const int HW = H * W;
    const int64_t img = (int64_t)blockIdx.y * HW;
    const int y0 = (blockIdx.x / tiles_x) * kTile, x0 = (blockIdx.x % tiles_x) * kTile;
    for (int k = threadIdx.x; k < kTilePix; k += kThreads) {
        const int y = y0 + k / kTile, x = x0 + k % kTile;
        const uint8_t c = (y < H && x < W) ? cls[img + (int64_t)y * W + x] : 0;
        s_cls[k] = c;
        s_lab[k] = c ? (c >= 2 ? 0 : kTilePix) + k : kNoLabel;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kTilePix; k += kThreads) {
        if (!s_cls[k]) continue;
        const int ty = k / kTile, tx = k % kTile;
        const int own = (s_cls[k] >= 2 ? 0 : kTilePix) + k;
        // the four forward neighbours; the backward ones are somebody else's forward ones
        if (tx + 1 < kTile && s_cls[k + 1]) union_lds(s_lab, own, (s_cls[k + 1] >= 2 ? 0 : kTilePix) + k + 1);
        if (ty + 1 < kTile) {
            const int d = k + kTile;
            if (tx > 0 && s_cls[d - 1]) union_lds(s_lab, own, (s_cls[d - 1] >= 2 ? 0 : kTilePix) + d - 1);
            if (s_cls[d]) union_lds(s_lab, own, (s_cls[d] >= 2 ? 0 : kTilePix) + d);
            if (tx + 1 < kTile && s_cls[d + 1]) union_lds(s_lab, own, (s_cls[d + 1] >= 2 ? 0 : kTilePix) + d + 1);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kTilePix; k += kThreads) {
        const int y = y0 + k / kTile, x = x0 + k % kTile;
        if (y >= H || x >= W) continue;
        int out = kNoLabel;
        if (s_cls[k]) {
            const int r = find_lds(s_lab, (s_cls[k] >= 2 ? 0 : kTilePix) + k);
            const int rl = r & (kTilePix - 1);
            out = (r < kTilePix ? 0 : HW) + (y0 + rl / kTile) * W + (x0 + rl % kTile);
        }
        label[img + (int64_t)y * W + x] = out;
    }
}

// across tile borders: other workgroups link at the same time, so labels are read past the vector L1 and linked with atomicMin.
// A stale read is an earlier parent, which is still an ancestor: it costs a step, never a wrong component.
__device__ __forceinline__ int load_label(const int *label, int HW, int key)
{
    return __hip_atomic_load(label + (key >= HW ? key - HW : key), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ int find_global(const int *label, int HW, int k)
{
    for (int64_t it = 0; it < 2 * (int64_t)HW; ++it) {
        const int p = load_label(label, HW, k);
        if (p == k) break;
        k = p;
    }
    return k;
}

__device__ __forceinline__ void union_global(int *label, int HW, int a, int b)
{
    for (int64_t it = 0; it < 4 * (int64_t)HW; ++it) {
        a = find_global(label, HW, a);
        b = find_global(label, HW, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(label + (a >= HW ? a - HW : a), b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(kThreads) void canny_merge_borders_kernel(const uint8_t *__restrict__ cls, int H, int W,
                                                                       int *__restrict__ label)
{
    const int HW = H * W;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= HW) return;
    cls += (int64_t)blockIdx.y * HW;
    label += (int64_t)blockIdx.y * HW;
    const int y = p / W, x = p % W, ty = y % kTile, tx = x % kTile;
    const bool last_col = tx == kTile - 1, last_row = ty == kTile - 1;
    if (!(last_col || last_row || tx == 0) || !cls[p]) return;
    const int own = (cls[p] >= 2 ? 0 : HW) + p;
    // forward neighbours that lie in another tile
    if (last_col && x + 1 < W && cls[p + 1]) union_global(label, HW, own, (cls[p + 1] >= 2 ? 0 : HW) + p + 1);
    if (y + 1 < H) {
        const int d = p + W;
        if ((last_row || tx == 0) && x > 0 && cls[d - 1]) union_global(label, HW, own, (cls[d - 1] >= 2 ? 0 : HW) + d - 1);
        if (last_row && cls[d]) union_global(label, HW, own, (cls[d] >= 2 ? 0 : HW) + d);
        if ((last_row || last_col) && x + 1 < W && cls[d + 1]) union_global(label, HW, own, (cls[d + 1] >= 2 ? 0 : HW) + d + 1);
    }
}

__global__ __launch_bounds__(kThreads) void canny_flatten_kernel(const int *__restrict__ label, int H, int W,
                                                                 uint8_t *__restrict__ edges)
{
    const int HW = H * W;
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= HW) return;
    label += (int64_t)blockIdx.y * HW;
    edges += (int64_t)blockIdx.y * HW;
    int k = label[p];
    uint8_t e = 0;
    if (k != kNoLabel) {
        for (int64_t it = 0; it < 2 * (int64_t)HW; ++it) {
            const int q = label[k >= HW ? k - HW : k];
            if (q == k) break;
            k = q;
        }
        e = k < HW ? 255 : 0;
    }
    edges[p] = e;
}

// ---------------------------------------------------------------------------------------------------- panels
// min / max that hand a NaN on, as torch.min / torch.max do
__device__ __forceinline__ float nan_min(float a, float b) { return (b < a || b != b) ? b : a; }
__device__ __forceinline__ float nan_max(float a, float b) { return (b > a || b != b) ? b : a; }

// both over the workgroup; valid in every thread
__device__ __forceinline__ void block_min_max(float &lo, float &hi, float (*s)[kThreads / 64])
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = nan_min(lo, __shfl_xor(lo, off, 64));
        hi = nan_max(hi, __shfl_xor(hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        s[0][threadIdx.x >> 6] = lo;
        s[1][threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    lo = s[0][0];
    hi = s[1][0];
    for (int k = 1; k < kThreads / 64; ++k) {
        lo = nan_min(lo, s[0][k]);
        hi = nan_max(hi, s[1][k]);
    }
}

// stage 1: per workgroup the min and max of its pixels -> part[2 + blockIdx.x], part[2 + G + blockIdx.x]
__global__ __launch_bounds__(kThreads) void depth_range_kernel(const float *__restrict__ depth, int64_t HW, float *__restrict__ part)
{
    __shared__ float s[2][kThreads / 64];
    float lo = INFINITY, hi = -INFINITY;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x; p < HW; p += stride) {
        const float v = depth[p];
        lo = nan_min(lo, v);
        hi = nan_max(hi, v);
    }
    block_min_max(lo, hi, s);
    if (threadIdx.x == 0) {
        part[2 + blockIdx.x] = lo;
        part[2 + gridDim.x + blockIdx.x] = hi;
    }
}

struct PanelArgs {
    const float *gt_planes, *pred_planes, *rgb, *pair_gt, *pair_pred, *depth, *acc, *ev_out;
    const uint8_t *edges;
    int ev_channels, H, W, flags, G, n_cols;
};

__device__ __forceinline__ float clip01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }          // a NaN stays

// one thread per pixel of the grid [H, n_cols * W, 3]; stage 2 of the depth range in every workgroup (the same G partials, so the
// same near / far everywhere), left in part[0], part[1] by workgroup 0
__global__ __launch_bounds__(kThreads) void eval_panels_kernel(PanelArgs a, float *__restrict__ part, uint8_t *__restrict__ grid)
{
    __shared__ float s[2][kThreads / 64];
    float near = 0.0f, far = 0.0f;
    if (a.flags & LSE_PANEL_DEPTH) {
        near = INFINITY;
        far = -INFINITY;
        for (int k = threadIdx.x; k < a.G; k += kThreads) {
            near = nan_min(near, part[2 + k]);
            far = nan_max(far, part[2 + a.G + k]);
        }
        block_min_max(near, far, s);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            part[0] = near;
            part[1] = far;
        }
    }
    const int HW = a.H * a.W, Wtot = a.n_cols * a.W;
    const int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (q >= (int64_t)a.H * Wtot) return;
    const int y = (int)(q / Wtot), X = (int)(q % Wtot), x = X % a.W, p = y * a.W + x;
    int col = X / a.W;
    float v[3];
    bool done = false;
    if (a.flags & LSE_PANEL_IMG) {
        if (col == 0) {          // the masked ground truth (or the grey one of the event-only metric)
            if (a.pair_gt) v[0] = v[1] = v[2] = a.pair_gt[p];
            else { v[0] = a.gt_planes[p]; v[1] = a.gt_planes[HW + p]; v[2] = a.gt_planes[2 * HW + p]; }
            done = true;
        } else if (col == 1) {   // the unmasked prediction (or the scale-corrected one)
            if (a.pair_pred) v[0] = v[1] = v[2] = a.pair_pred[p];
            else { v[0] = a.rgb[3 * (int64_t)p]; v[1] = a.rgb[3 * (int64_t)p + 1]; v[2] = a.rgb[3 * (int64_t)p + 2]; }
            done = true;
        }
        col -= 2;
    }
    if (!done && (a.flags & LSE_PANEL_DEPTH)) {
        if (col == 0) {          // depth_gray_map
            const float d = clip01((a.depth[p] - near) / ((far - near) + 1e-10f));
            const float acc = a.acc[p];
            v[0] = v[1] = v[2] = (1.0f - clip01(d)) * acc + (1.0f - acc);
            done = true;
        }
        col -= 1;
    }
    if (!done && (a.flags & LSE_PANEL_ERR_MAP)) {
        if (col == 0) {          // make_error_map, norm_cnst 6
            const float gi = gray3(a.gt_planes[p], a.gt_planes[HW + p], a.gt_planes[2 * HW + p]);
            const float gp = gray3(a.pred_planes[p], a.pred_planes[HW + p], a.pred_planes[2 * HW + p]);
            const float err = (gi - gp) * 6.0f;
            const bool pos = err > 0.0f, neg = err < 0.0f;
            v[0] = neg ? 1.0f - fabsf(err) : 1.0f;
            v[1] = pos ? 1.0f - err : (neg ? 1.0f - fabsf(err) : 1.0f);
            v[2] = pos ? 1.0f - err : 1.0f;
            done = true;
        }
        col -= 1;
    }
    uint8_t o[3];
    if (!done && (a.flags & LSE_PANEL_OVERLAY)) {
        if (col == 0) {          // white; black on an edge; red on the ground truth's, blue on the prediction's (both: magenta)
            const bool ge = a.edges[p] != 0, pe = a.edges[HW + p] != 0;
            o[0] = ge ? 255 : (pe ? 0 : 255);
            o[1] = (ge || pe) ? 0 : 255;
            o[2] = pe ? 255 : (ge ? 0 : 255);
            uint8_t *dst = grid + 3 * q;
            dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
            return;
        }
        col -= 1;
    }
    if (!done) {                 // ev_out: [H, W, 1] tiled to three channels, or [H, W, 3]
        const float *e = a.ev_out + (int64_t)p * a.ev_channels;
        v[0] = e[0];
        v[1] = a.ev_channels == 3 ? e[1] : e[0];
        v[2] = a.ev_channels == 3 ? e[2] : e[0];
    }
    uint8_t *dst = grid + 3 * q;
    dst[0] = to_u8(v[0]); dst[1] = to_u8(v[1]); dst[2] = to_u8(v[2]);
}

int image_shape(int32_t n, int32_t H, int32_t W, const char *what)
{
    LSE_REQUIRE(n >= 1, "%s: n_images must be >= 1 (got %d)", what, n);
    LSE_REQUIRE(H >= 1 && W >= 1, "%s: H and W must be >= 1 (got H=%d, W=%d)", what, H, W);
    LSE_REQUIRE((int64_t)H * W < (1 << 30), "%s: %lld pixels exceed the supported image size (below 2^30)", what, (long long)H * W);
    LSE_REQUIRE(n <= 65535, "%s: at most 65535 images per call (got %d)", what, n);
    return LSE_OK;
}

int64_t canny_bytes(int32_t H, int32_t W) { return ((int64_t)H * W * (int64_t)sizeof(int) + 7) / 8 * 8; }

int tiles(int32_t H, int32_t W, int *tiles_x) { *tiles_x = (W + kTile - 1) / kTile; return *tiles_x * ((H + kTile - 1) / kTile); }

int range_blocks(int64_t HW) { return (int)std::min<int64_t>(kMinMaxBlocks, (HW + kThreads - 1) / kThreads); }

int panel_cols(int flags)
{
    return 2 * !!(flags & LSE_PANEL_IMG) + !!(flags & LSE_PANEL_DEPTH) + !!(flags & LSE_PANEL_ERR_MAP) + !!(flags & LSE_PANEL_OVERLAY) +
           !!(flags & LSE_PANEL_EV_OUT);
}

int launch_classify(const uint8_t *gray, int32_t n, int32_t H, int32_t W, int32_t low, int32_t high, uint8_t *cls, hipStream_t st)
{
    if (low > high) std::swap(low, high);          // as OpenCV does
    int tx;
    const int nt = tiles(H, W, &tx);
    hipLaunchKernelGGL(canny_classify_kernel, dim3(nt, n), dim3(kThreads), 0, st, gray, (int)H, (int)W, tx, (int)low, (int)high, cls);
    return LSE_OK;
}

int launch_hysteresis(const uint8_t *cls, int32_t n, int32_t H, int32_t W, int *label, uint8_t *edges, hipStream_t st)
{
    int tx;
    const int nt = tiles(H, W, &tx);
    const int blocks = (int)(((int64_t)H * W + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(canny_label_tiles_kernel, dim3(nt, n), dim3(kThreads), 0, st, cls, (int)H, (int)W, tx, label);
    hipLaunchKernelGGL(canny_merge_borders_kernel, dim3(blocks, n), dim3(kThreads), 0, st, cls, (int)H, (int)W, label);
    hipLaunchKernelGGL(canny_flatten_kernel, dim3(blocks, n), dim3(kThreads), 0, st, (const int *)label, (int)H, (int)W, edges);
    return LSE_OK;
}

int check_canny_ws(const void *ws, int64_t ws_bytes, int32_t n, int32_t H, int32_t W, const char *what)
{
    LSE_REQUIRE(ws, "%s: null workspace", what);
    LSE_REQUIRE(ws_bytes >= n * canny_bytes(H, W), "%s: workspace of %lld bytes, %lld needed", what, (long long)ws_bytes,
                (long long)(n * canny_bytes(H, W)));
    LSE_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 8 == 0, "%s: workspace not 8-byte aligned", what);
    return LSE_OK;
}

}  // namespace

extern "C" int lse_gray8_planes(const float *planes_a, const float *planes_b, int32_t H, int32_t W, uint8_t *out, lse_stream_t stream)
{
    const char *what = "lse_gray8_planes";
    const int rc = image_shape(1, H, W, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(planes_a && out, "%s: null pointer", what);
    const int64_t HW = (int64_t)H * W;
    const int blocks = (int)std::min<int64_t>((HW + kThreads - 1) / kThreads, 4096);
    hipLaunchKernelGGL(gray8_kernel, dim3(blocks, planes_b ? 2 : 1), dim3(kThreads), 0, lse::as_stream(stream), planes_a, planes_b, HW,
                       out);
    return lse::check_launch(what);
}

extern "C" int lse_canny_workspace(int32_t H, int32_t W, int64_t *h_bytes)
{
    const char *what = "lse_canny_workspace";
    LSE_REQUIRE(h_bytes, "%s: null pointer", what);
    const int rc = image_shape(1, H, W, what);
    if (rc != LSE_OK) return rc;
    *h_bytes = canny_bytes(H, W);
    return LSE_OK;
}

extern "C" int lse_canny_classify(const uint8_t *gray, int32_t n_images, int32_t H, int32_t W, int32_t low, int32_t high,
                                  uint8_t *classes, lse_stream_t stream)
{
    const char *what = "lse_canny_classify";
    const int rc = image_shape(n_images, H, W, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(gray && classes, "%s: null pointer", what);
    LSE_REQUIRE(gray != classes, "%s: the class map cannot alias the image", what);
    launch_classify(gray, n_images, H, W, low, high, classes, lse::as_stream(stream));
    return lse::check_launch(what);
}

extern "C" int lse_canny_hysteresis(const uint8_t *classes, int32_t n_images, int32_t H, int32_t W, void *workspace,
                                    int64_t workspace_bytes, uint8_t *edges, lse_stream_t stream)
{
    const char *what = "lse_canny_hysteresis";
    int rc = image_shape(n_images, H, W, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(classes && edges, "%s: null pointer", what);
    if ((rc = check_canny_ws(workspace, workspace_bytes, n_images, H, W, what)) != LSE_OK) return rc;
    launch_hysteresis(classes, n_images, H, W, static_cast<int *>(workspace), edges, lse::as_stream(stream));
    return lse::check_launch(what);
}

extern "C" int lse_canny_u8(const uint8_t *gray, int32_t n_images, int32_t H, int32_t W, int32_t low, int32_t high, void *workspace,
                            int64_t workspace_bytes, uint8_t *edges, lse_stream_t stream)
{
    const char *what = "lse_canny_u8";
    int rc = image_shape(n_images, H, W, what);
    if (rc != LSE_OK) return rc;
    LSE_REQUIRE(gray && edges, "%s: null pointer", what);
    LSE_REQUIRE(gray != edges, "%s: the edge map cannot alias the image", what);
    if ((rc = check_canny_ws(workspace, workspace_bytes, n_images, H, W, what)) != LSE_OK) return rc;
    hipStream_t st = lse::as_stream(stream);
    launch_classify(gray, n_images, H, W, low, high, edges, st);          // the class map lives in `edges` until the last launch
    launch_hysteresis(edges, n_images, H, W, static_cast<int *>(workspace), edges, st);
    return lse::check_launch(what);
}

extern "C" int lse_eval_panels_workspace(int32_t H, int32_t W, int64_t *h_bytes)
{
    const char *what = "lse_eval_panels_workspace";
    LSE_REQUIRE(h_bytes, "%s: null pointer", what);
    const int rc = image_shape(1, H, W, what);
    if (rc != LSE_OK) return rc;
    *h_bytes = ((int64_t)sizeof(float) * (2 + 2 * range_blocks((int64_t)H * W)) + 7) / 8 * 8;
    return LSE_OK;
}

extern "C" int lse_eval_panels(const float *gt_planes, const float *pred_planes, const float *rgb, const float *pair_gt,
                               const float *pair_pred, const float *depth, const float *accumulation, const uint8_t *edges,
                               const float *ev_out, int32_t ev_channels, int32_t H, int32_t W, int32_t flags, void *workspace,
                               int64_t workspace_bytes, uint8_t *grid, lse_stream_t stream)
{
    const char *what = "lse_eval_panels";
    const int rc = image_shape(1, H, W, what);
    if (rc != LSE_OK) return rc;
    const int all = LSE_PANEL_IMG | LSE_PANEL_DEPTH | LSE_PANEL_ERR_MAP | LSE_PANEL_OVERLAY | LSE_PANEL_EV_OUT;
    LSE_REQUIRE(flags != 0 && (flags & ~all) == 0, "%s: flags %d select no panel or an unknown one", what, flags);
    LSE_REQUIRE(grid, "%s: null grid", what);
    LSE_REQUIRE((pair_gt == nullptr) == (pair_pred == nullptr), "%s: the grey pair is two images or none", what);
    if (flags & LSE_PANEL_IMG) LSE_REQUIRE(pair_gt || (gt_planes && rgb), "%s: img needs gt_planes and rgb, or the grey pair", what);
    if (flags & LSE_PANEL_DEPTH) LSE_REQUIRE(depth && accumulation, "%s: depth needs depth and accumulation", what);
    if (flags & LSE_PANEL_ERR_MAP) LSE_REQUIRE(gt_planes && pred_planes, "%s: err_map needs both masked planes", what);
    if (flags & LSE_PANEL_OVERLAY) LSE_REQUIRE(edges, "%s: overlay needs the two edge maps", what);
    if (flags & LSE_PANEL_EV_OUT)
        LSE_REQUIRE(ev_out && (ev_channels == 1 || ev_channels == 3), "%s: ev_out needs 1 or 3 channels (got %d)", what, ev_channels);
    const int64_t HW = (int64_t)H * W;
    const int n_cols = panel_cols(flags), G = range_blocks(HW);
    const int64_t total = HW * n_cols;
    LSE_REQUIRE(3 * total <= INT32_MAX, "%s: a grid of %lld bytes exceeds the supported size", what, (long long)(3 * total));
    float *part = static_cast<float *>(workspace);
    hipStream_t st = lse::as_stream(stream);
    if (flags & LSE_PANEL_DEPTH) {
        LSE_REQUIRE(workspace, "%s: null workspace", what);
        LSE_REQUIRE(workspace_bytes >= (int64_t)sizeof(float) * (2 + 2 * G), "%s: workspace of %lld bytes, %lld needed", what,
                    (long long)workspace_bytes, (long long)(sizeof(float) * (2 + 2 * G)));
        LSE_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 8 == 0, "%s: workspace not 8-byte aligned", what);
        hipLaunchKernelGGL(depth_range_kernel, dim3(G), dim3(kThreads), 0, st, depth, HW, part);
    }
    PanelArgs a{gt_planes, pred_planes, rgb, pair_gt, pair_pred, depth, accumulation, ev_out, edges, (int)ev_channels, (int)H, (int)W,
                (int)flags, G, n_cols};
    hipLaunchKernelGGL(eval_panels_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, a, part, grid);
    return lse::check_launch(what);
}
