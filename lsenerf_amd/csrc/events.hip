// Event synthesis for gfx950: log-intensity planes of a trajectory -> signed per-interval event counts and an ordered event stream
// (x, y, t, p), and the inverse, a stream -> accumulated event frames.  The sensor model -- ideal, noise-free, per pixel, linear in
// time between two planes -- is defined in include/lse_hip.h ("event synthesis") and, as numpy, in tests/events_ref.py; the kernels
// restate it operation by operation, hence -ffp-contract=off.
//   walk_kernel      lane = pixel: one pass over the K intervals carries the reference level, writes counts[k][p] and ref_out[p] and,
//                    for the stream, the interval's starting level and signed count per item (k, p) into the workspace
//   rank_kernel      the rank pass of compact.h over segments of LSE_EVENT_SEGMENT items, weighted: an item carries |n| events, not
//                    0 or 1, so a wave prefix SUM of |n| (a shuffle scan in place of ballot / popcount) gives every item the rank
//                    of its first event inside the segment and the segment its event count
//   scan_kernel      compact.h's scan, all in int64, behind the *total of entry: *total += the sum
//   emit_kernel      one thread per item rewalks its one interval from the stored level and writes its events at offset + rank + e;
//                    rows at or beyond cap are not written
//   sum_kernel       lse_event_count's window total: one block sums |counts| in a fixed order (int64)
//   accumulate_kernel one thread per event: frame by binary search over the bounds, a 32-bit integer vector atomic add into acc
// Fixed grids sized from the extent, plain vector stores, no host read.  The only atomics are accumulate's integer adds, whose sum
// does not depend on their order: two runs give the same bytes everywhere.
#include "compact.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSumThreads = 1024;            // the one block of lse_event_count's total
constexpr int kSeg = LSE_EVENT_SEGMENT;       // consecutive items owned by one wave
constexpr int kIters = kSeg / 64;
static_assert(kThreads == lse::kScanThreads, "scan_kernel is one block of kScanThreads");
constexpr int64_t kMaxItems = 1ll << 40;      // K * P, and the events of one accumulate call
constexpr int64_t kMaxPixels = 1ll << 30;     // P: 32767 x 32767 lies below
constexpr int kMaxAxis = 32767;               // x and y are int16
constexpr int kGridX = 1 << 20;               // blocks along x of the per-item grids; the rest goes to y

struct Sensor {
    float c_pos, c_neg;
    int cap_step;
};

// The walk of one interval: `ref` is carried, the return value is the signed count.  Every comparison is false on NaN, so a NaN level
// or plane gives no event and leaves ref; both loops are bounded by cap_step.
__device__ __forceinline__ int walk_interval(float &ref, float L1, Sensor s)
{
    int n = 0, pol = 0;
    if (L1 - ref >= s.c_pos) {
        pol = 1;
        while (L1 - ref >= s.c_pos && n < s.cap_step) {
            ref = ref + s.c_pos;
            ++n;
        }
    } else if (ref - L1 >= s.c_neg) {
        pol = -1;
        while (ref - L1 >= s.c_neg && n < s.cap_step) {
            ref = ref - s.c_neg;
            ++n;
        }
    }
    if (n == s.cap_step) ref = L1;            // saturated pixel: the level is re-armed at the interval's end
    return pol * n;
}

// time of the event that moved the level to `level` inside the interval (L0 at t0) .. (L1 at t1)
__device__ __forceinline__ double event_time(float level, float L0, float L1, double t0, double t1)
{
    const float d = L1 - L0;
    const float num = level - L0;
    const float q = (float)((double)num / (double)d);         // the correctly rounded f32 quotient
    const float frac = (d == 0.f || q != q) ? 0.f : (q < 0.f ? 0.f : (q > 1.f ? 1.f : q));
    const double dt = t1 - t0;
    const double prod = (double)frac * dt;
    return t0 + prod;
}

__global__ __launch_bounds__(kThreads) void walk_kernel(const float *__restrict__ L, int64_t K, int64_t P, const float *__restrict__ ref_in,
                                                        Sensor s, int32_t *__restrict__ counts, float *__restrict__ ref_out,
                                                        float *__restrict__ ws_ref, int32_t *__restrict__ ws_n)
{
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    float ref = ref_in[p];
    for (int64_t k = 0; k < K; ++k) {
        const int64_t i = k * P + p;
        const float start = ref;
        const int n = walk_interval(ref, L[i + P], s);
        if (counts) counts[i] = n;
        if (ws_n) {
            ws_ref[i] = start;
            ws_n[i] = n;
        }
    }
    ref_out[p] = ref;
}

// A segment holds at most kSeg * 32767 < 2^25 events: ranks and the running count fit an int.
__global__ __launch_bounds__(kThreads) void rank_kernel(const int32_t *__restrict__ ws_n, int64_t items, int n_segs,
                                                        int32_t *__restrict__ rank, int64_t *__restrict__ seg_counts)
{
    const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (seg >= n_segs) return;                          // (wave-uniform)
    const int lane = lse::lane_id();
    int run = 0;
    for (int it = 0; it < kIters; ++it) {
        const int64_t i = (int64_t)seg * kSeg + it * 64 + lane;
        const bool valid = i < items;
        const int n = valid ? ws_n[i] : 0;
        const int v = n < 0 ? -n : n;
        const int inc = lse::wave_inclusive_sum_i(v);
        if (valid) rank[i] = run + inc - v;
        run += __shfl(inc, 63, 64);
    }
    if (lane == 0) seg_counts[seg] = run;
}

// one block.  Counts -> exclusive offsets in place, starting at the *total of entry; *total += sum.  All in int64.
__global__ __launch_bounds__(kThreads) void scan_kernel(int64_t *__restrict__ seg, int n_segs, int64_t *__restrict__ total)
{
    const int64_t sum = lse::block_exclusive_scan<int64_t>(seg, n_segs, *total);
    if (threadIdx.x == 0) *total = sum;
}

__global__ __launch_bounds__(kThreads) void emit_kernel(const float *__restrict__ L, const double *__restrict__ times, int64_t items,
                                                        int64_t P, int W, Sensor s, const float *__restrict__ ws_ref,
                                                        const int32_t *__restrict__ ws_n, const int32_t *__restrict__ rank,
                                                        const int64_t *__restrict__ seg_off, int64_t cap, int16_t *__restrict__ out_x,
                                                        int16_t *__restrict__ out_y, double *__restrict__ out_t, int8_t *__restrict__ out_p)
{
    const int64_t i = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x;
    if (i >= items) return;
    const int n = ws_n[i];
    if (n == 0) return;
    const int64_t row0 = lse::segment_row<kSeg>(i, rank, seg_off);
    if (row0 >= cap) return;
    const int64_t k = i / P, p = i - k * P;
    const float L0 = L[i], L1 = L[i + P];
    const double t0 = times[k], t1 = times[k + 1];
    const int16_t x = (int16_t)(p % W), y = (int16_t)(p / W);
    const int8_t pol = n > 0 ? 1 : -1;
    const int count = n > 0 ? n : -n;
    float ref = ws_ref[i];
    for (int e = 0; e < count && e < s.cap_step; ++e) {
        ref = n > 0 ? ref + s.c_pos : ref - s.c_neg;
        const int64_t row = row0 + e;
        if (row >= cap) return;
        out_x[row] = x;
        out_y[row] = y;
        out_t[row] = event_time(ref, L0, L1, t0, t1);
        out_p[row] = pol;
    }
}

// one block of kSumThreads: |counts| summed per thread over a fixed stride -- four 16-byte loads in flight per thread where the pointer
// allows them, single elements for the rest -- then over the threads in a fixed tree.  |n| <= 32767: four of them fit an int.
__device__ __forceinline__ int abs_sum4(int4 v)
{
    return (v.x < 0 ? -v.x : v.x) + (v.y < 0 ? -v.y : v.y) + (v.z < 0 ? -v.z : v.z) + (v.w < 0 ? -v.w : v.w);
}

__global__ __launch_bounds__(kSumThreads) void sum_kernel(const int32_t *__restrict__ counts, int64_t items, int64_t *__restrict__ total)
{
    __shared__ int64_t part[kSumThreads];
    const int64_t quads = ((uintptr_t)counts & 15) == 0 ? items / 4 : 0;
    const int4 *__restrict__ c4 = reinterpret_cast<const int4 *>(counts);
    int64_t s = 0;
    int64_t i = threadIdx.x;
    for (; i + 3 * kSumThreads < quads; i += 4 * kSumThreads) {
        const int4 a = c4[i], b = c4[i + kSumThreads], c = c4[i + 2 * kSumThreads], d = c4[i + 3 * kSumThreads];
        s += abs_sum4(a) + abs_sum4(b);
        s += abs_sum4(c) + abs_sum4(d);
    }
    for (; i < quads; i += kSumThreads) s += abs_sum4(c4[i]);
    for (int64_t j = quads * 4 + threadIdx.x; j < items; j += kSumThreads) {
        const int n = counts[j];
        s += n < 0 ? -n : n;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = kSumThreads / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = part[0];
}

__global__ __launch_bounds__(kThreads) void accumulate_kernel(const int16_t *__restrict__ x, const int16_t *__restrict__ y,
                                                              const double *__restrict__ t, const int8_t *__restrict__ pol, int64_t n,
                                                              const int64_t *__restrict__ n_dev, const double *__restrict__ bounds,
                                                              int F, int H, int W, int32_t *__restrict__ acc)
{
    const int64_t i = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * kThreads + threadIdx.x;
    if (i >= lse::clamp_count(n, n_dev)) return;
    const double ti = t[i];
    if (!(bounds[0] <= ti && ti < bounds[F])) return;           // (false on NaN)
    const int xi = x[i], yi = y[i];
    if (xi < 0 || xi >= W || yi < 0 || yi >= H) return;
    int lo = 0, hi = F;                                          // bounds[lo] <= ti < bounds[hi]
    for (int it = 0; it < 32 && hi - lo > 1; ++it) {
        const int mid = lo + ((hi - lo) >> 1);
        if (bounds[mid] <= ti) lo = mid; else hi = mid;
    }
    atomicAdd(&acc[((int64_t)lo * H + yi) * W + xi], (int)pol[i]);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
inline dim3 item_grid(int64_t items)
{
    const int64_t blocks = (items + kThreads - 1) / kThreads;
    const int64_t gx = blocks < kGridX ? blocks : kGridX;
    return dim3((unsigned)gx, (unsigned)((blocks + gx - 1) / gx));
}

// per segment an int64 count / offset; per item the interval's starting level (f32), its signed count and its rank (int32)
inline int64_t workspace_bytes_for(int64_t items) { return 8 * (int64_t)lse::n_segments<kSeg>(items) + 12 * items; }

int check_extent(const char *what, int64_t K, int64_t P)
{
    LSE_REQUIRE(K >= 0 && K <= kMaxItems, "%s: %lld intervals outside [0, 2^40]", what, (long long)K);
    LSE_REQUIRE(P >= 0 && P <= kMaxPixels, "%s: %lld pixels outside [0, 2^30]", what, (long long)P);
    LSE_REQUIRE(K == 0 || P == 0 || K <= kMaxItems / P, "%s: K * P = %lld * %lld exceeds 2^40", what, (long long)K, (long long)P);
    return LSE_OK;
}

int check_sensor(const char *what, float c_pos, float c_neg, int32_t cap_step, Sensor &s)
{
    LSE_REQUIRE(c_pos > 0.f && c_pos < INFINITY && c_neg > 0.f && c_neg < INFINITY,
                "%s: the thresholds must be positive and finite, got %g and %g", what, (double)c_pos, (double)c_neg);
    LSE_REQUIRE(cap_step >= 1 && cap_step <= kMaxAxis, "%s: cap_step %d outside [1, 32767]", what, cap_step);
    s.c_pos = c_pos, s.c_neg = c_neg, s.cap_step = cap_step;
    return LSE_OK;
}

int copy_levels(const char *what, const float *ref_in, float *ref_out, int64_t P, hipStream_t st)
{
    if (P == 0) return LSE_OK;
    const hipError_t e = hipMemcpyAsync(ref_out, ref_in, (size_t)P * 4, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
        lse::set_error("%s: %s", what, hipGetErrorString(e));
        return LSE_E_LAUNCH;
    }
    return LSE_OK;
}

}  // namespace

extern "C" int lse_event_workspace(int64_t K, int64_t P, int64_t *h_bytes)
{
    const char *what = "lse_event_workspace";
    if (int rc = check_extent(what, K, P)) return rc;
    LSE_REQUIRE(h_bytes, "%s: null pointer", what);
    *h_bytes = workspace_bytes_for(K * P);
    return LSE_OK;
}

extern "C" int lse_event_count(const float *L, int64_t K, int64_t P, const float *ref_in, float c_pos, float c_neg, int32_t cap_step,
                               int32_t *counts, float *ref_out, int64_t *window_total, lse_stream_t stream)
{
    const char *what = "lse_event_count";
    Sensor s;
    if (int rc = check_extent(what, K, P)) return rc;
    if (int rc = check_sensor(what, c_pos, c_neg, cap_step, s)) return rc;
    LSE_REQUIRE(window_total && ((uintptr_t)window_total & 7) == 0, "%s: window_total must be a non-null, 8-byte aligned device pointer",
                what);
    LSE_REQUIRE(P == 0 || (ref_in && ref_out && ref_in != ref_out), "%s: ref_in and ref_out must be two non-null buffers", what);
    const int64_t items = K * P;
    LSE_REQUIRE(items == 0 || (L && counts), "%s: null pointer", what);
    hipStream_t st = lse::as_stream(stream);
    if (items == 0) {
        if (int rc = copy_levels(what, ref_in, ref_out, P, st)) return rc;
    } else {
        hipLaunchKernelGGL(walk_kernel, dim3(lse::blocks_for(P, kThreads)), dim3(kThreads), 0, st, L, K, P, ref_in, s, counts, ref_out,
                           (float *)nullptr, (int32_t *)nullptr);
    }
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(kSumThreads), 0, st, (const int32_t *)counts, items, window_total);
    return lse::check_launch(what);
}

extern "C" int lse_event_append(const float *L, const double *times, int64_t K, int64_t P, int32_t W, const float *ref_in, float c_pos,
                                float c_neg, int32_t cap_step, void *workspace, int64_t workspace_bytes, int64_t cap, int16_t *out_x,
                                int16_t *out_y, double *out_t, int8_t *out_p, int32_t *counts, float *ref_out, int64_t *total,
                                lse_stream_t stream)
{
    const char *what = "lse_event_append";
    Sensor s;
    if (int rc = check_extent(what, K, P)) return rc;
    if (int rc = check_sensor(what, c_pos, c_neg, cap_step, s)) return rc;
    LSE_REQUIRE(W >= 1 && W <= kMaxAxis, "%s: width %d outside [1, 32767]", what, W);
    LSE_REQUIRE(P % W == 0, "%s: %lld pixels are no whole number of rows of %d", what, (long long)P, W);
    LSE_REQUIRE(P / W <= kMaxAxis, "%s: height %lld above 32767", what, (long long)(P / W));
    LSE_REQUIRE(cap >= 0, "%s: negative capacity", what);
    LSE_REQUIRE(total && ((uintptr_t)total & 7) == 0, "%s: total must be a non-null, 8-byte aligned device pointer", what);
    LSE_REQUIRE(P == 0 || (ref_in && ref_out && ref_in != ref_out), "%s: ref_in and ref_out must be two non-null buffers", what);
    const int64_t items = K * P;
    hipStream_t st = lse::as_stream(stream);
    if (items == 0) return copy_levels(what, ref_in, ref_out, P, st);          // no interval: the levels pass through, *total stays
    const int64_t need = workspace_bytes_for(items);
    LSE_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: workspace must be a non-null, 8-byte aligned device pointer", what);
    LSE_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld", what, (long long)workspace_bytes, (long long)need);
    LSE_REQUIRE(L && times, "%s: null pointer", what);
    LSE_REQUIRE(cap == 0 || (out_x && out_y && out_t && out_p), "%s: null output for a capacity > 0", what);
    const int n_segs = lse::n_segments<kSeg>(items);
    int64_t *seg = static_cast<int64_t *>(workspace);
    float *ws_ref = reinterpret_cast<float *>(seg + n_segs);
    int32_t *ws_n = reinterpret_cast<int32_t *>(ws_ref + items);
    int32_t *rank = ws_n + items;
    hipLaunchKernelGGL(walk_kernel, dim3(lse::blocks_for(P, kThreads)), dim3(kThreads), 0, st, L, K, P, ref_in, s, counts, ref_out, ws_ref,
                       ws_n);
    hipLaunchKernelGGL(rank_kernel, dim3(lse::blocks_for(n_segs, kWaves)), dim3(kThreads), 0, st, (const int32_t *)ws_n, items, n_segs,
                       rank, seg);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, st, seg, n_segs, total);
    if (cap > 0)
        hipLaunchKernelGGL(emit_kernel, item_grid(items), dim3(kThreads), 0, st, L, times, items, P, (int)W, s, (const float *)ws_ref,
                           (const int32_t *)ws_n, (const int32_t *)rank, (const int64_t *)seg, cap, out_x, out_y, out_t, out_p);
    return lse::check_launch(what);
}

extern "C" int lse_event_accumulate(const int16_t *x, const int16_t *y, const double *t, const int8_t *p, int64_t n, const int64_t *n_dev,
                                    const double *bounds, int32_t F, int32_t H, int32_t W, int32_t *acc, lse_stream_t stream)
{
    const char *what = "lse_event_accumulate";
    LSE_REQUIRE(n >= 0 && n <= kMaxItems, "%s: extent %lld outside [0, 2^40]", what, (long long)n);
    LSE_REQUIRE(F >= 1 && H >= 1 && W >= 1, "%s: %d frames of %d x %d: every extent must be at least 1", what, F, H, W);
    LSE_REQUIRE(bounds && acc, "%s: null pointer", what);
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(x && y && t && p, "%s: null pointer", what);
    hipLaunchKernelGGL(accumulate_kernel, item_grid(n), dim3(kThreads), 0, lse::as_stream(stream), x, y, t, p, n, n_dev, bounds, (int)F,
                       (int)H, (int)W, acc);
    return lse::check_launch(what);
}
