// Point-cloud export for gfx950: rays of an eval render -> world points (unproject + validity filter, appended image after image),
// voxel keys, the per-voxel merge of a key-sorted cloud, and the neighbour-support ("floater") filter.  The definition is in
// include/lse_hip.h ("point-cloud export") and, as numpy, in tests/pointcloud_ref.py; the kernels restate it operation by operation,
// hence -ffp-contract=off.
// The three compacting entry points (count_* / scan_kernel / emit_*) are the ordered compaction of compact.h over segments of
// LSE_PC_SEGMENT items, with the plain workspace.
#include "compact.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSeg = LSE_PC_SEGMENT;          // consecutive items owned by one wave
static_assert(kThreads == lse::kScanThreads, "scan_kernel is one block of kScanThreads");
constexpr int kMaxAxis = 1 << 20;             // voxels per axis: a key stays below 2^60
constexpr int64_t kNoKey = INT64_MAX;

// one block.  Counts -> exclusive offsets in place; append: offsets start at the *total of entry and *total += sum, else *total = sum.
// A segment's count is at most kSeg, so a 256-segment step sums in int; the carry is int64.
__global__ __launch_bounds__(kThreads) void scan_kernel(int64_t *__restrict__ seg, int n_segs, int append, int64_t *__restrict__ total)
{
    const int64_t sum = lse::block_exclusive_scan<int>(seg, n_segs, append ? *total : (int64_t)0);
    if (threadIdx.x == 0) *total = sum;
}

__device__ __forceinline__ void copy3(float *__restrict__ dst, int64_t row, const float *__restrict__ src, int64_t i)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) dst[row * 3 + k] = src[i * 3 + k];
}

struct Box3 {
    float lo[3], hi[3];
};

// ---- unproject ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void unproject(const float *__restrict__ o, const float *__restrict__ d, float depth, int64_t r, float p[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float prod = d[r * 3 + k] * depth;
        p[k] = o[r * 3 + k] + prod;
    }
}

__global__ __launch_bounds__(kThreads) void count_rays_kernel(const float *__restrict__ origins, const float *__restrict__ directions,
                                                              const float *__restrict__ depth, const float *__restrict__ acc, int64_t n,
                                                              Box3 box, float min_acc, int n_segs, int32_t *__restrict__ rank,
                                                              int64_t *__restrict__ seg_counts)
{
    const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (seg >= n_segs) return;                          // (wave-uniform)
    lse::segment_rank<kSeg>(seg, n, rank, seg_counts, [&](int64_t r) {
        const float t = depth[r];
        bool keep = acc[r] >= min_acc && t > 0.f && t < INFINITY;       // every comparison is false on NaN
        float p[3];
        unproject(origins, directions, t, r, p);
#pragma unroll
        for (int k = 0; k < 3; ++k) keep = keep && box.lo[k] <= p[k] && p[k] <= box.hi[k];
        return keep;
    });
}

__global__ __launch_bounds__(kThreads) void emit_rays_kernel(const float *__restrict__ origins, const float *__restrict__ directions,
                                                             const float *__restrict__ depth, const float *__restrict__ colors,
                                                             const float *__restrict__ normals, int64_t n,
                                                             const int32_t *__restrict__ rank, const int64_t *__restrict__ seg_off,
                                                             int64_t cap, float *__restrict__ out_points, float *__restrict__ out_colors,
                                                             float *__restrict__ out_normals)
{
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (r >= n) return;
    const int64_t row = lse::emit_row<kSeg>(r, rank, seg_off, cap);
    if (row < 0) return;
    float p[3];
    unproject(origins, directions, depth[r], r, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) out_points[row * 3 + k] = p[k];
    if (out_colors) copy3(out_colors, row, colors, r);
    if (out_normals) copy3(out_normals, row, normals, r);
}

// ---- voxel keys -----------------------------------------------------------------------------------------------------------------
struct Voxels {
    int n[3];
};

__global__ __launch_bounds__(kThreads) void voxel_keys_kernel(const float *__restrict__ points, int64_t n, const int64_t *__restrict__ n_dev,
                                                              Box3 box, float voxel, Voxels V, int64_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    if (i >= lse::clamp_count(n, n_dev)) {
        keys[i] = kNoKey;
        return;
    }
    int v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float f = floorf((points[i * 3 + k] - box.lo[k]) / voxel);
        v[k] = f >= (float)(V.n[k] - 1) ? V.n[k] - 1 : (f > 0.f ? (int)f : 0);        // NaN -> 0
    }
    keys[i] = ((int64_t)v[0] * V.n[1] + v[1]) * V.n[2] + v[2];
}

// ---- voxel merge ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const int64_t *__restrict__ keys, int64_t i)
{
    const int64_t k = keys[i];
    return k != kNoKey && (i == 0 || k != keys[i - 1]);
}

__global__ __launch_bounds__(kThreads) void count_heads_kernel(const int64_t *__restrict__ sorted_keys, int64_t n, int n_segs,
                                                               int32_t *__restrict__ rank, int64_t *__restrict__ seg_counts)
{
    const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (seg >= n_segs) return;                          // (wave-uniform)
    lse::segment_rank<kSeg>(seg, n, rank, seg_counts, [&](int64_t i) { return is_head(sorted_keys, i); });
}

// s = first element, then + the others one by one in run order; an index outside [0, n) is skipped (never an out-of-bounds read)
__device__ __forceinline__ void run_sum(const float *__restrict__ values, const int64_t *__restrict__ order, int64_t first, int c,
                                        int64_t n, float s[3])
{
    s[0] = s[1] = s[2] = 0.f;
    bool any = false;
    for (int e = 0; e < c; ++e) {
        const int64_t src = order[first + e];
        if ((uint64_t)src >= (uint64_t)n) continue;
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = any ? s[k] + values[src * 3 + k] : values[src * 3 + k];
        any = true;
    }
}

// The thread that owns a head walks its run: O(longest run) -- the pixels of all views inside one voxel.
__global__ __launch_bounds__(kThreads) void emit_voxels_kernel(const int64_t *__restrict__ sorted_keys, const int64_t *__restrict__ order,
                                                               const float *__restrict__ points, const float *__restrict__ colors,
                                                               const float *__restrict__ normals, int64_t n,
                                                               const int32_t *__restrict__ rank, const int64_t *__restrict__ seg_off,
                                                               int64_t cap, int64_t *__restrict__ out_keys, int32_t *__restrict__ out_counts,
                                                               float *__restrict__ out_points, float *__restrict__ out_colors,
                                                               float *__restrict__ out_normals)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int64_t row = lse::emit_row<kSeg>(i, rank, seg_off, cap);
    if (row < 0) return;
    const int64_t key = sorted_keys[i];
    int c = 1;
    while (i + c < n && c < INT32_MAX && sorted_keys[i + c] == key) ++c;
    out_keys[row] = key;
    out_counts[row] = c;
    const float fc = (float)c;
    float s[3];
    run_sum(points, order, i, c, n, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) out_points[row * 3 + k] = s[k] / fc;
    if (out_colors) {
        run_sum(colors, order, i, c, n, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) out_colors[row * 3 + k] = s[k] / fc;
    }
    if (out_normals) {
        run_sum(normals, order, i, c, n, s);
        const float xx = s[0] * s[0], yy = s[1] * s[1], zz = s[2] * s[2];
        const float len = sqrtf((xx + yy) + zz);
        const float div = len > 1e-12f ? len : 1e-12f;
#pragma unroll
        for (int k = 0; k < 3; ++k) out_normals[row * 3 + k] = s[k] / div;
    }
}

// ---- support filter -------------------------------------------------------------------------------------------------------------
// first position in keys[0, m) whose key is >= key
__device__ __forceinline__ int64_t lower_bound(const int64_t *__restrict__ keys, int64_t m, int64_t key)
{
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Sum of the counts of the present voxels among the (up to) 27 of the 3 x 3 x 3 block around voxel j that lie inside the lattice.
// The (up to) three voxels of one (dx, dy) are consecutive keys: one binary search finds the first, the walk takes the others.
__device__ __forceinline__ int64_t support_of(const int64_t *__restrict__ keys, const int32_t *__restrict__ counts, int64_t m, Voxels V,
                                              int64_t j)
{
    const int64_t key = keys[j];
    const int64_t nz = V.n[2], ny = V.n[1], nx = V.n[0];
    const int64_t z = key % nz, y = (key / nz) % ny, x = key / (nz * ny);
    const int64_t z0 = z > 0 ? z - 1 : 0, z1 = z + 1 < nz ? z + 1 : nz - 1;
    int64_t sum = 0;
    for (int dx = -1; dx <= 1; ++dx) {
        const int64_t xx = x + dx;
        if (xx < 0 || xx >= nx) continue;
        for (int dy = -1; dy <= 1; ++dy) {
            const int64_t yy = y + dy;
            if (yy < 0 || yy >= ny) continue;
            const int64_t row = (xx * ny + yy) * nz;
            const int64_t k0 = row + z0, k1 = row + z1;
            for (int64_t p = lower_bound(keys, m, k0); p < m && keys[p] <= k1; ++p) sum += counts[p];     // (at most 3 steps: keys are unique)
        }
    }
    return sum;
}

__global__ __launch_bounds__(kThreads) void count_support_kernel(const int64_t *__restrict__ keys, const int32_t *__restrict__ counts,
                                                                 int64_t m, const int64_t *__restrict__ m_dev, Voxels V,
                                                                 int32_t min_support, int n_segs, int32_t *__restrict__ rank,
                                                                 int64_t *__restrict__ seg_counts, int32_t *__restrict__ out_support)
{
    const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (seg >= n_segs) return;                          // (wave-uniform)
    const int64_t count = lse::clamp_count(m, m_dev);
    lse::segment_rank<kSeg>(seg, m, rank, seg_counts, [&](int64_t j) {
        const bool present = j < count;
        const int64_t s = present ? support_of(keys, counts, count, V, j) : 0;
        if (out_support) out_support[j] = s > INT32_MAX ? INT32_MAX : (int32_t)s;
        return present && s >= (int64_t)min_support;
    });
}

__global__ __launch_bounds__(kThreads) void emit_kept_kernel(const int64_t *__restrict__ keys, const int32_t *__restrict__ counts,
                                                             const float *__restrict__ points, const float *__restrict__ colors,
                                                             const float *__restrict__ normals, int64_t m,
                                                             const int32_t *__restrict__ rank, const int64_t *__restrict__ seg_off,
                                                             int64_t cap, int64_t *__restrict__ out_keys, int32_t *__restrict__ out_counts,
                                                             float *__restrict__ out_points, float *__restrict__ out_colors,
                                                             float *__restrict__ out_normals)
{
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= m) return;
    const int64_t row = lse::emit_row<kSeg>(j, rank, seg_off, cap);
    if (row < 0) return;
    out_keys[row] = keys[j];
    out_counts[row] = counts[j];
    copy3(out_points, row, points, j);
    if (out_colors) copy3(out_colors, row, colors, j);
    if (out_normals) copy3(out_normals, row, normals, j);
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int workspace_bytes_of(const char *what, int64_t items, int64_t *h_bytes)
{
    LSE_REQUIRE(items >= 0 && items <= lse::kMaxCompactItems, "%s: extent %lld outside [0, 2^40]", what, (long long)items);
    LSE_REQUIRE(h_bytes, "%s: null pointer", what);
    *h_bytes = lse::compact_workspace_bytes<kSeg>(items);
    return LSE_OK;
}

bool make_voxels(int32_t nx, int32_t ny, int32_t nz, Voxels &V)
{
    if (nx < 1 || ny < 1 || nz < 1 || nx > kMaxAxis || ny > kMaxAxis || nz > kMaxAxis) return false;
    V.n[0] = nx, V.n[1] = ny, V.n[2] = nz;
    return true;
}

Box3 make_box(const float *h_lo, const float *h_hi)
{
    Box3 box;
    for (int k = 0; k < 3; ++k) { box.lo[k] = h_lo[k]; box.hi[k] = h_hi ? h_hi[k] : h_lo[k]; }
    return box;
}

}  // namespace

extern "C" int lse_unproject_workspace(int64_t n_rays, int64_t *h_bytes)
{
    return workspace_bytes_of("lse_unproject_workspace", n_rays, h_bytes);
}

extern "C" int lse_unproject_append(const float *origins, const float *directions, const float *depth, const float *acc,
                                    const float *colors, const float *normals, int64_t n_rays, const float *h_lo, const float *h_hi,
                                    float min_acc, void *workspace, int64_t workspace_bytes, int64_t cap, float *out_points,
                                    float *out_colors, float *out_normals, int64_t *total, lse_stream_t stream)
{
    const char *what = "lse_unproject_append";
    if (int rc = lse::check_compaction<kSeg>(what, n_rays, workspace, workspace_bytes, cap, total)) return rc;
    LSE_REQUIRE(h_lo && h_hi, "%s: null box", what);
    if (n_rays == 0) return LSE_OK;                     // nothing to append: *total stays
    LSE_REQUIRE((!out_colors || colors) && (!out_normals || normals), "%s: an output without its input", what);
    LSE_REQUIRE(origins && directions && depth && acc, "%s: null pointer", what);
    LSE_REQUIRE(cap == 0 || out_points, "%s: null output for a capacity > 0", what);
    const lse::CompactWorkspace w = lse::carve_compact<kSeg>(n_rays, workspace);
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(count_rays_kernel, dim3(lse::blocks_for(w.n_segs, kWaves)), dim3(kThreads), 0, st, origins, directions, depth, acc,
                       n_rays, make_box(h_lo, h_hi), min_acc, w.n_segs, w.rank, w.seg);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, st, w.seg, w.n_segs, 1, total);
    if (cap > 0)
        hipLaunchKernelGGL(emit_rays_kernel, dim3(lse::blocks_for(n_rays, kThreads)), dim3(kThreads), 0, st, origins, directions, depth,
                           colors, normals, n_rays, (const int32_t *)w.rank, (const int64_t *)w.seg, cap, out_points, out_colors, out_normals);
    return lse::check_launch(what);
}

extern "C" int lse_voxel_keys(const float *points, int64_t n, const int64_t *n_dev, const float *h_lo, float voxel, int32_t nx,
                              int32_t ny, int32_t nz, int64_t *keys, lse_stream_t stream)
{
    const char *what = "lse_voxel_keys";
    Voxels V;
    LSE_REQUIRE(make_voxels(nx, ny, nz, V), "%s: lattice %d x %d x %d: every count in [1, 2^20]", what, nx, ny, nz);
    LSE_REQUIRE(n >= 0 && n <= lse::kMaxCompactItems, "%s: extent %lld outside [0, 2^40]", what, (long long)n);
    LSE_REQUIRE(voxel > 0.f && voxel < INFINITY, "%s: the voxel size must be positive and finite", what);
    LSE_REQUIRE(h_lo, "%s: null box", what);
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(points && keys, "%s: null pointer", what);
    hipLaunchKernelGGL(voxel_keys_kernel, dim3(lse::blocks_for(n, kThreads)), dim3(kThreads), 0, lse::as_stream(stream), points, n, n_dev,
                       make_box(h_lo, nullptr), voxel, V, keys);
    return lse::check_launch(what);
}

extern "C" int lse_voxel_merge_workspace(int64_t n, int64_t *h_bytes)
{
    return workspace_bytes_of("lse_voxel_merge_workspace", n, h_bytes);
}

extern "C" int lse_voxel_merge(const int64_t *sorted_keys, const int64_t *order, const float *points, const float *colors,
                               const float *normals, int64_t n, void *workspace, int64_t workspace_bytes, int64_t cap,
                               int64_t *out_keys, int32_t *out_counts, float *out_points, float *out_colors, float *out_normals,
                               int64_t *total, lse_stream_t stream)
{
    const char *what = "lse_voxel_merge";
    if (int rc = lse::check_compaction<kSeg>(what, n, workspace, workspace_bytes, cap, total)) return rc;
    LSE_REQUIRE(n == 0 || ((!out_colors || colors) && (!out_normals || normals)), "%s: an output without its input", what);
    LSE_REQUIRE(n == 0 || (sorted_keys && order && points), "%s: null pointer", what);
    LSE_REQUIRE(n == 0 || cap == 0 || (out_keys && out_counts && out_points), "%s: null output for a capacity > 0", what);
    const lse::CompactWorkspace w = lse::carve_compact<kSeg>(n, workspace);
    hipStream_t st = lse::as_stream(stream);
    if (n > 0)
        hipLaunchKernelGGL(count_heads_kernel, dim3(lse::blocks_for(w.n_segs, kWaves)), dim3(kThreads), 0, st, sorted_keys, n, w.n_segs,
                           w.rank, w.seg);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, st, w.seg, w.n_segs, 0, total);       // (no segment: *total = 0)
    if (n > 0 && cap > 0)
        hipLaunchKernelGGL(emit_voxels_kernel, dim3(lse::blocks_for(n, kThreads)), dim3(kThreads), 0, st, sorted_keys, order, points,
                           colors, normals, n, (const int32_t *)w.rank, (const int64_t *)w.seg, cap, out_keys, out_counts, out_points,
                           out_colors, out_normals);
    return lse::check_launch(what);
}

extern "C" int lse_voxel_support_workspace(int64_t m, int64_t *h_bytes)
{
    return workspace_bytes_of("lse_voxel_support_workspace", m, h_bytes);
}

extern "C" int lse_voxel_support_filter(const int64_t *keys, const int32_t *counts, const float *points, const float *colors,
                                        const float *normals, int64_t m, const int64_t *m_dev, int32_t nx, int32_t ny, int32_t nz,
                                        int32_t min_support, void *workspace, int64_t workspace_bytes, int64_t cap, int64_t *out_keys,
                                        int32_t *out_counts, float *out_points, float *out_colors, float *out_normals,
                                        int32_t *out_support, int64_t *total, lse_stream_t stream)
{
    const char *what = "lse_voxel_support_filter";
    Voxels V;
    LSE_REQUIRE(make_voxels(nx, ny, nz, V), "%s: lattice %d x %d x %d: every count in [1, 2^20]", what, nx, ny, nz);
    if (int rc = lse::check_compaction<kSeg>(what, m, workspace, workspace_bytes, cap, total)) return rc;
    LSE_REQUIRE(m == 0 || ((!out_colors || colors) && (!out_normals || normals)), "%s: an output without its input", what);
    LSE_REQUIRE(m == 0 || (keys && counts && points), "%s: null pointer", what);
    LSE_REQUIRE(m == 0 || cap == 0 || (out_keys && out_counts && out_points), "%s: null output for a capacity > 0", what);
    const lse::CompactWorkspace w = lse::carve_compact<kSeg>(m, workspace);
    hipStream_t st = lse::as_stream(stream);
    if (m > 0)
        hipLaunchKernelGGL(count_support_kernel, dim3(lse::blocks_for(w.n_segs, kWaves)), dim3(kThreads), 0, st, keys, counts, m, m_dev, V,
                           min_support, w.n_segs, w.rank, w.seg, out_support);
    hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(kThreads), 0, st, w.seg, w.n_segs, 0, total);       // (no segment: *total = 0)
    if (m > 0 && cap > 0)
        hipLaunchKernelGGL(emit_kept_kernel, dim3(lse::blocks_for(m, kThreads)), dim3(kThreads), 0, st, keys, counts, points, colors, normals,
                           m, (const int32_t *)w.rank, (const int64_t *)w.seg, cap, out_keys, out_counts, out_points, out_colors,
                           out_normals);
    return lse::check_launch(what);
}
