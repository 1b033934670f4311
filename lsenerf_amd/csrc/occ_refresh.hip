// Count-free occupancy-grid refresh for gfx950: the index generation of nerfacc's OccGridEstimator._update as
// device code, so that a refresh sizes nothing from a device value and captures into a HIP graph.
//   list_count / list_scan / list_write   ascending indices of the set cells of every level (== torch.nonzero): the ordered
//                    compaction of compact.h in this file's own layout -- one wave owns 1024 consecutive cells of a 4096-cell
//                    tile, int32 tile counts are scanned by one block per level, and the write pass recomputes the ballots
//                    instead of reading stored ranks.  No atomics.
//   draw_kernel      one thread per slot: Philox4x32-10 (philox.h, shared with compose.hip) at counter (step, slot, level, 0), the
//                    cell (occupied list / uniform / every cell during warm-up), its jittered position, n_dev of the level.
//   ema_pass1..3     lse_occ_update_cells' three passes with the count read from n_dev and ids < 0 skipped.
//   mean_stage1 / 2  mean(occs) and min(mean(occs[occs >= 0]), occ_thre): fixed grid, double accumulators, fixed order.
// All of it is bandwidth- or latency-bound work over at most a few million cells.  Compiled with -ffp-contract=off: the position
// arithmetic restates the torch expression of _update_samples operation by operation (lsenerf_amd/occ_refresh.py: draw_cells_host).
#include "compact.h"
#include "philox.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kWaveCells = LSE_OCC_LIST_TILE / kWaves;      // consecutive cells owned by one wave
constexpr int kIters = kWaveCells / 64;
static_assert(kThreads == lse::kScanThreads, "list_scan_kernel is blocks of kScanThreads");

using lse::U4;
using lse::wave_sum_d;

// ---- 1. occupied-cell list ----------------------------------------------------------------------------------------------------
// set cells among the 1024 cells of this wave that start at `base` (wave-uniform result; every lane takes every iteration)
__device__ __forceinline__ int wave_segment_count(const uint8_t *__restrict__ lv, int64_t base, int64_t cells, int lane)
{
    int c = 0;
#pragma unroll 4
    for (int it = 0; it < kIters; ++it) {
        const int64_t i = base + it * 64 + lane;
        int total;
        lse::wave_prefix_count(i < cells && lv[i] != 0, total);
        c += total;
    }
    return c;
}

__global__ __launch_bounds__(kThreads) void list_count_kernel(const uint8_t *__restrict__ bin, int64_t cells, int n_tiles,
                                                              int32_t *__restrict__ tile_counts)
{
    __shared__ int sh[kWaves];
    const int level = blockIdx.y, tile = blockIdx.x, w = threadIdx.x >> 6, lane = lse::lane_id();
    const int c = wave_segment_count(bin + (int64_t)level * cells, (int64_t)tile * LSE_OCC_LIST_TILE + w * kWaveCells, cells, lane);
    if (lane == 0) sh[w] = c;
    __syncthreads();
    if (threadIdx.x == 0) tile_counts[(int64_t)level * n_tiles + tile] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// one block per level: tile counts -> exclusive offsets (in place), total -> counts[level]
__global__ __launch_bounds__(kThreads) void list_scan_kernel(int32_t *__restrict__ tile_counts, int n_tiles, int64_t *__restrict__ counts)
{
    const int sum = lse::block_exclusive_scan<int>(tile_counts + (int64_t)blockIdx.x * n_tiles, n_tiles, 0);
    if (threadIdx.x == 0) counts[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kThreads) void list_write_kernel(const uint8_t *__restrict__ bin, int64_t cells, int n_tiles,
                                                              const int32_t *__restrict__ tile_offsets, int32_t *__restrict__ list)
{
    __shared__ int sh[kWaves];
    const int level = blockIdx.y, tile = blockIdx.x, w = threadIdx.x >> 6, lane = lse::lane_id();
    const uint8_t *lv = bin + (int64_t)level * cells;
    const int64_t base = (int64_t)tile * LSE_OCC_LIST_TILE + w * kWaveCells;
    const int c = wave_segment_count(lv, base, cells, lane);
    if (lane == 0) sh[w] = c;
    __syncthreads();
    int64_t off = tile_offsets[(int64_t)level * n_tiles + tile];
#pragma unroll
    for (int k = 0; k < kWaves; ++k)
        if (k < w) off += sh[k];
    if (c == 0) return;                         // (wave-uniform)
    int32_t *out = list + (int64_t)level * cells;
    for (int it = 0; it < kIters; ++it) {
        const int64_t i = base + it * 64 + lane;
        const bool set = i < cells && lv[i] != 0;
        int total;
        const int below = lse::wave_prefix_count(set, total);
        // rank < the level's count <= cells: inside the level's row of the list
        if (set) out[off + below] = (int32_t)i;
        off += total;
    }
}

// ---- 2. cell draw + positions of one level ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void draw_kernel(const float *__restrict__ occs, const int32_t *__restrict__ list,
                                                        const int64_t *__restrict__ counts, const float *__restrict__ aabbs, int level,
                                                        int64_t cells, int rx, int ry, int rz, int warmup,
                                                        const int64_t *__restrict__ step_dev, uint32_t k0, uint32_t k1, int64_t cap,
                                                        int64_t *__restrict__ ids, float *__restrict__ pos, int64_t *__restrict__ n_dev)
{
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t N = cells / 4;
    int64_t cnt = 0, m = 0, n = cells;
    if (!warmup) {
        cnt = counts[level];
        cnt = cnt < 0 ? 0 : (cnt > cells ? cells : cnt);
        m = cnt < N ? cnt : N;
        n = m + N;
    }
    if (n > cap) n = cap;                       // (the entry point checks cap >= cells / 2 N: never taken)
    if (i == 0) *n_dev = n;
    if (i >= n) return;
    const U4 r = lse::philox4x32_10(U4{(uint32_t)*step_dev, (uint32_t)i, (uint32_t)level, 0u}, k0, k1);
    const int64_t row = (int64_t)level * cells;
    int64_t idx;
    if (warmup)
        idx = i;
    else if (i < m)
        idx = cnt <= N ? list[row + i] : list[row + __umulhi(r.x, (uint32_t)cnt)];
    else
        idx = __umulhi(r.x, (uint32_t)cells);
    idx = idx < 0 ? 0 : (idx >= cells ? cells - 1 : idx);      // (a list that was not built for this grid must not lead outside it)
    const int cz = (int)(idx % rz), cy = (int)((idx / rz) % ry), cx = (int)(idx / ((int64_t)rz * ry));
    const float *ab = aabbs + 6 * level;
    const float ux = (float)(r.y >> 8) * 5.9604644775390625e-08f;
    const float uy = (float)(r.z >> 8) * 5.9604644775390625e-08f;
    const float uz = (float)(r.w >> 8) * 5.9604644775390625e-08f;
    const float fx = ((float)cx + ux) / (float)rx, fy = ((float)cy + uy) / (float)ry, fz = ((float)cz + uz) / (float)rz;
    pos[3 * i] = ab[0] + fx * (ab[3] - ab[0]);
    pos[3 * i + 1] = ab[1] + fy * (ab[4] - ab[1]);
    pos[3 * i + 2] = ab[2] + fz * (ab[5] - ab[2]);
    ids[i] = occs[row + idx] < 0.f ? (int64_t)-1 : row + idx;
}

// ---- 3. EMA-max with the count on the device (passes of optim.hip: occ_pass1..3) -----------------------------------------------
__global__ void ema_pass1(const float *__restrict__ occs, const int64_t *__restrict__ ids, const float *__restrict__ sigma,
                          float step_size, const int64_t *__restrict__ n_dev, int64_t cap, float ema, float *__restrict__ ws)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lse::clamp_count(cap, n_dev)) return;
    const int64_t id = ids[i];
    if (id >= 0) ws[i] = fmaxf(occs[id] * ema, sigma[i] * step_size);
}
__global__ void ema_pass2(float *__restrict__ occs, const int64_t *__restrict__ ids, const int64_t *__restrict__ n_dev, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lse::clamp_count(cap, n_dev)) return;
    const int64_t id = ids[i];
    if (id >= 0) occs[id] = 0.f;
}
__global__ void ema_pass3(float *__restrict__ occs, const int64_t *__restrict__ ids, const float *__restrict__ ws,
                          const int64_t *__restrict__ n_dev, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= lse::clamp_count(cap, n_dev)) return;
    const int64_t id = ids[i];
    if (id >= 0) atomicMax(reinterpret_cast<int *>(occs) + id, __float_as_int(fmaxf(ws[i], 0.f)));
}

// ---- 4. mean and threshold ----------------------------------------------------------------------------------------------------
// sums of one block's three accumulators, in a fixed order; valid in thread 0
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c)
{
    __shared__ double sh[3][kWaves];
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    c = wave_sum_d(c);
    const int w = threadIdx.x >> 6;
    if (lse::lane_id() == 0) {
        sh[0][w] = a;
        sh[1][w] = b;
        sh[2][w] = c;
    }
    __syncthreads();
    a = (sh[0][0] + sh[0][1]) + (sh[0][2] + sh[0][3]);
    b = (sh[1][0] + sh[1][1]) + (sh[1][2] + sh[1][3]);
    c = (sh[2][0] + sh[2][1]) + (sh[2][2] + sh[2][3]);
}

__global__ __launch_bounds__(kThreads) void mean_stage1(const float *__restrict__ occs, int64_t n, double *__restrict__ part)
{
    double s_all = 0.0, s_pos = 0.0, c_pos = 0.0;
    const int64_t stride = (int64_t)gridDim.x * kThreads;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride) {
        const float v = occs[i];
        s_all += (double)v;
        if (v >= 0.f) {
            s_pos += (double)v;
            c_pos += 1.0;
        }
    }
    block_sum3(s_all, s_pos, c_pos);
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = s_all;
        part[3 * blockIdx.x + 1] = s_pos;
        part[3 * blockIdx.x + 2] = c_pos;
    }
}

__global__ __launch_bounds__(kThreads) void mean_stage2(const double *__restrict__ part, int n_blocks, int64_t n, float occ_thre,
                                                        float *__restrict__ mean_all, float *__restrict__ thre)
{
    double s_all = 0.0, s_pos = 0.0, c_pos = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += kThreads) {
        s_all += part[3 * b];
        s_pos += part[3 * b + 1];
        c_pos += part[3 * b + 2];
    }
    block_sum3(s_all, s_pos, c_pos);
    if (threadIdx.x == 0) {
        *mean_all = (float)(s_all / (double)n);
        const float m = (float)(s_pos / c_pos);          // 0 / 0 = NaN: torch's mean of an empty selection
        *thre = m > occ_thre ? occ_thre : m;             // torch.clamp(m, max=occ_thre): NaN stays NaN
    }
}

}  // namespace

extern "C" int lse_occ_list_occupied(const uint8_t *binaries, int32_t levels, int64_t cells, int32_t *list, int64_t *counts,
                                     int32_t *workspace, lse_stream_t stream)
{
    const char *what = "lse_occ_list_occupied";
    LSE_REQUIRE(levels >= 1 && levels <= 65535, "%s: levels %d", what, levels);
    LSE_REQUIRE(cells >= 1 && cells < (1ll << 31), "%s: cells per level must be in [1, 2^31)", what);
    LSE_REQUIRE(binaries && list && counts && workspace, "%s: null pointer", what);
    const int n_tiles = (int)((cells + LSE_OCC_LIST_TILE - 1) / LSE_OCC_LIST_TILE);
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(list_count_kernel, dim3(n_tiles, levels), dim3(kThreads), 0, st, binaries, cells, n_tiles, workspace);
    hipLaunchKernelGGL(list_scan_kernel, dim3(levels), dim3(kThreads), 0, st, workspace, n_tiles, counts);
    hipLaunchKernelGGL(list_write_kernel, dim3(n_tiles, levels), dim3(kThreads), 0, st, binaries, cells, n_tiles,
                       (const int32_t *)workspace, list);
    return lse::check_launch(what);
}

extern "C" int lse_occ_draw_cells(const float *occs, const int32_t *list, const int64_t *counts, const float *aabbs, int32_t level,
                                  int64_t cells, int32_t res_x, int32_t res_y, int32_t res_z, int32_t warmup, const int64_t *step_dev,
                                  uint64_t seed, int64_t cap, int64_t *cell_ids, float *positions, int64_t *n_dev, lse_stream_t stream)
{
    const char *what = "lse_occ_draw_cells";
    LSE_REQUIRE(level >= 0 && level < LSE_MAX_OCC_LEVELS, "%s: level %d", what, level);
    LSE_REQUIRE(cells >= 1 && cells < (1ll << 31), "%s: cells per level must be in [1, 2^31)", what);
    LSE_REQUIRE(res_x >= 1 && res_y >= 1 && res_z >= 1 && (int64_t)res_x * res_y * res_z == cells,
                "%s: resolution %d x %d x %d is not the %lld cells of a level", what, res_x, res_y, res_z, (long long)cells);
    LSE_REQUIRE(occs && aabbs && step_dev && cell_ids && positions && n_dev, "%s: null pointer", what);
    LSE_REQUIRE(warmup || (list && counts), "%s: the sampled branch needs the occupied-cell list", what);
    const int64_t need = warmup ? cells : 2 * (cells / 4);
    LSE_REQUIRE(cap >= need && cap >= 1, "%s: capacity %lld < %lld slots", what, (long long)cap, (long long)need);
    const int64_t threads = std::max<int64_t>(need, 1);
    hipLaunchKernelGGL(draw_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, lse::as_stream(stream),
                       occs, list, counts, aabbs, (int)level, cells, (int)res_x, (int)res_y, (int)res_z, (int)warmup, step_dev,
                       (uint32_t)seed, (uint32_t)(seed >> 32), cap, cell_ids, positions, n_dev);
    return lse::check_launch(what);
}

extern "C" int lse_occ_update_cells_dev(float *occs, const int64_t *cell_ids, const float *sigma, float step_size,
                                        const int64_t *n_dev, int64_t cap, float ema_decay, float *workspace, lse_stream_t stream)
{
    const char *what = "lse_occ_update_cells_dev";
    LSE_REQUIRE(cap >= 0, "%s: cap < 0", what);
    if (cap == 0) return LSE_OK;
    LSE_REQUIRE(occs && cell_ids && sigma && n_dev && workspace, "%s: null pointer", what);
    const unsigned blocks = (unsigned)((cap + 255) / 256);
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(ema_pass1, dim3(blocks), dim3(256), 0, st, (const float *)occs, cell_ids, sigma, step_size, n_dev, cap, ema_decay,
                       workspace);
    hipLaunchKernelGGL(ema_pass2, dim3(blocks), dim3(256), 0, st, occs, cell_ids, n_dev, cap);
    hipLaunchKernelGGL(ema_pass3, dim3(blocks), dim3(256), 0, st, occs, cell_ids, (const float *)workspace, n_dev, cap);
    return lse::check_launch(what);
}

extern "C" int lse_occ_mean_threshold(const float *occs, int64_t n, float occ_thre, double *workspace, float *mean_all,
                                      float *threshold, lse_stream_t stream)
{
    const char *what = "lse_occ_mean_threshold";
    LSE_REQUIRE(n >= 1, "%s: n < 1", what);
    LSE_REQUIRE(occs && workspace && mean_all && threshold, "%s: null pointer", what);
    LSE_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", what);
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(mean_stage1, dim3(LSE_OCC_MEAN_BLOCKS), dim3(kThreads), 0, st, occs, n, workspace);
    hipLaunchKernelGGL(mean_stage2, dim3(1), dim3(kThreads), 0, st, (const double *)workspace, (int)LSE_OCC_MEAN_BLOCKS, n, occ_thre,
                       mean_all, threshold);
    return lse::check_launch(what);
}
