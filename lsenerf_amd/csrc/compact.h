// The ordered compaction of the export and refresh kernels (mesh.hip, pointcloud.hip, events.hip, occ_refresh.hip), written once.
// Items are cut into segments of SEG consecutive items, one wave per segment:
//   rank    segment_rank: ballot + popcount give every kept item its rank inside the segment (-1: dropped) and the segment its
//           count.  (An item that carries a weight instead of 0 / 1 ranks by wave_inclusive_sum_i: events.hip.)
//   scan    block_exclusive_scan, one 256-thread block: segment counts -> exclusive offsets in place, the total to the caller.
//   emit    one thread per item: row = offset of its segment + rank (segment_row); rows at or beyond the capacity are not written
//           (emit_row).
// Fixed grids sized from the extent, no atomics, plain vector stores, no host read: two runs give the same bytes.
#pragma once
#include "common.h"

namespace lse {

constexpr int kScanThreads = 256;             // block size of every kernel that calls block_exclusive_scan
constexpr int kScanWaves = kScanThreads / 64;
constexpr int64_t kMaxCompactItems = 1ll << 40;   // extent limit of check_compaction: segment and block counts stay far inside int

// wave-wide inclusive sum over 64 lanes, T = int or int64_t
template <class T>
__device__ __forceinline__ T wave_inclusive_sum_i(T v)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T n = __shfl_up(v, off, 64);
        if (lane_id() >= off) v += n;
    }
    return v;
}

// lanes below this one with `keep` set; total = lanes of the wave with it set.  Every lane of the wave must call.
__device__ __forceinline__ int wave_prefix_count(bool keep, int &total)
{
    const uint64_t mask = __ballot(keep);
    total = __popcll(mask);
    return __popcll(mask & ((1ull << lane_id()) - 1ull));
}

// Called by every lane of the wave that owns segment `seg`; keep(i) is evaluated once per item i < n, in ascending i per lane.
template <int SEG, class Keep>
__device__ __forceinline__ void segment_rank(int seg, int64_t n, int32_t *__restrict__ rank, int64_t *__restrict__ seg_counts, Keep keep)
{
    const int lane = lane_id();
    int run = 0;
    for (int it = 0; it < SEG / 64; ++it) {
        const int64_t i = (int64_t)seg * SEG + it * 64 + lane;
        const bool valid = i < n;
        const bool k = valid ? keep(i) : false;
        int total;
        const int below = wave_prefix_count(k, total);
        if (valid) rank[i] = k ? run + below : -1;
        run += total;
    }
    if (lane == 0) seg_counts[seg] = run;
}

// Called by every thread of a block of kScanThreads.  t[0, n): counts -> exclusive offsets in place, starting at carry0; returns
// carry0 + the sum of the counts, in every thread.  A 256-element step is summed in Sum, which the caller chooses so that 256 counts
// fit; the carry has its own type.
// A caller that read carry0 from memory may overwrite that location after the call: with n > 0 the loop's barriers lie between every
// thread's read and the write.  With n == 0 there is no barrier, and the only value the function can return is carry0 itself.
template <class Sum, class Elem, class Carry>
__device__ __forceinline__ Carry block_exclusive_scan(Elem *__restrict__ t, int n, Carry carry)
{
    __shared__ Sum wsum[kScanWaves];
    const int w = threadIdx.x >> 6, lane = lane_id();
    for (int c0 = 0; c0 < n; c0 += kScanThreads) {
        const int i = c0 + threadIdx.x;
        const Sum v = i < n ? (Sum)t[i] : 0;
        const Sum inc = wave_inclusive_sum_i(v);
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        Sum woff = 0, sum = 0;
#pragma unroll
        for (int k = 0; k < kScanWaves; ++k) {
            if (k < w) woff += wsum[k];
            sum += wsum[k];
        }
        if (i < n) t[i] = carry + woff + inc - v;
        carry += sum;
        __syncthreads();
    }
    return carry;
}

// output row of the kept item i (rank[i] >= 0)
template <int SEG>
__device__ __forceinline__ int64_t segment_row(int64_t i, const int32_t *__restrict__ rank, const int64_t *__restrict__ seg_off)
{
    return seg_off[i / SEG] + rank[i];
}

// output row of item i, or -1: dropped, or at or beyond the capacity
template <int SEG>
__device__ __forceinline__ int64_t emit_row(int64_t i, const int32_t *__restrict__ rank, const int64_t *__restrict__ seg_off, int64_t cap)
{
    if (rank[i] < 0) return -1;
    const int64_t row = segment_row<SEG>(i, rank, seg_off);
    return row < cap ? row : -1;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
template <int SEG>
inline int n_segments(int64_t items) { return (int)((items + SEG - 1) / SEG); }
inline unsigned blocks_for(int64_t items, int per_block) { return (unsigned)((items + per_block - 1) / per_block); }

// the plain workspace of a compacting entry point: per segment an int64 count / offset, per item an int32 rank
struct CompactWorkspace {
    int64_t *seg;
    int32_t *rank;
    int n_segs;
};

template <int SEG>
inline int64_t compact_workspace_bytes(int64_t items) { return 8 * (int64_t)n_segments<SEG>(items) + 4 * items; }

template <int SEG>
inline CompactWorkspace carve_compact(int64_t items, void *base)
{
    CompactWorkspace w;
    w.n_segs = n_segments<SEG>(items);
    w.seg = static_cast<int64_t *>(base);
    w.rank = base ? reinterpret_cast<int32_t *>(w.seg + w.n_segs) : nullptr;      // (no workspace: an extent of 0)
    return w;
}

// what such an entry point checks about (extent, workspace, cap, total) before it launches anything
template <int SEG>
inline int check_compaction(const char *what, int64_t items, const void *workspace, int64_t workspace_bytes, int64_t cap,
                            const int64_t *total)
{
    LSE_REQUIRE(items >= 0 && items <= kMaxCompactItems, "%s: extent %lld outside [0, 2^40]", what, (long long)items);
    LSE_REQUIRE(cap >= 0, "%s: negative capacity", what);
    LSE_REQUIRE(total && ((uintptr_t)total & 7) == 0, "%s: total must be a non-null, 8-byte aligned device pointer", what);
    if (items == 0) return LSE_OK;
    const int64_t need = compact_workspace_bytes<SEG>(items);
    LSE_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0, "%s: workspace must be a non-null, 8-byte aligned device pointer", what);
    LSE_REQUIRE(workspace_bytes >= need, "%s: workspace of %lld bytes < %lld", what, (long long)workspace_bytes, (long long)need);
    return LSE_OK;
}

}  // namespace lse
