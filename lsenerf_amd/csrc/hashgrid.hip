// Multiresolution hash-grid encoding for gfx950 (tiny-cuda-nn 1.7 `HashGrid` semantics, Linear interpolation,
// F = 2 features per entry) -- the kernels behind `tcnn.Encoding` as built at R:lse_nerf/lse_field.py:72-86 and
// evaluated at R:lse_nerf/lse_field.py:279.
//
// MI355X-first layout decisions
//   * features are produced level-major, y[L][N][2]: a wave writes 64 consecutive float2 (512 contiguous
//     bytes) per level, and the fused MLP reads the same array as MFMA B-operands with full-line loads;
//   * lanes are consecutive samples.  Samples of one ray are consecutive, so at the coarse levels the 64
//     lanes of a gather instruction fall into a handful of cells (same cache lines) and the hardware
//     coalesces them; only the fine hashed levels are true 8-byte random gathers;
//   * forward: one (level, sample-chunk) per workgroup, LEVEL-MAJOR in dispatch order (finest level first): workgroups
//     are dispatched in order and dealt round-robin over the 8 XCDs, so at any time all XCDs work on the same level and
//     each private 4 MiB L2 holds just that 4 MB table.  (Binding whole levels to single XCDs -- blockIdx % 8 -- gives the
//     same locality but the levels cost 0.03 ... 0.10 ms each, and the two XCDs that own two fine levels set the time:
//     0.85 ms against 0.60 ms; tools/hash_fwd_level_cost.py.)  Placement affects speed only, never results.
//   * backward: 16 lanes per sample (one per corner x feature) with run-length pre-accumulation, see hash_bwd_kernel;
//     table gradients are f32 global atomics (memory-side on gfx950, so no level/XCD affinity is attempted there).
//   * backward of a FROZEN table (lse_hash_bwd_input): d(x) alone, the forward's lane mapping with a level loop per workgroup --
//     a gather without atomics, see hash_bwd_input_kernel.
#include "common.h"
#include <stdlib.h>

namespace {

struct GridParams {
    int n_levels;
    int l_begin, l_end;   // backward only: levels [l_begin, l_end) of this launch
    int dx_accumulate;    // backward only: dx += instead of dx = (second launch of a split backward)
    // backward only: the direct (cache-free) adds of levels < rep_levels go to one of rep_mask + 1 replicas of those levels'
    // gradient (workspace, rep_stride floats apart, chosen by the workgroup index) instead of the table gradient itself
    int rep_levels, rep_mask;
    uint32_t rep_stride;
    uint32_t offsets[LSE_MAX_GRID_LEVELS + 1];
    float scales[LSE_MAX_GRID_LEVELS];
    uint32_t res[LSE_MAX_GRID_LEVELS];
};

constexpr uint32_t kPrimeY = 2654435761u;
constexpr uint32_t kPrimeZ = 805459861u;

struct LevelInfo {
    uint32_t offset, size, res;
    float scale;
    bool dense, pow2;
};

__device__ __forceinline__ LevelInfo level_info(const GridParams &g, int l)
{
    LevelInfo li;
    li.offset = g.offsets[l];
    li.size = g.offsets[l + 1] - g.offsets[l];
    li.res = g.res[l];
    li.scale = g.scales[l];
    // tcnn grid_index(): stride loop guarded by stride <= hashmap_size; hash iff hashmap_size < final stride
    // (computed here with scalar instructions: fetching precomputed per-level flags from the kernel arguments was slower)
    uint64_t stride = 1;
    for (int d = 0; d < 3 && stride <= li.size; ++d) stride *= li.res;
    li.dense = !(li.size < stride);
    li.pow2 = (li.size & (li.size - 1)) == 0;
    return li;
}

__device__ __forceinline__ uint32_t grid_index(const LevelInfo &li, uint32_t px, uint32_t py, uint32_t pz)
{
    uint32_t idx;
    if (li.dense) {
        idx = px + py * li.res + pz * li.res * li.res;
        // == idx % size: px,py,pz <= res so idx < 2*res^3 <= 2*size
        if (idx >= li.size) idx -= li.size;
        if (idx >= li.size) idx %= li.size;   // never taken for inputs in [0,1]; keeps the exact modulo otherwise
    } else {
        idx = px ^ (py * kPrimeY) ^ (pz * kPrimeZ);
        idx = li.pow2 ? (idx & (li.size - 1)) : (idx % li.size);
    }
    return idx;
}

// The 8 corner indices of the cell (p0, p1, p2) at once.  Same values as grid_index() per corner (all arithmetic is mod 2^32:
// (p + 1) * prime == p * prime + prime), but the two quarter-rate 32-bit multiplies of the hash are issued once per sample
// instead of once per corner, and a dense level costs one multiply-add pair plus wave-uniform offsets (the per-corner form
// compiles to 16 v_mul_lo_u32 / v_mad_u64_u32 per sample and level, each a 16-cycle instruction on CDNA).
__device__ __forceinline__ void corner_indices(const LevelInfo &li, uint32_t p0, uint32_t p1, uint32_t p2, uint32_t (&idx)[8])
{
    if (li.dense) {
        const uint32_t r2 = li.res * li.res;                       // (scalar)
        const uint32_t b = p0 + p1 * li.res + p2 * r2;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            uint32_t i = b + ((c & 1) ? 1u : 0u) + ((c & 2) ? li.res : 0u) + ((c & 4) ? r2 : 0u);
            if (i >= li.size) i -= li.size;                        // == i % size for inputs in [0,1] (see grid_index)
            if (i >= li.size) i %= li.size;
            idx[c] = i;
        }
    } else {
        const uint32_t hy0 = p1 * kPrimeY, hz0 = p2 * kPrimeZ;
        const uint32_t hy1 = hy0 + kPrimeY, hz1 = hz0 + kPrimeZ;
        const uint32_t h[4] = {hy0 ^ hz0, hy1 ^ hz0, hy0 ^ hz1, hy1 ^ hz1};
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const uint32_t i = (p0 + (c & 1)) ^ h[c >> 1];
            idx[c] = li.pow2 ? (i & (li.size - 1)) : (i % li.size);
        }
    }
}

__device__ __forceinline__ void pos_fract(float x, float scale, float &w, uint32_t &p)
{
    const float pos = fmaf(scale, x, 0.5f);
    const float fl = floorf(pos);
    p = (uint32_t)(int)fl;
    w = pos - fl;
}

constexpr int kFwdThreads = 256;
constexpr int kFwdItems = 4;   // samples per lane -> 32 independent gathers in flight

__global__ __launch_bounds__(kFwdThreads) void hash_fwd_kernel(GridParams g, const float *__restrict__ x,
                                                               const float2 *__restrict__ table,
                                                               float2 *__restrict__ y, int64_t n_cap, int64_t chunks,
                                                               const int64_t *__restrict__ n_dev)
{
    // n_cap: the level stride of y and the sample capacity the grid was sized for; n: the samples that exist (device-side
    // count when one is set: workgroups past it leave at once)
    const int64_t n = lse::clamp_count(n_cap, n_dev);
    // level-major, finest level first (short tail on a cheap level): see the file header
    const int bid = blockIdx.x;
    const int level = g.n_levels - 1 - (int)(bid / chunks);
    const int64_t chunk = bid % chunks;
    const LevelInfo li = level_info(g, level);
    const float2 *__restrict__ tab = table + li.offset;
    const int64_t base = chunk * (int64_t)(kFwdThreads * kFwdItems) + threadIdx.x;
    if (chunk * (int64_t)(kFwdThreads * kFwdItems) >= n) return;

    float w[kFwdItems][3];
    uint32_t p[kFwdItems][3];
    bool valid[kFwdItems];
#pragma unroll
    for (int it = 0; it < kFwdItems; ++it) {
        const int64_t i = base + (int64_t)it * kFwdThreads;
        valid[it] = i < n;
        const int64_t ii = valid[it] ? i : (n - 1);
#pragma unroll
        for (int d = 0; d < 3; ++d) pos_fract(x[ii * 3 + d], li.scale, w[it][d], p[it][d]);
    }
    float2 v[kFwdItems][8];
#pragma unroll
    for (int it = 0; it < kFwdItems; ++it) {
        uint32_t idx[8];
        corner_indices(li, p[it][0], p[it][1], p[it][2], idx);
#pragma unroll
        for (int c = 0; c < 8; ++c) v[it][c] = tab[idx[c]];
    }
#pragma unroll
    for (int it = 0; it < kFwdItems; ++it) {
        float2 r = make_float2(0.f, 0.f);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float wt = 1.f;
            wt *= (c & 1) ? w[it][0] : 1.f - w[it][0];
            wt *= (c & 2) ? w[it][1] : 1.f - w[it][1];
            wt *= (c & 4) ? w[it][2] : 1.f - w[it][2];
            r.x = fmaf(wt, v[it][c].x, r.x);
            r.y = fmaf(wt, v[it][c].y, r.y);
        }
        const int64_t i = base + (int64_t)it * kFwdThreads;
        if (valid[it]) y[(int64_t)level * n_cap + i] = r;
    }
}

// Backward, generic kernel (opts.impl 0, and every grid whose levels do not start on 64-byte lines).  Lane mapping: 16 lanes per
// sample -- lane k of a 16-lane group owns (corner k>>1, feature k&1) -- and a wave owns 4 * kRounds = 128 consecutive samples of
// the packed (ray-sorted) stream, processed in kRounds rounds of 4 samples.
//   * one atomic wave-instruction covers 4 samples x 8 corners x 2 features: the two features of an entry and the
//     x / x+1 corner pair are neighbouring dwords, so the instruction touches far fewer 64-byte lines than lanes
//     (memory-side float atomics are priced per line request, MI355X_MICROARCH.md "Global float atomics"; measured
//     here: identical rate for agent / workgroup / wavefront scope, tools/micro/atomic_scope.hip);
//   * every lane run-length accumulates (index, sum) in registers and only issues an atomic when its entry index
//     changes between consecutive rounds;
//   * group g of a wave walks the samples kRounds * g + r: long runs wherever consecutive samples share a cell.  (Giving a round
//     4 CONSECUTIVE samples instead models ~25 % fewer line requests at the fine levels, tools/sim_hash_bwd_requests.py, and was
//     20 - 80 % slower in hardware: lanes of one instruction then hit the same addresses.  Retired, DESIGN_HISTORY.md.)
//   * positions are staged once per wave in LDS; d(x) is reduced over the 16 lanes of a group and accumulated per sample
//     in LDS by the group's first lane (plain read-add-write: within a round the 4 groups own 4 different samples, rounds
//     are sequential).
constexpr int kRounds = 32;      // rounds of 4 samples per wave of hash_bwd_kernel
template <bool WITH_DX>
__global__ __launch_bounds__(256) void hash_bwd_kernel(GridParams g, const float *__restrict__ x,
                                                       const float *__restrict__ dy,
                                                       const float *__restrict__ table, float *__restrict__ dtable,
                                                       float *__restrict__ dx, int64_t n)
{
    constexpr int kChunk = 4 * kRounds;        // samples per wave
    // SoA + one pad word per 16-lane group: the 4 groups of a wave touch slots kRounds apart, which would otherwise fall
    // into the same LDS bank (4-way conflict on every position read and every d(x) update)
    constexpr int kPitch = kChunk + 4;
    __shared__ float s_x[4][3][kPitch];
    __shared__ float s_dx[4][3][kPitch];
#define LSE_SLOT(sl) ((sl) + (sl) / kRounds)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = lane >> 4, k = lane & 15;
    const int corner = k >> 1, f = k & 1;
    const int64_t wave_base = ((int64_t)blockIdx.x * 4 + wave) * kChunk;
    if (wave_base >= n) return;
#pragma unroll
    for (int c = lane; c < kChunk; c += 64) {
        const int64_t i = wave_base + c;
        const int64_t ii = i < n ? i : n - 1;
        s_x[wave][0][LSE_SLOT(c)] = x[ii * 3 + 0];
        s_x[wave][1][LSE_SLOT(c)] = x[ii * 3 + 1];
        s_x[wave][2][LSE_SLOT(c)] = x[ii * 3 + 2];
        if (WITH_DX) s_dx[wave][0][LSE_SLOT(c)] = s_dx[wave][1][LSE_SLOT(c)] = s_dx[wave][2][LSE_SLOT(c)] = 0.f;
    }
    __builtin_amdgcn_wave_barrier();   // LDS slots are private to this wave; DS ops of a wave execute in order
    const uint32_t cx = corner & 1, cy = (corner >> 1) & 1, cz = (corner >> 2) & 1;
    constexpr uint32_t kNone = 0xFFFFFFFFu;

    for (int l = g.l_begin; l < g.l_end; ++l) {
        const LevelInfo li = level_info(g, l);
        float *__restrict__ dt = dtable + 2 * (size_t)li.offset + f;
        const float *__restrict__ tab = WITH_DX ? table + 2 * (size_t)li.offset + f : nullptr;
        const float *__restrict__ dyl = dy + 2 * (size_t)l * n + f;
        uint32_t cur = kNone;
        float acc = 0.f;
#pragma unroll 4
        for (int r = 0; r < kRounds; ++r) {
            const int sl = kRounds * grp + r;   // sample slot within the wave's chunk
            const bool valid = wave_base + sl < n;
            float w0, w1, w2;
            uint32_t p0, p1, p2;
            const int slot = LSE_SLOT(sl);
            pos_fract(s_x[wave][0][slot], li.scale, w0, p0);
            pos_fract(s_x[wave][1][slot], li.scale, w1, p1);
            pos_fract(s_x[wave][2][slot], li.scale, w2, p2);
            const uint32_t idx = valid ? grid_index(li, p0 + cx, p1 + cy, p2 + cz) : kNone;
            const float sx = cx ? w0 : 1.f - w0, sy = cy ? w1 : 1.f - w1, sz = cz ? w2 : 1.f - w2;
            const int64_t ii = valid ? wave_base + sl : n - 1;
            const float gy = dyl[2 * ii];
            const float v = sx * sy * sz * gy;
            if (idx == cur) {
                acc += v;
            } else {
                if (cur != kNone) atomicAdd(dt + 2 * (size_t)cur, acc);
                cur = idx;
                acc = v;
            }
            if (WITH_DX) {
                const float tv = valid ? tab[2 * (size_t)idx] : 0.f;
                const float t = li.scale * gy * tv;
                float d0 = t * (cx ? 1.f : -1.f) * (sy * sz);
                float d1 = t * (cy ? 1.f : -1.f) * (sx * sz);
                float d2 = t * (cz ? 1.f : -1.f) * (sx * sy);
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) {
                    d0 += __shfl_xor(d0, o, 64);
                    d1 += __shfl_xor(d1, o, 64);
                    d2 += __shfl_xor(d2, o, 64);
                }
                if (k == 0) {
                    s_dx[wave][0][slot] += d0;
                    s_dx[wave][1][slot] += d1;
                    s_dx[wave][2][slot] += d2;
                }
            }
        }
        if (cur != kNone) atomicAdd(dt + 2 * (size_t)cur, acc);
    }
    if (WITH_DX) {
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int c = lane; c < kChunk; c += 64) {
            const int64_t i = wave_base + c;
            if (i < n) {
                const float a0 = g.dx_accumulate ? dx[i * 3 + 0] : 0.f, a1 = g.dx_accumulate ? dx[i * 3 + 1] : 0.f,
                            a2 = g.dx_accumulate ? dx[i * 3 + 2] : 0.f;
                dx[i * 3 + 0] = a0 + s_dx[wave][0][LSE_SLOT(c)];
                dx[i * 3 + 1] = a1 + s_dx[wave][1][LSE_SLOT(c)];
                dx[i * 3 + 2] = a2 + s_dx[wave][2][LSE_SLOT(c)];
            }
        }
    }
#undef LSE_SLOT
}

// Backward with a per-wave LDS cache of table sectors (the default, hash_bwd_batched_kernel below; opts.impl 0 selects the kernel above).
// The 16-lanes-per-sample kernel recomputes the position maths 16x and sends ~19 line requests per sample to the
// memory-side atomic units (it is bound by them: 4.4 ms with, 1.2 ms without the atomics).  Here:
//   * lane = sample (64 consecutive samples of the packed, ray-sorted stream): the position maths, the 8 indices and
//     d(x) are computed once per sample, d(x) needs no cross-lane reduction at all;
//   * consecutive lanes that sit in the same cell form a run; a flag-based segmented scan (DPP inside the 16-lane rows,
//     early exit once no run is longer than the step, serial carry over the 3 row borders) leaves each run's 8 x 2
//     corner sums in the run's last lane;
//   * run ends add into a per-wave LDS cache of table SECTORS (key = entry index >> 2, payload 8 floats = one 32-B
//     sector of 4 entries x 2 features; 512 slots, 1 + second_probe probes): a 32-bit compare-and-swap claims the slot, a 64-bit
//     compare-and-swap adds both features (ds_add_f32 runs at ~3 cycles per LANE on gfx950, tools/micro/lds_ops.hip);
//     a corner whose slot belongs to another sector goes straight to memory, so the cache is purely an optimisation;
//   * after each cache pass the occupied slots (kept in a list) are flushed with one 8-lane x 32-B atomic per sector;
//   * a wave that ends at most `few_runs` (8) runs at a level -- the coarse levels -- skips the cache: the run ends park
//     their 8 indices + 16 sums in LDS and the wave adds them to memory with 16 lanes per run (lane = corner x feature),
//     because the ~500 instructions of the cache path would be spent on idle lanes (levels 0-3: 0.66 -> 0.37 ms).
//   The memory-side atomic units are priced per 32-B sector request at ~20 G/s (rocprof WRITE_SIZE / 32 B tracks the
//   kernel time).  tools/sim_hash_bwd_requests.py models the policy: 256 slots of a 64-B line flush 9.1 sectors per
//   sample and send 4.2 corner updates straight to memory (3.54 ms); 512 sector-sized slots in the same 16 KB collide
//   less: 9.8 + 2.6 (measured 12.3 sector writes per sample, 3.23 ms); writing a collision's two features through a lane
//   pair in one instruction instead of two: 3.05 ms; the few-runs path: 2.91 ms.  The kernel above writes 21 sectors per
//   sample (4.37 ms).  It now sits at the atomic rate for its ~13 requests per sample (2.7 ms); the issue slots
//   (VALU+SALU+LDS ~ 75 % of the SIMD cycles before the last two steps, at the 2 waves/SIMD that 79 KB of LDS allow) are
//   the second bound.  Tried and dropped: more probe rounds (second_probe: neutral), two half-wave phases per fine
//   level, ds_add_f32 payload adds, a slot function linear in the cell coordinates, one probe per x-row.
constexpr uint32_t kNoLine = 0xFFFFFFFFu;

// LDS pointers carry their address space so that every cache access is a ds_* instruction (generic pointers make the
// compiler fold the LDS and the global fall-back path into flat atomics).
typedef __attribute__((address_space(3))) uint32_t lds_u32;
typedef __attribute__((address_space(3))) uint16_t lds_u16;
typedef __attribute__((address_space(3))) float lds_f32;
typedef __attribute__((address_space(3))) uint64_t lds_u64;

// relaxed LDS compare-and-swap returning the previous value (no ordering fences: DS ops of a wave execute in order)
__device__ __forceinline__ uint32_t lds_cas(lds_u32 *p, uint32_t expect, uint32_t desired)
{
    __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return expect;
}
__device__ __forceinline__ uint64_t lds_cas(lds_u64 *p, uint64_t expect, uint64_t desired)
{
    __hip_atomic_compare_exchange_strong(p, &expect, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    return expect;
}

__device__ __forceinline__ uint64_t add_pair(uint64_t bits, float a0, float a1)
{
    const float lo = __uint_as_float((uint32_t)bits) + a0, hi = __uint_as_float((uint32_t)(bits >> 32)) + a1;
    return (uint64_t)__float_as_uint(lo) | ((uint64_t)__float_as_uint(hi) << 32);
}

// Row-local DPP shift: lane i receives the value of lane i-OFF of its 16-lane row, 0 if that lane is outside the row.
template <int OFF>
__device__ __forceinline__ float row_shr_f32(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x110 + OFF, 0xF, 0xF, true));
}
template <int OFF>
__device__ __forceinline__ int row_shr_i32(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, 0x110 + OFF, 0xF, 0xF, true);
}

// Whole-wave shifts by one lane as DPP moves (GFX9 wave_shr / wave_shl): `__shfl_up(v, 1)` compiles to ds_bpermute_b32, an LDS
// instruction, and the hash backward is bound by the LDS pipe.  Lane 0 (63) receives its own value; callers test the lane.
__device__ __forceinline__ uint32_t wave_shr1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xF, 0xF, false); }
__device__ __forceinline__ int wave_shl1(int v) { return __builtin_amdgcn_update_dpp(v, v, 0x130, 0xF, 0xF, false); }

// lane <-> lane^1 exchange (DPP quad_perm [1,0,3,2])
__device__ __forceinline__ int quad_swap1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, true); }

// acc += (value of acc in the lane OFF below, same 16-lane row; 0 outside the row) * mul -- one fused DPP instruction
// (the compiler emits v_mov_b32_dpp + v_fma for the builtin form).  The s_nop covers the "VALU write -> DPP read" wait
// states for the first value of a step; the 16 values of a step are independent of each other.
#define LSE_FMAC_DPP(acc, mul, CTRL) asm volatile("v_fmac_f32_dpp %0, %0, %1 " CTRL : "+v"(acc) : "v"(mul))

// One step of the flag-based segmented inclusive scan inside the 16-lane rows.
// Returns false (wave-uniform) when no lane needs this or any later step.
template <int OFF>
__device__ __forceinline__ bool seg_scan_row_step(float (&v)[16], int &flag, int row_pos)
{
    const bool need = !flag && row_pos >= OFF;
    if (__builtin_amdgcn_ballot_w64(need) == 0) return false;
    const float nf = need ? 1.f : 0.f;
    const int fo = row_shr_i32<OFF>(flag);
    asm volatile("s_nop 1");
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (OFF == 1) LSE_FMAC_DPP(v[k], nf, "row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:1");
        if (OFF == 2) LSE_FMAC_DPP(v[k], nf, "row_shr:2 row_mask:0xf bank_mask:0xf bound_ctrl:1");
        if (OFF == 4) LSE_FMAC_DPP(v[k], nf, "row_shr:4 row_mask:0xf bank_mask:0xf bound_ctrl:1");
        if (OFF == 8) LSE_FMAC_DPP(v[k], nf, "row_shr:8 row_mask:0xf bank_mask:0xf bound_ctrl:1");
    }
    flag |= need ? fo : 0;
    return true;
}

// Carry of the row-local scans across the three row borders: rows 1 and 3 take the last lane of rows 0 and 2
// (row_bcast:15), then rows 2 and 3 take lane 31 (row_bcast:31), each lane only while its run reaches back that far.
// open = "no run head between my row's first lane and me".
__device__ __forceinline__ void seg_scan_cross_rows(float (&v)[16], int open, int lane)
{
    const int row = lane >> 4;
    if (__builtin_amdgcn_ballot_w64(open && row != 0) == 0) return;
    const float fa = (open && (row & 1)) ? 1.f : 0.f;
    int open47 = open;       // rows 1, 3 receive open(lane 15), open(lane 47)
    asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(open47));
#pragma unroll
    for (int k = 0; k < 16; ++k) LSE_FMAC_DPP(v[k], fa, "row_bcast:15 row_mask:0xa bank_mask:0xf");
    const float fb = (row == 2 ? open : (row == 3 ? (open && open47) : 0)) ? 1.f : 0.f;
    asm volatile("s_nop 1");
#pragma unroll
    for (int k = 0; k < 16; ++k) LSE_FMAC_DPP(v[k], fb, "row_bcast:31 row_mask:0xc bank_mask:0xf");
}

// The batched sector-cache kernel (the default, opts.impl 2): the design above, with the run ends of SEVERAL levels sharing one cache pass.
// Paired sectors: the memory-side units charge a float-atomic REQUEST per 64-byte LINE, whatever part of it the request covers
// (tools/micro/atomic_gran.hip: 21 G requests/s for 4 ... 64 contiguous bytes, half of that for 128).  With 32-byte slots a line
// whose two sectors were both touched would be flushed as two requests, so the LINE is hashed to a pair of neighbouring slots (even /
// odd sector) and the flush list is built by scanning the keys in slot order: sibling sectors sit in neighbouring 8-lane groups of
// one flush instruction and go out as ONE contiguous 64-byte request; the scan also replaces per-corner list appends in the insert path.
// Second-generation flush: the kernel is bound by the CU's LDS pipe -- every DS wave-instruction costs 7 .. 8 cycles of it (13 / 22
// for the 32- / 64-bit compare-and-swap; profiles/r02_micro_lds_ops.txt) -- so the flush is written for few DS instructions: the list
// is stored trip-major transposed, so the 4 slots a lane group handles in a trip are one 8-byte read; the payload is read AND zeroed
// by one ds_wrxchg_rtn_b32; the keys are reset in bulk after the last trip (2 x ds_write_b128 per lane).  Per 32 slots: 1 + 4 + 4 = 9
// DS instructions (a list read, key read, payload read, payload reset and key reset per slot took 20).
// One wave per workgroup: nothing below synchronises across waves (every wave owns its cache), so the workgroup size only sets the
// granularity at which LDS is handed out and released.  A workgroup's LDS is released when its last wave retires, and waves differ in
// how many cache passes their samples need: in workgroups of four a CU held 20 KB per early finisher idle (samples in the contracted
// shell 2.53 -> 2.40 ms, headline, M-packed and the default configuration within +-1 %: profiles/r05_hash_bwd_workgroup_size.txt).
// Retired variants of this kernel (DESIGN_HISTORY.md; last present in commit eb3e47d):
//   * one cache pass per level, with 256 slots of a 64-byte line or 512 unpaired sectors: 3.54 / 3.23 ms, 2.91 with the few-runs
//     path, where batching the levels reached 2.7 (the comment above; no profile file was kept);
//   * paired slots with the first-generation flush: 2.75 against 2.71 ms (profiles/r04_hash_bwd_defaults_recheck.txt, gran 4);
//   * the next level's operands fetched ahead of the cache pass: +-0 (profiles/r03_hash_bwd_prefetch.txt, r05_hash_bwd_prefetch_retest.txt);
//   * pair-aligned flush lists: identical request counts, 2 - 3 % slower (profiles/r03_hash_bwd_aligned_pairs.txt);
//   * 256 / 320 / 384 / 448 slots and workgroups of 2 / 4 waves: flat or slower (profiles/r05_hash_bwd_slots320.txt,
//     r05_hash_bwd_workgroup_size.txt);
//   * a cache-free high-occupancy kernel for the coarse levels: +-2 % (profiles/r03_hash_bwd_coarse_kernel_attribution.txt).
template <bool WITH_DX>
__global__ __launch_bounds__(64) void hash_bwd_batched_kernel(GridParams g, const float *__restrict__ x,
                                                              const float2 *__restrict__ dy,
                                                              const float2 *__restrict__ table,
                                                              float *__restrict__ dtable, float *__restrict__ dx,
                                                              int64_t n_cap, int few_runs, int second_probe, int stage_max,
                                                              float *__restrict__ ws, const int64_t *__restrict__ n_dev)
{
    const int64_t n = lse::clamp_count(n_cap, n_dev);      // n_cap stays the level stride of dy
    constexpr int kSlots = 512;                // cache slots per wave
    constexpr int kEntLog2 = 2;
    constexpr int kEnt = 1 << kEntLog2;        // table entries per cache slot (4 = one 32-B sector)
    constexpr int kPay = 2 * kEnt;             // payload floats per slot = lanes per slot in the flush
    constexpr int kSlotBits = 31 - __builtin_clz((unsigned)kSlots);
    constexpr int kWaves = 1;                  // waves per workgroup (the launch bound above)
    constexpr int kChunk = 64;                 // samples per wave: lane = sample
    static_assert(kPay == 8 && kSlots == 512, "flush: 8 lanes per slot, bulk key reset of 8 keys per lane");
    __shared__ uint32_t s_key[kWaves][kSlots];
    __shared__ float s_val[kWaves][kSlots * kPay];
    __shared__ uint16_t s_list[kWaves][kSlots];      // occupied slots
    __shared__ uint32_t s_dummy32[kWaves][64];
    __shared__ uint64_t s_dummy64[kWaves][64];
    __shared__ uint32_t s_perm[kWaves][64];          // rank -> lane of the run ends being staged
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    // Which 64-sample chunks a workgroup takes.  The hardware deals workgroups round-robin to the 8 XCDs, so with the identity
    // mapping XCD x gets the chunks c = x (mod 8) -- and in ray-ordered samples the cost of a chunk depends on where on its ray it
    // lies (dense cells near the camera, long runs in the contracted shell): with 1024 samples per ray XCD x saw the chunks x and
    // x + 8 of EVERY ray, a static load imbalance between XCDs.  Workgroup b therefore takes position (b % 8) * ceil(B / 8) + b / 8
    // of the B positions the samples actually fill (device-side count: a captured step's capacity is larger): every XCD walks one
    // contiguous eighth, i.e. whole rays whatever their length.  Inside-box rays 2.39 -> 2.19 ms, the reference's default
    // configuration 1.51 -> 1.47, headline +-0.3 % (profiles/r05_hash_bwd_xcd_mapping.txt).
    int64_t wg = blockIdx.x;
    const int64_t positions = (n + (int64_t)kChunk * kWaves - 1) / ((int64_t)kChunk * kWaves);
    const int64_t per_xcd = (positions + 7) >> 3;
    if ((wg >> 3) >= per_xcd) return;      // (the grid covers the capacity, rounded up to a multiple of 8)
    wg = (wg & 7) * per_xcd + (wg >> 3);
    const int64_t wave_base = (wg * kWaves + wave) * kChunk;
    if (wave_base >= n) return;
    lds_u32 *key = (lds_u32 *)&s_key[wave][0];
    lds_f32 *val = (lds_f32 *)&s_val[wave][0];
    lds_u16 *list = (lds_u16 *)&s_list[wave][0];
    lds_u32 *dummy32 = (lds_u32 *)&s_dummy32[wave][lane];
    lds_u64 *dummy64 = (lds_u64 *)&s_dummy64[wave][lane];
    lds_u32 *perm = (lds_u32 *)&s_perm[wave][0];
    *dummy32 = kNoLine;
    *dummy64 = 0;
    for (int s = lane; s < kSlots; s += 64) key[s] = kNoLine;
    for (int s = lane; s < kSlots * kPay; s += 64) val[s] = 0.f;

    const int64_t i = wave_base + lane;
    const bool valid = i < n;
    const int64_t si = valid ? i : n - 1;
    float px[3], dacc[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        px[d] = x[si * 3 + d];
        dacc[d] = 0.f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // the cache is private to this wave; DS ops of a wave execute in order

    // ---- register queue of run ends waiting for a cache pass: lane t < fill holds one run end (8 GLOBAL entry indices =
    // level offset + index inside the level, and its 8 x 2 corner sums).  Cache keys are global sector ids, so run ends of
    // several levels share one pass: the insert + flush below costs ~0.1 ms per pass at the metric size however few lanes
    // take part (measured: 1.5 of the kernel's 2.9 ms), and the levels 4 .. 9 end only 5 .. 15 runs per wave each.
    uint32_t q_idx[8];
    float q_v[16];
#pragma unroll
    for (int c = 0; c < 8; ++c) q_idx[c] = 0u;
#pragma unroll
    for (int k = 0; k < 16; ++k) q_v[k] = 0.f;
    int fill = 0;

    auto insert_pass = [&](const bool act, const uint32_t (&gi)[8], const float (&vv)[16]) {
        uint32_t used = 0;   // occupied cache slots (wave-uniform)
        if (__builtin_amdgcn_ballot_w64(act) != 0) {
            // multiplicative hash of the LINE id picks the pair bucket, the sector's parity the slot inside it (a slot function
            // linear in the cell coordinates was tried: more collisions on ray-shaped line sets, tools/sim_hash_bwd_requests.py)
            uint32_t slot[8], old[8];
#pragma unroll
            for (int c = 0; c < 8; ++c)
                slot[c] = (((__umul24(gi[c] >> (kEntLog2 + 1), 0x9E3779u) >> (25 - kSlotBits)) & (kSlots / 2 - 1)) << 1) |
                          ((gi[c] >> kEntLog2) & 1u);
            uint32_t keyc[8];      // the sector a corner belongs to = the cache key
#pragma unroll
            for (int c = 0; c < 8; ++c) keyc[c] = gi[c] >> kEntLog2;
#pragma unroll
            for (int c = 0; c < 8; ++c)
                old[c] = lds_cas(act ? &key[slot[c]] : dummy32, kNoLine, act ? keyc[c] : kNoLine);
            // float LDS atomics run at ~3 cycles per LANE on gfx950 (tools/micro/lds_ops.hip: ds_add_f32 194 cycles
            // per instruction, ds_cmpst_b64 22): add both features with one 64-bit compare-and-swap
            lds_u64 *va[8];
            // ONE piece of state per corner: to_mem = "active and not (yet) at home in a slot", updated with selects (a second
            // array and exec-masked update blocks cost ~300 instructions per probe round, half of them scalar mask bookkeeping;
            // selects on one mask per corner need ~90)
            bool to_mem[8];
            uint64_t cur[8], prev[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const bool home = (old[c] == kNoLine) || (old[c] == keyc[c]);      // claimed the slot, or found its own sector there
                to_mem[c] = act && !home;
            }
            for (int pr = 0; pr < second_probe; ++pr) {
                // another chance in the next slot of the same parity for the corners that lost the previous one (batched the same
                // way); a loser keeps its home slot, so round pr probes home + 2 * (pr + 1)
                bool any = false;
#pragma unroll
                for (int c = 0; c < 8; ++c) any = any || to_mem[c];
                // rounds after the first only when at least 8 lanes still hold a loser: a round costs the whole wave its
                // instructions whatever the number of losers, and where the kernel is bound by its own instructions (samples in
                // the contracted shell: 2.57 -> 2.71 ms with unconditional rounds, 2.66 with the threshold) a handful of direct adds
                // is cheaper; the atomic-bound regimes keep their gain (default configuration 1.51 -> 1.48 ms either way)
                const int min_losers = pr == 0 ? 1 : 8;
                if (__builtin_popcountll(__builtin_amdgcn_ballot_w64(any)) >= min_losers) {
                    uint32_t old2[8], nxt[8];
                    const uint32_t hop = (uint32_t)(pr + 1) * 2;
#pragma unroll
                    for (int c = 0; c < 8; ++c) nxt[c] = (slot[c] + hop) & (uint32_t)(kSlots - 1);
#pragma unroll
                    for (int c = 0; c < 8; ++c)
                        old2[c] = lds_cas(to_mem[c] ? &key[nxt[c]] : dummy32, kNoLine, to_mem[c] ? keyc[c] : kNoLine);
#pragma unroll
                    for (int c = 0; c < 8; ++c) {
                        const bool won = to_mem[c] && ((old2[c] == kNoLine) || (old2[c] == keyc[c]));
                        slot[c] = won ? nxt[c] : slot[c];
                        to_mem[c] = to_mem[c] && !won;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                // address for every lane, then ONE select (left to itself the compiler guards each address with its own
                // exec-masked block: 29 s_and_saveexec + 17 branches for the eight corners)
                uint32_t home_p = (uint32_t)(uintptr_t)(lds_u64 *)&val[slot[c] * kPay + (gi[c] & (kEnt - 1)) * 2];
                asm volatile("" : "+v"(home_p));
                va[c] = (act && !to_mem[c]) ? (lds_u64 *)(uintptr_t)home_p : dummy64;
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) cur[c] = *va[c];
#pragma unroll
            for (int c = 0; c < 8; ++c) prev[c] = lds_cas(va[c], cur[c], add_pair(cur[c], vv[2 * c], vv[2 * c + 1]));
            bool retry = false;
#pragma unroll
            for (int c = 0; c < 8; ++c) retry = retry || prev[c] != cur[c];
            if (__builtin_amdgcn_ballot_w64(retry) != 0) {   // rare: two lanes (or two corners of a lane) on one entry
#pragma unroll
                for (int c = 0; c < 8; ++c)
                    while (prev[c] != cur[c]) {
                        cur[c] = prev[c];
                        prev[c] = lds_cas(va[c], cur[c], add_pair(cur[c], vv[2 * c], vv[2 * c + 1]));
                    }
            }
            // Corners whose slot is owned by another sector go straight to memory.  The two features of an entry are
            // written by a PAIR of lanes in one instruction (lane and lane^1 swap operands through DPP), so the
            // 8 bytes cost one request to the atomic units instead of two.
            const bool is_odd = lane & 1;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                if (__builtin_amdgcn_ballot_w64(to_mem[c]) == 0) continue;
                const uint32_t gi_n = (uint32_t)quad_swap1((int)gi[c]);
                const float v0_n = __int_as_float(quad_swap1(__float_as_int(vv[2 * c])));
                const float v1_n = __int_as_float(quad_swap1(__float_as_int(vv[2 * c + 1])));
                const bool tm_n = quad_swap1((int)to_mem[c]) != 0;
                // first instruction serves the even lanes' corners, second one the odd lanes'
                if (is_odd ? tm_n : to_mem[c]) atomicAdd(dtable + 2 * (size_t)(is_odd ? gi_n : gi[c]) + is_odd, is_odd ? v1_n : vv[2 * c]);
                if (is_odd ? to_mem[c] : tm_n) atomicAdd(dtable + 2 * (size_t)(is_odd ? gi[c] : gi_n) + is_odd, is_odd ? vv[2 * c + 1] : v0_n);
            }
        }
        // flush list: the occupied slots in slot order, so that sibling sectors of a line become list neighbours
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int s0 = 0; s0 < kSlots; s0 += 64) {
            const bool occ = key[s0 + lane] != kNoLine;
            const uint64_t om = __builtin_amdgcn_ballot_w64(occ);
            if (occ) {
                uint32_t pos = used + __builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)om, 0));
                // trip-major transposed: list position i of trip i / 32 is handled by lane group i % 8 as its (i % 32) / 8-th slot
                pos = (pos & ~31u) + ((pos & 7u) << 2) + ((pos >> 3) & 3u);
                list[pos] = (uint16_t)(s0 + lane);
            }
            used += __builtin_popcountll(om);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // flush: 8 lanes per sector, 8 sectors per instruction, 32 per trip
        const int sub = lane & (kPay - 1);
        const uint32_t gq = (uint32_t)lane >> 3;
        for (uint32_t t0 = 0; t0 < used; t0 += 32) {
            const uint64_t four = *(lds_u64 *)&list[t0 + 4 * gq];
            uint32_t sl[4], ln[4];
            float fv[4];
            bool ok[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t e = (uint32_t)(four >> (16 * u)) & 0xFFFFu;
                ok[u] = t0 + 8 * u + gq < used;
                sl[u] = ok[u] ? e : (uint32_t)lane;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) ln[u] = key[sl[u]];
#pragma unroll
            for (int u = 0; u < 4; ++u)       // read + zero in one DS instruction; idle lanes swap their private dummy word
                fv[u] = __hip_atomic_exchange(ok[u] ? &val[sl[u] * kPay + sub] : (lds_f32 *)dummy32, 0.f, __ATOMIC_RELAXED,
                                              __HIP_MEMORY_SCOPE_WAVEFRONT);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (ok[u] && fv[u] != 0.f) atomicAdd(dtable + (size_t)ln[u] * kPay + sub, fv[u]);
        }
        if (used) {      // every occupied key was in the list: reset all of them, 8 keys per lane
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) u32x4_t lds_u32x4;
            lds_u32x4 *k4 = (lds_u32x4 *)key;
            const u32x4_t none = {kNoLine, kNoLine, kNoLine, kNoLine};
            k4[lane] = none;
            k4[64 + lane] = none;
            *dummy32 = kNoLine;      // (the exchange above left 0.f in the idle lanes' dummy word)
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };

    for (int l = g.l_begin; l < g.l_end; ++l) {
        const LevelInfo li = level_info(g, l);
        // (few-runs path only)  The coarsest levels are a few thousand lines that every wave of the launch adds to: the
        // memory-side units serialise same-line requests (M-packed: 5 % of the kernel's requests, 0.6 of its 3.6 ms), so
        // those adds go to one of several replicas of the level, picked by the index of the wave's group of four, and
        // hash_bwd_reduce_replicas_kernel folds the replicas into the table gradient afterwards
        float *__restrict__ dt = (ws != nullptr && l < g.rep_levels)
                                     ? ws + (size_t)((blockIdx.x * kWaves / 4) & (unsigned)g.rep_mask) * g.rep_stride + 2 * (size_t)li.offset
                                     : dtable + 2 * (size_t)li.offset;
        const float2 *__restrict__ tab = table + li.offset;
        float w0, w1, w2;
        uint32_t p0, p1, p2;
        uint32_t idx[8];
        float2 tv[8];
        pos_fract(px[0], li.scale, w0, p0);
        pos_fract(px[1], li.scale, w1, p1);
        pos_fract(px[2], li.scale, w2, p2);
        float2 gy = dy[(int64_t)l * n_cap + si];
        corner_indices(li, p0, p1, p2, idx);
        if (WITH_DX) {
#pragma unroll
            for (int c = 0; c < 8; ++c) tv[c] = tab[idx[c]];
        }
        if (!valid) gy = make_float2(0.f, 0.f);
        // runs of lanes in the same cell
        const uint32_t q0 = wave_shr1(p0), q1 = wave_shr1(p1), q2 = wave_shr1(p2);
        const int head = (lane == 0) || (q0 != p0) || (q1 != p1) || (q2 != p2);
        const int next_head = wave_shl1(head);
        const bool run_end = (lane == 63) || next_head;
        float v[16];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float wt = ((c & 1) ? w0 : 1.f - w0) * ((c & 2) ? w1 : 1.f - w1) * ((c & 4) ? w2 : 1.f - w2);
            v[2 * c] = wt * gy.x;
            v[2 * c + 1] = wt * gy.y;
        }
        // segmented inclusive scan: inside the 16-lane rows with DPP, then a serial carry across the 3 row borders
        const int row_pos = lane & 15;
        int flag = head | (row_pos == 0);   // "my partial sum already starts at my run's head (or my row's start)"
        if (seg_scan_row_step<1>(v, flag, row_pos) && seg_scan_row_step<2>(v, flag, row_pos) &&
            seg_scan_row_step<4>(v, flag, row_pos))
            seg_scan_row_step<8>(v, flag, row_pos);
        // `open` = no run head between my row's first lane and me (inclusive): my run continues from the row before
        int open = !head;
#pragma unroll
        for (int off = 1; off < 16; off <<= 1) {
            const int o = (off == 1) ? row_shr_i32<1>(open) : (off == 2) ? row_shr_i32<2>(open)
                        : (off == 4) ? row_shr_i32<4>(open) : row_shr_i32<8>(open);
            open &= (row_pos >= off) ? o : 1;
        }
        seg_scan_cross_rows(v, open, lane);
        if (WITH_DX) {
            // d(x): t_c = <dy, table[c]>; along each axis the difference of the two faces, weighted by the other two axes
            const float a0 = 1.f - w0, a1 = 1.f - w1, a2 = 1.f - w2;
            float t[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) t[c] = gy.x * tv[c].x + gy.y * tv[c].y;
            const float d0 = a2 * (a1 * (t[1] - t[0]) + w1 * (t[3] - t[2])) + w2 * (a1 * (t[5] - t[4]) + w1 * (t[7] - t[6]));
            const float d1 = a2 * (a0 * (t[2] - t[0]) + w0 * (t[3] - t[1])) + w2 * (a0 * (t[6] - t[4]) + w0 * (t[7] - t[5]));
            const float d2 = a1 * (a0 * (t[4] - t[0]) + w0 * (t[5] - t[1])) + w1 * (a0 * (t[6] - t[2]) + w0 * (t[7] - t[3]));
            dacc[0] = fmaf(li.scale, d0, dacc[0]);
            dacc[1] = fmaf(li.scale, d1, dacc[1]);
            dacc[2] = fmaf(li.scale, d2, dacc[2]);
        }
        // ---- run ends add their 8 corner sums into the sector cache, or straight to memory where the wave ends only a few.
        // The kernel is instruction-issue bound (rocprof: VALU+SALU+LDS issue ~ 3 ms of a 3.6 ms launch), so this part
        // is written for few instructions: every DS operation is issued by all lanes (idle lanes aim at a private dummy
        // word) so that a batch of 8 goes out back to back with one wait.
        const uint64_t ends_mask = __builtin_amdgcn_ballot_w64(run_end);
        const int n_ends = __builtin_popcountll(ends_mask);
        if (n_ends <= few_runs) {
            // Coarse levels: a wave ends only a handful of runs, and almost all of the ~500 instructions of the cache
            // path below would be spent on idle lanes.  Instead the run ends park their 8 indices + 16 sums in LDS
            // (the zeroed payload area doubles as staging) and the wave re-reads them with 16 lanes per run -- lane =
            // (corner, feature), 4 runs per instruction -- and adds straight to memory: the two features and the
            // x / x+1 neighbours of an entry share requests inside the instruction.
            if (n_ends > 0) {
                lds_u32 *stage = (lds_u32 *)val;           // [run][8 idx | 16 values]
                if (run_end) {
                    const int rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(ends_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ends_mask, 0));
#pragma unroll
                    for (int c = 0; c < 8; ++c) stage[rank * 24 + c] = idx[c];
#pragma unroll
                    for (int k = 0; k < 16; ++k) stage[rank * 24 + 8 + k] = __float_as_uint(v[k]);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int k16 = lane & 15;
                for (int r0 = lane >> 4; r0 < n_ends; r0 += 4) {
                    const uint32_t e = stage[r0 * 24 + (k16 >> 1)];
                    const float a = __uint_as_float(stage[r0 * 24 + 8 + k16]);
                    if (a != 0.f) atomicAdd(dt + 2 * (size_t)e + (k16 & 1), a);
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                for (int s_ = lane; s_ < n_ends * 24; s_ += 64) stage[s_] = 0u;   // the payload area must read zero again
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
        } else {
            uint32_t gidx[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) gidx[c] = li.offset + idx[c];
            if (fill + n_ends > 64) {               // the queue cannot take this level: run the pending pass first
                insert_pass(lane < fill, q_idx, q_v);
                fill = 0;
            }
            if (fill == 0 && n_ends > stage_max) {
                // fine level: most lanes end a run -- pass straight from the lanes that hold them (no compaction)
                insert_pass(run_end, gidx, v);
            } else {
                // append: queue lane fill + r takes the r-th run end of this level (rank -> lane through LDS, then 24
                // ds_bpermute moves); the pass runs when the queue is full, at a fine level, or after the last level
                if (run_end)
                    perm[__builtin_amdgcn_mbcnt_hi((uint32_t)(ends_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)ends_mask, 0))] = (uint32_t)lane;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                __builtin_amdgcn_wave_barrier();
                const int r = lane - fill;
                const bool take = r >= 0 && r < n_ends;
                const int src = take ? (int)perm[r] : lane;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const uint32_t t = (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)gidx[c]);
                    q_idx[c] = take ? t : q_idx[c];
                }
#pragma unroll
                for (int k2 = 0; k2 < 16; ++k2) {
                    const float t = __int_as_float(__builtin_amdgcn_ds_bpermute(src << 2, __float_as_int(v[k2])));
                    q_v[k2] = take ? t : q_v[k2];
                }
                fill += n_ends;
                __builtin_amdgcn_wave_barrier();
            }
        }
    }
    if (fill > 0) insert_pass(lane < fill, q_idx, q_v);
    if (WITH_DX && valid) {
        if (g.dx_accumulate) {
            dacc[0] += dx[si * 3 + 0];
            dacc[1] += dx[si * 3 + 1];
            dacc[2] += dx[si * 3 + 2];
        }
        dx[si * 3 + 0] = dacc[0];
        dx[si * 3 + 1] = dacc[1];
        dx[si * 3 + 2] = dacc[2];
    }
}

// dtable[i] += sum over replicas; the workspace reads zero again afterwards (it is handed over zeroed and returned zeroed)
__global__ __launch_bounds__(256) void hash_bwd_reduce_replicas_kernel(float *__restrict__ ws, float *__restrict__ dtable,
                                                                       uint32_t n4, int n_rep, uint32_t stride)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = 0; r < n_rep; ++r) {
        float4 *p = reinterpret_cast<float4 *>(ws + (size_t)r * stride) + i;
        const float4 v = *p;
        if (v.x != 0.f || v.y != 0.f || v.z != 0.f || v.w != 0.f) {
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
            *p = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    if (s.x != 0.f || s.y != 0.f || s.z != 0.f || s.w != 0.f) {
        float4 *d = reinterpret_cast<float4 *>(dtable) + i;
        float4 t = *d;
        t.x += s.x; t.y += s.y; t.z += s.z; t.w += s.w;
        *d = t;
    }
}

// Input-only backward (frozen table): dx[i] = sum_l sum_f dy[l][i][f] * d y[l][i][f] / d x[i], nothing else.  A pure gather -- no
// table gradient, no atomics, no LDS -- with the forward's lane mapping (lane = sample, kFwdItems samples per lane, so 32 gathers
// are in flight per lane) and the forward's cell (pos_fract, corner_indices: out-of-range positions wrap the same way).
// Schedule: ONE pass; a workgroup owns kFwdThreads * kFwdItems samples, walks the levels 0 .. L-1 and keeps the three sums in
// registers, so dx is written once and the level order of the sum is fixed (two runs give the same bits).  The workgroups drift
// apart, so an XCD's L2 serves several level tables at once and the fine levels come from the Infinity Cache: 0.60 / 0.70 ms for
// 4096 x 1024 samples (inside-box / sphere rays) against the forward's 0.44 / 0.48.  That gather traffic is the bound -- 1 to 4
// samples per lane (2 to 8 waves per SIMD) and a factored form with half the multiply-adds all land within 3 % on the sphere rays.
// The forward's level-major dispatch keeps each L2 on one table but has to write per-level partial dx and sum them in a second
// pass: 0.93 / 0.96 ms, dropped (DESIGN_HISTORY.md).
__global__ __launch_bounds__(kFwdThreads) void hash_bwd_input_kernel(GridParams g, const float *__restrict__ x,
                                                                     const float2 *__restrict__ dy,
                                                                     const float2 *__restrict__ table, float *__restrict__ dx,
                                                                     int64_t n_cap, const int64_t *__restrict__ n_dev)
{
    const int64_t n = lse::clamp_count(n_cap, n_dev);      // n_cap stays the level stride of dy
    const int64_t base = (int64_t)blockIdx.x * (kFwdThreads * kFwdItems) + threadIdx.x;
    if ((int64_t)blockIdx.x * (kFwdThreads * kFwdItems) >= n) return;

    float px[kFwdItems][3], acc[kFwdItems][3];
    int64_t si[kFwdItems];
    bool valid[kFwdItems];
#pragma unroll
    for (int it = 0; it < kFwdItems; ++it) {
        const int64_t i = base + (int64_t)it * kFwdThreads;
        valid[it] = i < n;
        si[it] = valid[it] ? i : (n - 1);
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            px[it][d] = x[si[it] * 3 + d];
            acc[it][d] = 0.f;
        }
    }
    for (int l = 0; l < g.n_levels; ++l) {
        const LevelInfo li = level_info(g, l);
        const float2 *__restrict__ tab = table + li.offset;
        const float2 *__restrict__ dyl = dy + (int64_t)l * n_cap;
        float w[kFwdItems][3];
        float2 gy[kFwdItems], v[kFwdItems][8];
#pragma unroll
        for (int it = 0; it < kFwdItems; ++it) {
            uint32_t p[3], idx[8];
#pragma unroll
            for (int d = 0; d < 3; ++d) pos_fract(px[it][d], li.scale, w[it][d], p[d]);
            corner_indices(li, p[0], p[1], p[2], idx);
#pragma unroll
            for (int c = 0; c < 8; ++c) v[it][c] = tab[idx[c]];
            gy[it] = dyl[si[it]];
        }
#pragma unroll
        for (int it = 0; it < kFwdItems; ++it) {
            const float w0 = w[it][0], w1 = w[it][1], w2 = w[it][2];
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const float sx = (c & 1) ? w0 : 1.f - w0, sy = (c & 2) ? w1 : 1.f - w1, sz = (c & 4) ? w2 : 1.f - w2;
                const float t = gy[it].x * v[it][c].x + gy[it].y * v[it][c].y;
                d0 += ((c & 1) ? t : -t) * (sy * sz);
                d1 += ((c & 2) ? t : -t) * (sx * sz);
                d2 += ((c & 4) ? t : -t) * (sx * sy);
            }
            acc[it][0] += li.scale * d0;
            acc[it][1] += li.scale * d1;
            acc[it][2] += li.scale * d2;
        }
    }
#pragma unroll
    for (int it = 0; it < kFwdItems; ++it)
        if (valid[it]) {
            dx[si[it] * 3 + 0] = acc[it][0];
            dx[si[it] * 3 + 1] = acc[it][1];
            dx[si[it] * 3 + 2] = acc[it][2];
        }
}

int fill_params(const lse_grid_desc *desc, GridParams &g, const char *who)
{
    LSE_REQUIRE(desc, "%s: null desc", who);
    LSE_REQUIRE(desc->n_levels >= 1 && desc->n_levels <= LSE_MAX_GRID_LEVELS, "%s: n_levels %d out of range", who,
                desc->n_levels);
    LSE_REQUIRE(desc->n_features == 2, "%s: only n_features == 2 is implemented (got %d)", who, desc->n_features);
    g.n_levels = desc->n_levels;
    g.l_begin = 0;
    g.l_end = desc->n_levels;
    g.dx_accumulate = 0;
    g.rep_levels = 0;
    g.rep_mask = 0;
    g.rep_stride = 0;
    for (int l = 0; l <= desc->n_levels; ++l) g.offsets[l] = desc->offsets[l];
    for (int l = 0; l < desc->n_levels; ++l) {
        LSE_REQUIRE(desc->offsets[l + 1] > desc->offsets[l], "%s: level %d is empty", who, l);
        LSE_REQUIRE(desc->resolutions[l] >= 2, "%s: level %d resolution < 2", who, l);
        g.scales[l] = desc->scales[l];
        g.res[l] = desc->resolutions[l];
    }
    return LSE_OK;
}

}  // namespace

extern "C" int lse_hash_fwd(const lse_grid_desc *desc, const float *x01, const float *table, float *y, int64_t n,
                            const int64_t *n_dev, lse_stream_t stream)
{
    GridParams g;
    int rc = fill_params(desc, g, "lse_hash_fwd");
    if (rc) return rc;
    LSE_REQUIRE(n >= 0, "lse_hash_fwd: n < 0");
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(x01 && table && y, "lse_hash_fwd: null pointer");
    const int64_t chunks = (n + kFwdThreads * kFwdItems - 1) / (kFwdThreads * kFwdItems);
    hipStream_t st = lse::as_stream(stream);
    const int64_t blocks = chunks * g.n_levels;
    LSE_REQUIRE(blocks < (1ll << 31), "lse_hash_fwd: grid too large");
    hipLaunchKernelGGL(hash_fwd_kernel, dim3((unsigned)blocks), dim3(kFwdThreads), 0, st, g, x01,
                       reinterpret_cast<const float2 *>(table), reinterpret_cast<float2 *>(y), n, chunks, n_dev);
    return lse::check_launch("lse_hash_fwd");
}

extern "C" int lse_hash_bwd_input(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table,
                                  float *dx, int64_t n, const int64_t *n_dev, lse_stream_t stream)
{
    GridParams g;
    int rc = fill_params(desc, g, "lse_hash_bwd_input");
    if (rc) return rc;
    LSE_REQUIRE(n >= 0, "lse_hash_bwd_input: n < 0");
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(x01 && dy && table && dx, "lse_hash_bwd_input: null pointer");
    const int64_t chunks = (n + kFwdThreads * kFwdItems - 1) / (kFwdThreads * kFwdItems);
    LSE_REQUIRE(chunks < (1ll << 31), "lse_hash_bwd_input: grid too large");
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(hash_bwd_input_kernel, dim3((unsigned)chunks), dim3(kFwdThreads), 0, st, g, x01,
                       reinterpret_cast<const float2 *>(dy), reinterpret_cast<const float2 *>(table), dx, n, n_dev);
    return lse::check_launch("lse_hash_bwd_input");
}

extern "C" void lse_hash_bwd_default_opts(lse_hash_bwd_opts *o)
{
    if (!o) return;
    o->impl = 2;           // lane-per-sample + LDS sector cache, run ends of several levels batched per cache pass
    o->stage_max = (int32_t)lse::option("hash_bwd_stage_max");   // impl 2: a level ending more runs than this per wave passes unstaged
                           // when the queue is empty
    o->few_runs = (int32_t)lse::option("hash_bwd_few_runs");     // 8 (profiles/r05_hash_bwd_thresholds.txt: with stage_max 48 the best pair for steps
                           // that grow with the distance -- the reference's default configuration 1.51 -> 1.43 ms -- and neutral
                           // (+0.2 %) at the metric size, whose constant step prefers fewer direct adds -- (3, 56) on the final kernel; callers that know the
                           // regime pass the pair (lsenerf_amd/ops.py: HASH_BWD_DENSE_STEPS); 10 and 16: slower everywhere)
    o->second_probe = (int32_t)lse::option("hash_bwd_probes");   // extra probe rounds (home + 2 * k) before a corner goes to memory
                           // alone; pays wherever the kernel is bound by atomic requests, costs ~2 % per round where it is issue-bound.
                           // 1 -> 3 rounds: requests 50.5 -> 48.2 M (metric size), 28.3 -> 26.9 M (default configuration); hash_bwd
                           // 2.66 -> 2.66 / 1.40 -> 1.34 / 1.13 -> 1.05 ms (metric size / default configuration / 3-bundle step),
                           // M-packed step 6.07 -> 5.99; 4 rounds: slower everywhere (profiles/r03_hash_bwd_probe_rounds.txt)
    o->replicas = 16;      // direct adds of the levels < replica_levels go to this many replicas (power of two); needs `workspace`
                           // (M-packed 3.67 -> 3.21 ms with 8, 3.16 with 16, 3.18 with 32; M-march and the default configuration +-1 %)
    o->replica_levels = 4; // 16^3 .. 43^3: 125 568 entries = 1 MB per replica
    o->workspace = nullptr;
    o->workspace_bytes = 0;
    // reserved (include/lse_hip.h): the values lse_hash_bwd_ex insists on
    o->gran = 6;
    o->rounds = 32;
    o->dbg = 0;
    o->interleave_from_scale = 1e30f;
    o->coarse_levels = 0;
    o->prefetch = 0;
}

// The replicas pay where a level is a few thousand lines that every wave of the launch adds to (16^3 .. 43^3: 1 MB per replica); for
// a grid whose coarse levels are already big (base_res >= ~64 at T = 2^19: 4 hashed levels = 16 MB per replica, 268 MB for 16, all of
// it swept by hash_bwd_reduce_replicas_kernel after every backward) they would cost memory and time for nothing: the replicated
// levels stop at the first level that would push ONE replica past this budget.
constexpr int64_t kReplicaBudgetFloats = (2 << 20) / (int64_t)sizeof(float);      // 2 MB per replica

static int64_t replica_floats(const lse_grid_desc *desc, const lse_hash_bwd_opts &o, int *levels_out)
{
    int lv = std::min<int>(o.replica_levels, desc->n_levels);
    while (lv > 0 && (int64_t)2 * desc->offsets[lv] > kReplicaBudgetFloats) --lv;
    if (o.replicas < 2 || lv <= 0) { if (levels_out) *levels_out = 0; return 0; }
    if (levels_out) *levels_out = lv;
    return (int64_t)2 * desc->offsets[lv];        // floats per replica (level offsets are multiples of 8 entries)
}

extern "C" int64_t lse_hash_bwd_workspace_bytes(const lse_grid_desc *desc, const lse_hash_bwd_opts *opts)
{
    if (!desc) return 0;
    lse_hash_bwd_opts o;
    lse_hash_bwd_default_opts(&o);
    if (opts) o = *opts;
    return replica_floats(desc, o, nullptr) * (int64_t)sizeof(float) * std::max(o.replicas, 0);
}

extern "C" int lse_hash_bwd(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table,
                            float *dtable, float *dx, int64_t n, const int64_t *n_dev, lse_stream_t stream)
{
    return lse_hash_bwd_ex(desc, x01, dy, table, dtable, dx, 0, 0, desc ? desc->n_levels : 0, n, n_dev, nullptr, stream);
}

extern "C" int lse_hash_bwd_levels(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table,
                                   float *dtable, float *dx, int32_t dx_accumulate, int32_t level_begin,
                                   int32_t level_end, int64_t n, const int64_t *n_dev, lse_stream_t stream)
{
    return lse_hash_bwd_ex(desc, x01, dy, table, dtable, dx, dx_accumulate, level_begin, level_end, n, n_dev, nullptr, stream);
}

extern "C" int lse_hash_bwd_ex(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table,
                               float *dtable, float *dx, int32_t dx_accumulate, int32_t level_begin, int32_t level_end,
                               int64_t n, const int64_t *n_dev, const lse_hash_bwd_opts *opts, lse_stream_t stream)
{
    lse_hash_bwd_opts o;
    lse_hash_bwd_default_opts(&o);
    if (opts) o = *opts;
    // two kernels exist: the batched sector-cache kernel (impl 2) and the generic 16-lanes-per-sample kernel (impl 0; also taken for
    // grids whose levels do not start on 64-byte lines).  The reserved fields once selected variants that are retired
    // (DESIGN_HISTORY.md): anything but the value lse_hash_bwd_default_opts writes is refused before anything is launched.
    if ((o.impl != 0 && o.impl != 2) || o.gran != 6 || o.prefetch != 0 || o.coarse_levels != 0 || o.rounds != 32 || o.dbg != 0 ||
        o.interleave_from_scale < 1e29f) {
        lse::set_error("lse_hash_bwd: impl %d / gran %d / prefetch %d / coarse_levels %d / rounds %d / dbg %d / interleave_from_scale %g "
                       "selects a retired development variant (DESIGN_HISTORY.md)", o.impl, o.gran, o.prefetch, o.coarse_levels, o.rounds,
                       o.dbg, (double)o.interleave_from_scale);
        return LSE_E_UNSUPPORTED;
    }
    LSE_REQUIRE(o.stage_max >= 0 && o.stage_max <= 64, "lse_hash_bwd: opts.stage_max must be in [0, 64]");
    LSE_REQUIRE(o.few_runs >= 0 && o.few_runs <= 16, "lse_hash_bwd: opts.few_runs must be in [0, 16]");
    GridParams g;
    int rc = fill_params(desc, g, "lse_hash_bwd");
    if (rc) return rc;
    LSE_REQUIRE(0 <= level_begin && level_begin <= level_end && level_end <= g.n_levels,
                "lse_hash_bwd_levels: bad level range [%d, %d)", level_begin, level_end);
    g.l_begin = level_begin;
    g.l_end = level_end;
    g.dx_accumulate = dx_accumulate;
    if (level_begin == level_end && !(dx && !dx_accumulate)) return LSE_OK;
    LSE_REQUIRE(n >= 0, "lse_hash_bwd: n < 0");
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(x01 && dy && dtable, "lse_hash_bwd: null pointer");
    LSE_REQUIRE(!dx || table, "lse_hash_bwd: dx requested but table is null");
    // the sector cache needs every level to start on a 64-B line (tcnn pads level sizes to 8 entries)
    bool lines_ok = true;
    for (int l = 0; l <= g.n_levels; ++l) lines_ok = lines_ok && (g.offsets[l] % 8 == 0);
    const bool batched = o.impl == 2 && lines_ok;
    // device-side sample count: honoured by the batched kernel only
    LSE_REQUIRE(!n_dev || o.impl == 2, "lse_hash_bwd: a device-side count needs opts.impl == 2");
    LSE_REQUIRE(!n_dev || lines_ok, "lse_hash_bwd: a device-side count needs 64-byte aligned levels (the default kernel)");
    // batched: one wave = 64 samples per workgroup, rounded up to a multiple of 8 for the XCD chunk mapping;
    // 16 lanes per sample: four waves of 4 * kRounds samples
    const int64_t blocks = batched ? ((n + 63) / 64 + 7) / 8 * 8 : (n + 16 * kRounds - 1) / (16 * kRounds);
    LSE_REQUIRE(blocks < (1ll << 31), "lse_hash_bwd: grid too large");
    // replicas of the coarsest levels for the direct adds of the batched kernel's few-runs path
    float *ws = nullptr;
    int rep_lv = 0;
    const int64_t rep_floats = replica_floats(desc, o, &rep_lv);
    if (o.workspace && rep_floats > 0 && level_begin < rep_lv) {
        LSE_REQUIRE((o.replicas & (o.replicas - 1)) == 0 && o.replicas <= 64, "lse_hash_bwd: opts.replicas must be a power of two <= 64");
        LSE_REQUIRE(o.workspace_bytes >= rep_floats * (int64_t)sizeof(float) * o.replicas,
                    "lse_hash_bwd: workspace of %lld bytes, %lld needed (lse_hash_bwd_workspace_bytes)", (long long)o.workspace_bytes,
                    (long long)(rep_floats * (int64_t)sizeof(float) * o.replicas));
        LSE_REQUIRE(((uintptr_t)o.workspace & 15) == 0, "lse_hash_bwd: workspace must be 16-byte aligned");
        ws = static_cast<float *>(o.workspace);
        g.rep_levels = rep_lv;
        g.rep_mask = o.replicas - 1;
        g.rep_stride = (uint32_t)rep_floats;
    }
    hipStream_t st = lse::as_stream(stream);
    const float *tb = dx ? table : nullptr;
    if (batched) {
        const float2 *dy2 = reinterpret_cast<const float2 *>(dy);
        const float2 *tb2 = reinterpret_cast<const float2 *>(tb);
        if (dx) hipLaunchKernelGGL((hash_bwd_batched_kernel<true>), dim3((unsigned)blocks), dim3(64), 0, st, g, x01, dy2, tb2, dtable, dx,
                                   n, o.few_runs, o.second_probe, o.stage_max, ws, n_dev);
        else hipLaunchKernelGGL((hash_bwd_batched_kernel<false>), dim3((unsigned)blocks), dim3(64), 0, st, g, x01, dy2, tb2, dtable, dx,
                                n, o.few_runs, o.second_probe, o.stage_max, ws, n_dev);
    } else {
        if (dx) hipLaunchKernelGGL((hash_bwd_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, st, g, x01, dy, tb, dtable, dx, n);
        else hipLaunchKernelGGL((hash_bwd_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, st, g, x01, dy, tb, dtable, dx, n);
    }
    if (ws) {      // fold the replicas into the table gradient
        const uint32_t n4 = (uint32_t)(rep_floats / 4);
        hipLaunchKernelGGL(hash_bwd_reduce_replicas_kernel, dim3((n4 + 255) / 256), dim3(256), 0, st, ws, dtable, n4, o.replicas,
                           (uint32_t)rep_floats);
    }
    return lse::check_launch("lse_hash_bwd");
}
