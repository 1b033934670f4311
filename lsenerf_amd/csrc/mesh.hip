// Mesh export for gfx950: naive surface nets of a density lattice (one vertex per active cell, one quad per sign-changing interior
// lattice edge), the lattice's point positions, and world-space normals at arbitrary points.  The definition is in include/lse_hip.h
// (and, as numpy, in tests/mesh_ref.py); the kernels restate it operation by operation, hence -ffp-contract=off.
// Vertices and quads are two ordered compactions (compact.h) over segments of LSE_MESH_SEGMENT cells / lattice points:
//   count_cells      the active cells; cell ranks go to the workspace.
//   count_quads      a lattice point carries up to three quads (one per axis), so its rank is "all quads of lower lanes, then its
//                    own in axis order": three prefix counts per iteration.  Only the segment counts are kept.
//   scan_kernel      one block per row (vertices, quads), totals -> device int64[2].
//   emit_vertices    one thread per cell: rank >= 0 -> the mean of the edge crossings, mapped to world.
//   emit_quads       the walk of count_quads again, with the ranks: two triangles per quad, in ascending (point, axis).
// All passes are bandwidth-bound flat maps over sigma with iz fastest (a wave's corner reads are coalesced rows); nothing is staged
// in LDS.
// LSE_NETS_SKIP_NAN (the _ex entry points; include/lse_hip.h, "TSDF fusion"): NaN marks unobserved points.  count_cells keeps no cell
// with a NaN corner, and both quad walks keep an edge only if the four cells around it have a rank >= 0 -- the cell pass runs first
// on the same stream.  With flags == 0 the kernels take the paths they always took.
#include "compact.h"

namespace {

#include "positions.h"      // Box, positions_bwd_sample: the world-space Jacobian of the normals
#include "lattice.h"        // Lattice, cell_coords, point_coords, make_lattice, make_box

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kSeg = LSE_MESH_SEGMENT;        // consecutive cells / lattice points owned by one wave
constexpr int kIters = kSeg / 64;
static_assert(kThreads == lse::kScanThreads, "scan_kernel is one block of kScanThreads");

// 8 corner values of cell (cx, cy, cz), index dx * 4 + dy * 2 + dz; all 8 points are inside the lattice for every valid cell
__device__ __forceinline__ void load_corners(const float *__restrict__ sigma, const Lattice &L, int cx, int cy, int cz, float s[8])
{
    const int64_t p = (int64_t)cx * L.sx + (int64_t)cy * L.sy + cz;
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = sigma[p + (k >> 2) * L.sx + ((k >> 1) & 1) * L.sy + (k & 1)];
}

// skip_nan (LSE_NETS_SKIP_NAN): a cell with a NaN corner is never active
__device__ __forceinline__ bool cell_active(const float s[8], float level, bool skip_nan)
{
    int in = 0, nan = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        in += s[k] > level ? 1 : 0;      // NaN is outside
        nan += s[k] != s[k] ? 1 : 0;
    }
    return in != 0 && in != 8 && !(skip_nan && nan != 0);
}

// ---- count ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void count_cells_kernel(const float *__restrict__ sigma, Lattice L, float level, int n_segs,
                                                               bool skip_nan, int32_t *__restrict__ cell_rank,
                                                               int64_t *__restrict__ seg_counts)
{
    const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (seg >= n_segs) return;                          // (wave-uniform)
    lse::segment_rank<kSeg>(seg, L.cells, cell_rank, seg_counts, [&](int64_t c) {
        int cc[3];
        float s[8];
        cell_coords(L, c, cc);
        load_corners(sigma, L, cc[0], cc[1], cc[2], s);
        return cell_active(s, level, skip_nan);
    });
}

// index of the cell C_k around the edge (i, a): C0 = i - e_b - e_c, C1 = i - e_c, C2 = i, C3 = i - e_b
__device__ __forceinline__ int64_t edge_cell(const Lattice &L, const int i[3], int b, int c, int k)
{
    int cc[3] = {i[0], i[1], i[2]};
    cc[b] -= (k == 0 || k == 3) ? 1 : 0;
    cc[c] -= (k == 0 || k == 1) ? 1 : 0;
    return ((int64_t)cc[0] * L.n[1] + cc[1]) * L.n[2] + cc[2];
}

// bit a: the lattice edge (p, a) gives a quad -- q = p + e_a exists, the edge is interior in the other two axes, inside(p) != inside(q)
// and, with active_rank (LSE_NETS_SKIP_NAN: the ranks count_cells_kernel wrote), all four cells around the edge are active
__device__ __forceinline__ int quad_bits(const float *__restrict__ sigma, const Lattice &L, int64_t p, const int i[3], float level,
                                         const int32_t *__restrict__ active_rank, bool &in_p)
{
    in_p = sigma[p] > level;
    const int64_t stride[3] = {L.sx, L.sy, 1};
    bool mid[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) mid[k] = i[k] >= 1 && i[k] <= L.n[k] - 1;
    int bits = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        if (i[a] < L.n[a] && mid[b] && mid[c]) {
            const bool in_q = sigma[p + stride[a]] > level;
            bool quad = in_q != in_p;
            if (quad && active_rank) {
#pragma unroll
                for (int k = 0; k < 4; ++k) quad = quad && active_rank[edge_cell(L, i, b, c, k)] >= 0;
            }
            bits |= quad ? (1 << a) : 0;
        }
    }
    return bits;
}

__global__ __launch_bounds__(kThreads) void count_quads_kernel(const float *__restrict__ sigma, Lattice L, float level, int n_segs,
                                                               const int32_t *__restrict__ active_rank,
                                                               int64_t *__restrict__ seg_counts)
{
    const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = lse::lane_id();
    if (seg >= n_segs) return;                          // (wave-uniform)
    int run = 0;
    for (int it = 0; it < kIters; ++it) {
        const int64_t p = (int64_t)seg * kSeg + it * 64 + lane;
        int bits = 0;
        if (p < L.points) {
            int i[3];
            bool in_p;
            point_coords(L, p, i);
            bits = quad_bits(sigma, L, p, i, level, active_rank, in_p);
        }
        int t0, t1, t2;
        lse::wave_prefix_count(bits & 1, t0);
        lse::wave_prefix_count(bits & 2, t1);
        lse::wave_prefix_count(bits & 4, t2);
        run += t0 + t1 + t2;
    }
    if (lane == 0) seg_counts[seg] = run;
}

// block 0: vertex segments, block 1: quad segments.  Counts -> exclusive offsets (in place), total -> totals[block].  A segment's
// count is at most 3 * kSeg, so a 256-segment step sums in int; the carry is int64.
__global__ __launch_bounds__(kThreads) void scan_kernel(int64_t *__restrict__ seg_v, int n_v, int64_t *__restrict__ seg_q, int n_q,
                                                        int64_t *__restrict__ totals)
{
    const int64_t sum = lse::block_exclusive_scan<int>(blockIdx.x ? seg_q : seg_v, blockIdx.x ? n_q : n_v, (int64_t)0);
    if (threadIdx.x == 0) totals[blockIdx.x] = sum;
}

// ---- emit -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void emit_vertices_kernel(const float *__restrict__ sigma, Lattice L, Box box, float level,
                                                                 const int32_t *__restrict__ cell_rank,
                                                                 const int64_t *__restrict__ seg_off, int64_t cap,
                                                                 float *__restrict__ vertices)
{
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= L.cells) return;
    const int64_t vid = lse::emit_row<kSeg>(c, cell_rank, seg_off, cap);
    if (vid < 0) return;
    int cc[3];
    float s[8];
    cell_coords(L, c, cc);
    load_corners(sigma, L, cc[0], cc[1], cc[2], s);
    float sum[3] = {0.f, 0.f, 0.f};
    int count = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c2 = (a + 2) % 3;
#pragma unroll
        for (int ob = 0; ob < 2; ++ob) {
#pragma unroll
            for (int oc = 0; oc < 2; ++oc) {
                int d[3];
                d[a] = 0, d[b] = ob, d[c2] = oc;
                const float sp = s[d[0] * 4 + d[1] * 2 + d[2]];
                const float sq = s[d[0] * 4 + d[1] * 2 + d[2] + (4 >> a)];
                if ((sp > level) != (sq > level)) {
                    float t = (level - sp) / (sq - sp);
                    t = (t != t) ? 0.5f : t;
                    t = fminf(fmaxf(t, 0.f), 1.f);
                    float pt[3];
#pragma unroll
                    for (int k = 0; k < 3; ++k) pt[k] = (float)(cc[k] + d[k]);
                    pt[a] = pt[a] + t;
#pragma unroll
                    for (int k = 0; k < 3; ++k) sum[k] = sum[k] + pt[k];
                    ++count;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float uk = sum[k] / (float)count;       // (an active cell has at least one crossing)
        vertices[vid * 3 + k] = box.lo[k] + (uk / (float)L.n[k]) * (box.hi[k] - box.lo[k]);
    }
}

__global__ __launch_bounds__(kThreads) void emit_quads_kernel(const float *__restrict__ sigma, Lattice L, float level, int n_segs,
                                                              const int32_t *__restrict__ active_rank,
                                                              const int32_t *__restrict__ cell_rank,
                                                              const int64_t *__restrict__ seg_off_v,
                                                              const int64_t *__restrict__ seg_off_q, int64_t cap,
                                                              int32_t *__restrict__ triangles)
{
    const int seg = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = lse::lane_id();
    if (seg >= n_segs) return;                          // (wave-uniform)
    int64_t off = seg_off_q[seg];
    for (int it = 0; it < kIters; ++it) {
        const int64_t p = (int64_t)seg * kSeg + it * 64 + lane;
        int bits = 0, i[3] = {0, 0, 0};
        bool in_p = false;
        if (p < L.points) {
            point_coords(L, p, i);
            bits = quad_bits(sigma, L, p, i, level, active_rank, in_p);
        }
        int t0, t1, t2;
        const int b0 = lse::wave_prefix_count(bits & 1, t0), b1 = lse::wave_prefix_count(bits & 2, t1);
        const int b2 = lse::wave_prefix_count(bits & 4, t2);
        int64_t qid = off + b0 + b1 + b2;       // all quads of lower lanes, then this point's own in axis order
        off += t0 + t1 + t2;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (!(bits & (1 << a))) continue;
            const int64_t q = qid++;
            if (q >= cap) continue;
            const int b = (a + 1) % 3, c = (a + 2) % 3;
            // the four cells around the edge: i_a <= n_a - 1 and 1 <= i_b, i_c <= n_b - 1, n_c - 1, so all four are cells of the lattice
            int32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) w[k] = (int32_t)lse::segment_row<kSeg>(edge_cell(L, i, b, c, k), cell_rank, seg_off_v);
            if (!in_p) {
                const int32_t t0 = w[0], t1 = w[1];
                w[0] = w[3], w[1] = w[2], w[2] = t1, w[3] = t0;
            }
            int32_t *tri = triangles + q * 6;
            tri[0] = w[0], tri[1] = w[1], tri[2] = w[2];
            tri[3] = w[0], tri[4] = w[2], tri[5] = w[3];
        }
    }
}

// ---- lattice positions and point normals ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void lattice_positions_kernel(Lattice L, Box box, int64_t first, int64_t n,
                                                                     float *__restrict__ positions)
{
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    int i[3];
    point_coords(L, first + j, i);
#pragma unroll
    for (int k = 0; k < 3; ++k) positions[j * 3 + k] = box.lo[k] + ((float)i[k] / (float)L.n[k]) * (box.hi[k] - box.lo[k]);
}

// n = -J^T g / max(|J^T g|, 1e-12): the per-sample arithmetic of eval_composite_normals_kernel (volrend.hip) with LSE_NORMALS_WORLD
__global__ __launch_bounds__(kThreads) void point_normals_kernel(const float *__restrict__ dx01, const float *__restrict__ positions,
                                                                 int contraction, Box box, int64_t n,
                                                                 const int64_t *__restrict__ n_dev, float *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= lse::clamp_count(n, n_dev)) return;
    const float g[3] = {dx01[j * 3 + 0], dx01[j * 3 + 1], dx01[j * 3 + 2]};
    const float p[3] = {positions[j * 3 + 0], positions[j * 3 + 1], positions[j * 3 + 2]};
    float gw[3];
    positions_bwd_sample(p, g, contraction, box, gw);
    const float len = sqrtf(fmaf(gw[2], gw[2], fmaf(gw[1], gw[1], gw[0] * gw[0])));
    const float inv = -1.f / fmaxf(len, 1e-12f);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[j * 3 + k] = gw[k] * inv;
}

struct Workspace {
    int64_t *seg_v, *seg_q;
    int32_t *cell_rank;
    int n_v, n_q;
    int64_t bytes;
};

Workspace carve(const Lattice &L, void *base)
{
    Workspace w;
    w.n_v = lse::n_segments<kSeg>(L.cells);
    w.n_q = lse::n_segments<kSeg>(L.points);
    w.seg_v = static_cast<int64_t *>(base);
    w.seg_q = w.seg_v + w.n_v;
    w.cell_rank = reinterpret_cast<int32_t *>(w.seg_q + w.n_q);
    w.bytes = 8 * ((int64_t)w.n_v + w.n_q) + 4 * L.cells;
    return w;
}

}  // namespace

extern "C" int lse_lattice_positions(const float *h_lo, const float *h_hi, int32_t nx, int32_t ny, int32_t nz, int64_t first,
                                     int64_t n, float *positions, lse_stream_t stream)
{
    const char *what = "lse_lattice_positions";
    Lattice L;
    LSE_REQUIRE(make_lattice(nx, ny, nz, L), "%s: resolution %d x %d x %d: every count >= 1 and fewer than 2^31 points", what, nx, ny,
                nz);
    LSE_REQUIRE(h_lo && h_hi, "%s: null box", what);
    LSE_REQUIRE(first >= 0 && n >= 0 && first <= L.points && n <= L.points - first, "%s: points [%lld, %lld + %lld) of %lld", what,
                (long long)first, (long long)first, (long long)n, (long long)L.points);
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(positions, "%s: null pointer", what);
    hipLaunchKernelGGL(lattice_positions_kernel, dim3(lse::blocks_for(n, kThreads)), dim3(kThreads), 0, lse::as_stream(stream), L,
                       make_box(h_lo, h_hi), first, n, positions);
    return lse::check_launch(what);
}

extern "C" int lse_surface_nets_workspace(int32_t nx, int32_t ny, int32_t nz, int64_t *h_bytes)
{
    const char *what = "lse_surface_nets_workspace";
    Lattice L;
    LSE_REQUIRE(make_lattice(nx, ny, nz, L), "%s: resolution %d x %d x %d: every count >= 1 and fewer than 2^31 points", what, nx, ny,
                nz);
    LSE_REQUIRE(h_bytes, "%s: null pointer", what);
    *h_bytes = carve(L, nullptr).bytes;
    return LSE_OK;
}

// the body of lse_surface_nets_count and lse_surface_nets_count_ex
static int nets_count(const char *what, const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, int32_t flags,
                      void *workspace, int64_t workspace_bytes, int64_t *totals, lse_stream_t stream)
{
    Lattice L;
    LSE_REQUIRE(make_lattice(nx, ny, nz, L), "%s: resolution %d x %d x %d: every count >= 1 and fewer than 2^31 points", what, nx, ny,
                nz);
    LSE_REQUIRE((flags & ~LSE_NETS_SKIP_NAN) == 0, "%s: unknown flags 0x%x", what, (unsigned)flags);
    LSE_REQUIRE(sigma && workspace && totals, "%s: null pointer", what);
    LSE_REQUIRE(((uintptr_t)workspace & 7) == 0 && ((uintptr_t)totals & 7) == 0, "%s: workspace and totals must be 8-byte aligned",
                what);
    const Workspace w = carve(L, workspace);
    LSE_REQUIRE(workspace_bytes >= w.bytes, "%s: workspace of %lld bytes < %lld (lse_surface_nets_workspace)", what,
                (long long)workspace_bytes, (long long)w.bytes);
    const bool skip_nan = (flags & LSE_NETS_SKIP_NAN) != 0;
    hipStream_t st = lse::as_stream(stream);
    hipLaunchKernelGGL(count_cells_kernel, dim3(lse::blocks_for(w.n_v, kWaves)), dim3(kThreads), 0, st, sigma, L, level, w.n_v, skip_nan,
                       w.cell_rank, w.seg_v);
    // (stream order: the quad pass of the masked mode reads the ranks the cell pass wrote)
    hipLaunchKernelGGL(count_quads_kernel, dim3(lse::blocks_for(w.n_q, kWaves)), dim3(kThreads), 0, st, sigma, L, level, w.n_q,
                       skip_nan ? (const int32_t *)w.cell_rank : nullptr, w.seg_q);
    hipLaunchKernelGGL(scan_kernel, dim3(2), dim3(kThreads), 0, st, w.seg_v, w.n_v, w.seg_q, w.n_q, totals);
    return lse::check_launch(what);
}

// the body of lse_surface_nets_emit and lse_surface_nets_emit_ex
static int nets_emit(const char *what, const float *sigma, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi,
                     float level, int32_t flags, const void *workspace, int64_t workspace_bytes, int64_t cap_vertices,
                     int64_t cap_quads, float *vertices, int32_t *triangles, lse_stream_t stream)
{
    Lattice L;
    LSE_REQUIRE(make_lattice(nx, ny, nz, L), "%s: resolution %d x %d x %d: every count >= 1 and fewer than 2^31 points", what, nx, ny,
                nz);
    LSE_REQUIRE((flags & ~LSE_NETS_SKIP_NAN) == 0, "%s: unknown flags 0x%x", what, (unsigned)flags);
    LSE_REQUIRE(sigma && workspace && h_lo && h_hi, "%s: null pointer", what);
    LSE_REQUIRE(((uintptr_t)workspace & 7) == 0, "%s: workspace must be 8-byte aligned", what);
    const Workspace w = carve(L, const_cast<void *>(workspace));
    LSE_REQUIRE(workspace_bytes >= w.bytes, "%s: workspace of %lld bytes < %lld (lse_surface_nets_workspace)", what,
                (long long)workspace_bytes, (long long)w.bytes);
    LSE_REQUIRE(cap_vertices >= 0 && cap_quads >= 0, "%s: negative capacity", what);
    LSE_REQUIRE((cap_vertices == 0 || vertices) && (cap_quads == 0 || triangles), "%s: null output for a capacity > 0", what);
    const bool skip_nan = (flags & LSE_NETS_SKIP_NAN) != 0;
    hipStream_t st = lse::as_stream(stream);
    if (cap_vertices > 0)
        hipLaunchKernelGGL(emit_vertices_kernel, dim3(lse::blocks_for(L.cells, kThreads)), dim3(kThreads), 0, st, sigma, L,
                           make_box(h_lo, h_hi), level, (const int32_t *)w.cell_rank, (const int64_t *)w.seg_v, cap_vertices, vertices);
    if (cap_quads > 0)
        hipLaunchKernelGGL(emit_quads_kernel, dim3(lse::blocks_for(w.n_q, kWaves)), dim3(kThreads), 0, st, sigma, L, level, w.n_q,
                           skip_nan ? (const int32_t *)w.cell_rank : nullptr, (const int32_t *)w.cell_rank, (const int64_t *)w.seg_v,
                           (const int64_t *)w.seg_q, cap_quads, triangles);
    return lse::check_launch(what);
}

extern "C" int lse_surface_nets_count(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace,
                                      int64_t workspace_bytes, int64_t *totals, lse_stream_t stream)
{
    return nets_count("lse_surface_nets_count", sigma, nx, ny, nz, level, 0, workspace, workspace_bytes, totals, stream);
}

extern "C" int lse_surface_nets_count_ex(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, int32_t flags,
                                         void *workspace, int64_t workspace_bytes, int64_t *totals, lse_stream_t stream)
{
    return nets_count("lse_surface_nets_count_ex", sigma, nx, ny, nz, level, flags, workspace, workspace_bytes, totals, stream);
}

extern "C" int lse_surface_nets_emit(const float *sigma, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi,
                                     float level, const void *workspace, int64_t workspace_bytes, int64_t cap_vertices,
                                     int64_t cap_quads, float *vertices, int32_t *triangles, lse_stream_t stream)
{
    return nets_emit("lse_surface_nets_emit", sigma, nx, ny, nz, h_lo, h_hi, level, 0, workspace, workspace_bytes, cap_vertices,
                     cap_quads, vertices, triangles, stream);
}

extern "C" int lse_surface_nets_emit_ex(const float *sigma, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi,
                                        float level, int32_t flags, const void *workspace, int64_t workspace_bytes,
                                        int64_t cap_vertices, int64_t cap_quads, float *vertices, int32_t *triangles,
                                        lse_stream_t stream)
{
    return nets_emit("lse_surface_nets_emit_ex", sigma, nx, ny, nz, h_lo, h_hi, level, flags, workspace, workspace_bytes,
                     cap_vertices, cap_quads, vertices, triangles, stream);
}

extern "C" int lse_point_normals_world(const float *d_x01, const float *positions, int32_t contraction, const float *h_aabb, int64_t n,
                                       const int64_t *n_dev, float *out, lse_stream_t stream)
{
    const char *what = "lse_point_normals_world";
    LSE_REQUIRE(n >= 0, "%s: n < 0", what);
    LSE_REQUIRE(contraction || h_aabb, "%s: aabb normalisation needs h_aabb", what);
    if (n == 0) return LSE_OK;
    LSE_REQUIRE(d_x01 && positions && out, "%s: null pointer", what);
    Box box;
    for (int k = 0; k < 3; ++k) { box.lo[k] = h_aabb ? h_aabb[k] : -1.f; box.hi[k] = h_aabb ? h_aabb[3 + k] : 1.f; }
    hipLaunchKernelGGL(point_normals_kernel, dim3(lse::blocks_for(n, kThreads)), dim3(kThreads), 0, lse::as_stream(stream), d_x01, positions,
                       (int)contraction, box, n, n_dev, out);
    return lse::check_launch(what);
}
