// The point / cell lattice of the export kernels (mesh.hip, tsdf.hip), written once: include/lse_hip.h, "mesh export".  Included
// inside the including file's anonymous namespace, behind positions.h (Box).
#pragma once

struct Lattice {
    int n[3];               // cells per axis
    int64_t sx, sy;         // point strides of ix and iy (iz is fastest)
    int64_t cells, points;
};

// cell index -> (cx, cy, cz), cz fastest
__device__ __forceinline__ void cell_coords(const Lattice &L, int64_t c, int cc[3])
{
    const uint32_t u = (uint32_t)c;
    cc[2] = (int)(u % (uint32_t)L.n[2]);
    cc[1] = (int)((u / (uint32_t)L.n[2]) % (uint32_t)L.n[1]);
    cc[0] = (int)(u / ((uint32_t)L.n[2] * (uint32_t)L.n[1]));
}

__device__ __forceinline__ void point_coords(const Lattice &L, int64_t p, int i[3])
{
    const uint32_t u = (uint32_t)p, mz = (uint32_t)L.n[2] + 1u, my = (uint32_t)L.n[1] + 1u;
    i[2] = (int)(u % mz);
    i[1] = (int)((u / mz) % my);
    i[0] = (int)(u / (mz * my));
}

// position of the lattice point (i0, i1, i2) along axis k
__device__ __forceinline__ float point_position(const Lattice &L, const Box &box, const int i[3], int k)
{
    return box.lo[k] + ((float)i[k] / (float)L.n[k]) * (box.hi[k] - box.lo[k]);
}

// false when the resolution is not a lattice the kernels index: every n_k >= 1 and fewer than 2^31 points
inline bool make_lattice(int32_t nx, int32_t ny, int32_t nz, Lattice &L)
{
    if (nx < 1 || ny < 1 || nz < 1) return false;
    const int64_t lim = 1ll << 31;
    const int64_t yz = ((int64_t)ny + 1) * ((int64_t)nz + 1);
    if (yz >= lim) return false;
    const int64_t points = ((int64_t)nx + 1) * yz;      // < 2^31 * 2^31: no overflow
    if (points >= lim) return false;
    L.n[0] = nx, L.n[1] = ny, L.n[2] = nz;
    L.sy = (int64_t)nz + 1;
    L.sx = yz;
    L.points = points;
    L.cells = (int64_t)nx * ny * nz;
    return true;
}

inline Box make_box(const float *h_lo, const float *h_hi)
{
    Box box;
    for (int k = 0; k < 3; ++k) { box.lo[k] = h_lo[k]; box.hi[k] = h_hi[k]; }
    return box;
}
