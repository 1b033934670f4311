// The position map of the field (L-inf contraction or aabb normalisation onto the unit cube) and its Jacobian.  Included inside the
// anonymous namespace of field_misc.hip (positions forward / backward) and volrend.hip (world-space normals), so that every kernel
// that maps a position or a gradient through it runs one definition.
#pragma once

struct Box { float lo[3], hi[3]; };

// Unit-cube coordinates of a position and the in-bounds selector: L-inf contraction -> (c + 2) / 4, or aabb normalisation.  ONE body
// for the forward and for the selector of the backward: the backward used to re-derive x from s(m) * p with s = (2 - 1/m) / m, which
// rounds differently -- at |p|_inf = 3e38 (1/m denormal) it gave x = 0.9999999 where the forward's (2 - 1/m) * (p / m) gives exactly 1,
// so the forward left the sample out and the backward let a gradient of 1e-39 through.
__device__ __forceinline__ bool unit_cube_coords(const float p[3], int contraction, const Box &box, float x[3])
{
    if (contraction) {
        const float mag = fmaxf(fabsf(p[0]), fmaxf(fabsf(p[1]), fabsf(p[2])));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = mag < 1.f ? p[k] : (2.f - (1.f / mag)) * (p[k] / mag);
            x[k] = (c + 2.f) / 4.f;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = (p[k] - box.lo[k]) / (box.hi[k] - box.lo[k]);
    }
    return x[0] > 0.f && x[0] < 1.f && x[1] > 0.f && x[1] < 1.f && x[2] > 0.f && x[2] < 1.f;
}

// d(pos) of one sample from d(x01) = g: Jacobian of the contraction / aabb normalisation at p, selector-masked.  One body for
// positions_bwd_kernel and ray_grad_dx01_kernel, so that both produce the same bits.
__device__ __forceinline__ void positions_bwd_sample(const float p[3], const float g[3], int contraction, const Box &box,
                                                     float out[3])
{
    if (contraction) {
        const float a0 = fabsf(p[0]), a1 = fabsf(p[1]), a2 = fabsf(p[2]);
        const float mag = fmaxf(a0, fmaxf(a1, a2));
        if (mag < 1.f) {
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = g[k] * 0.25f;
        } else {
            // y = s(m) p, s = 2/m - 1/m^2, m = |p_a| (a = argmax):  dy_i/dp_j = s delta_ij + p_i s'(m) sign(p_a) delta_ja
            const int am = (a0 >= a1 && a0 >= a2) ? 0 : (a1 >= a2 ? 1 : 2);
            const float inv = 1.f / mag;
            const float s = (2.f - inv) * inv;
            const float ds = (-2.f * inv * inv) + (2.f * inv * inv * inv);
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) dot += g[k] * p[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) out[k] = 0.25f * s * g[k];
            out[am] += 0.25f * dot * ds * (p[am] >= 0.f ? 1.f : -1.f);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) out[k] = g[k] / (box.hi[k] - box.lo[k]);
    }
    float x[3];
    const bool s = unit_cube_coords(p, contraction, box, x);      // the forward's selector, bit for bit
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = s ? out[k] : 0.f;
}
