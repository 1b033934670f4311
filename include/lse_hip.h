/*
 * lse_hip.h -- C-ABI of the MI355X (gfx950) LSENeRF hot path.
 *
 * This is the drop-in boundary named by BASELINE.json `north_star`: the entry points below are what a
 * Python binding replaces `tinycudann._C` and `nerfacc.cuda._C` with for the path
 *     LSENeRFModel.exec_get_outputs            R:lse_nerf/lsenerf.py:278-326
 *       -> LSEOccGridEstimator.sampling        R:lse_nerf/lse_grid_estimator.py:15-143
 *       -> LSEField.get_density / get_outputs  R:lse_nerf/lse_field.py:264-360
 *       -> nerfacc volrend + renderers         R:lse_nerf/lsenerf.py:300-318, R:lse_nerf/lse_renderer.py:4-10
 * (`R:` = /root/reference/).  INTEGRATION.md shows the ctypes stubs a maintainer of the reference adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless its name starts with `h_` or it is a `*_desc` struct (host);
 *   - tensors are dense row-major fp32 unless stated; sizes are element counts;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued on it and
 *     nothing synchronises: callers own ordering, memory and lifetime (no allocation inside the library);
 *   - return value: 0 = OK, <0 = error (LSE_E_*), message via lse_last_error();
 *   - functions marked "accumulate" add into their output (callers zero it), others overwrite;
 *   - NO GLOBAL OR THREAD-LOCAL STATE (ABI 5): every entry point is a function of its arguments alone -- what a call does never
 *     depends on an earlier call.  Kernel variants, arithmetic conventions and device-side sample counts are call arguments
 *     (lse_hash_bwd_opts, lse_mlp_desc.arith, `flags`, `n_dev`); there is nothing to set, reset or bracket, and any number of
 *     host threads may call concurrently on their own streams.  The one thread-local datum is the MESSAGE of the calling thread's
 *     last failed call (lse_last_error): written by a failing call, never read by the library.  The tuning knobs of the
 *     development build (csrc/dev_knobs.h, `make dev` -> liblse_hip_dev.so) are not part of this library.
 */
#ifndef LSE_HIP_H
#define LSE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LSE_ABI_VERSION 6

#define LSE_OK 0
#define LSE_E_INVALID (-1)   /* bad argument (null pointer, unsupported size) */
#define LSE_E_LAUNCH (-2)    /* HIP launch / runtime error */
#define LSE_E_UNSUPPORTED (-3)

#define LSE_MAX_GRID_LEVELS 32
#define LSE_MAX_OCC_LEVELS 8

typedef void *lse_stream_t;

/* ---- descriptors ------------------------------------------------------------------------------------ */

/* tiny-cuda-nn HashGrid level table (replaces tcnn.Encoding(...) built at R:lse_nerf/lse_field.py:72-86).
 * offsets are in ENTRIES of n_features floats; offsets[n_levels] = total entries. */
typedef struct lse_grid_desc {
    int32_t n_levels;
    int32_t n_features;                              /* 2 */
    uint32_t offsets[LSE_MAX_GRID_LEVELS + 1];
    float scales[LSE_MAX_GRID_LEVELS];               /* grid_scale(level)            */
    uint32_t resolutions[LSE_MAX_GRID_LEVELS];       /* grid_resolution(scale)       */
} lse_grid_desc;

#define LSE_IN_ROWMAJOR 0   /* in[N, n_in]                                                           */
#define LSE_IN_LEVELMAJOR 1 /* in[n_in/2][N][2]  (the layout lse_hash_fwd writes)                      */
#define LSE_ACT_NONE 0
#define LSE_ACT_SIGMOID 1

/* Bias-free fused MLP in tcnn parameter layout (replaces tcnn.Network via nerfstudio MLP,
 * R:lse_nerf/lse_field.py:199-207 and :254-262): params = [W_0 (width x n_in) | W_h (width x width) x
 * (n_hidden_layers-1) | W_out (16 x width)], each row-major [out,in].  Output always padded to 16. */
typedef struct lse_mlp_desc {
    int32_t n_in;            /* 8, 16, 32 or 64 (padded input width)                */
    int32_t width;           /* 32 or 64                                            */
    int32_t n_hidden_layers; /* 1 or 2                                              */
    int32_t out_activation;  /* LSE_ACT_*                                           */
    int32_t in_layout;       /* LSE_IN_*                                            */
    /* optional first-layer VIEW into params / d_params (all zero = the plain layout above):
     * W_0[row][c] = params[row * w0_ld + w0_col + c] for c < n_in, the other layers follow at params + width * w0_ld.
     * w0_mask_col0: input column 0 has no weight (reads 0, gets no gradient).  The head MLP uses (w0_ld 64, w0_col 15,
     * mask 1): its per-sample input h[N,16] = [density logit | 15 geometry features] meets columns 16..30 of tcnn's
     * [width x 64] input matrix in place (R:lse_nerf/lse_field.py:254-262, :347-356) -- no per-step split copy. */
    int32_t w0_ld, w0_col, w0_mask_col0;
    /* arithmetic route of the FORWARD where two are built (width 64 with 16 row-major or 32 inputs): LSE_MLP_ARITH_AUTO = the
     * bf16-piece kernels (f32 operands cut into three bf16 pieces, six piece products per multiply on the bf16 matrix cores, f32
     * accumulate: the f32 error bound, csrc/mlp_x6.h); LSE_MLP_ARITH_F32_MFMA = v_mfma_f32_16x16x4_f32 (what every other shape
     * runs on).  The two routes differ in the last bits, both within f32 rounding of the exact result.  The backward's route
     * follows act_tiled (3 = bf16 pieces).
     * LSE_MLP_ARITH_BF16X3 / LSE_MLP_ARITH_BF16X1: reduced-piece INFERENCE forward of the same two shapes (lse_mlp_fwd with
     * nothing saved -- act == NULL, or act_tiled == 3 whose act is ignored -- and lse_mlp_fwd_pair with the same route in both
     * descriptors; anything else, every backward included, is LSE_E_UNSUPPORTED).  With NP = 2 (BF16X3) or 1 (BF16X1) pieces per
     * operand, cut by round-to-nearest-even (p0 = bf16_rn(x), p1 = bf16_rn(x - p0), weights and activations alike), a layer's
     * pre-activation is the row bias (f32, uncut) plus exactly the piece products a_i * b_j with i + j < NP -- hi*hi + hi*mid +
     * mid*hi, or hi*hi alone -- each exact in f32 and accumulated in f32 on the matrix core.  Activations, density head, stores,
     * n_dev and tails are those of LSE_MLP_ARITH_AUTO.  Relative error of a multiply: 2^-16 (BF16X3), 2^-8 (BF16X1). */
    int32_t arith;
} lse_mlp_desc;
#define LSE_MLP_ARITH_AUTO 0
#define LSE_MLP_ARITH_F32_MFMA 1
#define LSE_MLP_ARITH_BF16X3 2
#define LSE_MLP_ARITH_BF16X1 3

/* ---- misc -------------------------------------------------------------------------------------------- */
int lse_abi_version(void);
const char *lse_last_error(void);

/* ---- sampler: replaces nerfacc.grid.traverse_grids + the mask extraction at
 *      R:lse_nerf/lse_grid_estimator.py:93-106.  Two passes like the upstream kernel:
 *      mode 0 fills chunk_cnts[R]; mode 1 reads chunk_starts[R] and writes the packed samples.
 *      binaries [levels, rx, ry, rz] uint8; aabbs [levels, 6]; near/far per ray.  Integer outputs are
 *      bit-exact against oracle/c/lse_oracle.c.
 *      flags: 0 = every product and sum of the traversal set-up rounded separately (bit-exact against
 *      oracle/c/liblse_oracle.so); LSE_TRAVERSE_FMA_SETUP = the a*b+c sites of nerfacc's grid.cu (ray start / end, the two
 *      products of tmax_xyz) as fused multiply-adds -- what nvcc's default contraction emits -- bit-exact against
 *      liblse_oracle_fma.so.  The two conventions differ in about one sample interval per million. ------------ */
#define LSE_TRAVERSE_FMA_SETUP 1
int lse_traverse_grids(const float *rays_o, const float *rays_d, int32_t n_rays, const uint8_t *binaries,
                       const float *aabbs, int32_t levels, int32_t rx, int32_t ry, int32_t rz,
                       const float *near_planes, const float *far_planes, float step_size, float cone_angle,
                       int32_t mode, int64_t *chunk_cnts, const int64_t *chunk_starts, int32_t *ray_indices,
                       float *t_starts, float *t_ends, int32_t flags, lse_stream_t stream);

/* Single-pass variant of the same traversal (same arithmetic, same samples): ray r writes its (t_start, t_end) pairs into
 * the fixed-capacity slots [r*cap, (r+1)*cap) and its count into chunk_cnts[r]; *overflow is OR-ed with 1 if a ray
 * produced more than cap samples (the caller then falls back to the two-pass calls above).  The host bound
 * cap >= (t_exit - t_enter) / step_size + slack holds because every sample interval is at least step_size long.
 * lse_compact_ray_slots packs the slots: ray_indices / t_starts / t_ends [N] at packed_info[r] = (start, count). */
int lse_traverse_grids_slots(const float *rays_o, const float *rays_d, int32_t n_rays, const uint8_t *binaries,
                             const float *aabbs, int32_t levels, int32_t rx, int32_t ry, int32_t rz,
                             const float *near_planes, const float *far_planes, float step_size, float cone_angle,
                             int64_t cap, int64_t *chunk_cnts, float *t_start_slots, float *t_end_slots,
                             int32_t *overflow, int32_t flags, lse_stream_t stream);
int lse_compact_ray_slots(const float *t_start_slots, const float *t_end_slots, int64_t cap, const int64_t *packed_info,
                          int32_t n_rays, int32_t *ray_indices, float *t_starts, float *t_ends, lse_stream_t stream);

/* nerfacc.pack_info (R:lse_nerf/lsenerf.py:300): packed_info[R,2] = (exclusive cumsum, count); total[1]. */
int lse_pack_info_from_counts(const int64_t *chunk_cnts, int32_t n_rays, int64_t *packed_info, int64_t *total,
                              lse_stream_t stream);
/* nerfstudio VolumetricSampler.forward: "if num_samples == 0: create a single fake sample" (ray 0, starts = ends = 1,
 * packed_info[0] = (0, 1)) -- applied on the device to a device-side count (*n_dev == 0 -> 1).  Arrays need room for 1 sample.
 * feat_x01 [C,3] / feat_sel [C] / feat_y [n_levels][y_level_stride floats] (each nullable; ABI 4): the visibility pre-pass's
 * compacted survivor features that the main pass re-uses (lse_compact_features).  With no survivor they hold nothing for slot 0,
 * where the fake sample lands: the slot is zeroed (the sample has zero extent -- weight and gradients exactly 0 -- so any FINITE
 * features give the reference's outputs; uninitialised ones may hold NaN). */
int lse_fake_sample_if_empty(int64_t *packed_info, int32_t n_rays, int64_t *n_dev, int32_t *ray_indices, float *t_starts,
                             float *t_ends, float *feat_x01, uint8_t *feat_sel, float *feat_y, int64_t y_level_stride,
                             int32_t n_levels, int32_t n_features, lse_stream_t stream);

/* Per-ray near / far planes of R:lse_nerf/lse_grid_estimator.py:83-92 in one launch (bit-identical to the torch ops):
 * near = max(near_plane, t_min[r]) (+ jitter[r] * step_size when jitter is given: stratified sampling),
 * far = min(far_plane, t_max[r]).  t_min / t_max / jitter are nullable. */
int lse_ray_planes(float near_plane, float far_plane, const float *t_min, const float *t_max, const float *jitter,
                   float step_size, int32_t n_rays, float *near_planes, float *far_planes, lse_stream_t stream);

/* nerfacc.render_visibility_from_density (R:lse_nerf/lse_grid_estimator.py:120-127): mask[N] uint8 and the
 * per-ray surviving counts new_cnts[R]. */
int lse_visibility_mask(const float *t_starts, const float *t_ends, const float *sigmas,
                        const int64_t *packed_info, int32_t n_rays, float early_stop_eps, float alpha_thre,
                        uint8_t *mask, int64_t *new_cnts, lse_stream_t stream);
/* The same with R:lse_nerf/lse_grid_estimator.py:112-116's `alpha_thre = min(alpha_thre, self.occs.mean().item())` evaluated on
 * the device: alpha_cap points to occs.mean() in device memory (no host read-back; a captured launch follows grid refreshes). */
int lse_visibility_mask_cap(const float *t_starts, const float *t_ends, const float *sigmas,
                            const int64_t *packed_info, int32_t n_rays, float early_stop_eps, float alpha_thre,
                            const float *alpha_cap, uint8_t *mask, int64_t *new_cnts, lse_stream_t stream);
/* Survivors of the visibility culling keep what the sigma_fn pre-pass computed for them: x01[N,3], selector[N] and the
 * level-major hash features y[L][N][2] (F = 2) are compacted with the same mask / packed_info pair as
 * lse_compact_samples, so the main field pass does not encode them again (R:lse_nerf/lse_grid_estimator.py:109-143 evaluates
 * the field twice on every survivor). */
int lse_compact_features(const uint8_t *mask, const int64_t *packed_info, const int64_t *new_packed_info, int32_t n_rays,
                         const float *x01, const uint8_t *selector, const float *y, int32_t n_levels, int64_t n_old,
                         int64_t n_new, float *out_x01, uint8_t *out_selector, float *out_y, lse_stream_t stream);

/* nerfacc.render_visibility_from_alpha (the alpha_fn branch, R:lse_nerf/lse_grid_estimator.py:128-138): same scan on
 * per-sample opacities; T_k = prod_{i<k} (1 - alpha_i), mask = T >= early_stop_eps && alpha >= alpha_thre. */
int lse_visibility_mask_alpha(const float *alphas, const int64_t *packed_info, int32_t n_rays, float early_stop_eps,
                              float alpha_thre, uint8_t *mask, int64_t *new_cnts, lse_stream_t stream);

/* mask compaction at R:lse_nerf/lse_grid_estimator.py:139-143 (order preserving, per ray). */
int lse_compact_samples(const uint8_t *mask, const int64_t *packed_info, const int64_t *new_packed_info,
                        int32_t n_rays, const int32_t *ray_indices, const float *t_starts, const float *t_ends,
                        int32_t *out_ray_indices, float *out_t_starts, float *out_t_ends, lse_stream_t stream);

/* ---- field ------------------------------------------------------------------------------------------- */

/* Device-side sample count `n_dev` (nullable) of the PER-SAMPLE entry points
 *     lse_positions_fwd / _bwd, lse_hash_fwd, lse_hash_bwd / _levels / _ex / _input, lse_mlp_fwd / _fwd_pair / _bwd.
 * The sampler knows the number of packed samples only on the device (lse_pack_info_from_counts); reading it back costs a host
 * synchronisation per sampler call, twice per step with the visibility pre-pass.  With n_dev != NULL the `n` argument is a
 * CAPACITY -- buffer extents, level strides and the launch grid are sized by it -- and every kernel clamps it to the int64 that
 * n_dev addresses when it starts; workgroups past the count leave at once.  Nothing at or beyond the count is read or written.
 * The per-ray entry points (visibility, compaction, volume rendering, ray reductions) take their counts from packed_info.
 * (Until ABI 4 this pointer was ambient per-thread state, lse_set_device_count.) */

/* R:lse_nerf/lse_field.py:266-274: pos = o[ri] + d[ri]*(ts+te)/2 -> L-inf contraction -> (x+2)/4 (contraction=1)
 * or aabb normalisation (contraction=0, h_aabb[6]) -> selector -> x*selector.  ray_idx==NULL: rays_o holds N
 * positions directly (Field.density_fn). */
int lse_positions_fwd(const float *rays_o, const float *rays_d, const int32_t *ray_idx, const float *t_starts,
                      const float *t_ends, int64_t n, const int64_t *n_dev, int32_t contraction, const float *h_aabb,
                      float *x01, uint8_t *selector, lse_stream_t stream);
/* d(pos)[N,3] from d(x01)[N,3] (Jacobian of contraction/normalisation, selector-masked). */
int lse_positions_bwd(const float *rays_o, const float *rays_d, const int32_t *ray_idx, const float *t_starts,
                      const float *t_ends, int64_t n, const int64_t *n_dev, int32_t contraction, const float *h_aabb,
                      const float *d_x01, float *d_pos, lse_stream_t stream);
/* per-ray sums: d_o[r] = sum d_pos, d_d[r] = sum d_pos*(ts+te)/2 over the ray's packed samples. */
int lse_ray_grad_reduce(const float *d_pos, const float *t_starts, const float *t_ends, const int64_t *packed_info,
                        int32_t n_rays, float *d_rays_o, float *d_rays_d, lse_stream_t stream);

/* lse_positions_bwd -> lse_ray_grad_reduce in one launch for the ray path (one wave per ray over packed_info): d(pos) is formed
 * per sample from d_x01 and summed on the fly, in the order lse_ray_grad_reduce sums it, so d_rays_o / d_rays_d (either nullable)
 * carry the same bits and d_pos[N,3] is neither written nor read.  Replaces the two calls at the end of the backward of
 * R:lse_nerf/lse_field.py:266-274 when the positions come from rays.  Per-ray entry point: counts come from packed_info. */
int lse_ray_grad_from_dx01(const float *rays_o, const float *rays_d, const float *t_starts, const float *t_ends,
                           const int64_t *packed_info, int32_t n_rays, int32_t contraction, const float *h_aabb,
                           const float *d_x01, float *d_rays_o, float *d_rays_d, lse_stream_t stream);

/* tcnn kernel_grid forward (R:lse_nerf/lse_field.py:279 via HashEncoding.forward): x01[N,3] -> y[L][N][F]. */
int lse_hash_fwd(const lse_grid_desc *desc, const float *x01, const float *table, float *y, int64_t n,
                 const int64_t *n_dev, lse_stream_t stream);
/* tcnn kernel_grid_backward (+_input): dtable accumulate (float atomics); dx[N,3] overwritten (NULL: skip). */
int lse_hash_bwd(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table, float *dtable,
                 float *dx, int64_t n, const int64_t *n_dev, lse_stream_t stream);

/* The same backward restricted to levels [level_begin, level_end); dx_accumulate != 0 adds this launch's share to dx.
 * Lets the caller finish the fine levels' table gradients (most of the bytes) first and start their all-reduce while
 * the remaining levels are still being computed (lsenerf_amd.dist.OverlappedGradExchange). */
int lse_hash_bwd_levels(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table,
                        float *dtable, float *dx, int32_t dx_accumulate, int32_t level_begin, int32_t level_end,
                        int64_t n, const int64_t *n_dev, lse_stream_t stream);

/* Options of the hash backward as CALL ARGUMENTS (so that two settings can be compared inside one process):
 *   impl          2 = lane-per-sample kernel with a per-wave LDS cache of 512 table sectors (32 B, paired by 64-B line, keyed by
 *                     GLOBAL sector id), the run ends of several levels batched into one cache pass, one wave per workgroup
 *                     (default; csrc/hashgrid.hip); 0 = 16-lanes-per-sample kernel (also taken when a level does not start on a
 *                     64-byte line)
 *   stage_max     impl 2: with an empty queue, a level that ends more than stage_max runs in the wave passes unstaged (default 48;
 *                     56 is better when the step size is constant: profiles/r05_hash_bwd_thresholds_final.txt)
 *   few_runs      impl 2: a wave that ends <= few_runs runs at a level adds them straight to memory (default 8; 3 is better when
 *                     the step size is constant)
 *   second_probe  impl 2: extra probe rounds (home slot + 2 * k, k = 1 .. second_probe) before a corner falls back to memory (default 3)
 *   replicas, replica_levels, workspace, workspace_bytes
 *                 the coarsest levels are a few thousand 64-byte lines that EVERY wave of a launch adds to, and the memory-side
 *                 atomic units serialise requests to one line: the direct adds (few_runs path) of the levels below
 *                 replica_levels (default 4: 1 MB of table) go to one of `replicas` (default 16, a power of two) zero-initialised copies
 *                 in `workspace`, chosen by the index of the wave's group of four, and a small kernel folds them into dtable at the end of the call
 *                 (leaving the workspace zero).  workspace == NULL (lse_hash_bwd, lse_hash_bwd_levels): no replicas, same values
 *   gran, rounds, dbg, interleave_from_scale, coarse_levels, prefetch
 *                 RESERVED: they selected development variants that are retired (DESIGN_HISTORY.md).  Leave them at the value
 *                 lse_hash_bwd_default_opts writes; any other value, and impl 1, is answered with LSE_E_UNSUPPORTED.
 * lse_hash_bwd / lse_hash_bwd_levels use lse_hash_bwd_default_opts(). */
typedef struct lse_hash_bwd_opts {
    int32_t impl, gran, few_runs, second_probe, rounds, dbg;
    float interleave_from_scale;
    int32_t stage_max;
    int32_t coarse_levels;
    int32_t replicas, replica_levels;
    void *workspace;            /* device memory, zero on entry, zero again when the call's kernels have run; NULL = no replicas */
    int64_t workspace_bytes;
    int32_t prefetch;           /* reserved (see above) */
} lse_hash_bwd_opts;
void lse_hash_bwd_default_opts(lse_hash_bwd_opts *opts);
/* bytes of `workspace` that lse_hash_bwd_ex needs for opts->replicas x the levels below opts->replica_levels (NULL = defaults).
 * The replicated levels stop at the first level that would push ONE replica past 2 MB (grids whose coarse levels are already
 * large gain nothing from replicas): 0 is a valid answer and means "no workspace, no replicas". */
int64_t lse_hash_bwd_workspace_bytes(const lse_grid_desc *desc, const lse_hash_bwd_opts *opts);
int lse_hash_bwd_ex(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table, float *dtable,
                    float *dx, int32_t dx_accumulate, int32_t level_begin, int32_t level_end, int64_t n,
                    const int64_t *n_dev, const lse_hash_bwd_opts *opts /* NULL = defaults */, lse_stream_t stream);

/* tcnn kernel_grid_backward_input alone, for a FROZEN table (test-time refinement): dx[N,3] = d(loss)/d(x01) from dy[L][N][2]
 * (level stride n, as lse_hash_bwd_ex reads it), overwritten.  The cell is the one lse_hash_fwd picks, out-of-range positions
 * included.  A pure gather: no table gradient, no workspace, no atomics; the levels are summed in a fixed order, so two calls
 * give the same bits.  Serves every geometry lse_hash_fwd serves (no level alignment needed).  Rows at or beyond the count are
 * not written. */
int lse_hash_bwd_input(const lse_grid_desc *desc, const float *x01, const float *dy, const float *table, float *dx,
                       int64_t n, const int64_t *n_dev, lse_stream_t stream);

/* fused MLP forward on the matrix cores (f32 MFMA, or bf16 MFMA on three-piece operands with the same error bound:
 * lse_mlp_desc.arith).  row_bias[R,width] (nullable) is added to layer-0 pre-activations of sample i
 * from row row_bias_idx[i].  act (nullable) receives the post-ReLU hidden activations: act_tiled = 0 -> row-major
 * [n_hidden_layers][N][width] (what lse_mlp_wgrad reads); act_tiled = 1 -> tile-major, an opaque workspace of
 * n_hidden_layers * roundup(N,16) * width floats that only lse_mlp_bwd (same act_tiled) understands; act_tiled = 2 (two
 * hidden layers, row-major input): tile-major WITHOUT the first hidden layer ((n_hidden_layers - 1) * roundup(N,16) * width
 * floats) -- lse_mlp_bwd recomputes it from `in` and `row_bias` (32 extra MFMAs per 32 samples against 2 KiB per sample of
 * activation traffic), bit-identical to what the forward computed;  act_tiled = 3 (width 64 with 16 row-major inputs and two
 * hidden layers, or 32 inputs and one): NOTHING is saved (act may be NULL) -- lse_mlp_bwd recomputes every hidden layer on the
 * bf16 matrix cores (three-piece operands, csrc/mlp_x6.h), fused weight gradients only (d_params required; d_out_pre / d_act /
 * d_act0 not available).
 * out is [N,16] (out_cols = 16) or the compact [N,4] holding outputs 0..3 (out_cols = 4, e.g. rgb).
 * sigma_out (nullable): fused density head sigma[N] = density_scale * exp(out[:,0]) * selector (trunc_exp,
 * R:lse_nerf/lse_field.py:286-287); selector nullable. */
int lse_mlp_fwd(const lse_mlp_desc *desc, const float *params, const float *in, const float *row_bias,
                const int32_t *row_bias_idx, float *out, int32_t out_cols, float *act, int32_t act_tiled,
                float *sigma_out, const uint8_t *selector, float density_scale, int64_t n, const int64_t *n_dev,
                lse_stream_t stream);
/* Base MLP (R:lse_nerf/lse_field.py:280-287: mlp_base_mlp + trunc_exp density) and head MLP (R:lse_nerf/lse_field.py:347-358: mlp_head)
 * on the same samples in ONE launch: per 32-sample tile the base output h stays in registers and is the head's k = 16 input
 * (same lane / register layout), so h[N,16] is written once (the backward and the caller read it) and never read back.
 * Equivalent to, and bitwise equal to,
 *     lse_mlp_fwd(base_desc, base_params, y, NULL, NULL, h, 16, NULL, 3, sigma, selector, density_scale, n, n_dev, stream);
 *     lse_mlp_fwd(head_desc, head_params, h, row_bias, row_bias_idx, out, out_cols, NULL, 3, NULL, NULL, 0, n, n_dev, stream);
 * Shapes: the recompute-all production pair only -- base 32 -> 64 -> 16 (one hidden layer, level-major or row-major input, no
 * output activation), head 16 -> 64 -> 64 -> 16 (row-major, first-layer view w0_ld / w0_col / w0_mask_col0 as in lse_mlp_fwd),
 * both LSE_MLP_ARITH_AUTO, or both the same reduced-piece route (the bitwise equality to two lse_mlp_fwd calls holds per
 * route); anything else is LSE_E_UNSUPPORTED (call lse_mlp_fwd twice).  Nothing is saved for the backward
 * (lse_mlp_bwd with act_tiled = 3 recomputes; LSE_MLP_ARITH_AUTO only).  selector, row_bias, row_bias_idx nullable as in lse_mlp_fwd. */
int lse_mlp_fwd_pair(const lse_mlp_desc *base_desc, const float *base_params, const float *y, const uint8_t *selector,
                     float density_scale, const lse_mlp_desc *head_desc, const float *head_params, const float *row_bias,
                     const int32_t *row_bias_idx, float *h, float *sigma, float *out, int32_t out_cols, int64_t n,
                     const int64_t *n_dev, lse_stream_t stream);
/* backward: d_out[N,out_cols] (w.r.t. the activated output) -> d_in (layout of desc->in_layout; nullable) and, when
 * d_params is given, the weight gradients of every layer accumulated into d_params (same layout as params) in the
 * same pass (`in` = the layer-0 input is then required).  d_sigma (nullable): gradient of the fused density head, folded
 * into the gradient of output 0 (trunc_exp backward: * density_scale * exp(clamp(out0,-15,15)) * selector).
 * Optional outputs: d_out_pre[N,16], d_act[n_hidden_layers][N][width] (pre-activation gradients of every layer, what
 * lse_mlp_wgrad consumes), d_act0[N][width] (layer 0 only: the row_bias gradient before the per-row sum), or directly
 * d_row_bias[rows][width] (accumulate; row_bias_idx[N] must be sorted, i.e. each row's samples contiguous). */
int lse_mlp_bwd(const lse_mlp_desc *desc, const float *params, const float *in, const float *act, int32_t act_tiled,
                const float *out, int32_t out_cols, const float *d_out, const float *d_sigma, const uint8_t *selector, float density_scale,
                float *d_out_pre, float *d_act, float *d_act0, float *d_in, float *d_params,
                const float *row_bias, const int32_t *row_bias_idx, float *d_row_bias, int64_t n, const int64_t *n_dev,
                lse_stream_t stream);
/* The data gradients of lse_mlp_bwd(act_tiled = 3) alone, for FROZEN parameters (test-time refinement): d_in (overwritten,
 * layout of desc->in_layout; nullable) and d_row_bias[rows][width] (accumulated; nullable, needs row_bias and a sorted
 * row_bias_idx), at least one of the two.  No weight-gradient product is formed and there is no d_params: every hidden layer is
 * recomputed from `in` (and row_bias) on the bf16 matrix cores (three-piece operands) and only the transposed-weight products
 * run.  out / out_cols / d_out / d_sigma / selector / density_scale as in lse_mlp_bwd.
 * Contract: d_in is BIT-EQUAL to what lse_mlp_bwd(act_tiled = 3) writes for the same arguments (the same matrix-core products
 * in the same order, no atomics), and two calls give the same bits.  d_row_bias sums the same f32 terms as lse_mlp_bwd in
 * another order (fixed inside a wave, float atomics across waves): equal up to f32 summation order, not bitwise.  Rows of d_in
 * at or beyond the count are not written.
 * Shapes: width 64 with 16 row-major inputs and two hidden layers (first-layer view w0_ld / w0_col / w0_mask_col0 honoured) or
 * 32 inputs (either layout) and one, LSE_MLP_ARITH_AUTO; anything else is LSE_E_UNSUPPORTED.  Keeps no state. */
int lse_mlp_bwd_input(const lse_mlp_desc *desc, const float *params, const float *in, const float *out, int32_t out_cols,
                      const float *d_out, const float *d_sigma, const uint8_t *selector, float density_scale, float *d_in,
                      const float *row_bias, const int32_t *row_bias_idx, float *d_row_bias, int64_t n, const int64_t *n_dev,
                      lse_stream_t stream);
/* d_in = d(out[0]) / d(in) of the base network (32 inputs in either layout, width 64, one hidden layer, no output activation,
 * LSE_MLP_ARITH_AUTO): the gradient of the density logit with respect to the hash features, for analytic normals.  This is
 * lse_mlp_bwd_input for a d_out of (1, 0, .., 0) without the seed: the hidden layer is recomputed on the bf16 matrix cores, the
 * output layer's backward is row 0 of the output matrix through the ReLU mask (no product), and neither `out` nor a d_out is read.
 * d_in is overwritten in the layout of desc->in_layout (level-major is what lse_hash_bwd_input reads); rows at or beyond the
 * count are not written; two calls give the same bits.  Any other shape or arithmetic route is LSE_E_UNSUPPORTED before any
 * launch.  Keeps no state. */
int lse_density_logit_grad(const lse_mlp_desc *desc, const float *params, const float *in, float *d_in, int64_t n,
                           const int64_t *n_dev, lse_stream_t stream);
/* unfused weight gradients from materialised d_act / d_out_pre, accumulate into d_params (same layout as params). */
int lse_mlp_wgrad(const lse_mlp_desc *desc, const float *in, const float *act, const float *d_act,
                  const float *d_out_pre, float *d_params, int64_t n, lse_stream_t stream);
/* out[R,width] += per-ray sum of d_act0[N,width] (gradient of row_bias). */
int lse_segment_sum_rows(const float *rows, int32_t width, const int64_t *packed_info, int32_t n_rays, float *out,
                         lse_stream_t stream);

/* per-ray head features in tcnn column order [SH16(dir) | 15 zeros (geo slots) | emb(32) | 1]
 * (R:lse_nerf/lse_field.py:298-300, 306-310, 347-356; SH of tcnn, degree 4). emb_table NULL -> zeros. */
int lse_ray_features_fwd(const float *rays_d, const float *emb_table, const int32_t *emb_idx, int32_t n_rays,
                         int32_t emb_dim, float *feat, lse_stream_t stream);
/* d_rays_d[R,3] overwritten (nullable); d_emb_table[n_emb_rows, emb_dim] accumulate (nullable). */
int lse_ray_features_bwd(const float *rays_d, const float *d_feat, const int32_t *emb_idx, int32_t n_rays,
                         int32_t emb_dim, int32_t n_emb_rows, float *d_rays_d, float *d_emb_table, lse_stream_t stream);
/* small dense helpers on per-ray matrices: y[R,M] = x[R,K] W[M,K]^T ; dx[R,K] = dy[R,M] W[M,K] ;
 * dW[M,K] += dy^T x. */
/* The same features AND the per-ray share of the head's first layer in one launch:
 *   feat[R, in_pad] = [SH16 | 0 x 15 | emb (emb_dim) | ones padding],  in_pad = roundup(31 + emb_dim, 16)  (tcnn's layout);
 *   0 <= emb_dim <= 97 (the reference's LSEEmbeddingConfig.emb_dim, default 32: in_pad 64)
 *   row_bias[R, width] = feat * W_in^T with W_in[width][w_ld] the head's tcnn input matrix in place.
 * Backward: d_feat[R, in_pad] = d_row_bias * W_in (workspace, overwritten), d_rays_d[R,3] (nullable) through the SH
 * Jacobian, d_emb_table[n_emb_rows, emb_dim] (nullable, accumulate).  The weight gradient d W_in += d_row_bias^T feat is
 * lse_gemm_tn_acc(d_row_bias, width, feat, in_pad, ..., dw_ld = w_ld) straight into the parameter gradient. */
int lse_ray_bias_fwd(const float *rays_d, const float *emb_table, const int32_t *emb_idx, int32_t n_rays,
                     int32_t emb_dim, const float *w_in, int32_t w_ld, int32_t width, float *feat, float *row_bias,
                     lse_stream_t stream);
int lse_ray_bias_bwd(const float *rays_d, const int32_t *emb_idx, int32_t n_rays, int32_t emb_dim, int32_t n_emb_rows,
                     const float *w_in, int32_t w_ld, int32_t width, const float *d_row_bias, float *d_feat,
                     float *d_rays_d, float *d_emb_table, lse_stream_t stream);
int lse_linear_fwd(const float *w, const float *x, int32_t rows, int32_t m, int32_t k, float *y, lse_stream_t stream);
int lse_linear_bwd_input(const float *w, const float *dy, int32_t rows, int32_t m, int32_t k, float *dx,
                         lse_stream_t stream);
int lse_gemm_tn_acc(const float *g, int32_t m, const float *a, int32_t k, int32_t a_layout, int64_t n, float *dw,
                    int32_t dw_ld, lse_stream_t stream);

/* density = scale * exp(h[:,0]) * selector (trunc_exp, R:lse_nerf/lse_field.py:286-287); h is [N,16]. */
int lse_density_fwd(const float *h, const uint8_t *selector, float scale, float *sigma, int64_t n, lse_stream_t stream);
/* d_h[:,0] = d_sigma * scale * exp(clamp(h0,-15,15)) * selector (overwrites column 0 only). */
int lse_density_bwd(const float *h, const uint8_t *selector, float scale, const float *d_sigma, float *d_h, int64_t n,
                    lse_stream_t stream);

/* ---- renderer: nerfacc.render_weight_from_density + accumulate_along_rays
 *      (R:lse_nerf/lsenerf.py:301-318, R:lse_nerf/lse_renderer.py:6-10).  rgb has row stride rgb_stride floats. */
int lse_volrend_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                    int32_t rgb_stride, const int64_t *packed_info, int32_t n_rays, float *weights, float *out_rgb,
                    float *out_acc, float *out_depth_num, lse_stream_t stream);
int lse_volrend_bwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                    int32_t rgb_stride, const int64_t *packed_info, int32_t n_rays, const float *weights,
                    const float *d_out_rgb, const float *d_out_acc, const float *d_out_depth_num, float *d_sigmas,
                    float *d_rgb, lse_stream_t stream);

/* lse_volrend_fwd + the DepthRenderer("expected") epilogue of R:lse_nerf/lsenerf.py:315-317 in the same call:
 * out_depth[r] = clip(out_depth_num[r] / (out_acc[r] + 1e-10), lo, hi) with (lo, hi) the global min / max of the interval
 * mid-points (nerfstudio clips to steps.min() / steps.max()); samples are sorted inside a ray, so the range is reduced
 * from the per-ray first / last mid-point (mid_range [R,2], workspace) instead of two passes over all N samples.
 * depth_range[2] (nullable) receives (lo, hi) for the backward. */
int lse_volrend_depth_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb,
                          int32_t rgb_stride, const int64_t *packed_info, int32_t n_rays, float *weights, float *out_rgb,
                          float *out_acc, float *out_depth_num, float *mid_range, float *out_depth, float *depth_range,
                          lse_stream_t stream);
/* nerfacc.render_weight_from_density alone (R:lse_nerf/lsenerf.py:301-306): weights, and optionally transmittance and
 * alphas per sample; the backward takes a per-sample d_weights (the generic route: renderers applied by the caller). */
int lse_render_weight_fwd(const float *t_starts, const float *t_ends, const float *sigmas, const int64_t *packed_info,
                          int32_t n_rays, float *weights, float *trans, float *alphas, lse_stream_t stream);
int lse_render_weight_bwd(const float *t_starts, const float *t_ends, const float *sigmas, const int64_t *packed_info,
                          int32_t n_rays, const float *weights, const float *d_weights, float *d_sigmas,
                          lse_stream_t stream);

/* Distortion loss of mip-NeRF 360 (nerfacc.losses.distortion) on the render weights of packed, ray-sorted samples (csrc/volrend.hip;
 * ABI 6, additive).  One 64-lane wave per ray, no atomics, no LDS, no workspace, the same inputs give the same bits.  Per ray with
 * samples [a_k, b_k), k = 0 .. n-1, mid-points non-decreasing (how the marcher emits them), weights w_k as lse_volrend_fwd /
 * lse_volrend_depth_fwd / lse_render_weight_fwd wrote them, and the host scalar t_scale >= 0 (finite):
 *   m_k = t_scale * ((a_k - a_0) + (b_k - b_0)) / 2   the scaled mid-point RELATIVE TO THE RAY'S FIRST -- L and dL/dw do not change
 *                                                     under m -> m - c, and without the shift m_i W_<i - M_<i cancels at the size of t;
 *   delta_k = t_scale * (b_k - a_k),   W_<i = sum_{j<i} w_j,   M_<i = sum_{j<i} w_j m_j   (W_>i, M_>i: the sums over j > i);
 *   L       = sum_i sum_j w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i  =  2 sum_i w_i (m_i W_<i - M_<i) + (1/3) sum_i w_i^2 delta_i
 *   dL/dw_i = 2 [m_i (W_<i - W_>i) - (M_<i - M_>i)] + (2/3) w_i delta_i.
 * lse_distortion_fwd: out_loss [n_rays] = L; out_totals [n_rays,2] (nullable) = (W_tot, M_tot) = (sum w, sum w m), what the backward
 *   takes in place of a pass of its own.
 *     a ray without samples: L = 0, totals (0, 0);  one sample: the second term alone, w_0^2 delta_0 / 3;
 *     weights are in [0, 1] whatever the density (sigma = 3e38, +inf): every output is finite.
 * lse_distortion_bwd: g = g_loss[r * g_stride] -- the upstream gradient per ray (g_stride 1) or one device scalar for all rays
 *   (g_stride 0); totals: out_totals of the forward over the same inputs.
 *     d_weights (nullable) [N]: g * dL/dw_i -- the generic route, the caller composites with the weights;
 *     d_sigmas (nullable) [N]: that gradient through render_weight_from_density in the same launch, by the recurrence of
 *        lse_volrend_bwd:  d_sigma_k = (b_k - a_k) (dw_k (T_end + W_>k) - sum_{i>k} dw_i w_i);
 *     sigmas (nullable; read only for d_sigmas): the densities the weights came from.  Given, T_end = exp(-sum_k sigma_k (b_k - a_k));
 *        null, T_end = 1 - W_tot, which on an opaque ray is 0 or +-2^-24 by the last bits of the forward's expf -- behind a surface
 *        that leaves dw_k 2^-24 (b_k - a_k) where the true d_sigma is ~ 0, and this loss's dw grows with the distance from the ray's
 *        centre of mass.  Pass them wherever they exist.  d_weights does not depend on them;
 *     at least one of the two outputs is given; every sample a packed_info row covers is written, nothing else is (no zero-fill
 *     needed; a ray without samples writes nothing).  t_starts / t_ends are not differentiated.
 * Sample arrays may have capacity extent: packed_info [n_rays,2] = (start, count) int64 rows are authoritative.  t_scale negative,
 * NaN or infinite, a g_stride other than 0 / 1 or a missing pointer: LSE_E_INVALID, checked before anything is launched. */
int lse_distortion_fwd(const float *t_starts, const float *t_ends, const float *weights, const int64_t *packed_info, int32_t n_rays,
                       float t_scale, float *out_loss, float *out_totals, lse_stream_t stream);
int lse_distortion_bwd(const float *t_starts, const float *t_ends, const float *sigmas, const float *weights,
                       const int64_t *packed_info, int32_t n_rays, float t_scale, const float *totals, const float *g_loss,
                       int32_t g_stride, float *d_weights, float *d_sigmas, lse_stream_t stream);

/* Forward-only compositing of an EVALUATION render (no autograd, nothing kept for a backward pass): the per-ray walk and summation
 * order of lse_volrend_depth_fwd, bit for bit, plus the renderer epilogue of LSENeRFModel.render_packed in the same call:
 *   flags & LSE_EVAL_NAN_TO_NUM: torch.nan_to_num of the three colour columns per sample (renderers other than LinearRenderer);
 *   depth = clip(num / (acc + 1e-10), lo, hi), (lo, hi) the min / max interval mid-point over the n_rays rays of this call (always);
 *   flags & LSE_EVAL_BACKGROUND: rgb + background * (1 - acc)   ("black" 0 / "white" 1);
 *   flags & LSE_EVAL_CLAMP: clamp(rgb, 0, 1), NaN propagated like torch.clamp.
 * Sample arrays may have capacity extent: packed_info rows are authoritative.  The outputs out_rgb [n,3], out_acc [n], out_depth [n],
 * out_nsamples [n] (int64: the packed_info counts) may be row offsets into a larger image.  workspace: 3 * n_rays floats. */
#define LSE_EVAL_NAN_TO_NUM 1
#define LSE_EVAL_BACKGROUND 2
#define LSE_EVAL_CLAMP 4
int lse_eval_composite(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb, int32_t rgb_stride,
                       const int64_t *packed_info, int32_t n_rays, int32_t flags, float background, float *workspace, float *out_rgb,
                       float *out_acc, float *out_depth, int64_t *out_nsamples, lse_stream_t stream);

/* Rendered normals of an evaluation render, one launch: the per-ray walk and the render weights w_i of lse_eval_composite over
 * the same t_starts / t_ends / sigmas / packed_info (capacity-extent sample arrays, packed_info authoritative), applied to
 *   n_i = -g_i / max(|g_i|, 1e-12),   g_i = d_x01[i]  (the gradient of the density logit with respect to the unit-cube position),
 *   N = sum_i w_i n_i,   and with LSE_NORMALS_RENORMALIZE   N / (|N| + 1e-10)        (nerfstudio's NormalsRenderer).
 * LSE_NORMALS_WORLD multiplies g_i by the transposed Jacobian of the position map at the sample (what lse_positions_bwd applies:
 * contraction or aabb normalisation, selector-masked) before it is normalised; it needs rays_o, rays_d [n_rays,3] and, without
 * contraction, h_aabb[6] -- all three are unused and nullable otherwise.  A zero gradient gives a zero normal, a ray without
 * samples or with zero weights gives (0, 0, 0); a NaN sigma propagates as in lse_eval_composite.  out_normals [n_rays,3] may be a
 * row offset into a larger image.  No atomics, no workspace, no state. */
#define LSE_NORMALS_WORLD 1
#define LSE_NORMALS_RENORMALIZE 2
int lse_eval_composite_normals(const float *t_starts, const float *t_ends, const float *sigmas, const float *d_x01,
                               const int64_t *packed_info, int32_t n_rays, const float *rays_o, const float *rays_d,
                               int32_t contraction, const float *h_aabb, int32_t flags, float *out_normals, lse_stream_t stream);

/* The same compositing walked in SEGMENTS of the ray, for early ray termination: between two segments the caller evaluates the field
 * only on the rays that are still alive.  Ray sample k meets lane k mod 64 in lse_eval_composite; every segment but the last ends
 * at a multiple of 64 samples, the lane accumulators are carried un-reduced, and the arithmetic is that kernel's operation by
 * operation -- so a ray that composited its first m samples here has, bit for bit, the outputs lse_eval_composite gives for a
 * packed_info count of m.  The library keeps nothing: the caller owns `state`.
 *   lse_eval_segment_state_bytes: size of `state` for n_rays rays (1312 bytes per ray: 5 x 64 lane accumulators, the scan's carry,
 *      the mid-point range, the composited count, the alive flag); the buffer is 16-byte aligned.
 *   lse_eval_segment_begin: resets the state of every ray and writes the sample counts of segment 0,
 *      seg_cnts[r] = min(ray_cnts[r], first_len).
 *   lse_eval_composite_segment: continues every ray over the samples seg_packed [R,2] = (start, count) assigns it in the packed arrays
 *      of THIS segment (t_starts / t_ends / sigmas / rgb [*, rgb_stride]; seg_packed counts are authoritative, so nerfstudio's fake
 *      sample composites on segment 0).  ray_cnts [R]: the rays' full counts; seg_end: samples of a ray covered once this segment is
 *      done (offset + length, a multiple of 64 unless next_len == 0).  A ray is finished when ray_cnts[r] <= seg_end or its carried
 *      optical depth (f32, as lse_eval_composite carries it between 64-sample groups) is >= tau_stop; +inf finishes it, NaN never
 *      does.  next_seg_cnts [R] (nullable when next_len == 0) = finished ? 0 : min(ray_cnts[r] - seg_end, next_len): the counts of
 *      the next segment, ready for lse_pack_info_from_counts.  Of `flags` only LSE_EVAL_NAN_TO_NUM acts here.
 *   lse_eval_composite_finish: the wave reductions and the epilogue of lse_eval_composite (background, clamp, depth clipped to the
 *      mid-point range of the samples that were composited over the n_rays rays); out_nsamples = samples composited per ray.
 *      Outputs may be row offsets into an image; workspace: 3 * n_rays floats. */
int lse_eval_segment_state_bytes(int32_t n_rays, int64_t *h_bytes);
int lse_eval_segment_begin(const int64_t *ray_cnts, int32_t n_rays, int64_t first_len, void *state, int64_t *seg_cnts,
                           lse_stream_t stream);
int lse_eval_composite_segment(const float *t_starts, const float *t_ends, const float *sigmas, const float *rgb, int32_t rgb_stride,
                               const int64_t *seg_packed, const int64_t *ray_cnts, int32_t n_rays, int32_t flags, int64_t seg_end,
                               int64_t next_len, float tau_stop, void *state, int64_t *next_seg_cnts, lse_stream_t stream);
int lse_eval_composite_finish(const void *state, int32_t n_rays, int32_t flags, float background, float *workspace, float *out_rgb,
                              float *out_acc, float *out_depth, int64_t *out_nsamples, lse_stream_t stream);

/* Quantile depths of an evaluation render (csrc/volrend.hip; ABI 6, additive): the depth at which a ray's accumulated weight
 * crosses q -- q = 0.5 is the median depth -- for up to four q at once.  One 64-lane wave per ray, the walk and the scan of
 * lse_eval_composite.  Per ray with samples [a_k, b_k), sigma_k, mid_k = (a_k + b_k) * 0.5f:
 *   tau_front(k), tau_behind(k): the optical depth in front of / behind sample k, as lse_eval_composite's scan forms them in f32
 *      (exclusive / inclusive prefix of sigma * dt inside the 64-sample group + the carry in front of the group; tau_behind of a
 *      group's last sample is the next group's carry, bit for bit).  The weights through sample k sum to 1 - exp(-tau_behind(k)),
 *      so  sum_{i<=k} w_i >= q   is   tau_behind(k) >= tau_q = -ln(1 - q):  nothing is summed, nothing cancels.
 *   k_j = the first k with tau_behind(k) >= tau_q[j]  (a NaN never compares true, +inf does).
 *   k_j exists:  depth_q[r][j] = mid_{k_j}; with LSE_DEPTH_INTERPOLATE  clamp(a + (tau_q[j] - tau_front(k_j)) / sigma, a, b) of that
 *      sample -- the exact crossing under piecewise-constant density; sigma = +inf gives a, a NaN quotient gives mid.  Bit j of
 *      reached[r] is set.
 *   no such k:   depth_q[r][j] = the mid-point of the ray's last sample (nerfstudio's clamp of searchsorted to n - 1); bit j clear.
 *   a ray without samples: depth_q[r][*] = 0.0f, reached[r] = 0.
 *   depth_sel[r] (nullable), sel = (flags >> 8) & 3 < n_q:  depth_q[r][sel] if bit sel of reached[r] is set and -- when max_spread is
 *      finite -- bit n_q - 1 is set too and depth_q[r][n_q - 1] - depth_q[r][0] <= max_spread;  NaN otherwise, which is what
 *      lse_unproject_append (the point is dropped) and lse_tsdf_integrate (the pixel is skipped without carving) take as "no usable
 *      depth".  max_spread >= 0; +inf: no spread test.
 * t_starts / t_ends / sigmas: packed f32, packed_info [n_rays,2] = (start, count) int64; h_tau_q: HOST array of n_q (1..4) strictly
 * ascending positive values; depth_q f32 [n_rays, n_q], reached u8 [n_rays], depth_sel f32 [n_rays]: may be row offsets into image
 * buffers.  No atomics, no LDS, no workspace.
 *   lse_eval_depth_quantiles_segment: the same walk over ONE segment of the early-stop route (seg_packed as for
 *      lse_eval_composite_segment).  state: [n_rays][2] 4-byte words owned by the caller -- the carry (f32) and the found mask (int32);
 *      all zero is the start, and it is independent of lse_eval_composite_segment's state.  A ray whose segment count is 0 is left
 *      alone, so depth_q / reached (/ depth_sel) must persist between the segments and start as what a ray without samples gets
 *      (0.0f / 0 (/ NaN)); a quantile found in an earlier segment is read back from depth_q, not written again.  After every
 *      segment depth_q holds the crossing where found and the mid-point of the last sample walked where not: once the last segment
 *      has run, the outputs are those of lse_eval_depth_quantiles over the samples walked, bit for bit. */
#define LSE_DEPTH_INTERPOLATE 1
int lse_eval_depth_quantiles(const float *t_starts, const float *t_ends, const float *sigmas, const int64_t *packed_info,
                             int32_t n_rays, int32_t n_q, const float *h_tau_q, int32_t flags, float max_spread, float *depth_q,
                             uint8_t *reached, float *depth_sel, lse_stream_t stream);
int lse_eval_depth_quantiles_segment(const float *t_starts, const float *t_ends, const float *sigmas, const int64_t *seg_packed,
                                     int32_t n_rays, int32_t n_q, const float *h_tau_q, int32_t flags, float max_spread, void *state,
                                     float *depth_q, uint8_t *reached, float *depth_sel, lse_stream_t stream);

/* ---- image metrics: SSIM and MSE of preds / target, contiguous f32 [B,C,H,W] with H, W >= 11 (else LSE_E_INVALID) -----------
 *      torchmetrics structural_similarity_index_measure(preds, target) with its defaults (R:lse_nerf/lsenerf.py:206, :512), restated
 *      from the published algorithm (parity unpinned): data_range R = max(max p - min p, max t - min t) on the device,
 *      C1 = (0.01 R)^2, C2 = (0.03 R)^2, h_window[11] (host) the normalised Gaussian taps used as their outer product, sigma^2 =
 *      E[x^2] - mu^2, mean over B*C and the (H-10) x (W-10) windows that lie inside the image.  out_mse = mean (p - t)^2 over every
 *      pixel.  Two device scalars, no host read-back, no atomics: fixed-order two-stage sums (deterministic), moments in double.
 *      workspace: lse_image_metrics_workspace bytes (8-byte aligned), written. */
int lse_image_metrics_workspace(int32_t B, int32_t C, int32_t H, int32_t W, int64_t *h_bytes);
int lse_image_metrics(const float *preds, const float *target, int32_t B, int32_t C, int32_t H, int32_t W, const float *h_window,
                      void *workspace, int64_t workspace_bytes, float *out_ssim, float *out_mse, lse_stream_t stream);

/* ---- eval images: a resident ground truth and a rendered image -> the planes lse_image_metrics takes ----------------------
 *   lse_eval_image_prep: one launch per image.  gt [H, W, 3] of gt_type (LSE_PIX_U8: value = (float)u8 / 255.0f, a division;
 *      LSE_PIX_F32: the value itself), msk [H, W] of msk_type (LSE_PIX_U8 | LSE_PIX_F32; LSE_PIX_NONE: msk is ignored), rgb
 *      [H * W, 3] f32 the rendered image.  Writes the contiguous [3, H, W] f32 planes gt_planes = value * msk and pred_planes =
 *      rgb * msk (no multiplication without a mask): R:lse_nerf/lsenerf.py:477-530's `image * msk` / `rgb * msk` after moveaxis.
 *      flags & LSE_PREP_EVENT_STATS: also the moments of the event-only metric (R:lse_nerf/lse_pipeline.py:149-164 over
 *      R:lse_nerf/utils.py:99-135) into `stats`: per pixel y = log(gray + 1e-6), gray = (0.2989 r + 0.5870 g) + 0.1140 b of the
 *      MASKED ground truth, and x = log((r + g) + 1e-6) of the UNMASKED prediction (the reference zeroes blue and sums the
 *      channels of the image dictionary's halves, of which only the ground truth is masked), sums and logarithms in double from
 *      the f32 pixels (the reference's are f32: with a prediction whose spread is 1e-3 of its level, f32 logarithms alone move the
 *      fitted slope by 5e-3); per workgroup the sums of x, x^2, y, x y in double, in a fixed order, no atomics.  stats:
 *      lse_log_scale_correct_workspace bytes, 8-byte aligned.
 *   lse_log_scale_correct: one launch.  Sums the partials in a fixed order and solves the normal equations of y ~ a x + b in double,
 *      N = H * W: det = N Sxx - Sx^2, a = (N Sxy - Sx Sy) / det, b = (Sxx Sy - Sx Sxy) / det.  A NaN a or b becomes 5/255 (the
 *      reference's rule); a det that is not finite, or zero to within the rounding of its two terms (|det| <= 2^-40 N Sxx), counts
 *      as NaN for both -- there the reference's torch.linalg.inv raises, or inverts rounding noise.  Writes coef[2] = (a, b) as
 *      f32, corrected[H * W] = expf((float)(a x + b)) and gray[H * W] (the grey masked ground truth): two [1, H, W] planes for
 *      lse_image_metrics with C = 1 (the reference feeds three identical channels, whose mean over C is this one's value).
 *      x is recomputed from rgb with the arithmetic of the prep launch; the gray PLANE is f32 with single roundings.  Two calls
 *      are bit-identical. */
#define LSE_PREP_EVENT_STATS 1
int lse_eval_image_prep(const void *gt, int32_t gt_type, const void *msk, int32_t msk_type, const float *rgb, int32_t H, int32_t W,
                        int32_t flags, float *gt_planes, float *pred_planes, void *stats, int64_t stats_bytes, lse_stream_t stream);
int lse_log_scale_correct_workspace(int32_t H, int32_t W, int64_t *h_bytes);
int lse_log_scale_correct(const float *gt_planes, const float *rgb, int32_t H, int32_t W, const void *stats, int64_t stats_bytes,
                          float *coef, float *corrected, float *gray, lse_stream_t stream);

/* ---- eval panels (csrc/panels.hip; ABI 6, additive): the images the reference's evaluation writes, as uint8, on the device -----
 * No host read-back, no host loop over device data, no cooperative launch or spin wait; every device loop is bounded by the image
 * size.  H * W < 2^30.  u8(v) below is (uint8) trunc(min(max(v * 255.0f, 0), 255)) with a NaN giving 0 (numpy's and torch's cast
 * of a NaN to uint8 is undefined; 0 is this library's choice).
 *   lse_gray8_planes: planes_a, planes_b f32 [3, H, W] (the planes of lse_eval_image_prep; planes_b nullable: one image) ->
 *      out uint8 [2, H, W] (or [1, H, W]) = u8((0.2989f r + 0.5870f g) + 0.1140f b), each operation rounded: the grey of
 *      lse_eval_image_prep.  (R:lse_nerf/lsenerf.py:463-464 takes the grey by a matmul whose order on a GPU is not knowable.)
 *   lse_canny_classify: gray uint8 [n_images, H, W] -> classes uint8 [n_images, H, W], 0 = none, 1 = weak, 2 = strong: OpenCV's
 *      Canny(image, low, high, apertureSize = 3, L2gradient = false) up to the hysteresis, restated from the published algorithm
 *      (parity unpinned).  3 x 3 Sobel dx, dy with a replicated border; mag = |dx| + |dy|, 0 outside the image; a pixel is a
 *      candidate when mag > low and strong when also mag > high (low > high are swapped); it must pass the non-maximum
 *      suppression: with x = |dx|, y = |dy| << 15, tg22x = x * 13573: y < tg22x: mag > mag[left] and mag >= mag[right]; else
 *      y > tg22x + (x << 16): mag > mag[up] and mag >= mag[down]; else s = ((dx ^ dy) < 0) ? -1 : 1 and mag > mag[up, j - s] and
 *      mag > mag[down, j + s].  The strict / non-strict asymmetry is part of the contract.  All arithmetic is integer.
 *   lse_canny_hysteresis: classes -> edges uint8 [n_images, H, W], 255 where the pixel is strong, or weak and 8-connected to a
 *      strong one through weak and strong pixels, else 0.  A set, so independent of any order: two calls are bit-identical.
 *      Union-find in three launches (merge inside a tile in LDS; merge across tile borders with 32-bit atomicMin on the labels;
 *      flatten).  workspace: n_images * lse_canny_workspace bytes, 8-byte aligned, written before it is read (never assumed zero).
 *      edges may alias classes.
 *   lse_canny_u8: lse_canny_classify then lse_canny_hysteresis on one stream; the class map passes through `edges`.
 *   lse_eval_panels: the writer's combined image (R:lse_nerf/lse_writer.py:32-64) of one eval image, grid uint8 [H, n_cols * W, 3].
 *      `flags` selects the panels, laid out left to right in this order:
 *        LSE_PANEL_IMG      2 W wide: gt_planes [3, H, W] (masked) beside rgb [H * W, 3] (unmasked); or, when pair_gt / pair_pred
 *                           [H * W] are given, that grey pair of the event-only metric, each tiled to three channels
 *        LSE_PANEL_DEPTH    ((1 - clip((depth - near) / ((far - near) + 1e-10f), 0, 1)) * acc) + (1 - acc), depth and accumulation
 *                           [H * W]; near / far = min / max of depth (a NaN is handed on), by a fixed-order two-stage reduction
 *                           without atomics that leaves them in workspace[0], workspace[1] (f32)
 *        LSE_PANEL_ERR_MAP  make_error_map of gt_planes and pred_planes, norm_cnst 6, the grey as in lse_gray8_planes
 *        LSE_PANEL_OVERLAY  edges uint8 [2, H, W] (ground truth, prediction): white; black where either is set; then channel 0 =
 *                           255 on the ground truth's edges and channel 2 = 255 on the prediction's (both: magenta)
 *        LSE_PANEL_EV_OUT   ev_out [H * W, ev_channels], ev_channels 1 (tiled to three) or 3
 *      Every value is the float expression of lsenerf_amd/evaluation.py with each operation rounded once in f32, then u8().
 *      Inputs of unselected panels may be NULL.  workspace: lse_eval_panels_workspace bytes, 8-byte aligned, written. */
#define LSE_PANEL_IMG 1
#define LSE_PANEL_DEPTH 2
#define LSE_PANEL_ERR_MAP 4
#define LSE_PANEL_OVERLAY 8
#define LSE_PANEL_EV_OUT 16
int lse_gray8_planes(const float *planes_a, const float *planes_b, int32_t H, int32_t W, uint8_t *out, lse_stream_t stream);
int lse_canny_workspace(int32_t H, int32_t W, int64_t *h_bytes);
int lse_canny_classify(const uint8_t *gray, int32_t n_images, int32_t H, int32_t W, int32_t low, int32_t high, uint8_t *classes,
                       lse_stream_t stream);
int lse_canny_hysteresis(const uint8_t *classes, int32_t n_images, int32_t H, int32_t W, void *workspace, int64_t workspace_bytes,
                         uint8_t *edges, lse_stream_t stream);
int lse_canny_u8(const uint8_t *gray, int32_t n_images, int32_t H, int32_t W, int32_t low, int32_t high, void *workspace,
                 int64_t workspace_bytes, uint8_t *edges, lse_stream_t stream);
int lse_eval_panels_workspace(int32_t H, int32_t W, int64_t *h_bytes);
int lse_eval_panels(const float *gt_planes, const float *pred_planes, const float *rgb, const float *pair_gt, const float *pair_pred,
                    const float *depth, const float *accumulation, const uint8_t *edges, const float *ev_out, int32_t ev_channels,
                    int32_t H, int32_t W, int32_t flags, void *workspace, int64_t workspace_bytes, uint8_t *grid,
                    lse_stream_t stream);

/* ---- occupancy grid (nerfacc OccGridEstimator._update) --------------------------- */
/* occs[id] = max(occs[id]*ema_decay, occ_new); duplicate ids resolve to the maximum over the duplicates (upstream:
 * an arbitrary one of them wins).  workspace: n floats. */
int lse_occ_update_cells(float *occs, const int64_t *cell_ids, const float *occ_new, int64_t n, float ema_decay,
                         float *workspace, lse_stream_t stream);
int lse_occ_binarize(const float *occs, int64_t n, const float *d_threshold, uint8_t *binaries, lse_stream_t stream);

/* ---- count-free occupancy refresh (csrc/occ_refresh.hip; ABI 6, additive): the index generation of `_update` on the device ----
 * Nothing below sizes anything from a device value: every launch has a fixed grid, counts stay in device memory, so the four
 * jobs (with the field's count-free density pass between 2 and 3, and lse_occ_binarize at the end) capture into a HIP graph.
 *
 * 1. Occupied-cell list.  binaries u8 [levels, cells]; list int32 [levels, cells]: per level the ASCENDING indices of the set
 *    cells in list[l, 0 .. counts[l]) (the rest is left alone); counts int64 [levels].  == torch.nonzero(binaries[l])[:, 0].
 *    Count per tile of LSE_OCC_LIST_TILE cells, exclusive scan of the tile counts, ordered write (ballot / popcount per wave);
 *    no atomics.  workspace: levels * ceil(cells / LSE_OCC_LIST_TILE) int32. */
#define LSE_OCC_LIST_TILE 4096
int lse_occ_list_occupied(const uint8_t *binaries, int32_t levels, int64_t cells, int32_t *list, int64_t *counts,
                          int32_t *workspace, lse_stream_t stream);
/* 2. Cell draw and positions of ONE level (N = cells / 4, cells < 2^31, cells == res[0] * res[1] * res[2]).
 *    warmup != 0: slot i is cell i, *n_dev = cells (cap >= cells).
 *    warmup == 0: cnt = counts[level], m = min(cnt, N); slots [0, m): occupied cells -- list[level, i] when cnt <= N, else
 *      list[level, mulhi32(w0, cnt)]; slots [m, m + N): uniform cells mulhi32(w0, cells); *n_dev = m + N (cap >= 2 N); slots
 *      beyond are not written.
 *    Per slot ONE Philox4x32-10 call, key (seed & 0xffffffff, seed >> 32), counter (*step_dev & 0xffffffff, slot, level, 0):
 *    w0 picks the cell, w1..w3 the in-cell jitter u = (w >> 8) * 2^-24.  The library's own stream (uniform with replacement, like
 *    torch.randint); no bit parity with any torch generator.  cell (x, y, z) = unravel(idx, res), position_k = lo_k + ((coord_k +
 *    u_k) / res_k) * (hi_k - lo_k) in float32, every operation rounded on its own; aabbs f32 [levels, 6] in device memory.
 *    cell_ids int64 [cap]: level * cells + idx, or -1 where occs of that cell < 0 (the position is still that cell's).
 *    positions f32 [cap, 3]. */
int lse_occ_draw_cells(const float *occs, const int32_t *list, const int64_t *counts, const float *aabbs, int32_t level,
                       int64_t cells, int32_t res_x, int32_t res_y, int32_t res_z, int32_t warmup, const int64_t *step_dev,
                       uint64_t seed, int64_t cap, int64_t *cell_ids, float *positions, int64_t *n_dev, lse_stream_t stream);
/* 3. lse_occ_update_cells with the count in device memory: n = clamp(*n_dev, 0, cap), ids < 0 are skipped, and the new value is
 *    sigma[i] * step_size (one float32 multiply).  Given the same cells: bit-equal to lse_occ_update_cells.  workspace: cap floats. */
int lse_occ_update_cells_dev(float *occs, const int64_t *cell_ids, const float *sigma, float step_size, const int64_t *n_dev,
                             int64_t cap, float ema_decay, float *workspace, lse_stream_t stream);
/* 4. *mean_all = mean(occs) and *threshold = min(mean(occs[occs >= 0]), occ_thre) (NaN when no cell is >= 0, like torch) in one
 *    fixed-order two-stage reduction: LSE_OCC_MEAN_BLOCKS blocks, double accumulators, no atomics -- two runs are bit-equal.
 *    workspace: 3 * LSE_OCC_MEAN_BLOCKS doubles. */
#define LSE_OCC_MEAN_BLOCKS 1024
int lse_occ_mean_threshold(const float *occs, int64_t n, float occ_thre, double *workspace, float *mean_all, float *threshold,
                           lse_stream_t stream);

/* ---- mesh export (csrc/mesh.hip; ABI 6, additive): naive surface nets of a density lattice ------------------------------------
 * Lattice.  res = (nx, ny, nz) cells, every count >= 1.  Points (ix, iy, iz), 0 <= i_k <= n_k, index
 *   p = (ix * (ny + 1) + iy) * (nz + 1) + iz (fewer than 2^31 points), position_k = lo_k + ((float)i_k / (float)n_k) * (hi_k - lo_k)
 *   in float32, every operation rounded on its own (the form of lse_occ_draw_cells).  Cells (cx, cy, cz), 0 <= c_k < n_k, index
 *   c = (cx * ny + cy) * nz + cz; a cell's lowest corner is the point with its coordinates.  sigma: f32, one value per point.
 * inside(p) = sigma[p] > level: NaN is outside.
 * Vertices.  A cell is active when its 8 corners are neither all inside nor all outside; the vertices are the active cells in
 *   ascending cell index.  The position is the mean of the crossings on the cell's 12 edges, visited as: axis a = 0, 1, 2 with
 *   b = (a + 1) % 3, c = (a + 2) % 3; offset ob in (0, 1) along b (outer), oc in (0, 1) along c (inner); the edge runs from
 *   P = cell + ob e_b + oc e_c to Q = P + e_a.  An edge with inside(P) != inside(Q) contributes the lattice-unit point P + t e_a,
 *   t = (level - sigma[P]) / (sigma[Q] - sigma[P]), NaN replaced by 0.5, then clamped to [0, 1].  The three coordinates are summed
 *   in float32 in that order, divided by (float)count and mapped to world as lo_k + (u_k / (float)n_k) * (hi_k - lo_k).
 * Faces.  A lattice edge (p, a) from p to q = p + e_a (both in the lattice) with inside(p) != inside(q) that is interior in the
 *   other two axes (1 <= p_b <= n_b - 1, 1 <= p_c <= n_c - 1) gives one quad over the cells C0 = p - e_b - e_c, C1 = p - e_c,
 *   C2 = p, C3 = p - e_b (all active by construction): corners (C0, C1, C2, C3) if inside(p), else (C3, C2, C1, C0), so that the
 *   geometric normal points from high to low density; triangles (w0, w1, w2), (w0, w2, w3) of int32 vertex ids; quads in ascending
 *   (p, a).  Edges on the box surface give nothing: the mesh is open exactly where the surface leaves the box, and an active
 *   boundary cell keeps its (possibly unreferenced) vertex.
 *
 * lse_lattice_positions: positions [n, 3] of the points first .. first + n (0 <= first, first + n <= points).
 * lse_surface_nets_workspace: *h_bytes = size of the workspace the two passes share: per cell an int32 rank inside its segment
 *   of LSE_MESH_SEGMENT consecutive cells, per segment of cells and of points an int64 offset.
 * lse_surface_nets_count: fills the workspace and totals (device int64[2] = {vertices, quads}).  One wave per segment, ballot /
 *   popcount ranks, one block per row scans the segment counts: fixed grids, no atomics, no host read.
 * lse_surface_nets_emit: vertices f32 [cap_vertices, 3], triangles int32 [2 * cap_quads, 3] from the SAME sigma, resolution and
 *   level as the count that filled the workspace (which it only reads).  Rows at or beyond a capacity are not written; totals keeps
 *   the true counts, so a caller sizes exactly after one read or runs with fixed capacities.  Workspace and totals are 8-byte aligned. */
#define LSE_MESH_SEGMENT 1024
int lse_lattice_positions(const float *h_lo, const float *h_hi, int32_t nx, int32_t ny, int32_t nz, int64_t first, int64_t n,
                          float *positions, lse_stream_t stream);
int lse_surface_nets_workspace(int32_t nx, int32_t ny, int32_t nz, int64_t *h_bytes);
int lse_surface_nets_count(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, void *workspace,
                           int64_t workspace_bytes, int64_t *totals, lse_stream_t stream);
int lse_surface_nets_emit(const float *sigma, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi, float level,
                          const void *workspace, int64_t workspace_bytes, int64_t cap_vertices, int64_t cap_quads, float *vertices,
                          int32_t *triangles, lse_stream_t stream);
/* World-space normals at n points: out[i] = -g / max(|g|, 1e-12) with g = J^T d_x01[i], J the Jacobian of the position map at
 * positions[i] (what lse_positions_bwd applies: contraction or aabb normalisation by h_aabb[6], selector-masked) -- the per-sample
 * arithmetic of lse_eval_composite_normals with LSE_NORMALS_WORLD.  d_x01, positions, out: f32 [n, 3]; n_dev: nullable device
 * count as in the per-sample entry points; h_aabb is unused and nullable with contraction. */
int lse_point_normals_world(const float *d_x01, const float *positions, int32_t contraction, const float *h_aabb, int64_t n,
                            const int64_t *n_dev, float *out, lse_stream_t stream);

/* ---- point-cloud export (csrc/pointcloud.hip; ABI 6, additive): eval renders -> one merged, filtered cloud ---------------------
 * All floats are f32, every operation is rounded on its own, every comparison is false on NaN.  The three compacting entry points
 * (append, merge, filter) share one ordered compaction: one wave owns LSE_PC_SEGMENT consecutive items, ballot / popcount give every
 * kept item its rank inside the segment, one block scans the segment counts as int64, the emit pass writes at offset + rank.  Fixed
 * grids sized from the extent, no atomics, no host read: two runs give the same bytes.  Each takes a workspace of the size its
 * *_workspace function returns for the same extent (per segment an int64, per item an int32 rank; 8-byte aligned, contents need not
 * survive the call) and a device int64 `total` (8-byte aligned).  Rows at or beyond `cap` are not written and `total` keeps the true
 * count, as lse_surface_nets_emit's totals do.  Outputs must not alias inputs.  An extent is at most 2^40.
 *
 * lse_unproject_append.  origins, directions [n_rays, 3], depth, acc [n_rays]; colors, normals [n_rays, 3] nullable.
 *   p_k = o_k + d_k * depth (the product rounded, then the sum).  Ray r is kept iff acc[r] >= min_acc, depth[r] > 0,
 *   depth[r] < +inf and lo_k <= p_k <= hi_k for k = 0, 1, 2.  Kept rays take the rows *total + rank in ascending r, *total being
 *   the value on entry; out_points [cap, 3] gets p, out_colors / out_normals [cap, 3] (each nullable; needs its input) get the
 *   ray's row bit for bit.  Afterwards *total += kept: successive images append without a host read.  n_rays == 0: no-op.
 * lse_voxel_keys.  points [n, 3]; count = min(n, *n_dev) (n_dev nullable: count = n).  For i < count
 *   f_k = floorf((p_k - lo_k) / voxel),  v_k = f_k >= (float)(n_k - 1) ? n_k - 1 : (f_k > 0 ? (int)f_k : 0)  (NaN -> 0),
 *   keys[i] = ((int64)vx * ny + vy) * nz + vz;  for count <= i < n keys[i] = INT64_MAX.  Refused: an n_k outside [1, 2^20], a voxel
 *   size that is not positive and finite.  Sorting is the caller's: a STABLE sort of keys gives sorted_keys and order, so equal
 *   keys keep ascending original index.
 * lse_voxel_merge.  sorted_keys, order [n] (order: a permutation of 0 .. n - 1; an index outside is skipped, never read through);
 *   points [n, 3], colors / normals [n, 3] nullable, indexed through order.  Position i is a head iff sorted_keys[i] != INT64_MAX
 *   and (i == 0 or sorted_keys[i] != sorted_keys[i - 1]); its run extends to the next position with another key.  Voxel j is the
 *   j-th head (keys ascending and unique): out_keys[j], out_counts[j] = run length c (int32), position and colour = s / (float)c
 *   where s starts as the run's first element and adds the others one by one in run order, normal = s_n / max(len, 1e-12f) with
 *   s_n summed the same way and len = sqrtf((sx * sx + sy * sy) + sz * sz) -- a zero sum stays zero.  *total = voxels (set, not
 *   incremented; 0 for n == 0).  The thread that owns a head walks its run -- the pixels of all views inside one voxel -- so the
 *   cost is O(longest run).
 * lse_voxel_support_filter.  keys (ascending, unique), counts, points [m, 3], colors / normals nullable: the merge's outputs;
 *   present voxels are j < min(m, *m_dev) (m_dev nullable).  Coordinates come back from the key (z = key % nz, y = (key / nz) % ny,
 *   x = key / (nz * ny)); support_j = the sum of counts over the present voxels among the 27 offsets (dx, dy, dz) in {-1, 0, 1}^3
 *   whose coordinates lie inside the lattice, j itself included, each found by binary search over keys (an adjacent key is not
 *   necessarily a neighbour: (x, y, nz - 1) and (x, y + 1, 0) differ by one).  Voxel j is kept iff support_j >= min_support; the
 *   kept voxels' keys, counts, points, colours and normals are compacted in order, *total = kept.  out_support (int32 [m], nullable,
 *   indexed by INPUT voxel) receives every support, saturated at INT32_MAX, and 0 for j that is not present. */
#define LSE_PC_SEGMENT 1024
int lse_unproject_workspace(int64_t n_rays, int64_t *h_bytes);
int lse_unproject_append(const float *origins, const float *directions, const float *depth, const float *acc, const float *colors,
                         const float *normals, int64_t n_rays, const float *h_lo, const float *h_hi, float min_acc, void *workspace,
                         int64_t workspace_bytes, int64_t cap, float *out_points, float *out_colors, float *out_normals,
                         int64_t *total, lse_stream_t stream);
int lse_voxel_keys(const float *points, int64_t n, const int64_t *n_dev, const float *h_lo, float voxel, int32_t nx, int32_t ny,
                   int32_t nz, int64_t *keys, lse_stream_t stream);
int lse_voxel_merge_workspace(int64_t n, int64_t *h_bytes);
int lse_voxel_merge(const int64_t *sorted_keys, const int64_t *order, const float *points, const float *colors, const float *normals,
                    int64_t n, void *workspace, int64_t workspace_bytes, int64_t cap, int64_t *out_keys, int32_t *out_counts,
                    float *out_points, float *out_colors, float *out_normals, int64_t *total, lse_stream_t stream);
int lse_voxel_support_workspace(int64_t m, int64_t *h_bytes);
int lse_voxel_support_filter(const int64_t *keys, const int32_t *counts, const float *points, const float *colors,
                             const float *normals, int64_t m, const int64_t *m_dev, int32_t nx, int32_t ny, int32_t nz,
                             int32_t min_support, void *workspace, int64_t workspace_bytes, int64_t cap, int64_t *out_keys,
                             int32_t *out_counts, float *out_points, float *out_colors, float *out_normals, int32_t *out_support,
                             int64_t *total, lse_stream_t stream);

/* ---- event synthesis (csrc/events.hip; ABI 6, additive): log-intensity planes -> event counts and an event stream, and back -------
 * The sensor model is ideal, noise-free and per pixel: the linear-interpolation model of ESIM.  Inputs: K + 1 log-intensity planes
 * L[k][p], f32, plane-major [K + 1, P] with P = H * W in row-major pixel order; times t[k], f64 [K + 1], on the device, ascending; a
 * per-pixel reference level ref[p], f32; the thresholds c_pos, c_neg, positive and finite; a per-interval cap cap_step in
 * [1, 32767].  Every f32 operation is rounded on its own, every comparison is false on NaN.
 *
 * The walk of interval k at pixel p, with L0 = L[k][p], L1 = L[k + 1][p], n = 0 and ref the level the previous interval left
 * (ref_in[p] for k = 0):
 *   if (L1 - ref >= c_pos)      while (L1 - ref >= c_pos && n < cap_step) { ref = ref + c_pos; emit(+1, ref); n++; }
 *   else if (ref - L1 >= c_neg) while (ref - L1 >= c_neg && n < cap_step) { ref = ref - c_neg; emit(-1, ref); n++; }
 *   if (n == cap_step) ref = L1;             (a saturated pixel: the level is re-armed at the interval's end)
 *   counts[k][p] = polarity * n              (int32, signed)
 * and ref_out[p] is the level behind the last interval.  NaN in L or ref gives no event and leaves ref unchanged.
 * emit(pol, level) gives the event its time:
 *   d    = L1 - L0
 *   frac = (d == 0 || q is NaN) ? 0 : min(max(q, 0), 1)   with q = (level - L0) / d, the correctly rounded f32 quotient
 *          ((float)((double)a / (double)d) is exactly that)
 *   time = t[k] + (double)frac * (t[k + 1] - t[k])         in f64: the difference, then the product, then the sum, each rounded
 * An event is x = p % W (int16), y = p / W (int16), t (f64), p (int8, +1 or -1); the stream order is (k ascending, pixel ascending,
 * emission order).  Every device loop is bounded by cap_step or a host-known extent.
 *
 * Conventions are those of the point-cloud section: fixed grids sized from the extent, no host read, a workspace of the size
 * lse_event_workspace returns for the same (K, P) (8-byte aligned, contents need not survive the call: per segment of
 * LSE_EVENT_SEGMENT consecutive items (k, p) an int64, per item the interval's starting level, its signed count and the rank of its
 * first event), a device int64 `total` (8-byte aligned), rows at or beyond `cap` not written while `total` keeps the true count,
 * outputs that do not alias inputs (ref_out is not ref_in), and two runs that give the same bytes.  The rank of an item is a wave
 * prefix SUM of |n| (an item carries |n| events, not 0 or 1), one block scans the segment sums as int64, the emit pass rewalks one
 * interval per item.  Refused: K or P negative, P > 2^30, K * P > 2^40, a threshold that is not positive and finite, cap_step
 * outside [1, 32767].
 *
 * lse_event_count.  The walk without emission: counts (int32 [K, P]), ref_out, and *window_total = the sum of |counts| (int64, set,
 *   summed in a fixed order).  K == 0: ref_out = ref_in, *window_total = 0.
 * lse_event_append.  The same walk; the window's events take the rows *total + rank in stream order, *total being the value on
 *   entry; afterwards *total += the window's events, so successive windows (ref_out of one as ref_in of the next, the last plane of
 *   one as the first of the next) chain without a host read.  out_x, out_y (int16), out_t (f64), out_p (int8): [cap]; counts is
 *   nullable.  Also refused: P % W != 0, W outside [1, 32767], P / W > 32767, a workspace too small.  K == 0 is a no-op that copies
 *   ref_in to ref_out.
 * lse_event_accumulate.  A stream -> frames.  x, y, t, p [n]; count = min(n, *n_dev) (n_dev nullable: count = n); bounds: f64
 *   [F + 1] on the device, ascending.  For i < count, frame f is the largest index with bounds[f] <= t_i; the event counts iff
 *   bounds[0] <= t_i < bounds[F], 0 <= x_i < W and 0 <= y_i < H, and a counted event does acc[f][y_i][x_i] += (int)p_i (acc: int32
 *   [F, H, W]).  It ADDS into acc, so a stream can arrive in pieces and the caller zeroes acc first.  The adds are 32-bit integer
 *   vector atomics: integer sums do not depend on the order of their terms, so the result is still bit-reproducible.  Saturation
 *   to int8 (the format of eimgs_1x.npy) is the caller's. */
#define LSE_EVENT_SEGMENT 1024
int lse_event_workspace(int64_t K, int64_t P, int64_t *h_bytes);
int lse_event_count(const float *L, int64_t K, int64_t P, const float *ref_in, float c_pos, float c_neg, int32_t cap_step,
                    int32_t *counts, float *ref_out, int64_t *window_total, lse_stream_t stream);
int lse_event_append(const float *L, const double *times, int64_t K, int64_t P, int32_t W, const float *ref_in, float c_pos,
                     float c_neg, int32_t cap_step, void *workspace, int64_t workspace_bytes, int64_t cap, int16_t *out_x,
                     int16_t *out_y, double *out_t, int8_t *out_p, int32_t *counts, float *ref_out, int64_t *total,
                     lse_stream_t stream);
int lse_event_accumulate(const int16_t *x, const int16_t *y, const double *t, const int8_t *p, int64_t n, const int64_t *n_dev,
                         const double *bounds, int32_t F, int32_t H, int32_t W, int32_t *acc, lse_stream_t stream);

/* ---- training epilogue: output routing + intensity mappers + both losses, O(rays), one launch each way
 *      (R:lse_nerf/lsenerf.py:329-377 routing, :392-439 losses; R:lse_nerf/intensity_mappers.py:64-94 mappers).
 * Colour bundle:  v = rgb_mapped ? m_rgb(max(rgb, 1e-5)) : rgb;  mean over deblur_group consecutive rays (the 4 virtual
 *   cameras of a pixel, R:lse_nerf/lsenerf.py:365-370);  max(., 1e-5);  rgb_loss = mean (v - col_gt)^2.
 * Event bundles (prev, next):  c = max(rgb, 1e-5);  ev_one_dim != NONE: m_evs(sum_k w_k c_k) with w = softmax(w31)
 *   (ThreeToOne, LEARNED) or the gray vector (GRAY);  NONE: gray(m_evs(c));  L = log(. + 1e-6);
 *   event_loss = evs_loss_weight * mean (L_next - L_prev - evs_gt)^2          (log_loss, R:lse_nerf/lsenerf.py:392-399), or with
 *   event_loss_kind = LSE_EVLOSS_ENERF_NORM (enerf_norm_loss, :406-419; ABI 6):  d_r = L_next - L_prev,  c_r = evs_gt[r] / e_thresh[r],
 *   event_loss = evs_loss_weight * mean (d_r / (||d||_2 + 1e-6) - c_r / (||c||_2 + 1e-6))^2, norms over the event rays, c constant.
 * m = identity | x^(1/2.4) ("gt") | x^p ("powpow", p = *pow_rgb / *pow_evs, learnable) | "mlp" | "rgb_mlp" (ABI 6): the
 *   identity-initialised nerfstudio MLP(in, num_layers = 4, layer_width = 16, out = in, ReLU, out_activation = Sigmoid) of
 *   R:lse_nerf/intensity_mappers.py:28-62 -- "mlp" maps ONE channel (in = 1: the event side behind ev_one_dim; on three channels
 *   the reference's nn.Linear(1, 16) raises, and so does the call), "rgb_mlp" the three channels together (in = 3: the colour
 *   side, or the event side with ev_one_dim == NONE).  Their parameters come as lse_mapper_mlp. */
#define LSE_MAP_IDENTITY 1
#define LSE_MAP_GT 2
#define LSE_MAP_POWPOW 3
#define LSE_MAP_MLP 4
#define LSE_MAP_RGB_MLP 5
/* The four nn.Linear layers of an MLP mapper, in = 1 ("mlp") | 3 ("rgb_mlp"): w[l] row-major [out][in] = [16,in] [16,16] [16,16]
 * [in,16], b[l] = [16] [16] [16] [in] (device pointers; the struct itself is host memory, read during the call).  dw / db: the
 * gradients, same shapes, ACCUMULATED into (+=) by lse_loss_epilogue_bwd in a fixed order (no atomics); all eight NULL = not
 * wanted; the forward ignores them. */
typedef struct lse_mapper_mlp {
    const float *w[4];
    const float *b[4];
    float *dw[4];
    float *db[4];
} lse_mapper_mlp;
#define LSE_ONE_DIM_NONE 0
#define LSE_ONE_DIM_LEARNED 1
#define LSE_ONE_DIM_GRAY 2
#define LSE_EVLOSS_LOG 0
#define LSE_EVLOSS_ENERF_NORM 1
typedef struct lse_epilogue_desc {
    int32_t rgb_mapped;      /* 0: the colour loss sees the raw render; 1: m_rgb(max(rgb, 1e-5)) */
    int32_t rgb_mapper;      /* LSE_MAP_* */
    int32_t evs_mapper;      /* LSE_MAP_* applied on the event side */
    int32_t ev_one_dim;      /* LSE_ONE_DIM_* */
    int32_t deblur_group;    /* 1, or 4 for rgb_loss_type == "deblur" */
    float evs_loss_weight;
    int32_t event_loss_kind; /* LSE_EVLOSS_* */
} lse_epilogue_desc;
/* losses[2] = (rgb_loss, event_loss); a bundle whose pointer is NULL contributes 0.  Deterministic (no atomics). */
/* mlp_rgb / mlp_evs: parameters of the colour-side / event-side mapper when its kind is LSE_MAP_MLP / LSE_MAP_RGB_MLP (else ignored,
 * NULL allowed).  e_thresh [n_ev]: the per-ray event threshold of LSE_EVLOSS_ENERF_NORM (NULL = 1; ignored by log_loss). */
int lse_loss_epilogue_fwd(const lse_epilogue_desc *desc, const float *col_rgb, const float *col_gt, int32_t n_col,
                          const float *prev_rgb, const float *next_rgb, const float *evs_gt, const float *e_thresh, int32_t n_ev,
                          const float *pow_rgb, const float *pow_evs, const float *w31, const lse_mapper_mlp *mlp_rgb,
                          const lse_mapper_mlp *mlp_evs, float *losses, lse_stream_t stream);
/* g_rgb_loss / g_event_loss: device scalars, the upstream gradients of the two losses (NULL = 0).  d_col [n_col*deblur_group,3], d_prev / d_next [n_ev,3]
 * (each nullable) are overwritten; d_scalars[5] = (d pow_rgb, d pow_evs, d w31[3]) is overwritten; the gradients of an MLP mapper's
 * parameters are accumulated into mlp_*->dw / db. */
int lse_loss_epilogue_bwd(const lse_epilogue_desc *desc, const float *col_rgb, const float *col_gt, int32_t n_col,
                          const float *prev_rgb, const float *next_rgb, const float *evs_gt, const float *e_thresh, int32_t n_ev,
                          const float *pow_rgb, const float *pow_evs, const float *w31, const lse_mapper_mlp *mlp_rgb,
                          const lse_mapper_mlp *mlp_evs, const float *g_rgb_loss, const float *g_event_loss, float *d_col,
                          float *d_prev, float *d_next, float *d_scalars, lse_stream_t stream);

/* ---- optimiser: torch.optim.Adam semantics on a flat buffer (R:lse_nerf/lse_config.py:29-33) -----------
 * lse_adam_step and lse_adam_step_dev are kept for ABI compatibility only (they take 1 - beta from the float betas, see below);
 * this package calls lse_adam_step_f64 and lse_adam_step_dev_sched. */
int lse_adam_step(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, float lr,
                  float beta1, float beta2, float eps, int32_t step, float grad_scale, lse_stream_t stream);
/* The same with the scalars as doubles.  A float cannot hold 1 - beta next to beta: 0.999 rounds to 0.999000013 and 1.f - that is
 * 1.3e-5 short of 0.001, which exp_avg_sq then is too.  Here 1 - beta and the bias corrections come from the double betas, each
 * rounded once -- torch.optim.Adam's arithmetic.  (lse_adam_step is Adam for the betas AS ROUNDED, exact in itself.) */
int lse_adam_step_f64(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, double lr,
                      double beta1, double beta2, double eps, int32_t step, float grad_scale, lse_stream_t stream);
/* The same with EVERY scalar of the step in device memory: hyper[6] = {lr, 1 - beta1^step, 1 / sqrt(1 - beta2^step), beta1, beta2,
 * eps}.  A launch captured into a HIP graph cannot carry new scalar arguments; lse_adam_schedule_dev (captured in front of it)
 * writes all six. */
int lse_adam_step_dev(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, const float *hyper,
                      float grad_scale, lse_stream_t stream);
/* lse_adam_step_dev with 1 - beta1 and 1 - beta2 taken from the schedule's double constants (sched[6] of lse_adam_schedule_dev, in
 * device memory) instead of from the rounded betas in hyper: the bias corrections in hyper come from the double betas too, and
 * lse_adam_step_dev's float differences do not match them (the step is 6e-6 too long while the moments are young). */
int lse_adam_step_dev_sched(float *params, const float *grads, float *exp_avg, float *exp_avg_sq, int64_t n, const float *hyper,
                            const double *sched, float grad_scale, lse_stream_t stream);
/* Device-side optimizer clock: *step (optimizer steps taken so far, int64 in device memory) is advanced by one and hyper[6] of
 * the NEW step is written, with nerfstudio's ExponentialDecayScheduler lr = lr_init * (lr_final / lr_init)^(min(steps taken /
 * max_steps, 1)) (max_steps <= 0 or lr_final <= 0: constant lr_init; R:lse_nerf/lse_config.py:29-38).  The schedule's constants
 * are read from device memory too -- sched[6] = {lr_init, lr_final, max_steps, beta1, beta2, eps} as doubles (ABI 5; they were
 * launch arguments, frozen into a captured graph) -- so a replayed graph depends on nothing the host writes per step, however far
 * the host runs ahead, and follows a changed learning-rate schedule without being captured again. */
int lse_adam_schedule_dev(int64_t *step, float *hyper, const double *sched, lse_stream_t stream);

/* ---- batch composer: the data manager's hot loop (R:lse_nerf/lse_datamanager.py:337-372) as one launch -------------------
 * The scene's pixels and camera tables live in device memory; one launch draws the pixels of a step, gathers their targets and
 * writes the rays and the metadata of all three bundles (colour | previous events | next events) into caller-owned buffers.
 *   draw     (c, y, x) of pixel i of a stream: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (step & 0xffffffff, i,
 *            stream id (0 colour / 1 events), 0); c = mulhi32(w0, n_images), y = mulhi32(w1, H), x = mulhi32(w2, W).  This
 *            library's own convention (uniform i.i.d. over images x pixels); no bit parity with any torch generator.
 *   gather   colour target float(u8) / 255.0f, event target float(e) * e_scale, mask, appearance id, camera = image_idx[c].
 *   rays     EdCameras.generate_rays (R:lse_nerf/lse_cameras.py:340-586): no half-pixel offset, the camera-frame points of
 *            (x, y), (x+1, y), (x, y+1), the 10-step Newton undistortion, rotation by a pose read from a POSE TABLE, pixel_area,
 *            directions_norm.  Origins are copies of the table's translation.
 *   metadata as R:lse_nerf/utils.py:153-194 (add_metadata) and R:lse_nerf/data_components.py:70-90 (CameraIdxFixer, from a table).
 * Ray rows: colour pixel i owns rows row_col + i*G + k (k-th virtual camera of a deblur pixel, G = 4; else G = 1), event pixel j owns
 * row_prev + j and row_next + j.  Per-pixel batch rows are i and j. */
#define LSE_PIX_I8 0
#define LSE_PIX_U8 1
#define LSE_PIX_I16 2
#define LSE_PIX_I32 3
#define LSE_PIX_F32 4
#define LSE_PIX_NONE (-1)
typedef struct lse_compose_stream {      /* one camera set: colour or events */
    float fx, fy, cx, cy;
    float dist[6];          /* (k1, k2, k3, k4, p1, p2); read when `distort` != 0 */
    int32_t H, W;
    int32_t n_images;       /* resident images: the range of the drawn c */
    int32_t n_cameras;      /* cameras of the set = rows of its per-camera tables (pose table rows / G) */
    int32_t n_pixels;       /* pixels sampled per step from this stream (0: stream absent) */
    int32_t pix_type;       /* LSE_PIX_* of `images` (colour: LSE_PIX_U8, three channels) */
    int32_t msk_type;       /* LSE_PIX_U8 | LSE_PIX_F32 | LSE_PIX_NONE */
    int32_t distort;        /* non-zero: undistort with `dist` */
} lse_compose_stream;
typedef struct lse_compose_desc {
    lse_compose_stream col, evs;
    int32_t G;              /* rays per colour pixel: 1, or 4 (deblur) */
    int32_t num_embd;       /* colour appearance ids with G = 4 are id + (k - 2) clipped to [0, num_embd - 1] */
    int32_t consecutive;    /* 1: ConsecRayGenerator -- the next bundle reads the prev tables at camera + 1 (needs image_idx + 1 <
                               evs.n_cameras); 0: PrevNextRayGenerator -- its own tables at the same camera */
    float e_scale;          /* event target = float(e) * e_scale (the contrast threshold for integer frames; 1 for LSE_PIX_F32) */
    float e_thresh;         /* written per event ray */
    uint64_t seed;
} lse_compose_desc;
/* device pointers (the struct itself is host memory, read during the call); a stream with n_pixels == 0 may leave its rows NULL */
typedef struct lse_compose_scene {
    const uint8_t *col_images;        /* [n_images, H, W, 3] */
    const void *col_msk;              /* [n_images, H, W] of msk_type, or NULL */
    const int32_t *col_appearance_id; /* [n_images] */
    const int32_t *col_image_idx;     /* [n_images] -> camera of the colour set */
    const float *col_times;           /* [n_cameras] */
    const float *col_pose;            /* [n_cameras, G, 3, 4] */
    const void *evs_images;           /* [n_images, H, W] of pix_type */
    const void *evs_msk;
    const int32_t *evs_appearance_id;
    const int32_t *evs_image_idx;
    const float *prev_times, *next_times;            /* [n_cameras] (consecutive: the same table twice) */
    const int32_t *prev_closest, *next_closest;      /* [n_cameras] index of the closest colour-camera time */
    const float *prev_pose, *next_pose;              /* [n_cameras, 3, 4] */
} lse_compose_scene;
typedef struct lse_compose_out {
    int32_t row_col, row_prev, row_next;   /* first ray row of each bundle in the per-ray buffers */
    int32_t n_rows;                        /* rows of the per-ray buffers (checked against the three blocks) */
    float *origins, *directions;           /* [n_rows, 3] */
    float *pixel_area, *directions_norm, *times;   /* [n_rows, 1] */
    int64_t *camera_indices;               /* [n_rows, 1] */
    int32_t *appearance_id;                /* [n_rows, 1] */
    int32_t *cam_type;                     /* [n_rows]    0 colour / 1 events */
    int32_t *coords;                       /* [n_rows, 3] (camera, y, x); the colour block holds its pixel list G times over
                                              (torch.tile, as add_metadata's fix_datashape leaves it) */
    int32_t *ray_px;                       /* [n_rows, 3] (pose-table row, y, x) of every ray: what lse_compose_rays_bwd reads */
    float *col_image;                      /* [col.n_pixels, 3] */
    float *col_msk;                        /* [col.n_pixels, 1] or NULL */
    int32_t *col_indices;                  /* [col.n_pixels, 3] (camera, y, x) */
    int32_t *col_batch_appearance_id;      /* [col.n_pixels] */
    float *evs_image;                      /* [evs.n_pixels, 1] */
    float *evs_msk;
    float *evs_e_thresh;                   /* [evs.n_pixels, 1] */
    int32_t *evs_indices;
    int32_t *evs_batch_appearance_id;
} lse_compose_out;
/* step: *step_dev (int64, device) when step_dev != NULL, else `step`; its low 32 bits enter the counter.  advance != 0 (needs
 * step_dev): a one-thread launch behind the composer adds 1 to *step_dev, so replay k of a captured graph draws what an eager call
 * with step k0 + k draws.  col_indices_in / evs_indices_in (int32 [n_pixels, 3] = (c, y, x), nullable): given pixels instead of the
 * draw; values outside the scene are clamped into it. */
int lse_compose_batch(const lse_compose_desc *desc, const lse_compose_scene *scene, const lse_compose_out *out, int64_t *step_dev,
                      int64_t step, int32_t advance, const int32_t *col_indices_in, const int32_t *evs_indices_in,
                      lse_stream_t stream);
/* Gradient w.r.t. the pose tables from d_origins / d_directions [n_rows, 3] and the saved ray_px: d_col_pose [col.n_cameras, G, 3, 4],
 * d_prev_pose / d_next_pose [evs.n_cameras, 3, 4] are OVERWRITTEN (rows no ray touched get zero).  The camera-frame point is
 * recomputed.  One wave per table row sums its rays in a fixed order (no atomics): two runs are bit-equal.  consecutive != 0: both
 * event bundles index ONE table, and d_prev_pose receives the sum of both (d_next_pose is ignored, NULL allowed). */
int lse_compose_rays_bwd(const lse_compose_desc *desc, const lse_compose_scene *scene, const lse_compose_out *out,
                         const float *d_origins, const float *d_directions, float *d_col_pose, float *d_prev_pose,
                         float *d_next_pose, lse_stream_t stream);

/* ---- weighted pixel draw (csrc/pixel_draw.hip; ABI 6, additive): the composer's pixels by integer weight instead of uniformly ----
 * Pixel x of image row r = c * H + y of one camera set has the integer weight
 *   w(r, x) = 0                        where msk != NULL and (float)msk[r, x] == 0,
 *             w_idle                   where images == NULL (a set whose pixels differ only by the mask: needs w_active == w_idle),
 *             w_active or w_idle       by (float)images[r, x] != 0 or == 0 (-0.0f and a net-zero frame pixel are idle, NaN is active),
 * with the float conversions of the composer's gather.  images: [n_images, H, W] of pix_type (one channel: event frames); msk:
 * [n_images, H, W] of msk_type (LSE_PIX_U8 | LSE_PIX_F32), or NULL with LSE_PIX_NONE.  Weights lie in [0, 255], not both zero.
 *   lse_pixel_rows_build  row_off int64 [rows + 1], rows = n_images * H: the exclusive prefix sums of the row sums, row_off[rows] =
 *      the total weight.  One wave per row, then one block scans; once per scene (and again after the images or masks were edited).
 *   lse_pixel_draw  pixel i < n at step s (*step_dev when step_dev != NULL, else `step`), all integers:
 *        (w0, w1, ., .) = Philox4x32-10(counter (s & 0xffffffff, i, stream_id, 0), key (seed & 0xffffffff, seed >> 32))
 *        t = mulhi64((w0 << 32) | w1, total)                       0 <= t < total
 *        r = #{r' in [0, rows) : row_off[r'] <= t} - 1             v = t - row_off[r]
 *        x = #{x' in [0, W) : sum_{j < x'} w(r, j) <= v} - 1       c = r / H,  y = r % H
 *      writes indices[i] = (c, y, x) (int32 [n, 3], the col_indices_in / evs_indices_in of lse_compose_batch) and weights[i] =
 *      w(r, x) (int32 [n]).  Rows and pixels of weight zero are never drawn, wherever they sit.  One wave per pixel: a 64-ary
 *      search of row_off, then a walk of the row 64 pixels at a time.  No atomics, no LDS, no workspace; the grid depends on n only,
 *      so the launch can be captured, and it reads *step_dev like lse_compose_batch: launch it in front of that call's advance.
 *      A total of zero is the caller's to refuse (it is row_off[rows]); the kernel then still writes pixels inside the images.
 * LSE_E_INVALID before any launch: a type code outside the lists above, n_images, H or W < 1, n_images * H > INT32_MAX, W >
 * INT32_MAX / 255, a weight outside [0, 255] or both zero, images == NULL with unequal weights, n < 0, stream_id outside {0, 1},
 * step < 0 without step_dev, a null or misaligned row_off, a null output.  n == 0: no launch. */
int lse_pixel_rows_build(const void *images, int32_t pix_type, const void *msk, int32_t msk_type, int32_t n_images, int32_t H,
                         int32_t W, int32_t w_active, int32_t w_idle, int64_t *row_off, lse_stream_t stream);
int lse_pixel_draw(const void *images, int32_t pix_type, const void *msk, int32_t msk_type, int32_t n_images, int32_t H, int32_t W,
                   int32_t w_active, int32_t w_idle, const int64_t *row_off, uint64_t seed, int32_t stream_id,
                   const int64_t *step_dev, int64_t step, int32_t n, int32_t *indices, int32_t *weights, lse_stream_t stream);

/* ---- whole-image rays of one camera (the eval set): the composer's ray arithmetic over a row-major pixel range -------------
 * Pixel p = first + i (y = p / W, x = p % W) of an H x W camera with the pose pose[3, 4] (device, f32; one row of a pose table)
 * writes row i of origins / directions [n, 3] and pixel_area / directions_norm [n]: the device functions of lse_compose_batch, so
 * the values are bit-equal to what the composer writes for the same (pose, y, x).  One thread per pixel, one launch.
 * LSE_E_INVALID before any launch: first < 0, n < 0, first + n > H * W, a zero focal length, a null pose or output.  n == 0: no-op. */
typedef struct lse_camera_desc {
    float fx, fy, cx, cy;
    float dist[6];          /* (k1, k2, k3, k4, p1, p2); read when `distort` != 0 */
    int32_t distort;
    int32_t H, W;
} lse_camera_desc;
int lse_camera_rays(const lse_camera_desc *cam, const float *pose, int64_t first, int64_t n, float *origins, float *directions,
                    float *pixel_area, float *directions_norm, lse_stream_t stream);

/* ---- spline camera poses: the composer's pose tables from a SplineCameraOptimizer's parameters, on the device -------------
 * Replaces, in front of every step, SplineCameraOptimizer.get_rgb_cameras / get_evs_cameras / get_deblur_cameras of
 * lsenerf_amd/cameras.py (with exp_map_to_quat_map, vectorized_generalized_interpolation, slerp, quat_map_to_mtx;
 * R:lse_nerf/ns_camera_optimizer.py:130-197 over R:lse_nerf/interpolation_utils.py:56-233) -- what lsenerf_amd.data.spline_tables
 * + BatchComposer.set_poses did with some 60 torch launches per step.
 * A QUERY is one 3x4 row of a pose table.  Queries are numbered over up to three segments, colour | prev | next (n_query[s] rows
 * of table s; 0 = the table is not fed).  A segment is "rgb" (evs[s] = 0: the plain spline pose; the deblur table is an "rgb"
 * segment whose queries are the four exposure times of every camera) or "evs" (evs[s] = 1: pose @ dM', dM' = dM with its
 * translation column times *scale, as get_evs_cameras builds it while the optimiser is on).
 * Per query the caller gives the bracketing control index idx (searchsorted(right = True), clamped to [1, n_ctrl - 1], minus 1,
 * after the clip of the time to the control times) and the fraction frac = (ts - t0) / (t1 - t0): they depend on buffers that
 * never change during training, so they are computed once, with the torch expressions of cameras.py.  ctrl_tangents and scale
 * are read from the parameters' own storage at every launch: an in-place optimiser update is seen by the next launch (or graph
 * replay) without a copy.  Everything is evaluated in f32. */
typedef struct lse_spline_desc {
    int32_t n_ctrl;              /* control points K >= 2 */
    int32_t n_query[3];          /* rows of the colour | prev | next table fed by the spline */
    int32_t evs[3];              /* per segment: 0 "rgb", 1 "evs" */
    int32_t csr_len;             /* entries of csr_query = 2 * (n_query[0] + n_query[1] + n_query[2]); read by the backward */
    float dM[16];                /* row-major 4x4 relative pose rgb camera -> event camera (host values; "evs" segments) */
    const float *ctrl_tangents;  /* [n_ctrl, 6] (translation, rotation vector) */
    const float *scale;          /* [1] */
    const int32_t *idx;          /* [queries] in [0, n_ctrl - 2] */
    const float *frac;           /* [queries] */
    const int32_t *csr_start;    /* [n_ctrl + 1]: control point k owns csr_query[csr_start[k] .. csr_start[k + 1]) */
    const int32_t *csr_query;    /* the queries with idx == k or idx + 1 == k, ascending; read by the backward */
} lse_spline_desc;
/* One launch writes every row of the fed tables: col_pose [n_query[0], 3, 4] (= [cameras, G, 3, 4]), prev_pose / next_pose
 * [n_query[1 / 2], 3, 4].  The table of a segment with n_query == 0 is not touched (NULL allowed). */
int lse_spline_poses(const lse_spline_desc *desc, float *col_pose, float *prev_pose, float *next_pose, lse_stream_t stream);
/* d tables (the layout lse_compose_rays_bwd writes) -> d_ctrl_tangents [n_ctrl, 6], d_scale [1], both OVERWRITTEN; one launch.
 * The exact derivative of the expressions above as torch autograd takes it: `where` selects a branch, a clamped value passes no
 * gradient, norm at exactly zero has gradient zero (a control point whose rotation vector is exactly zero gets a zero rotation
 * gradient).  One wave per control point sums the queries of its list in a fixed order, one block sums d_scale over the "evs"
 * queries in a fixed order (no atomics): two runs are bit-equal, and a control point no query brackets receives exactly zero. */
int lse_spline_poses_bwd(const lse_spline_desc *desc, const float *d_col_pose, const float *d_prev_pose, const float *d_next_pose,
                         float *d_ctrl_tangents, float *d_scale, lse_stream_t stream);

/* ---- per-camera pose deltas: the composer's pose tables from the pose_adjustment of CameraOptimizer / PrevNextCamOptimizer ------
 * Replaces, in front of every step, lsenerf_amd.data.camera_tables + BatchComposer.set_poses for the per-camera optimisers of
 * lsenerf_amd/cameras.py (CameraOptimizer.forward over hom_exp_map_SO3xR3 / exp_map_SE3; R:lse_nerf/ns_camera_optimizer.py:214-414,
 * which R:lse_nerf/lse_datamanager.py:285-304 builds whenever optim_type is not "spline").
 * Up to three tables, colour | prev | next, are fed (n_cam[s] cameras; 0 = the table is not fed).  Row c of table s is
 *   [R_corr(c) R0(c) | t0(c) + t_corr(c)],  (R_corr | t_corr) = exp_map(adj[s][c]),  (R0 | t0) = base[s][c];
 * a camera with frozen[s][c] != 0 gets (R_corr | t_corr) = (I | 0).  mode[s] picks the exponential:
 *   LSE_POSE_SO3XR3  theta = sqrt(max(|w|^2, 1e-4)), R = I + (sin theta / theta) K + ((1 - cos theta) / theta^2) K^2, t_corr = v;
 *   LSE_POSE_SE3     |w|^2 < 1e-4: a = 1 - t2/6, b = 1/2 - t2/24, c = 1/6 - t2/120, else the closed forms;
 *                    R = I + a W + b W^2, t_corr = (I + b W + c W^2) v,
 * with adj row = (v, w).  adj is read from the parameters' own storage at every launch: an in-place optimiser update is seen by the
 * next launch (or graph replay) without a copy.  Everything is f32; (1 - cos t) / t^2 and (t - sin t) / t^3 and their derivatives
 * are evaluated without cancellation (series below t = 2, half-angle form above).
 * shared_prev_next != 0: ONE parameter block feeds prev and next (adj[2] == adj[1], frozen[2] == frozen[1], equal counts and
 * modes), each over its own base poses; its gradient is the sum of the two rows. */
#define LSE_POSE_SO3XR3 0
#define LSE_POSE_SE3 1
typedef struct lse_pose_delta_desc {
    int32_t n_cam[3];            /* cameras (= rows) of the colour | prev | next table fed */
    int32_t mode[3];             /* LSE_POSE_SO3XR3 | LSE_POSE_SE3 */
    int32_t shared_prev_next;    /* 0 | 1 */
    const float *base[3];        /* [n_cam[s], 3, 4] the scene's camera_to_worlds (static) */
    const float *adj[3];         /* [n_cam[s], 6] pose_adjustment (translation part, rotation vector) */
    const uint8_t *frozen[3];    /* [n_cam[s]] non-trainable cameras, or NULL */
} lse_pose_delta_desc;
/* One launch (one thread per row) writes every row of the fed tables [n_cam[s], 3, 4]; the table of a segment with n_cam == 0 is
 * not touched (NULL allowed). */
int lse_pose_delta_tables(const lse_pose_delta_desc *desc, float *col_pose, float *prev_pose, float *next_pose, lse_stream_t stream);
/* d tables -> d_adj_* [n_cam[s], 6], every element OVERWRITTEN; one launch, one thread per (parameter block, camera), no atomics: two
 * runs are bit-equal.  The derivative torch autograd takes of cameras.py: `where` selects a branch and the clamp passes no gradient
 * below its bound (SO3xR3 coefficients are constants below |w| = 0.01); a frozen camera gets exact zeros.  With shared_prev_next the
 * camera's gradient, row(prev) + row(next) in that order, goes to d_adj_prev and d_adj_next is not written (NULL allowed). */
int lse_pose_delta_tables_bwd(const lse_pose_delta_desc *desc, const float *d_col_pose, const float *d_prev_pose,
                              const float *d_next_pose, float *d_adj_col, float *d_adj_prev, float *d_adj_next, lse_stream_t stream);

/* ---- TSDF fusion (csrc/tsdf.hip, csrc/mesh.hip; ABI 6, additive): depth renders -> a mesh of the observed surface ----------------
 * All floats are f32, every operation is rounded on its own (no FMA), `/` and sqrtf are the correctly rounded ones, every
 * comparison is false on NaN.  The lattice, its point order and its positions are those of the mesh-export section
 * (lse_lattice_positions, bit for bit).
 *
 * State.  tw f32 [points, 2] = (tsdf, weight) and cw f32 [points, 4] = (r, g, b, colour weight), both zero before the first view;
 *   tw 8-byte, cw 16-byte aligned.  Colours are fused iff cw and rgb are both non-null; otherwise cw is not touched.
 * lse_tsdf_integrate.  cam: intrinsics of all views; poses f32 [n_views, 3, 4] (device; rows M[r][c] of a pose table, camera to
 *   world, the camera looks along -z); depth, acc f32 [n_views, H * W] row-major; rgb f32 [n_views, H * W, 3] or NULL.  For every
 *   lattice point x the views j = 0 .. n_views - 1 are folded in ascending order; "skip" leaves the point's state as it is:
 *     v_k  = x_k - M[k][3]
 *     xc   = (v_0 * M[0][0] + v_1 * M[1][0]) + v_2 * M[2][0],  yc and zc with columns 1 and 2         (R^T v)
 *     z    = -zc;  skip unless z > 0
 *     X    = xc / z,  Y = yc / z
 *     if cam.distort, with (k1, k2, k3, k4, p1, p2) = cam.dist:
 *       r  = X * X + Y * Y;  skip unless r <= r2_max
 *       d  = 1 + r * (k1 + r * (k2 + r * (k3 + r * k4)))
 *       xd = (d * X + ((2 * p1) * X) * Y) + p2 * (r + (2 * X) * X)
 *       yd = (d * Y + ((2 * p2) * X) * Y) + p1 * (r + (2 * Y) * Y);  (X, Y) = (xd, yd)
 *     u    = rintf(X * fx + cx),  v = rintf(cy - Y * fy)       (rays sit at integer pixel coordinates; ties to even)
 *     skip unless u >= 0 && u < (float)W && v >= 0 && v < (float)H        (in float, before any conversion)
 *     dp   = depth[j][(int)v * W + (int)u],  a = acc[j][same]
 *     dist = sqrtf((v_0 * v_0 + v_1 * v_1) + v_2 * v_2)
 *     if a >= min_acc:  skip unless dp > 0 && dp < +inf;  sdf = dp - dist          ("surface")
 *     else if carve:    sdf = +inf                       (the ray sees through: observed empty; a NaN accumulation lands here)
 *     else skip
 *     skip if sdf < -truncation                                                    (occluded)
 *     t    = fminf(1, sdf / truncation)
 *     tsdf = (tsdf * weight + t) / (weight + 1);  weight = weight + 1
 *     if colours are fused, "surface" and sdf <= truncation, with q = rgb[j][pixel]:
 *       c_k = (c_k * cweight + q_k) / (cweight + 1) for k = 0, 1, 2;  cweight = cweight + 1
 *   The state passes through f32 registers only, so one call with V views gives the bytes of V calls with one view each, in order.
 *   r2_max: the largest X^2 + Y^2 of the undistorted camera points of the image's border pixels (+inf for a pinhole camera; unread
 *   without cam.distort): beyond it the polynomial may fold far-off points back into the image.
 *   One thread per lattice point; per launch the state costs one 8-byte and one 16-byte load and store per point (48 B), whatever
 *   n_views.  LSE_E_INVALID before any launch: a bad lattice, n_views < 0, a truncation that is not positive and finite, a zero focal
 *   length, H or W outside [1, 2^24] or 2^31 pixels or more, a null tw / cam / box (and, with n_views > 0, poses / depth / acc),
 *   misaligned tw or cw.  n_views == 0: no-op.
 * Field.  The surface-nets input of a fused volume is -tsdf where weight >= min_weight and NaN elsewhere ("unobserved"), at level 0:
 *   inside = behind the observed surface.
 * lse_surface_nets_count_ex / lse_surface_nets_emit_ex: the mesh-export pair with `flags`; flags == 0 is that pair, bit for bit (the
 *   old entry points call the same bodies with 0), any other unknown bit is refused.  With LSE_NETS_SKIP_NAN
 *     a cell is active iff its corners are neither all inside nor all outside AND none of the 8 is NaN;
 *     a lattice edge gives its quad iff it does without the flag AND the four cells C0 .. C3 around it are all active (equivalently:
 *     none of the 18 lattice points of those cells is NaN);
 *   order, winding, vertex placement, workspace and capacities are unchanged.  Count and emit must be given the same flags.  No
 *   surface is built against unobserved space: the mesh is open where observation ends.
 * lse_tsdf_vertex_colors.  vertices, out f32 [n, 3]; count = min(n, *n_dev) (n_dev nullable); rows at or beyond count are not
 *   written.  Per vertex and axis k
 *     u_k = ((vertex_k - lo_k) / (hi_k - lo_k)) * (float)n_k,  fl = floorf(u_k)
 *     c_k = fl >= (float)(n_k - 1) ? n_k - 1 : (fl > 0 ? (int)fl : 0)         (NaN -> 0: clamped into the first / last cell)
 *     f_k = fminf(fmaxf(u_k - (float)c_k, 0), 1)                              (NaN -> 0)
 *   and over the corners (dx, dy, dz) of cell c in ascending dx * 4 + dy * 2 + dz, starting from sums of 0:
 *     wt = ((dx ? f_0 : 1 - f_0) * (dy ? f_1 : 1 - f_1)) * (dz ? f_2 : 1 - f_2)
 *     if cw[corner].weight > 0:  s_k = s_k + wt * cw[corner].c_k;  W = W + wt
 *   out_k = W > 0 ? s_k / W : 0. */
#define LSE_NETS_SKIP_NAN 1
int lse_tsdf_integrate(float *tw, float *cw, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi,
                       const lse_camera_desc *cam, const float *poses, int32_t n_views, const float *depth, const float *acc,
                       const float *rgb, float truncation, float min_acc, int32_t carve, float r2_max, lse_stream_t stream);
int lse_surface_nets_count_ex(const float *sigma, int32_t nx, int32_t ny, int32_t nz, float level, int32_t flags, void *workspace,
                              int64_t workspace_bytes, int64_t *totals, lse_stream_t stream);
int lse_surface_nets_emit_ex(const float *sigma, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi, float level,
                             int32_t flags, const void *workspace, int64_t workspace_bytes, int64_t cap_vertices, int64_t cap_quads,
                             float *vertices, int32_t *triangles, lse_stream_t stream);
int lse_tsdf_vertex_colors(const float *cw, int32_t nx, int32_t ny, int32_t nz, const float *h_lo, const float *h_hi,
                           const float *vertices, int64_t n, const int64_t *n_dev, float *out, lse_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LSE_HIP_H */
