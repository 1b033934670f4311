/*
 * dev_knobs.h -- tuning knobs of the DEVELOPMENT build (make dev -> liblse_hip_dev.so, compiled with -DLSE_DEV_KNOBS).
 *
 * Not part of the C-ABI: the library that ships (liblse_hip.so, include/lse_hip.h) has no global or thread-local state, does not
 * export these two functions and compiles the knobs below in as constants (csrc/api.cpp); the superseded kernel variants they
 * select (other MLP tile shapes, the generic MLP backward, the serial marcher) exist in the development build only.  The hash-grid
 * kernels have no such variants: csrc/hashgrid.hip compiles to the same kernels in both builds.  Used by the A/B tools under tools/
 * and by the tests that hold every variant against the oracle (tests/test_gpu_parity.py, `_lib.dev_library()`).
 *
 *   "compact_features_groups"  level groups per launch of lse_compact_features (default 4)
 *   "mlp_fwd_cfg" / "mlp_bwd_cfg"  CT * 10 + NW tile shape of the f32-MFMA fused MLP kernels (default 28; 44 = A/B partner)
 *   "mlp_bwd_impl"      1 = contiguous-tiles fused backward (bias gradient inside the dW0 MFMAs; default), 0 = generic kernel
 *   "mlp_bwd3_cfg"      CT * 100 + NW of the bf16-piece fused backward (default 208; 112, 108, 204 = A/B partners)
 *   "mlp_act_nt"        non-temporal stores of saved activations (default 0)
 *   "hash_bwd_probes" / "hash_bwd_few_runs" / "hash_bwd_stage_max"   defaults of lse_hash_bwd_opts.second_probe (3), .few_runs (8)
 *                       and .stage_max (48), for A/B runs of whole steps (a single call sets them in lse_hash_bwd_opts;
 *                       lsenerf_amd/ops.py HASH_BWD_DENSE_STEPS passes few_runs 3 / stage_max 56 that way, as call arguments)
 *   "traverse_vec"      1 = 64-steps-at-once marcher for constant step sizes (default, bit-identical), 0 = serial loop only
 * Integer outputs never depend on these; floating-point results agree within rounding.  Returns LSE_E_INVALID for an unknown name.
 */
#ifndef LSE_DEV_KNOBS_H
#define LSE_DEV_KNOBS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int lse_set_option(const char *name, int64_t value);
int lse_get_option(const char *name, int64_t *value);
#ifdef __cplusplus
}
#endif
#endif
