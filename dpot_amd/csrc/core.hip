// core.hip - error reporting + version for libdpot_hip.so
#include "common.h"

namespace dpot {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    set_error("%s: %s", what, hipGetErrorString(err));
    return DPOT_EHIP;
  }
  return DPOT_OK;
}

// DPOT_TUNE="key=val,key=val" (integers; unknown keys are ignored here - dpot_amd/ops.py rejects them): parsed on first use.
// Spaces around an entry are skipped, as ops.py strips them ("panel=0, gn_fuse=0").
int tune(const char* key, int dflt) {
  static const char* env = getenv("DPOT_TUNE");
  if (!env || !*env) return dflt;
  const size_t kl = strlen(key);
  for (const char* p = env; *p;) {
    const char* end = strchr(p, ',');
    while (*p == ' ' || *p == '\t') ++p;
    const size_t len = end ? (size_t)(end - p) : strlen(p);
    if (len > kl + 1 && strncmp(p, key, kl) == 0 && p[kl] == '=') return atoi(p + kl + 1);
    if (!end) break;
    p = end + 1;
  }
  return dflt;
}

}  // namespace dpot

/* 0.2.6: round 6 ABI - dpot_adam_step_packs (Adam that writes the bf16 weight packs); dpot_gemm_bf16p_pair back to its 0.2.0
 * argument list (the row-form operand / transposed-output arguments of 0.2.5 are gone with the kernels they selected);
 * dpot_afno_fused_bwd removed; every fallback selector behind DPOT_TUNE
 * 264: dpot_spectral_resize, dpot_spectral_resize_pad (csrc/resize.hip)
 * 266: dpot_mlp_wgrad_batch, dpot_afno_wgrad_batch, dpot_wgrad_batch_finalize and their queries (csrc/gemm_tn.hip): the weight
 * gradients of several DPOT blocks per launch
 * 267: dpot_dft3_supported, dpot_rfft3, dpot_irfft3 (csrc/dft3.hip): the transforms of the 3-D model's AFNO3D
 * 268: dpot_wgrad_flush_async, dpot_wgrad_wait, dpot_wgrad_lane_* (csrc/gemm_tn.hip): the batched weight gradients on a
 * library-owned stream beside the caller's
 * 269: dpot_patchify3, dpot_unpatchify3, dpot_fold3 (csrc/patch3d.hip): the index rearrangements at the two ends of DPOTNet3D
 * 270: dpot_eval3_stats, dpot_eval3_finalize and their queries (csrc/evalmetrics3d.hip): the evaluation metrics of 3-D rollouts
 * 271: mlp_chain / afno_chain on dpot_mlp_wgrad_batch, dpot_afno_wgrad_batch, dpot_wgrad_batch_finalize, dpot_wgrad_flush_async;
 * dpot_tn_chain_count, dpot_tn_chain_nodes, dpot_*_wgrad_batch_chain, dpot_*_wgrad_chain_ws_elems (csrc/gemm_tn.hip): chained
 * token ranges in the batched weight gradients
 * 272: dpot_lane_init, dpot_lane_ready, dpot_lane_pending, dpot_lane_shutdown, dpot_lane_fork, dpot_lane_join (csrc/gemm_tn.hip):
 * a table of library-owned lanes; the weight-gradient lane is lane 0, the side lane of the step's small chains lane 1
 * 273: dpot_aa_lrelu_fwd, dpot_aa_lrelu_bwd, dpot_aa_up_fwd, dpot_aa_up_adj and their queries (csrc/aa_act.hip): the anti-aliased
 * activation of the CDPOT model
 * 274: the lanes move to csrc/lane.hip; dpot_wgrad_flush_async, dpot_wgrad_wait and dpot_wgrad_lane_* removed (lane 0 is forked
 * and joined through dpot_lane_* like lane 1)
 * 275: dpot_fno_rfft2, dpot_fno_irfft2, dpot_fno_mix, dpot_fno_mix_wgrad, dpot_fno_dact, dpot_fno_max_size (csrc/fno.hip): the
 * kernels of the FNO baseline; nothing existing changed
 * 276: dpot_groupnorm_kernel_kind, dpot_groupnorm_kernel_kinds, dpot_groupnorm_chunks (csrc/norm.hip): host-only queries of the
 * GroupNorm route selection the launchers read; nothing existing changed
 * 277: dpot_fno3_rfft3, dpot_fno3_irfft3, dpot_fno3_mix, dpot_fno3_mix_wgrad, dpot_fno3_max_size, dpot_fno3_ws_elems
 * (csrc/fno3.hip): the kernels of the 3-D FNO baseline; dpot_adam_step_pairs (csrc/loss_opt.hip): Adam with one second moment
 * per complex pair; nothing existing changed
 * 278: dpot_afno_mlp2_plan, dpot_afno_mlp2_plans (csrc/afno_mlp.hip): host-only queries of the mixer's kernel selection the
 * launcher reads; nothing existing changed */
extern "C" int dpot_version(void) { return 280; }
extern "C" int dpot_tune(const char* key, int dflt) { return dpot::tune(key, dflt); }
extern "C" const char* dpot_last_error(void) { return dpot::g_err; }
