// Error string + device probe for libmirror_hip.
#include <stdarg.h>
#include <string.h>

#include "common.h"

static thread_local char g_err[512] = "";

void mh_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

extern "C" const char* mh_last_error(void) { return g_err; }

// The kernel instance the calling thread's last mh_gemm launched ("gemm_pq_kernel<float,false,false,part>", ...): the launch sites
// record it, so profilers name launches without restating the dispatch rules (mh_gemm_variant_name)
static thread_local char g_variant[160] = "";
void gemm_note_variant(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_variant, sizeof(g_variant), fmt, ap);
    va_end(ap);
}
extern "C" const char* mh_gemm_variant_name(void) { return g_variant; }
// The form ("add:quad", "softmax_fwd:block,scalar", ...) the calling thread's last elementwise / row-kernel entry point chose: the
// pointer of a string literal, so a call pays one store (mh_last_form)
static thread_local const char* g_form = "";
extern "C" void mh_note_form(const char* literal) { g_form = literal; }
extern "C" const char* mh_last_form(void) { return g_form; }
extern "C" int mh_version(void) { return 123; }   // 123: mh_layernorm_bwd takes one descriptor (mh_ln_bwd) — mh_layernorm_bwd_lm / _fan / _drop are gone, an argument list changed, later mh_note_form / mh_last_form, later mh_survprobe_grad / mh_survprobe_risk (survprobe.hip), later mh_linprobe_proba (linprobe.hip) and mh_auroc_counts_many (classify.hip) — new entry points only (a library without them fails in _lib.load()); 122 (later): mh_rna_block_fits / mh_rna_block_lds_bytes (rna_block.hip) — new entry points only (a library without them fails in _lib.load()); mh_loss_terms.scratch grows from 8 floats to 8 + Bc + 64, no argument list or field changed (kernels.py checks the size); 122: two entry points removed (the four-wave GEMM experiment and the main-loop switch of the 256 x 256-tile GEMM are gone), no argument list changed, later mh_ppeg_bwd (ppeg.hip) — a new entry point only (a library without it fails in _lib.load()); 121: mh_nys_attn1_bwd and mh_nys_attn3_bwd lost their trailing selector argument (the two-kernel backward paths it chose are gone): argument lists changed, later mh_optim_step (optim.hip) — a new entry point only (a library without it fails in _lib.load()); 120: mh_cls_ce_fwd / _bwd, mh_cls_confusion, mh_auroc_counts (classify.hip), later mh_adam_ema (loss.hip) and mh_ema_update_many (ema.hip) — new entry points only, no argument list changed (a library without them fails in _lib.load()); 119: mh_surv_loss_fwd / _bwd, mh_surv_risk, mh_cindex_counts (survival.hip); 118: mh_gemm_desc.r_bf16 = 2 (f32 R beside a bf16 C); 117: mh_skinny_fwd takes any K / row stride; 116: mh_keymask_plan; 115: lm_scale of mh_layernorm_fwd_lm / _bwd_lm; 114: mlm / heads of mh_pinv_s2_bwd; 113: mlm of mh_nys_sim2; 112: row_mask of mh_layernorm_fwd_lm / _bwd_lm; 111: drop_rows_per_batch of mh_layernorm_bwd_drop; 110: mh_layernorm_bwd_drop, dt_dy of mh_layernorm_bwd_fan, the four-wave GEMM experiment (removed in 122); 109 (round 5, late): mh_adam(tick, hole), mh_noise_draws, mh_layernorm_bwd_fan, bias-gradient outputs of mh_mask_apply_bwd / mh_mse_masked_bwd / mh_layernorm_bwd_lm; 107-108 (round 5): mirror_amd/_lib.py refuses any other generation (ABI_VERSION), mh_resconv_bwd, res_conv inside mh_nys_attn3_fwd; 106 (round 4, late): step glue riding on other launches (mh_adam clamp / counter, mh_rownorm_ shadow, scratch_zeroed of the pinv backward tails, addends of mh_skinny_fwd / mh_reparam_bwd), mh_exp_*; 105 (round 4): lm_ld of the mh_nys_* entry points, mh_lm_merge, gadd in dy's dtype, xpm optional;   // 104 (round 3): mh_gemm_desc.epi / row windows, mh_layernorm_fwd_lm(xpm_bf16), mh_skinny_fwd(dt_x, dt_y), mh_pinv_chain_fwd(z0f, stats64), new entry points

// 1 when the library was built with -DMH_EXP (make EXP=1): the timing-experiment switches (MH_EXP_CHAIN_SKIP, and MH_EXP_SKIP
// in the Python host) only exist in such a build; the default build answers 0 and the host refuses the variables.
extern "C" int mh_exp_build(void) {
#ifdef MH_EXP
    return 1;
#else
    return 0;
#endif
}

extern "C" int mh_device_ok(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        mh_set_error("mh_device_ok: no HIP device visible");
        return 0;
    }
    int ok = 0;
    for (int i = 0; i < n; i++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, i) == hipSuccess && strstr(p.gcnArchName, "gfx950")) ok++;
    }
    if (!ok) mh_set_error("mh_device_ok: no gfx950 device (this library is MI355X-only)");
    return ok;
}
