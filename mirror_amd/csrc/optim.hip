// The arena optimizer: torch.optim.Adam(weight_decay), torch.optim.AdamW and torch.optim.SGD(momentum, nesterov) over the flat f32
// arenas of TrainEngine (what timm's create_optimizer_v2 builds for --opt adam / adamw / sgd / nesterov / momentum,
// train_mirror.py:742-746).  One device body serves the four entry points: mh_optim_step, mh_optim_groups (one learning
// rate per parameter group and a group that is skipped: mirror_amd.optim.ArenaOptimizer), and mh_adam / mh_adam_ema, which are rule
// Adam without decay behind their older argument lists.  Everything a step carries rides in the same pass: the hole of a two-launch
// step, the clamped element, the dropout counter, the bf16 shadow, the EMA.
//
// The device step state is six floats {t, 1 - b1^t, 1 - b2^t, lr, clip, |g|}: optim_tick_kernel advances t and refreshes the two
// bias corrections, the host writes lr, mh_grad_clip writes the clip factor and the gradient norm it came from, and the update reads
// [1..4] (the EMA decay reads t) — nothing step-dependent is a launch argument, so a captured HIP graph replays with the right step.
//
// HBM-bound, 4 elements per thread, 16-B accesses.  Bytes per parameter (f32 p r/w, g r, moments r/w, bf16 shadow w):
//   adam / adamw  8 + 4 + 8 + 8 + 2 = 30      sgd (momentum)  8 + 4 + 8 + 2 = 22      sgd (momentum = 0)  8 + 4 + 2 = 14
// plus 1/8 B for the decay-group byte of each 8-element block (every parameter starts on one), plus 8 B with the EMA.
#include "common.h"

// one update of one element; `wd` is the element's own weight decay, `c` what is uniform over the launch
struct optim_consts {
    float lr, b1, b2, eps, step, isq, mu, gscale;
    int nesterov;
};

// The two moment updates are written with explicit fmaf, in the forms that the Adam kernel before this one was compiled to and that
// tests/golden/golden_adam_bits.npz pins: in the quad loop m = fma(1 - b1, gr, b1 m), in the scalar tail (TAIL)
// m = fma(b1, m, (1 - b1) gr); v = fma((1 - b2) gr, gr, b2 v) in both.
template <int RULE, bool MOM, bool TAIL = false>
__device__ __forceinline__ void optim_elem(float& p, const float g, float& m, float& v, const float wd, const optim_consts& c) {
    if constexpr (RULE == MH_OPT_SGD) {
        const float gr = g * c.gscale + wd * p;          // grad.add(param, alpha=weight_decay)
        float st = gr;
        if constexpr (MOM) {
            m = c.mu * m + gr;                           // buf.mul_(momentum).add_(grad): a zero buffer gives torch's first-step buf = grad
            st = c.nesterov ? gr + c.mu * m : m;
        }
        p -= c.lr * st;
    } else {
        float gr = g * c.gscale;
        if constexpr (RULE == MH_OPT_ADAM) gr += wd * p;             // L2: the decay goes through the moments
        if constexpr (RULE == MH_OPT_ADAMW) p *= 1.f - c.lr * wd;    // decoupled: param.mul_(1 - lr * weight_decay) first
        m = TAIL ? fmaf(c.b1, m, (1.f - c.b1) * gr) : fmaf(1.f - c.b1, gr, c.b1 * m);
        v = fmaf((1.f - c.b2) * gr, gr, c.b2 * v);
        p -= c.step * m / (sqrtf(v) * c.isq + c.eps);
    }
}

#define OPTIM_PARAMS_ float *__restrict__ p, const float *__restrict__ g, float *__restrict__ m, float *__restrict__ v, bf16_t *__restrict__ shadow, \
                      long n, mh_optim_cfg o, float lr, float bc1, float bc2, const uint8_t *__restrict__ gmap,                                     \
                      const float *__restrict__ group_wd, const float *__restrict__ group_lr, int n_groups, float gscale, const float *__restrict__ state, long clamp_i,               \
                      float clamp_lo, float clamp_hi, long hole_lo4, long hole_hi4, float *__restrict__ ema, mh_ema_cfg ecfg
#define OPTIM_ARGS_ p, g, m, v, shadow, n, o, lr, bc1, bc2, gmap, group_wd, group_lr, n_groups, gscale, state, clamp_i, clamp_lo, clamp_hi, hole_lo4, hole_hi4, ema, ecfg

// gmap: one byte per 8-element block = the block's decay group, group_wd[byte] its weight decay (NULL: no decay anywhere).
// Quads [hole_lo4, hole_hi4) are left alone: the range the other launch of a two-launch step updates (the RNA encoder's parameters,
// whose gradients are complete 2 ms before the step's last one: TrainEngine's early update).
// state == NULL (mh_adam only): lr and the bias corrections bc1, bc2 are the launch arguments, and there is no clip factor.
// GROUPS (mh_optim_groups; gmap and state are required): group_lr[byte] is the block's learning rate in place of state[3], held in a
// second LDS table beside wd_s together with the step size lr / bc1 it gives — the same division that forms c.step below, done once
// per group — and blocks whose byte is MH_OPT_SKIP_GROUP are left alone.
template <int RULE, bool EMA, bool MOM, bool GROUPS = false>
__device__ __forceinline__ void optim_body(OPTIM_PARAMS_) {
    __shared__ float wd_s[256];
    __shared__ float lr_s[GROUPS ? 256 : 1], step_s[GROUPS && RULE != MH_OPT_SGD ? 256 : 1];
    __shared__ float ew_s;
    if (gmap && (int)threadIdx.x < n_groups) wd_s[threadIdx.x] = group_wd[threadIdx.x];
    if constexpr (GROUPS) {
        if ((int)threadIdx.x < n_groups) {
            const float glr = group_lr[threadIdx.x];
            lr_s[threadIdx.x] = glr;
            if constexpr (RULE != MH_OPT_SGD) step_s[threadIdx.x] = glr / state[1];
        }
    }
    if (EMA && threadIdx.x == 0) ew_s = ema_weight(ecfg, (double)state[0]);     // 1 - decay(t), t as the tick has just left it
    if (gmap || EMA) __syncthreads();
    const float ew = EMA ? ew_s : 0.f;
    if (state) {
        bc1 = state[1];
        bc2 = state[2];
        lr = state[3];
        gscale *= state[4];              // the gradient is scaled (average, clip factor) BEFORE any weight decay
    }
    optim_consts c;
    c.lr = lr;
    c.b1 = o.beta1; c.b2 = o.beta2; c.eps = o.eps; c.mu = o.momentum; c.nesterov = o.nesterov;
    c.gscale = gscale;
    c.step = RULE == MH_OPT_SGD ? 0.f : lr / bc1;
    c.isq = RULE == MH_OPT_SGD ? 0.f : rsqrtf(bc2);
    const long n4 = n / 4;
    const long hole = hole_hi4 - hole_lo4, live4 = n4 - hole;
    for (long q0 = (long)blockIdx.x * 256 + threadIdx.x; q0 < live4; q0 += (long)gridDim.x * 256) {
        const long q = q0 < hole_lo4 ? q0 : q0 + hole;       // the live quads are numbered densely: no idle threads over the hole
        const int grp = gmap ? gmap[q >> 1] : 0;
        if (GROUPS && grp == MH_OPT_SKIP_GROUP) continue;
        const float wd = gmap ? wd_s[grp] : 0.f;
        if constexpr (GROUPS) {
            c.lr = lr_s[grp];
            if constexpr (RULE != MH_OPT_SGD) c.step = step_s[grp];
        }
        float4 pp = reinterpret_cast<float4*>(p)[q];
        const float4 gg = reinterpret_cast<const float4*>(g)[q];
        float4 mm = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
        if constexpr (MOM) mm = reinterpret_cast<float4*>(m)[q];
        if constexpr (RULE != MH_OPT_SGD) vv = reinterpret_cast<float4*>(v)[q];
        float* pa = &pp.x; const float* ga = &gg.x; float* ma = &mm.x; float* va = &vv.x;
#pragma unroll
        for (int e = 0; e < 4; e++) optim_elem<RULE, MOM>(pa[e], ga[e], ma[e], va[e], wd, c);
        // one element (logit_scale, train_mirror.py:1255) is clamped right behind its update: master, shadow and EMA get the clamped value
        if ((clamp_i >> 2) == q && clamp_i >= 0) pa[clamp_i & 3] = clamp_keep_nan(pa[clamp_i & 3], clamp_lo, clamp_hi);
        reinterpret_cast<float4*>(p)[q] = pp;
        if constexpr (MOM) reinterpret_cast<float4*>(m)[q] = mm;
        if constexpr (RULE != MH_OPT_SGD) reinterpret_cast<float4*>(v)[q] = vv;
        if constexpr (EMA) {
            float4 ee = reinterpret_cast<float4*>(ema)[q];
            ee.x = ema_lerp(ee.x, pp.x, ew);
            ee.y = ema_lerp(ee.y, pp.y, ew);
            ee.z = ema_lerp(ee.z, pp.z, ew);
            ee.w = ema_lerp(ee.w, pp.w, ew);
            reinterpret_cast<float4*>(ema)[q] = ee;
        }
        if (shadow) {
            uint2 sh;
            sh.x = pack_bf2(pa[0], pa[1]);
            sh.y = pack_bf2(pa[2], pa[3]);
            reinterpret_cast<uint2*>(shadow)[q] = sh;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = n4 * 4 + threadIdx.x;
        const int grp = gmap ? gmap[i >> 3] : 0;
        if (GROUPS && grp == MH_OPT_SKIP_GROUP) return;
        const float wd = gmap ? wd_s[grp] : 0.f;
        if constexpr (GROUPS) {
            c.lr = lr_s[grp];
            if constexpr (RULE != MH_OPT_SGD) c.step = step_s[grp];
        }
        float pn = p[i], mi = 0.f, vi = 0.f;
        if constexpr (MOM) mi = m[i];
        if constexpr (RULE != MH_OPT_SGD) vi = v[i];
        optim_elem<RULE, MOM, true>(pn, g[i], mi, vi, wd, c);
        if (i == clamp_i) pn = clamp_keep_nan(pn, clamp_lo, clamp_hi);
        p[i] = pn;
        if constexpr (MOM) m[i] = mi;
        if constexpr (RULE != MH_OPT_SGD) v[i] = vi;
        if (shadow) shadow[i] = f2bf(pn);
        if constexpr (EMA) ema[i] = ema_lerp(ema[i], pn, ew);
    }
}

// 8 waves per SIMD asked for outright: left alone, the compiler spends 75 VGPRs (6 waves) on the EMA instances of the Adam rules, all
// of the excess on hoisting the run-time decay lookup
template <int RULE, bool EMA, bool MOM>
__global__ __launch_bounds__(256, 8) void optim_kernel(OPTIM_PARAMS_) {
    optim_body<RULE, EMA, MOM>(OPTIM_ARGS_);
}
// mh_optim_groups' instances: the same body with the per-group learning rate and the skipped group
template <int RULE, bool EMA, bool MOM>
__global__ __launch_bounds__(256, 8) void optim_groups_kernel(OPTIM_PARAMS_) {
    optim_body<RULE, EMA, MOM, true>(OPTIM_ARGS_);
}
// Rule Adam with no group map and no EMA runs under two plain names, which profiling tools read.  adam_kernel is the launch that ENDS
// a step (the whole arena, or everything around the hole): the tools cut a trace into steps at this name.
__global__ __launch_bounds__(256) void adam_kernel(OPTIM_PARAMS_) {
    optim_body<MH_OPT_ADAM, false, true>(OPTIM_ARGS_);
}
// the early launch of a two-launch step (a sub-range, beside the backward): same arithmetic under another name
__global__ __launch_bounds__(256) void adam_range_kernel(OPTIM_PARAMS_) {
    optim_body<MH_OPT_ADAM, false, true>(OPTIM_ARGS_);
}
#undef OPTIM_ARGS_

// t += 1 on the device (SGD too: the EMA decay and the fp8 delayed scaling read t); the Adam rules refresh their bias corrections
__global__ void optim_tick_kernel(float* state, int adam, float b1, float b2, long long* counter, long long counter_add) {
    if (counter) *counter += counter_add;      // the dropout streams' device-side base (functional.dropout_step_end) rides along
    if (!state) return;
    const float t = state[0] + 1.f;
    state[0] = t;
    if (adam) {
        state[1] = 1.f - powf(b1, t);
        state[2] = 1.f - powf(b2, t);
    }
}

// the argument checks and the launches of all four entry points; `name` is the entry point's own, for its messages
static int optim_launch(const char* name, float* p, const float* g, float* m, float* v, void* shadow, int64_t n, const mh_optim_cfg& o,
                        float lr, float bc1, float bc2, const uint8_t* group_map, const float* group_wd, const float* group_lr,
                        int n_groups, float gscale, float* dev_state, int64_t clamp_index, float clamp_lo, float clamp_hi, int64_t* counter, int64_t counter_add,
                        int tick, int64_t hole_lo, int64_t hole_hi, float* ema, const mh_ema_cfg* ema_cfg, mh_stream s) {
    if (n == 0) return MH_OK;
    const bool sgd = o.rule == MH_OPT_SGD, mom = !sgd || o.momentum != 0.f;
    MH_REQUIRE(p && g && (m || !mom) && (v || sgd), "%s: a buffer the rule reads is NULL", name);
    MH_REQUIRE(((uintptr_t)p & 15) == 0 && ((uintptr_t)g & 15) == 0 && ((uintptr_t)m & 15) == 0 && ((uintptr_t)v & 15) == 0 &&
                   ((uintptr_t)shadow & 7) == 0 && ((uintptr_t)ema & 15) == 0, "%s: buffers must be 16-byte aligned", name);
    MH_REQUIRE(!sgd || !o.nesterov || o.momentum > 0.f, "%s: Nesterov momentum requires a momentum", name);
    MH_REQUIRE(!group_map || (group_wd && n_groups >= 1 && n_groups <= 256), "%s: a group map needs 1..256 group decays", name);
    MH_REQUIRE(!group_lr || (group_map && dev_state && n_groups < MH_OPT_SKIP_GROUP + 1),
               "%s: per-group learning rates need a group map, dev_state and at most %d groups", name, MH_OPT_SKIP_GROUP);
    MH_REQUIRE(!ema || (dev_state && ema_cfg && ema_cfg->warmup_gamma > 0.0), "%s: the EMA needs dev_state and settings with warmup_gamma > 0", name);
    MH_REQUIRE(clamp_index < n, "%s: clamp_index %ld outside the %ld parameters", name, (long)clamp_index, (long)n);
    MH_REQUIRE(hole_lo >= 0 && hole_lo <= hole_hi && hole_hi <= n && hole_lo % 4 == 0 && (hole_hi % 4 == 0 || hole_hi == hole_lo) &&
                   (clamp_index < hole_lo || clamp_index >= hole_hi || hole_lo == hole_hi),
               "%s: hole [%ld, %ld) must be quad-aligned, inside the %ld parameters and not hold the clamped one", name, (long)hole_lo, (long)hole_hi, (long)n);
    if ((dev_state && tick) || counter)
        hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, tick ? dev_state : nullptr, sgd ? 0 : 1, o.beta1,
                           o.beta2, (long long*)counter, (long long)counter_add);
    const long live = n - (hole_hi - hole_lo);
    if (live == 0) return MH_OK;
    const mh_ema_cfg ec = ema ? *ema_cfg : mh_ema_cfg{0.0, 0.0, 1.0, 0.0, 0, 0};
#define OPTIM_LAUNCH_(KERN)                                                                                                               \
    hipLaunchKernelGGL(KERN, dim3((unsigned)min((long)mh_cdiv(mh_cdiv(live, 4), 256), 8192L)), dim3(256), 0, (hipStream_t)s, p, g, m, v,  \
                       (bf16_t*)shadow, (long)n, o, lr, bc1, bc2, group_map, group_wd, group_lr, n_groups, gscale, (const float*)dev_state,         \
                       clamp_index < 0 ? -1L : (long)clamp_index, clamp_lo, clamp_hi, (long)(hole_lo / 4), (long)(hole_hi / 4), ema, ec)
#define OPTIM_RULE_(RULE, MOM)                                                                                                  \
    do {                                                                                                                       \
        if (group_lr) { if (ema) OPTIM_LAUNCH_((optim_groups_kernel<RULE, true, MOM>)); else OPTIM_LAUNCH_((optim_groups_kernel<RULE, false, MOM>)); } \
        else if (ema) OPTIM_LAUNCH_((optim_kernel<RULE, true, MOM>));                                                          \
        else OPTIM_LAUNCH_((optim_kernel<RULE, false, MOM>));                                                                  \
    } while (0)
    // the kernel follows what is launched, not the entry point: plain Adam keeps the two names the profiling tools know
    if (o.rule == MH_OPT_ADAM && !group_map && !ema) { if (tick == 2) OPTIM_LAUNCH_(adam_range_kernel); else OPTIM_LAUNCH_(adam_kernel); }
    else if (o.rule == MH_OPT_ADAM) OPTIM_RULE_(MH_OPT_ADAM, true);
    else if (o.rule == MH_OPT_ADAMW) OPTIM_RULE_(MH_OPT_ADAMW, true);
    else if (mom) OPTIM_RULE_(MH_OPT_SGD, true);
    else OPTIM_RULE_(MH_OPT_SGD, false);
#undef OPTIM_RULE_
#undef OPTIM_LAUNCH_
    MH_LAUNCH_CHECK(name);
    return MH_OK;
}

extern "C" int mh_optim_step(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, const mh_optim_cfg* opt,
                             const uint8_t* group_map, const float* group_wd, int n_groups, float gscale, float* dev_state,
                             int64_t clamp_index, float clamp_lo, float clamp_hi, int64_t* counter, int64_t counter_add, int tick,
                             int64_t hole_lo, int64_t hole_hi, float* ema, const mh_ema_cfg* ema_cfg, mh_stream s) {
    if (n == 0) return MH_OK;
    MH_REQUIRE(opt && (opt->rule == MH_OPT_ADAM || opt->rule == MH_OPT_ADAMW || opt->rule == MH_OPT_SGD), "mh_optim_step: no settings, or an unknown rule");
    MH_REQUIRE(dev_state, "mh_optim_step: lr, the step and the clip factor are read from dev_state: it is required");
    return optim_launch("mh_optim_step", p, g, m, v, shadow, n, *opt, 0.f, 1.f, 1.f, group_map, group_wd, nullptr, n_groups, gscale, dev_state,
                        clamp_index, clamp_lo, clamp_hi, counter, counter_add, tick, hole_lo, hole_hi, ema, ema_cfg, s);
}

extern "C" int mh_optim_groups(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, const mh_optim_cfg* opt,
                               const uint8_t* group_map, const float* group_wd, const float* group_lr, int n_groups, float gscale,
                               float* dev_state, int64_t clamp_index, float clamp_lo, float clamp_hi, int64_t* counter,
                               int64_t counter_add, int tick, int64_t hole_lo, int64_t hole_hi, float* ema, const mh_ema_cfg* ema_cfg,
                               mh_stream s) {
    if (n == 0) return MH_OK;
    MH_REQUIRE(opt && (opt->rule == MH_OPT_ADAM || opt->rule == MH_OPT_ADAMW || opt->rule == MH_OPT_SGD), "mh_optim_groups: no settings, or an unknown rule");
    MH_REQUIRE(dev_state && group_map && group_wd && group_lr, "mh_optim_groups: dev_state, the group map and both group tables are required");
    return optim_launch("mh_optim_groups", p, g, m, v, shadow, n, *opt, 0.f, 1.f, 1.f, group_map, group_wd, group_lr, n_groups, gscale, dev_state,
                        clamp_index, clamp_lo, clamp_hi, counter, counter_add, tick, hole_lo, hole_hi, ema, ema_cfg, s);
}

// torch.optim.Adam without weight decay behind the argument lists that predate mh_optim_cfg: rule Adam, no group map
extern "C" int mh_adam(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, float lr, float b1, float b2,
                       float eps, float bc1, float bc2, float gscale, float* dev_state, int64_t clamp_index, float clamp_lo,
                       float clamp_hi, int64_t* counter, int64_t counter_add, int tick, int64_t hole_lo, int64_t hole_hi, mh_stream s) {
    return optim_launch("mh_adam", p, g, m, v, shadow, n, mh_optim_cfg{MH_OPT_ADAM, b1, b2, eps, 0.f, 0}, lr, bc1, bc2, nullptr, nullptr, nullptr, 0,
                        gscale, dev_state, clamp_index, clamp_lo, clamp_hi, counter, counter_add, tick, hole_lo, hole_hi, nullptr, nullptr, s);
}

extern "C" int mh_adam_ema(float* p, const float* g, float* m, float* v, void* shadow, int64_t n, float lr, float b1, float b2,
                           float eps, float bc1, float bc2, float gscale, float* dev_state, int64_t clamp_index, float clamp_lo,
                           float clamp_hi, int64_t* counter, int64_t counter_add, int tick, int64_t hole_lo, int64_t hole_hi, float* ema,
                           const mh_ema_cfg* cfg, mh_stream s) {
    MH_REQUIRE(ema && ((uintptr_t)ema & 15) == 0, "mh_adam_ema: the EMA buffer must be 16-byte aligned");
    MH_REQUIRE(dev_state, "mh_adam_ema: the EMA decay follows the device step: dev_state is required");
    MH_REQUIRE(cfg && cfg->warmup_gamma > 0.0, "mh_adam_ema: no settings, or warmup_gamma <= 0");
    return optim_launch("mh_adam_ema", p, g, m, v, shadow, n, mh_optim_cfg{MH_OPT_ADAM, b1, b2, eps, 0.f, 0}, lr, bc1, bc2, nullptr, nullptr, nullptr, 0,
                        gscale, dev_state, clamp_index, clamp_lo, clamp_hi, counter, counter_add, tick, hole_lo, hole_hi, ema, cfg, s);
}

// ---- gradient clipping by global L2 norm (timm's clip_grad "norm" mode, train_mirror.py:1206-1230): the factor stays on
// the device (state[4]) and the update multiplies it into its gradient scale — no host round trip, graph-capturable
__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ g, long n, float* __restrict__ acc) {
    __shared__ float red[4];
    float s = 0.f;
    const long n4 = n / 4;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(g)[q];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) { const float v = g[n4 * 4 + threadIdx.x]; s += v * v; }
    s = block_sum256(s, red);
    if (threadIdx.x == 0) atomicAdd(acc, s);
}
__global__ void clip_factor_kernel(const float* acc, float gscale, float max_norm, float* state) {
    const float norm = sqrtf(acc[0]) * gscale;
    state[5] = norm;
    state[4] = max_norm > 0.f ? fminf(1.f, max_norm / (norm + 1e-6f)) : 1.f;
}

extern "C" int mh_grad_clip(const float* g, int64_t n, float grad_scale, float max_norm, float* scratch1, float* dev_state,
                            mh_stream s) {
    MH_REQUIRE(((uintptr_t)g & 15) == 0 && dev_state && scratch1, "mh_grad_clip: bad arguments");
    if (hipMemsetAsync(scratch1, 0, sizeof(float), (hipStream_t)s) != hipSuccess) { mh_set_error("mh_grad_clip: memset failed"); return MH_EHIP; }
    if (n > 0) hipLaunchKernelGGL(sumsq_kernel, dim3((unsigned)min((long)mh_cdiv(mh_cdiv(n, 4), 256), 2048L)), dim3(256), 0, (hipStream_t)s, g, (long)n, scratch1);
    hipLaunchKernelGGL(clip_factor_kernel, dim3(1), dim3(1), 0, (hipStream_t)s, (const float*)scratch1, grad_scale, max_norm, dev_state);
    MH_LAUNCH_CHECK("mh_grad_clip");
    return MH_OK;
}

// ---- scattered tensors into an arena (ArenaOptimizer: gradients that were left outside the gradient arena, load_state_dict): the
// write-side twin of ema_update_many_kernel.  One workgroup per table row {arena offset (elements), source address, n, MH_F32 / MH_BF16}.
// 16-B accesses where source and destination reach a 16-B boundary at the same element (a scalar head up to the source's boundary),
// scalar otherwise, scalar tail; a bf16 source is widened.  HBM-bound: 8 B per f32 element, 6 B per bf16 element.
__global__ __launch_bounds__(256) void gather_many_kernel(float* __restrict__ arena, const long long* __restrict__ tab) {
    const long long* row = tab + 4 * (long)blockIdx.x;
    float* __restrict__ dst = arena + row[0];
    const long n = (long)row[2];
    if (row[3] == MH_BF16) {
        const bf16_t* __restrict__ src = reinterpret_cast<const bf16_t*>(row[1]);
        long h = (long)(((16 - ((uintptr_t)src & 15)) & 15) >> 1);
        if (h > n) h = n;
        if (((uintptr_t)(dst + h) & 15) != 0) h = n;       // the boundaries fall on different elements: all scalar
        for (long i = threadIdx.x; i < h; i += 256) dst[i] = bf2f(src[i]);
        const long n8 = (n - h) >> 3;
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + h);
        const uint4* __restrict__ s8 = reinterpret_cast<const uint4*>(src + h);
        for (long q = threadIdx.x; q < n8; q += 256) {
            const uint4 u = s8[q];                           // 8 bf16: the low half of each dword is the earlier element
            d4[2 * q] = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                                    __uint_as_float(u.y & 0xffff0000u));
            d4[2 * q + 1] = make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u), __uint_as_float(u.w << 16),
                                        __uint_as_float(u.w & 0xffff0000u));
        }
        for (long i = h + n8 * 8 + threadIdx.x; i < n; i += 256) dst[i] = bf2f(src[i]);
    } else {
        const float* __restrict__ src = reinterpret_cast<const float*>(row[1]);
        long h = (long)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
        if (h > n) h = n;
        if (((uintptr_t)(dst + h) & 15) != 0) h = n;
        for (long i = threadIdx.x; i < h; i += 256) dst[i] = src[i];
        const long n4 = (n - h) >> 2;
        float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + h);
        const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + h);
        for (long q = threadIdx.x; q < n4; q += 256) d4[q] = s4[q];
        for (long i = h + n4 * 4 + threadIdx.x; i < n; i += 256) dst[i] = src[i];
    }
}

extern "C" int mh_gather_many(float* arena, const int64_t* table, int nrows, mh_stream s) {
    MH_REQUIRE(nrows >= 0 && (nrows == 0 || (arena && table)), "mh_gather_many: bad arguments");
    MH_REQUIRE(((uintptr_t)arena & 3) == 0 && ((uintptr_t)table & 7) == 0, "mh_gather_many: misaligned arena / table");
    if (nrows == 0) return MH_OK;
    hipLaunchKernelGGL(gather_many_kernel, dim3((unsigned)nrows), dim3(256), 0, (hipStream_t)s, arena, (const long long*)table);
    MH_LAUNCH_CHECK("mh_gather_many");
    return MH_OK;
}
