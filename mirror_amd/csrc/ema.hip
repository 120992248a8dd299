// Model EMA over scattered source tensors (timm ModelEmaV3.update, train_mirror.py:1283-1284; train_subtyping.py:1293;
// train_survival.py:1322): the standalone path, for an EMA whose parameters are not one optimizer arena (a plain torch.optim model,
// frozen parameters, floating-point buffers).  The arena path is the optimizer's own pass (optim.hip), which lerps each element behind its update.
#include "common.h"

// One workgroup per table row {ema offset (elements), source address, n}: 16-B accesses where source and destination share their
// alignment (a scalar head up to the source's 16-B boundary), scalar otherwise, scalar tail.  HBM-bound: 12 B per element.
__global__ __launch_bounds__(256) void ema_update_many_kernel(float* __restrict__ ema, const long long* __restrict__ tab, float w_arg,
                                                              const float* __restrict__ state, mh_ema_cfg cfg) {
    __shared__ float ew_s;
    if (threadIdx.x == 0) ew_s = state ? ema_weight(cfg, (double)state[0]) : w_arg;
    __syncthreads();
    const float w = ew_s;
    const long long* row = tab + 3 * (long)blockIdx.x;
    float* __restrict__ dst = ema + row[0];
    const float* __restrict__ src = reinterpret_cast<const float*>(row[1]);
    const long n = (long)row[2];
    long h = (long)(((16 - ((uintptr_t)src & 15)) & 15) >> 2);
    if (h > n) h = n;
    if (((uintptr_t)(dst + h) & 15) != 0) h = n;       // alignments differ: all scalar
    for (long i = threadIdx.x; i < h; i += 256) dst[i] = ema_lerp(dst[i], src[i], w);
    const long n4 = (n - h) >> 2;
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst + h);
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src + h);
    for (long q = threadIdx.x; q < n4; q += 256) {
        float4 e = d4[q];
        const float4 p = s4[q];
        e.x = ema_lerp(e.x, p.x, w);
        e.y = ema_lerp(e.y, p.y, w);
        e.z = ema_lerp(e.z, p.z, w);
        e.w = ema_lerp(e.w, p.w, w);
        d4[q] = e;
    }
    for (long i = h + n4 * 4 + threadIdx.x; i < n; i += 256) dst[i] = ema_lerp(dst[i], src[i], w);
}

extern "C" int mh_ema_update_many(float* ema, const int64_t* table, int nseg, float weight, const float* dev_state, const mh_ema_cfg* cfg,
                                  mh_stream s) {
    MH_REQUIRE(nseg >= 0 && (nseg == 0 || (ema && table)), "mh_ema_update_many: bad arguments");
    MH_REQUIRE(((uintptr_t)ema & 3) == 0 && ((uintptr_t)table & 7) == 0, "mh_ema_update_many: misaligned ema / table");
    MH_REQUIRE(dev_state || (weight >= 0.f && weight <= 1.f), "mh_ema_update_many: weight %g outside [0, 1]", (double)weight);
    MH_REQUIRE(!dev_state || (cfg && cfg->warmup_gamma > 0.0), "mh_ema_update_many: dev_state needs settings with warmup_gamma > 0");
    if (nseg == 0) return MH_OK;
    const mh_ema_cfg c = dev_state ? *cfg : mh_ema_cfg{0.0, 0.0, 1.0, 0.0, 0, 0};
    hipLaunchKernelGGL(ema_update_many_kernel, dim3((unsigned)nseg), dim3(256), 0, (hipStream_t)s, ema, (const long long*)table, weight,
                       dev_state, c);
    MH_LAUNCH_CHECK("mh_ema_update_many");
    return MH_OK;
}
