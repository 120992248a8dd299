// GEMM family: bf16 operands, v_mfma_f32_32x32x16_bf16, f32 accumulate, bf16 or f32 output
#include "gemm_kernel.h"
#include <cstdlib>
bool gemm_try_big_bf16(GemmArgs& a, int akc, int bkc, int dtC, int batch, const GemmTail* tail, bool* tail_added, hipStream_t s);   // gemm_big.hip
bool gemm_launch_bf16(GemmArgs& a, int akc, int bkc, int dtC, int batch, const GemmTail* tail, hipStream_t s) {
    bool tail_added = false;
    if (gemm_try_big_bf16(a, akc, bkc, dtC, batch, tail, &tail_added, s)) return tail_added;
    if (dtC == MH_BF16) launch_l<1, bf16_t, bf16_t, bf16_t>(a, akc, bkc, batch, s);
    else launch_l<1, bf16_t, bf16_t, float>(a, akc, bkc, batch, s);
    return false;
}
