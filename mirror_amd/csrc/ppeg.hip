// PPEG (models/mirror.py:317-331): proj7(x) + x + proj5(x) + proj3(x) on the sqrt(N) x sqrt(N) token grid.
// The three depthwise convs and the identity are merged on the fly into ONE 7x7 depthwise filter
// (5x5 / 3x3 zero-embedded at the centre, +1 at the centre tap, biases summed): exact, and the tokens
// stay token-major [B, 1+S*S, D] so channel reads are coalesced (no NCHW round trip).
#include "common.h"

__global__ __launch_bounds__(256) void ppeg_merge_kernel(const float* __restrict__ w7, const float* __restrict__ w5,
                                                         const float* __restrict__ w3, const float* __restrict__ b7,
                                                         const float* __restrict__ b5, const float* __restrict__ b3,
                                                         float* __restrict__ merged, float* __restrict__ bsum, int D) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < 49 * D) {
        const int tap = idx / D, c = idx % D;
        const int ky = tap / 7, kx = tap % 7;
        float v = w7[c * 49 + tap];
        if (ky >= 1 && ky <= 5 && kx >= 1 && kx <= 5) v += w5[c * 25 + (ky - 1) * 5 + (kx - 1)];
        if (ky >= 2 && ky <= 4 && kx >= 2 && kx <= 4) v += w3[c * 9 + (ky - 2) * 3 + (kx - 2)];
        if (ky == 3 && kx == 3) v += 1.f;
        merged[idx] = v;
    }
    if (idx < D) bsum[idx] = b7[idx] + b5[idx] + b3[idx];
}

extern "C" int mh_ppeg_merge(const float* w7, const float* w5, const float* w3, const float* b7, const float* b5,
                             const float* b3, float* merged, float* bsum, int D, mh_stream s) {
    hipLaunchKernelGGL(ppeg_merge_kernel, dim3(mh_cdiv(49 * D, 256)), dim3(256), 0, (hipStream_t)s, w7, w5, w3, b7, b5, b3, merged, bsum, D);
    MH_LAUNCH_CHECK("mh_ppeg_merge");
    return MH_OK;
}

// y[b, 1 + yy*S + xx, c] = bsum[c] + sum_tap merged[tap'][c] * x[b, 1 + (yy+ky-3)*S + (xx+kx-3), c]
// flip: tap' = 48 - tap and no bias (adjoint, used for the data gradient). cls row (token 0) is copied.
// Block: 256 channels x PX_T pixels along x for one (b, yy); weights for the thread's channel live in registers.
#define PX_T 8
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void ppeg_kernel(const TX* __restrict__ x, TY* __restrict__ y, const float* __restrict__ merged,
                                                   const float* __restrict__ bsum, int S, int D, int flip) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    const int tiles_x = (S + PX_T - 1) / PX_T;
    const int yy = blockIdx.y / tiles_x, x0 = (blockIdx.y % tiles_x) * PX_T;
    const long b = blockIdx.z;
    const long n = 1 + (long)S * S;
    const TX* xb = x + b * n * D + c;
    TY* yb = y + b * n * D + c;
    if (blockIdx.y == 0) stf(yb, ldf(xb));  // cls token passes through
    float w[49];
#pragma unroll
    for (int t = 0; t < 49; t++) w[t] = merged[(flip ? 48 - t : t) * D + c];
    float acc[PX_T];
    const float bias = flip ? 0.f : bsum[c];
#pragma unroll
    for (int i = 0; i < PX_T; i++) acc[i] = bias;
#pragma unroll
    for (int ky = 0; ky < 7; ky++) {
        const int sy = yy + ky - 3;
        if (sy < 0 || sy >= S) continue;
        const TX* row = xb + (1 + (long)sy * S) * D;
#pragma unroll
        for (int u = 0; u < PX_T + 6; u++) {
            const int sx = x0 - 3 + u;
            const float v = (sx >= 0 && sx < S) ? ldf(row + (long)sx * D) : 0.f;
#pragma unroll
            for (int i = 0; i < PX_T; i++) {
                const int kx = u - i;
                if (kx >= 0 && kx < 7) acc[i] += w[ky * 7 + kx] * v;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PX_T; i++) {
        const int xx = x0 + i;
        if (xx < S) stf(yb + (1 + (long)yy * S + xx) * D, acc[i]);
    }
}

// Column-strip variant: a thread owns one channel and PX_T pixels along x and walks DOWN the grid with a 7-row register
// window (row r lives in slot r mod 7; the walk is unrolled by 7 so every slot index is a compile-time constant).  Each
// input row is loaded once per strip: (PX_T + 6) / PX_T = 1.75 loads per output instead of 12.25.
#define PY_T 16   // grid rows per block
template <typename TX, typename TY>
__global__ __launch_bounds__(256) void ppeg_strip_kernel(const TX* __restrict__ x, TY* __restrict__ y, const float* __restrict__ merged,
                                                         const float* __restrict__ bsum, int S, int D, int flip) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    const int tiles_x = (S + PX_T - 1) / PX_T;
    const int y0 = (blockIdx.y / tiles_x) * PY_T, x0 = (blockIdx.y % tiles_x) * PX_T;
    const long b = blockIdx.z;
    const long n = 1 + (long)S * S;
    const TX* xb = x + b * n * D + c;
    TY* yb = y + b * n * D + c;
    if (blockIdx.y == 0) stf(yb, ldf(xb));  // cls token passes through
    float w[49];
#pragma unroll
    for (int t = 0; t < 49; t++) w[t] = merged[(flip ? 48 - t : t) * D + c];
    const float bias = flip ? 0.f : bsum[c];
    float win[7][PX_T + 6];
    auto load_row = [&](float (&dst)[PX_T + 6], int sy) {
        const bool rok = sy >= 0 && sy < S;
        const TX* row = xb + (1 + (long)(rok ? sy : 0) * S) * D;
#pragma unroll
        for (int u = 0; u < PX_T + 6; u++) {
            const int sx = x0 - 3 + u;
            dst[u] = (rok && sx >= 0 && sx < S) ? ldf(row + (long)sx * D) : 0.f;
        }
    };
    // rows y0-3 .. y0+2 -> slots 4, 5, 6, 0, 1, 2
    load_row(win[4], y0 - 3); load_row(win[5], y0 - 2); load_row(win[6], y0 - 1);
    load_row(win[0], y0); load_row(win[1], y0 + 1); load_row(win[2], y0 + 2);
    for (int yb0 = y0; yb0 < y0 + PY_T && yb0 < S; yb0 += 7) {
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const int yy = yb0 + j;
            if (yy >= y0 + PY_T || yy >= S) break;
            load_row(win[(j + 3) % 7], yy + 3);
            float acc[PX_T];
#pragma unroll
            for (int i = 0; i < PX_T; i++) acc[i] = bias;
#pragma unroll
            for (int ky = 0; ky < 7; ky++)
#pragma unroll
                for (int kx = 0; kx < 7; kx++) {
                    const float wv = w[ky * 7 + kx];
#pragma unroll
                    for (int i = 0; i < PX_T; i++) acc[i] += wv * win[(j + ky + 4) % 7][i + kx];
                }
#pragma unroll
            for (int i = 0; i < PX_T; i++)
                if (x0 + i < S) stf(yb + (1 + (long)yy * S + x0 + i) * D, acc[i]);
        }
    }
}

// Channel-pair form of the strip kernel (f32 in / out, D even): a thread owns TWO adjacent channels, so window, weights and
// accumulators are float2 and every multiply-add is a v_pk_fma_f32 — the depthwise 7 x 7 filter is 49 FMAs per output
// element (1.6 G per launch at c2: 42 us of plain v_fma issue, 21 us packed) and nothing else in the kernel is close.
#define P2_T 4    // pixels along x per thread (the 7 x (P2_T + 6) float2 window is 140 registers)
typedef float pp2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void ppeg_strip2_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ merged,
                                                          const float* __restrict__ bsum, int S, int D, int flip) {
    const int c = 2 * (blockIdx.x * 256 + threadIdx.x);
    if (c >= D) return;
    const int tiles_x = (S + P2_T - 1) / P2_T;
    const int y0 = (blockIdx.y / tiles_x) * PY_T, x0 = (blockIdx.y % tiles_x) * P2_T;
    const long b = blockIdx.z;
    const long n = 1 + (long)S * S;
    const float* xb = x + b * n * D + c;
    float* yb = y + b * n * D + c;
    if (blockIdx.y == 0) *reinterpret_cast<pp2*>(yb) = *reinterpret_cast<const pp2*>(xb);  // cls token passes through
    pp2 w[49];
#pragma unroll
    for (int t = 0; t < 49; t++) w[t] = *reinterpret_cast<const pp2*>(merged + (flip ? 48 - t : t) * D + c);
    const pp2 bias = flip ? (pp2){0.f, 0.f} : *reinterpret_cast<const pp2*>(bsum + c);
    pp2 win[7][P2_T + 6];
    auto load_row = [&](pp2 (&dst)[P2_T + 6], int sy) {
        const bool rok = sy >= 0 && sy < S;
        const float* row = xb + (1 + (long)(rok ? sy : 0) * S) * D;
#pragma unroll
        for (int u = 0; u < P2_T + 6; u++) {
            const int sx = x0 - 3 + u;
            dst[u] = (rok && sx >= 0 && sx < S) ? *reinterpret_cast<const pp2*>(row + (long)sx * D) : (pp2){0.f, 0.f};
        }
    };
    load_row(win[4], y0 - 3); load_row(win[5], y0 - 2); load_row(win[6], y0 - 1);
    load_row(win[0], y0); load_row(win[1], y0 + 1); load_row(win[2], y0 + 2);
    for (int yb0 = y0; yb0 < y0 + PY_T && yb0 < S; yb0 += 7) {
#pragma unroll
        for (int j = 0; j < 7; j++) {
            const int yy = yb0 + j;
            if (yy >= y0 + PY_T || yy >= S) break;
            load_row(win[(j + 3) % 7], yy + 3);
            pp2 acc[P2_T];
#pragma unroll
            for (int i = 0; i < P2_T; i++) acc[i] = bias;
#pragma unroll
            for (int ky = 0; ky < 7; ky++)
#pragma unroll
                for (int kx = 0; kx < 7; kx++) {
                    const pp2 wv = w[ky * 7 + kx];
#pragma unroll
                    for (int i = 0; i < P2_T; i++) acc[i] = __builtin_elementwise_fma(wv, win[(j + ky + 4) % 7][i + kx], acc[i]);
                }
#pragma unroll
            for (int i = 0; i < P2_T; i++)
                if (x0 + i < S) *reinterpret_cast<pp2*>(yb + (1 + (long)yy * S + x0 + i) * D) = acc[i];
        }
    }
}

// Input-stationary form of the channel-pair kernel: instead of a 7-row input window (140 registers, the newest row loaded
// and consumed in the same row step) a thread keeps SEVEN partial output rows (56 registers) and two input rows: input row
// sy adds its seven filter rows into output rows sy - 3 .. sy + 3, output row sy - 3 is then complete and stored, and row
// sy + 1 was requested a whole row step earlier.  Rows outside the strip are skipped by uniform branches.
#ifndef P2_FORM
#define P2_FORM 1     // 1: input-stationary rows (ppeg_rows2_kernel), 0: 7-row input window (ppeg_strip2_kernel)
#endif
#ifndef PR_T
#define PR_T 32       // grid rows per strip of ppeg_rows2_kernel
#endif
__global__ __launch_bounds__(256) void ppeg_rows2_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ merged,
                                                         const float* __restrict__ bsum, int S, int D, int flip, int nb, int pr) {
    // pr = grid rows per strip, chosen by the host so that the launch is whole rounds of resident workgroups (mh_ppeg_fwd)
    // 1-D grid, XCD-aware: workgroup L runs on XCD L % 8 and neighbours in time are L +- 8.  Six of the ten columns a thread loads per
    // row belong to the x-tiles next to its own, so the x-tiles of one (batch, strip) are walked by ONE XCD back to back (their halo
    // columns then come out of that XCD's L2; with x-tiles on consecutive workgroup ids every halo column was fetched from the fabric
    // by two or three XCDs: 73.2 -> 65.5 us alone on the chip at B = 16, S = 64, D = 512; 2 x 64-row strips or 2-pixel tiles: 91 / 68 us).  groups = (batch, strip) pairs, a multiple of 8 or the plain order.
    const int tiles_x = (S + P2_T - 1) / P2_T, strips = (S + pr - 1) / pr;
    const int per_cb = tiles_x * strips * nb;
    const int cb = blockIdx.x / per_cb, L = blockIdx.x % per_cb;
    const int c = 2 * (cb * 256 + threadIdx.x);
    if (c >= D) return;
    int xt, grp;
    if ((strips * nb) % 8 == 0) { const int q = L >> 3; xt = q % tiles_x; grp = (q / tiles_x) * 8 + (L & 7); }
    else { xt = L % tiles_x; grp = L / tiles_x; }
    const int y0 = (grp % strips) * pr, x0 = xt * P2_T;
    const int rows = min(pr, S - y0);
    const long b = grp / strips;
    const bool first = (y0 == 0 && x0 == 0);
    const long n = 1 + (long)S * S;
    const float* xb = x + b * n * D + c;
    float* yb = y + b * n * D + c;
    if (first) *reinterpret_cast<pp2*>(yb) = *reinterpret_cast<const pp2*>(xb);  // cls token passes through
    pp2 w[49];
#pragma unroll
    for (int t = 0; t < 49; t++) w[t] = *reinterpret_cast<const pp2*>(merged + (flip ? 48 - t : t) * D + c);
    const pp2 bias = flip ? (pp2){0.f, 0.f} : *reinterpret_cast<const pp2*>(bsum + c);
    pp2 in[2][P2_T + 6];
    auto load_row = [&](pp2 (&dst)[P2_T + 6], int sy) {
        const bool rok = sy >= 0 && sy < S;
        const float* row = xb + (1 + (long)(rok ? sy : 0) * S) * D;
#pragma unroll
        for (int u = 0; u < P2_T + 6; u++) {
            const int sx = x0 - 3 + u;
            dst[u] = (rok && sx >= 0 && sx < S) ? *reinterpret_cast<const pp2*>(row + (long)sx * D) : (pp2){0.f, 0.f};
        }
    };
    pp2 acc[7][P2_T];          // output row y0 + o lives in slot o % 7
#pragma unroll
    for (int i = 0; i < P2_T; i++) acc[0][i] = bias;
    const int steps = rows + 6;   // input rows y0 - 3 .. y0 + rows + 2
    load_row(in[0], y0 - 3);
    for (int kb = 0; kb < steps; kb += 14) {
#pragma unroll
        for (int j = 0; j < 14; j++) {
            const int k = kb + j;
            if (k >= steps) break;
            const int sy = y0 - 3 + k;
            if (k + 1 < steps) load_row(in[(j + 1) & 1], sy + 1);
            if (sy >= 0 && sy < S) {      // a row of zero padding adds nothing
#pragma unroll
                for (int ky = 0; ky < 7; ky++) {
                    const int o = k - ky;
                    if (o >= 0 && o < rows) {
#pragma unroll
                        for (int kx = 0; kx < 7; kx++) {
                            const pp2 wv = w[ky * 7 + kx];
#pragma unroll
                            for (int i = 0; i < P2_T; i++)
                                acc[(j - ky + 14) % 7][i] = __builtin_elementwise_fma(wv, in[j & 1][i + kx], acc[(j - ky + 14) % 7][i]);
                        }
                    }
                }
            }
            const int od = k - 6;         // this output row has seen all seven input rows
            if (od >= 0) {
#pragma unroll
                for (int i = 0; i < P2_T; i++)
                    if (x0 + i < S) *reinterpret_cast<pp2*>(yb + (1 + (long)(y0 + od) * S + x0 + i) * D) = acc[(j + 1) % 7][i];
            }
#pragma unroll
            for (int i = 0; i < P2_T; i++) acc[(j + 1) % 7][i] = bias;      // slot of output row k + 1
        }
    }
}

extern "C" int mh_ppeg_fwd(const void* x, void* y, const float* merged, const float* bsum, int B, int S, int D, int flip,
                           int dt_x, int dt_y, mh_stream s) {
    mh_note_form("ppeg_fwd:none");
    MH_REQUIRE(S >= 1 && D >= 1, "mh_ppeg_fwd: bad shape S=%d D=%d", S, D);
    MH_REQUIRE((dt_x == MH_F32 || dt_x == MH_BF16) && (dt_y == MH_F32 || dt_y == MH_BF16), "mh_ppeg_fwd: unknown dtype code (dt_x=%d dt_y=%d)", dt_x, dt_y);
    if (B == 0) return MH_OK;
    if (dt_x == MH_F32 && dt_y == MH_F32 && D % 2 == 0 && (((uintptr_t)x | (uintptr_t)y | (uintptr_t)merged | (uintptr_t)bsum) & 7) == 0) {
        mh_note_form("ppeg_fwd:pair");
#if P2_FORM
        // rows per strip: two workgroups of ~200 VGPRs fit a CU, so the launch runs in rounds of 512; fewest (rounds x row steps of a
        // strip, 6 of them halo), PR_T rows when that is as good (c2: 2 strips of 32 rows = 512 workgroups; config 4's 91 x 91 grid at B = 8:
        // 3 strips were 552 workgroups = a second round for 40 of them)
        int pr = PR_T;
        {
            const long per = (long)mh_cdiv(D / 2, 256) * mh_cdiv(S, P2_T) * B;
            long best = -1;
            for (int st = 1; st <= mh_cdiv(S, 8); st++) {
                const int rows = mh_cdiv(S, st);
                if (rows > 64) continue;
                const long cost = mh_cdiv(per * mh_cdiv(S, rows), 512) * (rows + 6);
                if (best < 0 || cost < best || (cost == best && rows == PR_T)) { best = cost; pr = rows; }
            }
#ifdef MH_EXP
            if (const char* e = getenv("MH_PPEG_PR")) pr = atoi(e);      // tools/exp/ppeg_rows_per_strip.sh
#endif
        }
        dim3 g2(mh_cdiv(D / 2, 256) * mh_cdiv(S, pr) * mh_cdiv(S, P2_T) * B);
        hipLaunchKernelGGL(ppeg_rows2_kernel, g2, dim3(256), 0, (hipStream_t)s, (const float*)x, (float*)y, merged, bsum, S, D, flip, B, pr);
#else
        dim3 g2(mh_cdiv(D / 2, 256), mh_cdiv(S, PY_T) * mh_cdiv(S, P2_T), B);
        hipLaunchKernelGGL(ppeg_strip2_kernel, g2, dim3(256), 0, (hipStream_t)s, (const float*)x, (float*)y, merged, bsum, S, D, flip);
#endif
        MH_LAUNCH_CHECK("mh_ppeg_fwd");
        return MH_OK;
    }
    // PY_T = 16 rows per strip is not a multiple of the unroll (7): the walk is 7 + 7 + 2 rows with the window slots
    // following the row index, so a strip must start at a slot-0 row -> strips are re-based every PY_T rows
    dim3 grid(mh_cdiv(D, 256), mh_cdiv(S, PY_T) * mh_cdiv(S, PX_T), B);
    mh_note_form("ppeg_fwd:strip");
#define PP(TX, TY) hipLaunchKernelGGL((ppeg_strip_kernel<TX, TY>), grid, dim3(256), 0, (hipStream_t)s, (const TX*)x, (TY*)y, merged, bsum, S, D, flip)
    if (dt_x == MH_F32 && dt_y == MH_F32) PP(float, float);
    else if (dt_x == MH_BF16 && dt_y == MH_BF16) PP(bf16_t, bf16_t);
    else if (dt_x == MH_F32 && dt_y == MH_BF16) PP(float, bf16_t);
    else PP(bf16_t, float);
#undef PP
    MH_LAUNCH_CHECK("mh_ppeg_fwd");
    return MH_OK;
}

// dmerged[tap][c] += sum_{b,yy,xx} dout[b,yy,xx,c] * x[b,yy+ky-3,xx+kx-3,c]; dbsum[c] += sum dout.
// Block = 64 channels x 4 grid rows (one wave per row, lanes = channels: 256-B coalesced loads).  Each thread
// sweeps its row with a 7x7 register window of x (column X lives in slot X mod 7; the sweep is unrolled by 7 so
// every slot index is a compile-time constant): 7 loads + 49 FMAs per pixel.  The 4 rows are reduced through
// LDS, then one f32 atomic per (tap, channel) per block.
#define WG_ROWS 4
template <typename TX, typename TO>
__global__ __launch_bounds__(256) void ppeg_wgrad_kernel(const TX* __restrict__ x, const TO* __restrict__ dout,
                                                         float* __restrict__ dmerged, float* __restrict__ dbsum, int S, int D) {
    __shared__ float red[4][50][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int yy = blockIdx.y * WG_ROWS + slice;
    const long b = blockIdx.z;
    const long n = 1 + (long)S * S;
    const bool live = (c < D) && (yy < S);
    const TX* xb = x + b * n * D + (live ? c : 0);
    const TO* db = dout + b * n * D + (live ? c : 0);
    float acc[49], win[7][7];
#pragma unroll
    for (int t = 0; t < 49; t++) acc[t] = 0.f;
    float bacc = 0.f;
    if (live) {
        bool rowok[7];
#pragma unroll
        for (int ky = 0; ky < 7; ky++) {
            const int sy = yy + ky - 3;
            rowok[ky] = (sy >= 0 && sy < S);
#pragma unroll
            for (int sl = 0; sl < 7; sl++)
                win[ky][sl] = (sl < 3 && sl < S && rowok[ky]) ? ldf(xb + (1 + (long)sy * S + sl) * D) : 0.f;
        }
        for (int xx0 = 0; xx0 < S; xx0 += 7) {
#pragma unroll
            for (int u = 0; u < 7; u++) {
                const int xx = xx0 + u;
                const int xn = xx + 3;  // column entering the window
#pragma unroll
                for (int ky = 0; ky < 7; ky++)
                    win[ky][(u + 3) % 7] = (xn < S && rowok[ky]) ? ldf(xb + (1 + (long)(yy + ky - 3) * S + xn) * D) : 0.f;
                const float g = (xx < S) ? ldf(db + (1 + (long)yy * S + xx) * D) : 0.f;
                bacc += g;
#pragma unroll
                for (int ky = 0; ky < 7; ky++)
#pragma unroll
                    for (int kx = 0; kx < 7; kx++) acc[ky * 7 + kx] += g * win[ky][(u + kx + 4) % 7];
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 49; t++) red[slice][t][lane] = acc[t];
    red[slice][49][lane] = bacc;
    __syncthreads();
    if (c < D) {
        for (int t = slice; t < 50; t += 4) {
            const float v = red[0][t][lane] + red[1][t][lane] + red[2][t][lane] + red[3][t][lane];
            if (t < 49) atomicAdd(dmerged + t * D + c, v);
            else atomicAdd(dbsum + c, v);
        }
    }
}

// Column-strip weight gradient: a thread owns one channel and PX_T pixels along x, walks down PW_ROWS grid rows with a
// register window of input rows: 8 + 14 loads feed 49 x 8 FMAs (the row-sweep kernel needs 64).
// The window is a ring of EIGHT rows and the gradient row is double-buffered: row yy + 4 and the gradients of row yy + 1
// are requested while row yy is accumulated, so no FMA waits for a load issued in its own iteration (with the 7-row
// window every row step began with a full memory latency, at two waves per SIMD: 173 us for 268 MB).
// (A channel-pair v_pk_fma form like ppeg_strip2_kernel was slower here: 98 accumulator + 140 window registers leave one
// wave per SIMD and nothing to hide the row loads behind.)
#ifndef PW_ROWS
#define PW_ROWS 64   // multiple of 8 (the ring is unrolled by its length)
#endif
#ifndef PW_X
#define PW_X 4       // pixels along x per thread
#endif
#ifndef PW_RED
#define PW_RED 1     // 1: workgroup = 64 channels x 4 strips with an LDS reduction, 0: 256 channels x 1 strip
#endif
template <typename TX, typename TO>
__global__ __launch_bounds__(256) void ppeg_wgrad_strip_kernel(const TX* __restrict__ x, const TO* __restrict__ dout,
                                                               float* __restrict__ dmerged, float* __restrict__ dbsum, int S, int D, int pr) {
    // pr = grid rows per strip (<= PW_ROWS): the host cuts the S rows into EQUAL strips (S = 91: 46 + 45 rows, not 64 + 27 — the long
    // strips set the launch's time)
    const int tiles_x = (S + PW_X - 1) / PW_X;
#if PW_RED
    // a workgroup = 64 channels x 4 strips (one per wave); the four partial filters are summed through LDS, so a
    // workgroup issues 50 x 64 atomics instead of 50 x 256
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: addresses stay scalar
    const int c = blockIdx.x * 64 + lane;
    const int strip = blockIdx.y * 4 + wave;
    const bool live = c < D && strip < tiles_x * ((S + pr - 1) / pr);
#else
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= D) return;
    const int strip = blockIdx.y;
    const bool live = true;
#endif
    const int y0 = (strip / tiles_x) * pr, x0 = (strip % tiles_x) * PW_X;
    const int y1 = live ? min(y0 + pr, S) : y0;      // one past the last row of this strip
    const long b = blockIdx.z;
    const long n = 1 + (long)S * S;
    const TX* xb = x + b * n * D + (live ? c : 0);
    const TO* gb = dout + b * n * D + (live ? c : 0);
    float acc[49];
#pragma unroll
    for (int t = 0; t < 49; t++) acc[t] = 0.f;
    float bacc = 0.f;
    float win[8][PW_X + 6];      // row r of the grid lives in slot (r - y0 + 3) & 7
    float g[2][PW_X];
    auto load_row = [&](float (&dst)[PW_X + 6], int sy) {
        const bool rok = sy >= 0 && sy < S;
        const TX* row = xb + (1 + (long)(rok ? sy : 0) * S) * D;
#pragma unroll
        for (int u = 0; u < PW_X + 6; u++) {
            const int sx = x0 - 3 + u;
            dst[u] = (rok && sx >= 0 && sx < S) ? ldf(row + (long)sx * D) : 0.f;
        }
    };
    auto load_g = [&](float (&dst)[PW_X], int yy) {
        const bool rok = yy < y1;
        const TO* row = gb + (1 + (long)(rok ? yy : 0) * S) * D;
#pragma unroll
        for (int i = 0; i < PW_X; i++) dst[i] = (rok && x0 + i < S) ? ldf(row + (long)(x0 + i) * D) : 0.f;
    };
    if (live) {
#pragma unroll
        for (int r = 0; r < 7; r++) load_row(win[r], y0 - 3 + r);
        load_g(g[0], y0);
    }
    for (int yb0 = y0; yb0 < y1; yb0 += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int yy = yb0 + j;
            if (yy >= y1) break;
            if (yy + 1 < y1) {                      // the next row step exists: its newest window row and its gradients
                load_row(win[(j + 7) & 7], yy + 4);
                load_g(g[(j + 1) & 1], yy + 1);
            }
#pragma unroll
            for (int i = 0; i < PW_X; i++) bacc += g[j & 1][i];
#pragma unroll
            for (int ky = 0; ky < 7; ky++)
#pragma unroll
                for (int kx = 0; kx < 7; kx++) {
                    float a = acc[ky * 7 + kx];
#pragma unroll
                    for (int i = 0; i < PW_X; i++) a += g[j & 1][i] * win[(j + ky) & 7][i + kx];
                    acc[ky * 7 + kx] = a;
                }
        }
    }
#if PW_RED
    __shared__ float red[3][50][64];
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < 49; t++) red[wave - 1][t][lane] = acc[t];
        red[wave - 1][49][lane] = bacc;
    }
    __syncthreads();
    if (wave == 0 && c < D) {
#pragma unroll
        for (int t = 0; t < 49; t++) atomicAdd(dmerged + t * D + c, acc[t] + red[0][t][lane] + red[1][t][lane] + red[2][t][lane]);
        atomicAdd(dbsum + c, bacc + red[0][49][lane] + red[1][49][lane] + red[2][49][lane]);
    }
#else
#pragma unroll
    for (int t = 0; t < 49; t++) atomicAdd(dmerged + t * D + c, acc[t]);
    atomicAdd(dbsum + c, bacc);
#endif
}

extern "C" int mh_ppeg_wgrad(const void* x, const void* dout, float* dmerged, float* dbsum, int B, int S, int D, int dt_x,
                             int dt_o, mh_stream s) {
    mh_note_form("ppeg_wgrad:none");
    MH_REQUIRE((dt_x == MH_F32 || dt_x == MH_BF16) && (dt_o == MH_F32 || dt_o == MH_BF16), "mh_ppeg_wgrad: unknown dtype code (dt_x=%d dt_o=%d)", dt_x, dt_o);
    if (B == 0) return MH_OK;
    const int pr = mh_cdiv(S, mh_cdiv(S, PW_ROWS));       // equal strips of at most PW_ROWS rows
#if PW_RED
    dim3 grid(mh_cdiv(D, 64), mh_cdiv(mh_cdiv(S, pr) * mh_cdiv(S, PW_X), 4), B);
#else
    dim3 grid(mh_cdiv(D, 256), mh_cdiv(S, pr) * mh_cdiv(S, PW_X), B);
#endif
    mh_note_form("ppeg_wgrad:strip");
#define PW(TX, TO) hipLaunchKernelGGL((ppeg_wgrad_strip_kernel<TX, TO>), grid, dim3(256), 0, (hipStream_t)s, (const TX*)x, (const TO*)dout, dmerged, dbsum, S, D, pr)
    if (dt_x == MH_F32 && dt_o == MH_F32) PW(float, float);
    else if (dt_x == MH_BF16 && dt_o == MH_BF16) PW(bf16_t, bf16_t);
    else if (dt_x == MH_F32 && dt_o == MH_BF16) PW(float, bf16_t);
    else PW(bf16_t, float);
#undef PW
    MH_LAUNCH_CHECK("mh_ppeg_wgrad");
    return MH_OK;
}

// ------------------------------------------------------------------ the whole backward in one walk over the grid
// Data gradient (the adjoint filter over dy), filter gradient (dy x x), bias gradient (sum of dy) and — when the tensor PPEG read came
// out of a Dropout ([3P] to_out of layer 1) — that Dropout's backward (masked, scaled bf16 copy of dx and its column sums), from ONE
// read of dy and x.  The data gradient is ppeg_rows2_kernel's input-stationary form: dy row sy (with its 3-column halo) adds its seven
// filter rows into the seven partial dx rows sy - 3 .. sy + 3.  The same ten dy columns serve the filter gradient: x row r pairs with dy
// rows r - 3 .. r + 3, so a ring of seven x rows (the thread's 4 centre columns only, kept in LDS) meets every dy row as it passes,
//     dmerged[ky][kx] += dy[sy][cx - kx + 3] * x[sy + ky - 3][cx]   over the strip's own x pixels (cx = the thread's columns).
// A thread owns ONE channel: the channel-pair form would hold 2 x (49 taps + 49 weights + 28 partial rows + 28 ring + 20 dy) = 348
// registers, one wave per SIMD with spills.  The multiply-adds are still v_pk_fma_f32, paired along x (data gradient: two pixels) and
// along kx (filter gradient: two taps), 182 packed + 28 plain per row step instead of 392.
// Workgroup = 64 channels (lanes) x 4 ADJACENT x-tiles of one (batch, strip) (waves): their halo columns are each other's centre
// columns.  The four partial filters are summed through LDS and leave as one atomic per (tap, channel) and workgroup.
// Dropout: one drop16_keep8 block covers 8 channels, so the 4 pixels x 64 channels a wave writes per row step are 32 blocks.  Every
// second row step lane l draws the block of (row = l / 32, pixel = l / 8 % 4, channel group = l % 8) for the NEXT TWO dx rows, and
// the lanes fetch their bit with one cross-lane read per pixel: 1/16 draw per element instead of 1.
#define PB_X 4
// acc += a[ha] * b (a[ha] to both halves) and acc += (a.y, a.x) * b[hb]: the compiler builds every splat and swap of a v_pk_fma_f32 operand
// with moves (one or two per multiply-add); the instruction's op_sel bits select the halves for nothing.  ha / hb are constants after unrolling.
__device__ __forceinline__ void pb_fma_splat_a(pp2& acc, pp2 a, int ha, pp2 b) {
    if (ha) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[1,1,1]" : "+v"(acc) : "v"(a), "v"(b));
    else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(a), "v"(b));
}
__device__ __forceinline__ void pb_fma_swap_a_splat_b(pp2& acc, pp2 a, pp2 b, int hb) {
    if (hb) asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[0,1,1]" : "+v"(acc) : "v"(a), "v"(b));
    else asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,0,0] op_sel_hi:[0,0,1]" : "+v"(acc) : "v"(a), "v"(b));
}
template <int N> struct pb_ic { static constexpr int value = N; };
template <bool DROP>
__global__ __launch_bounds__(256, 2) void ppeg_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ merged,
                                                          float* __restrict__ dx, float* __restrict__ dmerged, float* __restrict__ dbsum,
                                                          int S, int D, int nb, int pr, bf16_t* __restrict__ drop_out,
                                                          float* __restrict__ drop_db, float p, uint64_t seed, uint64_t offset,
                                                          const uint64_t* __restrict__ dev_base) {
    // the x ring lives in LDS (each thread reads back only what it wrote: no barrier), 28 registers that two waves per SIMD do not have;
    // the reduction at the end reuses the space
    __shared__ __attribute__((aligned(16))) float smem[3 * 51 * 64 > 7 * 256 * PB_X ? 3 * 51 * 64 : 7 * 256 * PB_X];
    f4_t* ring = reinterpret_cast<f4_t*>(smem) + threadIdx.x;       // slot s at ring[s * 256]
    float (*red)[51][64] = reinterpret_cast<float (*)[51][64]>(smem);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tiles_x = (S + PB_X - 1) / PB_X, xgroups = (tiles_x + 3) / 4, strips = (S + pr - 1) / pr, cblocks = (D + 63) / 64;
    // XCD-aware order as in ppeg_rows2_kernel: the x-groups of one (batch, strip, channel block) run back to back on ONE XCD
    const int groups = cblocks * strips * nb;
    const int L = blockIdx.x;
    int xg, grp;
    if (groups % 8 == 0) { const int q = L >> 3; xg = q % xgroups; grp = (q / xgroups) * 8 + (L & 7); }
    else { xg = L % xgroups; grp = L / xgroups; }
    const int cb = grp % cblocks, sb = grp / cblocks;
    const int c = cb * 64 + lane;
    const bool cok = c < D;                  // dead lanes walk along on channel 0 (they serve the cross-lane reads) and store nothing
    const int xt = xg * 4 + wave;
    const bool wlive = xt < tiles_x;         // wave-uniform
    const int y0 = (sb % strips) * pr, x0 = xt * PB_X;
    const int rows = min(pr, S - y0);
    const long b = sb / strips;
    const long n = 1 + (long)S * S;
    const long boff = b * n * D + cb * 64;     // workgroup-uniform: row addresses stay scalar, the lane adds cl
    const int cl = cok ? lane : 0;
    uint32_t thr = 0;
    float scale = 1.f;
    uint64_t blk0 = 0;
    const int D8 = D >> 3;
    if (DROP) {
        if (dev_base) offset += *dev_base & ~7ull;
        thr = drop16_thr(p);
        scale = drop16_scale(thr);
        blk0 = (offset >> 3) + (uint64_t)(b * n) * (uint64_t)D8 + (uint64_t)(cb * 8);      // block of (row 0 of this batch, channel cb * 64)
    }
    pp2 wp[25];                              // the adjoint filter: wp[u] = taps (2u, 2u + 1) of merged read backwards
    float dm6[7];
    pp2 dmp[7][3];                           // dmp[ky][q] = taps (ky, 2q) and (ky, 2q + 1), dm6[ky] = tap (ky, 6)
#pragma unroll
    for (int t = 0; t < 50; t++) wp[t >> 1][t & 1] = t < 49 ? merged[(48 - t) * D + cb * 64 + cl] : 0.f;
#pragma unroll
    for (int ky = 0; ky < 7; ky++) { dm6[ky] = 0.f; dmp[ky][0] = dmp[ky][1] = dmp[ky][2] = (pp2){0.f, 0.f}; }
    float bacc = 0.f, dsum = 0.f;
    if (wlive) {
        const float* xb = x + boff;
        const float* gb = dy + boff;
        float* ob = dx + boff;
        bf16_t* qb = DROP ? drop_out + boff : nullptr;
        if (y0 == 0 && x0 == 0) {            // cls token passes through (and through the Dropout)
            const float v = gb[cl];
            if (cok) ob[cl] = v;
            if (DROP) {
                const uint32_t keep = drop16_keep8(blk0 + (uint64_t)(lane >> 3), seed, thr);
                const bf16_t o = f2bf((keep >> (lane & 7)) & 1u ? __fmul_rn(v, scale) : 0.f);
                if (cok) { qb[cl] = o; dsum += bf2f(o); }
            }
        }
        // rows in flight: TWO row steps ahead (one step of multiply-adds is shorter than the memory latency under load).  The loads are
        // unconditional, from addresses clamped into the grid — a load under a branch costs the exact vmcnt bookkeeping, and with it the
        // second row in flight; the zero padding is applied when a row is taken into ce / co and the ring
        float nb[2][PB_X + 6];
        f4_t xq[2];
        pp2 ce[5], co[4], acc[7][2];         // dy columns (2u, 2u + 1) and (2u + 1, 2u + 2) of the row in hand; dx pixels (2h, 2h + 1)
        auto load_dy = [&](float (&dst)[PB_X + 6], int sy) {      // a row outside the grid is never used (the step skips its products)
            const float* row = gb + (1 + (long)min(max(sy, 0), S - 1) * S) * D + cl;
#pragma unroll
            for (int u = 0; u < PB_X + 6; u++) dst[u] = row[(long)min(max(x0 - 3 + u, 0), S - 1) * D];
        };
        auto load_x = [&](f4_t& dst, int r) {      // row r of this strip (rows past its end are never used)
            const float* row = xb + (1 + (long)(y0 + min(r, rows - 1)) * S) * D + cl;
#pragma unroll
            for (int i = 0; i < PB_X; i++) dst[i] = row[(long)min(x0 + i, S - 1) * D];
        };
        auto col = [&](const float (&src)[PB_X + 6], int u) { return (x0 - 3 + u >= 0 && x0 - 3 + u < S) ? src[u] : 0.f; };
#pragma unroll
        for (int r = 0; r < 7; r++)
#pragma unroll
            for (int h = 0; h < 2; h++) acc[r][h] = (pp2){0.f, 0.f};
        uint32_t keep2 = 0;
        const int steps = rows + 6;          // dy rows y0 - 3 .. y0 + rows + 2
        load_dy(nb[0], y0 - 3);
        load_x(xq[0], 0);
        load_dy(nb[1], y0 - 2);              // (steps >= 7)
        load_x(xq[1], 1);
        for (int kb = 0; kb < steps; kb += 14) {
            // 14 row steps spelled out (the seven slots of the rings x the two rows in flight): `#pragma unroll` gives up on a body this long,
            // and a rolled loop would index the register arrays at run time
            auto step = [&](auto jc) __attribute__((always_inline)) -> bool {
                constexpr int j = decltype(jc)::value;
                const int k = kb + j;
                if (k >= steps) return false;
                const int sy = y0 - 3 + k;
#pragma unroll
                for (int u = 0; u < 5; u++) ce[u] = (pp2){col(nb[j & 1], 2 * u), col(nb[j & 1], 2 * u + 1)};
#pragma unroll
                for (int u = 0; u < 4; u++) co[u] = (pp2){col(nb[j & 1], 2 * u + 1), col(nb[j & 1], 2 * u + 2)};
                {
                    f4_t xm;
#pragma unroll
                    for (int i = 0; i < PB_X; i++) xm[i] = x0 + i < S ? xq[j & 1][i] : 0.f;
                    ring[(j % 7) * 256] = xm;          // x row k of the strip lives in slot k % 7
                }
                load_dy(nb[j & 1], sy + 2);  // two row steps ahead; unconditional (the last two steps of a strip fetch clamped rows again for
                load_x(xq[j & 1], k + 2);    // nothing): a load that may not have been issued cannot be counted past by s_waitcnt
                if (sy >= 0 && sy < S) {     // a row of zero padding adds nothing
                    if (k >= 3 && k < rows + 3) bacc += (co[1][0] + co[1][1]) + (co[2][0] + co[2][1]);
#pragma unroll
                    for (int ky = 0; ky < 7; ky++) {
                        const int o = k - ky;                          // dx row (of the strip) this filter row lands in
                        if (o >= 0 && o < rows) {
#pragma unroll
                            for (int kx = 0; kx < 7; kx++)
#pragma unroll
                                for (int h = 0; h < 2; h++)      // pixels (2h, 2h + 1) read columns (2h + kx, 2h + kx + 1)
                                    pb_fma_splat_a(acc[(j - ky + 14) % 7][h], wp[(ky * 7 + kx) >> 1], (ky * 7 + kx) & 1, (kx & 1) ? co[h + kx / 2] : ce[h + kx / 2]);
                        }
                    }
#pragma unroll
                    for (int ky = 0; ky < 7; ky++) {
                        const int r = k + ky - 6;                      // x row (of the strip) this dy row meets at filter row ky
                        if (r >= 0 && r < rows) {
                            const f4_t xv = ring[((j + ky + 1) % 7) * 256];
#pragma unroll
                            for (int i = 0; i < PB_X; i++) {
                                const pp2 xp = (i & 2) ? (pp2){xv[2], xv[3]} : (pp2){xv[0], xv[1]};
#pragma unroll
                                for (int q = 0; q < 3; q++) {    // taps (2q, 2q + 1) read columns (i + 6 - 2q, i + 5 - 2q): a pair, swapped
                                    const int a = i + 5 - 2 * q;
                                    pb_fma_swap_a_splat_b(dmp[ky][q], (a & 1) ? co[a / 2] : ce[a / 2], xp, i & 1);
                                }
                                asm("v_fmac_f32 %0, %1, %2" : "+v"(dm6[ky]) : "v"((i & 1) ? ce[i / 2][1] : ce[i / 2][0]), "v"(xv[i]));
                            }
                        }
                    }
                }
                const int od = k - 6;        // this dx row has seen all seven dy rows
                if (od >= 0) {
                    const long prow = 1 + (long)(y0 + od) * S + x0;
                    if (DROP) {
                        if ((k & 1) == 0) {  // od = 0 falls on an even step: rows od (lanes 0..31) and od + 1 (lanes 32..63)
                            const uint64_t r = (uint64_t)(prow + (long)(lane >> 5) * S + ((lane >> 3) & 3));
                            keep2 = drop16_keep8(blk0 + r * (uint64_t)D8 + (uint64_t)(lane & 7), seed, thr);
                        }
                        uint32_t kp[PB_X];
#pragma unroll
                        for (int i = 0; i < PB_X; i++) kp[i] = (uint32_t)__shfl((int)keep2, ((k & 1) << 5) + i * 8 + (lane >> 3));
#pragma unroll
                        for (int i = 0; i < PB_X; i++) {
                            const float v = acc[(j + 1) % 7][i >> 1][i & 1];
                            const bf16_t o = f2bf((kp[i] >> (lane & 7)) & 1u ? __fmul_rn(v, scale) : 0.f);     // two roundings, as mh_dropout_lite
                            if (cok && x0 + i < S) {
                                ob[(prow + i) * D + cl] = v;
                                qb[(prow + i) * D + cl] = o;
                                dsum += bf2f(o);                        // the sums are those of the ROUNDED values
                            }
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < PB_X; i++)
                            if (cok && x0 + i < S) ob[(prow + i) * D + cl] = acc[(j + 1) % 7][i >> 1][i & 1];
                    }
                }
#pragma unroll
                for (int h = 0; h < 2; h++) acc[(j + 1) % 7][h] = (pp2){0.f, 0.f};      // slot of dx row k + 1
                return true;
            };
            if (!(step(pb_ic<0>{}) && step(pb_ic<1>{}) && step(pb_ic<2>{}) && step(pb_ic<3>{}) && step(pb_ic<4>{}) && step(pb_ic<5>{}) &&
                  step(pb_ic<6>{}) && step(pb_ic<7>{}) && step(pb_ic<8>{}) && step(pb_ic<9>{}) && step(pb_ic<10>{}) && step(pb_ic<11>{}) &&
                  step(pb_ic<12>{}) && step(pb_ic<13>{})))
                break;
        }
    }
    auto tap = [&](int t) { return t % 7 == 6 ? dm6[t / 7] : dmp[t / 7][(t % 7) >> 1][t % 7 & 1]; };
    __syncthreads();                         // the ring is done with
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < 49; t++) red[wave - 1][t][lane] = tap(t);
        red[wave - 1][49][lane] = bacc;
        red[wave - 1][50][lane] = dsum;
    }
    __syncthreads();
    if (wave == 0 && cok) {
#pragma unroll
        for (int t = 0; t < 49; t++) atomicAdd(dmerged + t * D + c, tap(t) + red[0][t][lane] + red[1][t][lane] + red[2][t][lane]);
        atomicAdd(dbsum + c, bacc + red[0][49][lane] + red[1][49][lane] + red[2][49][lane]);
        if (DROP) {
            const float t = dsum + red[0][50][lane] + red[1][50][lane] + red[2][50][lane];
            if (t != 0.f) atomicAdd(drop_db + c, t);
        }
    }
}

extern "C" int mh_ppeg_bwd(const float* x, const float* dy, const float* merged, float* dx, float* dmerged, float* dbsum, int B, int S,
                           int D, void* drop_out, float* drop_db, float p, uint64_t seed, uint64_t offset, const uint64_t* dev_base,
                           mh_stream s) {
    mh_note_form("ppeg_bwd:none");
    MH_REQUIRE(S >= 1 && D >= 1, "mh_ppeg_bwd: bad shape S=%d D=%d", S, D);
    MH_REQUIRE(x && dy && merged && dx && dmerged && dbsum, "mh_ppeg_bwd: null pointer");
    MH_REQUIRE(!drop_out || (drop_db && D % 8 == 0 && (offset & 7) == 0 && p >= 0.f && p < 1.f && ((uintptr_t)drop_out & 1) == 0),
               "mh_ppeg_bwd: the Dropout site needs D %% 8 == 0 (D=%d), offset %% 8 == 0, 0 <= p < 1 and a bias-gradient destination", D);
    if (B == 0) return MH_OK;
    // rows per strip: two workgroups fit a CU, so the launch runs in rounds of 512; equal strips of at most 64 rows, the count with the
    // fewest (rounds x row steps of a strip, 6 of them halo); the longer strips on a tie (fewer atomics)
    int pr = S;
    {
        const long per = (long)mh_cdiv(D, 64) * mh_cdiv(mh_cdiv(S, PB_X), 4) * B;
        long best = -1;
        for (int st = 1; st <= mh_cdiv(S, 8); st++) {
            const int rows = mh_cdiv(S, st);
            if (rows > 64) continue;
            const long cost = (long)mh_cdiv(per * mh_cdiv(S, rows), 512) * (rows + 6);
            if (best < 0 || cost < best) { best = cost; pr = rows; }
        }
    }
    const dim3 grid(mh_cdiv(D, 64) * mh_cdiv(S, pr) * mh_cdiv(mh_cdiv(S, PB_X), 4) * B);
    mh_note_form(drop_out ? "ppeg_bwd:one,drop" : "ppeg_bwd:one");
    if (drop_out)
        hipLaunchKernelGGL(ppeg_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)s, x, dy, merged, dx, dmerged, dbsum, S, D, B, pr,
                           (bf16_t*)drop_out, drop_db, p, seed, offset, dev_base);
    else
        hipLaunchKernelGGL(ppeg_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)s, x, dy, merged, dx, dmerged, dbsum, S, D, B, pr,
                           (bf16_t*)nullptr, (float*)nullptr, 0.f, (uint64_t)0, (uint64_t)0, (const uint64_t*)nullptr);
    MH_LAUNCH_CHECK("mh_ppeg_bwd");
    return MH_OK;
}

// ------------------------------------------------------------------ merged gradient -> the six parameter gradients
// The forward folds the 7x7, 5x5 and 3x3 depthwise kernels (and their biases) into one 7x7 (mh_ppeg_merge), so the gradient
// of the merged kernel IS the 7x7's, its centre 5x5 the 5x5's, its centre 3x3 the 3x3's, and all three biases get dbsum
// (models/mirror.py:324-331).  One launch that ACCUMULATES into the six buffers (the training engine's gradient arena)
// instead of two zero fills, a transposing copy, two window copies, two clones and six `grad += new` launches of autograd.
__global__ __launch_bounds__(256) void ppeg_grad_scatter_kernel(const float* __restrict__ dm, const float* __restrict__ dbs,
                                                                float* __restrict__ dw7, float* __restrict__ dw5, float* __restrict__ dw3,
                                                                float* __restrict__ db7, float* __restrict__ db5, float* __restrict__ db3, int D) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < D * 49) {
        const int c = i / 49, t = i - c * 49, ky = t / 7, kx = t - ky * 7;
        const float v = dm[(long)t * D + c];          // dmerged is tap-major [49, D]
        dw7[i] += v;
        if (ky >= 1 && ky <= 5 && kx >= 1 && kx <= 5) dw5[c * 25 + (ky - 1) * 5 + (kx - 1)] += v;
        if (ky >= 2 && ky <= 4 && kx >= 2 && kx <= 4) dw3[c * 9 + (ky - 2) * 3 + (kx - 2)] += v;
    }
    if (i < D) {
        const float b = dbs[i];
        db7[i] += b;
        db5[i] += b;
        db3[i] += b;
    }
}

extern "C" int mh_ppeg_grad_scatter(const float* dmerged, const float* dbsum, float* dw7, float* dw5, float* dw3, float* db7,
                                    float* db5, float* db3, int D, mh_stream s) {
    MH_REQUIRE(dmerged && dbsum && dw7 && dw5 && dw3 && db7 && db5 && db3, "mh_ppeg_grad_scatter: null pointer");
    if (D == 0) return MH_OK;
    hipLaunchKernelGGL(ppeg_grad_scatter_kernel, dim3(mh_cdiv(D * 49, 256)), dim3(256), 0, (hipStream_t)s, dmerged, dbsum, dw7, dw5, dw3, db7, db5, db3, D);
    MH_LAUNCH_CHECK("mh_ppeg_grad_scatter");
    return MH_OK;
}
