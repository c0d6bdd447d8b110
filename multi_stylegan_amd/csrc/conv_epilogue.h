// The epilogue of the MFMA convolution kernels (internal; included by the conv_*.hip files): accumulators -> wave-private LDS
// patch -> 16-byte channel vectors -> global stores.  The patch layout is a data format the kernels share; it is stated here once.
//
// Who owns what.  The MFMAs run with the operands swapped, so an accumulator block holds the TRANSPOSED product and a lane owns
// one pixel and runs of four CONSECUTIVE channels:
//   * v_mfma_f32_32x32x*: lane (lr = lane & 31, lh = lane >> 5) owns pixel 32 i + lr of block (i, j) and, per group g = e >> 2 of
//     its 16 accumulator elements, channels 32 j + 8 g + 4 lh + (0..3) -- the 4-channel unit 8 j + 2 g + lh of the patch row;
//   * v_mfma_f32_16x16x32_bf16 (conv_fprop_row3.hip, S16): lane (lr = lane & 15, lh = lane >> 4) owns pixel 16 i + lr and the
//     channels 16 j + 4 lh + (0..3) of block (i, j) -- one group, unit 4 j + lh.
// The patch.  Each wave has its own: rows = pixels of the wave tile (or a slice of it), COLS channels of storage type T per row,
// pitch COLS * sizeof(T) bytes, COLS >= 64.  A unit is four channels -- 8 bytes of bf16, 16 bytes of f32 -- and goes to LDS as ONE
// packed write (32 ds_write_b64 per 64 x 64 bf16 patch instead of 128 ds_write_b16); unit u of row r lives at unit u ^ (r & 15),
// which spreads the 16 rows a lane group writes over all banks.
// Reading back.  COLS * sizeof(T) / 16 lanes share a row, lane u of them reads the row's 16-byte vector u.  f32: that is unit u,
// at byte (u ^ (r & 15)) << 4.  Two-byte storage: it is the 8-byte units 2 u and 2 u + 1, which the swizzle keeps together, at
// byte (u ^ ((r & 15) >> 1)) << 4 -- one aligned read -- in swapped order when r is odd (conv_patch_swap_odd).
#pragma once
#include "conv_dispatch.h"

// One unit: the four channels `a` of row `row` into the patch at `ep`.
template <typename T, int COLS>
__device__ __forceinline__ void conv_patch_write(char* ep, int row, int unit, f32x4 a) {
    char* dst = ep + row * (COLS * (int)sizeof(T)) + ((unit ^ (row & 15)) * (4 * (int)sizeof(T)));
    if constexpr (sizeof(T) == 2) {
        uint2 pk;
        pk.x = (unsigned)f2bf(a[0]) | ((unsigned)f2bf(a[1]) << 16);
        pk.y = (unsigned)f2bf(a[2]) | ((unsigned)f2bf(a[3]) << 16);
        *reinterpret_cast<uint2*>(dst) = pk;
    } else {
        *reinterpret_cast<f32x4*>(dst) = a;
    }
}
// ... plus the four bias values of its channels
template <typename T, int COLS>
__device__ __forceinline__ void conv_patch_write(char* ep, int row, int unit, f32x4 a, f32x4 bv) {
    conv_patch_write<T, COLS>(ep, row, unit, f32x4{a[0] + bv[0], a[1] + bv[1], a[2] + bv[2], a[3] + bv[3]});
}
// bias[nb .. nb + 3], zeros without a bias and past channel N
__device__ __forceinline__ f32x4 conv_patch_bias(const float* bias, int nb, int N) {
    f32x4 bv = {0.f, 0.f, 0.f, 0.f};
    if (bias) {
#pragma unroll
        for (int e = 0; e < 4; ++e) bv[e] = nb + e < N ? bias[nb + e] : 0.f;
    }
    return bv;
}

// Rows row0 + pass * RPP (pass < NP) of the patch, this lane's 16-byte vector `u` of each.  All of them are requested before any
// is used: one LDS latency for the lot.  Two-byte storage: conv_patch_swap_odd finishes the read (its own call, so that a
// kernel may put other loads between the two).
template <typename T, int COLS, int NP, int RPP>
__device__ __forceinline__ void conv_patch_read(const char* ep, int row0, int u, u32x4 (&v)[NP]) {
#pragma unroll
    for (int pass = 0; pass < NP; ++pass) {
        const int row = row0 + pass * RPP;
        const int sw = sizeof(T) == 2 ? (row & 15) >> 1 : row & 15;
        v[pass] = *reinterpret_cast<const u32x4*>(ep + row * (COLS * (int)sizeof(T)) + ((u ^ sw) << 4));
    }
}
// RPP is even in every kernel, so a lane's rows are all odd or all even: `row0` decides for the lot.
template <int NP>
__device__ __forceinline__ void conv_patch_swap_odd(int row0, u32x4 (&v)[NP]) {
    if (row0 & 1) {
#pragma unroll
        for (int pass = 0; pass < NP; ++pass) v[pass] = u32x4{v[pass][2], v[pass][3], v[pass][0], v[pass][1]};
    }
}

// The rest of the generic and ping-pong kernels' epilogue: the wave's ROWS x 64 patch at `ep` (written; this call holds the
// barrier) to y, through the fused activation stage or the residual merge where `p.act` asks for one.  m_wave / n_wave: first GEMM
// row / column of the wave tile; P: ConvParams or ConvParamsPP.
template <typename T, int ROWS, typename P>
__device__ __forceinline__ void conv_tile_store(const P& p, T* __restrict__ y, const char* ep, int lane, int m_wave, int n_wave,
                                                int bz, int ohw) {
    constexpr int VEC = 16 / sizeof(T);
    constexpr int LPR = 64 / VEC;                                  // lanes per 64-element row
    constexpr int RPP = 64 / LPR;                                  // rows per pass
    constexpr int NPASS = ROWS / RPP;
    const int er = lane / LPR, ec = (lane % LPR) * VEC;
    const int n = n_wave + ec;
    int nn = n, q = 0;
    if (p.pixel_shuffle) { const int oc = p.N >> 2; q = n / oc; nn = n - q * oc; }
    const int lim = p.pixel_shuffle ? (p.N >> 2) - nn : p.N - n;  // valid elements left in this channel run
    const bool n_ok = n < p.N;
    // Row coordinates (sample, oh, ow) of this lane's row of pass 0 by division ONCE; later passes are RPP pixels further
    // along and are reached by stepping.  gp[pass] = index of the OUTPUT pixel the row is stored to (sample-major,
    // pixel-shuffled where asked), -1 for rows past M; the fused stage's bias vector and per-row noise values are
    // fetched in the same sweep, before the barrier.
    int gp[NPASS];
    float a_bias[VEC], a_noise[NPASS];
    {
        const int m_first = min(m_wave + er, p.Mtot - 1);
        int b = p.per_sample ? bz : m_first / ohw;
        const int pix0 = p.per_sample ? m_first : m_first - b * ohw;
        int oh = pix0 / p.OW, ow = pix0 - oh * p.OW;
        const bool want_noise = p.act.enabled == 1 && p.act.noise;
        const float nw = want_noise ? p.act.noise_w[0] : 0.f;
        if (p.act.enabled == 1) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) a_bias[e] = (p.act.bias && n + e < p.N) ? p.act.bias[n + e] : 0.f;
        }
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            const bool ok = m_wave + pass * RPP + er < p.Mtot;
            const int pix = oh * p.OW + ow;
            const int g = p.pixel_shuffle ? ((b * 2 * p.OH + 2 * oh + (q >> 1)) * (2 * p.OW) + 2 * ow + (q & 1))
                                          : b * ohw + pix;
            gp[pass] = ok ? g : -1;
            a_noise[pass] = (want_noise && ok) ? nw * p.act.noise[(long long)(p.act.noise_batch == 1 ? 0 : b) * ohw + pix] : 0.f;
            ow += RPP;
            while (ow >= p.OW) { ow -= p.OW; ++oh; }
            if (!p.per_sample) while (oh >= p.OH) { oh -= p.OH; ++b; }
        }
    }
    __syncthreads();
    // (for the residual merge all residual vectors are requested before any is used too: one HBM latency per tile)
    u32x4 v[NPASS];
    conv_patch_read<T, 64, NPASS, RPP>(ep, er, lane & (LPR - 1), v);
    if constexpr (sizeof(T) == 2) conv_patch_swap_odd<NPASS>(er, v);
    if (p.act.enabled == 1) {
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) v[pass] = act_epilogue_apply<T>(v[pass], a_bias, a_noise[pass], p.act.alpha, p.act.scale);
    } else if (p.act.enabled == 2) {                          // residual merge (never with pixel_shuffle)
        const T* rbase = reinterpret_cast<const T*>(p.act.residual) + (n_ok ? n : 0);
        u32x4 r[NPASS];
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass)
            r[pass] = *reinterpret_cast<const u32x4*>(rbase + (long long)max(gp[pass], 0) * p.act.res_ld);
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) v[pass] = residual_epilogue_apply<T>(v[pass], r[pass], p.act.res_gain);
    }
    T* ybase = y + (p.pixel_shuffle ? nn : n);
    if (n_ok && lim >= VEC) {
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass)
            if (gp[pass] >= 0) *reinterpret_cast<u32x4*>(ybase + (long long)gp[pass] * p.ldy) = v[pass];
    } else if (n_ok) {                                        // ragged channel tail: element stores
#pragma unroll
        for (int pass = 0; pass < NPASS; ++pass) {
            if (gp[pass] < 0) continue;
            T tmp[VEC];
            *reinterpret_cast<u32x4*>(tmp) = v[pass];
            T* dst = ybase + (long long)gp[pass] * p.ldy;
            for (int e = 0; e < lim; ++e) dst[e] = tmp[e];
        }
    }
}
