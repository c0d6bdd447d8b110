// What the weight-gradient kernels share (internal; included by conv_wgrad.hip and conv_wgrad_row3.hip): the LDS image of an
// operand tile, the transposing fragment read, the fp32 store and the common fields of the parameter structs.  The image is a
// data format of both kernels; it is stated here once.
//
// The image.  A tile is [pixel row][128 channels] exactly as in global memory, pitch ROW bytes: 256 for a bf16 tile or one bf16
// plane of a split fp32 operand, 512 for fp32.  Row r is ROTATED by 64 B * (r & 3): byte column c of row r lives at column
// (c + 64 (r & 3)) mod ROW.  That keeps the transposing reads of the four pixel rows of a block on disjoint banks.
// Filling it.  Register staging writes through wg_image_off.  LDS-DMA writes whole rows in lane order and cannot rotate on the
// way, so the rotation is applied on the GLOBAL side: the lane whose 16 bytes land in physical chunk c of row r fetches the
// logical chunk wg_dma_chunk(r, c).
// Reading it (bf16).  ds_read_b64_tr_b16: within a group of 16 lanes, lane 4 q + pq supplies the address of pixel row q of a
// 4-pixel block, channels 4 pq .. 4 pq + 3 of a 16-channel block, and receives channel (lane % 16) of the block's four pixel rows.
// An MFMA operand of eight pixels is two such reads four pixel rows apart (rows r and r + 4 share their rotation), joined.
// fp32 needs no transposition: an operand is one element per lane, read at wg_image_off.
#pragma once
#include "conv_dispatch.h"

// byte offset of (pixel row r, byte column col) in a tile of pitch ROW
template <int ROW>
__device__ __forceinline__ int wg_image_off(int r, int col) { return r * ROW + ((col + ((r & 3) << 6)) & (ROW - 1)); }

// LDS-DMA: the logical 16-B chunk that belongs in physical chunk c of row r (the inverse of the rotation; only r & 3 matters)
template <int ROW>
__device__ __forceinline__ int wg_dma_chunk(int r, int c) { return (c - 4 * (r & 3)) & (ROW / 16 - 1); }

// the two transposing reads at `a` and four pixel rows (`four_rows` bytes) further down, joined into one MFMA operand
__device__ __forceinline__ bf16v8 wg_frag_read(const char* a, int four_rows) {
    s16x4 part[2];
#pragma unroll
    for (int half = 0; half < 2; ++half)
        part[half] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3)))*)(a + half * four_rows));
    return __builtin_bit_cast(bf16v8, (s16x8)__builtin_shufflevector(part[0], part[1], 0, 1, 2, 3, 4, 5, 6, 7));
}

// The operand of a 32x32x16 MFMA from a bf16 tile or split plane (pitch 256) at `base`: pixels 16 ks .. 16 ks + 15, channels
// col0 .. col0 + 31.  Lane = 16 g + 4 q + pq supplies the address of pixel row (kb + q), channels cb + 4 pq ..+3; it receives
// channel (cb + lane % 16) of pixel rows kb .. kb + 3 and kb + 4 .. kb + 7.
__device__ __forceinline__ bf16v8 wg_frag(const char* base, int lane, int ks, int col0) {
    const int g = lane >> 4, q = (lane >> 2) & 3, pq = lane & 3;
    const int kb = 8 * (g >> 1), cb = 16 * (g & 1);
    return wg_frag_read(base + wg_image_off<256>(ks * 16 + kb + q, (col0 + cb + 4 * pq) * 2), 4 * 256);
}

// Where a workgroup stores: K-slice z of a split sum owns slab z of the workspace (kernel layout, every element written, zeros
// included: the fixed-order reduce reads all of it); an unsplit result goes to gw (sample b's with per-sample weights), in the
// parameter's own layout when the caller asked for it.
template <typename P>
__device__ __forceinline__ float* wg_store_base(const P& p, float* gw, float* ws, int z, int b, bool& oi_major) {
    oi_major = p.oi_major && !p.split;
    return p.split ? ws + (long long)z * p.slab : gw + (p.per_sample ? (long long)b * p.gw_zstride : 0);
}
// One element: kernel layout gz[o][tap][ldgw] (the padding columns I .. ldgw - 1 are written, with the zeros the padded
// operand channels give), or oi_major gz[o][i][tap] (no padding: nothing past I).
template <typename P>
__device__ __forceinline__ void wg_store(const P& p, float* gz, bool oi_major, int o, int ic, int tap, int taps, float v) {
    if (ic >= p.ldgw || o >= p.O) return;
    float* dst = oi_major ? gz + ((long long)o * p.I + ic) * taps + tap : gz + ((long long)o * taps + tap) * p.ldgw + ic;
    if (oi_major && ic >= p.I) return;
    *dst = v * p.gain;
}

// The fields the two parameter structs (WgradParams, Row3Params) share under one name.
template <typename P>
inline void wgrad_fill_common(P& p, const WgradProblem& q, const WgradPlan& plan) {
    p.B = q.B; p.Cx = q.Cx; p.I = q.I; p.ldgy = q.ldgy; p.O = q.O; p.ldgw = q.ldgw;
    p.per_sample = q.per_sample; p.oi_major = q.oi_major; p.gain = q.gain;
    p.o_tiles = (q.O + 127) / 128; p.i_tiles = (q.I + 127) / 128;
    p.gw_zstride = q.gw_zstride(); p.slab = q.slab();
    p.nz = plan.nz; p.split = plan.chunks_per_out > 1;
}
