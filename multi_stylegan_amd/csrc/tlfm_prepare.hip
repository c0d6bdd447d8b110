// The data feed's batch prepare: raw 16-bit camera counts [B, C, T, H, W] -> the normalised (and flipped) float frames the
// reference's dataset computes on the host, sample by sample, in its DataLoader workers (dataset/tlfm_dataset.py:186-197,
// dataset/utils.py:4-23).  Channel 0 (bright field) is min-max normalised per (b, t) frame, channels 1 / 2 (GFP / RFP) are
// ((x - lo).clamp(min=0) / div).clamp(max=1); the flips happen on the store side, which equals "flip, then normalise" because
// the arithmetic is per pixel and a frame's minimum / maximum do not depend on the order of its pixels.
//
// Arithmetic: counts are unsigned and exact in fp32; IEEE subtract, IEEE (correctly rounded) divide, the clamps in the
// reference's order -- the fp32 result equals torch's on the CPU bit for bit, the bf16 result is its round-to-nearest-even.
//
// Two launches per call.  Every frame is split over `S` workgroups (tlfm_split: ~4096 pixels each), so that the 96 frames of the
// benchmark batch (16 x 2 x 3 at 256^2) become 1536 workgroups instead of 96 on 256 CUs:
//   1. tlfm_minmax_kernel   one (min, max) pair of integers per bright-field frame and split into ws -- every word the second
//                           launch reads is written here, so the workspace needs no initialisation and carries nothing from
//                           call to call; integer min / max are order-independent, the result is deterministic;
//   2. tlfm_normalise_kernel combines the S pairs of its frame (a handful of uniform loads) and streams its rows.  Bright-field
//                           workgroups come first in the grid with the block index they had in launch 1, so a frame's second
//                           read is issued from the XCD whose L2 took the first.
// W % 8 == 0 and 16-byte aligned bases: 16 bytes (8 pixels) per lane and load; a mirrored row loads the mirrored vector and
// reverses its 8 pixels in registers, so loads and stores both stay coalesced.  Anything else takes the scalar path.
#include "msg_common.h"

constexpr int TLFM_MAX_SPLIT = 32;              // workspace words per bright-field frame: 2 * TLFM_MAX_SPLIT
constexpr int TLFM_PIXELS_PER_BLOCK = 4096;

static int tlfm_split(int H, int W) {
    long long s = ((long long)H * W + TLFM_PIXELS_PER_BLOCK - 1) / TLFM_PIXELS_PER_BLOCK;
    if (s > TLFM_MAX_SPLIT) s = TLFM_MAX_SPLIT;
    if (s > H) s = H;                           // the normalise kernel splits a frame by rows
    return (int)s;
}

__device__ __forceinline__ void tlfm_unpack8(uint4 v, unsigned int* px) {
    const unsigned int w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        px[2 * k] = w[k] & 0xffffu;
        px[2 * k + 1] = w[k] >> 16;
    }
}

// block (f, s) of B*T x S, flat: f = blockIdx.x / S -> ws[2 * blockIdx.x] = min, [.. + 1] = max over its share of the frame
// (an empty share leaves the identities 0xffffffff / 0)
template <bool VEC>
__global__ __launch_bounds__(256) void tlfm_minmax_kernel(const unsigned short* __restrict__ raw, unsigned int* __restrict__ ws,
                                                          int C, int T, long long P, int S) {
    const long long f = blockIdx.x / S;
    const int s = (int)(blockIdx.x - f * S);
    const long long b = f / T, t = f - b * T;
    const unsigned short* src = raw + (b * C * T + t) * P;                       // channel 0 of sample b, frame t
    const long long items = VEC ? P / 8 : P;
    const long long per = (items + S - 1) / S;
    const long long i0 = s * per, i1 = i0 + per < items ? i0 + per : items;
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
        if constexpr (VEC) {
            unsigned int px[8];
            tlfm_unpack8(*reinterpret_cast<const uint4*>(src + i * 8), px);
#pragma unroll
            for (int e = 0; e < 8; ++e) { lo = min(lo, px[e]); hi = max(hi, px[e]); }
        } else {
            const unsigned int x = src[i];
            lo = min(lo, x); hi = max(hi, x);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, (unsigned int)__shfl_xor((int)lo, off, 64));
        hi = max(hi, (unsigned int)__shfl_xor((int)hi, off, 64));
    }
    __shared__ unsigned int s_lo[4], s_hi[4];
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[2 * (long long)blockIdx.x] = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
        ws[2 * (long long)blockIdx.x + 1] = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
    }
}

template <bool CLAMP>
__device__ __forceinline__ float tlfm_value(unsigned int count, float lo, float div) {
    float v = (float)count - lo;
    if constexpr (CLAMP) {
        v = v < 0.f ? 0.f : v;                 // .clamp(min=0): a NaN stays a NaN, as in torch
        v = v / div;
        return v > 1.f ? 1.f : v;              // .clamp(max=1)
    } else {
        return v / div;                        // a constant frame: 0 / 0 = NaN, as the reference
    }
}

template <typename OT, bool VEC, bool CLAMP>
__device__ __forceinline__ void tlfm_rows(const unsigned short* __restrict__ src, OT* __restrict__ dst, int H, int W, int r0,
                                          int r1, bool hf, int vflip, float lo, float div) {
    if constexpr (VEC) {
        const int wv = W / 8;
        const long long items = (long long)(r1 - r0) * wv;
        for (long long i = threadIdx.x; i < items; i += 256) {
            const int row = r0 + (int)(i / wv), v = (int)(i % wv);
            const int hs = vflip ? H - 1 - row : row, vs = hf ? wv - 1 - v : v;
            unsigned int px[8];
            tlfm_unpack8(*reinterpret_cast<const uint4*>(src + (long long)hs * W + (long long)vs * 8), px);
            float f[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = tlfm_value<CLAMP>(hf ? px[7 - e] : px[e], lo, div);
            OT* p = dst + (long long)row * W + (long long)v * 8;
            if constexpr (sizeof(OT) == 4) {
                *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
                *reinterpret_cast<float4*>(p + 4) = make_float4(f[4], f[5], f[6], f[7]);
            } else {
                Vec16<bf16_t> o;
#pragma unroll
                for (int e = 0; e < 4; ++e) o.set2(e, f[2 * e], f[2 * e + 1]);
                *reinterpret_cast<uint4*>(p) = o.raw;
            }
        }
    } else {
        const long long items = (long long)(r1 - r0) * W;
        for (long long i = threadIdx.x; i < items; i += 256) {
            const int row = r0 + (int)(i / W), x = (int)(i % W);
            const int hs = vflip ? H - 1 - row : row, xs = hf ? W - 1 - x : x;
            store_from_f32<OT>(dst + (long long)row * W + x, tlfm_value<CLAMP>(src[(long long)hs * W + xs], lo, div));
        }
    }
}

// grid: the B*T*S bright-field blocks in the order of tlfm_minmax_kernel, then B*(C-1)*T*S blocks of the other channels
template <typename OT, bool VEC>
__global__ __launch_bounds__(256) void tlfm_normalise_kernel(const unsigned short* __restrict__ raw,
                                                             const unsigned char* __restrict__ hflip, OT* __restrict__ out,
                                                             const unsigned int* __restrict__ ws, int B, int C, int T, int H,
                                                             int W, int S, int vflip, float lo1, float div1, float lo2,
                                                             float div2) {
    const long long n = blockIdx.x, nbf = (long long)B * T * S;
    long long b, t;
    int c, s;
    if (n < nbf) {
        const long long f = n / S;
        s = (int)(n - f * S);
        b = f / T; t = f - b * T; c = 0;
    } else {
        const long long m = n - nbf, f = m / S, ct = (long long)(C - 1) * T;
        s = (int)(m - f * S);
        b = f / ct;
        const long long r = f - b * ct;
        c = 1 + (int)(r / T);
        t = r - (long long)(c - 1) * T;
    }
    const long long P = (long long)H * W, base = ((b * C + c) * T + t) * P;
    const int per = (H + S - 1) / S;
    const int r0 = s * per < H ? s * per : H, r1 = r0 + per < H ? r0 + per : H;
    const bool hf = hflip != nullptr && hflip[b] != 0;
    if (c == 0) {
        unsigned int mn = 0xffffffffu, mx = 0u;
        const unsigned int* part = ws + 2 * (b * T + t) * S;
        for (int k = 0; k < S; ++k) { mn = min(mn, part[2 * k]); mx = max(mx, part[2 * k + 1]); }
        const float lo = (float)mn;
        tlfm_rows<OT, VEC, false>(raw + base, out + base, H, W, r0, r1, hf, vflip, lo, (float)mx - lo);
    } else {
        tlfm_rows<OT, VEC, true>(raw + base, out + base, H, W, r0, r1, hf, vflip, c == 1 ? lo1 : lo2, c == 1 ? div1 : div2);
    }
}

extern "C" long long msg_tlfm_prepare_workspace(int B, int T) {
    if (B <= 0 || T <= 0) return 0;
    return 2ll * TLFM_MAX_SPLIT * B * T;
}

template <typename OT>
static void tlfm_launch(const unsigned short* raw, const unsigned char* hflip, OT* out, int B, int C, int T, int H, int W, int vflip,
                        float lo1, float div1, float lo2, float div2, unsigned int* ws, hipStream_t s) {
    const int S = tlfm_split(H, W);
    const bool vec = W % 8 == 0 && ((((uintptr_t)raw) | ((uintptr_t)out)) & 15u) == 0;
    const long long P = (long long)H * W;
    const unsigned nbf = (unsigned)((long long)B * T * S), nall = (unsigned)((long long)B * C * T * S);
    if (vec) {
        hipLaunchKernelGGL((tlfm_minmax_kernel<true>), dim3(nbf), dim3(256), 0, s, raw, ws, C, T, P, S);
        hipLaunchKernelGGL((tlfm_normalise_kernel<OT, true>), dim3(nall), dim3(256), 0, s, raw, hflip, out, ws, B, C, T, H, W, S,
                           vflip, lo1, div1, lo2, div2);
    } else {
        hipLaunchKernelGGL((tlfm_minmax_kernel<false>), dim3(nbf), dim3(256), 0, s, raw, ws, C, T, P, S);
        hipLaunchKernelGGL((tlfm_normalise_kernel<OT, false>), dim3(nall), dim3(256), 0, s, raw, hflip, out, ws, B, C, T, H, W, S,
                           vflip, lo1, div1, lo2, div2);
    }
}

extern "C" int msg_tlfm_prepare(const unsigned short* raw, const unsigned char* hflip, void* out, int dtype, int B, int C, int T,
                                int H, int W, int vflip, float lo1, float div1, float lo2, float div2, unsigned int* ws,
                                void* stream) {
    if (B <= 0 || C <= 0 || C > 3 || T <= 0 || H <= 0 || W <= 0 || !raw || !out || !ws) return MSG_EINVAL;
    if (dtype != MSG_F32 && dtype != MSG_BF16) return MSG_EINVAL;
    if ((long long)B * C * T * TLFM_MAX_SPLIT > 0x7fffffffll) return MSG_EINVAL;      // (one block index per frame and split)
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MSG_BF16)
        tlfm_launch<bf16_t>(raw, hflip, (bf16_t*)out, B, C, T, H, W, vflip, lo1, div1, lo2, div2, ws, s);
    else
        tlfm_launch<float>(raw, hflip, (float*)out, B, C, T, H, W, vflip, lo1, div1, lo2, div2, ws, s);
    return MSG_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------------------------
// The resident dataset (resident.py): every frame of the dataset decoded once into one store [N, H, W] of counts in HBM, a
// batch built by ONE launch that gathers the frames its samples name.  Replaces the per-epoch re-read of
// dataset/tlfm_dataset.py:128-198 in the DataLoader workers of train_multi_stylegan.py:60-63 and, with it, the first of the
// two launches above: a frame's bright-field minimum and maximum do not change between epochs, so they are computed when the
// store is built (tlfm_frame_range_kernel) and the gather reads one (min, max) pair per frame instead of a workspace.
// The arithmetic is tlfm_value / tlfm_rows above, unchanged -- the fp32 result equals msg_tlfm_prepare's on the stacked frames.

// one workgroup per frame: range[2 f] = min, range[2 f + 1] = max of its P counts (integers: order-independent, deterministic)
template <bool VEC>
__global__ __launch_bounds__(256) void tlfm_frame_range_kernel(const unsigned short* __restrict__ frames,
                                                               unsigned int* __restrict__ range, long long P) {
    const long long f = blockIdx.x;
    const unsigned short* src = frames + f * P;
    const long long items = VEC ? P / 8 : P;
    unsigned int lo = 0xffffffffu, hi = 0u;
    for (long long i = threadIdx.x; i < items; i += 256) {
        if constexpr (VEC) {
            unsigned int px[8];
            tlfm_unpack8(*reinterpret_cast<const uint4*>(src + i * 8), px);
#pragma unroll
            for (int e = 0; e < 8; ++e) { lo = min(lo, px[e]); hi = max(hi, px[e]); }
        } else {
            const unsigned int x = src[i];
            lo = min(lo, x); hi = max(hi, x);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, (unsigned int)__shfl_xor((int)lo, off, 64));
        hi = max(hi, (unsigned int)__shfl_xor((int)hi, off, 64));
    }
    __shared__ unsigned int s_lo[4], s_hi[4];
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        range[2 * f] = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
        range[2 * f + 1] = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
    }
}

// block (f, s) of B*C*T x S, flat; f is also the position in `index` [B, C, T].  The frame id is one uniform load, the bounds
// check on it uniform per workgroup: an id outside [0, N) reads nothing and fills its share of the output frame with NaN.
template <typename OT, bool VEC>
__global__ __launch_bounds__(256) void tlfm_gather_kernel(const unsigned short* __restrict__ frames,
                                                          const unsigned int* __restrict__ range, long long N,
                                                          const int* __restrict__ index, const unsigned char* __restrict__ hflip,
                                                          OT* __restrict__ out, int C, int T, int H, int W, int S, int vflip,
                                                          float lo1, float div1, float lo2, float div2) {
    const long long f = blockIdx.x / S;
    const int s = (int)(blockIdx.x - f * S);
    const long long b = f / ((long long)C * T);
    const int c = (int)((f / T) % C);
    const long long P = (long long)H * W;
    const int per = (H + S - 1) / S;
    const int r0 = s * per < H ? s * per : H, r1 = r0 + per < H ? r0 + per : H;
    OT* dst = out + f * P;
    const long long id = index[f];
    if (id < 0 || id >= N) {
        const float nan = __builtin_nanf("");
        for (long long i = (long long)r0 * W + threadIdx.x; i < (long long)r1 * W; i += 256) store_from_f32<OT>(dst + i, nan);
        return;
    }
    const unsigned short* src = frames + id * P;                                  // 64-bit: N * P may exceed 2^31 elements
    const bool hf = hflip != nullptr && hflip[b] != 0;
    if (c == 0) {
        const float lo = (float)range[2 * id];
        tlfm_rows<OT, VEC, false>(src, dst, H, W, r0, r1, hf, vflip, lo, (float)range[2 * id + 1] - lo);
    } else {
        tlfm_rows<OT, VEC, true>(src, dst, H, W, r0, r1, hf, vflip, c == 1 ? lo1 : lo2, c == 1 ? div1 : div2);
    }
}

extern "C" int msg_tlfm_frame_range(const unsigned short* frames, long long N, int H, int W, unsigned int* range, void* stream) {
    if (N <= 0 || H <= 0 || W <= 0 || !frames || !range) return MSG_EINVAL;
    if (N > 0x7fffffffll) return MSG_EINVAL;                                      // (one block index per frame)
    const long long P = (long long)H * W;
    hipStream_t s = (hipStream_t)stream;
    if (P % 8 == 0 && (((uintptr_t)frames) & 15u) == 0)
        hipLaunchKernelGGL((tlfm_frame_range_kernel<true>), dim3((unsigned)N), dim3(256), 0, s, frames, range, P);
    else
        hipLaunchKernelGGL((tlfm_frame_range_kernel<false>), dim3((unsigned)N), dim3(256), 0, s, frames, range, P);
    return MSG_CHECK_LAUNCH();
}

template <typename OT>
static void tlfm_gather_launch(const unsigned short* frames, const unsigned int* range, long long N, const int* index,
                               const unsigned char* hflip, OT* out, int B, int C, int T, int H, int W, int vflip, float lo1,
                               float div1, float lo2, float div2, hipStream_t s) {
    const int S = tlfm_split(H, W);
    const bool vec = W % 8 == 0 && ((((uintptr_t)frames) | ((uintptr_t)out)) & 15u) == 0;
    const unsigned blocks = (unsigned)((long long)B * C * T * S);
    if (vec)
        hipLaunchKernelGGL((tlfm_gather_kernel<OT, true>), dim3(blocks), dim3(256), 0, s, frames, range, N, index, hflip, out, C,
                           T, H, W, S, vflip, lo1, div1, lo2, div2);
    else
        hipLaunchKernelGGL((tlfm_gather_kernel<OT, false>), dim3(blocks), dim3(256), 0, s, frames, range, N, index, hflip, out, C,
                           T, H, W, S, vflip, lo1, div1, lo2, div2);
}

extern "C" int msg_tlfm_gather(const unsigned short* frames, const unsigned int* range, long long N, const int* index,
                               const unsigned char* hflip, void* out, int dtype, int B, int C, int T, int H, int W, int vflip,
                               float lo1, float div1, float lo2, float div2, void* stream) {
    if (N <= 0 || B <= 0 || C <= 0 || C > 3 || T <= 0 || H <= 0 || W <= 0 || !frames || !range || !index || !out)
        return MSG_EINVAL;
    if (dtype != MSG_F32 && dtype != MSG_BF16) return MSG_EINVAL;
    if ((long long)B * C * T * TLFM_MAX_SPLIT > 0x7fffffffll) return MSG_EINVAL;      // (one block index per frame and split)
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MSG_BF16)
        tlfm_gather_launch<bf16_t>(frames, range, N, index, hflip, (bf16_t*)out, B, C, T, H, W, vflip, lo1, div1, lo2, div2, s);
    else
        tlfm_gather_launch<float>(frames, range, N, index, hflip, (float*)out, B, C, T, H, W, vflip, lo1, div1, lo2, div2, s);
    return MSG_CHECK_LAUNCH();
}
