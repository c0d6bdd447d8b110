// Simulated datasets: the generator's frames [B, C, T, H, W] -> the 16-bit camera counts the dataset would have read them from
// (dataset/tlfm_dataset.py:186-197 and dataset/utils.py:4-23 read backwards): tlfm_prepare.hip's inverse.  Channel 0 (bright
// field) is min-max normalised per (b, t) frame and spread over that frame's count range [lo, hi]; channels 1 / 2 (GFP / RFP)
// are clamp(x, 0, 1) * div + low with the dataset's (min, max) -- it divides by max, not by max - min.  The vertical flip is a
// whole-row remap on the load side (a frame's minimum / maximum do not depend on the order of its rows).
//
// Arithmetic: fp32 throughout (bf16 is widened first), every operation rounded on its own -- IEEE subtract, correctly rounded
// divide, the product and the sum kept apart (fp contract off: no FMA), rint to nearest-even -- so the counts equal
// the host's torch statement (simulate._export_tlfm_host) one for one.
//
// Two launches per call (one when the bright field is not normalised).  Every frame is split over `S` workgroups by rows
// (tlfm_export_split: ~4096 pixels each, at most 32, at most H):
//   1. tlfm_export_minmax_kernel  one (min, max) pair of floats per bright-field frame and split into ws -- every word launch 2
//                                 reads is written here, the workspace needs no initialisation; fminf / fmaxf skip NaN and are
//                                 order-independent in value, nothing is atomic: the result is deterministic.  Split s reads the
//                                 input rows that split s of launch 2 streams;
//   2. tlfm_export_kernel         combines the S pairs of its frame and streams its rows.  Bright-field workgroups come first in
//                                 the grid with the block index they had in launch 1.
// W % 8 == 0 and 16-byte aligned bases: 8 pixels per lane -- 16-byte loads (two for fp32, one for bf16), one 16-byte store.
// Anything else takes the scalar path.
#include "msg_common.h"

constexpr int TLFM_EXPORT_MAX_SPLIT = 32;       // workspace words per bright-field frame: 2 * TLFM_EXPORT_MAX_SPLIT
constexpr int TLFM_EXPORT_PIXELS_PER_BLOCK = 4096;

static int tlfm_export_split(int H, int W) {
    long long s = ((long long)H * W + TLFM_EXPORT_PIXELS_PER_BLOCK - 1) / TLFM_EXPORT_PIXELS_PER_BLOCK;
    if (s > TLFM_EXPORT_MAX_SPLIT) s = TLFM_EXPORT_MAX_SPLIT;
    if (s > H) s = H;                           // a frame is split by rows
    return (int)s;
}

// 8 consecutive pixels (p 16-byte aligned) as fp32
template <typename IT> __device__ __forceinline__ void tlfm_export_load8(const IT* __restrict__ p, float* f);
template <> __device__ __forceinline__ void tlfm_export_load8<float>(const float* __restrict__ p, float* f) {
    const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
    f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
template <> __device__ __forceinline__ void tlfm_export_load8<bf16_t>(const bf16_t* __restrict__ p, float* f) {
    Vec16<bf16_t> v;
    v.raw = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = v.get(e);
}

// the rows [r0, r1) of the OUTPUT frame that split s of S writes (empty when s * ceil(H / S) >= H)
__device__ __forceinline__ void tlfm_export_share(int H, int S, int s, int& r0, int& r1) {
    const int per = (H + S - 1) / S;
    r0 = s * per < H ? s * per : H;
    r1 = r0 + per < H ? r0 + per : H;
}

// block (f, s) of B*T x S, flat: f = blockIdx.x / S -> ws[2 * blockIdx.x] = min, [.. + 1] = max over the non-NaN values of its
// rows of the frame (an empty or all-NaN share leaves the identities +inf / -inf)
template <typename IT, bool VEC>
__global__ __launch_bounds__(256) void tlfm_export_minmax_kernel(const IT* __restrict__ x, float* __restrict__ ws, int C, int T,
                                                                 int H, int W, int S, int vflip) {
    const long long f = blockIdx.x / S;
    const int s = (int)(blockIdx.x - f * S);
    const long long b = f / T, t = f - b * T;
    int r0, r1;
    tlfm_export_share(H, S, s, r0, r1);
    const int first = vflip ? H - r1 : r0;                                       // the input rows behind output rows [r0, r1)
    const IT* src = x + (b * C * T + t) * ((long long)H * W) + (long long)first * W;
    const long long n = (long long)(r1 - r0) * W;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    if constexpr (VEC) {
        for (long long i = threadIdx.x; i < n / 8; i += 256) {
            float v[8];
            tlfm_export_load8<IT>(src + i * 8, v);
#pragma unroll
            for (int e = 0; e < 8; ++e) { lo = fminf(lo, v[e]); hi = fmaxf(hi, v[e]); }
        }
    } else {
        for (long long i = threadIdx.x; i < n; i += 256) {
            const float v = load_as_f32<IT>(src + i);
            lo = fminf(lo, v); hi = fmaxf(hi, v);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, off, 64));
        hi = fmaxf(hi, __shfl_xor(hi, off, 64));
    }
    __shared__ float s_lo[4], s_hi[4];
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[2 * (long long)blockIdx.x] = fminf(fminf(s_lo[0], s_lo[1]), fminf(s_lo[2], s_lo[3]));
        ws[2 * (long long)blockIdx.x + 1] = fmaxf(fmaxf(s_hi[0], s_hi[1]), fmaxf(s_hi[2], s_hi[3]));
    }
}

// NORM: n = (x - m) / d, a constant frame (d unused) 0 with NaN kept; else n = clamp(x, 0, 1) with NaN kept.
// count = rint(n * scale + offset) in [0, 65535], the product and the sum rounded separately; NaN -> 0 (fmaxf drops it)
// (not __fmul_rn / __fadd_rn: this compiler's headers define them as the plain operators inside functions of their own, which it
//  inlines and contracts under HIP's default -ffp-contract=fast.  The pragma on plain operators is what keeps the product and
//  the sum apart, as in sample_sheet.hip)
template <bool NORM>
__device__ __forceinline__ unsigned int tlfm_export_count(float x, float m, float d, bool constant, float scale, float offset) {
#pragma clang fp contract(off)
    float n;
    if constexpr (NORM) {
        n = constant ? (x != x ? x : 0.f) : (x - m) / d;
    } else {
        n = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
    }
    float v = n * scale;
    v = v + offset;
    return (unsigned int)fminf(fmaxf(rintf(v), 0.f), 65535.f);
}

template <typename IT, bool VEC, bool NORM>
__device__ __forceinline__ void tlfm_export_rows(const IT* __restrict__ src, unsigned short* __restrict__ dst, int H, int W,
                                                 int r0, int r1, int vflip, float m, float d, bool constant, float scale,
                                                 float offset) {
    if constexpr (VEC) {
        const int wv = W / 8;
        const long long items = (long long)(r1 - r0) * wv;
        for (long long i = threadIdx.x; i < items; i += 256) {
            const int row = r0 + (int)(i / wv), v = (int)(i % wv);
            const int hs = vflip ? H - 1 - row : row;
            float f[8];
            tlfm_export_load8<IT>(src + (long long)hs * W + (long long)v * 8, f);
            unsigned int q[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) q[e] = tlfm_export_count<NORM>(f[e], m, d, constant, scale, offset);
            *reinterpret_cast<uint4*>(dst + (long long)row * W + (long long)v * 8) =
                make_uint4(q[0] | q[1] << 16, q[2] | q[3] << 16, q[4] | q[5] << 16, q[6] | q[7] << 16);
        }
    } else {
        const long long items = (long long)(r1 - r0) * W;
        for (long long i = threadIdx.x; i < items; i += 256) {
            const int row = r0 + (int)(i / W), col = (int)(i % W);
            const int hs = vflip ? H - 1 - row : row;
            dst[(long long)row * W + col] = (unsigned short)tlfm_export_count<NORM>(
                load_as_f32<IT>(src + (long long)hs * W + col), m, d, constant, scale, offset);
        }
    }
}

// grid: the B*T*S bright-field blocks in the order of tlfm_export_minmax_kernel, then B*(C-1)*T*S blocks of the other channels
template <typename IT, bool VEC>
__global__ __launch_bounds__(256) void tlfm_export_kernel(const IT* __restrict__ x, const int* __restrict__ bf_range,
                                                          unsigned short* __restrict__ out, const float* __restrict__ ws, int B,
                                                          int C, int T, int H, int W, int S, int vflip, int bf_normalise,
                                                          float low1, float div1, float low2, float div2) {
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
    int r0, r1;
    tlfm_export_share(H, S, s, r0, r1);
    if (c == 0) {
        const int lo = bf_range[2 * (b * T + t)], hi = bf_range[2 * (b * T + t) + 1];
        const float scale = (float)(hi - lo), offset = (float)lo;
        if (bf_normalise) {
            float mn = __builtin_inff(), mx = -__builtin_inff();
            const float* part = ws + 2 * (b * T + t) * S;
            for (int k = 0; k < S; ++k) { mn = fminf(mn, part[2 * k]); mx = fmaxf(mx, part[2 * k + 1]); }
            tlfm_export_rows<IT, VEC, true>(x + base, out + base, H, W, r0, r1, vflip, mn, mx - mn, mx == mn, scale, offset);
        } else {
            tlfm_export_rows<IT, VEC, false>(x + base, out + base, H, W, r0, r1, vflip, 0.f, 1.f, false, scale, offset);
        }
    } else {
        tlfm_export_rows<IT, VEC, false>(x + base, out + base, H, W, r0, r1, vflip, 0.f, 1.f, false, c == 1 ? div1 : div2,
                                         c == 1 ? low1 : low2);
    }
}

extern "C" long long msg_tlfm_export_workspace(int B, int T) {
    if (B <= 0 || T <= 0) return 0;
    return 2ll * TLFM_EXPORT_MAX_SPLIT * B * T;
}

template <typename IT>
static void tlfm_export_launch(const IT* x, const int* bf_range, unsigned short* out, int B, int C, int T, int H, int W, int vflip,
                               int bf_normalise, float low1, float div1, float low2, float div2, float* ws, hipStream_t s) {
    const int S = tlfm_export_split(H, W);
    const bool vec = W % 8 == 0 && ((((uintptr_t)x) | ((uintptr_t)out)) & 15u) == 0;
    const unsigned nbf = (unsigned)((long long)B * T * S), nall = (unsigned)((long long)B * C * T * S);
    if (vec) {
        if (bf_normalise)
            hipLaunchKernelGGL((tlfm_export_minmax_kernel<IT, true>), dim3(nbf), dim3(256), 0, s, x, ws, C, T, H, W, S, vflip);
        hipLaunchKernelGGL((tlfm_export_kernel<IT, true>), dim3(nall), dim3(256), 0, s, x, bf_range, out, ws, B, C, T, H, W, S,
                           vflip, bf_normalise, low1, div1, low2, div2);
    } else {
        if (bf_normalise)
            hipLaunchKernelGGL((tlfm_export_minmax_kernel<IT, false>), dim3(nbf), dim3(256), 0, s, x, ws, C, T, H, W, S, vflip);
        hipLaunchKernelGGL((tlfm_export_kernel<IT, false>), dim3(nall), dim3(256), 0, s, x, bf_range, out, ws, B, C, T, H, W, S,
                           vflip, bf_normalise, low1, div1, low2, div2);
    }
}

extern "C" int msg_tlfm_export(const void* x, int dtype, const int* bf_range, unsigned short* out, int B, int C, int T, int H,
                               int W, int vflip, int bf_normalise, float low1, float div1, float low2, float div2, float* ws,
                               void* stream) {
    if (B <= 0 || C <= 0 || C > 3 || T <= 0 || H <= 0 || W <= 0 || !x || !bf_range || !out) return MSG_EINVAL;
    if (bf_normalise && !ws) return MSG_EINVAL;
    if (dtype != MSG_F32 && dtype != MSG_BF16) return MSG_EINVAL;
    if ((long long)B * C * T * TLFM_EXPORT_MAX_SPLIT > 0x7fffffffll) return MSG_EINVAL;   // (one block index per frame and split)
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MSG_BF16)
        tlfm_export_launch<bf16_t>((const bf16_t*)x, bf_range, out, B, C, T, H, W, vflip, bf_normalise != 0, low1, div1, low2,
                                   div2, ws, s);
    else
        tlfm_export_launch<float>((const float*)x, bf_range, out, B, C, T, H, W, vflip, bf_normalise != 0, low1, div1, low2, div2,
                                  ws, s);
    return MSG_CHECK_LAUNCH();
}
