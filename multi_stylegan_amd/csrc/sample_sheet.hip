// Sample output: a generated batch [B, C, T, H, W] (fp32 / bf16) -> the 8-bit RGB pictures the reference writes with
// torchvision.utils.save_image, composed in one pass.  The reference builds each picture as a chain of elementwise passes
// (repeat_interleave to three planes, two zero fills, cat, permute), copies the fp32 planes to the host and quantises there:
// multi_stylegan/misc.py:132-166 (Logger.save_prediction), scripts/get_gan_samples.py:44-60,
// scripts/gan_latent_space_interpolation.py:46-59.
//
// out is [B, C, H, T*W, 3] bytes.  Read as [B, C] sheets of H x (T*W) it holds a sequence's frames side by side
// (save_image(nrow=T, padding=0)); read as [B] pictures of (C*H) x (T*W) it holds the channels stacked top to bottom (the
// interpolation frame) -- the same memory.  Channel c is written to the colour planes its three tint bits name, 0 elsewhere.
//
// Arithmetic (torchvision's save_image with normalize=False): q = (uint8) trunc(min(max(fl(fl(x * 255) + 0.5), 0), 255)) in
// fp32, the multiply and the add rounded separately (no FMA); NaN -> 0, +inf -> 255, -inf -> 0.
//
// In output order a row of the whole batch (B*C*H of them) is T segments of W pixels, so the k-th group of 16 output pixels
// starts at byte 48 k: the vector path (W % 16 == 0, 16-byte aligned bases) gives a lane one group -- four 16-byte loads (two
// for bf16), three 16-byte stores -- and the grid is flat over groups, so one sample fills the chip as well as 32 do.  Anything
// else takes the scalar path, one pixel per lane, with the same arithmetic.  No LDS, no workspace, one launch.
#include "msg_common.h"

__device__ __forceinline__ unsigned int sheet_quantise(float x) {
#pragma clang fp contract(off)
    float v = x * 255.0f;
    v = v + 0.5f;
    v = v > 0.0f ? v : 0.0f;                        // NaN -> 0
    v = v < 255.0f ? v : 255.0f;
    return (unsigned int)v;                         // truncation
}

// bit 0 of a channel's tint -> byte 0 (red), bit 1 -> byte 1, bit 2 -> byte 2: the mask of one RGB pixel in its low 24 bits
__device__ __forceinline__ unsigned int sheet_tint_mask(int tints, int c) {
    const unsigned int t = ((unsigned int)tints >> (3 * c)) & 7u;
    return ((t & 1u) ? 0xffu : 0u) | ((t & 2u) ? 0xff00u : 0u) | ((t & 4u) ? 0xff0000u : 0u);
}

// item i = (row r of B*C*H, frame t, group g of W / 16): reads seq[((r / H) * T + t) * H + r % H][16 g ..], writes out[48 i ..]
template <typename T>
__global__ __launch_bounds__(256) void sample_sheet_vec_kernel(const T* __restrict__ seq, unsigned char* __restrict__ out, int C,
                                                               int Tn, int H, int W, int tints, long long items) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const int wv = W >> 4;
    const long long rt = i / wv;
    const int g = (int)(i - rt * wv);
    const long long r = rt / Tn;
    const int t = (int)(rt - r * Tn);
    const long long sheet = r / H;
    const int h = (int)(r - sheet * H);
    const unsigned int mask = sheet_tint_mask(tints, (int)(sheet % C));
    const T* src = seq + (((sheet * Tn + t) * H + h) * W + 16ll * g);
    constexpr int N = Vec16<T>::N;
    unsigned int q[16];
#pragma unroll
    for (int k = 0; k < 16 / N; ++k) {
        Vec16<T> v;
        v.raw = *reinterpret_cast<const uint4*>(src + k * N);
#pragma unroll
        for (int e = 0; e < N; ++e) q[k * N + e] = sheet_quantise(v.get(e));
    }
    // 16 pixels x 3 bytes = 12 words; pixel p occupies bytes 3 p .. 3 p + 2
    unsigned int w[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned int p0 = (q[4 * k] * 0x010101u) & mask, p1 = (q[4 * k + 1] * 0x010101u) & mask;
        const unsigned int p2 = (q[4 * k + 2] * 0x010101u) & mask, p3 = (q[4 * k + 3] * 0x010101u) & mask;
        w[3 * k] = p0 | (p1 << 24);
        w[3 * k + 1] = (p1 >> 8) | (p2 << 16);
        w[3 * k + 2] = (p2 >> 16) | (p3 << 8);
    }
    // (written once and read next by a copy engine: non-temporal, which also keeps the three 16-byte stores as they are)
    u32x4* dst = reinterpret_cast<u32x4*>(out + 48ll * i);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        u32x4 v;
        v[0] = w[4 * k]; v[1] = w[4 * k + 1]; v[2] = w[4 * k + 2]; v[3] = w[4 * k + 3];
        __builtin_nontemporal_store(v, dst + k);
    }
}

// item i = one output pixel (row r, frame t, column x), three byte stores
template <typename T>
__global__ __launch_bounds__(256) void sample_sheet_scalar_kernel(const T* __restrict__ seq, unsigned char* __restrict__ out,
                                                                  int C, int Tn, int H, int W, int tints, long long items) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= items) return;
    const long long rt = i / W;
    const int x = (int)(i - rt * W);
    const long long r = rt / Tn;
    const int t = (int)(rt - r * Tn);
    const long long sheet = r / H;
    const int h = (int)(r - sheet * H);
    const unsigned int mask = sheet_tint_mask(tints, (int)(sheet % C));
    const unsigned int p = (sheet_quantise(load_as_f32<T>(seq + (((sheet * Tn + t) * H + h) * W + x))) * 0x010101u) & mask;
    unsigned char* dst = out + 3 * i;
    dst[0] = (unsigned char)(p & 0xffu);
    dst[1] = (unsigned char)((p >> 8) & 0xffu);
    dst[2] = (unsigned char)(p >> 16);
}

template <typename T>
static int sample_sheet_launch(const T* seq, unsigned char* out, int C, int Tn, int H, int W, int tints, long long pixels,
                               hipStream_t s) {
    const bool vec = W % 16 == 0 && ((((uintptr_t)seq) | ((uintptr_t)out)) & 15u) == 0;
    const long long items = vec ? pixels / 16 : pixels;
    const long long blocks = (items + 255) / 256;
    if (blocks > 0x7fffffffll) return MSG_EINVAL;                          // (what blockIdx.x can address)
    if (vec)
        hipLaunchKernelGGL((sample_sheet_vec_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, seq, out, C, Tn, H, W, tints,
                           items);
    else
        hipLaunchKernelGGL((sample_sheet_scalar_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, s, seq, out, C, Tn, H, W,
                           tints, items);
    return MSG_CHECK_LAUNCH();
}

extern "C" int msg_sample_sheet(const void* seq, unsigned char* out, int dtype, int B, int C, int T, int H, int W, int tints,
                                void* stream) {
    if (B <= 0 || C <= 0 || C > 3 || T <= 0 || H <= 0 || W <= 0 || !seq || !out) return MSG_EINVAL;
    if (dtype != MSG_F32 && dtype != MSG_BF16) return MSG_EINVAL;
    if (tints < 0 || (tints >> (3 * C)) != 0) return MSG_EINVAL;           // bits above 3 C - 1
    if ((double)B * C * T * H * W > 4.0e18) return MSG_EINVAL;             // (the 64-bit counts below must not wrap)
    const long long pixels = (long long)B * C * T * H * W;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == MSG_BF16) return sample_sheet_launch<bf16_t>((const bf16_t*)seq, out, C, T, H, W, tints, pixels, s);
    return sample_sheet_launch<float>((const float*)seq, out, C, T, H, W, tints, pixels, s);
}
