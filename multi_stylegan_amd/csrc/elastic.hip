// Elastic deformation of a batch of frames [B, F, H, W]: the dataset's augmentation (dataset/tlfm_dataset.py:230-275) for a
// whole batch on the device.  The reference convolves two planes of uniform noise with a dense (4 sigma + 1)^2 Gaussian
// (truncated at +-2 sigma, not renormalised, zero padding), scales by alpha, adds the result to the pixel grid and resamples
// every frame of the sample bilinearly with border padding (grid_sample, align_corners=False).  Its 2-D kernel is exactly
// g (x) g, so the blur is done separably here: 2 (4 sigma + 1) taps per field value instead of (4 sigma + 1)^2.
//
// Two launches per call:
//   1. elastic_row_kernel         the row pass, noise -> ws [B, 2, H, W]: a workgroup stages 4 rows x (256 + 4 sigma) columns in
//                                 LDS (noise outside the frame is zero on the load side) and every lane keeps 4 adjacent sums,
//                                 16 multiply-adds per two 16-byte LDS reads;
//   2. elastic_col_gather_kernel  a 32 x 64 tile per workgroup: the column pass over ws (a +-2 sigma halo of rows in LDS, rows
//                                 outside the frame zero; one component after the other through the same buffer) leaves the
//                                 field values of a lane's pixels in registers; they are written to `field` and turned into four
//                                 offsets and four weights per pixel ONCE, which the loop over the sample's F frames reuses.
//                                 A lane owns 16 bytes of adjacent output pixels (4 fp32, 8 bf16): 16-byte stores; the gathers of
//                                 neighbouring lanes fall into neighbouring lines because the field is smooth.
// The taps are computed once per call on the host (double, rounded to fp32) and travel as a kernel argument.
// No atomics, no dependence on workgroup order, a sample's values depend on that sample alone: bit-identical from run to run
// and from batch to batch.  The position arithmetic is written with explicitly rounded operations so that the vector and the
// scalar instantiations (and any compiler's contraction choices) give the same bits.
#include <math.h>
#include "msg_common.h"

constexpr int EL_MAX_TAPS = 4 * MSG_ELASTIC_MAX_SIGMA + 4;       // 4 sigma + 1 taps, padded with zeros to a multiple of 4
constexpr int EL_ROW_W = 256, EL_ROW_R = 4;                      // row pass: output columns and rows per workgroup
constexpr int EL_ROW_PITCH = EL_ROW_W + EL_MAX_TAPS;             // staged columns per row: 256 + 4 sigma + 4 are used
constexpr int EL_TX = 64, EL_TY = 32;                            // column pass + gather: the output tile

struct ElasticTaps { float g[EL_MAX_TAPS]; };

// grid: (plane = b * 2 + component, block of 4 rows, block of 256 columns), flat
__global__ __launch_bounds__(256) void elastic_row_kernel(const float* __restrict__ noise, float* __restrict__ tmp,
                                                          ElasticTaps taps, int H, int W, int sigma, int row_blocks,
                                                          int col_blocks) {
    __shared__ __attribute__((aligned(16))) float s_g[EL_MAX_TAPS];
    __shared__ __attribute__((aligned(16))) float s_row[EL_ROW_R][EL_ROW_PITCH];
    const int tid = threadIdx.x, k4 = 4 * sigma + 4, halo = 2 * sigma, used = EL_ROW_W + 4 * sigma;
    unsigned n = blockIdx.x;
    const int cb = (int)(n % (unsigned)col_blocks);
    n /= (unsigned)col_blocks;
    const int rb = (int)(n % (unsigned)row_blocks);
    const long long plane = n / (unsigned)row_blocks;
    const int c0 = cb * EL_ROW_W, r0 = rb * EL_ROW_R;
    const float* src = noise + plane * H * W;
    if (tid < k4) s_g[tid] = taps.g[tid];
    for (int idx = tid; idx < EL_ROW_R * (used + 4); idx += 256) {
        const int r = idx / (used + 4), j = idx - r * (used + 4);
        const int y = r0 + r, x = c0 + j - halo;
        s_row[r][j] = (j < used && y < H && x >= 0 && x < W) ? src[(long long)y * W + x] : 0.f;
    }
    __syncthreads();
    const int r = tid >> 6, xs = (tid & 63) * 4;
    const float4* row = reinterpret_cast<const float4*>(&s_row[r][xs]);
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float4 lo = row[0];
    for (int i = 0; i < k4; i += 4) {                            // taps i .. i + 3 on the window s_row[r][xs + i .. xs + i + 7]
        const float4 hi = row[(i >> 2) + 1];
        const float4 g = *reinterpret_cast<const float4*>(&s_g[i]);
        const float win[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        const float gk[4] = {g.x, g.y, g.z, g.w};
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = fmaf(gk[k], win[e + k], acc[e]);
        lo = hi;
    }
    const int y = r0 + r, x = c0 + xs;
    if (y < H) {
        float* dst = tmp + plane * H * W + (long long)y * W + x;
        if (x + 3 < W && (((uintptr_t)dst) & 15u) == 0) {
            *reinterpret_cast<float4*>(dst) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < W) dst[e] = acc[e];
        }
    }
}

// The sampling position of grid_sample(padding_mode='border', align_corners=False) for the reference's grid, one axis:
// g = 2 (p + d - half) / den;  pos = ((g + 1) size - 1) / 2, clamped to [0, size - 1].  The reference divides the x coordinate
// by the HEIGHT and the y coordinate by the width (dataset/tlfm_dataset.py:269-270): `den` / `half` are the caller's.
__device__ __forceinline__ float elastic_position(int p, float d, float half, float den, float size) {
    const float g = __fdiv_rn(__fmul_rn(2.f, __fsub_rn(__fadd_rn((float)p, d), half)), den);
    const float pos = __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(g, 1.f), size), 1.f), 0.5f);
    return fminf(fmaxf(pos, 0.f), size - 1.f);                   // (a NaN position becomes 0: every index stays in the frame)
}

// grid: (sample, tile row, tile column), flat.  VEC: W a multiple of the lane's pixels and 16-byte aligned bases.
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void elastic_col_gather_kernel(const T* __restrict__ in, const float* __restrict__ tmp,
                                                                 float* __restrict__ field, T* __restrict__ out,
                                                                 ElasticTaps taps, int F, int H, int W, int sigma, float alpha,
                                                                 int tiles_y, int tiles_x) {
    constexpr int NPX = 16 / (int)sizeof(T);                     // adjacent pixels per lane: 4 (fp32) or 8 (bf16)
    constexpr int TPR = EL_TX / NPX;                             // lanes per tile row
    constexpr int RSTEP = 256 / TPR;                             // tile rows covered by one sweep of the workgroup
    constexpr int NROW = EL_TY / RSTEP;                          // rows per lane: 2 (fp32) or 1 (bf16)
    extern __shared__ __attribute__((aligned(16))) float s_tile[];   // [EL_TY + 4 sigma][EL_TX]
    __shared__ float s_g[EL_MAX_TAPS];
    const int tid = threadIdx.x, K = 4 * sigma + 1, halo = 2 * sigma, rows = EL_TY + 4 * sigma;
    unsigned n = blockIdx.x;
    const int tx = (int)(n % (unsigned)tiles_x);
    n /= (unsigned)tiles_x;
    const int ty = (int)(n % (unsigned)tiles_y);
    const long long b = n / (unsigned)tiles_y;
    const int x0 = tx * EL_TX, y0 = ty * EL_TY;
    const int cx = (tid % TPR) * NPX, rg = tid / TPR;
    const long long P = (long long)H * W;
    if (tid < K) s_g[tid] = taps.g[tid];

    float d[2][NROW][NPX];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const float* src = tmp + (b * 2 + c) * P;
        __syncthreads();                                         // the previous component's reads of s_tile are done
        for (int idx = tid; idx < rows * EL_TX; idx += 256) {
            const int j = idx / EL_TX, i = idx - j * EL_TX;
            const int gy = y0 + j - halo, gx = x0 + i;
            s_tile[idx] = (gy >= 0 && gy < H && gx < W) ? src[(long long)gy * W + gx] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NROW; ++r) {
            const int ry = rg + r * RSTEP;
            float acc[NPX];
#pragma unroll
            for (int e = 0; e < NPX; ++e) acc[e] = 0.f;
            for (int i = 0; i < K; ++i) {
                const float g = s_g[i];
                const float4* p = reinterpret_cast<const float4*>(&s_tile[(ry + i) * EL_TX + cx]);
#pragma unroll
                for (int q = 0; q < NPX / 4; ++q) {
                    const float4 v = p[q];
                    acc[4 * q + 0] = fmaf(g, v.x, acc[4 * q + 0]);
                    acc[4 * q + 1] = fmaf(g, v.y, acc[4 * q + 1]);
                    acc[4 * q + 2] = fmaf(g, v.z, acc[4 * q + 2]);
                    acc[4 * q + 3] = fmaf(g, v.w, acc[4 * q + 3]);
                }
            }
#pragma unroll
            for (int e = 0; e < NPX; ++e) d[c][r][e] = __fmul_rn(acc[e], alpha);
            const int y = y0 + ry, x = x0 + cx;
            if (y < H && x < W) {
                float* dst = field + (b * 2 + c) * P + (long long)y * W + x;
                if constexpr (VEC) {
#pragma unroll
                    for (int q = 0; q < NPX / 4; ++q)
                        *reinterpret_cast<float4*>(dst + 4 * q) =
                            make_float4(d[c][r][4 * q], d[c][r][4 * q + 1], d[c][r][4 * q + 2], d[c][r][4 * q + 3]);
                } else {
#pragma unroll
                    for (int e = 0; e < NPX; ++e)
                        if (x + e < W) dst[e] = d[c][r][e];
                }
            }
        }
    }

    const float fH = (float)H, fW = (float)W, half_h = (float)(H / 2), half_w = (float)(W / 2);
#pragma unroll
    for (int r = 0; r < NROW; ++r) {
        const int y = y0 + rg + r * RSTEP, x = x0 + cx;
        if (y >= H || x >= W) continue;
        int o[NPX][4];
        float w[NPX][4];
#pragma unroll
        for (int e = 0; e < NPX; ++e) {
            const float px = elastic_position(x + e, d[0][r][e], half_h, fH, fW);
            const float py = elastic_position(y, d[1][r][e], half_w, fW, fH);
            const float flx = floorf(px), fly = floorf(py);
            const int ix0 = min(max((int)flx, 0), W - 1), iy0 = min(max((int)fly, 0), H - 1);
            const int ix1 = min(ix0 + 1, W - 1), iy1 = min(iy0 + 1, H - 1);
            const float ax = __fsub_rn(px, flx), ay = __fsub_rn(py, fly);                       // weights of the upper index
            const float bx = __fsub_rn(__fadd_rn(flx, 1.f), px), by = __fsub_rn(__fadd_rn(fly, 1.f), py);
            o[e][0] = iy0 * W + ix0; o[e][1] = iy0 * W + ix1; o[e][2] = iy1 * W + ix0; o[e][3] = iy1 * W + ix1;
            w[e][0] = __fmul_rn(bx, by); w[e][1] = __fmul_rn(ax, by); w[e][2] = __fmul_rn(bx, ay); w[e][3] = __fmul_rn(ax, ay);
        }
        const long long at = (long long)y * W + x;
        for (int f = 0; f < F; ++f) {
            const T* src = in + (b * F + f) * P;
            T* dst = out + (b * F + f) * P + at;
            float v[NPX];
#pragma unroll
            for (int e = 0; e < NPX; ++e) {
                float s = __fmul_rn(load_as_f32<T>(src + o[e][0]), w[e][0]);
                s = fmaf(load_as_f32<T>(src + o[e][1]), w[e][1], s);
                s = fmaf(load_as_f32<T>(src + o[e][2]), w[e][2], s);
                v[e] = fmaf(load_as_f32<T>(src + o[e][3]), w[e][3], s);
            }
            if constexpr (!VEC) {
#pragma unroll
                for (int e = 0; e < NPX; ++e)
                    if (x + e < W) store_from_f32<T>(dst + e, v[e]);
            } else if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                Vec16<bf16_t> pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk.set2(e, v[2 * e], v[2 * e + 1]);
                *reinterpret_cast<uint4*>(dst) = pk.raw;
            }
        }
    }
}

extern "C" long long msg_elastic_workspace(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return 8ll * B * H * W;                                      // the row pass's output: one more [B, 2, H, W] fp32 array
}

template <typename T>
static void elastic_launch(const T* in, const float* tmp, float* field, T* out, const ElasticTaps& taps, int B, int F, int H,
                           int W, int sigma, float alpha, hipStream_t s) {
    constexpr int NPX = 16 / (int)sizeof(T);
    const int tiles_y = (H + EL_TY - 1) / EL_TY, tiles_x = (W + EL_TX - 1) / EL_TX;
    const unsigned grid = (unsigned)((long long)B * tiles_y * tiles_x);
    const size_t lds = (size_t)(EL_TY + 4 * sigma) * EL_TX * sizeof(float);
    const bool vec = W % NPX == 0 && ((((uintptr_t)in) | ((uintptr_t)out) | ((uintptr_t)field)) & 15u) == 0;
    if (vec)
        hipLaunchKernelGGL((elastic_col_gather_kernel<T, true>), dim3(grid), dim3(256), lds, s, in, tmp, field, out, taps, F, H, W,
                           sigma, alpha, tiles_y, tiles_x);
    else
        hipLaunchKernelGGL((elastic_col_gather_kernel<T, false>), dim3(grid), dim3(256), lds, s, in, tmp, field, out, taps, F, H, W,
                           sigma, alpha, tiles_y, tiles_x);
}

extern "C" int msg_elastic_deform(const void* in, const float* noise, float* field, void* out, int dtype, int B, int F, int H,
                                  int W, int sigma, float alpha, void* ws, void* stream) {
    if (!in || !noise || !field || !out || !ws || B <= 0 || F <= 0 || H <= 0 || W <= 0 || sigma < 1) return MSG_EINVAL;
    if (dtype != MSG_F32 && dtype != MSG_BF16) return MSG_EUNSUPPORTED;
    if (sigma > MSG_ELASTIC_MAX_SIGMA) return MSG_EUNSUPPORTED;
    const int row_blocks = (H + EL_ROW_R - 1) / EL_ROW_R, col_blocks = (W + EL_ROW_W - 1) / EL_ROW_W;
    const long long row_grid = 2ll * B * row_blocks * col_blocks;
    // (offsets inside a frame are 32-bit; one block index per 4 x 256 piece of a plane)
    if ((long long)H * W > 0x7fffffffll || row_grid > 0x7fffffffll) return MSG_EINVAL;
    ElasticTaps taps;
    const double s2 = 2.0 * sigma * sigma, norm = 1.0 / (sqrt(2.0 * M_PI) * sigma);
    for (int i = 0; i < EL_MAX_TAPS; ++i) {
        const double t = i - 2.0 * sigma;
        taps.g[i] = i <= 4 * sigma ? (float)(exp(-t * t / s2) * norm) : 0.f;
    }
    hipStream_t s = (hipStream_t)stream;
    float* tmp = (float*)ws;
    hipLaunchKernelGGL(elastic_row_kernel, dim3((unsigned)row_grid), dim3(256), 0, s, noise, tmp, taps, H, W, sigma, row_blocks,
                       col_blocks);
    if (dtype == MSG_BF16)
        elastic_launch<bf16_t>((const bf16_t*)in, tmp, field, (bf16_t*)out, taps, B, F, H, W, sigma, alpha, s);
    else
        elastic_launch<float>((const float*)in, tmp, field, (float*)out, taps, B, F, H, W, sigma, alpha, s);
    return MSG_CHECK_LAUNCH();
}
