// Sliced Wasserstein distance over Laplacian-pyramid patches (validation_metrics.py: SWD / SWVD): the
// pyramid level, the patch gather, the per-plane statistics, the projection with the normalisation folded in, and the L1
// distance of two sorted projections.  The sort between the last two is torch.sort.
//
// msg_laplacian_level   one workgroup per 32 x 64 tile of the fine plane.  The tile's source patch (39 x 71, mirrored at the
//   plane's borders) is loaded once into LDS; the 5-tap row pass and column pass of down() give the tile's 16 x 32 coarse values
//   and a one-sample halo of them (18 x 34, recomputed by the neighbouring workgroups with the same bits: the taps are folded in
//   symmetric pairs, so that a mirrored halo value is the interior value it mirrors); up() is a 3 / 2-tap row pass and column pass
//   over those, and lap = fine - up(coarse) is stored from the patch already in LDS.
// msg_swd_gather        a flat copy: lane q forms four consecutive elements of the [B K, P 49] descriptor matrix.
// msg_swd_plane_sums    256 rows per workgroup, a fixed assignment of elements to lanes, a fixed tree in LDS, partials merged in
//   index order by a second launch.
// msg_swd_project       the main loop of feature_pairs.hip with the directions as the A operand and the descriptor rows as
//   the B operand of __builtin_amdgcn_mfma_f32_32x32x2f32: in the C/D layout a lane's column is then one ROW i and its
//   registers run along the directions, so every store instruction writes 32 consecutive i of one direction -- one full
//   128-byte line of the direction-major [R, n] output per half wave.  The rows are normalised while they are staged.
// msg_sorted_l1         4096 elements of one direction per workgroup, merged like the plane sums.
// No atomics anywhere: every output is bit-identical from run to run.
#include <limits.h>
#include "msg_common.h"

// ------------------------------------------------------------------------------------------------------ Laplacian level
constexpr int LP_TH = 32, LP_TW = 64;                 // fine tile of one workgroup
constexpr int LP_PH = LP_TH + 7;                      // patch rows: 4 above (the halo's coarse row reads 2 x (-1) - 2), 3 below
constexpr int LP_PW = LP_TW + 8;                      // patch columns: 71 used, loaded as 18 groups of four
constexpr int LP_CH = LP_TH / 2 + 2, LP_CW = LP_TW / 2 + 2;   // coarse tile with its halo
constexpr int LP_CLD = LP_CW + 1;

// "mirror": -1 reads 1, n reads n - 2; the clamp only keeps the unused part of a partial tile's patch inside the plane
__device__ __forceinline__ int lp_mirror(int v, int n) {
    v = v < 0 ? -v : v;
    v = v >= n ? 2 * (n - 1) - v : v;
    return min(max(v, 0), n - 1);
}

// f = [1 4 6 4 1] / 16 on five samples: the outer pair, then the inner pair, then the centre; the scalings by 1/16 and 1/4
// are exact, so a value meets at most three roundings (its pair's sum and two fused multiply-adds)
__device__ __forceinline__ float lp_down5(float a, float b, float c, float d, float e) {
    return fmaf(0.375f, c, fmaf(0.25f, __fadd_rn(b, d), __fmul_rn(0.0625f, __fadd_rn(a, e))));
}
// 2 f on the zero-stuffed samples: an even position sees [1 6 1] / 8 (two roundings), an odd one [1 1] / 2 (one)
__device__ __forceinline__ float lp_up_even(float l, float c, float r) {
    return fmaf(0.75f, c, __fmul_rn(0.125f, __fadd_rn(l, r)));
}
__device__ __forceinline__ float lp_up_odd(float c, float r) { return __fmul_rn(0.5f, __fadd_rn(c, r)); }

template <bool VEC>
__global__ __launch_bounds__(256) void laplacian_level_kernel(const float* fine, float* coarse, float* lap, int h, int w,
                                                              int tiles_x, int tiles_y) {
    __shared__ __attribute__((aligned(16))) float sF[LP_PH * LP_PW];
    __shared__ float sH[LP_PH * LP_CW];
    __shared__ float sC[LP_CH * LP_CLD];
    __shared__ float sU[LP_CH * LP_TW];
    const int t = threadIdx.x;
    long long tile = blockIdx.x;
    const int tx = (int)(tile % tiles_x);
    tile /= tiles_x;
    const int ty = (int)(tile % tiles_y);
    const long long m = tile / tiles_y;
    const int y0 = ty * LP_TH, x0 = tx * LP_TW, hc = h >> 1, wc = w >> 1;
    const float* src = fine + m * (long long)h * w;

    // the patch: row py is fine row y0 - 4 + py, column px is fine column x0 - 4 + px, both mirrored
    for (int g = t; g < LP_PH * (LP_PW / 4); g += 256) {
        const int py = g / (LP_PW / 4), gx = g - py * (LP_PW / 4);
        const int xv = x0 - 4 + 4 * gx;
        const float* row = src + (long long)lp_mirror(y0 - 4 + py, h) * w;
        f32x4 v;
        if (VEC && xv >= 0 && xv + 3 < w) {
            v = *reinterpret_cast<const f32x4*>(row + xv);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = row[lp_mirror(xv + e, w)];
        }
        *reinterpret_cast<f32x4*>(sF + py * LP_PW + 4 * gx) = v;
    }
    __syncthreads();
    // down(), row pass: coarse column cx of the tile (cx = 0 and LP_CW - 1: the halo) is centred on patch column 2 cx + 2
    for (int i = t; i < LP_PH * LP_CW; i += 256) {
        const int py = i / LP_CW, cx = i - py * LP_CW;
        const float* p = sF + py * LP_PW + 2 * cx;
        sH[i] = lp_down5(p[0], p[1], p[2], p[3], p[4]);
    }
    __syncthreads();
    // down(), column pass: coarse row cy is centred on patch row 2 cy + 2
    for (int i = t; i < LP_CH * LP_CW; i += 256) {
        const int cy = i / LP_CW, cx = i - cy * LP_CW;
        const float* p = sH + (2 * cy) * LP_CW + cx;
        const float v = lp_down5(p[0], p[LP_CW], p[2 * LP_CW], p[3 * LP_CW], p[4 * LP_CW]);
        sC[cy * LP_CLD + cx] = v;
        const int gy = (y0 >> 1) + cy - 1, gx = (x0 >> 1) + cx - 1;
        if (cy >= 1 && cy <= LP_TH / 2 && cx >= 1 && cx <= LP_TW / 2 && gy < hc && gx < wc)
            coarse[m * (long long)hc * wc + (long long)gy * wc + gx] = v;
    }
    if (!lap) return;
    __syncthreads();
    // up(), row pass: fine column lx of the tile sits on coarse column lx / 2 (+ 1 for the halo)
    for (int i = t; i < LP_CH * LP_TW; i += 256) {
        const int cy = i / LP_TW, lx = i - cy * LP_TW;
        const float* c = sC + cy * LP_CLD + (lx >> 1) + 1;
        sU[i] = (lx & 1) ? lp_up_odd(c[0], c[1]) : lp_up_even(c[-1], c[0], c[1]);
    }
    __syncthreads();
    // up(), column pass, and the difference: four columns per lane
    for (int g = t; g < LP_TH * (LP_TW / 4); g += 256) {
        const int ly = g / (LP_TW / 4), lx = 4 * (g - ly * (LP_TW / 4));
        const int y = y0 + ly, x = x0 + lx;
        if (y >= h || x >= w) continue;
        const float* u = sU + ((ly >> 1) + 1) * LP_TW + lx;
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float up = (ly & 1) ? lp_up_odd(u[e], u[e + LP_TW]) : lp_up_even(u[e - LP_TW], u[e], u[e + LP_TW]);
            o[e] = __fsub_rn(sF[(ly + 4) * LP_PW + lx + 4 + e], up);
        }
        float* dst = lap + m * (long long)h * w + (long long)y * w + x;
        if (VEC) {
            *reinterpret_cast<f32x4*>(dst) = o;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (x + e < w) dst[e] = o[e];
        }
    }
}

extern "C" int msg_laplacian_level(const float* fine, int M, int h, int w, float* coarse, float* lap, void* stream) {
    if (!fine || !coarse) return MSG_EINVAL;
    if (M <= 0 || h < 8 || w < 8 || (h & 1) || (w & 1)) return MSG_EINVAL;
    if ((((uintptr_t)fine) | ((uintptr_t)coarse) | ((uintptr_t)lap)) & 3u) return MSG_EINVAL;
    const int tiles_x = (w + LP_TW - 1) / LP_TW, tiles_y = (h + LP_TH - 1) / LP_TH;
    const long long tiles = (long long)M * tiles_x * tiles_y;
    if (tiles > INT_MAX) return MSG_EINVAL;
    const bool vec = w % 4 == 0 && ((((uintptr_t)fine) | ((uintptr_t)lap)) & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((laplacian_level_kernel<true>), dim3((unsigned)tiles), dim3(256), 0, s, fine, coarse, lap, h, w, tiles_x, tiles_y);
    else     hipLaunchKernelGGL((laplacian_level_kernel<false>), dim3((unsigned)tiles), dim3(256), 0, s, fine, coarse, lap, h, w, tiles_x, tiles_y);
    return MSG_CHECK_LAUNCH();
}

// --------------------------------------------------------------------------------------------------------------- gather
template <bool VEC>
__global__ __launch_bounds__(256) void swd_gather_kernel(const float* level, const int* pos, float* rows, int P, int h, int w,
                                                         int K, long long total) {
    const long long q = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (q >= total) return;
    const int d = P * 49;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const long long f = q + e;
        float x = 0.f;
        if (f < total) {
            const long long row = f / d;
            const int j = (int)(f - row * d), p = j / 49, r = j - p * 49, dy = r / 7, dx = r - dy * 7;
            const long long y = (long long)pos[2 * row] - 3 + dy, xx = (long long)pos[2 * row + 1] - 3 + dx;
            if (y >= 0 && y < h && xx >= 0 && xx < w) x = level[(((row / K) * P + p) * h + y) * w + xx];
        }
        v[e] = x;
    }
    if (VEC && q + 4 <= total) {
        *reinterpret_cast<f32x4*>(rows + q) = v;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q + e < total) rows[q + e] = v[e];
    }
}

extern "C" int msg_swd_gather(const float* level, int B, int P, int h, int w, const int* pos, int K, float* rows, void* stream) {
    if (!level || !pos || !rows) return MSG_EINVAL;
    if (B <= 0 || P <= 0 || h <= 0 || w <= 0 || K <= 0 || P > INT_MAX / 49) return MSG_EINVAL;
    if ((((uintptr_t)level) | ((uintptr_t)pos) | ((uintptr_t)rows)) & 3u) return MSG_EINVAL;
    const long long total = (long long)B * K * P * 49;
    const long long blocks = (total + 1023) / 1024;
    if ((long long)B * K > INT_MAX || blocks > INT_MAX) return MSG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if ((((uintptr_t)rows) & 15u) == 0)
        hipLaunchKernelGGL((swd_gather_kernel<true>), dim3((unsigned)blocks), dim3(256), 0, s, level, pos, rows, P, h, w, K, total);
    else
        hipLaunchKernelGGL((swd_gather_kernel<false>), dim3((unsigned)blocks), dim3(256), 0, s, level, pos, rows, P, h, w, K, total);
    return MSG_CHECK_LAUNCH();
}

// ------------------------------------------------------------------------------------------- fixed-order float64 sums
// the workgroup's 256 lane sums through a fixed tree; the result is in sd[0]
__device__ __forceinline__ void swd_tree(double* sd, int t, double v) {
    sd[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) sd[t] += sd[t + s];
        __syncthreads();
    }
}

// out[o] = sum_i ws[o * stride_o + i * stride_i], i ascending
__global__ void swd_merge_kernel(const double* ws, double* out, int outs, long long parts, long long stride_o, long long stride_i) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= outs) return;
    const double* src = ws + o * stride_o;
    double s = 0.0;
    for (long long i = 0; i < parts; ++i) s += src[i * stride_i];
    out[o] = s;
}

constexpr int PS_ROWS = 256;                          // descriptor rows per workgroup

__global__ __launch_bounds__(256) void swd_plane_sums_kernel(const float* rows, int n, int P, double* ws) {
    __shared__ double sd[256];
    const int t = threadIdx.x;
    const long long r0 = (long long)blockIdx.x * PS_ROWS;
    const int nr = (int)min((long long)PS_ROWS, n - r0);
    const long long d = (long long)P * 49;
    for (int p = 0; p < P; ++p) {
        double a = 0.0, b = 0.0;
        for (int q = t; q < nr * 49; q += 256) {
            const int r = q / 49, e = q - r * 49;
            const double x = (double)rows[(r0 + r) * d + p * 49 + e];
            a += x;
            b += x * x;
        }
        swd_tree(sd, t, a);
        if (t == 0) ws[((long long)blockIdx.x * P + p) * 2] = sd[0];
        __syncthreads();
        swd_tree(sd, t, b);
        if (t == 0) ws[((long long)blockIdx.x * P + p) * 2 + 1] = sd[0];
        __syncthreads();
    }
}

extern "C" long long msg_swd_plane_sums_workspace(int n, int P) {
    if (n <= 0 || P <= 0 || P > INT_MAX / 98) return -1;
    return 16ll * P * ((n + PS_ROWS - 1) / PS_ROWS);
}

extern "C" int msg_swd_plane_sums(const float* rows, int n, int P, double* sums, void* ws, void* stream) {
    if (!rows || !sums || !ws) return MSG_EINVAL;
    if (msg_swd_plane_sums_workspace(n, P) < 0) return MSG_EINVAL;
    if ((((uintptr_t)rows) & 3u) || ((((uintptr_t)sums) | ((uintptr_t)ws)) & 7u)) return MSG_EINVAL;
    const int blocks = (n + PS_ROWS - 1) / PS_ROWS;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(swd_plane_sums_kernel, dim3((unsigned)blocks), dim3(256), 0, s, rows, n, P, (double*)ws);
    hipLaunchKernelGGL(swd_merge_kernel, dim3((unsigned)((2 * P + 63) / 64)), dim3(64), 0, s, (const double*)ws, sums, 2 * P,
                       (long long)blocks, 1ll, 2ll * P);
    return MSG_CHECK_LAUNCH();
}

// ----------------------------------------------------------------------------------------------------------- sorted L1
constexpr int L1_CHUNK = 4096;                        // elements of one direction per workgroup: 256 lanes x 4 x 4

template <bool VEC>
__global__ __launch_bounds__(256) void sorted_l1_kernel(const float* a, const float* b, int n, int chunks, double* ws) {
    __shared__ double sd[256];
    const int t = threadIdx.x, r = blockIdx.y;
    const float* pa = a + (long long)r * n;
    const float* pb = b + (long long)r * n;
    double acc = 0.0;
#pragma unroll
    for (int it = 0; it < L1_CHUNK / 1024; ++it) {
        const long long i = (long long)blockIdx.x * L1_CHUNK + (it * 256 + t) * 4;
        if (i >= n) continue;
        f32x4 xa = {0.f, 0.f, 0.f, 0.f}, xb = {0.f, 0.f, 0.f, 0.f};
        if (VEC) {
            xa = *reinterpret_cast<const f32x4*>(pa + i);
            xb = *reinterpret_cast<const f32x4*>(pb + i);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i + e < n) { xa[e] = pa[i + e]; xb[e] = pb[i + e]; }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (i + e < n) acc += (double)fabsf(__fsub_rn(xa[e], xb[e]));
    }
    swd_tree(sd, t, acc);
    if (t == 0) ws[(long long)r * chunks + blockIdx.x] = sd[0];
}

extern "C" long long msg_sorted_l1_workspace(int R, int n) {
    if (R <= 0 || n <= 0 || R > 65535) return -1;
    return 8ll * R * ((n + L1_CHUNK - 1) / L1_CHUNK);
}

extern "C" int msg_sorted_l1(const float* a, const float* b, int R, int n, double* sums, void* ws, void* stream) {
    if (!a || !b || !sums || !ws) return MSG_EINVAL;
    if (msg_sorted_l1_workspace(R, n) < 0) return MSG_EINVAL;
    if (((((uintptr_t)a) | ((uintptr_t)b)) & 3u) || ((((uintptr_t)sums) | ((uintptr_t)ws)) & 7u)) return MSG_EINVAL;
    const int chunks = (n + L1_CHUNK - 1) / L1_CHUNK;
    const bool vec = n % 4 == 0 && ((((uintptr_t)a) | ((uintptr_t)b)) & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)chunks, (unsigned)R);
    if (vec) hipLaunchKernelGGL((sorted_l1_kernel<true>), grid, dim3(256), 0, s, a, b, n, chunks, (double*)ws);
    else     hipLaunchKernelGGL((sorted_l1_kernel<false>), grid, dim3(256), 0, s, a, b, n, chunks, (double*)ws);
    hipLaunchKernelGGL(swd_merge_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, s, (const double*)ws, sums, R,
                       (long long)chunks, (long long)chunks, 1ll);
    return MSG_CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------------------------------------- projection
constexpr int PJ_T = 128;                 // descriptor rows per workgroup = directions per workgroup
constexpr int PJ_K = 32;                  // contraction step staged through LDS
constexpr int PJ_LX = PJ_K + 1;           // staged row of x^: odd, so that 32 rows at one k fall into 32 banks
constexpr int PJ_LDD = PJ_T + 32;         // staged k-row of the directions: the two lane halves (k, k + 1) fall into disjoint banks

template <bool VEC>
__global__ __launch_bounds__(256) void swd_project_kernel(const float* rows, int n, int d, const float* mean, const float* istd,
                                                          const float* dirs, int R, float* out) {
    __shared__ float sX[PJ_T * PJ_LX];
    __shared__ float sD[PJ_K * PJ_LDD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wi = wave >> 1, wd = wave & 1, col = lane & 31, half = lane >> 5;
    const long long i0 = (long long)blockIdx.x * PJ_T;
    const int r0 = blockIdx.y * PJ_T;
    const int lrow = t >> 3, kcol = (t & 7) * 4;       // staging: 32 rows x 32 k per pass, four passes

    f32x16 acc[2][2];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[g][s][e] = 0.f;

    for (int k0 = 0; k0 < d; k0 += PJ_K) {
        __syncthreads();                               // the previous step's reads of the staged tiles are done
        // x^ = (x - mean[plane]) * istd[plane], IEEE subtract and multiply; zero past the last row and past d
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const long long i = i0 + p * 32 + lrow;
            const int k = k0 + kcol;
            f32x4 x = {0.f, 0.f, 0.f, 0.f};
            if (i < n) {
                const float* src = rows + i * d + k;
                if constexpr (VEC) {
                    if (k < d) x = *reinterpret_cast<const f32x4*>(src);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (k + e < d) x[e] = src[e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float v = 0.f;
                if (i < n && k + e < d) {
                    const int pl = (k + e) / 49;
                    v = __fmul_rn(__fsub_rn(x[e], mean[pl]), istd[pl]);
                }
                sX[(p * 32 + lrow) * PJ_LX + kcol + e] = v;
            }
        }
#pragma unroll
        for (int p = 0; p < PJ_K * PJ_T / 256; ++p) {
            const int idx = p * 256 + t, k = idx / PJ_T, c = idx - k * PJ_T;
            sD[k * PJ_LDD + c] = (k0 + k < d && r0 + c < R) ? dirs[(long long)(k0 + k) * R + r0 + c] : 0.f;
        }
        __syncthreads();
        // instruction kk / 2 of the step takes j = k0 + kk (lower lane half) and k0 + kk + 1 (upper): ascending j per output
#pragma unroll
        for (int kk = 0; kk < PJ_K; kk += 2) {
            float fa[2], fb[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) fa[s] = sD[(kk + half) * PJ_LDD + wd * 64 + s * 32 + col];
#pragma unroll
            for (int g = 0; g < 2; ++g) fb[g] = sX[(wi * 64 + g * 32 + col) * PJ_LX + kk + half];
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    acc[g][s] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s], fb[g], acc[g][s], 0, 0, 0);
        }
    }

    // C/D layout: column = lane & 31 = the row i, register e = direction (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const long long i = i0 + wi * 64 + g * 32 + col;
        if (i >= n) continue;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int r = r0 + wd * 64 + s * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                if (r < R) out[(long long)r * n + i] = acc[g][s][e];
            }
    }
}

extern "C" int msg_swd_project(const float* rows, int n, int P, const float* mean, const float* istd, const float* dirs, int R,
                               float* out, void* stream) {
    if (!rows || !mean || !istd || !dirs || !out) return MSG_EINVAL;
    if (n <= 0 || P <= 0 || R <= 0 || P > INT_MAX / 49) return MSG_EINVAL;
    if ((((uintptr_t)rows) | ((uintptr_t)mean) | ((uintptr_t)istd) | ((uintptr_t)dirs) | ((uintptr_t)out)) & 3u) return MSG_EINVAL;
    const int d = P * 49;
    const long long tiles_n = ((long long)n + PJ_T - 1) / PJ_T, tiles_r = ((long long)R + PJ_T - 1) / PJ_T;
    if (tiles_r > 65535) return MSG_EINVAL;            // (what blockIdx.y can address)
    const dim3 grid((unsigned)tiles_n, (unsigned)tiles_r);
    hipStream_t s = (hipStream_t)stream;
    if (d % 4 == 0 && (((uintptr_t)rows) & 15u) == 0)
        hipLaunchKernelGGL((swd_project_kernel<true>), grid, dim3(256), 0, s, rows, n, d, mean, istd, dirs, R, out);
    else
        hipLaunchKernelGGL((swd_project_kernel<false>), grid, dim3(256), 0, s, rows, n, d, mean, istd, dirs, R, out);
    return MSG_CHECK_LAUNCH();
}
