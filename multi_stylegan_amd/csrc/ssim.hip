// One scale of the multi-scale structural similarity (ssim.py: ms_ssim; validation_metrics.py: MSSSIM / MSSSIMVideo; project.py;
// DESIGN.md section 5, "MS-SSIM"): the sums of the contrast-structure and SSIM maps of two planes, the L1 sum and the 2 x 2
// mean planes of the next scale in one launch, and the gradient of the three means in one more.  The order of operations is
// stated at the entries in include/msg_hip.h; the functions below are that statement.
//
// msg_ssim_scale            one workgroup per 16 x 64 tile of the plane.  The tile's 26 x 74 patch of x and y (the halo: 10 rows
//   below, 10 columns to the right) is loaded once into LDS; the row pass leaves the five row-filtered maps (x, y, x^2, y^2, x y)
//   of the patch's 26 rows in LDS; in the column pass a lane owns one column and four consecutive rows, reads the 14 values it
//   needs of each map once and forms cs and cs l of its four positions.  The moment maps exist only in registers.  The L1 terms and
//   the 2 x 2 means come from the patch already in LDS.  Per-lane float64 sums -> wave shuffles -> four wave sums added in wave
//   order -> ws; a second launch adds a plane's tiles in index order.
// msg_ssim_scale_backward   one workgroup per 16 x 32 tile of grad_x.  The positions whose windows touch the tile are the 26 x 42
//   above and to the left of it; their moments are recomputed from the 36 x 52 patch (row pass, column pass as above), the three
//   coefficient maps A, B, C are left in LDS, and the transposed window (row pass, column pass) gathers them per pixel.
// No atomics anywhere: every output is bit-identical from run to run.
#include <limits.h>
#include "msg_common.h"

// g_k = exp(-(k - 5)^2 / 4.5) / sum, k = 0 .. 10, computed in float64 and rounded once to fp32
__host__ __device__ constexpr float ss_g(int k) {
    k = k > 5 ? 10 - k : k;
    return k == 0 ? 0x1.0d956cp-10f : k == 1 ? 0x1.f1fe02p-8f : k == 2 ? 0x1.26eb18p-5f : k == 3 ? 0x1.bff0fep-4f
         : k == 4 ? 0x1.b43c4p-3f : 0x1.10656p-2f;
}

// sum_k g_k p[k s]: one multiply, then ten fused multiply-adds in ascending k
__device__ __forceinline__ float ss_fir(const float* p, int s) {
    float a = __fmul_rn(ss_g(0), p[0]);
#pragma unroll
    for (int k = 1; k < 11; ++k) a = fmaf(ss_g(k), p[k * s], a);
    return a;
}

// the five row-filtered values of one patch position: x^2, y^2 and x y are rounded to fp32 before they are filtered
__device__ __forceinline__ void ss_row5(const float* px, const float* py, float* o) {
    float ax, ay, axx, ayy, axy;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
        const float xv = px[k], yv = py[k], g = ss_g(k);
        const float xx = __fmul_rn(xv, xv), yy = __fmul_rn(yv, yv), xy = __fmul_rn(xv, yv);
        if (k == 0) {
            ax = __fmul_rn(g, xv); ay = __fmul_rn(g, yv); axx = __fmul_rn(g, xx); ayy = __fmul_rn(g, yy); axy = __fmul_rn(g, xy);
        } else {
            ax = fmaf(g, xv, ax); ay = fmaf(g, yv, ay); axx = fmaf(g, xx, axx); ayy = fmaf(g, yy, ayy); axy = fmaf(g, xy, axy);
        }
    }
    o[0] = ax; o[1] = ay; o[2] = axx; o[3] = ayy; o[4] = axy;
}

struct SsimPoint { float mx, my, cs, l, d1, d2; };

// the pointwise part, every operation one IEEE fp32 operation (2 s + c is one fused multiply-add: the doubling is exact)
__device__ __forceinline__ SsimPoint ss_point(const float* m, float c1, float c2) {
    SsimPoint p;
    p.mx = m[0]; p.my = m[1];
    const float mxx = __fmul_rn(p.mx, p.mx), myy = __fmul_rn(p.my, p.my), mxy = __fmul_rn(p.mx, p.my);
    const float sxx = __fsub_rn(m[2], mxx), syy = __fsub_rn(m[3], myy), sxy = __fsub_rn(m[4], mxy);
    p.d2 = __fadd_rn(__fadd_rn(sxx, syy), c2);
    p.d1 = __fadd_rn(__fadd_rn(mxx, myy), c1);
    p.cs = __fdiv_rn(fmaf(2.f, sxy, c2), p.d2);
    p.l = __fdiv_rn(fmaf(2.f, mxy, c1), p.d1);
    return p;
}

// ---------------------------------------------------------------------------------------------------------------- forward
constexpr int SF_TH = 16, SF_TW = 64;                 // tile of one workgroup: pixels and window positions alike
constexpr int SF_PH = SF_TH + 10;                     // patch rows
constexpr int SF_PW = SF_TW + 12;                     // patch columns: 74 used, loaded as 19 groups of four

template <bool VEC>
__global__ __launch_bounds__(256) void ssim_scale_kernel(const float* x, const float* y, int h, int w, int tiles_x, int tiles_y,
                                                         float c1, float c2, double* ws, int with_l1, float* xh, float* yh) {
    __shared__ __attribute__((aligned(16))) float sX[SF_PH * SF_PW];
    __shared__ __attribute__((aligned(16))) float sY[SF_PH * SF_PW];
    __shared__ float sR[5][SF_PH * SF_TW];
    __shared__ double sD[3][4];
    const int t = threadIdx.x;
    long long tile = blockIdx.x;
    const int tx = (int)(tile % tiles_x);
    tile /= tiles_x;
    const int ty = (int)(tile % tiles_y);
    const long long m = tile / tiles_y;
    const int y0 = ty * SF_TH, x0 = tx * SF_TW;
    const float* px = x + m * (long long)h * w;
    const float* py = y + m * (long long)h * w;

    // the patch: row r is plane row y0 + r, column c is plane column x0 + c; zero outside the plane (only positions outside
    // the valid range read those, and they are not summed)
    for (int g = t; g < SF_PH * (SF_PW / 4); g += 256) {
        const int r = g / (SF_PW / 4), gx = g - r * (SF_PW / 4);
        const int yy = y0 + r, xv = x0 + 4 * gx;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (yy < h) {
            const float* rx = px + (long long)yy * w;
            const float* ry = py + (long long)yy * w;
            if (VEC && xv + 3 < w) {
                a = *reinterpret_cast<const f32x4*>(rx + xv);
                b = *reinterpret_cast<const f32x4*>(ry + xv);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (xv + e < w) { a[e] = rx[xv + e]; b[e] = ry[xv + e]; }
            }
        }
        *reinterpret_cast<f32x4*>(sX + r * SF_PW + 4 * gx) = a;
        *reinterpret_cast<f32x4*>(sY + r * SF_PW + 4 * gx) = b;
    }
    __syncthreads();

    // rows first
    for (int i = t; i < SF_PH * SF_TW; i += 256) {
        const int r = i / SF_TW, c = i - r * SF_TW;
        float o[5];
        ss_row5(sX + r * SF_PW + c, sY + r * SF_PW + c, o);
#pragma unroll
        for (int q = 0; q < 5; ++q) sR[q][i] = o[q];
    }

    // the L1 terms and the 2 x 2 means of the tile's own pixels, from the patch
    double dl1 = 0.0;
    if (with_l1) {
#pragma unroll
        for (int j = 0; j < SF_TH * SF_TW / 256; ++j) {
            const int i = j * 256 + t, r = i / SF_TW, c = i - r * SF_TW;
            if (y0 + r < h && x0 + c < w) dl1 += (double)fabsf(__fsub_rn(sX[r * SF_PW + c], sY[r * SF_PW + c]));
        }
    }
    if (xh) {
        const int oy = t / (SF_TW / 2), ox = t - oy * (SF_TW / 2);
        const int gy = (y0 >> 1) + oy, gx = (x0 >> 1) + ox, hc = h >> 1, wc = w >> 1;
        if (gy < hc && gx < wc) {
            const float* a = sX + (2 * oy) * SF_PW + 2 * ox;
            const float* b = sY + (2 * oy) * SF_PW + 2 * ox;
            const long long o = m * (long long)hc * wc + (long long)gy * wc + gx;
            xh[o] = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(a[0], a[1]), __fadd_rn(a[SF_PW], a[SF_PW + 1])));
            yh[o] = __fmul_rn(0.25f, __fadd_rn(__fadd_rn(b[0], b[1]), __fadd_rn(b[SF_PW], b[SF_PW + 1])));
        }
    }
    __syncthreads();

    // then columns: this lane's column c, positions in rows 4 rg .. 4 rg + 3
    const int c = t & (SF_TW - 1), rg = t / SF_TW;
    float mom[4][5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        float v[14];
#pragma unroll
        for (int j = 0; j < 14; ++j) v[j] = sR[q][(4 * rg + j) * SF_TW + c];
#pragma unroll
        for (int i = 0; i < 4; ++i) mom[i][q] = ss_fir(v + i, 1);
    }
    double dcs = 0.0, dss = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const SsimPoint p = ss_point(mom[i], c1, c2);
        if (y0 + 4 * rg + i < h - 10 && x0 + c < w - 10) {
            dcs += (double)p.cs;
            dss += (double)__fmul_rn(p.cs, p.l);
        }
    }

    // lanes -> wave (shuffles, a fixed tree) -> the four waves in their order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        dcs += __shfl_down(dcs, off, 64);
        dss += __shfl_down(dss, off, 64);
        dl1 += __shfl_down(dl1, off, 64);
    }
    if ((t & 63) == 0) { sD[0][t >> 6] = dcs; sD[1][t >> 6] = dss; sD[2][t >> 6] = dl1; }
    __syncthreads();
    if (t < 3) ws[(long long)blockIdx.x * 3 + t] = ((sD[t][0] + sD[t][1]) + sD[t][2]) + sD[t][3];
}

// sums[m, 0 .. 1] and l1[m]: the plane's tiles in index order
__global__ void ssim_merge_kernel(const double* ws, int M, int tiles, double* sums, double* l1) {
    const int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= 3 * M) return;
    const int m = o / 3, q = o - 3 * m;
    if (q == 2 && !l1) return;
    const double* src = ws + (long long)m * tiles * 3 + q;
    double s = 0.0;
    for (int i = 0; i < tiles; ++i) s += src[3ll * i];
    if (q == 2) l1[m] = s; else sums[2 * m + q] = s;
}

static long long ssim_tiles(int M, int h, int w, int th, int tw) {
    if (M <= 0 || h < 11 || w < 11) return -1;
    const long long tiles = (long long)M * ((w + tw - 1) / tw) * ((h + th - 1) / th);
    return tiles > INT_MAX ? -1 : tiles;
}

extern "C" long long msg_ssim_scale_workspace(int M, int h, int w) {
    const long long tiles = ssim_tiles(M, h, w, SF_TH, SF_TW);
    return tiles < 0 ? -1 : 24 * tiles;
}

extern "C" int msg_ssim_scale(const float* x, const float* y, int M, int h, int w, float c1, float c2, double* sums, double* l1,
                              float* x_half, float* y_half, void* ws, void* stream) {
    if (!x || !y || !sums || !ws) return MSG_EINVAL;
    if ((x_half == nullptr) != (y_half == nullptr)) return MSG_EINVAL;
    const long long tiles = ssim_tiles(M, h, w, SF_TH, SF_TW);
    if (tiles < 0 || M > INT_MAX / 3) return MSG_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)x_half) | ((uintptr_t)y_half)) & 3u) return MSG_EINVAL;
    if ((((uintptr_t)sums) | ((uintptr_t)l1) | ((uintptr_t)ws)) & 7u) return MSG_EINVAL;
    const int tiles_x = (w + SF_TW - 1) / SF_TW, tiles_y = (h + SF_TH - 1) / SF_TH;
    const bool vec = w % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)y)) & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((ssim_scale_kernel<true>), dim3((unsigned)tiles), dim3(256), 0, s, x, y, h, w, tiles_x, tiles_y, c1, c2,
                                (double*)ws, l1 ? 1 : 0, x_half, y_half);
    else     hipLaunchKernelGGL((ssim_scale_kernel<false>), dim3((unsigned)tiles), dim3(256), 0, s, x, y, h, w, tiles_x, tiles_y, c1, c2,
                                (double*)ws, l1 ? 1 : 0, x_half, y_half);
    hipLaunchKernelGGL(ssim_merge_kernel, dim3((unsigned)((3 * M + 63) / 64)), dim3(64), 0, s, (const double*)ws, M, tiles_x * tiles_y,
                       sums, l1);
    return MSG_CHECK_LAUNCH();
}

// --------------------------------------------------------------------------------------------------------------- backward
constexpr int SB_TH = 16, SB_TW = 32;                 // tile of grad_x of one workgroup
constexpr int SB_QH = SB_TH + 10, SB_QW = SB_TW + 10; // the window positions that touch it: 10 rows above, 10 columns to the left
constexpr int SB_PH = SB_QH + 10;                     // patch rows: from plane row y0 - 10
constexpr int SB_PW = 56;                             // patch columns: from plane column x0 - 12 (a multiple of four), columns 2 .. 53 used
constexpr int SB_LD = SB_QW + 1;                      // row of a position map in LDS

template <bool VEC>
__global__ __launch_bounds__(256) void ssim_scale_backward_kernel(const float* x, const float* y, const float* g, const float* gh,
                                                                  int h, int w, int tiles_x, int tiles_y, float c1, float c2,
                                                                  float* gx) {
    __shared__ __attribute__((aligned(16))) float sX[SB_PH * SB_PW];
    __shared__ __attribute__((aligned(16))) float sY[SB_PH * SB_PW];
    __shared__ float sR[5 * SB_PH * SB_LD];           // the row-filtered maps; later the row-gathered A, B, C [3][SB_QH][SB_TW]
    __shared__ float sA[3][SB_QH * SB_LD];
    const int t = threadIdx.x;
    long long tile = blockIdx.x;
    const int tx = (int)(tile % tiles_x);
    tile /= tiles_x;
    const int ty = (int)(tile % tiles_y);
    const long long m = tile / tiles_y;
    const int y0 = ty * SB_TH, x0 = tx * SB_TW;
    const float* px = x + m * (long long)h * w;
    const float* py = y + m * (long long)h * w;
    const int nh = h - 10, nw = w - 10;
    // the gradients of the three means -> of the sums: divided by the counts as fp32 numbers
    const float n = (float)((long long)nh * nw), np = (float)((long long)h * w);
    const float gcs = __fdiv_rn(g[m * 3], n), gss = __fdiv_rn(g[m * 3 + 1], n), gl1 = __fdiv_rn(g[m * 3 + 2], np);

    for (int q = t; q < SB_PH * (SB_PW / 4); q += 256) {
        const int r = q / (SB_PW / 4), gq = q - r * (SB_PW / 4);
        const int yy = y0 - 10 + r, xv = x0 - 12 + 4 * gq;
        f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
        if (yy >= 0 && yy < h && xv >= 0) {
            const float* rx = px + (long long)yy * w;
            const float* ry = py + (long long)yy * w;
            if (VEC && xv + 3 < w) {
                a = *reinterpret_cast<const f32x4*>(rx + xv);
                b = *reinterpret_cast<const f32x4*>(ry + xv);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (xv + e < w) { a[e] = rx[xv + e]; b[e] = ry[xv + e]; }
            }
        }
        *reinterpret_cast<f32x4*>(sX + r * SB_PW + 4 * gq) = a;
        *reinterpret_cast<f32x4*>(sY + r * SB_PW + 4 * gq) = b;
    }
    __syncthreads();

    // the moments as in the forward kernel -- rows: position column c is plane column x0 - 10 + c = patch column c + 2
    for (int i = t; i < SB_PH * SB_QW; i += 256) {
        const int r = i / SB_QW, c = i - r * SB_QW;
        float o[5];
        ss_row5(sX + r * SB_PW + c + 2, sY + r * SB_PW + c + 2, o);
#pragma unroll
        for (int q = 0; q < 5; ++q) sR[q * (SB_PH * SB_LD) + r * SB_LD + c] = o[q];
    }
    __syncthreads();
    // ... columns: position row r is plane row y0 - 10 + r = patch row r; then the three coefficient maps, zero where there is
    // no position
    for (int i = t; i < SB_QH * SB_QW; i += 256) {
        const int r = i / SB_QW, c = i - r * SB_QW;
        const int qy = y0 - 10 + r, qx = x0 - 10 + c;
        float A = 0.f, B = 0.f, C = 0.f;
        if (qy >= 0 && qy < nh && qx >= 0 && qx < nw) {
            float mom[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) mom[q] = ss_fir(sR + q * (SB_PH * SB_LD) + r * SB_LD + c, SB_LD);
            const SsimPoint p = ss_point(mom, c1, c2);
            const float a = fmaf(gss, p.l, gcs), b = __fmul_rn(gss, p.cs);
            const float t2 = __fdiv_rn(a, p.d2), t1 = __fdiv_rn(b, p.d1);
            const float u = __fmul_rn(2.f, __fsub_rn(__fmul_rn(p.mx, p.cs), p.my));
            const float v = __fmul_rn(2.f, __fsub_rn(p.my, __fmul_rn(p.mx, p.l)));
            A = fmaf(t2, u, __fmul_rn(t1, v));
            B = -__fmul_rn(t2, p.cs);
            C = __fmul_rn(2.f, t2);
        }
        sA[0][r * SB_LD + c] = A;
        sA[1][r * SB_LD + c] = B;
        sA[2][r * SB_LD + c] = C;
    }
    __syncthreads();
    // the transposed window, rows: pixel column lx of the tile takes tap k from position column lx + 10 - k
    float* sT = sR;
    for (int i = t; i < 3 * SB_QH * SB_TW; i += 256) {
        const int q = i / (SB_QH * SB_TW), rem = i - q * (SB_QH * SB_TW), r = rem / SB_TW, lx = rem - r * SB_TW;
        sT[i] = ss_fir(sA[q] + r * SB_LD + lx + 10, -1);
    }
    __syncthreads();
    // ... columns, and the pixel's own factors: four pixels of one row per lane
    if (t < SB_TH * SB_TW / 4) {
        const int ly = t / (SB_TW / 4), lx = 4 * (t - ly * (SB_TW / 4));
        const int yy = y0 + ly, xx = x0 + lx, hc = h >> 1, wc = w >> 1;
        if (yy < h && xx < w) {
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float GA = ss_fir(sT + (ly + 10) * SB_TW + lx + e, -SB_TW);
                const float GB = ss_fir(sT + SB_QH * SB_TW + (ly + 10) * SB_TW + lx + e, -SB_TW);
                const float GC = ss_fir(sT + 2 * SB_QH * SB_TW + (ly + 10) * SB_TW + lx + e, -SB_TW);
                const float xv = sX[(ly + 10) * SB_PW + lx + e + 12], yv = sY[(ly + 10) * SB_PW + lx + e + 12];
                float v = fmaf(yv, GC, fmaf(__fmul_rn(2.f, xv), GB, GA));
                const float d = __fsub_rn(xv, yv);
                v = fmaf(gl1, d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f), v);
                if (gh && (yy >> 1) < hc && ((xx + e) >> 1) < wc && xx + e < w)
                    v = fmaf(0.25f, gh[m * (long long)hc * wc + (long long)(yy >> 1) * wc + ((xx + e) >> 1)], v);
                o[e] = v;
            }
            float* dst = gx + m * (long long)h * w + (long long)yy * w + xx;
            if (VEC && xx + 3 < w) {
                *reinterpret_cast<f32x4*>(dst) = o;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (xx + e < w) dst[e] = o[e];
            }
        }
    }
}

extern "C" int msg_ssim_scale_backward(const float* x, const float* y, const float* g, const float* g_half, int M, int h, int w,
                                       float c1, float c2, float* grad_x, void* stream) {
    if (!x || !y || !g || !grad_x) return MSG_EINVAL;
    const long long tiles = ssim_tiles(M, h, w, SB_TH, SB_TW);
    if (tiles < 0) return MSG_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)g) | ((uintptr_t)g_half) | ((uintptr_t)grad_x)) & 3u) return MSG_EINVAL;
    const int tiles_x = (w + SB_TW - 1) / SB_TW, tiles_y = (h + SB_TH - 1) / SB_TH;
    const bool vec = w % 4 == 0 && ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)grad_x)) & 15u) == 0;
    hipStream_t s = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((ssim_scale_backward_kernel<true>), dim3((unsigned)tiles), dim3(256), 0, s, x, y, g, g_half, h, w,
                                tiles_x, tiles_y, c1, c2, grad_x);
    else     hipLaunchKernelGGL((ssim_scale_backward_kernel<false>), dim3((unsigned)tiles), dim3(256), 0, s, x, y, g, g_half, h, w,
                                tiles_x, tiles_y, c1, c2, grad_x);
    return MSG_CHECK_LAUNCH();
}
