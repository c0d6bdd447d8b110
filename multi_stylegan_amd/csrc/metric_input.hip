// Metric inputs: what a pretrained feature network receives from the validation pass -- one channel of a batch [B, C, T, H, W]
// (fp32 / bf16), one time step or the whole clip, resized with torch's anti-aliased bilinear filter, mapped per sample to
// [-1, 1] and replicated on one or three colour planes: out [B, planes, T', out_h, out_w].  The reference does this as a chain
// of stock calls (multi_stylegan/validation_metrics.py:44-52 for IS: resize, then normalise; :589-590 for FID and :941-943
// for FVD: normalise, then resize inside the network's forward; misc.normalize_m1_1_batch), about ten launches per channel.
//
// The filter.  Per axis, output index i reads the source taps j whose triangle weight max(0, 1 - |j + 0.5 - c| / support) is
// positive, c = (i + 0.5) n_in / n_out, support = max(n_in / n_out, 1), the weights divided by their sum.  With
// D = 2 max(n_in, n_out) that weight is (D - |n_out (2j + 1) - n_in (2i + 1)|) / D: an INTEGER over D.  The kernel forms the
// numerators and their sum in integer arithmetic and divides once, so every weight is the correctly rounded fp32 value of the
// exact one -- fp32 evaluation of c alone would be off by 1e-5 at 256 pixels -- and the tap range is exactly the taps with a
// positive weight (torch's range can add one tap of weight zero at its end).  At equal size the weight is D / D = 1 on one tap
// and the result is a copy, bit for bit; up-scaling gives at most two taps (bilinear with border clamp), scale s at most
// 2 s taps; MSG_METRIC_MAX_SCALE = 8 bounds them by MI_TAPS = 16.
//
// One workgroup (256 lanes) makes a tile of MI_TY x MI_TX = 16 x 64 output pixels of one frame:
//   * the first 80 lanes compute the taps and weights of the tile's 64 columns and 16 rows into LDS;
//   * the source window of the tile (at most 137 rows x 521 columns at the cap) is walked in chunks of as many rows as fit
//     the staging buffer: a chunk is loaded once (16 bytes per lane where the base and W allow it, element by element
//     otherwise), normalised on the way in the SOURCE mode, and the row pass leaves [rows][64] fp32 in LDS;
//   * the column pass reads that with 16-byte LDS reads, a lane owning 16 bytes of adjacent output pixels (4 fp32, 8 bf16),
//     normalises in the RESIZED mode and stores 16 bytes to each plane (element by element when out or out_w is not aligned).
// The row-pass result never leaves LDS.  LDS per workgroup: 35,072 B (row pass) + 8,448 B (staging) + 5,120 B (weights) +
// tap tables = 49,312 B, three workgroups per CU.
//
// Normalised modes: two launches, no synchronisation.  The first leaves one (min, max) pair per workgroup in ws: over a
// piece of the sample's selected source frames (SOURCE: metric_minmax_kernel), or over a tile of the resized values (RESIZED:
// the resize kernel itself with its stores switched off).  Every workgroup of the second reads its sample's pairs; min and
// max are exact and NaN wins every comparison here (torch's min / max propagate NaN, fminf does not), so the order of the
// reduction cannot change the result.  RESIZED computes the resized values twice with the same instruction sequence: the
// extreme values come out as exactly 0 and 1 before the clamp, and no fp32 intermediate is written to memory.
// No atomics; a sample's result depends on that sample alone; bit-identical from run to run.  The vector and the scalar paths
// differ in how values travel, never in arithmetic: every product and sum below is an explicitly rounded operation.
#include <math.h>
#include "msg_common.h"

constexpr int MI_TX = 64, MI_TY = 16;                                       // the output tile
constexpr int MI_TAPS = 2 * MSG_METRIC_MAX_SCALE;                           // taps of one output at the cap
// taps of m consecutive outputs span at most scale (m - 1) + 2 max(scale, 1) + 1 source indices
constexpr int MI_ROWS = (MI_TY - 1) * MSG_METRIC_MAX_SCALE + MI_TAPS + 1;   // 137
constexpr int MI_COLS = (MI_TX - 1) * MSG_METRIC_MAX_SCALE + MI_TAPS + 1;   // 521
constexpr int MI_PITCH = (MI_COLS + 7 + 7) & ~7;                            // window start and end rounded to 8 elements: 528
constexpr int MI_STAGE = 4 * MI_PITCH;                                      // staging: at least 4 source rows per chunk
constexpr int MI_MINMAX_PIECES = 64;                                        // SOURCE: at most this many workgroups per sample
constexpr long long MI_MINMAX_MIN = 4096;                                   // ... of at least this many elements each

// min / max in which NaN wins (torch.min / torch.max)
__device__ __forceinline__ float mi_min(float a, float b) { return (a != a || a <= b) ? a : b; }
__device__ __forceinline__ float mi_max(float a, float b) { return (a != a || a >= b) ? a : b; }

// (lo, hi) of the workgroup's lanes -> every lane; s_red: 8 floats
__device__ __forceinline__ void mi_block_minmax(float& lo, float& hi, float* s_red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = mi_min(lo, __shfl_xor(lo, off, 64));
        hi = mi_max(hi, __shfl_xor(hi, off, 64));
    }
    __syncthreads();                                                        // (s_red may still be read from a previous use)
    if ((threadIdx.x & 63) == 0) {
        s_red[2 * (threadIdx.x >> 6)] = lo;
        s_red[2 * (threadIdx.x >> 6) + 1] = hi;
    }
    __syncthreads();
    lo = mi_min(mi_min(s_red[0], s_red[2]), mi_min(s_red[4], s_red[6]));
    hi = mi_max(mi_max(s_red[1], s_red[3]), mi_max(s_red[5], s_red[7]));
}

// misc.normalize_m1_1_batch on one value: 2 max((x - lo) / span, 1e-3) - 1, IEEE subtract and divide, the clamp from below only
// and transparent to NaN (a constant sample: 0 / 0)
__device__ __forceinline__ float mi_normalise(float x, float lo, float span) {
    float v = __fdiv_rn(__fsub_rn(x, lo), span);
    v = v < 1e-3f ? 1e-3f : v;
    return __fsub_rn(__fmul_rn(2.f, v), 1.f);
}

__device__ __forceinline__ long long mi_floordiv(long long a, long long b) {   // b > 0
    const long long q = a / b;
    return (a % b < 0) ? q - 1 : q;
}

// taps of output index i of an axis n_in -> n_out: first source index, count (1 .. MI_TAPS), weights w[k * stride]
__device__ __forceinline__ void mi_axis(int n_in, int n_out, int i, int* first, int* count, float* w, int stride) {
    const long long no = n_out, D = 2ll * (n_in > n_out ? n_in : n_out), A = (long long)n_in * (2 * i + 1);
    long long lo = mi_floordiv(A - D - no, 2 * no) + 1;                       // n_out (2j + 1) > A - D
    long long hi = -mi_floordiv(-(A + D - no), 2 * no);                       // n_out (2j + 1) < A + D, exclusive
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_in ? n_in : hi;
    long long total = 0;
    for (long long j = lo; j < hi; ++j) total += D - llabs(no * (2 * j + 1) - A);
    const float ft = (float)total;
    const int n = (int)(hi - lo) < MI_TAPS ? (int)(hi - lo) : MI_TAPS;        // (never more: 2 D / n_out <= 4 MSG_METRIC_MAX_SCALE)
    for (int k = 0; k < n; ++k) w[k * stride] = __fdiv_rn((float)(D - llabs(no * (2 * (lo + k) + 1) - A)), ft);
    *first = (int)lo;
    *count = n;
}

struct MetricGeom {
    int C, T, H, W, channel, t, frames, planes, out_h, out_w, tiles_y, tiles_x;
    int norm, stats, vec_in, vec_out;
    long long parts;                                                        // (min, max) pairs per sample in ws
};

// grid: (sample, selected frame, tile row, tile column), flat.  stats: leave the tile's (min, max) in ws, store nothing.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void metric_input_kernel(const TI* __restrict__ images, TO* __restrict__ out,
                                                           float* __restrict__ ws, MetricGeom g) {
    __shared__ __attribute__((aligned(16))) float s_h[MI_ROWS * MI_TX];
    __shared__ __attribute__((aligned(16))) float s_stage[MI_STAGE];
    __shared__ float s_wx[MI_TAPS * MI_TX], s_wy[MI_TAPS * MI_TY];
    __shared__ int s_x0[MI_TX], s_xn[MI_TX], s_y0[MI_TY], s_yn[MI_TY];
    __shared__ float s_red[8];
    constexpr int NIN = Vec16<TI>::N;
    constexpr int NPX = 16 / (int)sizeof(TO);                               // adjacent output pixels per lane
    constexpr int TPR = MI_TX / NPX, RSTEP = 256 / TPR;                     // lanes per tile row, rows per sweep
    const int tid = threadIdx.x;
    unsigned n = blockIdx.x;
    const int tx = (int)(n % (unsigned)g.tiles_x);
    n /= (unsigned)g.tiles_x;
    const int ty = (int)(n % (unsigned)g.tiles_y);
    n /= (unsigned)g.tiles_y;
    const int f = (int)(n % (unsigned)g.frames);
    const long long b = n / (unsigned)g.frames;
    const int ox0 = tx * MI_TX, oy0 = ty * MI_TY;
    const int mx = min(MI_TX, g.out_w - ox0), my = min(MI_TY, g.out_h - oy0);

    if (tid < mx) mi_axis(g.W, g.out_w, ox0 + tid, &s_x0[tid], &s_xn[tid], s_wx + tid, MI_TX);
    else if (tid >= 64 && tid < 64 + my)
        mi_axis(g.H, g.out_h, oy0 + tid - 64, &s_y0[tid - 64], &s_yn[tid - 64], s_wy + tid - 64, MI_TY);

    float lo = 0.f, span = 1.f;
    const bool normalise = g.norm != MSG_METRIC_NORM_NONE && !g.stats;
    if (normalise) {
        const float* pairs = ws + 2 * b * g.parts;
        float l = INFINITY, h = -INFINITY;
        for (long long k = tid; k < g.parts; k += 256) {
            l = mi_min(l, pairs[2 * k]);
            h = mi_max(h, pairs[2 * k + 1]);
        }
        mi_block_minmax(l, h, s_red);
        lo = l;
        span = __fsub_rn(h, l);
    }
    __syncthreads();

    const int r_lo = s_y0[0], rows = s_y0[my - 1] + s_yn[my - 1] - r_lo;
    const int c0 = s_x0[0] & ~7, pitch = (s_x0[mx - 1] + s_xn[mx - 1] - c0 + 7) & ~7;
    const int rc = MI_STAGE / pitch;
    const bool pre = normalise && g.norm == MSG_METRIC_NORM_SOURCE;
    const TI* src = images + ((b * g.C + g.channel) * g.T + (g.t < 0 ? f : g.t)) * ((long long)g.H * g.W);
    for (int r0 = 0; r0 < rows; r0 += rc) {
        const int nr = min(rc, rows - r0);
        __syncthreads();                                                    // the previous chunk's row pass has read s_stage
        if (g.vec_in) {                                                     // W % NIN == 0: a vector that starts inside a row ends inside it
            const int pv = pitch / NIN;
            for (int idx = tid; idx < nr * pv; idx += 256) {
                const int r = idx / pv, v = idx - r * pv, x = c0 + v * NIN;
                if (x >= g.W) continue;
                Vec16<TI> q;
                q.raw = *reinterpret_cast<const uint4*>(src + (long long)(r_lo + r0 + r) * g.W + x);
#pragma unroll
                for (int e = 0; e < NIN; ++e) {
                    const float val = q.get(e);
                    s_stage[r * pitch + v * NIN + e] = pre ? mi_normalise(val, lo, span) : val;
                }
            }
        } else {
            for (int idx = tid; idx < nr * pitch; idx += 256) {
                const int r = idx / pitch, j = idx - r * pitch, x = c0 + j;
                if (x >= g.W) continue;
                const float val = load_as_f32<TI>(src + (long long)(r_lo + r0 + r) * g.W + x);
                s_stage[idx] = pre ? mi_normalise(val, lo, span) : val;
            }
        }
        __syncthreads();
        for (int idx = tid; idx < nr * MI_TX; idx += 256) {
            const int r = idx / MI_TX, i = idx - r * MI_TX;
            if (i >= mx) continue;
            const float* p = s_stage + r * pitch + (s_x0[i] - c0);
            const int taps = s_xn[i];
            float acc = __fmul_rn(s_wx[i], p[0]);
            for (int k = 1; k < taps; ++k) acc = fmaf(s_wx[k * MI_TX + i], p[k], acc);
            s_h[(r0 + r) * MI_TX + i] = acc;
        }
    }
    __syncthreads();

    float tl = INFINITY, th = -INFINITY;
    const bool post = normalise && g.norm == MSG_METRIC_NORM_RESIZED;
    const long long plane = (long long)g.frames * g.out_h * g.out_w;
    for (int ry = tid / TPR; ry < my; ry += RSTEP) {
        const int cx = (tid % TPR) * NPX;
        if (cx >= mx) continue;
        const int taps = s_yn[ry];
        const float* p = s_h + (s_y0[ry] - r_lo) * MI_TX + cx;
        float acc[NPX];
        {
            const float w = s_wy[ry];
#pragma unroll
            for (int q = 0; q < NPX / 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(p + 4 * q);
                acc[4 * q] = __fmul_rn(w, v.x); acc[4 * q + 1] = __fmul_rn(w, v.y);
                acc[4 * q + 2] = __fmul_rn(w, v.z); acc[4 * q + 3] = __fmul_rn(w, v.w);
            }
        }
        for (int k = 1; k < taps; ++k) {
            const float w = s_wy[k * MI_TY + ry];
#pragma unroll
            for (int q = 0; q < NPX / 4; ++q) {
                const float4 v = *reinterpret_cast<const float4*>(p + k * MI_TX + 4 * q);
                acc[4 * q] = fmaf(w, v.x, acc[4 * q]); acc[4 * q + 1] = fmaf(w, v.y, acc[4 * q + 1]);
                acc[4 * q + 2] = fmaf(w, v.z, acc[4 * q + 2]); acc[4 * q + 3] = fmaf(w, v.w, acc[4 * q + 3]);
            }
        }
        if (g.stats) {
#pragma unroll
            for (int e = 0; e < NPX; ++e)
                if (cx + e < mx) {
                    tl = mi_min(tl, acc[e]);
                    th = mi_max(th, acc[e]);
                }
            continue;
        }
        if (post) {
#pragma unroll
            for (int e = 0; e < NPX; ++e) acc[e] = mi_normalise(acc[e], lo, span);
        }
        TO* dst = out + (b * g.planes * g.frames + f) * ((long long)g.out_h * g.out_w) + (long long)(oy0 + ry) * g.out_w
                  + ox0 + cx;
        if (g.vec_out) {                                                    // out_w % NPX == 0: the lane's pixels are all inside
            uint4 raw;
            if constexpr (sizeof(TO) == 4) {
                raw = make_uint4(__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3]));
            } else {
                Vec16<bf16_t> pk;
#pragma unroll
                for (int e = 0; e < 4; ++e) pk.set2(e, acc[2 * e], acc[2 * e + 1]);
                raw = pk.raw;
            }
            for (int c = 0; c < g.planes; ++c) *reinterpret_cast<uint4*>(dst + c * plane) = raw;
        } else {
            for (int c = 0; c < g.planes; ++c)
#pragma unroll
                for (int e = 0; e < NPX; ++e)
                    if (cx + e < mx) store_from_f32<TO>(dst + c * plane + e, acc[e]);
        }
    }
    if (g.stats) {
        mi_block_minmax(tl, th, s_red);
        if (tid == 0) {
            ws[2ll * blockIdx.x] = tl;
            ws[2ll * blockIdx.x + 1] = th;
        }
    }
}

// SOURCE, first launch: workgroup (sample b, piece p) leaves (min, max) of elements [p per, min((p + 1) per, count)) of the
// sample's selected frames -- contiguous in memory: one frame, or the channel's T frames -- in ws[b pieces + p].
template <typename TI>
__global__ __launch_bounds__(256) void metric_minmax_kernel(const TI* __restrict__ images, float* __restrict__ ws,
                                                            long long sample_stride, long long first, long long count,
                                                            long long per, int pieces, int vec) {
    __shared__ float s_red[8];
    constexpr int NIN = Vec16<TI>::N;
    const long long b = blockIdx.x / (unsigned)pieces;
    const int p = (int)(blockIdx.x % (unsigned)pieces);
    const TI* src = images + b * sample_stride + first;
    const long long beg = p * per, end = beg + per < count ? beg + per : count;
    float lo = INFINITY, hi = -INFINITY;
    if (vec) {                                                              // per and count are multiples of NIN
        for (long long i = beg + (long long)threadIdx.x * NIN; i < end; i += 256 * NIN) {
            Vec16<TI> q;
            q.raw = *reinterpret_cast<const uint4*>(src + i);
#pragma unroll
            for (int e = 0; e < NIN; ++e) {
                lo = mi_min(lo, q.get(e));
                hi = mi_max(hi, q.get(e));
            }
        }
    } else {
        for (long long i = beg + threadIdx.x; i < end; i += 256) {
            const float v = load_as_f32<TI>(src + i);
            lo = mi_min(lo, v);
            hi = mi_max(hi, v);
        }
    }
    mi_block_minmax(lo, hi, s_red);
    if (threadIdx.x == 0) {
        ws[2ll * blockIdx.x] = lo;
        ws[2ll * blockIdx.x + 1] = hi;
    }
}

// What both entries derive from the sizes: the status the launch entry would return for them, the grids, the pairs per sample.
struct MetricPlan {
    int frames, tiles_y, tiles_x, pieces;
    long long blocks, count, per, parts;
};

static int metric_plan(int B, int T, int H, int W, int t, int out_h, int out_w, int norm, MetricPlan* p) {
    if (B <= 0 || T <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0) return MSG_EINVAL;
    if (t < -1 || t >= T) return MSG_EINVAL;
    if (norm != MSG_METRIC_NORM_NONE && norm != MSG_METRIC_NORM_SOURCE && norm != MSG_METRIC_NORM_RESIZED) return MSG_EINVAL;
    if ((long long)H > (long long)MSG_METRIC_MAX_SCALE * out_h || (long long)W > (long long)MSG_METRIC_MAX_SCALE * out_w)
        return MSG_EUNSUPPORTED;
    p->frames = t < 0 ? T : 1;
    p->tiles_y = (out_h + MI_TY - 1) / MI_TY;
    p->tiles_x = (out_w + MI_TX - 1) / MI_TX;
    if ((double)B * p->frames * p->tiles_y * p->tiles_x > 2147483647.0) return MSG_EINVAL;   // (what blockIdx.x can address)
    p->blocks = (long long)B * p->frames * p->tiles_y * p->tiles_x;
    p->count = (long long)p->frames * H * W;
    const long long even = (p->count + MI_MINMAX_PIECES - 1) / MI_MINMAX_PIECES;
    p->per = ((even > MI_MINMAX_MIN ? even : MI_MINMAX_MIN) + 7) & ~7ll;
    p->pieces = (int)((p->count + p->per - 1) / p->per);
    if ((double)B * p->pieces > 2147483647.0) return MSG_EINVAL;
    p->parts = norm == MSG_METRIC_NORM_SOURCE ? p->pieces : norm == MSG_METRIC_NORM_RESIZED ? p->blocks / B : 0;
    return MSG_OK;
}

extern "C" long long msg_metric_input_workspace(int B, int T, int H, int W, int t, int out_h, int out_w, int norm) {
    MetricPlan p;
    if (metric_plan(B, T, H, W, t, out_h, out_w, norm, &p) != MSG_OK) return -1;
    return 8ll * B * p.parts;
}

template <typename TI, typename TO>
static int metric_launch(const TI* images, TO* out, float* ws, const MetricPlan& p, int B, int C, int T, int H, int W,
                         int channel, int t, int planes, int out_h, int out_w, int norm, hipStream_t s) {
    constexpr int NIN = 16 / (int)sizeof(TI), NPX = 16 / (int)sizeof(TO);
    MetricGeom g;
    g.C = C; g.T = T; g.H = H; g.W = W; g.channel = channel; g.t = t; g.frames = p.frames; g.planes = planes;
    g.out_h = out_h; g.out_w = out_w; g.tiles_y = p.tiles_y; g.tiles_x = p.tiles_x; g.norm = norm; g.stats = 0;
    g.vec_in = W % NIN == 0 && (((uintptr_t)images) & 15u) == 0;
    g.vec_out = out_w % NPX == 0 && (((uintptr_t)out) & 15u) == 0;
    g.parts = p.parts;
    if (norm == MSG_METRIC_NORM_SOURCE) {
        const long long first = ((long long)channel * T + (t < 0 ? 0 : t)) * H * W;
        hipLaunchKernelGGL((metric_minmax_kernel<TI>), dim3((unsigned)((long long)B * p.pieces)), dim3(256), 0, s, images, ws,
                           (long long)C * T * H * W, first, p.count, p.per, p.pieces, g.vec_in);
    } else if (norm == MSG_METRIC_NORM_RESIZED) {
        g.stats = 1;
        hipLaunchKernelGGL((metric_input_kernel<TI, TO>), dim3((unsigned)p.blocks), dim3(256), 0, s, images, out, ws, g);
        g.stats = 0;
    }
    hipLaunchKernelGGL((metric_input_kernel<TI, TO>), dim3((unsigned)p.blocks), dim3(256), 0, s, images, out, ws, g);
    return MSG_CHECK_LAUNCH();
}

extern "C" int msg_metric_input(const void* images, int in_dtype, int B, int C, int T, int H, int W, int channel, int t,
                                void* out, int out_dtype, int planes, int out_h, int out_w, int norm, void* ws, void* stream) {
    if (!images || !out || C <= 0 || channel < 0 || channel >= C || (planes != 1 && planes != 3)) return MSG_EINVAL;
    if ((in_dtype != MSG_F32 && in_dtype != MSG_BF16) || (out_dtype != MSG_F32 && out_dtype != MSG_BF16)) return MSG_EINVAL;
    MetricPlan p;
    const int status = metric_plan(B, T, H, W, t, out_h, out_w, norm, &p);
    if (status != MSG_OK) return status;
    if (norm != MSG_METRIC_NORM_NONE && !ws) return MSG_EINVAL;
    // (the 64-bit element offsets below must not wrap)
    if ((double)B * C * T * H * W > 4.0e18 || (double)B * planes * p.frames * out_h * out_w > 4.0e18) return MSG_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    float* w = (float*)ws;
#define MI_GO(TI, TO) \
    return metric_launch<TI, TO>((const TI*)images, (TO*)out, w, p, B, C, T, H, W, channel, t, planes, out_h, out_w, norm, s)
    if (in_dtype == MSG_F32 && out_dtype == MSG_F32) MI_GO(float, float);
    if (in_dtype == MSG_F32) MI_GO(float, bf16_t);
    if (out_dtype == MSG_F32) MI_GO(bf16_t, float);
    MI_GO(bf16_t, bf16_t);
#undef MI_GO
}
