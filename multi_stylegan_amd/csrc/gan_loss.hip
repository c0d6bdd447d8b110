// The adversarial objectives of the step as one streaming pass per direction: the non-saturating logistic, Wasserstein and hinge
// losses of the reference, their weight-map forms and their CutMix (label-map) forms (multi_stylegan/loss.py:9-94, 97-196,
// 198-280).  The reference evaluates each as a chain of stock operators -- softplus / minimum, a broadcast multiply, a mean,
// and their three backward kernels -- about ten tiny launches per real / fake pair.  All of them are
//
//     out[0] = (1 / n_real) sum_i a_i  r(x_i)        (the "real" side; a generator loss is this side applied to fake predictions)
//     out[1] = (1 / n_fake) sum_i a'_i f(x_i)        (the "fake" side)
//
//     kind          r(x)              f(x)               r'(x)                           f'(x)
//     logistic      softplus(-x)      softplus(x)        -sigmoid(-x)                    sigmoid(x)
//     Wasserstein   -x                x                  -1                              1
//     hinge         -min(0, x - 1)    -min(0, -x - 1)    -1 (x < 1), -1/2 (x == 1), 0    1 (x > -1), 1/2 (x == -1), 0
//
// with a = a' = 1 (MSG_GAN_AUX_NONE), a_i = a'_i = w[i mod P] (MSG_GAN_AUX_WEIGHT: the reference's weight.view(1, 1, 1, H, W)
// broadcast, P = H W) or a_i = label_i, a'_i = 1 - label_i on ONE prediction tensor (MSG_GAN_AUX_LABEL).  The half slope at the
// hinge's kink is what torch.minimum's backward gives at a tie; a NaN prediction gives a NaN term (the hinge is written with
// compares, not with fminf, which would drop it); softplus is torch's threshold-20 form, log1p(exp(z)) below it.
//
// Summation order (the results are bit-identical from run to run, and do not depend on dtype or alignment either): the n
// elements are cut into groups of 8 consecutive ones; a group's terms are summed as a balanced tree; group g belongs to lane
// g % 256 of workgroup (g / 256) % G, G = gan_loss_blocks(n), which adds its groups in increasing order; the 256 lanes are
// combined by a butterfly over the wave and a fixed tree over the four waves; G == 1 writes the mean itself, otherwise the G
// partial sums go to the workspace and a one-workgroup-per-side second launch adds them in a fixed order.  No atomics.
// A full group of a 16-byte aligned tensor is loaded with 16-byte loads (one for bf16, two for fp32; the fp32 label / weight
// values likewise where they are contiguous and aligned); the ragged last group, and every group of a misaligned tensor, with
// scalar loads into the same registers -- the arithmetic behind the loads is one piece of code.
//
// Backward, one launch: grad_x[i] = ((g / n) a_i) r'(x_i) in the rounding order of torch's mean / mul / minimum backward
// (bit-identical to it for Wasserstein and hinge), g read from device memory; in label mode both sides add into the one
// gradient.  A zero slope or a zero label gives an exact zero.  bf16 is rounded to nearest even.
#include "msg_common.h"

// every product and sum below is rounded on its own: what a lane computes must not depend on which load path fed it (a fused
// multiply-add chosen in one copy of the arithmetic and not in the other would break "the same bits at any alignment")
#pragma clang fp contract(off)

constexpr int GL_GROUP = 8;                     // elements per lane and step
constexpr int GL_MAX_BLOCKS = 1024;             // partial sums per side

__host__ __device__ static inline int gan_loss_blocks(long long n) {
    const long long groups = (n + GL_GROUP - 1) / GL_GROUP;
    const long long b = (groups + 255) / 256;
    return b < 1 ? 1 : (b > GL_MAX_BLOCKS ? GL_MAX_BLOCKS : (int)b);
}

__device__ __forceinline__ float gl_softplus(float z) { return z > 20.f ? z : log1pf(expf(z)); }
// -min(0, t) with torch.minimum's NaN
__device__ __forceinline__ float gl_hinge(float t) { return t < 0.f ? -t : (t == t ? 0.f : t); }
// d min(0, t) / dt: 1, 1/2 at the tie, 0 (NaN stays NaN)
__device__ __forceinline__ float gl_hinge_slope(float t) { return t < 0.f ? 1.f : (t == 0.f ? 0.5f : (t == t ? 0.f : t)); }
__device__ __forceinline__ float gl_sigmoid(float x) {
    const float e = expf(-fabsf(x));            // in (0, 1]: no overflow at either end
    const float s = 1.f / (1.f + e);
    return x >= 0.f ? s : (x == x ? e * s : x);
}

template <int KIND, bool FAKE>
__device__ __forceinline__ float gl_term(float x) {
    if constexpr (KIND == MSG_GAN_LOGISTIC) return gl_softplus(FAKE ? x : -x);
    else if constexpr (KIND == MSG_GAN_WASSERSTEIN) return FAKE ? x : -x;
    else return gl_hinge(FAKE ? -x - 1.f : x - 1.f);
}
template <int KIND, bool FAKE>
__device__ __forceinline__ float gl_slope(float x) {
    if constexpr (KIND == MSG_GAN_LOGISTIC) return FAKE ? gl_sigmoid(x) : -gl_sigmoid(-x);
    else if constexpr (KIND == MSG_GAN_WASSERSTEIN) return FAKE ? 1.f : -1.f;
    else return FAKE ? gl_hinge_slope(-x - 1.f) : -gl_hinge_slope(x - 1.f);
}

__device__ __forceinline__ bool gl_aligned(const void* p) { return (((uintptr_t)p) & 15u) == 0; }

// x[e] = p[i0 + e], 0 past n.  `fast`: the group is full and p is 16-byte aligned
template <typename T>
__device__ __forceinline__ void gl_load8(const T* __restrict__ p, long long i0, long long n, bool fast, float* x) {
    if (fast) {
        if constexpr (sizeof(T) == 4) {
            const float4 lo = *reinterpret_cast<const float4*>(p + i0), hi = *reinterpret_cast<const float4*>(p + i0 + 4);
            x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w; x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
        } else {
            Vec16<T> v;
            v.raw = *reinterpret_cast<const uint4*>(p + i0);
#pragma unroll
            for (int e = 0; e < GL_GROUP; ++e) x[e] = v.get(e);
        }
    } else {
#pragma unroll
        for (int e = 0; e < GL_GROUP; ++e) x[e] = i0 + e < n ? load_as_f32<T>(p + i0 + e) : 0.f;
    }
}

template <typename T>
__device__ __forceinline__ void gl_store8(T* __restrict__ p, long long i0, long long n, bool fast, const float* d) {
    if (fast) {
        if constexpr (sizeof(T) == 4) {
            *reinterpret_cast<float4*>(p + i0) = make_float4(d[0], d[1], d[2], d[3]);
            *reinterpret_cast<float4*>(p + i0 + 4) = make_float4(d[4], d[5], d[6], d[7]);
        } else {
            Vec16<T> o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o.set2(e, d[2 * e], d[2 * e + 1]);
            *reinterpret_cast<uint4*>(p + i0) = o.raw;
        }
    } else {
#pragma unroll
        for (int e = 0; e < GL_GROUP; ++e)
            if (i0 + e < n) store_from_f32<T>(p + i0 + e, d[e]);
    }
}

// a[e] of the group at i0: the weight map's w[(i0 + e) mod P] (every index read is below P, also past n) or label[i0 + e]
template <int AUX>
__device__ __forceinline__ void gl_load_aux(const float* __restrict__ aux, long long i0, long long n, long long P, bool full,
                                            bool aux_vec, float* a) {
    if constexpr (AUX == MSG_GAN_AUX_WEIGHT) {
        long long j = i0 % P;
        if (aux_vec && full) {                  // P % 8 == 0: the group does not wrap
            gl_load8<float>(aux, j, P, true, a);
        } else {
#pragma unroll
            for (int e = 0; e < GL_GROUP; ++e) {
                a[e] = aux[j];
                j = j + 1 == P ? 0 : j + 1;
            }
        }
    } else if constexpr (AUX == MSG_GAN_AUX_LABEL) {
        gl_load8<float>(aux, i0, n, aux_vec && full, a);
    }
}

__device__ __forceinline__ float gl_tree8(const float* s) {
    return ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}

// the 256 lanes' values -> their sum in lane 0 (butterfly over each wave, then a fixed tree over the four waves)
__device__ __forceinline__ float gl_block_sum(float v, float* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// grid (max G, 2 sides); label mode: (G, 1), both sums from one read of the prediction.  ws: [2][ws_stride] partial sums
template <typename T, int KIND, int AUX>
__global__ __launch_bounds__(256) void gan_loss_kernel(const T* __restrict__ pred_real, const T* __restrict__ pred_fake,
                                                       const float* __restrict__ aux, float* __restrict__ out,
                                                       float* __restrict__ ws, long long n_real, long long n_fake, long long P,
                                                       int ws_stride) {
    __shared__ float lds[8];
    constexpr bool LABEL = AUX == MSG_GAN_AUX_LABEL;
    const int side = LABEL ? 0 : (int)blockIdx.y;
    const T* __restrict__ pred = side ? pred_fake : pred_real;
    const long long n = side ? n_fake : n_real;
    if (n == 0) {                                                           // an absent side
        if (blockIdx.x == 0 && threadIdx.x == 0) out[side] = 0.f;
        return;
    }
    const int G = gan_loss_blocks(n);
    if ((int)blockIdx.x >= G) return;
    const long long groups = (n + GL_GROUP - 1) / GL_GROUP;
    const bool vec = gl_aligned(pred);
    const bool aux_vec = AUX == MSG_GAN_AUX_NONE ? false : (gl_aligned(aux) && (AUX == MSG_GAN_AUX_LABEL || P % GL_GROUP == 0));
    float acc = 0.f, acc2 = 0.f;
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += (long long)G * 256) {
        const long long i0 = g * GL_GROUP;
        const bool full = i0 + GL_GROUP <= n;
        float x[GL_GROUP], a[GL_GROUP], s[GL_GROUP], s2[GL_GROUP];
        gl_load8<T>(pred, i0, n, vec && full, x);
        gl_load_aux<AUX>(aux, i0, n, P, full, aux_vec, a);
#pragma unroll
        for (int e = 0; e < GL_GROUP; ++e) {
            const bool valid = full || i0 + e < n;
            if constexpr (LABEL) {
                s[e] = valid ? a[e] * gl_term<KIND, false>(x[e]) : 0.f;
                s2[e] = valid ? (1.f - a[e]) * gl_term<KIND, true>(x[e]) : 0.f;
            } else {
                float t = side ? gl_term<KIND, true>(x[e]) : gl_term<KIND, false>(x[e]);
                if constexpr (AUX == MSG_GAN_AUX_WEIGHT) t *= a[e];
                s[e] = valid ? t : 0.f;
            }
        }
        acc += gl_tree8(s);
        if constexpr (LABEL) acc2 += gl_tree8(s2);
    }
    const float total = gl_block_sum(acc, lds);
    float total2 = 0.f;
    if constexpr (LABEL) total2 = gl_block_sum(acc2, lds + 4);
    if (threadIdx.x != 0) return;
    if (G == 1) {
        out[side] = total / (float)n;
        if constexpr (LABEL) out[1] = total2 / (float)n;
    } else {
        ws[(long long)side * ws_stride + blockIdx.x] = total;
        if constexpr (LABEL) ws[(long long)ws_stride + blockIdx.x] = total2;
    }
}

// grid (2): side blockIdx.x adds its G > 1 partial sums, lane l those at l, l + 256, ... in that order
__global__ __launch_bounds__(256) void gan_loss_reduce_kernel(const float* __restrict__ ws, float* __restrict__ out,
                                                              long long n_real, long long n_fake, int ws_stride) {
    __shared__ float lds[4];
    const int side = (int)blockIdx.x;
    const long long n = side ? n_fake : n_real;
    const int G = n > 0 ? gan_loss_blocks(n) : 0;
    if (G <= 1) return;                                                     // (written by the first launch)
    float v = 0.f;
    for (int k = threadIdx.x; k < G; k += 256) v += ws[(long long)side * ws_stride + k];
    const float total = gl_block_sum(v, lds);
    if (threadIdx.x == 0) out[side] = total / (float)n;
}

// grid (max blocks, 2 sides), one group per lane; label mode (blocks, 1).  A side whose gradient is not wanted has n = 0 here.
template <typename T, int KIND, int AUX>
__global__ __launch_bounds__(256) void gan_loss_backward_kernel(const T* __restrict__ pred_real, const T* __restrict__ pred_fake,
                                                                const float* __restrict__ aux,
                                                                const float* __restrict__ grad_out, T* __restrict__ grad_real,
                                                                T* __restrict__ grad_fake, long long n_real, long long n_fake,
                                                                long long P) {
    constexpr bool LABEL = AUX == MSG_GAN_AUX_LABEL;
    const int side = LABEL ? 0 : (int)blockIdx.y;
    const T* __restrict__ pred = side ? pred_fake : pred_real;
    T* __restrict__ grad = side ? grad_fake : grad_real;
    const long long n = side ? n_fake : n_real;
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * GL_GROUP;
    if (i0 >= n) return;
    const bool full = i0 + GL_GROUP <= n;
    const bool vec = gl_aligned(pred) && gl_aligned(grad);
    const bool aux_vec = AUX == MSG_GAN_AUX_NONE ? false : (gl_aligned(aux) && (AUX == MSG_GAN_AUX_LABEL || P % GL_GROUP == 0));
    const float c = grad_out[side] / (float)n;                              // torch's mean backward
    float x[GL_GROUP], a[GL_GROUP], d[GL_GROUP];
    gl_load8<T>(pred, i0, n, vec && full, x);
    gl_load_aux<AUX>(aux, i0, n, P, full, aux_vec, a);
    if constexpr (LABEL) {
        const float c2 = grad_out[1] / (float)n;
#pragma unroll
        for (int e = 0; e < GL_GROUP; ++e)
            d[e] = (c * a[e]) * gl_slope<KIND, false>(x[e]) + (c2 * (1.f - a[e])) * gl_slope<KIND, true>(x[e]);
    } else {
#pragma unroll
        for (int e = 0; e < GL_GROUP; ++e) {
            const float ca = AUX == MSG_GAN_AUX_WEIGHT ? c * a[e] : c;
            d[e] = ca * (side ? gl_slope<KIND, true>(x[e]) : gl_slope<KIND, false>(x[e]));
        }
    }
    gl_store8<T>(grad, i0, n, vec && full, d);
}

static bool gan_loss_args_ok(const void* pred_real, const void* pred_fake, const float* aux, int dtype, int kind, int aux_mode,
                             long long n_real, long long n_fake, long long P) {
    if (dtype != MSG_F32 && dtype != MSG_BF16) return false;
    if (kind != MSG_GAN_LOGISTIC && kind != MSG_GAN_WASSERSTEIN && kind != MSG_GAN_HINGE) return false;
    if (n_real < 0 || n_fake < 0 || (n_real == 0 && n_fake == 0)) return false;
    if ((n_real > 0) != (pred_real != nullptr)) return false;
    if (aux_mode != MSG_GAN_AUX_LABEL && (n_fake > 0) != (pred_fake != nullptr)) return false;
    if (n_real > (1ll << 40) || n_fake > (1ll << 40)) return false;         // (what the backward's block index can address)
    switch (aux_mode) {
    case MSG_GAN_AUX_NONE: return aux == nullptr;
    case MSG_GAN_AUX_WEIGHT: return aux != nullptr && P > 0;
    case MSG_GAN_AUX_LABEL:                                                 // one prediction tensor, read by both sides
        return aux != nullptr && n_real > 0 && n_fake == n_real && (pred_fake == nullptr || pred_fake == pred_real);
    default: return false;
    }
}

extern "C" long long msg_gan_loss_workspace(long long n_real, long long n_fake) {
    const int g = gan_loss_blocks(n_real > n_fake ? n_real : n_fake);
    return g > 1 ? 2ll * g : 0;
}

template <typename T, int KIND, int AUX>
static void gan_loss_launch(const T* pr, const T* pf, const float* aux, float* out, float* ws, long long nr, long long nf,
                            long long P, int G, hipStream_t s) {
    const dim3 grid((unsigned)G, AUX == MSG_GAN_AUX_LABEL ? 1 : 2);
    hipLaunchKernelGGL((gan_loss_kernel<T, KIND, AUX>), grid, dim3(256), 0, s, pr, pf, aux, out, ws, nr, nf, P, G);
    if (G > 1) hipLaunchKernelGGL(gan_loss_reduce_kernel, dim3(2), dim3(256), 0, s, ws, out, nr, nf, G);
}

template <typename T, int KIND, int AUX>
static void gan_loss_backward_launch(const T* pr, const T* pf, const float* aux, const float* gout, T* gr, T* gf, long long nr,
                                     long long nf, long long P, hipStream_t s) {
    const long long n = nr > nf ? nr : nf;
    const long long blocks = ((n + GL_GROUP - 1) / GL_GROUP + 255) / 256;
    const dim3 grid((unsigned)blocks, AUX == MSG_GAN_AUX_LABEL ? 1 : 2);
    hipLaunchKernelGGL((gan_loss_backward_kernel<T, KIND, AUX>), grid, dim3(256), 0, s, pr, pf, aux, gout, gr, gf, nr, nf, P);
}

// CALL(T, KIND, AUX) for the run-time (dtype, kind, aux_mode)
#define GL_DISPATCH_AUX(T, KIND, CALL)                                   \
    switch (aux_mode) {                                                  \
    case MSG_GAN_AUX_NONE: CALL(T, KIND, MSG_GAN_AUX_NONE); break;       \
    case MSG_GAN_AUX_WEIGHT: CALL(T, KIND, MSG_GAN_AUX_WEIGHT); break;   \
    default: CALL(T, KIND, MSG_GAN_AUX_LABEL); break;                    \
    }
#define GL_DISPATCH_KIND(T, CALL)                                                      \
    switch (kind) {                                                                    \
    case MSG_GAN_LOGISTIC: GL_DISPATCH_AUX(T, MSG_GAN_LOGISTIC, CALL) break;           \
    case MSG_GAN_WASSERSTEIN: GL_DISPATCH_AUX(T, MSG_GAN_WASSERSTEIN, CALL) break;     \
    default: GL_DISPATCH_AUX(T, MSG_GAN_HINGE, CALL) break;                            \
    }
#define GL_DISPATCH(CALL)                                  \
    if (dtype == MSG_BF16) { GL_DISPATCH_KIND(bf16_t, CALL) } \
    else { GL_DISPATCH_KIND(float, CALL) }

extern "C" int msg_gan_loss(const void* pred_real, const void* pred_fake, const float* aux, float* out, int dtype, int kind,
                            int aux_mode, long long n_real, long long n_fake, long long P, float* ws, long long ws_floats,
                            void* stream) {
    if (!out || !gan_loss_args_ok(pred_real, pred_fake, aux, dtype, kind, aux_mode, n_real, n_fake, P)) return MSG_EINVAL;
    const long long need = msg_gan_loss_workspace(n_real, n_fake);
    if (need > 0 && (!ws || ws_floats < need)) return MSG_EINVAL;
    const int G = gan_loss_blocks(n_real > n_fake ? n_real : n_fake);
    hipStream_t s = (hipStream_t)stream;
#define GL_FWD(T, KIND, AUX) \
    gan_loss_launch<T, KIND, AUX>((const T*)pred_real, (const T*)pred_fake, aux, out, ws, n_real, n_fake, P, G, s)
    GL_DISPATCH(GL_FWD)
#undef GL_FWD
    return MSG_CHECK_LAUNCH();
}

extern "C" int msg_gan_loss_backward(const void* pred_real, const void* pred_fake, const float* aux, const float* grad_out,
                                     void* grad_real, void* grad_fake, int dtype, int kind, int aux_mode, long long n_real,
                                     long long n_fake, long long P, void* stream) {
    if (!grad_out || !gan_loss_args_ok(pred_real, pred_fake, aux, dtype, kind, aux_mode, n_real, n_fake, P)) return MSG_EINVAL;
    if (aux_mode == MSG_GAN_AUX_LABEL) {
        if (!grad_real || grad_fake) return MSG_EINVAL;                     // both sides add into grad_real
    } else {
        if (!grad_real && !grad_fake) return MSG_EINVAL;
        if ((grad_real && n_real == 0) || (grad_fake && n_fake == 0)) return MSG_EINVAL;
        if (!grad_real) n_real = 0;                                         // that side's gradient is not wanted
        if (!grad_fake) n_fake = 0;
    }
    hipStream_t s = (hipStream_t)stream;
#define GL_BWD(T, KIND, AUX)                                                                                              \
    gan_loss_backward_launch<T, KIND, AUX>((const T*)pred_real, (const T*)pred_fake, aux, grad_out, (T*)grad_real, (T*)grad_fake, \
                                           n_real, n_fake, P, s)
    GL_DISPATCH(GL_BWD)
#undef GL_BWD
    return MSG_CHECK_LAUNCH();
}
