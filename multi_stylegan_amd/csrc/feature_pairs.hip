// Pairwise feature kernels of the sample-based validation metrics (validation_metrics.py: KID / KVD, manifold precision /
// recall / density / coverage): every pair (q_i, r_j) of two fp32 feature sets is formed and reduced on the spot -- the
// N x M matrix of products never reaches memory.
//
// One main loop, three epilogues.  A workgroup (256 lanes, 4 waves as 2 x 2) owns FP_T = 128 query rows and sweeps its slice
// of the set in tiles of FP_T rows.  Per tile the contraction runs over d in steps of FP_K = 32: both operands are staged
// through LDS (rows padded to FP_LD = 36 floats; 16-byte loads where the base and d allow, element by element otherwise, with
// the same bits; the next step's loads are issued before the current step's products), and every wave forms a 64 x 64 piece of
// Q R^T as 2 x 2 independent accumulators of __builtin_amdgcn_mfma_f32_32x32x2f32: exact fp32, a k-ordered fmaf chain per
// output.  The lane halves take k = 8 s + 4 h + e, so that one 16-byte LDS read feeds four instructions.
// Orientation: the SET is the A operand and the QUERIES are the B operand.  In the C/D layout (col = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)) a lane's column is then one query and its 16 registers run along the set:
// the k smallest distances, the minimum margin, the hit count and the kernel sum of a query are lane-local over the whole
// sweep, and are merged once at the end -- the two lane halves and the two waves that share a query, through LDS.
// Row norms |x|^2 come from the staged tiles (one fmaf chain per row in k order, the same bits whichever workgroup forms them).
// The grid is (query tiles, sweep slices, products); every workgroup leaves its partial results in the workspace and a small
// second launch merges the slices in slice order.  No atomics, no float reduction whose order depends on scheduling:
// bit-identical from run to run.
#include <math.h>
#include "msg_common.h"

constexpr int FP_T = 128;                 // query rows per workgroup = set rows per sweep tile
constexpr int FP_K = 32;                  // contraction step staged through LDS
constexpr int FP_LD = FP_K + 4;           // padded LDS row (floats): rows stay 16-byte aligned
constexpr int FP_KNN = 8;                 // neighbours kept per query
constexpr int FP_TARGET_BLOCKS = 512;     // workgroups the sweep split aims for (two per CU)
constexpr int FP_MAX_SLICES = 64;

enum { FP_MODE_KNN = 0, FP_MODE_BALL = 1, FP_MODE_MMD = 2 };

struct PairArgs {
    const float* q;  const float* r;      // KNN / BALL: the two sets.  MMD: x and y
    const int* qi;   const int* ri;       // MMD: ix [S][mx], iy [S][my] or NULL
    const float* radius2;                 // BALL
    void* ws;
    int nq, nr;                           // rows swept (MMD: mx, my)
    int src_q, src_r;                     // rows of the arrays behind them (MMD: nx, ny)
    int d, tiles_per_slice, slices;
    int exclude_self, vec;
    float gamma, coef0;
};

// sorted insertion into the k smallest, fully unrolled: no dynamic indexing, no scratch
__device__ __forceinline__ void fp_insert(float (&best)[FP_KNN], float v) {
#pragma unroll
    for (int i = 0; i < FP_KNN; ++i) {
        const float lo = fminf(best[i], v);
        v = fmaxf(best[i], v);
        best[i] = lo;
    }
}

// element offset of the row at position `pos` of an operand (-1: a zero row -- past the end, or an index outside its set)
__device__ __forceinline__ long long fp_row_offset(const int* idx, int pos, int n, int src_n, int d) {
    if (pos >= n) return -1;
    const long long row = idx ? (long long)idx[pos] : (long long)pos;
    if (row < 0 || row >= src_n) return -1;
    return row * (long long)d;
}

template <bool VEC>
__device__ __forceinline__ void fp_fetch(const float* base, const long long (&off)[4], int d, int k, f32x4 (&v)[4]) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
        if (off[p] >= 0) {
            const float* src = base + off[p] + k;
            if constexpr (VEC) {
                if (k < d) x = *reinterpret_cast<const f32x4*>(src);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (k + e < d) x[e] = src[e];
            }
        }
        v[p] = x;
    }
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void feature_pairs_kernel(PairArgs a) {
    // one LDS object: the two staged tiles, then the row norms and radii; the staged tiles are reused by the final merge
    __shared__ __attribute__((aligned(16))) float smem[2 * FP_T * FP_LD + 3 * FP_T];
    float* sQ = smem;
    float* sR = smem + FP_T * FP_LD;
    float* sQn = smem + 2 * FP_T * FP_LD;
    float* sRn = sQn + FP_T;
    float* sRad = sRn + FP_T;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wq = wave >> 1, wr = wave & 1, col = lane & 31, half = lane >> 5;
    const int qt = blockIdx.x, slice = blockIdx.y;
    const int q0 = qt * FP_T;

    const float* qbase = a.q;
    const float* rbase = a.r;
    const int* qidx = nullptr;
    const int* ridx = nullptr;
    int nq = a.nq, nr = a.nr, src_q = a.src_q, src_r = a.src_r;
    bool sym = false;
    if constexpr (MODE == FP_MODE_MMD) {
        // blockIdx.z = 3 subset + product: 0 = (x, x), 1 = (y, y), 2 = (x, y)
        const int subset = blockIdx.z / 3, prod = blockIdx.z - 3 * subset;
        const int* ix = a.qi ? a.qi + (long long)subset * a.nq : nullptr;
        const int* iy = a.ri ? a.ri + (long long)subset * a.nr : nullptr;
        if (prod == 0)      { rbase = a.q; ridx = qidx = ix; nr = a.nq; src_r = a.src_q; sym = true; }
        else if (prod == 1) { qbase = a.r; ridx = qidx = iy; nq = a.nr; src_q = a.src_r; sym = true; }
        else                { qidx = ix; ridx = iy; }
        if (q0 >= nq) {                                            // (the grid is sized for the longer of the two lists)
            if (t == 0)
                reinterpret_cast<double*>(a.ws)[((long long)blockIdx.z * gridDim.x + qt) * a.slices + slice] = 0.0;
            return;
        }
    }
    const int d = a.d;
    const int lrow = t >> 3, kcol = (t & 7) * 4;                   // staging: 32 rows x 32 k per pass, four passes per tile

    long long qoff[4], roff[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) qoff[p] = fp_row_offset(qidx, q0 + p * 32 + lrow, nq, src_q, d);

    // lane-local results of the whole sweep
    float best[2][FP_KNN];
    float margin[2] = {INFINITY, INFINITY};
    int hits[2] = {0, 0};
    double ksum = 0.0;
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int i = 0; i < FP_KNN; ++i) best[g][i] = INFINITY;

    const int tiles_r = (nr + FP_T - 1) / FP_T;
    const int rt_begin = slice * a.tiles_per_slice;
    const int rt_end = min(rt_begin + a.tiles_per_slice, tiles_r);
    for (int rt = rt_begin; rt < rt_end; ++rt) {
        if (sym && rt < qt) continue;                              // (symmetric products: the upper triangle of tiles, doubled)
        const int r0 = rt * FP_T;
#pragma unroll
        for (int p = 0; p < 4; ++p) roff[p] = fp_row_offset(ridx, r0 + p * 32 + lrow, nr, src_r, d);

        f32x16 acc[2][2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[g][s][e] = 0.f;
        float norm = 0.f;                                          // |row|^2 of staged row t & 127 (queries: t < 128)

        f32x4 vq[4], vr[4];
        fp_fetch<VEC>(qbase, qoff, d, kcol, vq);
        fp_fetch<VEC>(rbase, roff, d, kcol, vr);
        for (int k0 = 0; k0 < d; k0 += FP_K) {
            __syncthreads();                                       // the previous step's reads of the staged tiles are done
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                *reinterpret_cast<f32x4*>(sQ + (p * 32 + lrow) * FP_LD + kcol) = vq[p];
                *reinterpret_cast<f32x4*>(sR + (p * 32 + lrow) * FP_LD + kcol) = vr[p];
            }
            __syncthreads();
            if (k0 + FP_K < d) {                                   // the next step's loads fly during this step's products
                fp_fetch<VEC>(qbase, qoff, d, k0 + FP_K + kcol, vq);
                fp_fetch<VEC>(rbase, roff, d, k0 + FP_K + kcol, vr);
            }
            if constexpr (MODE != FP_MODE_MMD) {
                const float* row = (t < FP_T ? sQ : sR) + (t & (FP_T - 1)) * FP_LD;
#pragma unroll
                for (int kk = 0; kk < FP_K; kk += 4) {
                    const f32x4 x = *reinterpret_cast<const f32x4*>(row + kk);
#pragma unroll
                    for (int e = 0; e < 4; ++e) norm = fmaf(x[e], x[e], norm);
                }
            }
#pragma unroll
            for (int kk = 0; kk < FP_K; kk += 8) {
                f32x4 fa[2], fb[2];
#pragma unroll
                for (int s = 0; s < 2; ++s)
                    fa[s] = *reinterpret_cast<const f32x4*>(sR + (wr * 64 + s * 32 + col) * FP_LD + kk + 4 * half);
#pragma unroll
                for (int g = 0; g < 2; ++g)
                    fb[g] = *reinterpret_cast<const f32x4*>(sQ + (wq * 64 + g * 32 + col) * FP_LD + kk + 4 * half);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int g = 0; g < 2; ++g)
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            acc[g][s] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[s][e], fb[g][e], acc[g][s], 0, 0, 0);
            }
        }

        if constexpr (MODE != FP_MODE_MMD) {
            (t < FP_T ? sQn : sRn)[t & (FP_T - 1)] = norm;
            if constexpr (MODE == FP_MODE_BALL)
                if (t >= FP_T) sRad[t - FP_T] = (r0 + t - FP_T < nr) ? a.radius2[r0 + t - FP_T] : 0.f;
            __syncthreads();
        }

        // ---- the tile's 64 x 64 piece, reduced into the lane's results
        double tile_sum = 0.0;
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int lq = wq * 64 + g * 32 + col;
            const int gq = q0 + lq;
            const float qn = (MODE != FP_MODE_MMD) ? sQn[lq] : 0.f;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int lr = wr * 64 + s * 32 + (e & 3) + 8 * (e >> 2) + 4 * half;
                    const int gr = r0 + lr;
                    const float dot = acc[g][s][e];
                    if constexpr (MODE == FP_MODE_MMD) {
                        const float u = a.gamma * dot + a.coef0;
                        const float kv = (u * u) * u;
                        const bool take = gr < nr && gq < nq && !(sym && gr == gq);
                        tile_sum += take ? (double)kv : 0.0;
                    } else {
                        const float d2 = fmaxf(0.f, fmaf(-2.f, dot, qn + sRn[lr]));
                        if constexpr (MODE == FP_MODE_KNN) {
                            const bool take = gr < nr && !(a.exclude_self && gr == gq);
                            fp_insert(best[g], take ? d2 : INFINITY);
                        } else {
                            const float r2 = sRad[lr];
                            if (gr < nr) {
                                margin[g] = fminf(margin[g], d2 - r2);
                                hits[g] += (d2 <= r2) ? 1 : 0;
                            }
                        }
                    }
                }
            }
        }
        if constexpr (MODE == FP_MODE_MMD) ksum += (sym && rt > qt) ? 2.0 * tile_sum : tile_sum;
    }

    // ---- one merge: the four lanes (two halves x two waves along the set) that share a query, through LDS
    __syncthreads();
    if constexpr (MODE == FP_MODE_KNN) {
        float* lists = smem;                                       // [4][FP_T][FP_KNN]
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            float* dst = lists + ((wr * 2 + half) * FP_T + wq * 64 + g * 32 + col) * FP_KNN;
#pragma unroll
            for (int i = 0; i < FP_KNN; ++i) dst[i] = best[g][i];
        }
        __syncthreads();
        if (t < FP_T && q0 + t < nq) {
            float m[FP_KNN];
#pragma unroll
            for (int i = 0; i < FP_KNN; ++i) m[i] = INFINITY;
#pragma unroll
            for (int l = 0; l < 4; ++l)
#pragma unroll
                for (int i = 0; i < FP_KNN; ++i) fp_insert(m, lists[(l * FP_T + t) * FP_KNN + i]);
            float* dst = reinterpret_cast<float*>(a.ws) + ((long long)slice * nq + q0 + t) * FP_KNN;
#pragma unroll
            for (int i = 0; i < FP_KNN; ++i) dst[i] = m[i];
        }
    } else if constexpr (MODE == FP_MODE_BALL) {
        float* sm = smem;                                          // [4][FP_T] margins, then [4][FP_T] counts
        int* sc = reinterpret_cast<int*>(smem + 4 * FP_T);
#pragma unroll
        for (int g = 0; g < 2; ++g) {
            const int at = (wr * 2 + half) * FP_T + wq * 64 + g * 32 + col;
            sm[at] = margin[g];
            sc[at] = hits[g];
        }
        __syncthreads();
        if (t < FP_T && q0 + t < nq) {
            float m = sm[t];
            int c = sc[t];
#pragma unroll
            for (int l = 1; l < 4; ++l) {
                m = fminf(m, sm[l * FP_T + t]);
                c += sc[l * FP_T + t];
            }
            float* wm = reinterpret_cast<float*>(a.ws);
            int* wc = reinterpret_cast<int*>(a.ws) + (long long)a.slices * nq;
            wm[(long long)slice * nq + q0 + t] = m;
            wc[(long long)slice * nq + q0 + t] = c;
        }
    } else {
        double* sd = reinterpret_cast<double*>(smem);              // [256], a fixed tree
        sd[t] = ksum;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (t < s) sd[t] += sd[t + s];
            __syncthreads();
        }
        if (t == 0)
            reinterpret_cast<double*>(a.ws)[((long long)blockIdx.z * gridDim.x + qt) * a.slices + slice] = sd[0];
    }
}

// ---- second launch: the slices' partial results in slice order
__global__ void feature_knn_merge_kernel(const float* ws, float* out, int nq, int slices, int k) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    float m[FP_KNN];
#pragma unroll
    for (int i = 0; i < FP_KNN; ++i) m[i] = INFINITY;
    for (int s = 0; s < slices; ++s) {
        const float* src = ws + ((long long)s * nq + q) * FP_KNN;
#pragma unroll
        for (int i = 0; i < FP_KNN; ++i) fp_insert(m, src[i]);
    }
    float v = m[0];
#pragma unroll
    for (int i = 1; i < FP_KNN; ++i) v = (i == k - 1) ? m[i] : v;
    out[q] = v;
}

__global__ void feature_ball_merge_kernel(const void* ws, float* margin, int* count, int nq, int slices) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const float* wm = reinterpret_cast<const float*>(ws);
    const int* wc = reinterpret_cast<const int*>(ws) + (long long)slices * nq;
    float m = INFINITY;
    int c = 0;
    for (int s = 0; s < slices; ++s) {
        m = fminf(m, wm[(long long)s * nq + q]);
        c += wc[(long long)s * nq + q];
    }
    if (margin) margin[q] = m;
    if (count) count[q] = c;
}

// one lane per (subset, product): its workgroups' sums in (query tile, slice) order
__global__ void poly_mmd_merge_kernel(const double* ws, double* sums, int products, int per_product) {
    const int z = blockIdx.x * blockDim.x + threadIdx.x;
    if (z >= products) return;
    const double* src = ws + (long long)z * per_product;
    double s = 0.0;
    for (int i = 0; i < per_product; ++i) s += src[i];
    sums[z] = s;
}

// The sweep split: what both the workspace query and the entry derive from the sizes.
struct PairPlan {
    int tiles_q, tiles_r, tiles_per_slice, slices;
};

static void pair_plan(int nq, int nr, long long products, PairPlan* p) {
    p->tiles_q = (nq + FP_T - 1) / FP_T;
    p->tiles_r = (nr + FP_T - 1) / FP_T;
    const long long have = (long long)p->tiles_q * products;
    long long want = (FP_TARGET_BLOCKS + have - 1) / have;
    if (want > FP_MAX_SLICES) want = FP_MAX_SLICES;
    if (want > p->tiles_r) want = p->tiles_r;
    if (want < 1) want = 1;
    p->tiles_per_slice = (int)((p->tiles_r + want - 1) / want);
    p->slices = (p->tiles_r + p->tiles_per_slice - 1) / p->tiles_per_slice;
}

static bool pair_vec(const void* a, const void* b, int d) {
    return d % 4 == 0 && ((((uintptr_t)a) | ((uintptr_t)b)) & 15u) == 0;
}

template <int MODE>
static void pair_launch(const PairArgs& a, dim3 grid, hipStream_t s) {
    if (a.vec) hipLaunchKernelGGL((feature_pairs_kernel<MODE, true>), grid, dim3(256), 0, s, a);
    else       hipLaunchKernelGGL((feature_pairs_kernel<MODE, false>), grid, dim3(256), 0, s, a);
}

static int knn_check(int nq, int nr, int d, int k, int exclude_self) {
    if (nq <= 0 || nr <= 0 || d <= 0 || k < 1 || k > MSG_FEATURE_KNN_MAX) return MSG_EINVAL;
    if (exclude_self && nq != nr) return MSG_EINVAL;
    if (k > nr - (exclude_self ? 1 : 0)) return MSG_EINVAL;
    return MSG_OK;
}

extern "C" long long msg_feature_knn_workspace(int nq, int nr, int d, int k, int exclude_self) {
    if (knn_check(nq, nr, d, k, exclude_self) != MSG_OK) return -1;
    PairPlan p;
    pair_plan(nq, nr, 1, &p);
    return 4ll * FP_KNN * p.slices * nq;
}

extern "C" int msg_feature_knn(const float* q, int nq, const float* r, int nr, int d, int k, int exclude_self, float* out,
                               void* ws, void* stream) {
    if (!q || !r || !out || !ws) return MSG_EINVAL;
    const int status = knn_check(nq, nr, d, k, exclude_self);
    if (status != MSG_OK) return status;
    if (exclude_self && q != r) return MSG_EINVAL;
    if ((((uintptr_t)q) | ((uintptr_t)r) | ((uintptr_t)out) | ((uintptr_t)ws)) & 3u) return MSG_EINVAL;
    PairPlan p;
    pair_plan(nq, nr, 1, &p);
    PairArgs a = {};
    a.q = q; a.r = r; a.ws = ws; a.nq = a.src_q = nq; a.nr = a.src_r = nr; a.d = d;
    a.tiles_per_slice = p.tiles_per_slice; a.slices = p.slices;
    a.exclude_self = exclude_self ? 1 : 0; a.vec = pair_vec(q, r, d);
    hipStream_t s = (hipStream_t)stream;
    pair_launch<FP_MODE_KNN>(a, dim3((unsigned)p.tiles_q, (unsigned)p.slices, 1), s);
    hipLaunchKernelGGL(feature_knn_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const float*)ws, out, nq,
                       p.slices, k);
    return MSG_CHECK_LAUNCH();
}

extern "C" long long msg_feature_ball_hits_workspace(int nq, int nr, int d) {
    if (nq <= 0 || nr <= 0 || d <= 0) return -1;
    PairPlan p;
    pair_plan(nq, nr, 1, &p);
    return 8ll * p.slices * nq;
}

extern "C" int msg_feature_ball_hits(const float* q, int nq, const float* r, int nr, int d, const float* radius2, float* margin,
                                     int* count, void* ws, void* stream) {
    if (!q || !r || !radius2 || !ws || (!margin && !count)) return MSG_EINVAL;
    if (nq <= 0 || nr <= 0 || d <= 0) return MSG_EINVAL;
    if ((((uintptr_t)q) | ((uintptr_t)r) | ((uintptr_t)radius2) | ((uintptr_t)margin) | ((uintptr_t)count) | ((uintptr_t)ws)) & 3u)
        return MSG_EINVAL;
    PairPlan p;
    pair_plan(nq, nr, 1, &p);
    PairArgs a = {};
    a.q = q; a.r = r; a.radius2 = radius2; a.ws = ws; a.nq = a.src_q = nq; a.nr = a.src_r = nr; a.d = d;
    a.tiles_per_slice = p.tiles_per_slice; a.slices = p.slices; a.vec = pair_vec(q, r, d);
    hipStream_t s = (hipStream_t)stream;
    pair_launch<FP_MODE_BALL>(a, dim3((unsigned)p.tiles_q, (unsigned)p.slices, 1), s);
    hipLaunchKernelGGL(feature_ball_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, (const void*)ws, margin,
                       count, nq, p.slices);
    return MSG_CHECK_LAUNCH();
}

static int mmd_check(int nx, int ny, int d, int S, int mx, int my) {
    if (nx <= 0 || ny <= 0 || d <= 0 || S <= 0 || mx <= 0 || my <= 0) return MSG_EINVAL;
    if (3ll * S > 65535) return MSG_EINVAL;                        // (what blockIdx.z can address)
    return MSG_OK;
}

extern "C" long long msg_poly_mmd_workspace(int nx, int ny, int d, int S, int mx, int my) {
    if (mmd_check(nx, ny, d, S, mx, my) != MSG_OK) return -1;
    PairPlan p;
    pair_plan(mx > my ? mx : my, mx > my ? mx : my, 3ll * S, &p);
    return 8ll * 3 * S * p.tiles_q * p.slices;
}

extern "C" int msg_poly_mmd(const float* x, int nx, const float* y, int ny, int d, const int* ix, const int* iy, int S, int mx,
                            int my, float gamma, float coef0, double* sums, void* ws, void* stream) {
    if (!x || !y || !sums || !ws) return MSG_EINVAL;
    const int status = mmd_check(nx, ny, d, S, mx, my);
    if (status != MSG_OK) return status;
    if ((!ix && mx != nx) || (!iy && my != ny)) return MSG_EINVAL;
    if ((((uintptr_t)x) | ((uintptr_t)y) | ((uintptr_t)ix) | ((uintptr_t)iy)) & 3u) return MSG_EINVAL;
    if ((((uintptr_t)sums) | ((uintptr_t)ws)) & 7u) return MSG_EINVAL;
    const int m = mx > my ? mx : my;
    PairPlan p;
    pair_plan(m, m, 3ll * S, &p);
    PairArgs a = {};
    a.q = x; a.r = y; a.qi = ix; a.ri = iy; a.ws = ws; a.nq = mx; a.nr = my; a.src_q = nx; a.src_r = ny; a.d = d;
    a.tiles_per_slice = p.tiles_per_slice; a.slices = p.slices; a.vec = pair_vec(x, y, d);
    a.gamma = gamma; a.coef0 = coef0;
    hipStream_t s = (hipStream_t)stream;
    pair_launch<FP_MODE_MMD>(a, dim3((unsigned)p.tiles_q, (unsigned)p.slices, (unsigned)(3 * S)), s);
    hipLaunchKernelGGL(poly_mmd_merge_kernel, dim3((unsigned)((3 * S + 63) / 64)), dim3(64), 0, s, (const double*)ws, sums, 3 * S,
                       p.tiles_q * p.slices);
    return MSG_CHECK_LAUNCH();
}
