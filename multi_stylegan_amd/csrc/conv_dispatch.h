// Host-side dispatch of the convolution family (internal; included by the conv_*.hip files): the description of a problem,
// the answer to "which kernel runs it", and the prototype of every function one file of the family calls in another --
// declared here once, and seen by the definitions too, so that the compiler checks them (msg_bias_act_reduce_launch, which files
// outside the family call as well, is in msg_common.h).
//
// Forward convolutions and data gradients (msg_conv2d_fprop*): conv_fprop_select (conv_fprop.hip) is the only place that knows the
// order thin, upconv, row3, pp, generic.  Each kernel file gives it `bool conv_<k>_eligible(problem, ..., ConvPlan*)` holding ALL of
// that kernel's conditions (it fills the plan when it says yes) and `void conv_<k>_launch(problem, plan, pointers, stream)`, which
// cannot decline.  Every launch takes its plan from fprop_plan_for (conv_fprop.hip: the argument checks, written once, then
// conv_fprop_select), and so does the one query, msg_conv2d_fprop_launch_plan, which has the launch's own argument list.
// Weight gradients (msg_conv2d_wgrad*): the same shape.  conv_wgrad_select (conv_wgrad.hip) is the only place that knows the order
// row3, generic; a WgradPlan is a value -- kernel, K split, logical rows, grid, workspace -- that the launch, the workspace query and
// msg_conv2d_wgrad_plan all take from it.  `conv_wgrad_<k>_eligible(problem, WgradPlan*)` holds all of a kernel's conditions and
// fills the plan; `conv_wgrad_<k>_launch(problem, plan, pointers, stream)` fills the kernel's parameter struct from the two and
// cannot decline.  The K split is decided in this order: a k_chunks of MSG_WGRAD_K_AUTO becomes conv_wgrad_default_chunks (below)
// in wgrad_plan_for, before anything reads it, so the kernel files only ever see a positive number; then each kernel's own model,
// conv_wgrad_ksplit (below) with its constants, where that number has no say -- the row-sharing kernel when it is 1, and every
// shared-weight problem whose batch folds into K.
#pragma once
#include "msg_common.h"

struct ConvProblem {
    int dtype;                      // MSG_F32 or MSG_BF16 (MSG_F32_SPLIT arrives here as MSG_F32 with split = 3)
    int split;
    int B, IH, IW, Cx, Ck, OH, OW, N, ldy;
    int kh, kw, stride, pad, in_up, pixel_shuffle;
    long long w_batch_stride;       // elements between the weight sets of two samples; 0: one set for the batch

    bool per_sample() const { return w_batch_stride != 0; }
    int samples() const { return per_sample() ? B : 1; }                                   // grid.z of the tile kernels
    long long mtot() const { return per_sample() ? (long long)OH * OW : (long long)B * OH * OW; }   // GEMM rows of one grid.z slice
    int esz() const { return dtype == MSG_BF16 ? 2 : 4; }
    long long x_bstride() const { return (long long)IH * IW * Cx; }                        // elements per sample
    long long y_bstride() const { return (pixel_shuffle ? 4ll : 1ll) * OH * OW * ldy; }
    // what one buffer descriptor spans: the activations of the batch (of one sample with per-sample weights), one weight set
    long long x_bytes() const { return (long long)(per_sample() ? 1 : B) * IH * IW * Cx * esz(); }
    long long w_bytes() const { return (long long)N * kh * kw * Ck * esz(); }
    // the kernels that address through descriptors use 31-bit offsets (num_records 2^31 - 16, msg_make_desc)
    bool fits31() const { return x_bytes() < 0x7ffffff0ll && w_bytes() < 0x7ffffff0ll; }
};

enum ConvKernel {
    CONV_THIN_N, CONV_THIN_K,       // conv_thin.hip: streaming 1x1 kernels, <= 8 output / 8 input channels
    CONV_UPCONV,                    // conv_upconv.hip: activation-stationary sub-pixel up-convolution
    CONV_ROW3, CONV_ROW3N,          // conv_fprop_row3.hip: row-sharing 3x3, 256 x 256 / 128 x 128 tile
    CONV_PP,                        // conv_fprop_pp.hip: 256 x 256 ping-pong
    CONV_DMA, CONV_REG, CONV_REG_LEAN, CONV_REG_SPLIT   // conv_fprop.hip: 128 x 128 tile; LDS-DMA / register staging (+ lean, split-bf16)
};

struct ConvPlan {
    ConvKernel kernel;
    int tile_m, tile_n;             // output tile of the MFMA kernels (pixels x channels); 0 for the streaming kernels
    bool supported;                 // false: no kernel takes the problem (the generic kernel's own limits): MSG_EUNSUPPORTED
};

inline int conv_act_mode(const ActEpilogue* act) { return act ? act->enabled : 0; }

// The fields the tile kernels' parameter structs (ConvParams, ConvParamsPP, ConvParamsR3) share under one name.
template <typename P>
inline void conv_fill_common(P& p, const ConvProblem& q, const ActEpilogue* act) {
    p.B = q.B; p.IH = q.IH; p.IW = q.IW; p.Cx = q.Cx; p.Ck = q.Ck; p.OH = q.OH; p.OW = q.OW; p.N = q.N; p.ldy = q.ldy;
    p.per_sample = q.per_sample();
    if (act) p.act = *act;
    p.x_bstride = q.x_bstride();
    p.w_bstride = q.w_batch_stride;
    p.y_bstride = q.y_bstride();
    p.Mtot = (int)q.mtot();
}
// ... and the tap geometry of the two that take any (ConvParams, ConvParamsPP)
template <typename P>
inline void conv_fill_taps(P& p, const ConvProblem& q) {
    p.kh = q.kh; p.kw = q.kw; p.stride = q.stride; p.pad = q.pad; p.in_up = q.in_up; p.pixel_shuffle = q.pixel_shuffle;
}

ConvPlan conv_fprop_select(const ConvProblem& q, const ActEpilogue* act, bool has_bias);

// conv_thin.hip
bool conv_thin_eligible(const ConvProblem& q, const ActEpilogue* act, ConvPlan* plan);
void conv_thin_launch(const ConvProblem& q, const ConvPlan& plan, const void* x, const void* w, const float* bias, void* y,
                      const ActEpilogue* act, void* stream);
// conv_upconv.hip
bool conv_upconv_eligible(const ConvProblem& q, const ActEpilogue* act, bool has_bias, ConvPlan* plan);
void conv_upconv_launch(const ConvProblem& q, const ConvPlan& plan, const void* x, const void* w, void* y, void* stream);
// conv_fprop_row3.hip
bool conv_row3_eligible(const ConvProblem& q, const ActEpilogue* act, bool has_bias, ConvPlan* plan);
void conv_row3_launch(const ConvProblem& q, const ConvPlan& plan, const void* x, const void* w, const float* bias, void* y,
                      const ActEpilogue* act, void* stream);
// conv_fprop_pp.hip
bool conv_pp_eligible(const ConvProblem& q, ConvPlan* plan);
void conv_pp_launch(const ConvProblem& q, const ConvPlan& plan, const void* x, const void* w, const float* bias, void* y,
                    const ActEpilogue* act, void* stream);

// ---- weight gradients
struct WgradProblem {
    int dtype, split;               // MSG_F32 or MSG_BF16 (MSG_F32_SPLIT: MSG_F32 with split = 3)
    int B, IH, IW, Cx, I, OH, OW, ldgy, O, ldgw;
    int kh, kw, stride, pad, pixel_shuffle;
    int per_sample, k_chunks, oi_major;
    float gain;
    int esz() const { return dtype == MSG_BF16 ? 2 : 4; }
    long long gy_bytes() const { return (long long)(pixel_shuffle ? 4 : 1) * OH * OW * ldgy * esz(); }   // of one sample
    long long x_bytes() const { return (long long)IH * IW * Cx * esz(); }
    long long slab() const { return (long long)O * kh * kw * ldgw; }                      // floats of one result in the kernel layout
    long long gw_zstride() const { return oi_major ? (long long)O * I * kh * kw : slab(); }
};

enum WgradKernel {                  // (the values are the MSG_WPLAN_* codes of msg_hip.h)
    WGRAD_GENERIC, WGRAD_DMA, WGRAD_UNI,    // conv_wgrad.hip: 128 x 128 tile of one tap; incremental addressing / LDS-DMA staging (A/B) / uniform rows
    WGRAD_ROW3, WGRAD_ROW3_W32              // conv_wgrad_row3.hip: the three horizontal taps in one workgroup; maps of 64 k / exactly 32 columns
};

struct WgradPlan {                  // (value-initialised: the plan of an empty batch -- nothing to launch, no workspace)
    WgradKernel kernel;
    int nz, slice_pixels;           // K-slices in the grid, and the logical pixels of one
    int chunks_per_out, n_out;      // K-slices that add up to one result (> 1: slabs + the fixed-order reduce), and results
    int OWv, OHv;                   // logical row width / row count of the K loop (WgradParams)
    int fold, xcd_slices;           // the batch is folded into K; one K-slice per XCD
    long long blocks, need;         // workgroups of the contraction kernel; workspace floats (0: no split)
    bool supported;                 // false: the generic kernel's own grid limits: MSG_EUNSUPPORTED
};

// The K split both files use: the chunk count c in 1 .. max_chunks that minimises (rounds of `round_wgs` co-resident workgroups) x
// (K-steps per workgroup + fixed_steps + slab_steps when the sum is split); the first minimum wins, and no count beyond the first with
// more than max_wgs workgroups is tried.  by8: only 1, 8, 16, ... (K-slices dealt to the XCDs eight at a time).  wgs: per chunk.
struct WgradSplitModel { int round_wgs, fixed_steps, slab_steps; long long max_chunks, max_wgs; bool by8; };
inline long long conv_wgrad_ksplit(long long steps, long long wgs, const WgradSplitModel& m) {
    long long chunks = 1, best = -1;
    for (long long c = 1; c <= m.max_chunks; c += (m.by8 && c >= 8 ? 8 : 1)) {
        if (m.by8 && c > 1 && c < 8) continue;
        const long long rounds = (wgs * c + m.round_wgs - 1) / m.round_wgs;
        const long long cost = rounds * ((steps + c - 1) / c + m.fixed_steps + (c > 1 ? m.slab_steps : 0));
        if (best < 0 || cost < best) { best = cost; chunks = c; }
        if (wgs * c > m.max_wgs) break;
    }
    return chunks;
}

// What MSG_WGRAD_K_AUTO stands for: the k_chunks the Python layer used to compute and pass, as it was (a rule of its own, not
// conv_wgrad_ksplit: the plans of the models' layers depend on it).  The extents are positive here (wgrad_check).  0 for shared
// weights over more than 65535 samples: MSG_EINVAL, as the caller's own 0 is.
inline int conv_wgrad_default_chunks(const WgradProblem& q) {
    const long long kp = q.dtype == MSG_BF16 ? 64 : 32, npix = (long long)q.OH * q.OW;      // pixels per K-step, per sample
    // (128 x 128 tiles x taps x samples; counted up to 1024 -- every count from there on gives the same answers -- so that no
    //  extent can overflow the product)
    long long tiles = (long long)((q.O + 127ll) / 128) * ((q.I + 127ll) / 128);
    for (const int n : {q.kh, q.kw, q.B}) tiles = tiles < 1024 ? tiles * n : 1024;
    if (q.per_sample) {
        // one K sweep per (sample, tile, tap) unless that leaves most of the chip idle (the 512 -> 3 toRGB layers: 64
        // workgroups); then the pixels are split into K-slices
        if (tiles >= 256) return 1;
        return (int)std::max(1ll, std::min(npix / (16 * kp), 1024 / tiles));
    }
    // (shared weights: the batch is folded into K and the kernel's own model picks the slice count; this only matters where it cannot)
    long long chunks = std::max(1ll, std::min((npix + 4 * kp - 1) / (4 * kp), (1024 + tiles - 1) / tiles));
    while (q.B * chunks > 65535) --chunks;
    return (int)chunks;
}

WgradPlan conv_wgrad_select(const WgradProblem& q);
// conv_wgrad_row3.hip
bool conv_wgrad_row3_eligible(const WgradProblem& q, WgradPlan* plan);
void conv_wgrad_row3_launch(const WgradProblem& q, const WgradPlan& plan, const void* gy, const void* x, float* gw, float* ws,
                            void* stream);
