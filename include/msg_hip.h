/*
 * msg_hip.h -- C ABI of libmsg_hip.so: the MI355X (gfx950) kernels behind the
 * Multi-StyleGAN generator/discriminator hot path.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless it is named host_*;
 *   - `stream` is a hipStream_t passed as void*; launches are asynchronous on it,
 *     nothing here synchronises, allocates or keeps state between calls;
 *   - inputs are borrowed, outputs are caller-allocated and fully overwritten
 *     unless the entry says "accumulates";
 *   - return value: MSG_OK (0) or a negative MSG_E* code -- an unsupported
 *     configuration is an error, never a silent no-op (the reference silently
 *     launches nothing for unmatched modes: op_static/upfirdn2d_kernel.cu:172-211);
 *   - dtype: MSG_F32 or MSG_BF16 storage; arithmetic is always fp32.  The two entries that replace the
 *     reference's CUDA modules (msg_upfirdn2d[_pitched], msg_fused_bias_act) take every type of
 *     AT_DISPATCH_FLOATING_TYPES_AND_HALF (op_static/upfirdn2d_kernel.cu:225, op_static/fused_bias_act_kernel.cu:79):
 *     also MSG_F16 (`half`; fp32 arithmetic) and MSG_F64 (`double`: storage AND arithmetic in float64, and the `fir` /
 *     `bias` operands then point to float64 values too, as the reference's kernel / bias tensors share the input's
 *     dtype -- the precision torch.autograd.gradcheck needs).  msg_bias_act_backward takes MSG_F16 as well.
 *
 * Each entry cites the reference interface it replaces (paths relative to the
 * reference repository root).
 */
#ifndef MSG_HIP_H
#define MSG_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

enum { MSG_OK = 0, MSG_EINVAL = -1, MSG_EUNSUPPORTED = -2, MSG_ELAUNCH = -3 };
enum { MSG_F32 = 0, MSG_BF16 = 1, MSG_F16 = 2, MSG_F64 = 3, MSG_F32_SPLIT = 4 };
/* MSG_F32_SPLIT (msg_conv2d_fprop* / msg_conv2d_wgrad* only): fp32 STORAGE like MSG_F32, but every product of the contraction
 * is taken as SIX bf16 MFMA products with fp32 accumulation: x = xh + xm + xl, w = wh + wm + wl (xh = bf16(x), xm = bf16(x - xh),
 * xl = bf16(x - xh - xm): all 24 mantissa bits), x w ~ xh wh + xh wm + xm wh + xh wl + xl wh + xm wm -- everything down to
 * 2^-16 of the leading product; the error is at fp32-rounding level (the exact-fp32 MFMA of MSG_F32 runs at a sixteenth of the
 * bf16 matrix rate, this at a sixth).  Workspaces and layouts are those of MSG_F32.  (A three-product form on (hi, lo) splits
 * was built too: 16 mantissa bits per operand move the training step's gradients by up to 1e-2 -- not a parity path; removed.) */

/* Library/ABI version and the code-object architecture it was built for ("gfx950").  A caller compiled against this header
 * compares msg_abi_version() with MSG_ABI_VERSION before its first launch (workspace sizes and argument lists change with it):
 *   3  deterministic reductions (workspace arguments of msg_conv2d_wgrad, msg_bias_act_backward)
 *   4  msg_scale_reduce_channels / msg_scale_bias_act removed; msg_rgb_skip_merge(+_backward) and MSG_F32_SPLIT added;
 *      msg_affine_warp's backward workspace is B*C*H*W + 1 words (the last one is the poison word)
 *   5  round-5 entries (marked "ABI 5" below) */
#define MSG_ABI_VERSION 5
int msg_abi_version(void);
const char* msg_build_arch(void);
/* Text for a MSG_E* code. */
const char* msg_strerror(int code);

/* ---------------------------------------------------------------------------
 * a1  upfirdn2d -- replaces upfirdn2d_cuda.upfirdn2d
 *     (multi_stylegan/op_static/upfirdn2d.cpp:12-19 -> upfirdn2d_op,
 *      multi_stylegan/op_static/upfirdn2d_kernel.cu:140-272).
 * x   [major, in_h, in_w, minor]   (NCHW planes: major=B*C, minor=1;
 *                                   channels-last: major=B, minor=C)
 * fir [kh, kw] float32 (un-flipped, exactly what the reference passes)
 * y   [major, out_h, out_w, minor], out = (in*up + pad0 + pad1 - k) / down + 1
 * Zero-insert by up, pad (negative = crop), true convolution with fir, keep
 * every down-th sample.  Any up/down/pad/k combination is accepted (fast
 * paths: k<=4x4 with (up,down) in {(1,1),(2,1),(1,2)} and minor % vec == 0).
 * ------------------------------------------------------------------------- */
int msg_upfirdn2d(const void* x, const float* fir, void* y, int dtype,
                  int major, int in_h, int in_w, int minor, int kh, int kw,
                  int up_x, int up_y, int down_x, int down_y,
                  int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* msg_upfirdn2d whose input pixels are `in_pitch` (>= minor) elements apart: a channel-slice of a wider channels-last
 * map, e.g. the gradient of one piece of a channel concatenation, filtered in place instead of being compacted first. */
int msg_upfirdn2d_pitched(const void* x, const float* fir, void* y, int dtype,
                          int major, int in_h, int in_w, int minor, int in_pitch, int kh, int kw,
                          int up_x, int up_y, int down_x, int down_y,
                          int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* msg_upfirdn2d_pitched whose OUTPUT pixels are `out_pitch` (>= minor) elements apart as well: the result is written
 * straight into its channel-slice of the map it is concatenated into (u_net_2d_discriminator.py:128-131 in the
 * reference: torch.cat of the upsampled features and the encoder's skip features). */
int msg_upfirdn2d_pitched2(const void* x, const float* fir, void* y, int dtype,
                           int major, int in_h, int in_w, int minor, int in_pitch, int out_pitch, int kh, int kw,
                           int up_x, int up_y, int down_x, int down_y,
                           int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* msg_upfirdn2d for up = down = 1 and a SEPARABLE 4x4 FIR given by its factors (fir2d = fir_y fir_x^T, which is how
 * every FIR of the models is built: multi_stylegan_generator.py:244-258, u_net_2d_discriminator.py:186-203), on a
 * channels-last map (major = B, minor = C, minor % vec == 0).  Sliding-window evaluation, 8 instead of 16 taps per
 * output; results equal msg_upfirdn2d's up to fp32 re-association.  Other shapes: MSG_EUNSUPPORTED (use msg_upfirdn2d). */
int msg_upfirdn2d_separable(const void* x, const float* fir_y, const float* fir_x, void* y, int dtype,
                            int major, int in_h, int in_w, int minor, int kh, int kw,
                            int pad_x0, int pad_x1, int pad_y0, int pad_y1, void* stream);

/* msg_upfirdn2d_separable with the activation stage of the layer that owns the blur fused behind it:
 *   y = leaky_relu(blur(x) + noise_weight[0] * noise[b or 0, pixel] + act_bias[c], alpha) * scale
 * (the upsampling StyledConv2d: transposed conv -> Blur -> NoiseInjection -> FusedLeakyReLU,
 * multi_stylegan_generator.py:267-292,329-344).  The activation sees the fp32 blur result, i.e. one rounding less than
 * msg_upfirdn2d_separable followed by msg_fused_bias_act (within one unit in the last place of the storage type). */
int msg_upfirdn2d_separable_act(const void* x, const float* fir_y, const float* fir_x, void* y, int dtype,
                                int major, int in_h, int in_w, int minor, int kh, int kw,
                                int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                                const float* act_bias, const float* noise, const float* noise_weight,
                                int noise_batch, float alpha, float scale, void* stream);
/* ... which also leaves the SIGN BYTES of its output for the activation's backward (bf16, minor % 8 == 0; mask may be NULL):
 * mask [major * out_h * out_w][minor / 8] (tile 1 x minor in msg_bias_act_backward_mask's terms), bit e of byte
 * (pixel, c / 8) = (y[pixel][c + e] > 0) -- everything
 * FusedLeakyReLUFunctionBackward (op_static/fused_act.py:22-51) reads of `out`, at a sixteenth of its size; see
 * msg_bias_act_backward_mask. */
int msg_upfirdn2d_separable_act_mask(const void* x, const float* fir_y, const float* fir_x, void* y, int dtype,
                                     int major, int in_h, int in_w, int minor, int kh, int kw,
                                     int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                                     const float* act_bias, const float* noise, const float* noise_weight,
                                     int noise_batch, float alpha, float scale, unsigned char* mask, void* stream);

/* ---------------------------------------------------------------------------
 * a2  fused bias + (noise) + leaky-ReLU -- replaces fused_act_cuda.fused_bias_act
 *     (multi_stylegan/op_static/fused_bias_act.cpp:11-17 -> fused_bias_act_op,
 *      multi_stylegan/op_static/fused_bias_act_kernel.cu:18-99) and fuses the
 *     NoiseInjection add in front of it (multi_stylegan_generator.py:288-292).
 * x, y   flat [size_x]; bias index of element i is (i / step_b) % size_b
 *        (NCHW: step_b = H*W; channels-last or [B,C]: step_b = 1).
 * bias   [size_b] float32 or NULL.
 * ref    flat [size_x] or NULL; with grad=1 the slope is chosen by sign(ref)
 *        (the saved forward OUTPUT) instead of sign(x+b): kernel.cu:44.
 * noise  NULL, or float32 [noise_batch(1 or B), pix] added as
 *        (*noise_weight) * noise[pixel(i)] before the bias; pixel(i) is
 *        (i / step_b / size_b) * pix + i % step_b   for NCHW  (pix = step_b)
 *        i / size_b                                  for channels-last (step_b == 1)
 *        and wraps modulo `pix` when noise_batch == 1.
 * act    3 = leaky ReLU (the only activation the reference ever uses), 1 = linear.
 * grad   0 forward, 1 first derivative (needs ref), 2 -> zeros.
 * y = act(x + w*noise + b) * scale, computed in fp32.
 * ------------------------------------------------------------------------- */
int msg_fused_bias_act(const void* x, const float* bias, const void* ref, void* y, int dtype,
                       long long size_x, int step_b, int size_b,
                       const float* noise, const float* noise_weight, int noise_batch, int pix,
                       int act, int grad, float alpha, float scale, void* stream);

/* ---------------------------------------------------------------------------
 * a2  backward of the above with its reductions -- replaces
 *     FusedLeakyReLUFunctionBackward.forward (multi_stylegan/op_static/fused_act.py:24-42:
 *     one fused_bias_act(grad=1) call + grad_input.sum(dim) in PyTorch).
 * gx = gy * scale * (out > 0 ? 1 : alpha);  grad_bias[c] = sum gx;
 * grad_noise_weight[0] = sum gx * noise[pixel]   (if noise != NULL).
 * grad_bias / grad_noise_weight are float32 and OVERWRITTEN.  The sums are deterministic: workgroups leave partial sums
 * in `ws` (float32, at least msg_bias_act_backward_workspace(...) elements, contents irrelevant) and a second launch adds
 * them in index order -- no float atomics, bit-identical results for identical inputs.  ws may be NULL when neither sum
 * is requested.
 * ------------------------------------------------------------------------- */
long long msg_bias_act_backward_workspace(long long size_x, int step_b, int size_b, int has_noise);
int msg_bias_act_backward(const void* gy, const void* out, void* gx, int dtype,
                          long long size_x, int step_b, int size_b,
                          float* grad_bias, const float* noise, float* grad_noise_weight,
                          int noise_batch, int pix, float alpha, float scale,
                          float* ws, long long ws_floats, void* stream);
/* sums[c] = sum over the pixels of a channels-last map x [size_x / C][C]: the bias gradient of a convolution with no activation
 * behind it (`F.conv2d(..., bias)` of the discriminator's strided convs, multi_stylegan/equalized_layer.py:63-74).  fp32,
 * overwritten, deterministic (workspace and second stage of msg_bias_act_backward: ws_floats >=
 * msg_bias_act_backward_workspace(size_x, 1, C, 0)).  MSG_F32 / MSG_BF16, C a whole number of 16-byte vectors. */
int msg_channel_sums(const void* x, float* sums, int dtype, long long size_x, int C, float* ws, long long ws_floats,
                     void* stream);
/* msg_bias_act_backward for a channels-last bf16 map (step_b = 1, size_b % 8 == 0) whose forward launch left the sign
 * bytes of its output (msg_conv2d_fprop_act_mask / msg_upfirdn2d_separable_act_mask): `mask` replaces `out` -- the pass
 * moves 2 1/16 instead of 3 maps.  The bytes lie in the PRODUCER's tile order: tiles of tile_m consecutive pixels x tile_n
 * channels one after the other, [tile_m][tile_n / 8] bytes each, pixel tiles outermost (a workgroup of the producer writes one
 * contiguous block); tile 1 x size_b is the plain [pixel][size_b / 8] map.  Same results bit for bit (the bytes are the test
 * `out > 0` on the stored values), same workspace (msg_bias_act_backward_workspace(size_x, 1, size_b, has_noise)). */
int msg_bias_act_backward_mask(const void* gy, const unsigned char* mask, int tile_m, int tile_n, void* gx, int dtype,
                               long long size_x, int size_b,
                               float* grad_bias, const float* noise, float* grad_noise_weight,
                               int noise_batch, int pix, float alpha, float scale,
                               float* ws, long long ws_floats, void* stream);
/* (ABI 5) out[c] = sum_r part[r][cols], r in index order (fp32, deterministic): the second stage of the partial-sum reductions as an
 * entry of its own -- e.g. the [groups][B][I] style-gradient partials of msg_modulate_backward. */
int msg_sum_rows(const float* part, float* out, long long rows, int cols, void* stream);
/* (ABI 5) msg_bias_act_backward_mask for the output of a styled layer that ALSO feeds the level's image head -- a 1x1 modulated
 * conv without demodulation to n_head <= 8 planes (reference: OutputBlock, multi_stylegan_generator.py:513-523, reading the
 * StyledConv2d output of :384-411).  The head's data gradient is formed inside this pass instead of being written as a full map
 * and summed by autograd:
 *     gx = (gy + h) * scale * (out > 0 ? 1 : alpha),   h[q][c] = wscale * style[b][c] * sum_o ghead[q][o] * whead[o][c]
 * gy: the other consumer's gradient (bf16 [pixels][size_b]) or NULL; ghead: bf16 [pixels][8], planes >= n_head padding; whead fp32
 * [n_head][size_b]; style fp32 [pixels / pix][size_b]; pix = pixels per sample (a workgroup's pixel range must lie inside one
 * sample: MSG_EUNSUPPORTED otherwise, as for anything but bf16).  Sums, workspace and determinism as msg_bias_act_backward_mask. */
int msg_bias_act_backward_mask_head(const void* gy, const void* ghead, const float* whead, const float* style,
                                    float wscale, int n_head, const unsigned char* mask, int tile_m, int tile_n,
                                    void* gx, int dtype, long long size_x, int size_b,
                                    float* grad_bias, const float* noise, float* grad_noise_weight,
                                    int noise_batch, int pix, float alpha, float scale,
                                    float* ws, long long ws_floats, void* stream);

/* ---------------------------------------------------------------------------
 * a3/a4  dense contractions on the matrix cores (channels-last, implicit GEMM).
 * The reference has no native boundary here: it calls F.conv2d / F.conv_transpose2d with groups = batch
 * (multi_stylegan/multi_stylegan_generator.py:391-411) and F.conv2d / F.linear for the equalized layers
 * (multi_stylegan/equalized_layer.py:63-74, 244-254).  These two entries sit behind ModulatedConv2d.forward,
 * EqualizedConv2d.forward and EqualizedLinear.forward.
 *
 * msg_conv2d_fprop:
 *   y[b,oh,ow,n] = bias[n] + sum_{kh,kw,c} x[b, (oh*stride+kh-pad)/in_up, (ow*stride+kw-pad)/in_up, c] * w[(b)][n][kh][kw][c]
 *   x  [B, IH, IW, Cx]   Cx = channel stride (multiple of 16 B); channels >= the real count must hold finite values
 *   w  [(B)][N][kh*kw][Ck]  Ck = input channels zero-padded to a multiple of 128 B; w_batch_stride = 0 -> shared
 *   y  [B, OH, OW, ldy]  (pixel_shuffle = 1: N = 4*O and y is [B, 2*OH, 2*OW, ldy] with
 *                         y[b, 2oh+dy, 2ow+dx, o] = result[n = (2dy+dx)*O + o] -- the 2x2 stride-2 transposed conv)
 *   in_up > 1 (stride must be 1): samples exist only where the numerator is divisible (transposed strided conv).
 *   Data gradients are the same entry with the caller's re-laid weights.
 * msg_conv2d_wgrad:
 *   gw[(b)][o][tap][i] (+)= sum_{pixels} gy[b,oh,ow,o] * x[b, oh*stride+kh-pad, ow*stride+kw-pad, i]
 *   gw fp32 [(B)][O][kh*kw][ldgw] (ldgw % 4 == 0), OVERWRITTEN; per_sample = 1: one result per sample, otherwise ONE result
 *   for the whole batch.  k_chunks (the same in msg_conv2d_wgrad_workspace and msg_conv2d_wgrad_plan):
 *     MSG_WGRAD_K_AUTO  the library's own split for this problem -- what callers pass unless they have a reason not to.  It is
 *                       resolved to a positive number first (for per-sample weights one K sweep per sample, or a few K-slices
 *                       where that leaves most of the chip idle; for shared weights at most 65535 / B), and the call then
 *                       goes on exactly as if the caller had passed that number.  Shared weights with more than 65535 samples
 *                       resolve to 0 slices: MSG_EINVAL, as k_chunks = 0 is.
 *     k_chunks >= 1     per_sample = 1: the pixels of a sample are split into k_chunks K-slices (on the kh x 3 row-sharing
 *                       kernel 1 means "no opinion": that kernel's own model chooses).  per_sample = 0: the library folds the batch into K and chooses
 *                       the number of K-slices itself; k_chunks slices per sample only where folding is impossible (2^31 pixels
 *                       or more in the batch).
 *     0, or any other negative value: MSG_EINVAL.
 *   A result that is the sum of several K-slices is formed deterministically: every slice stores its partial result into
 *   its own slab of `ws` (float32, at least msg_conv2d_wgrad_workspace(...) elements -- 0 when nothing is split; contents
 *   irrelevant) and a second launch adds the slabs in slice order.  No float atomics: identical inputs give bit-identical
 *   gradients (the reference's cuDNN weight gradients are not deterministic; its training step is what ours must match).
 *   pixel_shuffle = 1: OH,OW are the LOW-res extent, gy is [B,2*OH,2*OW,ldgy], tap = (dy,dx).
 *   oi_major = 1 writes gw[(b)][o][i][tap] (the parameter's own [O,I,kh,kw] layout) instead; gain multiplies the result.
 * ------------------------------------------------------------------------- */
int msg_conv2d_fprop(const void* x, const void* w, const float* bias, void* y, int dtype,
                     int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int ldy,
                     int kh, int kw, int stride, int pad, int in_up, int pixel_shuffle,
                     long long w_batch_stride, void* stream);
enum { MSG_WGRAD_K_AUTO = -1 };
int msg_conv2d_wgrad(const void* gy, const void* x, float* gw, int dtype,
                     int B, int IH, int IW, int Cx, int I, int OH, int OW, int ldgy, int O, int ldgw,
                     int kh, int kw, int stride, int pad, int pixel_shuffle,
                     int per_sample, int k_chunks, int oi_major, float gain,
                     float* ws, long long ws_floats, void* stream);
/* Workspace elements (float32) the call above needs for the same geometry; negative = MSG_E* code. */
long long msg_conv2d_wgrad_workspace(int dtype, int B, int IH, int IW, int Cx, int I, int OH, int OW, int ldgy,
                                     int O, int ldgw, int kh, int kw, int stride, int pad, int pixel_shuffle,
                                     int per_sample, int k_chunks);

/* ---------------------------------------------------------------------------
 * a3  weight modulation / demodulation of the dual-styled conv (multi_stylegan/multi_stylegan_generator.py:379-388).
 * The reference does this with elementwise torch ops on a [B,O,I,kh,kw] tensor; these entries write the per-sample
 * weights directly in the contraction kernels' layouts and turn per-sample weight gradients back into parameter and
 * style gradients (including the derivative of the demodulation norm).
 *   msg_demod_coeff:       d[b,o] = rsqrt(scale^2 * sum_{i,t} (W[o,i,t]*s[b,i])^2 + eps);  W [O][I][taps], s [B][I]
 *   msg_scale_rows_cols:   out[b][r][t][c] = gain * base[r][t][c] * rowscale[b][r] * colscale[b][c], c >= C -> 0;
 *                          base fp32 [R][T][C]; rowscale/colscale fp32 or NULL (= 1); out [B][R][T][Ck] f32/bf16
 *   msg_modulate_backward: gwk fp32 [B][O][taps][ldg] (per-sample dL/dw, w = d*scale*W*s) ->
 *                          gW fp32 [O][I][taps] (overwritten) and gs_part fp32 [ceil(O/o_group)][B][I] (overwritten;
 *                          the caller sums over the first axis); d = NULL means "no demodulation".
 *                          Limits: I <= 512, taps <= 9, B <= 16 (else MSG_EUNSUPPORTED).
 * ------------------------------------------------------------------------- */
int msg_demod_coeff(const float* W, const float* s, float* d, int B, int O, int I, int taps,
                    float scale, float eps, void* stream);
int msg_scale_rows_cols(const float* base, const float* rowscale, const float* colscale, void* out,
                        int dtype, int B, int R, int T, int C, int Ck, float gain, void* stream);
/* Demodulation coefficients + forward per-sample weights in one launch (supersedes msg_demod_coeff followed by
 * msg_scale_rows_cols on the forward path): wsq [O][C] = sum over taps of W^2 (cached by the caller per weight update),
 * base [R][T][C] (R = O, or 4*O for the 2x2 transposed conv), style [B][C];
 * out[b][r][t][c] = scale * d[b][r % O] * base[r][t][c] * style[b][c],  d_out[b][o] = d (may be NULL). */
int msg_modulate_weights(const float* base, const float* wsq, const float* style, void* out, float* d_out,
                         int dtype, int B, int R, int O, int T, int C, int Ck, float scale, float eps, void* stream);
int msg_modulate_backward(const float* gwk, const float* W, const float* s, const float* d, float* gW,
                          float* gs_part, int B, int O, int I, int taps, int ldg, int o_group,
                          float scale, void* stream);
/* Second order of the same (the path-length regulariser differentiates the style gradient of the first backward once more,
 * multi_stylegan_generator.py:193-200 through :384-388): for a cotangent v [B][I] of the style gradient gs,
 *   msg_scale_rows_cols2:   out[b][r][t][c] = gain * base[r][t][c] * (row1[b][r]*col1[b][c] + row2[b][r]*col2[b][c]) -- with
 *                           (row1,col1,row2,col2) = (d, v, dd, s), dd[b][o] = -scale^2 d^3 sum_i s v wsq[o][i], the derivative of
 *                           the per-sample weight set along v (= dL2/d gwk), in the contraction kernels' layouts;
 *   msg_modulate_backward2: dL2/dW -> gW [O][I][taps] and dL2/ds -> gs_part [ceil(O/o_group)][B][I] at fixed gwk, L2 = <v, gs>
 *                           (both overwritten; d = NULL: no demodulation).  Limits: I % 4 == 0, I <= 512, taps in {1,4,9},
 *                           B <= 16, 16-byte aligned operands (else MSG_EUNSUPPORTED).                                        */
int msg_scale_rows_cols2(const float* base, const float* row1, const float* col1, const float* row2, const float* col2,
                         void* out, int dtype, int B, int R, int T, int C, int Ck, float gain, void* stream);
int msg_modulate_backward2(const float* gwk, const float* W, const float* s, const float* d, const float* v,
                           float* gW, float* gs_part, int B, int O, int I, int taps, int ldg, int o_group,
                           float scale, void* stream);

/* Every K-contiguous image the contraction / modulation kernels read from ONE parameter, in one pass (all outputs
 * optional): w [O][I][T] fp32 as the reference stores it (equalized_layer.py, multi_stylegan_generator.py:330);
 * fwd [O][T][Ck] (t_major: [T][O][Ck]) = gain*w zero-padded in i; dgrad [I][T][Ok] with the taps flipped when flip != 0,
 * zero-padded in o; wsq [O][I] = sum over taps of w^2.  fwd/dgrad in `dtype`.  T <= 16. */
int msg_relayout_weight(const float* w, void* fwd, void* dgrad, float* wsq, int dtype,
                        int O, int I, int T, int Ck, int Ok, int flip, int t_major, float gain, void* stream);

/* Tap gathering for convolutions with very few input channels (the discriminator's first layer, 6 channels):
 * y[b][h][w][t*C + c] = x[b][h + kh_t - pad][w + kw_t - pad][c] (zero outside the image / beyond taps*C), Ko channels per
 * output pixel, x with channel pitch Cx.  The kh x kw conv then runs as a 1x1 conv over the gathered map (one K-step
 * instead of kh*kw mostly-zero ones; the weight gradient reads gy once instead of once per tap). */
int msg_gather_taps(const void* x, void* y, int dtype, int B, int H, int W, int Cx, int C, int kh, int kw,
                    int pad, int Ko, void* stream);
/* ABI 5.  The adjoint of msg_gather_taps: g [B, H, W, Ko] (K index tap * C + c, as msg_gather_taps writes it) ->
 * gx [B, H, W, ldx], gx[q, c] = sum over taps of g[q - offset(tap), tap * C + c] (+ add[q, c] when add != NULL, pixel pitch
 * ld_add), fp32 accumulation, channels C .. ldx - 1 zeroed; C <= 8.  The data gradient of a few-channel 'same' convolution =
 * a 1x1 contraction to Ko channels followed by this fold (EqualizedConv2d of the first discriminator block,
 * multi_stylegan/u_net_2d_discriminator.py:161-170 with equalized_layer.py:57-74). */
int msg_fold_taps(const void* g, const void* add, void* gx, int dtype, int B, int H, int W, int Ko, int C, int kh, int kw,
                  int pad, int ldx, int ld_add, void* stream);

/* y = (a + beta*b) * gain over n elements (n multiple of the 16-byte vector, all pointers 16-B aligned): the
 * residual merges (main + residual)/sqrt(2) of multi_stylegan/u_net_2d_discriminator.py:185,381 in one pass. */
int msg_scaled_add(const void* a, const void* b, void* y, int dtype, long long n, float beta, float gain, void* stream);
/* y = (gamma[0] * a + b) * gain with gamma a DEVICE fp32 scalar -- the merge of the NonLocalBlock, (gamma * o + residual) / sqrt(2)
 * (multi_stylegan/u_net_2d_discriminator.py:381; gamma is a learnt parameter) -- and its backward in one pass:
 *   ga = gamma * gain * gy,  gb = gain * gy,  g_gamma[0] = gain * sum(gy * a)   (block partials in ws, added in a fixed order by a
 * second launch: deterministic).  Dense maps of n elements in one layout, MSG_F32 / MSG_BF16, n a multiple of the 16-byte vector. */
/* The generator's RGB skip path, one launch per level (multi_stylegan_generator.py:513-523: OutputBlock.forward):
 *   out[b,c,y,x] = float(conv[b,y,x,c]) + bias[c] + upfirdn2d(skip, fir, up = 2, pad = (2, 1))[b,c,y,x]
 * conv [B][H][W][ld] channels-last (MSG_F32 / MSG_BF16, pixel pitch ld >= C elements: the thin 1x1 conv's output), bias fp32
 * [C] or NULL, skip fp32 planes [B][C][H/2][W/2] or NULL (first level), fir DEVICE pointer to the 4 x 4 taps (required with
 * skip), out fp32 planes [B][C][H][W].  C <= 8, W % 4 == 0, H even; anything else MSG_EUNSUPPORTED.
 * msg_rgb_skip_merge_backward: g fp32 planes [B][C][H][W] -> g_conv [B][H][W][ld] (cast, padding channels zeroed; may be
 * NULL) and g_skip fp32 [B][C][H/2][W/2] (the transposed FIR as a gather: no atomics; may be NULL).  The op is linear: its
 * second-order pass is msg_rgb_skip_merge on the cotangents. */
int msg_rgb_skip_merge(const void* conv, int dtype, int ld, const float* bias, const float* skip, const float* fir,
                       float* out, int B, int C, int H, int W, void* stream);
int msg_rgb_skip_merge_backward(const float* g, void* g_conv, int dtype, int ld, float* g_skip, const float* fir,
                                int B, int C, int H, int W, void* stream);
int msg_gamma_merge(const void* a, const void* b, const float* gamma, void* y, int dtype, long long n, float gain, void* stream);
long long msg_gamma_merge_backward_workspace(void);
int msg_gamma_merge_backward(const void* gy, const void* a, const float* gamma, void* ga, void* gb, float* g_gamma, int dtype,
                             long long n, float gain, float* ws, void* stream);
/* The same for [rows][cols] operands with row pitches (elements): channel-slices of channels-last buffers, e.g. the
 * gradient of a skip connection (a slice of the concatenated map's gradient).  cols and pitches multiples of the vector. */
int msg_scaled_add_rows(const void* a, const void* b, void* y, int dtype, long long rows, int cols,
                        long long lda, long long ldb, long long ldy, float beta, float gain, void* stream);

/* Row softmax of the non-local block's attention map and its backward (u_net_2d_discriminator.py:378:
 * F.softmax(torch.bmm(theta^T, phi), -1)): x, y [rows][cols] contiguous in the storage type, fp32 arithmetic,
 *   y = softmax(x) along cols;   gx = y * (gy - sum_c gy[c] * y[c]).
 * One wave keeps a row in registers (read once, written once): cols a multiple of the 16-byte vector and at most 4096;
 * larger rows: MSG_EUNSUPPORTED. */
int msg_softmax_rows(const void* x, void* y, int dtype, long long rows, int cols, void* stream);
int msg_softmax_rows_backward(const void* y, const void* gy, void* gx, int dtype, long long rows, int cols,
                              void* stream);
/* ABI 5.  Second-order terms of the softmax backward for a cotangent v of gx (R1: the backward is differentiated again,
 * reference loss.py:311-316 through u_net_2d_discriminator.py:378), one pass over the maps:
 *   d_gy = y * (v - <v, y>),   d_y = v * (gy - <gy, y>) - gy * <v, y>     (row-wise inner products, fp32 arithmetic). */
int msg_softmax_rows_backward2(const void* y, const void* gy, const void* v, void* d_y, void* d_gy, int dtype,
                               long long rows, int cols, void* stream);

/* ---------------------------------------------------------------------------
 * a6 / 8f-1  fused attention of the NonLocalBlock -- replaces the torch.bmm -> F.softmax -> torch.bmm sequence of
 *     multi_stylegan/u_net_2d_discriminator.py:376-380 (beta = softmax(theta^T phi), o = g beta^T) without the
 *     [B, Nq, Nk] attention map ever reaching HBM.
 * q  [B, Nq, dk]  theta(x), one row per query pixel        k  [B, Nk, dk]  max-pooled phi(x), one row per key pixel
 * v  [B, Nk, dv]  max-pooled g(x)                           vt [B, dv, Nk]  its transpose (the caller provides both
 * orientations of the operands whose contraction index would otherwise be strided: qt [B,dk,Nq], kt [B,dk,Nk],
 * dOt [B,dv,Nq]); all dense, in the storage type.
 * forward:  o [B, Nq, dv] = softmax_rows(q k^T) v,  lse [B, Nq] fp32 = log sum_j exp(q_i . k_j)  (kept for backward)
 * backward: given dO [B, Nq, dv], o and lse of the forward:  dq, dk_out, dv_out  (probabilities are recomputed from q,
 *           k and lse; delta [B, Nq] fp32 is scratch the caller provides (it receives sum_d dO * o); no atomics:
 *           results are deterministic).
 * Supported: (dk, dv) = (48, 192) -- the reference's 384-channel blocks -- and (16, 64); Nq, Nk multiples of 128;
 * MSG_BF16 (bf16 MFMA, fp32 accumulate / softmax) and MSG_F32 (exact-fp32 MFMA).  Anything else:
 * MSG_EUNSUPPORTED (msg_nonlocal_attention_supported tells beforehand). */
int msg_nonlocal_attention_supported(int B, int Nq, int Nk, int dk, int dv);
int msg_nonlocal_attention_fwd(const void* q, const void* k, const void* vt, void* o, float* lse, int dtype,
                               int B, int Nq, int Nk, int dk, int dv, void* stream);
/* The 2x2 / stride-2 max-pooling in front of the attention (F.max_pool2d on phi(x) and g(x),
 * multi_stylegan/u_net_2d_discriminator.py:366-370), channels-last, MSG_BF16 / MSG_F32, H and W even, C a whole number of
 * 16-byte vectors.  x [B, H, W, C] with pixel pitch ldx >= C; y [B, H/2, W/2, C] dense; idx (NULL when no backward follows):
 * one 16-bit word per 16-byte vector of y, two bits per element = the window position that won (first maximum in scan
 * order, NaN wins: the library's rule).  Backward: gx [B, H, W, C] dense, every element written (gy at the winner, 0 elsewhere). */
int msg_maxpool2x2_fwd(const void* x, void* y, unsigned short* idx, int dtype, int B, int H, int W, int C, long long ldx,
                       void* stream);
int msg_maxpool2x2_bwd(const void* gy, const unsigned short* idx, void* gx, int dtype, int B, int H, int W, int C,
                       void* stream);
/* ABI 5.  The transpose of the backward's scatter, i.e. the derivative of msg_maxpool2x2_bwd with respect to gy for a cotangent
 * v of gx (second-order graphs, R1): v [B, H, W, C] channels-last with pixel pitch ldv, read at the positions idx names ->
 * out [B, H/2, W/2, C] dense. */
int msg_maxpool2x2_gather(const void* v, const unsigned short* idx, void* out, int dtype, int B, int H, int W, int C,
                          long long ldv, void* stream);

/* msg_nonlocal_attention_bwd_splits: in how many parts the dK / dV kernel splits its query sweep for this problem; when
 * it is more than 1 the caller passes `workspace` with splits * B * Nk * (dk + dv) floats (scratch, fully overwritten). */
int msg_nonlocal_attention_bwd_splits(int B, int Nq, int Nk);
/* (qt and dOt -- transposed copies of q and dO -- are no longer read and may be NULL: the dK / dV kernel takes Q^T and dO^T
 *  out of the row-major tiles with transposing LDS reads.  kt, the small [B, dk, Nk] copy of k, is still an operand.) */
int msg_nonlocal_attention_bwd(const void* q, const void* qt, const void* k, const void* kt, const void* v,
                               const void* dO, const void* dOt, const void* o, const float* lse, float* delta,
                               void* dq, void* dk_out, void* dv_out, float* workspace, int dtype,
                               int B, int Nq, int Nk, int dk, int dv, void* stream);

/* ---------------------------------------------------------------------------
 * 8f-2  batched affine warp of adaptive discriminator augmentation -- replaces the per-stage
 *     images[idx] = kaf.rotate(...) / kaf.apply_affine(images[idx], params, flags) of
 *     multi_stylegan/adaptive_discriminator_augmentation.py:120-199 (kornia 0.4.1) for a whole batch in one launch.
 * x, y      [B, C, H, W] fp32 (NCHW planes).
 * select_u  [B] uniform numbers; image b is transformed iff select_u[b] <= thr with thr = *p (rot_prob = 0) or
 *           1 - sqrt(1 - *p) (rot_prob = 1); p is a DEVICE scalar (the augmentation probability the controller
 *           adapts); other images are copied through.
 * angle_deg [B] degrees or NULL (then angle_const for every image); scale_xy [B, 2] or NULL (1, 1).
 * The warp is kornia's: M = [[cos, sin], [-sin, cos]] diag(scale) about (cx, cy) with the translation column
 * ((1 - m00) cx - m01 cy, m01 cx + (1 - m00) cy); output pixel -> normalised (affine_grid, align_corners) ->
 * N M^-1 N^-1 (N: pixel [0, size-1] -> [-1, 1]) -> pixel (grid_sample, align_corners), bilinear, padding 0 = zeros /
 * 2 = reflection.  (kaf.apply_affine passes -angle: the caller negates.)
 * backward != 0: x is the gradient of y, y receives the gradient of x (overwritten) -- the transpose of the bilinear
 * gather, a scatter, accumulated in 64-bit FIXED POINT (2^-38 resolution) in `workspace` (B*C*H*W + 1 8-byte words,
 * contents irrelevant) and converted by a second launch: integer addition is associative, so the result does not depend on
 * the order in which the atomics arrive (deterministic).  A contribution that is not finite or is >= 2^17 in magnitude
 * has no fixed-point image: it raises the last workspace word and the gradient of every transformed image comes out NaN
 * (a diverged gradient stays visible downstream instead of wrapping into finite values).  workspace may be NULL for
 * the forward.
 * Parity unpinned, see oracle/ada.py. */
int msg_affine_warp(const float* x, float* y, const float* angle_deg, float angle_const, const float* scale_xy,
                    const float* select_u, const float* p, int rot_prob, float cx, float cy, int padding,
                    int align_corners, int B, int C, int H, int W, int backward, void* workspace, void* stream);

/* ---------------------------------------------------------------------------
 * a5 / 8f-1  minibatch standard deviation -- replaces MinibatchStdDev.forward
 *     (multi_stylegan/u_net_2d_discriminator.py:205-217: std over the batch, mean over (c, h, w), one extra plane, cat).
 * x  channels-last [B, H, W] pixels of C channels, `ldx` elements apart;  y the same pixels with `ldy` > C channels:
 * y[..., :C] = x, y[..., C] = stat[g], further pad channels 0, where the batch is `groups` independent batches of
 * B / groups samples concatenated along dim 0 and stat[g] = mean_{c,h,w} sqrt(max(var_group(x), alpha)).
 * stat [groups] fp32 out; workspace: msg_minibatch_stddev_workspace(...) floats.  Deterministic (fixed-order sums).
 * backward: gx[..., :C] (pitch ldgx) = gy[..., :C] + gstat[g] * d stat / d x, gstat [groups] fp32 = the summed
 * gradient of each group's plane. */
long long msg_minibatch_stddev_workspace(int C, int H, int W, int groups, int dtype);
int msg_minibatch_stddev(const void* x, void* y, float* stat, float* workspace, int dtype,
                         int B, int C, int H, int W, int ldx, int ldy, int groups, float alpha, void* stream);
int msg_minibatch_stddev_backward(const void* x, const void* gy, const float* gstat, void* gx, int dtype,
                                  int B, int C, int H, int W, int ldx, int ldgy, int ldgx, int groups,
                                  float alpha, void* stream);

/* msg_conv2d_fprop with the activation stage of the layer fused into the epilogue:
 *   y = leaky_relu(conv(x, w) + noise_weight[0] * noise[b or 0, pixel] + act_bias[n], alpha) * scale
 * i.e. EqualizedConv2d -> FusedLeakyReLU (u_net_2d_discriminator.py:160-171) and ModulatedConv2d -> NoiseInjection ->
 * FusedLeakyReLU (multi_stylegan_generator.py:267-292) in one launch.  The activation is applied to the conv result
 * rounded to the storage type, so the output is bit-identical to msg_conv2d_fprop followed by msg_fused_bias_act.
 * act_bias [N] fp32 or NULL; noise [noise_batch][OH*OW] fp32 or NULL (noise_batch 1 or B); noise_weight: device scalar.
 * No in_up / pixel_shuffle forms (those layers are followed by a FIR pass before their activation). */
int msg_conv2d_fprop_act(const void* x, const void* w, void* y, int dtype,
                         int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int ldy,
                         int kh, int kw, int stride, int pad, long long w_batch_stride,
                         const float* act_bias, const float* noise, const float* noise_weight,
                         int noise_batch, float alpha, float scale, void* stream);
/* ... which also leaves the sign bytes of its output (see msg_upfirdn2d_separable_act_mask): mask, B * OH * OW * N / 8 bytes
 * in the order of the kernel's output tiles (256 pixels x 256 channels for MSG_PLAN_ROW3, 128 x 128 for MSG_PLAN_ROW3N: the
 * tile_m / tile_n of msg_bias_act_backward_mask), or NULL.  Only the row-sharing 3x3 kernels write them (msg_conv2d_fprop_launch_plan
 * with these arguments at epilogue 1 is MSG_PLAN_ROW3 or MSG_PLAN_ROW3N): any other problem with mask != NULL is MSG_EUNSUPPORTED
 * -- ask the plan first. */
int msg_conv2d_fprop_act_mask(const void* x, const void* w, void* y, int dtype,
                              int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int ldy,
                              int kh, int kw, int stride, int pad, long long w_batch_stride,
                              const float* act_bias, const float* noise, const float* noise_weight,
                              int noise_batch, float alpha, float scale, unsigned char* mask, void* stream);

/* msg_conv2d_fprop with the residual merge of a discriminator block fused into the epilogue:
 *   y = (conv(x, w) + residual) * gain        (u_net_2d_discriminator.py:185: (main + residual_mapping(x)) / sqrt(2))
 * residual: a map with the output's pixels and >= N channels, channel pitch res_ld elements, same storage type.
 * Bit-identical to msg_conv2d_fprop followed by msg_scaled_add. */
int msg_conv2d_fprop_residual(const void* x, const void* w, void* y, int dtype,
                              int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int ldy,
                              int kh, int kw, int stride, int pad, long long w_batch_stride,
                              const void* residual, int res_ld, float gain, void* stream);

/* (ABI 5) The DATA GRADIENT of a 3x3 'same' conv whose input was the output of a fused bias (+ noise) + leaky-ReLU stage, with
 * that stage's backward in the epilogue -- what the reference runs as conv2d_backward_input followed by
 * FusedLeakyReLUFunctionBackward (op_static/fused_act.py:24-42) on the map in between, which here is never written:
 *   y = (conv(x, w) [+ residual]) * (s > 0 ? scale : scale * alpha),  grad_bias[n] = sum_pixels y,  grad_noise_weight = sum y * noise
 * x: the gradient arriving at the conv's output, w: its data-gradient weight image (as for msg_conv2d_fprop).  s = the stage's
 * stored output, given by `sign_mask` (the bytes of msg_conv2d_fprop_act_mask / msg_upfirdn2d_separable_act_mask, tiles
 * mask_tile_m x mask_tile_n with mask_tile_m 1 or a multiple of 64, mask_tile_n a multiple of 128) or by `sign_map` (that output itself, bf16, channel pitch
 * sign_ld) -- exactly one of the two.  residual: a second gradient of the same map (added first), or NULL.  noise [noise_batch]
 * [OH*OW] fp32 with grad_noise_weight, or both NULL.  Sums: fp32, overwritten, deterministic (per-tile partials in `ws`, summed in
 * index order).  Ask msg_conv2d_fprop_launch_plan with these arguments at epilogue 3 first: ws_floats >= act_rows * N floats with
 * grad_bias, + act_entries with noise.  Only the row-sharing kernels have this epilogue, for a dense output (ldy == N):
 * MSG_EUNSUPPORTED where the plan gives act_rows = 0. */
int msg_conv2d_fprop_act_backward(const void* x, const void* w, void* y, int dtype,
                                  int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int ldy,
                                  int kh, int kw, int stride, int pad, long long w_batch_stride,
                                  const void* residual, int res_ld,
                                  const unsigned char* sign_mask, int mask_tile_m, int mask_tile_n,
                                  const void* sign_map, int sign_ld, float alpha, float scale,
                                  float* grad_bias, const float* noise, int noise_batch, float* grad_noise_weight,
                                  float* ws, long long ws_floats, void* stream);

/* (ABI 5) The discriminator's pixel-wise head -- FusedLeakyReLU(C) followed by a bias-free 1x1 equalized conv to one plane
 * (reference u_net_2d_discriminator.py:93-97, `final_mapping`; op_static/fused_act.py:64-89 + equalized_layer.py:63-74) -- as one
 * streaming pass per direction over the channels-last bf16 map x [npix][C]:
 *   y[p] = wscale * sum_c w[c] * a[p][c],  a = lrelu(x[p][c] + bias[c]) * scale            (fp32 out; the activated map is not stored)
 *   gx[p][c] = gy[p] * wscale * w[c] * slope(x[p][c] + bias[c]);  grad_bias_and_w[0..C) = sum_p gx,  [C..2C) = wscale * sum_p gy[p] a[p][c]
 * C / 8 a power of two <= 64, bf16 only (MSG_EUNSUPPORTED otherwise).  Sums fp32, overwritten, deterministic
 * (ws_floats >= msg_act_pointwise_head_backward_workspace(npix, C)). */
int msg_act_pointwise_head(const void* x, const float* bias, const float* w, float* y, int dtype,
                           long long npix, int C, float wscale, float alpha, float scale, void* stream);
long long msg_act_pointwise_head_backward_workspace(long long npix, int C);
int msg_act_pointwise_head_backward(const void* x, const float* bias, const float* w, const float* gy, void* gx,
                                    float* grad_bias_and_w, int dtype, long long npix, int C, float wscale,
                                    float alpha, float scale, float* ws, long long ws_floats, void* stream);

/* -------------------------------------------------------------------------
 * Equalized-lr fully connected layers with few rows (mapping network, style affines, classification head), fp32,
 * dense row-major operands.  Replaces F.linear(input, weight * scale, bias * scale_bias) of
 * multi_stylegan/equalized_layer.py (EqualizedLinear.forward) and its autograd derivatives; one launch per call.
 *   msg_linear_fprop   y[M][N]  = gain * x[M][K] . w[N][K]^T + bias_gain * bias[N]   (bias may be NULL)
 *   msg_linear_dgrad   gx[M][K] = gain * gy[M][N] . w[N][K]
 *   msg_linear_wgrad   gw[N][K] = gain * gy[M][N]^T . x[M][K];  gb[N] = bias_gain * sum_m gy[m][n]  (gb may be NULL)
 * ------------------------------------------------------------------------- */
int msg_linear_fprop(const float* x, const float* w, const float* bias, float* y, int M, int N, int K,
                     float gain, float bias_gain, void* stream);
int msg_linear_dgrad(const float* gy, const float* w, float* gx, int M, int N, int K, float gain, void* stream);
int msg_linear_wgrad(const float* gy, const float* x, float* gw, float* gb, int M, int N, int K,
                     float gain, float bias_gain, void* stream);

/* G layers of the same shape in ONE launch (the generator's style affines, multi_stylegan_generator.py:379-382: every
 * ModulatedConv2d's modulation_mapping applied to its slot of the latent [M][L][K], all known before the first conv):
 * group g reads rows x + slot[g]*K (row pitch L*K), its own weight w[g] ([N][K]) / bias[g] (device pointer tables;
 * `bias` itself may be NULL), and writes the g-th slab of the [G][M][N] (fprop), [G][M][K] (dgrad), [G][N][K] / [G][N]
 * (wgrad) outputs.  Same arithmetic per group as msg_linear_fprop / _dgrad / _wgrad.  M == 0: fprop and dgrad are no-ops; both
 * wgrad entries, like msg_linear_wgrad, still write their (zero) gradients, and gy and x may then be NULL.  G == 0: no-op. */
int msg_linear_grouped_fprop(const float* x, const int* slot, const float* const* w, const float* const* bias, float* y,
                             int G, int M, int N, int K, int L, float gain, float bias_gain, void* stream);
int msg_linear_grouped_dgrad(const float* gy, const float* const* w, float* gx, int G, int M, int N, int K, float gain,
                             void* stream);
int msg_linear_grouped_wgrad(const float* gy, const float* x, const int* slot, float* gw, float* gb, int G, int M, int N,
                             int K, int L, float gain, float bias_gain, void* stream);
/* msg_linear_grouped_wgrad with one destination per layer: gw / gb are DEVICE arrays of G device pointers ([N][K] / [N] each;
 * gb may be NULL) -- the layers' slices of a flat gradient store, so that no per-layer accumulation copy follows. */
int msg_linear_grouped_wgrad_ptrs(const float* gy, const float* x, const int* slot, float* const* gw, float* const* gb, int G,
                                  int M, int N, int K, int L, float gain, float bias_gain, void* stream);

/* What a forward convolution or data gradient launches for a problem (no launch): the geometry arguments of msg_conv2d_fprop --
 * those of the launch in question, its real ldy, stride and padding --, whether it has a bias, and its epilogue: 0 plain
 * (msg_conv2d_fprop), 1 the fused activation (msg_conv2d_fprop_act / _act_mask), 2 the residual merge (msg_conv2d_fprop_residual),
 * 3 the activation backward in a data gradient (msg_conv2d_fprop_act_backward); 1 .. 3 have no bias, in_up or pixel_shuffle.
 * `out` receives the first min(n_out_fields, MSG_FPLAN_FIELDS) of
 *   [0] kernel              a MSG_PLAN_* code
 *   [1] tile_m  [2] tile_n  the kernel's output tile, pixels x channels (0: the streaming kernels); with MSG_PLAN_ROW3 / ROW3N
 *                           the tile of the sign bytes msg_conv2d_fprop_act_mask leaves (no other kernel writes them)
 *   [3] act_rows  [4] act_entries   epilogue 3 on a row-sharing kernel: the partial-sum rows ([N] floats each) and noise entries
 *                           of msg_conv2d_fprop_act_backward; else 0 -- at epilogue 3 that launch is then MSG_EUNSUPPORTED
 * Returns MSG_OK, or the MSG_E* code the launch returns for the geometry before it looks at a pointer (`out` is then left alone).
 * B = 0: MSG_OK and all fields 0.  This is the selection the launches themselves go through: timing labels, the sign-byte gate,
 * workspace sizes and tests ask it, and nothing else. */
enum {
    MSG_PLAN_REG = 0,   /* 128x128 tile, register staging */
    MSG_PLAN_DMA = 1,   /* 128x128 tile, LDS-DMA staging */
    MSG_PLAN_PP = 2,    /* 256x256 ping-pong */
    MSG_PLAN_ROW3 = 3,  /* 3x3 row-sharing kernel, 256x256 tile */
    MSG_PLAN_ROW3N = 4, /* 3x3 row-sharing kernel, 128x128 tile */
    MSG_PLAN_THIN = 5,  /* the streaming kernels for 1x1 convolutions with <= 8 channels on one side (conv_thin.hip) */
    MSG_PLAN_UPCONV = 6, /* the activation-stationary sub-pixel up-convolution (conv_upconv.hip) */
    MSG_FPLAN_FIELDS = 5
};
int msg_conv2d_fprop_launch_plan(int dtype, int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int ldy,
                                 int kh, int kw, int stride, int pad, int in_up, int pixel_shuffle,
                                 long long w_batch_stride, int has_bias, int epilogue, long long* out, int n_out_fields);
/* What msg_conv2d_wgrad launches for a problem (no launch): the arguments of msg_conv2d_wgrad_workspace, and `out` receives the
 * first min(n_out_fields, MSG_WPLAN_FIELDS) of
 *   [0] kernel          a MSG_WPLAN_* code
 *   [1] nz              K-slices in the grid
 *   [2] chunks_per_out  K-slices that add up to one result (> 1: slabs in the workspace + the fixed-order sum)
 *   [3] n_out           results: B with per-sample weights, else 1
 *   [4] slice_pixels    logical pixels of one K-slice
 *   [5] OWv  [6] OHv    logical row width / row count of the K loop (OW x OH, or rows padded to a power of two)
 *   [7] fold            1: the batch is folded into K     [8] xcd_slices  1: one K-slice per XCD
 *   [9] blocks          workgroups of the contraction kernel
 *   [10] need           what msg_conv2d_wgrad_workspace returns
 * Returns MSG_OK, or the MSG_E* code msg_conv2d_wgrad returns for the geometry before it looks at a pointer (`out` is then left
 * alone).  B = 0: MSG_OK and all fields 0.  For tests and timing labels. */
enum {
    MSG_WPLAN_GENERIC = 0,  /* 128x128 tile of one tap, incremental addressing */
    MSG_WPLAN_DMA = 1,      /* ... LDS-DMA staging (tuning builds only: MSG_CONV_VARIANT=1) */
    MSG_WPLAN_UNI = 2,      /* ... uniform-row addressing (buffer loads; power-of-two or padded rows) */
    MSG_WPLAN_ROW3 = 3,     /* kh x 3 row-sharing kernel, maps a multiple of 64 wide */
    MSG_WPLAN_ROW3_W32 = 4, /* kh x 3 row-sharing kernel, maps exactly 32 wide */
    MSG_WPLAN_FIELDS = 11
};
int msg_conv2d_wgrad_plan(int dtype, int B, int IH, int IW, int Cx, int I, int OH, int OW, int ldgy,
                          int O, int ldgw, int kh, int kw, int stride, int pad, int pixel_shuffle,
                          int per_sample, int k_chunks, long long* out, int n_out_fields);
/* The four queries from before msg_conv2d_fprop_launch_plan, kept until the next ABI version: each is that query for the problem
 * it ASSUMES around the arguments it has, without the argument checks (so never an MSG_E* code).
 *   msg_conv2d_fprop_plan: stride 1, the 'same' padding kh / 2, no in_up, no pixel shuffle, ldy = N rounded up to 8, no bias,
 *     epilogue 0; returns the MSG_PLAN_* code (a pixel shuffle is needed for MSG_PLAN_UPCONV: never returned).
 *   msg_conv2d_fprop_act_backward_workspace: the same problem at epilogue 3; act_rows * N (+ act_entries with has_noise) floats.
 *   msg_conv2d_fprop_upconv_eligible: bf16, ldy = N / 4, no bias, epilogue 0; 1 for MSG_PLAN_UPCONV, else 0.
 *   msg_conv2d_fprop_thin_eligible: bf16, one weight set for the batch, no bias, epilogue act_mode (0 .. 2); for MSG_PLAN_THIN
 *     1 (N <= 8 output channels) or 2 (an 8-channel-padded input), else 0. */
int msg_conv2d_fprop_plan(int dtype, int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N,
                          int kh, int kw, long long w_batch_stride);
long long msg_conv2d_fprop_act_backward_workspace(int dtype, int B, int IH, int IW, int Cx, int Ck, int OH, int OW,
                                                  int N, int kh, int kw, long long w_batch_stride, int has_noise);
int msg_conv2d_fprop_upconv_eligible(int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int kh, int kw,
                                     int stride, int pad, int in_up, int pixel_shuffle, long long w_batch_stride);
int msg_conv2d_fprop_thin_eligible(int B, int IH, int IW, int Cx, int Ck, int OH, int OW, int N, int ldy, int kh, int kw,
                                   int stride, int pad, int in_up, int pixel_shuffle, int act_mode);

/* ---------------------------------------------------------------------------
 * Adam over a flat fp32 store, optionally with an exponential moving average of the stepped parameters in the same pass
 * (replaces: torch.optim.Adam.step() at multi_stylegan/model_wrapper.py:296-300, :410-414 and
 * misc.exponential_moving_average, multi_stylegan/misc.py -- ~400 small tensors per network each):
 *   g = grad * coef[0] (coef: device scalar or NULL = 1);  m += (1 - beta1)(g - m);  v = beta2 v + (1 - beta2) g^2;
 *   param -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps);  ema = d ema + (1 - d) param (ema != NULL)
 * All arrays n floats, 16-byte aligned; step >= 1 is the number of this update.  msg_flat_ema: the EMA alone.
 * ------------------------------------------------------------------------- */
int msg_flat_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, long long n,
                  const float* coef, float lr, float beta1, float beta2, float eps, int step, float ema_decay,
                  void* stream);
int msg_flat_ema(float* ema, const float* param, long long n, float decay, void* stream);

/* ---------------------------------------------------------------------------
 * The data feed's batch prepare: raw camera counts -> normalised, flipped float frames.  Replaces, for a whole batch in one
 * call, what the reference's dataset does per sample on the host in its DataLoader workers: dataset/tlfm_dataset.py:186-197
 * (bright-field normalisation, GFP / RFP range normalisation, vertical flip), dataset/utils.py:4-23 (normalize_0_1) and
 * the RandomHorizontalFlip of the default `transformations` (dataset/tlfm_dataset.py:24-25, applied at :163/:172/:181).
 * raw    [B, C, T, H, W] unsigned 16-bit counts, contiguous; C = 1 (bright field), 2 (+ GFP) or 3 (+ RFP)
 * hflip  [B] bytes, non-zero = mirror every frame of that sample left-right; NULL = no sample is mirrored
 * out    [B, C, T, H, W] MSG_F32 or MSG_BF16, every element written
 * vflip  non-zero = every frame upside down (the dataset's `flip`)
 * channel 0: (x - min) / (max - min) with min / max over the (b, t) frame; a CONSTANT frame gives 0 / 0 = NaN in all of its
 *            pixels, exactly as the reference's normalize_0_1 does;
 * channel 1: min(max(x - lo1, 0) / div1, 1); channel 2 likewise with (lo2, div2) -- the divisor is the reference's gfp_max /
 *            rfp_max itself, not a range.
 * Counts are unsigned (65535 is 65535.f), subtract and divide are IEEE fp32 (correctly rounded divide, no reciprocal), so the
 * MSG_F32 result equals the reference's CPU result bit for bit; MSG_BF16 is its round-to-nearest-even.  Flips are applied on
 * the store side, which equals the reference's "flip, then normalise".
 * ws     msg_tlfm_prepare_workspace(B, T) 32-bit words; needs no initialisation and carries nothing between calls (the
 *        entry writes every word it reads).  Two launches, no synchronisation.
 * MSG_EINVAL: a non-positive size, C > 3, any other dtype, NULL raw / out / ws.
 * ------------------------------------------------------------------------- */
long long msg_tlfm_prepare_workspace(int B, int T);
int msg_tlfm_prepare(const unsigned short* raw, const unsigned char* hflip, void* out, int dtype,
                     int B, int C, int T, int H, int W, int vflip,
                     float lo1, float div1, float lo2, float div2,
                     unsigned int* ws, void* stream);

/* ---------------------------------------------------------------------------
 * The resident dataset: every frame decoded once into one store of counts in device memory, a batch built by one launch that
 * gathers, normalises and flips the frames its samples name.  Replaces the per-epoch re-read of every file in the DataLoader
 * workers -- dataset/tlfm_dataset.py:128-198 (__getitem__: cv2.imread of every frame of every sample, the normalisation, the
 * flips), dataset/utils.py:4-23 (normalize_0_1) and the DataLoader of train_multi_stylegan.py:60-63 with its collate, pinned
 * staging and host-to-device copy.
 * frames [N, H, W] unsigned 16-bit counts, contiguous: the store
 * range  [N, 2] 32-bit words: the integer (min, max) of each frame.  msg_tlfm_frame_range writes it -- one launch, one
 *        workgroup per frame, integer min / max without atomics: deterministic, equal to numpy's.  Once per store.
 * index  [B, C, T] int32 frame ids in device memory: out[b, c, t] is made from frames[index[b, c, t]]
 * hflip, out, dtype, vflip, lo1 .. div2: as msg_tlfm_prepare
 * channel 0: lo = (float) min, div = (float) max - lo from range[id]; channels 1 / 2: (lo1, div1) / (lo2, div2).  The same
 *            arithmetic as msg_tlfm_prepare (IEEE subtract and divide, the clamps in the reference's order, flips on the store
 *            side): the MSG_F32 result equals msg_tlfm_prepare's on the stacked frames bit for bit, MSG_BF16 is its
 *            round-to-nearest-even; a constant bright-field frame is NaN in every pixel.
 * One launch, no workspace, no atomics, nothing carried between calls.  A frame is split over workgroups in row ranges of
 * ~4096 pixels; W % 8 == 0 and 16-byte aligned store and output bases: 16-byte loads, anything else the scalar path.  A
 * frame's offset in the store is 64-bit (N * H * W may exceed 2^31 elements).
 * An id outside [0, N) never reads the store: the check is uniform per workgroup and that frame of `out` is NaN throughout.
 * MSG_EINVAL (both): a non-positive size, C > 3, any other dtype, NULL frames / range / index / out, more frames (or frames
 * and splits) than the launch's block index can address.
 * ------------------------------------------------------------------------- */
int msg_tlfm_frame_range(const unsigned short* frames, long long N, int H, int W,
                         unsigned int* range, void* stream);
int msg_tlfm_gather(const unsigned short* frames, const unsigned int* range, long long N,
                    const int* index, const unsigned char* hflip, void* out, int dtype,
                    int B, int C, int T, int H, int W, int vflip,
                    float lo1, float div1, float lo2, float div2, void* stream);

/* ---------------------------------------------------------------------------
 * Simulated datasets: a generated batch -> the 16-bit camera counts the dataset would have read it from, so that the generator's
 * output can be written as TIFF files and read back as data.  dataset/tlfm_dataset.py:186-197 (with dataset/utils.py:4-23) read
 * backwards: the inverse of msg_tlfm_prepare, which the reference does not have.
 * x         [B, C, T, H, W] MSG_F32 or MSG_BF16 (widened to fp32 first), contiguous; C = 1 (bright field), 2 (+ GFP), 3 (+ RFP)
 * bf_range  [B, T, 2] int32 in device memory: the count range (lo, hi) of every bright-field frame, 0 <= lo < hi <= 65535 (the
 *           caller validates; other values are used as they are, the counts are clamped to [0, 65535] whatever they give)
 * out       [B, C, T, H, W] unsigned 16-bit counts, every element written; a frame is one contiguous strip of H * W counts
 * vflip     non-zero: output row r holds input row H - 1 - r (the dataset flips on load)
 * All arithmetic fp32, every operation rounded on its own (no fused multiply-add):
 *   count = (uint16) min(max(rint(fl(fl(n * scale) + offset)), 0), 65535), rint = ties to even, NaN -> 0
 * channel 0, bf_normalise != 0: n = (x - m) / (M - m), m / M the frame's minimum / maximum over its non-NaN values (+-inf take
 *            part as they are), IEEE subtract and correctly rounded divide; M == m: n = 0 (NaN where x is NaN);
 *            scale = (float)(hi - lo), offset = (float) lo.  The frame's minimum writes lo, its maximum hi, exactly.
 * channel 0, bf_normalise == 0: n = min(max(x, 0), 1), same scale and offset; no reduction, one launch.
 * channels 1 / 2: n = min(max(x, 0), 1), scale = div1 / div2, offset = low1 / low2 -- the dataset's (gfp_min, gfp_max) /
 *            (rfp_min, rfp_max): it divides by max, not by max - min, and so does this.
 * ws        msg_tlfm_export_workspace(B, T) 32-bit words, read only when bf_normalise != 0; needs no initialisation and carries
 *           nothing between calls (launch 1 writes every word launch 2 reads).  A frame is split over workgroups in row ranges
 *           of ~4096 pixels (at most 32, at most H); fminf / fmaxf reductions, no atomics: bit-identical from run to run.
 * W % 8 == 0 and 16-byte aligned x and out: 16-byte loads (4 fp32 / 8 bf16 pixels) and 16-byte stores (8 counts); anything else
 * one pixel per lane with the same arithmetic.
 * MSG_EINVAL: a non-positive size, C > 3, any other dtype, NULL x / bf_range / out, NULL ws with bf_normalise != 0, more frames
 * and splits than the launch's block index can address.
 * ------------------------------------------------------------------------- */
long long msg_tlfm_export_workspace(int B, int T);
int msg_tlfm_export(const void* x, int dtype, const int* bf_range, unsigned short* out,
                    int B, int C, int T, int H, int W, int vflip, int bf_normalise,
                    float low1, float div1, float low2, float div2,
                    float* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Sample output: a generated batch -> the 8-bit RGB pictures the reference writes through torchvision.utils.save_image, composed
 * in one pass.  Replaces the repeat_interleave / zero-fill / cat / permute chains, the fp32 device-to-host copy and the host
 * quantisation of multi_stylegan/misc.py:132-166 (Logger.save_prediction, called at model_wrapper.py:166-174),
 * scripts/get_gan_samples.py:44-60 and scripts/gan_latent_space_interpolation.py:46-59.
 * seq    [B, C, T, H, W] MSG_F32 or MSG_BF16 (widened to fp32 first), contiguous; C = 1 .. 3
 * out    [B, C, H, T*W, 3] bytes, interleaved RGB, every byte written.  As [B, C] sheets of H x (T*W): a sequence's frames side
 *        by side, save_image(nrow=T, padding=0).  As [B] pictures of (C*H) x (T*W): the channels stacked top to bottom, the
 *        interpolation frame.  The same memory.
 * tints  three bits per channel at bits 3c .. 3c+2: bit 0 = write the red byte, bit 1 green, bit 2 blue; a cleared bit writes
 *        0.  The reference's colours: bright field 7, GFP 2, RFP 1 -> 7 | 2 << 3 | 1 << 6.
 * q = (uint8) trunc(min(max(fl(fl(x * 255) + 0.5), 0), 255)) in fp32, multiply and add rounded separately (torchvision's
 * save_image with normalize=False); NaN -> 0, +inf -> 255, -inf -> 0.
 * W % 16 == 0 and 16-byte aligned bases: 16 pixels per lane, 16-byte loads and stores; anything else one pixel per lane with the
 * same arithmetic.  One launch, no workspace.
 * MSG_EINVAL: a non-positive size, C > 3, any other dtype, NULL seq / out, tint bits above bit 3C - 1, more pixels than the
 * launch's block index can address.
 * ------------------------------------------------------------------------- */
int msg_sample_sheet(const void* seq, unsigned char* out, int dtype,
                     int B, int C, int T, int H, int W, int tints, void* stream);

/* ---------------------------------------------------------------------------
 * The adversarial objectives of the step: two means over up to two prediction tensors in one streaming pass, and their
 * gradient in one more.  Replaces the softplus / minimum, broadcast-multiply and mean chains (and their backward kernels) of
 * multi_stylegan/loss.py:9-94 (Wasserstein discriminator, CutMix and generator losses), :97-196 (the non-saturating logistic
 * ones) and :198-280 (the hinge ones):
 *   out[0] = (1 / n_real) sum_i a_i  r(x_i)   over pred_real   (a generator loss is this side applied to fake predictions)
 *   out[1] = (1 / n_fake) sum_i a'_i f(x_i)   over pred_fake
 *   kind                   r(x)              f(x)               r'(x)                            f'(x)
 *   MSG_GAN_LOGISTIC       softplus(-x)      softplus(x)        -sigmoid(-x)                     sigmoid(x)
 *   MSG_GAN_WASSERSTEIN    -x                x                  -1                               1
 *   MSG_GAN_HINGE          -min(0, x - 1)    -min(0, -x - 1)    -1 (x < 1), -1/2 (x == 1), 0     1 (x > -1), 1/2 (x == -1), 0
 * (the half slope at the kink is torch.minimum's at a tie; a NaN prediction gives a NaN loss, as torch.minimum does; softplus
 * is torch's: z for z > 20, log1p(exp(z)) otherwise.)
 *   aux_mode
 *   MSG_GAN_AUX_NONE     a = a' = 1; aux = NULL
 *   MSG_GAN_AUX_WEIGHT   a_i = a'_i = aux[i mod P], aux [P] fp32: the reference's weight.view(1, 1, 1, H, W) broadcast over
 *                        predictions whose last two dimensions are H x W, P = H W (P need not divide n)
 *   MSG_GAN_AUX_LABEL    CutMix: a_i = aux[i], a'_i = 1 - aux[i], aux [n_real] fp32, and BOTH sides read pred_real
 *                        (n_fake == n_real; pred_fake NULL or pred_real itself)
 * pred_real / pred_fake  n_real / n_fake elements, MSG_F32 or MSG_BF16 (widened to fp32; sums and results are fp32), contiguous,
 *                        any alignment (16-byte aligned tensors are read 16 bytes per lane and load).  The counts may differ.
 *                        A side with n = 0 and a NULL pointer is absent and its out is 0; both absent is MSG_EINVAL.
 * out    [2] fp32, both written.
 * ws     msg_gan_loss_workspace(n_real, n_fake) fp32 words (0 for small inputs: ws may then be NULL); needs no initialisation
 *        and carries nothing between calls.  ws_floats: what the caller allocated.
 * Bit-identical from run to run: no atomics; the grid and the summation order follow from the element counts alone (not from
 * dtype or alignment): one launch writes per-workgroup partial sums, a second, one workgroup per side, adds them in a fixed
 * order; a single launch where one workgroup per side suffices.
 *
 * msg_gan_loss_backward: grad_real[i] = ((grad_out[0] / n_real) a_i) r'(x_i), grad_fake[i] = ((grad_out[1] / n_fake) a'_i)
 * f'(x_i), in the predictions' dtype (bf16: round to nearest even); MSG_GAN_AUX_LABEL: grad_real[i] is the sum of the two and
 * grad_fake must be NULL.  grad_out [2] fp32 is read on the device.  A NULL grad_real / grad_fake (not both) skips that side.
 * A zero slope or a zero label gives an exact zero.  One launch, no workspace.
 * MSG_EINVAL: any other dtype, kind or aux_mode, a negative count, a count without its pointer, aux against its mode, P <= 0
 * with a weight map, a workspace that is NULL or too small where one is needed.
 * ------------------------------------------------------------------------- */
enum { MSG_GAN_LOGISTIC = 0, MSG_GAN_WASSERSTEIN = 1, MSG_GAN_HINGE = 2 };
enum { MSG_GAN_AUX_NONE = 0, MSG_GAN_AUX_WEIGHT = 1, MSG_GAN_AUX_LABEL = 2 };
long long msg_gan_loss_workspace(long long n_real, long long n_fake);
int msg_gan_loss(const void* pred_real, const void* pred_fake, const float* aux, float* out, int dtype, int kind,
                 int aux_mode, long long n_real, long long n_fake, long long P, float* ws, long long ws_floats,
                 void* stream);
int msg_gan_loss_backward(const void* pred_real, const void* pred_fake, const float* aux, const float* grad_out,
                          void* grad_real, void* grad_fake, int dtype, int kind, int aux_mode,
                          long long n_real, long long n_fake, long long P, void* stream);

/* ---------------------------------------------------------------------------
 * Elastic deformation of a batch of frames: the dataset's augmentation for a whole batch in one call.  Replaces the dense
 * (4 sigma + 1)^2 conv2d of two noise planes and the grid_sample call per sample of dataset/tlfm_dataset.py:230-275
 * (elastic_deformation, which ElasticDeformation.forward at :221-227 calls).
 * in     [B, F, H, W] MSG_F32 or MSG_BF16 (read as stored, all arithmetic fp32), contiguous
 * noise  [B, 2, H, W] fp32 in [-1, 1): plane 0 the horizontal component (the reference's FIRST torch.rand draw), plane 1 the
 *        vertical one
 * field  [B, 2, H, W] fp32, every element written: the displacement in pixels,
 *          d[c, y, x] = alpha sum_i sum_j g[i] g[j] noise[c, y + i - 2 sigma, x + j - 2 sigma],
 *          g[i] = exp(-(i - 2 sigma)^2 / (2 sigma^2)) / (sqrt(2 pi) sigma), i = 0 .. 4 sigma
 *        -- the reference's kernel, which is exactly g (x) g: truncated at +-2 sigma and NOT renormalised (sum g ~ 0.954); noise
 *        outside the frame counts as zero.  Evaluated separably (row pass, column pass) with fp32 multiply-adds.  One field per
 *        sample, shared by its F frames.
 * out    [B, F, H, W] in the dtype of `in`, every element written, not aliasing `in`: the bilinear sample of each frame at
 *          px = ((gx + 1) W - 1) / 2,  gx = 2 (x + d[0, y, x] - H / 2) / H   (integer H / 2)
 *          py = ((gy + 1) H - 1) / 2,  gy = 2 (y + d[1, y, x] - W / 2) / W
 *        -- the x coordinate is divided by the HEIGHT and the y coordinate by the width, as the reference does (:269-270);
 *        grid_sample's align_corners=False un-normalisation; px clamped to [0, W - 1], py to [0, H - 1] (border padding);
 *        neighbours floor and floor + 1, the upper index clamped to the frame.  The four indices and weights of a position are
 *        computed once and applied to all F frames.  bf16: rounded to nearest even on the store.
 * ws     msg_elastic_workspace(B, H, W) BYTES (the row pass's output, one more [B, 2, H, W] fp32 array), 16-byte aligned; needs
 *        no initialisation and carries nothing between calls.  Two launches, no synchronisation.
 * Deterministic: no atomics, nothing depends on workgroup order, a sample's result does not depend on the rest of the batch.
 * W a multiple of 4 (fp32) / 8 (bf16) and 16-byte aligned in / out / field: 16-byte stores; anything else a scalar path with the
 * same arithmetic and the same bits.
 * MSG_EINVAL: a NULL pointer (ws included), a non-positive size, sigma < 1, H W or the row pass's block count above 2^31 - 1.
 * MSG_EUNSUPPORTED: any other dtype; sigma > MSG_ELASTIC_MAX_SIGMA (the halo the LDS tiles are sized for).  Nothing is launched
 * in any of these cases.
 * ------------------------------------------------------------------------- */
#define MSG_ELASTIC_MAX_SIGMA 32
long long msg_elastic_workspace(int B, int H, int W);
int msg_elastic_deform(const void* in, const float* noise, float* field, void* out, int dtype,
                       int B, int F, int H, int W, int sigma, float alpha, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Baseline JPEG (ITU T.81: sequential DCT, Huffman, 8 bit), 4:2:0, for a batch of pictures: from the interleaved RGB bytes
 * msg_sample_sheet writes to the entropy-coded scan of every frame, so that the compressed stream and not 3 B per pixel goes to
 * the host.  Replaces the PNG frame directory and the ffmpeg call of scripts/gan_latent_space_interpolation.py:57-59; the host
 * adds the headers and the container (multi_stylegan_amd/video.py).
 * rgb      [N, H, W, 3] bytes, any alignment; any H, W >= 1
 * qtables  [2][64] on the HOST (read during the call, passed to the kernels by value): luma then chroma, natural (row-major)
 *          order, every entry 1 .. 255
 * coef     NULL, or [N, MR, MC, 6, 64] 16-bit (2-byte aligned), every element written: per MCU the blocks Y00, Y01, Y10, Y11,
 *          Cb, Cr, each in zigzag order, quantised, DC not yet differenced
 * scan     as many bytes as msg_jpeg_scan_capacity(N, H, W, &bytes) says, any alignment; scan[offsets[n] .. offsets[n + 1]) is frame n's complete
 *          entropy-coded segment, what stands between the SOS header and EOI.  Frames are dense, one after the other.  Bytes at
 *          and past offsets[N] are not written.
 * offsets  [N + 1] (8-byte aligned), all written; offsets[0] = 0
 * ws       msg_jpeg_workspace(N, H, W) BYTES, 16-byte aligned: the coefficients, one slot of bytes per restart interval, the
 *          intervals' lengths and starts.  Needs no initialisation and carries nothing between calls.  The capacity and the
 *          slots are sized for the longest stream the tables can produce (208 B per block, every byte stuffed): 2496 B per MCU,
 *          3.25 x the RGB bytes, of which a sheet touches a few per cent.
 * Geometry: an MCU is 16 x 16 pixels, MR = ceil(H / 16), MC = ceil(W / 16); pixels outside the picture repeat its last row or
 * column.
 * Colour (JFIF, full range), in fp32 from the bytes: Y = 0.299 R + 0.587 G + 0.114 B, Cb = -0.168736 R - 0.331264 G + 0.5 B + 128,
 * Cr = 0.5 R - 0.418688 G - 0.081312 B + 128; 128 is subtracted from each of the three; a chroma sample is the mean of its 2 x 2
 * pixels, taken in float (no rounding to bytes in between).
 * Transform: the 8 x 8 DCT-II of T.81 A.3.3, F(v, u) = 1/4 C(u) C(v) sum_y sum_x f(y, x) cos((2x + 1) u pi / 16)
 * cos((2y + 1) v pi / 16), C(0) = 1 / sqrt 2, evaluated separably in fp32 (rows, then columns).
 * Quantisation: q = sign(c) floor(|c| / Q + 1/2); AC clamped to +-1023 and the DC difference to +-2047, the ranges the Annex K
 * tables code.
 * Scan: the four Huffman tables of T.81 Annex K.3 (K.3 / K.5 for Y, K.4 / K.6 for Cb and Cr); one restart interval is one MCU
 * row (Ri = MC) and DC prediction starts from 0 in each; every interval is padded to a byte with 1-bits and RSTm, FF D0+(r mod 8),
 * follows interval r of a frame except its last; every FF the coder produces is followed by 00.
 * Four launches (transform and quantise; code one interval per workgroup, the bits assembled in LDS; prefix sum of the N MR
 * interval lengths; pack), no synchronisation, nothing read back.  Bit-identical from run to run, and a frame's bytes do not
 * depend on the rest of the batch: the only atomics are ORs into LDS words.
 * msg_jpeg_scan_capacity writes the byte count to *bytes (host memory) and returns a status like every entry that is not a
 * workspace size; msg_jpeg_workspace returns -1, and the capacity query MSG_EINVAL, for sizes the entry refuses with MSG_EINVAL.
 * MSG_EINVAL: a NULL pointer other than coef, a misaligned ws / coef / offsets, a non-positive size, a table entry outside
 * 1 .. 255, N or MR above 65535, N MR above 2^31 - 1, byte counts that do not fit 63 bits.
 * MSG_EUNSUPPORTED: W > MSG_JPEG_MAX_WIDTH.  The interval coder walks an interval in chunks of 256 blocks, so its LDS buffer
 * bounds the chunk and not the width; the limit keeps an interval's slot (and the 32-bit byte counts within it) below 2^23.
 * Nothing is launched in any of these cases.
 * ------------------------------------------------------------------------- */
#define MSG_JPEG_MAX_WIDTH 16384
long long msg_jpeg_workspace(int N, int H, int W);
int msg_jpeg_scan_capacity(int N, int H, int W, long long* bytes);
int msg_jpeg_encode(const unsigned char* rgb, const unsigned short* qtables, short* coef, unsigned char* scan,
                    long long* offsets, int N, int H, int W, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Metric inputs: the tensor a pretrained feature network receives from the validation pass -- select one channel, resize with
 * anti-aliasing, map each sample to [-1, 1], replicate on the colour planes -- in one launch, or two with a normalisation.
 * Replaces the chain of stock calls of multi_stylegan/validation_metrics.py: :44-52 (IS: kornia.resize to 299 x 299, THEN
 * misc.normalize_m1_1_batch), :589-590 (FID: normalised frames resized to 299 x 299 inside InceptionNetworkFID.forward),
 * :941-943 (FVD: normalised clips resized to 224 x 224 inside InceptionI3d.forward), with the frame selection and
 * repeat_interleave(3) of :93-94, :246-247 and :451-452.
 * images   [B, C, T, H, W] MSG_F32 or MSG_BF16, contiguous, any alignment; widened to fp32, all arithmetic fp32
 * channel  in [0, C)
 * t        >= 0: that time step alone (T' = 1); -1: all of them (T' = T, the FVD clip)
 * out      [B, planes, T', out_h, out_w] MSG_F32 or MSG_BF16 (round to nearest even), whatever in_dtype is; planes 1 or 3, the
 *          planes identical copies; every element written
 * Resize: separable, with the weights of torch's interpolate(mode="bilinear", align_corners=False, antialias=True).  Per
 * axis, scale = n_in / n_out, support = max(scale, 1), c = scale (i + 0.5): output i reads the taps
 * j = max(int(c - support + 0.5), 0) .. min(int(c + support + 0.5), n_in) - 1 with w_j = max(0, 1 - |j - c + 0.5| / support),
 * divided by the sum over the taps used.  Up-scaling is plain bilinear with border clamp; equal sizes give an exact copy.  The
 * kernel forms the weights as integer numerators over one integer sum (w_j is (D - |n_out (2j + 1) - n_in (2i + 1)|) / D with
 * D = 2 max(n_in, n_out)) and rounds once, and uses exactly the taps whose weight is positive.  The row-pass result lives in
 * LDS; the source is read once per launch, plus the tiles' halo.
 * Normalisation (misc.normalize_m1_1_batch, per sample over all selected frames): 2 max((x - lo) / (hi - lo), 1e-3) - 1 with
 * IEEE subtract and divide, clamped from below only.
 *   MSG_METRIC_NORM_NONE     resize and replicate only; one launch, ws may be NULL
 *   MSG_METRIC_NORM_SOURCE   (FID, FVD) lo, hi from the sample's selected SOURCE frames; applied to every tap value before the
 *                            filter (the clamp is not linear: it cannot be moved behind the filter)
 *   MSG_METRIC_NORM_RESIZED  (IS) lo, hi from the sample's resized fp32 values; applied after the filter
 * A constant sample gives 0 / 0 = NaN in all of its outputs, as the reference does; a NaN anywhere in a sample's selected frames
 * makes that sample's whole output NaN (torch's min / max propagate NaN) and leaves the other samples alone.
 * ws       msg_metric_input_workspace(...) BYTES, 4-byte aligned: per-workgroup (min, max) pairs, written by the first of the two
 *          launches and read by every workgroup of the second; needs no initialisation, carries nothing between calls.
 * No atomics, no synchronisation; a sample's result does not depend on the rest of the batch; bit-identical from run to run.
 * 16-byte aligned images with W a multiple of 4 (fp32) / 8 (bf16) are read 16 bytes per lane, 16-byte aligned out with out_w
 * such a multiple is stored 16 bytes per lane; anything else goes element by element, with the same bits.
 * MSG_EINVAL: a NULL images or out, a NULL ws with a normalisation, a non-positive size, channel or t out of range, planes other
 * than 1 or 3, an unknown norm or dtype code, more workgroups than a block index addresses.
 * MSG_EUNSUPPORTED: n_in / n_out > MSG_METRIC_MAX_SCALE on either axis (the cap bounds the taps, 2 x the scale, and with them the
 * LDS tile).  Nothing is launched in any of these cases; msg_metric_input_workspace returns -1 for sizes the entry refuses.
 * ------------------------------------------------------------------------- */
enum { MSG_METRIC_NORM_NONE = 0, MSG_METRIC_NORM_SOURCE = 1, MSG_METRIC_NORM_RESIZED = 2 };
#define MSG_METRIC_MAX_SCALE 8
long long msg_metric_input_workspace(int B, int T, int H, int W, int t, int out_h, int out_w, int norm);
int msg_metric_input(const void* images, int in_dtype, int B, int C, int T, int H, int W,
                     int channel, int t, void* out, int out_dtype, int planes,
                     int out_h, int out_w, int norm, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Pairwise feature kernels: what the sample-based validation metrics (validation_metrics.py: KID / KVD, manifold precision /
 * recall / density / coverage) need of two sets of feature rows -- every pair (q_i, r_j), reduced where it is formed.  The
 * nq x nr matrix is never written; the reference has no such metric (its FID / FVD keep moments only).
 * Feature sets are fp32 [n, d], contiguous, 4-byte aligned (16-byte aligned sets with d % 4 == 0 are read 16 bytes per lane,
 * anything else element by element, with the same bits), d >= 1, all values finite (the caller's duty: max(0, .) and the
 * comparisons drop a NaN silently).  Row offsets are 64-bit.
 * Arithmetic: q . r is the exact-fp32 matrix instruction (one fmaf chain in ascending k per pair, the same bits for (a, b) and
 * (b, a)); |x|^2 likewise one fmaf chain per row; dist2(q, r) = max(0, (|q|^2 + |r|^2) - 2 q . r) in fp32.  Its error grows with
 * the norms, not with the distance: callers centre their sets first (validation_metrics.manifold_scores does).
 * One launch sweeps the pairs on a (query tile, sweep slice[, product]) grid and leaves per-slice results in ws; a second, small
 * launch merges the slices in slice order.  ws: the entry's _workspace(...) BYTES, needs no initialisation, carries nothing
 * between calls.  No atomics; every output is bit-identical from run to run.
 * MSG_EINVAL (all three): a NULL pointer where none is allowed, a non-positive size, a misaligned pointer (4 bytes; 8 for the
 * float64 sums and their ws).  Nothing is launched and no output byte is written on refusal; the _workspace queries return -1
 * for sizes the entry refuses.
 *
 * msg_feature_knn   out[i] (fp32 [nq]) = the k-th smallest dist2(q_i, r_j) over j, 1 <= k <= MSG_FEATURE_KNN_MAX.
 *   exclude_self != 0 (legal only with q == r and nq == nr, else MSG_EINVAL): j = i is skipped BY INDEX -- a duplicate of row i
 *   elsewhere in the set is a genuine neighbour at distance 0.  MSG_EINVAL if k exceeds the rows available (nr, less one with
 *   exclude_self).  Uses: manifold radii (q = r, exclude_self, k = 3 or 5); nearest cross-set distance (k = 1).
 * msg_feature_ball_hits   radius2 fp32 [nr], >= 0.  margin[i] (fp32 [nq]) = min_j (dist2(q_i, r_j) - radius2[j]);
 *   count[i] (int32 [nq]) = #{j : dist2(q_i, r_j) <= radius2[j]}.  Either output may be NULL (both: MSG_EINVAL).  margin <= 0
 *   is "inside the union of balls"; its size says how near a tie the decision was.  Uses: precision, recall, density.
 * msg_poly_mmd   the three kernel sums of the polynomial-kernel MMD^2 (KID), for S subsets in one call.
 *   x [nx, d], y [ny, d]; ix int32 [S, mx], iy int32 [S, my]: row indices into x / y, gathered while staging (no gathered copy is
 *   written).  Either may be NULL: the identity 0 .. n - 1, and then m must equal n (else MSG_EINVAL).  The indices live on
 *   the device and are not checked by the entry: an index in [0, n) is the caller's duty; one outside it reads as a row of zeros.
 *   k(u, v) = (gamma u . v + coef0)^3 in fp32, the cube as two multiplies; every value is widened to float64 before it is added.
 *   sums float64 [S, 3]: sum_{a != b} k(x_a, x_b), sum_{a != b} k(y_a, y_b), sum_{a, b} k(x_a, y_b), a and b positions in the
 *   subset's lists (a row listed twice is two positions).  The two symmetric sums visit the upper triangle of tiles and double
 *   it.  MSG_EINVAL also for 3 S > 65535 (what a block index addresses).
 * ------------------------------------------------------------------------- */
#define MSG_FEATURE_KNN_MAX 8
long long msg_feature_knn_workspace(int nq, int nr, int d, int k, int exclude_self);
int msg_feature_knn(const float* q, int nq, const float* r, int nr, int d, int k, int exclude_self, float* out,
                    void* ws, void* stream);
long long msg_feature_ball_hits_workspace(int nq, int nr, int d);
int msg_feature_ball_hits(const float* q, int nq, const float* r, int nr, int d, const float* radius2, float* margin,
                          int* count, void* ws, void* stream);
long long msg_poly_mmd_workspace(int nx, int ny, int d, int S, int mx, int my);
int msg_poly_mmd(const float* x, int nx, const float* y, int ny, int d, const int* ix, const int* iy, int S, int mx, int my,
                 float gamma, float coef0, double* sums, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Sliced Wasserstein kernels: what validation_metrics.py's SWD / SWVD (Karras et al. 2018, section 5: the sliced Wasserstein
 * distance over 7 x 7 patches of a Laplacian pyramid) run on the device -- one pyramid level, the patch gather, the per-plane
 * statistics, the projection with the normalisation folded in, the L1 distance of two sorted projections.  The sort between
 * the last two is the caller's (torch.sort).  The [n, P 49] normalised copy and an [n, R] product are never written; the
 * reference has no such metric.
 * All tensors fp32, contiguous, 4-byte aligned (8 for the float64 sums and their ws); row offsets are 64-bit.  Where the
 * shape allows, 16-byte aligned tensors are read / stored 16 bytes per lane, with the same bits as element by element (stated
 * per entry).  No atomics; every output is bit-identical from run to run.  ws: the entry's _workspace(...) BYTES, needs no
 * initialisation, carries nothing between calls.
 * MSG_EINVAL (all five): a NULL pointer where none is allowed, a non-positive size, a misaligned pointer.  Nothing is launched
 * and no output byte is written on refusal; the _workspace queries return -1 for sizes the entry refuses.
 *
 * msg_laplacian_level   fine [M, h, w] -> coarse [M, h/2, w/2] = down(fine) and lap [M, h, w] = fine - up(coarse); lap may be
 *   NULL (the Gaussian pyramid only).  h and w even and >= 8, else MSG_EINVAL (also for more than 2^31 - 1 tiles of 32 x 64).
 *   f = [1 4 6 4 1] / 16; boundary rule "mirror" on every axis: index -1 reads 1, -2 reads 2, n reads n - 2 (the edge sample is
 *   not repeated; scipy.ndimage's mode="mirror").  Order of operations -- SEPARABLE, rows first, then columns:
 *     down, per axis, on the five samples a b c d e around an even index:  fmaf(3/8, c, fmaf(1/4, b + d, (a + e) / 16))
 *       -- the pairs are folded first, the scalings by 1/16 and 1/4 are exact: 3 roundings per axis, 6 for a coarse value;
 *     up, per axis, on the zero-stuffed coarse samples with 2 f (4 F in two dimensions): an even index sees l c r of the coarse
 *       axis as fmaf(3/4, c, (l + r) / 8) (2 roundings), an odd index between c and r sees (c + r) / 2 (1 rounding); with the
 *       mirror rule on the stuffed axis coarse index -1 reads 1 and coarse index n/2 reads n/2 - 1;
 *     lap = fine - up, one IEEE subtract: at most 6 + 2 + 2 + 1 = 11 roundings on the way to a lap value.
 *   up() is taken of the ROUNDED coarse values, those the entry stores.  The source is read once per launch plus the tiles'
 *   halo (4 rows above, 3 below, 4 columns left, 3 right); the halo's coarse values are recomputed per tile, with the same bits.
 *   16-byte path: w % 4 == 0 and fine, lap 16-byte aligned (loads of fine, stores of lap; coarse is stored by element).
 * msg_swd_gather   level [B, P, h, w]; pos int32 [B, K, 2] = (y, x) patch centres on the device; rows [B K, P 49]: row b K + k,
 *   column 49 p + 7 dy + dx = level[b, p, y - 3 + dy, x - 3 + dx].  A plain copy: the bits of the source.  Positions are not
 *   checked by the entry: a tap outside the plane reads as zero.  rows 16-byte aligned: stored 16 bytes per lane.
 *   MSG_EINVAL also for B K > 2^31 - 1.
 * msg_swd_plane_sums   rows [n, P 49] -> sums float64 [P, 2] = (sum x, sum x^2) over the n 49 values of each plane; every value
 *   is widened to float64 before it is squared or added.  Fixed order: a workgroup sums 256 rows (a fixed lane assignment and a
 *   fixed tree) into ws, a second launch merges the workgroups' partials in index order.  Read element by element (a plane's
 *   runs of 49 floats have no common alignment).
 * msg_swd_project   out [R, n] (direction-major: the sort runs along the contiguous axis),
 *   out[r, i] = sum_j x^_ij dirs[j, r],  x^_ij = (rows[i, j] - mean[j / 49]) * istd[j / 49],  dirs [P 49, R], mean / istd [P].
 *   x^ is formed in fp32 with an IEEE subtract and an IEEE multiply while the rows are staged; the sum is one fmaf chain in
 *   ascending j from 0, on the exact-fp32 matrix instruction (v_mfma_f32_32x32x2_f32): P 49 roundings, P 49 + 2 with those of
 *   x^.  Row tile 128, direction tile 128; one launch.  16-byte loads of rows when P 49 % 4 == 0 and rows is 16-byte aligned.
 *   MSG_EINVAL also for more than 65535 direction tiles (what a block index addresses).
 * msg_sorted_l1   a, b [R, n] -> sums float64 [R], sums[r] = sum_i |a[r, i] - b[r, i]|: difference and absolute value in fp32,
 *   every term widened to float64 before it is added.  Fixed order: 4096 elements per workgroup into ws, merged in index order
 *   by a second launch.  16-byte loads when n % 4 == 0 and a, b are 16-byte aligned.  MSG_EINVAL also for R > 65535.
 * ------------------------------------------------------------------------- */
int msg_laplacian_level(const float* fine, int M, int h, int w, float* coarse, float* lap, void* stream);
int msg_swd_gather(const float* level, int B, int P, int h, int w, const int* pos, int K, float* rows, void* stream);
long long msg_swd_plane_sums_workspace(int n, int P);
int msg_swd_plane_sums(const float* rows, int n, int P, double* sums, void* ws, void* stream);
int msg_swd_project(const float* rows, int n, int P, const float* mean, const float* istd, const float* dirs, int R,
                    float* out, void* stream);
long long msg_sorted_l1_workspace(int R, int n);
int msg_sorted_l1(const float* a, const float* b, int R, int n, double* sums, void* ws, void* stream);

/* ---------------------------------------------------------------------------
 * Structural similarity, one scale: what ssim.py's ms_ssim (Wang et al. 2003; the diversity metric MSSSIM / MSSSIMVideo of
 * validation_metrics.py, the image loss of project.py) runs on the device -- per plane pair the sums of the contrast-structure
 * map cs and of the SSIM map cs l over the valid window positions, optionally the sum of |x - y| over all pixels and both
 * planes halved by the 2 x 2 mean for the next scale, in one launch (plus the merge of the tiles' partial sums); and the
 * gradient of those three MEANS with respect to x in one more.  The five moment maps are never written to memory; x and y are
 * read once per launch plus the tiles' halo.  The combination of the scales (a few values per plane) is the caller's.  The
 * reference has no such function.
 * Window: 11 taps g_k = exp(-(k - 5)^2 / (2 1.5^2)) / sum, computed in float64 and rounded once to fp32; separable, "valid": a
 * plane h x w has (h - 10)(w - 10) positions, position (i, j) covers pixels (i .. i + 10, j .. j + 10).
 * All tensors fp32, contiguous, 4-byte aligned (8 for the float64 sums and ws); plane offsets are 64-bit.  16-byte path (both
 * entries): w % 4 == 0 and x, y (and grad_x) 16-byte aligned -> the patches are loaded and grad_x is stored 16 bytes per lane;
 * only the memory instructions differ, the bits are those of the element-by-element path.  No atomics; every output is
 * bit-identical from run to run.  ws: msg_ssim_scale_workspace(M, h, w) BYTES (24 per tile), needs no initialisation, carries
 * nothing between calls; -1 for a size the entry refuses.
 * MSG_EINVAL (both): a NULL pointer where none is allowed, h or w < 11, M <= 0, a misaligned pointer, only one of x_half /
 * y_half, more than 2^31 - 1 tiles (16 x 64 forward, 16 x 32 backward).  Nothing is launched and no output byte is written.
 *
 * msg_ssim_scale   x, y [M, h, w]; c1 = (0.01 R)^2, c2 = (0.03 R)^2 for a data range R; sums float64 [M, 2] = (sum cs, sum cs l)
 *   over the positions; l1 float64 [M] = sum |x - y| over the h w pixels, or NULL; x_half, y_half [M, h / 2, w / 2] (floor; an
 *   odd trailing row or column is dropped), both or neither.  Order of operations, all fp32, every operation rounded once:
 *     xx = x x, yy = y y, xy = x y are ROUNDED to fp32 per pixel before any filtering;
 *     SEPARABLE, rows first, then columns.  Each pass of each of the five maps (x, y, xx, yy, xy) is one chain in ascending tap
 *       k: g_0 v_0 (a multiply), then fmaf(g_k, v_k, acc) for k = 1 .. 10 -- 11 roundings per pass, 22 + 1 for a second moment;
 *     mu_x mu_x, mu_y mu_y, mu_x mu_y rounded; s_xx = E_xx - mu_x mu_x, s_yy, s_xy likewise (one subtract each);
 *     D2 = (s_xx + s_yy) + c2, D1 = (mu_x mu_x + mu_y mu_y) + c1; cs = fmaf(2, s_xy, c2) / D2, l = fmaf(2, mu_x mu_y, c1) / D1
 *       (IEEE divisions); the SSIM term is the rounded product cs l;
 *     |x - y|: one subtract;  half = 0.25 ((v00 + v01) + (v10 + v11)): three roundings.
 *   Every cs, cs l and |x - y| term is widened to float64 before it is added.  Fixed order: a lane adds its four positions (its
 *   four pixels) in row order, a wave folds its lanes by shuffles (a fixed tree), the four wave sums are added in wave order into
 *   ws, and a second launch adds a plane's tiles in index order (row-major).
 * msg_ssim_scale_backward   g [M, 3] fp32: the gradients with respect to the plane's MEAN cs, MEAN cs l and MEAN |x - y|; the
 *   entry divides them by the counts (h - 10)(w - 10), (h - 10)(w - 10) and h w, each converted to fp32 (IEEE divisions): gcs,
 *   gss, gl1.  g_half [M, h / 2, w / 2] or NULL: the gradient with respect to x_half.  grad_x [M, h, w]: every element written.
 *   One launch; the moments are recomputed per 16 x 32 tile of grad_x from its 10-pixel halo with the forward's operations.  Per
 *   position:  a = fmaf(gss, l, gcs), b = gss cs, t2 = a / D2, t1 = b / D1,
 *     A = fmaf(t2, 2 (mu_x cs - mu_y), t1 (2 (mu_y - mu_x l))),  B = -(t2 cs),  C = 2 t2   (zero where there is no position);
 *   per pixel p the transposed window GA = sum_k sum_k' g_k g_k' A[p - (k, k')] (likewise GB, GC): rows first (tap k takes the
 *   position k columns to the left), then columns, each an ascending-tap chain as above;
 *     grad = fmaf(y, GC, fmaf(2 x, GB, GA));  grad = fmaf(gl1, sign(x - y), grad) with sign(0) = 0;
 *     with g_half, for pixels inside the 2 (h / 2) x 2 (w / 2) block:  grad = fmaf(0.25, g_half[p / 2], grad).
 *   SSIM is symmetric: the gradient with respect to y is the same call with x and y exchanged.
 * ------------------------------------------------------------------------- */
long long msg_ssim_scale_workspace(int M, int h, int w);
int msg_ssim_scale(const float* x, const float* y, int M, int h, int w, float c1, float c2, double* sums, double* l1,
                   float* x_half, float* y_half, void* ws, void* stream);
int msg_ssim_scale_backward(const float* x, const float* y, const float* g, const float* g_half, int M, int h, int w,
                            float c1, float c2, float* grad_x, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MSG_HIP_H */
