"""Convolution test shapes that say which forward-family kernel they are for (conv_fprop_select: thin, upconv, row3, pp, generic),
and the launches they turn into.  tests/test_host.py asserts with msg_conv2d_fprop_launch_plan, on any machine, that every case
selects the kernel it names and that the table as a whole reaches every large-tile kernel, weight mode and tile tail;
tests/test_hip_conv.py runs the cases against float64 and asserts the kernel-clock label of what ran.

The shapes sit at or just above each kernel's own floor -- 224 workgroups for the 256 x 256 tiles, 448 for the 128 x 128 row-sharing
tile, 1024 GEMM rows -- so that the float64 reference stays quick.  They are not the workload's shapes.

THIN_CASES, UPCONV_CASES and STREAM_GUARD_CASES further down do the same for the two streaming files that come first in the
selection order, conv_thin.hip and conv_upconv.hip."""
from collections import namedtuple

Case = namedtuple("Case", "name kind B I O H W k stride pad per_sample fwd dgrad")

# kind 'conv': y = conv2d(x, w, stride, pad);  kind 'up2': y = conv_transpose2d(x, w^T, kernel 2, stride 2)
# fwd / dgrad: the MSG_PLAN_* kernel of the forward launch and of the data-gradient launch, bf16, epilogue 0
CASES = [
    # ---- the 256 x 256 ping-pong kernel (conv_fprop_pp.hip)
    Case("pp_1x1_floor_ragged_m", "conv", 1, 256, 256, 239, 240, 1, 1, 0, False, "PP", "PP"),   # 4 K-steps (floor), 225 tiles, last tile 16 pixels
    Case("pp_1x1_n_tail", "conv", 1, 256, 480, 120, 240, 1, 1, 0, False, "PP", "DMA"),           # 480 of 512 columns
    Case("pp_1x1_per_sample", "conv", 45, 256, 256, 33, 33, 1, 1, 0, True, "PP", "PP"),          # ragged M per sample (1089), grid.z = 45
    Case("pp_3x3_ragged_k", "conv", 9, 72, 256, 80, 80, 3, 1, 1, False, "PP", "DMA"),            # Cx 72 under Ck 128, halo at every edge, samples folded into M
    Case("pp_3x3_per_sample", "conv", 45, 64, 256, 33, 33, 3, 1, 1, True, "PP", "DMA"),          # odd map, per-sample halo
    Case("pp_3x3_pad0", "conv", 4, 64, 256, 122, 122, 3, 1, 0, False, "PP", "DMA"),              # no padding, OW != IW
    Case("pp_3x3_s2", "conv", 4, 64, 256, 241, 241, 3, 2, 0, False, "PP", "PP"),                 # strided gather; parity data gradient, cropped odd map
    Case("pp_s2_dgrad_only", "conv", 4, 64, 128, 241, 241, 3, 2, 0, False, "DMA", "PP"),         # the discriminator's down-conv data gradient
    Case("pp_up2_shared", "up2", 4, 256, 64, 120, 120, 2, 2, 0, False, "PP", "PP"),              # pixel-shuffle store, N = 4 * O = 256
    Case("pp_up2_per_sample", "up2", 45, 256, 64, 33, 33, 2, 2, 0, True, "PP", "PP"),
    # ---- the row-sharing 3x3 kernel, 256 x 256 tile (conv_fprop_row3.hip)
    Case("row3_256w_floor", "conv", 1, 192, 256, 224, 256, 3, 1, 1, False, "ROW3", "DMA"),       # one image row per tile, 3 channel chunks, top / bottom rows
    Case("row3_128w", "conv", 2, 192, 256, 224, 128, 3, 1, 1, False, "ROW3", "DMA"),             # two rows per tile, sample boundary inside the launch
    Case("row3_64w_per_sample", "conv", 14, 192, 256, 64, 64, 3, 1, 1, True, "ROW3", "DMA"),     # four rows per tile, per-sample
    Case("row3_64w_square", "conv", 14, 256, 256, 64, 64, 3, 1, 1, False, "ROW3", "ROW3"),       # row-sharing data gradient, 256 tile
    Case("row3_512w", "conv", 1, 192, 256, 112, 512, 3, 1, 1, False, "ROW3", "DMA"),             # tiles start mid-row: live left / right neighbours
    # ---- ... 128 x 128 tile
    Case("row3n_128w_floor", "conv", 1, 64, 128, 448, 128, 3, 1, 1, False, "ROW3N", "DMA"),      # one K chunk, 448 tiles (floor)
    Case("row3n_64w_square", "conv", 14, 128, 128, 64, 64, 3, 1, 1, False, "ROW3N", "ROW3N"),    # row-sharing data gradient, 128 tile
    Case("row3n_64w_per_sample", "conv", 7, 64, 256, 64, 64, 3, 1, 1, True, "ROW3N", "DMA"),     # short-K rule, per-sample
    Case("row3n_256w", "conv", 1, 64, 128, 224, 256, 3, 1, 1, False, "ROW3N", "DMA"),            # half an image row per tile
    Case("row3n_32w", "conv", 28, 64, 256, 32, 32, 3, 1, 1, False, "ROW3N", "DMA"),              # the W32 form: four image rows per 128-pixel tile
    Case("row3n_32w_square", "conv", 56, 128, 128, 32, 32, 3, 1, 1, False, "ROW3N", "ROW3N"),    # W32 data gradient, many samples
    Case("row3n_32w_per_sample", "conv", 28, 64, 256, 32, 32, 3, 1, 1, True, "ROW3N", "DMA"),
    Case("row3n_384", "conv", 5, 64, 384, 64, 64, 3, 1, 1, False, "ROW3N", "DMA"),               # three N tiles
]

# one tile below a floor (223 / 446 workgroups): the 128 x 128 kernels take them.  Asserted on the host only, so that a moved
# floor is seen
GUARD_CASES = [
    Case("below_pp_floor", "conv", 1, 256, 256, 223, 256, 1, 1, 0, False, "REG", None),
    Case("below_row3_floor", "conv", 1, 192, 256, 223, 256, 3, 1, 1, False, "DMA", None),
]

EPILOGUE_CASES = ("pp_1x1_floor_ragged_m", "row3_256w_floor", "row3n_128w_floor")    # the floor shapes the epilogue legs run at

BY_NAME = {c.name: c for c in CASES}

# fields of a msg_conv2d_fprop_launch_plan argument tuple
(DTYPE, B_, IH, IW, CX, CK, OH, OW, N_, LDY, KH, KW, STRIDE, PAD, IN_UP, PIXEL_SHUFFLE, W_BATCH_STRIDE, HAS_BIAS, EPILOGUE) = range(19)


def _up(n, m):
    return (n + m - 1) // m * m


def out_hw(c):
    if c.kind == "up2":
        return 2 * c.H, 2 * c.W
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def parity_taps(k, pad):
    """The stride-2 data gradient as a stride-1 gather over gy, one sub-filter per output parity:
    gx[2c + ph] = sum_u gy[c + e - u] * w[t0 + 2u] with t0 = (ph + pad) % 2, e = (ph + pad - t0) / 2.  -> (taps, padding) of the
    gather that holds both parities' offsets e - u."""
    offsets = [(ph + pad - (ph + pad) % 2) // 2 - u for ph in (0, 1) for u in range((k - (ph + pad) % 2 + 1) // 2)]
    return max(offsets) - min(offsets) + 1, -min(offsets)


def launches(c, bf16, has_bias=0, epilogue=0):
    """-> (forward tuple, data-gradient tuple) of msg_conv2d_fprop_launch_plan arguments for a case, bf16 storage (bf16: the
    library's MSG_BF16 code), as the Python layer issues the two launches for a channels-last map with whole 16-byte channel
    vectors: Ck = the K extent rounded up to a 128-byte run, ldy = N rounded up to 8, the per-sample weight stride one dense image.
    has_bias / epilogue apply to the forward launch; the data gradient is plain."""
    assert c.I % 8 == 0 and c.O % 8 == 0
    oh, ow = out_hw(c)
    ck, ok = _up(c.I, 64), _up(c.O, 64)
    ps = int(c.per_sample)
    if c.kind == "up2":
        # forward: a 1x1 conv to the 4 * O sub-pixel planes, stored pixel-shuffled; data gradient: a 2x2 stride-2 conv of gy
        fwd = (bf16, c.B, c.H, c.W, c.I, ck, c.H, c.W, 4 * c.O, _up(c.O, 8), 1, 1, 1, 0, 1, 1, ps * 4 * c.O * ck, has_bias, epilogue)
        dgrad = (bf16, c.B, oh, ow, c.O, ok, c.H, c.W, c.I, _up(c.I, 8), 2, 2, 2, 0, 1, 0, ps * c.I * 4 * ok, 0, 0)
        return fwd, dgrad
    fwd = (bf16, c.B, c.H, c.W, c.I, ck, oh, ow, c.O, _up(c.O, 8), c.k, c.k, c.stride, c.pad, 1, 0, ps * c.O * c.k * c.k * ck,
           has_bias, epilogue)
    if c.stride == 2:
        # the parity form: taps x taps stride-1 conv of gy to the 4 * I parity planes of the half-size map, pixel-shuffled
        taps, pad2 = parity_taps(c.k, c.pad)
        hc, wc = (c.H + 1) // 2, (c.W + 1) // 2
        dgrad = (bf16, c.B, oh, ow, c.O, ok, hc, wc, 4 * c.I, _up(c.I, 8), taps, taps, 1, pad2, 1, 1, ps * 4 * c.I * taps * taps * ok, 0, 0)
    else:
        assert c.stride == 1
        # I and O swapped, flipped taps, padding k - 1 - pad
        dgrad = (bf16, c.B, oh, ow, c.O, ok, c.H, c.W, c.I, _up(c.I, 8), c.k, c.k, 1, c.k - 1 - c.pad, 1, 0, ps * c.I * c.k * c.k * ok, 0, 0)
    return fwd, dgrad


def gemm_rows(args):
    """GEMM rows of one grid.z slice of a launch: the pixels of one sample with per-sample weights, of the batch otherwise."""
    return args[OH] * args[OW] * (1 if args[W_BATCH_STRIDE] else args[B_])


# ---------------------------------------------------------------------------------------------------------------------------
# The two streaming files that come first in conv_fprop_select: conv_thin.hip (thin N: <= 8 outputs, thin K: <= 8 inputs, and
# thin K with scalar loads) and conv_upconv.hip.  tests/test_host.py asserts that every row selects THIN / UPCONV and that the
# tables reach every instantiation and loop edge named below; tests/test_hip_conv.py runs them exactly (small-integer operands)
# and against float64.
#
# cx: the channel count of the map x is a channel slice of (None: x is its own map, I rounded up to 8)
Thin = namedtuple("Thin", "name B I O H W per_sample cx", defaults=(None,))

THIN_CASES = [
    # ---- thin N (conv_thin_n_kernel<KC>, KC = Ck / 32; a wave takes groups_per_wave groups of 16 pixels)
    Thin("n_kc2_floor", 1, 64, 3, 64, 64, False),                # M = 4096, the floor; KC 2
    Thin("n_one_pixel_group", 1, 64, 5, 17, 241, False),         # M = 4097: the last group holds one pixel; N = 5
    Thin("n_n1_ragged", 1, 128, 1, 67, 62, False),               # N = 1, M % 16 = 10; KC 4
    Thin("n_n4_ragged", 1, 128, 4, 67, 62, False),               # N = 4: the second half-wave still carries no real output
    Thin("n_kc6_per_sample", 2, 192, 4, 50, 47, True),           # KC 6, per-sample, M % 16 = 14
    Thin("n_n8", 1, 256, 8, 65, 64, False),                      # N = 8, every weight row live; KC 8
    Thin("n_kc12", 1, 384, 6, 67, 62, False),                    # KC 12
    Thin("n_kc16_per_sample", 2, 512, 6, 47, 45, True),          # KC 16, the RGB heads, per-sample, M % 16 = 3
    Thin("n_two_groups", 1, 64, 3, 363, 362, False),             # M = 131406: groups_per_wave 2; 8213 groups: the last wave takes one of its two and breaks
    Thin("n_two_groups_per_sample", 3, 64, 5, 210, 209, True),   # groups_per_wave 2 through the sample count (2744 groups x 3)
    Thin("n_eight_groups", 1, 64, 3, 1025, 1024, False),         # groups_per_wave clamped at 8 (65600 groups); 134 MB of input
    Thin("n_channel_slice", 1, 64, 3, 64, 64, False, 72),        # Cx = 72 > Ck = 64: the first 64 channels of a 72-channel map
    # ---- thin K (conv_thin_k_kernel<NV, 8> and, for N = 512 on whole 64-byte runs, conv_thin_k_sload_kernel<64>; NV = N / 8)
    Thin("k_nv8_floor", 1, 6, 64, 64, 64, False),                # NV 8, the floor
    Thin("k_nv16_one_channel", 1, 1, 128, 17, 241, False),       # NV 16, one real input channel, M % 4 = 1
    Thin("k_nv32", 2, 6, 256, 47, 45, False),                    # NV 32
    Thin("k_nv32_per_sample", 2, 8, 256, 64, 64, True),          # NV 32, per-sample, all eight inputs real
    Thin("k_sload_one_group", 1, 6, 512, 17, 241, False),        # scalar-load kernel; M = 4097, 8 groups per wave: the last wave holds one group
    Thin("k_nv64_per_sample", 3, 6, 512, 67, 61, True),          # 4087 pixels per sample: the stride fails the 64-byte test, NV 64 on the plain kernel
    Thin("k_sixteen_groups", 1, 6, 512, 363, 362, False),        # groups_per_wave 16; the last wave holds 14.  134 MB of output
]
THIN_BY_NAME = {c.name: c for c in THIN_CASES}
THIN_LARGE = ("n_eight_groups", "k_sixteen_groups")              # rows above 100 MB: operands and reference on the device
THIN_K_RESIDUAL_CASES = ("k_nv8_floor", "k_nv32_per_sample", "k_sload_one_group", "k_nv64_per_sample")    # the residual-merge legs
# the layers whose forward AND data gradient are thin launches: (B, I, O, H, W, per_sample)
THIN_DGRAD_LAYERS = [(2, 512, 6, 47, 45, True), (1, 128, 1, 67, 62, False), (1, 6, 128, 67, 62, False), (1, 256, 8, 65, 64, False)]

# up-convolution (conv_upconv_kernel): I = 512, per-sample weights, N = 4 * O columns in slices of 64 over 8 waves
Upconv = namedtuple("Upconv", "name B O H W")
UPCONV_CASES = [
    Upconv("up_4_slices", 2, 64, 128, 128),                      # 4 slices for 8 waves; each slice is a different sub-pixel (dy, dx)
    Upconv("up_12_slices", 2, 192, 128, 128),                    # 12 slices: a ragged second round, three slices per sub-pixel
    Upconv("up_xcd_samples", 16, 64, 128, 128),                  # samples dealt to XCDs with j in {0, 1}
    Upconv("up_ragged_odd_w", 2, 64, 130, 127),                  # last tile has 126 live rows; odd W in the pixel-shuffle address
    Upconv("up_one_sample", 1, 64, 256, 128),                    # one sample, 256 tiles
]

# one step outside a rule: another kernel's name.  Asserted on the host only.  (family, row, the kernel that takes it)
STREAM_GUARD_CASES = [
    ("thin", Thin("guard_n_below_floor", 1, 64, 3, 63, 65, False), "REG"),          # M = 4095
    ("thin", Thin("guard_k_below_floor", 1, 6, 64, 63, 65, False), "REG"),          # M = 4095
    ("thin", Thin("guard_k_nv24", 2, 6, 192, 50, 47, True), "REG"),                 # N / 8 = 24 does not divide 64
    ("upconv", Upconv("guard_up_128_tiles", 1, 64, 128, 128), "DMA"),               # 128 tiles, below the 256 needed
    ("upconv", Upconv("guard_up_16383_pixels", 3, 128, 129, 127), "PP"),            # one pixel below the 16384 of the rule
    ("upconv", Upconv("guard_up_o96", 2, 96, 128, 128), "DMA"),                     # O not a multiple of 64
]

UPCONV_I = 512


def thin_launch(c, bf16, has_bias=0, epilogue=0):
    """msg_conv2d_fprop_launch_plan arguments of a Thin row as the Python layer forms them: Cx = the map's channels in whole 16-byte
    vectors, Ck = I rounded up to a 128-byte run, ldy = O rounded up to 8, the per-sample weight stride one dense image."""
    ck = _up(c.I, 64)
    return (bf16, c.B, c.H, c.W, c.cx or _up(c.I, 8), ck, c.H, c.W, c.O, _up(c.O, 8), 1, 1, 1, 0, 1, 0, int(c.per_sample) * c.O * ck,
            has_bias, epilogue)


def upconv_launch(c, bf16):
    """... of an Upconv row: a 1x1 conv to the 4 * O sub-pixel planes, stored pixel-shuffled, one dense weight image per sample."""
    return (bf16, c.B, c.H, c.W, UPCONV_I, UPCONV_I, c.H, c.W, 4 * c.O, _up(c.O, 8), 1, 1, 1, 0, 1, 1, 4 * c.O * UPCONV_I, 0, 0)


def thin_groups_per_wave(args):
    """The pixel groups each wave of a thin launch takes.  The plan query does not show it, so this MIRRORS thin_grid in
    csrc/conv_thin.hip and must move with it: thin N (N <= 8) has groups of 16 pixels, one group per 8192 groups of the launch,
    between 1 and 8; thin K has groups of 64 / (N / 8) pixels, one per 16384, rounded up to whole steps of THIN_K_U = 8, between 8
    and 32."""
    thin_n = args[N_] <= 8
    ppw = 16 if thin_n else 64 // (args[N_] // 8)
    groups = (gemm_rows(args) + ppw - 1) // ppw
    samples = args[B_] if args[W_BATCH_STRIDE] else 1
    per, lo, hi = (8192, 1, 8) if thin_n else (16384, 8, 32)
    g = (groups * samples + per - 1) // per
    if not thin_n:
        g = _up(g, 8)
    return min(max(g, lo), hi)
