"""Convolution test shapes that say which forward-family kernel they are for (conv_fprop_select: thin, upconv, row3, pp, generic),
and the launches they turn into.  tests/test_host.py asserts with msg_conv2d_fprop_launch_plan, on any machine, that every case
selects the kernel it names and that the table as a whole reaches every large-tile kernel, weight mode and tile tail;
tests/test_hip_conv.py runs the cases against float64 and asserts the kernel-clock label of what ran.

The shapes sit at or just above each kernel's own floor -- 224 workgroups for the 256 x 256 tiles, 448 for the 128 x 128 row-sharing
tile, 1024 GEMM rows -- so that the float64 reference stays quick.  They are not the workload's shapes."""
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
