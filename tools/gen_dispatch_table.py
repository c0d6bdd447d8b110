"""Record what the host-side dispatch of the convolution family answers, over a grid of problems, into
tests/golden/dispatch_table.json (replayed by tests/test_host.py::test_dispatch_answers_match_the_recorded_table).

    python -m tools.gen_dispatch_table [--out tests/golden/dispatch_table.json] [--only TABLE]

Host-only: the seven queried entries launch nothing, so no GPU is needed.  The grid (the *_rows functions below; a few thousand
rows): every convolution geometry the two networks issue at 256^2 / batch 16 (+ the discriminator's doubled batch) and 512^2 /
batch 8 -- forward, data gradient, stride-2 data gradient, sub-pixel up-convolution, the thin RGB / head layers -- with shared and
per-sample weights at batch 1, 4, 8, 16, 32, 33, and one value on each side of every threshold of the eligibility functions.
The file holds the ANSWERS, row by row in the order of the *_rows functions, and a digest of the argument rows they belong to: a
changed grid without a regenerated table is an error, not a misaligned comparison.  Regenerate it only from a library whose
dispatch is known good: the table is the reference, not the code."""
import argparse
import hashlib
import json
import os

F32, BF16, SPLIT = 0, 1, 4
BATCHES = (1, 4, 8, 16, 32, 33)
SIZES = (4, 8, 16, 32, 64, 128, 256, 512)
# (input channels, output channels, map sizes) of the 'same' convolutions of the two networks and of their data gradients, at the
# 256^2 and the 512^2 configuration: the generator's 512 -> 512 at every size, the discriminator's encoder / decoder per level
LAYERS = ((512, 512, SIZES), (128, 128, (256, 512)), (128, 256, (128, 256, 512)), (256, 128, (128, 256, 512)), (256, 256, (128, 256)),
          (256, 384, (128, 256)), (384, 256, (128, 256)), (384, 384, (64, 128)), (384, 768, (64, 128)), (768, 384, (64, 128)),
          (768, 768, (32, 64)), (768, 1024, (32, 64)), (1024, 768, (32, 64)), (1024, 1024, (16, 32)))
STRIDE2 = ((128, (256, 512)), (256, (128, 256)), (384, (64, 128)), (768, (32, 64)))      # the discriminator's down-sampling convs


def plan_rows():
    """Arguments of msg_conv2d_fprop_plan (and, with has_noise appended, of msg_conv2d_fprop_act_backward_workspace)."""
    rows = []

    def add(dtype, b, ih, iw, cx, ck, oh, ow, n, kh, kw, per_sample, wstride=None):
        rows.append([dtype, b, ih, iw, cx, ck, oh, ow, n, kh, kw, (n * kh * kw * ck if wstride is None else wstride) if per_sample else 0])

    for b in BATCHES:
        for ps in (0, 1):
            for cin, cout, sizes in LAYERS:
                for r in sizes:
                    for k in (1, 3):
                        add(BF16, b, r, r, cin, cin, r, r, cout, k, k, ps)
            for c, sizes in STRIDE2:
                for r in sizes:
                    add(BF16, b, r, r, c, c, r // 2 - 1, r // 2 - 1, c, 3, 3, ps)               # stride-2 3x3, no padding
                    add(BF16, b, r // 2 - 1, r // 2 - 1, c, c, r // 2, r // 2, 4 * c, 2, 2, ps)  # ... its data gradient, sub-pixel form
            for r in SIZES:
                if r >= 8:
                    add(BF16, b, r, r, 512, 512, r // 2, r // 2, 512, 2, 2, ps)                 # the up-convolution's data gradient
                    add(BF16, b, r, r, 512, 512, r, r, 2048, 1, 1, ps)                          # sub-pixel up-convolution
                # thin layers: RGB heads (512 -> 6), their data gradient and the first residual conv (8-padded input), the head
                add(BF16, b, r, r, 512, 512, r, r, 6, 1, 1, ps)
                add(BF16, b, r, r, 8, 64, r, r, 512, 1, 1, ps)
                add(BF16, b, r, r, 8, 64, r, r, 128, 1, 1, ps)
                add(BF16, b, r, r, 128, 128, r, r, 1, 1, 1, ps)
    # fp32 storage (exact and split products): the small-model paths
    for dtype in (F32, SPLIT):
        for b in (1, 16):
            for r in (16, 256):
                for cin, cout in ((128, 128), (256, 256), (512, 512)):
                    for k in (1, 3):
                        for ps in (0, 1):
                            add(dtype, b, r, r, cin, cin, r, r, cout, k, k, ps)
    # ---- thresholds.  mtot 1024 (row3 / pp floor): 31x33 = 1023, 32x32 = 1024
    for hw in ((31, 33), (32, 32), (16, 64), (16, 32)):
        for n in (128, 256, 512):
            for b in (1, 2, 64):
                add(BF16, b, hw[0], hw[1], 512, 512, hw[0], hw[1], n, 3, 3, 0)
                add(BF16, b, hw[0], hw[1], 512, 512, hw[0], hw[1], n, 1, 1, 0)
    # block floors 224 (256-tile) / 448 (128-tile): blocks = mtot / tile * n_tiles
    for r, n in ((64, 256), (64, 512), (32, 128), (64, 128), (32, 768)):
        for b in range(1, 40):
            add(BF16, b, r, r, 256, 256, r, r, n, 3, 3, b % 2)
            add(BF16, b, r, r, 256, 256, r, r, n, 1, 1, 0)
    # the 15 % padding rule at N = 128 / 256 / 384 / 640 and around them; OW 32 on both sides; Ck <= 128 short-K rule
    for n in (64, 120, 128, 136, 192, 224, 248, 256, 264, 296, 320, 384, 392, 448, 512, 576, 640, 648, 704, 768, 896, 1024):
        for r in (32, 64):
            for ck in (128, 192):
                for k in (1, 3):
                    add(BF16, 16, r, r, ck, ck, r, r, n, k, k, 0)
    # n_iters 7 / 8 (DMA rule: bf16 chunks of 64, fp32 of 32) and PP's n_iters 3 / 4
    for dtype, chunk in ((BF16, 64), (F32, 32), (SPLIT, 32)):
        for m in (1, 2, 3, 4, 5, 7, 8, 9, 16):
            for n in (128, 256):
                add(dtype, 16, 64, 64, m * chunk, m * chunk, 64, 64, n, 1, 1, 0)
                add(dtype, 16, 64, 64, m * chunk, m * chunk, 64, 64, n, 1, 1, 1)
        add(dtype, 16, 64, 64, chunk, chunk, 64, 64, 128, 3, 3, 0)
    # 2 GiB limits: activations behind one descriptor (shared: the batch; per-sample: one sample) and one weight set
    for b in (31, 32, 33, 64):
        for ps in (0, 1):
            for k in (1, 3):
                add(BF16, b, 256, 256, 512, 512, 256, 256, 512, k, k, ps)
                add(BF16, b, 256, 256, 512, 512, 256, 256, 256, k, k, ps)
                add(F32, b, 256, 256, 256, 256, 256, 256, 256, k, k, ps)
    for b in (1, 2, 3, 4, 5):
        add(BF16, b, 1024, 1024, 512, 512, 1024, 1024, 512, 3, 3, 1)
        add(BF16, b, 2048, 1024, 512, 512, 2048, 1024, 512, 3, 3, 1)
    for n in (8192, 16384, 32768):                                                     # weight set: N * 9 * Ck * 2 bytes
        add(BF16, 16, 64, 64, 8192, 8192, 64, 64, n, 3, 3, 0)
        add(BF16, 16, 64, 64, 8192, 8192, 64, 64, n, 1, 1, 0)
    # map widths against the row-sharing tiles: whole segments per tile or not
    for ow in (16, 32, 48, 64, 96, 128, 192, 256, 320, 384, 512):
        for n in (128, 256):
            add(BF16, 16, 128, ow, 256, 256, 128, ow, n, 3, 3, 0)
    # thin: m 4096, Ck 32 .. 512 in steps of 32, N around 8
    for ck in range(32, 545, 32):
        for n in (1, 6, 8, 9):
            add(BF16, 16, 256, 256, ck, ck, 256, 256, n, 1, 1, 1)
            add(BF16, 16, 256, 256, ck, ck, 256, 256, n, 1, 1, 0)
    for hw in ((63, 65), (64, 64), (32, 64)):
        add(BF16, 1, hw[0], hw[1], 512, 512, hw[0], hw[1], 6, 1, 1, 0)
        add(BF16, 1, hw[0], hw[1], 8, 64, hw[0], hw[1], 512, 1, 1, 0)
    for b in (65535, 65536):                                                            # per-sample weights: grid.y counts samples
        add(BF16, b, 4, 4, 512, 512, 4, 4, 6, 1, 1, 1)
        add(BF16, b, 4, 4, 8, 64, 4, 4, 512, 1, 1, 1)
    return rows


def upconv_rows():
    """Arguments of msg_conv2d_fprop_upconv_eligible."""
    rows = []
    for b in BATCHES + (2, 3):
        for r in SIZES + (127, 129):
            rows.append([b, r, r, 512, 512, r, r, 2048, 1, 1, 1, 0, 1, 1, 2048 * 512])
            rows.append([b, r, r, 512, 512, r, r, 2048, 1, 1, 1, 0, 1, 1, 0])
    base = [16, 128, 128, 512, 512, 128, 128, 2048, 1, 1, 1, 0, 1, 1, 2048 * 512]
    for i, vals in ((3, (256, 1024)), (4, (256, 1024)), (7, (1024, 1536, 1792, 2304, 4096)), (8, (3,)), (9, (3,)), (10, (2,)), (11, (1,)),
                    (12, (2,)), (13, (0,)), (5, (64,)), (6, (64,)), (14, (4096 * 512, 2048 * 512 - 8, 512))):
        for v in vals:
            row = list(base)
            row[i] = v
            if i == 7:
                row[14] = v * 512
            rows.append(row)
    for b in (1, 2):                                                                    # hw 16384; tiles * B 256
        for hw in ((127, 129), (128, 128), (64, 128), (128, 256), (181, 181)):
            rows.append([b, hw[0], hw[1], 512, 512, hw[0], hw[1], 2048, 1, 1, 1, 0, 1, 1, 2048 * 512])
    return rows


def thin_rows():
    """Arguments of msg_conv2d_fprop_thin_eligible."""
    rows = []
    for act in (0, 1, 2):
        for b in BATCHES:
            for r in (16, 32, 64, 256, 512):
                rows.append([b, r, r, 512, 512, r, r, 6, 8, 1, 1, 1, 0, 1, 0, act])    # RGB heads
                rows.append([b, r, r, 128, 128, r, r, 1, 8, 1, 1, 1, 0, 1, 0, act])    # pixel-wise head
                rows.append([b, r, r, 8, 64, r, r, 512, 512, 1, 1, 1, 0, 1, 0, act])   # RGB heads' data gradient
                rows.append([b, r, r, 8, 64, r, r, 128, 128, 1, 1, 1, 0, 1, 0, act])   # first residual conv / head's data gradient
        for ck in range(32, 545, 32):
            for n in (6, 9):
                rows.append([16, 256, 256, max(ck, 512), ck, 256, 256, n, 8, 1, 1, 1, 0, 1, 0, act])
            rows.append([16, 256, 256, ck, ck, 256, 256, 1, 8, 1, 1, 1, 0, 1, 0, act])
        for n in (8, 56, 64, 72, 128, 192, 256, 320, 384, 512, 576, 1024):
            for ldy in (n, n + 8, n + 4):
                rows.append([16, 256, 256, 8, 64, 256, 256, n, ldy, 1, 1, 1, 0, 1, 0, act])
        for hw in ((63, 65), (64, 64), (32, 64)):                                       # m 4096
            rows.append([1, hw[0], hw[1], 512, 512, hw[0], hw[1], 6, 8, 1, 1, 1, 0, 1, 0, act])
            rows.append([1, hw[0], hw[1], 8, 64, hw[0], hw[1], 512, 512, 1, 1, 1, 0, 1, 0, act])
    base = [16, 256, 256, 512, 512, 256, 256, 6, 8, 1, 1, 1, 0, 1, 0, 0]
    for i, v in ((8, 16), (9, 3), (10, 3), (11, 2), (12, 1), (13, 2), (14, 1), (5, 128), (6, 128), (0, 0), (3, 256), (3, 516)):
        row = list(base)
        row[i] = v
        rows.append(row)
    return rows


def model_k_chunks(b, o, i, taps, oh, ow, per_sample, kp=64):
    """The K split the Python layer passed for the models' layers when the table was recorded (kp: pixels per K-step, 64 bf16 /
    32 fp32) -- the rule the recorded rows were built with, frozen here: NOT to be edited.  The library's MSG_WGRAD_K_AUTO
    (conv_wgrad_default_chunks, csrc/conv_dispatch.h) must give the same number; tests/test_host.py holds it to that."""
    tiles = ((o + 127) // 128) * ((i + 127) // 128) * taps * b
    if per_sample:
        return max(1, min((oh * ow) // (16 * kp), 1024 // tiles)) if tiles < 256 else 1
    k_chunks = max(1, min((oh * ow + 4 * kp - 1) // (4 * kp), (1024 + tiles - 1) // tiles))
    while b * k_chunks > 65535:
        k_chunks -= 1
    return k_chunks


def missing_profile_geometries(paths):
    """The conv_fprop* / conv_wgrad labels of the per-shape kernel tables (profiles/*shape_table*.txt: what the benchmarked models
    launch) that have no row in the grid -- matched on batch, maps, channels (input channels padded to 64), taps, stride,
    pixel shuffle and shared / per-sample weights."""
    import re
    pat = re.compile(r"(conv_fprop\w*|conv_wgrad)\|B(\d+) (\d+)x(\d+)->(\d+)x(\d+) (\d+)->(\d+) (\d)x(\d) s(\d)(?: up\d)?( ps)?( per-sample)?")
    fprop = {(r[1], r[2], r[3], r[6], r[7], r[5], r[8], r[9], r[10], int(r[11] != 0)) for r in plan_rows()}
    wgrad = {(r[1], r[2], r[3], r[6], r[7], r[5], r[9], r[11], r[12], r[13], r[15], r[16]) for r in wgrad_rows()}
    missing = set()
    for path in paths:
        for m in pat.finditer(open(path).read()):
            b, ih, iw, oh, ow, c, n, kh, kw, s = map(int, m.groups()[1:11])
            ps, per = int(bool(m.group(12))), int(bool(m.group(13)))
            found = (b, ih, iw, oh, ow, c, n, kh, kw, s, ps, per) in wgrad if m.group(1) == "conv_wgrad" else \
                (b, ih, iw, oh, ow, -(-c // 64) * 64, n, kh, kw, per) in fprop
            if not found:
                missing.add(m.group(0))
    return sorted(missing)


def wgrad_rows():
    """Arguments of msg_conv2d_wgrad_workspace."""
    rows = []

    def add(dtype, b, ih, iw, cx, i, oh, ow, o, kh, kw, stride, pad, shuffle, per_sample, k_chunks=1, ldgy=None, ldgw=None):
        rows.append([dtype, b, ih, iw, cx, i, oh, ow, (o // 4 if shuffle else o) if ldgy is None else ldgy, o,
                     (i + 3) // 4 * 4 if ldgw is None else ldgw, kh, kw, stride, pad, shuffle, per_sample, k_chunks])

    for b in BATCHES:
        for ps in (0, 1):
            # (the models' rows carry the k_chunks the library's MSG_WGRAD_K_AUTO stands for on them: model_k_chunks)
            for cin, cout, sizes in LAYERS:
                for r in sizes:
                    for k in (1, 3):
                        add(BF16, b, r, r, cin, cin, r, r, cout, k, k, 1, k // 2, 0, ps, model_k_chunks(b, cout, cin, k * k, r, r, ps))
            for c, sizes in STRIDE2:
                for r in sizes:                                                                    # stride-2 3x3, no padding
                    add(BF16, b, r, r, c, c, r // 2 - 1, r // 2 - 1, c, 3, 3, 2, 0, 0, ps, model_k_chunks(b, c, c, 9, r // 2 - 1, r // 2 - 1, ps))
            for r in SIZES[:-1]:                                         # sub-pixel up-convolution: 2x2 taps, gradient map of 2r x 2r x 512
                add(BF16, b, r, r, 512, 512, r, r, 512, 2, 2, 1, 0, 1, ps, model_k_chunks(b, 512, 512, 4, r, r, ps), ldgy=512)
            for r in (16, 64, 256, 512):
                add(BF16, b, r, r, 512, 512, r, r, 6, 1, 1, 1, 0, 0, ps, model_k_chunks(b, 6, 512, 1, r, r, ps), ldgy=8)
                add(BF16, b, r, r, 8, 6, r, r, 128, 1, 1, 1, 0, 0, ps)
                add(BF16, b, r, r, 128, 128, r, r, 1, 1, 1, 1, 0, 0, ps, ldgy=8)
    for dtype in (F32, SPLIT):
        for b in (1, 16):
            for r in (31, 64, 256):
                for c in (128, 512):
                    for k in (1, 3):
                        for ps in (0, 1):
                            add(dtype, b, r, r, c, c, r, r, c, k, k, 1, k // 2, 0, ps)
    for k_chunks in (2, 3, 4, 8):                                                       # the caller's K split (per-sample weights)
        for b in (8, 16):
            for r in (32, 64, 128, 256):
                add(BF16, b, r, r, 512, 512, r, r, 512, 3, 3, 1, 1, 0, 1, k_chunks)
                add(BF16, b, r, r, 512, 512, r, r, 512, 1, 1, 1, 0, 0, 1, k_chunks)
    for ow in (15, 16, 24, 30, 31, 32, 33, 48, 60, 63, 64, 65, 96, 120, 127, 128, 129, 255):   # padded rows, row-sharing widths
        for oh in ((ow, ow + 1) if ow in (31, 32, 33) else (ow,)):
            for ps in (0, 1):
                add(BF16, 16, oh, ow, 256, 256, oh, ow, 256, 3, 3, 1, 1, 0, ps)
                add(BF16, 16, oh, ow, 256, 256, oh, ow, 256, 1, 3, 1, 1, 0, ps)
                add(F32, 16, oh, ow, 256, 256, oh, ow, 256, 3, 3, 1, 1, 0, ps)
    for b in (15, 16, 17, 31, 32, 33, 64):                                              # 2 GiB limits
        for ps in (0, 1):
            add(BF16, b, 256, 256, 512, 512, 256, 256, 512, 3, 3, 1, 1, 0, ps)
            add(BF16, b, 256, 256, 512, 512, 256, 256, 512, 1, 1, 1, 0, 0, ps)
            add(BF16, b, 512, 512, 512, 512, 512, 512, 512, 3, 3, 1, 1, 0, ps)
    for b in (1, 2):
        add(BF16, b, 2048, 1024, 512, 512, 2048, 1024, 512, 3, 3, 1, 1, 0, 1)
        add(BF16, b, 1024, 1024, 512, 512, 1024, 1024, 512, 3, 3, 1, 1, 0, 1)
    add(BF16, 16, 64, 64, 128, 126, 64, 64, 128, 3, 3, 1, 1, 0, 0, ldgw=126)             # refused: ldgw % 4
    add(BF16, 0, 64, 64, 128, 128, 64, 64, 128, 3, 3, 1, 1, 0, 0)
    return rows


def wgrad_plan_extra_rows():
    """Arguments of msg_conv2d_wgrad_plan beyond wgrad_rows(): the branches of the plan that the workspace size cannot tell apart."""
    rows = []

    def add(dtype, b, h, w, c, o, kh, kw, per_sample, k_chunks=1, shuffle=0):                # stride 1, 'same' padding
        rows.append([dtype, b, h, w, c, c, h, w, o, o, c, kh, kw, 1, 0 if shuffle else kh // 2, shuffle, per_sample, k_chunks])

    for ps in (0, 1):                                                                   # the small shapes of tests/test_hip_conv.py
        for b in (1, 2):
            for h, w in ((8, 64), (8, 32), (7, 32), (16, 16), (15, 15), (12, 24), (32, 64), (6, 15), (3, 8)):
                for dtype in (BF16, F32, SPLIT):
                    add(dtype, b, h, w, 64, 64, 3, 3, ps)
                    add(dtype, b, h, w, 64, 64, 1, 1, ps, 2)
            add(BF16, b, 8, 8, 64, 256, 2, 2, ps, shuffle=1)
    for b in (1, 2, 4, 8, 12, 16):                                                      # row3, per-sample: the library's own split
        for r in (32, 64, 128, 256):
            for c in (128, 256, 512):
                add(BF16, b, r, r, c, c, 3, 3, 1)
    for c, o in ((64, 64), (128, 128), (128, 256), (256, 768), (896, 896), (1024, 512)):     # slice-per-XCD order: <= 6 channel tiles
        for b in (1, 3, 16):
            for r in (8, 16, 48):
                add(BF16, b, r, r, c, o, 3, 3, 0)
                add(BF16, b, r, r, c, o, 3, 3, 1, 8)
    for b in (7, 8, 15, 16, 31, 32):                                                    # row3's 2 GiB rule: gy / x of the batch behind one descriptor
        add(BF16, b, 512, 512, 256, 256, 3, 3, 0)
        add(BF16, b, 1024, 512, 64, 64, 3, 3, 0)
    add(BF16, 1 << 20, 64, 64, 64, 64, 3, 3, 1, 32)                                      # refused: more than 2^24 K-slices
    add(BF16, 70000, 4, 4, 64, 64, 1, 1, 1, 1024)
    add(7, 16, 64, 64, 64, 64, 3, 3, 0)                                                 # refused: no such dtype
    add(BF16, 16, 64, 64, 60, 64, 3, 3, 0)                                              # refused: channel stride not a multiple of 16 bytes
    add(BF16, 16, 64, 64, 64, 64, 3, 3, 0, 0)                                           # invalid: k_chunks 0
    return rows


def wgrad_plan_rows():
    return wgrad_rows() + wgrad_plan_extra_rows()


def wgrad_plan(lib, row):
    """msg_conv2d_wgrad_plan's answer for a row: the MSG_WPLAN_FIELDS fields, or its negative code."""
    import ctypes
    out = (ctypes.c_longlong * 11)()
    rc = lib.msg_conv2d_wgrad_plan(*row, ctypes.addressof(out), 11)
    return list(out) if rc == 0 else rc


def fprop_plan_rows():
    """Arguments of msg_conv2d_fprop_launch_plan: dtype .. w_batch_stride as msg_conv2d_fprop takes them, has_bias, epilogue (0 plain,
    1 fused activation, 2 residual merge, 3 activation backward)."""
    # plan_rows() with what msg_conv2d_fprop_plan assumes spelled out: ldy = N rounded up to 8, stride 1, 'same' padding, no bias
    rows = [r[:9] + [max(8, (r[8] + 7) // 8 * 8)] + r[9:11] + [1, r[9] // 2, 1, 0, r[11], 0, 0] for r in plan_rows()]

    def add(dtype, b, ih, iw, cx, ck, oh, ow, n, kh, kw, stride, pad, per_sample, in_up=1, shuffle=0, ldy=None, bias=0, epilogue=0,
            wstride=None):
        ldy = (max(8, (n + 7) // 8 * 8) if not shuffle else n // 4) if ldy is None else ldy
        wstride = (n * (1 if shuffle else kh * kw) * ck if wstride is None else wstride) if per_sample else 0
        rows.append([dtype, b, ih, iw, cx, ck, oh, ow, n, ldy, kh, kw, stride, pad, in_up, shuffle, wstride, bias, epilogue])

    # the models' launches at batch 16, as conv_ops issues them: every epilogue, and the plain form with a bias
    for ps in (0, 1):
        for bias, epilogue in ((1, 0), (0, 1), (0, 2), (0, 3)):
            for cin, cout, sizes in LAYERS:
                for r in sizes:
                    for k in (1, 3):
                        add(BF16, 16, r, r, cin, cin, r, r, cout, k, k, 1, k // 2, ps, bias=bias, epilogue=epilogue)
            for r in SIZES:                                                                     # the thin layers
                add(BF16, 16, r, r, 512, 512, r, r, 6, 1, 1, 1, 0, ps, bias=bias, epilogue=epilogue)
                add(BF16, 16, r, r, 8, 64, r, r, 512, 1, 1, 1, 0, ps, bias=bias, epilogue=epilogue)
                add(BF16, 16, r, r, 8, 64, r, r, 128, 1, 1, 1, 0, ps, bias=bias, epilogue=epilogue)
                add(BF16, 16, r, r, 128, 128, r, r, 1, 1, 1, 1, 0, ps, bias=bias, epilogue=epilogue)
            for c, sizes in STRIDE2:                                                            # real stride 2, no padding
                for r in sizes:
                    add(BF16, 16, r, r, c, c, r // 2 - 1, r // 2 - 1, c, 3, 3, 2, 0, ps, bias=bias, epilogue=epilogue)
        for bias in (0, 1):                                 # what the old queries could not say: pixel shuffle (ldy = N / 4), in_up
            for c, sizes in STRIDE2:                        # the stride-2 data gradient, sub-pixel form: 2x2 taps, padding 1
                for r in sizes:
                    add(BF16, 16, r // 2 - 1, r // 2 - 1, c, c, r // 2, r // 2, 4 * c, 2, 2, 1, 1, ps, shuffle=1, bias=bias)
            for r in SIZES:
                for b in (1, 2, 16):                        # the sub-pixel up-convolution (its own kernel from 128^2 maps on) ...
                    add(BF16, b, r, r, 512, 512, r, r, 2048, 1, 1, 1, 0, ps, shuffle=1, bias=bias)
                if r >= 8:                                  # ... and its data gradient
                    add(BF16, 16, r, r, 512, 512, r // 2, r // 2, 512, 2, 2, 2, 0, ps, bias=bias)
                add(BF16, 16, r, r, 512, 512, 2 * r, 2 * r, 512, 3, 3, 1, 1, ps, in_up=2, bias=bias)   # zero insertion (transposed 3x3)
        add(BF16, 16, 128, 128, 512, 512, 128, 128, 2048, 1, 1, 1, 0, ps, shuffle=1, wstride=512)      # weight sets that overlap
    for epilogue in (0, 1, 2, 3):
        for n, ldy in ((256, 384), (128, 384), (512, 520)):                                  # a channel slice of a wider map
            for k in (1, 3):
                add(BF16, 16, 128, 128, 256, 256, 128, 128, n, k, k, 1, k // 2, 0, ldy=ldy, epilogue=epilogue)
        add(BF16, 16, 256, 256, 8, 64, 256, 256, 128, 1, 1, 1, 0, 0, ldy=136, epilogue=epilogue)
    for dtype in (F32, SPLIT):                                                                # fp32: ldy a multiple of 4
        for n in (6, 12, 100, 128):
            for k, cx in ((1, 128), (3, 128), (1, 256), (3, 100)):
                for epilogue in (0, 1, 2):
                    add(dtype, 16, 64, 64, cx, (cx + 31) // 32 * 32, 64, 64, n, k, k, 1, k // 2, 0, ldy=(n + 3) // 4 * 4, epilogue=epilogue)
    base = dict(dtype=BF16, b=16, ih=128, iw=128, cx=256, ck=256, oh=128, ow=128, n=256, kh=3, kw=3, stride=1, pad=1, per_sample=0)
    refused = (dict(b=0), dict(b=-1), dict(ih=0), dict(n=0), dict(kh=0), dict(stride=0), dict(in_up=0), dict(ck=0), dict(ldy=0),   # MSG_EINVAL,
               dict(epilogue=4), dict(epilogue=-1), dict(epilogue=1, bias=1), dict(epilogue=2, in_up=2), dict(epilogue=3, shuffle=1),
               dict(dtype=2), dict(dtype=7), dict(ck=224), dict(cx=260, ck=320), dict(ldy=260), dict(n=258, shuffle=1),        # MSG_EUNSUPPORTED
               dict(n=240, shuffle=1, ldy=64), dict(in_up=2, stride=2), dict(dtype=F32, ck=272), dict(dtype=SPLIT, cx=258),
               dict(ck=32704, cx=32704, kh=1, kw=1, pad=0, n=128), dict(ck=32640, cx=32640, kh=1, kw=1, pad=0, n=128))           # K sweep against the 64 KiB zero page: 511 / 510 steps
    for change in refused:
        add(**{**base, **change})
    return rows


def fprop_plan(lib, row):
    """msg_conv2d_fprop_launch_plan's answer for a row: the MSG_FPLAN_FIELDS fields without trailing zeros, or its negative code."""
    import ctypes
    out = (ctypes.c_longlong * 5)()
    rc = lib.msg_conv2d_fprop_launch_plan(*row, ctypes.addressof(out), 5)
    fields = list(out)
    while len(fields) > 1 and not fields[-1]:
        fields.pop()
    return fields if rc == 0 else rc


ROWS = {"plan": plan_rows, "upconv_eligible": upconv_rows, "thin_eligible": thin_rows, "wgrad_workspace": wgrad_rows}
# every table of the file: the four above as they always were (a reader that knows only them still finds each of its digests), and
# the weight-gradient plans and the plans of the forward family
ALL_ROWS = {**ROWS, "wgrad_plan": wgrad_plan_rows, "fprop_plan": fprop_plan_rows}


def digest(rows):
    return hashlib.sha256(json.dumps(rows).encode()).hexdigest()[:16]


def evaluate(lib):
    """{table name: the answers, one per row of ALL_ROWS[name]()}.  plan: [MSG_PLAN_* code, msg_conv2d_fprop_act_backward_workspace
    without and with noise] (the code alone where both are 0)."""
    out = {}
    out["plan"] = []
    for r in plan_rows():
        ans = [lib.msg_conv2d_fprop_plan(*r), lib.msg_conv2d_fprop_act_backward_workspace(*r, 0),
               lib.msg_conv2d_fprop_act_backward_workspace(*r, 1)]
        out["plan"].append(ans if ans[1] or ans[2] else ans[0])
    out["upconv_eligible"] = [lib.msg_conv2d_fprop_upconv_eligible(*r) for r in upconv_rows()]
    out["thin_eligible"] = [lib.msg_conv2d_fprop_thin_eligible(*r) for r in thin_rows()]
    out["wgrad_workspace"] = [lib.msg_conv2d_wgrad_workspace(*r) for r in wgrad_rows()]
    out["wgrad_plan"] = [wgrad_plan(lib, r) for r in wgrad_plan_rows()]
    out["fprop_plan"] = [fprop_plan(lib, r) for r in fprop_plan_rows()]
    return out


def main():
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(root, "tests", "golden", "dispatch_table.json"))
    ap.add_argument("--only", action="append", choices=sorted(ALL_ROWS), help="record this table alone (repeatable); the others keep "
                    "the answers the file holds -- how a NEW table is recorded without re-recording the reference of the rest")
    a = ap.parse_args()
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    build(verbose=False)
    tables = evaluate(_lib.lib())
    if a.only:
        with open(a.out) as f:
            kept = json.load(f)
        tables = {k: v if k in a.only else kept[k] for k, v in tables.items()}
    with open(a.out, "w") as f:
        f.write('{\n "rows": "tools/gen_dispatch_table.py: ALL_ROWS[name]() gives the arguments, in this order; digest = of those rows",\n')
        f.write(' "digest": ' + json.dumps({k: digest(fn()) for k, fn in ALL_ROWS.items()}))
        for k, v in tables.items():
            body = textwrap.fill(json.dumps(v, separators=(",", ":")).replace(",", ", "), 180).replace(", ", ",")
            f.write(f',\n "{k}": ' + body.replace("\n", "\n  "))
        f.write("\n}\n")
    print({k: len(v) for k, v in tables.items()}, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
