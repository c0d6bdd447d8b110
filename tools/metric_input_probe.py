#!/usr/bin/env python3
"""Metric inputs (csrc/metric_input.hip, validation_metrics.metric_inputs) against the chain of stock torch calls they replace, at
the validation pass's shapes: B = 16, one channel of [B, 2, 3, 256, 256] frames, fp32 and bf16.

  IS   one frame, 256^2 -> 299^2, resize then normalise: select_frames, interpolate(antialias=True), normalize_m1_1_batch -- what
       IS._preprocessing ran before metric_inputs
  FVD  the clip, 256^2 -> 224^2, normalise then resize: select_clips, normalize_m1_1_batch, interpolate -- what a caller had to
       wrap an I3D in (FVD did not resize)

Per case, stock and new alternate in one process.  Two figures each, HIP events on the launching stream, median of --reps:
`call` is one call between two events on an otherwise idle stream (what the validation loop sees: host enqueue included);
`stream` is --burst calls back to back between two events, per call (device time once the launches queue up).  The bytes are the
algorithmic ones: the selected source frames once, the output once.  GPU box:  python tools/metric_input_probe.py"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_stylegan_amd import misc                                                # noqa: E402
from multi_stylegan_amd.validation_metrics import metric_inputs, select_clips, select_frames   # noqa: E402

DEV = "cuda:0"


def stock_is(images, channel, size):
    x = select_frames(images, channel)[:, :, 0]
    x = F.interpolate(x.float(), size=size, mode="bilinear", align_corners=False, antialias=True)
    return misc.normalize_m1_1_batch(x[:, :, None])[:, :, 0]


def stock_fvd(images, channel, size):
    x = misc.normalize_m1_1_batch(select_clips(images, channel))
    b, p, t, h, w = x.shape
    return F.interpolate(x.float().reshape(b, p * t, h, w), size=size, mode="bilinear", align_corners=False,
                         antialias=True).reshape(b, p, t, *size)


def median_ms(fn, reps, burst):
    spans = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(burst):
            fn()
        b.record()
        spans.append((a, b))
    torch.cuda.synchronize()
    times = sorted(a.elapsed_time(b) / burst for a, b in spans)
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--burst", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metric_input_probe needs the GPU: a host timing says nothing about it")
    torch.manual_seed(0)
    print(f"B = {args.batch}, reps = {args.reps}, burst = {args.burst}; times in microseconds per call")
    print(f"{'case':34s} {'stock call':>11s} {'new call':>9s} {'stock stream':>13s} {'new stream':>11s} {'new GB/s':>9s}")
    with torch.no_grad():
        for dtype in (torch.float32, torch.bfloat16):
            images = torch.rand(args.batch, 2, 3, 256, 256, device=DEV).to(dtype)
            cases = (("IS  1 frame 256^2->299^2", lambda: stock_is(images, 1, (299, 299)),
                      lambda: metric_inputs(images, 1, t=int(torch.randint(0, 3, (1,))), size=(299, 299),
                                            normalize="resized")[:, :, 0], 1, 299),
                     ("FVD 3 frames 256^2->224^2", lambda: stock_fvd(images, 1, (224, 224)),
                      lambda: metric_inputs(images, 1, size=(224, 224), normalize="source"), 3, 224))
            for name, stock, new, frames, side in cases:
                for _ in range(args.warmup):
                    stock(), new()
                got = {}
                for burst in (1, args.burst):                               # stock and new alternate within each figure
                    for label, fn in (("stock", stock), ("new", new)):
                        got[label, burst] = 1e3 * median_ms(fn, args.reps, burst)
                nbytes = args.batch * frames * (256 * 256 * images.element_size() + 3 * side * side * 4)
                print(f"{name + ' ' + str(dtype).split('.')[1]:34s} {got['stock', 1]:11.1f} {got['new', 1]:9.1f} "
                      f"{got['stock', args.burst]:13.1f} {got['new', args.burst]:11.1f} "
                      f"{nbytes / got['new', args.burst] / 1e3:9.1f}", flush=True)


if __name__ == "__main__":
    main()
