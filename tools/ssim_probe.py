#!/usr/bin/env python3
"""The structural-similarity kernels (csrc/ssim.hip: msg_ssim_scale, msg_ssim_scale_backward), timed per launch at
[48, 256, 256] and at each coarser scale of its pyramid (128, 64, 32, 16), and one 1000-pair MSSSIM score end to end.

Per launch: --repeats launches between two HIP events after a warm-up on the same shape, the median of --rounds such
windows; achieved GB/s against the ALGORITHMIC bytes -- forward 2 M h w 4 read (+ 2 M (h / 2)(w / 2) 4 written with the halved
planes), backward 3 M h w 4 (x, y read, grad_x written; g_half adds M (h / 2)(w / 2) 4) -- and that rate's share of the 8 TB/s
HBM peak.  The forward launch includes its merge launch over the tiles' partial sums.  The score: 1000 pairs of 256 x 256
single-plane frames through ``validation_metrics.MSSSIM._pair_mean`` (five scales, chunks of 64 pairs), a host clock around the
call and a device synchronise.  The whole run ends itself after --time-limit seconds.
GPU box:  python tools/ssim_probe.py [--out FILE]"""
import argparse
import os
import signal
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_stylegan_amd import _lib, validation_metrics as vm                       # noqa: E402

DEV = "cuda:0"
PEAK = 8.0e12


def window(fn, repeats, rounds):
    """Median over ``rounds`` of the time per call (us) of ``repeats`` calls between two events."""
    times = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(1e3 * a.elapsed_time(b) / repeats)
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--planes", type=int, default=48)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--time-limit", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ssim_probe needs the GPU: a host timing says nothing about it")
    signal.alarm(args.time_limit)
    lib, dev = _lib.lib(), torch.device(DEV)
    stream = _lib.stream_of(dev)
    M = args.planes
    lines = [f"[{M}, h, w] fp32 planes; per launch: median of {args.rounds} windows of {args.repeats} launches; "
             "GB/s against the algorithmic bytes, share of 8 TB/s",
             f"{'launch':34s} {'us':>9s} {'MB':>9s} {'GB/s':>9s} {'of peak':>8s}"]
    gen = torch.Generator(device=DEV).manual_seed(0)
    side = args.side
    while side >= 11:
        x = torch.rand((M, side, side), device=DEV, generator=gen)
        y = (x + 0.05 * torch.randn((M, side, side), device=DEV, generator=gen)).clamp(0.0, 1.0)
        half = side // 2
        sums = torch.empty((M, 2), dtype=torch.float64, device=DEV)
        l1 = torch.empty(M, dtype=torch.float64, device=DEV)
        xh, yh = torch.empty((M, half, half), device=DEV), torch.empty((M, half, half), device=DEV)
        ws = torch.empty(lib.msg_ssim_scale_workspace(M, side, side), dtype=torch.uint8, device=DEV)
        g = torch.randn((M, 3), device=DEV, generator=gen)
        gh = torch.randn((M, half, half), device=DEV, generator=gen)
        grad = torch.empty_like(x)

        def forward(halves):
            _lib.check(lib.msg_ssim_scale(x.data_ptr(), y.data_ptr(), M, side, side, 1e-4, 9e-4, sums.data_ptr(), l1.data_ptr(),
                                          xh.data_ptr() if halves else None, yh.data_ptr() if halves else None, ws.data_ptr(),
                                          stream), "msg_ssim_scale")

        def backward(below):
            _lib.check(lib.msg_ssim_scale_backward(x.data_ptr(), y.data_ptr(), g.data_ptr(), gh.data_ptr() if below else None,
                                                   M, side, side, 1e-4, 9e-4, grad.data_ptr(), stream), "msg_ssim_scale_backward")
        plane, small = 4.0 * M * side * side, 4.0 * M * half * half
        cases = [("forward", lambda: forward(False), 2 * plane), ("forward + halved planes", lambda: forward(True), 2 * plane + 2 * small),
                 ("backward", lambda: backward(False), 3 * plane), ("backward + g_half", lambda: backward(True), 3 * plane + small)]
        for name, fn, nbytes in cases:
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            us = window(fn, args.repeats, args.rounds)
            rate = nbytes / (us * 1e-6)
            lines.append(f"{side:4d} x {side:<4d} {name:23s} {us:9.1f} {nbytes / 1e6:9.2f} {rate / 1e9:9.1f} {rate / PEAK:8.3f}")
        print("\n".join(lines[-4:]), flush=True)
        side = half
        if side < 16:
            break
    # one MSSSIM score: 1000 disjoint pairs out of 2000 kept frames
    metric = vm.MSSSIM(device=DEV, batch_size=64, data_samples=2 * args.pairs, no_rfp=True, no_gfp=True, pairs=args.pairs)
    frames = torch.rand((2 * args.pairs, 1, args.side, args.side), device=DEV, generator=gen)
    with torch.no_grad():
        metric._pair_mean(frames[:256])
        torch.cuda.synchronize()
        walls = []
        for _ in range(3):
            start = time.perf_counter()
            score = metric._pair_mean(frames)
            torch.cuda.synchronize()
            walls.append(time.perf_counter() - start)
    lines.append(f"MSSSIM score, {args.pairs} pairs of 1 x {args.side} x {args.side}, five scales: wall {1e3 * sorted(walls)[1]:.1f} ms "
                 f"(median of 3; {1e3 * min(walls):.1f} .. {1e3 * max(walls):.1f}), score {score:.4f}")
    print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
