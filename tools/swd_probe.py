#!/usr/bin/env python3
"""The sliced Wasserstein kernels (csrc/swd.hip: msg_laplacian_level, msg_swd_gather, msg_swd_plane_sums, msg_swd_project,
msg_sorted_l1) and torch.sort, timed over ONE score of the default validation pass -- 5 000 samples of 256 x 256 per set, five
pyramid levels, 128 descriptors per sample (n = 640 000 rows per level and set), 4 x 128 directions -- and beside it the same
definition on stock device operators in fp32:

  pyramid     conv2d on a reflect-padded batch (stride 2 down; zero-stuffed, 4 F up) and a subtraction
  descriptors unfold(7) of a chunk of planes, then an index_select of the K drawn patches per sample
  normalise   mean / std per plane over the rows, a normalised copy of the [n, P 49] matrix
  project     torch.mm(rows, dirs): [n, R], sorted along dim 0
  l1          (a - b).abs().mean()

Both walk the samples in batches of --batch (the sets are never whole on the device as frames).  Kernel times are the sums of
HIP-event spans around every launch (``_lib.kernel_clock``); the sort is timed between events around ``torch.sort`` on the
projected arrays themselves; stock times are event spans around each group of statements.  `score` columns show that both
computed the same number.  The whole run ends itself after --time-limit seconds.
GPU box:  python tools/swd_probe.py [--planes 3] [--out FILE]"""
import argparse
import collections
import os
import signal
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_stylegan_amd import _lib, validation_metrics as vm                       # noqa: E402

DEV = "cuda:0"


class Spans:
    """Event spans summed per label."""

    def __init__(self):
        self.items = collections.defaultdict(list)

    def __call__(self, label, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        self.items[label].append((a, b))
        return out

    def totals(self):
        torch.cuda.synchronize()
        return {k: sum(a.elapsed_time(b) for a, b in v) for k, v in self.items.items()}


def frames_batch(n, planes, side, seed, blur):
    """Smooth random frames (so that the pyramid's levels differ): noise, box-blurred ``blur`` times."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((n, planes, side, side), device=DEV, generator=gen)
    for _ in range(blur):
        x = F.avg_pool2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), 3, stride=1)
    return x * 100.0 + 500.0


def kernel_rows(args, seed, blur):
    """[levels] -> [n, P 49]: the package's path, batch by batch."""
    parts, cpu = None, torch.Generator().manual_seed(seed)
    for start in range(0, args.samples, args.batch):
        frames = frames_batch(min(args.batch, args.samples - start), args.planes, args.side, seed * 100003 + start, blur)
        levels = vm.laplacian_pyramid(frames)
        parts = parts or [[] for _ in levels]
        for level, into in zip(levels, parts):
            pos = vm.swd_positions(level.shape[0], level.shape[2], level.shape[3], args.descriptors, cpu)
            into.append(vm.swd_descriptors(level, pos))
    return [torch.cat(p) for p in parts]


def stock_filter(x, gain, stride):
    f = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], device=x.device) / 16.0
    k = (gain * torch.outer(f, f))[None, None]
    n, p, h, w = x.shape
    return F.conv2d(F.pad(x.reshape(n * p, 1, h, w), (2, 2, 2, 2), mode="reflect"), k, stride=stride).reshape(n, p, h // stride, w // stride)


def stock_rows(args, seed, blur, spans):
    parts, cpu = None, torch.Generator().manual_seed(seed)
    sizes = vm._pyramid_sizes(args.side, args.side, 16)
    for start in range(0, args.samples, args.batch):
        g = frames_batch(min(args.batch, args.samples - start), args.planes, args.side, seed * 100003 + start, blur)
        levels = []

        def pyramid():
            nonlocal g
            for _ in sizes[:-1]:
                coarse = stock_filter(g, 1.0, 2)
                stuffed = torch.zeros_like(g)
                stuffed[..., ::2, ::2] = coarse
                levels.append(g - stock_filter(stuffed, 4.0, 1))
                g = coarse
            levels.append(g)
        spans("pyramid", pyramid)
        parts = parts or [[] for _ in levels]
        for level, into in zip(levels, parts):
            B, P, h, w = level.shape
            pos = vm.swd_positions(B, h, w, args.descriptors, cpu).to(DEV).long()
            which = (pos[..., 0] - 3) * (w - 6) + (pos[..., 1] - 3)                 # the patch's index among unfold's columns

            def gather():
                out = []
                for i in range(0, B, args.unfold_chunk):
                    cols = F.unfold(level[i:i + args.unfold_chunk], 7)             # [b, P 49, (h - 6) (w - 6)]
                    pick = which[i:i + args.unfold_chunk, None, :].expand(-1, cols.shape[1], -1)
                    out.append(cols.gather(2, pick).transpose(1, 2).reshape(-1, P * 49))
                return torch.cat(out)
            into.append(spans("descriptors", gather))
    return [torch.cat(p) for p in parts]


def stock_score(real, fake, planes, dirs, spans):
    n, d = real.shape

    def normalised(rows):
        x = rows.view(n, planes, 49)
        mean, std = x.mean(dim=(0, 2), keepdim=True), x.std(dim=(0, 2), keepdim=True, unbiased=False)
        return ((x - mean) / std).reshape(n, d)
    a, b = spans("normalise", lambda: normalised(real)), spans("normalise", lambda: normalised(fake))
    total = torch.zeros((), device=DEV, dtype=torch.float64)
    for rep in range(dirs.shape[0]):
        dr = dirs[rep].to(DEV)
        pa, pb = spans("project", lambda: torch.mm(a, dr)), spans("project", lambda: torch.mm(b, dr))
        pa, pb = spans("sort", lambda: pa.sort(dim=0).values), spans("sort", lambda: pb.sort(dim=0).values)
        total += spans("l1", lambda: (pa - pb).abs().mean(dtype=torch.float64))
    return 1000.0 * float(total) / dirs.shape[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--samples", type=int, default=5000)
    ap.add_argument("--side", type=int, default=256)
    ap.add_argument("--planes", type=int, default=1, help="1: SWD; T: SWVD on clips of T frames")
    ap.add_argument("--descriptors", type=int, default=128)
    ap.add_argument("--batch", type=int, default=250)
    ap.add_argument("--unfold-chunk", type=int, default=8)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("swd_probe needs the GPU: a host timing says nothing about it")
    signal.alarm(args.time_limit)
    lines = [f"{args.samples} samples of {args.planes} x {args.side} x {args.side} per set, {args.descriptors} descriptors per sample, "
             "4 x 128 directions; times in ms, summed over one score"]
    with torch.no_grad():
        # warm-up: every kernel and stock operator once on one batch of the timed shape (libraries pick their algorithms per shape)
        small = argparse.Namespace(**{**vars(args), "samples": args.batch})
        warm = kernel_rows(small, 1, 0)
        vm.sliced_wasserstein(warm[0], warm[0].flip(0), args.planes, generator=torch.Generator().manual_seed(0))
        stock_rows(small, 1, 0, Spans())
        stock_score(warm[0], warm[0].flip(0), args.planes, vm.swd_directions(warm[0].shape[1], 1, 128), Spans())
        torch.cuda.synchronize()

        # ---- the kernels
        _lib.kernel_clock.reset(True)
        real, fake = kernel_rows(args, 1, 0), kernel_rows(args, 2, 1)
        sort_ms, scores = 0.0, []
        for lvl, (r, f) in enumerate(zip(real, fake)):
            scores.append(vm.sliced_wasserstein(r, f, args.planes, generator=torch.Generator().manual_seed(10 + lvl)))
            probe = torch.randn((128, r.shape[0]), device=DEV)
            spans = Spans()
            for _ in range(3):
                spans("sort", lambda: torch.sort(probe, dim=1).values)
            torch.cuda.synchronize()
            sort_ms += 8 * sorted(a.elapsed_time(b) for a, b in spans.items["sort"])[1]       # the median; 2 sets x 4 repeats
            del probe
        torch.cuda.synchronize()
        by_kernel = collections.defaultdict(float)
        for key, item in _lib.kernel_clock.summary().items():
            by_kernel[key.split("/")[0]] += item["total_ms"]
        _lib.kernel_clock.reset(False)
        lines.append(f"kernels: n = {real[0].shape[0]} rows of {real[0].shape[1]} per level and set, {len(real)} levels")
        for key in ("laplacian_level", "swd_gather", "swd_plane_sums", "swd_project", "sorted_l1"):
            lines.append(f"  {key:18s} {by_kernel[key]:10.2f}")
        lines.append(f"  {'torch.sort (40 x)':18s} {sort_ms:10.2f}")
        lines.append(f"  {'sum':18s} {sum(by_kernel.values()) + sort_ms:10.2f}")
        lines.append("  score per level   " + " ".join(f"{s:.4f}" for s in scores))
        print("\n".join(lines), flush=True)
        del real, fake
        torch.cuda.empty_cache()

        # ---- stock operators
        spans = Spans()
        real, fake = stock_rows(args, 1, 0, spans), stock_rows(args, 2, 1, spans)
        stock = [stock_score(r, f, args.planes, vm.swd_directions(r.shape[1], 4, 128, torch.Generator().manual_seed(10 + lvl)), spans)
                 for lvl, (r, f) in enumerate(zip(real, fake))]
        totals = spans.totals()
        tail = ["stock operators, fp32:"] + [f"  {k:18s} {totals[k]:10.2f}" for k in ("pyramid", "descriptors", "normalise", "project", "sort", "l1")]
        tail.append(f"  {'sum':18s} {sum(totals.values()):10.2f}")
        tail.append("  score per level   " + " ".join(f"{s:.4f}" for s in stock))
        print("\n".join(tail), flush=True)
        lines += tail
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
