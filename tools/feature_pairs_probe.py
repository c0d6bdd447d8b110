#!/usr/bin/env python3
"""The pairwise feature kernels (csrc/feature_pairs.hip: msg_feature_knn, msg_feature_ball_hits, msg_poly_mmd) against the
stock-operator statement of the same outputs, at the sizes of a validation pass: N = M = 500 and 5 000 rows of d = 2048 features.

  knn    radii of a set against itself, k = 3, row i excluded; stock: per block of --chunk query rows, |q|^2 + |r|^2 - 2 q r^T by
         torch.mm, the diagonal masked, topk
  ball   margins and counts of one set against the other's balls; stock: the same distance block, min and a compared sum
  kid    the three kernel sums of S = 100 subsets of m = min(N, 1000) rows; stock: per subset two gathers, three torch.mm,
         pow(3), sum in float64

Per case the stock statement and the kernel alternate in one process; a time is the median of --reps runs between two HIP events
on the launching stream, after --warmup runs of each.  `extra MiB` is the peak of torch's allocator above what was allocated
before the call (inputs excluded, outputs and workspaces included).  `same bits` is the kernel called twice on the same inputs.
The whole run ends itself after --time-limit seconds.  GPU box:  python tools/feature_pairs_probe.py [--out FILE]"""
import argparse
import os
import signal
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_stylegan_amd import validation_metrics as vm                            # noqa: E402

DEV = "cuda:0"


def stock_blocks(q, r, chunk):
    rn = r.square().sum(dim=1)
    for i in range(0, q.shape[0], chunk):
        part = q[i:i + chunk]
        yield i, (part.square().sum(dim=1)[:, None] + rn[None, :] - 2.0 * torch.mm(part, r.t())).clamp_min_(0.0)


def stock_knn_self(x, k, chunk):
    out = []
    for i, dist in stock_blocks(x, x, chunk):
        rows = torch.arange(dist.shape[0], device=x.device)
        dist[rows, rows + i] = float("inf")
        out.append(dist.topk(k, dim=1, largest=False).values[:, k - 1])
    return torch.cat(out)


def stock_ball(q, r, radius2, chunk):
    margin, count = [], []
    for _, dist in stock_blocks(q, r, chunk):
        margin.append((dist - radius2[None, :]).min(dim=1).values)
        count.append((dist <= radius2[None, :]).sum(dim=1, dtype=torch.int32))
    return torch.cat(margin), torch.cat(count)


def stock_kid(x, y, ix, iy):
    gamma = 1.0 / x.shape[1]
    out = torch.empty((ix.shape[0], 3), dtype=torch.float64, device=x.device)
    for s in range(ix.shape[0]):
        xs, ys = x[ix[s]], y[iy[s]]
        kxx, kyy, kxy = ((torch.mm(a, b.t()) * gamma + 1.0).pow(3) for a, b in ((xs, xs), (ys, ys), (xs, ys)))
        out[s, 0] = kxx.sum(dtype=torch.float64) - kxx.diagonal().sum(dtype=torch.float64)
        out[s, 1] = kyy.sum(dtype=torch.float64) - kyy.diagonal().sum(dtype=torch.float64)
        out[s, 2] = kxy.sum(dtype=torch.float64)
    return out


def timed(fn, reps):
    spans = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        spans.append((a, b))
    torch.cuda.synchronize()
    times = sorted(a.elapsed_time(b) for a, b in spans)
    return times[len(times) // 2]


def extra_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    result = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del result
    return peak / 2.0 ** 20


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", type=int, nargs="+", default=[500, 5000])
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--subsets", type=int, default=100)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--time-limit", type=int, default=420)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("feature_pairs_probe needs the GPU: a host timing says nothing about it")
    signal.alarm(args.time_limit)
    lines = [f"d = {args.d}, k = 3, S = {args.subsets}, stock chunk = {args.chunk} query rows, median of {args.reps}; times in ms",
             f"{'case':18s} {'stock ms':>9s} {'kernel ms':>10s} {'stock/kernel':>13s} {'stock extra MiB':>16s} {'kernel extra MiB':>17s} "
             f"{'kernel TFLOP/s':>15s} {'same bits':>10s} {'max |stock - kernel|':>21s}"]
    print("\n".join(lines), flush=True)
    with torch.no_grad():
        for n in args.sizes:
            gen = torch.Generator(device=DEV).manual_seed(n)
            x = torch.randn(n, args.d, device=DEV, generator=gen)
            y = 0.8 * torch.randn(n, args.d, device=DEV, generator=gen) + 0.05
            x, y = x - x.mean(dim=0, keepdim=True), y - x.mean(dim=0, keepdim=True)
            radius2 = vm._knn(x, x, 3, True, True)
            m = min(n, 1000)
            cpu = torch.Generator().manual_seed(n)
            ix, iy = vm.subset_indices(n, m, args.subsets, cpu).to(DEV), vm.subset_indices(n, m, args.subsets, cpu).to(DEV)
            ixl, iyl = ix.long(), iy.long()
            pair_flop = 2.0 * n * n * args.d
            cases = (("knn", lambda: stock_knn_self(x, 3, args.chunk), lambda: vm._knn(x, x, 3, True, True), pair_flop),
                     ("ball", lambda: stock_ball(y, x, radius2, args.chunk), lambda: vm._ball_hits(y, x, radius2, True), pair_flop),
                     ("kid", lambda: stock_kid(x, y, ixl, iyl), lambda: vm._poly_sums(x, y, ix, iy, 1.0 / args.d, 1.0, True),
                      args.subsets * 2.0 * args.d * 2.0 * m * m))       # (x x and y y over the upper triangle: half each)
            for name, stock, new, flop in cases:
                for _ in range(args.warmup):
                    stock(), new()
                t_stock, t_new = [], []
                for _ in range(3):                                          # stock and kernel alternate
                    t_stock.append(timed(stock, max(1, args.reps // 3)))
                    t_new.append(timed(new, max(1, args.reps // 3)))
                t_stock, t_new = sorted(t_stock)[1], sorted(t_new)[1]
                mem_stock, mem_new = extra_mib(stock), extra_mib(new)
                a, b, ref = new(), new(), stock()
                a, b, ref = (tuple(t.cpu() for t in (v if isinstance(v, tuple) else (v,))) for v in (a, b, ref))
                same = all(torch.equal(p, q_) for p, q_ in zip(a, b))
                diff = max(float((p.double() - q_.double()).abs().max()) for p, q_ in zip(a, ref))
                line = (f"{name + ' n = ' + str(n):18s} {t_stock:9.3f} {t_new:10.3f} {t_stock / t_new:13.2f} {mem_stock:16.1f} "
                        f"{mem_new:17.1f} {flop / t_new / 1e9:15.1f} {str(same):>10s} {diff:21.3e}")
                lines.append(line)
                print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
