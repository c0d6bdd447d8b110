#!/usr/bin/env python3
"""Where the data feed's residual cost comes from (GPU box only): 256^2, batch 16 plain iterations fed (a) from a resident
batch, (b) through DevicePrefetcher from pageable host memory, (c) from page-locked host memory (no staging copy), (d) through
the prefetcher with batches that already live on the device (thread + queue only), (e) by `.to(device)` per step.

``--raw``: the raw-count feed instead (data.TLFMDeviceFeed over uint16 batches, normalised on the device by
msg_tlfm_prepare) -- the HIP-event time of the prepare call for fp32 and bf16 output, the H2D time of the batch as fp32 and as
counts, and plain-iteration ms on a resident batch / the prefetched fp32 feed / the raw feed, alternating A / B / C / A / B / C
as tests/test_hip_data.py::test_pageable_host_feed_does_not_slow_the_step does (each feed is judged against the resident leg
of the same run)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multi_stylegan_amd as m
from multi_stylegan_amd.config import generator_config_for_resolution
from multi_stylegan_amd.data import DevicePrefetcher, TLFMDeviceFeed, prepare_tlfm_batch

ap = argparse.ArgumentParser()
ap.add_argument("--raw", action="store_true", help="measure the raw-count feed (see the module docstring)")
args = ap.parse_args()

DEV = "cuda:0"
torch.manual_seed(1)
gen = m.MultiStyleGANGenerator(generator_config_for_resolution(256))
dis = m.MultiStyleGANDiscriminator(m.u_net_2d_discriminator_config, no_rfp=True)
gen.compute_dtype = dis.compute_dtype = torch.bfloat16
tr = m.ModelWrapper(gen, dis, device=DEV)
tr.generator_ema.compute_dtype = torch.bfloat16
n = 12


def timed(feed):
    tr.iteration = 16
    t0 = None
    for k, batch in enumerate(feed):
        if k == 2:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        tr.train_iteration(batch)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def event_us(fn, calls=30, warmup=5):
    """Median HIP-event time of one call, in microseconds."""
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b))
    return statistics.median(times)


if not args.raw:
    host = torch.rand(16, 2, 3, 256, 256)
    pinned = host.pin_memory()
    resident = host.to(DEV)
    feeds = {"resident": lambda: [resident] * (n + 2),
             "prefetch pageable": lambda: DevicePrefetcher([host] * (n + 2), DEV),
             "prefetch pinned": lambda: DevicePrefetcher([pinned] * (n + 2), DEV),
             "prefetch device (thread only)": lambda: DevicePrefetcher([resident] * (n + 2), DEV),
             ".to(device) per step": lambda: [host] * (n + 2)}
    timed(feeds["resident"]())
    for rnd in range(3):
        print("  ".join(f"{name}: {timed(make()):.2f}" for name, make in feeds.items()), flush=True)
else:
    counts = torch.randint(0, 4000, (16, 2, 3, 256, 256), dtype=torch.int32).to(torch.uint16)      # pageable, as a DataLoader's
    hflip = (torch.rand(16) < 0.5).to(torch.uint8)
    host = prepare_tlfm_batch(counts, hflip)                                                       # the fp32 form of the same batch
    resident = host.to(DEV)
    counts_dev, hflip_dev = counts.to(DEV), hflip.to(DEV)
    assert torch.equal(prepare_tlfm_batch(counts_dev, hflip_dev).cpu(), host)
    pixels = counts.numel()
    for dtype, name in ((torch.float32, "fp32"), (torch.bfloat16, "bf16")):
        us = event_us(lambda: prepare_tlfm_batch(counts_dev, hflip_dev, out_dtype=dtype))
        nbytes = pixels * (2 + (4 if dtype == torch.float32 else 2))
        print(f"msg_tlfm_prepare {name}: {us:.1f} us, {nbytes / 1e6:.1f} MB algorithmic -> {nbytes / us / 1e3:.0f} GB/s", flush=True)
    tiny, tiny_flip = counts_dev[:1, :, :1, :8, :8].contiguous(), hflip_dev[:1]
    print(f"msg_tlfm_prepare on one 8 x 8 frame per channel (the two launches' floor under the same events): "
          f"{event_us(lambda: prepare_tlfm_batch(tiny, tiny_flip)):.1f} us", flush=True)
    for name, src in (("fp32", host.pin_memory()), ("uint16", counts.pin_memory())):
        dst = torch.empty(src.shape, dtype=src.dtype, device=DEV)
        us = event_us(lambda: dst.copy_(src, non_blocking=True), calls=20)
        print(f"H2D {name} (page-locked, {src.numel() * src.element_size() / 1e6:.1f} MB): {us:.0f} us", flush=True)
    feeds = {"resident": lambda: [resident] * (n + 2),
             "prefetch fp32": lambda: DevicePrefetcher([host] * (n + 2), DEV),
             "raw feed": lambda: TLFMDeviceFeed([(counts, hflip)] * (n + 2), DEV)}
    timed(feeds["resident"]())
    runs = {name: [] for name in feeds}
    for rnd in range(3):
        for name, make in feeds.items():
            runs[name].append(timed(make()))
    runs["resident"].append(timed(feeds["resident"]()))
    res = statistics.median(runs["resident"])
    for name, values in runs.items():
        med = statistics.median(values)
        print(f"{name}: {med:.2f} ms/step ({' '.join(f'{v:.2f}' for v in values)}), {100 * (med / res - 1):+.2f} % of resident",
              flush=True)
