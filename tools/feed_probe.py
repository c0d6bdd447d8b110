#!/usr/bin/env python3
"""Where the data feed's residual cost comes from (GPU box only): 256^2, batch 16 plain iterations fed (a) from a resident
batch, (b) through DevicePrefetcher from pageable host memory, (c) from page-locked host memory (no staging copy), (d) through
the prefetcher with batches that already live on the device (thread + queue only), (e) by `.to(device)` per step.

``--raw``: the raw-count feed instead (data.TLFMDeviceFeed over uint16 batches, normalised on the device by
msg_tlfm_prepare) -- the HIP-event time of the prepare call for fp32 and bf16 output, the H2D time of the batch as fp32 and as
counts, and plain-iteration ms on a resident batch / the prefetched fp32 feed / the raw feed, alternating A / B / C / A / B / C
as tests/test_hip_data.py::test_pageable_host_feed_does_not_slow_the_step does (each feed is judged against the resident leg
of the same run).

``--resident``: the resident dataset (resident.ResidentTLFMStore / ResidentTLFMFeed, msg_tlfm_gather), three parts in one run:
(c) FIRST, before this process touches the GPU (the DataLoader's workers are forks): the wall time of one epoch's data side
alone -- ``DataLoader(TFLMDatasetGAN(raw=True), batch_size=16, num_workers=w)`` at w = 0, 4, 16 over a synthetic tree the tool
writes (uncompressed 256^2 TIFFs, 4 traps x 40 time steps x 2 kinds = 320 frames, 152 samples) -- against the store's one-off
build from the same tree and one epoch of the resident feed; (a) the HIP-event time of msg_tlfm_gather against msg_tlfm_prepare
on the same B = 16, C = 2, T = 3, 256^2 batch, fp32 and bf16, the four legs alternating, medians; (b) plain-iteration ms on a
resident batch / the raw feed / the resident feed, alternating, each read against the resident-batch leg of the run."""
import argparse
import atexit
import os
import shutil
import statistics
import struct
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multi_stylegan_amd as m
from multi_stylegan_amd.config import generator_config_for_resolution
from multi_stylegan_amd.data import DevicePrefetcher, TLFMDeviceFeed, prepare_tlfm_batch

ap = argparse.ArgumentParser()
ap.add_argument("--raw", action="store_true", help="measure the raw-count feed (see the module docstring)")
ap.add_argument("--resident", action="store_true", help="measure the resident dataset (see the module docstring)")
args = ap.parse_args()


def write_tree(root, traps=4, steps=40, size=256):
    """Little-endian, uncompressed, single-strip 16-bit TIFFs named as the dataset expects (the trap number in the last field too:
    the dataset sorts by it first), bright field and GFP."""
    import numpy as np
    rng = np.random.default_rng(0)
    os.makedirs(os.path.join(root, "pos1"))
    for kind, top in (("BF0", 65536), ("GFP", 3000)):
        for trap in range(1, traps + 1):
            for step in range(steps):
                pixels = rng.integers(0, top, size=(size, size)).astype("<u2").tobytes()
                tags = [(256, 3, size), (257, 3, size), (258, 3, 16), (259, 3, 1), (262, 3, 1), (273, 4, 8), (277, 3, 1),
                        (278, 3, size), (279, 4, len(pixels))]
                ifd = struct.pack("<H", len(tags)) + b"".join(struct.pack("<HHII", t, k, 1, v) for t, k, v in tags) + struct.pack("<I", 0)
                with open(os.path.join(root, "pos1", f"pos1_t{step:03d}_x_trap{trap:04d}-{kind}_000_{trap:04d}.tif"), "wb") as f:
                    f.write(b"II" + struct.pack("<HI", 42, 8 + len(pixels)) + pixels + ifd)


host_side = {}
if args.resident:
    # (c), host part: nothing here opens the GPU, so the forked workers do not hold it either
    from torch.utils.data import DataLoader
    tree = tempfile.mkdtemp(prefix="msg-feed-probe-")
    atexit.register(shutil.rmtree, tree, True)
    write_tree(tree)
    dataset = m.TFLMDatasetGAN(tree, no_rfp=True, raw=True)
    for workers in (0, 4, 16):
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            batches = sum(1 for _ in DataLoader(dataset, batch_size=16, num_workers=workers, drop_last=True))
            walls.append(time.perf_counter() - t0)
        host_side[workers] = walls
        print(f"(c) DataLoader(TFLMDatasetGAN(raw=True), 16, num_workers={workers}): one epoch ({batches} batches of {len(dataset)} "
              f"samples, {6 * 16 * batches} TIFF decodes), data side alone: {1e3 * statistics.median(walls):.0f} ms "
              f"({' '.join(f'{1e3 * w:.0f}' for w in walls)})", flush=True)

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


if args.resident:
    pass                                                  # (below)
elif not args.raw:
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

if args.resident:
    from multi_stylegan_amd import ResidentTLFMFeed, ResidentTLFMStore, gather_tlfm_batch
    # (c), device part: the one-off build from the same tree (twice: the second finds the files in the page cache, as the
    # DataLoader legs above did), its saved form, and one epoch of the feed with nothing else on the stream
    for attempt in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = ResidentTLFMStore.from_dataset(dataset, DEV, workers=8)
        torch.cuda.synchronize()
        print(f"(c) ResidentTLFMStore.from_dataset (8 threads, {built.frames.shape[0]} files once, upload, ranges): "
              f"{1e3 * (time.perf_counter() - t0):.0f} ms", flush=True)
    built.save(os.path.join(tree, "store.npz"))
    t0 = time.perf_counter()
    ResidentTLFMStore.load(os.path.join(tree, "store.npz"), DEV)
    torch.cuda.synchronize()
    print(f"(c) ResidentTLFMStore.load of the saved store: {1e3 * (time.perf_counter() - t0):.0f} ms", flush=True)
    epoch_feed = ResidentTLFMFeed(built, 16)
    walls = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for batch in epoch_feed:
            pass
        torch.cuda.synchronize()
        walls.append(time.perf_counter() - t0)
    print(f"(c) ResidentTLFMFeed, one epoch ({len(epoch_feed)} batches), data side alone: {1e3 * statistics.median(walls):.2f} ms "
          f"({' '.join(f'{1e3 * w:.2f}' for w in walls)})", flush=True)

    # (a) the same batch through both entries
    g = torch.Generator().manual_seed(2)
    frames = torch.randint(0, 4000, (300, 256, 256), generator=g, dtype=torch.int32).to(torch.uint16)
    samples = torch.randint(0, 300, (16 * (n + 2), 2, 3), generator=g, dtype=torch.int32)
    store = ResidentTLFMStore.from_frames(frames, samples, device=DEV)
    hflip = (torch.rand(16, generator=g) < 0.5).to(torch.uint8)
    index = samples[:16]
    counts = torch.from_numpy(frames.numpy()[index.numpy()])                          # the stacked batch: pageable, as a DataLoader's
    counts_dev, hflip_dev, index_dev = counts.to(DEV), hflip.to(DEV), index.to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        assert torch.equal(gather_tlfm_batch(store.frames, store.ranges, index_dev, hflip_dev, out_dtype=dtype),
                           prepare_tlfm_batch(counts_dev, hflip_dev, out_dtype=dtype))
    legs = {"msg_tlfm_prepare fp32": lambda: prepare_tlfm_batch(counts_dev, hflip_dev),
            "msg_tlfm_gather fp32": lambda: gather_tlfm_batch(store.frames, store.ranges, index_dev, hflip_dev),
            "msg_tlfm_prepare bf16": lambda: prepare_tlfm_batch(counts_dev, hflip_dev, out_dtype=torch.bfloat16),
            "msg_tlfm_gather bf16": lambda: gather_tlfm_batch(store.frames, store.ranges, index_dev, hflip_dev, out_dtype=torch.bfloat16)}
    times = {name: [] for name in legs}
    for rnd in range(5):
        for name, fn in legs.items():
            times[name].append(event_us(fn))
    for name, values in times.items():
        print(f"(a) {name}: {statistics.median(values):.1f} us (medians of 30 over 5 alternating rounds: "
              f"{' '.join(f'{v:.1f}' for v in values)})", flush=True)
    tiny = ResidentTLFMStore.from_frames(frames[:6, :8, :8].contiguous(), torch.arange(6, dtype=torch.int32).view(1, 2, 3), device=DEV)
    print(f"(a) msg_tlfm_gather on one 8 x 8 frame per channel (one launch's floor under the same events): "
          f"{event_us(lambda: gather_tlfm_batch(tiny.frames, tiny.ranges, tiny.samples)):.1f} us", flush=True)

    # (b) the step on three feeds
    resident = prepare_tlfm_batch(counts_dev, hflip_dev)
    feeds = {"resident batch": lambda: [resident] * (n + 2),
             "raw feed": lambda: TLFMDeviceFeed([(counts, hflip)] * (n + 2), DEV),
             "resident feed": lambda: ResidentTLFMFeed(store, 16)}
    assert len(feeds["resident feed"]()) == n + 2
    timed(feeds["resident batch"]())
    runs = {name: [] for name in feeds}
    for rnd in range(3):
        for name, make in feeds.items():
            runs[name].append(timed(make()))
    runs["resident batch"].append(timed(feeds["resident batch"]()))
    res = statistics.median(runs["resident batch"])
    for name, values in runs.items():
        med = statistics.median(values)
        print(f"(b) {name}: {med:.2f} ms/step ({' '.join(f'{v:.2f}' for v in values)}), {100 * (med / res - 1):+.2f} % of the "
              f"resident batch", flush=True)
