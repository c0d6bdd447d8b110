#!/usr/bin/env python3
"""What the device-side elastic deformation costs (GPU box only).

Default: the HIP-event median of 30 ``msg_elastic_deform`` calls after warm-up on the workload's own batch (B = 16, C = 2, T = 3,
256^2), fp32 and bf16 frames, at sigma = 16 / alpha = 80 (the class defaults) and sigma = 4 / alpha = 50, with the spread, and the
rate on the call's algorithmic bytes (noise read 8 + field write 8 + field read 8 per pixel, frames read and written once).
The same run times the reference's formulation in stock torch operators on the same inputs: per sample, as a ``Compose`` in the
dataset would call it, the dense (4 sigma + 1)^2 Gaussian built and applied with ``conv2d`` to the two noise planes, the grid,
one ``grid_sample`` (dataset/tlfm_dataset.py:230-275) -- looped over the batch.  The ratio stock / fused is printed.

``--step``: plain-iteration ms at 256^2, batch 16, bf16 storage, on a resident batch / the raw-count feed / the raw-count feed with
``elastic=ElasticDeformation()``, alternating A / B / C as tools/feed_probe.py --raw does; the elastic leg is reported against
the raw-feed leg and against the resident leg of the same run."""
import argparse
import math
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multi_stylegan_amd as m
from multi_stylegan_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--step", action="store_true", help="measure inside the training step (see the module docstring)")
args = ap.parse_args()
DEV = "cuda:0"
B, C, T, H, W = 16, 2, 3, 256, 256


def event_us(fn, calls=30, warmup=5):
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
    return statistics.median(times), min(times), max(times)


def stock_sample(img, noise, sigma, alpha):
    """One sample [F, H, W] the reference's way, in stock operators, on given noise planes [2, H, W]."""
    size = 4 * sigma + 1
    at = torch.arange(size, device=img.device, dtype=torch.float) - (size - 1) / 2.
    dense = torch.exp(-(at[:, None] ** 2 + at[None, :] ** 2) / (2. * sigma ** 2)) / (2. * math.pi * sigma ** 2)
    dx, dy = F.conv2d(noise[:, None], dense[None, None], padding=size // 2) * alpha
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float, device=img.device),
                            torch.arange(W, dtype=torch.float, device=img.device), indexing="ij")
    grid = torch.stack([2 * (xs + dx[0] - H // 2) / H, 2 * (ys + dy[0] - W // 2) / W], dim=-1)[None]
    return F.grid_sample(img[None], grid, mode="bilinear", padding_mode="border", align_corners=False)[0]


def call_probe():
    lib = _lib.lib()
    g = torch.Generator(device=DEV).manual_seed(1)
    frames32 = torch.rand((B, C * T, H, W), device=DEV, generator=g)
    noise = torch.rand((B, 2, H, W), device=DEV, generator=g) * 2 - 1
    field = torch.empty_like(noise)
    ws = torch.empty(lib.msg_elastic_workspace(B, H, W) // 4, device=DEV)
    stream = _lib.stream_of(frames32.device)
    for sigma, alpha in ((16, 80.0), (4, 50.0)):
        fused = {}
        for name, src in (("fp32", frames32), ("bf16", frames32.bfloat16())):
            out = torch.empty_like(src)

            def run():
                _lib.check(lib.msg_elastic_deform(src.data_ptr(), noise.data_ptr(), field.data_ptr(), out.data_ptr(),
                                                  _lib.dtype_code(src), B, C * T, H, W, sigma, alpha, ws.data_ptr(), stream),
                           "msg_elastic_deform")
            med, lo, hi = event_us(run)
            nbytes = B * H * W * 24 + 2 * src.numel() * src.element_size()
            fused[name] = (med, out)
            print(f"sigma {sigma} alpha {alpha:g} {name}: {med:.1f} us (min {lo:.1f}, max {hi:.1f}), {nbytes / 1e6:.1f} MB algorithmic "
                  f"-> {nbytes / med / 1e6:.2f} TB/s", flush=True)
        for name, src in (("fp32", frames32),):
            def stock():
                return torch.stack([stock_sample(src[b], noise[b], sigma, alpha) for b in range(B)])
            med, lo, hi = event_us(stock, calls=10, warmup=2)
            err = (stock() - fused[name][1]).abs().max().item()
            print(f"sigma {sigma} alpha {alpha:g} {name} stock conv2d + grid_sample per sample: {med:.1f} us (min {lo:.1f}, max {hi:.1f}) "
                  f"= {med / fused[name][0]:.1f} x the fused call; max |stock - fused| = {err:.1e}", flush=True)


def step_probe():
    from multi_stylegan_amd.config import generator_config_for_resolution
    from multi_stylegan_amd.data import TLFMDeviceFeed, prepare_tlfm_batch
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

    counts = torch.randint(0, 4000, (B, C, T, H, W), dtype=torch.int32).to(torch.uint16)
    hflip = (torch.rand(B) < 0.5).to(torch.uint8)
    resident = prepare_tlfm_batch(counts, hflip).to(DEV)
    elastic = m.ElasticDeformation(generator=torch.Generator(device=DEV).manual_seed(2))
    feeds = {"resident": lambda: [resident] * (n + 2),
             "raw feed": lambda: TLFMDeviceFeed([(counts, hflip)] * (n + 2), DEV),
             "raw feed + elastic": lambda: TLFMDeviceFeed([(counts, hflip)] * (n + 2), DEV, elastic=elastic)}
    timed(feeds["resident"]())
    runs = {name: [] for name in feeds}
    for _ in range(3):
        for name, make in feeds.items():
            runs[name].append(timed(make()))
    runs["resident"].append(timed(feeds["resident"]()))
    res, raw = statistics.median(runs["resident"]), statistics.median(runs["raw feed"])
    for name, values in runs.items():
        med = statistics.median(values)
        print(f"{name}: {med:.2f} ms/step ({' '.join(f'{v:.2f}' for v in values)}), {100 * (med / res - 1):+.2f} % of resident, "
              f"{100 * (med - raw) / res:+.2f} % of resident against the raw feed", flush=True)


if __name__ == "__main__":
    step_probe() if args.step else call_probe()
