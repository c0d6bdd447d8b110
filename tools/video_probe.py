#!/usr/bin/env python3
"""What the interpolation video costs against the PNG frames it replaces (GPU box only; DESIGN.md section 5, "Interpolation
video").  One process under its own time limit:

    timeout -k 10 900 python tools/video_probe.py --bf16

On a randomly initialised full-size generator, for the reference's 1600 frames of 512 x 768 (16 anchors x 100 steps, batch 32):
wall time of ``interpolation_frames`` (its own ``SheetWriter``, four workers) and of ``interpolation_video``, alternating,
``--rounds`` times, around a device synchronise, into a temporary directory; the bytes copied to the host per frame against
the 1 179 648 of RGB; the file size; and the device time of ``msg_jpeg_encode`` for one batch of 32 such frames (HIP events,
``--calls`` launches per pair, the median of ``--repeats`` pairs).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multi_stylegan_amd as m
from multi_stylegan_amd import video
from multi_stylegan_amd.config import generator_config_for_resolution

DEV = "cuda:0"


class _Recording(video.MjpegWriter):
    """The writer ``interpolation_video`` makes for itself, kept so that its counters can be read afterwards."""
    last = None

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        _Recording.last = self


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--anchors", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--bf16", action="store_true", help="bf16 compute in the generator (the benchmark's setting)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("video_probe measures on the GPU; there is none here")
    torch.manual_seed(1)
    generator = m.MultiStyleGANGenerator(generator_config_for_resolution(args.resolution)).to(DEV)
    if args.bf16:
        generator.compute_dtype = torch.bfloat16
    anchors = torch.randn(args.anchors, generator.latent_dimensions, generator=torch.Generator().manual_seed(2))
    video.MjpegWriter = _Recording
    result = {"resolution": args.resolution, "frames": args.anchors * args.steps, "batch": args.batch, "quality": args.quality,
              "compute_dtype": "bf16" if args.bf16 else "fp32", "legs": []}

    def frames_leg(directory):
        return m.interpolation_frames(generator, directory, anchors=anchors, steps_per_anchor=args.steps, batch_size=args.batch)

    def video_leg(directory):
        return video.interpolation_video(generator, os.path.join(directory, "video.avi"), anchors=anchors,
                                         steps_per_anchor=args.steps, batch_size=args.batch, quality=args.quality)

    with tempfile.TemporaryDirectory() as warm:                              # capture, code objects, weight images, pinned memory
        frames_leg(warm)
        video_leg(warm)
    for _ in range(args.rounds):
        for name, leg in (("interpolation_frames", frames_leg), ("interpolation_video", video_leg)):
            with tempfile.TemporaryDirectory() as directory:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                frames = leg(directory)
                torch.cuda.synchronize()
                seconds = time.perf_counter() - t0
                files = os.listdir(directory)
                size = sum(os.path.getsize(os.path.join(directory, f)) for f in files)
            row = {"leg": name, "frames": frames, "files": len(files), "seconds": round(seconds, 3), "bytes_written": size}
            if name == "interpolation_video":
                row["bytes_copied_per_frame"] = round(_Recording.last.bytes_copied / frames)
                row["rgb_bytes_per_frame"] = 3 * _Recording.last.size[0] * _Recording.last.size[1]
            result["legs"].append(row)
            print(json.dumps(row), flush=True)

    sampler = m.GeneratorSampler(generator, batch_size=args.batch, randomize_noise=False, device=DEV)
    sheets = m.sample_sheets(sampler(torch.randn(args.batch, generator.latent_dimensions, device=DEV)))
    B, C, H, TW, _ = sheets.shape
    pictures = sheets.reshape(B, C * H, TW, 3)
    tables = video.jpeg_tables(args.quality)
    for _ in range(3):
        video._encode_device(pictures, tables)
    times = []
    for _ in range(args.repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            video._encode_device(pictures, tables)
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b) / args.calls)
    _, offsets, _ = video._encode_device(pictures, tables)
    result["encode"] = {"shape": list(pictures.shape), "us_median_min_max": [statistics.median(times), min(times), max(times)],
                        "payload_bytes": int(offsets[-1])}
    print(json.dumps(result["encode"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
