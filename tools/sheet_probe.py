#!/usr/bin/env python3
"""What the sample output costs (GPU box only; DESIGN.md section 5, "Sample sheets").  Two steps, each a process of its own
under its own time limit:

    timeout -k 10 300 python tools/sheet_probe.py --step kernel && timeout -k 10 900 python tools/sheet_probe.py --step frames

``--step kernel``: HIP-event time of ``msg_sample_sheet`` at [32, 2, 3, 256, 256], fp32 and bf16 input (the C entry into a
preallocated output, and ``sample_sheets`` with its allocation and checks), against the reference's
composition in stock torch operators on the device (repeat_interleave, the zero fills, cat, mul / add / clamp, permute,
to(uint8): misc.py:138-166 and save_image's quantisation), alternating; ``calls`` launches per event pair, the median of
``repeats`` pairs; the kernel's share of HBM bandwidth for its algorithmic bytes (sizeof(dtype) + 3) * B * C * T * H * W; and
whether the two compositions give the same bytes.

``--step frames``: the 1600-frame interpolation at 256^2 (16 anchors x 100 steps, batch 32) from a randomly initialised
generator: the generator and the composition alone (nothing copied or written), ``SheetWriter(workers=4)`` and
``SheetWriter(workers=0)``, in that order, ``--rounds`` times; wall clock around a device synchronise, files in a temporary
directory.  Also the encode time of one frame on one thread.
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
from multi_stylegan_amd import _lib
from multi_stylegan_amd.config import generator_config_for_resolution

DEV = "cuda:0"
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12                   # bytes / s: specification, measured float4 copy


def torch_compose(x):
    """The reference's chain for a whole batch on the device -> uint8 [B, C, H, T*W, 3]."""
    B, C, T, H, W = x.shape
    sheets = []
    for c in range(C):
        images = x[:, c].unsqueeze(2).repeat_interleave(3, dim=2)            # [B, T, 3, H, W]
        if c == 1:
            images[:, :, 0] = 0.0
            images[:, :, 2] = 0.0
        if c == 2:
            images[:, :, 1] = 0.0
            images[:, :, 2] = 0.0
        sheets.append(torch.cat(list(images.unbind(1)), dim=-1))             # nrow = T, padding = 0: [B, 3, H, T*W]
    grid = torch.stack(sheets, dim=1).float()
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(0, 1, 3, 4, 2).to(torch.uint8).contiguous()


def event_us(fn, calls, repeats, warmup=3):
    for _ in range(warmup * calls // 4 + 1):
        fn()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        times.append(1e3 * a.elapsed_time(b) / calls)
    return statistics.median(times), min(times), max(times)


def step_kernel(args):
    shape = (32, 2, 3, 256, 256)
    result = {"shape": shape, "calls_per_pair": args.calls, "pairs": args.repeats}
    base = torch.rand(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 1.2 - 0.1
    for dtype in (torch.float32, torch.bfloat16):
        x = base.to(dtype)
        same = torch.equal(m.sample_sheets(x), torch_compose(x))
        rows = {"entry": [], "op": [], "torch": []}
        out = torch.empty(shape[0], shape[1], shape[3], shape[2] * shape[4], 3, dtype=torch.uint8, device=DEV)
        lib, code, stream = _lib.lib(), _lib.dtype_code(x), _lib.stream_of(x.device)

        def entry():                                                         # the C entry alone: no allocation, no checks
            lib.msg_sample_sheet(x.data_ptr(), out.data_ptr(), code, *shape, 7 | 2 << 3, stream)
        for _ in range(2):                                                   # alternating: entry, op, torch, entry, op, torch
            rows["entry"].append(event_us(entry, args.calls, args.repeats))
            rows["op"].append(event_us(lambda: m.sample_sheets(x), args.calls, args.repeats))
            rows["torch"].append(event_us(lambda: torch_compose(x), max(1, args.calls // 10), args.repeats))
        nbytes = (x.element_size() + 3) * x.numel()
        best = min(r[0] for r in rows["entry"])
        result[str(dtype)] = {"same_bytes_as_torch_ops": same, "algorithmic_bytes": nbytes,
                              "entry_us_median_min_max": rows["entry"], "sample_sheets_us_median_min_max": rows["op"],
                              "torch_ops_us_median_min_max": rows["torch"],
                              "kernel_TBps": nbytes / (best * 1e-6) / 1e12,
                              "share_of_8.0TBps_spec": nbytes / (best * 1e-6) / HBM_SPEC,
                              "share_of_6.29TBps_copy": nbytes / (best * 1e-6) / HBM_COPY}
        print(json.dumps({str(dtype): result[str(dtype)]}), flush=True)
    return result


class _NoWriter:
    """The generator-only leg: the sheets are composed and dropped."""
    written = 0

    def submit(self, names, sheets):
        pass


def step_frames(args):
    torch.manual_seed(1)
    generator = m.MultiStyleGANGenerator(generator_config_for_resolution(args.resolution)).to(DEV)
    if args.bf16:
        generator.compute_dtype = torch.bfloat16
    anchors = torch.randn(args.anchors, generator.latent_dimensions, generator=torch.Generator().manual_seed(2))

    def leg(workers, directory):
        writer = _NoWriter() if workers is None else m.SheetWriter(directory, workers=workers, compress_level=args.level)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frames = m.interpolation_frames(generator, directory, anchors=anchors, steps_per_anchor=args.steps,
                                        batch_size=args.batch, writer=writer)
        if workers is not None:
            writer.close()
        torch.cuda.synchronize()
        return frames, time.perf_counter() - t0

    result = {"resolution": args.resolution, "frames": args.anchors * args.steps, "batch": args.batch,
              "compute_dtype": "bf16" if args.bf16 else "fp32", "compress_level": args.level, "legs": []}
    with tempfile.TemporaryDirectory() as warm:
        leg(None, warm)                                                      # capture, code objects, weight images
    for _ in range(args.rounds):
        for name, workers in (("generator only", None), ("workers=4", 4), ("workers=0", 0)):
            with tempfile.TemporaryDirectory() as directory:
                frames, seconds = leg(workers, directory)
                files = len(os.listdir(directory))
                size = sum(os.path.getsize(os.path.join(directory, f)) for f in os.listdir(directory))
            row = {"leg": name, "frames": frames, "files": files, "seconds": round(seconds, 3), "MB_written": round(size / 1e6, 1)}
            result["legs"].append(row)
            print(json.dumps(row), flush=True)
    sampler = m.GeneratorSampler(generator, batch_size=args.batch, randomize_noise=False, device=DEV)
    one = m.sample_sheets(sampler(torch.randn(args.batch, generator.latent_dimensions, device=DEV)))
    pixels = one.reshape(args.batch, -1, one.shape[3], 3).cpu().numpy()
    with tempfile.TemporaryDirectory() as directory:
        t0 = time.perf_counter()
        for k in range(args.batch):
            m.write_png(os.path.join(directory, f"{k}.png"), pixels[k], args.level)
        result["encode_ms_per_frame_one_thread"] = round((time.perf_counter() - t0) / args.batch * 1e3, 2)
    print(json.dumps({"encode_ms_per_frame_one_thread": result["encode_ms_per_frame_one_thread"]}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("kernel", "frames"), required=True)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--anchors", type=int, default=16)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--level", type=int, default=3, help="zlib level of the PNG writer")
    ap.add_argument("--bf16", action="store_true", help="bf16 compute in the generator (the benchmark's setting)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sheet_probe measures on the GPU; there is none here")
    result = step_kernel(args) if args.step == "kernel" else step_frames(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
