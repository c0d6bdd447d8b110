#!/usr/bin/env python3
"""What a simulated dataset costs (GPU box only; DESIGN.md section 5, "Simulated datasets").  Two steps, each a process of its own
under its own time limit:

    timeout -k 10 300 python tools/simulate_probe.py --step kernel && timeout -k 10 900 python tools/simulate_probe.py --step dataset

``--step kernel``: HIP-event time of ``msg_tlfm_export`` at [16, 2, 3, 256, 256], fp32 and bf16 input (the C entry into a
preallocated output, and ``export_tlfm_batch`` with its allocation, range upload and checks), against the same definition in
stock torch operators on the device (isnan / where / amin / amax, subtract, divide, multiply, add, round, nan_to_num, clamp,
flip, to(uint16)), alternating; ``calls`` launches per event pair, the median of ``repeats`` pairs; the kernels' share of HBM
bandwidth for their algorithmic bytes (the bright field is read twice: sizeof(dtype) * (1 + 1 / C) + 2 per pixel); and whether
the two give the same counts.

``--step dataset``: ``simulate_dataset`` end to end for ``--samples`` sequences at 256^2 (batch 16) from a randomly initialised
generator: the generator and the export alone (nothing copied or written), ``TLFMDatasetWriter(workers=4)`` and
``TLFMDatasetWriter(workers=0)``, in that order, ``--rounds`` times; wall clock around a device synchronise, files in a temporary
directory.  Also the time to read the written dataset back through ``TFLMDatasetGAN(raw=True)`` on one thread.
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
GFP, RFP = (150.0, 2200.0), (20.0, 2000.0)


def torch_export(x, ranges):
    """The definition of export_tlfm_batch in stock torch operators on the device -> uint16 [B, C, T, H, W]."""
    x = x.float()
    B, C, T, H, W = x.shape
    v = torch.empty_like(x)
    offset = ranges[..., 0].float().view(B, T, 1, 1)
    scale = (ranges[..., 1] - ranges[..., 0]).float().view(B, T, 1, 1)
    bf = x[:, 0]
    nan = bf.isnan()
    lo = torch.where(nan, float("inf"), bf).flatten(start_dim=2).amin(dim=2).view(B, T, 1, 1)
    hi = torch.where(nan, float("-inf"), bf).flatten(start_dim=2).amax(dim=2).view(B, T, 1, 1)
    n = torch.where(hi == lo, torch.where(nan, bf, 0.0), (bf - lo) / (hi - lo))
    v[:, 0] = (n * scale) + offset
    for c, (low, div) in zip(range(1, C), (GFP, RFP)):
        v[:, c] = (x[:, c].clamp(0.0, 1.0) * div) + low
    return v.flip(dims=(-2,)).round().nan_to_num(nan=0.0, posinf=65535.0, neginf=0.0).clamp(0.0, 65535.0).to(torch.int32).to(torch.uint16)


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
    shape = (16, 2, 3, 256, 256)
    B, C, T, H, W = shape
    result = {"shape": shape, "calls_per_pair": args.calls, "pairs": args.repeats}
    base = torch.rand(shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 1.2 - 0.1
    ranges = torch.tensor([300, 41000], dtype=torch.int32, device=DEV).expand(B, T, 2).contiguous()
    for dtype in (torch.float32, torch.bfloat16):
        x = base.to(dtype)
        same = bool((m.export_tlfm_batch(x, ranges).cpu().view(torch.int16) == torch_export(x, ranges).cpu().view(torch.int16)).all())
        rows = {"entry": [], "op": [], "torch": []}
        out = torch.empty(shape, dtype=torch.uint16, device=DEV)
        lib, code, stream = _lib.lib(), _lib.dtype_code(x), _lib.stream_of(x.device)
        ws = _lib.scratch_ptr(lib.msg_tlfm_export_workspace(B, T), x.device)

        def entry():                                                         # the C entry alone: no allocation, no checks
            lib.msg_tlfm_export(x.data_ptr(), code, ranges.data_ptr(), out.data_ptr(), *shape, 1, 1, *GFP, *RFP, ws, stream)
        for _ in range(2):                                                   # alternating: entry, op, torch, entry, op, torch
            rows["entry"].append(event_us(entry, args.calls, args.repeats))
            rows["op"].append(event_us(lambda: m.export_tlfm_batch(x, (300, 41000)), args.calls, args.repeats))
            rows["torch"].append(event_us(lambda: torch_export(x, ranges), max(1, args.calls // 10), args.repeats))
        nbytes = (x.element_size() * (1.0 + 1.0 / C) + 2) * x.numel()
        best = min(r[0] for r in rows["entry"])
        result[str(dtype)] = {"same_counts_as_torch_ops": same, "algorithmic_bytes": nbytes,
                              "entry_us_median_min_max": rows["entry"], "export_tlfm_batch_us_median_min_max": rows["op"],
                              "torch_ops_us_median_min_max": rows["torch"],
                              "kernels_TBps": nbytes / (best * 1e-6) / 1e12,
                              "share_of_8.0TBps_spec": nbytes / (best * 1e-6) / HBM_SPEC,
                              "share_of_6.29TBps_copy": nbytes / (best * 1e-6) / HBM_COPY}
        print(json.dumps({str(dtype): result[str(dtype)]}), flush=True)
    return result


class _NoWriter:
    """The generator-and-export leg: the counts are made and dropped."""
    position_prefix, traps_per_position = "none", 0

    def submit(self, counts):
        pass


def step_dataset(args):
    torch.manual_seed(1)
    generator = m.MultiStyleGANGenerator(generator_config_for_resolution(args.resolution)).to(DEV)
    if args.bf16:
        generator.compute_dtype = torch.bfloat16

    def leg(workers, directory):
        writer = _NoWriter() if workers is None else m.TLFMDatasetWriter(directory, workers=workers)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        count = m.simulate_dataset(generator, args.samples, directory, batch_size=args.batch, bf_range=(300, 41000), seed=3,
                                   writer=writer)
        if workers is not None:
            writer.close()
        torch.cuda.synchronize()
        return count, time.perf_counter() - t0

    result = {"resolution": args.resolution, "sequences": args.samples, "batch": args.batch,
              "compute_dtype": "bf16" if args.bf16 else "fp32", "legs": []}
    with tempfile.TemporaryDirectory(prefix="simprobe") as warm:
        leg(None, warm)                                                      # capture, code objects, weight images
    read_back = None
    for _ in range(args.rounds):
        for name, workers in (("generator and export only", None), ("workers=4", 4), ("workers=0", 0)):
            with tempfile.TemporaryDirectory(prefix="simprobe") as directory:
                count, seconds = leg(workers, directory)
                files = sum(len(f) for _, _, f in os.walk(directory)) - 1     # (simulation.json)
                size = sum(os.path.getsize(os.path.join(r, n)) for r, _, f in os.walk(directory) for n in f)
                if workers == 4 and read_back is None:
                    t0 = time.perf_counter()
                    dataset = m.TFLMDatasetGAN(directory, sequence_length=3, no_rfp=True, raw=True)
                    for k in range(len(dataset)):
                        dataset[k]
                    read_back = {"samples": len(dataset), "seconds": round(time.perf_counter() - t0, 3)}
            row = {"leg": name, "sequences": count, "files": files, "seconds": round(seconds, 3), "MB_written": round(size / 1e6, 1),
                   "sequences_per_second": round(count / seconds, 1)}
            result["legs"].append(row)
            print(json.dumps(row), flush=True)
    result["read_back_one_thread"] = read_back
    print(json.dumps({"read_back_one_thread": read_back}), flush=True)
    return result


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("kernel", "dataset"), required=True)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--resolution", type=int, default=256)
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--bf16", action="store_true", help="bf16 compute in the generator (the benchmark's setting)")
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("simulate_probe measures on the GPU; there is none here")
    result = step_kernel(args) if args.step == "kernel" else step_dataset(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
