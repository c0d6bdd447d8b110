#!/usr/bin/env python3
"""What the adversarial losses cost, fused kernel pair against stock-torch composite (GPU box only; DESIGN.md section 5,
"Adversarial losses").  Two steps, each a process of its own under its own time limit:

    timeout -k 10 300 python tools/loss_probe.py --step fp32 && timeout -k 10 300 python tools/loss_probe.py --step bf16

One "unit" is what a training iteration asks of the losses for one discriminator output: the discriminator pair on (real, fake)
predictions, forward and backward, plus the generator loss on fake predictions, forward and backward -- on the benchmark's
pixel-wise shape [16, 1, 256, 256] and on its scalar shape [16, 1].  Per shape, dtype and family (hinge, logistic) it reports

  * the HIP-event time of a unit, fused (op_static.gan_loss -> csrc/gan_loss.hip) and composite (the same formulas in stock
    torch operators: gan_loss.composite, which for the logistic family is what loss.NonSaturatingLogistic* do), alternating,
    ``calls`` units per event pair, the median / min / max of ``repeats`` pairs.  The events bracket the whole unit as the
    trainer runs it (autograd included), so at the scalar shape both numbers are launch- and host-bound;
  * the device kernels a unit launches, counted with torch.profiler in a pass of its own ("not measured" if the profiler
    yields no kernel events);
  * whether both give the same losses (to 1e-5).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from multi_stylegan_amd.op_static import gan_loss as op                     # noqa: E402

DEV = "cuda:0"
SHAPES = {"pixel_wise": (16, 1, 256, 256), "scalar": (16, 1)}


def unit(fn, real, fake, fake_g):
    """fn(pred_real, pred_fake) -> (loss_real, loss_fake): the discriminator pair and the generator loss, forward + backward."""
    real.grad = fake.grad = fake_g.grad = None
    l_real, l_fake = fn(real, fake)
    (l_real + l_fake).backward()
    l_gen = fn(fake_g, None)[0]
    l_gen.backward()
    return l_real.detach(), l_fake.detach(), l_gen.detach()


def event_us(fn, calls, repeats):
    for _ in range(max(10, calls // 4)):
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
    return [round(statistics.median(times), 2), round(min(times), 2), round(max(times), 2)]


def kernel_count(fn):
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(4):
                fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                 and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        return len(names) / 4 if names else "not measured"
    except Exception as exc:                                                 # the figure is optional, the timings are not
        return f"not measured ({type(exc).__name__})"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--step", choices=("fp32", "bf16"), required=True)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=None, help="write the JSON result here as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_probe measures on the GPU; there is none here")
    dtype = torch.float32 if args.step == "fp32" else torch.bfloat16
    result = {"dtype": args.step, "calls_per_pair": args.calls, "pairs": args.repeats, "rows": []}
    gen = torch.Generator(device=DEV).manual_seed(1)
    for shape_name, shape in SHAPES.items():
        leaves = [(torch.randn(shape, device=DEV, generator=gen) * 2).to(dtype).requires_grad_(True) for _ in range(3)]
        for kind in ("hinge", "logistic"):
            fused = lambda: unit(lambda r, f: op.gan_loss(r, f, kind=kind), *leaves)
            plain = lambda: unit(lambda r, f: op.composite(r, f, kind=kind), *leaves)
            a, b = fused(), plain()
            same = all(abs(u.item() - v.item()) <= 1e-5 * max(abs(v.item()), 1e-30) for u, v in zip(a, b))
            row = {"shape": shape_name, "dims": list(shape), "kind": kind, "same_losses": same, "fused_us": [], "composite_us": []}
            for _ in range(2):                                               # alternating: fused, composite, fused, composite
                row["fused_us"].append(event_us(fused, args.calls, args.repeats))
                row["composite_us"].append(event_us(plain, args.calls, args.repeats))
            row["fused_kernels_per_unit"], row["composite_kernels_per_unit"] = kernel_count(fused), kernel_count(plain)
            result["rows"].append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
