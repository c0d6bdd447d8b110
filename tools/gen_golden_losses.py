#!/usr/bin/env python3
"""Generate tests/golden/losses.npz (+ losses.json, its manifest) by running the REFERENCE's own loss modules
(multi_stylegan/loss.py:9-280) on the CPU: the three families (non-saturating logistic, Wasserstein, hinge), each as the
discriminator pair, the generator loss and the CutMix pair, with and without a weight map.

Runs only in the build container (needs /root/reference; its loss.py is loaded with importlib and imports nothing but torch).
The fixture is plain data -- predictions, weight and label maps, and what the reference's modules return for them -- and nothing
of the reference travels with it.

Cases (real / fake predictions; n_real != n_fake in each):
  s   [5, 1] / [3, 1]                  no weight map (a [B, 1] prediction has no H x W); label [5, 1]
  m   [2, 1, 3, 8, 8] / [3, 1, 3, 8, 8]    weight [8, 8]; label like real
  l   [3, 1, 37, 41] / [1, 1, 37, 41]      weight [37, 41]; label like real
Every prediction is exactly representable in bfloat16, so that one fixture serves the fp32 and the bf16 kernels: case s holds
the hinge's ties and the softplus extremes (1, -1, 90, -90, ...), cases m and l are multiples of 1/2 in [-3, 3] -- one value in
13, so that x == 1 and x == -1 are each hit about 77 times per thousand elements -- with +-90 planted in them; weights are
multiples of 1/2 in [0.5, 2], labels 0 / 1 rectangles with both values present.  (Few distinct values keep the compressed
file small; the sums still run over full-mantissa terms.)

Per case, family in (logistic, wasserstein, hinge), form and precision p in (f32, f64: the same inputs as float64), the results
are named
  <case>.<family>.disc.<none|weight>.<p>.loss        [2]  (loss_real, loss_fake) of <Family>DiscriminatorLoss(real, fake[, weight])
  <case>.<family>.disc.<none|weight>.<p>.absmean     [2]  mean |a_i r(x_i)|, mean |a'_i f(x_i)|: the scale of the tolerances
  <case>.<family>.disc.<none|weight>.<p>.grad_real / .grad_fake   d (0.7 loss_real - 1.3 loss_fake) / d prediction
  <case>.<family>.cutmix.label.<p>.loss / .absmean / .grad_real    <Family>DiscriminatorLossCutMix(real, label), same cotangents
  <case>.<family>.gen.<none|weight>.<p>.loss [1] / .absmean [1] / .grad_real   <Family>GeneratorLoss(fake[, weight]), d (0.7 loss)
(the generator form's "real" operand is the case's FAKE prediction tensor.)  absmean comes from the reference's modules as
well: the logistic and hinge terms are non-negative (weights and labels are), so it is the loss itself; the Wasserstein one is
the Wasserstein loss of |x|.  Case l's gradients are recorded from the float64 run only (the file's size: the fp32 ones differ
from them by fp32 rounding, which is what the tests allow).

In the file they are packed (an .npz member costs ~250 bytes whatever it holds): ``scalars.<p>`` [rows, 4] = (loss_real,
loss_fake, absmean_real, absmean_fake), zeros where a form has no fake side, rows named by the manifest's ``rows``; and
``grads.<case>.<p>``, flat, cut by the manifest's ``grads`` = {"<case>.<p>": [[name, offset, shape], ...]}.
tests/losses_util.py unpacks them into the names above.

Usage: python tools/gen_golden_losses.py [--check-only]
"""
import argparse
import importlib.util
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LOSS = "/root/reference/multi_stylegan/loss.py"
OUT = os.path.join(ROOT, "tests", "golden")
COTANGENTS = (0.7, -1.3)
FAMILIES = {"logistic": ("NonSaturatingLogisticDiscriminatorLoss", "NonSaturatingLogisticDiscriminatorLossCutMix",
                         "NonSaturatingLogisticGeneratorLoss"),
            "wasserstein": ("WassersteinDiscriminatorLoss", "WassersteinDiscriminatorLossCutMix", "WassersteinGeneratorLoss"),
            "hinge": ("HingeDiscriminatorLoss", "HingeDiscriminatorLossCutMix", "HingeGeneratorLoss")}
SHAPES = {"s": ((5, 1), (3, 1)), "m": ((2, 1, 3, 8, 8), (3, 1, 3, 8, 8)), "l": ((3, 1, 37, 41), (1, 1, 37, 41))}


def reference_loss():
    spec = importlib.util.spec_from_file_location("reference_loss", REF_LOSS)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def inputs():
    g = torch.Generator().manual_seed(20)
    arrays = {"s.real": torch.tensor([1.0, -1.0, 90.0, 0.375, -2.5]).reshape(5, 1),
              "s.fake": torch.tensor([-1.0, -90.0, 1.0]).reshape(3, 1),
              "s.label": torch.tensor([1.0, 0.0, 0.0, 1.0, 1.0]).reshape(5, 1)}
    for case in ("m", "l"):
        real_shape, fake_shape = SHAPES[case]
        for name, shape in (("real", real_shape), ("fake", fake_shape)):
            x = torch.randint(-6, 7, shape, generator=g).float() / 2.0
            flat = x.reshape(-1)
            flat[3], flat[-2] = 90.0, -90.0
            flat[5], flat[6] = 1.0, -1.0                                     # ties, whatever the draw gave
            arrays[f"{case}.{name}"] = x
        h, w = real_shape[-2:]
        arrays[f"{case}.weight"] = torch.randint(1, 5, (h, w), generator=g).float() / 2.0
        label = torch.zeros(real_shape)
        label[..., h // 4: h // 4 + h // 2, w // 3:] = 1.0
        label[0] = 1.0 - label[0]                                            # (not the same map in every sample)
        arrays[f"{case}.label"] = label
    for k, v in arrays.items():
        assert torch.equal(v, v.bfloat16().float()), k
    return arrays


def record(arrays, key, losses, leaves, absmean):
    losses = losses if isinstance(losses, tuple) else (losses,)
    sum(c * v for c, v in zip(COTANGENTS, losses)).backward()
    arrays[key + ".loss"] = torch.stack([v.detach() for v in losses]).numpy()
    arrays[key + ".absmean"] = torch.stack([v.detach().abs() for v in (absmean if isinstance(absmean, tuple) else (absmean,))]).numpy()
    for name, leaf in leaves.items():
        arrays[f"{key}.{name}"] = leaf.grad.numpy()


def pack(flat):
    packed = {k: v for k, v in flat.items() if k.count(".") == 1}
    rows = sorted({k.rsplit(".", 2)[0] for k in flat if k.endswith(".loss")})
    grads = {}
    for prec, dtype in (("f32", np.float32), ("f64", np.float64)):
        table = np.zeros((len(rows), 4), dtype=dtype)
        for i, row in enumerate(rows):
            loss, scale = flat[f"{row}.{prec}.loss"], flat[f"{row}.{prec}.absmean"]
            table[i, :len(loss)], table[i, 2:2 + len(scale)] = loss, scale
        packed[f"scalars.{prec}"] = table
        for case in SHAPES:
            if case == "l" and prec == "f32":
                continue
            names = sorted(k for k in flat if k.startswith(case + ".") and f".{prec}.grad_" in k)
            offset, index = 0, []
            for k in names:
                index.append([k, offset, list(flat[k].shape)])
                offset += flat[k].size
            packed[f"grads.{case}.{prec}"] = np.concatenate([flat[k].reshape(-1) for k in names])
            grads[f"{case}.{prec}"] = index
    return packed, {"rows": rows, "grads": grads}


def generate():
    ref = reference_loss()
    data = inputs()
    arrays = {k: v.numpy() for k, v in data.items()}
    for case in SHAPES:
        for family, (disc_name, cutmix_name, gen_name) in FAMILIES.items():
            disc, cutmix, gen = getattr(ref, disc_name)(), getattr(ref, cutmix_name)(), getattr(ref, gen_name)()
            # mean |term|: the Wasserstein modules applied to |x|; the other families' terms are non-negative
            w_disc, w_cutmix, w_gen = (getattr(ref, n)() for n in FAMILIES["wasserstein"])
            for prec, dtype in (("f32", torch.float32), ("f64", torch.float64)):
                def leaf(name):
                    return data[f"{case}.{name}"].clone().to(dtype).requires_grad_(True)
                label = data[f"{case}.label"].to(dtype)
                for aux in ("none", "weight"):
                    if aux == "weight" and f"{case}.weight" not in data:
                        continue
                    kw = {"weight": data[f"{case}.weight"].to(dtype)} if aux == "weight" else {}
                    real, fake = leaf("real"), leaf("fake")
                    out = disc(real, fake, **kw)
                    scale = w_disc(-real.detach().abs(), fake.detach().abs(), **kw) if family == "wasserstein" else \
                        tuple(v.detach() for v in out)
                    record(arrays, f"{case}.{family}.disc.{aux}.{prec}", out, {"grad_real": real, "grad_fake": fake}, scale)
                    fake = leaf("fake")
                    out = gen(fake, **kw)
                    scale = w_gen(-fake.detach().abs(), **kw) if family == "wasserstein" else out.detach()
                    record(arrays, f"{case}.{family}.gen.{aux}.{prec}", out, {"grad_real": fake}, scale)
                real = leaf("real")
                out = cutmix(real, label)
                scale = w_cutmix(-real.detach().abs(), label)[0], w_cutmix(real.detach().abs(), label)[1]
                record(arrays, f"{case}.{family}.cutmix.label.{prec}", out, {"grad_real": real},
                       scale if family == "wasserstein" else tuple(v.detach() for v in out))
    arrays, layout = pack(arrays)
    manifest = {"rows": layout["rows"], "grads": layout["grads"], "generator": "tools/gen_golden_losses.py", "cotangents": list(COTANGENTS), "families": sorted(FAMILIES),
                "cases": {c: {"real": list(r), "fake": list(f), "weight": f"{c}.weight" in data} for c, (r, f) in SHAPES.items()},
                "keys": "<case>.<family>.<disc|gen|cutmix>.<none|weight|label>.<f32|f64>.<loss|absmean|grad_real|grad_fake>"}
    return arrays, manifest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true", help="regenerate and compare with the committed fixture, write nothing")
    args = ap.parse_args()
    arrays, manifest = generate()
    npz, man = os.path.join(OUT, "losses.npz"), os.path.join(OUT, "losses.json")
    if args.check_only:
        have = np.load(npz)
        assert sorted(have.files) == sorted(arrays), "the fixture's keys differ"
        assert all(np.array_equal(have[k], arrays[k], equal_nan=True) for k in arrays), "the fixture's arrays differ"
        assert json.load(open(man)) == manifest, "the manifest differs"
        print("tests/golden/losses.npz agrees with the reference (nothing written)")
        return
    np.savez_compressed(npz, **arrays)
    with open(man, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {npz} ({os.path.getsize(npz)} bytes, {len(arrays)} arrays) and {man}")


if __name__ == "__main__":
    main()
