"""Shared by tests/test_losses.py and tests/test_hip_losses.py: tests/golden/losses.npz unpacked into the names
tools/gen_golden_losses.py documents, the float64 composite the ragged GPU cases are compared with, and the comparisons."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAMILIES = ("logistic", "wasserstein", "hinge")
CLASSES = {"logistic": ("NonSaturatingLogisticDiscriminatorLoss", "NonSaturatingLogisticDiscriminatorLossCutMix",
                        "NonSaturatingLogisticGeneratorLoss"),
           "wasserstein": ("WassersteinDiscriminatorLoss", "WassersteinDiscriminatorLossCutMix", "WassersteinGeneratorLoss"),
           "hinge": ("HingeDiscriminatorLoss", "HingeDiscriminatorLossCutMix", "HingeGeneratorLoss")}
FLT_MIN = 2.0 ** -126         # below it fp32 has no full mantissa and exponentials flush: the floor of every relative comparison
_CACHE = {}


def fixtures():
    """-> (dict of torch tensors under the documented names, manifest).  Loaded once, never written to."""
    if not _CACHE:
        z = np.load(os.path.join(GOLDEN, "losses.npz"))
        man = json.load(open(os.path.join(GOLDEN, "losses.json")))
        out = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith(("scalars.", "grads."))}
        for prec in ("f32", "f64"):
            table = torch.from_numpy(z[f"scalars.{prec}"])
            for i, row in enumerate(man["rows"]):
                width = 1 if ".gen." in row else 2
                out[f"{row}.{prec}.loss"], out[f"{row}.{prec}.absmean"] = table[i, :width], table[i, 2:2 + width]
        for key, index in man["grads"].items():
            flat = torch.from_numpy(z["grads." + key])
            for name, offset, shape in index:
                out[name] = flat[offset:offset + int(np.prod(shape))].reshape(shape)
        _CACHE["data"], _CACHE["manifest"] = out, man
    return _CACHE["data"], _CACHE["manifest"]


def forms(case, manifest):
    """Every (form, aux) the fixture records for a case."""
    out = [("disc", "none"), ("gen", "none"), ("cutmix", "label")]
    if manifest["cases"][case]["weight"]:
        out += [("disc", "weight"), ("gen", "weight")]
    return out


def operands(data, case, form, aux):
    """-> (pred_real, pred_fake, weight, label) of a recorded form, fp32 CPU tensors (absent: None)."""
    weight = data[f"{case}.weight"] if aux == "weight" else None
    if form == "disc":
        return data[f"{case}.real"], data[f"{case}.fake"], weight, None
    if form == "gen":
        return data[f"{case}.fake"], None, weight, None
    return data[f"{case}.real"], None, None, data[f"{case}.label"]


def composite64(pred_real, pred_fake, kind, weight=None, label=None, cotangents=(0.7, -1.3)):
    """The formulas in float64 on the CPU (from whatever dtype / device the operands have: a bf16 prediction is taken at its
    rounded value) -> dict(loss [2], absmean [2], grad_real, grad_fake)."""
    def term(x, fake):
        if kind == "logistic":
            return torch.nn.functional.softplus(x if fake else -x)
        if kind == "wasserstein":
            return x if fake else -x
        return -torch.minimum(torch.zeros((), dtype=torch.float64), (-x if fake else x) - 1.0)

    def leaf(t):
        return None if t is None else t.detach().cpu().double().requires_grad_(True)
    real, fake = leaf(pred_real), leaf(pred_fake)
    w = None if weight is None else weight.detach().cpu().double().reshape(1, -1)
    lab = None if label is None else label.detach().cpu().double().expand(pred_real.shape)
    losses, scales = [], []
    for x, is_fake in ((real, False), (real if lab is not None else fake, True)):
        if x is None:
            losses.append(torch.zeros((), dtype=torch.float64)); scales.append(torch.zeros((), dtype=torch.float64))
            continue
        t = term(x, is_fake)
        if w is not None:
            t = (t.reshape(-1, w.numel()) * w)
        if lab is not None:
            t = t * ((1.0 - lab) if is_fake else lab)
        losses.append(t.mean()); scales.append(t.detach().abs().mean())
    (cotangents[0] * losses[0] + cotangents[1] * losses[1]).backward()
    return {"loss": torch.stack([v.detach() for v in losses]), "absmean": torch.stack(scales),
            "grad_real": None if real is None else real.grad, "grad_fake": None if fake is None else fake.grad}


def worst_rel(got, ref):
    """max over elements of |got - ref| / max(|ref|, FLT_MIN): the element-wise relative error, references below the smallest
    normal fp32 number measured against that number instead."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return ((got - ref).abs() / ref.abs().clamp_min(FLT_MIN)).max().item() if ref.numel() else 0.0


def zeros_kept(got, ref):
    """Exact zeros where the reference has them."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    return bool((got[ref == 0] == 0).all())


def bf16_ulps(got, ref):
    """max |got - ref| in units of ref's bf16 spacing (2^(floor(log2 |ref|) - 7); references below the smallest normal number
    take that number's spacing)."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    spacing = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(FLT_MIN))) - 7.0)
    return ((got - ref).abs() / spacing).max().item()
