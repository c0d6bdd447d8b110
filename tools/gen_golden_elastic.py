#!/usr/bin/env python3
"""Generate tests/golden/elastic.npz by running the REFERENCE's own ``elastic_deformation`` (dataset/tlfm_dataset.py:230-275) on
the CPU under recorded seeds.

Runs only in the build container (needs /root/reference).  The reference module imports cv2 and torchvision at its top (for the
dataset class beside the function): empty stand-ins are registered for both, nothing of them is called.  The fixture is plain
data and nothing of the reference travels with it.

Cases (F frames of H x W, sigma, alpha):
  defaults   6 x 64 x 64, 16, 80   the class defaults: the 65-tap kernel is wider than the frame
  even       2 x 48 x 48,  4, 50   even square: the half-pixel shift
  nonsquare  3 x 40 x 56,  3, 30   the swapped divisors
  odd        1 x 33 x 33,  2, 20   odd: no half-pixel shift; no 16-byte row
  tiny       2 x  8 x  8,  4, 10   a frame smaller than the halo
Frames are independent random multiples of 1/64 in [0, 1] -- full contrast between neighbours (a smooth image hides position
errors), exact in bfloat16 (one fixture serves both storage types) and compressible.

Per case the file holds
  <case>.frames  [F, H, W] float32
  <case>.params  [3] int64: seed, sigma, alpha
  <case>.noise   [2, H, W] float32: the two planes ``torch.rand((H, W)) * 2 - 1`` the reference drew, obtained by replaying the
                 seed -- first draw (horizontal component), then second draw (vertical)
  <case>.out     [F, H, W] float32: what the reference's function returned after ``torch.manual_seed(seed)``
  <case>.next    [1] float32: ``torch.rand(1)`` right after the reference's call (where it leaves the global generator)

Usage: python tools/gen_golden_elastic.py [--check-only]
"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "elastic.npz")
CASES = {"defaults": (6, 64, 64, 16, 80, 101), "even": (2, 48, 48, 4, 50, 102), "nonsquare": (3, 40, 56, 3, 30, 103),
         "odd": (1, 33, 33, 2, 20, 104), "tiny": (2, 8, 8, 4, 10, 105)}


def reference_module():
    class _Anything:
        def __init__(self, *args, **kwargs):
            pass

    vision, transforms = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    transforms.Compose = transforms.RandomHorizontalFlip = _Anything      # (the dataset class's default argument)
    vision.transforms = transforms
    sys.modules.setdefault("torchvision", vision)
    sys.modules.setdefault("torchvision.transforms", transforms)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    package = types.ModuleType("dataset")
    package.__path__ = [os.path.join(REF, "dataset")]
    sys.modules["dataset"] = package
    spec = importlib.util.spec_from_file_location("dataset.tlfm_dataset", os.path.join(REF, "dataset", "tlfm_dataset.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def generate():
    ref = reference_module()
    sys.path.insert(0, ROOT)
    from multi_stylegan_amd.elastic import elastic_deformation
    arrays = {}
    for name, (frames, height, width, sigma, alpha, seed) in CASES.items():
        g = torch.Generator().manual_seed(1000 + seed)
        x = torch.randint(0, 65, (frames, height, width), generator=g).float() / 64.0
        assert torch.equal(x, x.bfloat16().float())
        torch.manual_seed(seed)
        out = ref.elastic_deformation(x.clone(), alpha=alpha, sigma=sigma)
        after = torch.rand(1)
        torch.manual_seed(seed)
        noise = torch.stack([torch.rand((height, width), dtype=torch.float) * 2. - 1. for _ in range(2)])
        assert torch.equal(torch.rand(1), after), "the replay does not consume what the reference consumed"
        torch.manual_seed(seed)
        mine = elastic_deformation(x.clone(), alpha=alpha, sigma=sigma)
        err = (mine - out).abs().max().item()
        assert err <= 1e-4, (name, err)                                    # also proves the order of the two planes
        print(f"{name}: product CPU function vs reference {err:.2e}")
        arrays.update({f"{name}.frames": x.numpy(), f"{name}.params": np.array([seed, sigma, alpha], dtype=np.int64),
                       f"{name}.noise": noise.numpy(), f"{name}.out": out.numpy(), f"{name}.next": after.numpy()})
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true", help="regenerate and compare with the committed fixture, write nothing")
    args = ap.parse_args()
    arrays = generate()
    if args.check_only:
        have = np.load(OUT)
        assert sorted(have.files) == sorted(arrays), "the fixture's keys differ"
        assert all(np.array_equal(have[k], arrays[k]) for k in arrays), "the fixture's arrays differ"
        print("tests/golden/elastic.npz agrees with the reference (nothing written)")
        return
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(arrays)} arrays)")


if __name__ == "__main__":
    main()
