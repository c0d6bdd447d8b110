#!/usr/bin/env python3
"""Generate tests/golden/sheets/ by running the REFERENCE's own ``Logger.save_prediction`` (multi_stylegan/misc.py:132-166) with
``torchvision.utils.save_image`` replaced by a recorder.

Runs only in the build container (needs /root/reference); the fixtures are plain data -- the input predictions, the float
tensors the reference hands to ``save_image``, the file names and the two grid settings -- and nothing of the reference travels
with them.

How the reference's ``misc`` is made importable: ``multi_stylegan`` is an empty package over the reference's directory (its
``__init__`` would import the CUDA operators), ``torchvision`` is a stand-in whose ``utils.save_image`` records its arguments.  The
``Logger`` is built with ``object.__new__`` and given ``path_plots`` only: its constructor creates directories, ``save_prediction``
reads nothing else.

What this pins to the reference: the colour mapping (which planes of which channel are zero), the channel order, the file names
and the sheet geometry (T pictures, ``nrow=T``, ``padding=0``: side by side).  The quantisation that follows inside
``save_image`` is torchvision's published ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)`` and cannot be pinned to an installed
copy; the tests restate it in numpy.

What is written:
  save_prediction.npz   per case c1 / c2 / c3: ``<case>.prediction`` [2, C, 3, 8, 16] fp32 over about [-0.2, 1.2] and, per
                        recorded call k, ``<case>.call<k>`` = the [T, 3, H, W] tensor handed to save_image
  manifest.json         per case: the ``name`` argument and, per call, the file's base name, nrow and padding

Usage: python tools/gen_golden_sheets.py [--check-only]
"""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "sheets")
CASES = {"c1": 1, "c2": 2, "c3": 3}
SHAPE = (2, 3, 8, 16)                                     # B, T, H, W


def import_reference_misc(recorder):
    sys.path.insert(0, REF)
    pkg = types.ModuleType("multi_stylegan")
    pkg.__path__ = [os.path.join(REF, "multi_stylegan")]
    sys.modules["multi_stylegan"] = pkg
    tv, utils = types.ModuleType("torchvision"), types.ModuleType("torchvision.utils")
    utils.save_image = recorder
    tv.utils = utils
    sys.modules["torchvision"], sys.modules["torchvision.utils"] = tv, utils
    return importlib.import_module("multi_stylegan.misc")


def generate():
    calls = []

    def save_image(tensor, fp, nrow=8, padding=2, **rest):
        assert not rest, f"save_image was given {sorted(rest)}: the fixture's format does not record them"
        calls.append({"tensor": tensor.detach().clone(), "file": os.path.basename(fp), "nrow": int(nrow), "padding": int(padding)})

    misc = import_reference_misc(save_image)
    logger = object.__new__(misc.Logger)
    logger.path_plots = os.path.join("nowhere", "plots")
    arrays, manifest = {}, {"generator": "tools/gen_golden_sheets.py", "cases": {}}
    for case, channels in sorted(CASES.items()):
        g = torch.Generator().manual_seed(100 + channels)
        B, T, H, W = SHAPE
        prediction = torch.rand(B, channels, T, H, W, generator=g) * 1.4 - 0.2
        name = f"prediction_{case}_7"
        del calls[:]
        logger.save_prediction(prediction=prediction.clone(), name=name)
        arrays[f"{case}.prediction"] = prediction.numpy()
        listed = []
        for k, call in enumerate(calls):
            arrays[f"{case}.call{k}"] = call["tensor"].numpy()
            listed.append({"file": call["file"], "nrow": call["nrow"], "padding": call["padding"]})
        manifest["cases"][case] = {"name": name, "channels": channels, "calls": listed}
    return arrays, manifest


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true", help="regenerate and compare with the committed fixture, write nothing")
    args = ap.parse_args()
    arrays, manifest = generate()
    npz, man = os.path.join(OUT, "save_prediction.npz"), os.path.join(OUT, "manifest.json")
    if args.check_only:
        have = np.load(npz)
        assert sorted(have.files) == sorted(arrays), "the fixture's keys differ"
        assert all(np.array_equal(have[k], arrays[k], equal_nan=True) for k in arrays), "the fixture's arrays differ"
        assert json.load(open(man)) == manifest, "the manifest differs"
        print("tests/golden/sheets agrees with the reference (nothing written)")
        return
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(npz, **arrays)
    with open(man, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {npz} ({os.path.getsize(npz)} bytes) and {man}")


if __name__ == "__main__":
    main()
