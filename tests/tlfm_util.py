"""Shared by tests/test_tlfm_dataset.py and tests/test_hip_tlfm.py: the tests' own minimal TIFF writer, the recorded fixtures of
tests/golden/tlfm/ (tools/gen_golden_tlfm.py) and a torch restatement of the reference's sample arithmetic."""
import json
import os
import struct

import numpy as np
import torch

from conftest import GOLDEN

TLFM = os.path.join(GOLDEN, "tlfm")


def write_tiff(path, image):
    """Little-endian, uncompressed, single-strip, 16-bit grey-scale TIFF: header, pixels, image directory."""
    image = np.ascontiguousarray(image, dtype="<u2")
    height, width = image.shape
    pixels = image.tobytes()
    tags = [(256, 3, width), (257, 3, height), (258, 3, 16), (259, 3, 1), (262, 3, 1), (273, 4, 8), (277, 3, 1),
            (278, 3, height), (279, 4, len(pixels))]
    ifd = struct.pack("<H", len(tags)) + b"".join(struct.pack("<HHII", t, k, 1, v) for t, k, v in tags) + struct.pack("<I", 0)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        f.write(b"II" + struct.pack("<HI", 42, 8 + len(pixels)) + pixels + ifd)


def listing():
    with open(os.path.join(TLFM, "listing.json")) as f:
        return json.load(f)


_SAMPLES = {}


def samples():
    """tests/golden/tlfm/samples.npz, loaded once and shared (read-only)."""
    if not _SAMPLES:
        with np.load(os.path.join(TLFM, "samples.npz")) as z:
            _SAMPLES.update({k: z[k] for k in z.files})
        for a in _SAMPLES.values():
            a.setflags(write=False)
    return _SAMPLES


def case_counts(case):
    """uint16 [C, T, H, W] counts of a recorded case: the channels its dataset settings keep."""
    raw = samples()["raw." + case["raw"]]
    return raw[:1 if case["no_gfp"] else (2 if case["no_rfp"] else 3)]


def write_case_tree(root, case):
    """The recorded sample's own files (all three kinds) under ``root``: a dataset directory with exactly this sample."""
    raw = samples()["raw." + case["raw"]]
    for kind, names in zip(raw, case["paths"]):
        for image, name in zip(kind, names):
            write_tiff(os.path.join(root, name), image)


def reference_sample(counts, hflip, vflip, gfp=(150.0, 2200.0), rfp=(20.0, 2000.0)):
    """One sample as the reference computes it (dataset/tlfm_dataset.py:186-197, dataset/utils.py:4-23), written from those
    lines: counts [C, T, H, W] (any integer array) -> float32 [C, T, H, W].  Flip first, then normalise."""
    x = torch.from_numpy(np.asarray(counts).astype(np.float32))
    x = x.flip(-1) if hflip else x
    flat = x[0].flatten(start_dim=1)
    lo, hi = flat.min(dim=1, keepdim=True)[0], flat.max(dim=1, keepdim=True)[0]
    out = [((flat - lo) / (hi - lo)).reshape(x[0].shape)]
    out += [((x[c] - low).clamp(min=0.0) / div).clamp(max=1.0) for c, (low, div) in zip(range(1, x.shape[0]), (gfp, rfp))]
    out = torch.stack(out)
    return out.flip(dims=(-2,)) if vflip else out


def same_bits(a, b):
    """Bit equality of two float tensors (NaN payloads included)."""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))
