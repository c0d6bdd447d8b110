#!/usr/bin/env python3
"""Generate tests/golden/tlfm/ by running the REFERENCE's own ``dataset.TFLMDatasetGAN`` on a small tree of TIFF files.

Runs only in the build container (needs /root/reference); the fixtures are plain data -- file names, pixel counts and the
reference's outputs -- and nothing of the reference travels with them.

How the reference's dataset is made importable: it imports cv2 and torchvision, neither of which is installed, so
  * ``cv2.imread(path, -1)`` is this package's ``read_tiff`` (the reference only calls it with flag -1),
  * ``torchvision.transforms`` has ``Compose`` and ``RandomHorizontalFlip`` (the constructor's default argument; the draw
    ``torch.rand(1) < p`` is torchvision's),
  * ``os.listdir`` is sorted (the package visits directories in sorted order; the reference in the file system's).

What is written:
  listing.json   the tree's file names and the reference's ``paths_to_dataset_samples`` for three settings (each path as its
                 index into "files"), and which files make up the recorded samples
  samples.npz    the uint16 frames of two samples (12 x 20 and 16 x 24 pixels) and the reference's outputs for six cases
                 (C = 1, 2, 3; vertical flip on / off; horizontal flip forced on / off through a deterministic callable)
  le16_single.tif, be16_strips.tif, u8.tif, lzw16.tif (+ their pixels in reader.npz) and manifest.json (which writer made them)

Usage: python tools/gen_golden_tlfm.py [--check-only]
"""
import argparse
import io
import json
import os
import struct
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
OUT = os.path.join(ROOT, "tests", "golden", "tlfm")
sys.path.insert(0, ROOT)

from multi_stylegan_amd.tlfm_dataset import read_tiff  # noqa: E402

POSITIONS = {"posA": (12, 20), "posB": (16, 24)}          # frame sizes: W no multiple of 8, and one vector row of three
Z_POSITIONS = ("_000_", "_001_", "_002_")
TRAPS, TIME_STEPS = (1, 2), 4                              # 8 files per kind and z: windows of 3 straddle the trap boundary
LISTING_SETTINGS = [(3, True, None), (3, False, None), (2, True, ("posB",))]
# name: (position folder, sample index within that folder's own dataset, no_gfp, no_rfp, vertical flip, horizontal flip)
SAMPLE_CASES = {"c3_vflip_hflip": ("posA", 0, False, False, True, True),
                "c3_plain": ("posB", 1, False, False, False, False),
                "c2_vflip": ("posB", 1, False, True, True, False),
                "c2_hflip": ("posA", 0, False, True, False, True),
                "c1_vflip_hflip": ("posB", 1, True, True, True, True),
                "c1_plain": ("posA", 0, True, True, False, False)}


def file_name(position, kind, z, trap, time):
    """``split("-")[-1].split("_")[-1]`` is the trap and ``split("_")[-5]`` the time step: the reference's sort key puts a trap's
    time steps next to each other."""
    return f"{position}_t{time:03d}_x_trap{trap:04d}-{kind}{z}{trap:04d}.tif"


# ------------------------------------------------------------------------------------------------ the tool's own TIFF writer
def lzw_literals(data: bytes) -> bytes:
    """A valid TIFF LZW stream that never uses a table entry: 9-bit codes, most significant bit first, a ClearCode before the
    decoder's table could reach 511 entries (where the code width would grow), EndOfInformation at the end."""
    codes = []
    for k, byte in enumerate(data):
        if k % 200 == 0:
            codes.append(256)
        codes.append(byte)
    codes.append(257)
    bits = "".join(format(c, "09b") for c in codes)
    bits += "0" * (-len(bits) % 8)
    return bytes(int(bits[i:i + 8], 2) for i in range(0, len(bits), 8))


def own_tiff(image: np.ndarray, byte_order="<", rows_per_strip=None, compression=1) -> bytes:
    """Baseline grey-scale TIFF of a uint8 / uint16 image: header, strips, then the image directory."""
    height, width = image.shape
    rows_per_strip = rows_per_strip or height
    pixels = image.astype(image.dtype.newbyteorder(byte_order))
    strips = [pixels[r:r + rows_per_strip].tobytes() for r in range(0, height, rows_per_strip)]
    if compression == 5:
        strips = [lzw_literals(s) for s in strips]
    body, offsets = b"", []
    for s in strips:
        offsets.append(8 + len(body))
        body += s + b"\0" * (len(s) % 2)
    extra_at = 8 + len(body)
    extra = b""
    entries = []

    def entry(tag, typ, values):
        nonlocal extra
        code = {3: "H", 4: "I"}[typ]
        payload = struct.pack(byte_order + str(len(values)) + code, *values)
        if len(payload) <= 4:
            field = payload + b"\0" * (4 - len(payload))
        else:
            field = struct.pack(byte_order + "I", extra_at + len(extra))
            extra += payload
        entries.append(struct.pack(byte_order + "HHI", tag, typ, len(values)) + field)

    entry(256, 3, [width]); entry(257, 3, [height]); entry(258, 3, [8 * image.dtype.itemsize]); entry(259, 3, [compression])
    entry(262, 3, [1]); entry(273, 4, offsets); entry(277, 3, [1]); entry(278, 3, [rows_per_strip])
    entry(279, 4, [len(s) for s in strips]); entry(339, 3, [1])
    ifd_at = extra_at + len(extra)
    head = (b"II" if byte_order == "<" else b"MM") + struct.pack(byte_order + "HI", 42, ifd_at)
    return head + body + extra + struct.pack(byte_order + "H", len(entries)) + b"".join(entries) + struct.pack(byte_order + "I", 0)


def pil_tiff(image: np.ndarray):
    """The same image written by PIL (a foreign writer for the reader to be checked against), or None without PIL."""
    try:
        from PIL import Image
    except ImportError:
        return None
    buffer = io.BytesIO()
    Image.fromarray(image).save(buffer, format="TIFF")
    return buffer.getvalue()


# ------------------------------------------------------------------------------------------------ the tree and the reference
def frame_counts(rng, kind, shape, k):
    """Counts that reach the corners of the arithmetic: 0 and 65535, GFP / RFP below their minimum and above minimum + maximum."""
    if kind == "BF0":
        lo, hi = [(0, 65536), (300, 5000), (32000, 40000), (1000, 1256)][k % 4]      # also values >= 32768 (unsigned!)
        image = rng.integers(lo, hi, size=shape, dtype=np.int64)
        if k % 4 == 0:
            image.flat[rng.choice(image.size, size=2, replace=False)] = [0, 65535]
    else:
        low, top = (150, 2200) if kind == "GFP" else (20, 2000)
        image = rng.integers(0, low + top + 600, size=shape, dtype=np.int64)
        image.flat[rng.choice(image.size, size=6, replace=False)] = [0, 65535, low, low + top, low - 1, low + top + 1]
    return image.astype(np.uint16)


def build_tree(root):
    """-> ({relative name: uint16 image}, [every relative name of the tree, strays included])."""
    rng = np.random.default_rng(2024)
    images, names, k = {}, [], 0
    for position, shape in POSITIONS.items():
        os.makedirs(os.path.join(root, position))
        for kind in ("BF0", "GFP", "RFP"):
            for z in Z_POSITIONS:
                for trap in TRAPS:
                    for time in range(TIME_STEPS):
                        name = os.path.join(position, file_name(position, kind, z, trap, time))
                        images[name] = frame_counts(rng, kind, shape, k)
                        k += 1
                        with open(os.path.join(root, name), "wb") as f:
                            f.write(own_tiff(images[name]))
                        names.append(name)
        stray = os.path.join(position, "acquisition_notes.txt")
        open(os.path.join(root, stray), "w").close()
        names.append(stray)
    open(os.path.join(root, "readme.md"), "w").close()                     # a non-folder beside the position folders
    names.append("readme.md")
    return images, sorted(names)


def import_reference_dataset():
    cv2 = types.ModuleType("cv2")
    cv2.imread = lambda path, flag: read_tiff(path)
    sys.modules["cv2"] = cv2

    class Compose:
        def __init__(self, transforms):
            self.transforms = transforms

        def __call__(self, image):
            for t in self.transforms:
                image = t(image)
            return image

    class RandomHorizontalFlip:
        def __init__(self, p=0.5):
            self.p = p

        def __call__(self, image):
            return image.flip(-1) if torch.rand(1) < self.p else image

    tv, transforms = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    transforms.Compose, transforms.RandomHorizontalFlip = Compose, RandomHorizontalFlip
    tv.transforms = transforms
    sys.modules["torchvision"], sys.modules["torchvision.transforms"] = tv, transforms
    listdir = os.listdir
    os.listdir = lambda path=".": sorted(listdir(path))
    sys.path.insert(0, REF)
    from dataset.tlfm_dataset import TFLMDatasetGAN
    return TFLMDatasetGAN


def generate():
    """-> {file name under tests/golden/tlfm: bytes}."""
    reference = import_reference_dataset()
    files = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "dataset")
        os.makedirs(root)
        images, names = build_tree(root)
        relative = lambda paths: [[os.path.relpath(p, root) for p in kind] for kind in paths]
        number = lambda paths: [[names.index(p) for p in kind] for kind in relative(paths)]     # (files by their place in "files")
        listing = {"files": names, "settings": []}
        for sequence_length, overlap, positions in LISTING_SETTINGS:
            ds = reference(root, sequence_length=sequence_length, overlap=overlap, positions=positions)
            listing["settings"].append({"sequence_length": sequence_length, "overlap": overlap, "positions": positions,
                                        "samples": [number(s) for s in ds.paths_to_dataset_samples]})
        arrays, listing["cases"] = {}, {}
        for case, (position, index, no_gfp, no_rfp, vflip, hflip) in SAMPLE_CASES.items():
            force = (lambda x: x.flip(-1)) if hflip else (lambda x: x)
            ds = reference(root, transformations=force, positions=(position,), flip=vflip, no_rfp=no_rfp, no_gfp=no_gfp)
            paths = relative(ds.paths_to_dataset_samples[index])
            key = f"{position}.{index}"
            arrays["raw." + key] = np.stack([np.stack([images[p] for p in kind]) for kind in paths])
            arrays["out." + case] = ds[index].numpy()
            listing["cases"][case] = {"raw": key, "paths": paths, "no_gfp": no_gfp, "no_rfp": no_rfp, "flip": vflip,
                                      "hflip": hflip}
    files["listing.json"] = (json.dumps(listing) + "\n").encode()
    buffer = io.BytesIO()
    np.savez_compressed(buffer, **arrays)
    files["samples.npz"] = buffer.getvalue()
    # reader fixtures
    rng = np.random.default_rng(7)
    reader = {"le16_single": rng.integers(0, 65536, size=(9, 14)).astype(np.uint16),
              "be16_strips": rng.integers(0, 65536, size=(11, 13)).astype(np.uint16),
              "u8": rng.integers(0, 256, size=(10, 15)).astype(np.uint8),
              "lzw16": rng.integers(0, 65536, size=(8, 12)).astype(np.uint16)}
    for image in reader.values():
        image.flat[:2] = [0, np.iinfo(image.dtype).max]
    manifest = {}
    for name in ("le16_single", "u8"):
        foreign = pil_tiff(reader[name])
        files[name + ".tif"] = foreign if foreign is not None else own_tiff(reader[name])
        manifest[name + ".tif"] = "PIL" if foreign is not None else "tools/gen_golden_tlfm.py"
    files["be16_strips.tif"] = own_tiff(reader["be16_strips"], byte_order=">", rows_per_strip=4)
    files["lzw16.tif"] = own_tiff(reader["lzw16"], compression=5)
    manifest["be16_strips.tif"] = manifest["lzw16.tif"] = "tools/gen_golden_tlfm.py"
    files["manifest.json"] = (json.dumps({"writer": manifest}, indent=1) + "\n").encode()
    buffer = io.BytesIO()
    np.savez(buffer, **reader)
    files["reader.npz"] = buffer.getvalue()
    return files


def same(name, new, path):
    """Fixture content, not container bytes: archives by their arrays, PIL-written files by their pixels."""
    with open(path, "rb") as f:
        old = f.read()
    if name.endswith(".npz"):
        a, b = np.load(io.BytesIO(new)), np.load(io.BytesIO(old))
        return sorted(a.files) == sorted(b.files) and all(a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True)
                                                          for k in a.files)
    if name in ("le16_single.tif", "u8.tif"):
        with tempfile.NamedTemporaryFile(suffix=".tif") as tmp:
            tmp.write(new)
            tmp.flush()
            return np.array_equal(read_tiff(tmp.name), read_tiff(path))
    if name == "manifest.json":
        return True                                          # (which writer was at hand; the pixels are compared above)
    return new == old


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check-only", action="store_true", help="regenerate and compare with the committed fixtures")
    args = ap.parse_args()
    files = generate()
    if args.check_only:
        bad = [n for n, data in files.items() if not os.path.exists(os.path.join(OUT, n)) or not same(n, data, os.path.join(OUT, n))]
        print("fixtures differ: " + ", ".join(bad) if bad else f"{len(files)} fixtures reproduce")
        return 1 if bad else 0
    os.makedirs(OUT, exist_ok=True)
    for name, data in files.items():
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(data)
        print(f"{name}: {len(data)} bytes")
    print(f"total {sum(map(len, files.values()))} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
