"""The trapped-yeast-cell TLFM dataset of the reference (dataset/tlfm_dataset.py:15-198, the class train_multi_stylegan.py:60-63
builds), without its cv2 / torchvision dependencies, and with a second mode that leaves the arithmetic to the GPU.

* ``read_tiff``: a baseline-TIFF reader in numpy (what ``cv2.imread(path, -1)`` returns for the camera's files).
* ``TFLMDatasetGAN`` (the reference's spelling): same constructor, same file discovery, same samples.
  ``raw=False`` returns the reference's normalised float32 ``[C, T, H, W]``; ``raw=True`` returns the untouched 16-bit counts
  and the horizontal-flip decision, for ``data.TLFMDeviceFeed`` / ``data.prepare_tlfm_batch`` to normalise on the device:
  half the bytes over the bus and no float arithmetic on the host.
* ``ElasticDeformation`` / ``elastic_deformation`` (dataset/tlfm_dataset.py:201-275) live in ``elastic.py`` and are importable from
  here, as in the reference.
"""
import os
import struct
from typing import Callable, List, Optional, Tuple, Union

import numpy as np
import torch
from torch.utils.data import Dataset

from .data import prepare_tlfm_batch
from .elastic import ElasticDeformation, elastic_deformation          # (where the reference defines them)

_TYPE_CODES = {1: "B", 3: "H", 4: "I", 6: "b", 8: "h", 9: "i"}          # the integer field types (BYTE, SHORT, LONG and signed)
_TAG_NAMES = {258: "BitsPerSample", 259: "Compression", 262: "PhotometricInterpretation", 274: "Orientation",
              277: "SamplesPerPixel", 284: "PlanarConfiguration", 322: "TileWidth", 339: "SampleFormat"}


def _fallback_read(path: str, why: str) -> np.ndarray:
    """A file outside the baseline subset: through cv2 or PIL when one of them happens to be importable, else the
    ValueError that names the file and the tag."""
    image = None
    try:
        import cv2
        image = cv2.imread(path, -1)
    except ImportError:
        try:
            from PIL import Image
            with Image.open(path) as handle:
                image = np.asarray(handle)
        except ImportError:
            pass
        except Exception as exc:
            raise ValueError(f"{path}: {why}, and PIL could not read it either ({exc})") from exc
    if image is None:
        raise ValueError(f"{path}: {why} (read_tiff reads uncompressed single-sample 8/16-bit unsigned strips; neither cv2 "
                         "nor PIL is importable for anything else)")
    if image.ndim != 2 or image.dtype not in (np.uint8, np.uint16):
        raise ValueError(f"{path}: {why}; the fallback reader returned {image.dtype} {image.shape}, not one 8/16-bit plane")
    return np.ascontiguousarray(image.astype(np.uint16))


def read_tiff(path: str) -> np.ndarray:
    """``[H, W]`` uint16 pixels of a baseline TIFF: ``II`` or ``MM`` byte order, Compression = 1, one sample per pixel,
    8-bit (widened) or 16-bit unsigned, one or many strips; the first image of the file, as ``cv2.imread(path, -1)``.
    Anything else -- compression, tiles, RGB / palette, signed or float samples, BigTIFF -- is read through cv2 / PIL if one is
    importable and otherwise raises a ValueError naming the file and the unsupported tag value; never wrong pixels."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 8 or data[:2] not in (b"II", b"MM"):
        raise ValueError(f"{path}: not a TIFF file (byte-order mark {data[:2]!r})")
    e = "<" if data[:2] == b"II" else ">"
    magic, ifd = struct.unpack(e + "HI", data[2:8])
    if magic == 43:
        return _fallback_read(path, "BigTIFF (version 43) is not supported")
    if magic != 42:
        raise ValueError(f"{path}: not a TIFF file (version {magic})")
    if ifd + 2 > len(data):
        raise ValueError(f"{path}: truncated (image directory at {ifd}, file has {len(data)} bytes)")
    (count,) = struct.unpack(e + "H", data[ifd:ifd + 2])
    tags = {}
    for k in range(count):
        entry = data[ifd + 2 + 12 * k:ifd + 14 + 12 * k]
        if len(entry) < 12:
            raise ValueError(f"{path}: truncated image directory")
        tag, typ, n = struct.unpack(e + "HHI", entry[:8])
        if typ not in _TYPE_CODES:
            continue                                              # ASCII, rationals, ...: nothing the pixels depend on
        size = struct.calcsize(_TYPE_CODES[typ]) * n
        if size <= 4:
            payload = entry[8:8 + size]
        else:
            (at,) = struct.unpack(e + "I", entry[8:12])
            payload = data[at:at + size]
        if len(payload) < size:
            raise ValueError(f"{path}: truncated (values of tag {tag})")
        tags[tag] = struct.unpack(e + str(n) + _TYPE_CODES[typ], payload)

    def one(tag, default):
        return tags[tag][0] if tag in tags and len(tags[tag]) else default

    if 322 in tags:
        return _fallback_read(path, f"TileWidth = {one(322, None)}: tiled files are not supported")
    if 256 not in tags or 257 not in tags or 273 not in tags:
        raise ValueError(f"{path}: ImageWidth / ImageLength / StripOffsets missing")
    width, height = int(one(256, 0)), int(one(257, 0))
    bits = tags.get(258, (1,))
    for tag in (259, 277, 339, 262, 274):
        if one(tag, 1) != 1:
            return _fallback_read(path, f"{_TAG_NAMES[tag]} = {one(tag, 1)} is not supported")
    if len(bits) != 1 or bits[0] not in (8, 16):
        return _fallback_read(path, f"BitsPerSample = {bits if len(bits) != 1 else bits[0]} is not supported")
    nbytes = bits[0] // 8
    offsets = tags[273]
    rows_per_strip = min(int(one(278, height)), height)
    if width <= 0 or height <= 0 or rows_per_strip <= 0 or len(offsets) != -(-height // rows_per_strip):
        raise ValueError(f"{path}: {len(offsets)} strips of {rows_per_strip} rows do not make {height} rows")
    counts = tags.get(279)
    image = np.empty((height, width), dtype=np.uint16)
    dtype = np.dtype(np.uint8 if nbytes == 1 else np.uint16).newbyteorder(e)
    for k, at in enumerate(offsets):
        rows = min(rows_per_strip, height - k * rows_per_strip)
        need = rows * width * nbytes
        if at + need > len(data) or (counts is not None and (len(counts) != len(offsets) or counts[k] < need)):
            raise ValueError(f"{path}: truncated (strip {k} needs {need} bytes at {at})")
        image[k * rows_per_strip:k * rows_per_strip + rows] = np.frombuffer(data, dtype, rows * width, at).reshape(rows, width)
    return image


def _sort_key(item: str) -> str:
    """Time step, then trap number (dataset/tlfm_dataset.py:82-84)."""
    return item.split("-")[-1].split("_")[-1].replace(".tif", "") + item.split("_")[-5]


class TFLMDatasetGAN(Dataset):
    """The reference's unsupervised TLFM dataset (dataset/tlfm_dataset.py:15-198): bright-field / GFP / RFP sequences of
    ``sequence_length`` frames of one trap and z position, found under ``path/<position folder>/``.

    Differences from the reference, all stated here:
      * ``transformations`` defaults to None = a random horizontal flip with p = 0.5 drawn as ``torch.rand(1) < p``, the draw
        torchvision's ``RandomHorizontalFlip`` makes (equal seeds flip equal samples); any callable on the stacked float frames
        ``[C * T, H, W]`` is still accepted;
      * position folders and directory listings are visited in sorted order (the reference: whatever ``os.listdir`` returns), so
        epochs are reproducible across file systems;
      * files are read with ``read_tiff`` (no cv2);
      * ``raw=True``: ``__getitem__`` returns ``(frames, hflip)`` -- ``frames`` the untouched counts as ``torch.uint16``
        ``[C, T, H, W]``, ``hflip`` a ``torch.uint8`` scalar holding the flip draw -- and does no float arithmetic;
        ``default_collate`` stacks both, ``data.TLFMDeviceFeed`` normalises the batch on the GPU.  Not with a callable
        ``transformations`` (ValueError): a callable works on float frames.
      * ``no_gfp`` without ``no_rfp`` is refused at construction (the reference fails on its first sample, :195).

    ``raw=False`` returns the reference's sample (:186-198), float32 ``[C, T, H, W]``, C = 1 (``no_gfp``), 2 (``no_rfp``) or
    3: bright field min-max normalised per frame (dataset/utils.py:4-23 -- a constant frame is 0 / 0 = NaN in every pixel, as
    there), GFP ``((x - gfp_min).clamp(min=0) / gfp_max).clamp(max=1)`` (divided by ``gfp_max``, not by the range), RFP
    likewise, the horizontal flip on all C * T frames together, the vertical flip when ``flip``.  Works without a GPU.
    """

    def __init__(self, path: str,
                 sequence_length: int = 3,
                 overlap: bool = True,
                 transformations: Optional[Callable[[torch.Tensor], torch.Tensor]] = None,
                 z_position_indications: Tuple[str, ...] = ("_000_", "_001_", "_002_"),
                 gfp_min: Union[float, int] = 150.0,
                 gfp_max: Union[float, int] = 2200.0,
                 rfp_min: Union[float, int] = 20.0,
                 rfp_max: Union[float, int] = 2000.0,
                 flip: bool = True,
                 positions: Optional[Tuple[str, ...]] = None,
                 no_rfp: bool = False,
                 no_gfp: bool = False,
                 raw: bool = False) -> None:
        if raw and transformations is not None:
            raise ValueError("raw=True returns integer counts and a flip flag; a `transformations` callable works on float "
                             "frames -- use raw=False with it")
        if no_gfp and not no_rfp:
            raise ValueError("no_gfp=True needs no_rfp=True (a sample without GFP has one channel)")
        self.transformations = transformations
        self.horizontal_flip_probability = 0.5
        self.gfp_min, self.gfp_max = gfp_min, gfp_max
        self.rfp_min, self.rfp_max = rfp_min, rfp_max
        self.flip = flip
        self.no_rfp, self.no_gfp = no_rfp, no_gfp
        self.raw = raw
        self.paths_to_dataset_samples: List[Tuple[Tuple[str, ...], Tuple[str, ...], Tuple[str, ...]]] = []
        for position_folder in sorted(os.listdir(path)):
            if (positions is not None) and (position_folder not in positions):
                continue
            if not os.path.isdir(os.path.join(path, position_folder)):
                continue
            all_images = [os.path.join(path, position_folder, image_file)
                          for image_file in sorted(os.listdir(os.path.join(path, position_folder))) if "tif" in image_file]
            by_kind = []
            for mark in ("-BF0_", "-GFP", "-RFP"):                 # substring tests on the full path, as the reference
                of_kind = [image_file for image_file in all_images if mark in image_file]
                per_z = []
                for z_position_indication in z_position_indications:
                    per_z.append(sorted((image_file for image_file in of_kind if z_position_indication in image_file),
                                        key=_sort_key))
                by_kind.append(per_z)
            bf_images, gfp_images, rfp_images = by_kind
            for z_position in range(len(z_position_indications)):
                for index in range(0, len(bf_images[z_position]) - sequence_length + 1, 1 if overlap else sequence_length):
                    if self._check_if_same_trap(bf_images[z_position][index:index + sequence_length]):
                        self.paths_to_dataset_samples.append(
                            (tuple(bf_images[z_position][index:index + sequence_length]),
                             tuple(gfp_images[z_position][index:index + sequence_length]),
                             tuple(rfp_images[z_position][index:index + sequence_length])))

    def _check_if_same_trap(self, path_list: List[str]) -> bool:
        traps = [path[path.find("trap"):path.find("trap") + 8] for path in path_list]
        return all(trap == traps[0] for trap in traps)

    def __len__(self) -> int:
        return len(self.paths_to_dataset_samples)

    def _counts(self, item: int) -> torch.Tensor:
        """The sample's files as one uint16 ``[C, T, H, W]`` tensor."""
        kinds = self.paths_to_dataset_samples[item][:1 if self.no_gfp else (2 if self.no_rfp else 3)]
        return torch.from_numpy(np.stack([np.stack([read_tiff(p) for p in paths]) for paths in kinds]))

    def __getitem__(self, item: int):
        counts = self._counts(item)
        if self.transformations is None:
            hflip = (torch.rand(1) < self.horizontal_flip_probability).to(torch.uint8).reshape(())
            if self.raw:
                return counts, hflip
            frames = counts[None]
            hflip = hflip[None]
        else:
            channels, length = counts.shape[:2]
            images = torch.from_numpy(counts.numpy().astype(np.float32)).flatten(0, 1)
            images = self.transformations(images)
            images = images[0] if images.ndimension() == 4 else images
            frames = images.reshape(channels, length, *images.shape[-2:])[None]
            hflip = None
        return prepare_tlfm_batch(frames, hflip, vertical_flip=self.flip, gfp=(self.gfp_min, self.gfp_max),
                                  rfp=(self.rfp_min, self.rfp_max))[0]
