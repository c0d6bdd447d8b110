"""Simulated TLFM datasets: what the generator produces, handed back as data -- 16-bit camera counts in TIFF files under the
directory layout ``TFLMDatasetGAN`` discovers, so that a segmentation or tracking model (or a ``ResidentTLFMStore``) can train on
simulated traps exactly as it would on an experiment's.

The reference only ever reads such data (dataset/tlfm_dataset.py:128-198) and writes 8-bit pictures (``save_image``); the writing
direction is defined here as the inverse of the reading one:

* ``export_tlfm_batch`` turns generated frames ``[B, C, T, H, W]`` into counts (csrc/tlfm_export.hip: ``msg_tlfm_export``, the
  inverse of ``msg_tlfm_prepare``; CPU tensors take one torch statement of the same arithmetic, count for count);
* ``write_tiff`` is the counterpart of ``tlfm_dataset.read_tiff``: one plane as a baseline TIFF on ``struct`` and numpy;
* ``TLFMDatasetWriter`` moves the counts through a ring of pinned buffers on a copy stream and writes the files on worker
  threads, under the names the dataset's discovery code parses;
* ``bf_ranges_like`` draws bright-field count ranges from a real experiment, ``simulate_dataset`` runs generator -> export ->
  writer and records what it did in ``simulation.json``.

Command line: ``python -m multi_stylegan_amd.simulate --load_checkpoint F --samples N --out DIR ...``.
"""
import json
import os
import re
import struct
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from .samples import SheetWriter, _device_of, _generator_of

MAX_COUNT = 65535
KINDS = ("BF0", "GFP", "RFP")                      # the marks the dataset looks for: "-BF0_", "-GFP", "-RFP"
MAX_TRAPS_PER_POSITION = 9999                      # "trap" + four digits: the eight characters the dataset compares
MAX_SEQUENCE_LENGTH = 1000                         # "t" + three digits
#: what a directory or position prefix must not contain, and why: the dataset's substring tests run on the whole path
_FORBIDDEN = (("trap", "the dataset tells traps apart by the 8 characters at the FIRST 'trap' of the whole path"),
              ("tif", "the dataset takes every name containing 'tif' for an image"),
              ("-BF0_", "the dataset takes every path containing '-BF0_' for a bright-field image"),
              ("-GFP", "the dataset takes every path containing '-GFP' for a GFP image"),
              ("-RFP", "the dataset takes every path containing '-RFP' for an RFP image"))
_Z_MARK = re.compile(r"_00\d_")


# ------------------------------------------------------------------------------------------------------------------ export
def _check_ranges(bf_range, B: int, T: int) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """``bf_range`` as a validated CPU int32 ``[B, T, 2]`` tensor (one pair for every frame: an expanded view of that pair), and
    the caller's own tensor when it already lives on a device (its values are read back once to be checked)."""
    given, uniform = None, False
    if isinstance(bf_range, torch.Tensor):
        if bf_range.dtype not in (torch.int32, torch.int64, torch.int16, torch.uint16, torch.uint8) or \
                tuple(bf_range.shape) != (B, T, 2):
            raise ValueError(f"bf_range is (lo, hi) or an integer tensor [B = {B}, T = {T}, 2], got {bf_range.dtype} "
                             f"{tuple(bf_range.shape)}")
        if bf_range.is_cuda:
            given = bf_range
        ranges = bf_range.detach().cpu().to(torch.int32)
    else:
        pair = tuple(bf_range)
        if len(pair) != 2 or any(int(v) != v for v in pair):
            raise ValueError(f"bf_range is (lo, hi), two integer counts, or an integer tensor [B, T, 2]; got {bf_range!r}")
        ranges = torch.tensor([int(pair[0]), int(pair[1])], dtype=torch.int32).expand(B, T, 2)
        uniform = True
    if ranges.numel():
        lo, hi = ranges[..., 0], ranges[..., 1]
        if int(lo.min()) < 0 or int(hi.max()) > MAX_COUNT or bool((lo >= hi).any()):
            raise ValueError(f"bright-field count ranges need 0 <= lo < hi <= {MAX_COUNT}; got lo {int(lo.min())} .. "
                             f"{int(lo.max())}, hi {int(hi.min())} .. {int(hi.max())}")
    return (ranges if uniform else ranges.contiguous()), given


_UNIFORM_RANGES: dict = {}


def _uniform_ranges(pair: torch.Tensor, B: int, T: int, device: torch.device) -> torch.Tensor:
    """One validated (lo, hi) for every frame, as the device tensor the entry reads: uploaded once and kept (a handful of
    entries; they are constants, so sharing them between calls and streams is sound)."""
    key = (int(pair[0]), int(pair[1]), B, T, device.index if device.index is not None else torch.cuda.current_device())
    cached = _UNIFORM_RANGES.get(key)
    if cached is None:
        if len(_UNIFORM_RANGES) >= 16:
            _UNIFORM_RANGES.clear()
        cached = _UNIFORM_RANGES[key] = pair.to(device).expand(B, T, 2).contiguous()
    return cached


def _pair(name: str, value) -> Tuple[float, float]:
    pair = tuple(value)
    if len(pair) != 2:
        raise ValueError(f"{name} is the dataset's (min, max), got {value!r}")
    return float(pair[0]), float(pair[1])


def _to_counts(v: torch.Tensor) -> torch.Tensor:
    """fp32 -> uint16: rint (ties to even), NaN -> 0, clamped to [0, 65535]."""
    q = torch.round(v).nan_to_num(nan=0.0, posinf=float(MAX_COUNT), neginf=0.0).clamp(0.0, float(MAX_COUNT))
    return torch.from_numpy(q.to(torch.int32).numpy().astype(np.uint16))


def _export_tlfm_host(x: torch.Tensor, ranges: torch.Tensor, vertical_flip: bool, gfp, rfp, bf_normalise: bool) -> torch.Tensor:
    """The host's one definition of the export, ``msg_tlfm_export``'s arithmetic in torch: fp32 ``[B, C, T, H, W]`` frames and
    int32 ``[B, T, 2]`` ranges -> uint16 counts.  Every operation is a torch call of its own, so each is rounded once (no fused
    multiply-add), as in the kernel."""
    x = x.to(torch.float32)
    B, C, T, H, W = x.shape
    v = torch.empty_like(x)
    offset = ranges[..., 0].to(torch.float32).view(B, T, 1, 1)
    scale = (ranges[..., 1] - ranges[..., 0]).to(torch.float32).view(B, T, 1, 1)
    bf = x[:, 0]
    if bf_normalise:
        nan = bf.isnan()                                                     # NaN takes no part in the minimum / maximum
        m = torch.where(nan, torch.full_like(bf, float("inf")), bf).flatten(start_dim=2).amin(dim=2).view(B, T, 1, 1)
        M = torch.where(nan, torch.full_like(bf, float("-inf")), bf).flatten(start_dim=2).amax(dim=2).view(B, T, 1, 1)
        n = torch.where(M == m, torch.where(nan, bf, torch.zeros_like(bf)), (bf - m) / (M - m))
    else:
        n = bf.clamp(0.0, 1.0)
    v[:, 0] = (n * scale) + offset
    for c, (low, div) in zip(range(1, C), (gfp, rfp)):
        v[:, c] = (x[:, c].clamp(0.0, 1.0) * div) + low
    if vertical_flip:
        v = v.flip(dims=(-2,))
    return _to_counts(v)


def export_tlfm_batch(x: torch.Tensor, bf_range, *, gfp=(150., 2200.), rfp=(20., 2000.), vertical_flip: bool = True,
                      bf_normalise: bool = True) -> torch.Tensor:
    """Generated frames ``[B, C, T, H, W]`` (float32 or bfloat16; C = 1 bright field, 2 + GFP, 3 + RFP) -> the camera counts
    ``torch.uint16 [B, C, T, H, W]`` the dataset would have read them from: ``data.prepare_tlfm_batch`` backwards.

    * Bright field: the frame is min-max normalised over its non-NaN values, ``n = (x - m) / (M - m)``, and spread over its count
      range, ``count = rint(n * (hi - lo) + lo)``; the frame's minimum writes ``lo`` and its maximum ``hi`` exactly, so the
      dataset's own normalisation of the counts returns ``n`` to within half a count.  ``bf_range`` is ``(lo, hi)`` for every
      frame or an integer tensor ``[B, T, 2]`` of per-frame ranges (``bf_ranges_like`` draws them from a real experiment),
      ``0 <= lo < hi <= 65535``.  A constant frame writes ``lo``.  ``bf_normalise=False``: ``n = clamp(x, 0, 1)`` instead.
    * GFP / RFP: ``count = rint(clamp(x, 0, 1) * max + min)`` with ``gfp`` / ``rfp`` = the dataset's ``(min, max)``: it divides
      by ``max``, not by the range, and the export mirrors that.
    * ``vertical_flip``: the rows are written bottom to top, because the dataset flips on load.  There is no horizontal flip
      (that is the dataset's augmentation, not part of the format).
    * fp32 arithmetic, each operation rounded on its own, rint to nearest-even, NaN -> 0, counts clamped to [0, 65535].

    Device tensors go through ``msg_tlfm_export`` (one call on the current stream, a fresh output tensor), CPU tensors through a
    torch statement of the same definition: the counts are identical for float32 input, and for bfloat16 input (widened first)
    too."""
    if x.ndim != 5 or not 1 <= x.shape[1] <= 3:
        raise ValueError(f"expected [B, C <= 3, T, H, W] frames, got {tuple(x.shape)}")
    if x.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames are float32 or bfloat16, got {x.dtype}")
    B, C, T, H, W = x.shape
    ranges, given = _check_ranges(bf_range, B, T)
    gfp, rfp = _pair("gfp", gfp), _pair("rfp", rfp)
    x = x.detach()
    if not x.is_cuda:
        if given is not None:
            raise ValueError("bf_range lives on a device, the frames on the CPU")
        if x.numel() == 0:
            return torch.from_numpy(np.empty(tuple(x.shape), dtype=np.uint16))
        return _export_tlfm_host(x, ranges, bool(vertical_flip), gfp, rfp, bool(bf_normalise))
    dev = _lib.require_gpu(x, given)
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.uint16, device=dev)
    if x.numel() == 0:
        return out
    if given is not None:
        ranges = given.to(torch.int32).contiguous()
    elif ranges.stride(0) == 0 and ranges.stride(1) == 0:                    # one (lo, hi) for every frame
        ranges = _uniform_ranges(ranges[0, 0], B, T, dev)
    else:
        ranges = ranges.to(dev)
    lib = _lib.lib()
    with _lib.on_device(dev):
        ws = _lib.scratch_ptr(lib.msg_tlfm_export_workspace(B, T), dev)
        with _lib.kernel_clock.span(("tlfm_export", x.dtype), x.numel() * (x.element_size() * (1.0 + 1.0 / C) + 2.0)):
            _lib.check(lib.msg_tlfm_export(x.data_ptr(), _lib.dtype_code(x), ranges.data_ptr(), out.data_ptr(), B, C, T, H, W,
                                           int(bool(vertical_flip)), int(bool(bf_normalise)), gfp[0], gfp[1], rfp[0], rfp[1],
                                           ws, _lib.stream_of(dev)), "msg_tlfm_export")
    return out


# -------------------------------------------------------------------------------------------------------------------- TIFF
def write_tiff(path_or_file, array) -> None:
    """One ``[H, W]`` plane (uint16 or uint8; a numpy array or CPU tensor) -> a baseline little-endian TIFF at ``path_or_file`` (a
    path or a binary file object): Compression 1, one sample per pixel, PhotometricInterpretation 1 (black is zero), one strip
    right behind the 8-byte header, the image directory after it.  What ``tlfm_dataset.read_tiff`` reads back exactly, and what
    ``cv2.imwrite`` would produce for the camera's frames."""
    pixels = array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else np.asarray(array)
    if pixels.dtype not in (np.uint16, np.uint8) or pixels.ndim != 2 or pixels.shape[0] < 1 or pixels.shape[1] < 1:
        raise ValueError(f"expected one uint16 or uint8 [H >= 1, W >= 1] plane, got {pixels.dtype} {tuple(pixels.shape)}")
    height, width = pixels.shape
    strip = np.ascontiguousarray(pixels, dtype=pixels.dtype.newbyteorder("<")).tobytes()
    pad = b"\0" * (len(strip) & 1)                                           # the directory starts on a word boundary
    tags = [(256, 4, width), (257, 4, height), (258, 3, 8 * pixels.dtype.itemsize), (259, 3, 1), (262, 3, 1), (273, 4, 8),
            (277, 3, 1), (278, 4, height), (279, 4, len(strip))]
    entries = b"".join(struct.pack("<HHI", tag, kind, 1) + (struct.pack("<HH", value, 0) if kind == 3 else struct.pack("<I", value))
                       for tag, kind, value in tags)
    data = (b"II" + struct.pack("<HI", 42, 8 + len(strip) + len(pad)) + strip + pad
            + struct.pack("<H", len(tags)) + entries + struct.pack("<I", 0))
    if hasattr(path_or_file, "write"):
        path_or_file.write(data)
    else:
        with open(path_or_file, "wb") as f:
            f.write(data)


# ------------------------------------------------------------------------------------------------------------------ writer
def _refuse_marks(what: str, text: str) -> None:
    for mark, why in _FORBIDDEN:
        if mark in text:
            raise ValueError(f"{what} {text!r} contains {mark!r}: {why}")
    z = _Z_MARK.search(text)
    if z:
        raise ValueError(f"{what} {text!r} contains {z.group(0)!r}: the dataset takes every path containing '_000_', '_001_' or "
                         "'_002_' for an image of that z position")


class TLFMDatasetWriter(SheetWriter):
    """``with TLFMDatasetWriter(directory) as writer: writer.submit(counts)``: a dataset directory ``TFLMDatasetGAN`` reads, written
    behind the caller's back.

    ``submit`` takes ``torch.uint16 [B, C, T, H, W]`` counts (device or CPU; ``export_tlfm_batch``'s result) and appends B
    sequences.  Sequence ``k``, counted across submits, becomes trap ``k % traps_per_position + 1`` of the position folder
    ``f"{position_prefix}{k // traps_per_position:04d}"``; channel ``c`` of its frame ``t`` is the file
    ``<pos>/<pos>_t{t:03d}_x_trap{trap:04d}-{channels[c]}_000_{trap:04d}.tif`` (``write_tiff``).  The machinery is
    ``SheetWriter``'s: a ring of ``depth`` pinned host buffers filled on a copy stream that waits for the caller's stream, which
    itself is never synchronised; ``workers`` threads that wait for the copy and write; ``submit`` blocks while the ring is full;
    a worker's exception is re-raised by the next ``submit`` or by ``close()``; ``workers=0`` writes on the calling thread.

    Why the layout is what it is -- the reader's rules (tlfm_dataset.py, as the reference's dataset/tlfm_dataset.py:60-126):
      * a position's files are sorted by ``_sort_key``: the trap number behind the last ``_``, then the ``t...`` field -- fixed
        widths keep that string order numeric, hence ``T <= 1000`` (three digits) and four-digit traps;
      * ``_check_if_same_trap`` compares the 8 characters starting at the FIRST occurrence of ``"trap"`` in the whole path:
        ``trap`` + four digits, hence ``traps_per_position <= 9999``, and hence a ``directory`` or ``position_prefix`` containing
        ``trap`` is refused -- as is one containing ``tif``, ``-BF0_``, ``-GFP``, ``-RFP`` or a z mark ``_00k_``, the other
        substring tests the dataset runs on whole paths.  The ValueError names the substring;
      * a window of ``sequence_length`` consecutive files is a sample when it stays within one trap.

    The result: ``TFLMDatasetGAN(directory, sequence_length=T, no_rfp=(C < 3), no_gfp=(C < 2))`` yields exactly one sample per
    submitted sequence, in submission order, with ``overlap=True`` or ``False`` -- a trap holds exactly T frames.  ``directory``
    is checked as given and as an absolute path; hand the dataset the same spelling."""

    def __init__(self, directory: str, position_prefix: str = "sim", traps_per_position: int = MAX_TRAPS_PER_POSITION,
                 channels: Sequence[str] = KINDS, workers: int = 4, depth: int = 2):
        directory, position_prefix = str(directory), str(position_prefix)
        for spelling in dict.fromkeys((directory, os.path.abspath(directory))):
            _refuse_marks("directory", spelling)
        _refuse_marks("position_prefix", position_prefix)
        if not position_prefix or os.sep in position_prefix or "/" in position_prefix:
            raise ValueError(f"position_prefix {position_prefix!r}: a non-empty folder-name prefix without a path separator")
        if not 1 <= int(traps_per_position) <= MAX_TRAPS_PER_POSITION:
            raise ValueError(f"traps_per_position {traps_per_position}: 1 .. {MAX_TRAPS_PER_POSITION} (the dataset compares "
                             "'trap' and four digits)")
        channels = tuple(str(c) for c in channels)
        if not 1 <= len(channels) <= 3 or channels != KINDS[:len(channels)]:
            raise ValueError(f"channels {channels}: a leading part of {KINDS}, the marks the dataset looks for")
        super().__init__(directory, workers=workers, depth=depth)
        self.position_prefix, self.traps_per_position, self.channels = position_prefix, int(traps_per_position), channels
        self.sequences = 0                                                   # submitted so far
        self._shape: Optional[Tuple[int, ...]] = None                        # [C, T, H, W] of the first submit

    def _encode(self, path: str, pixels) -> None:
        write_tiff(path, pixels.view(np.uint16))                             # (the ring moves bytes)

    def sequence_files(self, k: int, C: int, T: int) -> List[str]:
        """The ``C * T`` file names of sequence ``k`` relative to the directory, channel-major."""
        position = f"{self.position_prefix}{k // self.traps_per_position:04d}"
        trap = k % self.traps_per_position + 1
        return [os.path.join(position, f"{position}_t{t:03d}_x_trap{trap:04d}-{self.channels[c]}_000_{trap:04d}.tif")
                for c in range(C) for t in range(T)]

    def submit(self, counts: torch.Tensor) -> None:                          # noqa: D102  (documented on the class)
        if self._closed:
            raise RuntimeError("TLFMDatasetWriter is closed")
        if counts.dtype != torch.uint16 or counts.ndim != 5:
            raise ValueError(f"expected torch.uint16 [B, C, T, H, W] counts, got {counts.dtype} {tuple(counts.shape)}")
        B, C, T, H, W = counts.shape
        if not 1 <= C <= len(self.channels) or not 1 <= T <= MAX_SEQUENCE_LENGTH or H < 1 or W < 1:
            raise ValueError(f"counts {tuple(counts.shape)}: 1 .. {len(self.channels)} channels ({self.channels}), 1 .. "
                             f"{MAX_SEQUENCE_LENGTH} frames of at least one pixel")
        if self._shape is not None and self._shape != (C, T, H, W):
            raise ValueError(f"sequences of {(C, T, H, W)} after sequences of {self._shape}: one dataset, one [C, T, H, W]")
        last = (self.sequences + B - 1) // self.traps_per_position
        if B and last > 9999:
            raise ValueError(f"position folder {last} does not fit four digits: raise traps_per_position or start another directory")
        if B == 0:
            self._raise_pending()
            return
        self._raise_pending()
        first = self.sequences
        names = [name for k in range(first, first + B) for name in self.sequence_files(k, C, T)]
        for folder in dict.fromkeys(os.path.dirname(name) for name in names):
            os.makedirs(os.path.join(self.directory, folder), exist_ok=True)
        planes = counts.detach().contiguous().view(torch.uint8).reshape(B * C * T, H, 2 * W)
        self._enqueue([os.path.join(self.directory, name) for name in names], planes)
        self._shape, self.sequences = (C, T, H, W), first + B                # (a refused submit appends nothing)


# ------------------------------------------------------------------------------------------------------------------ ranges
def bf_ranges_like(source, samples: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Bright-field count ranges from a real experiment: int32 ``[samples, T, 2]`` on the CPU, ``[s, t] = (min, max)`` of frame
    ``t`` of one real sample, drawn uniformly with replacement for every simulated one (``generator``: a CPU ``torch.Generator``;
    None: the global one) -- so that simulated frames get count ranges from the real experiment's distribution.

    ``source``: a ``TFLMDatasetGAN`` (``raw=True``: nothing but its sample list is used, and each bright-field file a draw names
    is read once) or a ``ResidentTLFMStore`` (the ranges it already holds).  A constant real frame (min == max) cannot be the
    range of an export; its maximum is moved one count up (at 65535: its minimum one down)."""
    samples = int(samples)
    if samples < 0:
        raise ValueError(f"samples {samples}: a non-negative count")
    if len(source) == 0:
        raise ValueError("the source has no samples")
    ids = torch.randint(len(source), (samples,), generator=generator)
    if hasattr(source, "ranges") and hasattr(source, "samples_host"):         # a ResidentTLFMStore
        frames = source.samples_host[ids][:, 0].long()                        # [samples, T] frame ids of channel 0
        ranges = source.ranges.cpu()[frames.reshape(-1)].reshape(samples, -1, 2).to(torch.int32)
    elif hasattr(source, "paths_to_dataset_samples"):
        from .tlfm_dataset import read_tiff
        seen = {}

        def one(path):
            if path not in seen:
                image = read_tiff(path)
                seen[path] = (int(image.min()), int(image.max()))
            return seen[path]

        ranges = torch.tensor([[one(path) for path in source.paths_to_dataset_samples[int(i)][0]] for i in ids],
                              dtype=torch.int32).reshape(samples, -1, 2)
    else:
        raise ValueError(f"source is a TFLMDatasetGAN or a ResidentTLFMStore, got {type(source).__name__}")
    ranges = ranges.clone()
    flat = ranges[..., 0] == ranges[..., 1]
    ranges[..., 1] += (flat & (ranges[..., 1] < MAX_COUNT)).to(torch.int32)
    ranges[..., 0] -= (ranges[..., 0] == ranges[..., 1]).to(torch.int32)
    return ranges


# --------------------------------------------------------------------------------------------------------------- simulation
def simulation_latents(seed: int, samples: int, latent_dimensions: int) -> torch.Tensor:
    """The latents of ``simulate_dataset(..., seed=seed)``: ``[samples, D]`` drawn on the host from a generator of their own."""
    return torch.randn(int(samples), int(latent_dimensions), generator=torch.Generator().manual_seed(int(seed)))


@torch.no_grad()
def simulate_dataset(generator_or_checkpoint, samples: int, directory: str, batch_size: int = 8, bf_range=None, like=None,
                     seed: int = 0, use_graph: bool = True, writer: Optional[TLFMDatasetWriter] = None,
                     randomize_noise: bool = True, **export_kwargs) -> int:
    """``samples`` generated sequences as a dataset directory: ``GeneratorSampler`` -> ``export_tlfm_batch`` ->
    ``TLFMDatasetWriter``, ``batch_size`` at a time.  Returns the number of sequences written -- exactly ``samples``: a trailing
    partial batch is padded with its last latent and the padding is not written.

    ``generator_or_checkpoint``: a generator module, or a checkpoint (path or dict) whose ``generator_ema`` weights go into the
    reference's full-size generator.  Latents: ``simulation_latents(seed, samples, D)``, one per sequence; per-layer noise is
    fresh for every batch (``randomize_noise=False``: the generator's registered buffers).  Bright-field count ranges: either
    ``bf_range=(lo, hi)`` for every frame (default ``(0, 65535)``) or ``like=source``, one real sample's per-frame ranges per
    sequence (``bf_ranges_like`` with a generator seeded by ``seed``).  ``export_kwargs``: ``gfp``, ``rfp``, ``vertical_flip``,
    ``bf_normalise`` of ``export_tlfm_batch``.  ``writer``: the caller's own (left open); by default one is made for
    ``directory`` and closed, so the files are complete on return.

    ``simulation.json`` beside the position folders records the seed, the ranges used, ``gfp`` / ``rfp``, the checkpoint's name
    and the sample count."""
    from .inference import GeneratorSampler
    samples, batch_size = int(samples), int(batch_size)
    if samples < 0 or batch_size < 1:
        raise ValueError(f"samples {samples}, batch_size {batch_size}: a non-negative count and a positive batch")
    if bf_range is not None and like is not None:
        raise ValueError("bf_range and like are two ways to say the same thing: give one")
    unknown = set(export_kwargs) - {"gfp", "rfp", "vertical_flip", "bf_normalise"}
    if unknown:
        raise TypeError(f"unexpected keyword arguments {sorted(unknown)}")
    device = _device_of(generator_or_checkpoint)
    generator = _generator_of(generator_or_checkpoint, device)
    sampler = GeneratorSampler(generator, batch_size=batch_size, randomize_noise=randomize_noise, use_graph=use_graph,
                               device=device)
    latents = simulation_latents(seed, samples, generator.latent_dimensions).to(device)
    if like is not None:
        ranges = bf_ranges_like(like, samples, torch.Generator().manual_seed(int(seed)))
    else:
        ranges = None
        bf_range = (0, MAX_COUNT) if bf_range is None else (int(bf_range[0]), int(bf_range[1]))
    own = TLFMDatasetWriter(directory) if writer is None else None
    sink = own or writer
    root = os.path.abspath(str(directory))
    os.makedirs(root, exist_ok=True)
    shape = None
    try:
        for first in range(0, samples, batch_size):
            z = latents[first:first + batch_size]
            count = z.shape[0]
            if count < batch_size:
                z = torch.cat([z, z[-1:].expand(batch_size - count, -1)], dim=0)
            sequence = sampler(z.contiguous())[:count]
            shape = tuple(sequence.shape[1:])
            if ranges is not None and ranges.shape[1] != sequence.shape[2]:
                raise ValueError(f"`like` holds samples of {ranges.shape[1]} frames, the generator makes {sequence.shape[2]}")
            sink.submit(export_tlfm_batch(sequence, bf_range if ranges is None else ranges[first:first + count],
                                          **export_kwargs))
    finally:
        if own is not None:
            own.close()
    checkpoint = generator_or_checkpoint if isinstance(generator_or_checkpoint, str) else None
    record = {"samples": samples, "seed": int(seed), "batch_size": batch_size, "randomize_noise": bool(randomize_noise),
              "checkpoint": None if checkpoint is None else os.path.basename(checkpoint),
              "bf_range": list(bf_range) if ranges is None else None,
              "bf_ranges": None if ranges is None else ranges.tolist(),
              "gfp": list(_pair("gfp", export_kwargs.get("gfp", (150., 2200.)))),
              "rfp": list(_pair("rfp", export_kwargs.get("rfp", (20., 2000.)))),
              "vertical_flip": bool(export_kwargs.get("vertical_flip", True)),
              "bf_normalise": bool(export_kwargs.get("bf_normalise", True)),
              "sequence_shape": None if shape is None else list(shape),
              "position_prefix": sink.position_prefix, "traps_per_position": sink.traps_per_position}
    with open(os.path.join(root, "simulation.json"), "w") as f:
        json.dump(record, f, indent=1)
    return samples


# ----------------------------------------------------------------------------------------------------------- command line
def _parser():
    import argparse
    parser = argparse.ArgumentParser(prog="python -m multi_stylegan_amd.simulate", description=__doc__.split("\n\n")[0])
    parser.add_argument("--load_checkpoint", default="checkpoint_100.pt", type=str, help="Path to checkpoint to be loaded.")
    parser.add_argument("--samples", default=100, type=int, help="Number of sequences to be generated.")
    parser.add_argument("--out", required=True, type=str, help="Output directory: the dataset's root.")
    parser.add_argument("--batch_size", default=8, type=int)
    parser.add_argument("--seed", default=0, type=int)
    ranges = parser.add_mutually_exclusive_group()
    ranges.add_argument("--bf_range", nargs=2, type=int, metavar=("LO", "HI"), default=None,
                        help="Count range of every bright-field frame (default 0 65535).")
    ranges.add_argument("--like", default=None, type=str, metavar="REAL_DIR",
                        help="A real dataset directory: bright-field count ranges are drawn from its samples.")
    parser.add_argument("--no_graph", action="store_true", help="Run the generator eagerly instead of replaying a captured graph.")
    return parser


def main(argv: Optional[Sequence[str]] = None) -> int:
    args = _parser().parse_args(argv)
    like = None
    if args.like is not None:
        from .tlfm_dataset import TFLMDatasetGAN
        like = TFLMDatasetGAN(args.like, raw=True, no_rfp=True)
    written = simulate_dataset(args.load_checkpoint, args.samples, args.out, batch_size=args.batch_size,
                               bf_range=None if args.bf_range is None else tuple(args.bf_range), like=like, seed=args.seed,
                               use_graph=not args.no_graph)
    print(f"{written} sequences in {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
