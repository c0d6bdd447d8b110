"""Pictures of what the generator produces: per-epoch prediction sheets, sample sequences and latent-space interpolation frames.

The reference writes all three through ``torchvision.utils.save_image``: ``Logger.save_prediction`` (multi_stylegan/misc.py:132-166,
called at model_wrapper.py:166-174), scripts/get_gan_samples.py:30-60 and scripts/gan_latent_space_interpolation.py:28-59.  Each
picture is composed there as a chain of elementwise passes (``repeat_interleave``, two zero fills, ``cat``, ``permute``), copied to
the host as fp32 RGB planes (12 B per pixel, synchronously) and quantised and PNG-encoded on the calling thread.  Here:

* ``sample_sheets`` composes and quantises a whole batch in one pass (csrc/sample_sheet.hip: ``msg_sample_sheet``; 4 B or 2 B read
  and 3 B written per pixel); CPU tensors take one torch statement of the same arithmetic;
* ``write_png`` is an 8-bit truecolour PNG writer on ``zlib`` and ``struct`` (no PIL, cv2 or torchvision);
* ``SheetWriter`` moves the uint8 sheets through a ring of pinned buffers on a copy stream and encodes them on worker threads
  while the generator already produces the next batch;
* ``save_prediction`` / ``epoch_sample_dump`` / ``dump_samples`` / ``interpolation_frames`` are the three outputs, with the
  reference's file names.  The interpolation as a video, encoded on the device: video.py.

Command line: ``python -m multi_stylegan_amd.samples samples|interpolate --load_checkpoint F --out DIR ...``.
"""
import os
import queue
import struct
import threading
import zlib
from typing import Callable, List, Optional, Sequence, Union

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

#: three bits per channel (bit 0 red, bit 1 green, bit 2 blue): bright field on all planes, GFP green, RFP red -- misc.py:140-154
DEFAULT_TINTS = 7 | 2 << 3 | 1 << 6
CHANNEL_NAMES = ("bf", "gfp", "rfp")
MAX_WORKERS = 16


# ------------------------------------------------------------------------------------------------------------ composition
def _check_tints(tints: Optional[int], channels: int) -> int:
    if tints is None:
        return DEFAULT_TINTS & ((1 << 3 * channels) - 1)
    tints = int(tints)
    if tints < 0 or tints >> (3 * channels):
        raise ValueError(f"tints {tints:#o} has bits above bit {3 * channels - 1} ({channels} channel(s), three bits each)")
    return tints


def _sheets_host(x: torch.Tensor, tints: int) -> torch.Tensor:
    """The host's one definition of the composition: torchvision's ``save_image(normalize=False)`` quantisation,
    ``trunc(min(max(fl(fl(x * 255) + 0.5), 0), 255))`` with NaN -> 0, on fp32 ``[B, C, T, H, W]``, laid out ``[B, C, H, T*W, 3]``
    with each channel on the colour planes its tint bits name."""
    B, C, T, H, W = x.shape
    planes = torch.tensor([[(tints >> (3 * c + k)) & 1 for k in range(3)] for c in range(C)], dtype=torch.uint8)
    return ((x * 255.0).add(0.5).nan_to_num(nan=0.0).clamp(0.0, 255.0).to(torch.uint8)
            .permute(0, 1, 3, 2, 4).reshape(B, C, H, T * W, 1) * planes.view(1, C, 1, 1, 3))


def sample_sheets(sequence: torch.Tensor, tints: Optional[int] = None) -> torch.Tensor:
    """``[B, C, T, H, W]`` (C = 1 .. 3) -> uint8 ``[B, C, H, T*W, 3]``, interleaved RGB.

    ``out[b, c]`` is the sheet ``save_image(nrow=T, padding=0)`` writes for channel ``c`` of sample ``b``: its T frames side by
    side (misc.py:156-166, get_gan_samples.py:55-60).  ``out[b].reshape(C * H, T * W, 3)`` is the interpolation frame: the
    channels' sheets stacked top to bottom (gan_latent_space_interpolation.py:46-55).  ``tints``: three bits per channel at bits
    ``3c .. 3c+2`` (red, green, blue; a cleared bit writes 0); default bright field 7, GFP 2, RFP 1.

    Device tensors (float32 / bfloat16; anything else is cast to float32) go through ``msg_sample_sheet`` on the current stream,
    CPU tensors through a torch statement of the same arithmetic: the results are equal byte for byte."""
    if sequence.ndim != 5 or not 1 <= sequence.shape[1] <= 3:
        raise ValueError(f"expected [B, C <= 3, T, H, W] frames, got {tuple(sequence.shape)}")
    B, C, T, H, W = sequence.shape
    tints = _check_tints(tints, C)
    sequence = sequence.detach()
    if not sequence.is_cuda:
        return _sheets_host(sequence.to(torch.float32), tints)
    if sequence.dtype not in (torch.float32, torch.bfloat16):
        sequence = sequence.to(torch.float32)
    sequence = sequence.contiguous()
    dev = _lib.require_gpu(sequence)
    out = torch.empty((B, C, H, T * W, 3), dtype=torch.uint8, device=dev)
    if sequence.numel() == 0:
        return out
    lib = _lib.lib()
    with _lib.on_device(dev):
        with _lib.kernel_clock.span(("sample_sheet", sequence.dtype), sequence.numel() * (sequence.element_size() + 3.0)):
            _lib.check(lib.msg_sample_sheet(sequence.data_ptr(), out.data_ptr(), _lib.dtype_code(sequence), B, C, T, H, W, tints,
                                            _lib.stream_of(dev)), "msg_sample_sheet")
    return out


# -------------------------------------------------------------------------------------------------------------------- PNG
_PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xffffffff)


def write_png(path_or_file, array, compress_level: int = 3) -> None:
    """8-bit ``[H, W, 3]`` (a uint8 numpy array or CPU tensor) -> a truecolour, non-interlaced PNG at ``path_or_file`` (a path
    or a binary file object).  Every scan line uses the Up filter (one vectorised subtraction for the picture; the sheets'
    backgrounds and their zero colour planes become runs of zeros), one IDAT chunk.  ``compress_level``: zlib's, 0 .. 9."""
    import numpy
    pixels = array.detach().cpu().numpy() if isinstance(array, torch.Tensor) else numpy.asarray(array)
    if pixels.dtype != numpy.uint8 or pixels.ndim != 3 or pixels.shape[2] != 3 or pixels.shape[0] < 1 or pixels.shape[1] < 1:
        raise ValueError(f"expected uint8 [H >= 1, W >= 1, 3] pixels, got {pixels.dtype} {tuple(pixels.shape)}")
    height, width = pixels.shape[:2]
    lines = numpy.empty((height, 1 + 3 * width), dtype=numpy.uint8)
    lines[:, 0] = 2                                                          # filter type Up: byte - byte above (mod 256)
    flat = pixels.reshape(height, 3 * width)
    lines[0, 1:] = flat[0]
    numpy.subtract(flat[1:], flat[:-1], out=lines[1:, 1:])
    data = (_PNG_SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))
            + _chunk(b"IDAT", zlib.compress(lines.tobytes(), int(compress_level))) + _chunk(b"IEND", b""))
    if hasattr(path_or_file, "write"):
        path_or_file.write(data)
    else:
        with open(path_or_file, "wb") as f:
            f.write(data)


# ----------------------------------------------------------------------------------------------------------------- writer
class _Ring:
    """One buffer of the writer's ring: host memory (page-locked when there is a GPU), the copy's event, and how many of its
    pictures are still to be written."""

    def __init__(self):
        self.buffer: Optional[torch.Tensor] = None
        self.event: Optional[torch.cuda.Event] = None
        self.pending = 0

    def fit(self, nbytes: int, pinned: bool) -> torch.Tensor:
        if self.buffer is None or self.buffer.numel() < nbytes:
            self.buffer = torch.empty(nbytes, dtype=torch.uint8, pin_memory=pinned)
        return self.buffer[:nbytes]


class SheetWriter:
    """``with SheetWriter(directory) as writer: writer.submit(names, sheets)``: PNG files written behind the caller's back.

    ``submit`` copies a uint8 batch ``[N, H, W, 3]`` (device or CPU) into one of ``depth`` host buffers -- device batches on a
    copy stream that waits for the caller's stream, which itself is never synchronised -- and returns; ``workers`` threads wait
    for the copy, encode and write ``names[k]`` (relative to ``directory``, or absolute).  When all ``depth`` buffers are in use
    ``submit`` blocks until one is free: the memory is bounded, as in ``DevicePrefetcher``.  An exception in a worker is kept
    and re-raised by the next ``submit`` or by ``close()``.  ``workers=0`` is the synchronous mode: copy, encode and write on
    the calling thread.  At most 16 workers, never derived from the machine's core count."""

    def __init__(self, directory: str, workers: int = 4, depth: int = 2, compress_level: int = 3):
        self.directory = str(directory)
        self.workers, self.depth = max(0, min(int(workers), MAX_WORKERS)), max(1, int(depth))
        self.compress_level = compress_level
        os.makedirs(self.directory, exist_ok=True)
        self._slots = [_Ring() for _ in range(self.depth)]
        self._free: "queue.Queue[_Ring]" = queue.Queue()
        for slot in self._slots:
            self._free.put(slot)
        self._jobs: "queue.Queue" = queue.Queue()
        self._lock = threading.Lock()
        self._error: Optional[BaseException] = None
        self._copy_stream: Optional[torch.cuda.Stream] = None
        self._closed = False
        self.written = 0
        self._threads = [threading.Thread(target=self._work, name=f"msg-sheet-{k}", daemon=True) for k in range(self.workers)]
        for thread in self._threads:
            thread.start()

    # -- the ring
    @property
    def outstanding(self) -> int:
        """Buffers of the ring that hold pictures not yet written."""
        return self.depth - self._free.qsize()

    def _release(self, slot: _Ring) -> None:
        with self._lock:
            slot.pending -= 1
            done = slot.pending == 0
        if done:
            self._free.put(slot)

    def _encode(self, path: str, pixels) -> None:
        write_png(path, pixels, self.compress_level)

    def _work(self) -> None:
        while True:
            job = self._jobs.get()
            if job is None:
                return
            slot, pixels, path = job
            try:
                if slot.event is not None:
                    slot.event.synchronize()                                 # the copy, not the caller's stream
                self._encode(path, pixels)
                with self._lock:
                    self.written += 1
            except BaseException as exc:                                     # kept for the next submit() / close()
                with self._lock:
                    if self._error is None:
                        self._error = exc
            finally:
                self._release(slot)

    def _raise_pending(self) -> None:
        with self._lock:
            error, self._error = self._error, None
        if error is not None:
            raise error

    # -- the public surface
    def submit(self, names: Sequence[str], sheets: torch.Tensor) -> None:
        if self._closed:
            raise RuntimeError("SheetWriter is closed")
        if sheets.dtype != torch.uint8 or sheets.ndim != 4 or sheets.shape[-1] != 3:
            raise ValueError(f"expected uint8 [N, H, W, 3] sheets, got {sheets.dtype} {tuple(sheets.shape)}")
        names = list(names)
        if len(names) != sheets.shape[0]:
            raise ValueError(f"{len(names)} file names for {sheets.shape[0]} sheets")
        self._enqueue([os.path.join(self.directory, name) for name in names], sheets)

    def _enqueue(self, paths: List[str], sheets: torch.Tensor) -> None:
        """``sheets[k]`` (a uint8 batch of any trailing shape) to ``_encode(paths[k], ...)``, through the ring."""
        self._raise_pending()
        if not paths:
            return
        if self.workers == 0:
            host = sheets.cpu().numpy()
            for path, pixels in zip(paths, host):
                self._encode(path, pixels)
                self.written += 1
            return
        slot = self._free.get()                                              # blocks while the ring is full
        try:
            self._raise_pending()                                            # (what failed while this call waited)
            staged = slot.fit(sheets.numel(), torch.cuda.is_available()).view(sheets.shape)
            if sheets.is_cuda:
                if self._copy_stream is None or self._copy_stream.device != sheets.device:
                    self._copy_stream = torch.cuda.Stream(device=sheets.device)
                current = torch.cuda.current_stream(sheets.device)
                self._copy_stream.wait_stream(current)                       # the kernels that produce the sheets
                with torch.cuda.stream(self._copy_stream):
                    staged.copy_(sheets, non_blocking=True)
                    slot.event = torch.cuda.Event()
                    slot.event.record(self._copy_stream)
                sheets.record_stream(self._copy_stream)
            else:
                slot.event = None
                staged.copy_(sheets)
            pixels = staged.numpy()
            slot.pending = len(paths)
        except BaseException:
            self._free.put(slot)
            raise
        for k, path in enumerate(paths):
            self._jobs.put((slot, pixels[k], path))

    def close(self) -> None:
        """Write what is queued, stop the workers, re-raise a worker's exception."""
        if not self._closed:
            self._closed = True
            for _ in self._threads:
                self._jobs.put(None)
            for thread in self._threads:
                thread.join()
        self._raise_pending()

    def __enter__(self) -> "SheetWriter":
        return self

    def __exit__(self, exc_type, exc, tb) -> bool:
        if exc_type is None:
            self.close()
        else:                                                                # the caller's exception is the one to report
            try:
                self.close()
            except BaseException:
                pass
        return False


# ---------------------------------------------------------------------------------------------------------- the three outputs
def save_prediction(prediction: torch.Tensor, name: str, directory: str, writer: Optional[SheetWriter] = None) -> List[str]:
    """``Logger.save_prediction`` (misc.py:132-166): ``{name}_bf_{b}.png``, ``{name}_gfp_{b}.png`` (C > 1) and ``{name}_rfp_{b}.png``
    (C > 2) in ``directory`` for every sample ``b`` of ``prediction [B, C, T, H, W]``, each the T frames side by side.  Returns the
    file names.  With a ``writer`` the files are complete once it is closed; without one they are written before this returns."""
    sheets = sample_sheets(prediction)
    B, C, H, TW, _ = sheets.shape
    names = [f"{name}_{CHANNEL_NAMES[c]}_{b}.png" for b in range(B) for c in range(C)]
    paths = [os.path.join(os.path.abspath(str(directory)), n) for n in names]
    if writer is None:
        with SheetWriter(directory, workers=0) as own:
            own.submit(paths, sheets.reshape(B * C, H, TW, 3))
    else:
        os.makedirs(str(directory), exist_ok=True)
        writer.submit(paths, sheets.reshape(B * C, H, TW, 3))
    return names


def _rank() -> int:
    return torch.distributed.get_rank() if torch.distributed.is_available() and torch.distributed.is_initialized() else 0


def epoch_sample_dump(directory: str, workers: int = 4) -> Callable:
    """The ``on_epoch_end(wrapper, epoch)`` hook of ``ModelWrapper.train`` that writes the reference's per-epoch plots
    (model_wrapper.py:147-174): ``validation_samples`` of the wrapper, then ``prediction_ema_{epoch+1}``,
    ``prediction_ema_rand_{epoch+1}``, ``prediction_{epoch+1}`` and ``prediction_rand_{epoch+1}`` through ``save_prediction``.
    Rank 0 only."""
    from .inference import validation_samples

    def on_epoch_end(wrapper, epoch: int) -> None:
        if _rank() != 0:
            return
        predictions = validation_samples(wrapper)
        with SheetWriter(directory, workers=workers) as writer:
            for key in ("prediction_ema", "prediction_ema_rand", "prediction", "prediction_rand"):
                save_prediction(predictions[key], f"{key}_{epoch + 1}", directory, writer)
    return on_epoch_end


def _generator_of(generator_or_checkpoint, device) -> nn.Module:
    """A generator as it is, or the reference's full-size generator with the ``generator_ema`` weights of a checkpoint (a path or
    the loaded dict): get_gan_samples.py:33-36."""
    if isinstance(generator_or_checkpoint, nn.Module):
        return generator_or_checkpoint
    from .config import multi_style_gan_generator_config
    from .inference import load_generator_ema
    from .multi_stylegan_generator import Generator
    return load_generator_ema(Generator(config=multi_style_gan_generator_config), generator_or_checkpoint).to(device)


def _device_of(generator_or_checkpoint) -> torch.device:
    if isinstance(generator_or_checkpoint, nn.Module):
        device = next(generator_or_checkpoint.parameters()).device
        if device.type == "cuda":
            return device
    return torch.device("cuda", torch.cuda.current_device())


@torch.no_grad()
def dump_samples(generator_or_checkpoint, samples: int, directory: str, batch_size: int = 8, use_graph: bool = True,
                 writer: Optional[SheetWriter] = None) -> int:
    """scripts/get_gan_samples.py:38-60: ``sample_bf_{i}.png`` and ``sample_gfp_{i}.png`` for ``i`` in ``range(samples)``, one latent
    per sample (``get_noise(p_mixed_noise=0)``), fresh per-layer noise -- sampled ``batch_size`` at a time through
    ``GeneratorSampler``.  Returns the number of samples."""
    from .inference import GeneratorSampler
    device = _device_of(generator_or_checkpoint)
    generator = _generator_of(generator_or_checkpoint, device)
    sampler = GeneratorSampler(generator, batch_size=batch_size, randomize_noise=True, use_graph=use_graph, device=device)
    own = SheetWriter(directory) if writer is None else None
    root = os.path.abspath(str(directory))
    os.makedirs(root, exist_ok=True)
    try:
        for first in range(0, int(samples), batch_size):
            count = min(batch_size, int(samples) - first)
            sequence = sampler(torch.randn(batch_size, generator.latent_dimensions, device=device))
            sheets = sample_sheets(sequence[:count, :2])
            n, C, H, TW, _ = sheets.shape
            names = [os.path.join(root, f"sample_{CHANNEL_NAMES[c]}_{first + b}.png") for b in range(n) for c in range(C)]
            (own or writer).submit(names, sheets.reshape(n * C, H, TW, 3))
    finally:
        if own is not None:
            own.close()
    return int(samples)


def interpolation_latents(anchors: torch.Tensor, steps_per_anchor: int = 100) -> torch.Tensor:
    """gan_latent_space_interpolation.py:37-38: ``[K, D]`` anchors -> ``[K * steps_per_anchor, D]`` latents, linearly interpolated
    along the anchor axis with ``align_corners=True`` (the first and the last latent are the first and the last anchor)."""
    return F.interpolate(anchors.permute(1, 0).unsqueeze(dim=1), size=(steps_per_anchor * anchors.shape[0]),
                         mode="linear", align_corners=True).squeeze(dim=1).permute(1, 0)


@torch.no_grad()
def interpolation_frames(generator_or_checkpoint, directory: str, anchors: Union[int, torch.Tensor] = 16,
                         steps_per_anchor: int = 100, batch_size: int = 32, seed: Optional[int] = None, use_graph: bool = True,
                         writer: Optional[SheetWriter] = None, anchors_are_latents: bool = False) -> int:
    """scripts/gan_latent_space_interpolation.py:28-59 without its ffmpeg call: ``frame_{index:05d}.png`` in ``directory`` for
    every interpolated latent, each the channels' sheets stacked top to bottom (bright field over GFP).  Returns their number.

    ``anchors``: a ``[K, D]`` tensor, or K for ``torch.randn(K, D, generator=torch.Generator().manual_seed(seed))`` drawn on the
    host (``seed=None``: the global generator).  Batches are ``batch_size`` consecutive latents, ``randomize_noise=False``; a
    trailing partial batch is padded with its last latent and the padding is not written.
    ``anchors_are_latents=True``: ``anchors`` is a ``[K, D]`` (W) or ``[K, n, D]`` (W+, e.g. ``project.project_sequences(...).latent``)
    tensor, interpolated the same way and handed to the generator with ``input_is_latent=True``."""
    from .inference import GeneratorSampler
    device = _device_of(generator_or_checkpoint)
    generator = _generator_of(generator_or_checkpoint, device)
    latent_shape = None
    if anchors_are_latents:
        if not isinstance(anchors, torch.Tensor) or anchors.ndim not in (2, 3):
            raise ValueError("anchors_are_latents=True takes [K, D] or [K, n, D] W / W+ anchors")
        latent_shape = tuple(anchors.shape[1:])
        anchors = anchors.reshape(anchors.shape[0], -1)
    if not isinstance(anchors, torch.Tensor):
        draw = None if seed is None else torch.Generator().manual_seed(int(seed))
        anchors = torch.randn(int(anchors), generator.latent_dimensions, generator=draw)
    latents = interpolation_latents(anchors.to(device=device, dtype=torch.float32), steps_per_anchor)
    total = latents.shape[0]
    if latent_shape is not None:
        latents = latents.reshape(total, *latent_shape)
    sampler = GeneratorSampler(generator, batch_size=batch_size, randomize_noise=False, use_graph=use_graph, device=device,
                               latent_shape=latent_shape)
    own = SheetWriter(directory) if writer is None else None
    root = os.path.abspath(str(directory))
    os.makedirs(root, exist_ok=True)
    try:
        for first in range(0, total, batch_size):
            z = latents[first:first + batch_size]
            count = z.shape[0]
            if count < batch_size:
                z = torch.cat([z, z[-1:].expand(batch_size - count, *z.shape[1:])], dim=0)
            sheets = sample_sheets(sampler(z.contiguous()))
            B, C, H, TW, _ = sheets.shape
            names = [os.path.join(root, f"frame_{first + b:05d}.png") for b in range(count)]
            (own or writer).submit(names, sheets.reshape(B, C * H, TW, 3)[:count])
    finally:
        if own is not None:
            own.close()
    return total


# ----------------------------------------------------------------------------------------------------------- command line
def main(argv: Optional[Sequence[str]] = None) -> int:
    import argparse
    parser = argparse.ArgumentParser(prog="python -m multi_stylegan_amd.samples", description=__doc__.split("\n\n")[0])
    sub = parser.add_subparsers(dest="command", required=True)
    s = sub.add_parser("samples", help="sample_bf_{i}.png / sample_gfp_{i}.png (scripts/get_gan_samples.py)")
    s.add_argument("--load_checkpoint", default="checkpoint_100.pt", type=str, help="Path to checkpoint to be loaded.")
    s.add_argument("--samples", default=100, type=int, help="Number of samples to be generated.")
    s.add_argument("--out", required=True, type=str, help="Output directory.")
    s.add_argument("--batch", default=8, type=int)
    i = sub.add_parser("interpolate", help="frame_{index:05d}.png (scripts/gan_latent_space_interpolation.py)")
    i.add_argument("--load_checkpoint", default="checkpoint_100.pt", type=str, help="Path to checkpoint to be loaded.")
    i.add_argument("--out", required=True, type=str, help="Output directory.")
    i.add_argument("--anchors", default=16, type=int)
    i.add_argument("--steps", default=100, type=int, help="Interpolation steps per anchor.")
    i.add_argument("--batch", default=32, type=int)
    i.add_argument("--seed", default=None, type=int)
    args = parser.parse_args(argv)
    if args.command == "samples":
        print(f"{dump_samples(args.load_checkpoint, args.samples, args.out, batch_size=args.batch)} samples in {args.out}")
    else:
        frames = interpolation_frames(args.load_checkpoint, args.out, anchors=args.anchors, steps_per_anchor=args.steps,
                                      batch_size=args.batch, seed=args.seed)
        print(f"{frames} frames in {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
