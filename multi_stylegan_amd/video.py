"""The interpolation video: frame-wise baseline JPEG on the device, a Motion-JPEG AVI on the host.

scripts/gan_latent_space_interpolation.py ends in ``ffmpeg -r 60 ... -pix_fmt yuv420p`` over its 1 600 PNG frames.  Here the
frames never become files: ``msg_jpeg_encode`` (csrc/jpeg.hip) turns a batch of the uint8 sheets ``sample_sheets`` composes into
the entropy-coded JPEG scans, the compressed bytes -- not 3 B per pixel -- cross to the host, and ``MjpegWriter`` puts the JFIF
headers around each and appends it to one RIFF AVI (``MJPG``), which every player opens and ffmpeg transcodes to H.264 without a
frame directory in between.

* ``jpeg_tables``   the Annex K quantisation tables under the IJG quality scaling;
* ``jpeg_encode``   a batch of pictures -> the scans and their offsets: device tensors through ``msg_jpeg_encode``, CPU tensors
  through the host statement of the same format (numpy float64 transform, a plain entropy coder: slow, for tests and machines
  without a GPU);
* ``jpeg_file``     a scan -> a complete JFIF file;
* ``MjpegWriter``   the AVI, written behind the caller's back as ``SheetWriter`` writes its PNG files;
* ``interpolation_video``  ``interpolation_frames`` with the writer at its end.

Command line: ``python -m multi_stylegan_amd.video --load_checkpoint F --out FILE.avi ...``.
"""
import ctypes
import queue
import struct
import threading
from typing import Optional, Sequence, Union

import numpy
import torch

from . import _lib
from .samples import _Ring, _device_of, _generator_of, interpolation_latents, sample_sheets

# ---------------------------------------------------------------------------------------------------------------- tables
#: T.81 Annex K.1 / K.2, natural (row-major) order
_K1_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
            80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
            95, 98, 112, 100, 103, 99)
_K2_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
              99, 99, 99) + (99,) * 32
#: T.81 Annex K.3.3 as (BITS, HUFFVAL): DC luminance, DC chrominance, AC luminance, AC chrominance
_AC_LUMA_VALUES = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALUES = bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_SPECS = (
    (0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), bytes(range(12))),
    (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d)), _AC_LUMA_VALUES),
    (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), bytes(range(12))),
    (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)), _AC_CHROMA_VALUES),
)                                                      # (Tc << 4 | Th, BITS, HUFFVAL), in the order jpeg_file writes them


def _zigzag():
    """Natural index of every position of the zigzag sequence (T.81 figure A.6), walked."""
    order, r, c = [], 0, 0
    for _ in range(64):
        order.append(r * 8 + c)
        if (r + c) % 2 == 0:
            if c == 7:
                r += 1
            elif r == 0:
                c += 1
            else:
                r, c = r - 1, c + 1
        elif r == 7:
            c += 1
        elif c == 0:
            r += 1
        else:
            r, c = r + 1, c - 1
    return numpy.array(order)


ZIGZAG = _zigzag()


def _codes(bits: bytes, values: bytes):
    """T.81 Annex C: {symbol: (code, length)}."""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[values[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return table


def jpeg_tables(quality: int = 90) -> numpy.ndarray:
    """uint16 ``[2, 64]``: the luminance and the chrominance table of T.81 Annex K.1 / K.2 in natural (row-major) order under
    the IJG scaling -- ``s = 5000 / quality`` below 50, ``200 - 2 quality`` from 50 on, ``(t s + 50) // 100`` clamped to
    1 .. 255.  Quality 50 is Annex K itself, 100 is all ones."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"quality {quality} is outside 1 .. 100")
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    base = numpy.array([_K1_LUMA, _K2_CHROMA], dtype=numpy.int64)
    return numpy.clip((base * scale + 50) // 100, 1, 255).astype(numpy.uint16)


def _check_tables(tables) -> numpy.ndarray:
    tables = numpy.ascontiguousarray(tables, dtype=numpy.uint16)
    if tables.shape != (2, 64) or tables.min() < 1 or tables.max() > 255:
        raise ValueError("expected [2, 64] quantisation tables with entries 1 .. 255")
    return tables


# ------------------------------------------------------------------------------------------------- the host statement
def _dct_matrix() -> numpy.ndarray:
    u, j = numpy.arange(8)[:, None], numpy.arange(8)[None, :]
    d = 0.5 * numpy.cos((2 * j + 1) * u * numpy.pi / 16)
    d[0] /= numpy.sqrt(2.0)
    return d


def _coefficients_host(rgb: numpy.ndarray, tables: numpy.ndarray) -> numpy.ndarray:
    """uint8 ``[N, H, W, 3]`` -> int16 ``[N, MR, MC, 6, 64]``: the arithmetic include/msg_hip.h fixes for msg_jpeg_encode, in
    float64."""
    N, H, W, _ = rgb.shape
    MR, MC = -(-H // 16), -(-W // 16)
    x = numpy.pad(rgb, ((0, 0), (0, 16 * MR - H), (0, 16 * MC - W), (0, 0)), mode="edge").astype(numpy.float64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    luma = 0.299 * r + 0.587 * g + 0.114 * b - 128.0
    cb = (-0.168736 * r - 0.331264 * g + 0.5 * b + 128.0) - 128.0
    cr = (0.5 * r - 0.418688 * g - 0.081312 * b + 128.0) - 128.0
    d = _dct_matrix()

    def blocks(plane, table):                                                # [N, h, w] -> [N, h / 8, w / 8, 64] zigzag
        n, h, w = plane.shape
        tiles = plane.reshape(n, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4)
        c = numpy.einsum("vy,nrcyx,ux->nrcvu", d, tiles, d).reshape(n, h // 8, w // 8, 64)
        q = numpy.sign(c) * numpy.floor(numpy.abs(c) / table.astype(numpy.float64) + 0.5)
        q[..., 1:] = numpy.clip(q[..., 1:], -1023, 1023)
        return q[..., ZIGZAG].astype(numpy.int16)

    def mean2(plane):
        n, h, w = plane.shape
        return plane.reshape(n, h // 2, 2, w // 2, 2).mean(axis=(2, 4))

    y = blocks(luma, tables[0]).reshape(N, MR, 2, MC, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(N, MR, MC, 4, 64)
    return numpy.concatenate([y, blocks(mean2(cb), tables[1])[:, :, :, None], blocks(mean2(cr), tables[1])[:, :, :, None]], axis=3)


_HUFFMAN = {spec[0]: _codes(spec[1], spec[2]) for spec in HUFFMAN_SPECS}


def _scan_host(coef: numpy.ndarray) -> bytes:
    """One frame's ``[MR, MC, 6, 64]`` coefficients -> its entropy-coded segment: one restart interval per MCU row, DC prediction
    from 0 in each, 1-bits up to the byte, FF -> FF 00, ``FF D0+(r mod 8)`` behind every interval but the last."""
    MR = coef.shape[0]
    out = bytearray()
    for r in range(MR):
        acc, nbits = 0, 0
        pred = [0, 0, 0]
        for mcu in coef[r].tolist():
            for k, block in enumerate(mcu):
                comp = max(0, k - 3)
                dc, ac = _HUFFMAN[0x00 if comp == 0 else 0x01], _HUFFMAN[0x10 if comp == 0 else 0x11]
                diff = max(-2047, min(2047, block[0] - pred[comp]))
                pred[comp] = block[0]
                size = abs(diff).bit_length()
                code, length = dc[size]
                acc = (acc << length | code) << size | ((diff if diff >= 0 else diff - 1) & ((1 << size) - 1))
                nbits += length + size
                run = 0
                for v in block[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run >= 16:
                        code, length = ac[0xf0]
                        acc, nbits, run = acc << length | code, nbits + length, run - 16
                    size = abs(v).bit_length()
                    code, length = ac[run << 4 | size]
                    acc = (acc << length | code) << size | ((v if v >= 0 else v - 1) & ((1 << size) - 1))
                    nbits += length + size
                    run = 0
                if run:
                    code, length = ac[0x00]
                    acc, nbits = acc << length | code, nbits + length
        pad = -nbits % 8
        acc, nbits = acc << pad | ((1 << pad) - 1), nbits + pad
        out += acc.to_bytes(nbits // 8, "big").replace(b"\xff", b"\xff\x00")
        if r != MR - 1:
            out += bytes((0xff, 0xd0 + r % 8))
    return bytes(out)


# ---------------------------------------------------------------------------------------------------------------- encode
def _check_sheets(sheets: torch.Tensor) -> None:
    if sheets.dtype != torch.uint8 or sheets.ndim != 4 or sheets.shape[-1] != 3 or min(sheets.shape) < 1:
        raise ValueError(f"expected uint8 [N >= 1, H >= 1, W >= 1, 3] pictures, got {sheets.dtype} {tuple(sheets.shape)}")


def _encode_device(sheets: torch.Tensor, tables: numpy.ndarray, want_coef: bool = False):
    """One ``msg_jpeg_encode`` call on the current stream -> (scan buffer at its full capacity, offsets, coef or None), all on
    the device; nothing is synchronised, so only ``offsets[N]`` bytes of the buffer mean anything."""
    sheets = sheets.contiguous()
    dev = _lib.require_gpu(sheets)
    N, H, W, _ = sheets.shape
    lib = _lib.lib()
    capacity, workspace = ctypes.c_longlong(0), lib.msg_jpeg_workspace(N, H, W)
    _lib.check(lib.msg_jpeg_scan_capacity(N, H, W, ctypes.addressof(capacity)), "msg_jpeg_scan_capacity")
    payload = torch.empty(capacity.value, dtype=torch.uint8, device=dev)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    coef = torch.empty((N, -(-H // 16), -(-W // 16), 6, 64), dtype=torch.int16, device=dev) if want_coef else None
    with _lib.on_device(dev):
        ws = _lib.scratch_ptr((workspace + 3) // 4, dev)
        with _lib.kernel_clock.span(("jpeg_encode", (N, "x", H, "x", W)), sheets.numel()):
            _lib.check(lib.msg_jpeg_encode(sheets.data_ptr(), tables.ctypes.data, _lib.ptr(coef), payload.data_ptr(),
                                           offsets.data_ptr(), N, H, W, ws, _lib.stream_of(dev)), "msg_jpeg_encode")
    return payload, offsets, coef


def jpeg_encode(sheets: torch.Tensor, quality: int = 90, return_coef: bool = False):
    """uint8 ``[N, H, W, 3]`` pictures (what ``sample_sheets(...).reshape(N, C * H, T * W, 3)`` gives) -> ``(payload, offsets)``:
    ``payload[offsets[n]:offsets[n + 1]]`` is the entropy-coded segment of picture ``n`` as a baseline 4:2:0 JPEG with the
    ``jpeg_tables(quality)`` tables, the Annex K Huffman tables and one restart interval per row of 16 x 16 MCUs;
    ``jpeg_file`` makes a file of it.  ``return_coef=True`` adds the quantised coefficients, int16 ``[N, MR, MC, 6, 64]``.

    Device tensors take one ``msg_jpeg_encode`` call on the current stream (this convenience form then waits for it, to learn
    the payload's length; ``MjpegWriter`` does not); CPU tensors take the host statement of the same format."""
    _check_sheets(sheets)
    tables = jpeg_tables(quality)
    if sheets.is_cuda:
        payload, offsets, coef = _encode_device(sheets, tables, return_coef)
        payload = payload[:int(offsets[-1].item())]
    else:
        coef_host = _coefficients_host(sheets.numpy(), tables)
        segments = [_scan_host(frame) for frame in coef_host]
        payload = torch.frombuffer(bytearray(b"".join(segments)), dtype=torch.uint8)
        offsets = torch.tensor([0] + list(numpy.cumsum([len(s) for s in segments])), dtype=torch.int64)
        coef = torch.from_numpy(coef_host)
    return (payload, offsets, coef) if return_coef else (payload, offsets)


def _segment(marker: int, body: bytes) -> bytes:
    return struct.pack(">BBH", 0xff, marker, len(body) + 2) + body


def jpeg_file(segment: bytes, height: int, width: int, tables) -> bytes:
    """The JFIF file around one entropy-coded segment of ``jpeg_encode``: SOI, APP0 (JFIF 1.01), DQT for both tables in zigzag
    order, SOF0 (Y 2 x 2 on table 0, Cb / Cr 1 x 1 on table 1), the four Annex K DHT, DRI (one MCU row), SOS, the segment, EOI."""
    tables = _check_tables(tables)
    if not (1 <= int(height) <= 65535 and 1 <= int(width) <= 65535):
        raise ValueError(f"a JPEG picture is 1 .. 65535 pixels a side, got {height} x {width}")
    parts = [b"\xff\xd8", _segment(0xe0, b"JFIF\0" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))]
    parts += [_segment(0xdb, bytes((k,)) + tables[k][ZIGZAG].astype(numpy.uint8).tobytes()) for k in range(2)]
    parts.append(_segment(0xc0, struct.pack(">BHHB", 8, int(height), int(width), 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1))))
    parts += [_segment(0xc4, bytes((kind,)) + bits + values) for kind, bits, values in HUFFMAN_SPECS]
    parts.append(_segment(0xdd, struct.pack(">H", -(-int(width) // 16))))
    parts.append(_segment(0xda, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))
    return b"".join(parts) + bytes(segment) + b"\xff\xd9"


# ------------------------------------------------------------------------------------------------------------ the writer
#: what a RIFF AVI without OpenDML extensions can address
AVI_LIMIT = 2 ** 31 - 1
_HEADER_BYTES = 224                                    # RIFF .. the first chunk of movi; the fourcc "movi" is at 220


class _Slot(_Ring):
    """A buffer of the ring and the pinned words its batch's offsets arrive in."""

    def __init__(self):
        super().__init__()
        self.offsets: Optional[torch.Tensor] = None


class MjpegWriter:
    """``with MjpegWriter(path, fps=60, quality=90) as video: video.submit(sheets)``: a Motion-JPEG AVI written behind the
    caller's back.

    ``submit`` takes a uint8 batch ``[N, H, W, 3]``.  A device batch is encoded by one ``msg_jpeg_encode`` call enqueued on the
    caller's stream, which is never synchronised; a copy stream that waits for it brings the ``N + 1`` offsets to pinned memory,
    and the worker thread, once it has read the total there, issues the second copy itself: exactly the used bytes of the
    payload.  A CPU batch is encoded by the host statement on the calling thread.  One worker thread wraps every segment into a
    JFIF file and appends the frames in submission order.  ``depth`` pinned buffers bound the memory: with all of them in use
    ``submit`` blocks.  A worker's exception is kept and re-raised by the next ``submit`` or by ``close()``, as in
    ``SheetWriter``.

    The file is a RIFF AVI: ``hdrl`` with ``avih`` and one ``strl`` (``strh`` ``vids`` / ``MJPG``, ``strf`` a 24-bit
    BITMAPINFOHEADER with compression ``MJPG``), ``movi`` with word-padded ``00dc`` chunks, ``idx1``; sizes and frame counts
    are patched by ``close()``.  The first ``submit`` fixes the picture size and another size raises ``ValueError``, as does a
    ``submit`` after ``close()``.  A batch that would take the file past ``AVI_LIMIT`` (2^31 - 1 bytes; OpenDML is not
    written) is not appended and raises ``ValueError`` -- on the ``submit`` or ``close()`` that follows where the sizes were
    only known to the worker.

    ``frames``: appended so far; ``bytes_copied``: device-to-host bytes so far (offsets and payload)."""

    def __init__(self, path: str, fps: float = 60, quality: int = 90, depth: int = 2):
        if not fps > 0:
            raise ValueError(f"fps {fps} is not positive")
        self.path, self.fps, self.quality, self.depth = str(path), fps, int(quality), max(1, int(depth))
        self.tables = jpeg_tables(quality)
        self.limit = AVI_LIMIT
        self.frames = 0
        self.bytes_copied = 0
        self.size = None                                                     # (height, width) once the first batch came
        self._file = open(self.path, "wb")
        self._index = []                                                     # (offset from "movi", length) per frame
        self._position = _HEADER_BYTES
        self._slots = [_Slot() for _ in range(self.depth)]
        self._free: "queue.Queue[_Slot]" = queue.Queue()
        for slot in self._slots:
            self._free.put(slot)
        self._jobs: "queue.Queue" = queue.Queue()
        self._lock = threading.Lock()
        self._error: Optional[BaseException] = None
        self._copy_stream: Optional[torch.cuda.Stream] = None
        self._closed = False
        self._thread = threading.Thread(target=self._work, name="msg-mjpeg", daemon=True)
        self._thread.start()

    # -- the file
    def _header(self) -> bytes:
        height, width = self.size or (0, 0)
        scale, rate = (1, int(self.fps)) if float(self.fps).is_integer() else (1000, int(round(self.fps * 1000)))
        largest = max((length for _, length in self._index), default=0)
        movi = self._position - _HEADER_BYTES
        avih = struct.pack("<14I", int(round(1e6 * scale / rate)), 0, 0, 0x10, self.frames, 0, 1, largest, width, height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIIIHHHH", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, self.frames, largest,
                           0xffffffff, 0, 0, 0, width, height)
        strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        riff = 4 + 8 + len(hdrl) + 8 + 4 + movi + 8 + 16 * len(self._index)
        head = (b"RIFF" + struct.pack("<I", riff) + b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl
                + b"LIST" + struct.pack("<I", 4 + movi) + b"movi")
        assert len(head) == _HEADER_BYTES
        return head

    def _append(self, segments: Sequence[bytes]) -> None:
        """Worker thread: the frames of one batch, all or none (the 2 GiB rule)."""
        height, width = self.size
        files = [jpeg_file(segment, height, width, self.tables) for segment in segments]
        grown = sum(8 + len(f) + len(f) % 2 for f in files)
        if self._position + grown + 8 + 16 * (len(self._index) + len(files)) > self.limit:
            raise ValueError(f"{self.path}: {len(files)} more frames would take the file past {self.limit} bytes "
                             "(a RIFF AVI without OpenDML extensions ends there)")
        if self.frames == 0:
            self._file.write(self._header())                                 # placeholder sizes: close() patches them
        for f in files:
            self._file.write(b"00dc" + struct.pack("<I", len(f)) + f + b"\0" * (len(f) % 2))
            self._index.append((self._position - _HEADER_BYTES + 4, len(f)))
            self._position += 8 + len(f) + len(f) % 2
            self.frames += 1

    def _work(self) -> None:
        while True:
            job = self._jobs.get()
            if job is None:
                return
            slot, count, payload, offsets_host, segments = job
            try:
                if segments is None:                                         # a device batch: its offsets are on their way
                    slot.event.synchronize()
                    bounds = offsets_host.tolist()
                    total = bounds[count]
                    with torch.cuda.device(payload.device), torch.cuda.stream(self._copy_stream):
                        staged = slot.fit(total, True)
                        staged.copy_(payload[:total], non_blocking=True)
                        done = torch.cuda.Event()
                        done.record(self._copy_stream)
                    done.synchronize()
                    self.bytes_copied += total + 8 * (count + 1)
                    data = staged.numpy()
                    segments = [data[bounds[k]:bounds[k + 1]].tobytes() for k in range(count)]
                self._append(segments)
            except BaseException as exc:                                     # kept for the next submit() / close()
                with self._lock:
                    if self._error is None:
                        self._error = exc
            finally:
                del payload
                self._free.put(slot)

    def _raise_pending(self) -> None:
        with self._lock:
            error, self._error = self._error, None
        if error is not None:
            raise error

    # -- the public surface
    def submit(self, sheets: torch.Tensor) -> None:
        if self._closed:
            raise ValueError("MjpegWriter is closed")
        _check_sheets(sheets)
        size = (int(sheets.shape[1]), int(sheets.shape[2]))
        if self.size is not None and size != self.size:
            raise ValueError(f"this video is {self.size[0]} x {self.size[1]}, got frames of {size[0]} x {size[1]}")
        if max(size) > 65535:
            raise ValueError(f"a JPEG picture is at most 65535 pixels a side, got {size[0]} x {size[1]}")
        self._raise_pending()
        slot = self._free.get()                                              # blocks while the ring is full
        try:
            self._raise_pending()                                            # (what failed while this call waited)
            count = int(sheets.shape[0])
            if sheets.is_cuda:
                payload, offsets, _ = _encode_device(sheets, self.tables)
                if self._copy_stream is None or self._copy_stream.device != sheets.device:
                    self._copy_stream = torch.cuda.Stream(device=sheets.device)
                if slot.offsets is None or slot.offsets.numel() < count + 1:
                    slot.offsets = torch.empty(count + 1, dtype=torch.int64, pin_memory=True)
                offsets_host = slot.offsets[:count + 1]
                self._copy_stream.wait_stream(torch.cuda.current_stream(sheets.device))   # the encoder's launches
                with torch.cuda.stream(self._copy_stream):
                    offsets_host.copy_(offsets, non_blocking=True)
                    slot.event = torch.cuda.Event()
                    slot.event.record(self._copy_stream)
                offsets.record_stream(self._copy_stream)
                payload.record_stream(self._copy_stream)
                job = (slot, count, payload, offsets_host, None)
            else:
                payload, offsets = jpeg_encode(sheets, self.quality)
                data, bounds = payload.numpy(), offsets.tolist()
                job = (slot, count, None, None, [data[bounds[k]:bounds[k + 1]].tobytes() for k in range(count)])
        except BaseException:
            self._free.put(slot)
            raise
        self.size = size                                                     # the first batch that is accepted fixes it
        self._jobs.put(job)

    def close(self) -> None:
        """Append what is queued, stop the worker, patch the sizes and the frame counts, write ``idx1``; re-raise a worker's
        exception."""
        if not self._closed:
            self._closed = True
            self._jobs.put(None)
            self._thread.join()
            try:
                if self.frames == 0:
                    self._file.write(self._header())
                self._file.write(b"idx1" + struct.pack("<I", 16 * len(self._index))
                                 + b"".join(struct.pack("<4sIII", b"00dc", 0x10, at, length) for at, length in self._index))
                self._file.seek(0)
                self._file.write(self._header())
            finally:
                self._file.close()
        self._raise_pending()

    def __enter__(self) -> "MjpegWriter":
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


# ------------------------------------------------------------------------------------------------------------- the output
@torch.no_grad()
def interpolation_video(generator_or_checkpoint, path: str, anchors: Union[int, torch.Tensor] = 16, steps_per_anchor: int = 100,
                        batch_size: int = 32, seed: Optional[int] = None, use_graph: bool = True, fps: float = 60,
                        quality: int = 90, anchors_are_latents: bool = False) -> int:
    """scripts/gan_latent_space_interpolation.py:28-59 with its video as the output: the frames ``interpolation_frames`` writes
    as ``frame_{index:05d}.png`` -- the same latents, batches and padding rule, the same
    ``sample_sheets(...).reshape(B, C * H, T * W, 3)`` pictures -- as the frames of one Motion-JPEG AVI at ``path``.  Returns
    their number.  ``anchors_are_latents=True``: ``[K, D]`` or ``[K, n, D]`` W / W+ anchors, as there."""
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
    with MjpegWriter(path, fps=fps, quality=quality) as video:
        for first in range(0, total, batch_size):
            z = latents[first:first + batch_size]
            count = z.shape[0]
            if count < batch_size:
                z = torch.cat([z, z[-1:].expand(batch_size - count, *z.shape[1:])], dim=0)
            sheets = sample_sheets(sampler(z.contiguous()))
            B, C, H, TW, _ = sheets.shape
            video.submit(sheets.reshape(B, C * H, TW, 3)[:count])
    return total


# ----------------------------------------------------------------------------------------------------------- command line
def main(argv: Optional[Sequence[str]] = None) -> int:
    import argparse
    parser = argparse.ArgumentParser(prog="python -m multi_stylegan_amd.video", description=__doc__.split("\n\n")[0])
    parser.add_argument("--load_checkpoint", default="checkpoint_100.pt", type=str, help="Path to checkpoint to be loaded.")
    parser.add_argument("--out", required=True, type=str, help="The AVI file.")
    parser.add_argument("--anchors", default=16, type=int)
    parser.add_argument("--steps", default=100, type=int, help="Interpolation steps per anchor.")
    parser.add_argument("--batch", default=32, type=int)
    parser.add_argument("--seed", default=None, type=int)
    parser.add_argument("--fps", default=60, type=float)
    parser.add_argument("--quality", default=90, type=int)
    args = parser.parse_args(argv)
    frames = interpolation_video(args.load_checkpoint, args.out, anchors=args.anchors, steps_per_anchor=args.steps,
                                 batch_size=args.batch, seed=args.seed, fps=args.fps, quality=args.quality)
    print(f"{frames} frames in {args.out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
