"""A small PNG decoder for the tests, independent of the code under test: 8-bit truecolour, non-interlaced, all five filter
types, ``zlib`` and ``struct`` only (PNG specification, second edition: sections 5 "Datastream structure", 9 "Filtering")."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


def chunks(data: bytes):
    """[(type, payload, stored crc, computed crc)] of a PNG datastream; raises on a broken structure."""
    assert data[:8] == SIGNATURE, "not a PNG signature"
    out, at = [], 8
    while at < len(data):
        (length,), kind = struct.unpack(">I", data[at:at + 4]), data[at + 4:at + 8]
        payload = data[at + 8:at + 8 + length]
        assert len(payload) == length, "truncated chunk"
        (stored,) = struct.unpack(">I", data[at + 8 + length:at + 12 + length])
        out.append((kind, payload, stored, zlib.crc32(kind + payload) & 0xffffffff))
        at += 12 + length
    assert at == len(data) and out and out[0][0] == b"IHDR" and out[-1][0] == b"IEND", "chunk order"
    return out


def header(data: bytes):
    """IHDR as a dict."""
    kind, payload = chunks(data)[0][:2]
    names = ("width", "height", "bit_depth", "colour_type", "compression", "filter", "interlace")
    return dict(zip(names, struct.unpack(">IIBBBBB", payload)))


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else (b if pb <= pc else c)


def decode(data: bytes) -> np.ndarray:
    """The pixels [H, W, 3] uint8 of an 8-bit RGB PNG; every chunk's CRC is verified on the way."""
    parts = chunks(data)
    assert all(stored == computed for _, _, stored, computed in parts), "chunk CRC"
    head = header(data)
    assert (head["bit_depth"], head["colour_type"], head["compression"], head["filter"], head["interlace"]) == (8, 2, 0, 0, 0)
    width, height, bpp = head["width"], head["height"], 3
    raw = zlib.decompress(b"".join(payload for kind, payload, _, _ in parts if kind == b"IDAT"))
    stride = 1 + bpp * width
    assert len(raw) == height * stride, "scan line data"
    image = np.zeros((height, bpp * width), dtype=np.uint8)
    previous = [0] * (bpp * width)
    for y in range(height):
        kind, line = raw[y * stride], list(raw[y * stride + 1:(y + 1) * stride])
        assert 0 <= kind <= 4, "filter type"
        if kind == 2:                                   # Up needs no left neighbour: a whole line at once
            line = [(v + u) & 0xff for v, u in zip(line, previous)]
        for x in range(len(line) if kind in (1, 3, 4) else 0):
            left = line[x - bpp] if x >= bpp else 0
            up = previous[x]
            upper_left = previous[x - bpp] if x >= bpp else 0
            predictor = (0, left, up, (left + up) // 2, _paeth(left, up, upper_left))[kind]
            line[x] = (line[x] + predictor) & 0xff
        image[y] = line
        previous = line
    return image.reshape(height, width, bpp)


def encode_with_filter(pixels: np.ndarray, kind: int) -> bytes:
    """A valid PNG of ``pixels`` whose scan lines all use filter ``kind`` -- only for checking this decoder against a second
    decoder (PIL) on the filter types the package's writer does not produce."""
    height, width, bpp = pixels.shape
    flat = pixels.reshape(height, bpp * width).astype(int)
    lines = bytearray()
    for y in range(height):
        lines.append(kind)
        for x in range(bpp * width):
            left = flat[y, x - bpp] if x >= bpp else 0
            up = flat[y - 1, x] if y else 0
            upper_left = flat[y - 1, x - bpp] if y and x >= bpp else 0
            predictor = (0, left, up, (left + up) // 2, _paeth(left, up, upper_left))[kind]
            lines.append((flat[y, x] - predictor) & 0xff)

    def chunk(name, payload):
        return struct.pack(">I", len(payload)) + name + payload + struct.pack(">I", zlib.crc32(name + payload) & 0xffffffff)
    return (SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(bytes(lines))) + chunk(b"IEND", b""))
