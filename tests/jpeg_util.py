"""What the JPEG / AVI tests measure against, written from ITU T.81 and the RIFF AVI layout and not from the package:

* ``coefficients``   the arithmetic include/msg_hip.h fixes for ``msg_jpeg_encode`` -- colour, subsampling, DCT, quantisation --
  in float64 (or, for the rounding-noise estimate, in float32), with the unquantised ``c / Q`` beside the integers;
* ``encode_scan``    a plain-Python entropy coder, coefficients -> one frame's segment, which also counts ZRL symbols and
  stuffed bytes;
* ``decode``         a plain-Python baseline decoder: the headers, DQT and DHT as the file has them, restart markers,
  stuffing, IDCT, crop, JFIF inverse colour, nearest-neighbour chroma;
* ``walk_avi``       a RIFF walker for the Motion-JPEG files.
"""
import struct

import numpy as np

# ------------------------------------------------------------------------------------------------------------- T.81 tables
K1 = np.array([[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56],
               [14, 17, 22, 29, 51, 87, 80, 62], [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92],
               [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]])
K2 = np.full((8, 8), 99)
K2[:4, :4] = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

# figure A.6 as printed: the zigzag position of every (row, column)
A6 = np.array([[0, 1, 5, 6, 14, 15, 27, 28], [2, 4, 7, 13, 16, 26, 29, 42], [3, 8, 12, 17, 25, 30, 41, 43],
               [9, 11, 18, 24, 31, 40, 44, 53], [10, 19, 23, 32, 39, 45, 52, 54], [20, 22, 33, 38, 46, 51, 55, 60],
               [21, 34, 37, 47, 50, 56, 59, 61], [35, 36, 48, 49, 57, 58, 62, 63]])
NATURAL_OF_ZIGZAG = np.argsort(A6.reshape(64))          # zigzag position -> natural index

# tables K.3 - K.6 as (BITS, HUFFVAL)
_DC_VALUES = list(range(12))
_AC_LUMA = [int(x, 16) for x in """
01 02 03 00 04 11 05 12 21 31 41 06 13 51 61 07 22 71 14 32 81 91 a1 08 23 42 b1 c1 15 52 d1 f0 24 33 62 72 82 09 0a 16 17 18 19 1a
25 26 27 28 29 2a 34 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78 79
7a 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7 c8 c9
ca d2 d3 d4 d5 d6 d7 d8 d9 da e1 e2 e3 e4 e5 e6 e7 e8 e9 ea f1 f2 f3 f4 f5 f6 f7 f8 f9 fa""".split()]
_AC_CHROMA = [int(x, 16) for x in """
00 01 02 03 11 04 05 21 31 06 12 41 51 07 61 71 13 22 32 81 08 14 42 91 a1 b1 c1 09 23 33 52 f0 15 62 72 d1 0a 16 24 34 e1 25 f1 17
18 19 1a 26 27 28 29 2a 35 36 37 38 39 3a 43 44 45 46 47 48 49 4a 53 54 55 56 57 58 59 5a 63 64 65 66 67 68 69 6a 73 74 75 76 77 78
79 7a 82 83 84 85 86 87 88 89 8a 92 93 94 95 96 97 98 99 9a a2 a3 a4 a5 a6 a7 a8 a9 aa b2 b3 b4 b5 b6 b7 b8 b9 ba c2 c3 c4 c5 c6 c7
c8 c9 ca d2 d3 d4 d5 d6 d7 d8 d9 da e2 e3 e4 e5 e6 e7 e8 e9 ea f2 f3 f4 f5 f6 f7 f8 f9 fa""".split()]
ANNEX_K3 = {
    (0, 0): ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], _DC_VALUES),
    (0, 1): ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], _DC_VALUES),
    (1, 0): ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], _AC_LUMA),
    (1, 1): ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119], _AC_CHROMA),
}                                                       # (class: 0 DC / 1 AC, destination: 0 luminance / 1 chrominance)


def huffman_codes(bits, values):
    """Annex C -> {symbol: (code, length)}."""
    out, code, k = {}, 0, 0
    for length, count in enumerate(bits, start=1):
        for _ in range(count):
            out[values[k]] = (code, length)
            code += 1
            k += 1
        code *= 2
    return out


# ------------------------------------------------------------------------------------------------- the float64 statement
def coefficients(rgb, qtables, dtype=np.float64):
    """uint8 ``[N, H, W, 3]``, ``qtables [2, 64]`` natural order -> ``(coef int [N, MR, MC, 6, 64], ratio, quant)``: ``ratio`` is
    the unquantised ``c / Q`` and ``quant`` the Q of every element, both laid out like ``coef``.  Every operation is carried
    out in ``dtype``."""
    rgb = np.asarray(rgb)
    N, H, W, _ = rgb.shape
    MR, MC = (H + 15) // 16, (W + 15) // 16
    rows = np.minimum(np.arange(16 * MR), H - 1)
    cols = np.minimum(np.arange(16 * MC), W - 1)
    x = rgb[:, rows][:, :, cols].astype(dtype)
    f = lambda v: dtype(v)
    R, G, B = x[..., 0], x[..., 1], x[..., 2]
    Y = f(0.299) * R + f(0.587) * G + f(0.114) * B - f(128)
    Cb = f(-0.168736) * R + f(-0.331264) * G + f(0.5) * B + f(128) - f(128)
    Cr = f(0.5) * R + f(-0.418688) * G + f(-0.081312) * B + f(128) - f(128)
    sub = lambda p: ((p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) * f(0.25)).astype(dtype)
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    basis[0] *= np.sqrt(0.5)
    basis = basis.astype(dtype)

    def transform(plane, table):                        # -> ratio [N, h / 8, w / 8, 64] zigzag, and Q likewise
        n, h, w = plane.shape
        b = plane.reshape(n, h // 8, 8, w // 8, 8).transpose(0, 1, 3, 2, 4)
        rowpass = np.matmul(b, basis.T)                  # along x
        c = np.matmul(basis, rowpass).astype(dtype)      # along y: c[v, u]
        q = np.asarray(table, dtype=dtype).reshape(8, 8)
        ratio = (c / q).reshape(n, h // 8, w // 8, 64)[..., NATURAL_OF_ZIGZAG]
        return ratio, np.broadcast_to(q.reshape(64)[NATURAL_OF_ZIGZAG], ratio.shape)

    def mcus(luma, cb, cr):                             # [N, 2 MR, 2 MC, 64], [N, MR, MC, 64] x 2 -> [N, MR, MC, 6, 64]
        y = luma.reshape(N, MR, 2, MC, 2, 64).transpose(0, 1, 3, 2, 4, 5).reshape(N, MR, MC, 4, 64)
        return np.concatenate([y, cb[:, :, :, None], cr[:, :, :, None]], axis=3)

    parts = [transform(Y, qtables[0]), transform(sub(Cb), qtables[1]), transform(sub(Cr), qtables[1])]
    ratio = mcus(*[p[0] for p in parts])
    quant = mcus(*[p[1] for p in parts])
    coef = np.sign(ratio) * np.floor(np.abs(ratio) + dtype(0.5))
    coef[..., 1:] = np.clip(coef[..., 1:], -1023, 1023)
    return coef.astype(np.int64), ratio, quant


def check_coefficients(got, rgb, qtables, floor=2.0 ** -12, scale=8.0, cap=0.02):
    """``got`` against the float64 statement under the tie-band rule (the one tests/test_hip_modulate.py uses for its
    reductions): every difference is at most 1 in magnitude and occurs only where the float64 ``c / Q`` lies within
    ``max(scale * e32, floor) / Q`` of a rounding tie, ``e32`` being the largest |float32 - float64| of a numpy float32
    evaluation of the same formulas on this input; at most ``cap`` of an input's coefficients may lie in its band, which is
    asserted before the band is used.  (``floor`` = 2^-12: two fp32 units at the largest possible coefficient, 1024.)
    -> (differences, share of the coefficients in the band, e32)."""
    want, ratio, quant = coefficients(rgb, qtables)
    _, ratio32, _ = coefficients(rgb, qtables, np.float32)
    e32 = float(np.abs((ratio32.astype(np.float64) - ratio) * quant).max())
    half = max(scale * e32, floor) / quant
    tie = np.abs(np.abs(ratio) - np.floor(np.abs(ratio)) - 0.5)            # distance of |c / Q| from the nearest n + 1/2
    band = tie <= half
    share = float(band.mean())
    print(f"e32 {e32:.2e}, {100 * share:.3f} % of the coefficients within the tie band")
    assert share <= cap, f"{100 * share:.2f} % of the coefficients lie in the tie band: the input does not test the rounding"
    got = np.asarray(got).astype(np.int64)
    assert got.shape == want.shape, (got.shape, want.shape)
    diff = got != want
    assert np.abs(got - want).max() <= 1, f"a coefficient is off by {np.abs(got - want).max()}"
    assert not (diff & ~band).any(), f"{int((diff & ~band).sum())} coefficients differ outside the tie band"
    return int(diff.sum()), share, e32


# ------------------------------------------------------------------------------------------------------ the entropy coder
class _Bits:
    def __init__(self):
        self.text = []

    def put(self, value, length):
        if length:
            self.text.append(format(value, "0%db" % length))


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def encode_scan(coef, stats=None):
    """``coef [MR, MC, 6, 64]`` (zigzag, DC not differenced) -> the frame's segment between the SOS header and EOI, as
    include/msg_hip.h states it (Annex K.3 tables, Ri = MC).  ``stats`` (a dict) receives the ZRL symbols and the stuffed bytes."""
    tables = {key: huffman_codes(*spec) for key, spec in ANNEX_K3.items()}
    coef = np.asarray(coef)
    MR = coef.shape[0]
    out = bytearray()
    zrl = stuffed = 0
    for r in range(MR):
        bits = _Bits()
        last = {0: 0, 1: 0, 2: 0}
        for mcu in coef[r].tolist():
            for k, block in enumerate(mcu):
                comp = 0 if k < 4 else k - 3
                dest = 0 if comp == 0 else 1
                diff = block[0] - last[comp]
                diff = -2047 if diff < -2047 else 2047 if diff > 2047 else diff
                last[comp] = block[0]
                size, extra = _magnitude(diff)
                bits.put(*tables[(0, dest)][size])
                bits.put(extra, size)
                zeros = 0
                for v in block[1:]:
                    if v == 0:
                        zeros += 1
                        continue
                    while zeros > 15:
                        bits.put(*tables[(1, dest)][0xF0])
                        zeros -= 16
                        zrl += 1
                    size, extra = _magnitude(v)
                    bits.put(*tables[(1, dest)][zeros * 16 + size])
                    bits.put(extra, size)
                    zeros = 0
                if zeros:
                    bits.put(*tables[(1, dest)][0x00])
        text = "".join(bits.text)
        text += "1" * (-len(text) % 8)
        for i in range(0, len(text), 8):
            byte = int(text[i:i + 8], 2)
            out.append(byte)
            if byte == 0xFF:
                out.append(0)
                stuffed += 1
        if r != MR - 1:
            out += bytes([0xFF, 0xD0 + r % 8])
    if stats is not None:
        stats["zrl"] = stats.get("zrl", 0) + zrl
        stats["stuffed"] = stats.get("stuffed", 0) + stuffed
    return bytes(out)


# ------------------------------------------------------------------------------------------------------------ the decoder
class _Reader:
    """The bits of one restart interval, the stuffed zeros removed."""

    def __init__(self, data):
        self.bits = "".join(format(b, "08b") for b in data.replace(b"\xff\x00", b"\xff"))
        self.at = 0

    def take(self, n):
        if self.at + n > len(self.bits):
            raise ValueError("the interval ends inside a symbol")
        v = int(self.bits[self.at:self.at + n], 2) if n else 0
        self.at += n
        return v

    def symbol(self, lookup):
        code, length = 0, 0
        while length < 16:
            code, length = code * 2 + self.take(1), length + 1
            if (code, length) in lookup:
                return lookup[(code, length)]
        raise ValueError("no Huffman code matches")


def _extend(v, size):
    return v if size == 0 or v >> (size - 1) else v - (1 << size) + 1


def decode(data):
    """A baseline JFIF file as the package writes them (three components, 4:2:0, interleaved, restart intervals) ->
    ``(rgb uint8 [H, W, 3], coef int [MR, MC, 6, 64] zigzag as read from the stream, luma uint8 [H, W])``.  Tables are the
    file's own DQT / DHT segments."""
    if data[:2] != b"\xff\xd8":
        raise ValueError("no SOI")
    at, quant, huff, frame, restart, scan_components = 2, {}, {}, None, 0, None
    while True:
        if data[at] != 0xFF:
            raise ValueError(f"no marker at {at}")
        marker = data[at + 1]
        (length,) = struct.unpack(">H", data[at + 2:at + 4])
        body = data[at + 4:at + 2 + length]
        at += 2 + length
        if marker == 0xDB:
            while body:
                if body[0] >> 4:
                    raise ValueError("16-bit quantisation table in a baseline file")
                quant[body[0] & 15] = np.array(list(body[1:65]))[np.argsort(NATURAL_OF_ZIGZAG)]   # -> natural order
                body = body[65:]
        elif marker == 0xC4:
            while body:
                counts = list(body[1:17])
                values = list(body[17:17 + sum(counts)])
                huff[(body[0] >> 4, body[0] & 15)] = {v: k for k, v in huffman_codes(counts, values).items()}
                body = body[17 + sum(counts):]
        elif marker == 0xC0:
            precision, H, W, count = struct.unpack(">BHHB", body[:6])
            frame = [tuple(body[6 + 3 * i:9 + 3 * i]) for i in range(count)]
            if precision != 8 or [(c[0], c[1]) for c in frame] != [(1, 0x22), (2, 0x11), (3, 0x11)]:
                raise ValueError(f"not an 8-bit 4:2:0 frame: {precision}, {frame}")
        elif marker == 0xDD:
            (restart,) = struct.unpack(">H", body)
        elif marker == 0xDA:
            scan_components = [tuple(body[1 + 2 * i:3 + 2 * i]) for i in range(body[0])]
            if tuple(body[1 + 2 * body[0]:]) != (0, 63, 0):
                raise ValueError("not a sequential scan")
            break
        elif marker in (0xC1, 0xC2, 0xC3, 0xC9, 0xCA):
            raise ValueError("not a baseline frame")
    if data[-2:] != b"\xff\xd9":
        raise ValueError("no EOI")
    MR, MC = (H + 15) // 16, (W + 15) // 16
    if restart != MC:
        raise ValueError(f"restart interval {restart}, expected one MCU row ({MC})")
    # split at RSTm: inside entropy-coded data FF is followed by 00 or by a marker
    body, pieces, start, i = data[at:-2], [], 0, 0
    while i < len(body) - 1:
        if body[i] == 0xFF and body[i + 1] != 0:
            if body[i + 1] != 0xD0 + len(pieces) % 8:
                raise ValueError(f"marker FF{body[i + 1]:02X} where RST{len(pieces) % 8} belongs")
            pieces.append(body[start:i])
            start = i = i + 2
        else:
            i += 2 if body[i] == 0xFF else 1
    pieces.append(body[start:])
    if len(pieces) != MR:
        raise ValueError(f"{len(pieces)} restart intervals for {MR} MCU rows")
    selectors = {c: (td_ta >> 4, td_ta & 15) for c, td_ta in scan_components}
    coef = np.zeros((MR, MC, 6, 64), dtype=np.int64)
    for r, piece in enumerate(pieces):
        reader, last = _Reader(piece), {1: 0, 2: 0, 3: 0}
        for m in range(MC):
            for k in range(6):
                comp = 1 if k < 4 else k - 2
                dc, ac = huff[(0, selectors[comp][0])], huff[(1, selectors[comp][1])]
                size = reader.symbol(dc)
                last[comp] += _extend(reader.take(size), size)
                coef[r, m, k, 0] = last[comp]
                pos = 1
                while pos < 64:
                    sym = reader.symbol(ac)
                    run, size = sym >> 4, sym & 15
                    if size == 0:
                        if run != 15:
                            break                           # EOB
                        pos += 16
                        continue
                    pos += run
                    if pos > 63:
                        raise ValueError("a run leaves the block")
                    coef[r, m, k, pos] = _extend(reader.take(size), size)
                    pos += 1
        rest = reader.bits[reader.at:]
        if len(rest) > 7 or "0" in rest:
            raise ValueError(f"interval {r} ends with {rest!r}, expected up to seven 1-bits")
    k = np.arange(8)
    basis = np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16) * 0.5
    basis[0] *= np.sqrt(0.5)

    def plane(blocks, table):                           # [rows, cols, 64] zigzag -> samples [8 rows, 8 cols]
        natural = np.zeros(blocks.shape)
        natural[..., NATURAL_OF_ZIGZAG] = blocks
        c = (natural * table).reshape(blocks.shape[0], blocks.shape[1], 8, 8)
        s = np.matmul(basis.T, np.matmul(c, basis)) + 128.0
        return s.transpose(0, 2, 1, 3).reshape(8 * blocks.shape[0], 8 * blocks.shape[1])

    tq = {c[0]: quant[c[2]] for c in frame}
    luma_blocks = coef[:, :, :4].reshape(MR, MC, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * MR, 2 * MC, 64)
    Y = plane(luma_blocks, tq[1])[:H, :W]
    Cb = np.repeat(np.repeat(plane(coef[:, :, 4], tq[2]), 2, axis=0), 2, axis=1)[:H, :W] - 128.0
    Cr = np.repeat(np.repeat(plane(coef[:, :, 5], tq[3]), 2, axis=0), 2, axis=1)[:H, :W] - 128.0
    rgb = np.stack([Y + 1.402 * Cr, Y - 0.344136 * Cb - 0.714136 * Cr, Y + 1.772 * Cb], axis=-1)
    to_byte = lambda a: np.clip(np.floor(a + 0.5), 0, 255).astype(np.uint8)
    return to_byte(rgb), coef, to_byte(Y)


def psnr(a, b):
    err = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return float("inf") if err == 0 else 10 * np.log10(255.0 ** 2 / err)


# -------------------------------------------------------------------------------------------------------- the RIFF walker
def _chunks(data, start, end):
    at, out = start, []
    while at < end:
        if at + 8 > end:
            raise ValueError(f"a chunk header crosses the end of its list at {at}")
        kind, size = data[at:at + 4], struct.unpack("<I", data[at + 4:at + 8])[0]
        if at + 8 + size > end:
            raise ValueError(f"chunk {kind!r} at {at} ({size} bytes) crosses the end of its list")
        out.append((kind, at + 8, size))
        at += 8 + size + size % 2
        if size % 2 and (at > end or data[at - 1] != 0):
            raise ValueError(f"chunk {kind!r} of odd size {size} is not padded with a zero byte")
    if at != end:
        raise ValueError("the chunks do not fill their list")
    return out


def walk_avi(data):
    """Checks a Motion-JPEG AVI: every chunk size and the padding, the frame counts of ``avih`` and ``strh``, the stream format,
    and that every ``idx1`` entry points at a ``00dc`` chunk of the stated length.  -> dict(frames=[bytes], width, height,
    scale, rate)."""
    if data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("not a RIFF AVI")
    if struct.unpack("<I", data[4:8])[0] != len(data) - 8:
        raise ValueError(f"RIFF size {struct.unpack('<I', data[4:8])[0]} in a file of {len(data)} bytes")
    top = _chunks(data, 12, len(data))
    if [c[0] for c in top] != [b"LIST", b"LIST", b"idx1"] or data[top[0][1]:top[0][1] + 4] != b"hdrl" \
            or data[top[1][1]:top[1][1] + 4] != b"movi":
        raise ValueError(f"expected LIST hdrl, LIST movi, idx1; found {[c[0] for c in top]}")
    hdrl = _chunks(data, top[0][1] + 4, top[0][1] + top[0][2])
    if [c[0] for c in hdrl] != [b"avih", b"LIST"] or hdrl[0][2] != 56 or data[hdrl[1][1]:hdrl[1][1] + 4] != b"strl":
        raise ValueError("hdrl does not hold avih (56 bytes) and one strl")
    avih = struct.unpack("<14I", data[hdrl[0][1]:hdrl[0][1] + 56])
    strl = _chunks(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    if [c[0] for c in strl] != [b"strh", b"strf"] or strl[0][2] != 56 or strl[1][2] != 40:
        raise ValueError("strl does not hold strh (56 bytes) and strf (40 bytes)")
    strh = struct.unpack("<4s4sIHHIIIIIIII4H", data[strl[0][1]:strl[0][1] + 56])
    strf = struct.unpack("<IiiHH4sIiiII", data[strl[1][1]:strl[1][1] + 40])
    if strh[0] != b"vids" or strh[1] != b"MJPG" or strf[0] != 40 or strf[3] != 1 or strf[4] != 24 or strf[5] != b"MJPG":
        raise ValueError(f"not a 24-bit MJPG video stream: {strh[:2]}, {strf}")
    movi_at = top[1][1]                                  # the fourcc "movi": idx1 offsets count from here
    movi = _chunks(data, movi_at + 4, movi_at + top[1][2])
    if any(c[0] != b"00dc" for c in movi):
        raise ValueError("movi holds something other than 00dc chunks")
    frames = len(movi)
    if avih[4] != frames or strh[9] != frames:
        raise ValueError(f"{frames} frames in movi, avih says {avih[4]}, strh says {strh[9]}")
    if avih[6] != 1 or not avih[3] & 0x10:
        raise ValueError("avih: one stream and AVIF_HASINDEX expected")
    if (avih[8], avih[9]) != (strf[1], strf[2]) or tuple(strh[15:17]) != (strf[1], strf[2]):
        raise ValueError("avih, strh and strf disagree about the picture size")
    if strh[6] == 0 or abs(avih[0] - 1e6 * strh[6] / strh[7]) > 1:
        raise ValueError("dwMicroSecPerFrame does not match dwScale / dwRate")
    if top[2][2] != 16 * frames:
        raise ValueError(f"idx1 holds {top[2][2]} bytes for {frames} frames")
    for i, (kind, start, size) in enumerate(movi):
        fourcc, flags, offset, length = struct.unpack("<4sIII", data[top[2][1] + 16 * i:top[2][1] + 16 * i + 16])
        if fourcc != b"00dc" or movi_at + offset != start - 8 or length != size or not flags & 0x10:
            raise ValueError(f"idx1 entry {i} ({fourcc!r}, {offset}, {length}) does not name the chunk at {start - 8} ({size})")
    return {"frames": [data[s:s + n] for _, s, n in movi], "width": strf[1], "height": strf[2], "scale": strh[6], "rate": strh[7]}
