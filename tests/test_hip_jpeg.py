"""msg_jpeg_encode (csrc/jpeg.hip) on the GPU against tests/jpeg_util.py: the coefficients against the float64 statement under
the tie-band rule, the scan against the plain-Python coder fed the device's own coefficients, guards, refusals, and the
Motion-JPEG writer and interpolation_video end to end."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as ju

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0xA5


# ---------------------------------------------------------------------------------------------------------------- pictures
def noise(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def constant(H, W):
    return np.broadcast_to(np.array([200, 120, 40], dtype=np.uint8), (H, W, 3)).copy()


def checker(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.repeat((255 * ((x + y) & 1)).astype(np.uint8)[..., None], 3, axis=2)


def lone_high(H, W):
    """Grey, every 8 x 8 tile the highest basis function on mid grey: the only large coefficient is the last of the zigzag
    sequence, behind a run of zeros that takes ZRL symbols.  (One grey level of noise on top: the bare pattern's symmetry puts
    a twelfth of its coefficients exactly on a rounding tie at Q = 1.)"""
    y, x = np.mgrid[0:H, 0:W]
    v = 128 + 100 * np.cos((2 * (x % 8) + 1) * 7 * np.pi / 16) * np.cos((2 * (y % 8) + 1) * 7 * np.pi / 16)
    v = v + np.random.default_rng(4).integers(-1, 2, (H, W))
    return np.repeat(np.clip(np.round(v), 0, 255).astype(np.uint8)[..., None], 3, axis=2)


def blobs(H, W, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    field = sum(a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
                for a, cx, cy, s in zip(rng.uniform(80, 230, 8), rng.uniform(0, W, 8), rng.uniform(0, H, 8), rng.uniform(2, 7, 8)))
    return np.clip(field + 12, 0, 255).astype(np.uint8)


def grey(H, W):
    return np.repeat(blobs(H, W, 1)[..., None], 3, axis=2)


def green(H, W):
    out = np.zeros((H, W, 3), dtype=np.uint8)
    out[..., 1] = blobs(H, W, 2)
    return out


BATCHES = {"a": (noise, constant, checker), "b": (lone_high, grey, green)}


# ------------------------------------------------------------------------------------------------------------ the raw entry
def capacity(lib, N, H, W):
    """msg_jpeg_scan_capacity -> its byte count, or its status where it refuses."""
    out = ctypes.c_longlong(-12345)
    code = lib.msg_jpeg_scan_capacity(N, H, W, ctypes.addressof(out))
    assert (code == 0) == (out.value != -12345)
    return out.value if code == 0 else code


class Run:
    """One msg_jpeg_encode call into guard-filled buffers; ``shift`` offsets the rgb and scan base pointers by that many bytes."""

    def __init__(self, pictures, quality, shift=0, want_coef=True):
        from multi_stylegan_amd import _lib, video
        self.lib = _lib.lib()
        pictures = np.ascontiguousarray(pictures)
        N, H, W, _ = pictures.shape
        self.N, self.H, self.W, self.MR, self.MC = N, H, W, -(-H // 16), -(-W // 16)
        self.tables = np.ascontiguousarray(video.jpeg_tables(quality), dtype=np.uint16)
        self.capacity, self.ws_bytes = capacity(self.lib, N, H, W), self.lib.msg_jpeg_workspace(N, H, W)
        assert self.capacity > 0 and self.ws_bytes > 0
        self.rgb = torch.empty(pictures.size + 16, dtype=torch.uint8, device=DEV)
        self.rgb[shift:shift + pictures.size] = torch.from_numpy(pictures.reshape(-1)).to(DEV)
        self.scan = torch.full((self.capacity + 64 + 16,), GUARD, dtype=torch.uint8, device=DEV)
        self.offsets = torch.full((N + 1 + 4,), -0x5a5a5a5a5a5a5a5b, dtype=torch.int64, device=DEV)
        self.ncoef = N * self.MR * self.MC * 384
        self.coef = torch.full((self.ncoef + 32,), -23131, dtype=torch.int16, device=DEV) if want_coef else None   # 0xA5A5
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV)
        self.shift = shift
        assert self.rgb.data_ptr() % 16 == 0 and self.scan.data_ptr() % 16 == 0 and self.ws.data_ptr() % 16 == 0

    def call(self, **override):
        args = dict(rgb=self.rgb.data_ptr() + self.shift, qtables=self.tables.ctypes.data,
                    coef=None if self.coef is None else self.coef.data_ptr(), scan=self.scan.data_ptr() + self.shift,
                    offsets=self.offsets.data_ptr(), N=self.N, H=self.H, W=self.W, ws=self.ws.data_ptr(),
                    stream=torch.cuda.current_stream().cuda_stream)
        args.update(override)
        code = self.lib.msg_jpeg_encode(*[args[k] for k in ("rgb", "qtables", "coef", "scan", "offsets", "N", "H", "W", "ws", "stream")])
        torch.cuda.synchronize()
        return code

    def results(self):
        """-> (offsets list, payload bytes, coef [N, MR, MC, 6, 64] or None) after the guards were checked."""
        offsets = self.offsets.cpu().numpy()
        assert (offsets[self.N + 1:] == -0x5a5a5a5a5a5a5a5b).all(), "the guard behind offsets was written"
        bounds = offsets[:self.N + 1].tolist()
        assert bounds[0] == 0 and all(a < b for a, b in zip(bounds, bounds[1:])) and bounds[-1] <= self.capacity
        scan = self.scan.cpu().numpy()
        assert (scan[:self.shift] == GUARD).all() and (scan[self.shift + bounds[-1]:] == GUARD).all(), \
            "bytes of scan at or past offsets[N] (or before its base) were written"
        coef = None
        if self.coef is not None:
            c = self.coef.cpu().numpy()
            assert (c[self.ncoef:] == -23131).all(), "the guard behind coef was written"
            coef = c[:self.ncoef].reshape(self.N, self.MR, self.MC, 6, 64)
        return bounds, scan[self.shift:self.shift + bounds[-1]].tobytes(), coef

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.scan == GUARD).all()) and bool((self.offsets == -0x5a5a5a5a5a5a5a5b).all()) and \
            (self.coef is None or bool((self.coef == -23131).all()))


def verify(pictures, quality, shift, stats=None):
    """Everything one case holds; returns the payload."""
    from multi_stylegan_amd import video
    run = Run(pictures, quality, shift)
    assert run.call() == 0
    bounds, payload, coef = run.results()
    for k in range(run.N):                                                    # the cap and the band are per input
        ju.check_coefficients(coef[k:k + 1], pictures[k:k + 1], video.jpeg_tables(quality))
    segments = [ju.encode_scan(coef[k], stats) for k in range(run.N)]
    assert bounds == [0] + list(np.cumsum([len(s) for s in segments])), "offsets"
    assert payload == b"".join(segments), "scan differs from the plain coder's on the device's own coefficients"
    assert run.call() == 0 and run.results()[:2] == (bounds, payload), "two runs differ"
    bare = Run(pictures, quality, shift, want_coef=False)
    assert bare.call() == 0 and bare.results()[:2] == (bounds, payload), "coef = NULL changes the scan"
    if run.N > 1:
        alone = Run(pictures[1:2], quality, shift)
        assert alone.call() == 0
        b1, p1, c1 = alone.results()
        assert p1 == payload[bounds[1]:bounds[2]] and np.array_equal(c1[0], coef[1]), "a frame alone differs from its slice"
    return payload


SHAPES = [(8, 8), (16, 16), (17, 9), (40, 72), (145, 24)]
CASES = [(shape, batch, quality, shift) for i, shape in enumerate(SHAPES) for j, (batch, shift) in enumerate((("a", 0), ("b", 1)))
         for quality in ((50, 90, 100) if shape == (40, 72) else ((50, 90, 100)[(i + j) % 3],))]
CASES += [((40, 72), "a", 90, 1), ((40, 72), "b", 50, 0), ((17, 9), "a", 100, 1)]


@pytest.mark.parametrize("shape,batch,quality,shift", CASES)
def test_encode(shape, batch, quality, shift):
    H, W = shape
    pictures = np.stack([make(H, W) for make in BATCHES[batch]])
    stats = {}
    verify(pictures, quality, shift, stats)
    if shape == (40, 72) and batch == "a":
        assert stats["stuffed"] > 0, "the noise picture produced no FF byte: stuffing is not exercised"
    if shape == (40, 72) and batch == "b" and quality != 100:
        assert stats["zrl"] > 0, "no ZRL symbol: runs of 16 zeros are not exercised"


def test_constant_picture_is_dc_then_eob():
    run = Run(constant(40, 72)[None], 90)
    assert run.call() == 0
    _, payload, coef = run.results()
    assert (coef[..., 1:] == 0).all() and (coef[..., 0] == coef[0, 0, 0, :, 0]).all()
    assert payload == ju.encode_scan(coef[0])


def test_checkerboard_reaches_the_largest_categories():
    run = Run(checker(16, 16)[None], 100)
    assert run.call() == 0
    _, payload, coef = run.results()
    assert np.abs(coef[..., 1:]).max() >= 512                                 # category 10
    assert payload == ju.encode_scan(coef[0])


def test_one_interval_at_the_width_limit_the_header_must_admit():
    pictures = noise(16, 4096, 5)[None]
    verify(pictures, 90, 0)


def test_refusals():
    from multi_stylegan_amd import _lib
    lib = _lib.lib()
    EINVAL, EUNSUPPORTED = _lib.MSG_EINVAL, _lib.MSG_EUNSUPPORTED
    run = Run(noise(17, 9)[None], 90)
    for name in ("rgb", "qtables", "scan", "offsets", "ws"):
        assert run.call(**{name: None}) == EINVAL, name
    for name in ("N", "H", "W"):
        assert run.call(**{name: 0}) == EINVAL and run.call(**{name: -1}) == EINVAL, name
    for entry, value in ((0, 0), (63, 256), (64, 0), (127, 300)):
        tables = run.tables.copy()
        tables.reshape(-1)[entry] = value
        assert run.call(qtables=tables.ctypes.data) == EINVAL, (entry, value)
    assert run.call(ws=run.ws.data_ptr() + 4) == EINVAL and run.call(coef=run.coef.data_ptr() + 1) == EINVAL
    assert run.call(offsets=run.offsets.data_ptr() + 4) == EINVAL
    assert run.call(N=65536) == EINVAL and run.call(H=16 * 65536) == EINVAL
    limit = _lib._CONSTANTS["MSG_JPEG_MAX_WIDTH"]
    assert limit >= 4096 and run.call(W=limit + 1) == EUNSUPPORTED
    assert run.untouched(), "a refused call wrote to its outputs"
    for bad in ((0, 16, 16), (1, -1, 16), (1, 16, 0)):
        assert lib.msg_jpeg_workspace(*bad) == -1 and capacity(lib, *bad) == EINVAL
    assert lib.msg_jpeg_workspace(1, 16, 16) > 0 and capacity(lib, 1, 16, 16) > 0
    assert lib.msg_jpeg_scan_capacity(1, 16, 16, None) == EINVAL
    assert run.call() == 0                                                    # and the same buffers still serve a good call
    run.results()


# --------------------------------------------------------------------------------------------------------------- end to end
def host_psnr(pictures, quality):
    """PSNR of the host path's files, decoded by the util decoder, per picture."""
    from multi_stylegan_amd import video
    t = torch.from_numpy(np.ascontiguousarray(pictures))
    payload, offsets = video.jpeg_encode(t, quality=quality)
    data, bounds, tables = payload.numpy().tobytes(), offsets.tolist(), video.jpeg_tables(quality)
    files = [video.jpeg_file(data[bounds[k]:bounds[k + 1]], t.shape[1], t.shape[2], tables) for k in range(t.shape[0])]
    return [ju.psnr(ju.decode(f)[0], p) for f, p in zip(files, pictures)]


def test_jpeg_encode_on_device_tensors():
    from multi_stylegan_amd import video
    pictures = np.stack([grey(40, 72), green(40, 72), noise(40, 72)])
    payload, offsets, coef = video.jpeg_encode(torch.from_numpy(pictures).to(DEV), quality=90, return_coef=True)
    assert payload.is_cuda and payload.dtype == torch.uint8 and payload.numel() == int(offsets[-1]) and offsets.dtype == torch.int64
    assert coef.shape == (3, 3, 5, 6, 64) and coef.dtype == torch.int16
    coef = coef.cpu().numpy()
    assert payload.cpu().numpy().tobytes() == b"".join(ju.encode_scan(c) for c in coef)


def test_mjpeg_writer_on_device_batches(tmp_path):
    import multi_stylegan_amd as m
    pictures = np.stack([grey(40, 72), green(40, 72), noise(40, 72, 1), blobs(40, 72, 3)[..., None].repeat(3, 2), checker(40, 72),
                         constant(40, 72)])
    path = str(tmp_path / "device.avi")
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        dev = torch.from_numpy(pictures).to(DEV)
        with m.MjpegWriter(path, fps=60, quality=90) as writer:
            for first in range(0, 6, 2):
                writer.submit(dev[first:first + 2])
    info = ju.walk_avi(open(path, "rb").read())
    assert len(info["frames"]) == 6 == writer.frames and (info["height"], info["width"]) == (40, 72)
    payload = 0
    for frame, picture, floor in zip(info["frames"], pictures, host_psnr(pictures, 90)):
        rgb, _, _ = ju.decode(frame)
        got = ju.psnr(rgb, picture)
        print(f"PSNR {got:.2f} dB, host path {floor:.2f} dB")
        assert got >= floor - 0.1
        payload += len(frame) - len(m.jpeg_file(b"", 40, 72, writer.tables))
    assert writer.bytes_copied == payload + 3 * 8 * 3                         # the segments, and three offsets a batch


@pytest.fixture(scope="module")
def tiny(golden):
    """The golden tiny generator (32^2, two channels, three frames)."""
    from tools.gen_golden import TINY_G
    import multi_stylegan_amd as m
    g = m.MultiStyleGANGenerator(TINY_G)
    g.load_state_dict(golden("tiny_models").state_dict("tinyG.sd."))
    return g.to(DEV).eval().requires_grad_(False)


def test_interpolation_video(tiny, tmp_path):
    import multi_stylegan_amd as m
    path = str(tmp_path / "interpolation.avi")
    assert m.interpolation_video(tiny, path, anchors=3, steps_per_anchor=4, batch_size=5, seed=7, use_graph=False, quality=90) == 12
    info = ju.walk_avi(open(path, "rb").read())
    assert len(info["frames"]) == 12 and (info["height"], info["width"]) == (64, 96)
    anchors = torch.randn(3, tiny.latent_dimensions, generator=torch.Generator().manual_seed(7))
    latents = m.interpolation_latents(anchors.to(DEV), 4)
    want = []
    with torch.no_grad():
        for first in range(0, 12, 5):                                         # the batches of the call above, the last one padded
            z = latents[first:first + 5]
            count = z.shape[0]
            z = torch.cat([z, z[-1:].expand(5 - count, -1)], dim=0) if count < 5 else z
            want.append(m.sample_sheets(tiny(z.contiguous(), randomize_noise=False)).reshape(5, 64, 96, 3)[:count].cpu())
    want = torch.cat(want).numpy()
    for frame, picture, floor in zip(info["frames"], want, host_psnr(want, 90)):
        rgb, _, _ = ju.decode(frame)
        assert ju.psnr(rgb, picture) >= floor - 0.1
    assert len({bytes(f) for f in info["frames"]}) == 12                      # twelve different pictures
