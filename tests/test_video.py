"""The host side of the interpolation video (multi_stylegan_amd/video.py): quantisation tables, the host statement of the
JPEG format against tests/jpeg_util.py and PIL, the Motion-JPEG AVI container.  No GPU."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as ju

import multi_stylegan_amd as m
from multi_stylegan_amd import _lib, video


def gradient(H, W):
    y, x = np.mgrid[0:H, 0:W]
    return np.stack([255 * x / max(W - 1, 1), 255 * y / max(H - 1, 1), 255 - 127 * (x + y) / max(H + W - 2, 1)],
                    axis=-1).astype(np.uint8)


def sheet_like(H, W, seed=0):
    """Grey top half over pure-green bottom half, smooth blobs on a dark background: what an interpolation frame holds."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    field = sum(a * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * s * s))
                for a, cx, cy, s in zip(rng.uniform(80, 230, 12), rng.uniform(0, W, 12), rng.uniform(0, H, 12), rng.uniform(3, 9, 12)))
    v = np.clip(field + 12, 0, 255).astype(np.uint8)
    out = np.repeat(v[..., None], 3, axis=2)
    out[H // 2:, :, 0] = 0
    out[H // 2:, :, 2] = 0
    return out


def noise(H, W, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def files_of(pictures, quality):
    """[N, H, W, 3] uint8 -> the JFIF files of the host path, and its coefficients."""
    t = torch.from_numpy(np.ascontiguousarray(pictures))
    payload, offsets, coef = video.jpeg_encode(t, quality=quality, return_coef=True)
    data, bounds = payload.numpy().tobytes(), offsets.tolist()
    tables = video.jpeg_tables(quality)
    return [video.jpeg_file(data[bounds[k]:bounds[k + 1]], t.shape[1], t.shape[2], tables) for k in range(t.shape[0])], coef.numpy()


# ------------------------------------------------------------------------------------------------------------------ tables
def test_tables_follow_annex_k_and_the_ijg_scaling():
    t50 = video.jpeg_tables(50)
    assert t50.dtype == np.uint16 and t50.shape == (2, 64)
    assert np.array_equal(t50[0].reshape(8, 8), ju.K1) and np.array_equal(t50[1].reshape(8, 8), ju.K2)
    assert np.array_equal(video.jpeg_tables(100), np.ones((2, 64)))
    for q in (1, 2, 10, 25, 75, 90, 99):
        t = video.jpeg_tables(q)
        assert t.min() >= 1 and t.max() <= 255
    assert video.jpeg_tables(1).max() == 255 and np.array_equal(video.jpeg_tables(75)[0][:3], [8, 6, 5])   # libjpeg's quality 75
    for bad in (0, 101, -3):
        with pytest.raises(ValueError):
            video.jpeg_tables(bad)


def test_zigzag_and_huffman_tables_are_those_of_t81():
    assert np.array_equal(video.ZIGZAG, ju.NATURAL_OF_ZIGZAG)
    by_kind = {spec[0]: spec for spec in video.HUFFMAN_SPECS}
    for (cls, dest), (bits, values) in ju.ANNEX_K3.items():
        kind, b, v = by_kind[cls << 4 | dest]
        assert list(b) == bits and list(v) == values and sum(bits) == len(values)


# -------------------------------------------------------------------------------------- host encode -> file -> our decoder
@pytest.mark.parametrize("shape", [(8, 8), (16, 16), (17, 9), (40, 72)])
@pytest.mark.parametrize("quality", [50, 90, 100])
def test_host_path_round_trips_the_coefficients(shape, quality):
    H, W = shape
    pictures = np.stack([noise(H, W, 1), gradient(H, W), sheet_like(H, W)])
    files, coef = files_of(pictures, quality)
    assert coef.shape == (3, -(-H // 16), -(-W // 16), 6, 64)
    # two float64 evaluations of one statement: they may part only at an exact tie (integer pixels and tables produce some)
    ju.check_coefficients(coef, pictures, video.jpeg_tables(quality), floor=1e-9, scale=0.0)
    for k, data in enumerate(files):
        rgb, read, _ = ju.decode(data)
        assert rgb.shape == (H, W, 3)
        assert np.array_equal(read, coef[k])                                  # what the stream says, before any IDCT


def test_host_scan_equals_the_plain_coder_with_zrl_stuffing_and_restart_wrap():
    # 145 rows: ten intervals, RST7 is followed by RST0; noise at quality 100: long codes and FF bytes; a lone high coefficient: ZRL
    pictures = noise(145, 24, 3)[None]
    payload, offsets, coef = video.jpeg_encode(torch.from_numpy(pictures), quality=100, return_coef=True)
    stats = {}
    assert payload.numpy().tobytes() == ju.encode_scan(coef[0].numpy(), stats) and stats["stuffed"] > 0
    assert offsets.tolist() == [0, payload.numel()]
    sparse = np.zeros((1, 1, 6, 64), dtype=np.int64)
    sparse[0, 0, :, 40] = 3
    sparse[0, 0, 5, 63] = -1
    stats = {}
    assert video._scan_host(sparse) == ju.encode_scan(sparse, stats) and stats["zrl"] >= 12


# ---------------------------------------------------------------------------------------------------------------- PIL
def test_against_pil():
    """PIL (libjpeg) opens every file; its pixels and the util decoder's differ by at most 2 grey levels (measured: 1); and the
    PSNR against the source, decoded by PIL, is at most 0.5 dB below PIL's own encode with the same tables and 4:2:0 -- measured at
    quality 90, 128 x 192: gradient 48.47 dB against 48.01 dB, sheet-like 47.39 dB against 45.82 dB.  libjpeg's standard Huffman
    tables, read from a file of its own, are those this package writes."""
    Image = pytest.importorskip("PIL.Image")
    H, W, quality = 128, 192, 90
    tables = video.jpeg_tables(quality)
    grey = np.repeat(sheet_like(H, W)[:H // 2, :, :1], 3, axis=2)
    cases = {"gradient": gradient(H, W), "sheet": sheet_like(H, W), "grey": grey, "noise": noise(40, 72), "odd": gradient(17, 9)}
    buffer = io.BytesIO()
    Image.fromarray(cases["noise"]).save(buffer, "JPEG", quality=90)          # not optimised: libjpeg's standard tables
    data, at, found = buffer.getvalue(), 2, {}
    while data[at + 1] != 0xDA:
        length = int.from_bytes(data[at + 2:at + 4], "big")
        body = data[at + 4:at + 2 + length]
        while data[at + 1] == 0xC4 and body:
            count = sum(body[1:17])
            found[(body[0] >> 4, body[0] & 15)] = (list(body[1:17]), list(body[17:17 + count]))
            body = body[17 + count:]
        at += 2 + length
    assert found == ju.ANNEX_K3
    for name, picture in cases.items():
        (data,), _ = files_of(picture[None], quality)
        with Image.open(io.BytesIO(data)) as im:
            im.load()
            assert im.size == (picture.shape[1], picture.shape[0]) and im.mode == "RGB"
            theirs = np.asarray(im)
        ours, _, luma = ju.decode(data)
        if name == "grey":                                                    # constant chroma: the whole picture compares
            diff = np.abs(theirs.astype(int) - ours.astype(int)).max()
        else:                                                                 # PIL upsamples chroma its own way: Y only, which
            with Image.open(io.BytesIO(data)) as im:                          # libjpeg hands out unconverted on request
                im.draft("YCbCr", im.size)
                assert im.mode == "YCbCr"
                diff = np.abs(np.asarray(im)[..., 0].astype(int) - luma.astype(int)).max()
        print(f"{name}: PIL's decode and ours differ by at most {diff} grey levels")
        assert diff <= 2, (name, diff)
        if name in ("gradient", "sheet"):
            buffer = io.BytesIO()
            Image.fromarray(picture).save(buffer, "JPEG", qtables=[tables[0][video.ZIGZAG].tolist(), tables[1][video.ZIGZAG].tolist()],
                                          subsampling=2)
            with Image.open(io.BytesIO(buffer.getvalue())) as im:
                reference = ju.psnr(np.asarray(im.convert("RGB")), picture)
            mine = ju.psnr(theirs, picture)
            print(f"{name}: PSNR {mine:.2f} dB (ours, decoded by PIL) against {reference:.2f} dB (PIL's own encode)")
            assert mine >= reference - 0.5, (name, mine, reference)


# ----------------------------------------------------------------------------------------------------------- the container
@pytest.mark.parametrize("shape", [(8, 8), (17, 9), (40, 72)])
def test_avi_container(tmp_path, shape):
    H, W = shape
    pictures = np.stack([noise(H, W, k) if k % 2 else sheet_like(H, W, k) for k in range(5)])
    path = str(tmp_path / "video.avi")
    with m.MjpegWriter(path, fps=60, quality=90) as writer:
        writer.submit(torch.from_numpy(pictures[:2]))
        writer.submit(torch.from_numpy(pictures[2:]))
    assert writer.frames == 5 and writer.bytes_copied == 0                    # (host batches copy nothing)
    data = open(path, "rb").read()
    info = ju.walk_avi(data)
    assert (info["height"], info["width"], info["rate"] / info["scale"]) == (H, W, 60) and len(info["frames"]) == 5
    files, _ = files_of(pictures, 90)
    assert info["frames"] == files                                            # in submission order
    for k, frame in enumerate(info["frames"]):
        rgb, _, _ = ju.decode(frame)
        assert rgb.shape == (H, W, 3)


def test_avi_without_frames_and_fractional_rate(tmp_path):
    path = str(tmp_path / "empty.avi")
    m.MjpegWriter(path, fps=29.97).close()
    info = ju.walk_avi(open(path, "rb").read())
    assert info["frames"] == [] and (info["scale"], info["rate"]) == (1000, 29970)


def test_writer_refusals(tmp_path):
    a, b = torch.from_numpy(noise(16, 16)[None]), torch.from_numpy(noise(16, 24)[None])
    with m.MjpegWriter(str(tmp_path / "a.avi")) as writer:
        writer.submit(a)
        with pytest.raises(ValueError, match="16 x 16"):
            writer.submit(b)
        with pytest.raises(ValueError):
            writer.submit(a.to(torch.float32))
    with pytest.raises(ValueError, match="closed"):
        writer.submit(a)
    assert len(ju.walk_avi(open(str(tmp_path / "a.avi"), "rb").read())["frames"]) == 1


def test_the_2_gib_rule(tmp_path):
    a = torch.from_numpy(noise(16, 16)[None])
    path = str(tmp_path / "full.avi")
    writer = m.MjpegWriter(path)
    writer.submit(a)
    probe = str(tmp_path / "probe.avi")
    with m.MjpegWriter(probe) as p:
        p.submit(a)
    writer.limit = os.path.getsize(probe) + 10                                # room for one frame and not for a second
    with pytest.raises(ValueError, match="past"):
        writer.submit(a)
        writer.close()
    writer.close()                                                            # the file is still a whole AVI, one frame long
    assert len(ju.walk_avi(open(path, "rb").read())["frames"]) == 1
    fresh = m.MjpegWriter(probe)
    assert video.AVI_LIMIT == 2 ** 31 - 1 and fresh.limit == video.AVI_LIMIT
    fresh.close()


def test_worker_exception_is_reraised(tmp_path, monkeypatch):
    a = torch.from_numpy(noise(16, 16)[None])
    writer = m.MjpegWriter(str(tmp_path / "broken.avi"))

    def fail(segment, height, width, tables):
        raise OSError("disk on fire")
    monkeypatch.setattr(video, "jpeg_file", fail)
    writer.submit(a)
    with pytest.raises(OSError, match="disk on fire"):
        writer.submit(a)
        writer.close()
    writer.close()


# ------------------------------------------------------------------------------------------------------------------- ABI
def test_abi_and_exports():
    assert _lib.ABI_VERSION == 5
    for name, args, res in (("msg_jpeg_workspace", 3, _lib._L), ("msg_jpeg_scan_capacity", 4, _lib._I), ("msg_jpeg_encode", 10, _lib._I)):
        assert name in _lib.declared_symbols() and name in _lib._SIGNATURES
        assert _lib._SIGNATURES[name][0] is res and len(_lib._SIGNATURES[name][1]) == args
    assert _lib._CONSTANTS["MSG_JPEG_MAX_WIDTH"] >= 4096
    for name in ("jpeg_tables", "jpeg_encode", "jpeg_file", "MjpegWriter", "interpolation_video"):
        assert name in m.__all__ and getattr(m, name) is getattr(video, name)
