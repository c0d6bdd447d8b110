"""Sample sheets, PNG writer and the asynchronous sheet writer on the host (multi_stylegan_amd/samples.py).  The reference's
outputs: Logger.save_prediction (multi_stylegan/misc.py:132-166), scripts/get_gan_samples.py:30-60,
scripts/gan_latent_space_interpolation.py:28-59.  tests/golden/sheets/ records what the reference's save_prediction hands to
torchvision's save_image (tools/gen_golden_sheets.py); the quantisation behind it is restated here in numpy fp32 with a
separate multiply and add.  Every comparison is byte for byte."""
import ctypes
import io
import json
import os
import threading

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import png_util

SHEETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sheets")
CHANNELS = {"bf": 0, "gfp": 1, "rfp": 2}


def quantise(x):
    """torchvision's save_image(normalize=False): mul(255), add(0.5), clamp(0, 255), to(uint8) -- numpy fp32, two roundings;
    NaN -> 0."""
    v = np.asarray(x, dtype=np.float32) * np.float32(255.0)
    v = v + np.float32(0.5)
    v = np.where(np.isnan(v), np.float32(0.0), v)
    return np.clip(v, np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def edge_values():
    """k / 255 for all k, the fp32 neighbours either side of every (k + 0.5) / 255 (where trunc steps), negative values,
    values above 1, NaN and the infinities."""
    k = np.arange(256, dtype=np.float64)
    steps = ((k + 0.5) / 255.0).astype(np.float32)
    extra = np.array([-1.0, -0.2, -1e-8, -0.0, 0.0, 1e-8, 1.0 + 1e-6, 1.2, 7.0, 3e38, -3e38, np.nan, np.inf, -np.inf], np.float32)
    return np.concatenate([(k / 255.0).astype(np.float32), steps, np.nextafter(steps, np.float32(-np.inf)),
                           np.nextafter(steps, np.float32(np.inf)), extra]).astype(np.float32)


def fixture():
    return np.load(os.path.join(SHEETS, "save_prediction.npz")), json.load(open(os.path.join(SHEETS, "manifest.json")))["cases"]


def recorded_sheet(planes):
    """What save_image(nrow=T, padding=0) writes for the recorded [T, 3, H, W] tensor: the T pictures side by side, quantised,
    [H, T*W, 3]."""
    return quantise(np.concatenate(list(planes), axis=2)).transpose(1, 2, 0)


def file_index(file_name):
    """'<name>_<bf|gfp|rfp>_<b>.png' -> (b, c)."""
    stem = file_name[:-len(".png")].split("_")
    return int(stem[-1]), CHANNELS[stem[-2]]


# ------------------------------------------------------------------------------------------------------------- write_png
def _contents(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    return {"random": rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), "zeros": np.zeros((h, w, 3), np.uint8),
            "ones": np.full((h, w, 3), 255, np.uint8)}


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (8, 48), (33, 250)])
def test_write_png_round_trips(h, w, tmp_path):
    from multi_stylegan_amd import write_png
    for name, pixels in _contents(h, w).items():
        buffer = io.BytesIO()
        write_png(buffer, pixels)
        data = buffer.getvalue()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        assert png_util.header(data) == {"width": w, "height": h, "bit_depth": 8, "colour_type": 2, "compression": 0,
                                         "filter": 0, "interlace": 0}
        parts = png_util.chunks(data)
        assert [p[0] for p in parts][0] == b"IHDR" and parts[-1][0] == b"IEND" and any(p[0] == b"IDAT" for p in parts)
        assert all(stored == computed for _, _, stored, computed in parts), name
        assert np.array_equal(png_util.decode(data), pixels), name
        path = str(tmp_path / f"{name}.png")
        write_png(path, torch.from_numpy(pixels), compress_level=9)           # a path, a tensor, another level
        assert np.array_equal(png_util.decode(open(path, "rb").read()), pixels), name


@pytest.mark.parametrize("h,w", [(1, 1), (5, 7), (8, 48), (33, 250)])
def test_write_png_is_read_by_pil(h, w):
    Image = pytest.importorskip("PIL.Image")
    from multi_stylegan_amd import write_png
    for name, pixels in _contents(h, w).items():
        buffer = io.BytesIO()
        write_png(buffer, pixels)
        buffer.seek(0)
        image = Image.open(buffer)
        assert image.mode == "RGB" and image.size == (w, h)
        assert np.array_equal(np.asarray(image), pixels), name


def test_the_tests_decoder_knows_all_five_filters():
    pixels = _contents(5, 7)["random"]
    for kind in range(5):
        data = png_util.encode_with_filter(pixels, kind)
        assert np.array_equal(png_util.decode(data), pixels), kind
    Image = pytest.importorskip("PIL.Image")
    for kind in range(5):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(png_util.encode_with_filter(pixels, kind)))), pixels), kind


def test_write_png_rejects_other_arrays():
    from multi_stylegan_amd import write_png
    for bad in (np.zeros((4, 4), np.uint8), np.zeros((4, 4, 4), np.uint8), np.zeros((4, 4, 3), np.float32), np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_png(io.BytesIO(), bad)


# --------------------------------------------------------------------------------------------------------- sample_sheets
@pytest.mark.parametrize("case", ["c1", "c2", "c3"])
def test_sample_sheets_equal_the_recorded_save_image_calls(case):
    from multi_stylegan_amd import sample_sheets
    arrays, cases = fixture()
    prediction = torch.from_numpy(arrays[f"{case}.prediction"])
    B, C, T, H, W = prediction.shape
    sheets = sample_sheets(prediction)
    assert sheets.dtype == torch.uint8 and tuple(sheets.shape) == (B, C, H, T * W, 3)
    calls = cases[case]["calls"]
    assert len(calls) == B * C and cases[case]["channels"] == C
    for k, call in enumerate(calls):
        assert call["nrow"] == T and call["padding"] == 0                    # the geometry the sheets restate
        b, c = file_index(call["file"])
        assert np.array_equal(sheets[b, c].numpy(), recorded_sheet(arrays[f"{case}.call{k}"])), call["file"]
    # the same bytes from a non-contiguous view, from bf16 (widened first) and from float64 (cast to fp32)
    assert torch.equal(sample_sheets(prediction.transpose(3, 4).contiguous().transpose(3, 4)), sheets)
    assert torch.equal(sample_sheets(prediction.bfloat16()), sample_sheets(prediction.bfloat16().float()))
    assert torch.equal(sample_sheets(prediction.double()), sheets)


def test_quantisation_edge_values():
    from multi_stylegan_amd import sample_sheets
    values = edge_values()
    pad = (-len(values)) % 16
    x = torch.from_numpy(np.concatenate([values, np.zeros(pad, np.float32)])).reshape(1, 1, 1, -1, 16)
    got = sample_sheets(x)                                                   # [1, 1, H, 16, 3], bright field: three equal planes
    want = quantise(x.numpy().reshape(-1))
    assert np.array_equal(got[0, 0, :, :, 0].numpy().reshape(-1), want)
    assert torch.equal(got[..., 0], got[..., 1]) and torch.equal(got[..., 0], got[..., 2])
    by_value = dict(zip(values.tolist()[:256], want.tolist()[:256]))
    assert list(by_value.values()) == list(range(256))                       # k / 255 -> k
    n = len(values)
    assert want[n - 3] == 0 and want[n - 2] == 255 and want[n - 1] == 0      # NaN, +inf, -inf
    # either side of a step the numpy statement decides; the two neighbours differ by at most one level, every level is hit
    below, above = want[512:768].astype(int), want[768:1024].astype(int)
    assert ((above - below) >= 0).all() and ((above - below) <= 1).all() and set(want[:1024].tolist()) == set(range(256))


def test_tints():
    from multi_stylegan_amd import sample_sheets
    from multi_stylegan_amd.samples import DEFAULT_TINTS
    assert DEFAULT_TINTS == 7 | 2 << 3 | 1 << 6
    x = torch.rand(2, 3, 2, 4, 5, generator=torch.Generator().manual_seed(1))
    q = torch.from_numpy(quantise(x.numpy())).permute(0, 1, 3, 2, 4).reshape(2, 3, 4, 10)
    default = sample_sheets(x)
    for c, planes in enumerate(((1, 1, 1), (0, 1, 0), (1, 0, 0))):
        for k in range(3):
            assert torch.equal(default[:, c, :, :, k], q[:, c] * planes[k])
    swapped = sample_sheets(x, tints=4 | 5 << 3 | 0 << 6)                    # blue; red + blue; nothing
    for c, planes in enumerate(((0, 0, 1), (1, 0, 1), (0, 0, 0))):
        for k in range(3):
            assert torch.equal(swapped[:, c, :, :, k], q[:, c] * planes[k])
    with pytest.raises(ValueError):
        sample_sheets(x[:, :2], tints=1 << 6)                                # a bit above 3 C - 1
    with pytest.raises(ValueError):
        sample_sheets(torch.zeros(1, 4, 1, 2, 2))


# ------------------------------------------------------------------------------------------------------- save_prediction
@pytest.mark.parametrize("case", ["c1", "c2", "c3"])
@pytest.mark.parametrize("workers", [None, 2])
def test_save_prediction_writes_the_reference_files(case, workers, tmp_path):
    from multi_stylegan_amd import SheetWriter, save_prediction
    arrays, cases = fixture()
    prediction = torch.from_numpy(arrays[f"{case}.prediction"])
    out = str(tmp_path / "plots")
    if workers is None:
        names = save_prediction(prediction, cases[case]["name"], out)
    else:
        with SheetWriter(out, workers=workers) as writer:
            names = save_prediction(prediction, cases[case]["name"], out, writer)
    calls = cases[case]["calls"]
    assert names == [call["file"] for call in calls]                         # the reference's names, in its order
    assert sorted(os.listdir(out)) == sorted(names)
    for k, call in enumerate(calls):
        pixels = png_util.decode(open(os.path.join(out, call["file"]), "rb").read())
        assert np.array_equal(pixels, recorded_sheet(arrays[f"{case}.call{k}"])), call["file"]


# ----------------------------------------------------------------------------------------------------------- SheetWriter
def _batches(count, n=3, h=6, w=10):
    rng = np.random.default_rng(5)
    return [torch.from_numpy(rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)) for _ in range(count)]


@pytest.mark.parametrize("workers", [0, 3])
def test_sheet_writer_with_cpu_tensors(workers, tmp_path):
    from multi_stylegan_amd import SheetWriter
    batches = _batches(5)
    with SheetWriter(str(tmp_path), workers=workers, depth=2) as writer:
        assert writer.workers == workers
        for k, batch in enumerate(batches):
            writer.submit([f"b{k}_{i}.png" for i in range(len(batch))], batch)
            batch_copy = batch.clone()
            batch.zero_()                                                    # the caller's tensor is free once submit returns
            batches[k] = batch_copy
    assert writer.written == 15 and writer.outstanding == 0
    for k, batch in enumerate(batches):
        for i in range(len(batch)):
            assert np.array_equal(png_util.decode(open(tmp_path / f"b{k}_{i}.png", "rb").read()), batch[i].numpy())
    with pytest.raises(RuntimeError):
        writer.submit(["late.png"], batches[0][:1])
    with SheetWriter(str(tmp_path), workers=99) as capped:
        assert capped.workers == 16
    with pytest.raises(ValueError):
        SheetWriter(str(tmp_path), workers=0).submit(["a.png"], batches[0])  # three sheets, one name


@pytest.mark.parametrize("workers", [0, 3])
def test_sheet_writer_reports_a_failed_write(workers, tmp_path):
    """The target's parent is a regular file: no user can write there.  Asynchronous: the worker's exception surfaces in
    close(); synchronous: in submit() itself."""
    from multi_stylegan_amd import SheetWriter
    (tmp_path / "blocked").write_bytes(b"a file, not a directory")
    batch = _batches(1)[0]
    writer = SheetWriter(str(tmp_path), workers=workers)
    if workers == 0:
        with pytest.raises(OSError):
            writer.submit([os.path.join("blocked", f"{i}.png") for i in range(3)], batch)
        writer.close()
        return
    writer.submit([os.path.join("blocked", f"{i}.png") for i in range(3)], batch)
    with pytest.raises(OSError):
        writer.close()
    assert writer.outstanding == 0                                           # the failed pictures gave their buffer back
    writer.close()                                                           # reported once


def test_sheet_writer_error_surfaces_in_the_next_submit(tmp_path):
    from multi_stylegan_amd import SheetWriter
    (tmp_path / "blocked").write_bytes(b"x")
    batch = _batches(1)[0]
    writer = SheetWriter(str(tmp_path), workers=1, depth=1)
    writer.submit([os.path.join("blocked", "0.png")], batch[:1])
    with pytest.raises(OSError):                      # depth 1: the buffer is free only once the failed picture gave it back,
        writer.submit(["never.png"], batch[:1])       # and by then its exception is there
    assert writer.outstanding == 0
    writer.submit(["fine.png"], batch[:1])            # reported once; the writer goes on
    writer.close()
    assert os.path.exists(tmp_path / "fine.png") and not os.path.exists(tmp_path / "never.png")


def test_sheet_writer_ring_is_bounded(tmp_path):
    """Twelve batches through a ring of two: never more than two buffers hold unwritten pictures, and the same two host
    buffers serve all of them."""
    from multi_stylegan_amd import SheetWriter
    seen, pointers, lock = [], set(), threading.Lock()

    class Watching(SheetWriter):
        def _encode(self, path, pixels):
            with lock:
                seen.append(self.outstanding)
                pointers.update(slot.buffer.data_ptr() for slot in self._slots if slot.buffer is not None)
            super()._encode(path, pixels)

    batches = _batches(12)
    with Watching(str(tmp_path), workers=3, depth=2) as writer:
        for k, batch in enumerate(batches):
            writer.submit([f"b{k}_{i}.png" for i in range(len(batch))], batch)
            assert writer.outstanding <= 2
    assert len(seen) == 36 and 1 <= min(seen) and max(seen) <= 2 and len(pointers) <= 2 and len(writer._slots) == 2
    assert len(os.listdir(tmp_path)) == 36
    assert np.array_equal(png_util.decode(open(tmp_path / "b11_2.png", "rb").read()), batches[11][2].numpy())


# ------------------------------------------------------------------------------------------------- interpolation_latents
def test_interpolation_latents():
    from multi_stylegan_amd import interpolation_latents
    anchors = torch.randn(4, 16, generator=torch.Generator().manual_seed(2))
    latents = interpolation_latents(anchors, steps_per_anchor=6)
    assert tuple(latents.shape) == (24, 16)
    assert torch.equal(latents[0], anchors[0]) and torch.equal(latents[-1], anchors[-1])
    literal = F.interpolate(anchors.permute(1, 0).unsqueeze(dim=1), size=(6 * 4), mode="linear",
                            align_corners=True).squeeze(dim=1).permute(1, 0)
    assert torch.equal(latents, literal)
    assert tuple(interpolation_latents(torch.randn(16, 8)).shape) == (1600, 8)


# ---------------------------------------------------------------------------------------------------------------- header
def test_entry_is_declared_and_exported():
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    build(verbose=False)
    assert "msg_sample_sheet" in _lib.declared_symbols()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "msg_sample_sheet")
    res, args = _lib._SIGNATURES["msg_sample_sheet"]
    assert res is ctypes.c_int and len(args) == 10
    assert _lib.ABI_VERSION == 5


def test_command_line_is_the_reference_scripts_flags():
    from multi_stylegan_amd import samples
    for argv in (["samples", "--out", "x", "--bogus"], ["interpolate"], []):
        with pytest.raises(SystemExit):
            samples.main(argv)
