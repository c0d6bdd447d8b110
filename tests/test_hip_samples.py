"""The device-side sheet composition (csrc/sample_sheet.hip: msg_sample_sheet) and the outputs built on it
(multi_stylegan_amd/samples.py): Logger.save_prediction (multi_stylegan/misc.py:132-166, model_wrapper.py:166-174),
scripts/get_gan_samples.py:30-60, scripts/gan_latent_space_interpolation.py:28-59.  The kernel is held to the host's torch
statement of the same arithmetic (which tests/test_samples.py holds to the recorded reference calls and to numpy) byte for byte."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import png_util
from test_samples import edge_values, fixture

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(2, 2, 3, 8, 16),        # vector path, one 16-pixel group per row
          (1, 3, 2, 5, 12),        # scalar path
          (3, 1, 1, 7, 48),        # vector path
          (2, 2, 3, 64, 80),       # several workgroups per sheet
          (1, 2, 3, 33, 250)]      # scalar path


def _input(shape, dtype, seed=0):
    """Values over [-0.2, 1.2] with the quantisation's edge values (every k / 255, both neighbours of every step, NaN and the
    infinities among them) at the front, as many as fit, the special values always."""
    x = torch.rand(shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * 1.4 - 0.2
    flat = x.reshape(-1)
    edges = torch.from_numpy(edge_values())
    edges = torch.cat([edges[-14:], edges[:-14]])[:flat.numel()]
    flat[:edges.numel()] = edges
    return x.to(dtype)


def _entry(x_dev, tints, fill, out_offset=0):
    """msg_sample_sheet itself on a device tensor [B, C, T, H, W], into an output pre-filled with ``fill``."""
    from multi_stylegan_amd import _lib
    B, C, T, H, W = x_dev.shape
    n = B * C * H * T * W * 3
    backing = torch.full((n + out_offset,), fill, dtype=torch.uint8, device=DEV)
    out = backing[out_offset:]
    rc = _lib.lib().msg_sample_sheet(x_dev.data_ptr(), out.data_ptr(), _lib.dtype_code(x_dev), B, C, T, H, W, tints,
                                     _lib.stream_of(x_dev.device))
    assert rc == _lib.MSG_OK
    return out.view(B, C, H, T * W, 3).cpu()


def _default_tints(C):
    return (7 | 2 << 3 | 1 << 6) & ((1 << 3 * C) - 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_host_statement(shape, dtype):
    from multi_stylegan_amd import sample_sheets
    x = _input(shape, dtype)
    assert bool(x.float().isnan().any()) and bool(x.float().isinf().any())
    want = sample_sheets(x)                                                   # the host's statement
    x_dev = x.to(DEV)
    assert x_dev.data_ptr() % 16 == 0
    for fill in (0xAA, 0x55):                                                 # every byte is written, whatever was there
        assert torch.equal(_entry(x_dev, _default_tints(shape[1]), fill), want), fill
    got = sample_sheets(x_dev)                                                # the public op
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want)
    tints = (5 | 3 << 3 | 6 << 6) & ((1 << 3 * shape[1]) - 1)
    want_tinted = sample_sheets(x, tints=tints)
    assert not torch.equal(want_tinted, want)
    assert torch.equal(sample_sheets(x_dev, tints=tints).cpu(), want_tinted)
    assert torch.equal(_entry(x_dev, tints, 0xAA), want_tinted)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_misaligned_bases_take_the_scalar_path(dtype):
    """W % 16 == 0, but the input starts one element (or the output one byte) off a 16-byte boundary."""
    from multi_stylegan_amd import sample_sheets
    shape = (2, 2, 3, 8, 16)
    x = _input(shape, dtype, seed=1)
    want = sample_sheets(x)
    backing = torch.zeros(x.numel() + 1, dtype=dtype, device=DEV)
    backing[1:] = x.reshape(-1).to(DEV)
    shifted = backing[1:].view(shape)
    assert shifted.data_ptr() % 16 == x.element_size() and shifted.is_contiguous()
    assert torch.equal(_entry(shifted, _default_tints(2), 0xAA), want)
    assert torch.equal(sample_sheets(shifted).cpu(), want)
    assert torch.equal(_entry(x.to(DEV), _default_tints(2), 0xAA, out_offset=1), want)


def test_other_inputs_of_the_public_op():
    from multi_stylegan_amd import sample_sheets
    x = _input((2, 2, 3, 8, 16), torch.float32, seed=2)
    want = sample_sheets(x)
    strided = x.transpose(3, 4).contiguous().transpose(3, 4).to(DEV)
    assert not strided.is_contiguous() and torch.equal(sample_sheets(strided).cpu(), want)
    assert torch.equal(sample_sheets(x.double().to(DEV)).cpu(), want)                       # cast to fp32
    assert torch.equal(sample_sheets(x.half().to(DEV)).cpu(), sample_sheets(x.half()))      # likewise
    assert tuple(sample_sheets(torch.zeros(0, 2, 3, 8, 16, device=DEV)).shape) == (0, 2, 8, 48, 3)


def test_argument_errors_return_einval():
    from multi_stylegan_amd import _lib
    fn = _lib.lib()._ctypes.msg_sample_sheet                               # raw ctypes
    seq = torch.zeros(2 * 4 * 3 * 8 * 16, device=DEV)
    out = torch.full((2 * 4 * 3 * 8 * 16 * 3,), 0xAA, dtype=torch.uint8, device=DEV)
    stream = ctypes.c_void_p(_lib.stream_of(seq.device))

    def call(dtype=_lib.MSG_F32, B=2, C=2, T=3, H=8, W=16, tints=7 | 2 << 3, seq_p=seq.data_ptr(), out_p=out.data_ptr()):
        return fn(seq_p, out_p, dtype, B, C, T, H, W, tints, stream)
    assert call(C=4) == _lib.MSG_EINVAL and call(C=0) == _lib.MSG_EINVAL
    assert call(H=0) == _lib.MSG_EINVAL and call(B=0) == _lib.MSG_EINVAL and call(T=-1) == _lib.MSG_EINVAL and call(W=0) == _lib.MSG_EINVAL
    assert call(dtype=_lib.MSG_F16) == _lib.MSG_EINVAL and call(dtype=_lib.MSG_F64) == _lib.MSG_EINVAL and call(dtype=17) == _lib.MSG_EINVAL
    assert call(seq_p=None) == _lib.MSG_EINVAL and call(out_p=None) == _lib.MSG_EINVAL
    assert call(tints=1 << 6) == _lib.MSG_EINVAL and call(C=1, tints=7 | 2 << 3) == _lib.MSG_EINVAL and call(tints=-1) == _lib.MSG_EINVAL
    # more pixels than a launch can address (no memory is touched: the sizes alone decide)
    assert call(B=1 << 30, C=3, T=1 << 20, H=1 << 20, W=3, tints=0) == _lib.MSG_EINVAL
    assert call(B=1 << 30, C=1, T=1 << 10, H=1, W=1, tints=7) == _lib.MSG_EINVAL          # 2^40 pixels, 2^32 blocks
    torch.cuda.synchronize()
    assert bool((out == 0xAA).all())                                       # nothing was launched
    assert call() == _lib.MSG_OK
    torch.cuda.synchronize()
    written = 2 * 2 * 3 * 8 * 16 * 3
    assert bool((out[:written] == 0).all()) and bool((out[written:] == 0xAA).all())    # zeros quantise to 0; C = 2 of 4
    with pytest.raises(_lib.MsgHipError):
        _lib.check(call(C=4), "msg_sample_sheet")


@pytest.mark.parametrize("case", ["c1", "c2", "c3"])
def test_recorded_predictions_on_the_device(case):
    from multi_stylegan_amd import sample_sheets
    arrays, _ = fixture()
    prediction = torch.from_numpy(arrays[f"{case}.prediction"])
    assert torch.equal(sample_sheets(prediction.to(DEV)).cpu(), sample_sheets(prediction))
    assert torch.equal(sample_sheets(prediction.bfloat16().to(DEV)).cpu(), sample_sheets(prediction.bfloat16()))


# ----------------------------------------------------------------------------------------------------------- SheetWriter
def test_sheet_writer_with_device_batches(tmp_path):
    """The files decode to the device sheets, and submit() returns while the caller's stream is still busy with the work the
    sheets depend on: the copy waits for it on the copy stream, the workers wait for the copy, nobody waits on the caller."""
    from multi_stylegan_amd import SheetWriter, sample_sheets
    base = torch.rand(4, 2, 3, 16, 32, generator=torch.Generator().manual_seed(3))
    want = sample_sheets(base)
    base_dev = base.to(DEV)
    busy = torch.zeros(1 << 27, device=DEV)                                 # 512 MB: each pass over it is a fraction of a ms
    torch.cuda.synchronize()
    with SheetWriter(str(tmp_path), workers=3, depth=2) as writer:
        for _ in range(300):
            busy.add_(1.0)
        # = base only once all three hundred passes are done (300 - 300 = 0 exactly)
        sequence = base_dev + (busy[:base.numel()].view(base.shape) - 300.0)
        sheets = sample_sheets(sequence)
        done = torch.cuda.Event()
        done.record()
        writer.submit([f"s{i}.png" for i in range(8)], sheets.reshape(8, 16, 96, 3))
        still_running = not done.query()
        second = sample_sheets(base_dev.flip(0))                            # a second batch: the ring's other buffer
        writer.submit([f"t{i}.png" for i in range(8)], second.reshape(8, 16, 96, 3))
    assert still_running, "submit() returned only after the caller's stream had drained"
    assert writer.written == 16
    flat = want.reshape(8, 16, 96, 3)
    flipped = want.flip(0).reshape(8, 16, 96, 3)
    for i in range(8):
        assert np.array_equal(png_util.decode(open(tmp_path / f"s{i}.png", "rb").read()), flat[i].numpy()), i
        assert np.array_equal(png_util.decode(open(tmp_path / f"t{i}.png", "rb").read()), flipped[i].numpy()), i
    with SheetWriter(str(tmp_path / "sync"), workers=0) as sync:            # the synchronous mode
        sync.submit(["a.png"], sample_sheets(base_dev)[0, :1].reshape(1, 16, 96, 3))
    assert np.array_equal(png_util.decode(open(tmp_path / "sync" / "a.png", "rb").read()), flat[0].numpy())


# ------------------------------------------------------------------------------------------------ the tiny generator, 32^2
SEED, ANCHORS, STEPS, BATCH = 7, 4, 6, 8


@pytest.fixture(scope="module")
def tiny(golden):
    """The golden tiny generator and the 24 interpolation frames an eager forward gives, computed once."""
    from test_hip_models import _models
    from multi_stylegan_amd import interpolation_latents, sample_sheets
    _, g, _ = _models(golden)
    g.eval().requires_grad_(False)
    anchors = torch.randn(ANCHORS, g.latent_dimensions, generator=torch.Generator().manual_seed(SEED))
    latents = interpolation_latents(anchors.to(DEV), STEPS)
    frames = []
    with torch.no_grad():
        for first in range(0, ANCHORS * STEPS, BATCH):
            image = g(latents[first:first + BATCH].contiguous(), randomize_noise=False)
            B, C, T, H, W = image.shape
            assert (B, C, T, H, W) == (BATCH, 2, 3, 32, 32)
            frames.append(sample_sheets(image).reshape(B, C * H, T * W, 3).cpu())
    return g, torch.cat(frames).numpy()


def _frames(directory, count):
    assert sorted(os.listdir(directory)) == [f"frame_{i:05d}.png" for i in range(count)]
    return np.stack([png_util.decode(open(os.path.join(directory, f"frame_{i:05d}.png"), "rb").read()) for i in range(count)])


@pytest.mark.parametrize("use_graph", [False, True])
def test_interpolation_frames_equal_an_eager_forward(tiny, use_graph, tmp_path):
    from multi_stylegan_amd import interpolation_frames
    g, want = tiny
    out = str(tmp_path / "frames")
    assert interpolation_frames(g, out, anchors=ANCHORS, steps_per_anchor=STEPS, batch_size=BATCH, seed=SEED,
                                use_graph=use_graph) == 24
    got = _frames(out, 24)
    assert got.shape == (24, 64, 96, 3) and np.array_equal(got, want)
    assert len(np.unique(got.reshape(24, -1), axis=0)) == 24                # 24 different pictures


def test_interpolation_frames_partial_last_batch(tiny, tmp_path):
    from multi_stylegan_amd import SheetWriter, interpolation_frames
    g, _ = tiny
    out = str(tmp_path / "frames")
    with SheetWriter(out, workers=2) as writer:                             # a writer of the caller's
        assert interpolation_frames(g, out, anchors=ANCHORS, steps_per_anchor=5, batch_size=BATCH, seed=SEED, use_graph=False,
                                    writer=writer) == 20
    assert _frames(out, 20).shape == (20, 64, 96, 3)                        # exactly 20: the padding is not written


def test_dump_samples(tiny, tmp_path):
    from multi_stylegan_amd import dump_samples
    g, _ = tiny
    out = str(tmp_path / "samples")
    assert dump_samples(g, 5, out, batch_size=2) == 5
    assert sorted(os.listdir(out)) == sorted([f"sample_bf_{i}.png" for i in range(5)] + [f"sample_gfp_{i}.png" for i in range(5)])
    seen = set()
    for i in range(5):
        bf = png_util.decode(open(os.path.join(out, f"sample_bf_{i}.png"), "rb").read())
        gfp = png_util.decode(open(os.path.join(out, f"sample_gfp_{i}.png"), "rb").read())
        assert bf.shape == (32, 96, 3) and gfp.shape == (32, 96, 3)
        assert not gfp[..., 0].any() and not gfp[..., 2].any()              # green only
        assert np.array_equal(bf[..., 0], bf[..., 1]) and np.array_equal(bf[..., 0], bf[..., 2])
        seen.add(bf.tobytes())
    assert len(seen) == 5                                                   # one latent per sample


def test_epoch_sample_dump_on_the_golden_trainer(golden, tmp_path):
    from test_hip_models import _golden_trainer
    from multi_stylegan_amd import epoch_sample_dump, sample_sheets, validation_samples
    _, g, _, tr = _golden_trainer(golden)
    out = str(tmp_path / "plots")
    hook = epoch_sample_dump(out)
    random.seed(11); np.random.seed(11)              # the crossover layer of the mixed validation latents is drawn per forward
    hook(tr, 0)
    names = [f"{kind}_1_{channel}_{b}.png" for kind in ("prediction_ema", "prediction_ema_rand", "prediction", "prediction_rand")
             for channel in ("bf", "gfp") for b in range(15)]
    assert len(names) == 4 * 15 * 2 and sorted(os.listdir(out)) == sorted(names)
    assert g.training
    # with the same crossover draws the fixed-noise predictions come out again: the files are their sheets
    random.seed(11); np.random.seed(11)
    again = validation_samples(tr)
    for kind in ("prediction_ema", "prediction"):
        want = sample_sheets(again[kind]).cpu()
        for b in (0, 14):
            for c, channel in enumerate(("bf", "gfp")):
                pixels = png_util.decode(open(os.path.join(out, f"{kind}_1_{channel}_{b}.png"), "rb").read())
                assert np.array_equal(pixels, want[b, c].numpy()), (kind, b, channel)
