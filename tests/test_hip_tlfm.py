"""The device-side batch prepare (csrc/tlfm_prepare.hip: msg_tlfm_prepare) and the raw feed built on it (data.TLFMDeviceFeed).
Replaces, per batch on the GPU, what the reference's dataset computes per sample on the host: dataset/tlfm_dataset.py:186-197,
dataset/utils.py:4-23.  Every comparison is bit for bit: the counts are exact in fp32 and subtract / divide are IEEE."""
import ctypes
import itertools
import os
import random

import numpy as np
import pytest
import torch

from tlfm_util import case_counts, listing, same_bits, samples, write_tiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GFP, RFP = (150.0, 2200.0), (20.0, 2000.0)


def _expect(counts, hflip, vflip, gfp=GFP, rfp=RFP):
    """One sample [C, T, H, W] as the reference computes it, restated from dataset/tlfm_dataset.py:186-197 and
    dataset/utils.py:4-23 (flip, min-max per bright-field frame, clamp / divide / clamp, vertical flip)."""
    x = torch.from_numpy(np.asarray(counts).astype(np.float32))
    x = x.flip(-1) if hflip else x
    flat = x[0].flatten(start_dim=1)
    lo, hi = flat.min(dim=1, keepdim=True)[0].float(), flat.max(dim=1, keepdim=True)[0].float()
    out = [((flat - lo) / (hi - lo)).reshape(x[0].shape)]
    out += [((x[c] - low).clamp(min=0.0) / div).clamp(max=1.0) for c, (low, div) in zip(range(1, x.shape[0]), (gfp, rfp))]
    return torch.stack(out).flip(dims=(-2,)) if vflip else torch.stack(out)


def _expect_batch(counts, flags, vflip):
    return torch.stack([_expect(counts[b], flags is not None and bool(flags[b]), vflip) for b in range(counts.shape[0])])


def _workspace(B, T, fill=0x5A5A5A5A):
    from multi_stylegan_amd import _lib
    words = _lib.lib().msg_tlfm_prepare_workspace(B, T)
    assert words > 0
    return torch.full((words,), fill, dtype=torch.int32, device=DEV)      # (garbage: the entry must not rely on its content)


def _entry(counts, flags, vflip, dtype=torch.float32, ws=None):
    """msg_tlfm_prepare itself, with a workspace of the test's own."""
    from multi_stylegan_amd import _lib
    raw = torch.from_numpy(np.array(counts)).to(DEV)
    hflip = None if flags is None else torch.tensor(list(flags), dtype=torch.uint8, device=DEV)
    B, C, T, H, W = raw.shape
    ws = _workspace(B, T) if ws is None else ws
    out = torch.full(raw.shape, -7.0, dtype=dtype, device=DEV)
    rc = _lib.lib().msg_tlfm_prepare(raw.data_ptr(), _lib.ptr(hflip), out.data_ptr(), _lib.dtype_code(out), B, C, T, H, W,
                                     int(vflip), GFP[0], GFP[1], RFP[0], RFP[1], ws.data_ptr(), _lib.stream_of(raw.device))
    assert rc == _lib.MSG_OK
    return out


def _counts(rng, B, C, T, H, W, max_first):
    """Counts over the whole 16-bit range; every bright-field frame has its unique maximum at the first pixel and its unique
    minimum at the last (``max_first``) or the other way round: the head and the tail of the reduction."""
    counts = rng.integers(0, 65536, size=(B, C, T, H, W)).astype(np.uint16)
    counts[:, 0] = rng.integers(1000, 60000, size=(B, T, H, W))
    counts[:, 0, :, 0, 0], counts[:, 0, :, -1, -1] = (65535, 0) if max_first else (0, 65535)
    return counts


def test_recorded_samples_through_the_kernel():
    rec = listing()["cases"]
    for name, case in sorted(rec.items()):
        want = torch.from_numpy(samples()["out." + name].copy())
        got = _entry(case_counts(case)[None], [int(case["hflip"])], case["flip"])
        assert same_bits(got[0], want), name
        assert same_bits(_entry(case_counts(case)[None], [int(case["hflip"])], case["flip"], torch.bfloat16)[0], want.bfloat16()), name


@pytest.mark.parametrize("H,W", [(5, 12), (16, 8), (7, 24), (64, 72), (33, 250)])
def test_shape_sweep_is_bit_exact(H, W):
    """Scalar path (W % 8 != 0), exactly one vector per row, odd H under the vertical flip, several workgroups per frame
    (64 x 72 = 4608 pixels > one workgroup's 4096; 33 x 250 on the scalar path), B / T / C / flips in every combination."""
    rng = np.random.default_rng(H * 1000 + W)
    ws = {(B, T): _workspace(B, T) for B in (1, 3) for T in (1, 3)}          # shared by every call of a (B, T): see below
    for k, (B, T, C, vflip, with_flags) in enumerate(itertools.product((1, 3), (1, 3), (1, 2, 3), (0, 1), (False, True))):
        counts = _counts(rng, B, C, T, H, W, max_first=bool(k % 2) ^ bool(vflip))
        flags = [1, 0, 1][:B] if with_flags else None
        want = _expect_batch(counts, flags, vflip)
        got = _entry(counts, flags, vflip, ws=ws[(B, T)])
        assert same_bits(got, want), (B, T, C, vflip, flags)
        assert same_bits(_entry(counts, flags, vflip, torch.bfloat16, ws=ws[(B, T)]), got.bfloat16().cpu()), (B, T, C, vflip, flags)
        # the workspace now holds this call's (and the bf16 call's) minima / maxima: the next combination reuses it with new data


def test_consecutive_calls_share_one_workspace():
    rng = np.random.default_rng(11)
    a, b = _counts(rng, 3, 2, 3, 64, 72, True), _counts(rng, 3, 2, 3, 64, 72, False)
    b[:, 0] = b[:, 0] // 4 + 9000                                            # narrower frames: stale extrema would show
    ws = _workspace(3, 3)
    first = _entry(a, [1, 0, 1], 1, ws=ws)
    other = _entry(b, [1, 0, 1], 1, ws=ws)
    again = _entry(a, [1, 0, 1], 1, ws=ws)
    assert same_bits(first, _expect_batch(a, [1, 0, 1], 1)) and same_bits(other, _expect_batch(b, [1, 0, 1], 1))
    assert same_bits(again, first)


def test_full_size_frames():
    """256 x 256 (16 workgroups per frame), B = 2, C = 2, T = 3, through the public op (the library's launch-scoped workspace)."""
    from multi_stylegan_amd import prepare_tlfm_batch
    counts = _counts(np.random.default_rng(3), 2, 2, 3, 256, 256, True)
    flags = torch.tensor([0, 1], dtype=torch.uint8)
    want = _expect_batch(counts, flags, 1)
    raw = torch.from_numpy(counts).to(DEV)
    got = prepare_tlfm_batch(raw, flags.to(DEV))
    assert got.dtype == torch.float32 and same_bits(got, want)
    assert same_bits(prepare_tlfm_batch(raw, flags.to(DEV), out_dtype=torch.bfloat16), want.bfloat16())
    assert same_bits(prepare_tlfm_batch(raw, None, vertical_flip=False), _expect_batch(counts, None, 0))
    assert same_bits(prepare_tlfm_batch(torch.from_numpy(counts), flags), want)          # the host's definition, same bits


def test_constant_bright_field_frame_is_nan():
    counts = _counts(np.random.default_rng(4), 2, 3, 3, 16, 24, True)
    counts[1, 0, 2] = 4242
    want = _expect_batch(counts, [0, 1], 1)
    assert bool(want[1, 0, 2].isnan().all())
    keep = torch.ones(want.shape, dtype=torch.bool)
    keep[1, 0, 2] = False
    for dtype in (torch.float32, torch.bfloat16):
        got = _entry(counts, [0, 1], 1, dtype).cpu()
        assert bool(got[1, 0, 2].isnan().all())
        ref = want.to(dtype)
        assert same_bits(torch.where(keep, got, torch.zeros_like(got)), torch.where(keep, ref, torch.zeros_like(ref)))
        assert not bool(got[keep].isnan().any())


def test_argument_errors_return_einval():
    from multi_stylegan_amd import _lib
    fn = _lib.lib()._ctypes.msg_tlfm_prepare                              # raw ctypes
    raw = torch.zeros(2 * 4 * 3 * 8 * 8, dtype=torch.int16, device=DEV)
    out = torch.full((2 * 4 * 3 * 8 * 8,), -7.0, device=DEV)
    ws = _workspace(2, 3)
    stream = ctypes.c_void_p(_lib.stream_of(raw.device))

    def call(dtype=_lib.MSG_F32, C=2, H=8, raw_p=raw.data_ptr(), out_p=out.data_ptr(), ws_p=ws.data_ptr()):
        return fn(raw_p, None, out_p, dtype, 2, C, 3, H, 8, 1, 150.0, 2200.0, 20.0, 2000.0, ws_p, stream)
    assert call(C=4) == _lib.MSG_EINVAL and call(dtype=_lib.MSG_F16) == _lib.MSG_EINVAL and call(H=0) == _lib.MSG_EINVAL
    assert call(ws_p=None) == _lib.MSG_EINVAL and call(raw_p=None) == _lib.MSG_EINVAL and call(out_p=None) == _lib.MSG_EINVAL
    assert call(C=0) == _lib.MSG_EINVAL and call(dtype=_lib.MSG_F64) == _lib.MSG_EINVAL
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                     # nothing was launched
    assert call() == _lib.MSG_OK
    assert _lib.lib().msg_tlfm_prepare_workspace(2, 3) >= 2 * 2 * 3 and _lib.lib().msg_tlfm_prepare_workspace(0, 3) == 0


def _write_dataset(root, frames, H, W, seed):
    """One position, one trap, one z position, ``frames`` time steps of bright field and GFP: ``frames - 2`` samples."""
    rng = np.random.default_rng(seed)
    for kind, top in (("BF0", 65536), ("GFP", 3000)):
        for time in range(frames):
            write_tiff(os.path.join(root, "pos1", f"pos1_t{time:03d}_x_trap0001-{kind}_000_0001.tif"),
                       rng.integers(0, top, size=(H, W)).astype(np.uint16))


def test_raw_feed_equals_the_float_dataset(tmp_path):
    from torch.utils.data import DataLoader
    from multi_stylegan_amd import TFLMDatasetGAN, TLFMDeviceFeed
    from multi_stylegan_amd.data import prefetch
    root = str(tmp_path / "dataset")
    _write_dataset(root, 7, 16, 24, seed=8)                                   # 5 samples: batches of 2, 2, 1
    torch.manual_seed(21)
    want = list(DataLoader(TFLMDatasetGAN(root, no_rfp=True), batch_size=2))
    assert [len(b) for b in want] == [2, 2, 1] and want[0].dtype == torch.float32
    torch.manual_seed(21)
    feed = TLFMDeviceFeed(DataLoader(TFLMDatasetGAN(root, no_rfp=True, raw=True), batch_size=2), DEV)
    assert len(feed) == 3 and prefetch(feed, DEV) is feed
    got = [batch for batch in feed]                                          # fresh tensors: valid after the feed moved on
    assert len(got) == 3 and all(g.is_cuda and same_bits(g, w) for g, w in zip(got, want))
    torch.manual_seed(21)
    flags = torch.cat([h for _, h in DataLoader(TFLMDatasetGAN(root, no_rfp=True, raw=True), batch_size=2)])
    assert set(flags.tolist()) == {0, 1}                                     # both kinds of sample were in the comparison
    torch.manual_seed(21)
    half = list(TLFMDeviceFeed(DataLoader(TFLMDatasetGAN(root, no_rfp=True, raw=True, flip=False), batch_size=2), DEV,
                               vertical_flip=False, out_dtype=torch.bfloat16))
    assert all(same_bits(h, w.flip(-2).bfloat16()) for h, w in zip(half, want))


def test_training_on_the_raw_feed_equals_training_on_the_float_dataset(golden, tmp_path):
    """ModelWrapper._gan_training over TLFMDeviceFeed == the same iterations over the float dataset's host batches (as
    test_hip_data.py::test_epoch_loop_feeds_pageable_host_batches_through_the_prefetcher), and validation() hands a metric
    device float batches in [0, 1]."""
    from torch.utils.data import DataLoader
    import multi_stylegan_amd as m
    from test_hip_models import _models
    root = str(tmp_path / "dataset")
    _write_dataset(root, 11, 32, 32, seed=9)                                  # 9 samples: three batches of 3
    results = []
    for raw in (False, True):
        _, g, d = _models(golden)
        tr = m.ModelWrapper(g, d, device=DEV)
        torch.manual_seed(5)                                                 # the flips: drawn before the training's own draws
        batches = list(DataLoader(m.TFLMDatasetGAN(root, no_rfp=True, raw=raw), batch_size=3))
        assert len(batches) == 3
        feed = m.TLFMDeviceFeed(batches, DEV) if raw else batches
        torch.manual_seed(3)
        random.seed(3); np.random.seed(3)
        tr._gan_training(feed)
        results.append([p.detach().clone() for p in list(g.parameters()) + list(d.parameters())])
    assert all(torch.equal(a, b) for a, b in zip(*results))

    seen = []

    class Stub:
        def __call__(self, generator, dataset):
            for batch in dataset:
                assert batch.is_cuda and batch.dtype == torch.float32 and tuple(batch.shape) == (3, 2, 3, 32, 32)
                seen.append((float(batch.min()), float(batch.max())))
            return 1.0
    tr.validation_metrics = (Stub(),)
    assert tr.validation(feed) == {"Stub_bf": 1.0}
    assert len(seen) == 3 and all(lo == 0.0 and hi == 1.0 for lo, hi in seen)
