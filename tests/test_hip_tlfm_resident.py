"""The resident dataset on the device (csrc/tlfm_prepare.hip: msg_tlfm_frame_range, msg_tlfm_gather) and the feed built on it
(resident.ResidentTLFMStore / ResidentTLFMFeed).  Replaces the per-epoch re-read of dataset/tlfm_dataset.py:128-198 in the
DataLoader workers of train_multi_stylegan.py:60-63.  Expected values: the CPU path of prepare_tlfm_batch on the frames gathered
with numpy (pinned to the reference by tests/test_tlfm_dataset.py), msg_tlfm_prepare for the full-size batch -- never the code
under test.  Every comparison is bit for bit."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from tlfm_util import same_bits, write_tiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GFP, RFP = (150.0, 2200.0), (20.0, 2000.0)
SHAPES = [(5, 12), (16, 8), (7, 24), (64, 72), (33, 250)]
N = 11
# [B = 3, C = 3, T = 3] frame ids: repeated inside a sample (0, 0 / 3, 3, 3), shared between samples, every frame used, frame 0
# (which holds both 0 and 65535) as bright field and as a fluorescence frame
INDEX = np.array([[[0, 1, 2], [3, 4, 5], [6, 7, 8]],
                  [[1, 2, 9], [4, 5, 10], [7, 8, 0]],
                  [[0, 0, 10], [3, 3, 3], [9, 1, 2]]], dtype=np.int32)
FLAGS = (1, 0, 1)


def _frames(H, W, n=N, seed=None):
    """``n`` frames of counts over the whole 16-bit range; frame 0 holds both 0 and 65535 (first and last pixel)."""
    rng = np.random.default_rng(H * 1000 + W if seed is None else seed)
    frames = rng.integers(0, 65536, size=(n, H, W)).astype(np.uint16)
    frames[1::2] = rng.integers(1000, 4000, size=frames[1::2].shape)          # (narrow frames: fluorescence values below the clamp)
    frames[0, 0, 0], frames[0, -1, -1] = 65535, 0
    return frames


def _expect(frames, index, flags, vflip, dtype=torch.float32):
    """CPU prepare_tlfm_batch of the stack numpy gathers."""
    from multi_stylegan_amd import prepare_tlfm_batch
    hflip = None if flags is None else torch.tensor(list(flags), dtype=torch.uint8)
    return prepare_tlfm_batch(torch.from_numpy(frames[index]), hflip, vertical_flip=bool(vflip)).to(dtype)


def _ranges(frames):
    flat = frames.reshape(frames.shape[0], -1)
    return np.stack([flat.min(1), flat.max(1)], 1).astype(np.int32)


def _entry(store, ranges, index, flags, vflip, dtype=torch.float32):
    """msg_tlfm_gather itself on device tensors ``store`` [N, H, W] / ``ranges`` [N, 2]; the output starts as -7 everywhere."""
    from multi_stylegan_amd import _lib
    index = torch.from_numpy(np.ascontiguousarray(index)).to(DEV)
    hflip = None if flags is None else torch.tensor(list(flags), dtype=torch.uint8, device=DEV)
    (B, C, T), (n, H, W) = index.shape, store.shape
    out = torch.full((B, C, T, H, W), -7.0, dtype=dtype, device=DEV)
    rc = _lib.lib().msg_tlfm_gather(store.data_ptr(), ranges.data_ptr(), n, index.data_ptr(), _lib.ptr(hflip), out.data_ptr(),
                                    _lib.dtype_code(out), B, C, T, H, W, int(vflip), GFP[0], GFP[1], RFP[0], RFP[1],
                                    _lib.stream_of(store.device))
    assert rc == _lib.MSG_OK
    return out


def _range_entry(store):
    from multi_stylegan_amd import _lib
    n, H, W = store.shape
    out = torch.full((n, 2), -7, dtype=torch.int32, device=DEV)
    assert _lib.lib().msg_tlfm_frame_range(store.data_ptr(), n, H, W, out.data_ptr(), _lib.stream_of(store.device)) == _lib.MSG_OK
    return out


@pytest.mark.parametrize("H,W", SHAPES)
def test_shape_sweep_is_bit_exact(H, W):
    """Scalar path (W % 8 != 0), exactly one vector per row, the vector path under an odd H, a frame split over two workgroups
    (64 x 72 = 4608 pixels), a wide odd frame; C = 1, 2, 3, vertical flip on and off, fp32 and bf16."""
    frames = _frames(H, W)
    store, ranges = torch.from_numpy(frames).to(DEV), torch.from_numpy(_ranges(frames)).to(DEV)
    for C in (1, 2, 3):
        for vflip in (0, 1):
            index = INDEX[:, :C]
            want = _expect(frames, index, FLAGS, vflip)
            assert not bool(want.isnan().any())
            assert same_bits(_entry(store, ranges, index, FLAGS, vflip), want), (C, vflip)
            assert same_bits(_entry(store, ranges, index, FLAGS, vflip, torch.bfloat16), want.bfloat16()), (C, vflip)
    assert same_bits(_entry(store, ranges, INDEX, None, 1), _expect(frames, INDEX, None, 1))              # hflip = NULL


def test_frame_range_equals_numpy():
    for H, W in SHAPES:
        frames = _frames(H, W)
        got = _range_entry(torch.from_numpy(frames).to(DEV)).cpu().numpy()
        assert np.array_equal(got, _ranges(frames)), (H, W)
        assert tuple(got[0]) == (0, 65535)
    # extremes at the head and the tail of a frame that takes many strides of the workgroup, and a constant frame
    frames = np.full((3, 256, 256), 777, dtype=np.uint16)
    frames[0, 0, 0], frames[0, -1, -1], frames[2, 100, 7], frames[2, 255, 254] = 3, 60000, 776, 778
    assert _range_entry(torch.from_numpy(frames).to(DEV)).cpu().tolist() == [[3, 60000], [777, 777], [776, 778]]


def _offset_view(frames, elements=4):
    """The frames as a device view ``elements`` uint16 into a larger buffer: an 8-byte offset from a 16-byte aligned base."""
    host = np.zeros(frames.size + 16, dtype=np.uint16)
    host[elements:elements + frames.size] = frames.reshape(-1)
    buf = torch.from_numpy(host).to(DEV)
    view = buf[elements:elements + frames.size].view(frames.shape)
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 2 * elements and view.is_contiguous()
    return buf, view


def test_misaligned_store_takes_the_scalar_path():
    from multi_stylegan_amd import gather_tlfm_batch
    frames = _frames(7, 24)                                                 # W % 8 == 0: only the base rules the vector path out
    buf, store = _offset_view(frames)
    assert np.array_equal(_range_entry(store).cpu().numpy(), _ranges(frames))
    ranges = torch.from_numpy(_ranges(frames)).to(DEV)
    for vflip in (0, 1):
        want = _expect(frames, INDEX, FLAGS, vflip)
        assert same_bits(_entry(store, ranges, INDEX, FLAGS, vflip), want)
        assert same_bits(_entry(store, ranges, INDEX, FLAGS, vflip, torch.bfloat16), want.bfloat16())
    got = gather_tlfm_batch(store, ranges, torch.from_numpy(INDEX).to(DEV), torch.tensor(FLAGS, dtype=torch.uint8, device=DEV))
    assert same_bits(got, _expect(frames, INDEX, FLAGS, 1))


@pytest.mark.parametrize("H,W", [(7, 24), (33, 250), (64, 72)])
def test_out_of_range_ids_give_nan_frames_and_read_nothing(H, W):
    """The store is the interior of a larger allocation, so an id of -1 or N would still address valid memory if the guard were
    wrong -- and would show as numbers where NaN is expected."""
    frames = _frames(H, W, n=N + 2)
    big = torch.from_numpy(frames).to(DEV)
    store = big[1:-1]
    inner = frames[1:-1]
    ranges = torch.from_numpy(_ranges(inner)).to(DEV)
    index = INDEX.copy()
    bad = [(0, 0, 1), (1, 2, 2), (2, 1, 0), (2, 2, 2)]
    for (b, c, t), value in zip(bad, (-1, N, N, -1)):
        index[b, c, t] = value
    valid = np.where((index < 0) | (index >= N), 0, index)
    keep = torch.ones((3, 3, 3, H, W), dtype=torch.bool)
    for b, c, t in bad:
        keep[b, c, t] = False
    for dtype in (torch.float32, torch.bfloat16):
        want = _expect(inner, valid, FLAGS, 1, dtype)
        got = _entry(store, ranges, index, FLAGS, 1, dtype).cpu()
        assert all(bool(got[b, c, t].isnan().all()) for b, c, t in bad)
        assert not bool(got[keep].isnan().any())
        assert same_bits(torch.where(keep, got, torch.zeros_like(got)), torch.where(keep, want, torch.zeros_like(want)))


def test_frame_offsets_beyond_two_to_the_31_elements():
    """33 000 frames of 256 x 256: the last three start past element 2^31 of the store.  Only they (and their rows of `ranges`)
    are ever written or read."""
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    if free < 8 << 30:
        pytest.skip(f"needs 8 GiB of free device memory for a 4.3 GB store, {free / 2 ** 30:.1f} GiB are free")
    n, H, W = 33000, 256, 256
    assert (n - 3) * H * W > 2 ** 31
    tail = _frames(H, W, n=3, seed=31)
    store = torch.empty((n, H, W), dtype=torch.uint16, device=DEV)
    ranges = torch.empty((n, 2), dtype=torch.int32, device=DEV)
    store[n - 3:] = torch.from_numpy(tail).to(DEV)
    ranges[n - 3:] = torch.from_numpy(_ranges(tail)).to(DEV)
    local = np.array([[[0, 1, 2], [2, 0, 1]]], dtype=np.int32)
    want = _expect(tail, local, (1,), 1)
    assert same_bits(_entry(store, ranges, local + (n - 3), (1,), 1), want)
    assert same_bits(_entry(store, ranges, local + (n - 3), (1,), 1, torch.bfloat16), want.bfloat16())
    # msg_tlfm_frame_range addresses its frames the same way: the last three, through a store that starts three frames earlier
    from multi_stylegan_amd import _lib
    base = n - 6
    part = torch.full((6, 2), -7, dtype=torch.int32, device=DEV)
    assert _lib.lib().msg_tlfm_frame_range(store[base:].data_ptr(), 6, H, W, part.data_ptr(), _lib.stream_of(store.device)) == 0
    assert np.array_equal(part[3:].cpu().numpy(), _ranges(tail))
    del store, ranges
    torch.cuda.empty_cache()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_size_batch_equals_msg_tlfm_prepare(dtype):
    from multi_stylegan_amd import gather_tlfm_batch, prepare_tlfm_batch
    from multi_stylegan_amd.resident import _frame_ranges
    B, C, T, H, W, n = 16, 2, 3, 256, 256, 40
    frames = _frames(H, W, n=n, seed=5)
    rng = np.random.default_rng(6)
    index = rng.integers(0, n, size=(B, C, T)).astype(np.int32)
    flags = torch.from_numpy(rng.integers(0, 2, size=B).astype(np.uint8)).to(DEV)
    store = torch.from_numpy(frames).to(DEV)
    ranges = _frame_ranges(store)
    assert np.array_equal(ranges.cpu().numpy(), _ranges(frames))
    stacked = torch.from_numpy(frames[index]).to(DEV)
    want = prepare_tlfm_batch(stacked, flags, out_dtype=dtype)                 # msg_tlfm_prepare
    got = gather_tlfm_batch(store, ranges, torch.from_numpy(index).to(DEV), flags, out_dtype=dtype)
    assert got.dtype == dtype and tuple(got.shape) == (B, C, T, H, W) and torch.equal(got, want)
    assert torch.equal(gather_tlfm_batch(store, ranges, torch.from_numpy(index).to(DEV), None, vertical_flip=False, out_dtype=dtype),
                       prepare_tlfm_batch(stacked, None, vertical_flip=False, out_dtype=dtype))


def _write_dataset(root, frames, H, W, seed):
    """One position, one trap, one z position, ``frames`` time steps of bright field and GFP: ``frames - 2`` samples."""
    rng = np.random.default_rng(seed)
    for kind, top in (("BF0", 65536), ("GFP", 3000)):
        for time in range(frames):
            write_tiff(os.path.join(root, "pos1", f"pos1_t{time:03d}_x_trap0001-{kind}_000_0001.tif"),
                       rng.integers(0, top, size=(H, W)).astype(np.uint16))


def test_feed_equals_the_dataloader_path(tmp_path):
    from torch.utils.data import DataLoader
    from multi_stylegan_amd import (ElasticDeformation, ResidentTLFMFeed, ResidentTLFMStore, TFLMDatasetGAN, gather_tlfm_batch,
                                    prepare_tlfm_batch)
    from multi_stylegan_amd.data import prefetch
    root = str(tmp_path / "dataset")
    _write_dataset(root, 7, 16, 24, seed=8)                                   # 5 samples: batches of 2, 2, 1
    dataset = TFLMDatasetGAN(root, no_rfp=True, raw=True)
    store = ResidentTLFMStore.from_dataset(dataset, DEV)
    assert store.frames.is_cuda and tuple(store.frames.shape) == (14, 16, 24) and store.samples.is_cuda
    assert np.array_equal(store.ranges.cpu().numpy(), _ranges(store.frames.cpu().numpy()))
    feed = ResidentTLFMFeed(store, 2, shuffle=False, drop_last=False)
    assert len(feed) == 3 and prefetch(feed, DEV) is feed
    ids, flags = feed.plan(0)
    assert ids.tolist() == [[0, 1], [2, 3], [4, -1]]
    loader = list(DataLoader(dataset, batch_size=2))
    assert [len(counts) for counts, _ in loader] == [2, 2, 1]
    want = [prepare_tlfm_batch(counts, flags[k, :len(counts)]) for k, (counts, _) in enumerate(loader)]
    got = list(feed)                                                          # fresh tensors: valid after the feed moved on
    assert len(got) == 3 and all(g.is_cuda and g.dtype == torch.float32 and same_bits(g, w) for g, w in zip(got, want))
    assert feed.epoch == 1
    feed.set_epoch(0)
    again = list(feed)
    feed.set_epoch(0)
    assert all(same_bits(a, b) for a, b in zip(again, got)) and all(same_bits(a, b) for a, b in zip(list(feed), got))
    # a shuffled epoch with both kinds of flag, in bf16 and without the vertical flip: the plan's samples through the host path
    mixed = ResidentTLFMFeed(store, 2, seed=4, vertical_flip=False, out_dtype=torch.bfloat16)
    ids, flags = mixed.plan(0)
    assert len(mixed) == 2 and set(flags.flatten().tolist()) == {0, 1}
    for k, batch in enumerate(mixed):
        counts = torch.stack([dataset[int(i)][0] for i in ids[k]])
        assert same_bits(batch, prepare_tlfm_batch(counts, flags[k], vertical_flip=False).bfloat16())
    # store.gather with ids on the host and in device memory (one outside the store: a sample of NaN, no fault)
    host = store.gather([4, 1], torch.tensor([1, 0], dtype=torch.uint8))
    assert same_bits(host, prepare_tlfm_batch(torch.stack([dataset[4][0], dataset[1][0]]), torch.tensor([1, 0], dtype=torch.uint8)))
    there = store.gather(torch.tensor([4, 7, 1], device=DEV), torch.tensor([1, 0, 0], dtype=torch.uint8))
    assert same_bits(there[::2], host) and bool(there[1].isnan().all())
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames, store.ranges, store.samples[:2].cpu())         # mixed devices
    # elastic=: the plain batches deformed in order, noise from an equally seeded generator
    module = ElasticDeformation(alpha=12, sigma=3, generator=torch.Generator(device=DEV).manual_seed(33))
    deformed = list(ResidentTLFMFeed(store, 2, shuffle=False, drop_last=False, elastic=module))
    other = ElasticDeformation(alpha=12, sigma=3, generator=torch.Generator(device=DEV).manual_seed(33))
    assert len(deformed) == 3 and all(same_bits(d, other.deform_batch(g)) for d, g in zip(deformed, got))
    assert not any(same_bits(d, g) for d, g in zip(deformed, got))
    with pytest.raises(ValueError, match="ElasticDeformation"):
        ResidentTLFMFeed(store, 2, elastic=lambda x: x)
    # save / load on the device
    store.save(str(tmp_path / "store.npz"))
    back = ResidentTLFMStore.load(str(tmp_path / "store.npz"), DEV)
    assert back.frames.is_cuda and torch.equal(back.ranges, store.ranges) and same_bits(back.gather([0, 3]), store.gather([0, 3]))


def test_training_on_the_resident_feed_equals_training_on_its_batches(golden, tmp_path):
    """ModelWrapper._gan_training over ResidentTLFMFeed == the same iterations over the same batches materialised as a list (as
    test_hip_tlfm.py::test_training_on_the_raw_feed_equals_training_on_the_float_dataset), and validation() hands a metric device
    float batches in [0, 1]."""
    import multi_stylegan_amd as m
    from test_hip_models import _models
    root = str(tmp_path / "dataset")
    _write_dataset(root, 11, 32, 32, seed=9)                                  # 9 samples: three batches of 3
    store = m.ResidentTLFMStore.from_dataset(m.TFLMDatasetGAN(root, no_rfp=True, raw=True), DEV)
    feed = m.ResidentTLFMFeed(store, 3, seed=2)
    assert len(feed) == 3
    results = []
    for resident in (False, True):
        _, g, d = _models(golden)
        tr = m.ModelWrapper(g, d, device=DEV)
        feed.set_epoch(0)
        batches = feed if resident else list(feed)
        torch.manual_seed(3)
        random.seed(3); np.random.seed(3)
        tr._gan_training(batches)
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


def test_argument_errors_return_einval():
    from multi_stylegan_amd import _lib
    gather, frame_range = _lib.lib()._ctypes.msg_tlfm_gather, _lib.lib()._ctypes.msg_tlfm_frame_range          # raw ctypes
    store = torch.zeros(5 * 8 * 8, dtype=torch.int16, device=DEV)
    ranges = torch.zeros(5 * 2, dtype=torch.int32, device=DEV)
    ranges[1::2] = 1
    index = torch.zeros(2 * 3 * 3, dtype=torch.int32, device=DEV)
    out = torch.full((2 * 3 * 3 * 8 * 8,), -7.0, device=DEV)
    found = torch.full((5 * 2,), -7, dtype=torch.int32, device=DEV)
    stream = ctypes.c_void_p(_lib.stream_of(store.device))
    E = _lib.MSG_EINVAL

    def call(dtype=_lib.MSG_F32, N=5, B=2, C=2, T=3, H=8, W=8, store_p=store.data_ptr(), ranges_p=ranges.data_ptr(),
             index_p=index.data_ptr(), out_p=out.data_ptr()):
        return gather(store_p, ranges_p, N, index_p, None, out_p, dtype, B, C, T, H, W, 1, 150.0, 2200.0, 20.0, 2000.0, stream)
    assert call(C=4) == E and call(C=0) == E and call(dtype=_lib.MSG_F16) == E and call(dtype=_lib.MSG_F64) == E
    assert call(N=0) == E and call(N=-3) == E and call(B=0) == E and call(T=0) == E and call(H=0) == E and call(W=-1) == E
    assert call(store_p=None) == E and call(ranges_p=None) == E and call(index_p=None) == E and call(out_p=None) == E
    assert call(B=1 << 24, T=3) == E                                           # 2^24 * 2 * 3 frames x 32 splits: past the block index

    def call_range(N=5, H=8, W=8, store_p=store.data_ptr(), found_p=found.data_ptr()):
        return frame_range(store_p, N, H, W, found_p, stream)
    assert call_range(N=0) == E and call_range(H=0) == E and call_range(W=0) == E and call_range(N=1 << 31) == E
    assert call_range(store_p=None) == E and call_range(found_p=None) == E
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((found == -7).all())              # nothing was launched
    assert call() == _lib.MSG_OK and call_range() == _lib.MSG_OK
    torch.cuda.synchronize()
    assert found.tolist() == [0, 0] * 5 and bool((out[:2 * 2 * 3 * 64] == 0.0).all())
