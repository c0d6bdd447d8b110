"""Simulated datasets on the host (multi_stylegan_amd/simulate.py): the TIFF writer against the existing reader, the export's
torch statement against an independent float64 numpy statement, the round trip through the dataset's own arithmetic
(data._prepare_tlfm_host) and through its own discovery code (TFLMDatasetGAN), bf_ranges_like on the golden tree, the ABI
declaration and the command line."""
import ctypes
import io
import os
import threading

import numpy as np
import pytest
import torch

from simulate_util import (GFP, RFP, ROUND_TRIP_BOUND, assert_close_to_reference, assert_round_trip, clean_frames, counts_of,
                           edge_frames, ranges_for, reference_values)
from tlfm_util import listing, samples, write_case_tree


# -------------------------------------------------------------------------------------------------------------- write_tiff
def _plane(h, w, dtype):
    rng = np.random.default_rng(h * 1000 + w)
    top = np.iinfo(dtype).max
    plane = rng.integers(0, top + 1, size=(h, w)).astype(dtype)
    plane.reshape(-1)[0] = top                                               # the extremes are there, whatever the draw
    plane.reshape(-1)[-1 if h * w > 1 else 0] = 0 if h * w > 1 else top
    return plane


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (16, 24), (257, 33)])
def test_write_then_read(size, dtype, tmp_path):
    from multi_stylegan_amd import read_tiff, write_tiff
    plane = _plane(*size, dtype)
    assert plane.max() == np.iinfo(dtype).max and (size == (1, 1) or plane.min() == 0)
    path = str(tmp_path / "plane.tif")
    write_tiff(path, plane)
    back = read_tiff(path)
    assert back.dtype == np.uint16 and np.array_equal(back, plane)
    buffer = io.BytesIO()
    write_tiff(buffer, torch.from_numpy(plane))                              # a file object, a CPU tensor
    assert buffer.getvalue() == open(path, "rb").read()
    data = buffer.getvalue()
    assert data[:4] == b"II*\0" and int.from_bytes(data[4:8], "little") % 2 == 0        # the directory on a word boundary
    assert data[8:8 + plane.nbytes] == plane.astype(plane.dtype.newbyteorder("<")).tobytes()  # one strip behind the header


@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_pil_reads_the_same_pixels(dtype, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from multi_stylegan_amd import write_tiff
    for size in ((1, 1), (3, 5), (257, 33)):
        plane = _plane(*size, dtype)
        path = str(tmp_path / f"p{size[0]}.tif")
        write_tiff(path, plane)
        with Image.open(path) as handle:
            assert np.array_equal(np.asarray(handle), plane)


def test_write_refuses_other_planes(tmp_path):
    from multi_stylegan_amd import write_tiff
    path = str(tmp_path / "never.tif")
    for bad in (np.zeros((4, 4), np.int16), np.zeros((4, 4), np.float32), np.zeros((4, 4), np.uint32), np.zeros((4,), np.uint16),
                np.zeros((2, 4, 4), np.uint16), np.zeros((0, 4), np.uint16), np.zeros((4, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            write_tiff(path, bad)
    assert not os.path.exists(path)


# ------------------------------------------------------------------------------------------------------ the host statement
SHAPES = [(2, 2, 3, 8, 16), (1, 3, 2, 5, 12), (3, 1, 1, 1, 8), (1, 2, 1, 64, 72), (2, 3, 3, 7, 250), (2, 3, 3, 33, 40)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_host_statement_against_float64(dtype):
    """Edge values in every frame (x == m, x == M, 0, 1, just outside [0, 1], NaN, +-inf, a constant frame) under ranges with
    lo = 0, hi = 65535 and hi = lo + 1: at most one count from the float64 statement, only next to a tie; over all shapes
    together at most 1 % of the pixels."""
    from multi_stylegan_amd import export_tlfm_batch
    differing = pixels = 0
    for shape in SHAPES:
        x = edge_frames(shape, dtype)
        B, C, T, H, W = shape
        ranges = ranges_for(B, T, shift=H)
        for vflip in (True, False):
            for normalise in (True, False):
                got = export_tlfm_batch(x, ranges, vertical_flip=vflip, bf_normalise=normalise)
                assert got.dtype == torch.uint16 and tuple(got.shape) == shape
                values = reference_values(x, ranges, vflip, bf_normalise=normalise)
                got, want = got.numpy().astype(np.int64), counts_of(values)
                differ = got != want
                assert np.abs(got - want).max() <= 1
                at = values[differ]
                assert np.all(np.abs(np.abs(at - np.floor(at)) - 0.5) <= 2.0 ** -6), at[:8]
                differing, pixels = differing + int(differ.sum()), pixels + differ.size
                nan = np.isnan(x.float().numpy()[:, :, :, ::-1] if vflip else x.float().numpy())
                assert nan.any() and (got[nan] == 0).all()                   # a NaN pixel writes 0
    assert differing <= 0.01 * pixels, (differing, pixels)


def test_random_inputs_stay_far_below_the_cap():
    from multi_stylegan_amd import export_tlfm_batch
    shape = (4, 3, 3, 48, 64)
    x = clean_frames(shape, seed=3)
    ranges = ranges_for(4, 3)
    got = export_tlfm_batch(x, ranges).numpy()
    count = assert_close_to_reference(got, reference_values(x, ranges, True))
    assert count <= 0.002 * got.size, count                                  # (the cap is 1 %)
    plain = export_tlfm_batch(x, (0, 65535), gfp=(0.0, 65535.0), rfp=(100.0, 60000.0), vertical_flip=False).numpy()
    values = reference_values(x, np.broadcast_to(np.array([0, 65535]), (4, 3, 2)), False, gfp=(0.0, 65535.0), rfp=(100.0, 60000.0))
    assert assert_close_to_reference(plain, values) <= 0.002 * plain.size


def test_the_definition_s_special_cases():
    from multi_stylegan_amd import export_tlfm_batch
    nan, inf = float("nan"), float("inf")
    x = torch.tensor([[0.25, 0.25, nan, 0.25],                               # constant but for a NaN: lo, and 0 for the NaN
                      [0.0, 0.5, 1.0, 0.25],                                 # m = 0, M = 1: lo, the tie, hi
                      [-3.0, 5.0, 1.0, nan],                                 # x == m, x == M
                      [0.0, 1.0, inf, nan],                                  # M = inf: finite pixels lo, inf -> NaN -> 0
                      [nan, nan, nan, nan]]).reshape(5, 1, 1, 1, 4)
    ranges = torch.tensor([[10, 20], [0, 65535], [7, 8], [100, 200], [5, 6]], dtype=torch.int32).reshape(5, 1, 2)
    got = export_tlfm_batch(x, ranges, vertical_flip=False).numpy().reshape(5, 4)
    assert got.tolist() == [[10, 10, 0, 10], [0, 32768, 65535, 16384], [7, 8, 8, 0], [100, 100, 0, 0], [0, 0, 0, 0]]
    clamped = export_tlfm_batch(x, ranges, vertical_flip=False, bf_normalise=False).numpy().reshape(5, 4)
    assert clamped.tolist() == [[12, 12, 0, 12], [0, 32768, 65535, 16384], [7, 8, 8, 0], [100, 200, 200, 0], [0, 0, 0, 0]]
    flu = torch.tensor([-0.1, 0.0, 0.5, 1.0, 1.5, nan, inf, -inf]).reshape(1, 1, 1, 1, 8)
    both = export_tlfm_batch(torch.cat([flu, flu, flu], dim=1), (0, 1), vertical_flip=False).numpy().reshape(3, 8)
    assert both[1].tolist() == [150, 150, 1250, 2350, 2350, 0, 2350, 150]   # clamp(x, 0, 1) * gfp_max + gfp_min
    assert both[2].tolist() == [20, 20, 1020, 2020, 2020, 0, 2020, 20]
    rows = torch.arange(12, dtype=torch.float32).reshape(1, 1, 1, 3, 4)     # the vertical flip: output row r = input row H-1-r
    up = export_tlfm_batch(rows, (0, 11), vertical_flip=True).numpy().reshape(3, 4)
    assert up.tolist() == [[8, 9, 10, 11], [4, 5, 6, 7], [0, 1, 2, 3]]


def test_export_refusals():
    from multi_stylegan_amd import export_tlfm_batch
    x = clean_frames((2, 2, 3, 4, 8))
    for bad in ((5, 5), (-1, 10), (0, 65536), (10, 5), (0.5, 9), (1, 2, 3)):
        with pytest.raises(ValueError):
            export_tlfm_batch(x, bad)
    for bad in (torch.zeros(2, 3, 2, dtype=torch.int32), torch.tensor([[[0, 1]] * 3] * 2, dtype=torch.float32),
                torch.tensor([[[0, 1]] * 2] * 2, dtype=torch.int32), torch.tensor([[[0, 70000]] * 3] * 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            export_tlfm_batch(x, bad)
    for bad in (x[0], x.double(), x.half(), torch.zeros(1, 4, 1, 4, 8), torch.zeros(1, 0, 1, 4, 8)):
        with pytest.raises(ValueError):
            export_tlfm_batch(bad, (0, 100))
    with pytest.raises(ValueError):
        export_tlfm_batch(x, (0, 100), gfp=(1.0, 2.0, 3.0))
    assert tuple(export_tlfm_batch(torch.zeros(0, 2, 3, 4, 8), (0, 9)).shape) == (0, 2, 3, 4, 8)
    assert export_tlfm_batch(x, torch.tensor([[[0, 9]] * 3] * 2, dtype=torch.int64)).dtype == torch.uint16


# ------------------------------------------------------------------------------------------- round trip through the reader
@pytest.mark.parametrize("seed", range(4))
def test_round_trip_through_the_reader_s_arithmetic(seed):
    """_prepare_tlfm_host(export_tlfm_batch(x)) against the definition's n (bright field) and clamp(x, 0, 1) (GFP / RFP):
    |delta| * (hi - lo) and |delta| * div stay within 0.5 + 2^-6 counts, and a frame's counts span [lo, hi] exactly."""
    from multi_stylegan_amd import export_tlfm_batch
    from multi_stylegan_amd.data import _prepare_tlfm_host
    shape = (4, 3, 3, 24, 40)
    x = clean_frames(shape, seed=seed)
    draw = torch.Generator().manual_seed(100 + seed)
    lo = torch.randint(0, 5000, (4, 3), generator=draw)
    ranges = torch.stack([lo, lo + torch.randint(1, 60001, (4, 3), generator=draw)], dim=2).to(torch.int32)
    ranges[0, 0] = torch.tensor([0, 65535])
    ranges[1, 1] = torch.tensor([4000, 4001])
    counts = export_tlfm_batch(x, ranges)
    back = _prepare_tlfm_host(counts, None, True, GFP, RFP, torch.float32)
    worst_bf, worst_fl = assert_round_trip(x, ranges, counts, back)
    assert 0.4 < worst_bf <= ROUND_TRIP_BOUND and 0.4 < worst_fl <= ROUND_TRIP_BOUND    # (the bound is not loose either)
    plain = export_tlfm_batch(x, ranges, vertical_flip=False)                # no flip on either side
    assert_round_trip(x, ranges, plain, _prepare_tlfm_host(plain, None, False, GFP, RFP, torch.float32))
    other = export_tlfm_batch(x, ranges, gfp=(0.0, 65535.0), rfp=(300.0, 41000.0))
    assert_round_trip(x, ranges, other, _prepare_tlfm_host(other, None, True, (0.0, 65535.0), (300.0, 41000.0), torch.float32),
                      gfp=(0.0, 65535.0), rfp=(300.0, 41000.0))


# ------------------------------------------------------------------------------------------------------ writer and reader
def _sequences(channels, count=7):
    rng = np.random.default_rng(channels)
    return torch.from_numpy(rng.integers(0, 65536, size=(count, channels, 3, 8, 16)).astype(np.uint16))


@pytest.mark.parametrize("workers", [0, 3])
@pytest.mark.parametrize("channels", [2, 3])
def test_dataset_reads_what_the_writer_wrote(channels, workers, tmp_path):
    from multi_stylegan_amd import TFLMDatasetGAN, TLFMDatasetWriter
    counts = _sequences(channels)
    out = str(tmp_path / "sim")
    with TLFMDatasetWriter(out, traps_per_position=3, workers=workers, depth=2) as writer:
        for part in (counts[:2], counts[2:3], counts[3:7]):                  # sequences are counted across submits
            writer.submit(part.clone())
        assert writer.sequences == 7
    assert writer.written == 7 * channels * 3 and writer.outstanding == 0
    assert sorted(os.listdir(out)) == ["sim0000", "sim0001", "sim0002"]
    kinds = ("BF0", "GFP", "RFP")[:channels]
    assert sorted(os.listdir(os.path.join(out, "sim0001"))) == sorted(
        f"sim0001_t{t:03d}_x_trap{k:04d}-{kind}_000_{k:04d}.tif" for t in range(3) for k in (1, 2, 3) for kind in kinds)
    assert len(os.listdir(os.path.join(out, "sim0002"))) == channels * 3     # sequence 6 alone
    names = set(listing()["files"])                                          # the shape of the recorded experiment's names
    assert "posA/" + writer.sequence_files(0, channels, 3)[0].split(os.sep)[1].replace("sim0000", "posA") in names
    for overlap in (True, False):
        dataset = TFLMDatasetGAN(out, sequence_length=3, overlap=overlap, no_rfp=channels < 3, raw=True)
        assert len(dataset) == 7
        for k in range(7):
            frames, _ = dataset[k]
            assert frames.dtype == torch.uint16 and np.array_equal(frames.numpy(), counts[k].numpy()), (overlap, k)
    with pytest.raises(RuntimeError):
        writer.submit(counts[:1])                                            # closed


def test_writer_refusals(tmp_path):
    from multi_stylegan_amd import TLFMDatasetWriter
    for mark in ("trap", "tif", "-BF0_", "-GFP", "-RFP", "_000_", "_001_", "_002_"):
        with pytest.raises(ValueError, match=mark):
            TLFMDatasetWriter(str(tmp_path / f"a{mark}b"))
        with pytest.raises(ValueError, match=mark):
            TLFMDatasetWriter(str(tmp_path / "fine"), position_prefix=f"p{mark}")
        assert not os.path.exists(tmp_path / f"a{mark}b")
    for bad in (10000, 0):
        with pytest.raises(ValueError):
            TLFMDatasetWriter(str(tmp_path / "fine"), traps_per_position=bad)
    with pytest.raises(ValueError):
        TLFMDatasetWriter(str(tmp_path / "fine"), position_prefix="a/b")
    with pytest.raises(ValueError):
        TLFMDatasetWriter(str(tmp_path / "fine"), channels=("GFP", "BF0"))
    counts = _sequences(2)
    with TLFMDatasetWriter(str(tmp_path / "fine"), workers=0) as writer:
        writer.submit(counts[:2])
        for bad in (counts[:, :, :, :4], counts[:, :1], counts[:, :, :2], counts[0], counts.to(torch.int32),
                    torch.from_numpy(np.zeros((1, 2, 1001, 1, 1), np.uint16))):
            with pytest.raises(ValueError):
                writer.submit(bad)
        writer.submit(counts[:0])                                            # nothing: allowed
        assert writer.sequences == 2
    with TLFMDatasetWriter(str(tmp_path / "bf"), channels=("BF0",), workers=0) as only_bf:
        with pytest.raises(ValueError):
            only_bf.submit(counts[:1])                                       # two channels, one name
        only_bf.submit(counts[:1, :1])
    assert len(os.listdir(tmp_path / "bf" / "sim0000")) == 3


@pytest.mark.parametrize("workers", [0, 3])
def test_writer_reports_a_position_folder_it_cannot_make(workers, tmp_path):
    """The position folder's name is taken by a regular file: submit itself fails, nothing is queued or counted."""
    from multi_stylegan_amd import TLFMDatasetWriter
    counts = _sequences(2)
    os.makedirs(tmp_path / "out")
    (tmp_path / "out" / "sim0000").write_bytes(b"a file, not a directory")
    writer = TLFMDatasetWriter(str(tmp_path / "out"), workers=workers, depth=1)
    with pytest.raises(OSError):
        writer.submit(counts[:1])
    assert writer.sequences == 0 and writer.outstanding == 0
    writer.close()


def test_writer_error_surfaces_in_the_next_submit_and_in_close(tmp_path):
    from multi_stylegan_amd import TLFMDatasetWriter
    counts = _sequences(2)

    class Failing(TLFMDatasetWriter):
        def _encode(self, path, pixels):
            if "_0001.tif" in path or "_0004.tif" in path:                   # the first and the fourth sequence
                raise OSError(28, "No space left on device", path)
            super()._encode(path, pixels)

    writer = Failing(str(tmp_path / "out"), workers=1, depth=1)
    writer.submit(counts[:1])
    with pytest.raises(OSError):                      # depth 1: the buffer is free only once the failed files gave it back,
        writer.submit(counts[1:2])                    # and by then their exception is there
    assert writer.outstanding == 0 and writer.sequences == 1                 # a refused submit appends nothing
    writer.submit(counts[1:2])                        # reported once; the writer goes on
    writer.submit(counts[2:3])
    writer.submit(counts[3:4])
    with pytest.raises(OSError):
        writer.close()
    writer.close()                                    # reported once
    assert len(os.listdir(tmp_path / "out" / "sim0000")) == 12               # sequences two and three, whole


def test_writer_ring_is_bounded(tmp_path):
    """Twelve batches through a ring of two: never more than two buffers hold unwritten frames, and the same two host buffers
    serve all of them."""
    from multi_stylegan_amd import TLFMDatasetWriter
    seen, pointers, lock = [], set(), threading.Lock()

    class Watching(TLFMDatasetWriter):
        def _encode(self, path, pixels):
            with lock:
                seen.append(self.outstanding)
                pointers.update(slot.buffer.data_ptr() for slot in self._slots if slot.buffer is not None)
            super()._encode(path, pixels)

    counts = _sequences(2, count=12)
    with Watching(str(tmp_path / "out"), workers=3, depth=2) as writer:
        for k in range(12):
            writer.submit(counts[k:k + 1])
            assert writer.outstanding <= 2
    assert len(seen) == 72 and 1 <= min(seen) and max(seen) <= 2 and len(pointers) <= 2 and len(writer._slots) == 2
    assert len(os.listdir(tmp_path / "out" / "sim0000")) == 72


# ---------------------------------------------------------------------------------------------------------- bf_ranges_like
def test_ranges_like_the_golden_experiment(tmp_path, monkeypatch):
    from multi_stylegan_amd import ResidentTLFMStore, TFLMDatasetGAN, bf_ranges_like, export_tlfm_batch, tlfm_dataset
    rec = listing()
    root = str(tmp_path / "real")
    for name in ("c3_vflip_hflip", "c3_plain"):                              # posA trap 1, frames 0..2; posB trap 1, frames 1..3
        write_case_tree(root, rec["cases"][name])
    dataset = TFLMDatasetGAN(root, sequence_length=3, raw=True)
    assert len(dataset) == 2
    real = [[(int(f.min()), int(f.max())) for f in samples()["raw." + rec["cases"][name]["raw"]][0]]
            for name in ("c3_vflip_hflip", "c3_plain")]                      # (min, max) of each sample's bright-field frames
    reads = []
    reader = tlfm_dataset.read_tiff

    def counting(path):
        reads.append(path)
        return reader(path)

    monkeypatch.setattr(tlfm_dataset, "read_tiff", counting)
    ranges = bf_ranges_like(dataset, 40, torch.Generator().manual_seed(4))
    monkeypatch.undo()
    assert len(reads) == len(set(reads)) == 6           # every bright-field file once, nothing else
    assert ranges.dtype == torch.int32 and tuple(ranges.shape) == (40, 3, 2)
    rows = {tuple(map(tuple, r)) for r in ranges.tolist()}
    assert rows == {tuple(r) for r in real}                                  # whole samples, both drawn
    again = bf_ranges_like(dataset, 40, torch.Generator().manual_seed(4))
    assert torch.equal(again, ranges) and not torch.equal(bf_ranges_like(dataset, 40, torch.Generator().manual_seed(5)), ranges)
    only_a = TFLMDatasetGAN(root, sequence_length=2, positions=("posA",), raw=True)      # (posB's frames have another size)
    store = ResidentTLFMStore.from_dataset(only_a, device="cpu")             # a store answers from the ranges it holds
    from_store = bf_ranges_like(store, 9, torch.Generator().manual_seed(4))
    assert len(store) == 2 and torch.equal(from_store, bf_ranges_like(only_a, 9, torch.Generator().manual_seed(4)))
    assert {tuple(map(tuple, r)) for r in from_store.tolist()} == {tuple(real[0][:2]), tuple(real[0][1:])}
    counts = export_tlfm_batch(clean_frames((40, 1, 3, 4, 8)), ranges).numpy()
    assert np.array_equal(counts.reshape(40, 3, -1).min(axis=2), ranges[..., 0].numpy())
    flat = ResidentTLFMStore.from_frames(np.full((3, 2, 2), 65535, np.uint16), torch.tensor([[[0, 1, 2]]]))
    assert bf_ranges_like(flat, 2).tolist() == [[[65534, 65535]] * 3] * 2    # a constant frame still gives lo < hi
    with pytest.raises(ValueError):
        bf_ranges_like([1, 2, 3], 2)


# ------------------------------------------------------------------------------------------------- header and command line
def test_entries_are_declared_and_exported():
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    build(verbose=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("msg_tlfm_export", "msg_tlfm_export_workspace"):
        assert name in _lib.declared_symbols() and hasattr(handle, name)
    res, args = _lib._SIGNATURES["msg_tlfm_export"]
    assert res is ctypes.c_int and len(args) == 17
    assert _lib._SIGNATURES["msg_tlfm_export_workspace"] == (ctypes.c_longlong, [ctypes.c_int, ctypes.c_int])
    handle.msg_tlfm_export_workspace.restype = ctypes.c_longlong
    assert handle.msg_tlfm_export_workspace(2, 3) == 2 * 32 * 2 * 3 and handle.msg_tlfm_export_workspace(0, 3) == 0
    assert _lib.ABI_VERSION == 5


def test_command_line_flags():
    from multi_stylegan_amd import simulate
    args = simulate._parser().parse_args(["--load_checkpoint", "c.pt", "--samples", "12", "--out", "d", "--batch_size", "4",
                                          "--seed", "3", "--bf_range", "100", "4000", "--no_graph"])
    assert (args.load_checkpoint, args.samples, args.out, args.batch_size, args.seed, args.bf_range, args.like, args.no_graph) == \
        ("c.pt", 12, "d", 4, 3, [100, 4000], None, True)
    args = simulate._parser().parse_args(["--out", "d", "--like", "real"])
    assert args.like == "real" and args.bf_range is None and not args.no_graph and args.samples == 100 and args.batch_size == 8
    for argv in ([], ["--out", "d", "--bogus"], ["--out", "d", "--bf_range", "1"],
                 ["--out", "d", "--bf_range", "1", "2", "--like", "real"]):
        with pytest.raises(SystemExit):
            simulate.main(argv)
