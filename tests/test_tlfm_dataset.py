"""The TLFM dataset (multi_stylegan_amd.tlfm_dataset) and the host side of the batch prepare (data.prepare_tlfm_batch on CPU
tensors) against what the reference's own ``dataset.TFLMDatasetGAN`` listed and returned for a small tree of TIFF files
(tests/golden/tlfm/, written by tools/gen_golden_tlfm.py).  Reference: dataset/tlfm_dataset.py:21-198, dataset/utils.py:4-23."""
import os

import numpy as np
import pytest
import torch

from tlfm_util import TLFM, case_counts, listing, reference_sample, same_bits, samples, write_case_tree, write_tiff

CASES = sorted(listing()["cases"])


def _fallback_reader():
    for name in ("cv2", "PIL"):
        try:
            __import__(name)
            return name
        except ImportError:
            pass
    return None


@pytest.mark.parametrize("name", ["le16_single", "be16_strips", "u8"])
def test_read_tiff_reads_the_baseline_fixtures_exactly(name):
    from multi_stylegan_amd import read_tiff
    with np.load(os.path.join(TLFM, "reader.npz")) as z:
        want = z[name]
    got = read_tiff(os.path.join(TLFM, name + ".tif"))
    assert got.dtype == np.uint16 and got.shape == want.shape and np.array_equal(got, want)      # (8-bit: widened)
    assert int(want.min()) == 0 and int(want.max()) == np.iinfo(want.dtype).max


def test_read_tiff_refuses_what_it_cannot_read(tmp_path):
    """A compressed file: the named ValueError -- or, when cv2 / PIL happens to be importable, the fallback's exact pixels; a
    file that is no TIFF, BigTIFF and RGB raise whatever is installed (no reader may guess)."""
    from multi_stylegan_amd import read_tiff
    with np.load(os.path.join(TLFM, "reader.npz")) as z:
        want = z["lzw16"]
    path = os.path.join(TLFM, "lzw16.tif")
    if _fallback_reader() is None:
        with pytest.raises(ValueError, match=r"lzw16\.tif.*Compression = 5"):
            read_tiff(path)
    else:
        assert np.array_equal(read_tiff(path), want)
    # the refusal itself, with the fallback readers out of reach
    from multi_stylegan_amd import tlfm_dataset
    import builtins
    real_import = builtins.__import__

    def no_readers(name, *a, **k):
        if name.split(".")[0] in ("cv2", "PIL"):
            raise ImportError(name)
        return real_import(name, *a, **k)
    builtins.__import__ = no_readers
    try:
        with pytest.raises(ValueError, match=r"lzw16\.tif.*Compression = 5"):
            tlfm_dataset.read_tiff(path)
        rgb = tmp_path / "rgb.tif"
        write_tiff(str(rgb), np.zeros((4, 6), np.uint16))
        data = bytearray(rgb.read_bytes())
        at = data.index(b"\x15\x01\x03\x00")                                   # SamplesPerPixel (277), SHORT
        data[at + 8] = 3
        rgb.write_bytes(bytes(data))
        with pytest.raises(ValueError, match=r"rgb\.tif.*SamplesPerPixel = 3"):
            tlfm_dataset.read_tiff(str(rgb))
    finally:
        builtins.__import__ = real_import
    junk = tmp_path / "junk.tif"
    junk.write_bytes(b"not a tiff at all")
    with pytest.raises(ValueError, match=r"junk\.tif"):
        read_tiff(str(junk))


def test_read_tiff_round_trips_a_pil_written_file(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from multi_stylegan_amd import read_tiff
    want = np.random.default_rng(1).integers(0, 65536, size=(17, 23)).astype(np.uint16)
    Image.fromarray(want).save(str(tmp_path / "pil.tif"))
    assert np.array_equal(read_tiff(str(tmp_path / "pil.tif")), want)


def test_listing_equals_the_references(tmp_path):
    """The tree of listing.json rebuilt with empty files: exactly the reference's sample tuples, in order."""
    from multi_stylegan_amd import TFLMDatasetGAN
    rec = listing()
    root = tmp_path / "dataset"
    for name in rec["files"]:
        os.makedirs(root / os.path.dirname(name), exist_ok=True)
        (root / name).touch()
    assert len(rec["settings"]) == 3
    for setting in rec["settings"]:
        positions = None if setting["positions"] is None else tuple(setting["positions"])
        ds = TFLMDatasetGAN(str(root), sequence_length=setting["sequence_length"], overlap=setting["overlap"], positions=positions)
        want = [tuple(tuple(os.path.join(str(root), rec["files"][i]) for i in kind) for kind in sample)
                for sample in setting["samples"]]
        assert len(ds) == len(want) > 0 and ds.paths_to_dataset_samples == want


@pytest.mark.parametrize("name", CASES)
def test_float_samples_equal_the_references_bit_for_bit(name, tmp_path):
    """raw=False with the recorded (deterministic) flip callable, prepare_tlfm_batch on the CPU, and raw=True's counts."""
    from multi_stylegan_amd import TFLMDatasetGAN, prepare_tlfm_batch
    case = listing()["cases"][name]
    want = torch.from_numpy(samples()["out." + name].copy())
    write_case_tree(str(tmp_path / "dataset"), case)
    kw = dict(flip=case["flip"], no_rfp=case["no_rfp"], no_gfp=case["no_gfp"])
    force = (lambda x: x.flip(-1)) if case["hflip"] else (lambda x: x)
    ds = TFLMDatasetGAN(str(tmp_path / "dataset"), transformations=force, **kw)
    assert len(ds) == 1
    got = ds[0]
    assert got.dtype == torch.float32 and same_bits(got, want)
    counts = torch.from_numpy(case_counts(case).copy())
    flag = torch.tensor([int(case["hflip"])], dtype=torch.uint8)
    assert same_bits(prepare_tlfm_batch(counts[None], flag, vertical_flip=case["flip"])[0], want)
    assert same_bits(reference_sample(case_counts(case), case["hflip"], case["flip"]), want)      # the tests' own restatement
    # raw=True: the untouched counts, and the flip the float path takes under the same seed
    raw_ds = TFLMDatasetGAN(str(tmp_path / "dataset"), raw=True, **kw)
    float_ds = TFLMDatasetGAN(str(tmp_path / "dataset"), **kw)
    seen = set()
    for seed in range(6):
        torch.manual_seed(seed)
        frames, hflip = raw_ds[0]
        assert frames.dtype == torch.uint16 and hflip.dtype == torch.uint8 and hflip.shape == ()
        assert np.array_equal(frames.numpy(), case_counts(case))
        torch.manual_seed(seed)
        assert same_bits(float_ds[0], reference_sample(case_counts(case), bool(hflip), case["flip"]))
        seen.add(int(hflip))
    assert seen == {0, 1}


def test_raw_mode_refuses_a_callable_and_collates(tmp_path):
    from torch.utils.data import DataLoader
    from multi_stylegan_amd import TFLMDatasetGAN
    rec = listing()
    case = rec["cases"]["c3_plain"]
    with pytest.raises(ValueError, match="raw=True"):
        TFLMDatasetGAN(str(tmp_path), transformations=lambda x: x, raw=True)
    # four overlapping samples from six time steps of one trap, every kind: the recorded frames over and over
    raw = samples()["raw." + case["raw"]]
    root = str(tmp_path / "dataset")
    for c, kind in enumerate(("BF0", "GFP", "RFP")):
        for time in range(6):
            write_tiff(os.path.join(root, "posB", f"posB_t{time:03d}_x_trap0001-{kind}_000_0001.tif"), raw[c, time % 3])
    for no_rfp, channels in ((False, 3), (True, 2)):
        ds = TFLMDatasetGAN(root, no_rfp=no_rfp, raw=True)
        assert len(ds) == 4
        batches = list(DataLoader(ds, batch_size=3))
        assert [len(b) for b in batches] == [2, 2]
        frames, hflip = batches[0]
        assert frames.dtype == torch.uint16 and tuple(frames.shape) == (3, channels, 3, 16, 24)
        assert hflip.dtype == torch.uint8 and tuple(hflip.shape) == (3,)
        assert tuple(batches[1][0].shape) == (1, channels, 3, 16, 24) and tuple(batches[1][1].shape) == (1,)
        assert np.array_equal(frames[1, 0].numpy(), np.stack([raw[0, 1], raw[0, 2], raw[0, 0]]))


def test_prepare_on_the_host_batches_and_rounds():
    """A batch is its samples one by one (per-sample flip flags), bfloat16 is the rounded float32, a constant bright-field
    frame is NaN as in the reference, malformed arguments raise."""
    from multi_stylegan_amd import prepare_tlfm_batch
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 65536, size=(3, 3, 2, 5, 12)).astype(np.uint16)
    counts[1, 0, 1] = 777
    flags = torch.tensor([1, 0, 1], dtype=torch.uint8)
    got = prepare_tlfm_batch(torch.from_numpy(counts), flags, vertical_flip=True, gfp=(100.0, 3000.0), rfp=(5.0, 60000.0))
    for b in range(3):
        want = reference_sample(counts[b], bool(flags[b]), True, gfp=(100.0, 3000.0), rfp=(5.0, 60000.0))
        assert same_bits(got[b], want)
    assert bool(got[1, 0, 1].isnan().all()) and not bool(got[1, 0, 0].isnan().any()) and not bool(got[1, 1:].isnan().any())
    half = prepare_tlfm_batch(torch.from_numpy(counts), flags, gfp=(100.0, 3000.0), rfp=(5.0, 60000.0), out_dtype=torch.bfloat16)
    assert same_bits(half, got.bfloat16())
    assert same_bits(prepare_tlfm_batch(torch.from_numpy(counts), None, vertical_flip=False)[2], reference_sample(counts[2], False, False))
    with pytest.raises(ValueError):
        prepare_tlfm_batch(torch.from_numpy(counts[0]))
    with pytest.raises(ValueError):
        prepare_tlfm_batch(torch.from_numpy(counts), flags[:2])
    with pytest.raises(ValueError):
        prepare_tlfm_batch(torch.from_numpy(counts), out_dtype=torch.float16)
