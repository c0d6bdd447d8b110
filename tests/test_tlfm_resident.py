"""The resident dataset on the host (multi_stylegan_amd/resident.py): the store's frame table against the dataset's own sample
list, the CPU gather against the reference's sample arithmetic (tlfm_util.reference_sample, restated from
dataset/tlfm_dataset.py:186-197 and dataset/utils.py:4-23), the feed's epoch plan, save / load and the errors.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from tlfm_util import listing, reference_sample, same_bits, samples, write_case_tree, write_tiff

CASES = sorted(listing()["cases"])


def _write_dataset(root, frames, H, W, seed, kinds=(("BF0", 65536), ("GFP", 3000)), traps=("0001",), zs=("000",), pos="pos1"):
    """``frames`` time steps of every kind, trap and z position under one position folder: the file-name pattern of
    tests/test_hip_tlfm.py::_write_dataset, with the trap number in the last field too, which the dataset sorts by first."""
    rng = np.random.default_rng(seed)
    for kind, top in kinds:
        for trap in traps:
            for z in zs:
                for time in range(frames):
                    write_tiff(os.path.join(root, pos, f"{pos}_t{time:03d}_x_trap{trap}-{kind}_{z}_{trap}.tif"),
                               rng.integers(0, top, size=(H, W)).astype(np.uint16))


def _kinds(dataset):
    return 1 if dataset.no_gfp else (2 if dataset.no_rfp else 3)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """7 time steps of bright field + GFP at 16 x 24: the dataset and its CPU store, shared (read-only)."""
    from multi_stylegan_amd import ResidentTLFMStore, TFLMDatasetGAN
    root = str(tmp_path_factory.mktemp("resident") / "dataset")
    _write_dataset(root, 7, 16, 24, seed=8)
    dataset = TFLMDatasetGAN(root, no_rfp=True, raw=True)
    return dataset, ResidentTLFMStore.from_dataset(dataset, device="cpu")


def _check_table(dataset, store):
    from multi_stylegan_amd import read_tiff
    C = _kinds(dataset)
    assert len(store) == len(dataset) and store.samples.dtype == torch.int32
    assert tuple(store.samples.shape) == (len(dataset), C, len(dataset.paths_to_dataset_samples[0][0]))
    for s, sample in enumerate(dataset.paths_to_dataset_samples):
        for c in range(C):
            for t, path in enumerate(sample[c]):
                n = int(store.samples[s, c, t])
                assert store.paths[n] == path
                assert np.array_equal(store.frames[n].numpy(), read_tiff(path)), (s, c, t)


def test_shared_frames_are_stored_once(tree):
    dataset, store = tree
    assert len(dataset) == 5 and len(store) == 5
    assert tuple(store.frames.shape) == (14, 16, 24) and store.frames.dtype == torch.uint16      # 14 files, not 5 * 2 * 3 reads
    assert len(store.paths) == 14 and len(set(store.paths)) == 14
    assert tuple(store.samples.shape) == (5, 2, 3)
    _check_table(dataset, store)
    flat = store.frames.numpy().reshape(14, -1)
    assert store.ranges.dtype == torch.int32
    assert np.array_equal(store.ranges.numpy(), np.stack([flat.min(1), flat.max(1)], 1))
    assert (store.gfp, store.rfp, store.flip) == ((150.0, 2200.0), (20.0, 2000.0), True)


def test_two_cells_and_two_focal_planes_follow_the_dataset(tmp_path):
    """Two traps, two z positions (the test's own name must not hold the word the dataset looks for in a path)."""
    from multi_stylegan_amd import ResidentTLFMStore, TFLMDatasetGAN
    root = str(tmp_path / "dataset")
    _write_dataset(root, 4, 6, 8, seed=3, traps=("0001", "0002"), zs=("000", "001"))
    dataset = TFLMDatasetGAN(root, no_rfp=True, raw=True)
    store = ResidentTLFMStore.from_dataset(dataset, device="cpu", workers=3)
    assert len(dataset) > 0 and len(store) == len(dataset)
    assert store.frames.shape[0] == 2 * 2 * 2 * 4                                # every file once
    _check_table(dataset, store)
    for s in range(len(store)):
        names = [store.paths[n] for n in store.samples[s].flatten().tolist()]
        assert len({re.search(r"trap\d+", os.path.basename(name))[0] for name in names}) == 1, names
        assert len({os.path.basename(name).split("_")[-2] for name in names}) == 1, names             # nor z positions
    # non-overlapping samples and a sequence length of 2: inherited, not restated
    other = TFLMDatasetGAN(root, no_rfp=True, raw=True, overlap=False, sequence_length=2)
    _check_table(other, ResidentTLFMStore.from_dataset(other, device="cpu"))


def _expect(dataset, s, hflip, vflip, **kw):
    from multi_stylegan_amd import read_tiff
    counts = np.stack([np.stack([read_tiff(p) for p in paths]) for paths in dataset.paths_to_dataset_samples[s][:_kinds(dataset)]])
    return reference_sample(counts, hflip, vflip, **kw)


def test_cpu_gather_equals_the_reference_sample(tree):
    dataset, store = tree
    for s in range(len(store)):
        for hflip in (0, 1):
            for vflip in (False, True):
                got = store.gather([s], torch.tensor([hflip], dtype=torch.uint8), vertical_flip=vflip)
                assert got.dtype == torch.float32 and tuple(got.shape) == (1, 2, 3, 16, 24)
                assert same_bits(got[0], _expect(dataset, s, hflip, vflip)), (s, hflip, vflip)
    # a batch, in another order, without flags, in bf16; the store's own `flip` is the default
    want = torch.stack([_expect(dataset, s, h, True) for s, h in ((3, 1), (0, 0), (3, 0))])
    assert same_bits(store.gather(torch.tensor([3, 0, 3]), torch.tensor([1, 0, 0], dtype=torch.uint8)), want)
    assert same_bits(store.gather([3, 0, 3], torch.tensor([1, 0, 0]), out_dtype=torch.bfloat16), want.bfloat16())
    assert same_bits(store.gather([2]), _expect(dataset, 2, 0, True)[None])


@pytest.mark.parametrize("name", CASES)
def test_recorded_samples_through_the_store(name, tmp_path):
    from multi_stylegan_amd import ResidentTLFMStore, TFLMDatasetGAN
    case = listing()["cases"][name]
    write_case_tree(str(tmp_path / "dataset"), case)
    dataset = TFLMDatasetGAN(str(tmp_path / "dataset"), raw=True, flip=case["flip"], no_rfp=case["no_rfp"], no_gfp=case["no_gfp"])
    store = ResidentTLFMStore.from_dataset(dataset, device="cpu")
    assert len(store) == 1 and store.flip == case["flip"]
    want = torch.from_numpy(samples()["out." + name].copy())
    assert same_bits(store.gather([0], torch.tensor([int(case["hflip"])], dtype=torch.uint8))[0], want)


def test_three_channels_and_the_datasets_ranges(tmp_path):
    from multi_stylegan_amd import ResidentTLFMStore, TFLMDatasetGAN
    root = str(tmp_path / "dataset")
    _write_dataset(root, 4, 9, 10, seed=5, kinds=(("BF0", 65536), ("GFP", 3000), ("RFP", 3000)))
    dataset = TFLMDatasetGAN(root, raw=True, gfp_min=100, gfp_max=1800.0, rfp_min=30.0, rfp_max=2500, flip=False)
    store = ResidentTLFMStore.from_dataset(dataset, device="cpu")
    assert tuple(store.samples.shape) == (2, 3, 3) and store.frames.shape[0] == 12
    assert (store.gfp, store.rfp, store.flip) == ((100.0, 1800.0), (30.0, 2500.0), False)
    for s in range(2):
        for hflip in (0, 1):
            got = store.gather([s], torch.tensor([hflip], dtype=torch.uint8))
            assert same_bits(got[0], _expect(dataset, s, hflip, False, gfp=(100.0, 1800.0), rfp=(30.0, 2500.0)))
            assert same_bits(store.gather([s], torch.tensor([hflip]), vertical_flip=True, gfp=(150., 2200.), rfp=(20., 2000.))[0],
                             _expect(dataset, s, hflip, True))


def test_constant_bright_field_frame_is_nan():
    from multi_stylegan_amd import ResidentTLFMStore, gather_tlfm_batch
    rng = np.random.default_rng(4)
    frames = rng.integers(0, 65536, size=(6, 8, 8)).astype(np.uint16)
    frames[2] = 4242
    table = torch.tensor([[[0, 2, 1], [3, 4, 2]]], dtype=torch.int32)               # frame 2: bright field once, GFP once
    store = ResidentTLFMStore.from_frames(frames, table)
    got = store.gather([0])
    want = reference_sample(frames[table[0].numpy()], False, True)
    assert bool(got[0, 0, 1].isnan().all()) and bool(want[0, 1].isnan().all())
    keep = torch.ones(got.shape, dtype=torch.bool)
    keep[0, 0, 1] = False
    assert not bool(got[keep].isnan().any())
    assert same_bits(torch.where(keep, got, torch.zeros_like(got)), torch.where(keep, want[None], torch.zeros_like(got)))
    assert same_bits(gather_tlfm_batch(store.frames, store.ranges, table)[keep], got[keep])


def _feed(store, batch_size, **kw):
    from multi_stylegan_amd import ResidentTLFMFeed
    return ResidentTLFMFeed(store, batch_size, **kw)


def _store(S):
    """S one-frame samples (the plan depends on the number of samples only)."""
    from multi_stylegan_amd import ResidentTLFMStore
    frames = np.arange(S * 4, dtype=np.uint16).reshape(S, 2, 2)
    return ResidentTLFMStore.from_frames(frames, torch.arange(S, dtype=torch.int32).view(S, 1, 1))


@pytest.mark.parametrize("world", [1, 2, 4])
def test_plan_shards_one_permutation_over_the_ranks(world):
    S, B = 23, 2
    store = _store(S)
    feeds = [_feed(store, B, seed=7, rank=r, world=world) for r in range(world)]
    plans = [f.plan(3) for f in feeds]
    steps = S // (B * world)
    assert all(len(f) == steps for f in feeds)
    assert all(tuple(ids.shape) == (steps, B) and tuple(flags.shape) == (steps, B) for ids, flags in plans)
    assert all(ids.device.type == "cpu" and flags.dtype == torch.uint8 for ids, flags in plans)
    seen = torch.cat([ids.flatten() for ids, _ in plans]).tolist()
    assert len(seen) == len(set(seen)) == steps * B * world                        # disjoint
    assert set(seen) <= set(range(S)) and S - len(seen) < B * world
    # one draw per sample: a sample's flag does not depend on the rank that gets it
    flag_of = {}
    for ids, flags in plans:
        flag_of.update(zip(ids.flatten().tolist(), flags.flatten().tolist()))
    one = _feed(store, B, seed=7, rank=0, world=1).plan(3)
    assert all(flag_of[i] == f for i, f in zip(one[0].flatten().tolist(), one[1].flatten().tolist()) if i in flag_of)


def test_plan_is_a_function_of_seed_and_epoch():
    store = _store(40)
    a, b = _feed(store, 4, seed=1, rank=0, world=1), _feed(store, 4, seed=1, rank=0, world=1)
    for e in (0, 1, 5):
        assert all(torch.equal(x, y) for x, y in zip(a.plan(e), b.plan(e)))
        assert all(torch.equal(x, y) for x, y in zip(a.plan(e), a.plan(e)))          # nothing carried between calls
    assert not torch.equal(a.plan(0)[0], a.plan(1)[0]) and not torch.equal(a.plan(0)[1], a.plan(1)[1])
    other = _feed(store, 4, seed=2, rank=0, world=1)
    assert not torch.equal(a.plan(0)[0], other.plan(0)[0]) and not torch.equal(a.plan(0)[1], other.plan(0)[1])
    assert sorted(a.plan(0)[0].flatten().tolist()) == list(range(40))
    assert set(a.plan(0)[1].flatten().tolist()) == {0, 1}                           # both flip values occur
    assert int(_feed(store, 4, horizontal_flip_probability=0.0).plan(0)[1].sum()) == 0
    assert int(_feed(store, 4, horizontal_flip_probability=1.0).plan(0)[1].sum()) == 40
    ordered = _feed(store, 4, shuffle=False, rank=0, world=1)
    assert ordered.plan(0)[0].flatten().tolist() == list(range(40)) and ordered.plan(9)[0].flatten().tolist() == list(range(40))
    halves = [_feed(store, 4, shuffle=False, rank=r, world=2).plan(0)[0] for r in range(2)]
    assert halves[0][0].tolist() == [0, 1, 2, 3] and halves[1][0].tolist() == [4, 5, 6, 7] and halves[0][1].tolist() == [8, 9, 10, 11]


def test_short_last_batch_is_for_one_rank_only(tree):
    dataset, store = tree
    with pytest.raises(ValueError, match="drop_last"):
        _feed(store, 2, drop_last=False, rank=0, world=2)
    with pytest.raises(ValueError):
        _feed(store, 8)                                                            # five samples: not one full step
    with pytest.raises(ValueError):
        _feed(store, 2, rank=2, world=2)
    feed = _feed(store, 2, shuffle=False, drop_last=False)
    ids, flags = feed.plan(0)
    assert len(feed) == 3 and ids.tolist() == [[0, 1], [2, 3], [4, -1]] and int(flags[2, 1]) == 0
    assert len(_feed(store, 2)) == 2
    # the epoch loop itself runs on a CPU store too: the batches of the plan, the epoch counter, set_epoch
    batches = list(feed)
    assert [len(b) for b in batches] == [2, 2, 1] and feed.epoch == 1
    for k, batch in enumerate(batches):
        n = len(batch)
        assert same_bits(batch, store.gather(ids[k, :n], flags[k, :n]))
    shuffled = _feed(store, 2, seed=3)
    first, second = list(shuffled), list(shuffled)
    assert shuffled.epoch == 2 and not all(same_bits(a, b) for a, b in zip(first, second))
    shuffled.set_epoch(0)
    assert all(same_bits(a, b) for a, b in zip(first, list(shuffled)))


def test_save_and_load_round_trip(tree, tmp_path):
    from multi_stylegan_amd import ResidentTLFMStore
    from multi_stylegan_amd import resident
    dataset, store = tree
    path = str(tmp_path / "store.npz")
    store.save(path)
    back = ResidentTLFMStore.load(path, device="cpu")
    assert back.frames.dtype == torch.uint16 and np.array_equal(back.frames.numpy(), store.frames.numpy())
    assert torch.equal(back.samples, store.samples) and torch.equal(back.ranges, store.ranges) and back.paths == store.paths
    assert (back.gfp, back.rfp, back.flip) == (store.gfp, store.rfp, store.flip)
    assert same_bits(back.gather([1, 4]), store.gather([1, 4]))
    with np.load(path, allow_pickle=False) as z:
        arrays = {k: z[k] for k in z.files}
    assert int(arrays["version"]) == resident.FORMAT_VERSION
    wrong = str(tmp_path / "wrong.npz")
    np.savez(wrong, **{**arrays, "version": np.int64(resident.FORMAT_VERSION + 1)})
    with pytest.raises(ValueError, match="version"):
        ResidentTLFMStore.load(wrong, device="cpu")
    np.savez(wrong, **{**arrays, "paths": arrays["paths"][:-1]})
    with pytest.raises(ValueError, match="inconsistent"):
        ResidentTLFMStore.load(wrong, device="cpu")
    np.savez(wrong, **{**arrays, "samples": arrays["samples"] + 9})                 # ids past the last frame
    with pytest.raises(ValueError):
        ResidentTLFMStore.load(wrong, device="cpu")


def _dataset_root(dataset):
    return os.path.dirname(os.path.dirname(dataset.paths_to_dataset_samples[0][0][0]))


def test_errors(tree, tmp_path):
    from multi_stylegan_amd import ResidentTLFMStore, TFLMDatasetGAN, gather_tlfm_batch
    dataset, store = tree
    root = str(tmp_path / "dataset")
    _write_dataset(root, 4, 16, 24, seed=1)
    odd = os.path.join(root, "pos1", "pos1_t002_x_trap0001-GFP_000_0001.tif")
    write_tiff(odd, np.zeros((16, 20), dtype=np.uint16))
    with pytest.raises(ValueError, match="pos1_t002_x_trap0001-GFP_000_0001.tif"):
        ResidentTLFMStore.from_dataset(TFLMDatasetGAN(root, no_rfp=True, raw=True), device="cpu")
    with pytest.raises(ValueError, match="transformations"):
        ResidentTLFMStore.from_dataset(TFLMDatasetGAN(_dataset_root(dataset), no_rfp=True, transformations=lambda x: x), device="cpu")
    index = store.samples[:2].clone()
    for bad in (-1, 14):
        index[1, 1, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            gather_tlfm_batch(store.frames, store.ranges, index)
    with pytest.raises(ValueError, match="outside"):
        store.gather([0, 5])
    good = store.samples[:2]
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames.to(torch.int32), store.ranges, good)           # not counts
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames, store.ranges[:3], good)
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames, store.ranges, good[0])                        # [C, T]
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames, store.ranges, good.float())
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames, store.ranges, good, torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames, store.ranges, good, out_dtype=torch.float16)
    with pytest.raises(ValueError):
        gather_tlfm_batch(store.frames, store.ranges, good.to("meta"))                # mixed devices


def test_header_declares_the_entries_and_keeps_the_abi():
    import multi_stylegan_amd as m
    from multi_stylegan_amd import _lib
    for name, args in (("msg_tlfm_frame_range", 6), ("msg_tlfm_gather", 18)):
        assert name in _lib._SIGNATURES and name in _lib.declared_symbols()
        assert len(_lib._SIGNATURES[name][1]) == args
    assert _lib.ABI_VERSION == 5
    assert all(hasattr(m, name) and name in m.__all__ for name in ("ResidentTLFMStore", "ResidentTLFMFeed", "gather_tlfm_batch"))
    from multi_stylegan_amd.data import prefetch
    store = _store(4)
    feed = _feed(store, 2)
    assert prefetch(feed, "cpu") is feed
