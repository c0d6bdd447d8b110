"""The sample-based metrics of validation_metrics.py on the host (CPU tensors take the float64 statement of the definitions):
KID / KVD and manifold precision / recall / density / coverage against tests/sample_metrics_util.py, hand-computed values, the
StyleGAN2-ADA subset estimator, the metric classes' sweep, cache, warning and rank exchange, and the keys ModelWrapper.validation
logs.  The GPU kernels behind the same functions: tests/test_hip_sample_metrics.py."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist

import sample_metrics_util as su
from conftest import ROOT
from test_host import _ToyFeatures, _ToyGenerator, _cpu_trainer, _run_ranks


def _vm():
    from multi_stylegan_amd import validation_metrics as vm
    return vm


def _pair(n=37, m=29, d=11, shift=0.5, seed=3, offset=0.0):
    q, r = su.clouds(n, m, d, shift, seed, offset)
    return torch.from_numpy(q), torch.from_numpy(r)


def test_host_kernels_match_the_statement():
    vm = _vm()
    x, y = _pair()
    xd, yd = x.double(), y.double()
    for k, excl in ((1, False), (3, False), (8, False), (3, True), (5, True)):
        a, b = (xd, xd) if excl else (xd, yd)
        got = vm._knn(a, b, k, excl, False)
        assert np.allclose(got.numpy(), su.knn(a.numpy(), b.numpy(), k, excl), rtol=1e-12, atol=1e-12)
    radius = su.knn(yd.numpy(), yd.numpy(), 3, True)
    margin, count = vm._ball_hits(xd, yd, torch.from_numpy(radius), False)
    want = su.ball_hits(x.numpy(), y.numpy(), radius)
    assert np.allclose(margin.numpy(), want["margin"], rtol=1e-12, atol=1e-12) and np.array_equal(count.numpy(), want["count"])
    assert 0 < want["count"].sum() < want["count"].size * len(radius)          # (some pairs inside, some outside)
    ix = torch.stack([torch.arange(20).flip(0), torch.randint(0, 37, (20,), generator=torch.Generator().manual_seed(1))])
    iy = torch.stack([torch.arange(13), torch.tensor([5] * 6 + [7] * 7)])
    for lists in ((None, None), (ix, iy), (ix[:1], None)):
        got = vm._poly_sums(xd, yd, lists[0], lists[1], 1.0 / 11, 1.0, False)
        want, _ = su.poly_sums(x.numpy(), y.numpy(), *[None if l is None else l.numpy() for l in lists], 1.0 / 11, 1.0)
        assert np.allclose(got.numpy(), want, rtol=1e-12)
    with pytest.raises(ValueError, match="outside"):
        vm._poly_sums(xd, yd, torch.tensor([[0, 37]]), None, 1.0, 1.0, False)


def test_kernel_distance_of_three_rows_by_hand():
    """d = 1, k(u, v) = (u v + 1)^3.  x = 0, 1, 2: the unordered pairs give 1, 1, 27 -> sum over a != b = 58.  y = 1, 2, 2:
    27, 27, 125 -> 358.  Cross terms: x = 0: 1 + 1 + 1; x = 1: 8 + 27 + 27; x = 2: 27 + 125 + 125 -> 342.
    MMD^2 = 58 / 6 + 358 / 6 - 2 * 342 / 9 = -20 / 3 (the unbiased estimate may be negative)."""
    vm = _vm()
    x, y = torch.tensor([[0.0], [1.0], [2.0]]), torch.tensor([[1.0], [2.0], [2.0]])
    sums = vm._poly_sums(x.double(), y.double(), None, None, 1.0, 1.0, False)
    assert sums.tolist() == [[58.0, 358.0, 342.0]]
    assert vm.kernel_distance(x, y) == pytest.approx(-20.0 / 3.0, rel=1e-14)
    assert su.kernel_distance(x.numpy(), y.numpy()) == pytest.approx(-20.0 / 3.0, rel=1e-14)
    with pytest.raises(ValueError, match="two rows"):
        vm.kernel_distance(x[:1], y)


def test_subset_estimator_is_stylegan2_adas():
    """metrics/kernel_inception_distance.py of StyleGAN2-ADA on the same index lists:
    ``t += (sum a - tr a) / (m - 1) - 2 sum b / m`` per subset, ``t / S / m``."""
    vm = _vm()
    real, fake = _pair(n=60, m=45, d=9)
    S, size = 7, 20
    got = vm.kernel_distance(real, fake, subsets=S, subset_size=size, generator=torch.Generator().manual_seed(11))
    gen = torch.Generator().manual_seed(11)
    ix, iy = vm.subset_indices(60, size, S, gen), vm.subset_indices(45, size, S, gen)
    assert ix.shape == (S, size) and all(len(set(row.tolist())) == size for row in ix) and int(iy.max()) < 45
    n, t = real.shape[1], 0.0
    for s in range(S):
        x, y = fake.double().numpy()[iy[s].numpy()], real.double().numpy()[ix[s].numpy()]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (size - 1) - b.sum() * 2 / size
    assert got == pytest.approx(t / S / size, rel=1e-11)
    assert got == pytest.approx(su.kernel_distance(real.numpy(), fake.numpy(), ix.numpy(), iy.numpy()), rel=1e-11)
    # m = min(N, M, subset_size)
    big = vm.kernel_distance(real, fake, subsets=2, subset_size=1000, generator=torch.Generator().manual_seed(5))
    gen = torch.Generator().manual_seed(5)
    ix, iy = vm.subset_indices(60, 45, 2, gen), vm.subset_indices(45, 45, 2, gen)
    assert big == pytest.approx(su.kernel_distance(real.numpy(), fake.numpy(), ix.numpy(), iy.numpy()), rel=1e-11)


def test_manifold_scores_match_the_statement_and_do_not_move_with_the_origin():
    vm = _vm()
    for shift in (0.0, 0.5, 3.0):
        real, fake = _pair(n=60, m=50, d=6, shift=shift, seed=int(10 * shift) + 1)
        for k in (3, 5):
            got = vm.manifold_scores(real, fake, k=k)
            want = su.manifold(real.numpy(), fake.numpy(), k)
            assert isinstance(got, vm.ManifoldScores) and got._fields == ("precision", "recall", "density", "coverage")
            for field in got._fields:
                assert getattr(got, field) == pytest.approx(want[field], abs=1e-12), (shift, k, field)
            moved = vm.manifold_scores(real.double() + 2.0, fake.double() + 2.0, k=k)
            assert moved == pytest.approx(got, abs=1e-12)
    real, fake = _pair(n=60, m=50, d=6, shift=0.5)
    mid = vm.manifold_scores(real, fake)
    assert 0.0 < mid.precision < 1.0 and 0.0 < mid.recall < 1.0 and 0.0 < mid.coverage < 1.0 and mid.density > 0.0
    with pytest.raises(ValueError, match="k = 50"):
        vm.manifold_scores(real, fake, k=50)


def test_manifold_scores_of_identical_far_apart_and_collapsed_sets():
    vm = _vm()
    real, _ = _pair(n=40, m=40, d=5)
    same = vm.manifold_scores(real, real.clone())
    assert same.precision == same.recall == same.coverage == 1.0 and same.density >= 1.0
    far = vm.manifold_scores(real, real + 100.0)
    assert far == vm.ManifoldScores(0.0, 0.0, 0.0, 0.0)
    # a collapsed generator: every fake row is real row 0.  Its radius is 0 (its neighbours are its duplicates, distance 0: the
    # row itself is skipped by index, not by value) and the ball is still hit by the one real row that equals it
    fake = real[:1].repeat(40, 1)
    radii = vm._knn(fake.double(), fake.double(), 3, True, False)
    assert radii.tolist() == [0.0] * 40
    margin, count = vm._ball_hits(real.double(), fake.double(), radii, False)
    assert margin[0].item() == 0.0 and count[0].item() == 40 and bool((margin[1:] > 0).all()) and int(count[1:].sum()) == 0
    collapsed = vm.manifold_scores(real, fake)
    assert collapsed.recall == 1.0 / 40 and collapsed.precision == 1.0 and collapsed.coverage > 0.0
    # duplicates among the real rows: four copies of one row have radius 0 at k = 3, and a fake row on top of them is inside
    real4 = torch.cat([real[:1].repeat(4, 1), real[1:]])
    assert vm._knn(real4.double(), real4.double(), 3, True, False)[:4].tolist() == [0.0] * 4
    hit, n_hit = vm._ball_hits(real[:1].double(), real4[:4].double(), torch.zeros(4, dtype=torch.float64), False)
    assert hit.item() == 0.0 and n_hit.item() == 4


def test_feature_rows_keep_truncate_and_refuse():
    vm = _vm()
    rows = vm.FeatureRows(5)
    rows.update(torch.arange(12.0).view(3, 2, 2).double())
    assert not rows.full and rows.n == 3
    rows.update(torch.ones(4, 4))
    assert rows.full and rows.n == 5
    rows.update(torch.ones(4, 4))
    got = rows.rows
    assert got.shape == (5, 4) and got.dtype == torch.float32 and got.is_contiguous()
    assert got[:3].tolist() == torch.arange(12.0).view(3, 4).tolist() and rows.all_gather_() is rows
    with pytest.raises(ValueError, match="width"):
        vm.FeatureRows().update(torch.ones(2, 3)).update(torch.ones(2, 4))
    with pytest.raises(ValueError, match="not finite"):
        vm.FeatureRows().update(torch.tensor([[1.0, 2.0], [float("nan"), 0.0]])).rows
    with pytest.raises(ValueError, match="no feature rows"):
        vm.FeatureRows().rows


def _classes(vm):
    return ((vm.KID, {}), (vm.KVD, {}), (vm.PrecisionRecall, {"k": 3}), (vm.PrecisionRecallVideo, {"k": 2}))


def test_metric_classes_sweep_cache_and_warn():
    """The four classes on a toy feature network and a stub generator: what they return is the free function on the rows the
    network produced; the real rows are swept once and cached; a dataset shorter than ``data_samples`` is said to be."""
    vm = _vm()
    torch.manual_seed(7)
    gen = _ToyGenerator()
    dataset = [torch.rand(3, 2, 3, 8, 8) for _ in range(5)]
    for cls, extra in _classes(vm):
        net = _ToyFeatures()
        metric = cls(net, device="cpu", batch_size=4, data_samples=10, no_rfp=True, no_gfp=True, **extra)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = metric(gen, dataset)
        # 4 real batches (12 rows, cut to 10), then 3 generated batches
        assert len(net.rows) == 7 and metric.rows_real[0].shape == (10, 4)
        real, fake = torch.cat(net.rows[:4])[:10].float(), torch.cat(net.rows[4:])[:10].float()
        assert torch.equal(metric.rows_real[0], real)
        if "k" in extra:
            assert isinstance(got, vm.ManifoldScores) and got == vm.manifold_scores(real, fake, k=extra["k"])
        else:
            assert isinstance(got, float) and got == vm.kernel_distance(real, fake)
        metric(gen, dataset)
        assert len(net.rows) == 10                                             # the second call swept generated rows only
    # channels: with a GFP channel the pair (bf, gfp); frames vs clips
    pair = vm.KID(_ToyFeatures(), device="cpu", batch_size=5, data_samples=10, no_rfp=True)(gen, dataset)
    assert isinstance(pair, tuple) and len(pair) == 2 and all(isinstance(v, float) for v in pair)
    frames, clips = _ToyFeatures(), _ToyFeatures()
    frames.forward = lambda x, f=frames.forward: (frames.__dict__.setdefault("shape", x.shape), f(x))[1]
    clips.forward = lambda x, f=clips.forward: (clips.__dict__.setdefault("shape", x.shape), f(x))[1]
    vm.PrecisionRecall(frames, device="cpu", batch_size=5, data_samples=10, no_rfp=True, no_gfp=True)(gen, dataset)
    vm.PrecisionRecallVideo(clips, device="cpu", batch_size=5, data_samples=10, no_rfp=True, no_gfp=True)(gen, dataset)
    assert tuple(frames.shape) == (3, 3, 8, 8) and tuple(clips.shape) == (3, 3, 3, 8, 8)
    short = vm.KVD(_ToyFeatures(), device="cpu", batch_size=4, data_samples=40, no_rfp=True, no_gfp=True)
    with pytest.warns(UserWarning, match="fewer than data_samples"):
        short(gen, dataset)
    assert short.rows_real[0].shape[0] == 15
    with pytest.raises(ValueError, match="feature network"):
        vm.KID(None)


def test_wrapper_validation_logs_named_tuples_field_by_field(golden):
    vm = _vm()
    _, _, _, trainer = _cpu_trainer(golden)
    trainer.generator_ema = _ToyGenerator()
    dataset = [torch.rand(4, 2, 3, 8, 8) for _ in range(3)]
    kw = dict(device="cpu", batch_size=4, data_samples=8)
    trainer.validation_metrics = (vm.KID(_ToyFeatures(), no_rfp=True, **kw), vm.PrecisionRecall(_ToyFeatures(), no_rfp=True, **kw),
                                  vm.PrecisionRecallVideo(_ToyFeatures(), no_rfp=True, no_gfp=True, **kw),
                                  vm.FVD(_ToyFeatures(), no_rfp=True, no_gfp=True, **kw))
    best = trainer.best_fvd
    scores = trainer.validation(dataset)
    fields = ("precision", "recall", "density", "coverage")
    assert sorted(scores) == sorted(["KID_bf", "KID_gfp", "FVD_bf"] + [f"PrecisionRecall_{f}_{c}" for f in fields for c in ("bf", "gfp")]
                                    + [f"PrecisionRecallVideo_{f}_bf" for f in fields])
    assert all(np.isfinite(v) for v in scores.values())
    assert trainer.best_fvd == min(best, scores["FVD_bf"])                    # (KVD and the manifold scores leave the rule alone)
    assert set(trainer.pop_logs()) >= set(scores)


def _sample_metrics_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    sys.path.insert(0, ROOT)
    from multi_stylegan_amd import validation_metrics as vm
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(200 + rank)
    gen = _ToyGenerator()
    for p_ in gen.parameters():
        dist.broadcast(p_.data, 0)
    dataset = [torch.rand(3, 2, 3, 8, 8) for _ in range(5)]                  # rank-distinct shard
    for cls, score in ((vm.KID, vm.kernel_distance), (vm.PrecisionRecall, vm.manifold_scores)):
        net = _ToyFeatures()
        metric = cls(net, device="cpu", batch_size=3, data_samples=20, no_rfp=True, no_gfp=True)
        got = metric(gen, dataset)
        # every rank swept ceil(20 / 2) = 10 rows of its shard (4 batches, the last cut) and 10 generated rows
        assert len(net.rows) == 8
        mine = torch.stack([torch.cat(net.rows[:4])[:10], torch.cat(net.rows[4:])[:10]]).float()
        both = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        real, fake = torch.cat([b[0] for b in both]), torch.cat([b[1] for b in both])
        assert metric.rows_real[0].shape == (20, 4) and torch.equal(metric.rows_real[0], real)
        want = score(real, fake)                                               # the single-process value on the union
        assert got == want, (rank, got, want)
        mine = torch.tensor([got], dtype=torch.float64).flatten()
        seen = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(seen, mine)
        assert torch.equal(seen[0], seen[1])                                   # the same score on every rank
    if rank == 0:
        out.put("ok")
    dist.destroy_process_group()


def test_sample_metrics_are_shared_over_ranks_gloo_world2():
    _run_ranks(_sample_metrics_worker, 2, 29450 + os.getpid() % 300, 120)
