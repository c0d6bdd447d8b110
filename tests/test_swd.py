"""The sliced Wasserstein distance of validation_metrics.py on the host (CPU tensors take the float64 statement of the
definition) against the independent statement of tests/swd_util.py: the pyramid, the descriptors, the score, its exact
properties (zero on itself, permutation, the closed form under a shift, invariance under per-plane affine maps), that it tells
a blurred set from a sharp one, the SWD / SWVD classes' sweep, cache, warning and the keys ModelWrapper.validation logs, and
the C entries' declarations.  The GPU kernels behind the same functions: tests/test_hip_swd.py."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

import swd_util as su
from test_host import _cpu_trainer


def _vm():
    from multi_stylegan_amd import validation_metrics as vm
    return vm


def corner_positions(B, h, w, K, seed):
    """int32 [B, K, 2] patch centres: the four extreme corners first, the rest drawn by the package."""
    pos = _vm().swd_positions(B, h, w, K, torch.Generator().manual_seed(seed))
    pos[0, :4] = torch.tensor([[3, 3], [3, w - 4], [h - 4, 3], [h - 4, w - 4]], dtype=torch.int32)
    return pos


class StubGenerator(torch.nn.Module):
    """Stands in for the generator: ``[B, channels, frames, h, w]`` images from its OWN seeded CPU generator (whatever the
    latents hold, so that a CPU and a GPU sweep see the same images), on the latents' device."""
    latent_dimensions = 6

    def __init__(self, channels=2, frames=3, size=(32, 32), seed=0):
        super().__init__()
        self.shape, self.rng = (channels, frames) + tuple(size), torch.Generator().manual_seed(seed)
        self.calls = 0

    def forward(self, input):
        z = input[0] if isinstance(input, (list, tuple)) else input
        self.calls += 1
        return (torch.rand((z.shape[0],) + self.shape, generator=self.rng) * 3.0 + 1.0).to(z.device)


def stub_dataset(batches, batch, channels=2, frames=3, size=(32, 32), seed=1):
    rng = torch.Generator().manual_seed(seed)
    return [torch.rand((batch, channels, frames) + tuple(size), generator=rng) * 200.0 + 50.0 for _ in range(batches)]


@pytest.mark.parametrize("size", [(32, 32), (32, 48)])
@pytest.mark.parametrize("planes", [1, 3])
def test_host_statement_matches_the_util(size, planes):
    vm = _vm()
    B, K = 4, 5
    rng = torch.Generator().manual_seed(10 * planes + size[1])
    sets = []
    for s in range(2):
        frames = torch.randn((B, planes) + size, generator=rng) * (1.0 + s) + 0.25
        got, want = vm.laplacian_pyramid(frames), su.pyramid(frames.numpy())
        assert len(got) == len(want) == 2 and got[0].dtype == torch.float64
        pos = corner_positions(B, size[0], size[1], K, seed=s)
        rows = []
        for g, w_ in zip(got, want):
            assert g.shape == w_.shape and np.abs(g.numpy() - w_).max() <= 1e-12 * np.abs(w_).max()
        for lvl, (g, w_) in enumerate(zip(got, want)):
            p = pos if lvl == 0 else corner_positions(B, size[0] >> 1, size[1] >> 1, K, seed=7 + s)
            r = vm.swd_descriptors(g, p)
            assert r.shape == (B * K, planes * 49) and np.array_equal(r.numpy(), su.descriptors(g.numpy(), p.numpy()))
            rows.append(r)
        sets.append(rows)
    for lvl in range(2):
        a, b = sets[0][lvl], sets[1][lvl]
        got = vm.sliced_wasserstein(a, b, planes, generator=torch.Generator().manual_seed(3))
        dirs = vm.swd_directions(planes * 49, 4, 128, torch.Generator().manual_seed(3))
        want = su.swd(a.numpy(), b.numpy(), planes, dirs.numpy())
        assert want > 1.0 and abs(got - want) <= 1e-12 * want, (got, want)


def test_pyramid_levels_and_refusals():
    vm = _vm()
    assert [tuple(l.shape[-2:]) for l in vm.laplacian_pyramid(torch.zeros(1, 256, 256))] == [(256, 256), (128, 128), (64, 64),
                                                                                          (32, 32), (16, 16)]
    assert [tuple(l.shape[-2:]) for l in vm.laplacian_pyramid(torch.zeros(2, 3, 32, 48), min_size=8)] == [(32, 48), (16, 24), (8, 12)]
    assert len(vm.laplacian_pyramid(torch.zeros(1, 24, 24))) == 1
    with pytest.raises(ValueError, match="divisible"):
        vm.laplacian_pyramid(torch.zeros(1, 33, 64))                # two levels need even sides
    with pytest.raises(ValueError, match="divisible"):
        vm.laplacian_pyramid(torch.zeros(1, 34, 64), min_size=8)    # 34 -> 17 -> 8: three levels need multiples of 4
    # a descriptor whose patch leaves the plane reads zeros there
    lvl = torch.arange(2.0 * 81).view(1, 2, 9, 9).double()
    rows = vm.swd_descriptors(lvl, torch.tensor([[[0, 8]]], dtype=torch.int32))
    assert np.array_equal(rows.numpy(), su.descriptors(lvl.numpy(), [[[0, 8]]])) and int((rows == 0).sum()) >= 2 * (49 - 16)
    dirs = vm.swd_directions(98, 2, 5, torch.Generator().manual_seed(0))
    assert dirs.shape == (2, 98, 5) and dirs.dtype == torch.float32
    assert float((dirs.double().square().sum(dim=1) - 1.0).abs().max()) < 1e-6
    gen = torch.Generator().manual_seed(0)
    want = torch.randn([98, 5], generator=gen).double()
    assert torch.equal(dirs[0], (want / want.square().sum(dim=0, keepdim=True).sqrt()).float())
    pos = vm.swd_positions(50, 16, 24, 40, torch.Generator().manual_seed(1))
    assert pos.shape == (50, 40, 2) and pos.dtype == torch.int32
    assert (int(pos[..., 0].min()), int(pos[..., 0].max()), int(pos[..., 1].min()), int(pos[..., 1].max())) == (3, 12, 3, 20)


def _random_rows(n, planes, seed, scale=1.0):
    return torch.randn((n, planes * 49), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale


def test_a_set_against_itself_and_row_order():
    vm = _vm()
    a, b = _random_rows(60, 3, 1), _random_rows(60, 3, 2, 1.5)
    assert vm.sliced_wasserstein(a, a.clone(), 3, generator=torch.Generator().manual_seed(0)) == 0.0
    base = vm.sliced_wasserstein(a, b, 3, generator=torch.Generator().manual_seed(0))
    perm = torch.randperm(60, generator=torch.Generator().manual_seed(4))
    moved = vm.sliced_wasserstein(a, b[perm], 3, generator=torch.Generator().manual_seed(0))
    assert base > 1.0 and abs(moved - base) <= 1e-12
    with pytest.raises(ValueError, match="rows"):
        vm.sliced_wasserstein(a, b[:59], 3)
    with pytest.raises(ValueError, match="planes"):
        vm.sliced_wasserstein(a, b, 2)


def test_closed_form_under_a_shift():
    """normalize=False and B = A + c: every projection of B is that of A moved by c . theta, sorting keeps the pairing, and the
    score is 1000 mean_theta |c . theta|."""
    vm = _vm()
    a = _random_rows(40, 2, 5)
    c = torch.randn(98, generator=torch.Generator().manual_seed(6), dtype=torch.float64) * 0.1
    got = vm.sliced_wasserstein(a, a + c, 2, repeats=3, directions=50, generator=torch.Generator().manual_seed(9), normalize=False)
    dirs = vm.swd_directions(98, 3, 50, torch.Generator().manual_seed(9)).double()
    want = 1000.0 * float((c[None, :, None] * dirs).sum(dim=1).abs().mean())
    assert abs(got - want) <= 1e-12 * want, (got, want)


def test_invariance_under_per_plane_affine_maps():
    """x -> alpha_p x + beta_p on one set's plane p leaves x^ = (x - mean) / std alone -- in exact arithmetic.  The definition
    rounds mean and istd to fp32, so the score is unchanged to 1e-9 exactly where that rounding commutes with the map: alpha_p
    a power of two (istd scales exactly) and beta_p = 0.  Those cases are held to 1e-9; without the per-plane normalisation
    they would change the score by orders of magnitude.  For a general alpha_p > 0 and a shift beta_p the fp32-rounded mean
    and istd land up to half an ulp elsewhere before and after the map; the score may then move by what one ulp of each moves
    it by (swd_util.ulp_term, of the set before plus the set after the map), and is held to that.  Figures of the float64
    statement on these sets: the power-of-two scalings move the score of 191.6 by 0, the general map by 3.4e-6 (derived limit
    1.7e-2) -- 1e-9 cannot hold for a general map while mean and istd are fp32."""
    vm = _vm()
    planes = 3
    a, b = _random_rows(80, planes, 11), _random_rows(80, planes, 12, 1.3) + 0.01
    base = vm.sliced_wasserstein(a, b, planes, generator=torch.Generator().manual_seed(2))
    raw = vm.sliced_wasserstein(a, b, planes, generator=torch.Generator().manual_seed(2), normalize=False)

    def mapped(alpha, beta):
        out = b.clone().view(80, planes, 49)
        for p in range(planes):
            out[:, p] = alpha[p] * out[:, p] + beta[p]
        return out.view(80, planes * 49)

    scaled = mapped((1024.0, 0.125, 4.0), (0.0, 0.0, 0.0))
    assert abs(vm.sliced_wasserstein(a, scaled, planes, generator=torch.Generator().manual_seed(2)) - base) <= 1e-9
    assert abs(vm.sliced_wasserstein(a, scaled, planes, generator=torch.Generator().manual_seed(2), normalize=False) - raw) > 100.0
    general = mapped((2.5, 0.3, 40.0), (100.0, -3.0, 0.5))
    got = vm.sliced_wasserstein(a, general, planes, generator=torch.Generator().manual_seed(2))
    dirs = vm.swd_directions(planes * 49, 4, 128, torch.Generator().manual_seed(2)).numpy()
    limit = 0.0
    for rows in (b.numpy(), general.numpy()):
        mean, istd = su.plane_stats(rows, planes)
        limit += 1000.0 * np.mean([su.ulp_term(rows, planes, mean, istd, dirs[r]) for r in range(4)])
    print(f"general affine map: score moved by {abs(got - base):.3e}, derived limit {limit:.3e}")
    assert abs(got - base) <= limit and limit < 1e-4 * base


_TEXTURES = {}


def texture_rows():
    """{set: [levels][n, 147]} descriptor rows (float64, from the util's pyramid) of three sets of 64 three-plane 64 x 64
    textures: 'A', an independent 'B' from the same process, and 'C', a third sample blurred by sigma = 1.  Computed once."""
    if not _TEXTURES:
        vm = _vm()
        for name, seed, blur in (("A", 1, 0.0), ("B", 2, 0.0), ("C", 3, 1.0)):
            frames, gen = su.textures(seed, blur), torch.Generator().manual_seed(10 + seed)
            _TEXTURES[name] = [su.gather(lvl, vm.swd_positions(frames.shape[0], lvl.shape[2], lvl.shape[3], 128, gen).numpy())
                               for lvl in su.pyramid(frames)]
    return _TEXTURES


def test_the_metric_tells_a_blurred_set_from_a_sharp_one():
    """64 three-plane 64 x 64 textures per set.  Blur removes the finest level's detail: its score against a blurred set is at
    least twice that against an independent sharp set, while the coarsest level does not move."""
    vm = _vm()
    rows = texture_rows()
    score = lambda x, y, lvl: vm.sliced_wasserstein(torch.from_numpy(rows[x][lvl]), torch.from_numpy(rows[y][lvl]), 3,
                                                    generator=torch.Generator().manual_seed(5))
    fine_ab, fine_ac = score("A", "B", 0), score("A", "C", 0)
    coarse_ab, coarse_ac = score("A", "B", 2), score("A", "C", 2)
    print(f"finest: A-B {fine_ab:.2f}, A-C {fine_ac:.2f}; coarsest: A-B {coarse_ab:.2f}, A-C {coarse_ac:.2f}")
    assert fine_ac >= 2.0 * fine_ab
    assert abs(coarse_ac - coarse_ab) < 0.25 * coarse_ab


def test_classes_sweep_cache_fields_and_warn():
    vm = _vm()
    dataset = stub_dataset(3, 4)
    kw = dict(device="cpu", batch_size=4, data_samples=8, descriptors_per_image=16)
    for cls, planes in ((vm.SWD, 1), (vm.SWVD, 3)):
        torch.manual_seed(0)
        metric = cls(no_rfp=True, generator=torch.Generator().manual_seed(3), **kw)
        gen = StubGenerator(seed=5)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = metric(generator=gen, dataset=dataset)
        assert isinstance(got, tuple) and len(got) == 2                        # (bf, gfp)
        for score in got:
            assert score._fields == ("mean", "r32", "r16") and all(math.isfinite(v) and v > 0 for v in score)
            assert score.mean == pytest.approx((score.r32 + score.r16) / 2, rel=1e-15)
        assert gen.calls == 2 and len(metric.rows_real) == 2 and len(metric.rows_real[0]) == 2
        assert all(r.shape == (8 * 16, planes * 49) and r.dtype == torch.float32 for rows in metric.rows_real for r in rows)
        cached = metric.rows_real[0][0]

        def no_dataset():
            raise AssertionError("the real rows are cached: the dataset is not swept again")
            yield
        metric(generator=gen, dataset=no_dataset())
        assert metric.rows_real[0][0] is cached and gen.calls == 4
    single = vm.SWD(no_rfp=True, no_gfp=True, **kw)(generator=StubGenerator(), dataset=dataset)
    assert single._fields == ("mean", "r32", "r16")
    with pytest.raises(TypeError):
        vm.SWD(torch.nn.Identity(), network=None)


def test_swvd_is_the_free_functions_on_the_swept_rows():
    """One channel, clips: the class's draws in their order (per batch and level the positions, then per level the directions),
    redone by hand on the util's pyramid."""
    vm = _vm()
    dataset = stub_dataset(3, 4)
    metric = vm.SWVD(device="cpu", batch_size=4, data_samples=8, descriptors_per_image=16, no_rfp=True, no_gfp=True,
                     repeats=2, directions=32, generator=torch.Generator().manual_seed(3))
    got = metric(generator=StubGenerator(seed=5), dataset=dataset)
    gen, stub = torch.Generator().manual_seed(3), StubGenerator(seed=5)
    sets = []
    for batches in (dataset[:2], [stub(torch.zeros(4, 6)) for _ in range(2)]):
        rows = [[], []]
        for images in batches:
            for lvl, level in enumerate(su.pyramid(images[:, 0].numpy())):
                pos = vm.swd_positions(4, level.shape[2], level.shape[3], 16, gen)
                rows[lvl].append(su.descriptors(level, pos.numpy()).astype(np.float32))
        sets.append([np.concatenate(r) for r in rows])
    for lvl, field in enumerate(("r32", "r16")):
        dirs = vm.swd_directions(147, 2, 32, gen)
        want = su.swd(sets[0][lvl], sets[1][lvl], 3, dirs.numpy())
        assert getattr(got, field) == pytest.approx(want, rel=1e-9), field


def test_constant_plane_scores_nan_with_one_warning():
    vm = _vm()
    dataset = stub_dataset(2, 4)
    for images in dataset:
        images[:, 0, 1] = 7.0                                                  # frame 1 of the bright-field channel: constant
    metric = vm.SWVD(device="cpu", batch_size=4, data_samples=8, descriptors_per_image=16, no_rfp=True,
                     generator=torch.Generator().manual_seed(3))
    gen = StubGenerator(seed=5)
    with pytest.warns(UserWarning, match="channel 0, level r32") as caught:
        bf, gfp = metric(generator=gen, dataset=dataset)
    assert math.isnan(bf.r32) and math.isnan(bf.r16) and math.isnan(bf.mean) and math.isfinite(gfp.mean)
    assert sorted(str(w.message).split(":")[1].strip() for w in caught if "constant" in str(w.message)) == \
        ["channel 0, level r16", "channel 0, level r32"]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                         # once per channel and level
        metric(generator=gen, dataset=dataset)
    for value in (1.0, 0.1, -1234.567):                                        # (decided by min == max, not by a rounded variance)
        rows = torch.full((20, 49), value, dtype=torch.float32)
        assert math.isnan(vm.sliced_wasserstein(rows, _random_rows(20, 1, 0), 1))
        assert math.isnan(su.swd(rows.numpy(), _random_rows(20, 1, 0).numpy(), 1, vm.swd_directions(49, 1, 4).numpy()))


def test_short_dataset_warns_and_the_generator_sweep_follows_it():
    vm = _vm()
    metric = vm.SWD(device="cpu", batch_size=4, data_samples=40, descriptors_per_image=16, no_rfp=True, no_gfp=True)
    gen = StubGenerator()
    with pytest.warns(UserWarning, match="fewer than data_samples"):
        metric(generator=gen, dataset=stub_dataset(3, 4))
    assert metric.rows_real[0][0].shape[0] == 12 * 16 and gen.calls == 3


def test_wrapper_validation_logs_the_per_level_keys(golden):
    vm = _vm()
    _, _, _, trainer = _cpu_trainer(golden)
    trainer.generator_ema = StubGenerator()
    kw = dict(device="cpu", batch_size=4, data_samples=8, descriptors_per_image=16, no_rfp=True)
    trainer.validation_metrics = (vm.SWD(**kw), vm.SWVD(no_gfp=True, **kw))
    best = trainer.best_fvd
    scores = trainer.validation(stub_dataset(2, 4))
    fields = ("mean", "r32", "r16")
    assert sorted(scores) == sorted([f"SWD_{f}_{c}" for f in fields for c in ("bf", "gfp")] + [f"SWVD_{f}_bf" for f in fields])
    assert all(np.isfinite(v) for v in scores.values()) and trainer.best_fvd == best
    assert set(trainer.pop_logs()) >= set(scores)


def test_swd_entries_are_declared_and_exported():
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    build(verbose=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    I, L, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    want = {"msg_laplacian_level": (I, [P, I, I, I, P, P, P]),
            "msg_swd_gather": (I, [P, I, I, I, I, P, I, P, P]),
            "msg_swd_plane_sums_workspace": (L, [I, I]),
            "msg_swd_plane_sums": (I, [P, I, I, P, P, P]),
            "msg_swd_project": (I, [P, I, I, P, P, P, I, P, P]),
            "msg_sorted_l1_workspace": (L, [I, I]),
            "msg_sorted_l1": (I, [P, P, I, I, P, P, P])}
    for name, sig in want.items():
        assert name in _lib.declared_symbols() and hasattr(handle, name)
        assert _lib._SIGNATURES[name] == sig, name
    for name in ("msg_swd_plane_sums_workspace", "msg_sorted_l1_workspace"):
        getattr(handle, name).restype = L
    assert handle.msg_swd_plane_sums_workspace(256, 3) == 16 * 3 and handle.msg_swd_plane_sums_workspace(257, 3) == 2 * 16 * 3
    assert handle.msg_swd_plane_sums_workspace(0, 3) == -1 and handle.msg_swd_plane_sums_workspace(5, 0) == -1
    assert handle.msg_sorted_l1_workspace(128, 4096) == 8 * 128 and handle.msg_sorted_l1_workspace(128, 4097) == 2 * 8 * 128
    assert handle.msg_sorted_l1_workspace(0, 5) == -1 and handle.msg_sorted_l1_workspace(5, 0) == -1
