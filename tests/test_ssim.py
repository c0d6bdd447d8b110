"""ms_ssim of multi_stylegan_amd/ssim.py on the host (CPU tensors take the plain-torch statement of the definitions) against
the independent numpy statement of tests/ssim_util.py: values, gradients, the levels table, the clamp and its masked gradient;
the MSSSIM / MSSSIMVideo classes on stub generators and datasets, and the keys ModelWrapper.validation logs; the C entries'
declarations.  The GPU kernels behind the same function: tests/test_hip_ssim.py."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

import ssim_util as su
from test_host import _cpu_trainer


def _ssim():
    from multi_stylegan_amd import ssim
    return ssim


def _vm():
    from multi_stylegan_amd import validation_metrics as vm
    return vm


def _pair(shape, seed):
    x, y = su.parity_pair(shape, seed)
    return torch.from_numpy(x), torch.from_numpy(y)


class StubGenerator(torch.nn.Module):
    """Stands in for the generator: ``[B, channels, frames, h, w]`` images in [0, 1] from its OWN seeded CPU generator (whatever
    the latents hold, so that a CPU and a GPU sweep see the same images), on the latents' device.  ``collapsed``: one fixed image
    plus 1 % noise."""
    latent_dimensions = 6

    def __init__(self, channels=2, frames=3, size=(32, 32), seed=0, collapsed=False):
        super().__init__()
        self.shape, self.rng = (channels, frames) + tuple(size), torch.Generator().manual_seed(seed)
        self.base = torch.rand(self.shape, generator=self.rng) if collapsed else None
        self.calls = 0

    def forward(self, input):
        z = input[0] if isinstance(input, (list, tuple)) else input
        self.calls += 1
        draw = torch.rand((z.shape[0],) + self.shape, generator=self.rng)
        if self.base is not None:
            draw = (self.base[None] + 0.01 * (draw - 0.5)).clamp(0.0, 1.0)
        return draw.to(z.device)


def stub_dataset(batches, batch, channels=2, frames=3, size=(32, 32), seed=1, collapsed=False):
    rng = torch.Generator().manual_seed(seed)
    shape = (channels, frames) + tuple(size)
    base = torch.rand(shape, generator=rng)
    out = []
    for _ in range(batches):
        draw = torch.rand((batch,) + shape, generator=rng)
        out.append((base[None] + 0.01 * (draw - 0.5)).clamp(0.0, 1.0) if collapsed else draw)
    return out


def test_levels_table_and_weights():
    s = _ssim()
    table = {16: 1, 24: 2, 32: 2, 44: 3, 88: 4, 128: 4, 176: 5, 256: 5, 1024: 5, 10: 0, 11: 1, 21: 1, 22: 2}
    for side, want in table.items():
        assert s.ssim_levels(side, side) == want == su.levels(side, side), side
    assert s.ssim_levels(256, 16) == 1 and s.ssim_levels(24, 300) == 2
    assert s.MS_SSIM_WEIGHTS == su.WEIGHTS == (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
    assert np.array_equal(s.ssim_window(torch.float64).numpy(), su.window())
    assert np.array_equal(s.ssim_window(torch.float32).numpy(), su.window(np.float32))
    assert abs(float(s.ssim_window().sum()) - 1.0) < 1e-15
    with pytest.raises(ValueError, match="scale"):
        s.ms_ssim(torch.zeros(1, 1, 10, 32), torch.zeros(1, 1, 10, 32))
    with pytest.raises(ValueError, match="scale"):
        s.ms_ssim(torch.zeros(1, 1, 32, 32), torch.zeros(1, 1, 32, 32), levels=3)
    with pytest.raises(ValueError, match="shape"):
        s.ms_ssim(torch.zeros(1, 1, 32, 32), torch.zeros(1, 2, 32, 32))


@pytest.mark.parametrize("shape", [(3, 2, 16, 19), (2, 2, 24, 26), (2, 1, 45, 52), (1, 1, 88, 90)])
def test_host_statement_matches_the_util(shape):
    s = _ssim()
    x, y = _pair(shape, seed=shape[2])
    want, want_l1, factors = su.ms_ssim(x.numpy(), y.numpy())
    assert factors.shape[1] == su.levels(*shape[2:]) and (factors >= 0.9).all(), "a parity pair's factor is near the clamp"
    got, got_l1 = s.ms_ssim(x.double(), y.double(), return_l1=True)
    assert got.dtype == torch.float64 and got.shape == (shape[0],)
    assert np.abs(got.numpy() - want).max() <= 1e-12 and np.abs(got_l1.numpy() - want_l1).max() <= 1e-15
    assert torch.equal(s.ms_ssim(x.double(), y.double()), got)
    for levels in range(1, factors.shape[1] + 1):                              # fewer scales, another data range
        want_n = su.ms_ssim(x.double().numpy() * 255.0, y.double().numpy() * 255.0, levels, data_range=255.0)[0]
        got_n = s.ms_ssim(x.double() * 255.0, y.double() * 255.0, levels=levels, data_range=255.0)
        assert np.abs(got_n.numpy() - want_n).max() <= 1e-12
    # the tensor's own dtype: fp32 in, fp32 out, within the util's measured fp32 error of the float64 score
    low = s.ms_ssim(x, y)
    assert low.dtype == torch.float32 and np.abs(low.double().numpy() - want).max() <= 1e-4


def test_a_plane_against_itself_scores_one():
    s = _ssim()
    x = torch.rand((2, 3, 44, 50), generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    got, l1 = s.ms_ssim(x, x.clone(), return_l1=True)
    assert torch.equal(got, torch.ones(2, dtype=torch.float64)) and torch.equal(l1, torch.zeros(2, dtype=torch.float64))
    assert su.ms_ssim(x.numpy(), x.numpy())[0].tolist() == [1.0, 1.0]


def test_gradcheck_and_the_scale_gradient_of_the_util():
    s = _ssim()
    x, y = _pair((2, 2, 24, 26), seed=3)                                       # two scales, 26 -> 13: an odd halving
    x, y = x.double().requires_grad_(True), y.double().requires_grad_(True)

    def loss(a, b):
        score, l1 = s.ms_ssim(a, b, return_l1=True)
        return score + 0.5 * l1
    assert torch.autograd.gradcheck(loss, (x, y), eps=1e-6, atol=1e-7, rtol=1e-5, fast_mode=True)
    # the closed form the kernels implement (ssim_util.scale_backward) against autograd of the stock-operator statement
    a, b = _pair((3, 13, 15), seed=4)
    a, b = a.double().requires_grad_(True), b.double()
    g = torch.tensor([[0.3, -1.1, 0.7], [1.0, 0.0, 0.0], [0.0, 2.0, -0.4]], dtype=torch.float64)
    g_half = torch.randn((3, 6, 7), generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    cs, ss, l1 = s._host_scales(a, b, 1, *su.constants())
    half = torch.nn.functional.avg_pool2d(a[:, None], 2)[:, 0]
    total = (g[:, 0] * cs[:, 0] + g[:, 1] * ss[:, 0] + g[:, 2] * l1).sum() + (g_half * half).sum()
    want, = torch.autograd.grad(total, a)
    got = su.scale_backward(a.detach().numpy(), b.numpy(), g.numpy(), g_half.numpy())
    assert np.abs(got - want.numpy()).max() <= 1e-13 * max(1.0, float(want.abs().max()))
    assert np.abs(got[:, 12, :]).max() > 0 and np.array_equal(got[:, :, 14], su.scale_backward(a.detach().numpy(), b.numpy(), g.numpy())[:, :, 14])


def test_clamped_planes_score_zero_and_pass_zero_gradient():
    s = _ssim()
    rng = torch.Generator().manual_seed(7)
    # y = 1 - x on uniform noise: every mean sits near -0.99
    x = torch.rand((2, 2, 24, 26), generator=rng, dtype=torch.float64).requires_grad_(True)
    y = (1.0 - x.detach()).requires_grad_(True)
    factors = su.ms_ssim(x.detach().numpy(), y.detach().numpy())[2]
    assert (factors < -0.9).all()
    score = s.ms_ssim(x, y)
    assert torch.equal(score, torch.zeros(2, dtype=torch.float64))
    score.sum().backward()
    assert torch.equal(x.grad, torch.zeros_like(x)) and torch.equal(y.grad, torch.zeros_like(y))
    # independent uniform noise: means of either sign, planes of both kinds in one call
    a = torch.rand((6, 4, 24, 26), generator=rng, dtype=torch.float64).requires_grad_(True)
    b = torch.rand((6, 4, 24, 26), generator=rng, dtype=torch.float64)
    want, _, factors = su.ms_ssim(a.detach().numpy(), b.numpy())
    clamped = (factors <= 0).any(axis=1)
    assert clamped.any() and not clamped.all(), "this input is meant to mix clamped and kept planes"
    score = s.ms_ssim(a, b)
    assert np.abs(score.detach().numpy() - want).max() <= 1e-12
    score.sum().backward()
    grad = a.grad.reshape(24, -1)
    assert bool(torch.isfinite(grad).all())
    assert bool((grad[torch.from_numpy(clamped)] == 0).all()) and bool((grad[torch.from_numpy(~clamped)].abs().amax(dim=1) > 0).all())


KW = dict(device="cpu", batch_size=4, data_samples=16, no_rfp=True)


def test_diversity_tells_a_collapsed_set_from_a_varied_one():
    vm = _vm()
    for cls, planes in ((vm.MSSSIM, 1), (vm.MSSSIMVideo, 3)):
        torch.manual_seed(0)
        gen = StubGenerator(seed=5, collapsed=True)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            got = cls(**KW)(generator=gen, dataset=stub_dataset(4, 4))
        assert isinstance(got, tuple) and len(got) == 2 and gen.calls == 4                  # (bf, gfp)
        for score in got:
            assert score._fields == ("fake", "real", "gap") and score.gap == score.fake - score.real
            assert score.fake > score.real >= 0.0 and score.gap > 0.2
            # (MSSSIM draws its time step per batch, so pairs across batches compare different frames of the collapsed clip)
            assert planes == 1 or (score.fake > 0.9 > 0.1 > score.real and score.gap > 0.8)
        torch.manual_seed(0)
        back = cls(no_gfp=True, **KW)(generator=StubGenerator(seed=5), dataset=stub_dataset(4, 4, collapsed=True))
        assert back._fields == ("fake", "real", "gap") and back.real > back.fake >= 0.0 and back.gap < -0.2
        assert planes == 1 or (back.real > 0.9 > 0.1 > back.fake and back.gap < -0.8)


def test_diversity_is_the_free_function_on_the_seeded_pairs():
    vm, s = _vm(), _ssim()
    dataset = stub_dataset(4, 4)
    metric = vm.MSSSIMVideo(no_gfp=True, seed=3, pairs=5, **KW)
    got = metric(generator=StubGenerator(seed=5), dataset=dataset)
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(3))
    stub = StubGenerator(seed=5)
    sets = {"real": torch.cat(dataset)[:, 0], "fake": torch.cat([stub(torch.zeros(4, 6)) for _ in range(4)])[:, 0]}
    for name, planes in sets.items():
        want = su.ms_ssim(planes[perm[0:10:2]].numpy(), planes[perm[1:10:2]].numpy())[0].mean()
        assert getattr(got, name) == pytest.approx(want, abs=2e-5), name            # (the class scores fp32 planes in fp32)
    # equal seeds, equal scores; the real score is cached; another seed pairs differently
    def no_dataset():
        raise AssertionError("the real score is cached: the dataset is not swept again")
        yield
    again = metric(generator=StubGenerator(seed=5), dataset=no_dataset())
    assert again == got
    other = vm.MSSSIMVideo(no_gfp=True, seed=4, pairs=5, **KW)(generator=StubGenerator(seed=5), dataset=dataset)
    assert other.real != got.real
    with pytest.raises(TypeError):
        vm.MSSSIM(torch.nn.Identity(), network=None)


def test_short_dataset_warns_and_the_generator_sweep_follows_it():
    vm = _vm()
    metric = vm.MSSSIM(device="cpu", batch_size=4, data_samples=40, no_rfp=True, no_gfp=True)
    gen = StubGenerator()
    with pytest.warns(UserWarning, match="fewer than data_samples"):
        metric(generator=gen, dataset=stub_dataset(3, 4))
    assert metric.real[1] == 12 and gen.calls == 3


def test_wrapper_validation_logs_the_fields(golden):
    vm = _vm()
    _, _, _, trainer = _cpu_trainer(golden)
    trainer.generator_ema = StubGenerator()
    trainer.validation_metrics = (vm.MSSSIM(**KW), vm.MSSSIMVideo(no_gfp=True, **KW))
    best = trainer.best_fvd
    scores = trainer.validation(stub_dataset(4, 4))
    fields = ("fake", "real", "gap")
    assert sorted(scores) == sorted([f"MSSSIM_{f}_{c}" for f in fields for c in ("bf", "gfp")]
                                    + [f"MSSSIMVideo_{f}_bf" for f in fields])
    assert all(math.isfinite(v) for v in scores.values()) and trainer.best_fvd == best
    assert set(trainer.pop_logs()) >= set(scores)


def test_ssim_entries_are_declared_and_exported():
    from multi_stylegan_amd import _lib
    from multi_stylegan_amd.build import build
    build(verbose=False)
    handle = ctypes.CDLL(_lib.LIB_PATH)
    I, L, P, F = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p, ctypes.c_float
    want = {"msg_ssim_scale_workspace": (L, [I, I, I]),
            "msg_ssim_scale": (I, [P, P, I, I, I, F, F, P, P, P, P, P, P]),
            "msg_ssim_scale_backward": (I, [P, P, P, P, I, I, I, F, F, P, P])}
    for name, sig in want.items():
        assert name in _lib.declared_symbols() and hasattr(handle, name)
        assert _lib._SIGNATURES[name] == sig, name
    handle.msg_ssim_scale_workspace.restype = L
    assert handle.msg_ssim_scale_workspace(1, 11, 11) == 24 and handle.msg_ssim_scale_workspace(7, 17, 65) == 7 * 4 * 24
    assert handle.msg_ssim_scale_workspace(1, 10, 64) == -1 and handle.msg_ssim_scale_workspace(0, 64, 64) == -1
    assert handle.msg_ssim_scale_workspace(1 << 20, 1024, 4096) == -1              # 2^32 tiles
