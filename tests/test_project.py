"""multi_stylegan_amd/project.py on the host: the projector on the oracle's tiny generator (any module with ``style_mapping``,
``latent_dimensions`` and ``forward(latent, input_is_latent=True, randomize_noise=False)`` works; the package's own generator has
no CPU path), the mean latent, the truncation trick and the schedule.  On the GPU: tests/test_hip_project.py."""
import math

import pytest
import torch


def _project():
    from multi_stylegan_amd import project
    return project


@pytest.fixture(scope="module")
def tiny():
    """oracle.models.Generator(TINY_G) with seeded weights (32 x 32 frames: two scales) and a target it can reach: G(w*)."""
    from oracle import models as om
    from tools.gen_golden import TINY_G
    torch.manual_seed(11)
    generator = om.Generator(TINY_G).eval()
    with torch.no_grad():
        w_star = generator.style_mapping(torch.randn(2, 16, generator=torch.Generator().manual_seed(12)))
        target = generator(w_star, input_is_latent=True, randomize_noise=False)
    assert target.shape == (2, 2, 3, 32, 32)
    return generator, target


def test_projection_lowers_the_loss_and_is_reproducible(tiny):
    p = _project()
    generator, target = tiny
    first = p.project_sequences(generator, target, steps=60, seed=3, mean_samples=512)
    assert first.latent.shape == (2, 8, 16) and first.loss.shape == (60,) and first.image.shape == target.shape
    assert not first.latent.requires_grad and all(not q.requires_grad for q in generator.parameters())
    print(f"loss {float(first.loss[0]):.4f} -> {float(first.loss[-1]):.4f}: {float(first.loss[-1] / first.loss[0]):.3f} x")
    assert float(first.loss[-1]) < 0.5 * float(first.loss[0])
    # the loss of the returned image is the last one's neighbour, not the start's
    assert float(p.projection_loss(first.image, target)) < 0.5 * float(first.loss[0])
    # equal seeds, equal bits
    runs = [p.project_sequences(generator, target, steps=12, seed=3, mean_samples=512) for _ in range(2)]
    assert torch.equal(runs[0].latent, runs[1].latent) and torch.equal(runs[0].loss, runs[1].loss)
    assert torch.equal(runs[0].image, runs[1].image)
    other = p.project_sequences(generator, target, steps=5, seed=4, mean_samples=512)
    assert not torch.equal(other.loss[:5], runs[0].loss[:5])
    with pytest.raises(ValueError, match="sequences"):
        p.project_sequences(generator, target[0], steps=1)


def test_step_zero_starts_from_the_mean_latent(tiny):
    p = _project()
    generator, target = tiny
    w_avg, w_std = p.mean_latent(generator, 512, torch.Generator().manual_seed(3))
    run = p.project_sequences(generator, target, steps=1, seed=3, mean_samples=512, w_noise=0.0)
    # one step at t = 0: the warm-up's learning rate is 0, the latent is still the mean on every layer
    assert torch.equal(run.latent, w_avg[None, None].expand(2, 8, 16))
    with torch.no_grad():
        image = generator(w_avg[None].repeat(2, 1), input_is_latent=True, randomize_noise=False)
    assert float(run.loss[0]) == pytest.approx(float(p.projection_loss(image, target)), rel=1e-6)


def test_mean_latent_and_truncation(tiny):
    p = _project()
    generator, _ = tiny
    w_avg, w_std = p.mean_latent(generator, 2000, torch.Generator().manual_seed(0))
    z = torch.randn(2000, 16, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        w = generator.style_mapping(z)
    assert w_avg.shape == (16,) and w_std.ndim == 0
    assert torch.allclose(w_avg, w.mean(dim=0), atol=1e-6)
    assert float(w_std) == pytest.approx(float(((w - w.mean(dim=0)) ** 2).sum().div(2000).sqrt()), rel=1e-5)
    again = p.mean_latent(generator, 2000, torch.Generator().manual_seed(0))
    assert torch.equal(again[0], w_avg) and torch.equal(again[1], w_std)
    for latent in (w[:5], w[:24].reshape(3, 8, 16)):                           # W and W+
        assert torch.equal(p.truncate(latent, w_avg, 1.0), latent)
        assert torch.equal(p.truncate(latent, w_avg, 0.0), w_avg.expand_as(latent))
        half = p.truncate(latent, w_avg, 0.5)
        assert torch.allclose(half, w_avg + 0.5 * (latent - w_avg), atol=1e-6)


def test_schedule_endpoints():
    p = _project()
    lr, noise = p.projection_schedule(0, 1000, lr=0.1, w_noise=0.05, w_std=2.0)
    assert lr == 0.0 and noise == pytest.approx(0.05 * 2.0)
    assert p.projection_schedule(25, 1000, lr=0.1)[0] == pytest.approx(0.05)   # half way up the warm-up
    for step in (50, 400, 750):
        assert p.projection_schedule(step, 1000, lr=0.1)[0] == pytest.approx(0.1)
    assert p.projection_schedule(750, 1000, w_noise=0.05, w_std=2.0)[1] == 0.0
    assert p.projection_schedule(900, 1000)[1] == 0.0
    assert p.projection_schedule(375, 1000, w_noise=0.05, w_std=2.0)[1] == pytest.approx(0.1 * 0.25)
    assert p.projection_schedule(875, 1000, lr=0.1)[0] == pytest.approx(0.05)  # the cosine's middle
    last = p.projection_schedule(999, 1000, lr=0.1)[0]
    assert 0.0 < last < 1e-5 and last == pytest.approx(0.1 * (0.5 - 0.5 * math.cos(0.004 * math.pi)))
