"""multi_stylegan_amd/project.py on the GPU: the package's tiny generator with the golden ``tiny_models`` weights against
``oracle.models.Generator`` with the same weights on the CPU -- the projector's loss and its latent gradient at step 0 at the fp32
gate of the README (1e-3 by ``conftest.rel_err``) -- a short run, and the projected W+ latents as interpolation anchors."""
import os

import numpy as np
import pytest
import torch

import png_util
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-3


@pytest.fixture(scope="module")
def pair(golden):
    """(the package's tiny generator on the GPU, the oracle's on the CPU with the same weights, a target the generator can reach)."""
    from oracle import models as om
    from test_hip_models import _models
    from tools.gen_golden import TINY_G
    z, g, _ = _models(golden)
    host = om.Generator(TINY_G)
    host.load_state_dict(z.state_dict("tinyG.sd."))
    g.eval().requires_grad_(False)
    host.eval().requires_grad_(False)
    with torch.no_grad():
        w_star = host.style_mapping(torch.randn(2, 16, generator=torch.Generator().manual_seed(12)))
        target = host(w_star, input_is_latent=True, randomize_noise=False)
    return g, host, target


def _frames(directory, count):
    assert sorted(os.listdir(directory)) == [f"frame_{i:05d}.png" for i in range(count)]
    return np.stack([png_util.decode(open(os.path.join(directory, f"frame_{i:05d}.png"), "rb").read()) for i in range(count)])


def test_step_zero_loss_and_latent_gradient_match_the_oracle(pair):
    from multi_stylegan_amd import project as p
    g, host, target = pair
    w_avg, w_std = p.mean_latent(host, 512, torch.Generator().manual_seed(3))
    got_avg, got_std = p.mean_latent(g, 512, torch.Generator().manual_seed(3))
    assert got_avg.device.type == "cuda" and rel_err(got_avg, w_avg) < TOL and rel_err(got_std, w_std) < TOL
    start = w_avg[None, None].repeat(2, 8, 1) + 0.1 * torch.randn(2, 8, 16, generator=torch.Generator().manual_seed(4))
    results = []
    for generator, device in ((host, "cpu"), (g, DEV)):
        latent = start.to(device).requires_grad_(True)
        image = generator(latent, input_is_latent=True, randomize_noise=False)
        loss = p.projection_loss(image, target.to(device))
        grad, = torch.autograd.grad(loss, latent)
        results.append((float(loss.detach()), grad.cpu(), image.detach().cpu()))
    (want_loss, want_grad, want_image), (got_loss, got_grad, got_image) = results
    print(f"loss {want_loss:.5f} / {got_loss:.5f}, gradient rel_err {rel_err(got_grad, want_grad):.2e}")
    assert rel_err(got_image, want_image) < TOL
    assert abs(got_loss - want_loss) < TOL * abs(want_loss) and want_loss > 0.05
    assert float(want_grad.abs().max()) > 0 and rel_err(got_grad, want_grad) < TOL
    assert all(q.grad is None for q in g.parameters())                       # frozen: no weight gradient was computed


def test_a_short_run_lowers_the_loss_and_its_latents_are_anchors(pair, tmp_path):
    from multi_stylegan_amd import interpolation_frames, interpolation_latents, sample_sheets
    from multi_stylegan_amd import project as p
    g, _, target = pair
    run = p.project_sequences(g, target, steps=40, seed=3, mean_samples=512)
    assert run.latent.shape == (2, 8, 16) and run.latent.device.type == "cuda" and run.loss.shape == (40,)
    print(f"loss {float(run.loss[0]):.4f} -> {float(run.loss[-1]):.4f}")
    assert bool(torch.isfinite(run.loss).all()) and float(run.loss[-1]) < float(run.loss[0])
    assert float(p.projection_loss(run.image, target.to(DEV))) < float(run.loss[0])
    # the two projected W+ latents as anchors: 2 x 5 frames, those of an eager forward on the interpolated W+
    out = str(tmp_path / "latent_frames")
    assert interpolation_frames(g, out, anchors=run.latent, steps_per_anchor=5, batch_size=10, use_graph=False,
                                anchors_are_latents=True) == 10
    latents = interpolation_latents(run.latent.reshape(2, -1), 5).reshape(10, 8, 16)
    assert torch.equal(latents[0], run.latent[0]) and torch.equal(latents[-1], run.latent[1])
    with torch.no_grad():
        image = g(latents.contiguous(), input_is_latent=True, randomize_noise=False)
    want = sample_sheets(image).reshape(10, 64, 96, 3).cpu().numpy()
    assert np.array_equal(_frames(out, 10), want)
    # W anchors [K, D] go the same way
    out_w = str(tmp_path / "w_frames")
    assert interpolation_frames(g, out_w, anchors=run.latent[:, 0], steps_per_anchor=2, batch_size=4, use_graph=False,
                                anchors_are_latents=True) == 4
    with torch.no_grad():
        image = g(interpolation_latents(run.latent[:, 0], 2).contiguous(), input_is_latent=True, randomize_noise=False)
    assert np.array_equal(_frames(out_w, 4), sample_sheets(image).reshape(4, 64, 96, 3).cpu().numpy())
    with pytest.raises(ValueError, match="anchors_are_latents"):
        interpolation_frames(g, out_w, anchors=3, anchors_are_latents=True)


def test_with_the_flag_off_the_frames_are_those_of_z_anchors(pair, tmp_path):
    from multi_stylegan_amd import interpolation_frames, interpolation_latents, sample_sheets
    g, _, _ = pair
    anchors = torch.randn(3, 16, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        image = g(interpolation_latents(anchors.to(DEV), 4).contiguous(), randomize_noise=False)
    want = sample_sheets(image).reshape(12, 64, 96, 3).cpu().numpy()
    for name, kw in (("default", {}), ("off", {"anchors_are_latents": False})):
        out = str(tmp_path / name)
        assert interpolation_frames(g, out, anchors=anchors, steps_per_anchor=4, batch_size=12, use_graph=False, **kw) == 12
        assert np.array_equal(_frames(out, 12), want)
    drawn = str(tmp_path / "drawn")
    assert interpolation_frames(g, drawn, anchors=3, steps_per_anchor=4, batch_size=12, seed=7, use_graph=False) == 12
    assert np.array_equal(_frames(drawn, 12), want)
