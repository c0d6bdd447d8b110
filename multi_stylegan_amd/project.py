"""Embedding recorded sequences into the generator's W+ space -- what StyleGAN2 ships as ``projector.py``, with an image loss
that needs no feature network: MS-SSIM mixed with L1 (Zhao et al. 2017), both from the launches of ``ssim.ms_ssim``.

``mean_latent`` / ``truncate``: the centre of W and the truncation trick.  ``project_sequences``: Adam on W+ from the mean latent
on StyleGAN2's schedule (``projection_schedule``); the generator's parameters are frozen and its stored noise buffers are used,
noise maps are not optimised.  The projected W+ latents feed ``interpolation_frames`` / ``interpolation_video`` through
``anchors_are_latents=True``.  ``python -m multi_stylegan_amd.project`` projects sequences of a dataset directory.

The generator is used only through ``style_mapping``, ``latent_dimensions`` and ``forward(latent, input_is_latent=True,
randomize_noise=False)`` (once with ``return_main_style_vectors=True``, which tells the number of styled layers): any module with
that surface works, on its own device.
"""
import math
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from .ssim import ms_ssim

__all__ = ["Projection", "mean_latent", "truncate", "projection_schedule", "projection_loss", "project_sequences"]


class Projection(NamedTuple):
    latent: torch.Tensor                                # [B, n, D]: W+, one latent per styled layer
    loss: torch.Tensor                                  # [steps] on the host: the loss before each step
    image: torch.Tensor                                 # the generator's output at ``latent``


def _device_of(generator: nn.Module) -> torch.device:
    return next(generator.parameters()).device


@torch.no_grad()
def mean_latent(generator: nn.Module, samples: int = 10_000,
                generator_rng: Optional[torch.Generator] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(w_avg [D], w_std scalar)`` of ``style_mapping(z)`` over ``samples`` draws ``z ~ N(0, 1)`` (on the host, from
    ``generator_rng`` or the global generator): the mean, and ``sqrt(sum |w - w_avg|^2 / samples)`` as StyleGAN2's projector
    takes it."""
    device = _device_of(generator)
    z = torch.randn(int(samples), generator.latent_dimensions, generator=generator_rng).to(device)
    w = generator.style_mapping(z).float()
    w_avg = w.mean(dim=0)
    return w_avg, ((w - w_avg).square().sum() / float(samples)).sqrt()


def truncate(latent: torch.Tensor, w_avg: torch.Tensor, psi: float) -> torch.Tensor:
    """The truncation trick ``w_avg + psi (latent - w_avg)`` on W ``[..., D]`` or W+ ``[..., n, D]``; ``psi = 1`` returns the
    latent's bits and ``psi = 0`` the mean's."""
    return torch.lerp(w_avg.to(latent).expand_as(latent), latent, float(psi))


def projection_schedule(step: int, steps: int, lr: float = 0.1, w_noise: float = 0.05, w_std: float = 1.0) -> Tuple[float, float]:
    """StyleGAN2's projector schedule at ``t = step / steps`` -> ``(learning rate, latent noise scale)``: a linear warm-up over
    the first 5 %, a cosine ramp-down over the last 25 %, noise ``w_noise w_std max(0, 1 - t / 0.75)^2``."""
    t = step / steps
    ramp = min(1.0, (1.0 - t) / 0.25)
    ramp = 0.5 - 0.5 * math.cos(ramp * math.pi)
    ramp *= min(1.0, t / 0.05)
    return lr * ramp, w_noise * w_std * max(0.0, 1.0 - t / 0.75) ** 2


def projection_loss(image: torch.Tensor, target: torch.Tensor, alpha: float = 0.84, data_range: float = 1.0) -> torch.Tensor:
    """``[B, C, T, H, W]`` twice -> the mean over samples and planes of ``alpha (1 - ms_ssim) + (1 - alpha) mean |x - y|``."""
    B, C, T, H, W = target.shape
    score, l1 = ms_ssim(image.reshape(B, C * T, H, W).float(), target.reshape(B, C * T, H, W).float(), data_range=data_range,
                        return_l1=True)
    return (alpha * (1.0 - score) + (1.0 - alpha) * l1).mean()


def _generator_of(generator_or_checkpoint) -> nn.Module:
    if isinstance(generator_or_checkpoint, nn.Module):
        return generator_or_checkpoint
    from .samples import _device_of as cuda_device, _generator_of as load
    return load(generator_or_checkpoint, cuda_device(generator_or_checkpoint))


def project_sequences(generator_or_checkpoint, target: torch.Tensor, steps: int = 1000, lr: float = 0.1, alpha: float = 0.84,
                      w_noise: float = 0.05, seed: int = 0, data_range: float = 1.0, mean_samples: int = 10_000) -> Projection:
    """W+ latents ``[B, n, D]`` whose images are closest to ``target [B, C, T, H, W]`` under ``projection_loss``.

    Every latent starts at ``w_avg`` (``mean_latent`` on ``mean_samples`` draws from ``seed``); Adam (betas 0.9, 0.999) runs
    ``steps`` steps on ``projection_schedule``; before each forward the latent is perturbed by N(0, 1) noise of the schedule's
    scale, drawn on the host from ``seed``.  The generator's parameters are frozen (``requires_grad_(False)``: no weight gradient
    is computed) and stay so; its stored noise buffers are used.  Equal seeds give equal bits.  ``generator_or_checkpoint``: a
    module, or a checkpoint (path or dict) of the full-size generator."""
    generator = _generator_of(generator_or_checkpoint)
    device = _device_of(generator)
    generator.eval().requires_grad_(False)
    target = target.to(device=device, dtype=torch.float32)
    if target.ndim != 5:
        raise ValueError(f"expected [B, C, T, H, W] sequences, got {tuple(target.shape)}")
    rng = torch.Generator().manual_seed(int(seed))
    w_avg, w_std = mean_latent(generator, mean_samples, rng)
    w_std = float(w_std)
    probe = generator(w_avg[None], input_is_latent=True, randomize_noise=False, return_main_style_vectors=True)[1]
    latent = w_avg[None, None].repeat(target.shape[0], probe.shape[1], 1).clone().requires_grad_(True)
    optimizer = torch.optim.Adam([latent], lr=lr, betas=(0.9, 0.999))
    losses = []
    for step in range(int(steps)):
        rate, noise = projection_schedule(step, steps, lr, w_noise, w_std)
        for group in optimizer.param_groups:
            group["lr"] = rate
        w = latent if noise == 0.0 else latent + noise * torch.randn(latent.shape, generator=rng).to(device)
        image = generator(w, input_is_latent=True, randomize_noise=False)[:, :target.shape[1]]
        loss = projection_loss(image, target, alpha, data_range)
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        losses.append(loss.detach())
    with torch.no_grad():
        image = generator(latent.detach(), input_is_latent=True, randomize_noise=False)
    return Projection(latent.detach(), torch.stack(losses).cpu() if losses else torch.zeros(0), image)


# ----------------------------------------------------------------------------------------------------------- command line
def main(argv: Optional[Sequence[str]] = None) -> int:
    import argparse
    from .samples import SheetWriter, sample_sheets
    from .tlfm_dataset import TFLMDatasetGAN
    parser = argparse.ArgumentParser(prog="python -m multi_stylegan_amd.project", description=__doc__.split("\n\n")[0])
    parser.add_argument("--load_checkpoint", default="checkpoint_100.pt", type=str, help="Path to checkpoint to be loaded.")
    parser.add_argument("--data", required=True, type=str, help="Dataset directory (as TFLMDatasetGAN discovers it).")
    parser.add_argument("--samples", default=4, type=int, help="Number of sequences to project.")
    parser.add_argument("--out", required=True, type=str, help="Output directory.")
    parser.add_argument("--steps", default=1000, type=int)
    parser.add_argument("--seed", default=0, type=int)
    args = parser.parse_args(argv)
    dataset = TFLMDatasetGAN(path=args.data, raw=False, no_rfp=True, transformations=lambda frames: frames)    # (no flip draw)
    count = min(int(args.samples), len(dataset))
    target = torch.stack([torch.as_tensor(dataset[i]) for i in range(count)]).float()
    result = project_sequences(args.load_checkpoint, target, steps=args.steps, seed=args.seed)
    root = os.path.abspath(args.out)
    os.makedirs(root, exist_ok=True)
    torch.save({"latent": result.latent.cpu(), "loss": result.loss}, os.path.join(root, "latents.pt"))
    # target over projection, per channel, side by side in one sheet per sample
    channels = target.shape[1]
    both = torch.cat([sample_sheets(target.to(result.image.device)), sample_sheets(result.image[:, :channels].float())], dim=2)
    n, C, H, TW, _ = both.shape
    with SheetWriter(root) as writer:
        writer.submit([os.path.join(root, f"projection_{i}.png") for i in range(n)], both.reshape(n, C * H, TW, 3))
    print(f"{count} sequences projected into {root}: loss {float(result.loss[0]):.4f} -> {float(result.loss[-1]):.4f}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
