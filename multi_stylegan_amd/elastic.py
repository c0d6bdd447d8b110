"""Random elastic deformation: the reference's one augmentation besides the horizontal flip (dataset/tlfm_dataset.py:201-275).

* ``elastic_deformation`` / ``ElasticDeformation``: the reference's function and module, same signatures, shapes and random
  draws.  CPU tensors go through stock torch operators (with the blur done separably: the reference's (4 sigma + 1)^2 kernel is
  exactly ``g (x) g``), so the module is a drop-in ``transformations`` callable of ``TFLMDatasetGAN(..., raw=False)`` on a
  machine without a GPU; device tensors go through ``elastic_deform_batch``.
* ``elastic_deform_batch``: a whole batch on the GPU in one ``msg_elastic_deform`` call (csrc/elastic.hip): a separable blur of
  the noise field and a gather that computes a position's indices and weights once for all frames of the sample.
  ``data.TLFMDeviceFeed(..., elastic=ElasticDeformation(...))`` applies it to every batch of the raw-count feed.

The formulation, with the reference's quirks (all kept): the noise is two ``torch.rand((H, W)) * 2 - 1`` draws, the FIRST the
horizontal component; the Gaussian is truncated at +-2 sigma and not renormalised; zero padding; the x coordinate is divided by
the height and the y coordinate by the width; ``grid_sample(padding_mode='border', align_corners=False)``, which on an even
square frame shifts the picture by half a pixel.
"""
import math
from typing import Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib


def gaussian_taps(sigma: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """``g[i] = exp(-(i - 2 sigma)^2 / (2 sigma^2)) / (sqrt(2 pi) sigma)``, i = 0 .. 4 sigma (computed in float64)."""
    i = torch.arange(4 * sigma + 1, dtype=torch.float64) - 2 * sigma
    return (torch.exp(-i * i / (2.0 * sigma * sigma)) / (math.sqrt(2.0 * math.pi) * sigma)).to(dtype)


def _check_sigma(sigma) -> int:
    if int(sigma) != sigma or sigma < 1:
        raise ValueError(f"sigma {sigma!r}: an integer >= 1 (the kernel has 4 sigma + 1 taps)")
    return int(sigma)


def displacement_field(noise: torch.Tensor, alpha: float, sigma: int) -> torch.Tensor:
    """``[..., H, W]`` noise planes -> ``alpha *`` their zero-padded blur with ``g (x) g``, in stock torch (row pass, then
    column pass), in the noise's dtype."""
    g = gaussian_taps(sigma, noise.dtype).to(noise.device)
    planes = noise.reshape(-1, 1, *noise.shape[-2:])
    planes = F.conv2d(planes, g.view(1, 1, 1, -1), padding=(0, 2 * sigma))
    planes = F.conv2d(planes, g.view(1, 1, -1, 1), padding=(2 * sigma, 0))
    return planes.reshape(noise.shape) * alpha


def sampling_grid(field: torch.Tensor) -> torch.Tensor:
    """``[2, H, W]`` displacements in pixels -> the reference's ``[1, H, W, 2]`` grid (dataset/tlfm_dataset.py:263-270): x divided
    by the height, y by the width."""
    height, width = field.shape[-2:]
    ys = torch.arange(height, dtype=field.dtype, device=field.device).view(height, 1).expand(height, width)
    xs = torch.arange(width, dtype=field.dtype, device=field.device).view(1, width).expand(height, width)
    gx = 2 * (xs + field[0] - (height // 2)) / height
    gy = 2 * (ys + field[1] - (width // 2)) / width
    return torch.stack([gx, gy], dim=-1).unsqueeze(0)


def _frames_3d(img: torch.Tensor) -> torch.Tensor:
    if img.ndim == 4 and img.shape[0] == 1:
        return img[0]
    if img.ndim != 3:
        raise ValueError(f"expected [F, H, W] frames (or [1, F, H, W]), got {tuple(img.shape)}")
    return img


def _deform(img: torch.Tensor, sample_mode: str, alpha, sigma, generator: Optional[torch.Generator]) -> torch.Tensor:
    frames = _frames_3d(img)
    sigma = _check_sigma(sigma)
    height, width = frames.shape[-2:]
    on_host = frames.device.type == "cpu"
    if not on_host and sample_mode != "bilinear":
        raise ValueError(f"sample_mode {sample_mode!r}: the device path samples bilinearly only (move the frames to the CPU for "
                         "any other mode of grid_sample)")
    if height == 0 or width == 0:
        raise ValueError(f"empty frames {tuple(img.shape)}")
    # the reference's two draws, in its order: horizontal component first (dataset/tlfm_dataset.py:257-258)
    noise = torch.stack([torch.rand((height, width), dtype=torch.float, device=frames.device, generator=generator) * 2. - 1.
                         for _ in range(2)])
    if not on_host:
        return elastic_deform_batch(frames[None], noise[None], alpha=alpha, sigma=sigma)[0]
    grid = sampling_grid(displacement_field(noise, alpha, sigma))
    return F.grid_sample(frames[None], grid.to(frames.dtype), mode=sample_mode, padding_mode="border", align_corners=False)[0]


def elastic_deformation(img: torch.Tensor, sample_mode: str = "bilinear", alpha: int = 50, sigma: int = 12) -> torch.Tensor:
    """The reference's ``elastic_deformation`` (dataset/tlfm_dataset.py:230-275): ``img`` ``[F, H, W]`` (or ``[1, F, H, W]``) ->
    ``[F, H, W]``, every frame resampled along one random smooth displacement field; the two noise planes are drawn with
    ``torch.rand((H, W))`` on the image's device from the global generator, as there, so equal seeds give the reference's
    result (to fp32 rounding: the blur is separable here).

    CPU tensors: stock torch operators, any ``sample_mode`` that ``grid_sample`` takes.  Device tensors:
    ``elastic_deform_batch`` -- ``"bilinear"`` only, anything else is a ValueError."""
    return _deform(img, sample_mode, alpha, sigma, None)


class ElasticDeformation(nn.Module):
    """The reference's module (dataset/tlfm_dataset.py:201-227) with its defaults; ``generator`` (the one addition) is where the
    noise is drawn from, None = the global generator of the frames' device.  Usable as ``TFLMDatasetGAN(...,
    transformations=ElasticDeformation())`` with ``raw=False`` (no GPU needed), and as ``TLFMDeviceFeed(..., elastic=...)``."""

    def __init__(self, sample_mode: str = "bilinear", alpha: int = 80, sigma: int = 16,
                 generator: Optional[torch.Generator] = None) -> None:
        super().__init__()
        self.sample_mode = sample_mode
        self.alpha = alpha
        self.sigma = _check_sigma(sigma)
        self.generator = generator

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        return _deform(input, self.sample_mode, self.alpha, self.sigma, self.generator)

    def deform_batch(self, frames: torch.Tensor) -> torch.Tensor:
        """A device batch ``[B, C, T, H, W]`` / ``[B, F, H, W]``, one field per sample, noise from this module's generator."""
        if self.sample_mode != "bilinear":
            raise ValueError(f"sample_mode {self.sample_mode!r}: the device path samples bilinearly only")
        return elastic_deform_batch(frames, alpha=self.alpha, sigma=self.sigma, generator=self.generator)


def elastic_deform_batch(frames: torch.Tensor, noise: Optional[torch.Tensor] = None, *, alpha, sigma,
                         generator: Optional[torch.Generator] = None, return_field: bool = False):
    """``frames`` ``[B, C, T, H, W]`` or ``[B, F, H, W]`` (float32 or bfloat16, on the GPU) -> a fresh tensor of the same shape
    and dtype, every sample deformed along its own field (shared by all of its frames) by one ``msg_elastic_deform`` call on the
    current stream.  ``noise`` ``[B, 2, H, W]`` float32 in [-1, 1), plane 0 the horizontal component; None draws
    ``torch.rand((B, 2, H, W), device=..., generator=generator) * 2 - 1``.  ``return_field``: also the displacement field
    ``[B, 2, H, W]`` float32, in pixels.  Frames that require grad are refused: this augments real data."""
    if frames.ndim not in (4, 5):
        raise ValueError(f"expected [B, C, T, H, W] or [B, F, H, W] frames, got {tuple(frames.shape)}")
    if frames.requires_grad or (noise is not None and noise.requires_grad):
        raise ValueError("elastic deformation augments real data: there is no autograd through it (detach the frames)")
    if frames.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"frames are float32 or bfloat16, got {frames.dtype}")
    sigma = _check_sigma(sigma)
    if sigma > _lib.MSG_ELASTIC_MAX_SIGMA:
        raise ValueError(f"sigma {sigma}: the device kernels' halo holds sigma <= {_lib.MSG_ELASTIC_MAX_SIGMA}")
    B, (H, W) = frames.shape[0], frames.shape[-2:]
    if noise is not None and (tuple(noise.shape) != (B, 2, H, W) or noise.dtype != torch.float32):
        raise ValueError(f"noise is float32 [B, 2, H, W] = {(B, 2, H, W)}, got {noise.dtype} {tuple(noise.shape)}")
    dev = _lib.require_gpu(frames, noise)
    if noise is None:
        noise = torch.rand((B, 2, H, W), device=dev, generator=generator) * 2 - 1
    src, noise = frames.contiguous(), noise.contiguous()
    out = torch.empty_like(src)
    field = torch.empty((B, 2, H, W), dtype=torch.float32, device=dev)
    if src.numel():
        n_frames = src.numel() // (B * H * W)
        lib = _lib.lib()
        with _lib.on_device(dev):
            ws = _lib.scratch_ptr((lib.msg_elastic_workspace(B, H, W) + 3) // 4, dev)
            with _lib.kernel_clock.span(("elastic_deform", src.dtype), 24.0 * B * H * W + 2.0 * src.numel() * src.element_size()):
                _lib.check(lib.msg_elastic_deform(src.data_ptr(), noise.data_ptr(), field.data_ptr(), out.data_ptr(),
                                                  _lib.dtype_code(src), B, n_frames, H, W, sigma, float(alpha), ws,
                                                  _lib.stream_of(dev)), "msg_elastic_deform")
    return (out, field) if return_field else out
