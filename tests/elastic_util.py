"""Shared by tests/test_elastic.py and tests/test_hip_elastic.py: the recorded cases of tests/golden/elastic.npz
(tools/gen_golden_elastic.py) and a float64 restatement of the reference's elastic deformation (dataset/tlfm_dataset.py:230-275),
written from its formulas with explicit indices -- no conv2d, no grid_sample."""
import math
import os

import numpy as np
import torch

from conftest import GOLDEN

CASES = ("defaults", "even", "nonsquare", "odd", "tiny")
_FIXTURE = {}


def fixture():
    """tests/golden/elastic.npz, loaded once and shared (read-only)."""
    if not _FIXTURE:
        with np.load(os.path.join(GOLDEN, "elastic.npz")) as z:
            _FIXTURE.update({k: z[k] for k in z.files})
        for a in _FIXTURE.values():
            a.setflags(write=False)
    return _FIXTURE


def case(name):
    """-> dict(frames [F, H, W], noise [2, H, W], out [F, H, W], next [1] as float32 tensors (copies); seed, sigma, alpha ints)."""
    z = fixture()
    seed, sigma, alpha = (int(v) for v in z[name + ".params"])
    got = {k: torch.from_numpy(z[f"{name}.{k}"].copy()) for k in ("frames", "noise", "out", "next")}
    got.update(seed=seed, sigma=sigma, alpha=alpha)
    return got


def taps64(sigma):
    i = torch.arange(4 * sigma + 1, dtype=torch.float64) - 2 * sigma
    return torch.exp(-i * i / (2.0 * sigma * sigma)) / (math.sqrt(2.0 * math.pi) * sigma)


def field64(noise, sigma, alpha):
    """[..., H, W] noise -> float64 d = alpha sum_i sum_j g[i] g[j] n[y + i - 2 sigma, x + j - 2 sigma], zero outside the frame:
    the truncated, un-normalised Gaussian as two banded matrices, d = alpha Gy n Gx^T."""
    n = noise.double()
    g = taps64(sigma)
    height, width = n.shape[-2:]

    def band(size):
        at = torch.arange(size)
        offset = at[None, :] - at[:, None] + 2 * sigma            # tap index of source `col` for output `row`
        inside = (offset >= 0) & (offset <= 4 * sigma)
        return torch.where(inside, g[offset.clamp(0, 4 * sigma)], torch.zeros((), dtype=torch.float64))

    return alpha * (band(height) @ n @ band(width).transpose(0, 1))


def positions64(field):
    """[2, H, W] float64 displacements -> (px, py) float64 [H, W], clamped to the frame (border padding).  The x coordinate is
    divided by the height and the y coordinate by the width, as the reference does."""
    height, width = field.shape[-2:]
    ys = torch.arange(height, dtype=torch.float64).view(height, 1)
    xs = torch.arange(width, dtype=torch.float64).view(1, width)
    gx = 2.0 * (xs + field[0] - (height // 2)) / height
    gy = 2.0 * (ys + field[1] - (width // 2)) / width
    px = ((gx + 1.0) * width - 1.0) / 2.0
    py = ((gy + 1.0) * height - 1.0) / 2.0
    return px.clamp(0.0, width - 1.0), py.clamp(0.0, height - 1.0)


def deform64(frames, noise, sigma, alpha, return_field=False):
    """frames [F, H, W], noise [2, H, W] -> float64 [F, H, W]: the bilinear mix of floor and floor + 1 (upper index clamped)."""
    x = frames.double()
    height, width = x.shape[-2:]
    field = field64(noise, sigma, alpha)
    px, py = positions64(field)
    x0, y0 = px.floor(), py.floor()
    ax, ay = px - x0, py - y0
    ix0, iy0 = x0.long(), y0.long()
    ix1, iy1 = (ix0 + 1).clamp(max=width - 1), (iy0 + 1).clamp(max=height - 1)
    out = (x[:, iy0, ix0] * ((1 - ax) * (1 - ay)) + x[:, iy0, ix1] * (ax * (1 - ay))
           + x[:, iy1, ix0] * ((1 - ax) * ay) + x[:, iy1, ix1] * (ax * ay))
    return (out, field) if return_field else out


def deform64_batch(frames, noise, sigma, alpha):
    """frames [B, F, H, W], noise [B, 2, H, W] -> (out, field) float64, sample by sample."""
    pairs = [deform64(f, n, sigma, alpha, return_field=True) for f, n in zip(frames, noise)]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    view = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))
