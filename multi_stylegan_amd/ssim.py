"""Multi-scale structural similarity (Wang et al. 2003) between frames: the primitive under the diversity metrics
``validation_metrics.MSSSIM`` / ``MSSSIMVideo`` and under the image loss of ``project.py`` ("MS-SSIM").

Definitions.  Window: 11 taps ``g_k = exp(-(k - 5)^2 / (2 1.5^2)) / sum``, separable, "valid" -- a plane ``h x w`` has
``(h - 10)(w - 10)`` positions.  With ``C1 = (0.01 R)^2``, ``C2 = (0.03 R)^2``, ``R = data_range``, per position::

    mu_x = g*x, mu_y = g*y, s_xx = g*x^2 - mu_x^2, s_yy = g*y^2 - mu_y^2, s_xy = g*xy - mu_x mu_y
    cs = (2 s_xy + C2) / (s_xx + s_yy + C2),   l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1),   ssim = cs l

``ssim_levels(h, w)`` scales (at most 5); between scales both planes are halved by the 2 x 2 mean (an odd trailing row or column
is dropped); the weights are the first ``L`` of ``MS_SSIM_WEIGHTS`` renormalised to sum 1.  A plane scores ``prod_(j < L-1)
max(0, mean cs_j)^(w_j) * max(0, mean ssim_(L-1))^(w_(L-1))``; a plane with a factor clamped to 0 scores exactly 0 and passes
exactly zero gradient (masked: ``clamp`` followed by ``pow`` would pass NaN).  A sample ``[P, H, W]`` scores the mean over its
planes.

fp32 tensors on the GPU: ``msg_ssim_scale`` per scale (csrc/ssim.hip; the sums of cs and ssim, the L1 sum and the halved planes
in one launch, float64 sums in a fixed order) and ``msg_ssim_scale_backward`` per scale and differentiated argument, behind one
``autograd.Function``; the combination of the scales stays in torch on ``[N P, L]`` float64 values.  CPU tensors take the
plain-torch statement of the same definitions in their own dtype, differentiable by autograd.
"""
from typing import Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib

__all__ = ["MS_SSIM_WEIGHTS", "ssim_levels", "ssim_window", "ms_ssim"]

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
_TAPS, _SIGMA, _MAX_LEVELS = 11, 1.5, len(MS_SSIM_WEIGHTS)


def ssim_levels(h: int, w: int) -> int:
    """How many times ``min(h, w) >= 11`` holds while halving (floor), at most 5."""
    levels = 0
    while min(h, w) >= _TAPS and levels < _MAX_LEVELS:
        levels, h, w = levels + 1, h // 2, w // 2
    return levels


def ssim_window(dtype: torch.dtype = torch.float64) -> torch.Tensor:
    """The 11 taps, computed in float64 and rounded once to ``dtype``."""
    k = torch.arange(_TAPS, dtype=torch.float64)
    g = torch.exp(-(k - _TAPS // 2) ** 2 / (2.0 * _SIGMA ** 2))
    return (g / g.sum()).to(dtype)


def _level_weights(levels: int) -> torch.Tensor:
    w = torch.tensor(MS_SSIM_WEIGHTS[:levels], dtype=torch.float64)
    return w / w.sum()


def _host_scales(x: torch.Tensor, y: torch.Tensor, levels: int, c1: float, c2: float):
    """``x, y [M, h, w]`` -> ``(mean cs [M, L], mean ssim [M, L], mean |x - y| [M])`` in the tensors' dtype: stock operators."""
    win = ssim_window(x.dtype).to(x.device)
    rows, cols = win.view(1, 1, 1, _TAPS), win.view(1, 1, _TAPS, 1)

    def blur(v):
        return F.conv2d(F.conv2d(v, rows), cols)

    x, y = x[:, None], y[:, None]
    l1 = (x - y).abs().mean(dim=(1, 2, 3))
    cs_means, ss_means = [], []
    for level in range(levels):
        mu_x, mu_y = blur(x), blur(y)
        s_xx, s_yy, s_xy = blur(x * x) - mu_x * mu_x, blur(y * y) - mu_y * mu_y, blur(x * y) - mu_x * mu_y
        cs = (2.0 * s_xy + c2) / (s_xx + s_yy + c2)
        lum = (2.0 * mu_x * mu_y + c1) / (mu_x * mu_x + mu_y * mu_y + c1)
        cs_means.append(cs.mean(dim=(1, 2, 3)))
        ss_means.append((cs * lum).mean(dim=(1, 2, 3)))
        if level + 1 < levels:
            x, y = F.avg_pool2d(x, 2), F.avg_pool2d(y, 2)
    return torch.stack(cs_means, dim=1), torch.stack(ss_means, dim=1), l1


def _workspace(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


class _SsimScales(torch.autograd.Function):
    """``x, y [M, H, W]`` fp32 on the GPU -> float64 ``(mean cs [M, L], mean ssim [M, L], mean |x - y| [M])``: ``L`` launches of
    ``msg_ssim_scale``; backward: ``L`` launches of ``msg_ssim_scale_backward`` per argument that needs a gradient, coarsest
    scale first, each handing its ``grad_x`` down as the next one's ``g_half``."""

    @staticmethod
    def forward(ctx, x, y, levels, c1, c2):
        dev = _lib.require_gpu(x, y)
        lib = _lib.lib()
        M = x.shape[0]
        pyramid, cs, ss = [], [], []
        l1 = torch.empty(M, dtype=torch.float64, device=dev)
        with _lib.on_device(dev):
            stream = _lib.stream_of(dev)
            for level in range(levels):
                h, w = x.shape[1:]
                sums = torch.empty((M, 2), dtype=torch.float64, device=dev)
                ws = _workspace(lib.msg_ssim_scale_workspace(M, h, w), dev)
                last = level + 1 == levels
                xh = None if last else torch.empty((M, h // 2, w // 2), dtype=torch.float32, device=dev)
                yh = None if last else torch.empty_like(xh)
                with _lib.kernel_clock.span(("ssim_scale", h, w), 4.0 * (2.0 if last else 2.5) * x.numel()):
                    _lib.check(lib.msg_ssim_scale(x.data_ptr(), y.data_ptr(), M, h, w, c1, c2, sums.data_ptr(),
                                                  l1.data_ptr() if level == 0 else None, _lib.ptr(xh), _lib.ptr(yh),
                                                  ws.data_ptr(), stream), "msg_ssim_scale")
                means = sums / float((h - 10) * (w - 10))
                cs.append(means[:, 0])
                ss.append(means[:, 1])
                pyramid.append((x, y))
                x, y = xh, yh
        ctx.save_for_backward(*[t for level in pyramid for t in level])
        ctx.constants = (c1, c2)
        h, w = pyramid[0][0].shape[1:]
        return torch.stack(cs, dim=1), torch.stack(ss, dim=1), l1 / float(h * w)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cs, g_ss, g_l1):
        c1, c2 = ctx.constants
        saved = ctx.saved_tensors
        pyramid = [(saved[2 * level], saved[2 * level + 1]) for level in range(len(saved) // 2)]
        dev = pyramid[0][0].device
        lib = _lib.lib()
        M, levels = pyramid[0][0].shape[0], len(pyramid)
        g = torch.zeros((levels, M, 3), dtype=torch.float32, device=dev)
        g[:, :, 0], g[:, :, 1] = g_cs.t(), g_ss.t()
        g[0, :, 2] = g_l1
        grads = [None, None]
        with _lib.on_device(dev):
            stream = _lib.stream_of(dev)
            for which in range(2):
                if not ctx.needs_input_grad[which]:
                    continue
                below = None
                for level in reversed(range(levels)):
                    a, b = pyramid[level][which], pyramid[level][1 - which]
                    out = torch.empty_like(a)
                    h, w = a.shape[1:]
                    with _lib.kernel_clock.span(("ssim_scale_backward", h, w), 4.0 * 3.0 * a.numel()):
                        _lib.check(lib.msg_ssim_scale_backward(a.data_ptr(), b.data_ptr(), g[level].data_ptr(), _lib.ptr(below),
                                                               M, h, w, c1, c2, out.data_ptr(), stream),
                                   "msg_ssim_scale_backward")
                    below = out
                grads[which] = below
        return grads[0], grads[1], None, None, None


def ms_ssim(x: torch.Tensor, y: torch.Tensor, levels: Optional[int] = None, data_range: float = 1.0,
            return_l1: bool = False) -> Union[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]:
    """``x, y [N, P, H, W]`` -> the per-sample MS-SSIM ``[N]`` (the mean over the ``P`` planes), in the inputs' dtype; with
    ``return_l1`` also the per-sample mean ``|x - y|``, from the same launches.  ``levels``: 1 .. ``ssim_levels(H, W)`` (the
    default).  Differentiable in both arguments (once).  On the GPU the tensors are fp32 -- cast bf16 frames first."""
    if x.ndim != 4 or x.shape != y.shape:
        raise ValueError(f"expected two [N, P, H, W] tensors of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    if x.dtype != y.dtype or x.device != y.device:
        raise ValueError(f"x is {x.dtype} on {x.device}, y is {y.dtype} on {y.device}")
    N, P, H, W = x.shape
    most = ssim_levels(H, W)
    levels = most if levels is None else int(levels)
    if most < 1 or not 1 <= levels <= most:
        raise ValueError(f"{H} x {W} planes carry {most} scale(s) of an 11-tap window, not {levels}")
    data_range = float(data_range)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    if x.is_cuda:
        if x.dtype != torch.float32:
            raise _lib.MsgHipError(f"ms_ssim on the GPU takes float32 frames, not {x.dtype}: cast them first")
        cs, ss, l1 = _SsimScales.apply(x.contiguous().view(N * P, H, W), y.contiguous().view(N * P, H, W), levels, c1, c2)
    else:
        cs, ss, l1 = _host_scales(x.reshape(N * P, H, W), y.reshape(N * P, H, W), levels, c1, c2)
    # the combination: [N P, L] values.  Masked, not clamped: d/dv max(0, v)^w at a clamped v is 0 * inf in autograd
    factors = torch.cat([cs[:, :levels - 1], ss[:, levels - 1:]], dim=1)
    kept = (factors > 0).all(dim=1)
    safe = torch.where(kept[:, None], factors, torch.ones_like(factors))
    score = torch.where(kept, safe.pow(_level_weights(levels).to(safe)).prod(dim=1), torch.zeros_like(safe[:, 0]))
    score = score.view(N, P).mean(dim=1).to(x.dtype)
    if return_l1:
        return score, l1.view(N, P).mean(dim=1).to(x.dtype)
    return score
