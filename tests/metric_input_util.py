"""The float64 statement of the metric inputs (multi_stylegan_amd.validation_metrics.metric_inputs, msg_metric_input), the
input builders and the derived tolerances shared by test_metric_input.py and test_hip_metric_input.py.

The resize restates torch's ``interpolate(mode="bilinear", align_corners=False, antialias=True)``: per axis a weight matrix
built from the filter's formula in float64, the resize ``Mh @ x @ Mw^T``.  It is written from the formula, not from the kernel's
integer form of it."""
import functools

import torch

#: (H, W) -> (out_h, out_w) on which the statement is checked against F.interpolate in float64
RESIZE_SHAPES = [((256, 256), (299, 299)), ((256, 256), (224, 224)), ((512, 512), (299, 299)), ((13, 20), (7, 9)),
                 ((7, 9), (13, 20)), ((20, 12), (5, 9)), ((33, 17), (8, 31))]


@functools.lru_cache(maxsize=None)
def axis_weights(n_in: int, n_out: int) -> torch.Tensor:
    """``[n_out, n_in]`` float64 (cached: not to be written to).
    scale = n_in / n_out, support = max(scale, 1), c = scale (i + 0.5), inv = 1 / support; taps
    j = max(int(c - support + 0.5), 0) .. min(int(c + support + 0.5), n_in) - 1, w_j = max(0, 1 - |j - c + 0.5| inv), divided
    by the sum of the taps used."""
    scale = n_in / n_out
    support = max(scale, 1.0)
    inv = 1.0 / support
    m = torch.zeros(n_out, n_in, dtype=torch.float64)
    for i in range(n_out):
        c = scale * (i + 0.5)
        lo, hi = max(int(c - support + 0.5), 0), min(int(c + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs(j - c + 0.5) * inv) for j in range(lo, hi)]
        total = sum(w)
        for j, v in zip(range(lo, hi), w):
            m[i, j] = v / total
    return m


def max_taps(n_in: int, n_out: int) -> int:
    """The largest number of taps with a positive weight any output index of the axis uses."""
    return int((axis_weights(n_in, n_out) > 0).sum(dim=1).max())


def resize(x: torch.Tensor, size) -> torch.Tensor:
    """``[..., H, W]`` -> float64 ``[..., size[0], size[1]]``."""
    x = x.double()
    return axis_weights(x.shape[-2], size[0]) @ x @ axis_weights(x.shape[-1], size[1]).t()


def normalise(x: torch.Tensor) -> torch.Tensor:
    """misc.normalize_m1_1_batch in float64 on ``[B, ...]``: per sample 2 max((x - lo) / (hi - lo), 1e-3) - 1."""
    flat = x.reshape(x.shape[0], -1)
    shape = (-1,) + (1,) * (x.ndim - 1)
    lo, hi = flat.min(dim=1)[0].reshape(shape), flat.max(dim=1)[0].reshape(shape)
    return 2.0 * ((x - lo) / (hi - lo)).clamp(min=1e-3) - 1.0


def span(x: torch.Tensor) -> torch.Tensor:
    """hi - lo per sample of ``[B, ...]``."""
    flat = x.reshape(x.shape[0], -1)
    return flat.max(dim=1)[0] - flat.min(dim=1)[0]


def reference(images: torch.Tensor, channel: int, t, size, normalize, planes: int = 3):
    """-> (float64 ``[B, planes, T', out_h, out_w]``, hi - lo per sample of what was normalised (None without a normalisation)).
    ``images`` are taken as stored (bf16 widens exactly); ``t`` None or -1: the whole clip."""
    x = images[:, channel].double()
    x = x if t is None or t < 0 else x[:, t:t + 1]
    size = tuple(x.shape[-2:]) if size is None else tuple(size)
    spread = None
    if normalize == "source":
        spread, x = span(x), normalise(x)
    x = resize(x, size)
    if normalize == "resized":
        spread, x = span(x), normalise(x)
    return x[:, None].expand(-1, planes, -1, -1, -1).contiguous(), spread


def frames(B: int, C: int, T: int, H: int, W: int, seed: int = 0, ranges=((0.0, 1.0), (-3.0, 5.0))) -> torch.Tensor:
    """fp32 ``[B, C, T, H, W]`` noise.  Sample ``b`` lives in ``ranges[b % len(ranges)]`` -- the samples' ranges differ, so a
    normalisation over the batch instead of the sample is a gross error -- and in every (c, t) plane of it one pixel is set to
    the range's lower and one to its upper end.  On top, plane (c, t) carries the offset ``0.25 (c T + t)``: a wrong plane is a
    gross error too."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(B, C, T, H, W, generator=gen)
    x[..., 0, 0], x[..., H - 1, W - 1] = 0.0, 1.0
    lo = torch.tensor([ranges[b % len(ranges)][0] for b in range(B)]).view(B, 1, 1, 1, 1)
    hi = torch.tensor([ranges[b % len(ranges)][1] for b in range(B)]).view(B, 1, 1, 1, 1)
    offset = 0.25 * torch.arange(C * T, dtype=torch.float32).view(1, C, T, 1, 1)
    return (lo + (hi - lo) * x + offset).contiguous()


def none_bound(size_in, size_out, peak: float) -> float:
    """|got - ref| of the fp32 resize without a normalisation: two convex combinations whose weights are a few ulp off,
    (taps_h + taps_w + 8) 2^-24 max|x|."""
    return (max_taps(size_in[0], size_out[0]) + max_taps(size_in[1], size_out[1]) + 8) * 2.0 ** -24 * peak


def normalised_bound(size_in, size_out, peak: float, spread: float) -> float:
    """The same through 2 (x - lo) / (hi - lo) - 1: the resize's bound times 2 / (hi - lo), plus four roundings of values in
    [-1, 1].  ``peak``: max|x| of what the filter sees in ``x``'s units; ``spread``: hi - lo of the float64 reference."""
    return none_bound(size_in, size_out, peak) * 2.0 / spread + 4 * 2.0 ** -24
