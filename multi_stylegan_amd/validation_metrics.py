"""Sample-quality statistics of the validation pass (reference multi_stylegan/validation_metrics.py, call site
model_wrapper.py:197-243): inception score, Frechet inception distance, Frechet video distance.

What is here is the part of that file that is arithmetic: the per-channel frame selection, the feature sweeps over the
dataset and the EMA generator, and the statistics on the features.  What is NOT here are the feature networks: the
reference instantiates torchvision's pretrained Inception-v3 and a pretrained I3D (validation_metrics.py:48, 571-650) whose
weights are missing blobs of the reference repository and cannot be downloaded -- every metric class therefore takes the
network as an argument (any ``nn.Module`` mapping a ``[B, 3, H, W]`` image / ``[B, 3, T, H, W]`` clip batch in [-1, 1] to
features or logits); with the pretrained networks supplied the classes compute the reference's numbers.  The tensor the
network receives is made here: ``metric_inputs`` selects the channel and the time step (or the clip), resizes to the network's
input size and normalises in the reference's order, in one ``msg_metric_input`` call (csrc/metric_input.hip) on the GPU.

MI355X-first: the statistics stay on the GPU.  The reference moves every activation to the host, stacks 5000 x 2048
arrays and calls numpy / scipy.  Here a feature sweep folds each batch into running first and second moments (float64, one
``[d, d]`` GEMM per batch on the device), and tr(sqrtm(C_r C_f)) is taken as the sum of the square roots of the eigenvalues
of the SYMMETRIC matrix C_r^(1/2) C_f C_r^(1/2) (same spectrum as C_r C_f; ``eigh`` on the device, no complex arithmetic,
eigenvalues clamped at zero where scipy's ``sqrtm(...).real`` drops an imaginary part).
"""
import collections
import functools
import math
import warnings
from typing import Iterable, NamedTuple, Optional, Tuple, Union

import torch
import torch.distributed as torch_dist
import torch.nn as nn

from . import _lib, misc
from .ssim import ms_ssim


def _ranks() -> int:
    """Ranks that share a validation pass: in a data-parallel job every rank sweeps 1 / world of the samples (its own shard
    of the dataset, its own latents) and the additive statistics are summed over the ranks -- the reference runs the pass once,
    on the gathered DataParallel model (model_wrapper.py:197-243); repeating the whole pass per rank was world x the work."""
    return torch_dist.get_world_size() if torch_dist.is_available() and torch_dist.is_initialized() else 1

__all__ = ["IS", "FID", "FVD", "FeatureMoments", "frechet_distance", "frechet_distance_from_moments", "inception_score",
           "metric_inputs", "select_frames", "KID", "KVD", "PrecisionRecall", "PrecisionRecallVideo", "FeatureRows",
           "ManifoldScores", "kernel_distance", "manifold_scores", "subset_indices", "SWD", "SWVD", "laplacian_pyramid",
           "swd_positions", "swd_descriptors", "swd_directions", "sliced_wasserstein", "MSSSIM", "MSSSIMVideo", "DiversityScore"]


def select_frames(images: torch.Tensor, channel: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """validation_metrics.py:93-94, 246-247: channel ``c`` of ONE random time step of the batch (one ``torch.randint`` draw
    from the global CPU generator, like the reference), replicated on three colour planes: [B, C, T, H, W] -> [B, 3, 1, H, W]."""
    t = torch.randint(0, images.shape[2], (1,), generator=generator)
    return images[:, channel, t.to(images.device)].unsqueeze(dim=1).repeat_interleave(dim=1, repeats=3)


def select_clips(images: torch.Tensor, channel: int) -> torch.Tensor:
    """validation_metrics.py:451-452: the whole sequence of channel ``c`` on three colour planes: -> [B, 3, T, H, W]."""
    return images[:, channel].unsqueeze(dim=1).repeat_interleave(dim=1, repeats=3)


# ------------------------------------------------------------------------------------------------------------ metric inputs
def _draw_time_step(images: torch.Tensor) -> int:
    """The draw of ``select_frames``: one ``torch.randint`` from the global CPU generator per selected batch."""
    return int(torch.randint(0, images.shape[2], (1,)))


_NORM_CODES = {None: "MSG_METRIC_NORM_NONE", "source": "MSG_METRIC_NORM_SOURCE", "resized": "MSG_METRIC_NORM_RESIZED"}


@functools.lru_cache(maxsize=16)
def _resize_weights(n_in: int, n_out: int) -> torch.Tensor:
    """``[n_out, n_in]`` fp32: row ``i`` holds the weights of torch's ``interpolate(mode="bilinear", align_corners=False,
    antialias=True)`` for output index ``i`` -- the triangle ``max(0, 1 - |j + 0.5 - c| / support)``, ``c = (i + 0.5) n_in / n_out``,
    ``support = max(n_in / n_out, 1)``, over the sum of the row.  Formed as the kernel forms them (csrc/metric_input.hip): the integer
    numerators ``D - |n_out (2j + 1) - n_in (2i + 1)|``, ``D = 2 max(n_in, n_out)``, divided by their integer sum and rounded once."""
    i = torch.arange(n_out, dtype=torch.int64)[:, None]
    j = torch.arange(n_in, dtype=torch.int64)[None, :]
    u = (2 * max(n_in, n_out) - (n_out * (2 * j + 1) - n_in * (2 * i + 1)).abs()).clamp_min(0).double()
    return (u / u.sum(dim=1, keepdim=True)).float()


def _metric_inputs_host(x: torch.Tensor, size: Tuple[int, int], normalize: Optional[str], planes: int) -> torch.Tensor:
    """The host's one definition, on the selected fp32 frames ``[B, T', H, W]``: the two normalisation orders around
    ``Mh @ x @ Mw^T``."""
    if normalize == "source":
        x = misc.normalize_m1_1_batch(x[:, None])[:, 0]
    x = _resize_weights(x.shape[2], size[0]).to(x.device) @ x @ _resize_weights(x.shape[3], size[1]).to(x.device).t()
    if normalize == "resized":
        x = misc.normalize_m1_1_batch(x[:, None])[:, 0]
    return x[:, None].expand(-1, planes, -1, -1, -1)


def metric_inputs(images: torch.Tensor, channel: int, t: Optional[int] = None, size: Optional[Tuple[int, int]] = None,
                  normalize: Optional[str] = "source", planes: int = 3, dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """What a pretrained feature network receives: channel ``channel`` of ``images [B, C, T, H, W]``, time step ``t`` (``None``:
    the whole clip), resized to ``size`` (``None``: the source size), every sample mapped to [-1, 1] over all of its selected
    frames, replicated on ``planes`` (1 or 3) colour planes: ``[B, planes, T', size[0], size[1]]`` in ``dtype`` (``None``:
    float32; on the device float32 or bfloat16).

    ``normalize``: ``"source"`` -- ``misc.normalize_m1_1_batch`` on the source frames, then the resize, the order of the
    reference's FID and FVD (validation_metrics.py:589-590, 941-943: the networks resize what they are given);
    ``"resized"`` -- the resize first, the order of its IS (:44-52); ``None`` -- resize only.  A constant sample is NaN
    throughout, as in the reference, and so is a sample that holds a NaN.

    The resize is torch's ``interpolate(mode="bilinear", align_corners=False, antialias=True)``: a triangle filter as wide as
    the scale when shrinking, plain bilinear interpolation with border clamp when enlarging, a copy at equal size.  PARITY
    UNPINNED in one respect: the reference calls ``kornia.resize(..., antialias=True)``, whose anti-aliasing is a Gaussian
    blur in front of a plain bilinear resize.  As far as kornia's published source goes that blur is skipped when enlarging
    (this could not be run here); if so, 256 x 256 -> 299 x 299 is plain bilinear in both and only FVD's 224 x 224 and the
    512 x 512 configuration differ -- there by the shape of the low-pass filter.

    float32 / bfloat16 tensors on the GPU go through ``msg_metric_input`` on the current stream (one launch, two with a
    normalisation; a source side more than ``MSG_METRIC_MAX_SCALE`` = 8 times the output's is refused); CPU tensors and other dtypes take
    one torch statement of the same definition in float32 (there a NaN without a normalisation spreads over its row and column)."""
    if images.ndim != 5:
        raise ValueError(f"expected [B, C, T, H, W] images, got {tuple(images.shape)}")
    B, C, T, H, W = images.shape
    if not 0 <= int(channel) < C:
        raise ValueError(f"channel {channel} of {C}")
    if t is not None and not 0 <= int(t) < T:
        raise ValueError(f"time step {t} of {T}")
    if planes not in (1, 3):
        raise ValueError(f"planes is 1 or 3, not {planes}")
    if normalize not in _NORM_CODES:
        raise ValueError(f"normalize is 'source', 'resized' or None, not {normalize!r}")
    size = (H, W) if size is None else (int(size[0]), int(size[1]))
    if min(size) < 1 or min(H, W) < 1:
        raise ValueError(f"cannot resize {H} x {W} to {size[0]} x {size[1]}")
    dtype = torch.float32 if dtype is None else dtype
    images = images.detach()
    frames = 1 if t is not None else T
    if not (images.is_cuda and images.dtype in (torch.float32, torch.bfloat16)) or B == 0:
        x = images[:, channel, slice(None) if t is None else slice(int(t), int(t) + 1)].to(torch.float32)
        return _metric_inputs_host(x, size, normalize, planes).to(dtype).contiguous()
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"on the device the inputs are float32 or bfloat16, not {dtype}")
    images = images.contiguous()
    dev = _lib.require_gpu(images)
    out = torch.empty((B, planes, frames, size[0], size[1]), dtype=dtype, device=dev)
    lib, norm, t_arg = _lib.lib(), getattr(_lib, _NORM_CODES[normalize]), -1 if t is None else int(t)
    nbytes = lib.msg_metric_input_workspace(B, T, H, W, t_arg, size[0], size[1], norm)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes > 0 else None
    with _lib.on_device(dev):
        with _lib.kernel_clock.span(("metric_input", images.dtype, normalize),
                                    float(B * frames * H * W * images.element_size() + out.numel() * out.element_size())):
            _lib.check(lib.msg_metric_input(images.data_ptr(), _lib.dtype_code(images), B, C, T, H, W, int(channel), t_arg,
                                            out.data_ptr(), _lib.dtype_code(out), planes, size[0], size[1], norm, _lib.ptr(ws),
                                            _lib.stream_of(dev)), "msg_metric_input")
    return out


class FeatureMoments:
    """Running sample count, sum and sum of outer products of feature rows, float64 on the features' device.  ``limit``
    rows at most are taken (the reference truncates its activation lists to ``data_samples``)."""

    def __init__(self, limit: Optional[int] = None):
        self.limit, self.n = limit, 0
        self.s1: Optional[torch.Tensor] = None
        self.s2: Optional[torch.Tensor] = None

    @property
    def full(self) -> bool:
        return self.limit is not None and self.n >= self.limit

    def update(self, features: torch.Tensor) -> "FeatureMoments":
        f = features.detach().flatten(start_dim=1).double()
        if self.limit is not None:
            f = f[:max(0, self.limit - self.n)]
        if f.shape[0] == 0:
            return self
        if self.s1 is None:
            self.s1 = torch.zeros(f.shape[1], dtype=torch.float64, device=f.device)
            self.s2 = torch.zeros(f.shape[1], f.shape[1], dtype=torch.float64, device=f.device)
        self.s1 += f.sum(dim=0)
        self.s2.addmm_(f.t(), f)
        self.n += f.shape[0]
        return self

    def all_reduce_(self) -> "FeatureMoments":
        """Sum (n, s1, s2) over the ranks of the default process group: the moments are additive, so every rank ends with
        the statistics of all rows any rank folded in (one [d, d] float64 all-reduce)."""
        if _ranks() > 1:
            if self.s1 is None:
                raise ValueError("a rank without feature rows cannot join the exchange (its feature width is unknown)")
            n = torch.tensor([float(self.n)], dtype=torch.float64, device=self.s1.device)
            for t in (n, self.s1, self.s2):
                torch_dist.all_reduce(t)
            self.n = int(n.item())
        return self

    def mean_cov(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """Mean and the N - 1 normalised covariance (``np.cov(..., rowvar=False)``, validation_metrics.py:201-205)."""
        if self.n < 2:
            raise ValueError("a covariance needs at least two feature rows")
        mu = self.s1 / self.n
        cov = (self.s2 - self.n * torch.outer(mu, mu)) / (self.n - 1)
        return mu, cov


def _sqrt_product_trace(cov_a: torch.Tensor, cov_b: torch.Tensor) -> torch.Tensor:
    """tr(sqrtm(A B)) for symmetric positive semi-definite A, B."""
    cov_a, cov_b = 0.5 * (cov_a + cov_a.t()), 0.5 * (cov_b + cov_b.t())
    lam, q = torch.linalg.eigh(cov_a)
    root_a = (q * lam.clamp_min(0.0).sqrt()) @ q.t()
    inner = root_a @ cov_b @ root_a
    return torch.linalg.eigvalsh(0.5 * (inner + inner.t())).clamp_min(0.0).sqrt().sum()


def frechet_distance_from_moments(real: FeatureMoments, fake: FeatureMoments) -> float:
    (mu_r, cov_r), (mu_f, cov_f) = real.mean_cov(), fake.mean_cov()
    assert mu_r.shape == mu_f.shape and cov_r.shape == cov_f.shape
    diff = mu_r - mu_f
    value = diff @ diff + torch.trace(cov_r) + torch.trace(cov_f) - 2.0 * _sqrt_product_trace(cov_r, cov_f)
    return float(value)


def frechet_distance(real_activations: torch.Tensor, fake_activations: torch.Tensor) -> float:
    """FID._calc_fid / FVD._calc_fvd (validation_metrics.py:192-220, 401-429) on ``[samples, features]`` tensors, computed on
    the tensors' device."""
    return frechet_distance_from_moments(FeatureMoments().update(torch.as_tensor(real_activations)),
                                         FeatureMoments().update(torch.as_tensor(fake_activations)))


def inception_score(predictions: torch.Tensor) -> float:
    """validation_metrics.py:126-140: ``exp(mean_i KL(p_i || mean_j p_j))`` of softmax outputs ``[samples, classes]``."""
    p = torch.as_tensor(predictions).double()
    p_y = p.mean(dim=0, keepdim=True)
    kl = torch.sum(p * torch.log(p / p_y), dim=-1)
    return float(kl.mean().exp())


class _Metric:
    """Constructor of the three reference classes (validation_metrics.py:20-48, 162-189, 366-393) with the feature network
    as an argument.  ``data_parallel`` is accepted for signature compatibility and ignored: one process drives one GPU here
    (DESIGN.md section 6)."""

    def __init__(self, network: nn.Module, device: Union[str, torch.device] = "cuda", data_parallel: bool = False,
                 batch_size: int = 1, data_samples: int = 5000, no_rfp: bool = False, no_gfp: bool = False) -> None:
        if network is None:
            raise ValueError(f"{type(self).__name__} needs its feature network: the pretrained weights the reference loads "
                             "(torchvision Inception-v3 / I3D) are not part of this repository")
        self.network = network
        self.device, self.batch_size, self.data_samples = device, batch_size, data_samples
        self.no_rfp, self.no_gfp = no_rfp, no_gfp

    def _channels(self):
        return [0] + ([] if self.no_gfp else [1]) + ([] if self.no_rfp else [2])

    def _latents(self, generator):
        return misc.get_noise(batch_size=self.batch_size, latent_dimension=generator.latent_dimensions, p_mixed_noise=0.0,
                              device=self.device)

    def _result(self, scores):
        """The reference's return statements, in their order (validation_metrics.py:149-153, 352-358, 559-565): with a GFP
        channel the pair (bf, gfp) is returned whether or not RFP scores were computed."""
        if not self.no_gfp:
            return scores[0], scores[1]
        if not self.no_rfp:
            return tuple(scores)
        return scores[0]


class IS(_Metric):
    """Inception score of generated frames (validation_metrics.py:15-154).  ``network``: ``[B, 3, S, S]`` in [-1, 1] -> class
    logits (the reference: torchvision's Inception-v3).  Preprocessing as :44-52 -- channel ``c`` of one random time step,
    the bilinear, anti-aliased resize to ``input_size`` (299 x 299; ``None``: the frames' own size), then the sample-wise
    [-1, 1] normalisation: ``metric_inputs(..., normalize="resized")``, whose docstring says how its filter stands to
    kornia 0.4.1's (PARITY UNPINNED when shrinking)."""

    def __init__(self, *args, input_size: Optional[Tuple[int, int]] = (299, 299), **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.input_size = input_size

    def _preprocessing(self, images: torch.Tensor, channel: int) -> torch.Tensor:
        return metric_inputs(images, channel, t=_draw_time_step(images), size=self.input_size, normalize="resized")[:, :, 0]

    @torch.no_grad()
    def __call__(self, generator: nn.Module, **kwargs):
        net = self.network.to(self.device).eval()
        generator.to(self.device).eval()
        channels = self._channels()
        predictions = [[] for _ in channels]
        world = _ranks()
        share = math.ceil(self.data_samples / world)             # this rank's samples; the class probabilities are gathered
        for _ in range(math.ceil(share / self.batch_size)):
            fake_images = generator(input=self._latents(generator))
            for k, c in enumerate(channels):
                frames = self._preprocessing(fake_images, c)
                predictions[k].append(net(frames).float().softmax(dim=1))
        rows = []
        for p in predictions:
            p = torch.cat(p)[:share].contiguous()
            if world > 1:
                parts = [torch.empty_like(p) for _ in range(world)]
                torch_dist.all_gather(parts, p)
                p = torch.cat(parts)
            rows.append(p[:self.data_samples])
        return self._result([inception_score(p) for p in rows])


class _Frechet(_Metric):
    """``input_size``: what the frames are resized to AFTER the normalisation, as the reference's networks do in their forward
    (``metric_inputs(..., normalize="source")``); ``None`` hands the network the frames at their own size."""

    def __init__(self, *args, input_size: Optional[Tuple[int, int]] = None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.input_size = input_size
        self.moments_real = None                        # cached across calls like the reference's activations_real_*

    def _inputs(self, images: torch.Tensor, channel: int) -> torch.Tensor:
        raise NotImplementedError

    @torch.no_grad()
    def __call__(self, generator: nn.Module, dataset: Iterable):
        net = self.network.to(self.device).eval()
        channels = self._channels()
        share = math.ceil(self.data_samples / _ranks())          # rows this rank contributes (all of them in one process)
        if self.moments_real is None:
            moments = [FeatureMoments(share) for _ in channels]
            for real_images in dataset:
                real_images = real_images.to(self.device)
                for m, c in zip(moments, channels):
                    m.update(net(self._inputs(real_images, c)))
                if moments[0].full:
                    break
            moments = [m.all_reduce_() for m in moments]
            if moments[0].n < self.data_samples:
                # (the reference indexes its activation list up to data_samples and would use however many rows there are
                #  too, silently; the score is then NOT the nominal-sample-count metric)
                warnings.warn(f"{type(self).__name__}: the dataset held {moments[0].n} samples, fewer than data_samples = "
                              f"{self.data_samples}; the real statistics (cached from now on) are those of {moments[0].n} rows")
            self.moments_real = moments
        generator.to(self.device).eval()
        fake = [FeatureMoments(share) for _ in channels]
        for _ in range(math.ceil(share / self.batch_size)):
            fake_images = generator(input=self._latents(generator))
            for m, c in zip(fake, channels):
                m.update(net(self._inputs(fake_images, c)))
        fake = [m.all_reduce_() for m in fake]
        return self._result([frechet_distance_from_moments(r, f) for r, f in zip(self.moments_real, fake)])


class FID(_Frechet):
    """Frechet inception distance between dataset frames and generated frames (validation_metrics.py:157-358).
    ``network``: ``[B, 3, H, W]`` in [-1, 1] -> pooled features (the reference: Inception-v3 up to the last pooling, 2048).
    ``FID(net, input_size=(299, 299))`` feeds torchvision's Inception-v3 what the reference's wrapper feeds it (:589-590)."""

    def _inputs(self, images, channel):
        return metric_inputs(images, channel, t=_draw_time_step(images), size=self.input_size, normalize="source")[:, :, 0]


class FVD(_Frechet):
    """Frechet video distance between dataset sequences and generated sequences (validation_metrics.py:361-568).
    ``network``: ``[B, 3, T, H, W]`` in [-1, 1] -> features of any shape (flattened per sample, :466; the reference: I3D).
    ``FVD(net, input_size=(224, 224))`` is the reference's clip size (:941-943)."""

    def _inputs(self, images, channel):
        return metric_inputs(images, channel, t=None, size=self.input_size, normalize="source")


# ------------------------------------------------------------------------------------------------- sample-based metrics
# KID / KVD and manifold precision / recall / density / coverage ("Sample-based metrics").  They need the
# feature ROWS, not their moments; on the GPU every pair of rows is formed and reduced by csrc/feature_pairs.hip
# (msg_feature_knn, msg_feature_ball_hits, msg_poly_mmd) and no [N, M] array is written.  CPU tensors take the host statement
# of the same definitions in float64 (``_host_*`` below), as ``metric_inputs`` does.
class FeatureRows:
    """The sample-keeping sibling of ``FeatureMoments``: the feature rows themselves, fp32 on the features' device, ``limit``
    rows at most."""

    def __init__(self, limit: Optional[int] = None):
        self.limit, self.n = limit, 0
        self._parts: list = []

    @property
    def full(self) -> bool:
        return self.limit is not None and self.n >= self.limit

    def update(self, features: torch.Tensor) -> "FeatureRows":
        f = features.detach().flatten(start_dim=1).to(torch.float32)
        if self.limit is not None:
            f = f[:max(0, self.limit - self.n)]
        if f.shape[0] == 0:
            return self
        if self._parts and self._parts[0].shape[1] != f.shape[1]:
            raise ValueError(f"feature rows of width {f.shape[1]} after rows of width {self._parts[0].shape[1]}")
        self._parts.append(f.clone() if f.data_ptr() == features.data_ptr() else f)      # (never a view of the network's output)
        self.n += f.shape[0]
        return self

    @property
    def rows(self) -> torch.Tensor:
        """One contiguous fp32 ``[n, d]`` tensor.  A row that is not finite raises: the kernels' comparisons would drop it
        silently."""
        if not self._parts:
            raise ValueError("no feature rows were collected")
        if len(self._parts) > 1:
            self._parts = [torch.cat(self._parts)]
        rows = self._parts[0].contiguous()
        if not bool(torch.isfinite(rows).all()):
            bad = (~torch.isfinite(rows).all(dim=1)).nonzero().flatten()[:8].tolist()
            raise ValueError(f"feature rows {bad} hold values that are not finite")
        return rows

    def all_gather_(self) -> "FeatureRows":
        """Every rank ends with the rows of all ranks, in rank order (the exchange ``IS.__call__`` makes for its probabilities).
        The ranks' shares are equal by construction (``share = ceil(data_samples / ranks)`` rows each); unequal ones raise."""
        if _ranks() > 1:
            if not self._parts:
                raise ValueError("a rank without feature rows cannot join the exchange (its feature width is unknown)")
            mine = self.rows
            counts = [torch.zeros(1, dtype=torch.int64, device=mine.device) for _ in range(_ranks())]
            torch_dist.all_gather(counts, torch.tensor([mine.shape[0]], dtype=torch.int64, device=mine.device))
            if len({int(c) for c in counts}) != 1:
                raise ValueError(f"the ranks hold unequal shares of feature rows: {[int(c) for c in counts]}")
            parts = [torch.empty_like(mine) for _ in range(_ranks())]
            torch_dist.all_gather(parts, mine)
            self._parts, self.n = [torch.cat(parts)], sum(p.shape[0] for p in parts)
        return self


class ManifoldScores(NamedTuple):
    precision: float
    recall: float
    density: float
    coverage: float


def _feature_sets(*sets: torch.Tensor):
    """``[n, d]`` feature sets of one width on one device -> (on the GPU?, the sets: fp32 contiguous there, float64 on the host)."""
    sets = tuple(torch.as_tensor(s).detach() for s in sets)
    for s in sets:
        if s.ndim != 2 or s.shape[0] < 1 or s.shape[1] < 1:
            raise ValueError(f"expected [n, d] feature rows, got {tuple(s.shape)}")
        if s.shape[1] != sets[0].shape[1] or s.device != sets[0].device:
            raise ValueError("the feature sets differ in width or device")
    if sets[0].is_cuda:
        return True, tuple(s.to(torch.float32).contiguous() for s in sets)
    return False, tuple(s.to(torch.float64) for s in sets)


def _host_dist2(q: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """float64 ``[nq, nr]`` squared distances as sums of squared differences, a block of query rows at a time."""
    step = max(1, (1 << 24) // max(1, r.shape[0] * r.shape[1]))
    return torch.cat([(q[i:i + step, None, :] - r[None, :, :]).square().sum(dim=2) for i in range(0, q.shape[0], step)])


def _workspace(nbytes: int, device) -> torch.Tensor:
    if nbytes < 0:
        raise _lib.MsgHipError("the feature-pair kernels refuse these sizes")
    return torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)


def _knn(q: torch.Tensor, r: torch.Tensor, k: int, exclude_self: bool, gpu: bool) -> torch.Tensor:
    """The k-th smallest squared distance from every row of ``q`` to the rows of ``r`` (``exclude_self``: ``q is r``, row i
    skipped by index)."""
    if gpu:
        dev = _lib.require_gpu(q, r)
        (nq, d), nr, lib = q.shape, r.shape[0], _lib.lib()
        out = torch.empty(nq, dtype=torch.float32, device=dev)
        ws = _workspace(lib.msg_feature_knn_workspace(nq, nr, d, k, int(exclude_self)), dev)
        with _lib.on_device(dev):
            with _lib.kernel_clock.span(("feature_knn", k), 2.0 * nq * nr * d):
                _lib.check(lib.msg_feature_knn(q.data_ptr(), nq, r.data_ptr(), nr, d, k, int(exclude_self), out.data_ptr(),
                                               ws.data_ptr(), _lib.stream_of(dev)), "msg_feature_knn")
        return out
    dist = _host_dist2(q, r)
    if exclude_self:
        dist = dist.clone()
        dist.fill_diagonal_(math.inf)
    return dist.kthvalue(k, dim=1).values


def _ball_hits(q: torch.Tensor, r: torch.Tensor, radius2: torch.Tensor, gpu: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(min_j (dist2(q_i, r_j) - radius2[j]), #{j: dist2(q_i, r_j) <= radius2[j]}) for every row of ``q``."""
    if gpu:
        dev = _lib.require_gpu(q, r, radius2)
        (nq, d), nr, lib = q.shape, r.shape[0], _lib.lib()
        radius2 = radius2.to(torch.float32).contiguous()
        margin = torch.empty(nq, dtype=torch.float32, device=dev)
        count = torch.empty(nq, dtype=torch.int32, device=dev)
        ws = _workspace(lib.msg_feature_ball_hits_workspace(nq, nr, d), dev)
        with _lib.on_device(dev):
            with _lib.kernel_clock.span(("feature_ball_hits",), 2.0 * nq * nr * d):
                _lib.check(lib.msg_feature_ball_hits(q.data_ptr(), nq, r.data_ptr(), nr, d, radius2.data_ptr(), margin.data_ptr(),
                                                     count.data_ptr(), ws.data_ptr(), _lib.stream_of(dev)),
                           "msg_feature_ball_hits")
        return margin, count
    dist = _host_dist2(q, r)
    return (dist - radius2[None, :]).min(dim=1).values, (dist <= radius2[None, :]).sum(dim=1)


def _poly_sums(x: torch.Tensor, y: torch.Tensor, ix: Optional[torch.Tensor], iy: Optional[torch.Tensor], gamma: float,
               coef0: float, gpu: bool) -> torch.Tensor:
    """float64 ``[S, 3]`` on the host: per subset the sums of ``k(u, v) = (gamma u.v + coef0)^3`` over the ordered pairs of
    distinct positions of x's list, of y's list, and over all pairs of the two.  ``ix`` / ``iy``: int ``[S, m]`` row indices,
    ``None``: every row once (one subset)."""
    for idx, n in ((ix, x.shape[0]), (iy, y.shape[0])):
        if idx is not None and (idx.ndim != 2 or idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= n):
            raise ValueError("an index list is empty or points outside its feature set")
    S = 1 if ix is None and iy is None else (ix if ix is not None else iy).shape[0]
    if (ix is not None and ix.shape[0] != S) or (iy is not None and iy.shape[0] != S):
        raise ValueError("the two index lists differ in their number of subsets")
    if gpu:
        dev = _lib.require_gpu(x, y)
        lib, d = _lib.lib(), x.shape[1]
        ix = None if ix is None else ix.to(device=dev, dtype=torch.int32).contiguous()
        iy = None if iy is None else iy.to(device=dev, dtype=torch.int32).contiguous()
        mx = x.shape[0] if ix is None else ix.shape[1]
        my = y.shape[0] if iy is None else iy.shape[1]
        sums = torch.empty((S, 3), dtype=torch.float64, device=dev)
        ws = _workspace(lib.msg_poly_mmd_workspace(x.shape[0], y.shape[0], d, S, mx, my), dev)
        with _lib.on_device(dev):
            with _lib.kernel_clock.span(("poly_mmd", S), 2.0 * S * d * (0.5 * mx * mx + 0.5 * my * my + mx * my)):
                _lib.check(lib.msg_poly_mmd(x.data_ptr(), x.shape[0], y.data_ptr(), y.shape[0], d, _lib.ptr(ix), _lib.ptr(iy), S, mx,
                                            my, float(gamma), float(coef0), sums.data_ptr(), ws.data_ptr(), _lib.stream_of(dev)),
                           "msg_poly_mmd")
        return sums.cpu()
    out = torch.empty((S, 3), dtype=torch.float64)
    for s in range(S):
        xs = x if ix is None else x[ix[s].long()]
        ys = y if iy is None else y[iy[s].long()]
        kxx, kyy, kxy = ((gamma * (a @ b.t()) + coef0) ** 3 for a, b in ((xs, xs), (ys, ys), (xs, ys)))
        out[s, 0], out[s, 1], out[s, 2] = kxx.sum() - kxx.diagonal().sum(), kyy.sum() - kyy.diagonal().sum(), kxy.sum()
    return out


def subset_indices(n: int, m: int, subsets: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int32 ``[subsets, m]``: per subset ``m`` of ``n`` row indices drawn without replacement (the head of one
    ``torch.randperm`` per subset, from ``generator`` or the global CPU generator)."""
    if not 1 <= m <= n or subsets < 1:
        raise ValueError(f"cannot draw {subsets} subsets of {m} rows out of {n}")
    return torch.stack([torch.randperm(n, generator=generator)[:m] for _ in range(subsets)]).to(torch.int32)


def _mmd2(sums: torch.Tensor, mx: int, my: int) -> float:
    """The unbiased MMD^2 per subset from its three sums, float64 on the host, and the mean over the subsets."""
    sums = sums.double()
    per = sums[:, 0] / (mx * (mx - 1)) + sums[:, 1] / (my * (my - 1)) - 2.0 * sums[:, 2] / (mx * my)
    return float(per.mean())


def kernel_distance(real: torch.Tensor, fake: torch.Tensor, subsets: Optional[int] = None, subset_size: int = 1000,
                    generator: Optional[torch.Generator] = None) -> float:
    """Kernel inception distance of two feature sets ``[N, d]``, ``[M, d]``: the unbiased estimate of the squared maximum
    mean discrepancy under the kernel ``k(u, v) = (u.v / d + 1)^3``.

    ``subsets=None``: the full U-statistic over all rows, ``sum_{a != b} k(x_a, x_b) / (N (N - 1)) + sum_{a != b} k(y_a, y_b) /
    (M (M - 1)) - 2 sum_{a, b} k(x_a, y_b) / (N M)`` -- the right form for a few hundred samples.  ``subsets=S``: the
    StyleGAN2-ADA estimator, the mean of that statistic over ``S`` pairs of subsets of ``m = min(N, M, subset_size)`` rows drawn
    without replacement (``subset_indices``, from ``generator``; the real set's lists are drawn first).

    On the GPU the three sums of every subset come from one ``msg_poly_mmd`` call: fp32 products, every kernel value widened to
    float64 before it is added, rows gathered by index while staging; the final combination is float64 on the host.  CPU tensors:
    the same sums from float64 matrix products."""
    gpu, (x, y) = _feature_sets(real, fake)
    n, m_, d = x.shape[0], y.shape[0], x.shape[1]
    if min(n, m_) < 2:
        raise ValueError("the unbiased estimate needs at least two rows in each set")
    if subsets is None:
        return _mmd2(_poly_sums(x, y, None, None, 1.0 / d, 1.0, gpu), n, m_)
    m = min(n, m_, int(subset_size))
    if m < 2:
        raise ValueError("subset_size is at least 2")
    ix = subset_indices(n, m, int(subsets), generator)
    iy = subset_indices(m_, m, int(subsets), generator)
    return _mmd2(_poly_sums(x, y, ix, iy, 1.0 / d, 1.0, gpu), m, m)


def manifold_scores(real: torch.Tensor, fake: torch.Tensor, k: int = 3) -> ManifoldScores:
    """k-NN manifold precision and recall (Kynkaanniemi et al. 2019) and their outlier-robust forms density and coverage
    (Naeem et al. 2020) of feature sets ``real [N, d]``, ``fake [M, d]``.  Every row carries a ball whose squared radius is its
    squared distance to its k-th nearest neighbour within its OWN set (itself excluded by index: a duplicate row is a neighbour
    at distance 0).

    precision: the share of fake rows inside at least one real ball; recall: the share of real rows inside at least one fake
    ball; density: the number of real balls a fake row lies in, summed over the fake rows, over ``k M``; coverage: the share of
    real rows whose nearest fake row lies within the real row's own ball.  "Inside" is ``dist2 <= radius2``.

    Distances do not change under a translation, but the fp32 error of ``|a|^2 + |b|^2 - 2 a.b`` grows with the norms: the mean of
    the real rows is subtracted from BOTH sets first (one torch op each), then the kernels run -- ``msg_feature_knn`` for the radii
    and the nearest fake row, ``msg_feature_ball_hits`` for margins and counts.  CPU tensors take the same definitions in float64
    with distances as sums of squared differences."""
    gpu, (x, y) = _feature_sets(real, fake)
    k = int(k)
    if not 1 <= k <= min(x.shape[0], y.shape[0]) - 1:
        raise ValueError(f"k = {k} needs 1 <= k <= rows - 1 in both sets ({x.shape[0]}, {y.shape[0]} rows)")
    if gpu and k > _lib.MSG_FEATURE_KNN_MAX:
        raise ValueError(f"on the device k is at most {_lib.MSG_FEATURE_KNN_MAX}")
    centre = x.mean(dim=0, keepdim=True)
    x, y = x - centre, y - centre
    radius_x, radius_y = _knn(x, x, k, True, gpu), _knn(y, y, k, True, gpu)
    margin_y, count_y = _ball_hits(y, x, radius_x, gpu)
    margin_x, _ = _ball_hits(x, y, radius_y, gpu)
    nearest = _knn(x, y, 1, False, gpu)
    stats = torch.stack([(margin_y <= 0).double().mean(), (margin_x <= 0).double().mean(),
                         count_y.double().sum() / (k * y.shape[0]), (nearest <= radius_x).double().mean()]).tolist()
    return ManifoldScores(*stats)


class _Samples(_Metric):
    """The sweep of ``_Frechet.__call__`` with the rows kept: the real rows are swept once and cached, every rank contributes
    ``share = ceil(data_samples / ranks)`` rows of each kind and the rows are gathered in rank order, so every rank scores the
    union.  ``input_size`` as for ``FID`` / ``FVD``."""

    def __init__(self, *args, input_size: Optional[Tuple[int, int]] = None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.input_size = input_size
        self.rows_real = None

    def _inputs(self, images: torch.Tensor, channel: int) -> torch.Tensor:
        raise NotImplementedError

    def _score(self, real: torch.Tensor, fake: torch.Tensor):
        raise NotImplementedError

    @torch.no_grad()
    def __call__(self, generator: nn.Module, dataset: Iterable):
        net = self.network.to(self.device).eval()
        channels = self._channels()
        share = math.ceil(self.data_samples / _ranks())
        if self.rows_real is None:
            real = [FeatureRows(share) for _ in channels]
            for real_images in dataset:
                real_images = real_images.to(self.device)
                for m, c in zip(real, channels):
                    m.update(net(self._inputs(real_images, c)))
                if real[0].full:
                    break
            real = [m.all_gather_() for m in real]
            if real[0].n < self.data_samples:
                warnings.warn(f"{type(self).__name__}: the dataset held {real[0].n} samples, fewer than data_samples = "
                              f"{self.data_samples}; the real rows (cached from now on) are those {real[0].n}")
            self.rows_real = [m.rows[:self.data_samples] for m in real]
        generator.to(self.device).eval()
        fake = [FeatureRows(share) for _ in channels]
        for _ in range(math.ceil(share / self.batch_size)):
            fake_images = generator(input=self._latents(generator))
            for m, c in zip(fake, channels):
                m.update(net(self._inputs(fake_images, c)))
        fake = [m.all_gather_().rows[:self.data_samples] for m in fake]
        return self._result([self._score(r, f) for r, f in zip(self.rows_real, fake)])


class _KernelDistance(_Samples):
    """``subsets`` / ``subset_size`` / ``generator`` as in ``kernel_distance``: the full U-statistic by default.  In a
    multi-rank pass give every rank a ``generator`` with the same seed, or the ranks draw different subsets."""

    def __init__(self, *args, subsets: Optional[int] = None, subset_size: int = 1000,
                 generator: Optional[torch.Generator] = None, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.subsets, self.subset_size, self.generator = subsets, subset_size, generator

    def _score(self, real, fake):
        return kernel_distance(real, fake, self.subsets, self.subset_size, self.generator)


class _Manifold(_Samples):
    """``k``: the neighbour that sets a row's radius (3 in the precision / recall paper, 5 in density / coverage)."""

    def __init__(self, *args, k: int = 3, **kwargs) -> None:
        super().__init__(*args, **kwargs)
        self.k = k

    def _score(self, real, fake):
        return manifold_scores(real, fake, self.k)


class KID(_KernelDistance):
    """Kernel inception distance between dataset frames and generated frames: ``FID``'s inputs and network, scored by
    ``kernel_distance``.  A float per channel."""
    _inputs = FID._inputs


class KVD(_KernelDistance):
    """Kernel video distance: ``FVD``'s inputs and network, scored by ``kernel_distance``.  A float per channel."""
    _inputs = FVD._inputs


class PrecisionRecall(_Manifold):
    """``manifold_scores`` of dataset frames against generated frames (``FID``'s inputs): a ``ManifoldScores`` per channel."""
    _inputs = FID._inputs


class PrecisionRecallVideo(_Manifold):
    """``manifold_scores`` of dataset sequences against generated sequences (``FVD``'s inputs): a ``ManifoldScores`` per
    channel."""
    _inputs = FVD._inputs


# ------------------------------------------------------------------------------------------- sliced Wasserstein distance
# SWD / SWVD ("Sliced Wasserstein distance"; Karras et al. 2018, section 5): the one metric here that
# needs no feature network.  Per level of a Laplacian pyramid, 7 x 7 patches of both sets are normalised per plane, projected
# on random unit directions, sorted, and compared by the mean absolute difference.  On the GPU the level, the gather, the
# statistics, the projection (normalisation folded in) and the final reduction are csrc/swd.hip; the sort is torch.sort.
# CPU tensors take the float64 statement of the same definition.
_SWD_PATCH = 7
_SWD_TAPS = _SWD_PATCH * _SWD_PATCH


def _pyramid_sizes(h: int, w: int, min_size: int):
    if min_size < 1:
        raise ValueError(f"min_size is at least 1, not {min_size}")
    levels = 1
    while min(h, w) >> levels >= min_size:
        levels += 1
    if h % (1 << (levels - 1)) or w % (1 << (levels - 1)):
        raise ValueError(f"{h} x {w} frames are not divisible by 2^{levels - 1} (a pyramid of {levels} levels down to a "
                         f"shorter side >= {min_size})")
    return [(h >> l, w >> l) for l in range(levels)]


def _host_filter(x: torch.Tensor, gain: float) -> torch.Tensor:
    """``x [N, 1, h, w]`` float64 convolved with ``gain * f f^T``, ``f = [1, 4, 6, 4, 1] / 16``, boundary rule "mirror" (torch's
    ``reflect`` padding: the edge sample is not repeated)."""
    f = torch.tensor([1.0, 4.0, 6.0, 4.0, 1.0], dtype=torch.float64) / 16.0
    kernel = (gain * torch.outer(f, f))[None, None]
    return torch.nn.functional.conv2d(torch.nn.functional.pad(x, (2, 2, 2, 2), mode="reflect"), kernel)


def laplacian_pyramid(frames: torch.Tensor, min_size: int = 16) -> list:
    """The Laplacian pyramid of ``frames [..., H, W]``, finest level first: ``G_0`` the frames, ``G_(l+1) = down(G_l)`` (the
    binomial ``F = f f^T``, ``f = [1, 4, 6, 4, 1] / 16``, boundary rule "mirror", then every second row and column), level ``l`` is
    ``G_l - up(G_(l+1))`` (``up``: the samples on the even positions of a zero array of twice the size, convolved with ``4 F``), the
    coarsest level is ``G_L`` itself.  Levels run down to the last one whose shorter side is >= ``min_size``; ``H`` and ``W`` must
    be divisible by ``2^(levels - 1)``.

    fp32 tensors on the GPU: one ``msg_laplacian_level`` launch per level, fp32 out (sides below 8 are refused there).  CPU
    tensors: the float64 statement, float64 out."""
    if frames.ndim < 2:
        raise ValueError(f"expected [..., H, W] frames, got {tuple(frames.shape)}")
    lead, (h, w) = frames.shape[:-2], frames.shape[-2:]
    sizes = _pyramid_sizes(h, w, int(min_size))
    frames = frames.detach()
    if frames.is_cuda:
        dev = _lib.require_gpu(frames)
        g = frames.to(torch.float32).contiguous().view(-1, h, w)
        lib, levels = _lib.lib(), []
        with _lib.on_device(dev):
            for (fh, fw), (ch, cw) in zip(sizes[:-1], sizes[1:]):
                coarse = torch.empty((g.shape[0], ch, cw), dtype=torch.float32, device=dev)
                lap = torch.empty_like(g)
                with _lib.kernel_clock.span(("laplacian_level", fh, fw), 4.0 * (2.25 * g.numel())):
                    _lib.check(lib.msg_laplacian_level(g.data_ptr(), g.shape[0], fh, fw, coarse.data_ptr(), lap.data_ptr(),
                                                       _lib.stream_of(dev)), "msg_laplacian_level")
                levels.append(lap.view(*lead, fh, fw))
                g = coarse
        levels.append(g.view(*lead, *sizes[-1]) if len(sizes) > 1 else g.view(*lead, h, w).clone())
        return levels
    g = frames.to(torch.float64).reshape(-1, 1, h, w)
    levels = []
    for fh, fw in sizes[:-1]:
        coarse = _host_filter(g, 1.0)[..., ::2, ::2]
        stuffed = torch.zeros_like(g)
        stuffed[..., ::2, ::2] = coarse
        levels.append((g - _host_filter(stuffed, 4.0)).reshape(*lead, fh, fw))
        g = coarse
    levels.append(g.reshape(*lead, *sizes[-1]).clone())
    return levels


def swd_positions(samples: int, h: int, w: int, descriptors_per_image: int = 128,
                  generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """int32 ``[samples, descriptors_per_image, 2]`` on the host: patch centres ``(y, x)`` drawn uniformly from ``[3, h - 4] x
    [3, w - 4]`` (all ``y`` of the call first, then all ``x``; from ``generator`` or the global CPU generator), so that every 7 x 7
    patch lies inside its plane."""
    if samples < 1 or descriptors_per_image < 1 or min(h, w) < _SWD_PATCH:
        raise ValueError(f"cannot draw {descriptors_per_image} patches of 7 x 7 per sample from {samples} planes of {h} x {w}")
    y = torch.randint(3, h - 3, (samples, descriptors_per_image), generator=generator)
    x = torch.randint(3, w - 3, (samples, descriptors_per_image), generator=generator)
    return torch.stack([y, x], dim=2).to(torch.int32)


def swd_descriptors(level: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """The patches of ``level [B, P, h, w]`` centred at ``pos [B, K, 2]`` as rows ``[B K, P 49]``: plane-major, then patch row,
    then patch column.  A tap outside the plane reads as zero.  fp32 on the GPU (``msg_swd_gather``, a copy), the level's own
    dtype on the host."""
    if level.ndim != 4 or pos.ndim != 3 or pos.shape[0] != level.shape[0] or pos.shape[2] != 2:
        raise ValueError(f"expected a [B, P, h, w] level and [B, K, 2] positions, got {tuple(level.shape)}, {tuple(pos.shape)}")
    B, P, h, w = level.shape
    K = pos.shape[1]
    level = level.detach()
    if level.is_cuda:
        dev = _lib.require_gpu(level)
        level = level.to(torch.float32).contiguous()
        pos = pos.to(device=dev, dtype=torch.int32).contiguous()
        rows = torch.empty((B * K, P * _SWD_TAPS), dtype=torch.float32, device=dev)
        with _lib.on_device(dev):
            with _lib.kernel_clock.span(("swd_gather", P), 8.0 * rows.numel()):
                _lib.check(_lib.lib().msg_swd_gather(level.data_ptr(), B, P, h, w, pos.data_ptr(), K, rows.data_ptr(),
                                                     _lib.stream_of(dev)), "msg_swd_gather")
        return rows
    pos = pos.long()
    off = torch.arange(-3, 4)
    y = pos[:, :, 0, None, None] + off[None, None, :, None]                    # [B, K, 7, 1]
    x = pos[:, :, 1, None, None] + off[None, None, None, :]                    # [B, K, 1, 7]
    inside = ((y >= 0) & (y < h) & (x >= 0) & (x < w))[:, :, None]             # [B, K, 1, 7, 7]
    b = torch.arange(B)[:, None, None, None, None]
    p = torch.arange(P)[None, None, :, None, None]
    taps = level[b, p, y.clamp(0, h - 1)[:, :, None], x.clamp(0, w - 1)[:, :, None]]
    return (taps * inside.to(taps.dtype)).reshape(B * K, P * _SWD_TAPS)


def swd_directions(d: int, repeats: int = 4, directions: int = 128, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """fp32 ``[repeats, d, directions]`` on the host: per repeat one ``torch.randn([d, directions])`` draw (from ``generator`` or
    the global CPU generator), every column scaled to unit length in float64 and rounded once to fp32."""
    if d < 1 or repeats < 1 or directions < 1:
        raise ValueError(f"cannot draw {repeats} x {directions} directions of width {d}")
    out = []
    for _ in range(repeats):
        draw = torch.randn([d, directions], generator=generator).double()
        out.append((draw / draw.square().sum(dim=0, keepdim=True).sqrt()).float())
    return torch.stack(out)


def _plane_statistics(rows: torch.Tensor, planes: int, gpu: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """fp32 ``mean [P]`` and ``istd [P]`` = 1 / population standard deviation over all ``n 49`` values of each plane, on the
    host; both from float64 and rounded once.  A constant plane has ``istd = inf``."""
    n = rows.shape[0]
    count = float(n * _SWD_TAPS)
    if gpu:
        dev = _lib.require_gpu(rows)
        lib = _lib.lib()
        sums = torch.empty((planes, 2), dtype=torch.float64, device=dev)
        ws = _workspace(lib.msg_swd_plane_sums_workspace(n, planes), dev)
        with _lib.on_device(dev):
            with _lib.kernel_clock.span(("swd_plane_sums", planes), 4.0 * rows.numel()):
                _lib.check(lib.msg_swd_plane_sums(rows.data_ptr(), n, planes, sums.data_ptr(), ws.data_ptr(), _lib.stream_of(dev)),
                           "msg_swd_plane_sums")
        sums = sums.cpu()
        mean, square = sums[:, 0] / count, sums[:, 1] / count
        var = square - mean * mean
        # sum x^2 / N - mean^2 cancels when the spread is far below the mean; below 2^-36 of the mean square it is in the
        # rounding noise of the float64 sums, and the plane is measured directly
        doubtful = (var <= square * 2.0 ** -36).nonzero().flatten().tolist()
    else:
        x = rows.reshape(n, planes, _SWD_TAPS).transpose(0, 1).reshape(planes, -1)
        mean = x.mean(dim=1)
        var = (x - mean[:, None]).square().mean(dim=1)
        doubtful = list(range(planes))
    for p in doubtful:
        x = rows.reshape(n, planes, _SWD_TAPS)[:, p]
        lo, hi = float(x.min()), float(x.max())
        if lo == hi:                                    # a constant plane, decided exactly: std = 0
            mean[p], var[p] = lo, 0.0
        elif gpu:
            x = x.double()
            mean[p] = float(x.sum()) / count
            var[p] = float((x - mean[p]).square().sum()) / count
    return mean.float(), (1.0 / var.sqrt()).float()


def _project_sorted(rows: torch.Tensor, planes: int, mean: torch.Tensor, istd: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """Device: ``[R, n]`` fp32, the normalised rows projected on ``dirs [d, R]`` (``msg_swd_project``), every direction sorted
    ascending."""
    dev, lib = rows.device, _lib.lib()
    n, R = rows.shape[0], dirs.shape[1]
    out = torch.empty((R, n), dtype=torch.float32, device=dev)
    with _lib.on_device(dev):
        with _lib.kernel_clock.span(("swd_project", planes, R), 2.0 * n * R * rows.shape[1]):
            _lib.check(lib.msg_swd_project(rows.data_ptr(), n, planes, mean.data_ptr(), istd.data_ptr(), dirs.data_ptr(), R,
                                           out.data_ptr(), _lib.stream_of(dev)), "msg_swd_project")
    return torch.sort(out, dim=1).values


def sliced_wasserstein(real_rows: torch.Tensor, fake_rows: torch.Tensor, planes: int, repeats: int = 4, directions: int = 128,
                       generator: Optional[torch.Generator] = None, normalize: bool = True) -> float:
    """The sliced Wasserstein distance of two descriptor sets ``[n, planes * 49]`` of EQUAL ``n``, times 1000.

    Each set is normalised per plane (its mean and population standard deviation over all ``n 49`` values of the plane, from
    float64 sums, rounded once to fp32 ``mean`` and ``istd = 1 / std``; ``normalize=False``: mean 0, istd 1).  ``repeats`` x
    ``directions`` unit directions come from ``swd_directions(planes * 49, repeats, directions, generator)``; for every direction
    both sets' normalised rows are projected, each projection is sorted ascending, and the result is ``1000 mean |a_(i) -
    b_(i)|`` over rows and directions.  A constant plane in either set gives NaN.

    On the GPU, one repeat at a time: ``msg_swd_plane_sums`` -> ``msg_swd_project`` (the normalisation happens while the rows
    are staged; no normalised copy and no ``[n, R]`` product are written) -> ``torch.sort(dim=1)`` on the direction-major
    ``[directions, n]`` array -> ``msg_sorted_l1`` (float64 sums); two sorted ``[directions, n]`` arrays are live at its end.  CPU
    tensors take the float64 statement with the same fp32-rounded ``mean``, ``istd`` and directions."""
    gpu, (x, y) = _feature_sets(real_rows, fake_rows)
    planes = int(planes)
    if planes < 1 or x.shape[1] != planes * _SWD_TAPS:
        raise ValueError(f"rows of width {x.shape[1]} are not {planes} planes of 7 x 7")
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"the two sets hold {x.shape[0]} and {y.shape[0]} rows: the sorted projections are compared row by row")
    n, d = x.shape
    stats = []
    for s in (x, y):
        if normalize:
            stats.append(_plane_statistics(s, planes, gpu))
        else:
            stats.append((torch.zeros(planes), torch.ones(planes)))
    dirs = swd_directions(d, int(repeats), int(directions), generator)
    if not all(bool(torch.isfinite(istd).all()) for _, istd in stats):
        return math.nan
    if gpu:
        dev = _lib.require_gpu(x, y)
        lib = _lib.lib()
        stats = [(m.to(dev), i.to(dev)) for m, i in stats]
        R = dirs.shape[2]
        sums = torch.empty(R, dtype=torch.float64, device=dev)
        ws = _workspace(lib.msg_sorted_l1_workspace(R, n), dev)
        total = torch.zeros((), dtype=torch.float64, device=dev)
        for rep in range(dirs.shape[0]):
            dr = dirs[rep].to(dev).contiguous()
            a = _project_sorted(x, planes, stats[0][0], stats[0][1], dr)
            b = _project_sorted(y, planes, stats[1][0], stats[1][1], dr)
            with _lib.on_device(dev):
                with _lib.kernel_clock.span(("sorted_l1", R), 8.0 * R * n):
                    _lib.check(lib.msg_sorted_l1(a.data_ptr(), b.data_ptr(), R, n, sums.data_ptr(), ws.data_ptr(),
                                                 _lib.stream_of(dev)), "msg_sorted_l1")
            total += sums.sum()
            del a, b
        return 1000.0 * float(total) / (float(n) * dirs.shape[0] * dirs.shape[2])
    total = 0.0
    for rep in range(dirs.shape[0]):
        proj = []
        for s, (mean, istd) in zip((x, y), stats):
            hat = (s.reshape(n, planes, _SWD_TAPS) - mean.double()[None, :, None]) * istd.double()[None, :, None]
            proj.append((hat.reshape(n, d) @ dirs[rep].double()).sort(dim=0).values)
        total += float((proj[0] - proj[1]).abs().sum())
    return 1000.0 * total / (float(n) * dirs.shape[0] * dirs.shape[2])


@functools.lru_cache(maxsize=None)
def _swd_score_type(sides: Tuple[int, ...]):
    return collections.namedtuple("SlicedWassersteinScores", ("mean",) + tuple(f"r{s}" for s in sides))


class _SlicedWasserstein(_Metric):
    """The sweep of ``_Samples.__call__`` on pixels: no feature network.  Per channel and pyramid level the real descriptor rows
    are kept in ``FeatureRows`` and cached across calls; every rank contributes ``share = ceil(data_samples / ranks)`` samples of
    each kind and the rows are gathered in rank order; the generator sweep draws exactly as many sequences as the real sweep
    kept.  Patch positions and directions come from ``generator`` (``None``: the global CPU generator).  In a multi-rank pass
    give every rank a ``generator`` with the same seed, or the ranks draw different directions.

    The score per channel is a named tuple ``(mean, r<side>, ...)``: one field per level named by the level's height, finest
    first (256 x 256 frames: ``mean, r256, r128, r64, r32, r16``), ``mean`` their average.  A level one of whose planes is
    constant over a whole set scores NaN, with one warning per channel and level."""

    def __init__(self, device: Union[str, torch.device] = "cuda", data_parallel: bool = False, batch_size: int = 1,
                 data_samples: int = 5000, no_rfp: bool = False, no_gfp: bool = False, descriptors_per_image: int = 128,
                 repeats: int = 4, directions: int = 128, min_size: int = 16,
                 generator: Optional[torch.Generator] = None) -> None:
        self.network = None
        self.device, self.batch_size, self.data_samples = device, batch_size, data_samples
        self.no_rfp, self.no_gfp = no_rfp, no_gfp
        self.descriptors_per_image, self.repeats, self.directions = int(descriptors_per_image), int(repeats), int(directions)
        self.min_size, self.generator = int(min_size), generator
        self.rows_real = None                           # [channel][level] -> [n, P 49], cached across calls
        self._warned: set = set()

    def _inputs(self, images: torch.Tensor, channel: int) -> torch.Tensor:
        raise NotImplementedError

    def _fold(self, images: torch.Tensor, channel: int, into: Optional[list], limit: int) -> list:
        """One batch's descriptor rows of every level, appended to ``into`` (a ``FeatureRows`` per level)."""
        planes = self._inputs(images, channel)[:, 0]                           # [B, T', H, W]: the frames are the planes
        levels = laplacian_pyramid(planes, self.min_size)
        self._sides = [level.shape[2] for level in levels]
        if into is None:
            into = [FeatureRows(limit * self.descriptors_per_image) for _ in levels]
        for level, rows in zip(levels, into):
            pos = swd_positions(level.shape[0], level.shape[2], level.shape[3], self.descriptors_per_image, self.generator)
            rows.update(swd_descriptors(level, pos))
        return into

    @torch.no_grad()
    def __call__(self, generator: nn.Module, dataset: Iterable):
        channels, K = self._channels(), self.descriptors_per_image
        share = math.ceil(self.data_samples / _ranks())
        if self.rows_real is None:
            real = [None for _ in channels]
            for real_images in dataset:
                real_images = real_images.to(self.device)
                for k, c in enumerate(channels):
                    real[k] = self._fold(real_images, c, real[k], share)
                if real[0][0].full:
                    break
            if real[0] is None:
                raise ValueError("the dataset is empty")
            real = [[m.all_gather_() for m in levels] for levels in real]
            if real[0][0].n < self.data_samples * K:
                warnings.warn(f"{type(self).__name__}: the dataset held {real[0][0].n // K} samples, fewer than data_samples = "
                              f"{self.data_samples}; the real rows (cached from now on) are those {real[0][0].n // K}")
            self.rows_real = [[m.rows[:self.data_samples * K] for m in levels] for levels in real]
        kept = self.rows_real[0][0].shape[0] // K
        share = math.ceil(kept / _ranks())
        generator.to(self.device).eval()
        fake = [None for _ in channels]
        for _ in range(math.ceil(share / self.batch_size)):
            fake_images = generator(input=self._latents(generator))
            for k, c in enumerate(channels):
                fake[k] = self._fold(fake_images, c, fake[k], share)
        scores = []
        for c, real_levels, fake_levels in zip(channels, self.rows_real, fake):
            per_level = []
            for side, real_rows, rows in zip(self._sides, real_levels, fake_levels):
                fake_rows = rows.all_gather_().rows[:kept * K]
                value = sliced_wasserstein(real_rows, fake_rows, real_rows.shape[1] // _SWD_TAPS, self.repeats, self.directions,
                                           self.generator)
                if math.isnan(value) and (c, side) not in self._warned:
                    self._warned.add((c, side))
                    warnings.warn(f"{type(self).__name__}: channel {c}, level r{side}: a plane is constant over a whole set, "
                                  "its standard deviation is 0 and the level's score is NaN")
                per_level.append(value)
            scores.append(_swd_score_type(tuple(self._sides))(sum(per_level) / len(per_level), *per_level))
        return self._result(scores)


class SWD(_SlicedWasserstein):
    """Sliced Wasserstein distance between dataset frames and generated frames: channel ``c`` of one drawn time step (as ``FID``
    draws it) at its own size and intensity scale, ``metric_inputs(..., size=None, normalize=None, planes=1)``."""

    def _inputs(self, images, channel):
        return metric_inputs(images, channel, t=_draw_time_step(images), size=None, normalize=None, planes=1)


class SWVD(_SlicedWasserstein):
    """Sliced Wasserstein video distance: the whole clip of channel ``c`` (as ``FVD`` takes it); the ``T`` frames are the
    planes of a patch, so a descriptor spans time."""

    def _inputs(self, images, channel):
        return metric_inputs(images, channel, t=None, size=None, normalize=None, planes=1)


# ------------------------------------------------------------------------------------------------------ MS-SSIM diversity
# MSSSIM / MSSSIMVideo ("MS-SSIM"; Odena et al. 2017, section 4.3): the mean pairwise multi-scale structural
# similarity INSIDE a set, for the generated samples beside the dataset's.  Generated far above real: the generator repeats
# itself.  No feature network; on the GPU every pair is two planes through csrc/ssim.hip (ssim.py: ms_ssim).
class DiversityScore(NamedTuple):
    fake: float
    real: float
    gap: float


class _MsSsimDiversity(_Metric):
    """Per channel the samples of both kinds are kept on ``device`` as ``[n, P, H, W]`` fp32 planes at their own size (1000
    frames of 256 x 256: 262 MB per channel and set; ``MSSSIMVideo`` times ``T``); every rank contributes ``share =
    ceil(data_samples / ranks)`` samples of each kind.  A permutation drawn from ``seed`` forms the disjoint pairs ``(pi(2 i),
    pi(2 i + 1))`` of a rank's samples, at most ``pairs`` of them; the score of a set is the mean ``ms_ssim`` over the pairs of
    all ranks (the sum and the count are all-reduced).  The dataset's score is cached across calls.  Frames are expected in
    ``[0, data_range]``.  The score per channel is ``DiversityScore(fake, real, gap = fake - real)``."""

    def __init__(self, device: Union[str, torch.device] = "cuda", data_parallel: bool = False, batch_size: int = 1,
                 data_samples: int = 1000, no_rfp: bool = False, no_gfp: bool = False, pairs: Optional[int] = None,
                 seed: int = 0, data_range: float = 1.0) -> None:
        self.network = None
        self.device, self.batch_size, self.data_samples = device, batch_size, data_samples
        self.no_rfp, self.no_gfp = no_rfp, no_gfp
        self.pairs, self.seed, self.data_range = pairs, int(seed), float(data_range)
        self.real = None                                # (scores per channel, samples kept), cached across calls

    def _inputs(self, images: torch.Tensor, channel: int) -> torch.Tensor:
        raise NotImplementedError

    def _planes(self, images: torch.Tensor, channel: int) -> torch.Tensor:
        return self._inputs(images, channel)[:, 0].float()                     # [B, T', H, W]: the frames are the planes

    def _pair_mean(self, planes: torch.Tensor) -> float:
        n = planes.shape[0]
        k = n // 2 if self.pairs is None else min(n // 2, int(self.pairs))
        perm = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed)).to(planes.device)
        total = torch.zeros((), dtype=torch.float64, device=planes.device)
        chunk = max(int(self.batch_size), 64)
        for i in range(0, k, chunk):
            j = min(i + chunk, k)
            total += ms_ssim(planes[perm[2 * i:2 * j:2]], planes[perm[2 * i + 1:2 * j:2]], data_range=self.data_range).double().sum()
        stats = torch.stack([total, torch.tensor(float(k), dtype=torch.float64, device=planes.device)])
        if _ranks() > 1:
            torch_dist.all_reduce(stats)
        if float(stats[1]) < 1:
            raise ValueError(f"{type(self).__name__}: {n} samples form no pair")
        return float(stats[0] / stats[1])

    @torch.no_grad()
    def __call__(self, generator: nn.Module, dataset: Iterable):
        channels = self._channels()
        share = math.ceil(self.data_samples / _ranks())
        if self.real is None:
            real = [[] for _ in channels]
            held = 0
            for real_images in dataset:
                real_images = real_images.to(self.device)
                for k, c in enumerate(channels):
                    real[k].append(self._planes(real_images, c))
                held += real_images.shape[0]
                if held >= share:
                    break
            if held == 0:
                raise ValueError("the dataset is empty")
            if held < share:
                warnings.warn(f"{type(self).__name__}: the dataset held {held} samples, fewer than data_samples = "
                              f"{self.data_samples}; the real score (cached from now on) is that of {held} samples")
            kept = min(held, share)
            self.real = ([self._pair_mean(torch.cat(r)[:kept]) for r in real], kept)
        real_scores, kept = self.real
        generator.to(self.device).eval()
        fake = [[] for _ in channels]
        for _ in range(math.ceil(kept / self.batch_size)):
            fake_images = generator(input=self._latents(generator))
            for k, c in enumerate(channels):
                fake[k].append(self._planes(fake_images, c))
        scores = []
        for r, f in zip(real_scores, fake):
            value = self._pair_mean(torch.cat(f)[:kept])
            scores.append(DiversityScore(value, r, value - r))
        return self._result(scores)


class MSSSIM(_MsSsimDiversity):
    """Mean pairwise MS-SSIM of generated frames beside that of dataset frames: channel ``c`` of one drawn time step (as ``FID``
    draws it) at its own size, ``metric_inputs(..., size=None, normalize=None, planes=1)``."""

    def _inputs(self, images, channel):
        return metric_inputs(images, channel, t=_draw_time_step(images), size=None, normalize=None, planes=1)


class MSSSIMVideo(_MsSsimDiversity):
    """The same over whole clips of channel ``c`` (as ``FVD`` takes them): the ``T`` frames are the planes of a sample, and a
    pair scores the mean over them."""

    def _inputs(self, images, channel):
        return metric_inputs(images, channel, t=None, size=None, normalize=None, planes=1)
