"""Losses and regularisers of the adversarial step, with the reference's class names
(multi_stylegan/loss.py:97-170, 283-317, 353-395).  All of them return device tensors; nothing here forces a
host synchronisation."""
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch import autograd


def _weighted(values: torch.Tensor, weight: Optional[torch.Tensor]) -> torch.Tensor:
    if weight is None:
        return values.mean()
    return (values * weight.view(1, 1, 1, weight.shape[-2], weight.shape[-1]).to(values.device)).mean()


class NonSaturatingLogisticGeneratorLoss(nn.Module):
    def forward(self, prediction_fake: torch.Tensor, weight: torch.Tensor = None) -> torch.Tensor:
        return _weighted(F.softplus(-prediction_fake), weight)


class NonSaturatingLogisticDiscriminatorLoss(nn.Module):
    def forward(self, prediction_real: torch.Tensor, prediction_fake: torch.Tensor,
                weight: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        return _weighted(F.softplus(-prediction_real), weight), _weighted(F.softplus(prediction_fake), weight)


class NonSaturatingLogisticDiscriminatorLossCutMix(nn.Module):
    """Per-pixel logistic loss against a binary CutMix label map (reference loss.py:173-196): the real term counts
    where the label is 1, the fake term where it is 0; both are means over ALL pixels."""

    def forward(self, prediction: torch.Tensor, label: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return (F.softplus(-prediction) * label).mean(), (F.softplus(prediction) * (1. - label)).mean()


class R1Regularization(nn.Module):
    def forward(self, prediction_real: torch.Tensor, image_real: torch.Tensor,
                prediction_real_pixel_wise: Optional[torch.Tensor] = None) -> torch.Tensor:
        outputs = prediction_real.sum() if prediction_real_pixel_wise is None else \
            (prediction_real.sum(), prediction_real_pixel_wise.sum())
        grad_real, = autograd.grad(outputs=outputs, inputs=image_real, create_graph=True)
        return 0.5 * grad_real.pow(2).reshape(grad_real.shape[0], -1).sum(1).mean()


class PathLengthRegularization(nn.Module):
    """Running-mean path-length penalty.  ``mean_path_length`` is a plain attribute in the reference (so it is lost
    on checkpoint, loss.py:369); here it is a persistent buffer and is all-reduced by the trainer under DDP."""

    def __init__(self, decay: float = 0.01) -> None:
        super().__init__()
        self.decay = decay
        self.register_buffer("mean_path_length", torch.zeros(1, dtype=torch.float))

    def forward(self, grad: torch.Tensor, reduce_fn=None) -> Tuple[torch.Tensor, torch.Tensor]:
        path_lengths = torch.sqrt(grad.pow(2).sum(2).mean(1) + 1e-08).mean()
        if reduce_fn is not None:
            # value of the global batch (the reference sees the gathered batch), gradient of the local shard:
            # averaged over ranks by the gradient all-reduce this reproduces the global-batch gradient exactly
            path_lengths = path_lengths + (reduce_fn(path_lengths.detach()) - path_lengths.detach())
        mean = self.mean_path_length.detach().to(grad.device)
        # NOT detached from path_lengths: the reference lets the gradient flow through the running mean
        # (loss.py:389-394), which scales the penalty gradient by (1 - decay)
        mean = mean + self.decay * (path_lengths - mean)
        penalty = torch.mean((path_lengths - mean) ** 2)
        self.mean_path_length = mean.detach()
        return penalty, path_lengths


class TopK(nn.Module):
    """Top-k training of the generator (reference loss.py:398-444): only the k = max(1, int(B v)) samples the
    discriminator rates most realistic contribute; v anneals linearly from 1 to 0.5 between `starting_iteration` and
    `final_iteration` (counted in forward calls).  Returns torch.topk's (values, indices) of the flattened scores."""

    def __init__(self, starting_iteration: int, final_iteration: int) -> None:
        super().__init__()
        self.starting_iteration = starting_iteration
        self.final_iteration = final_iteration
        self.iterations = 0

    def calc_v(self) -> float:
        self.iterations += 1
        if self.iterations <= self.starting_iteration:
            return 1.
        if self.iterations >= self.final_iteration:
            return 0.5
        progress = float(self.iterations - self.starting_iteration) / float(self.final_iteration - self.starting_iteration)
        return 0.5 * (1. - progress) + 0.5

    def forward(self, input: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        v = self.calc_v()
        scores = input.reshape(-1)
        return torch.topk(scores, k=max(1, int(scores.shape[0] * v)))


# ---------------------------------------------------------------------------------------------------------------------------
# The Wasserstein and hinge families (reference loss.py:9-94, 198-280) and R2 (:320-350).  On fp32 / bf16 device tensors their
# means and gradients are one kernel pair (op_static/gan_loss.py -> csrc/gan_loss.hip); CPU tensors, other dtypes and weight
# maps whose last two dimensions are not the prediction's go through the same formulas in stock torch operators
# (gan_loss.composite).  Every loss is an fp32 0-dim tensor, for bf16 predictions too (the reference returns bf16 there).
def _fused(*predictions: Optional[torch.Tensor], weight: Optional[torch.Tensor] = None) -> bool:
    from .op_static import gan_loss as op
    given = [p for p in predictions if p is not None]
    if not all(p.is_cuda and p.dtype == given[0].dtype and p.device == given[0].device for p in given):
        return False
    if given[0].dtype not in (torch.float32, torch.bfloat16) or any(p.numel() == 0 for p in given):
        return False
    return weight is None or all(op.weight_fits(p, weight) for p in given)


def _pair(kind: str, prediction_real: Optional[torch.Tensor], prediction_fake: Optional[torch.Tensor],
          weight: Optional[torch.Tensor] = None, label: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    from .op_static import gan_loss as op
    if label is not None and label.shape != prediction_real.shape:
        label = label.expand_as(prediction_real)            # (what the reference's multiply broadcasts to)
    if _fused(prediction_real, prediction_fake, weight=weight):
        device = (prediction_real if prediction_real is not None else prediction_fake).device
        out = op.gan_loss(prediction_real, prediction_fake, kind=kind, weight=None if weight is None else weight.to(device),
                          label=None if label is None else label.to(device))
        return out[0], out[1]
    return op.composite(prediction_real, prediction_fake, kind=kind, weight=weight, label=label)


class WassersteinDiscriminatorLoss(nn.Module):
    """(-mean(real w), mean(fake w)) (reference loss.py:9-40).  fp32 0-dim tensors, for bf16 predictions too (the reference
    returns bf16 there)."""

    def forward(self, prediction_real: torch.Tensor, prediction_fake: torch.Tensor,
                weight: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        return _pair("wasserstein", prediction_real, prediction_fake, weight)


class WassersteinDiscriminatorLossCutMix(nn.Module):
    """(-mean(prediction label), mean(prediction (1 - label))) (reference loss.py:43-65); both are means over ALL pixels.  fp32
    0-dim tensors, for bf16 predictions too (the reference returns bf16 there)."""

    def forward(self, prediction: torch.Tensor, label: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return _pair("wasserstein", prediction, None, label=label)


class WassersteinGeneratorLoss(nn.Module):
    """-mean(fake w) (reference loss.py:68-94): the discriminator's real side applied to fake predictions.  An fp32 0-dim
    tensor, for bf16 predictions too (the reference returns bf16 there)."""

    def forward(self, prediction_fake: torch.Tensor, weight: torch.Tensor = None) -> torch.Tensor:
        return _pair("wasserstein", prediction_fake, None, weight)[0]


class HingeGeneratorLoss(WassersteinGeneratorLoss):
    """The generator's hinge loss IS its Wasserstein loss (reference loss.py:198-209)."""


class HingeDiscriminatorLoss(nn.Module):
    """(-mean(min(0, real - 1) w), -mean(min(0, -fake - 1) w)) (reference loss.py:212-252).  At the kink (real == 1, fake == -1)
    the gradient is half the active side's, as torch.minimum's is at a tie; a NaN prediction gives a NaN loss.  fp32 0-dim
    tensors, for bf16 predictions too (the reference returns bf16 there)."""

    def forward(self, prediction_real: torch.Tensor, prediction_fake: torch.Tensor,
                weight: torch.Tensor = None) -> Tuple[torch.Tensor, torch.Tensor]:
        return _pair("hinge", prediction_real, prediction_fake, weight)


class HingeDiscriminatorLossCutMix(nn.Module):
    """(-mean(min(0, prediction - 1) label), -mean(min(0, -prediction - 1) (1 - label))) (reference loss.py:255-280); both are
    means over ALL pixels.  fp32 0-dim tensors, for bf16 predictions too (the reference returns bf16 there)."""

    def forward(self, prediction: torch.Tensor, label: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        return _pair("hinge", prediction, None, label=label)


class R2Regularization(nn.Module):
    """The gradient penalty on FAKE images: 0.5 mean_b sum (d sum(prediction_fake) / d image_fake)^2, with create_graph=True --
    R1's formula on the other batch, riding the same discriminator double backward.
    PARITY UNPINNED, reference raises: its forward (loss.py:339-350) calls ``.pow`` on the TUPLE autograd.grad returns and ends
    in an AttributeError, so there is no reference result to compare with; this implements what it states."""

    def forward(self, prediction_fake: torch.Tensor, image_fake: torch.Tensor) -> torch.Tensor:
        grad_fake, = autograd.grad(outputs=prediction_fake.sum(), inputs=image_fake, create_graph=True)
        return 0.5 * grad_fake.pow(2).reshape(grad_fake.shape[0], -1).sum(1).mean()
