"""The adversarial objectives -- non-saturating logistic, Wasserstein, hinge; plain, weight-map and CutMix (label-map) forms --
as one streaming pass per direction (csrc/gan_loss.hip; reference multi_stylegan/loss.py:9-280).  ``gan_loss`` returns both
means of a real / fake pair as one fp32 [2] device tensor.  First-order backward on the kernel; a backward that is itself
differentiated re-derives itself from the plain-torch composite below, which is differentiable to any order and is also what
the loss modules use where the kernel does not apply (CPU tensors, other dtypes, weight maps of another shape).
"""
from typing import Optional

import torch
from torch.autograd import Function

from .. import _lib

KINDS = {"logistic": _lib.MSG_GAN_LOGISTIC, "wasserstein": _lib.MSG_GAN_WASSERSTEIN, "hinge": _lib.MSG_GAN_HINGE}


def _term(x: torch.Tensor, kind: str, fake: bool) -> torch.Tensor:
    """r(x) (fake=False) or f(x) (fake=True) of csrc/gan_loss.hip's table."""
    if kind == "logistic":
        return torch.nn.functional.softplus(x if fake else -x)
    if kind == "wasserstein":
        return x if fake else -x
    if kind == "hinge":
        return -torch.minimum(torch.zeros((), dtype=x.dtype, device=x.device), (-x if fake else x) - 1.)
    raise ValueError(f"kind {kind!r}: one of {sorted(KINDS)}")


def composite(pred_real: Optional[torch.Tensor], pred_fake: Optional[torch.Tensor], *, kind: str,
              weight: Optional[torch.Tensor] = None, label: Optional[torch.Tensor] = None):
    """(loss_real, loss_fake) in stock torch operators, any device and dtype: the reference's formulas.  An absent side is a
    zero.  Half-precision predictions are widened to fp32 first, as the kernel does; ``label``: both sides read pred_real."""
    def side(x, fake, like):
        if x is None:
            return torch.zeros((), dtype=like.dtype, device=like.device)
        if x.dtype in (torch.bfloat16, torch.float16):
            x = x.float()
        t = _term(x, kind, fake)
        if weight is not None:
            t = t * weight.view(1, 1, 1, weight.shape[-2], weight.shape[-1]).to(device=x.device, dtype=x.dtype)
        if label is not None:
            lab = label.to(device=x.device, dtype=x.dtype)
            t = t * ((-lab + 1.) if fake else lab)
        return t.mean()
    if label is not None:
        pred_fake = pred_real
    if pred_real is None and pred_fake is None:
        raise ValueError("gan_loss: both sides absent")
    like = (pred_real if pred_real is not None else pred_fake)
    like = like.float() if like.dtype in (torch.bfloat16, torch.float16) else like
    return side(pred_real, False, like), side(pred_fake, True, like)


def weight_fits(pred: Optional[torch.Tensor], weight: torch.Tensor) -> bool:
    """Whether ``weight.view(1, 1, 1, H, W) * pred`` is the kernel's a_i = w[i mod H W]: the last two dimensions agree."""
    return pred is None or (weight.ndim >= 2 and pred.ndim >= 2 and tuple(pred.shape[-2:]) == tuple(weight.shape[-2:])
                            and weight.numel() == weight.shape[-2] * weight.shape[-1])


class _GanLoss(Function):
    @staticmethod
    def forward(ctx, pred_real, pred_fake, aux, kind, mode):
        dev = _lib.require_gpu(pred_real, pred_fake, aux)
        first = pred_real if pred_real is not None else pred_fake
        code = _lib.dtype_code(first)
        n_real = pred_real.numel() if pred_real is not None else 0
        n_fake = pred_fake.numel() if pred_fake is not None else 0
        p = 0
        if mode == _lib.MSG_GAN_AUX_LABEL:
            n_fake = n_real
        elif mode == _lib.MSG_GAN_AUX_WEIGHT:
            p = aux.numel()
        out = torch.empty(2, dtype=torch.float32, device=dev)
        need = _lib.lib().msg_gan_loss_workspace(n_real, n_fake)
        with _lib.on_device(dev), _lib.kernel_clock.span(("gan_loss_fwd", kind, first.dtype),
                                                         (n_real + n_fake) * first.element_size()):
            status = _lib.lib().msg_gan_loss(_lib.ptr(pred_real), _lib.ptr(pred_fake), _lib.ptr(aux), out.data_ptr(), code,
                                             KINDS[kind], mode, n_real, n_fake, p, _lib.scratch_ptr(need, dev), need,
                                             _lib.stream_of(dev))
        _lib.check(status, "msg_gan_loss")
        ctx.save_for_backward(pred_real, pred_fake, aux)
        ctx.cfg = (kind, mode, code, n_real, n_fake, p)
        return out

    @staticmethod
    def backward(ctx, gout):
        pred_real, pred_fake, aux = ctx.saved_tensors
        kind, mode, code, n_real, n_fake, p = ctx.cfg
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():
            # a differentiated backward (R1 / R2 through a loss, gradient penalties): through the composite
            with torch.enable_grad():
                ins = [t for t, n in zip((pred_real, pred_fake), need[:2]) if n]
                first = pred_real if pred_real is not None else pred_fake
                outs = composite(pred_real, pred_fake, kind=kind,
                                 weight=aux.reshape(first.shape[-2:]) if mode == _lib.MSG_GAN_AUX_WEIGHT else None,
                                 label=aux.reshape(pred_real.shape) if mode == _lib.MSG_GAN_AUX_LABEL else None)
                grads = list(torch.autograd.grad(torch.stack([o.float() for o in outs]), ins, gout, create_graph=True,
                                                 allow_unused=True))
            got = [grads.pop(0) if n else None for n in need[:2]]
            return got[0], got[1], None, None, None
        dev = gout.device
        g32 = gout.detach().float().contiguous()
        g_real = torch.empty_like(pred_real) if need[0] and pred_real is not None else None
        g_fake = torch.empty_like(pred_fake) if need[1] and pred_fake is not None else None
        if g_real is None and g_fake is None:
            return None, None, None, None, None
        first = pred_real if pred_real is not None else pred_fake
        with _lib.on_device(dev), _lib.kernel_clock.span(("gan_loss_bwd", kind, first.dtype),
                                                         2 * (n_real + n_fake) * first.element_size()):
            status = _lib.lib().msg_gan_loss_backward(_lib.ptr(pred_real), _lib.ptr(pred_fake), _lib.ptr(aux), g32.data_ptr(),
                                                      _lib.ptr(g_real), _lib.ptr(g_fake), code, KINDS[kind], mode, n_real,
                                                      n_fake, p, _lib.stream_of(dev))
        _lib.check(status, "msg_gan_loss_backward")
        return g_real, g_fake, None, None, None


def gan_loss(pred_real: Optional[torch.Tensor], pred_fake: Optional[torch.Tensor], *, kind: str,
             weight: Optional[torch.Tensor] = None, label: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[loss_real, loss_fake] as an fp32 [2] device tensor (msg_gan_loss).  ``pred_real`` / ``pred_fake``: fp32 or bf16
    device tensors of the same dtype and any shape, either may be None (its loss is 0; a generator loss is the real side applied
    to fake predictions).  ``weight``: an H x W map over predictions [..., H, W] (the reference's weight.view(1, 1, 1, H, W)
    broadcast).  ``label``: a CutMix map with pred_real's element count; both sides then read pred_real and pred_fake must be
    None.  Raises MsgHipError for CPU tensors, other dtypes and mismatched shapes: there is no fallback here (the loss modules
    choose the composite themselves)."""
    if kind not in KINDS:
        raise _lib.MsgHipError(f"gan_loss: kind {kind!r} is not one of {sorted(KINDS)}")
    if pred_real is None and pred_fake is None:
        raise _lib.MsgHipError("gan_loss: both sides absent")
    if weight is not None and label is not None:
        raise _lib.MsgHipError("gan_loss: a weight map and a label map exclude each other")
    _lib.require_gpu(pred_real, pred_fake, weight, label)
    if pred_real is not None and pred_fake is not None and pred_real.dtype != pred_fake.dtype:
        raise _lib.MsgHipError(f"gan_loss: predictions of different dtypes ({pred_real.dtype}, {pred_fake.dtype})")
    _lib.dtype_code(pred_real if pred_real is not None else pred_fake)
    aux, mode = None, _lib.MSG_GAN_AUX_NONE
    if label is not None:
        if pred_real is None or pred_fake is not None:
            raise _lib.MsgHipError("gan_loss: the label form takes ONE prediction tensor, as pred_real")
        if label.numel() != pred_real.numel():
            raise _lib.MsgHipError(f"gan_loss: a label of {label.numel()} elements for a prediction of {pred_real.numel()}")
        aux, mode = label.detach().float().contiguous(), _lib.MSG_GAN_AUX_LABEL
    elif weight is not None:
        if not (weight_fits(pred_real, weight) and weight_fits(pred_fake, weight)):
            raise _lib.MsgHipError(f"gan_loss: a weight map of shape {tuple(weight.shape)} does not cover the predictions' last "
                                   "two dimensions")
        aux, mode = weight.detach().float().contiguous().reshape(-1), _lib.MSG_GAN_AUX_WEIGHT
    pred_real = pred_real.contiguous() if pred_real is not None else None
    pred_fake = pred_fake.contiguous() if pred_fake is not None else None
    return _GanLoss.apply(pred_real, pred_fake, aux, kind, mode)
