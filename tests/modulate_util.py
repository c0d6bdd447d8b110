"""Shared by tests/test_modulate_reference.py and tests/test_hip_modulate.py: the weight modulation / demodulation of the
dual-styled convolution and its first and second derivatives as plain torch, written from the definition
(multi_stylegan_generator.py:379-388) and differentiated by autograd -- nothing here is taken from csrc/modulate.hip, so none
of its factored closed forms.  Every function computes in the dtype of its inputs: float64 is the reference, the same call
on float32 inputs gives the rounding level of a plain fp32 evaluation that the kernels' bounds are derived from."""
import math

import torch


def draw(gen, *shape, mean=0.0, std=1.0):
    """Normal values drawn in float64 and made float32-exact: the reference and the kernel see the same numbers."""
    return (torch.randn(*shape, generator=gen, dtype=torch.float64) * std + mean).float().double()


def conv_scale(i, t):
    return math.sqrt(2.0) / math.sqrt(i * t)


def weights(W, s, scale, demod, eps=1e-8):
    """W [O,I,T], s [B,I] -> (w [B,O,I,T] = scale * d[b,o] * W[o,i,t] * s[b,i], d [B,O]);
    d = rsqrt(scale^2 * sum_{i,t} (W s)^2 + eps), or 1 without demodulation."""
    ws = W[None, :, :, :] * s[:, None, :, None]
    if demod:
        d = torch.rsqrt(scale * scale * ws.square().sum(dim=(2, 3)) + eps)
    else:
        d = torch.ones(s.shape[0], W.shape[0], dtype=W.dtype)
    return scale * d[:, :, None, None] * ws, d


def _leaves(*ts):
    return [t.detach().clone().requires_grad_(True) for t in ts]


def fold(W, s, g, scale, demod):
    """g [B,O,T,I]: the per-sample weight gradient as the kernels lay it out -> (gW [O,I,T], gs_by_o [O,B,I]): the gradient
    of <g, weights(W, s)> with respect to W, and with respect to s through output channel o alone."""
    W, s = _leaves(W, s)
    gt = g.permute(0, 1, 3, 2)
    w, _ = weights(W, s, scale, demod)
    gW, = torch.autograd.grad(w, W, gt, retain_graph=True)
    rows = [torch.autograd.grad(w[:, o], s, gt[:, o], retain_graph=True)[0] for o in range(W.shape[0])]
    return gW, torch.stack(rows)


def fold2(W, s, g, v, scale, demod):
    """-> (hW [O,I,T], hs_by_o [O,B,I]): the derivatives of L2 = <v, gs> with respect to W and s at fixed g, gs the style
    gradient of `fold`; row o of hs_by_o is the part of L2 that runs through output channel o.  (Without demodulation gs does
    not depend on s: those rows are exactly zero.)"""
    W, s = _leaves(W, s)
    gt = g.permute(0, 1, 3, 2)
    w, _ = weights(W, s, scale, demod)
    hW, rows = torch.zeros_like(W), []
    for o in range(W.shape[0]):
        gs_o, = torch.autograd.grad(w[:, o], s, gt[:, o], create_graph=True)
        hw_o, hs_o = torch.autograd.grad((v * gs_o).sum(), (W, s), retain_graph=True, allow_unused=True)
        hW = hW + hw_o
        rows.append(hs_o if hs_o is not None else torch.zeros_like(s))
    return hW, torch.stack(rows)


def scaled(base, row, col, gain):
    """base [R,T,C], row [B,R] | None, col [B,C] | None -> [B,R,T,C] = gain * base * row * col (None = 1; [1,R,T,C], to be broadcast, when both are None)."""
    out = gain * base[None]
    if row is not None:
        out = out * row[:, :, None, None]
    if col is not None:
        out = out * col[:, None, None, :]
    return out


def scaled2(base, row1, col1, row2, col2, gain):
    """-> [B,R,T,C] = gain * base * (row1 (x) col1 + row2 (x) col2)."""
    return gain * base[None] * (row1[:, :, None, None] * col1[:, None, None, :] + row2[:, :, None, None] * col2[:, None, None, :])


def bf16_rne(t):
    """Round to nearest even to bfloat16 (through float32: exact for float32-exact values), back in float64."""
    return t.float().bfloat16().double()


def bf16_ulp(t):
    """One bfloat16 unit in the last place at the magnitude of each element of t (0 for 0)."""
    _, e = torch.frexp(t.double().abs())                       # |t| = m * 2^e, m in [0.5, 1)
    return torch.where(t == 0, torch.zeros((), dtype=torch.float64), torch.ldexp(torch.ones((), dtype=torch.float64), e - 8))

