"""Weight images: the K-contiguous kernel-side copies of a weight that the contraction kernels read (conv_ops), how each is
built, and the store that keeps those of a PARAMETER until the parameter changes.

A caller asks for an image by what it is -- forward / dgrad / tap_square_sums / thin / thin_dgrad / dgrad_s2 -- and gets
(tensor, padded extent, ...) back.  Whether csrc/relayout.hip (one launch: forward image, data-gradient image and sum of squared
taps) or a torch transpose-copy built it is decided in here (_build); a weight that is no nn.Parameter (the per-sample weights of
the modulated convolution's composite form, the cotangents of second-order graphs) is built and never stored.
"""
from typing import Tuple

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_hook

from . import _lib


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _k_run(dtype) -> int:
    """Elements of one 128-byte K run: the unit the contraction kernels read, and every image's K extent is padded to."""
    return 64 if dtype == torch.bfloat16 else 32


def _oi(w):
    """(out channels, in channels) of a weight in [O,I], [O,I,kh,kw] or [B,O,I,kh,kw] form."""
    return (w.shape[0], w.shape[1]) if w.ndim == 2 else (w.shape[-4], w.shape[-3])


# ------------------------------------------------------------------------------------------- formats and builders
def _torch_fwd(w: torch.Tensor, dtype, kind="conv") -> Tuple[torch.Tensor, int]:
    """The forward image of [..., O, I, kh, kw] by a torch transpose-copy: where the kernel is not eligible, and the tests'
    reference for it."""
    *lead, o, i, kh, kw = w.shape
    ck = _round_up(i, _k_run(dtype))
    out = torch.zeros((*lead, o, kh * kw, ck), dtype=dtype, device=w.device)
    out[..., :i] = w.reshape(*lead, o, i, kh * kw).transpose(-1, -2)
    return _up2_rows(out, ck) if kind == "up2" else (out, ck)


def _torch_dgrad(w: torch.Tensor, dtype, flip: bool) -> Tuple[torch.Tensor, int]:
    """The data-gradient image by a torch transpose-copy (see _torch_fwd)."""
    *lead, o, i, kh, kw = w.shape
    ok = _round_up(o, _k_run(dtype))
    src = w.reshape(*lead, o, i, kh * kw)
    if flip:
        src = src.flip(-1)
    out = torch.zeros((*lead, i, kh * kw, ok), dtype=dtype, device=w.device)
    out[..., :o] = src.permute(*range(len(lead)), len(lead) + 1, len(lead) + 2, len(lead))
    return out, ok


def _up2_rows(wk, ck):
    """[..., O, 4, Ck] -> [..., 4*O, 1, Ck]: rows n = (2dy+dx)*O + o  <-  w[o, :, dy, dx]."""
    return wk.transpose(-3, -2).reshape(*wk.shape[:-3], 4 * wk.shape[-3], 1, ck).contiguous(), ck


def _relayout(src, fwd, dgr, wsq, rows, i, t, ck, ok, flip, up2, gain=1.0) -> None:
    """csrc/relayout.hip on `rows` x i x t weights at src: whichever of the forward image, the data-gradient image and the sum
    of squared taps is given."""
    dev = src.device
    with _lib.on_device(dev):
        code = _lib.lib().msg_relayout_weight(src.data_ptr(), _lib.ptr(fwd), _lib.ptr(dgr), _lib.ptr(wsq),
                                              _lib.dtype_code(fwd if fwd is not None else dgr), rows, i, t, ck, ok, int(flip),
                                              int(up2), float(gain), _lib.stream_of(dev))
    _lib.check(code, "msg_relayout_weight")


def _relayout_kernel_ok(w, dtype, taps) -> bool:
    return w.is_cuda and w.dtype == torch.float32 and dtype in (torch.bfloat16, torch.float32) and \
        taps <= 16 and w.ndim >= 4


def _relay_fwd(w: torch.Tensor, dtype, kind="conv") -> Tuple[torch.Tensor, int]:
    """[..., O, I, kh, kw] -> [..., O, kh*kw, Ck] (K-contiguous, input channels zero-padded to a 128-byte run); up2: see
    _up2_rows."""
    if w.ndim == 2:
        w = w[:, :, None, None]
    if not _relayout_kernel_ok(w, dtype, w.shape[-2] * w.shape[-1]):
        return _torch_fwd(w, dtype, kind)
    # per-sample (or any non-parameter) fp32 weights: the kernel of _fused_images, the leading dimensions folded
    # into the rows -- one pass instead of a zero fill and a transposing, casting copy
    *lead, o, i, kh, kw = w.shape
    ck = _round_up(i, _k_run(dtype))
    out = torch.empty((*lead, o, kh * kw, ck), dtype=dtype, device=w.device)
    _relayout(w.detach().contiguous(), out, None, None, w.numel() // (i * kh * kw), i, kh * kw, ck, ck, False, False)
    return _up2_rows(out, ck) if kind == "up2" else (out, ck)


def _relay_dgrad(w: torch.Tensor, dtype, flip: bool) -> Tuple[torch.Tensor, int]:
    """[..., O, I, kh, kw] -> [..., I, kh*kw (flipped if asked), Ok]: the weights of the data-gradient contraction."""
    if w.ndim == 2:
        w = w[:, :, None, None]
    if w.ndim > 5 or not _relayout_kernel_ok(w, dtype, w.shape[-2] * w.shape[-1]):
        return _torch_dgrad(w, dtype, flip)
    *lead, o, i, kh, kw = w.shape
    ok = _round_up(o, _k_run(dtype))
    n = lead[0] if lead else 1
    out = torch.empty((*lead, i, kh * kw, ok), dtype=dtype, device=w.device)
    w3 = w.detach().contiguous().view(n, o, i, kh * kw)
    ov = out.view(n, i, kh * kw, ok)
    for k in range(n):                          # (the data-gradient image is per sample: one small launch each)
        _relayout(w3[k], None, ov[k], None, o, i, kh * kw, ok, ok, flip, False)
    return out, ok


def _s2_plan(k: int, pad: int):
    """Stride-2 data gradient as a stride-1 gather over gy, one sub-filter per output parity (1-D plan).
    gx[2c + ph] = sum_u gy[c + e - u] * w[t0 + 2u]  with t0 = (ph + pad) % 2, e = (ph + pad - t0) / 2.
    -> (taps U, pad', table[ph][tau] = forward tap index or -1): gy index = c + tau - pad'."""
    offs = {}
    for ph in (0, 1):
        t0 = (ph + pad) % 2
        e = (ph + pad - t0) // 2
        for u in range((k - t0 + 1) // 2):
            offs[(ph, e - u)] = t0 + 2 * u
    dmin = min(d for _, d in offs)
    dmax = max(d for _, d in offs)
    taps = dmax - dmin + 1
    table = [[offs.get((ph, tau + dmin), -1) for tau in range(taps)] for ph in (0, 1)]
    return taps, -dmin, table


def _relay_dgrad_s2(w: torch.Tensor, dtype, pad: int) -> Tuple[torch.Tensor, int, int, int]:
    """[..., O, I, k, k] -> [..., 4*I, U*U, Ok]: the stride-2 data gradient as ONE stride-1 conv over gy with U x U taps
    whose 4*I output channels are the four output parities (written pixel-shuffled by the kernel).  Compared with
    the zero-insertion form (in_up = 2) the matrix cores skip the 3/4 of the taps that only ever meet parity holes."""
    *lead, o, i, kh, kw = w.shape
    assert kh == kw
    taps, pad2, table = _s2_plan(kh, pad)
    ok = _round_up(o, _k_run(dtype))
    # one gather instead of a copy per (parity, tap): source tap index per (parity, tap), kh * kw = "no tap" (a zero plane)
    src = [[(table[ph][th] * kw + table[pw][tw]) if table[ph][th] >= 0 and table[pw][tw] >= 0 else kh * kw
            for th in range(taps) for tw in range(taps)] for ph in (0, 1) for pw in (0, 1)]
    idx = torch.tensor(src, dtype=torch.long, device=w.device)                   # [4, taps^2]
    wt = w.transpose(-4, -3).reshape(*lead, i, o, kh * kw)                       # [..., I, O, kh*kw]
    wz = torch.cat([wt, wt.new_zeros((*lead, i, o, 1))], dim=-1)                 # (+ the zero plane)
    picked = wz[..., idx]                                                        # [..., I, O, 4, taps^2]
    n = len(lead)
    picked = picked.permute(*range(n), n + 2, n, n + 3, n + 1)                   # [..., 4, I, taps^2, O]
    out = torch.zeros((*lead, 4, i, taps * taps, ok), dtype=dtype, device=w.device)
    out[..., :o] = picked
    return out.reshape(*lead, 4 * i, taps * taps, ok), ok, taps, pad2


def _relay_thin(w, dtype):
    """[O, I, kh, kw] -> [O, 1, Ko] with K index (tap * I + channel), zero-padded to one 128-byte run."""
    o, i, kh, kw = w.shape
    ko = _k_run(dtype)
    out = torch.zeros((o, 1, ko), dtype=dtype, device=w.device)
    out[:, 0, :kh * kw * i] = w.permute(0, 2, 3, 1).reshape(o, kh * kw * i)
    return out, ko


def _relay_thin_dgrad(w, dtype):
    """[O, I, kh, kw] -> [Ko, 1, Ok]: row k = tap * I + c holds w[:, c, tap] -- the weights of the 1x1 contraction from the
    output gradient to the tap-gathered input's gradient (the transpose of _relay_thin)."""
    o, i, kh, kw = w.shape
    ko, ok = _k_run(dtype), _round_up(o, _k_run(dtype))
    out = torch.zeros((ko, 1, ok), dtype=dtype, device=w.device)
    out[:kh * kw * i, 0, :o] = w.permute(2, 3, 1, 0).reshape(kh * kw * i, o)
    return out, ok


def _torch_modulation_base(w, what, kind):
    """The fp32, unpadded images that the modulated conv scales per sample, from a shared weight [1, O, I, kh, kw]:
    'f' conv -> [O][taps][I], up2 -> rows n = q*O + o, one tap;  'd' [I][taps (flipped for convs)][O];  'wsq' [O][I]."""
    o, i = _oi(w)
    t = w.numel() // (o * i)
    w3 = w.detach().reshape(o, i, t)
    if what == "f":
        return (w3.permute(2, 0, 1).reshape(t * o, 1, i) if kind == "up2" else w3.transpose(1, 2)).contiguous(), i
    if what == "d":
        return (w3 if kind == "up2" else w3.flip(-1)).permute(1, 2, 0).contiguous(), o
    return w3.square().sum(dim=2).contiguous(), 0


def _fused_images(w, dtype, gain, kind, modulation):
    """'f', 'd' (and, for the modulation bases, 'wsq') of a shared weight by ONE launch of csrc/relayout.hip; the gain is
    multiplied in fp32, before the one rounding to the storage type.  None where that kernel does not apply: it takes a
    Parameter on the GPU, fp32, of at most 16 taps and a dense shape ([O,I,kh,kw] or the modulated conv's [1,O,I,kh,kw])."""
    if not (isinstance(w, torch.nn.Parameter) and w.is_cuda and w.dtype == torch.float32):
        return None
    o, i = _oi(w)
    t = w.numel() // (o * i)
    if t > 16 or w.numel() != o * i * t:
        return None
    dev = w.device
    unit = 1 if modulation else _k_run(dtype)
    ck, ok = _round_up(i, unit), _round_up(o, unit)
    up2 = kind == "up2"
    w3 = w.detach().reshape(o, i, t).contiguous()
    fwd = torch.empty((t * o, 1, ck) if up2 else (o, t, ck), dtype=dtype, device=dev)
    dgr = torch.empty((i, t, ok), dtype=dtype, device=dev)
    wsq = torch.empty((o, i), dtype=torch.float32, device=dev) if modulation else None
    _relayout(w3, fwd, dgr, wsq, o, i, t, ck, ok, not up2, up2, gain)
    out = {"f": (fwd, ck), "d": (dgr, ok)}
    if modulation:
        out["wsq"] = (wsq, 0)
    return out


def _scaled(out, gain):
    """A torch-built image takes the gain AFTER the cast, in the storage type."""
    return (out[0] * gain, *out[1:]) if gain != 1.0 else out


def _build(w, what, dtype, gain, kind, modulation, pad):
    """-> {name: image}: the image asked for, and whatever else its builder makes in the same pass."""
    fused = _fused_images(w, dtype, gain, kind, modulation) if what in ("f", "d", "wsq") else None
    if fused is not None:
        return fused
    if modulation:
        return {what: _torch_modulation_base(w, what, kind)}
    if what == "f":
        out = _relay_fwd(w, dtype, kind)
    elif what == "d":
        out = _relay_dgrad(w, dtype, flip=kind != "up2")
    elif what == "s2":
        out = _relay_dgrad_s2(w, dtype, pad)
    else:
        out = {"thin": _relay_thin, "dthin": _relay_thin_dgrad}[what](w, dtype)
    return {what: _scaled(out, gain)}


# ------------------------------------------------------------------------------------------------------ the store
# Re-laid copies of PARAMETERS are cached between weight updates: D runs three times and G two to three times per
# iteration on unchanged weights.  The cache lives ON the nn.Parameter object (it dies with it and can never alias a
# recycled address) and is validated against (a) the tensor's in-place version counter and (b) a global weight
# generation that every torch optimizer step bumps (fused/foreach optimizers and `.data` writes do not touch the
# version counter).  Code that writes parameters behind both mechanisms must call invalidate_weight_cache().
_WEIGHT_GENERATION = [0]


def invalidate_weight_cache(params=None) -> None:
    """Declare parameters changed behind autograd's back (`.data` writes, fused / foreach optimizers do not bump the
    tensors' version counters): the given ones, or -- with no argument -- every cached image of every parameter."""
    if params is None:
        _WEIGHT_GENERATION[0] += 1
        return
    for p in params:
        p.__dict__["_msg_gen"] = p.__dict__.get("_msg_gen", 0) + 1


def _after_optimizer_step(optimizer, *_args, **_kwargs) -> None:
    # only the parameters THIS optimizer owns changed: the discriminator's step must not throw away the generator's
    # re-laid weights (and vice versa) -- with one global generation every weight was re-laid twice per iteration
    for group in optimizer.param_groups:
        invalidate_weight_cache(group["params"])


_register_step_hook(_after_optimizer_step)


def _stamp(w):
    return (w._version, _WEIGHT_GENERATION[0], w.__dict__.get("_msg_gen", 0), w.data_ptr())


def _image(w, what, dtype, gain, kind="conv", modulation=False, pad=0):
    key = (what, dtype, gain, kind, modulation, pad)
    store = w.__dict__.get("_msg_relay")
    if store is not None:                      # (the hit path first: ~240 lookups per training iteration on the host's critical path)
        hit = store.get(key)
        if hit is not None and hit[0] == _stamp(w):
            return hit[1]
    if not isinstance(w, torch.nn.Parameter):
        return _build(w, *key)[what]
    stamp = _stamp(w)
    with torch.no_grad():
        built = _build(w, *key)
    store = w.__dict__.setdefault("_msg_relay", {})
    for name, image in built.items():          # (the fused kernel fills 'f', 'd' and 'wsq' under one stamp)
        store[(name, *key[1:])] = (stamp, image)
    return built[what]


# --------------------------------------------------------------------------------------------------- the accessors
def forward(w, dtype, gain=1.0, kind="conv", modulation=False, per_sample=False):
    """-> (forward image, Ck).  conv: [O][taps][Ck]; up2: [4*O][1][Ck]; per_sample: [B] of them, never stored.
    modulation (of the modulated conv's shared weight [1, O, I, kh, kw], fp32, no gain): the unpadded base that
    msg_modulate_weights / msg_scale_rows_cols scale per sample."""
    if per_sample:
        return _scaled(_relay_fwd(w, dtype, kind), gain)
    return _image(w, "f", dtype, gain, kind, modulation)


def dgrad(w, dtype, gain=1.0, kind="conv", modulation=False, per_sample=False):
    """-> (data-gradient image [I][taps, flipped for convs][Ok], Ok); modulation, per_sample as for forward()."""
    if per_sample:
        return _scaled(_relay_dgrad(w, dtype, flip=kind != "up2"), gain)
    return _image(w, "d", dtype, gain, kind, modulation)


def tap_square_sums(w, kind="conv"):
    """wsq[o][i] = sum over taps of W^2, fp32: built with the modulation bases."""
    return _image(w, "wsq", torch.float32, 1.0, kind, True)[0]


def thin(w, dtype, gain=1.0):
    """-> ([O][1][Ko], Ko): the forward image of the tap-gathered 1x1 form (_relay_thin)."""
    return _image(w, "thin", dtype, gain)


def thin_dgrad(w, dtype, gain=1.0):
    """-> ([Ko][1][Ok], Ok): the data-gradient image of the tap-gathered 1x1 form (_relay_thin_dgrad)."""
    return _image(w, "dthin", dtype, gain)


def dgrad_s2(w, dtype, gain, pad):
    """-> ([4*I][U*U][Ok], Ok, U, pad'): the parity image of a stride-2 conv's data gradient (_relay_dgrad_s2)."""
    return _image(w, "s2", dtype, gain, pad=pad)
