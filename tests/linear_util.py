"""Shared by tests/test_linear_reference.py and tests/test_hip_linear.py: the few-row equalized-lr linear layer and its
derivatives as plain torch, written from the formulas of include/msg_hip.h (msg_linear_fprop / _dgrad / _wgrad and their grouped
forms) -- nothing here calls multi_stylegan_amd.  Every function computes in the dtype of its inputs: float64 is the reference,
the same call on float32 inputs gives e32, the rounding level of a plain fp32 evaluation that the kernels' bounds are multiples
of.  The case lists of the GPU module live here too, so that the CPU module can hold e32 to rounding level for every one of them."""
import functools

import torch

GAIN, BIAS_GAIN = 0.37, 1.3
FLOOR = 2.0 ** -21


def draw(gen, *shape):
    """Normal values drawn in float64 and made float32-exact: the reference and the kernel see the same numbers."""
    return torch.randn(*shape, generator=gen, dtype=torch.float64).float().double()


def rel_err(a, b):
    """max|a - b| / max|b| in float64 (conftest.rel_err; an all-zero reference degenerates to the absolute error)."""
    a, b = a.double(), b.double()
    scale = b.abs().max().item() if b.numel() else 0.0
    return ((a - b).abs().max() / (scale if scale > 0 else 1.0)).item() if b.numel() else 0.0


# ------------------------------------------------------------------------------------------- the definitions
def fprop(x, w, bias, gain, bias_gain):
    """y[M,N] = gain * x[M,K] . w[N,K]^T + bias_gain * bias[N]   (bias may be None)"""
    y = gain * (x @ w.t())
    return y if bias is None else y + bias_gain * bias[None, :]


def dgrad(gy, w, gain):
    """gx[M,K] = gain * gy[M,N] . w[N,K]"""
    return gain * (gy @ w)


def wgrad(gy, x, gain, bias_gain):
    """-> (gw[N,K] = gain * gy[M,N]^T . x[M,K],  gb[N] = bias_gain * sum_m gy[m,n])"""
    return gain * (gy.t() @ x), bias_gain * gy.sum(dim=0)


def grouped_fprop(latent, slot, ws, biases, gain, bias_gain):
    """latent [M,L,K]; group g reads latent[:, slot[g]], its own ws[g] [N,K] and biases[g] [N] (biases may be None) -> [G,M,N]"""
    return torch.stack([fprop(latent[:, s], ws[g], None if biases is None else biases[g], gain, bias_gain)
                        for g, s in enumerate(slot)])


def grouped_dgrad(gy, ws, slot, n_slots, gain):
    """gy [G,M,N] -> (gx [G,M,K], glat [M,L,K]): glat[:, l] is the sum, in the order of g, of the gx[g] with slot[g] == l
    (zero for a slot no group reads)."""
    gx = torch.stack([dgrad(gy[g], ws[g], gain) for g in range(len(slot))])
    glat = torch.zeros(gx.shape[1], n_slots, gx.shape[2], dtype=gx.dtype)
    for g, s in enumerate(slot):
        glat[:, s] = glat[:, s] + gx[g]
    return gx, glat


def grouped_wgrad(gy, latent, slot, gain, bias_gain):
    """gy [G,M,N], latent [M,L,K] -> (gw [G,N,K], gb [G,N])"""
    pairs = [wgrad(gy[g], latent[:, s], gain, bias_gain) for g, s in enumerate(slot)]
    return torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])


# ------------------------------------------------------------------------------------------- the operators, by autograd
def _leaves(*ts):
    return [None if t is None else t.detach().clone().requires_grad_(True) for t in ts]


def operator_quantities(x, w, bias, gy, gain, bias_gain):
    """Everything tests/test_hip_linear.py asks of conv_ops.linear, by torch.autograd on `fprop`: the value, the first-order
    gradients, and the second order in the two forms the regularisers use -- d/d(w, gy) of |dy/dx|^2 (R1 through the head, path
    length through the style affines) and d/d(gy, x) of |dy/dw|^2 (whose derivative in w is identically zero: dy/dw does not
    depend on w).  dy/dx and dy/dw are taken with the cotangent gy."""
    x, w, bias, gy = _leaves(x, w, bias, gy)
    ins = [x, w] + ([bias] if bias is not None else [])
    y = fprop(x, w, bias, gain, bias_gain)
    first = torch.autograd.grad(y, ins, gy, create_graph=True)
    out = {"y": y, "gx": first[0], "gw": first[1]}
    if bias is not None:
        out["gb"] = first[2]
    out["d|gx|2/dw"], out["d|gx|2/dgy"] = torch.autograd.grad(first[0].square().sum(), (w, gy), retain_graph=True)
    out["d|gw|2/dgy"], out["d|gw|2/dx"] = torch.autograd.grad(first[1].square().sum(), (gy, x), retain_graph=True)
    return {k: v.detach() for k, v in out.items()}


def grouped_operator_quantities(latent, slot, ws, biases, gy, gain, bias_gain):
    """The same for conv_ops.grouped_linear: value, first order (latent, every weight, every bias), and the latent-only second
    order of the path-length regulariser, d/d(w_g, gy) of |d out / d latent|^2."""
    latent, gy = _leaves(latent, gy)
    ws, biases = _leaves(*ws), _leaves(*biases)
    y = grouped_fprop(latent, slot, ws, biases, gain, bias_gain)
    first = torch.autograd.grad(y, [latent, *ws, *biases], gy, create_graph=True)
    g = len(slot)
    out = {"y": y, "glat": first[0], "gw": torch.stack(first[1:1 + g]), "gb": torch.stack(first[1 + g:])}
    second = torch.autograd.grad(first[0].square().sum(), [*ws, gy])
    out["d|glat|2/dw"], out["d|glat|2/dgy"] = torch.stack(second[:g]), second[g]
    return {k: v.detach() for k, v in out.items()}


# ------------------------------------------------------------------------------------------- the cases
def _around(base, m=(), n=(), k=(), extra=()):
    """One axis at a time around `base` = (M,N,K), then the named combinations; no case twice."""
    out = [tuple(base)]
    for axis, values in enumerate((m, n, k)):
        for v in values:
            c = list(base)
            c[axis] = v
            out.append(tuple(c))
    out += list(extra)
    return [c for i, c in enumerate(out) if c not in out[:i]]


BASE = (3, 5, 70)
# LIN_MB = 16 rows per block; 4 columns n per workgroup; 64 lanes along k, LIN_KC = 1024 per register chunk
FPROP_CASES = _around(BASE, m=(1, 15, 16, 17, 33, 256), n=(1, 3, 4, 5, 9), k=(1, 63, 64, 65, 1023, 1024, 1025, 2049),
                      extra=[(17, 5, 1025)])
# 64 columns k per workgroup; 16 waves share the rows n of a staged chunk of LIN_NCH = 1024
DGRAD_CASES = _around(BASE, k=(1, 63, 64, 65, 130), n=(1, 15, 16, 17, 1023, 1024, 1025, 2050), m=(1, 16, 17, 40),
                      extra=[(40, 1025, 65)])
# one workgroup per n, 256 threads along k, a serial loop over m
WGRAD_CASES = _around(BASE, k=(1, 255, 256, 257, 600), n=(1, 5), m=(1, 17, 256))
# G, L, slot: repeats and unused slots
GROUPS = [(1, 1, (0,)), (3, 4, (2, 0, 2)), (20, 14, (13, 0, 5, 5, 2, 9, 0, 13, 7, 1, 5, 11, 3, 3, 8, 0, 12, 6, 13, 2))]
GROUPED_CASES = {"fprop": [g + s for g in GROUPS for s in ((17, 5, 1025), (3, 40, 24))],
                 "wgrad": [g + s for g in GROUPS for s in ((17, 5, 1025), (3, 40, 24))],
                 "dgrad": [g + (17, 1025, 65) for g in GROUPS]}
# M, N, K, with bias: conv_ops.linear
OPERATOR_CASES = [(17, 5, 1025, True), (17, 5, 1025, False), (33, 1025, 65, True), (33, 1025, 65, False), (1, 1, 128, True)]
GROUPED_OPERATOR_CASE = (3, 4, (2, 0, 2), 17, 5, 1025)                  # G, L, slot, B, N, K
ENTRY_SEED = {"fprop": 1, "dgrad": 2, "wgrad": 3, "operator": 4}


def case_id(c):
    return "-".join(("s" + "".join("%x" % s for s in v)) if isinstance(v, tuple) else str(int(v)) for v in c)


def _gen(entry, *dims):
    seed = ENTRY_SEED[entry]
    for d in dims:
        seed = (seed * 4099 + int(d)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def inputs(entry, m, n, k):
    gen = _gen(entry, m, n, k)
    return {"x": draw(gen, m, k), "w": draw(gen, n, k), "bias": draw(gen, n), "gy": draw(gen, m, n)}


@functools.lru_cache(maxsize=None)
def grouped_inputs(entry, g, l, slot, m, n, k):
    gen = _gen(entry, g, l, m, n, k)
    return {"latent": draw(gen, m, l, k), "slot": slot, "ws": [draw(gen, n, k) for _ in range(g)],
            "biases": [draw(gen, n) for _ in range(g)], "gy": draw(gen, g, m, n)}


@functools.lru_cache(maxsize=None)
def operator_inputs(m, n, k, slots=3, j=1):
    """x is the [:, j] slice of a [B,L,K] latent, the weight the transposed view of a [K,N] tensor: neither is contiguous."""
    gen = _gen("operator", m, n, k)
    return {"latent": draw(gen, m, slots, k), "j": j, "wt": draw(gen, k, n), "bias": draw(gen, n), "gy": draw(gen, m, n)}


def _f32(v):
    if isinstance(v, torch.Tensor):
        return v.float()
    if isinstance(v, (list, tuple)) and v and isinstance(v[0], torch.Tensor):
        return [t.float() for t in v]
    return v


def _both(fn, **kw):
    """-> {quantity: (float64 reference, e32)} of fn(**kw) -> {quantity: tensor}; for a [G,...] stack listed in fn.by_group e32
    is a list, one figure per group."""
    ref, f32 = fn(**kw), fn(**{k: _f32(v) for k, v in kw.items()})
    out = {}
    for q in ref:
        assert f32[q].dtype == torch.float32 and ref[q].dtype == torch.float64, q
        if q in getattr(fn, "by_group", ()):
            out[q] = (ref[q], [rel_err(f32[q][g], ref[q][g]) for g in range(ref[q].shape[0])])
        else:
            out[q] = (ref[q], rel_err(f32[q], ref[q]))
    return out


def _fprop_q(x, w, bias, gy):
    return {"y": fprop(x, w, bias, GAIN, BIAS_GAIN), "y bias=NULL": fprop(x, w, None, GAIN, BIAS_GAIN)}


def _dgrad_q(x, w, bias, gy):
    return {"gx": dgrad(gy, w, GAIN)}


def _wgrad_q(x, w, bias, gy):
    return dict(zip(("gw", "gb"), wgrad(gy, x, GAIN, BIAS_GAIN)))


def _grouped_fprop_q(latent, slot, ws, biases, gy):
    return {"y": grouped_fprop(latent, slot, ws, biases, GAIN, BIAS_GAIN),
            "y bias=NULL": grouped_fprop(latent, slot, ws, None, GAIN, BIAS_GAIN)}


def _grouped_dgrad_q(latent, slot, ws, biases, gy):
    return dict(zip(("gx", "glat"), grouped_dgrad(gy, ws, slot, latent.shape[1], GAIN)))


def _grouped_wgrad_q(latent, slot, ws, biases, gy):
    return dict(zip(("gw", "gb"), grouped_wgrad(gy, latent, slot, GAIN, BIAS_GAIN)))


_grouped_fprop_q.by_group = ("y", "y bias=NULL")
_grouped_dgrad_q.by_group = ("gx",)
_grouped_wgrad_q.by_group = ("gw", "gb")
_SINGLE = {"fprop": _fprop_q, "dgrad": _dgrad_q, "wgrad": _wgrad_q}
_GROUPED = {"fprop": _grouped_fprop_q, "dgrad": _grouped_dgrad_q, "wgrad": _grouped_wgrad_q}


@functools.lru_cache(maxsize=None)
def reference(entry, m, n, k):
    return _both(_SINGLE[entry], **inputs(entry, m, n, k))


@functools.lru_cache(maxsize=None)
def grouped_reference(entry, g, l, slot, m, n, k):
    return _both(_GROUPED[entry], **grouped_inputs(entry, g, l, slot, m, n, k))


def _operator_q(latent, j, wt, bias, gy):
    return operator_quantities(latent[:, j], wt.t(), bias, gy, GAIN, BIAS_GAIN)


@functools.lru_cache(maxsize=None)
def operator_reference(m, n, k, has_bias):
    x = dict(operator_inputs(m, n, k))
    if not has_bias:
        x["bias"] = None
    return _both(_operator_q, **x)


def _grouped_operator_q(latent, slot, ws, biases, gy):
    return grouped_operator_quantities(latent, slot, ws, biases, gy, GAIN, BIAS_GAIN)


_grouped_operator_q.by_group = ("y", "gw", "gb", "d|glat|2/dw", "d|glat|2/dgy")


@functools.lru_cache(maxsize=None)
def grouped_operator_reference(g, l, slot, m, n, k):
    return _both(_grouped_operator_q, **grouped_inputs("operator", g, l, slot, m, n, k))


def bound(e32, factor=8):
    """max|got - ref| / max|ref| <= max(factor * e32, 2^-21)"""
    return max(factor * e32, FLOOR)
