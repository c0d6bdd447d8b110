"""An independent numpy statement of the structural-similarity definitions (multi_stylegan_amd/ssim.py, csrc/ssim.hip) and the
error bounds the tests hold the kernels to.  Nothing here imports the package.

Definitions: 11 taps g_k = exp(-(k - 5)^2 / 4.5) / sum, separable, "valid"; C1 = (0.01 R)^2, C2 = (0.03 R)^2;
cs = (2 s_xy + C2) / (s_xx + s_yy + C2), l = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1), ssim = cs l; scales halved by the 2 x 2
mean (floor); the weights (0.0448, 0.2856, 0.3001, 0.2363, 0.1333) cut to L and renormalised; a plane scores the product of the
clamped mean cs of the first L - 1 scales and the clamped mean ssim of the last, each to its weight.

Every function takes ``dtype``: float64 is the statement; float32 is the SAME statement with every array operation rounded to
fp32 (taps rounded once to fp32, a filter pass is the chain acc = g_0 v_0, acc = acc + g_k v_k in ascending k, two roundings
per tap where the kernels' fmaf has one).

Bounds.  include/msg_hip.h states the kernels' order of operations: products rounded before filtering, rows then columns,
ascending-tap chains, every pointwise operation rounded once, float64 sums.
  * halved planes: 0.25 ((v00 + v01) + (v10 + v11)) -- three roundings, the scaling exact: |err| <= 3 u (|v00| + |v01| + |v10| +
    |v11|) / 4 (1 + 3 u), u = 2^-24.
  * sum |x - y|: one rounding per term, float64 accumulation: |err| <= u sum |x - y| (1 + 1e-6).
  * the cs / ssim means and the gradient: s = g*x^2 - mu^2 cancels and is divided by D2 >= C2 = 9e-4, so a rigorous bound is
    orders of magnitude above what any sane order of operations gives and would test nothing.  Instead the float32 statement above
    is measured against the float64 one ON THE SAME INPUTS and the kernels are allowed 4 x that: the kernels differ from the
    float32 statement only in the order of the roundings (fmaf chains: fewer of them), which moves an error by a small factor, not
    by an order of magnitude.  For a mean the measure is the mean absolute error of the map (|mean err| <= mean |err|, and it
    cannot vanish by cancellation); for the gradient it is the largest absolute error over the plane.  On a plane of one or a few
    positions the measured error can still be small by chance, so the bound has a floor: the pointwise tail alone (the numerator's
    fmaf, the two additions of D2, the division, and the same for l and the product cs l; for the gradient the three fmaf and the
    L1 / g_half terms) is 8 roundings of values of the result's size, 8 u times that size.
"""
import numpy as np

TAPS = 11
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
U = 2.0 ** -24


def window(dtype=np.float64):
    k = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-(k - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return (g / g.sum()).astype(dtype)


def levels(h, w):
    n = 0
    while min(h, w) >= TAPS and n < len(WEIGHTS):
        n, h, w = n + 1, h // 2, w // 2
    return n


def constants(data_range=1.0):
    return (0.01 * data_range) ** 2, (0.03 * data_range) ** 2


def _fir(v, axis, dtype):
    """"valid" correlation of ``v`` with the window along ``axis`` (the window is symmetric), one ascending-tap chain."""
    g = window(dtype)
    n = v.shape[axis] - (TAPS - 1)
    acc = g[0] * np.take(v, range(0, n), axis=axis)
    for k in range(1, TAPS):
        acc = acc + g[k] * np.take(v, range(k, k + n), axis=axis)
    return acc.astype(dtype)


def blur(v, dtype):
    """Rows first (along the width), then columns."""
    return _fir(_fir(v, v.ndim - 1, dtype), v.ndim - 2, dtype)


def blur_t(v, dtype):
    """The transposed window: the map zero-extended by 10 on every side, filtered."""
    pad = [(0, 0)] * (v.ndim - 2) + [(TAPS - 1, TAPS - 1)] * 2
    return blur(np.pad(v, pad), dtype)


def moments(x, y, data_range=1.0, dtype=np.float64):
    """-> dict of the per-position maps [M, h - 10, w - 10]."""
    x, y = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    c1, c2 = (dtype(c) for c in constants(data_range))
    two = dtype(2.0)
    mx, my = blur(x, dtype), blur(y, dtype)
    sxx, syy, sxy = blur(x * x, dtype) - mx * mx, blur(y * y, dtype) - my * my, blur(x * y, dtype) - mx * my
    d2, d1 = sxx + syy + c2, mx * mx + my * my + c1
    cs, lum = (two * sxy + c2) / d2, (two * mx * my + c1) / d1
    return dict(mx=mx, my=my, d1=d1, d2=d2, cs=cs, l=lum, ssim=cs * lum)


def halve(v, dtype=np.float64):
    v = np.asarray(v).astype(dtype)
    h, w = v.shape[-2] // 2 * 2, v.shape[-1] // 2 * 2
    v = v[..., :h, :w]
    return (dtype(0.25) * ((v[..., 0::2, 0::2] + v[..., 0::2, 1::2]) + (v[..., 1::2, 0::2] + v[..., 1::2, 1::2]))).astype(dtype)


def scale(x, y, data_range=1.0, dtype=np.float64):
    """One scale of ``x, y [M, h, w]`` -> float64 (mean cs [M], mean ssim [M], mean |x - y| [M]) and the halved planes."""
    m = moments(x, y, data_range, dtype)
    xd, yd = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype)
    return (m["cs"].astype(np.float64).mean(axis=(1, 2)), m["ssim"].astype(np.float64).mean(axis=(1, 2)),
            np.abs(xd - yd).astype(np.float64).mean(axis=(1, 2)), halve(xd, dtype), halve(yd, dtype))


def scale_backward(x, y, g, g_half=None, data_range=1.0, dtype=np.float64):
    """The gradient with respect to ``x`` of ``sum_m g[m, 0] mean cs + g[m, 1] mean ssim + g[m, 2] mean |x - y|`` (+ ``g_half``
    arriving through the halved plane)."""
    x, y, g = np.asarray(x).astype(dtype), np.asarray(y).astype(dtype), np.asarray(g).astype(dtype)
    M, h, w = x.shape
    m = moments(x, y, data_range, dtype)
    n, two = dtype((h - 10) * (w - 10)), dtype(2.0)
    gcs, gss, gl1 = (g[:, 0] / n)[:, None, None], (g[:, 1] / n)[:, None, None], (g[:, 2] / dtype(h * w))[:, None, None]
    a, b = gcs + gss * m["l"], gss * m["cs"]
    A = a * (two * m["mx"] * m["cs"] - two * m["my"]) / m["d2"] + b * (two * m["my"] - two * m["mx"] * m["l"]) / m["d1"]
    B = -a * m["cs"] / m["d2"]
    C = two * a / m["d2"]
    grad = blur_t(A, dtype) + two * x * blur_t(B, dtype) + y * blur_t(C, dtype) + gl1 * np.sign(x - y)
    if g_half is not None:
        gh = np.asarray(g_half).astype(dtype)
        grad[:, :2 * (h // 2), :2 * (w // 2)] += dtype(0.25) * np.repeat(np.repeat(gh, 2, axis=1), 2, axis=2)
    return grad.astype(dtype)


def ms_ssim(x, y, n_levels=None, data_range=1.0):
    """float64: ``x, y [N, P, H, W]`` -> (score [N], mean |x - y| [N], the factors before the clamp [N P, L])."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N, P, H, W = x.shape
    L = levels(H, W) if n_levels is None else n_levels
    w = np.array(WEIGHTS[:L]) / np.sum(WEIGHTS[:L])
    xs, ys = x.reshape(N * P, H, W), y.reshape(N * P, H, W)
    factors, l1 = [], None
    for j in range(L):
        cs, ss, l1_j, xh, yh = scale(xs, ys, data_range)
        l1 = l1_j if j == 0 else l1
        factors.append(ss if j == L - 1 else cs)
        xs, ys = xh, yh
    factors = np.stack(factors, axis=1)
    score = np.prod(np.maximum(factors, 0.0) ** w[None], axis=1)
    return score.reshape(N, P).mean(axis=1), l1.reshape(N, P).mean(axis=1), factors


def ms_ssim_backward(x, y, data_range=1.0, dtype=np.float64):
    """The gradient of ``sum_n ms_ssim(x, y)[n]`` with respect to ``x [N, P, H, W]`` for planes none of whose factors is clamped:
    the scales' means and their closed-form gradients in ``dtype``, chained through the halvings; the few values of the
    combination (d score / d factor_j = w_j score / factor_j, over P) in float64."""
    x, y = np.asarray(x), np.asarray(y)
    N, P, H, W = x.shape
    L = levels(H, W)
    w = np.array(WEIGHTS[:L]) / np.sum(WEIGHTS[:L])
    xs, ys = [x.reshape(N * P, H, W).astype(dtype)], [y.reshape(N * P, H, W).astype(dtype)]
    for _ in range(L - 1):
        xs.append(halve(xs[-1], dtype))
        ys.append(halve(ys[-1], dtype))
    factors = np.stack([scale(xs[j], ys[j], data_range, dtype)[1 if j == L - 1 else 0] for j in range(L)], axis=1)
    assert (factors > 0).all()
    d_factor = w[None] * np.prod(factors ** w[None], axis=1, keepdims=True) / factors / P
    below = None
    for j in reversed(range(L)):
        g = np.zeros((N * P, 3))
        g[:, 1 if j == L - 1 else 0] = d_factor[:, j]
        below = scale_backward(xs[j], ys[j], g, below, data_range, dtype)
    return below.reshape(N, P, H, W)


# ------------------------------------------------------------------------------------------------------------------ bounds
FACTOR = 4.0


def mean_bounds(x, y, data_range=1.0):
    """Per plane, what a kernel's mean cs and mean ssim may differ from the float64 statement by (module docstring)."""
    lo, hi = moments(x, y, data_range, np.float32), moments(x, y, data_range, np.float64)
    out = []
    for key in ("cs", "ssim"):
        err = np.abs(lo[key].astype(np.float64) - hi[key]).mean(axis=(1, 2))
        out.append(FACTOR * err + 8.0 * U * np.maximum(np.abs(hi[key]).mean(axis=(1, 2)), 1e-3))
    return out[0], out[1]


def l1_bound(x, y):
    return U * np.abs(np.asarray(x, np.float64) - np.asarray(y, np.float64)).mean(axis=(1, 2)) * (1.0 + 1e-6) + 1e-300


def half_bound(v):
    v = np.abs(np.asarray(v, np.float64))
    h, w = v.shape[-2] // 2 * 2, v.shape[-1] // 2 * 2
    v = v[..., :h, :w]
    return 3.0 * U * (1.0 + 3.0 * U) * 0.25 * (v[..., 0::2, 0::2] + v[..., 0::2, 1::2] + v[..., 1::2, 0::2] + v[..., 1::2, 1::2])


def grad_bound(x, y, g, g_half=None, data_range=1.0):
    """Per plane [M, 1, 1]: what a kernel's grad_x element may differ from the float64 statement by."""
    lo = scale_backward(x, y, g, g_half, data_range, np.float32).astype(np.float64)
    hi = scale_backward(x, y, g, g_half, data_range, np.float64)
    err = np.abs(lo - hi).max(axis=(1, 2), keepdims=True)
    return FACTOR * err + 8.0 * U * np.abs(hi).max(axis=(1, 2), keepdims=True)


def parity_pair(shape, seed):
    """The pairs every parity test uses: x uniform in [0, 1], y = clamp(x + 0.05 randn, 0, 1), float32 -- all means >= 0.9."""
    rng = np.random.default_rng(seed)
    x = rng.random(shape, dtype=np.float32)
    y = np.clip(x + np.float32(0.05) * rng.standard_normal(shape, dtype=np.float32), 0.0, 1.0).astype(np.float32)
    return x, y
