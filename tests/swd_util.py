"""An independent float64 statement of the sliced Wasserstein distance over Laplacian-pyramid patches (validation_metrics.py:
SWD / SWVD, csrc/swd.hip), and the error bounds the tests hold the kernels to.  The pyramid is scipy.ndimage.convolve with
mode="mirror"; everything else is numpy indexing, np.sort and means.  Nothing here imports the package.

Definition.  f = [1, 4, 6, 4, 1] / 16, F = f f^T; down(x) = (x * F) at even rows and columns; up(y) = (y on the even positions of
a zero array of twice the size) * 4 F; level l = G_l - up(G_(l+1)), G_(l+1) = down(G_l), the coarsest level G_L itself.  A
descriptor row is the 7 x 7 patch around (y, x) of every plane, plane-major.  A set is normalised per plane by the mean and the
population standard deviation of all of the plane's values, both rounded once to fp32 (mean, istd = 1 / std).  The score is
1000 mean_(i, theta) |a_(i) - b_(i)| of the sorted projections on unit directions theta.

Bounds, u = 2^-24 (fp32 unit roundoff).  None is taken from what a kernel returned.

* level_bounds -- include/msg_hip.h states the order of operations of msg_laplacian_level: separable; down per axis is
  fmaf(3/8, c, fmaf(1/4, b + d, (a + e) / 16)) with exact scalings, so a sample meets at most 3 roundings per axis (its pair's
  sum and two fmaf), 6 on the way to a coarse value; up per axis is fmaf(3/4, c, (l + r) / 8) or (c + r) / 2, at most 2
  roundings per axis; the subtraction is 1.  Every source sample x reaches an output through a product of its weights w (all
  non-negative except the final sign) and at most m roundings, so |error| <= m u sum |w x| over the taps: m = 6 for coarse, m =
  6 + 4 + 1 = 11 for lap, with sum |w x| = down(|x|) resp. |x| + up(down(|x|)).
* projection_bound -- x^ = (x - mean) istd is two fp32 roundings, the fmaf chain over d terms at most d more: (d + 2) u sum_j
  |x^_j dir_j| to first order, one more u for the higher-order terms: (d + 3) u sum_j |x^_j dir_j|, x^ in float64 from the same
  fp32 mean and istd.
* sorted L1 -- one fp32 subtraction per term (the float64 accumulation is below 1e-12 of it): 2^-23 sum |a - b|.
* plane sums -- float64 throughout: 1e-12 of sum |x| resp. sum x^2 covers n 49 <= 2^30 additions.
* end to end (score_bound) -- sorting is non-expansive: |W(a', b') - W(a, b)| <= mean |a' - a| + mean |b' - b| for sorted L1
  (mean |a'_(i) - a_(i)| <= mean |a'_i - a_i|).  So the score moves by at most 1000 x the mean of projection_bound over both
  sets, plus 1000 x 2^-23 W for the final subtraction.  One more term: mean and istd come from float64 sums formed in different
  orders on the device and here; when those differ in their last bits, an fp32-rounded mean or istd may land on the
  neighbouring fp32 value.  One ulp of mean_p is at most 2^-23 |mean_p| and moves x^_j (j in plane p) by 2^-23 |mean_p| istd_p,
  the projection by at most 2^-23 |mean_p| istd_p sum_(j in p) |dir_j|; one ulp of istd_p is at most 2^-23 istd_p and moves the
  projection by at most 2^-23 sum_(j in p) |x^_j dir_j|.  ulp_term is the mean over rows and directions of their sum."""
import numpy as np
import scipy.ndimage as ndi

U = 2.0 ** -24
F1 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
F2 = np.outer(F1, F1)
TAPS = 49


def _planes(x, fn):
    x = np.asarray(x, dtype=np.float64)
    flat = x.reshape((-1,) + x.shape[-2:])
    out = [fn(p) for p in flat]
    return np.stack(out).reshape(x.shape[:-2] + out[0].shape)


def down(x):
    return _planes(x, lambda p: ndi.convolve(p, F2, mode="mirror")[::2, ::2])


def up(y):
    def one(p):
        z = np.zeros((2 * p.shape[0], 2 * p.shape[1]))
        z[::2, ::2] = p
        return ndi.convolve(z, 4.0 * F2, mode="mirror")
    return _planes(y, one)


def level(fine):
    """(coarse, lap) of one pyramid step, float64."""
    coarse = down(fine)
    return coarse, np.asarray(fine, dtype=np.float64) - up(coarse)


def level_bounds(fine):
    """(coarse bound, lap bound) per element: m u sum |w x| with m = 6 and m = 11 (module docstring)."""
    mag = np.abs(np.asarray(fine, dtype=np.float64))
    coarse = down(mag)
    return 6 * U * coarse, 11 * U * (mag + up(coarse))


def pyramid(frames, min_size=16):
    g = np.asarray(frames, dtype=np.float64)
    h, w = g.shape[-2:]
    levels = 1
    while min(h, w) >> levels >= min_size:
        levels += 1
    assert h % (1 << (levels - 1)) == 0 and w % (1 << (levels - 1)) == 0
    out = []
    for _ in range(levels - 1):
        coarse, lap = level(g)
        out.append(lap)
        g = coarse
    return out + [g]


def descriptors(lvl, pos):
    """lvl [B, P, h, w], pos [B, K, 2] (y, x) -> [B K, P 49]; a tap outside the plane is zero.  The level's dtype is kept."""
    lvl, pos = np.asarray(lvl), np.asarray(pos)
    B, P, h, w = lvl.shape
    K = pos.shape[1]
    rows = np.zeros((B * K, P * TAPS), dtype=lvl.dtype)
    for b in range(B):
        for k in range(K):
            cy, cx = int(pos[b, k, 0]), int(pos[b, k, 1])
            for p in range(P):
                for dy in range(7):
                    for dx in range(7):
                        y, x = cy - 3 + dy, cx - 3 + dx
                        if 0 <= y < h and 0 <= x < w:
                            rows[b * K + k, p * TAPS + dy * 7 + dx] = lvl[b, p, y, x]
    return rows


def gather(lvl, pos):
    """``descriptors`` for the larger test sets (all taps inside the plane): slices instead of the five loops."""
    lvl, pos = np.asarray(lvl), np.asarray(pos)
    B, P, h, w = lvl.shape
    K = pos.shape[1]
    rows = np.empty((B * K, P * TAPS), dtype=lvl.dtype)
    for b in range(B):
        for k in range(K):
            cy, cx = int(pos[b, k, 0]), int(pos[b, k, 1])
            rows[b * K + k] = lvl[b, :, cy - 3:cy + 4, cx - 3:cx + 4].reshape(-1)
    return rows


def plane_stats(rows, planes):
    """fp32 (mean [P], istd [P]) of the set: np.mean and np.std (population) over all values of a plane, rounded once."""
    x = np.asarray(rows, dtype=np.float64).reshape(rows.shape[0], planes, TAPS)
    std = np.where(x.min(axis=(0, 2)) == x.max(axis=(0, 2)), 0.0, x.std(axis=(0, 2)))      # (a constant plane: exactly 0)
    with np.errstate(divide="ignore"):
        return x.mean(axis=(0, 2)).astype(np.float32), (1.0 / std).astype(np.float32)


def normalised(rows, planes, mean, istd):
    """x^ in float64 from the fp32 mean and istd."""
    x = np.asarray(rows, dtype=np.float64).reshape(rows.shape[0], planes, TAPS)
    hat = (x - np.asarray(mean, dtype=np.float64)[None, :, None]) * np.asarray(istd, dtype=np.float64)[None, :, None]
    return hat.reshape(rows.shape[0], planes * TAPS)


def unit_stats(planes):
    return np.zeros(planes, dtype=np.float32), np.ones(planes, dtype=np.float32)


def swd(a_rows, b_rows, planes, dirs, normalize=True):
    """dirs [repeats, d, directions] (the package's ``swd_directions``).  1000 x the mean of |a_(i) - b_(i)|."""
    assert a_rows.shape == b_rows.shape
    dirs = np.asarray(dirs, dtype=np.float64)
    hats = []
    for rows in (a_rows, b_rows):
        mean, istd = plane_stats(rows, planes) if normalize else unit_stats(planes)
        if not np.isfinite(istd).all():
            return float("nan")
        hats.append(normalised(rows, planes, mean, istd))
    total = 0.0
    for rep in range(dirs.shape[0]):
        pa, pb = (np.sort(hat @ dirs[rep], axis=0) for hat in hats)
        total += np.abs(pa - pb).mean()
    return 1000.0 * total / dirs.shape[0]


def projection_bound(rows, planes, mean, istd, dirs2):
    """[n, R]: (d + 3) u sum_j |x^_j dir_j| for dirs2 [d, R]."""
    hat = np.abs(normalised(rows, planes, mean, istd))
    return (hat.shape[1] + 3) * U * (hat @ np.abs(np.asarray(dirs2, dtype=np.float64)))


def ulp_term(rows, planes, mean, istd, dirs2):
    """Mean over rows and directions of what one fp32 ulp of every mean_p and istd_p moves a projection by (module docstring)."""
    d2 = np.abs(np.asarray(dirs2, dtype=np.float64))
    hat = np.abs(normalised(rows, planes, mean, istd))
    by_istd = (hat @ d2).mean()
    per_plane = d2.reshape(planes, TAPS, -1).sum(axis=1)                       # [P, R]
    by_mean = (np.abs(np.asarray(mean, dtype=np.float64)) * np.asarray(istd, dtype=np.float64))[:, None] * per_plane
    return 2.0 ** -23 * (by_istd + by_mean.sum(axis=0).mean())


def score_bound(a_rows, b_rows, planes, dirs, score, normalize=True):
    """What a fp32 evaluation of ``swd`` may differ by from the float64 statement ``score`` (module docstring)."""
    dirs = np.asarray(dirs, dtype=np.float64)
    total = 0.0
    for rows in (a_rows, b_rows):
        mean, istd = plane_stats(rows, planes) if normalize else unit_stats(planes)
        for rep in range(dirs.shape[0]):
            total += projection_bound(rows, planes, mean, istd, dirs[rep]).mean()
            if normalize:
                total += ulp_term(rows, planes, mean, istd, dirs[rep])
    return 1000.0 * total / dirs.shape[0] + 2.0 ** -23 * abs(score)


def textures(seed, blur=0.0, n=64, planes=3, side=64):
    """``n`` random ``planes``-plane textures of ``side`` x ``side``: smoothed white noise cut at a threshold (blobs with hard edges)
    plus a little pixel noise; ``blur``: a Gaussian blur of that sigma on top."""
    rng = np.random.default_rng(seed)
    x = ndi.gaussian_filter(rng.standard_normal((n, planes, side, side)), (0, 0, 1.5, 1.5))
    x = (x > 0.1).astype(np.float64) + 0.05 * rng.standard_normal((n, planes, side, side))
    if blur:
        x = ndi.gaussian_filter(x, (0, 0, blur, blur))
    return x.astype(np.float32)
