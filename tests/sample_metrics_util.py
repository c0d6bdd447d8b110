"""The float64 numpy statement of the sample-based metrics (KID, manifold precision / recall / density / coverage) and of the
three pairwise feature kernels behind them, written from the definitions and independently of the package: distances are direct
sums of squared differences, radii come by sorting, counts and minima are broadcasts, the kernel sums are straight sums over
pairs.  Also the input makers and the error bounds the tests hold the fp32 kernels to.

Bounds.  u = 2^-24, gamma_d = d u / (1 - d u).
  * squared distance: E(a, b) = (2 gamma_d + 4 u) (|a|^2 + |b|^2) bounds the error of ANY fp32 evaluation of |a|^2 + |b|^2 - 2 a.b:
    three length-d product sums in any order (|a|^2, |b|^2, and 2 |a.b| <= |a|^2 + |b|^2 by Cauchy-Schwarz: gamma_d times
    2 (|a|^2 + |b|^2) in all), and the roundings of the combination (the sum of the norms, the fused product-subtract; clamping at
    zero only moves a value towards the true one).
  * a radius the kernels computed themselves, radius2[j] = k-th smallest of dist2(r_j, r_l), is off by at most
    E_radius[j] = max_l E(r_j, r_l) (an order statistic moves by no more than the largest move of an element); a margin
    dist2(q_i, r_j) - radius2[j] is held to E(q_i, r_j) + E_radius[j].  Where the radius is an exact input the second term covers
    the subtraction's own rounding u |margin| <= u (dist2 + radius2), which it exceeds.
  * polynomial kernel k = t^3, t = gamma x.y + c: the dot product is off by at most gamma_d sum_c |x_c y_c|, so t by
    tau = gamma_d gamma sum_c |x_c y_c|, and the cube by 3 (|t| + tau)^2 tau; forming t (a product and a sum, or one fused
    operation) and cubing it (two products) add at most 8 u |k|.  The float64 accumulation adds nothing at these sizes.
"""
import numpy as np

U = 2.0 ** -24


def gamma_d(d):
    return d * U / (1.0 - d * U)


# ------------------------------------------------------------------------------------------------------------------ inputs
def clouds(n, m, d, shift, seed, offset=0.0):
    """(q [n, d], r [m, d]) fp32: N(0, 1) rows against 0.8 N(0, 1) + shift; ``offset`` moves both (0: centred clouds)."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((n, d)) + offset
    r = 0.8 * rng.standard_normal((m, d)) + shift + offset
    return q.astype(np.float32), r.astype(np.float32)


# ------------------------------------------------------------------------------------------------------------- definitions
def dist2(q, r):
    """float64 [n, m]: sum_c (q_ic - r_jc)^2, a block of query rows at a time."""
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    step = max(1, (1 << 23) // max(1, r.shape[0] * r.shape[1]))
    return np.concatenate([((q[i:i + step, None, :] - r[None, :, :]) ** 2).sum(axis=2) for i in range(0, q.shape[0], step)])


def dist2_bound(q, r):
    """E(a, b) for every pair, float64 [n, m]."""
    q, r = np.asarray(q, dtype=np.float64), np.asarray(r, dtype=np.float64)
    return (2.0 * gamma_d(q.shape[1]) + 4.0 * U) * ((q * q).sum(axis=1)[:, None] + (r * r).sum(axis=1)[None, :])


def knn(q, r, k, exclude_self=False):
    """The k-th smallest squared distance of every query row, by sorting (``exclude_self``: the diagonal is left out by index)."""
    dist = dist2(q, r)
    if exclude_self:
        assert dist.shape[0] == dist.shape[1]
        dist = dist[~np.eye(dist.shape[0], dtype=bool)].reshape(dist.shape[0], dist.shape[0] - 1)
    return np.sort(dist, axis=1)[:, k - 1]


def radius_bound(r):
    """E_radius[j] = max_l E(r_j, r_l)."""
    return dist2_bound(r, r).max(axis=1)


def ball_hits(q, r, radius2, radius_err=None):
    """-> dict(margin [n], count [n], tol [n, m], count_lo [n], count_hi [n], margin_tol [n], ambiguous [n]): the statement
    margin_i = min_j (dist2_ij - radius2_j), count_i = #{j: dist2_ij <= radius2_j}, and the interval a count may lie in when
    every dist2_ij - radius2_j is only known within tol_ij = E_ij + E_radius_j."""
    radius2 = np.asarray(radius2, dtype=np.float64)
    diff = dist2(q, r) - radius2[None, :]
    tol = dist2_bound(q, r) + (radius_bound(r) if radius_err is None else radius_err)[None, :]
    lo, hi = (diff < -tol).sum(axis=1), (diff <= tol).sum(axis=1)
    return dict(margin=diff.min(axis=1), count=(diff <= 0).sum(axis=1), tol=tol, count_lo=lo, count_hi=hi,
                margin_tol=tol.max(axis=1), ambiguous=lo != hi)


def poly_sums(x, y, ix, iy, gamma, coef0):
    """-> (sums [S, 3], bound [S, 3]) float64: per subset sum_{a != b} k(x_a, x_b), sum_{a != b} k(y_a, y_b), sum_{a, b} k(x_a, y_b)
    over POSITIONS of the index lists (None: every row once), and the fp32 error bound of each sum."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    S = 1 if ix is None and iy is None else len(ix if ix is not None else iy)
    sums, bound = np.zeros((S, 3)), np.zeros((S, 3))
    g = gamma_d(x.shape[1])
    for s in range(S):
        xs = x if ix is None else x[np.asarray(ix[s])]
        ys = y if iy is None else y[np.asarray(iy[s])]
        for p, (a, b, off_diagonal) in enumerate(((xs, xs, True), (ys, ys, True), (xs, ys, False))):
            t = gamma * np.einsum("ac,bc->ab", a, b) + coef0
            tau = g * gamma * np.einsum("ac,bc->ab", np.abs(a), np.abs(b))
            k = t ** 3
            err = 3.0 * (np.abs(t) + tau) ** 2 * tau + 8.0 * U * np.abs(k)
            if off_diagonal:
                keep = ~np.eye(a.shape[0], dtype=bool)
                k, err = k[keep], err[keep]
            sums[s, p], bound[s, p] = k.sum(), err.sum()
    return sums, bound


def mmd2(sums, mx, my):
    per = sums[:, 0] / (mx * (mx - 1)) + sums[:, 1] / (my * (my - 1)) - 2.0 * sums[:, 2] / (mx * my)
    return float(per.mean())


def mmd2_bound(bound, mx, my):
    per = bound[:, 0] / (mx * (mx - 1)) + bound[:, 1] / (my * (my - 1)) + 2.0 * bound[:, 2] / (mx * my)
    return float(per.mean())


def kernel_distance(x, y, ix=None, iy=None):
    """The unbiased MMD^2 under k(u, v) = (u.v / d + 1)^3: over all rows, or the mean over the subsets the lists name."""
    mx = len(x) if ix is None else len(ix[0])
    my = len(y) if iy is None else len(iy[0])
    return mmd2(poly_sums(x, y, ix, iy, 1.0 / np.asarray(x).shape[1], 1.0)[0], mx, my)


def manifold(real, fake, k):
    """-> dict(precision, recall, density, coverage, slack): the four scores from the definitions on the rows as given (no
    centring: float64 sums of squared differences do not need it), and ``slack``, per score the share of rows whose decision
    an fp32 evaluation ON THESE ROWS could turn (for density: the largest change of the score)."""
    real, fake = np.asarray(real, dtype=np.float64), np.asarray(fake, dtype=np.float64)
    rad_r, rad_f = knn(real, real, k, True), knn(fake, fake, k, True)
    f_in_r, r_in_f = ball_hits(fake, real, rad_r), ball_hits(real, fake, rad_f)
    d_rf = dist2(real, fake)
    nearest = d_rf.min(axis=1)
    near_tol = dist2_bound(real, fake).max(axis=1) + radius_bound(real)
    scores = dict(precision=float((f_in_r["margin"] <= 0).mean()), recall=float((r_in_f["margin"] <= 0).mean()),
                  density=float(f_in_r["count"].sum() / (k * len(fake))), coverage=float((nearest <= rad_r).mean()))
    scores["slack"] = dict(precision=float((np.abs(f_in_r["margin"]) <= f_in_r["margin_tol"]).mean()),
                           recall=float((np.abs(r_in_f["margin"]) <= r_in_f["margin_tol"]).mean()),
                           density=float((f_in_r["count_hi"] - f_in_r["count_lo"]).sum() / (k * len(fake))),
                           coverage=float((np.abs(nearest - rad_r) <= near_tol).mean()))
    scores["ambiguous_share"] = float(max(f_in_r["ambiguous"].mean(), r_in_f["ambiguous"].mean()))
    return scores
