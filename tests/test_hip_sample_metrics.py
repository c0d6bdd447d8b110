"""msg_feature_knn / msg_feature_ball_hits / msg_poly_mmd (csrc/feature_pairs.hip) and the sample-based metrics built on them,
on the GPU, against the float64 statement of tests/sample_metrics_util.py: every K-step, tile and sweep-slice edge of the kernel,
both load paths, index lists, the refusals, run-to-run identity, then validation_metrics' functions and classes on the device.

Tolerances are derived in sample_metrics_util's docstring from the arithmetic, not from what the kernels give.  Counts are held to
the interval the distance bound leaves open, and every case first shows ON THE REFERENCE ALONE that this interval is a point for
at least 95 % of its rows, so that the interval test cannot pass everything."""
import numpy as np
import pytest
import torch

import sample_metrics_util as su
from test_hip_metric_input import DEV, Region

pytestmark = pytest.mark.gpu
K, T = 32, 128                           # FP_K, FP_T of csrc/feature_pairs.hip: the staged contraction step, the tile of rows
EINVAL = -1
AMBIGUOUS_CAP = 0.05

# (nq, nr, d, shift): d over {1, 7, K - 1, K, K + 1, 130} (+ 2 K on the 16-byte path), rows over {1, 2, T - 1, T, T + 1, 2 T + 1};
# nr <= T sweeps in one slice, nr > T in several, and the last case (more than 512 pairs of tiles) gives every slice two tiles
CASES = [(1, 2, 1, 0.0), (2, 1, 7, 0.5), (T - 1, T, K - 1, 0.0), (T, T + 1, K, 0.5), (T + 1, T - 1, K + 1, 3.0),
         (2 * T + 1, 2 * T + 1, 130, 0.5), (T + 1, 257, 130, 0.0), (2, 2 * T + 1, K + 1, 3.0), (T + 2, T + 3, 2 * K, 0.0),
         (33 * T + 1, 17 * T + 1, 7, 0.5)]
IDS = [f"{c[0]}x{c[1]}x{c[2]}" for c in CASES]


def _lib():
    from multi_stylegan_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def inputs(case):
    """The case's two clouds; a case marked "swapped" is its original with the two clouds exchanged."""
    if case[-1] == "swapped":
        return inputs((case[1], case[0]) + case[2:-1])[::-1]
    return cached(("in", case), lambda: su.clouds(case[0], case[1], case[2], case[3], seed=sum(case[:3])))


def pairs(case):
    """(float64 squared distances, their fp32 bound) of the case's two clouds."""
    return cached(("pairs", case), lambda: (su.dist2(*inputs(case)), su.dist2_bound(*inputs(case))))


def own(case):
    """The same for the case's second cloud against itself."""
    r = inputs(case)[1]
    return cached(("own", case), lambda: (su.dist2(r, r), su.dist2_bound(r, r)))


def shifts(d):
    """Byte offsets of the operands: 16-byte aligned rows with d % 4 == 0 take the vector loads, everything else the scalar ones."""
    return (0, 4) if d % 4 == 0 else (4,) if d % 2 else (0,)


def call_knn(q, r, k, exclude_self, shift=0, ws_fill=0xFF, null=(), nq=None, nr=None, d=None):
    """The raw entry on guarded memory -> (status, fp32 [nq] on the host | None).  ``r is None``: the set IS the query set (one
    pointer).  The output is pre-filled with NaN bytes: an accepted call leaves none, a refused one leaves all of them."""
    lib = _lib().lib()
    rq = Region.of(torch.from_numpy(q), shift)
    rr = rq if r is None else Region.of(torch.from_numpy(r), shift)
    r = q if r is None else r
    nq, nr, d = q.shape[0] if nq is None else nq, r.shape[0] if nr is None else nr, q.shape[1] if d is None else d
    out = Region(4 * q.shape[0], shift)
    nbytes = lib.msg_feature_knn_workspace(nq, nr, d, k, exclude_self)
    ws = Region(max(nbytes, 0) + 8, 0, ws_fill)
    status = lib.msg_feature_knn(None if "q" in null else rq.ptr, nq, None if "r" in null else rr.ptr, nr, d, k, exclude_self,
                                 None if "out" in null else out.ptr, None if "ws" in null else ws.ptr, _stream())
    rq.bytes(), rr.bytes(), ws.bytes()
    if status != 0:
        assert nbytes == -1 or null or exclude_self, "the workspace query accepts what the entry refuses"
        assert bool((out.bytes() == 0xFF).all()), "a refused call wrote to its output"
        return status, None
    got = out.values(torch.float32, (q.shape[0],))
    assert not bool(got.isnan().any()), "an output element was not written"
    return status, got.numpy()


def call_ball(q, r, radius2, shift=0, ws_fill=0xFF, null=(), sizes=None):
    lib = _lib().lib()
    rq, rr, rad = Region.of(torch.from_numpy(q), shift), Region.of(torch.from_numpy(r), shift), Region.of(torch.from_numpy(radius2), shift)
    nq, nr, d = (q.shape[0], r.shape[0], q.shape[1]) if sizes is None else sizes
    margin, count = Region(4 * q.shape[0], shift), Region(4 * q.shape[0], shift)
    nbytes = lib.msg_feature_ball_hits_workspace(nq, nr, d)
    ws = Region(max(nbytes, 0) + 8, 0, ws_fill)
    status = lib.msg_feature_ball_hits(None if "q" in null else rq.ptr, nq, None if "r" in null else rr.ptr, nr, d,
                                       None if "radius2" in null else rad.ptr, None if "margin" in null else margin.ptr,
                                       None if "count" in null else count.ptr, None if "ws" in null else ws.ptr, _stream())
    rq.bytes(), rr.bytes(), rad.bytes(), ws.bytes()
    if status != 0:
        assert bool((margin.bytes() == 0xFF).all()) and bool((count.bytes() == 0xFF).all()), "a refused call wrote to an output"
        return status, None, None
    m = None if "margin" in null else margin.values(torch.float32, (q.shape[0],)).numpy()
    c = None if "count" in null else count.values(torch.int32, (q.shape[0],)).numpy()
    if "margin" in null:
        assert bool((margin.bytes() == 0xFF).all())
    if "count" in null:
        assert bool((count.bytes() == 0xFF).all())
    assert m is None or not np.isnan(m).any(), "a margin was not written"
    return status, m, c


def call_mmd(x, y, ix, iy, gamma, coef0, shift=0, ws_fill=0xFF, null=(), S=None, mx=None, my=None, sizes=None):
    lib = _lib().lib()
    rx, ry = Region.of(torch.from_numpy(x), shift), Region.of(torch.from_numpy(y), shift)
    lx = None if ix is None else Region.of(torch.from_numpy(np.ascontiguousarray(ix, dtype=np.int32)), shift)
    ly = None if iy is None else Region.of(torch.from_numpy(np.ascontiguousarray(iy, dtype=np.int32)), shift)
    S = (1 if ix is None and iy is None else len(ix if ix is not None else iy)) if S is None else S
    mx = (x.shape[0] if ix is None else np.shape(ix)[1]) if mx is None else mx
    my = (y.shape[0] if iy is None else np.shape(iy)[1]) if my is None else my
    nx, ny, d = (x.shape[0], y.shape[0], x.shape[1]) if sizes is None else sizes
    rows = max(S, 1)
    sums = Region(8 * 3 * rows, 0)
    nbytes = lib.msg_poly_mmd_workspace(nx, ny, d, S, mx, my)
    ws = Region(max(nbytes, 0) + 8, 0, ws_fill)
    status = lib.msg_poly_mmd(None if "x" in null else rx.ptr, nx, None if "y" in null else ry.ptr, ny, d,
                              None if lx is None else lx.ptr, None if ly is None else ly.ptr, S, mx, my, gamma, coef0,
                              None if "sums" in null else sums.ptr + (4 if "sums_misaligned" in null else 0),
                              None if "ws" in null else ws.ptr, _stream())
    rx.bytes(), ry.bytes(), ws.bytes()
    for region in (lx, ly):
        if region is not None:
            region.bytes()
    if status != 0:
        assert bool((sums.bytes() == 0xFF).all()), "a refused call wrote to its output"
        return status, None
    got = sums.values(torch.float64, (rows, 3)).numpy()
    assert not np.isnan(got).any(), "a sum was not written"
    return status, got


# ----------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_knn_at_every_step_tile_and_slice_edge(case):
    q, r = inputs(case)
    dist, bound = pairs(case)
    tol = bound.max(axis=1)
    order = np.sort(dist, axis=1)
    worst = 0.0
    for k in (1, 3, 8):
        if k > r.shape[0]:
            assert call_knn(q, r, k, 0)[0] == EINVAL
            continue
        results = [call_knn(q, r, k, 0, shift, fill) for shift in shifts(case[2]) for fill in (0xFF, 0x00)]
        assert all(status == 0 for status, _ in results)
        got = results[0][1]
        assert all(g.tobytes() == got.tobytes() for _, g in results[1:]), "the result depends on the run, the workspace or the load path"
        err = np.abs(got.astype(np.float64) - order[:, k - 1])
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (case, k, float((err / tol).max()))
    # the set against itself, row i skipped by index
    own_dist, own_bound = own(case)
    n = r.shape[0]
    if n >= 2:
        rest = np.sort(own_dist[~np.eye(n, dtype=bool)].reshape(n, n - 1), axis=1)
        for k in (1, 3, 8):
            if k > n - 1:
                assert call_knn(r, None, k, 1)[0] == EINVAL
                continue
            status, got = call_knn(r, None, k, 1, shifts(case[2])[-1])
            assert status == 0
            err = np.abs(got.astype(np.float64) - rest[:, k - 1])
            worst = max(worst, float((err / own_bound.max(axis=1)).max()))
            assert (err <= own_bound.max(axis=1)).all(), (case, k, "exclude_self")
    print(f"knn {case}: worst error / bound = {worst:.3f}")


def _radii(case):
    """fp32 radii for the case's second cloud: its rows' 3rd neighbours within the cloud (fewer than 4 rows: the median distance
    between the two clouds)."""
    r = inputs(case)[1]
    if r.shape[0] >= 4:
        return su.knn(r, r, 3, True).astype(np.float32)
    return np.full(r.shape[0], np.median(pairs(case)[0]), dtype=np.float32)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ball_hits_at_every_step_tile_and_slice_edge(case):
    """Both ways round: the second cloud's balls against the first cloud's rows, then (the case's sizes swapped) the first cloud's
    balls against the second's rows -- in many dimensions only the wider cloud's balls are ever hit."""
    hits = 0
    for way in (case, (case[1], case[0]) + case[2:] + ("swapped",)):
        q, r = inputs(way)
        radius2 = _radii(way)
        want = cached(("ball", way), lambda: su.ball_hits(q, r, radius2))
        share = float(want["ambiguous"].mean())
        print(f"ball_hits {way}: {100 * share:.2f} % of rows have an open count interval")
        assert share <= AMBIGUOUS_CAP, "the inputs leave the count test vacuous"
        results = [call_ball(q, r, radius2, shift, fill) for shift in shifts(case[2]) for fill in (0xFF, 0x00)]
        assert all(status == 0 for status, _m, _c in results)
        _, margin, count = results[0]
        assert all(m.tobytes() == margin.tobytes() and c.tobytes() == count.tobytes() for _, m, c in results[1:])
        err = np.abs(margin.astype(np.float64) - want["margin"])
        print(f"ball_hits {way}: worst margin error / bound = {float((err / want['margin_tol']).max()):.3f}; {int(want['count'].sum())} "
              f"hits, {int((count != want['count']).sum())} counts differ from the float64 count")
        assert (err <= want["margin_tol"]).all()
        assert ((want["count_lo"] <= count) & (count <= want["count_hi"])).all()
        hits += int(want["count"].sum())
    assert hits > 0 or case[3] == 3.0                                         # (balls are hit unless the clouds are far apart)


def test_ball_hits_outputs_are_optional_one_at_a_time():
    case = CASES[3]
    q, r = inputs(case)
    radius2 = _radii(case)
    _, margin, count = call_ball(q, r, radius2)
    status, m_only, none = call_ball(q, r, radius2, null=("count",))
    assert status == 0 and none is None and m_only.tobytes() == margin.tobytes()
    status, none, c_only = call_ball(q, r, radius2, null=("margin",))
    assert status == 0 and none is None and c_only.tobytes() == count.tobytes()
    assert call_ball(q, r, radius2, null=("margin", "count"))[0] == EINVAL


def _lists(n, m, S, seed):
    """Index lists with a reversal, repeats and a random draw."""
    rng = np.random.default_rng(seed)
    rows = [np.arange(n)[::-1][:m] if n >= m else np.resize(np.arange(n)[::-1], m), np.repeat(rng.integers(0, n, (m + 2) // 3), 3)[:m],
            rng.integers(0, n, m)]
    return np.stack(rows[:S]).astype(np.int32)


# (nx, ny, d, S, mx | None, my | None, shift)
MMD_CASES = [(2, 1, 1, 1, None, None, 0.0), (T + 1, T - 1, K + 1, 1, None, None, 0.5), (2 * T + 1, T, 130, 1, None, None, 0.0),
             (200, 150, K - 1, 3, T + 1, 70, 0.5), (150, 200, K, 3, 2 * T + 1, T - 1, 3.0), (90, 300, 2 * K, 1, None, T, 0.0),
             (40, 30, 7, 3, 1, 2, 0.5)]


@pytest.mark.parametrize("case", MMD_CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}-S{c[3]}" for c in MMD_CASES])
def test_poly_mmd_sums(case):
    nx, ny, d, S, mx, my, shift = case
    x, y = su.clouds(nx, ny, d, shift, seed=nx + ny + d)
    ix = None if mx is None else _lists(nx, mx, S, 1)
    iy = None if my is None else _lists(ny, my, S, 2)
    gamma, coef0 = 1.0 / d, 1.0
    want, bound = su.poly_sums(x, y, ix, iy, gamma, coef0)
    results = [call_mmd(x, y, ix, iy, gamma, coef0, sh, fill) for sh in shifts(d) for fill in (0xFF, 0x00)]
    assert all(status == 0 for status, _ in results)
    got = results[0][1]
    assert all(g.tobytes() == got.tobytes() for _, g in results[1:]), "the sums depend on the run, the workspace or the load path"
    err = np.abs(got - want)
    ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
    print(f"poly_mmd {case}: worst error / bound = {float(ratio.max()):.3f}")
    assert (err <= bound).all(), (case, err, bound)
    assert (np.abs(want) > 0).any()


def test_refused_calls_write_nothing():
    lib = _lib().lib()
    q, r = inputs(CASES[3])
    nq, nr, d = q.shape[0], r.shape[0], q.shape[1]
    for null in (("q",), ("r",), ("out",), ("ws",)):
        assert call_knn(q, r, 3, 0, null=null)[0] == EINVAL
    for bad in (dict(nq=0), dict(nr=0), dict(d=0), dict(nq=-1)):
        assert call_knn(q, r, 3, 0, **bad)[0] == EINVAL
    assert call_knn(q, r, 0, 0)[0] == EINVAL and call_knn(q, r, 9, 0)[0] == EINVAL
    assert call_knn(q, r, 3, 1)[0] == EINVAL                                  # exclude_self with two different sets
    assert call_knn(q, q.copy(), 3, 1)[0] == EINVAL                           # ... and with a copy: the sets must be one pointer
    assert call_knn(q[:3], None, 3, 1)[0] == EINVAL and call_knn(q[:4], None, 3, 1)[0] == 0     # k rows besides the row itself
    assert lib.msg_feature_knn_workspace(nq, nr, d, 9, 0) == -1 and lib.msg_feature_knn_workspace(3, 3, d, 3, 1) == -1
    assert lib.msg_feature_knn_workspace(nq, nr, d, 3, 0) > 0
    radius2 = _radii(CASES[3])
    for null in (("q",), ("r",), ("radius2",), ("ws",)):
        assert call_ball(q, r, radius2, null=null)[0] == EINVAL
    for sizes in ((0, nr, d), (nq, 0, d), (nq, nr, 0)):
        assert call_ball(q, r, radius2, sizes=sizes)[0] == EINVAL
        assert lib.msg_feature_ball_hits_workspace(*sizes) == -1
    ix, iy = _lists(nq, 20, 2, 1), _lists(nr, 30, 2, 2)
    for null in (("x",), ("y",), ("sums",), ("ws",), ("sums_misaligned",)):
        assert call_mmd(q, r, ix, iy, 1.0, 1.0, null=null)[0] == EINVAL
    assert call_mmd(q, r, None, iy, 1.0, 1.0, S=2, mx=20)[0] == EINVAL       # no list: every row, m = n
    assert call_mmd(q, r, ix, iy, 1.0, 1.0, S=0)[0] == EINVAL and call_mmd(q, r, ix, iy, 1.0, 1.0, mx=0)[0] == EINVAL
    assert call_mmd(q, r, ix, iy, 1.0, 1.0, sizes=(nq, nr, 0))[0] == EINVAL
    assert lib.msg_poly_mmd_workspace(nq, nr, d, 21846, 20, 30) == -1 and lib.msg_poly_mmd_workspace(nq, nr, d, 2, 20, 30) > 0
    # an index outside its set reads as a row of zeros (k = coef0^3 against everything), never out of bounds
    bad = ix.copy()
    bad[0, 3], bad[1, 5] = nq, -1
    zeroed = np.concatenate([q, np.zeros((1, d), dtype=np.float32)])
    status, got = call_mmd(q, r, bad, iy, 1.0 / d, 1.0)
    patched = np.where((bad < 0) | (bad >= nq), nq, bad)
    status2, want = call_mmd(zeroed, r, patched, iy, 1.0 / d, 1.0)
    assert status == 0 and status2 == 0 and got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------------------ python layer
def _vm():
    from multi_stylegan_amd import validation_metrics as vm
    return vm


@pytest.mark.parametrize("offset,d", [(0.0, 130), (2.0, 130), (2.0, 7)])
def test_manifold_scores_on_the_device(offset, d):
    """Uncentred clouds (offset 2) leave a fifth of the count intervals open at the kernel level; manifold_scores centres both
    sets first, which must bring the share back under the cap -- shown on the rows the kernels receive."""
    vm = _vm()
    real, fake = su.clouds(257, T + 1, d, 0.5, seed=5, offset=offset)
    x, y = torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV)
    centre = x.mean(dim=0, keepdim=True)
    xc, yc = (x - centre).cpu().numpy(), (y - centre).cpu().numpy()
    for k in (3, 5):
        want = cached(("manifold", offset, d, k), lambda: su.manifold(xc, yc, k))
        assert want["ambiguous_share"] <= AMBIGUOUS_CAP
        got = vm.manifold_scores(x, y, k=k)
        assert got == vm.manifold_scores(x, y, k=k)
        print(f"manifold offset {offset} k {k}: {got}; open intervals {100 * want['ambiguous_share']:.2f} % of rows; "
              f"raw rows: {100 * su.manifold(real, fake, k)['ambiguous_share']:.2f} %")
        for field in got._fields:
            assert abs(getattr(got, field) - want[field]) <= want["slack"][field] + 1e-12, (field, got, want)
        host = vm.manifold_scores(torch.from_numpy(real), torch.from_numpy(fake), k=k)
        for field in got._fields:
            assert abs(getattr(host, field) - want[field]) <= want["slack"][field] + 1e-12
    assert d > 7 or (0.0 < got.precision < 1.0 and 0.0 < got.recall < 1.0)   # (in 130 dimensions the narrower cloud has recall 0)
    with pytest.raises(ValueError, match="at most 8"):
        vm.manifold_scores(x, y, k=9)


def test_kernel_distance_on_the_device():
    vm = _vm()
    real, fake = su.clouds(300, 2 * T + 1, 130, 0.5, seed=9)
    x, y = torch.from_numpy(real).to(DEV), torch.from_numpy(fake).to(DEV)
    sums, bound = su.poly_sums(real, fake, None, None, 1.0 / 130, 1.0)
    got = vm.kernel_distance(x, y)
    assert got == vm.kernel_distance(x, y)
    assert abs(got - su.mmd2(sums, 300, 257)) <= su.mmd2_bound(bound, 300, 257)
    assert got > 10 * su.mmd2_bound(bound, 300, 257)                          # (the two clouds differ: the estimate is resolved)
    got = vm.kernel_distance(x, y, subsets=3, subset_size=T + 1, generator=torch.Generator().manual_seed(4))
    gen = torch.Generator().manual_seed(4)
    ix, iy = vm.subset_indices(300, T + 1, 3, gen).numpy(), vm.subset_indices(257, T + 1, 3, gen).numpy()
    sums, bound = su.poly_sums(real, fake, ix, iy, 1.0 / 130, 1.0)
    assert abs(got - su.mmd2(sums, T + 1, T + 1)) <= su.mmd2_bound(bound, T + 1, T + 1)
    with pytest.raises(ValueError, match="outside"):
        vm._poly_sums(x, y, torch.tensor([[0, 300]]), None, 1.0, 1.0, True)


def test_metric_classes_on_the_device():
    """KID and PrecisionRecall end to end on the GPU: device-side metric inputs, a toy feature network, the kernels; the score is
    the free function's on the rows the network produced."""
    from test_host import _ToyFeatures, _ToyGenerator
    vm = _vm()
    torch.manual_seed(3)
    gen = _ToyGenerator().to(DEV)
    dataset = [torch.rand(4, 2, 3, 8, 8) for _ in range(5)]
    for cls, score in ((vm.KID, vm.kernel_distance), (vm.KVD, vm.kernel_distance), (vm.PrecisionRecall, vm.manifold_scores)):
        net = _ToyFeatures()
        metric = cls(net, device=DEV, batch_size=4, data_samples=16, no_rfp=True)
        got = metric(gen, dataset)
        assert len(got) == 2 and len(net.rows) == 16 and metric.rows_real[0].is_cuda
        for c in range(2):
            real = torch.cat(net.rows[c:8:2]).float()
            fake = torch.cat(net.rows[8 + c::2]).float()
            assert torch.equal(metric.rows_real[c], real)
            assert got[c] == score(real, fake)
