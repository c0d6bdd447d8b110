"""The structural-similarity kernels (csrc/ssim.hip) on the GPU: both raw entries on guarded memory against the float64
statement of tests/ssim_util.py at every tile edge and on both memory paths, their refusals and run-to-run bit identity; then
``ms_ssim`` on device tensors against the CPU float64 run (values and gradients) and the MSSSIM / MSSSIMVideo classes against
their CPU run.

Every bound comes from ssim_util (its docstring says how: derived where that is tractable, 4 x the measured error of the fp32
statement of the same definitions where it is not), none from what a kernel returned."""
import numpy as np
import pytest
import torch

import ssim_util as su
from test_hip_metric_input import DEV, Region
from test_ssim import StubGenerator, stub_dataset

pytestmark = pytest.mark.gpu
FWD_TH, FWD_TW = 16, 64                  # SF_TH, SF_TW of csrc/ssim.hip: pixels and window positions of one forward workgroup
BWD_TH, BWD_TW = 16, 32                  # SB_TH, SB_TW: the tile of grad_x of one backward workgroup
NAN_FILL = 0xFF
# one position; odd sizes; one and two pixels past each tile edge, in pixels (h, w) and in positions (h - 10, w - 10); sizes whose
# width is a multiple of four (the 16-byte path: 76, 44, 68 -- a vector that straddles the plane's edge included); several tiles
SIZES = [(11, 11), (12, 27), (13, 15), (FWD_TH + 1, FWD_TW + 1), (FWD_TH + 2, FWD_TW + 2), (BWD_TH + 1, BWD_TW + 1),
         (BWD_TH + 2, BWD_TW + 2), (FWD_TH + 11, FWD_TW + 12), (BWD_TH + 12, BWD_TW + 12), (20, 68), (66, 130)]
C1, C2 = su.constants()


def _L():
    from multi_stylegan_amd import _lib
    return _lib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _untouched(*regions):
    return all(bool((r.bytes() == NAN_FILL).all()) for r in regions)


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


_PAIRS = {}


def pair(M, size):
    """The parity pair of one case and its float64 reference, computed once and shared."""
    key = (M,) + tuple(size)
    if key not in _PAIRS:
        x, y = su.parity_pair(key, seed=1000 * M + 10 * size[0] + size[1])
        _PAIRS[key] = (x, y, su.scale(x, y), su.mean_bounds(x, y))
    return _PAIRS[key]


# ---------------------------------------------------------------------------------------------------------- msg_ssim_scale
def run_forward(x, y, halves=True, l1=True, shift=0, null=(), dims=None, sums_shift=0, one_half=False):
    """-> (status, sums [M, 2], l1 [M] or None, x_half, y_half or None) on the host.  A refused call leaves every output's fill
    bytes alone; an accepted one leaves no element unwritten (the fill is a NaN) and does not touch an output it was not given."""
    lib = _L().lib()
    x, y = torch.as_tensor(x), torch.as_tensor(y)
    m, h, w = x.shape
    M, hh, ww = dims or (m, h, w)
    sx, sy = Region.of(x, shift), Region.of(y, shift)
    sums, l1s = Region(m * 16, sums_shift), Region(m * 8)
    xh, yh = Region(max(m * (h // 2) * (w // 2), 1) * 4, shift), Region(max(m * (h // 2) * (w // 2), 1) * 4, shift)
    ws = Region(max(lib.msg_ssim_scale_workspace(m, h, w), 8))
    status = lib.msg_ssim_scale(None if "x" in null else sx.ptr, None if "y" in null else sy.ptr, M, hh, ww, C1, C2,
                                None if "sums" in null else sums.ptr, l1s.ptr if l1 else None, xh.ptr if halves else None,
                                yh.ptr if halves and not one_half else None, None if "ws" in null else ws.ptr, _stream())
    sx.bytes(), sy.bytes(), ws.bytes()
    if status != 0:
        assert _untouched(sums, l1s, xh, yh), "a refused call wrote to an output"
        return status, None, None, None, None
    out = [sums.values(torch.float64, (m, 2)), l1s.values(torch.float64, (m,)) if l1 else None,
           xh.values(torch.float32, (m, h // 2, w // 2)) if halves else None,
           yh.values(torch.float32, (m, h // 2, w // 2)) if halves else None]
    assert l1 or _untouched(l1s)
    assert halves or _untouched(xh, yh)
    assert not any(bool(o.isnan().any()) for o in out if o is not None), "an element was not written"
    return (status,) + tuple(out)


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("M", [1, 7])
def test_forward_against_the_float64_statement(M, size):
    x, y, (cs, ss, l1, xh, yh), (b_cs, b_ss) = pair(M, size)
    assert cs.min() >= 0.9 and ss.min() >= 0.9
    h, w = size
    status, sums, got_l1, got_xh, got_yh = run_forward(x, y)
    assert status == 0
    means = sums.numpy() / float((h - 10) * (w - 10))
    e_cs, e_ss, e_l1 = np.abs(means[:, 0] - cs), np.abs(means[:, 1] - ss), np.abs(got_l1.numpy() / float(h * w) - l1)
    print(f"{M} x {size}: cs {e_cs.max():.2e} of {b_cs.min():.2e}, ssim {e_ss.max():.2e} of {b_ss.min():.2e}, l1 {e_l1.max():.2e}")
    assert (e_cs <= b_cs).all() and (e_ss <= b_ss).all() and (e_l1 <= su.l1_bound(x, y)).all()
    assert (np.abs(got_xh.double().numpy() - xh) <= su.half_bound(x)).all()
    assert (np.abs(got_yh.double().numpy() - yh) <= su.half_bound(y)).all()
    # without the halved planes, without the L1 sum: the same bits in what remains
    status, only, none, *_ = run_forward(x, y, halves=False, l1=False)
    assert status == 0 and none is None and torch.equal(_bits(only), _bits(sums))
    # a second run, and off the 16-byte alignment (element by element): the same bits
    for shift in (0, 4):
        status, s2, l2, xh2, yh2 = run_forward(x, y, shift=shift)
        assert status == 0 and torch.equal(_bits(s2), _bits(sums)) and torch.equal(_bits(l2), _bits(got_l1))
        assert torch.equal(_bits(xh2), _bits(got_xh)) and torch.equal(_bits(yh2), _bits(got_yh))


def test_forward_on_equal_planes_and_on_a_flat_bright_plane():
    x, _ = su.parity_pair((2, 33, 70), seed=5)
    status, sums, l1, xh, yh = run_forward(x, x.copy())
    assert status == 0 and torch.equal(sums, torch.full((2, 2), 23.0 * 60.0, dtype=torch.float64))       # cs = l = 1 exactly
    assert torch.equal(l1, torch.zeros(2, dtype=torch.float64)) and torch.equal(xh, yh)
    # nearly flat and bright: s = g*x^2 - mu^2 cancels; the bound follows the fp32 statement's own error there
    rng = np.random.default_rng(6)
    a = (0.9 + 1e-3 * rng.random((2, 40, 70))).astype(np.float32)
    b = (0.9 + 1e-3 * rng.random((2, 40, 70))).astype(np.float32)
    status, sums, *_ = run_forward(a, b)
    cs, ss, *_ = su.scale(a, b)
    b_cs, b_ss = su.mean_bounds(a, b)
    means = sums.numpy() / float(30 * 60)
    print(f"flat: cs {np.abs(means[:, 0] - cs).max():.2e} of {b_cs.min():.2e}")
    assert status == 0 and (np.abs(means[:, 0] - cs) <= b_cs).all() and (np.abs(means[:, 1] - ss) <= b_ss).all()


def test_forward_refusals():
    einval = _L().MSG_EINVAL
    x, y = su.parity_pair((2, 12, 16), seed=1)
    assert run_forward(x, y)[0] == 0
    for name in ("x", "y", "sums", "ws"):
        assert run_forward(x, y, null=(name,))[0] == einval, name
    assert run_forward(x, y, dims=(2, 10, 16))[0] == einval and run_forward(x, y, dims=(2, 12, 10))[0] == einval
    assert run_forward(x, y, dims=(0, 12, 16))[0] == einval and run_forward(x, y, dims=(-2, 12, 16))[0] == einval
    assert run_forward(x, y, shift=2)[0] == einval                             # fp32 tensors off their 4-byte alignment
    assert run_forward(x, y, sums_shift=4)[0] == einval                        # the float64 sums off their 8-byte alignment
    assert run_forward(x, y, one_half=True)[0] == einval
    assert run_forward(x, y, dims=(1 << 20, 1024, 4096))[0] == einval          # 2^32 tiles
    assert _L().lib().msg_ssim_scale_workspace(1 << 20, 1024, 4096) == -1


# ------------------------------------------------------------------------------------------------- msg_ssim_scale_backward
def run_backward(x, y, g, g_half=None, shift=0, null=(), dims=None, g_shift=0):
    """-> (status, grad_x [M, h, w]) on the host; refused: no output byte touched; accepted: no element left unwritten."""
    lib = _L().lib()
    x, y, g = torch.as_tensor(x), torch.as_tensor(y), torch.as_tensor(g, dtype=torch.float32)
    m, h, w = x.shape
    M, hh, ww = dims or (m, h, w)
    sx, sy, sg = Region.of(x, shift), Region.of(y, shift), Region.of(g, g_shift)
    sh = None if g_half is None else Region.of(torch.as_tensor(g_half, dtype=torch.float32), shift)
    out = Region(m * h * w * 4, shift)
    status = lib.msg_ssim_scale_backward(None if "x" in null else sx.ptr, None if "y" in null else sy.ptr,
                                         None if "g" in null else sg.ptr, None if sh is None else sh.ptr, M, hh, ww, C1, C2,
                                         None if "grad_x" in null else out.ptr, _stream())
    sx.bytes(), sy.bytes(), sg.bytes()
    if status != 0:
        assert _untouched(out), "a refused call wrote to its output"
        return status, None
    grad = out.values(torch.float32, (m, h, w))
    assert not bool(grad.isnan().any()), "an element was not written"
    return status, grad


def _cotangents(M, size, seed):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((M, 3)).astype(np.float32)
    g_half = rng.standard_normal((M, size[0] // 2, size[1] // 2)).astype(np.float32) * np.float32(1e-3)
    return g, g_half


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("M", [1, 7])
def test_backward_against_the_float64_statement(M, size):
    x, y = pair(M, size)[:2]
    g, g_half = _cotangents(M, size, seed=M + size[1])
    for half in (None, g_half):
        want = su.scale_backward(x, y, g, half)
        bound = su.grad_bound(x, y, g, half)
        status, grad = run_backward(x, y, g, half)
        assert status == 0
        err = np.abs(grad.double().numpy() - want)
        print(f"{M} x {size}, g_half {half is not None}: {(err / bound).max():.3f} of the bound, |grad| <= {np.abs(want).max():.2e}")
        assert (err <= bound).all()
        for shift in (0, 4):                                                   # run to run, and element by element: the same bits
            status, again = run_backward(x, y, g, half, shift=shift)
            assert status == 0 and torch.equal(_bits(again), _bits(grad))
    # SSIM is symmetric: the arguments exchanged give the gradient with respect to y
    want = su.scale_backward(y, x, g)
    status, grad = run_backward(y, x, g)
    assert status == 0 and (np.abs(grad.double().numpy() - want) <= su.grad_bound(y, x, g)).all()


def test_backward_impulse_selects_one_plane_and_one_mean():
    x, y = pair(7, (18, 34))[:2]
    for column in range(3):
        g = np.zeros((7, 3), dtype=np.float32)
        g[4, column] = 1.0
        status, grad = run_backward(x, y, g)
        want = su.scale_backward(x, y, g)
        assert status == 0 and (np.abs(grad.double().numpy() - want) <= su.grad_bound(x, y, g)).all()
        others = torch.cat([grad[:4], grad[5:]])
        assert bool((others == 0).all()) and float(grad[4].abs().max()) > 0
    # sign(0) = 0 for the L1 mean: equal pixels pass nothing
    g = np.zeros((7, 3), dtype=np.float32)
    g[:, 2] = 1.0
    y2 = y.copy()
    y2[:, ::2] = x[:, ::2]
    status, grad = run_backward(x, y2, g)
    assert status == 0 and bool((grad[:, ::2] == 0).all())
    assert bool((grad[:, 1::2].abs() == torch.tensor(1.0 / (18 * 34), dtype=torch.float32)).logical_or(torch.from_numpy(x == y2)[:, 1::2]).all())
    # g_half alone: a quarter at each of the four source pixels, nothing on the dropped odd row / column
    x3, y3 = pair(1, (13, 15))[:2]
    _, g_half = _cotangents(1, (13, 15), seed=9)
    status, grad = run_backward(x3, y3, np.zeros((1, 3), dtype=np.float32), g_half)
    want = np.zeros((1, 13, 15), dtype=np.float32)
    want[:, :12, :14] = np.float32(0.25) * np.repeat(np.repeat(g_half, 2, axis=1), 2, axis=2)
    assert status == 0 and np.array_equal(grad.numpy(), want)


def test_backward_refusals():
    einval = _L().MSG_EINVAL
    x, y = su.parity_pair((2, 12, 16), seed=1)
    g = np.ones((2, 3), dtype=np.float32)
    assert run_backward(x, y, g)[0] == 0
    for name in ("x", "y", "g", "grad_x"):
        assert run_backward(x, y, g, null=(name,))[0] == einval, name
    assert run_backward(x, y, g, dims=(2, 10, 16))[0] == einval and run_backward(x, y, g, dims=(2, 12, 10))[0] == einval
    assert run_backward(x, y, g, dims=(0, 12, 16))[0] == einval
    assert run_backward(x, y, g, shift=2)[0] == einval and run_backward(x, y, g, g_shift=2)[0] == einval
    assert run_backward(x, y, g, dims=(1 << 20, 1024, 2048))[0] == einval      # 2^32 tiles


# ------------------------------------------------------------------------------------------------------- ms_ssim, classes
def test_ms_ssim_on_device_tensors_against_the_cpu_float64_run():
    from multi_stylegan_amd.ssim import ms_ssim
    shape = (3, 2, 44, 52)                                                      # three scales
    xn, yn = su.parity_pair(shape, seed=11)
    want, want_l1, factors = su.ms_ssim(xn, yn)
    assert factors.shape[1] == 3 and factors.min() >= 0.9
    host = []
    for t in (xn, yn):
        host.append(torch.from_numpy(t).double().requires_grad_(True))
    score, l1 = ms_ssim(host[0], host[1], return_l1=True)
    assert np.abs(score.detach().numpy() - want).max() <= 1e-12
    (score.sum() + 0.5 * l1.sum()).backward()
    dev = [torch.from_numpy(t).to(DEV).requires_grad_(True) for t in (xn, yn)]
    got, got_l1 = ms_ssim(dev[0], dev[1], return_l1=True)
    assert got.dtype == torch.float32 and got.shape == (3,)
    (got.sum() + 0.5 * got_l1.sum()).backward()
    # values: every factor within its scale's bound (ssim_util.mean_bounds on the float64 pyramid; the fp32 halving is one more
    # rounding of the kind the bound measures); the score is a product of factors >= 0.9 to weights that sum to 1, so it moves by
    # at most the largest factor error / 0.9; the result is rounded to fp32 twice (the plane mean, the cast)
    xs, ys, tol = xn.reshape(6, 44, 52), yn.reshape(6, 44, 52), 0.0
    for level in range(3):
        tol = max(tol, max(b.max() for b in su.mean_bounds(xs, ys)))
        xs, ys = su.halve(xs).astype(np.float32), su.halve(ys).astype(np.float32)
    err = np.abs(got.detach().double().cpu().numpy() - want).max()
    print(f"ms_ssim: {err:.2e} of {tol / 0.9 + 2.0 ** -23:.2e}")
    assert err <= tol / 0.9 + 2.0 ** -23
    assert np.abs(got_l1.detach().double().cpu().numpy() - want_l1).max() <= 2.0 ** -23
    # gradients: the fp32 statement of the chained closed form against its float64 statement, times 4 (ssim_util); the float64
    # statement itself is autograd's to 1e-12; the L1 part is +-0.5 / (P H W), exact up to the division
    for d, h_, (a, b) in zip(dev, host, ((xn, yn), (yn, xn))):
        g64 = su.ms_ssim_backward(a, b)
        g32 = su.ms_ssim_backward(a, b, dtype=np.float32).astype(np.float64)
        sign = 0.5 * np.sign(a.astype(np.float64) - b) / (2 * 44 * 52)
        assert np.abs(g64 + sign - h_.grad.numpy()).max() <= 1e-12
        bound = (su.FACTOR * np.abs(g32 - g64).max(axis=(2, 3), keepdims=True)
                 + 8.0 * su.U * (np.abs(g64).max(axis=(2, 3), keepdims=True) + np.abs(sign).max()))
        err = np.abs(d.grad.double().cpu().numpy() - h_.grad.numpy())
        print(f"ms_ssim gradient: {(err / bound).max():.3f} of the bound")
        assert (err <= bound).all()
    # a plane with a clamped factor among kept ones: exactly zero score and gradient for it, no NaN anywhere
    xc = torch.rand((2, 2, 24, 26), generator=torch.Generator().manual_seed(3))
    yc = xc.clone()
    yc[0, 1] = 1.0 - xc[0, 1]
    xd, yd = xc.to(DEV).requires_grad_(True), yc.to(DEV)
    out = ms_ssim(xd, yd)
    out.sum().backward()
    assert out.tolist() == [0.5, 1.0] and bool((xd.grad[0, 1] == 0).all()) and bool(torch.isfinite(xd.grad).all())
    with pytest.raises(_L().MsgHipError, match="float32"):
        ms_ssim(xd.bfloat16(), yd.bfloat16())


@pytest.mark.parametrize("video", [False, True])
def test_diversity_classes_against_their_cpu_run(video):
    """Collapsed stubs on both sides (two different base clips): every factor is near 1, away from the clamp, where both fp32
    runs are within 1e-6 of the float64 score (|x - y| <= 0.01 against a variance of 1 / 12 in D2); held to 1e-5."""
    from multi_stylegan_amd import validation_metrics as vm
    cls = vm.MSSSIMVideo if video else vm.MSSSIM
    frames = 3 if video else 1
    scores = []
    for device in ("cpu", DEV):
        torch.manual_seed(0)
        metric = cls(device=device, batch_size=4, data_samples=16, no_rfp=True, seed=2)
        scores.append(metric(generator=StubGenerator(frames=frames, seed=5, collapsed=True),
                             dataset=stub_dataset(4, 4, frames=frames, collapsed=True)))
    for host, dev in zip(*scores):
        assert host._fields == dev._fields == ("fake", "real", "gap")
        assert host.fake > 0.99 and host.real > 0.99
        assert abs(host.fake - dev.fake) <= 1e-5 and abs(host.real - dev.real) <= 1e-5
