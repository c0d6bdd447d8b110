"""csrc/linear.hip through the C ABI (include/msg_hip.h), entry by entry, then through conv_ops.linear / conv_ops.grouped_linear,
against the float64 definitions of tests/linear_util.py (themselves checked against the CPU oracle, F.linear's autograd and the
golden layer in tests/test_linear_reference.py) -- at the smallest shapes that reach each loop and tile edge of the kernels: the
second and a ragged row block (LIN_MB = 16), columns that do not fill a workgroup of four, the lane and register-chunk limits
along K (64, LIN_KC = 1024), a second staged LDS chunk in dgrad (LIN_NCH = 1024) with waves whose row range is empty, LDS
restaged across row blocks and chunks, the second pass of wgrad's 256-thread loop, groups that share or skip latent slots.

Bound.  Every quantity is a reduction: max|got - ref| / max|ref| <= max(8 * e32, 2^-21), e32 being the same error of linear_util
run in float32 on the CPU for the same case (grouped stacks: group by group, each against its own e32).  Every output is
pre-filled with NaN and followed by a guard row: all of it must be written, nothing behind it; a refused or no-op call leaves
it untouched.

Largest errors measured on the MI355X (the case closest to its bound, per entry and quantity), next to that bound; cases are
M-N-K, grouped ones G-L-slots-M-N-K:
    msg_linear_fprop               y              1.0e-07  of 5.7e-07   3-5-65;      bias=NULL 9.5e-08 of 7.9e-07, same case
    msg_linear_dgrad               gx             1.3e-07  of 8.0e-07   17-5-70
    msg_linear_wgrad               gw             3.9e-07  of 2.4e-06   256-5-70
                                   gb             1.3e-06  of 2.0e-06   256-5-70     (0.64 of its bound, see below)
    msg_linear_grouped_fprop       y              1.0e-07  of 5.1e-07   20-14-...-3-40-24;  bias=NULL 1.0e-07 of 5.1e-07
    msg_linear_grouped_dgrad       gx             2.0e-07  of 3.2e-06   20-14-...-17-1025-65
    msg_linear_grouped_wgrad       gw             1.3e-07  of 1.0e-06   1-1-s0-17-5-1025;   _wgrad_ptrs: the same figures
                                   gb             1.3e-07  of 6.2e-07   20-14-...-17-5-1025
    conv_ops.linear                y              8.1e-08  of 1.1e-06   256-5-70
                                   gx             1.1e-07  of 5.7e-07   17-5-1025, with and without a graph
                                   gw             7.9e-08  of 4.8e-07   1-1-128,   with and without a graph
                                   gb             4.0e-07  of 1.7e-06   256-5-70 (fused with gw); 1.1e-07 of 9.0e-07 with a graph
                                   d|gx|2/dw      1.9e-07  of 1.3e-06   17-5-1025;   d|gx|2/dgy 1.8e-07 of 3.1e-06 (33-1025-65)
                                   d|gw|2/dx      1.3e-07  of 1.0e-06   17-5-1025;   d|gw|2/dgy 1.3e-07 of 1.8e-06 (33-1025-65)
    conv_ops.grouped_linear        y              1.2e-07  of 2.1e-06   3-4-s202-17-5-1025, as all of:
                                   glat           9.0e-08  of 8.1e-07   with and without a graph
                                   gw, gb         1.9e-07  of 1.2e-06,  1.0e-07 of 8.0e-07
                                   d|glat|2/dw    1.4e-07  of 7.6e-07;  d|glat|2/dgy below that
    257 rows (the convolution path, tolerance 1e-4): below 1e-6.
Everything stayed under a quarter of its bound but msg_linear_wgrad's gb at M = 256, at 0.64: thread 0 adds the 256 values of
a column one after the other in fp32, the longest serial sum of the file, while e32 comes from torch's blocked sum.  The factor
8 holds; no entry needed another.  Each case prints its own figures; the fixture prints the largest.
"""
import pytest
import torch
import torch.nn.functional as F

import linear_util as lu
from abi_util import DEV, Guarded, _ptr, _shifted, _stream
from linear_util import BIAS_GAIN, GAIN, case_id, rel_err

pytestmark = pytest.mark.gpu
OK, EINVAL = 0, -1
WORST = {}                              # entry / quantity -> (error, bound, case): printed when the module is done
FACTOR = {}                             # entry / quantity -> factor on e32 where a correct kernel needs more than 8 (see docstring)


@pytest.fixture(scope="module")
def lib():
    from multi_stylegan_amd import _lib
    yield _lib.lib()
    for key in sorted(WORST):
        print("\nworst %-44s %.2e  (bound %.2e, %s)" % ((key,) + WORST[key]), end="")
    print()


def _dev(t):
    return t.to(DEV, torch.float32).contiguous()


def _check(key, case, got, ref, e32):
    """One quantity against its bound; a [G,...] stack (e32 a list) group by group, so that a wrong group or slot shows as a
    whole wrong slab."""
    assert tuple(got.shape) == tuple(ref.shape), (key, case, got.shape, ref.shape)
    got = got.detach().double().cpu()
    groups = [(got, ref, e32)] if not isinstance(e32, list) else [(got[g], ref[g], e32[g]) for g in range(len(e32))]
    bad = []
    for g, (a, r, e) in enumerate(groups):
        err, bound = rel_err(a, r), lu.bound(e, FACTOR.get(key, 8))
        print("%s %s%s: %.2e (bound %.2e)" % (key, case, " group %d" % g if isinstance(e32, list) else "", err, bound))
        if key not in WORST or err / bound > WORST[key][0] / WORST[key][1]:
            WORST[key] = (err, bound, case)
        if not err <= bound:
            bad.append((g, err, bound))
    assert not bad, f"{key} {case}: (group, error, bound) {bad}"


def _table(tensors):
    return torch.tensor([t.data_ptr() for t in tensors], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------------------------------- msg_linear_fprop
@pytest.mark.parametrize("case", lu.FPROP_CASES, ids=[case_id(c) for c in lu.FPROP_CASES])
def test_fprop(lib, case):
    m, n, k = case
    x, refs = lu.inputs("fprop", m, n, k), lu.reference("fprop", m, n, k)
    xd, wd, bd = _dev(x["x"]), _dev(x["w"]), _dev(x["bias"])
    for q, bias in (("y", bd), ("y bias=NULL", None)):
        y = Guarded((m, n), n)
        assert lib.msg_linear_fprop(xd.data_ptr(), wd.data_ptr(), _ptr(bias), y.ptr, m, n, k, GAIN, BIAS_GAIN, _stream()) == OK
        _check("msg_linear_fprop " + q, case_id(case), y.read(), *refs[q])


def test_fprop_operands_off_their_alignment(lib):
    """x, w and y each 4 bytes off a 16-byte boundary."""
    m, n, k = 17, 5, 1025
    x, refs = lu.inputs("fprop", m, n, k), lu.reference("fprop", m, n, k)
    keep_x, xp = _shifted(_dev(x["x"]))
    keep_w, wp = _shifted(_dev(x["w"]))
    bd = _dev(x["bias"])
    y = Guarded((m * n + 1,), n)                               # the output starts at element 1
    assert lib.msg_linear_fprop(xp, wp, bd.data_ptr(), y.ptr + 4, m, n, k, GAIN, BIAS_GAIN, _stream()) == OK
    host = y._host()
    assert bool(torch.isnan(host[0])), "the element in front of the output was written"
    assert not bool(torch.isnan(host[1:]).any()), "output elements were not written"
    _check("msg_linear_fprop y", "17-5-1025 x,w,y+4B", host[1:].reshape(m, n), *refs["y"])


# ------------------------------------------------------------------------------------------- msg_linear_dgrad
@pytest.mark.parametrize("case", lu.DGRAD_CASES, ids=[case_id(c) for c in lu.DGRAD_CASES])
def test_dgrad(lib, case):
    m, n, k = case
    x, refs = lu.inputs("dgrad", m, n, k), lu.reference("dgrad", m, n, k)
    gyd, wd = _dev(x["gy"]), _dev(x["w"])
    runs = []
    for _ in range(2):
        gx = Guarded((m, k), k)
        assert lib.msg_linear_dgrad(gyd.data_ptr(), wd.data_ptr(), gx.ptr, m, n, k, GAIN, _stream()) == OK
        runs.append(gx.read())
    _check("msg_linear_dgrad gx", case_id(case), runs[0], *refs["gx"])
    assert torch.equal(runs[0], runs[1]), "two calls on the same operands differ: the reduction order is not fixed"


# ------------------------------------------------------------------------------------------- msg_linear_wgrad
@pytest.mark.parametrize("case", lu.WGRAD_CASES, ids=[case_id(c) for c in lu.WGRAD_CASES])
def test_wgrad(lib, case):
    m, n, k = case
    x, refs = lu.inputs("wgrad", m, n, k), lu.reference("wgrad", m, n, k)
    gyd, xd = _dev(x["gy"]), _dev(x["x"])
    for with_gb in (True, False):
        gw, gb = Guarded((n, k), k), Guarded((n,), n)
        assert lib.msg_linear_wgrad(gyd.data_ptr(), xd.data_ptr(), gw.ptr, gb.ptr if with_gb else None, m, n, k, GAIN, BIAS_GAIN,
                                    _stream()) == OK
        tag = case_id(case) + ("" if with_gb else " gb=NULL")
        _check("msg_linear_wgrad gw", tag, gw.read(), *refs["gw"])
        if with_gb:
            _check("msg_linear_wgrad gb", tag, gb.read(), *refs["gb"])
        else:
            gb.assert_untouched()


def test_wgrad_of_an_empty_batch_writes_zeros(lib):
    n, k = 5, 70
    for with_gb in (True, False):
        gw, gb = Guarded((n, k), k), Guarded((n,), n)
        assert lib.msg_linear_wgrad(None, None, gw.ptr, gb.ptr if with_gb else None, 0, n, k, GAIN, BIAS_GAIN, _stream()) == OK
        assert float(gw.read().abs().max()) == 0.0
        if with_gb:
            assert float(gb.read().abs().max()) == 0.0
        else:
            gb.assert_untouched()


def test_empty_batch_is_a_no_op_for_fprop_and_dgrad(lib):
    m, n, k = 3, 5, 70
    a = torch.zeros(m * max(n, k) + n * k, device=DEV)
    y, gx = Guarded((m, n), n), Guarded((m, k), k)
    assert lib.msg_linear_fprop(a.data_ptr(), a.data_ptr(), None, y.ptr, 0, n, k, GAIN, BIAS_GAIN, _stream()) == OK
    assert lib.msg_linear_dgrad(a.data_ptr(), a.data_ptr(), gx.ptr, 0, n, k, GAIN, _stream()) == OK
    assert lib.msg_linear_fprop(a.data_ptr(), a.data_ptr(), None, y.ptr, m, 0, k, GAIN, BIAS_GAIN, _stream()) == EINVAL
    assert lib.msg_linear_dgrad(a.data_ptr(), a.data_ptr(), gx.ptr, m, n, 0, GAIN, _stream()) == EINVAL
    y.assert_untouched()
    gx.assert_untouched()


# ------------------------------------------------------------------------------------------- the grouped entries
def _grouped_operands(entry, case):
    """Every group's w and bias in an allocation of its own: a wrong table index reads another layer."""
    g, l, slot, m, n, k = case
    x = lu.grouped_inputs(entry, *case)
    ops = {"latent": _dev(x["latent"]), "gy": _dev(x["gy"]), "ws": [_dev(w) for w in x["ws"]],
           "biases": [_dev(b) for b in x["biases"]], "slot": torch.tensor(slot, dtype=torch.int32, device=DEV)}
    ops["wt"], ops["bt"] = _table(ops["ws"]), _table(ops["biases"])
    return ops, lu.grouped_reference(entry, *case)


GF, GD, GW = (lu.GROUPED_CASES[e] for e in ("fprop", "dgrad", "wgrad"))


@pytest.mark.parametrize("case", GF, ids=[case_id(c) for c in GF])
def test_grouped_fprop(lib, case):
    g, l, slot, m, n, k = case
    ops, refs = _grouped_operands("fprop", case)
    for q, bias in (("y", ops["bt"]), ("y bias=NULL", None)):
        y = Guarded((g, m, n), n)
        assert lib.msg_linear_grouped_fprop(ops["latent"].data_ptr(), ops["slot"].data_ptr(), ops["wt"].data_ptr(), _ptr(bias), y.ptr,
                                            g, m, n, k, l, GAIN, BIAS_GAIN, _stream()) == OK
        _check("msg_linear_grouped_fprop " + q, case_id(case), y.read(), *refs[q])
    for g_, m_ in ((0, m), (g, 0)):
        y = Guarded((g, m, n), n)
        assert lib.msg_linear_grouped_fprop(ops["latent"].data_ptr(), ops["slot"].data_ptr(), ops["wt"].data_ptr(), ops["bt"].data_ptr(),
                                            y.ptr, g_, m_, n, k, l, GAIN, BIAS_GAIN, _stream()) == OK
        y.assert_untouched()


@pytest.mark.parametrize("case", GD, ids=[case_id(c) for c in GD])
def test_grouped_dgrad(lib, case):
    g, l, slot, m, n, k = case
    ops, refs = _grouped_operands("dgrad", case)
    runs = []
    for _ in range(2):
        gx = Guarded((g, m, k), k)
        assert lib.msg_linear_grouped_dgrad(ops["gy"].data_ptr(), ops["wt"].data_ptr(), gx.ptr, g, m, n, k, GAIN, _stream()) == OK
        runs.append(gx.read())
    _check("msg_linear_grouped_dgrad gx", case_id(case), runs[0], *refs["gx"])
    assert torch.equal(runs[0], runs[1])
    for g_, m_ in ((0, m), (g, 0)):
        gx = Guarded((g, m, k), k)
        assert lib.msg_linear_grouped_dgrad(ops["gy"].data_ptr(), ops["wt"].data_ptr(), gx.ptr, g_, m_, n, k, GAIN, _stream()) == OK
        gx.assert_untouched()


@pytest.mark.parametrize("case", GW, ids=[case_id(c) for c in GW])
def test_grouped_wgrad(lib, case):
    g, l, slot, m, n, k = case
    ops, refs = _grouped_operands("wgrad", case)
    head = (ops["gy"].data_ptr(), ops["latent"].data_ptr(), ops["slot"].data_ptr())
    for with_gb in (True, False):
        gw, gb = Guarded((g, n, k), k), Guarded((g, n), n)
        assert lib.msg_linear_grouped_wgrad(*head, gw.ptr, gb.ptr if with_gb else None, g, m, n, k, l, GAIN, BIAS_GAIN,
                                            _stream()) == OK
        tag = case_id(case) + ("" if with_gb else " gb=NULL")
        _check("msg_linear_grouped_wgrad gw", tag, gw.read(), *refs["gw"])
        if with_gb:
            _check("msg_linear_grouped_wgrad gb", tag, gb.read(), *refs["gb"])
        else:
            gb.assert_untouched()
    gw, gb = Guarded((g, n, k), k), Guarded((g, n), n)
    assert lib.msg_linear_grouped_wgrad(*head, gw.ptr, gb.ptr, 0, m, n, k, l, GAIN, BIAS_GAIN, _stream()) == OK     # G = 0
    gw.assert_untouched()
    gb.assert_untouched()
    # an empty batch: like msg_linear_wgrad the zero gradient is written, and neither gy nor x is read
    assert lib.msg_linear_grouped_wgrad(None, None, head[2], gw.ptr, gb.ptr, g, 0, n, k, l, GAIN, BIAS_GAIN, _stream()) == OK
    assert float(gw.read().abs().max()) == 0.0 and float(gb.read().abs().max()) == 0.0
    assert lib.msg_linear_grouped_wgrad(*head, None, gb.ptr, g, 0, n, k, l, GAIN, BIAS_GAIN, _stream()) == EINVAL
    assert lib.msg_linear_grouped_wgrad(*head[:2], None, gw.ptr, gb.ptr, g, 0, n, k, l, GAIN, BIAS_GAIN, _stream()) == EINVAL


class Scattered:
    """G destinations of `size` floats each, out of order and with gaps, inside one NaN-filled flat buffer with a sentinel tail."""

    def __init__(self, g, size, gap):
        order = [(5 * j + 3) % g for j in range(g)] if g % 5 else list(reversed(range(g)))      # a permutation of the groups
        assert sorted(order) == list(range(g))
        self.g, self.size = g, size
        self.flat = Guarded((gap + g * (size + gap),), 64)
        self.start = [0] * g
        for place, j in enumerate(order):
            self.start[j] = gap + place * (size + gap)
        self.table = torch.tensor([self.flat.ptr + 4 * s for s in self.start], dtype=torch.int64, device=DEV)

    def read(self, shape):
        """-> [G, *shape] in float64: every slice written, every other element of the buffer still NaN, the tail untouched."""
        host = self.flat._host()
        inside = torch.zeros(host.numel(), dtype=torch.bool)
        for s in self.start:
            inside[s:s + self.size] = True
        assert bool(torch.isnan(host[~inside]).all()), "something outside the G destinations was written"
        assert not bool(torch.isnan(host[inside]).any()), "destination elements were not written"
        return torch.stack([host[s:s + self.size] for s in self.start]).double().reshape((self.g,) + tuple(shape))


@pytest.mark.parametrize("case", GW, ids=[case_id(c) for c in GW])
def test_grouped_wgrad_ptrs(lib, case):
    g, l, slot, m, n, k = case
    ops, refs = _grouped_operands("wgrad", case)
    head = (ops["gy"].data_ptr(), ops["latent"].data_ptr(), ops["slot"].data_ptr())
    for with_gb in (True, False):
        gw, gb = Scattered(g, n * k, 7), Scattered(g, n, 3)
        assert lib.msg_linear_grouped_wgrad_ptrs(*head, gw.table.data_ptr(), gb.table.data_ptr() if with_gb else None, g, m, n, k, l,
                                                 GAIN, BIAS_GAIN, _stream()) == OK
        tag = case_id(case) + ("" if with_gb else " gb=NULL")
        _check("msg_linear_grouped_wgrad_ptrs gw", tag, gw.read((n, k)), *refs["gw"])
        if with_gb:
            _check("msg_linear_grouped_wgrad_ptrs gb", tag, gb.read((n,)), *refs["gb"])
        else:
            gb.flat.assert_untouched()
    gw, gb = Scattered(g, n * k, 7), Scattered(g, n, 3)
    assert lib.msg_linear_grouped_wgrad_ptrs(*head, gw.table.data_ptr(), gb.table.data_ptr(), 0, m, n, k, l, GAIN, BIAS_GAIN,
                                             _stream()) == OK                                                       # G = 0
    gw.flat.assert_untouched()
    gb.flat.assert_untouched()
    assert lib.msg_linear_grouped_wgrad_ptrs(None, None, head[2], gw.table.data_ptr(), gb.table.data_ptr(), g, 0, n, k, l, GAIN,
                                             BIAS_GAIN, _stream()) == OK                                            # M = 0: zeros
    assert float(gw.read((n, k)).abs().max()) == 0.0 and float(gb.read((n,)).abs().max()) == 0.0
    assert lib.msg_linear_grouped_wgrad_ptrs(*head, None, gb.table.data_ptr(), g, 0, n, k, l, GAIN, BIAS_GAIN, _stream()) == EINVAL


# ------------------------------------------------------------------------------------------- conv_ops.linear
def _linear_leaves(m, n, k, has_bias):
    """x a [:, j] slice of a [B,L,K] latent, the weight a transposed view of a [K,N] tensor: both reach the op non-contiguous."""
    x = lu.operator_inputs(m, n, k)
    lat = x["latent"].to(DEV, torch.float32).requires_grad_(True)
    wt = x["wt"].to(DEV, torch.float32).requires_grad_(True)
    b = x["bias"].to(DEV, torch.float32).requires_grad_(True) if has_bias else None
    gy = x["gy"].to(DEV, torch.float32).requires_grad_(True)
    return lat, x["j"], wt, b, gy


def _slice_only(key, glat, j):
    """The gradient of the latent is that of x in slot j and exactly zero elsewhere -> the slot."""
    rest = torch.cat([glat[:, :j], glat[:, j + 1:]], dim=1).detach()
    assert float(rest.abs().max()) == 0.0, f"{key}: gradient outside the slice that was read"
    return glat[:, j]


@pytest.mark.parametrize("case", lu.OPERATOR_CASES, ids=[case_id(c) for c in lu.OPERATOR_CASES])
def test_linear_operator(lib, case):
    from multi_stylegan_amd import conv_ops
    m, n, k, has_bias = case
    refs, tag = lu.operator_reference(*case), case_id(case)
    lat, j, wt, b, gy = _linear_leaves(*case)
    assert not lat[:, j].is_contiguous() or m == 1
    ins = [lat, wt] + ([b] if has_bias else [])
    names = ["gx", "gw"] + (["gb"] if has_bias else [])

    def first(grads):
        return [_slice_only("gx", grads[0], j), grads[1].t()] + list(grads[2:])

    # grad mode off in backward: with a bias, weight and bias gradient come from one msg_linear_wgrad launch
    y = conv_ops.linear(lat[:, j], wt.t(), b, GAIN, BIAS_GAIN)
    _check("linear y", tag, y, *refs["y"])
    for q, got in zip(names, first(torch.autograd.grad(y, ins, gy.detach()))):
        _check("linear %s (no graph)" % q, tag, got, *refs[q])
    # the same with a graph, then the second order in the regularisers' two forms
    y = conv_ops.linear(lat[:, j], wt.t(), b, GAIN, BIAS_GAIN)
    grads = torch.autograd.grad(y, ins, gy, create_graph=True)
    for q, got in zip(names, first(grads)):
        _check("linear %s (create_graph)" % q, tag, got, *refs[q])
    d_wt, d_gy = torch.autograd.grad(grads[0].square().sum(), (wt, gy), retain_graph=True)
    _check("linear d|gx|2/dw", tag, d_wt.t(), *refs["d|gx|2/dw"])
    _check("linear d|gx|2/dgy", tag, d_gy, *refs["d|gx|2/dgy"])
    d_wt, d_lat, d_gy = torch.autograd.grad(grads[1].square().sum(), (wt, lat, gy), retain_graph=True, allow_unused=True)
    assert d_wt is None or float(d_wt.abs().max()) == 0.0                  # dy/dw does not depend on w
    _check("linear d|gw|2/dx", tag, _slice_only("d|gw|2/dx", d_lat, j), *refs["d|gw|2/dx"])
    _check("linear d|gw|2/dgy", tag, d_gy, *refs["d|gw|2/dgy"])


def _clocked(fn):
    from multi_stylegan_amd import _lib
    _lib.kernel_clock.reset(enabled=True)
    try:
        out = fn()
        torch.cuda.synchronize()
        keys = set(_lib.kernel_clock.summary())
    finally:
        _lib.kernel_clock.reset(enabled=False)
    return out, keys


@pytest.mark.parametrize("rows", [256, 257])
def test_linear_operator_row_limit(lib, rows):
    """Up to _LINEAR_MAX_ROWS = 256 rows take the few-row kernels (16 row blocks); one more takes the convolution path, held to
    that path's fp32 tolerance (1e-4 of max|ref|, tests/test_hip_conv.py)."""
    from multi_stylegan_amd import conv_ops
    n, k = 5, 70
    gen = torch.Generator().manual_seed(rows)
    x, w, b, gy = lu.draw(gen, rows, k), lu.draw(gen, n, k), lu.draw(gen, n), lu.draw(gen, rows, n)
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = F.linear(xr, wr * GAIN, br * BIAS_GAIN)
    gr = torch.autograd.grad(yr, (xr, wr, br), gy)
    xd, wd, bd = (t.to(DEV, torch.float32).requires_grad_(True) for t in (x, w, b))
    y, keys = _clocked(lambda: conv_ops.linear(xd, wd, bd, GAIN, BIAS_GAIN))
    gd = torch.autograd.grad(y, (xd, wd, bd), gy.to(DEV, torch.float32))
    few_rows = any(key.startswith("linear_fprop/") for key in keys)
    if rows <= 256:
        assert few_rows, keys
        f32 = [t.float() for t in (x, w, b, gy)]
        e32 = [rel_err(a, r) for a, r in zip((lu.fprop(*f32[:3], GAIN, BIAS_GAIN), lu.dgrad(f32[3], f32[1], GAIN))
                                             + lu.wgrad(f32[3], f32[0], GAIN, BIAS_GAIN), (yr.detach(),) + gr)]
        for q, got, ref, e in zip(("y", "gx (no graph)", "gw (no graph)", "gb (no graph)"), (y,) + gd, (yr.detach(),) + gr, e32):
            _check("linear " + q, "256-5-70", got, ref, e)
    else:
        assert not few_rows, keys
        for q, got, ref in zip(("y", "gx", "gw", "gb"), (y,) + gd, (yr.detach(),) + gr):
            err = rel_err(got.detach().cpu(), ref)
            print("linear (conv path) %s 257-5-70: %.2e (tolerance 1e-4)" % (q, err))
            assert err < 1e-4, q


# ------------------------------------------------------------------------------------------- conv_ops.grouped_linear
def test_grouped_linear_operator(lib):
    from multi_stylegan_amd import conv_ops
    case = lu.GROUPED_OPERATOR_CASE
    g, l, slot, m, n, k = case
    x, refs, tag = lu.grouped_inputs("operator", *case), lu.grouped_operator_reference(*case), case_id(case)
    lat = x["latent"].to(DEV, torch.float32).requires_grad_(True)
    ws = [w.to(DEV, torch.float32).requires_grad_(True) for w in x["ws"]]
    bs = [b.to(DEV, torch.float32).requires_grad_(True) for b in x["biases"]]
    gy = x["gy"].to(DEV, torch.float32).requires_grad_(True)
    y, keys = _clocked(lambda: conv_ops.grouped_linear(lat, slot, ws, bs, GAIN, BIAS_GAIN))
    assert any(key.startswith("linear_grouped_fprop/") for key in keys), keys
    _check("grouped_linear y", tag, y, *refs["y"])
    grads = torch.autograd.grad(y, [lat, *ws, *bs], gy.detach())            # grad mode off: the grouped kernels
    _check("grouped_linear glat", tag, grads[0], *refs["glat"])
    _check("grouped_linear gw", tag, torch.stack(grads[1:1 + g]), *refs["gw"])
    _check("grouped_linear gb", tag, torch.stack(grads[1 + g:]), *refs["gb"])
    # the path-length regulariser's second order: the latent's gradient alone, differentiated once more (_GroupedLinD)
    y = conv_ops.grouped_linear(lat, slot, ws, bs, GAIN, BIAS_GAIN)
    glat, = torch.autograd.grad(y, lat, gy, create_graph=True)
    nodes, frontier = [], [glat.grad_fn]
    for _ in range(3):                                                      # (the node itself, or just behind a view / copy)
        nodes += frontier
        frontier = [f for nd in frontier if nd is not None for f, _ in nd.next_functions if f is not None]
    assert any(type(nd).__name__.startswith("_GroupedLinD") for nd in nodes), [type(nd).__name__ for nd in nodes]
    _check("grouped_linear glat (create_graph)", tag, glat, *refs["glat"])
    second = torch.autograd.grad(glat.square().sum(), [*ws, gy])
    _check("grouped_linear d|glat|2/dw", tag, torch.stack(second[:g]), *refs["d|glat|2/dw"])
    _check("grouped_linear d|glat|2/dgy", tag, second[g], *refs["d|glat|2/dgy"])
