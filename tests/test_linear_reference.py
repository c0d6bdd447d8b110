"""tests/linear_util.py is the yardstick of tests/test_hip_linear.py, so it is checked here first, in float64 on the CPU: against
the project's oracle (oracle.ops.equalized_linear), against torch.autograd of F.linear to the second order, and against the
recorded eqlinear.* layer of tests/golden/layers.npz.  Then every case of the GPU module is evaluated in float32 as well: the
GPU bounds are multiples of that error (e32), which therefore has to be a rounding error -- a reference that cancels or breaks
would otherwise widen a bound unnoticed."""
import math

import pytest
import torch
import torch.nn.functional as F

import linear_util as lu
from conftest import rel_err

M, N, K = 5, 7, 12


def _case(seed=0, bias=True):
    gen = torch.Generator().manual_seed(seed)
    return lu.draw(gen, M, K), lu.draw(gen, N, K), (lu.draw(gen, N) if bias else None), lu.draw(gen, M, N)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_fprop_is_the_oracles_equalized_linear(bias):
    from oracle import ops as oo
    x, w, b, _ = _case(1, bias)
    got = lu.fprop(x, w, b, oo.eq_scale(K), oo.eq_scale(N))
    assert rel_err(got, oo.equalized_linear(x, w, b)) < 1e-14


def test_golden_eqlinear_layer(golden):
    z = golden("layers")
    x, w, b = (z["eqlinear." + k].double() for k in ("x", "w", "b"))
    got = lu.fprop(x, w, b, math.sqrt(2.0 / w.shape[1]), math.sqrt(2.0 / w.shape[0]))
    assert rel_err(got, z["eqlinear.y"]) < 1e-6                              # (recorded in float32)
    # the grouped form with one group and one slot is the same layer
    got = lu.grouped_fprop(x[:, None, :], (0,), [w], [b], math.sqrt(2.0 / w.shape[1]), math.sqrt(2.0 / w.shape[0]))
    assert got.shape == (1,) + tuple(z["eqlinear.y"].shape) and rel_err(got[0], z["eqlinear.y"]) < 1e-6


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
def test_first_and_second_order_match_autograd_of_f_linear(bias):
    x, w, b, gy = _case(2, bias)
    xr, wr, gyr = (t.clone().requires_grad_(True) for t in (x, w, gy))
    br = b.clone().requires_grad_(True) if bias else None
    y = F.linear(xr, wr * lu.GAIN, None if br is None else br * lu.BIAS_GAIN)
    first = torch.autograd.grad(y, [xr, wr] + ([br] if bias else []), gyr, create_graph=True)
    assert rel_err(lu.fprop(x, w, b, lu.GAIN, lu.BIAS_GAIN), y.detach()) < 1e-14
    assert rel_err(lu.dgrad(gy, w, lu.GAIN), first[0].detach()) < 1e-14
    gw, gb = lu.wgrad(gy, x, lu.GAIN, lu.BIAS_GAIN)
    assert rel_err(gw, first[1].detach()) < 1e-14
    if bias:
        assert rel_err(gb, first[2].detach()) < 1e-14
    # second order: each derivative of one member of the family is another member
    u, v = _case(3)[0], _case(4)[1]                                        # cotangents of gx [M,K] and of gw [N,K]
    d_gy, d_w = torch.autograd.grad(first[0], (gyr, wr), u, retain_graph=True)
    assert rel_err(lu.fprop(u, w, None, lu.GAIN, 1.0), d_gy) < 1e-14
    assert rel_err(lu.wgrad(gy, u, lu.GAIN, 1.0)[0], d_w) < 1e-14
    d_gy, d_x = torch.autograd.grad(first[1], (gyr, xr), v, retain_graph=True)
    assert rel_err(lu.fprop(x, v, None, lu.GAIN, 1.0), d_gy) < 1e-14
    assert rel_err(lu.dgrad(gy, v, lu.GAIN), d_x) < 1e-14
    # the regularisers' forms, as operator_quantities hands them out
    q = lu.operator_quantities(x, w, b, gy, lu.GAIN, lu.BIAS_GAIN)
    pl_w, pl_gy = torch.autograd.grad(first[0].square().sum(), (wr, gyr), retain_graph=True)
    r_gy, r_x = torch.autograd.grad(first[1].square().sum(), (gyr, xr), retain_graph=True)
    for name, ref in (("y", y), ("gx", first[0]), ("gw", first[1]), ("d|gx|2/dw", pl_w), ("d|gx|2/dgy", pl_gy),
                      ("d|gw|2/dgy", r_gy), ("d|gw|2/dx", r_x)):
        assert rel_err(q[name], ref.detach()) < 1e-14, name
    assert ("gb" in q) == bias and (not bias or rel_err(q["gb"], first[2].detach()) < 1e-14)
    assert torch.autograd.grad(first[1].square().sum(), wr, allow_unused=True)[0] is None    # dy/dw does not depend on w


def test_grouped_forms_match_autograd_of_f_linear():
    g, l, slot = 3, 4, (2, 0, 2)
    x = lu.grouped_inputs("operator", g, l, slot, M, N, K)
    lat, gyr = (x[k].clone().requires_grad_(True) for k in ("latent", "gy"))
    ws, bs = [w.clone().requires_grad_(True) for w in x["ws"]], [b.clone().requires_grad_(True) for b in x["biases"]]
    y = torch.stack([F.linear(lat[:, slot[j]], ws[j] * lu.GAIN, bs[j] * lu.BIAS_GAIN) for j in range(g)])
    first = torch.autograd.grad(y, [lat, *ws, *bs], gyr, create_graph=True)
    assert rel_err(lu.grouped_fprop(x["latent"], slot, x["ws"], x["biases"], lu.GAIN, lu.BIAS_GAIN), y.detach()) < 1e-14
    gx, glat = lu.grouped_dgrad(x["gy"], x["ws"], slot, l, lu.GAIN)
    assert rel_err(glat, first[0].detach()) < 1e-14
    assert float(glat[:, 1].abs().max()) == 0.0 and float(glat[:, 3].abs().max()) == 0.0            # slots nobody reads
    for j in range(g):
        assert rel_err(gx[j], lu.dgrad(x["gy"][j], x["ws"][j], lu.GAIN)) == 0.0
    gw, gb = lu.grouped_wgrad(x["gy"], x["latent"], slot, lu.GAIN, lu.BIAS_GAIN)
    assert rel_err(gw, torch.stack(first[1:1 + g]).detach()) < 1e-14
    assert rel_err(gb, torch.stack(first[1 + g:]).detach()) < 1e-14
    second = torch.autograd.grad(first[0].square().sum(), [*ws, gyr])
    q = lu.grouped_operator_quantities(x["latent"], slot, x["ws"], x["biases"], x["gy"], lu.GAIN, lu.BIAS_GAIN)
    assert rel_err(q["d|glat|2/dw"], torch.stack(second[:g])) < 1e-14
    assert rel_err(q["d|glat|2/dgy"], second[g]) < 1e-14
    assert rel_err(q["glat"], first[0].detach()) < 1e-14 and rel_err(q["y"], y.detach()) < 1e-14


# ------------------------------------------------------------------------------------------- e32 of every GPU case
E32_MAX = 1e-5


def _hold(tag, refs):
    worst = 0.0
    for q, (ref, e32) in refs.items():
        for e in (e32 if isinstance(e32, list) else [e32]):
            assert math.isfinite(e) and e < E32_MAX, f"{tag} {q}: e32 = {e}"
            worst = max(worst, e)
        assert bool(torch.isfinite(ref).all()) and float(ref.abs().max()) > 0, f"{tag} {q}: the reference is degenerate"
    print("%s: largest e32 %.2e" % (tag, worst))


SINGLE = [(e, c) for e, cases in (("fprop", lu.FPROP_CASES), ("dgrad", lu.DGRAD_CASES), ("wgrad", lu.WGRAD_CASES)) for c in cases]


@pytest.mark.parametrize("entry,case", SINGLE, ids=["%s-%s" % (e, lu.case_id(c)) for e, c in SINGLE])
def test_e32_of_the_single_layer_cases(entry, case):
    _hold(entry, lu.reference(entry, *case))


GROUPED = [(e, c) for e in ("fprop", "dgrad", "wgrad") for c in lu.GROUPED_CASES[e]]


@pytest.mark.parametrize("entry,case", GROUPED, ids=["%s-%s" % (e, lu.case_id(c)) for e, c in GROUPED])
def test_e32_of_the_grouped_cases(entry, case):
    _hold("grouped " + entry, lu.grouped_reference(entry, *case))


@pytest.mark.parametrize("case", lu.OPERATOR_CASES, ids=[lu.case_id(c) for c in lu.OPERATOR_CASES])
def test_e32_of_the_operator_cases(case):
    _hold("linear", lu.operator_reference(*case))


def test_e32_of_the_grouped_operator_case():
    _hold("grouped_linear", lu.grouped_operator_reference(*lu.GROUPED_OPERATOR_CASE))
